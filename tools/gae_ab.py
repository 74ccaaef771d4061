"""On-device GAE against the torch loop, and the cost of the time-out record: go1gate 4096 envs x 2 agents, T = 200, two 64 x 64 tanh
networks, one handle, one process.
  (a) rollout(T) against rollout(T, time_outs=True): what the T N-byte copies of mqe_rollout_time_outs cost;
  (b) gae(traj) with and without normalisation (mqe_gae: k_gae, + k_gae_normalize);
  (c) the same advantages and returns from the loop over t a torch learner runs (rsl_rl's RolloutStorage.compute_returns, with the
      time-out bootstrap reward += gamma * value * time_outs folded in front of it and the advantage normalisation behind it), on the
      trajectory's own tensors.
Every figure is a HIP-event time (events recorded on the stream around a window, synchronised after it) per call; a window of (a) is one
rollout, a window of (b, c) is --reps calls back to back (one gae call is tens of microseconds: a single one would time the launch, not the
kernel); all paths are warmed up; the paths of a group alternate --rounds times.  The measured trajectory is the first window that holds
dones (all envs of a fresh batch time out in the same step, once per episode).  Prints median / min / max per path and the ratios of the
medians, then how far the two results are apart.  --gae-only: warm-up and seven calls of each gae form and nothing else, the run to put under
`rocprofv3 --kernel-trace --stats -- python tools/gae_ab.py --gae-only` for the kernels' own times.  --out FILE: the printed lines go to that
file as well (profiles/gae.txt keeps one run)."""
import argparse
import os
import statistics
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "multiagent-quadruped-environment_amd")]
from mqe.envs.utils import make_mqe_env, custom_cfg      # noqa: E402
from mqe.utils.helpers import finish_args                # noqa: E402


@torch.no_grad()
def torch_gae(reward, value, done, time_outs, gamma, lam, normalize):
    """rsl_rl: process_env_step's bootstrap, compute_returns' loop, and its normalisation"""
    T = reward.shape[0]
    reward = reward + gamma * value[:-1] * time_outs.unsqueeze(-1).float()
    returns = torch.empty_like(reward)
    advantage = 0
    for step in reversed(range(T)):
        next_is_not_terminal = 1.0 - done[step].unsqueeze(-1).float()
        delta = reward[step] + next_is_not_terminal * gamma * value[step + 1] - value[step]
        advantage = delta + next_is_not_terminal * gamma * lam * advantage
        returns[step] = advantage + value[step]
    advantages = returns - value[:-1]
    if normalize:
        advantages = (advantages - advantages.mean()) / (advantages.std() + 1e-8)
    return advantages, returns


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--T", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--gae-only", action="store_true")
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--gamma", type=float, default=0.99)
    ap.add_argument("--lam", type=float, default=0.95)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
    dev = "cuda:0"
    margs = finish_args(types.SimpleNamespace(task="go1gate", num_envs=a.envs, seed=0, headless=True, record_video=False, sim_device=dev,
                                              pipeline="gpu", subscenes=0, num_threads=0))
    env = make_mqe_env("go1gate", margs, custom_cfg(margs))[0]
    nn = torch.nn
    D, H = env.observation_space.shape[0], a.hidden
    torch.manual_seed(0)
    actor = nn.Sequential(nn.Linear(D, H), nn.Tanh(), nn.Linear(H, H), nn.Tanh(), nn.Linear(H, 3)).to(dev)
    critic = nn.Sequential(nn.Linear(D, H), nn.Tanh(), nn.Linear(H, H), nn.Tanh(), nn.Linear(H, 1)).to(dev)
    env.set_actor(actor, critic, log_std=torch.full((3,), -0.5, device=dev))
    env.reset()
    eng = env.env.engine
    T, g, lam = a.T, a.gamma, a.lam

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    def group(title, paths, reps=1):
        ms = {n: [] for n in paths}
        for _ in range(2):
            for fn in paths.values():
                fn()

        def window(fn):
            for _ in range(reps):
                fn()
        for r in range(a.rounds):
            for n, fn in paths.items():
                ms[n].append(timed(lambda: window(fn))[0] / reps)
        for n, v in ms.items():
            say(f"{title} {n:28s} median {statistics.median(v):9.4f} ms  min {min(v):9.4f}  max {max(v):9.4f}  "
                f"(spread {(max(v) - min(v)) / statistics.median(v) * 100:.1f} %) over {len(v)} windows")
        return {n: statistics.median(v) for n, v in ms.items()}

    if a.gae_only:
        traj = eng.rollout(T, time_outs=True)
        for _ in range(7):
            eng.gae(traj, g, lam, out=traj)
            eng.gae(traj, g, lam, normalize=True, out=traj)
        torch.cuda.synchronize()
        print(f"gae-only: 7 calls of gae and 7 of gae(normalize=True) on one trajectory of {T} steps at {a.envs} envs done")
        env.close()
        return
    say(f"go1gate {a.envs} envs x 2 agents, T = {T}, hidden {H}, gamma {g}, lam {lam}, {torch.cuda.get_device_name(0)}")
    m = ma = group("(a)", {"rollout(T)": lambda: eng.rollout(T), "rollout(T, time_outs=True)": lambda: eng.rollout(T, time_outs=True)})
    say(f"(a) time-out record: {(m['rollout(T, time_outs=True)'] / m['rollout(T)'] - 1) * 100:+.2f} % of the rollout "
        f"({(m['rollout(T, time_outs=True)'] - m['rollout(T)']) * 1e3 / T:+.2f} us per step), medians")
    for _ in range(int(env.env.max_episode_length) // T + 2):
        traj = eng.rollout(T, time_outs=True)
        if bool(traj.done.any()):
            break
    say(f"trajectory: {int(traj.done.sum())} dones, {int(traj.time_outs.sum())} of them time-outs, in {T * a.envs} env-steps")
    tg = lambda norm: (lambda: torch_gae(traj.reward, traj.value, traj.done, traj.time_outs, g, lam, norm))
    m = group("(b, c)", {"gae": lambda: eng.gae(traj, g, lam, out=traj), "gae normalize": lambda: eng.gae(traj, g, lam, normalize=True, out=traj),
                         "torch loop": tg(False), "torch loop normalize": tg(True)}, reps=a.reps)
    say(f"(b) normalisation adds {(m['gae normalize'] - m['gae']) * 1e3:.1f} us to gae's {m['gae'] * 1e3:.1f} us")
    say(f"(c) torch loop / gae (medians): {m['torch loop'] / m['gae']:.1f} x;  with normalisation: {m['torch loop normalize'] / m['gae normalize']:.1f} x")
    rollout_ms = ma["rollout(T)"]
    say(f"gae is {m['gae'] / rollout_ms * 100:.3f} % of a rollout(T) window ({rollout_ms:.2f} ms); the torch loop {m['torch loop'] / rollout_ms * 100:.2f} %")
    eng.gae(traj, g, lam)
    adv_t, ret_t = torch_gae(traj.reward, traj.value, traj.done, traj.time_outs, g, lam, False)
    say(f"engine against torch loop (both float32, different roundings): max |adv| diff {float((traj.advantages - adv_t).abs().max()):.3e}, "
        f"max |ret| diff {float((traj.returns - ret_t).abs().max()):.3e}")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    env.close()


if __name__ == "__main__":
    main()
