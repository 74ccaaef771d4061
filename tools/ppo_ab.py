"""The on-device PPO update against torch autograd: go1gate 4096 envs x 2 agents, T = 200, two 64 x 64 tanh networks, one epoch of 4
minibatches, one handle, one process, the two paths alternated --rounds times on the same trajectory.
  (a) ppo_update(traj, epochs=1, minibatches=4): per minibatch mqe_ppo_grad (k_ppo_grad, k_ppo_reduce) and mqe_ppo_adam (k_ppo_norm,
      k_ppo_adam) on the engine's own parameter buffer, plus the one torch.randperm of the epoch;
  (b) the same loss (rsl_rl's clipped surrogate, clipped value loss, entropy bonus) with torch autograd on the torch modules, gathering
      each minibatch from the trajectory's own tensors by the same kind of device permutation, clip_grad_norm_ and torch.optim.Adam, then
      sync_actor() to push the result into the buffer k_actor reads.
Every figure is a HIP-event time (events recorded on the stream around a window, synchronised after it); a window is one whole epoch; both
paths are warmed up.  Then the per-kernel times: each of the four kernels alone, --reps calls back to back inside one event window (a
single call would time the launch), on a 1/4 minibatch, with the arithmetic floor of DESIGN 3.5 beside k_ppo_grad.  Prints median / min /
max per path and the ratio of the medians.  --grad-only: warm-up and seven ppo_grad + adam_step calls and nothing else, the run to put under
`rocprofv3 --kernel-trace --stats -- python tools/ppo_ab.py --grad-only`.  --out FILE: the printed lines go to that file as well
(profiles/ppo.txt keeps one run, with the tests' figures).
--loss plain,joint,dual,joint+dual (default plain): the policy-loss heads to time (csrc/kernels_ppo.hpp: MQE_PPO_JOINT, MQE_PPO_DUAL_CLIP at c_d = 3).
With more than `plain` the windows are one ppo_update epoch per loss, alternated in this one process, each against the plain median; the torch path
and the per-kernel times are left out.  Every run but a --grad-only one first prints PPO_DIGEST {loss: sha256}: the bytes of the gradient and
statistics of one ppo_grad call per loss on the fresh handle with a fixed index list, before anything is timed or updated -- run once more with
MQE_HIP_LIB=<a build of the parent commit> and --loss plain, the line must be the same (profiles/joint_loss.txt keeps one such session)."""
import argparse
import hashlib
import json
import math
import os
import statistics
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "multiagent-quadruped-environment_amd")]
from mqe.envs.utils import make_mqe_env, custom_cfg      # noqa: E402
from mqe.utils.helpers import finish_args                # noqa: E402
from mqe.engine import abi                               # noqa: E402

LN2PI = math.log(2 * math.pi)


def torch_minibatch_loss(actor, critic, log_std, obs, actions, logp_old, v_old, adv, ret, clip, value_coef, entropy_coef, value_clip):
    mean, v = actor(obs), critic(obs)[:, 0]
    z = (actions - mean) * torch.exp(-log_std)
    logp = (-0.5 * z * z - log_std).sum(-1) - 1.5 * LN2PI
    ratio = torch.exp(logp - logp_old)
    l_pi = -torch.minimum(ratio * adv, torch.clamp(ratio, 1 - clip, 1 + clip) * adv).mean()
    v_c = v_old + torch.clamp(v - v_old, -value_clip, value_clip)
    l_v = torch.maximum((v - ret) ** 2, (v_c - ret) ** 2).mean()
    return l_pi + value_coef * l_v - entropy_coef * (log_std.sum() + 1.5 * (1 + LN2PI))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--T", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--minibatches", type=int, default=4)
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--grad-only", action="store_true")
    ap.add_argument("--loss", default="plain", help="comma-separated: plain, joint, dual, joint+dual")
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
    log_std = nn.Parameter(torch.full((3,), -0.5, device=dev))
    env.set_actor(actor, critic, log_std=log_std)
    env.reset()
    eng = env.env.engine
    T, mb = a.T, a.minibatches
    kw = dict(clip=0.2, value_coef=1.0, entropy_coef=0.01, value_clip=0.2)
    lr, max_norm = 1e-3, 1.0
    traj = env.rollout(T, gamma=0.99, lam=0.95, normalize_advantages=True)
    Aw = int(eng.tensor(abi.T_WRAPPER_OBS).shape[1])
    total = T * a.envs * Aw
    per = total // mb

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    if a.grad_only:
        grad = torch.empty(eng.actor_params()["flat"].numel(), device=dev)
        stats = torch.empty(6, device=dev)
        perm = torch.randperm(total, device=dev).to(torch.int32)
        for k in range(9):
            eng.ppo_grad(traj, index=perm, first=0, count=per, out=(grad, stats), **kw)
            eng.adam_step(grad, k + 1, lr, max_grad_norm=max_norm)
        torch.cuda.synchronize()
        print(f"grad-only: 9 calls of ppo_grad + adam_step on minibatches of {per} samples done")
        env.close()
        return

    losses = {"plain": {}, "joint": dict(joint=True), "dual": dict(dual_clip=3.0), "joint+dual": dict(joint=True, dual_clip=3.0)}
    losses = {n: losses[n] for n in a.loss.split(",")}
    digest = {}
    for n, lkw in losses.items():           # before anything is timed or updated: the handle as created, fixed seeds, a fixed index list
        units = total // Aw if lkw.get("joint") else total
        idx = torch.randperm(units, generator=torch.Generator().manual_seed(5)).to(torch.int32).to(dev)
        g, st = eng.ppo_grad(traj, index=idx, first=0, count=units // mb, **kw, **lkw)
        torch.cuda.synchronize()
        digest[n] = hashlib.sha256(g.cpu().numpy().tobytes() + st.cpu().numpy().tobytes()).hexdigest()
    print("PPO_DIGEST " + json.dumps(digest), flush=True)

    params = list(actor.parameters()) + list(critic.parameters()) + [log_std]
    opt = torch.optim.Adam(params, lr=lr)
    flat = lambda x, *tail: x.reshape(total, *tail)
    t_obs, t_act, t_lp, t_v = flat(traj.obs[:T], D), flat(traj.actions, 3), flat(traj.logp), flat(traj.value[:T])
    t_adv, t_ret = flat(traj.advantages), flat(traj.returns)

    def engine_epoch():
        eng.ppo_update(traj, epochs=1, minibatches=mb, lr=lr, max_grad_norm=max_norm, **kw)

    def torch_epoch():
        perm = torch.randperm(total, device=dev)
        for b in range(mb):
            sel = perm[b * per:(b + 1) * per if b + 1 < mb else total]
            loss = torch_minibatch_loss(actor, critic, log_std, t_obs[sel], t_act[sel], t_lp[sel], t_v[sel], t_adv[sel], t_ret[sel], **kw)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            torch.nn.utils.clip_grad_norm_(params, max_norm)
            opt.step()
        env.sync_actor()

    say(f"go1gate {a.envs} envs x 2 agents, T = {T}: {total} samples, {mb} minibatches of {per}, hidden {H} x {H} tanh, {torch.cuda.get_device_name(0)}")
    paths = {"(a) ppo_update": engine_epoch, "(b) torch autograd + Adam + sync_actor": torch_epoch}
    if list(losses) != ["plain"]:
        say(f"library {os.environ.get('MQE_HIP_LIB', 'in-tree')}; PPO_DIGEST {json.dumps(digest)}")
        paths = {f"ppo_update, {n}": (lambda lkw=lkw: eng.ppo_update(traj, epochs=1, minibatches=mb, lr=lr, max_grad_norm=max_norm, **kw, **lkw)) for n, lkw in losses.items()}
        ms = {n: [] for n in paths}
        for _ in range(2):
            for fn in paths.values():
                fn()
        for _ in range(a.rounds):
            for n, fn in paths.items():
                ms[n].append(timed(fn))
        base = statistics.median(ms[next(iter(ms))])
        for n, v in ms.items():
            m = statistics.median(v)
            say(f"{n:26s} median {m:9.3f} ms per epoch  min {min(v):9.3f}  max {max(v):9.3f}  (spread {(max(v) - min(v)) / m * 100:.1f} %) over {len(v)} windows"
                f"  = {m / base:.4f} x {next(iter(ms))}")
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        env.close()
        return
    ms = {n: [] for n in paths}
    for _ in range(2):
        for fn in paths.values():
            fn()
    for _ in range(a.rounds):
        for n, fn in paths.items():
            ms[n].append(timed(fn))
    med = {}
    for n, v in ms.items():
        med[n] = statistics.median(v)
        say(f"{n:42s} median {med[n]:9.3f} ms per epoch  min {min(v):9.3f}  max {max(v):9.3f}  (spread {(max(v) - min(v)) / med[n] * 100:.1f} %) over {len(v)} windows")
    ra, rb = med["(a) ppo_update"], med["(b) torch autograd + Adam + sync_actor"]
    say(f"library {os.environ.get('MQE_HIP_LIB', 'in-tree')}; PPO_DIGEST {json.dumps(digest)}")
    say(f"torch / engine (medians): {rb / ra:.2f} x  ({'the engine is faster' if rb > ra else 'TORCH IS FASTER'})")
    # the kernels alone
    grad = torch.empty(eng.actor_params()["flat"].numel(), device=dev)
    stats = torch.empty(6, device=dev)
    perm = torch.randperm(total, device=dev).to(torch.int32)
    step = [eng.ppo_step]

    def adam():
        step[0] += 1
        eng.adam_step(grad, step[0], lr, max_grad_norm=max_norm)
    singles = {"ppo_grad, shuffled index (k_ppo_grad + k_ppo_reduce)": lambda: eng.ppo_grad(traj, index=perm, first=0, count=per, out=(grad, stats), **kw),
               "ppo_grad, contiguous range": lambda: eng.ppo_grad(traj, first=0, count=per, out=(grad, stats), **kw),
               "adam_step (k_ppo_norm + k_ppo_adam)": adam,
               "torch.randperm + int32 cast": lambda: torch.randperm(total, device=dev).to(torch.int32)}
    for n, fn in singles.items():
        fn()
        v = [timed(lambda: [fn() for _ in range(a.reps)]) / a.reps for _ in range(a.rounds)]
        say(f"{n:56s} median {statistics.median(v) * 1e3:9.1f} us  min {min(v) * 1e3:9.1f}  max {max(v) * 1e3:9.1f}")
        if n.startswith("ppo_grad, shuffled"):
            grad_us = statistics.median(v) * 1e3
    macs = 2 * (D * H + H * H) + H * 3 + H * 1                 # multiply-adds per sample forward, both networks
    flop = 2 * 3 * macs * per
    say(f"k_ppo_grad arithmetic: {macs} multiply-adds per sample forward, x 3 with the backward = {flop / 1e9:.2f} GFLOP per minibatch; at 157.3 TFLOP/s "
        f"{flop / 157.3e12 * 1e6:.1f} us; measured {grad_us:.1f} us = {flop / 157.3e12 * 1e6 / grad_us * 100:.1f} % of the f32 peak")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    env.close()


if __name__ == "__main__":
    main()
