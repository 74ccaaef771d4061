"""The recurrent PPO update inside the engine (mqe_ppo_grad with MQE_PPO_BPTT: k_bptt_grad / k_bptt_ln_grad; csrc/kernels_bptt.hpp) against the torch
learner it replaces, on the same tensors: go1gate 4096 envs x 2 agents, T = 200, two 64 x 64 tanh recurrent networks (tools/actor_ab.py's), one epoch of
--minibatches slices of the (T / L) x N x A' chunks at --chunk-length L.  --kinds: gru (no norms, 64-chunk tiles), gru_norms (both norms, 32-chunk tiles).
    engine   env.ppo_update(traj, epochs=1, minibatches, chunk_length=L, max_grad_norm=1): per slice k_bptt_[ln_]grad + k_ppo_reduce + k_ppo_norm + k_ppo_adam
    torch    per slice of the SAME device permutation: RecurrentMLP.evaluate of both twins over the chunks from the masked recorded state (traj.hidden),
             the same loss, backward, clip_grad_norm_(1), torch.optim.Adam.step, and at the end of the epoch env.sync_actor()
Both are warmed up, alternated --rounds times and timed with HIP events around the whole epoch.  The parameters are restored before every window, so
every window does the same work.  The plain paths and bench.py against a library of the parent commit are tools/actor_ab.py --parent LIB --kinds plain,norms.
--loss plain,joint,dual,joint+dual: the engine's epoch under each policy-loss head (MQE_PPO_JOINT, MQE_PPO_DUAL_CLIP at c_d = 3; under the joint loss the
minibatches are sets of chunk groups), alternated in the same way, without the torch path.
--out FILE: the printed lines go to that file as well (profiles/bptt.txt keeps one run)."""
import argparse
import math
import os
import statistics
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "multiagent-quadruped-environment_amd"), os.path.dirname(os.path.abspath(__file__))]

from actor_ab import KINDS, networks, spread  # noqa: E402


def torch_epoch(env, traj, actor, critic, log_std, opt, perm, mb, L, kw):
    import torch
    T, N, Aw = traj.actions.shape[:3]
    R, Ha = N * Aw, actor.rnn.hidden_size
    obs, hid = traj.obs.reshape(T + 1, R, -1), traj.hidden.reshape(T + 1, R, -1)
    mask = torch.cat([torch.ones(1, N, device=obs.device), (~traj.done).float()])[:, :, None].expand(T + 1, N, Aw).reshape(T + 1, R)      # of the step before
    flat = lambda x: x.reshape(T, R, *x.shape[3:])
    act, lpo, adv, vo, ret = flat(traj.actions), flat(traj.logp), flat(traj.advantages), flat(traj.value[:T]), flat(traj.returns)
    steps = torch.arange(L, device=obs.device)[:, None]
    per = perm.numel() // mb
    params = list(actor.parameters()) + list(critic.parameters()) + [log_std]
    for b in range(mb):
        c = perm[b * per:(b + 1) * per if b + 1 < mb else None].long()
        t, r = (c // R)[None, :] * L + steps, (c % R)[None, :]
        m = mask[t, r][..., None]
        mean, _ = actor.evaluate(obs[t, r], hid[t[0], r[0], :Ha], m)
        v, _ = critic.evaluate(obs[t, r], hid[t[0], r[0], Ha:], m)
        z = (act[t, r] - mean) * torch.exp(-log_std)
        logp = (-0.5 * z * z - log_std).sum(-1) - 1.5 * math.log(2 * math.pi)
        ratio = torch.exp(logp - lpo[t, r])
        Lpi = -torch.minimum(ratio * adv[t, r], torch.clamp(ratio, 1 - kw["clip"], 1 + kw["clip"]) * adv[t, r])
        v = v[..., 0]
        v_c = vo[t, r] + torch.clamp(v - vo[t, r], -kw["value_clip"], kw["value_clip"])
        Lv = torch.maximum((v - ret[t, r]) ** 2, (v_c - ret[t, r]) ** 2)
        loss = Lpi.mean() + kw["value_coef"] * Lv.mean() - kw["entropy_coef"] * (log_std.sum() + 1.5 * (1 + math.log(2 * math.pi)))
        opt.zero_grad(set_to_none=True)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(params, 1.0)
        opt.step()
    env.sync_actor()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kinds", default="gru,gru_norms", type=lambda s: s.split(","))
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--T", type=int, default=200)
    ap.add_argument("--chunk-length", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--minibatches", type=int, default=4)
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--loss", default="plain", type=lambda s: s.split(","),
                    help="comma list out of plain, joint, dual, joint+dual (c_d = 3): with more than plain, the engine's epoch per loss, alternated, no torch path")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from mqe.envs.utils import make_mqe_env, custom_cfg
    from mqe.utils.helpers import finish_args
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    dev = "cuda:0"
    margs = finish_args(types.SimpleNamespace(task="go1gate", num_envs=a.envs, seed=0, headless=True, record_video=False, sim_device=dev, pipeline="gpu",
                                              subscenes=0, num_threads=0))
    T, L, mb = a.T, a.chunk_length, a.minibatches
    chunks = T // L * a.envs * 2
    kw = dict(clip=0.2, value_coef=1.0, entropy_coef=0.01, value_clip=0.2)
    say(f"go1gate {a.envs} envs x 2 agents, T = {T}, chunk length {L}: {chunks} chunks = {chunks * L} samples, {mb} minibatches of {chunks // mb} chunks, "
        f"hidden {a.hidden} x {a.hidden} tanh recurrent, {torch.cuda.get_device_name(0)}")
    for kind in a.kinds:
        norms, recurrent = KINDS[kind]
        assert recurrent, "--kinds: gru, gru_norms"
        env = make_mqe_env("go1gate", margs, custom_cfg(margs))[0]
        actor, critic = networks(env.observation_space.shape[0], a.hidden, norms, True, dev)
        log_std = torch.full((3,), -0.5, device=dev, requires_grad=True)
        env.set_actor(actor, critic, log_std=log_std, **({"layer_norm": True} if norms else {}), recurrent=True)
        env.reset()
        eng = env.env.engine
        traj = env.rollout(T, gamma=0.99, lam=0.95, normalize_advantages=True, record_hidden=True)
        start = eng.actor_params()["flat"].clone()
        opt = torch.optim.Adam(list(actor.parameters()) + list(critic.parameters()) + [log_std], lr=1e-4)
        perm = torch.randperm(chunks, device=dev, generator=torch.Generator(device=dev).manual_seed(1)).to(torch.int32)

        def restore():
            eng.actor_params()["flat"].copy_(start)
            env.pull_actor()

        paths = {"engine": lambda: env.ppo_update(traj, epochs=1, minibatches=mb, lr=1e-4, max_grad_norm=1.0, chunk_length=L,
                                                  generator=torch.Generator(device=dev).manual_seed(1), **kw),
                 "torch": lambda: torch_epoch(env, traj, actor, critic, log_std, opt, perm, mb, L, kw)}
        if a.loss != ["plain"]:                # the loss heads of csrc/kernels_ppo.hpp against each other: the engine's epoch alone
            heads = {"plain": {}, "joint": dict(joint=True), "dual": dict(dual_clip=3.0), "joint+dual": dict(joint=True, dual_clip=3.0)}
            paths = {n: (lambda lkw=heads[n]: env.ppo_update(traj, epochs=1, minibatches=mb, lr=1e-4, max_grad_norm=1.0, chunk_length=L,
                                                             generator=torch.Generator(device=dev).manual_seed(1), **kw, **lkw)) for n in a.loss}
        ms = {n: [] for n in paths}
        for n, fn in paths.items():            # warm-up: the first engine call allocates its scratch and synchronises once
            restore()
            fn()
        for _ in range(a.rounds):
            for n, fn in paths.items():
                restore()
                ms[n].append(timed(fn))
        for n, v in ms.items():
            say(f"ppo_update epoch, {kind:9s} {n:6s} median {statistics.median(v):10.3f} ms  min {min(v):10.3f}  max {max(v):10.3f}  (spread {spread(v):.1f} %) "
                f"over {len(v)} windows")
        if a.loss != ["plain"]:
            env.close()
            continue
        e, t = statistics.median(ms["engine"]), statistics.median(ms["torch"])
        say(f"ppo_update epoch, {kind:9s} engine / torch = {e / t:.3f}" + ("" if e <= t else "  (the engine's update is SLOWER than the torch learner)"))
        env.close()
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
