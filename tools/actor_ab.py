"""The four forms of the engine's actor-critic against each other, and all of them against a library of the parent commit: go1gate 4096 envs x 2 agents,
T = 200, two 64 x 64 tanh networks.  --kinds: a comma list out of
    plain      k_actor, k_ppo_grad                          norms      both layer norms: k_actor_ln, k_ln_grad
    gru        a GRU cell in both networks: k_actor_gru      gru_norms  the cells and both norms: k_actor_gru_ln
    mat        the Multi-Agent Transformer at n_embd = --hidden: k_actor_mat (not in the default list: a parent library may not know it).  Its paths:
               rollout(T) per step, and the same steps with the torch twin around step_torch -- MATNet.act on the device, then
               mqe_openrl_wrapper.step_torch, no host synchronisation in the loop; one ppo_update(transformer=True) epoch (k_mat_grad: per slice
               k_joint_expand, the gradient, k_mat_reduce, Adam) and the same epoch by a torch learner -- MATNet on the device, autograd of the same
               loss over the same number of slices, clip_grad_norm_, torch.optim.Adam, then sync_actor() -- which is the only way a library without
               the gradient has (such a library is noticed and measured through the torch learner alone).  Its digest covers the first rollout's
               actions, logp, value and the advantages of gae
  default     one process, one handle of the same scene per kind, the windows of all of them alternated --rounds times:
              rollout(T) per step, every kind: the physics launches are the same on every handle, so a difference of medians is a difference of the
                  rollout kernels (+ the recorded tails, for "recorded");
              one ppo_update epoch (--minibatches slices), the kinds without a cell: per slice the gradient pair of launches + k_ppo_reduce + Adam;
              rollout(T, record_hidden=True) per step, the kinds with a cell;
              one ppo_update(chunk_length=--chunk, value_norm=True) epoch on the gru handle, whose actor also keeps value normalisation: per slice
                  k_bptt_expand, k_vn_moments, k_vn_apply, the recurrent gradient pair and Adam.
  --parent LIB   starts NO GPU work itself: alternates child processes --parent-rounds times -- this tool with the same --kinds and `bench.py --gpus 1` --
              once with the in-tree library and once with MQE_HIP_LIB=LIB (a build of the parent commit), stops at the first child that does not exit 0,
              and prints per kind whether the digests are equal and per path the medians of both and the parent's own min .. max over the alternated blocks.
Every measuring child first prints ACTOR_DIGEST {kind: sha256}, taken before any timing while the handle is as created (fixed seeds): the bytes of the
first rollout's actions, logp and value and one ppo_grad on it (grad, stats); with a cell the rollout is a recorded one, traj.hidden is covered too and
the gradient is ppo_grad(chunk_length=--chunk); the gru handle adds a second call over a reversed chunk list with value_norm and update_value_norm, and
the bytes of actor_params()["value_norm"] behind it.  The same bits out, which the tests' float64 bounds do not show.
  --trace-only KIND   that handle alone, warm-up and then two rollouts of T steps and, without a cell, nine gradient calls: the run to put under
              `rocprofv3 --kernel-trace --stats -- python tools/actor_ab.py --trace-only KIND` for the kernels' own times.
Every figure is a HIP-event time (events recorded on the stream around a window, synchronised after it); all paths are warmed up.
--out FILE: the printed lines go to that file as well (profiles/actor_host_ab.txt keeps one run)."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "multiagent-quadruped-environment_amd")]

KINDS = {"plain": (False, False), "norms": (True, False), "gru": (False, True), "gru_norms": (True, True), "mat": (False, False)}      # (both norms, a GRU cell)
MAT_KIND = "mat"     # the transformer: one MATNet instead of the two stacks
VN_KIND = "gru"      # the handle whose actor also keeps value normalisation (only the flagged calls below read or change it)


def networks(D, H, norms, recurrent, dev):
    import torch
    from mqe.utils.actor_net import RecurrentMLP
    nn = torch.nn

    def net(out):
        layers, k = ([nn.LayerNorm(D)] if norms else []), D
        for _ in range(2):
            layers += [nn.Linear(k, H), nn.Tanh()] + ([nn.LayerNorm(H)] if norms else [])
            k = H
        base = nn.Sequential(*layers)
        return (RecurrentMLP(base, out) if recurrent else nn.Sequential(*base, nn.Linear(H, out))).to(dev)
    torch.manual_seed(0)
    return net(3), net(1)


def spread(v):
    return (max(v) - min(v)) / statistics.median(v) * 100


def measure(a, say):
    import torch
    from mqe.envs.utils import make_mqe_env, custom_cfg
    from mqe.utils.helpers import finish_args
    dev = "cuda:0"
    margs = finish_args(types.SimpleNamespace(task="go1gate", num_envs=a.envs, seed=0, headless=True, record_video=False, sim_device=dev,
                                              pipeline="gpu", subscenes=0, num_threads=0))
    T, mb, total = a.T, a.minibatches, a.T * a.envs * 2
    kw = dict(clip=0.2, value_coef=1.0, entropy_coef=0.01, value_clip=0.2)
    handles, digest = {}, {}
    for kind in ([a.trace_only] if a.trace_only else a.kinds):
        norms, recurrent = KINDS[kind]
        env = make_mqe_env("go1gate", margs, custom_cfg(margs))[0]
        if kind == MAT_KIND:
            from mqe.utils.actor_net import MATNet
            torch.manual_seed(0)
            net = MATNet(env.observation_space.shape[0], a.hidden).to(dev)
            with torch.no_grad():
                net.log_std.fill_(-0.5)
            env.set_actor(net)
            obs = env.reset()
            eng = env.env.engine
            traj = eng.gae(eng.rollout(T, time_outs=True), 0.99, 0.95, normalize=True)
            torch.cuda.synchronize()
            h = hashlib.sha256()
            for t in (traj.actions, traj.logp, traj.value, traj.advantages):
                h.update(t.detach().cpu().contiguous().numpy().tobytes())
            digest[kind] = h.hexdigest()
            handles[kind] = (eng, traj, False, env)
            twin = (net, obs)
            try:                                       # a library of the parent commit refuses the flag as unknown; any other failure is one
                eng.ppo_grad(traj, first=0, count=T * a.envs // mb, transformer=True, **kw)
                mat_grad = True
            except RuntimeError as e:
                if "unknown bits in flags" not in str(e) and "not in the engine yet" not in str(e):
                    raise
                mat_grad = False
            continue
        actor, critic = networks(env.observation_space.shape[0], a.hidden, norms, recurrent, dev)
        env.set_actor(actor, critic, log_std=torch.full((3,), -0.5, device=dev), **({"layer_norm": True} if norms else {}), **({"recurrent": True} if recurrent else {}),
                      **({"value_norm": True} if kind == VN_KIND else {}))
        env.reset()
        eng = env.env.engine
        # the first rollout of a fresh handle [and one gradient on it]: before anything is timed or updated
        if recurrent:
            traj = eng.gae(eng.rollout(T, record_hidden=True, time_outs=True), 0.99, 0.95, normalize=True, value_norm=False)
            chunks = total // a.chunk
            covered = (traj.actions, traj.logp, traj.value, traj.hidden, *eng.ppo_grad(traj, first=0, count=chunks // mb, chunk_length=a.chunk, value_norm=False, **kw))
            if kind == VN_KIND:
                last_first = torch.arange(chunks - 1, -1, -1, device=dev, dtype=torch.int32)
                covered += (*eng.ppo_grad(traj, index=last_first, first=3, count=chunks // mb, chunk_length=a.chunk, value_norm=True, update_value_norm=True, **kw),
                            eng.actor_params()["value_norm"])
        else:
            traj = eng.gae(eng.rollout(T, time_outs=True), 0.99, 0.95, normalize=True)
            covered = (traj.actions, traj.logp, traj.value, *eng.ppo_grad(traj, first=0, count=total // mb, **kw))
        torch.cuda.synchronize()
        h = hashlib.sha256()
        for t in covered:
            h.update(t.detach().cpu().contiguous().numpy().tobytes())
        digest[kind] = h.hexdigest()
        handles[kind] = (eng, traj, recurrent, env)
    print("ACTOR_DIGEST " + json.dumps(digest), flush=True)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    if a.trace_only:
        eng, traj, recurrent, _ = handles[a.trace_only]
        for _ in range(2):
            eng.rollout(T, out=traj, **({"record_hidden": True} if recurrent else {}))
        if a.trace_only == MAT_KIND and mat_grad:
            grad, stats = torch.empty(eng.actor_params()["flat"].numel(), device=dev), torch.empty(6, device=dev)
            perm = torch.randperm(T * a.envs, device=dev).to(torch.int32)
            for _ in range(9):
                eng.ppo_grad(traj, index=perm, first=0, count=T * a.envs // mb, out=(grad, stats), transformer=True, **kw)
        if not recurrent and a.trace_only != MAT_KIND:
            grad, stats = torch.empty(eng.actor_params()["flat"].numel(), device=dev), torch.empty(6, device=dev)
            perm = torch.randperm(total, device=dev).to(torch.int32)
            for _ in range(9):
                eng.ppo_grad(traj, index=perm, first=0, count=total // mb, out=(grad, stats), **kw)
        torch.cuda.synchronize()
        print(f"trace-only {a.trace_only}: {3 * T} rollout steps" + ("" if recurrent or (a.trace_only == MAT_KIND and not mat_grad) else f" and 10 gradient calls (minibatch of {total // mb} samples)") + " done")
    else:
        say(f"go1gate {a.envs} envs x 2 agents, T = {T}: {total} samples, {mb} minibatches of {total // mb}, hidden {a.hidden} x {a.hidden} tanh, "
            f"{torch.cuda.get_device_name(0)}, library {os.environ.get('MQE_HIP_LIB', 'in-tree')}, kinds {','.join(a.kinds)}")
        paths = {}
        for kind, (eng, traj, recurrent, env) in handles.items():
            if kind == MAT_KIND:
                from openrl_ws.utils import mqe_openrl_wrapper
                net, state = twin[0], {"obs": twin[1], "w": mqe_openrl_wrapper(env)}

                def torch_steps(net=net, state=state):
                    with torch.no_grad():
                        for _ in range(T):
                            act, _, _ = net.act(state["obs"])
                            state["obs"] = state["w"].step_torch(act)[0]
                paths[f"rollout per step, {kind}"] = (lambda eng=eng, traj=traj: eng.rollout(T, out=traj), 1e3 / T, "us")
                paths[f"torch twin + step_torch, {kind}"] = (torch_steps, 1e3 / T, "us")
                learner = torch.optim.Adam(net.parameters(), lr=1e-4)
                G, D = T * a.envs, traj.obs.shape[-1]
                flat = dict(obs=traj.obs[:T].reshape(G, 2, D), act=traj.actions.reshape(G, 2, 3), lpo=traj.logp.reshape(G, 2), vo=traj.value[:T].reshape(G, 2),
                            adv=traj.advantages.reshape(G, 2), ret=traj.returns.reshape(G, 2))

                def torch_epoch(net=net, env=env, flat=flat, G=G):
                    """ppo_update(transformer=True)'s epoch in torch: the same loss (csrc/kernels_mat_grad.hpp), slices, norm clip and optimiser"""
                    perm = torch.randperm(G, device=dev)
                    per = G // mb
                    for b in range(mb):
                        g = perm[b * per:] if b + 1 == mb else perm[b * per:(b + 1) * per]
                        _, logp, v = net.evaluate(flat["obs"][g], flat["act"][g])
                        ratio, adv, vo, ret = torch.exp(logp - flat["lpo"][g]), flat["adv"][g], flat["vo"][g], flat["ret"][g]
                        l_pi = -torch.minimum(ratio * adv, torch.clamp(ratio, 1 - kw["clip"], 1 + kw["clip"]) * adv).mean()
                        v_c = vo + torch.clamp(v - vo, -kw["value_clip"], kw["value_clip"])
                        l_v = torch.maximum((v - ret) ** 2, (v_c - ret) ** 2).mean()
                        entropy = torch.log(net.sigma()).sum() + 1.5 * (1.0 + 1.8378770664093453)
                        loss = l_pi + kw["value_coef"] * l_v - kw["entropy_coef"] * entropy
                        learner.zero_grad(set_to_none=True)
                        loss.backward()
                        torch.nn.utils.clip_grad_norm_(net.parameters(), 1.0)
                        learner.step()
                    env.sync_actor()
                if mat_grad:
                    paths[f"ppo_update epoch, {kind}, on-device"] = (lambda eng=eng, traj=traj: eng.ppo_update(
                        traj, epochs=1, minibatches=mb, lr=1e-4, max_grad_norm=1.0, transformer=True, **kw), 1.0, "ms")
                paths[f"ppo_update epoch, {kind}, torch learner"] = (torch_epoch, 1.0, "ms")
            elif recurrent:
                plain = eng.rollout(T)
                paths[f"rollout per step, {kind}"] = (lambda eng=eng, plain=plain: eng.rollout(T, out=plain), 1e3 / T, "us")
                paths[f"rollout per step, {kind}, recorded"] = (lambda eng=eng, traj=traj: eng.rollout(T, out=traj, record_hidden=True), 1e3 / T, "us")
                if kind == VN_KIND:
                    paths[f"ppo_update epoch, {kind}, value_norm"] = (lambda eng=eng, traj=traj: eng.ppo_update(
                        traj, epochs=1, minibatches=mb, lr=1e-4, max_grad_norm=1.0, chunk_length=a.chunk, value_norm=True, **kw), 1.0, "ms")
            else:
                paths[f"rollout per step, {kind}"] = (lambda eng=eng, traj=traj: eng.rollout(T, out=traj), 1e3 / T, "us")
                paths[f"ppo_update epoch, {kind}"] = (lambda eng=eng, traj=traj: eng.ppo_update(traj, epochs=1, minibatches=mb, lr=1e-4, max_grad_norm=1.0, **kw), 1.0, "ms")
        ms = {n: [] for n in paths}
        for _ in range(2):
            for fn, _, _ in paths.values():
                fn()
        for _ in range(a.rounds):
            for n, (fn, scale, _) in paths.items():
                ms[n].append(timed(fn) * scale)
        med = {}
        for n, v in ms.items():
            med[n] = statistics.median(v)
            say(f"{n:38s} median {med[n]:10.3f} {paths[n][2]}  min {min(v):10.3f}  max {max(v):10.3f}  (spread {spread(v):.1f} %) over {len(v)} windows")
        print("ACTOR_AB " + json.dumps(med), flush=True)
    for *_, env in handles.values():
        env.close()


def against_parent(a, say):
    """child processes only: the in-tree library and the parent's, alternated"""
    jobs = {"tool": [sys.executable, os.path.abspath(__file__), "--kinds", ",".join(a.kinds), "--envs", str(a.envs), "--T", str(a.T), "--rounds", str(a.rounds),
                     "--minibatches", str(a.minibatches), "--hidden", str(a.hidden), "--chunk", str(a.chunk)],
            "bench": [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(a.bench_steps), "--warmup", "50", "--no_cpu_baseline",
                      "--no_strict_f32", "--no_configs"]}
    got, digests = {}, {}
    for r in range(a.parent_rounds):
        for lib in (("in-tree", "parent") if r % 2 == 0 else ("parent", "in-tree")):      # neither library always goes first
            env = dict(os.environ)
            env.pop("MQE_HIP_LIB", None)
            if lib == "parent":
                env["MQE_HIP_LIB"] = os.path.abspath(a.parent)
            for job, cmd in jobs.items():
                out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=a.child_timeout)
                print(f"round {r + 1} of {a.parent_rounds}, {lib} library, {job}: exit {out.returncode}", file=sys.stderr, flush=True)      # a sign of life: the result comes at the end
                if out.returncode != 0:
                    say(f"{job} with the {lib} library ended with {out.returncode}: {out.stderr[-400:]}")
                    return 1
                if job == "tool":
                    tagged = {tag: json.loads(l[len(tag) + 1:]) for l in out.stdout.splitlines() for tag in ("ACTOR_DIGEST", "ACTOR_AB") if l.startswith(tag + " ")}
                    for kind, d in tagged["ACTOR_DIGEST"].items():
                        digests.setdefault((kind, lib), set()).add(d)
                    for n, v in tagged["ACTOR_AB"].items():
                        got.setdefault((n, lib), []).append(v)
                else:
                    res = json.loads(next(l for l in reversed(out.stdout.splitlines()) if l.startswith("{")))
                    got.setdefault(("bench.py ms_per_step", lib), []).append(res["ms_per_step"])
    say(f"kinds {','.join(a.kinds)}, in-tree library against {a.parent}: {a.parent_rounds} alternated child processes each")
    same = True
    for kind in a.kinds:
        mine, base = digests[(kind, "in-tree")], digests[(kind, "parent")]
        equal = len(mine) == 1 and mine == base
        same = same and equal
        say(f"ACTOR_DIGEST {kind:10s} " + (f"EQUAL in every child: {next(iter(mine))}" if equal else f"DIFFERENT: in-tree {sorted(mine)} parent {sorted(base)}"))
    for n in sorted({n for n, _ in got}):
        mine, base = got[(n, "in-tree")], got[(n, "parent")]
        m, b = statistics.median(mine), statistics.median(base)
        say(f"{n:38s} in-tree median {m:10.4f} ({min(mine):.4f} .. {max(mine):.4f})   parent median {b:10.4f} ({min(base):.4f} .. {max(base):.4f})   "
            f"{m - b:+.4f} against the parent's own min-to-max {max(base) - min(base):.4f}: {'inside' if m - b <= max(base) - min(base) else 'MISSED'}")
    return 0 if same else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kinds", default=[k for k in KINDS if k != MAT_KIND], type=lambda s: s.split(","))
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--T", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--minibatches", type=int, default=4)
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--chunk", type=int, default=8, help="the chunk length of the recurrent gradient calls; divides --T")
    ap.add_argument("--trace-only", default=None, metavar="KIND", choices=list(KINDS))
    ap.add_argument("--parent", default=None, metavar="LIB")
    ap.add_argument("--parent-rounds", type=int, default=3)
    ap.add_argument("--bench-steps", type=int, default=300)
    ap.add_argument("--child-timeout", type=int, default=300)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    unknown = [k for k in a.kinds if k not in KINDS]
    if unknown:
        ap.error(f"--kinds: {unknown} (out of {','.join(KINDS)})")
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
    rc = against_parent(a, say) if a.parent else measure(a, say)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return rc or 0


if __name__ == "__main__":
    sys.exit(main())
