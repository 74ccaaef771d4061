"""Layer normalisation inside the engine's actor-critic against the plain networks, and the plain path against a library of the parent commit:
go1gate 4096 envs x 2 agents, T = 200, two 64 x 64 tanh networks.
  default     one process, TWO handles of the same scene -- one actor created without the switches (k_actor, k_ppo_grad), one with both
              (k_actor_ln, k_ln_grad) -- and the windows of the two alternated --rounds times:
              (a) rollout(T) per step: the physics launches are the same on both handles, so the difference of the medians is k_actor_ln - k_actor;
              (b) one ppo_update epoch (--minibatches slices: per slice the gradient pair of launches + k_ppo_reduce + Adam).
  --plain-only   the plain handle alone: what a library of the parent commit (MQE_HIP_LIB) runs too.
  --parent LIB   starts NO GPU work itself: alternates child processes --rounds times -- this tool --plain-only and `bench.py --gpus 1` -- once
              with the in-tree library and once with MQE_HIP_LIB=LIB (a build of the parent commit), and prints per path the medians of both and
              their spread.  The plain path is expected inside the alternating windows' own spread of the parent.
  --all-paths    with --parent: the children run without --plain-only, for a parent library that has the norm kernels too: all four paths
              (rollout and epoch, plain and with norms) for both libraries.
Every measuring child first prints, per handle, LAYER_NORM_DIGEST: the SHA-256 of the bytes of the handle's first rollout (fixed seeds; actions,
logp, value) and of one ppo_grad on it (grad, stats), taken before any timing, while the handle is as created.  --parent prints whether the two
libraries' digests are equal: the same bits, which the tests' float64 bounds do not show.
  --trace-only   warm-up and seven rollout steps / gradient calls on the handle with the switches and nothing else: the run to put under
              `rocprofv3 --kernel-trace --stats -- python tools/layer_norm_ab.py --trace-only` for the kernels' own times.
Every figure of the first two modes is a HIP-event time (events recorded on the stream around a window, synchronised after it); all paths are
warmed up.  --out FILE: the printed lines go to that file as well (profiles/layer_norm.txt keeps one run)."""
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


def networks(D, H, norms, dev):
    import torch
    nn = torch.nn

    def net(out):
        layers, k = ([nn.LayerNorm(D)] if norms else []), D
        for _ in range(2):
            layers += [nn.Linear(k, H), nn.Tanh()] + ([nn.LayerNorm(H)] if norms else [])
            k = H
        return nn.Sequential(*layers, nn.Linear(k, out)).to(dev)
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
    kinds = ["plain"] if a.plain_only else (["norms"] if a.trace_only else ["plain", "norms"])
    T, mb = a.T, a.minibatches
    kw = dict(clip=0.2, value_coef=1.0, entropy_coef=0.01, value_clip=0.2)
    handles = {}
    for kind in kinds:
        env = make_mqe_env("go1gate", margs, custom_cfg(margs))[0]
        D = env.observation_space.shape[0]
        actor, critic = networks(D, a.hidden, kind == "norms", dev)
        env.set_actor(actor, critic, log_std=torch.full((3,), -0.5, device=dev), **({"layer_norm": True} if kind == "norms" else {}))
        env.reset()
        eng = env.env.engine
        traj = eng.gae(eng.rollout(T, time_outs=True), 0.99, 0.95, normalize=True)
        handles[kind] = (env, eng, traj)
    total = T * a.envs * 2
    digest = {}
    for kind, (_, eng, traj) in ({} if a.trace_only else handles).items():      # the first rollout of a fresh handle and one gradient on it: before anything is timed or updated
        grad, stats = eng.ppo_grad(traj, first=0, count=total // mb, **kw)
        torch.cuda.synchronize()
        h = hashlib.sha256()
        for t in (traj.actions, traj.logp, traj.value, grad, stats):
            h.update(t.detach().cpu().contiguous().numpy().tobytes())
        digest[kind] = h.hexdigest()
    if digest:
        print("LAYER_NORM_DIGEST " + json.dumps(digest), flush=True)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    if a.trace_only:
        _, eng, traj = handles["norms"]
        grad, stats = torch.empty(eng.actor_params()["flat"].numel(), device=dev), torch.empty(6, device=dev)
        perm = torch.randperm(total, device=dev).to(torch.int32)
        short = eng.rollout(2)
        for _ in range(9):
            eng.rollout(2, out=short)
            eng.ppo_grad(traj, index=perm, first=0, count=total // mb, out=(grad, stats), **kw)
        torch.cuda.synchronize()
        print(f"trace-only: 18 steps of k_actor_ln and 9 calls of k_ln_grad (minibatch of {total // mb} samples) done")
    else:
        say(f"go1gate {a.envs} envs x 2 agents, T = {T}: {total} samples, {mb} minibatches of {total // mb}, hidden {a.hidden} x {a.hidden} tanh, "
            f"{torch.cuda.get_device_name(0)}, library {os.environ.get('MQE_HIP_LIB', 'in-tree')}" + (" -- the plain handle only" if a.plain_only else ""))
        paths = {}
        for kind, (env, eng, traj) in handles.items():
            paths[f"(a) rollout per step, {kind}"] = (lambda eng=eng, traj=traj: eng.rollout(T, out=traj), 1e3 / T, "us")
            paths[f"(b) ppo_update epoch, {kind}"] = (lambda eng=eng, traj=traj: eng.ppo_update(traj, epochs=1, minibatches=mb, lr=1e-4, max_grad_norm=1.0, **kw), 1.0, "ms")
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
            say(f"{n:34s} median {med[n]:10.3f} {paths[n][2]}  min {min(v):10.3f}  max {max(v):10.3f}  (spread {spread(v):.1f} %) over {len(v)} windows")
        if len(kinds) == 2:
            da = med["(a) rollout per step, norms"] - med["(a) rollout per step, plain"]
            db = med["(b) ppo_update epoch, norms"] - med["(b) ppo_update epoch, plain"]
            say(f"(a) the norms add {da:.2f} us to a rollout step of {med['(a) rollout per step, plain']:.2f} us: k_actor_ln against k_actor")
            say(f"(b) the norms add {db * 1e3:.1f} us to an epoch of {med['(b) ppo_update epoch, plain']:.3f} ms ({mb} minibatches): k_ln_grad against k_ppo_grad, "
                f"{handles['norms'][1].actor_params()['flat'].numel()} parameters against {handles['plain'][1].actor_params()['flat'].numel()}")
        print("LAYER_NORM_AB " + json.dumps(med), flush=True)
    for env, _, _ in handles.values():
        env.close()


def against_parent(a, say):
    """child processes only: the in-tree library and the parent's, alternated"""
    me = os.path.abspath(__file__)
    jobs = {"tool": [sys.executable, me, *([] if a.all_paths else ["--plain-only"]), "--envs", str(a.envs), "--T", str(a.T), "--rounds", str(a.rounds), "--minibatches", str(a.minibatches)],
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
                if out.returncode != 0:
                    say(f"{job} with the {lib} library ended with {out.returncode}: {out.stderr[-400:]}")
                    return 1
                if job == "tool":
                    digests.setdefault(lib, set()).add(next(l for l in out.stdout.splitlines() if l.startswith("LAYER_NORM_DIGEST ")))
                    line = next(l for l in out.stdout.splitlines() if l.startswith("LAYER_NORM_AB "))
                    for n, v in json.loads(line[len("LAYER_NORM_AB "):]).items():
                        got.setdefault((n, lib), []).append(v)
                else:
                    res = json.loads(next(l for l in reversed(out.stdout.splitlines()) if l.startswith("{")))
                    got.setdefault(("bench.py ms_per_step", lib), []).append(res["ms_per_step"])
    say(f"{'all four paths' if a.all_paths else 'plain path'}, in-tree library against {a.parent}: {a.parent_rounds} alternated child processes each")
    for lib, lines in digests.items():
        say(f"{lib:8s} {' | '.join(sorted(lines))}")
    same = len(digests["in-tree"]) == 1 and digests["in-tree"] == digests["parent"]
    say("digests of the in-tree and the parent library: " + ("EQUAL in every child, for every handle" if same else "DIFFERENT"))
    for n in sorted({n for n, _ in got}):
        mine, base = got[(n, "in-tree")], got[(n, "parent")]
        m, b = statistics.median(mine), statistics.median(base)
        say(f"{n:34s} in-tree median {m:10.4f} ({min(mine):.4f} .. {max(mine):.4f})   parent median {b:10.4f} ({min(base):.4f} .. {max(base):.4f})   "
            f"{(m / b - 1) * 100:+.2f} %, the parent's own spread {spread(base):.2f} %")
    return 0 if same else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--T", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--minibatches", type=int, default=4)
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--parent", default=None, metavar="LIB")
    ap.add_argument("--all-paths", action="store_true")
    ap.add_argument("--parent-rounds", type=int, default=3)
    ap.add_argument("--bench-steps", type=int, default=300)
    ap.add_argument("--child-timeout", type=int, default=300)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
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
