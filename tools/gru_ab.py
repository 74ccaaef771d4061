"""The recurrent actor-critic (a GRU cell in both networks; csrc/kernels_gru.hpp) against the plain networks inside the engine's rollout, and the plain
path against a library of the parent commit: go1gate 4096 envs x 2 agents, T = 200, two 64 x 64 tanh networks.
  default     one process, TWO handles of the same scene -- one actor created plain (k_actor), one recurrent (k_actor_gru) -- and the windows
              alternated in --rounds blocks: rollout(T) per step on the plain handle, on the recurrent handle without record_hidden and with it.
              The physics launches are the same on every handle, so the difference of the medians is k_actor_gru - k_actor (+ the recorded tails).
  --plain-only   the plain handle alone: what a library of the parent commit (MQE_HIP_LIB) runs too.
  --parent LIB   starts NO GPU work itself: alternates child processes --parent-rounds times -- this tool --plain-only and `bench.py --gpus 1` -- once
              with the in-tree library and once with MQE_HIP_LIB=LIB (a build of the parent commit), and prints per path the medians of both and
              the parent's own spread over the alternated blocks.  The plain path is expected inside that spread.
Every measuring child first prints GRU_DIGEST: the SHA-256 of the bytes of each handle's first rollout (fixed seeds; actions, logp, value), taken
before any timing.  --parent prints whether the two libraries' plain digests are equal: the same bits out.
  --trace-only   warm-up and a 200-step rollout on the recurrent handle and nothing else: the run to put under
              `rocprofv3 --kernel-trace --stats -- python tools/gru_ab.py --trace-only` for k_actor_gru's own time.
Every figure of the first two modes is a HIP-event time (events recorded on the stream around a window, synchronised after it); all paths are
warmed up.  --out FILE: the printed lines go to that file as well (profiles/gru.txt keeps one run)."""
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


def networks(D, H, recurrent, dev):
    import torch
    from mqe.utils.actor_net import RecurrentMLP
    nn = torch.nn

    def net(out):
        base = nn.Sequential(nn.Linear(D, H), nn.Tanh(), nn.Linear(H, H), nn.Tanh())
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
    kinds = ["plain"] if a.plain_only else (["gru"] if a.trace_only else ["plain", "gru"])
    T = a.T
    handles, digest = {}, {}
    for kind in kinds:
        env = make_mqe_env("go1gate", margs, custom_cfg(margs))[0]
        D = env.observation_space.shape[0]
        actor, critic = networks(D, a.hidden, kind == "gru", dev)
        env.set_actor(actor, critic, log_std=torch.full((3,), -0.5, device=dev), **({"recurrent": True} if kind == "gru" else {}))
        env.reset()
        eng = env.env.engine
        traj = eng.rollout(T)                  # the first rollout of a fresh handle: before anything is timed
        torch.cuda.synchronize()
        h = hashlib.sha256()
        for t in (traj.actions, traj.logp, traj.value):
            h.update(t.detach().cpu().contiguous().numpy().tobytes())
        digest[kind] = h.hexdigest()
        handles[kind] = (env, eng, traj)
    print("GRU_DIGEST " + json.dumps(digest), flush=True)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    if a.trace_only:
        _, eng, traj = handles["gru"]
        for _ in range(2):
            eng.rollout(T, out=traj)
        torch.cuda.synchronize()
        print(f"trace-only: {3 * T} steps of k_actor_gru done")
    else:
        say(f"go1gate {a.envs} envs x 2 agents, T = {T}, hidden {a.hidden} x {a.hidden} tanh, {torch.cuda.get_device_name(0)}, "
            f"library {os.environ.get('MQE_HIP_LIB', 'in-tree')}" + (" -- the plain handle only" if a.plain_only else ""))
        paths = {}
        for kind, (env, eng, traj) in handles.items():
            paths[f"rollout per step, {kind}"] = (lambda eng=eng, traj=traj: eng.rollout(T, out=traj))
            if kind == "gru":
                rec = eng.rollout(T, record_hidden=True)
                paths["rollout per step, gru, recorded"] = (lambda eng=eng, rec=rec: eng.rollout(T, out=rec, record_hidden=True))
        us = {n: [] for n in paths}
        for _ in range(2):
            for fn in paths.values():
                fn()
        for _ in range(a.rounds):
            for n, fn in paths.items():
                us[n].append(timed(fn) * 1e3 / T)
        med = {}
        for n, v in us.items():
            med[n] = statistics.median(v)
            say(f"{n:34s} median {med[n]:10.3f} us  min {min(v):10.3f}  max {max(v):10.3f}  (spread {spread(v):.1f} %) over {len(v)} blocks")
        if len(kinds) == 2:
            p = med["rollout per step, plain"]
            say(f"the GRU cells add {med['rollout per step, gru'] - p:.2f} us to a rollout step of {p:.2f} us (k_actor_gru against k_actor); recording the state "
                f"adds {med['rollout per step, gru, recorded'] - med['rollout per step, gru']:.2f} us more ({a.envs * 2 * 2 * a.hidden * 4 / 1e6:.1f} MB of tails per step)")
        print("GRU_AB " + json.dumps(med), flush=True)
    for env, _, _ in handles.values():
        env.close()


def against_parent(a, say):
    """child processes only: the in-tree library and the parent's, alternated"""
    me = os.path.abspath(__file__)
    jobs = {"tool": [sys.executable, me, "--plain-only", "--envs", str(a.envs), "--T", str(a.T), "--rounds", str(a.rounds)],
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
                    digests.setdefault(lib, set()).add(next(l for l in out.stdout.splitlines() if l.startswith("GRU_DIGEST ")))
                    line = next(l for l in out.stdout.splitlines() if l.startswith("GRU_AB "))
                    for n, v in json.loads(line[len("GRU_AB "):]).items():
                        got.setdefault((n, lib), []).append(v)
                else:
                    res = json.loads(next(l for l in reversed(out.stdout.splitlines()) if l.startswith("{")))
                    got.setdefault(("bench.py ms_per_step", lib), []).append(res["ms_per_step"])
    say(f"plain path, in-tree library against {a.parent}: {a.parent_rounds} alternated child processes each")
    for lib, lines in digests.items():
        say(f"{lib:8s} {' | '.join(sorted(lines))}")
    same = len(digests["in-tree"]) == 1 and digests["in-tree"] == digests["parent"]
    say("digests of the in-tree and the parent library: " + ("EQUAL in every child" if same else "DIFFERENT"))
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
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--parent", default=None, metavar="LIB")
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
