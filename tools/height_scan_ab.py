"""Cost of the per-step terrain height scan (mqe_set_height_refresh): one go1gate handle stepped through the task wrapper, blocks of STEPS
fused steps with the scan dropped and registered, alternated on the same handle, REPEATS times; each block ends in a device synchronise
and is timed with the host clock.  One JSON line: ms per step of every block and the medians.  The kernel's own time comes from a
kernel trace of the --trace form, in a run of its own.  MQE_HIP_LIB=<a library built from the parent commit> with --off_only gives the
parent's step time on the same box: "off" launches the parent's kernels.

    python tools/height_scan_ab.py [--task go1gate] [--num_envs 4096] [--steps 500] [--repeats 3] [--off_only]
    python tools/height_scan_ab.py --trace on|off --steps 20        (a short run for rocprofv3 --kernel-trace: one mode, no timing)
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multiagent-quadruped-environment_amd"))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--task", default="go1gate")
    ap.add_argument("--num_envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--off_only", action="store_true", help="never register the scan (a library without it: the parent commit's)")
    ap.add_argument("--trace", choices=("on", "off"), default=None)
    a = ap.parse_args()
    import torch
    from bench import make_args
    from mqe.envs.utils import make_mqe_env, custom_cfg
    dev = "cuda:0"
    margs = make_args(a.task, a.num_envs, 0, dev)
    env, _ = make_mqe_env(a.task, margs, custom_cfg(margs))
    env.reset()
    go1 = env.env
    eng, grid = go1.engine, go1._height_grid()
    Aw = env.num_agents
    g = torch.Generator(device=dev).manual_seed(1234)
    acts = [torch.rand(a.num_envs, Aw, 3, device=dev, generator=g) * 2 - 1 for _ in range(64)]

    def run(n, t0=0):
        for t in range(n):
            env.step(acts[(t0 + t) % len(acts)])
        torch.cuda.synchronize()

    if a.trace is not None:
        eng.set_height_refresh(grid if a.trace == "on" else None)
        run(a.steps)
        print(json.dumps({"trace": a.trace, "task": a.task, "num_envs": a.num_envs, "steps": a.steps}))
        return
    modes = ("off",) if a.off_only else ("off", "on")
    for mode in modes:                       # both shapes warm
        if not a.off_only:
            eng.set_height_refresh(grid if mode == "on" else None)
        run(a.warmup)
    blocks = {m: [] for m in modes}
    for r in range(a.repeats):
        for mode in modes:
            if not a.off_only:
                eng.set_height_refresh(grid if mode == "on" else None)
            run(5)
            t0 = time.perf_counter()
            run(a.steps, r * a.steps)
            blocks[mode].append(1e3 * (time.perf_counter() - t0) / a.steps)
    med = {k: statistics.median(v) for k, v in blocks.items()}
    out = {"task": a.task, "num_envs": a.num_envs, "points": int(grid.shape[0]), "steps_per_block": a.steps, "repeats": a.repeats,
           "library": os.environ.get("MQE_HIP_LIB", "in-tree"), "device": torch.cuda.get_device_name(0),
           "ms_per_step": {k: [round(x, 4) for x in v] for k, v in blocks.items()}, "median_ms_per_step": {k: round(v, 4) for k, v in med.items()}}
    if "on" in med:
        out["on_over_off"] = round(med["on"] / med["off"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
