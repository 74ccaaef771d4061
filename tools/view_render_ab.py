"""Cost of episode recording (Go1.start_recording -> mqe_render_view, csrc/kernels_view.hpp): one handle stepped through the task wrapper,
blocks of STEPS fused steps with recording paused ("off") and live ("on"), alternated on the same handle, REPEATS times.  Every block
starts from reset() -- with recording started that opens an episode, so the block's steps each render a frame until env 0 is reset; the
JSON line reports how many did -- ends in a device synchronise and is timed with the host clock.  A live step includes the one-byte
read-back of reset_buf[0].  MQE_HIP_LIB=<a library built from the parent commit> with --off_only gives the parent's step time on the
same box.  The kernel's own time comes from a kernel trace of the --trace, --render or --depth forms, each in a run of its own.

    python tools/view_render_ab.py [--task go1gate] [--num_envs 4096] [--steps 200] [--repeats 3] [--off_only]
    python tools/view_render_ab.py --trace on|off --steps 20          (a short run for rocprofv3 --kernel-trace: one mode, no timing)
    python tools/view_render_ab.py --render 50 [--task T] [--relief] [--far 60]     (50 recording-size frames of env 0, no steps: k_view)
    python tools/view_render_ab.py --depth 50 --num_envs 1            (50 x mqe_render_depth at 204 x 320: the one-workgroup-per-env caster)
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
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--off_only", action="store_true", help="never record (a library without the camera: the parent commit's)")
    ap.add_argument("--trace", choices=("on", "off"), default=None)
    ap.add_argument("--render", type=int, default=0, help="render this many frames of env 0 from the current state and stop")
    ap.add_argument("--depth", type=int, default=0, help="call mqe_render_depth (204 x 320, every robot) this many times and stop")
    ap.add_argument("--relief", action="store_true", help="the task's track with the whole-map Perlin relief (zScale 0.08)")
    ap.add_argument("--far", type=float, default=60.0)
    a = ap.parse_args()
    import torch
    from bench import make_args
    from mqe.envs.utils import make_mqe_env, custom_cfg
    dev = "cuda:0"
    margs = make_args(a.task, a.num_envs, 0, dev)
    base = custom_cfg(margs)

    def cfg_fn(c):
        c = base(c)
        c.env.record_video = not a.off_only
        if a.relief:
            kw = dict(c.terrain.BarrierTrack_kwargs)
            kw.update(add_perlin_noise=True, border_perlin_noise=True)
            c.terrain.BarrierTrack_kwargs = kw
            c.terrain.TerrainPerlin_kwargs = dict(zScale=0.08, frequency=10)
        return c
    env, cfg = make_mqe_env(a.task, margs, cfg_fn)
    env.reset()
    go1 = env.env
    Aw = env.num_agents
    g = torch.Generator(device=dev).manual_seed(1234)
    acts = [torch.rand(a.num_envs, Aw, 3, device=dev, generator=g) * 2 - 1 for _ in range(64)]

    def run(n, t0=0):
        for t in range(n):
            env.step(acts[(t0 + t) % len(acts)])
        torch.cuda.synchronize()

    def mode_on(on):
        if a.off_only:
            return
        if on:
            go1.start_recording()
        else:
            go1.pause_recording()

    if a.render or a.depth:
        run(6)
        H, W = int(cfg.env.recording_height_px), int(cfg.env.recording_width_px)
        pixels = 0
        for i in range(a.render):
            go1.engine.render_view(0, H, W, 90.0, cfg.viewer.pos, cfg.viewer.lookat, far=a.far)
            pixels = H * W
        for i in range(a.depth):
            go1.engine.render_depth(204, 320, 87.0, [0.26, 0.0, 0.03], [0.0, 0.0, 0.0], 20.0)
            pixels = 204 * 320 * a.num_envs * go1.num_agents
        torch.cuda.synchronize()
        print(json.dumps({"kernel": "k_view" if a.render else "k_depth_camera", "task": a.task, "relief": a.relief, "num_envs": a.num_envs,
                          "launches": a.render or a.depth, "rays_per_launch": pixels, "far": a.far if a.render else 20.0}))
        return
    if a.trace is not None:
        mode_on(a.trace == "on")
        env.reset()
        run(a.steps)
        print(json.dumps({"trace": a.trace, "task": a.task, "num_envs": a.num_envs, "steps": a.steps, "frames": len(getattr(go1, "video_frames", []))}))
        return
    modes = ("off",) if a.off_only else ("off", "on")
    for mode in modes:
        mode_on(mode == "on")
        env.reset()
        run(a.warmup)
    blocks, frames = {m: [] for m in modes}, []
    for r in range(a.repeats):
        for mode in modes:
            mode_on(mode == "on")
            env.reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(a.steps, r * a.steps)
            blocks[mode].append(1e3 * (time.perf_counter() - t0) / a.steps)
            if mode == "on":
                frames.append(len(go1.video_frames) + len(go1.complete_video_frames or []))
    mode_on(False)
    med = {k: statistics.median(v) for k, v in blocks.items()}
    out = {"task": a.task, "num_envs": a.num_envs, "steps_per_block": a.steps, "repeats": a.repeats,
           "library": os.environ.get("MQE_HIP_LIB", "in-tree"), "device": torch.cuda.get_device_name(0),
           "ms_per_step": {k: [round(x, 4) for x in v] for k, v in blocks.items()}, "median_ms_per_step": {k: round(v, 4) for k, v in med.items()}}
    if "on" in med:
        out["frames_per_on_block"] = frames
        out["on_minus_off_ms"] = round(med["on"] - med["off"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
