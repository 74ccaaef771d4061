"""Record one episode of env 0 of a task under random actions (Go1.start_recording, the engine's free camera mqe_render_view) and write it
as one .npy stack (frames, H, W, 4) uint8 -- and as a GIF when PIL is importable.

    python tools/record_episode.py --task go1gate [--steps 400] [--num_envs 16] [--out recordings]

The episode ends when env 0 is reset (termination or time-out) or after --steps steps, whichever comes first; in the second case the
frames recorded so far are written.  cfg.viewer.pos / lookat place the camera, cfg.env.recording_width_px x recording_height_px size it."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multiagent-quadruped-environment_amd"))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--task", required=True)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--num_envs", type=int, default=16)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default="recordings")
    a = ap.parse_args()
    import numpy as np
    import torch
    from bench import make_args
    from mqe.envs.utils import make_mqe_env, custom_cfg
    dev = "cuda:0"
    margs = make_args(a.task, a.num_envs, a.seed, dev)
    margs.record_video = True
    env, _ = make_mqe_env(a.task, margs, custom_cfg(margs))
    env.start_recording()
    env.reset()
    g = torch.Generator(device=dev).manual_seed(a.seed)
    frames = []
    for t in range(a.steps):
        _, _, done, _ = env.step(torch.rand(a.num_envs, env.num_agents, 3, device=dev, generator=g) * 2 - 1)
        if bool(done[0]):                                    # fetch now: the next reset of env 0 overwrites the complete episode
            frames = env.get_complete_frames()
            break
    else:
        frames = [f.cpu().numpy() for f in env.env.video_frames]
    env.pause_recording()
    if not frames:
        raise SystemExit("no frame was recorded")
    os.makedirs(a.out, exist_ok=True)
    stack = np.stack(frames)
    path = os.path.join(a.out, f"{a.task}_episode.npy")
    np.save(path, stack)
    print(f"{path}: {stack.shape[0]} frames of {stack.shape[1]} x {stack.shape[2]}")
    try:
        from PIL import Image
    except ImportError:
        print("PIL is not installed: no GIF")
        return
    imgs = [Image.fromarray(f[..., :3]) for f in frames]
    gif = os.path.join(a.out, f"{a.task}_episode.gif")
    imgs[0].save(gif, save_all=True, append_images=imgs[1:], duration=20, loop=0)
    print(gif)


if __name__ == "__main__":
    main()
