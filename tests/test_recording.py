"""Episode recording, host side: Go1's restatement of upstream's state machine (legged_robot.py:916-957 -- start_recording, pause_recording,
get_complete_frames, store_recording, _render_headless) with its accidents, on the oracle-backed Go1 with a stub camera attached to the
engine object: the stub's frame n is a tensor filled with n, so the frames tell which render call made them.  The camera itself is
tests/test_view_gpu.py's subject."""
import types

import numpy as np
import pytest
import torch

from mqe.envs.go1.go1 import Go1
from mqe.envs.utils import ENV_DICT, make_mqe_env, custom_cfg
from mqe.utils.helpers import finish_args

L = 5          # max_episode_length of the test's go1plane


def _oracle_factory(desc, keep, device):
    from oracle_engine import OracleEngine
    return OracleEngine(desc, keep)


@pytest.fixture
def plane(monkeypatch):
    """make(record_video) -> the Go1 of a 2-env go1plane whose episodes last L steps, on the oracle engine; the shared config is restored"""
    monkeypatch.setattr(Go1, "engine_factory", staticmethod(_oracle_factory))
    monkeypatch.setattr(Go1, "shard", None)
    cfg = ENV_DICT["go1plane"]["config"]
    saved = (cfg.env.num_envs, cfg.env.episode_length_s, cfg.env.record_video)
    made = []

    def make(record_video):
        a = finish_args(types.SimpleNamespace(task="go1plane", num_envs=2, seed=0, headless=True, record_video=record_video,
                                              sim_device="cpu", pipeline="cpu", subscenes=0, num_threads=0))
        base = custom_cfg(a)

        def short(c):
            c = base(c)
            c.env.episode_length_s = (L - 0.5) * 0.02          # ceil(4.5) = L steps of 0.02 s
            return c
        env, _ = make_mqe_env("go1plane", a, short)
        made.append(env)
        return env.env
    yield make
    for env in made:
        env.close()
    cfg.env.num_envs, cfg.env.episode_length_s, cfg.env.record_video = saved


class StubCamera:
    """render_view of the engine: call n returns a (4, 6, 4) uint8 tensor filled with n"""

    def __init__(self):
        self.calls = []

    def __call__(self, env, height, width, hfov_deg, eye, lookat, **kw):
        self.calls.append((env, height, width, hfov_deg, list(eye), list(lookat)))
        return torch.full((4, 6, 4), len(self.calls), dtype=torch.uint8)


def _stamps(frames, kind=np.ndarray):
    """the render call that made each frame; get_complete_frames() returns numpy arrays, video_frames holds the stub's tensors"""
    assert all(isinstance(f, kind) and tuple(f.shape) == (4, 6, 4) and bool((f == f.flatten()[0]).all()) for f in frames)
    return [int(f.flatten()[0]) for f in frames]


def test_the_state_machine_and_its_accidents(plane):
    env = plane(True)
    assert env.max_episode_length == L
    cam = env.engine.render_view = StubCamera()
    zero = torch.zeros(env.num_envs * env.num_agents, 3)
    assert env.record_now is False and env.get_complete_frames() == []
    env.step(zero)
    assert cam.calls == []                                       # not recording: nothing rendered
    env.start_recording()
    assert env.get_complete_frames() == [] and env.complete_video_frames is None
    env.reset()
    assert env.get_complete_frames() == [] and env.complete_video_frames == [] and cam.calls == []      # reset() renders nothing
    for t in range(1, L + 1):                                    # steps 1 .. L record frames 1 .. L
        _, _, reset, _ = env.step(zero)
        assert not bool(reset[0])
        assert _stamps(env.video_frames, torch.Tensor) == list(range(1, t + 1)) and env.get_complete_frames() == []
    _, _, reset, _ = env.step(zero)                              # step L + 1 resets env 0
    assert bool(reset[0]) and bool(env.time_out_buf[0])          # by time-out alone
    # (collide_buf says nothing here: with contact termination on it is the same flag as reset_buf, legged_robot.py:165)
    assert not (bool(env.r_term_buff[0]) or bool(env.p_term_buff[0]) or bool(env.z_high_term_buff[0]))
    assert _stamps(env.get_complete_frames()) == list(range(1, L + 1))
    assert len(cam.calls) == L and env.video_frames == []        # L calls, not L + 1
    # the camera the frames were asked for: env 0, the recording size, the viewer's pose, CameraProperties' default 90 degrees
    c = env.cfg
    assert cam.calls[0] == (0, c.env.recording_height_px, c.env.recording_width_px, 90.0, list(c.viewer.pos), list(c.viewer.lookat))
    for t in range(L):                                           # a complete episode waits: further steps record nothing
        _, _, reset, _ = env.step(zero)
        assert not bool(reset[0])
    assert len(cam.calls) == L and _stamps(env.get_complete_frames()) == list(range(1, L + 1))
    _, _, reset, _ = env.step(zero)                              # the next reset of env 0 overwrites it with [] and recording resumes
    assert bool(reset[0])
    assert env.get_complete_frames() == [] and len(cam.calls) == L + 1 and _stamps(env.video_frames, torch.Tensor) == [L + 1]
    env.step(zero)
    assert _stamps(env.video_frames, torch.Tensor) == [L + 1, L + 2]
    env.pause_recording()
    assert env.record_now is False and env.video_frames == [] and env.get_complete_frames() == []
    env.step(zero)
    assert len(cam.calls) == L + 2


def test_render_rgb_array(plane):
    env = plane(False)
    assert env.render() is None
    env.engine.render_view = StubCamera()
    f = env.render(mode="rgb_array")
    assert isinstance(f, np.ndarray) and f.shape == (4, 6, 4) and f.dtype == np.uint8
    assert env.render() is None and env.render(mode="human") is None


def test_refused_without_record_video(plane):
    env = plane(False)
    env.engine.render_view = StubCamera()
    with pytest.raises(RuntimeError, match="record_video"):
        env.start_recording()
    assert env.record_now is False


def test_refused_without_a_camera_in_the_engine(plane):
    env = plane(True)
    assert not hasattr(env.engine, "render_view")
    with pytest.raises(NotImplementedError, match="mqe_render_view"):
        env.start_recording()
    with pytest.raises(NotImplementedError, match="mqe_render_view"):
        env.render(mode="rgb_array")
    assert env.record_now is False


def test_refused_on_a_shard_that_does_not_hold_env_0(plane, monkeypatch):
    monkeypatch.setattr(Go1, "shard", (4, 2))                    # this process owns global envs 2, 3
    env = plane(True)
    env.engine.render_view = StubCamera()
    with pytest.raises(NotImplementedError, match="env_id_offset"):
        env.start_recording()


def test_view_constants_mirror_the_header():
    """mqe.engine.abi's VIEW_* (what the GPU tests evaluate the colour formula with) are include/mqe_hip.h's MQE_VIEW_*"""
    import os
    import re
    from mqe.engine import abi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "mqe_hip.h")).read().replace("\\\n", " ")
    macro = {m.group(1): m.group(2) for m in re.finditer(r"^#define MQE_VIEW_(\w+)\s+(.+?)\s*(?:/\*.*)?$", text, re.M)}
    nums = lambda s: [float(x) for x in re.findall(r"-?\d+\.?\d*", s.replace("f", ""))]
    for name in ("NONE", "GROUND", "WALL", "ROBOT", "NPC", "LINK_SCENE", "SCENERY"):
        assert int(macro[name]) == getattr(abi, "VIEW_" + name)
    assert eval(macro["MAX_PIXELS"]) == abi.VIEW_MAX_PIXELS and eval(macro["CHECKER_BIT"]) == abi.VIEW_CHECKER_BIT
    assert nums(macro["AMBIENT"]) == [abi.VIEW_AMBIENT] and nums(macro["DIFFUSE"]) == [abi.VIEW_DIFFUSE] and nums(macro["CHECKER"]) == [abi.VIEW_CHECKER]
    assert nums(macro["LIGHT"]) == list(abi.VIEW_LIGHT) and nums(macro["SKY"]) == list(abi.VIEW_SKY)
    assert nums(macro["PALETTE"]) == [c for row in abi.VIEW_PALETTE for c in row] and int(macro["PALETTE_ROWS"]) == len(abi.VIEW_PALETTE)
    assert [abi.view_palette_row(c, 1) for c in range(1, 7)] == [0, 1, 3, 6, 7, 8]
