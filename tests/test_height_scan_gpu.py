"""-m gpu: the terrain height scan (mqe_measure_heights, mqe_set_height_refresh; Go1.measured_heights) against the float64 restatement of
its specification (tests/height_ref.py), at the shapes where the kernel's mapping can go wrong, at the point of the step where it runs,
with everything else bit-identical, with and without the scenery flag, and through make_mqe_env.

The comparison rule of every test that holds the kernel to float64: a height is discontinuous where the wall SDF's sample changes sign
(the wall's top against the ground) and, on walls with a wall_top map, where the nearer raster point changes (tx or ty = 0.5), so points
whose float64 |s| < 1e-3 m or (inside such a wall) whose tx or ty lies within 1e-3 of 0.5 are left out -- at most 1 % of the points --
and every other point agrees to 1e-5 m."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import height_ref
from helpers import make_desc, hip_engine, perlin_terrain, wall_heights_terrain
from mqe.engine import abi

pytestmark = pytest.mark.gpu

TOL, BAND, MAX_EXCLUDED = 1e-5, 1e-3, 0.01


def _grid(cfg):
    x, y = np.asarray(cfg.terrain.measured_points_x, np.float32), np.asarray(cfg.terrain.measured_points_y, np.float32)
    gx, gy = np.meshgrid(x, y, indexing="ij")
    return np.stack([gx.ravel(), gy.ravel()], 1).astype(np.float32)


def _root_np(e):
    torch.cuda.synchronize()
    return e.tensor(abi.T_ROOT_STATE).cpu().numpy()


def _check(got, root3, A, grid, terrain, d, scenery=False, what=""):
    """the kernel's (R, P) heights against float64 from the same f32 root rows and f32 grid, by the module's comparison rule"""
    want, s, tx, ty = height_ref.measured_heights(root3, A, grid, terrain, float(d.horizontal_scale), d, scenery, detail=True)
    got = got.detach().cpu().numpy().astype(np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    out = np.abs(s) < BAND
    if getattr(terrain, "wall_top", None) is not None:
        out |= (s <= 0) & ((np.abs(tx - 0.5) < BAND) | (np.abs(ty - 0.5) < BAND))
    err = np.where(out, 0.0, np.abs(got - want))
    print(f"{what}: {got.size} points, excluded {out.mean() * 100:.3f} %, max error outside the band {err.max():.3e}, walls under {np.mean(s <= 0) * 100:.1f} %")
    assert np.isfinite(got).all(), what
    assert out.mean() <= MAX_EXCLUDED, (what, out.mean())
    assert err.max() <= TOL, (what, err.max(), np.unravel_index(err.argmax(), err.shape))
    return want


def _scatter_roots(e, info, N, A, gen, spread=1.5):
    """root xy = agent origin + U(-spread, spread)^2, random unit quaternions (tilted bodies), written into the live state"""
    root = e.tensor(abi.T_ROOT_STATE)
    ao = torch.as_tensor(np.asarray(info["agent_origins"], np.float32)).reshape(N, A, -1)
    xy = ao[..., :2] + (torch.rand(N, A, 2, generator=gen) * 2 - 1) * spread
    q = torch.randn(N, A, 4, generator=gen)
    q = q / q.norm(dim=-1, keepdim=True)
    torch.cuda.synchronize()
    root[:, :A, 0:2] = xy.cuda()
    root[:, :A, 3:7] = q.cuda()
    torch.cuda.synchronize()


@pytest.mark.parametrize("terrain", ["own", "perlin", "wall_heights"])
def test_against_float64(terrain):
    """go1gate, 64 envs x 2 robots scattered +-1.5 m about their spawn points with random (tilted) orientations, the shipped 187-point grid.
    Measured on an MI355X: excluded 0.24 / 0.25 / 0.28 % of the points (own / Perlin / per-block wall heights), max error outside the
    band 4.5e-10 / 6.1e-7 / 4.5e-10 m; the f32 restatement of the formula on a CPU differs from float64 by 5.2e-7 m on the same inputs."""
    N = 64
    tcfg = {"own": None, "perlin": perlin_terrain("go1gate"), "wall_heights": wall_heights_terrain("go1gate")}[terrain]
    d, k, info = make_desc("go1gate", N, terrain_cfg=tcfg)
    A = d.num_agents
    assert A == 2
    t = info["terrain"]
    assert (getattr(t, "ground_height", None) is not None) == (terrain == "perlin")
    assert (getattr(t, "wall_top", None) is not None) == (terrain == "wall_heights")
    e = hip_engine(d, k)
    e.reset_all()
    _scatter_roots(e, info, N, A, torch.Generator().manual_seed(3))
    grid = _grid(info["cfg"])
    assert grid.shape == (187, 2)
    got = e.measure_heights(grid)
    want = _check(got, _root_np(e), A, grid, t, d, what=f"go1gate on {terrain} terrain")
    assert want.max() - want.min() > 0.05                                  # walls or relief are under the grids
    e.close()


@pytest.fixture(scope="module")
def small():
    """go1gate, N = 3: R = 6 robots, fewer than a workgroup owns at any P -- the last (only) workgroup is part-filled"""
    d, k, info = make_desc("go1gate", 3)
    e = hip_engine(d, k)
    e.reset_all()
    _scatter_roots(e, info, 3, d.num_agents, torch.Generator().manual_seed(21))
    yield d, e, info
    e.close()


@pytest.mark.parametrize("P", [1, 67, 187, 1024])
def test_shapes_and_an_output_that_is_only_4_byte_aligned(small, P):
    d, e, info = small
    A, R = d.num_agents, 3 * d.num_agents
    rng = np.random.default_rng(P)
    grid = _grid(info["cfg"]) if P == 187 else rng.uniform(-1.2, 1.2, (P, 2)).astype(np.float32)
    guard = 4
    buf = torch.full((R * P + 2 * guard + 1,), -777.0, device="cuda")
    out = buf[guard + 1:guard + 1 + R * P].view(R, P)                      # starts one float into a 16 B word
    assert buf.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 4
    got = e.measure_heights(grid, out=out)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    assert (buf[:guard + 1] == -777.0).all() and (buf[guard + 1 + R * P:] == -777.0).all(), "guard floats were written"
    assert (out != -777.0).all()
    _check(out, _root_np(e), A, grid, info["terrain"], d, what=f"R = {R}, P = {P}")
    assert torch.equal(e.measure_heights(grid), out)                         # an aligned output holds the same bits


def test_roots_far_outside_the_map_read_the_clamped_edge():
    d, k, info = make_desc("go1gate", 3, terrain_cfg=perlin_terrain("go1gate"))
    e = hip_engine(d, k)
    e.reset_all()
    A = d.num_agents
    t = info["terrain"]
    nx, ny = t.wall_sdf.shape
    hs = float(d.horizontal_scale)
    root = e.tensor(abi.T_ROOT_STATE)
    mid = (0.5 * nx * hs, 0.5 * ny * hs)
    xy = torch.tensor([[-1000.0, mid[1]], [1000.0 + nx * hs, mid[1]], [mid[0], -1000.0], [mid[0], 1000.0 + ny * hs], [-1000.0, -1000.0], [1000.0 + nx * hs, 1000.0 + ny * hs]])
    torch.cuda.synchronize()
    root[:, :A, 0:2] = xy.view(3, A, 2).cuda()
    grid = _grid(info["cfg"])
    got = e.measure_heights(grid)
    want = _check(got, _root_np(e), A, grid, t, d, what="roots 1 km outside the map")
    # the corners: every point of the grid clamps to the one corner entry
    gh = t.ground_height.astype(np.float64) + t.ground_z
    g = got.cpu().numpy()
    assert np.abs(g[4] - max(gh[0, 0], t.wall_height if t.wall_sdf[0, 0] <= 0 else -1e9)).max() <= TOL
    assert np.abs(g[5] - max(gh[-1, -1], t.wall_height if t.wall_sdf[-1, -1] <= 0 else -1e9)).max() <= TOL
    assert np.ptp(want[4]) == 0 and np.ptp(want[5]) == 0
    e.close()


def test_refusals_launch_nothing(small):
    d, e, info = small
    R = 3 * d.num_agents
    f, g = e.lib.mqe_measure_heights, e.lib.mqe_set_height_refresh
    pts = np.zeros((1025, 2), np.float32)
    out = torch.full((R * 1025,), -777.0, device="cuda")
    o, p = C.c_void_p(out.data_ptr()), C.c_void_p(pts.ctypes.data)
    for args, word in (((o, p, 1025, 0), "n_points"), ((o, p, 0, 0), "n_points"), ((o, p, 187, 2), "flag"), ((o, p, 187, -2), "flag"),
                       ((None, p, 187, 0), "out_dev"), ((o, None, 187, 0), "points_xy")):
        rc = f(e.h, *args, None)
        assert rc < 0 and word in e.lib.mqe_last_error().decode(), (args[2:], rc, e.lib.mqe_last_error())
        if args[0] is not None:
            rc = g(e.h, *args)
            assert rc < 0 and word in e.lib.mqe_last_error().decode(), (args[2:], rc, e.lib.mqe_last_error())
    assert f(None, o, p, 187, 0, None) < 0 and g(None, o, p, 187, 0) < 0
    torch.cuda.synchronize()
    assert (out == -777.0).all(), "a refused call wrote heights"
    with pytest.raises(RuntimeError, match="n_points"):
        e.measure_heights(pts)
    # nothing was registered by the refused calls: a step (from the spawn poses) leaves the buffer alone
    e.reset_all()
    e.step_command(torch.zeros(R, 3, device="cuda"))
    torch.cuda.synchronize()
    assert (out == -777.0).all()
    _scatter_roots(e, info, 3, d.num_agents, torch.Generator().manual_seed(21))      # the module's engine as the other tests expect it


def test_envs_reset_in_the_step_show_the_heights_under_their_terminal_pose():
    """test_rigid_body_state_gpu's terminal-pose test for the scan: episodes of 5 steps with random start lengths, a fused handle with the
    scan registered against a twin loaded with the same state and stepped in stages.  Envs that did not reset hold, bit for bit, what a
    one-shot measurement of the post-step state gives; envs that did hold what the twin's one-shot gives between POST_NPC and POST_RESET.
    The twin's physics runs the unfused kernels, whose root rows agree with the fused ones to 1e-6 (that test), not bit for bit: the reset
    envs are compared by the module's rule (1e-5 m outside the float64 discontinuity band of the twin's state)."""
    N = 96
    d1, k1, info = make_desc("go1gate", N, max_episode_length=5)
    d2, k2, _ = make_desc("go1gate", N, max_episode_length=5)
    ea, eb = hip_engine(d1, k1), hip_engine(d2, k2)
    grid = _grid(info["cfg"])
    live = ea.set_height_refresh(grid)
    assert live.shape == (N * d1.num_agents, 187) and ea.set_height_refresh(grid) is live
    ea.reset_all()
    A = d1.num_agents
    g = torch.Generator().manual_seed(5)
    ea.tensor(abi.T_EPISODE_LENGTH).copy_(torch.randint(0, 5, (N,), generator=g, dtype=torch.int32).cuda())
    n_reset = n_kept = 0
    for t in range(8):
        cmd = ((torch.rand(N * A, 3, generator=g) * 2 - 1) * torch.tensor([1.5, 0.5, 1.0])).cuda().contiguous()
        eb.load_state(ea.save_state())
        ea.step_command(cmd)
        eb.policy_step(cmd)
        for k in range(d2.decimation):
            eb.compute_torques(); eb.simulate(); eb.post_decimation_step(k)
        eb.post_physics_stage(abi.POST_FRAME)
        eb.post_physics_stage(abi.POST_NPC)
        terminal = eb.measure_heights(grid).view(N, A, -1)
        terminal_root = _root_np(eb)
        eb.post_physics_stage(abi.POST_RESET)
        eb.post_physics_stage(abi.POST_OBS)
        eb.post_physics_stage(abi.POST_WRAPPER)
        torch.cuda.synchronize()
        reset = ea.tensor(abi.T_RESET_BUF).bool()
        assert torch.equal(reset, eb.tensor(abi.T_RESET_BUF).bool()), t
        now = ea.measure_heights(grid).view(N, A, -1)
        torch.cuda.synchronize()
        lv = live.view(N, A, -1)
        assert torch.equal(lv[~reset], now[~reset]), t
        _, s, _, _ = height_ref.measured_heights(terminal_root, A, grid, info["terrain"], float(d1.horizontal_scale), detail=True)
        clear = torch.as_tensor(np.abs(s) >= BAND).view(N, A, -1).cuda()[reset]
        diff = (lv[reset] - terminal[reset]).abs()
        assert clear.float().mean() >= 1 - MAX_EXCLUDED if reset.any() else True
        assert (diff[clear] <= TOL).all(), (t, diff[clear].max().item())
        if reset.any():                                   # the reset moved them: the scan does not show the new pose
            assert not torch.equal(lv[reset], now[reset]), t
        n_reset += int(reset.sum()); n_kept += int((~reset).sum())
    assert n_reset > N and n_kept > N, (n_reset, n_kept)
    # dropped: the next step leaves the tensor alone
    ea.set_height_refresh(None)
    before = live.clone()
    ea.step_command(cmd)
    torch.cuda.synchronize()
    assert torch.equal(live, before)
    ea.close(); eb.close()


_FLAGS = (abi.T_RESET_BUF, abi.T_TIME_OUT_BUF, abi.T_COLLIDE_BUF, abi.T_R_TERM, abi.T_P_TERM, abi.T_Z_HIGH_TERM, abi.T_EPISODE_LENGTH,
          abi.T_RESET_COUNT, abi.T_CONTACT_OVERFLOW)
_VALUES = (abi.T_WRAPPER_OBS, abi.T_WRAPPER_REWARD, abi.T_ROOT_STATE, abi.T_DOF_STATE, abi.T_OBS_BAG)


@pytest.mark.parametrize("task", ["go1gate", "go1football-defender"])
def test_registered_scan_changes_nothing_else(task):
    """two handles of one scene and seed, the scan registered in one, 40 fused wrapper-level steps: flags, counters, the returned
    observation / reward and the root, joint and observation state are bit-identical at every step (go1gate gives up the physics kernel's
    epilogue for the separate post-physics launch, the defender scene runs the separate launch either way).  The football field's walls
    are 2 m and more from where its robots play, so that scene's scan takes the shipped grid stretched four times: it reaches them"""
    N = 128
    d1, k1, info = make_desc(task, N)
    d2, k2, _ = make_desc(task, N)
    on, off = hip_engine(d1, k1), hip_engine(d2, k2)
    live = on.set_height_refresh(_grid(info["cfg"]) * np.float32(4.0 if task == "go1football-defender" else 1.0))
    on.reset_all(); off.reset_all()
    Aw = on.tensor(abi.T_WRAPPER_OBS).shape[1]
    g = torch.Generator().manual_seed(13)
    for t in range(40):
        a = (torch.rand(N, Aw, 3, generator=g) * 2 - 1).cuda()
        on.step(a); off.step(a)
        torch.cuda.synchronize()
        for kind in _FLAGS + _VALUES:
            assert torch.equal(on.tensor(kind), off.tensor(kind)), (task, t, kind)
    assert torch.isfinite(live).all() and live.max() - live.min() > 0.05
    on.close(); off.close()


def test_scenery_flag():
    """go1bridge: a grid laid over the deck reads the deck's top with the flag and the terrain below without it; on go1gate (no scenery)
    the flag changes nothing"""
    N = 4
    d, k, info = make_desc("go1bridge", N)
    assert d.npc_kind == abi.NPC["bridge"] and d.n_static_boxes >= 1
    A = d.num_agents
    e = hip_engine(d, k)
    e.reset_all()
    root = e.tensor(abi.T_ROOT_STATE)
    # the longest box is the deck; the robots are put at its centre, heading along +x and +y
    b = max(range(d.n_static_boxes), key=lambda i: d.static_box_half[i][0])
    c, h = [d.static_box_center[b][i] for i in range(3)], [d.static_box_half[b][i] for i in range(3)]
    torch.cuda.synchronize()
    root[:, :A, 0] = root[:, A:A + 1, 0] + c[0]
    root[:, :A, 1] = root[:, A:A + 1, 1] + c[1]
    quat = torch.tensor([[0.0, 0.0, 0.0, 1.0], [0.0, 0.0, np.sin(np.pi / 4), np.cos(np.pi / 4)]])[torch.arange(A) % 2]
    root[:, :A, 3:7] = quat.cuda()
    r = 0.6 * min(h[0], h[1])
    u = np.linspace(-r, r, 7, dtype=np.float32)
    grid = np.stack(np.meshgrid(u, u, indexing="ij"), -1).reshape(-1, 2)
    with_flag, without = e.measure_heights(grid, scenery=True), e.measure_heights(grid)
    r3 = _root_np(e)
    want = _check(with_flag, r3, A, grid, info["terrain"], d, scenery=True, what="go1bridge, scenery seen")
    deck_top = r3[:, A, 2].astype(np.float64).repeat(A)[:, None] + c[2] + h[2]
    assert np.abs(want - deck_top).max() <= 1e-9                            # the reference's answer IS the deck's top, everywhere on the grid
    below = _check(without, r3, A, grid, info["terrain"], d, what="go1bridge, terrain only")
    assert (deck_top - below).min() > 0.01
    e.close()
    d, k, info = make_desc("go1gate", N)
    e = hip_engine(d, k)
    e.reset_all()
    _scatter_roots(e, info, N, d.num_agents, torch.Generator().manual_seed(9))
    grid = _grid(info["cfg"])
    assert torch.equal(e.measure_heights(grid, scenery=True), e.measure_heights(grid))
    e.close()


def test_measured_heights_through_make_mqe_env(monkeypatch):
    from mqe.envs.go1.go1 import Go1
    from mqe.envs.utils import ENV_DICT, make_mqe_env, custom_cfg
    from mqe.utils.helpers import finish_args
    monkeypatch.setattr(Go1, "shard", None)
    saved = ENV_DICT["go1gate"]["config"].env.num_envs
    a = finish_args(types.SimpleNamespace(task="go1gate", num_envs=8, seed=0, headless=True, record_video=False, sim_device="cuda:0",
                                          pipeline="gpu", subscenes=0, num_threads=0))
    try:
        env, cfg = make_mqe_env("go1gate", a, custom_cfg(a))
        go1 = env.env
        env.reset()
        mh = go1.measured_heights
        assert mh.shape == (16, 187) and mh.is_cuda and go1.measured_heights is mh
        assert go1.num_height_points == 187 and go1.height_points.shape == (16, 187, 3) and go1.height_points.is_cuda
        torch.cuda.synchronize()
        first, root0 = mh.clone(), go1.root_states.clone()
        for t in range(25):
            env.step(torch.tensor([1.0, 0.3, 0.5], device="cuda").expand(8, env.num_agents, 3).contiguous())
        torch.cuda.synchronize()
        assert go1.measured_heights is mh
        assert (go1.root_states[:, :2] - root0[:, :2]).norm(dim=1).max() > 0.05, "the robots did not move"
        assert not torch.equal(mh, first)
        # what _reward_base_height computes, root z - measured_heights, is the base's height above the surface under the grid.  Every
        # spawn row of go1gate has walls under a part of its grid, so (1) over the points the float64 reference puts on the slab, robot by
        # robot (envs reset in the last step hold the heights under their terminal pose: left out), and (2) over the whole grid for robots
        # moved to a place where the reference finds no wall under it, the mean is the base height of the root row
        t_, A = go1.terrain, go1.num_agents
        hs, grid = float(go1.engine.desc.horizontal_scale), _grid(cfg)
        want = height_ref.measured_heights(go1._root3.cpu().numpy(), A, grid, t_, hs)
        on_slab = torch.as_tensor(want == t_.ground_z).cuda()
        alive = ~go1.reset_buf.repeat_interleave(A)
        rows = go1.root_states
        dz = rows[:, 2].unsqueeze(1) - mh
        assert alive.any() and (on_slab.sum(1) > 20).all()
        mean_on_slab = (dz * on_slab).sum(1) / on_slab.sum(1)
        print("base height over the slab points:", mean_on_slab[alive].tolist())
        assert ((mean_on_slab - (rows[:, 2] - t_.ground_z)).abs()[alive] <= 0.02).all()
        nx, ny = t_.wall_sdf.shape
        cx, cy = np.meshgrid(np.arange(0.5, nx * hs, 0.25), np.arange(0.5, ny * hs, 0.25), indexing="ij")
        spots = np.zeros((cx.size, 13))
        spots[:, 0], spots[:, 1], spots[:, 6] = cx.ravel(), cy.ravel(), 1.0
        clear = (height_ref.surface_height(*height_ref.world_points(spots, grid), t_, hs) == t_.ground_z).all(axis=1)
        assert clear.any()
        here = rows[0, :2].cpu().numpy()
        spot = spots[clear][np.argmin(np.linalg.norm(spots[clear][:, :2] - here, axis=1)), :2]
        go1._root3[0, :A, 0:2] = torch.as_tensor(spot, dtype=torch.float32).cuda()
        go1._root3[0, :A, 3:7] = torch.tensor([0.0, 0.0, 0.0, 1.0]).cuda()
        moved = go1._get_heights()[:A]
        base_height = torch.mean(go1.root_states[:A, 2].unsqueeze(1) - moved, dim=1)
        print("robots moved to", spot.tolist(), "base heights", base_height.tolist())
        assert (moved == t_.ground_z).all()
        assert ((base_height - (go1.root_states[:A, 2] - t_.ground_z)).abs() <= 0.02).all()
        fresh = go1._get_heights()
        assert fresh.shape == (16, 187) and fresh is not mh
        ids = torch.tensor([3, 0, 11], device="cuda")
        assert torch.equal(go1._get_heights(ids), fresh[ids])
        env.close()
    finally:
        ENV_DICT["go1gate"]["config"].env.num_envs = saved
