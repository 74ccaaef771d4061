"""The free camera of episode recording on the HIP engine (mqe_render_view, csrc/kernels_view.hpp; include/mqe_hip.h is the specification):
(1) its depth plane against the CPU specification's scalar caster (oracle/: mqo_render_depth) through a borrowed mount, on the 8 scenes
of tests/test_camera_gpu.py; (2) a robot sees itself; (3) known answers for the id word and the normal on the set-ups of
tests/camera_cases.py; (4) the colour is the documented function of (id, normal); (5) image shapes: every pixel written, nothing
beyond; (6) no side effects; (7) a recorded episode through make_mqe_env; (8) every refusal of the C entry point."""
import ctypes as C
import math
import types

import numpy as np
import pytest
import torch

import camera_cases as cc
from helpers import make_desc, hip_engine, oracle_engine, perlin_terrain
from mqe.engine import abi

pytestmark = pytest.mark.gpu

H, W, FOV = 48, 64, 87.0


# ---- the specification's camera in float64 --------------------------------------------------------------------------------------------
def basis(eye, lookat):
    eye, lookat = np.asarray(eye, np.float64), np.asarray(lookat, np.float64)
    f = (lookat - eye) / np.linalg.norm(lookat - eye)
    nl = math.hypot(f[0], f[1])
    left = np.array([0.0, 1.0, 0.0]) if nl < 1e-6 else np.array([-f[1], f[0], 0.0]) / nl
    return f, left, np.cross(f, left)


def rays(h, w, fov, eye, lookat):
    """(h, w, 3) ray directions d = f + yc l + zc u, not normalised: the parameter is the depth along the optical axis"""
    f, left, up = basis(eye, lookat)
    th = math.tan(math.radians(fov) / 2)
    yc = -(2 * (np.arange(w) + 0.5) / w - 1) * th
    zc = -(2 * (np.arange(h) + 0.5) / h - 1) * th * h / w
    return f[None, None, :] + yc[None, :, None] * left[None, None, :] + zc[:, None, None] * up[None, None, :]


def f32(v):
    """what the entry point receives: eye3 / lookat3 are float arrays"""
    return np.asarray(v, np.float32).astype(np.float64)


def view(e, env, h, w, fov, eye, lookat, far=60.0):
    rgba, geom, ids = e.render_view(env, h, w, fov, eye, lookat, far, geom=True, ids=True)
    torch.cuda.synchronize()
    return rgba.cpu().numpy(), geom.cpu().numpy(), ids.cpu().numpy()


def raw_view(e, env, rgba, geom, ids, h, w, fov, eye, lookat, far):
    """mqe_render_view itself, with the caller's pointers (None = null): its return code"""
    f = e.lib.mqe_render_view
    ptr = lambda t: C.c_void_p(t if isinstance(t, int) else t.data_ptr()) if t is not None else C.c_void_p(None)
    v3 = lambda v: (C.c_float * 3)(*[float(x) for x in v]) if v is not None else None
    return f(e.h, int(env), ptr(rgba), ptr(geom), ptr(ids), int(h), int(w), float(fov), v3(eye), v3(lookat), float(far), e._stream())


def everywhere(geom, ids, d):
    """what holds at every pixel: unit normals that face the eye on hits, zero normal and id 0 on misses, a class in 0 .. 6"""
    depth, n = geom[..., 0].astype(np.float64), geom[..., 1:].astype(np.float64)
    hit = np.isfinite(depth)
    assert ((ids & 255) <= abi.VIEW_SCENERY).all() and (ids >= 0).all()
    assert (((ids & 255) != abi.VIEW_NONE) == hit).all()
    assert (depth[hit] < 0).all() and np.isneginf(depth[~hit]).all()
    assert (n[~hit] == 0).all() and (ids[~hit] == 0).all()
    assert (np.abs(np.linalg.norm(n[hit], axis=-1) - 1) <= 1e-5).all(), float(np.abs(np.linalg.norm(n[hit], axis=-1) - 1).max())
    assert ((n[hit] * d[hit]).sum(-1) <= 0).all()
    assert ((ids & abi.VIEW_CHECKER_BIT) == 0)[(ids & 255) != abi.VIEW_GROUND].all()


def expected_rgba(geom, ids):
    """the documented colour formula in float64, from the kernel's own id and normal planes"""
    n = geom[..., 1:].astype(np.float64)
    cls, idx = ids & 255, (ids >> 8) & 255
    row = np.where(cls == abi.VIEW_GROUND, 0, np.where(cls == abi.VIEW_WALL, 1, np.where(cls == abi.VIEW_ROBOT, 2 + idx % 4, cls + 2)))
    albedo = np.asarray(abi.VIEW_PALETTE, np.float64)[np.clip(row, 0, len(abi.VIEW_PALETTE) - 1)]
    k = np.where(cls == abi.VIEW_GROUND, np.where(ids & abi.VIEW_CHECKER_BIT, 1 + abi.VIEW_CHECKER, 1 - abi.VIEW_CHECKER), 1.0)
    shade = abi.VIEW_AMBIENT + abi.VIEW_DIFFUSE * np.maximum(0.0, n @ np.asarray(abi.VIEW_LIGHT, np.float64))
    rgb = np.floor(255 * np.minimum(1.0, albedo * (k * shade)[..., None]) + 0.5)
    rgb[cls == abi.VIEW_NONE] = abi.VIEW_SKY
    return rgb


def assert_colour(rgba, geom, ids):
    want = expected_rgba(geom, ids)
    assert (rgba[..., 3] == 255).all()
    assert np.abs(rgba[..., :3].astype(np.float64) - want).max() <= 1
    miss = (ids & 255) == abi.VIEW_NONE
    assert (rgba[..., :3][miss] == np.asarray(abi.VIEW_SKY, np.uint8)).all()


# ---- 1. the depth plane against the oracle's caster -----------------------------------------------------------------------------------
@pytest.mark.parametrize("task,relief", [("go1gate", False), ("go1sheep-hard", False), ("go1pushbox", False), ("go1seesaw", False), ("go1bridge", False),
                                         ("go1football-defender", False), ("go1tug", False), ("go1gate", True)])
def test_depth_plane_is_the_specifications(task, relief):
    """The free camera borrows robot a's mount: the oracle renders the onboard camera of robot a, upright with yaw psi, mounted at
    (1.0, 0, 0.1) -- farther ahead than feature_reach (0.72 m), every ray with a positive forward component, so robot a lies behind its own
    camera and the oracle's exclusion of it changes nothing -- and the free camera stands at eye = base + Rz(psi) (1.0, 0, 0.1) looking
    along Rz(psi) x.  Envs 0 and N - 1, every robot in turn, the other robots tilted as tests/test_camera_gpu.py tilts them.  Bounds: that
    test's (:59-65), summed over the scene's views."""
    N = 4
    kw = dict(terrain_cfg=perlin_terrain(task, zScale=0.08)) if relief else {}
    d1, k1, _ = make_desc(task, N, **kw)
    d2, k2, _ = make_desc(task, N, **kw)
    eh, eo = hip_engine(d1, k1), oracle_engine(d2, k2, f64=True)
    eh.reset_all(); eo.reset_all()
    g = torch.Generator().manual_seed(3)
    Aw = eh.tensor(abi.T_WRAPPER_OBS).shape[1]
    for t in range(6):
        eh.step((torch.rand(N, Aw, 3, generator=g) * 2 - 1).cuda())
    A = d1.num_agents
    ro, do = eh.tensor(abi.T_ROOT_STATE), eh.tensor(abi.T_DOF_STATE)
    yaw = torch.rand(N, A, generator=g) * 6.283
    pitch = (torch.rand(N, A, generator=g) - 0.5) * 0.6
    roll = (torch.rand(N, A, generator=g) - 0.5) * 0.4
    cy, sy, cp, sp, cr_, sr = torch.cos(yaw / 2), torch.sin(yaw / 2), torch.cos(pitch / 2), torch.sin(pitch / 2), torch.cos(roll / 2), torch.sin(roll / 2)
    tilted = torch.stack([sr * cp * cy - cr_ * sp * sy, cr_ * sp * cy + sr * cp * sy, cr_ * cp * sy - sr * sp * cy, cr_ * cp * cy + sr * sp * sy], -1).cuda()
    # the random yaw: the first draw that puts the eye in the open, more than 0.15 m from every wall footprint (1 m from a spawn point
    # most directions end inside a wall of the track, where every ray hits at once and the comparison says nothing)
    envs = (0, N - 1)
    sdf, hs = np.ctypeslib.as_array(d1.wall_sdf, shape=(d1.sdf_nx, d1.sdf_ny)), d1.horizontal_scale
    spawn = ro.cpu().numpy().astype(np.float64)
    psi = torch.zeros(2, A)
    for i, e in enumerate(envs):
        for a in range(A):
            for cand in (torch.rand(64, generator=g) * 6.283).tolist():
                x, y = spawn[e, a, 0] + math.cos(cand), spawn[e, a, 1] + math.sin(cand)
                if 0 <= x / hs < d1.sdf_nx and 0 <= y / hs < d1.sdf_ny and sdf[int(x / hs), int(y / hs)] > 0.15:
                    psi[i, a] = cand
                    break
            else:
                raise AssertionError((task, e, a, "no open spot 1 m from the robot"))
    bad = total = hits = 0
    errs, depths = [], []
    for a in range(A):
        q = tilted.clone()
        for i, e in enumerate(envs):
            q[e, a] = torch.tensor([0.0, 0.0, math.sin(psi[i, a] / 2), math.cos(psi[i, a] / 2)])
        ro[:, :A, 3:7] = q
        torch.cuda.synchronize()
        eo.tensor(abi.T_ROOT_STATE).copy_(ro.cpu()); eo.tensor(abi.T_DOF_STATE).copy_(do.cpu())
        io = eo.render_depth(H, W, FOV, [1.0, 0.0, 0.1], [0.0, 0.0, 0.0], 20.0).numpy().astype(np.float64).reshape(N, A, H, W)
        rows = ro.cpu().numpy().astype(np.float64)
        for e in envs:
            qz, qw = rows[e, a, 5], rows[e, a, 6]                      # the quaternion as stored (f32), its rotation in float64
            c, s = (qw * qw - qz * qz) / (qz * qz + qw * qw), 2 * qw * qz / (qz * qz + qw * qw)
            Rz = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
            eye = rows[e, a, :3] + Rz @ np.array([1.0, 0.0, 0.1])
            _, geom, _ = view(eh, e, H, W, FOV, eye, eye + Rz @ np.array([1.0, 0.0, 0.0]), far=20.0)
            ih, ref = geom[..., 0].astype(np.float64), io[e, a]
            mh, mo = np.isfinite(ih), np.isfinite(ref)
            both = mh & mo
            err = np.abs(ih[both] - ref[both])
            bad += int((mh != mo).sum()) + int((err > 1e-4 + 1e-5 * np.abs(ref[both])).sum())
            total += ih.size; hits += int(mo.sum())
            errs.append(err); depths.append(-ref[mo])
    errs, depths = np.concatenate(errs), np.concatenate(depths)
    print(f"{task} relief={relief}: {2 * A} views, {bad} of {total} pixels differ, median {np.median(errs):.3e}, max {errs.max():.3e}, hit {hits / total:.3f}, "
          f"median depth {np.median(depths):.2f} m")
    assert bad <= 2e-3 * total, (task, relief, bad, total)
    assert np.median(errs) < 2e-6
    assert hits > 0.3 * total
    assert np.median(depths) > 0.3                                         # ... at a distance: no eye stands inside a wall


# ---- the images of tests 2 - 4, rendered once -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shots():
    """name -> dict(rgba, geom, ids, d (ray directions), ...) of the known-answer set-ups"""
    out = {}

    def shoot(name, e, env, h, w, fov, eye, lookat, far=60.0, **extra):
        eye, lookat = f32(eye), f32(lookat)
        rgba, geom, ids = view(e, env, h, w, fov, eye, lookat, far)
        out[name] = dict(rgba=rgba, geom=geom, ids=ids, d=rays(h, w, fov, eye, lookat), eye=eye, **extra)

    # go1plane: robot 0 upright, seen from 2 m above its base (a robot sees itself); flat ground from 0.8 m above a corner of the checker
    N = 2
    d, k, _ = make_desc("go1plane", N)
    e = hip_engine(d, k)
    e.reset_all()
    ro, do = cc._upright(e, 1)
    ro[:, 0, 2] = d.ground_z + 0.40
    e.tensor(abi.T_ROOT_STATE).copy_(ro)
    base = ro[1, 0, :3].cpu().numpy().astype(np.float64)
    rm = d.robot
    trunk = next(q for q in range(rm.n_prims) if rm.prim_type[q] == abi.PRIM_BOX and rm.prim_body[q] == 0 and all(abs(rm.prim_center[q][i]) < 1e-9 for i in range(3)))
    shoot("self", e, 1, H, W, FOV, base + [0, 0, 2.0], base, trunk=trunk, top=float(rm.prim_center[trunk][2] + rm.prim_half[trunk][2]))
    corner = np.array([round(base[0]) + 2.0, round(base[1]), d.ground_z + 0.8])
    shoot("ground", e, 0, H, W, FOV, corner, corner - [0, 0, 1.0], ground_z=float(d.ground_z))
    e.close()

    # go1gate: robot 0 of every env looks along +x at mid wall height (camera_cases.a_wall_where_the_signed_distance_map_says)
    N = 4
    d, k, _ = make_desc("go1gate", N)
    e = hip_engine(d, k)
    e.reset_all()
    ro, do = cc._upright(e, 2)
    ro[:, 0, 2] = d.ground_z + 0.15
    ro[:, 1, 1] += 50.0 * d.horizontal_scale
    e.tensor(abi.T_ROOT_STATE).copy_(ro)
    nx, ny, hs = d.sdf_nx, d.sdf_ny, d.horizontal_scale
    sdf = np.ctypeslib.as_array(d.wall_sdf, shape=(nx, ny)).copy()
    walls = []
    for env in range(N):
        o = ro[env, 0, :3].cpu().numpy().astype(np.float64) + [0.26, 0, 0]
        t, hit = 0.0, None                                           # host march of the same map along the central ray
        while t < 20.0:
            fx, fy = (o[0] + t) / hs, o[1] / hs
            if fx >= nx - 1 or fy >= ny - 1 or fx < 0 or fy < 0:
                break
            ix, iy = int(fx), int(fy)
            tx, ty = fx - ix, fy - iy
            s = (sdf[ix, iy] * (1 - ty) + sdf[ix, iy + 1] * ty) * (1 - tx) + (sdf[ix + 1, iy] * (1 - ty) + sdf[ix + 1, iy + 1] * ty) * tx
            if s <= 0.002:
                hit = t
                break
            t += max(s, 0.002)
        if hit is not None and hit >= 0.3:
            shoot(f"wall{env}", e, env, H, W, 90.0, o, o + [1.0, 0, 0], far=30.0, hit=hit, hs=hs)
            walls.append(f"wall{env}")
    out["walls"] = walls
    e.close()

    # go1gate on Perlin relief, from above and behind env 0's robots
    d, k, _ = make_desc("go1gate", 2, terrain_cfg=perlin_terrain("go1gate", zScale=0.08))
    e = hip_engine(d, k)
    e.reset_all()
    base = e.tensor(abi.T_ROOT_STATE)[0, 0, :3].cpu().numpy().astype(np.float64)
    shoot("relief", e, 0, H, W, FOV, base + [-2.0, 0.5, 1.5], base + [1.0, 0, 0])
    e.close()

    # go1football-1vs1: robot 1 one metre ahead of robot 0, the ball up and to the left (camera_cases.another_robots_trunk_and_a_ball)
    N = 2
    d, k, _ = make_desc("go1football-1vs1", N)
    e = hip_engine(d, k)
    e.reset_all()
    ro, do = cc._upright(e, 2)
    do[:, :24, 0] = torch.tensor(np.ctypeslib.as_array(d.default_dof_pos, shape=(12,)).copy(), device=do.device).repeat(2)[None, :]
    base = ro[:, 0, :3].clone()
    base[:, 2] = d.ground_z + 0.32
    ro[:, 0, :3] = base
    ro[:, 1, :3] = base + torch.tensor([1.0, 0.0, 0.0], device=ro.device)
    ro[:, 2, :3] = base + torch.tensor([0.9, 0.6, cc.POS[2]], device=ro.device)
    e.tensor(abi.T_ROOT_STATE).copy_(ro); e.tensor(abi.T_DOF_STATE).copy_(do)
    b = ro[1, 0, :3].cpu().numpy().astype(np.float64)
    ball = ro[1, 2, :3].cpu().numpy().astype(np.float64)
    shoot("trunk", e, 1, 64, 64, 90.0, b + cc.POS, b + cc.POS + [1.0, 0, 0], far=10.0)
    # an odd size, so that the centre pixel's ray (yc = zc = 0) runs through the ball's centre
    shoot("ball", e, 1, 33, 33, 60.0, b + cc.POS, ball, far=10.0, centre=ball, radius=float(d.npc_sphere_radius[0]))
    e.close()
    return out


def test_everywhere_on_every_shot(shots):
    for name, s in shots.items():
        if name != "walls":
            everywhere(s["geom"], s["ids"], s["d"])


# ---- 2. a robot sees itself -----------------------------------------------------------------------------------------------------------
def test_a_robot_sees_itself(shots):
    s = shots["self"]
    c = (slice(H // 2 - 1, H // 2 + 1), slice(W // 2 - 1, W // 2 + 1))
    assert (s["ids"][c] == (abi.VIEW_ROBOT | 0 << 8 | s["trunk"] << 16)).all(), s["ids"][c]
    assert np.abs(s["geom"][c][..., 1:] - [0, 0, 1]).max() <= 1e-6
    assert np.abs(-s["geom"][c][..., 0] - (2.0 - s["top"])).max() <= 2e-4          # camera_cases.flat_ground_from_a_known_height's tolerance


# ---- 3. known answers for id and normal -----------------------------------------------------------------------------------------------
def test_flat_ground_and_its_checker(shots):
    s = shots["ground"]
    ids, geom, d, eye = s["ids"], s["geom"], s["d"], s["eye"]
    ground = (ids & 255) == abi.VIEW_GROUND
    assert ground.mean() > 0.5
    assert (geom[ground][:, 1:] == [0, 0, 1]).all()
    t = (s["ground_z"] - eye[2]) / d[..., 2]
    p = eye[None, None, :] + t[..., None] * d
    assert np.abs(-geom[ground][:, 0] - t[ground]).max() <= 2e-4
    fx, fy = p[..., 0] - np.floor(p[..., 0]), p[..., 1] - np.floor(p[..., 1])
    clear = ground & (np.minimum(fx, 1 - fx) > 0.01) & (np.minimum(fy, 1 - fy) > 0.01)      # farther than 1 cm from a cell border
    left_out = int(ground.sum() - clear.sum())
    print(f"checker: {left_out} of {int(ground.sum())} ground pixels within 1 cm of a cell border are left out ({left_out / ground.sum():.2%})")
    assert left_out < 0.05 * ground.sum()
    parity = (np.floor(p[..., 0]) + np.floor(p[..., 1])).astype(np.int64) & 1
    assert (((ids >> 24) & 1)[clear] == parity[clear]).all()
    assert len(np.unique(parity[clear])) == 2                              # both colours of the checker are in view


def test_a_wall_face_seen_head_on(shots):
    assert len(shots["walls"]) >= 2
    for name in shots["walls"]:
        s = shots[name]
        c = (slice(H // 2 - 1, H // 2 + 1), slice(W // 2 - 1, W // 2 + 1))
        assert ((s["ids"][c] & 255) == abi.VIEW_WALL).all(), (name, s["ids"][c])
        n = s["geom"][c][..., 1:].astype(np.float64)
        assert (n[..., 2] == 0).all() and np.abs(np.linalg.norm(n, axis=-1) - 1).max() <= 1e-5
        assert np.abs(n - [-1, 0, 0]).max() <= 1e-3, (name, n)
        assert np.abs(-s["geom"][c][..., 0] - s["hit"]).max() < 3 * s["hs"] + 0.02 * s["hit"]


def test_the_ball(shots):
    s = shots["ball"]
    i = j = 16                                                             # the centre pixel: d = f, through the ball's centre
    assert s["ids"][i, j] == (abi.VIEW_NPC | 0 << 8)
    d = s["d"][i, j]
    depth = -float(s["geom"][i, j, 0])
    want = np.linalg.norm(s["centre"] - s["eye"]) - s["radius"]
    tol = 1e-4 + 1e-5 * want                                               # test 1's depth tolerance; a hit point that far off turns the normal by tol / r
    assert abs(depth - want) <= tol + 2e-6                                 # (+ the f32 rounding of the ball's centre as the test reads it back)
    assert np.abs(s["geom"][i, j, 1:] + d / np.linalg.norm(d)).max() <= tol / s["radius"]


def test_another_robots_trunk_from_behind(shots):
    s = shots["trunk"]
    c = (slice(31, 33), slice(31, 33))
    assert ((s["ids"][c] & 0xFFFF) == (abi.VIEW_ROBOT | 1 << 8)).all(), s["ids"][c]
    assert np.abs(s["geom"][c][..., 1:] - [-1, 0, 0]).max() <= 1e-5        # minus robot 1's x axis (upright, heading +x)
    assert np.abs(-s["geom"][c][..., 0] - (1.0 - 0.3762 / 2 - cc.POS[0])).max() < 2e-3


# ---- 4. colour ------------------------------------------------------------------------------------------------------------------------
def test_colour_is_the_documented_function_of_id_and_normal(shots):
    for name, s in shots.items():
        if name != "walls":
            assert_colour(s["rgba"], s["geom"], s["ids"])
    assert ((shots["relief"]["ids"] & 255) == abi.VIEW_GROUND).mean() > 0.3
    # robots of different index: robot 0's trunk from above, robot 1's trunk from behind
    c0 = shots["self"]["rgba"][H // 2, W // 2, :3].astype(int)
    c1 = shots["trunk"]["rgba"][31, 31, :3].astype(int)
    assert np.abs(c0 - c1).max() > 40, (c0, c1)
    assert abi.VIEW_PALETTE[2] != abi.VIEW_PALETTE[3]
    assert abs(sum(x * x for x in abi.VIEW_LIGHT) - 1) < 1e-12


# ---- 5. shapes ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gate():
    d, k, _ = make_desc("go1gate", 2)
    e = hip_engine(d, k)
    e.reset_all()
    base = e.tensor(abi.T_ROOT_STATE)[1, 0, :3].cpu().numpy().astype(np.float64)
    yield e, base + [-2.0, 0.5, 1.5], base + [1.0, 0, 0]
    e.close()


GUARD = 64


def guarded(h, w, dev):
    """the three output buffers prefilled with sentinels no pixel can hold, GUARD elements longer than the image"""
    rgba = torch.full((h * w * 4 + GUARD,), 0x5A, dtype=torch.uint8, device=dev)        # (a written pixel's alpha is 255)
    geom = torch.full((h * w * 4 + GUARD,), 12345.0, dtype=torch.float32, device=dev)   # (a depth is negative)
    ids = torch.full((h * w + GUARD,), -1, dtype=torch.int32, device=dev)               # (an id word is not negative)
    return rgba, geom, ids


def untouched(rgba, geom, ids, n=0):
    return bool((rgba[n * 4:] == 0x5A).all()) and bool((geom[n * 4:] == 12345.0).all()) and bool((ids[n:] == -1).all())


@pytest.mark.parametrize("h,w", [(1, 1), (37, 51), (240, 360)])
def test_every_pixel_written_and_nothing_else(gate, h, w):
    e, eye, lookat = gate
    bufs = guarded(h, w, e.torch_device)
    assert raw_view(e, 1, *bufs, h, w, FOV, eye, lookat, 60.0) == 0
    torch.cuda.synchronize()
    rgba, geom, ids = bufs
    assert untouched(rgba, geom, ids, h * w)                               # the guard words behind each buffer
    assert (rgba[:h * w * 4].view(h, w, 4)[..., 3] == 255).all()
    assert (geom[:h * w * 4].view(h, w, 4)[..., 0] < 0).all()
    assert (ids[:h * w] >= 0).all()
    if (h, w) == (37, 51):                                                 # a second render: bit for bit
        again = guarded(h, w, e.torch_device)
        assert raw_view(e, 1, *again, h, w, FOV, eye, lookat, 60.0) == 0
        torch.cuda.synchronize()
        assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(bufs, again))
    if (h, w) == (240, 360):
        classes = set(np.unique(ids[:h * w].cpu().numpy() & 255).tolist())
        assert {abi.VIEW_GROUND, abi.VIEW_WALL, abi.VIEW_ROBOT} <= classes, classes


# ---- 6. no side effects ---------------------------------------------------------------------------------------------------------------
def test_a_render_changes_no_state_tensor(gate):
    e, eye, lookat = gate
    g = torch.Generator().manual_seed(5)
    for t in range(2):
        e.step((torch.rand(2, 2, 3, generator=g) * 2 - 1).cuda())
    tens = {k: e.tensor(k) for k in range(abi.T_COUNT)}
    tens = {k: t for k, t in tens.items() if t.numel() > 0}                # (a scene without NPCs has empty NPC tensors)
    assert len(tens) >= abi.T_COUNT - 3
    before = {k: t.clone() for k, t in tens.items()}
    view(e, 0, H, W, FOV, eye, lookat)
    view(e, 1, 240, 360, 90.0, eye, lookat)
    for k, b in before.items():
        assert torch.equal(tens[k].view(torch.uint8), b.view(torch.uint8)), k


def _gate_env(n, record_video, steps_per_episode=None):
    from mqe.envs.utils import make_mqe_env, custom_cfg
    from mqe.utils.helpers import finish_args
    a = finish_args(types.SimpleNamespace(task="go1gate", num_envs=n, seed=1, headless=True, record_video=record_video, sim_device="cuda:0", pipeline="gpu",
                                          subscenes=0, num_threads=0))
    base = custom_cfg(a)

    def cfg_fn(c):
        c = base(c)
        if steps_per_episode is not None:
            c.env.episode_length_s = (steps_per_episode - 0.5) * 0.02
        return c
    return make_mqe_env("go1gate", a, cfg_fn)[0]


@pytest.fixture
def gate_cfg_restored():
    from mqe.envs.utils import ENV_DICT
    c = ENV_DICT["go1gate"]["config"]
    saved = (c.env.num_envs, c.env.episode_length_s, c.env.record_video)
    yield
    c.env.num_envs, c.env.episode_length_s, c.env.record_video = saved


def test_recording_changes_no_rollout(gate_cfg_restored):
    outs = []
    for live in (False, True):
        env = _gate_env(4, True)
        if live:
            env.start_recording()
        g = torch.Generator().manual_seed(11)
        trace = [env.reset()]
        for t in range(8):
            obs, rew, done, _ = env.step((torch.rand(4, 2, 3, generator=g) * 2 - 1).cuda())
            trace += [obs, rew, done]
        torch.cuda.synchronize()
        outs.append([x.clone() for x in trace])
        if live:
            assert len(env.video_frames) == 8                     # reset() opened the episode, every step added its frame
        env.close()
    for x, y in zip(*outs):
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))


# ---- 7. through the public surface ----------------------------------------------------------------------------------------------------
def test_a_recorded_episode_through_make_mqe_env(gate_cfg_restored):
    env = _gate_env(2, True, steps_per_episode=6)
    env.start_recording()
    env.reset()
    g = torch.Generator().manual_seed(2)
    frames = []
    for t in range(12):
        _, _, done, _ = env.step((torch.rand(2, 2, 3, generator=g) * 2 - 1).cuda())
        if bool(done[0]):
            frames = env.get_complete_frames()
            break
    env.close()
    assert len(frames) > 0 and all(isinstance(f, np.ndarray) and f.shape == (240, 360, 4) and f.dtype == np.uint8 for f in frames)
    assert any(not np.array_equal(frames[0], f) for f in frames[1:])
    albedos = {"ground": abi.VIEW_PALETTE[0], "wall": abi.VIEW_PALETTE[1], "robot 0": abi.VIEW_PALETTE[2], "robot 1": abi.VIEW_PALETTE[3]}
    for f in frames:
        rgb = f[..., :3].reshape(-1, 3).astype(np.float64)
        seen = [name for name, a in albedos.items() if _pixels_of(rgb, a) >= 8]
        seen += ["sky"] if (rgb == np.asarray(abi.VIEW_SKY, np.float64)).all(-1).sum() >= 8 else []
        assert len(seen) >= 3, seen


def _pixels_of(rgb, albedo):
    """how many pixels are 255 * albedo * s for one brightness s in [(1 - checker) ambient, 1 + checker], each channel to the rounding's +-1"""
    a = 255 * np.asarray(albedo, np.float64)
    s = (rgb / a).mean(-1)
    ok = (np.abs(rgb - s[:, None] * a).max(-1) <= 1.0) & (s >= (1 - abi.VIEW_CHECKER) * abi.VIEW_AMBIENT - 0.01) & (s <= 1 + abi.VIEW_CHECKER + 0.01)
    return int(ok.sum())


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------------
def test_every_refusal_returns_its_code_and_launches_nothing(gate):
    e, eye, lookat = gate
    h, w = 8, 8
    bufs = guarded(h, w, e.torch_device)
    ok = dict(env=0, h=h, w=w, fov=FOV, eye=eye, lookat=lookat, far=60.0)

    def call(rgba=bufs[0], geom=bufs[1], ids=bufs[2], **over):
        a = dict(ok, **over)
        return raw_view(e, a["env"], rgba, geom, ids, a["h"], a["w"], a["fov"], a["eye"], a["lookat"], a["far"])
    cases = [(-6, dict(env=-1)), (-6, dict(env=2)), (-1, dict(rgba=None, geom=None, ids=None)),
             (-6, dict(h=0)), (-6, dict(w=-3)), (-6, dict(h=1024, w=1025)), (-6, dict(h=1 << 16, w=1 << 16)),
             (-6, dict(fov=1.0)), (-6, dict(fov=179.0)), (-6, dict(far=0.0)), (-6, dict(far=-1.0)),
             (-6, dict(lookat=eye)), (-6, dict(lookat=np.asarray(eye) + [0, 0, 5e-7])), (-1, dict(eye=None)), (-1, dict(lookat=None)),
             (-6, dict(rgba=bufs[0].data_ptr() + 1)), (-6, dict(geom=bufs[1].data_ptr() + 4)), (-6, dict(ids=bufs[2].data_ptr() + 2))]
    for code, over in cases:
        assert call(**over) == code, (code, {k: v for k, v in over.items() if k not in ("rgba", "geom", "ids")})
        assert e.lib.mqe_last_error().decode() != ""
    f = e.lib.mqe_render_view
    assert f(None, 0, C.c_void_p(bufs[0].data_ptr()), None, None, h, w, C.c_float(FOV), (C.c_float * 3)(*eye), (C.c_float * 3)(*lookat), C.c_float(60.0), None) == -1
    inside = []
    e.step(torch.zeros(2, 2, 3).cuda(), between=lambda: inside.append(call()))      # between mqe_step_begin and mqe_step_end
    assert inside == [-8]
    torch.cuda.synchronize()
    assert untouched(*bufs)
    assert call() == 0                                                      # ... and the same call with nothing wrong renders
    torch.cuda.synchronize()
    assert untouched(*bufs, n=h * w) and (bufs[0][:h * w * 4].view(h, w, 4)[..., 3] == 255).all()
    with pytest.raises(ValueError):
        e.render_view(0, 2048, 2048, FOV, eye, lookat)
    with pytest.raises(RuntimeError, match="mqe_render_view"):
        e.render_view(5, h, w, FOV, eye, lookat)
