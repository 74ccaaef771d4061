"""The terrain height scan's surface on a CPU-only host (mqe_measure_heights, mqe_set_height_refresh; Go1.measured_heights): the two entry
points are declared and exported without an ABI bump, the Go1-level grid follows upstream's _init_height_points and refuses an engine that
has no scan, the float64 reference (tests/height_ref.py) gives the known answers of its specification, and k_height_scan's code object
uses no scratch."""
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

import height_ref
from mqe.engine import abi
from mqe.engine.hip_engine import LIB_PATH
from mqe.envs.go1.go1 import Go1

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mqe_hip.h")
LLVM = "/opt/rocm/lib/llvm/bin"
TOOLS = ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")


def _header_code():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_entry_points_declared_and_exported_without_an_abi_bump():
    code = _header_code()
    assert re.search(r"\bint mqe_measure_heights\(mqe_sim\* s, float\* out_dev, const float\* points_xy, int n_points, int flags, void\* stream\);", code)
    assert re.search(r"\bint mqe_set_height_refresh\(mqe_sim\* s, float\* out_dev, const float\* points_xy, int n_points, int flags\);", code)
    assert re.search(r"#define MQE_MAX_HEIGHT_POINTS 1024\b", code) and abi.MAX_HEIGHT_POINTS == 1024
    assert re.search(r"#define MQE_HSCAN_SCENERY 1\b", code) and abi.HSCAN_SCENERY == 1
    assert re.search(r"#define MQE_ABI_VERSION 17\b", code)
    assert "v17, additive" in open(HEADER).read()
    assert os.path.isfile(LIB_PATH), "run __graft_entry__.build() first"
    lib = C.CDLL(LIB_PATH)
    assert hasattr(lib, "mqe_measure_heights") and hasattr(lib, "mqe_set_height_refresh")
    assert lib.mqe_abi_version() == abi.ABI_VERSION == 17


def _oracle_factory(desc, keep, device):
    from oracle_engine import OracleEngine
    return OracleEngine(desc, keep)


def _go1(monkeypatch, cfg):
    from mqe.envs.utils import ENV_DICT  # noqa: F401  (registers the task configs' classes)
    monkeypatch.setattr(Go1, "engine_factory", staticmethod(_oracle_factory))
    monkeypatch.setattr(Go1, "shard", None)
    env_cfg = type("env", (cfg.env,), {"num_envs": 2})
    cfg = type(cfg.__name__ + "Small", (cfg,), {"env": env_cfg})
    sim = types.SimpleNamespace(dt=cfg.sim.dt, use_gpu_pipeline=False)
    return Go1(cfg, sim, None, "cpu", True)


def test_height_points_on_oracle_backed_go1(monkeypatch):
    from mqe.envs.configs.go1_gate_config import Go1GateCfg
    env = _go1(monkeypatch, Go1GateCfg)
    try:
        assert env.cfg.terrain.measure_heights is True
        assert env.num_height_points == 187
        x = torch.tensor(env.cfg.terrain.measured_points_x)
        y = torch.tensor(env.cfg.terrain.measured_points_y)
        assert len(x) == 17 and len(y) == 11
        gx, gy = torch.meshgrid(x, y, indexing="ij")
        hp = env.height_points
        assert hp.shape == (2 * env.num_agents, 187, 3) and hp is env.height_points
        assert torch.equal(hp[:, :, 0], gx.flatten().expand(hp.shape[0], -1))
        assert torch.equal(hp[:, :, 1], gy.flatten().expand(hp.shape[0], -1))
        assert (hp[:, :, 2] == 0).all()
        assert hp[0, 1, 0] == x[0] and hp[0, 1, 1] == y[1]          # x-major: point i * len(y) + j = (x[i], y[j])
        with pytest.raises(NotImplementedError, match="HipEngine"):
            env.measured_heights
        with pytest.raises(NotImplementedError, match="HipEngine"):
            env._get_heights()
    finally:
        env.close()


def test_measured_heights_names_the_switch_when_it_is_off(monkeypatch):
    from mqe.envs.configs.go1_gate_config import Go1GateCfg
    terrain = type("terrain", (Go1GateCfg.terrain,), {"measure_heights": False})
    env = _go1(monkeypatch, type("NoHeightsCfg", (Go1GateCfg,), {"terrain": terrain}))
    try:
        with pytest.raises(RuntimeError, match="measure_heights"):
            env.measured_heights
    finally:
        env.close()


# ---- known answers of the float64 reference itself ---------------------------------------------------------------------------------
def _terrain(nx=40, ny=30, **kw):
    t = types.SimpleNamespace(wall_sdf=np.full((nx, ny), 1e3, np.float32), wall_height=0.5, ground_z=0.25, ground_height=None, wall_top=None)
    t.__dict__.update(kw)
    return t


def test_reference_flat_slab_gives_ground_z():
    t = _terrain()
    x, y = np.meshgrid(np.linspace(-1.0, 5.0, 13), np.linspace(-1.0, 4.0, 11), indexing="ij")
    assert (height_ref.surface_height(x, y, t, 0.1) == 0.25).all()


def test_reference_wall_footprint_gives_wall_height():
    sdf = np.full((40, 30), 0.3, np.float32)
    sdf[10:15, 5:9] = -0.2
    t = _terrain(wall_sdf=sdf)
    assert height_ref.surface_height(1.2, 0.65, t, 0.1) == 0.5            # well inside: the four corners of its cell are inside
    assert height_ref.surface_height(3.0, 2.0, t, 0.1) == 0.25
    # per-cell tops: the nearer raster point's entry
    wt = np.zeros((40, 30), np.float32)
    wt[12, 6], wt[13, 6], wt[12, 7], wt[13, 7] = 0.4, 0.6, 0.8, 1.0
    t2 = _terrain(wall_sdf=sdf, wall_top=wt)
    assert height_ref.surface_height(1.22, 0.63, t2, 0.1) == np.float64(np.float32(0.4))
    assert height_ref.surface_height(1.28, 0.63, t2, 0.1) == np.float64(np.float32(0.6))
    assert height_ref.surface_height(1.22, 0.68, t2, 0.1) == np.float64(np.float32(0.8))
    assert height_ref.surface_height(1.28, 0.68, t2, 0.1) == np.float64(np.float32(1.0))
    # a relief above the wall top wins: H = max(g, top)
    t3 = _terrain(wall_sdf=sdf, ground_height=np.full((40, 30), 0.5, np.float32))
    assert height_ref.surface_height(1.2, 0.65, t3, 0.1) == 0.75


def test_reference_relief_at_raster_points_and_clamped_edges():
    rng = np.random.default_rng(0)
    gh = rng.uniform(-0.2, 0.2, (40, 30)).astype(np.float32)
    t = _terrain(ground_height=gh, ground_z=0.0)
    hs = 0.125                                                              # exact in binary: raster points are hit exactly
    i, j = np.meshgrid(np.arange(40), np.arange(30), indexing="ij")
    assert np.array_equal(height_ref.surface_height(i * hs, j * hs, t, hs), gh.astype(np.float64))
    # the middle of a cell: the mean of its corners
    assert abs(height_ref.surface_height(3.5 * hs, 7.5 * hs, t, hs) - gh[3:5, 7:9].astype(np.float64).mean()) < 1e-15
    # 1 km outside the map on every side: the clamped edge value; a NaN lands on index 0
    assert height_ref.surface_height(-1000.0, 5 * hs, t, hs) == gh[0, 5]
    assert height_ref.surface_height(1000.0, 5 * hs, t, hs) == gh[39, 5]
    assert height_ref.surface_height(5 * hs, -1000.0, t, hs) == gh[5, 0]
    assert height_ref.surface_height(5 * hs, 1000.0, t, hs) == gh[5, 29]
    assert height_ref.surface_height(1000.0, 1000.0, t, hs) == gh[39, 29]
    assert height_ref.surface_height(np.nan, np.nan, t, hs) == gh[0, 0]


def test_reference_quat_apply_yaw_is_the_twist_about_z():
    rng = np.random.default_rng(1)
    q = rng.normal(size=(64, 4))
    q /= np.linalg.norm(q, axis=-1, keepdims=True)                        # tilted bodies
    c, s = height_ref.quat_apply_yaw_cs(q)
    for k in range(len(q)):
        z, w = q[k, 2], q[k, 3]
        n = np.hypot(z, w)
        z, w = z / n, w / n                                                 # the normalised (0, 0, z, w)
        # rotating (1, 0, 0) by it: v' = v + 2 w (u x v) + 2 u x (u x v), u = (0, 0, z)
        assert abs(c[k] - (1 - 2 * z * z)) < 1e-14 and abs(s[k] - 2 * w * z) < 1e-14
        assert abs(c[k] * c[k] + s[k] * s[k] - 1) < 1e-14
    # and it is NOT the Euler yaw of a tilted body in general
    x, y, z, w = q.T
    yaw = np.arctan2(2 * (w * z + x * y), 1 - 2 * (y * y + z * z))
    assert np.abs(np.arctan2(s, c) - yaw).max() > 0.1
    # degenerate: identity
    c0, s0 = height_ref.quat_apply_yaw_cs(np.array([[1.0, 0.0, 0.0, 0.0], [0.6, 0.8, 1e-10, 1e-10]]))
    assert (c0 == 1).all() and (s0 == 0).all()
    # the world point of a grid offset
    rows = np.zeros((1, 13)); rows[0, :2] = (3.0, 4.0); rows[0, 3:7] = (0, 0, np.sin(np.pi / 4), np.cos(np.pi / 4))       # +90 deg about z
    wx, wy = height_ref.world_points(rows, np.array([[1.0, 0.0], [0.0, 2.0]]))
    assert np.allclose(wx, [[3.0, 1.0]], atol=1e-15) and np.allclose(wy, [[5.0, 4.0]], atol=1e-15)


def test_reference_scenery_boxes_raise_the_surface():
    t = _terrain()
    boxes = [(np.array([2.0, 1.5, 0.4]), np.array([0.5, 0.25, 0.1]))]
    assert height_ref.surface_height(2.4, 1.6, t, 0.1, boxes) == 0.5
    assert height_ref.surface_height(2.6, 1.6, t, 0.1, boxes) == 0.25
    assert height_ref.surface_height(2.4, 1.6, t, 0.1) == 0.25


# ---- the code object ---------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not (os.path.isfile(LIB_PATH) and all(os.path.isfile(os.path.join(LLVM, t)) for t in TOOLS)),
                    reason="needs the built HIP engine and the ROCm LLVM tools")
def test_k_height_scan_uses_no_scratch(tmp_path):
    fat, co = str(tmp_path / "fat.bin"), str(tmp_path / "dev.co")
    subprocess.check_call([f"{LLVM}/llvm-objcopy", "--dump-section", f".hip_fatbin={fat}", LIB_PATH, str(tmp_path / "stripped.so")])
    subprocess.check_call([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"])
    notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True, check=True).stdout
    mine = [dict(re.findall(r"\.(\w+):\s*(\S+)", ".agpr_count:" + blk)) for blk in notes.split("- .agpr_count:")[1:]]
    mine = [f for f in mine if "k_height_scan" in f.get("name", "")]
    assert len(mine) == 1, [f.get("name") for f in mine]
    f = mine[0]
    print("k_height_scan: vgpr", f["vgpr_count"], "sgpr", f["sgpr_count"], "lds", f["group_segment_fixed_size"], "scratch", f["private_segment_fixed_size"],
          "vgpr spills", f["vgpr_spill_count"], "sgpr spills", f["sgpr_spill_count"])
    assert int(f["private_segment_fixed_size"]) == 0 and int(f["vgpr_spill_count"]) == 0
    assert int(f["max_flat_workgroup_size"]) == 256
    assert int(f["group_segment_fixed_size"]) <= 8192 + 1024          # the point table + the robots' records
