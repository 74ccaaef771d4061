"""-m gpu: the locomotion policy kernels -- layer 0 as k_gemm_h2 / k_gemm_h2_mix (split-f16) or k_gemm_f32 (exact), the rest as k_policy_tail
or the general chain -- against the float64 reference of tests/policy_ref.py on histories written by the host: every grid of policy_ref.GRIDS,
row counts at every kernel's tile edges, bodies of other shapes and weight ranges, and the inputs beyond the f16 planes' range, where the
kernels' behaviour is the clamp that forward64(clamp0, clamp_tail) states.  The bound is K_GPU * bound64, K_GPU measured on the CPU
(policy_ref.py); the worst ratio of every case goes to the measurement log (kind policy_f64)."""
import numpy as np
import pytest
import torch

import policy_ref as pr
from helpers import make_desc, hip_engine
from mqe.engine import abi
from mqe.utils import policy_weights as pw
from test_gpu_parity import _record

pytestmark = pytest.mark.gpu

SWITCHES = ("MQE_GEMM_SPLIT", "MQE_NO_FUSED_TAIL")
PATHS = [("split-fused", True, True), ("split-chain", True, False), ("exact-fused", False, True), ("exact-chain", False, False)]
_NETS = {}


def shipped():
    """(adaptation module, synthetic body) as build_desc loads them"""
    if not _NETS:
        Wb, bb, _ = pw.load_body(None, seed=0)
        _NETS["ada"], _NETS["body"] = pw.load_adaptation_module(), (Wb, bb)
    return _NETS["ada"], _NETS["body"]


def policy_engine(monkeypatch, task, N, split, fused, body=None, **kw):
    """(engine, desc) on `task` under MQE_GEMM_SPLIT = split and, unless fused, MQE_NO_FUSED_TAIL=1; after reset_all and one step of zero
    actions, so that the observation bag the next frame is made of is real"""
    env = {"MQE_GEMM_SPLIT": "1" if split else "0", **({} if fused else {"MQE_NO_FUSED_TAIL": "1"})}
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        if body is not None:
            kw["body"] = body
        d, keep, _ = make_desc(task, N, max_episode_length=100000, **kw)
        e = hip_engine(d, keep)
    finally:
        for k in env:
            monkeypatch.delenv(k)
    e.reset_all()
    e.step(torch.zeros(N, e.tensor(abi.T_WRAPPER_OBS).shape[1], 3, device="cuda"))
    torch.cuda.synchronize()
    return e, d


def run_policy(e, d, frames, seed=0, obs_bag=None, same=0):
    """one policy_step on the host-written history `frames` [R, 30, 70] (a grid): all 30 ring slots written (pad columns zero) so that
    frames[0 .. 28] are the 29 frames that stay once the step has pushed its own over the oldest slot (which gets frames[29]), the two action
    registers = frames[29]'s action columns (policy_ref.registers), history_sync, policy_step on a seeded command.  obs_bag: the observation
    bag to build the pushed frame from (another engine's); same: the first `same` rows get row 0's bag and command.  -> dict of host arrays:
    hist (what the kernels saw, HipEngine.history()), out (T_LAST_LOCO_ACTION), actions, last_two, wrote (the registers written)."""
    R = d.num_envs * d.num_agents
    assert frames.shape == (R, pr.HIST, pr.FRAME) and frames.dtype == np.float32
    pos = e._n_policy % abi.HIST                                          # the slot of the oldest frame = the one the step overwrites
    ring = np.zeros((R, abi.HIST, 72), np.float32)
    ring[:, (pos + np.arange(abi.HIST)) % abi.HIST, :pr.FRAME] = frames[:, np.r_[pr.HIST - 1, 0:pr.HIST - 1]]
    ll, l2 = pr.registers(frames)
    e.tensor(abi.T_HISTORY).copy_(torch.from_numpy(ring))
    e.tensor(abi.T_LAST_LOCO_ACTION).copy_(torch.from_numpy(ll))
    e.tensor(abi.T_LAST_TWO_LOCO_ACTION).copy_(torch.from_numpy(l2))
    bag = e.tensor(abi.T_OBS_BAG)
    if obs_bag is not None:
        bag.copy_(obs_bag)
    g = torch.Generator().manual_seed(seed)
    cmd = (torch.rand(R, d.num_command_dims, generator=g) * 2 - 1) * 0.8
    if same:
        bag[:same] = bag[0].clone()
        cmd[:same] = cmd[0]
    e.history_sync()
    e.policy_step(cmd.cuda().contiguous())
    torch.cuda.synchronize()
    hist = e.history().cpu().numpy()
    seen = hist.reshape(R, pr.HIST, pr.FRAME)
    assert np.array_equal(seen[:, :-1].view(np.int32), frames[:, :-1].view(np.int32)), "the written history did not reach the ring"
    assert np.array_equal(seen[:, -1, 42:54], ll) and np.array_equal(seen[:, -1, 54:66], l2), "the pushed frame does not carry the registers"
    assert np.array_equal(seen[:, -1, 6:18], np.broadcast_to(pr.command_obs(d), (R, 12)))
    return dict(hist=hist, wrote=ll, out=e.tensor(abi.T_LAST_LOCO_ACTION).cpu().numpy(), actions=e.tensor(abi.T_ACTIONS).cpu().numpy().reshape(R, 12),
                last_two=e.tensor(abi.T_LAST_TWO_LOCO_ACTION).cpu().numpy())


def check(d, res, ada, body, clamp0, clamp_tail, what):
    """the joint targets within K_GPU bound64 of forward64 on the history the kernels saw, everything finite, T_ACTIONS the clipped targets
    and T_LAST_TWO_LOCO_ACTION the previous targets bit for bit.  -> (worst ratio, its row, its output)"""
    ref, _, tr = pr.forward64(res["hist"], ada, body, clamp0=clamp0, clamp_tail=clamp_tail)
    bnd = pr.bound64(tr)
    r = pr.ratio(res["out"], ref, bnd)
    i, j = np.unravel_index(int(np.argmax(r)), r.shape)
    print(f"    {what}: worst |out - out64| / bound64 = {r[i, j]:.3f} (row {i}, output {j}: {res['out'][i, j]!r} vs {ref[i, j]!r}, bound {bnd[i, j]:.3e})")
    assert np.isfinite(res["out"]).all() and np.isfinite(res["actions"]).all(), what
    assert (r <= pr.K_GPU).all(), (f"{what}: row {i} output {j}: {res['out'][i, j]!r}, float64 {ref[i, j]!r}, bound64 {bnd[i, j]:.3e}, "
                                   f"ratio {r[i, j]:.2f} > K_GPU = {pr.K_GPU}; {int((r.max(1) > pr.K_GPU).sum())} of {len(r)} rows outside")
    c = np.float32(d.clip_actions)
    assert np.array_equal(res["actions"].view(np.int32), np.clip(res["out"], -c, c).view(np.int32)), f"{what}: T_ACTIONS is not the clipped target"
    assert np.array_equal(res["last_two"].view(np.int32), res["wrote"].view(np.int32)), f"{what}: T_LAST_TWO_LOCO_ACTION is not the previous target"
    return float(r[i, j]), int(i), int(j)


def l0_is_split(body, split):
    """mqe_engine.hip: the split kernel runs when asked for and the fused layer 0 (256 adaptation + body columns, padded to 64) tiles by 192"""
    n = 256 + body[0][0].shape[0]
    return bool(split) and ((n + 63) // 64 * 64) % 192 == 0


@pytest.mark.parametrize("path,split,fused", PATHS, ids=[p[0] for p in PATHS])
def test_policy_paths_against_float64(monkeypatch, path, split, fused):
    """the four arithmetic paths on every grid at R = 32 rows (exactly one tail block)"""
    N = 16
    ada, body = shipped()
    e, d = policy_engine(monkeypatch, "go1gate", N, split, fused)
    worst = {}
    for gi, g in enumerate(pr.GRIDS):
        res = run_policy(e, d, pr.grid(g, 2 * N, pr.command_obs(d), gi), seed=gi)
        worst[g] = check(d, res, ada, body, split, fused, f"{path} {g}")
    e.close()
    _record("policy_f64", {"test": "paths", "path": path, "N": N, "worst_ratio_row_output": worst, "K_GPU": pr.K_GPU})


def _mixed(R, cobs, seed):
    f = pr.grid("unit", R, cobs, seed)
    f[1::2] = pr.grid("irregular", R, cobs, seed + 1)[1::2]
    return f


TILINGS = [("go1gate", n, 0) for n in (1, 17, 32, 33, 64, 65, 129)] + [("go1football-defender", 5, 0), ("go1gate", 33, 40)]


@pytest.mark.parametrize("task,N,offset", TILINGS, ids=[f"{t}-{n}" + (f"-offset{o}" if o else "") for t, n, o in TILINGS])
def test_row_tiling_against_float64(monkeypatch, task, N, offset):
    """split and exact layer 0 with the fused tail at R = 2, 34, 64, 66, 128, 130, 258 and 15 rows -- the tail's 32 rows, the half tile's 64,
    the full tile's 128, k_gemm_f32's 64, ragged ends, one odd R -- on unit rows interleaved with irregular ones; once more with an
    env_id_offset of 40 (block0 = 2: the tail's k order starts elsewhere), under the same bound"""
    ada, body = shipped()
    worst = {}
    for split in (True, False):
        e, d = policy_engine(monkeypatch, task, N, split, True, **({"env_id_offset": offset} if offset else {}))
        R = d.num_envs * d.num_agents
        res = run_policy(e, d, _mixed(R, pr.command_obs(d), 50 + N), seed=N)
        worst["split" if split else "exact"] = check(d, res, ada, body, split, True, f"{task} N={N} offset={offset} {'split' if split else 'exact'}")
        e.close()
    _record("policy_f64", {"test": "tiling", "task": task, "N": N, "env_id_offset": offset, "worst_ratio_row_output": worst, "K_GPU": pr.K_GPU})


@pytest.mark.parametrize("split", [True, False], ids=["split", "exact"])
def test_rows_do_not_see_each_other(monkeypatch, split):
    """one history (and one observation bag and command) in all 32 rows of the first tail block, 32 rows of `wide` behind it: the 32 copies'
    joint targets are identical bit for bit, and stay what they are when the neighbours become `over` (every row is its own MFMA row,
    the epilogues mask by row)"""
    N = 32
    ada, body = shipped()
    e, d = policy_engine(monkeypatch, "go1gate", N, split, True)
    cobs = pr.command_obs(d)
    outs = []
    for other in ("wide", "over"):
        f = pr.grid(other, 2 * N, cobs, 7)
        f[:32] = _mixed(4, cobs, 90)[1]                       # an irregular row: the residual epilogue runs in all 32 copies
        res = run_policy(e, d, f, seed=4, same=32)
        assert (res["hist"][:32] == res["hist"][0]).all()
        check(d, res, ada, body, split, True, f"copies next to {other}")
        assert np.array_equal(res["out"][:32].view(np.int32), np.broadcast_to(res["out"][0], (32, 12)).view(np.int32)), f"copies differ next to {other}"
        outs.append(res["out"][:32])
    assert np.array_equal(outs[0].view(np.int32), outs[1].view(np.int32)), "the copies' targets changed with their neighbours"
    e.close()


def test_saturation_is_the_documented_clamp(monkeypatch):
    """edge1023 and over: the split + fused path is within the bound of the SATURATING reference (history operand clamped at +-1023.5, the
    tail's planes at +-65504) and finite; the exact + chain path on the same histories within the bound of the unclamped one; and the two
    differ by more than 2 K_GPU bound64 in some row: the grids did reach the clamp"""
    N = 16
    ada, body = shipped()
    e1, d = policy_engine(monkeypatch, "go1gate", N, True, True)
    e2, _ = policy_engine(monkeypatch, "go1gate", N, False, False)
    worst = {}
    for g in ("edge1023", "over"):
        f = pr.grid(g, 2 * N, pr.command_obs(d), pr.GRIDS.index(g))
        r1 = run_policy(e1, d, f, seed=1)
        r2 = run_policy(e2, d, f, seed=1, obs_bag=e1.tensor(abi.T_OBS_BAG))
        assert np.array_equal(r1["hist"], r2["hist"])
        worst[g] = {"split-fused": check(d, r1, ada, body, True, True, f"split-fused {g}"), "exact-chain": check(d, r2, ada, body, False, False, f"exact-chain {g}")}
        bnd = pr.bound64(pr.forward64(r1["hist"], ada, body, clamp0=True, clamp_tail=True)[2])
        apart = np.abs(r1["out"].astype(np.float64) - r2["out"]) / bnd
        print(f"    {g}: the two paths are up to {apart.max():.3g} bound64 apart, {int((apart.max(1) > 2 * pr.K_GPU).sum())} of {2 * N} rows beyond 2 K_GPU")
        assert (apart > 2 * pr.K_GPU).any(), f"{g} never reached the clamp"
    e1.close(); e2.close()
    _record("policy_f64", {"test": "saturation", "worst_ratio_row_output": worst, "K_GPU": pr.K_GPU})


@pytest.mark.parametrize("hidden", [(96, 40), (64,), (128, 64, 32, 16, 8)], ids=["96-40", "64", "128-64-32-16-8"])
def test_general_shape_bodies_against_float64(monkeypatch, hidden):
    """bodies of other shapes take the general chain (k_gemm_f32 per layer, padded to 64 columns and 16 k): widths that are no multiple of 64
    nor, as the next layer's K, of 16 (96: layer 0 pads the body's columns to 352 -> 384 with zero weights, which the engine refused until this
    test asked for it; 40: K = 48); one hidden layer; MQE_MAX_LAYERS layers.  Both settings of MQE_GEMM_SPLIT, grids unit and wide, R = 34.
    A layer 0 of 256 + 64 columns does not tile by 192, so there the switch must change nothing; elsewhere it must change the bits."""
    N = 17
    ada = shipped()[0]
    body = pr.general_body(hidden, seed=3)
    assert len(body[0]) <= 6
    outs, worst, bag = {}, {}, None
    for split in (True, False):
        e, d = policy_engine(monkeypatch, "go1gate", N, split, True, body=body)
        for g in ("unit", "wide"):
            res = run_policy(e, d, pr.grid(g, 2 * N, pr.command_obs(d), pr.GRIDS.index(g)), seed=2, obs_bag=bag)
            worst[f"{'split' if split else 'exact'} {g}"] = check(d, res, ada, body, l0_is_split(body, split), False, f"body {hidden} split={split} {g}")
            outs[split, g] = res["out"]
        bag = e.tensor(abi.T_OBS_BAG).clone()
        e.close()
    for g in ("unit", "wide"):
        same = np.array_equal(outs[True, g].view(np.int32), outs[False, g].view(np.int32))
        assert same != l0_is_split(body, True), f"body {hidden} {g}: MQE_GEMM_SPLIT {'did not reach' if same else 'changed'} layer 0"
    _record("policy_f64", {"test": "general_body", "hidden": list(hidden), "worst_ratio_row_output": worst, "K_GPU": pr.K_GPU})


def test_fused_shape_body_with_a_wide_weight_range(monkeypatch):
    """policy_ref.heavy_tailed_body: the fused tail's shape with weights of 0.05 next to a few of 20 .. 50 per layer, so that the per-layer
    weight scale leaves the small weights' low planes in the f16 subnormals (the emulated design holds there: tests/test_policy_ref.py).
    Both layer-0 kernels with the fused tail, grids unit and tiny, R = 32; the chain on the same histories gives other bits (the fused tail
    did run) within the same bound."""
    N = 16
    ada = shipped()[0]
    body = pr.heavy_tailed_body(0)
    outs, worst, bag = {}, {}, None
    for name, split, fused in (("split-fused", True, True), ("exact-fused", False, True), ("exact-chain", False, False)):
        e, d = policy_engine(monkeypatch, "go1gate", N, split, fused, body=body)
        for g in ("unit", "tiny"):
            res = run_policy(e, d, pr.grid(g, 2 * N, pr.command_obs(d), pr.GRIDS.index(g)), seed=3, obs_bag=bag)
            worst[f"{name} {g}"] = check(d, res, ada, body, split, fused, f"heavy-tailed body {name} {g}")
            outs[name, g] = res["out"]
        bag = e.tensor(abi.T_OBS_BAG).clone()
        e.close()
    for g in ("unit", "tiny"):
        assert not np.array_equal(outs["exact-fused", g], outs["exact-chain", g]), "MQE_NO_FUSED_TAIL changed nothing: did the fused tail run?"
        assert not np.array_equal(outs["split-fused", g], outs["exact-fused", g]), "MQE_GEMM_SPLIT changed nothing"
    _record("policy_f64", {"test": "heavy_tailed_body", "worst_ratio_row_output": worst, "K_GPU": pr.K_GPU})
