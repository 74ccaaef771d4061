"""On-device GAE on a CPU-only host (mqe_rollout_time_outs, mqe_gae; HipEngine.gae, FusedTaskWrapper.rollout(gamma=...)): the exports exist
without an ABI bump, the float64 reference of the GPU test is right on cases worked by hand, the synthetic trajectory hits every branch,
the derived tolerances hold a float32 evaluation and reject wrong variants, the kernels use no scratch, an oracle-backed env refuses."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import gae_ref as ref
from mqe.engine import abi
from mqe.engine.hip_engine import LIB_PATH, Rollout
from test_rollout import HEADER, LLVM, TOOLS, _header_code, gate_wrapper  # noqa: F401  (the oracle-backed go1gate wrapper fixture)

CASES = [(s, gl, to) for s in ref.SHAPES for gl in ref.GAMMA_LAM for to in (True, False)]
IDS = [f"N{s[0]}xA{s[1]}xT{s[2]}-g{gl[0]}-l{gl[1]}-{'to' if to else 'noto'}" for s, gl, to in CASES]


# ---- exports and header ----------------------------------------------------------------------------------------------------------------
def test_exports_declared_and_exported_without_an_abi_bump():
    code = re.sub(r"\s+", " ", _header_code())
    assert "int mqe_rollout_time_outs(mqe_sim* s, uint8_t* time_outs_dev, int capacity_steps);" in code
    assert ("int mqe_gae(mqe_sim* s, int T, const float* packed_dev, long long row_stride, const float* value_dev, const uint8_t* time_outs_dev, "
            "float gamma, float lam, int flags, float* adv_dev, float* ret_dev, float* stats_dev, void* stream);") in code
    assert re.search(r"#define MQE_ABI_VERSION 17\b", code)
    lib = C.CDLL(LIB_PATH)
    for name in ("mqe_rollout_time_outs", "mqe_gae"):
        assert hasattr(lib, name), name
    assert lib.mqe_abi_version() == abi.ABI_VERSION == 17
    assert lib.mqe_sizeof_desc() == C.sizeof(abi.SimDesc)
    assert abi.T_RIGID_BODY_STATE == abi.T_COUNT - 1            # no new tensor kind


def test_gae_constants_mirror_the_header():
    hdr = {k: int(v, 0) for k, v in re.findall(r"^#define (MQE_GAE_[A-Z_]+) (\w+)", _header_code(), re.M)}
    assert hdr == dict(MQE_GAE_NORMALIZE=abi.GAE_NORMALIZE) and abi.GAE_NORMALIZE == 1


def test_rollout_keeps_its_five_positional_arguments():
    import torch
    r = Rollout(torch.zeros(3, 2 * 2 * 4 + 2 * 2 + 1), torch.zeros(2, 2, 2, 3), None, None, (2, 2, 4))
    assert r.T == 2 and r.time_outs is None and r.advantages is None and r.returns is None and r.adv_stats is None
    rec = torch.tensor([[1, 0], [0, 1]], dtype=torch.uint8)
    r = Rollout(r.packed, r.actions, None, None, (2, 2, 4), time_outs=rec)
    assert r.time_outs.dtype == torch.bool and r.time_outs.data_ptr() == rec.data_ptr() and r.time_outs.tolist() == [[True, False], [False, True]]


# ---- the float64 reference on cases worked by hand ---------------------------------------------------------------------------------
def test_reference_on_a_hand_computed_case():
    """T = 3, one env, two agents that share done / time-out: t = 1 is a time-out, nothing else done; gamma = 0.5, lam = 0.5.
    agent 0: r = (1, 2, 3), v = (1, 2, 3, 4):
      t = 2: delta = 3 + 0.5 * 4 - 3 = 2, adv = 2, ret = 5
      t = 1: done, time-out: rr = 2 + 0.5 * 2 = 3, delta = 3 - 2 = 1, adv = 1, ret = 3
      t = 0: delta = 1 + 0.5 * 2 - 1 = 1, adv = 1 + 0.25 * 1 = 1.25, ret = 2.25
    agent 1: r = (0, -1, 1), v = (2, -2, 0, 8):
      t = 2: delta = 1 + 4 - 0 = 5, adv = 5, ret = 5
      t = 1: rr = -1 + 0.5 * (-2) = -2, delta = -2 + 2 = 0, adv = 0, ret = -2
      t = 0: delta = 0 + 0.5 * (-2) - 2 = -3, adv = -3 + 0.25 * 0 = -3, ret = -1
    Without the time-out record t = 1 is a failure: agent 0 delta = 2 - 2 = 0 -> adv = (1, 0, 2); agent 1 delta = -1 + 2 = 1 -> adv = (-2.75, 1, 5)."""
    reward = np.array([[[1, 0]], [[2, -1]], [[3, 1]]], np.float32)
    value = np.array([[[1, 2]], [[2, -2]], [[3, 0]], [[4, 8]]], np.float32)
    done = np.array([[0], [1], [0]], np.uint8)
    to = np.array([[1], [1], [0]], np.uint8)          # the byte at t = 0 is a stray one: not done, ignored
    for dtype in (np.float64, np.float32):
        adv, ret = ref.gae(reward, value, done, to, 0.5, 0.5, dtype)
        assert adv.dtype == dtype
        assert adv[:, 0].tolist() == [[1.25, -3.0], [1.0, 0.0], [2.0, 5.0]]
        assert ret[:, 0].tolist() == [[2.25, -1.0], [3.0, -2.0], [5.0, 5.0]]
        adv, _ = ref.gae(reward, value, done, None, 0.5, 0.5, dtype)
        assert adv[:, 0].tolist() == [[1.0, -2.75], [0.0, 1.0], [2.0, 5.0]]
        assert np.array_equal(ref.gae(reward, value, done, to, 0.5, 0.5, dtype, variant="timeout_is_failure")[0], adv)


@pytest.mark.parametrize("shape", ref.SHAPES, ids=str)
@pytest.mark.parametrize("gamma", [0.99, 1.0, 0.0])
def test_reference_against_the_closed_form_for_lambda_one(shape, gamma):
    """lam = 1: ret[t] = sum_{k = t .. e} gamma^(k - t) r[k] + the bootstrap, e = the next done at or after t (or T - 1): gamma^(e - t + 1)
    value[e + 1] when the window ends undone, gamma^(e - t + 1) value[e] when step e timed out, nothing when it failed"""
    N, Aw, T = shape
    s = ref.synth(N, Aw, T, 16, seed=11)
    _, ret = ref.gae(s["reward"], s["value"], s["done"], s["time_outs"], gamma, 1.0)
    r, v = s["reward"].astype(np.float64), s["value"].astype(np.float64)
    want = np.zeros_like(ret)
    for n in range(N):
        for t in range(T):
            e = t
            while e < T - 1 and not s["done"][e, n]:
                e += 1
            acc = sum(gamma ** (k - t) * r[k, n] for k in range(t, e + 1))
            if not s["done"][e, n]:
                acc = acc + gamma ** (e - t + 1) * v[e + 1, n]
            elif s["time_outs"][e, n]:
                acc = acc + gamma ** (e - t + 1) * v[e, n]
            want[t, n] = acc
    assert np.abs(ret - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


# ---- the synthetic trajectory ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ref.SHAPES, ids=str)
def test_generator_guarantees(shape):
    N, Aw, T = shape
    D = 16
    s = ref.synth(N, Aw, T, D, seed=5)
    done, to = s["done"], s["time_outs"]
    assert done[0, 0] == 1 and to[0, 0] == 1, "env 0: done (a time-out) at t = 0"
    if T >= 2:
        assert done[T - 1, 0] == 1 and to[T - 1, 0] == 0, "env 0: done (a failure) at t = T - 1"
    if N >= 2:
        assert not done[:, N - 1].any(), "the last env is never done"
    undone = done == 0
    assert bool((to[undone] != 0).any()) == bool(undone.any()), "stray time-out bytes wherever a step that is not done exists"
    assert undone.any() or (N, T) == (1, 1)
    assert set(np.unique(done)) <= {0, 1} and set(np.unique(to)) <= {0, 1}
    assert np.abs(s["reward"]).max() <= 1 and s["value"].shape == (T + 1, N, Aw)
    # the flat image: reward and done bytes where mqe_rollout puts them, the sentinel everywhere else
    R, nobs, pf, stride = s["R"], s["nobs"], s["pf"], s["stride"]
    assert stride % 4 == 0 and stride >= pf + 8 and nobs == N * Aw * D
    rows = s["packed"][:(T + 1) * stride].reshape(T + 1, stride)
    assert np.array_equal(rows[1:, nobs:nobs + R].view(np.float32), s["reward"].reshape(T, R))
    assert np.array_equal(rows[1:, nobs + R:pf].copy().view(np.uint8).reshape(T, -1)[:, :N], done)
    assert (rows[0] == ref.SENT).all() and (rows[:, :nobs] == ref.SENT).all() and (rows[:, pf:] == ref.SENT).all()
    assert (s["packed"][(T + 1) * stride:] == ref.SENT).all() and len(s["packed"]) == (T + 1) * stride + s["guard"]
    again = ref.synth(N, Aw, T, D, seed=5)
    assert all(np.array_equal(s[k], again[k]) for k in ("reward", "value", "done", "time_outs", "packed"))


# ---- the derived tolerances ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,gl,with_to", CASES, ids=IDS)
def test_float32_evaluation_is_inside_the_bounds_and_wrong_variants_are_far_outside(shape, gl, with_to):
    """The bounds the GPU test holds k_gae to (gae_ref.tolerances states the derivation: four roundings per step of at most 2^-24 B each,
    carried back with (gamma lam)^k) must hold for a plain float32 evaluation of the recursion -- no kernel involved -- and must not be so wide
    that a wrong recursion passes: gamma * value[t + 1] not masked at a done, and (with the record) a time-out treated as a failure, leave
    them by more than 100x.  gamma = 0 is the one exception, stated rather than skipped: every bootstrap term is multiplied by 0 and the wrong
    variants ARE the right recursion, which the test asserts."""
    N, Aw, T = shape
    gamma, lam = gl
    s = ref.synth(N, Aw, T, 16, seed=1000 + 7 * N + T)
    to = s["time_outs"] if with_to else None
    adv64, ret64 = ref.gae(s["reward"], s["value"], s["done"], to, gamma, lam)
    tol_adv, tol_ret = ref.tolerances(s["reward"], s["value"], adv64, gamma, lam)
    adv32, ret32 = ref.gae(s["reward"], s["value"], s["done"], to, gamma, lam, np.float32)
    dev_adv, dev_ret = float(np.abs(adv32 - adv64).max()), float(np.abs(ret32 - ret64).max())
    print(f"gae_f32 {shape} gamma {gamma} lam {lam} to {int(with_to)}: adv {dev_adv:.3e} (tol {tol_adv:.3e}) ret {dev_ret:.3e} (tol {tol_ret:.3e})")
    assert dev_adv <= tol_adv and dev_ret <= tol_ret
    for variant in ("vn_unmasked",) + (("timeout_is_failure",) if with_to else ()):
        bad, bad_ret = ref.gae(s["reward"], s["value"], s["done"], to, gamma, lam, np.float32, variant=variant)
        if gamma == 0.0:
            assert np.array_equal(bad, adv32) and np.array_equal(bad_ret, ret32)
            continue
        off, off_ret = float(np.abs(bad - adv64).max()), float(np.abs(bad_ret - ret64).max())
        print(f"    {variant}: adv off by {off:.3e} = {off / tol_adv:.0f} x tol, ret {off_ret / tol_ret:.0f} x tol")
        assert off > 100 * tol_adv and off_ret > 100 * tol_ret, variant


# ---- kernel resources ------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not (os.path.isfile(LIB_PATH) and all(os.path.isfile(os.path.join(LLVM, t)) for t in TOOLS)),
                    reason="needs the built HIP engine and the ROCm LLVM tools")
def test_gae_kernels_use_no_scratch(tmp_path):
    fat, co = str(tmp_path / "fat.bin"), str(tmp_path / "dev.co")
    subprocess.check_call([f"{LLVM}/llvm-objcopy", "--dump-section", f".hip_fatbin={fat}", LIB_PATH, str(tmp_path / "stripped.so")])
    subprocess.check_call([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"])
    notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True, check=True).stdout
    mine = []
    for blk in notes.split("- .agpr_count:")[1:]:
        f = dict(re.findall(r"\.(\w+):\s*(\S+)", ".agpr_count:" + blk))
        if re.match(r"_Z\d+k_gae", f.get("name", "")):
            mine.append(f)
    names = sorted(f["name"] for f in mine)
    assert len(names) == 3 and sum("k_gae_normalize" in n for n in names) == 1, names       # k_gae with and without the record, k_gae_normalize
    for f in mine:
        print(f["name"], "vgpr", f["vgpr_count"], "sgpr", f["sgpr_count"], "spills", f["vgpr_spill_count"], f["sgpr_spill_count"], "scratch", f["private_segment_fixed_size"])
        assert int(f["private_segment_fixed_size"]) == 0 and int(f["vgpr_spill_count"]) == 0 and int(f["sgpr_spill_count"]) == 0, f
        assert int(f.get("group_segment_fixed_size", 0)) == 0, "no LDS"


# ---- the oracle-backed env ---------------------------------------------------------------------------------------------------------------
def test_oracle_backed_env_refuses_by_name(gate_wrapper):  # noqa: F811
    w = gate_wrapper
    with pytest.raises(NotImplementedError, match="HipEngine"):
        w.rollout(4, gamma=0.99)
    with pytest.raises(NotImplementedError, match="HipEngine"):
        w.rollout(4, gamma=0.99, lam=0.9, normalize_advantages=True)
    with pytest.raises(NotImplementedError, match="HipEngine"):
        w.rollout(4)
