"""The on-device PPO update on a CPU-only host (mqe_ppo_grad, mqe_ppo_optimizer, mqe_ppo_adam; HipEngine.ppo_grad / adam_step / ppo_update,
FusedTaskWrapper.ppo_update / pull_actor): the exports exist without an ABI bump, the float64 reference of the GPU test equals torch autograd
of the stated loss, the synthetic trajectory is kink-free and hits every branch, the measured constant K holds two float32 evaluations and
rejects wrong gradients, the Adam reference is torch's and its derived bound holds a float32 evaluation, the kernels use no scratch, an
oracle-backed env refuses."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import ppo_ref as ref
from mqe.engine import abi
from mqe.engine.hip_engine import LIB_PATH
from test_rollout import HEADER, LLVM, TOOLS, _header_code, gate_wrapper  # noqa: F401  (the oracle-backed go1gate wrapper fixture)

CFG = dict(clip=ref.CLIP, value_coef=1.0, entropy_coef=0.01, value_clip=ref.VALUE_CLIP)
_SYNTH = {}


def synth(net, M, seed):
    if (net, M, seed) not in _SYNTH:
        _SYNTH[(net, M, seed)] = ref.synth(net, ref.shape_for(M), M, seed)
    return _SYNTH[(net, M, seed)]


def case(net, M, seed, cfg=CFG):
    s = synth(net, M, seed)
    b = ref.batch(s, s["index"][:M])
    return s, b, (s["params"], s["a_dims"], s["c_dims"], s["act"], b, cfg)


# ---- exports and header ----------------------------------------------------------------------------------------------------------------
def test_exports_declared_and_exported_without_an_abi_bump():
    code = re.sub(r"\s+", " ", _header_code())
    assert "typedef struct { float clip_ratio, value_coef, entropy_coef, value_clip; } mqe_ppo_loss;" in code
    assert ("int mqe_ppo_grad(mqe_sim* s, int T, const float* packed_dev, long long row_stride, const float* actions_dev, const float* logp_dev, "
            "const float* value_dev, const float* adv_dev, const float* ret_dev, const int32_t* index_dev, long long first, long long count, "
            "const mqe_ppo_loss* loss, int flags, float* grad_dev, float* stats_dev, void* stream);") in code
    assert "int mqe_ppo_optimizer(mqe_sim* s, mqe_tensor_view* m_out, mqe_tensor_view* v_out);" in code
    assert ("int mqe_ppo_adam(mqe_sim* s, const float* grad_dev, long long step, float lr, float beta1, float beta2, float eps, "
            "float max_grad_norm, float* norm_dev, void* stream);") in code
    assert re.search(r"#define MQE_ABI_VERSION 17\b", code)
    lib = C.CDLL(LIB_PATH)
    for name in ("mqe_ppo_grad", "mqe_ppo_optimizer", "mqe_ppo_adam"):
        assert hasattr(lib, name), name
    assert lib.mqe_abi_version() == abi.ABI_VERSION == 17
    assert lib.mqe_sizeof_desc() == C.sizeof(abi.SimDesc)
    assert abi.T_RIGID_BODY_STATE == abi.T_COUNT - 1            # no new tensor kind


def test_ppo_constants_and_struct_mirror_the_header():
    hdr = {k: int(v, 0) for k, v in re.findall(r"^#define (MQE_PPO_[A-Z_]+) (\w+)", _header_code(), re.M)}
    assert hdr == dict(MQE_PPO_CLIP_VALUE=abi.PPO_CLIP_VALUE, MQE_PPO_STATS=abi.PPO_STATS) and (abi.PPO_CLIP_VALUE, abi.PPO_STATS) == (1, 6)
    assert [f[0] for f in abi.PpoLoss._fields_] == ["clip_ratio", "value_coef", "entropy_coef", "value_clip"]
    assert C.sizeof(abi.PpoLoss) == 16 and all(f[1] is C.c_float for f in abi.PpoLoss._fields_)


# ---- the float64 reference -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vclip", [ref.VALUE_CLIP, None], ids=["vclip", "plain"])
@pytest.mark.parametrize("net", ["tanh64x64", "relu17x5", "relu128x3", "tanh7"])
def test_manual_float64_backward_is_autograd_of_the_stated_loss(net, vclip):
    cfg = dict(CFG, value_clip=vclip, entropy_coef=0.03, value_coef=0.7)
    _, _, args = case(net, 130, 1, cfg)
    g, st, S, _ = ref.manual(*args)
    ga, sta = ref.autograd(*args, torch.float64)
    for name in g:
        scale = max(float(ga[name].abs().max()), 1e-300)
        assert float((g[name] - ga[name]).abs().max()) <= 1e-12 * scale, name
        assert S[name] >= float(g[name].abs().max()) * (1 - 1e-12), name
    assert float((st - sta).abs().max()) <= 1e-12 * float(sta.abs().max())
    gt, stt, _, _ = ref.manual(*args, tile=64)            # the tiled accumulation is the same sum
    assert all(float((gt[n] - g[n]).abs().max()) <= 1e-12 * max(float(g[n].abs().max()), 1e-300) for n in g)


# ---- the synthetic trajectory ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net,M", [("tanh64x64", 63), ("relu128x3", 130), ("relu17x5", 1000), ("tanh7", 1)])
def test_generator_guarantees(net, M):
    s, b, args = case(net, M, 2)
    N, Aw, T, D = s["shape"]
    full = ref.batch(s, slice(None))
    assert not bool(ref.kinks(s["params"], s["a_dims"], s["c_dims"], s["act"], full, CFG).any()), "every row is outside the kink margins"
    p64 = {k: v.double() for k, v in s["params"].items()}
    mean = ref.forward(p64, "actor", s["a_dims"], s["act"], b["obs"].double())[0]
    v = ref.forward(p64, "critic", s["c_dims"], s["act"], b["obs"].double())[0][:, 0]
    z = (b["actions"].double() - mean) * torch.exp(-p64["log_std"])
    ratio = torch.exp((-0.5 * z * z - p64["log_std"]).sum(-1) - 1.5 * ref.LN2PI - b["logp_old"].double())
    adv, vo, ret = b["adv"].double(), b["v_old"].double(), b["ret"].double()
    assert float((ratio - 1.2).abs().min()) >= 1e-3 and float((ratio - 0.8).abs().min()) >= 1e-3 and float(adv.abs().min()) >= 1e-3
    assert float(((v - vo).abs() - ref.VALUE_CLIP).abs().min()) >= 1e-3
    if M >= 63:
        gate = ((adv > 0) & (ratio > 1.2)) | ((adv < 0) & (ratio < 0.8))
        assert bool(gate.any()) and bool((~gate).any()), "both gate states"
        clipped = (ratio - 1).abs() > ref.CLIP
        assert 0 < int(clipped.sum()) < M, "clip fraction strictly between 0 and 1"
        sat = (v - vo).abs() > ref.VALUE_CLIP
        v_c = vo + torch.clamp(v - vo, -ref.VALUE_CLIP, ref.VALUE_CLIP)
        unclipped_larger = (v - ret) ** 2 >= (v_c - ret) ** 2
        assert bool(sat.any()) and bool((~sat).any()), "the clamp both saturated and not"
        assert bool((sat & unclipped_larger).any()) and bool((sat & ~unclipped_larger).any()), "both value branches under a saturated clamp"
    # the image: observations of rows 0 .. T in place, the sentinel everywhere else
    R, nobs, pf, stride = s["R"], s["nobs"], s["pf"], s["stride"]
    assert stride % 4 == 0 and stride >= pf + 8 and nobs == N * Aw * D and s["n"] == T * R >= M
    rows = s["packed"][:(T + 1) * stride].reshape(T + 1, stride)
    assert np.array_equal(rows[:T, :nobs].view(np.float32).reshape(T * R, D), s["obs"].numpy())
    assert (rows[:, nobs:] == ref.SENT).all() and (s["packed"][(T + 1) * stride:] == ref.SENT).all()
    assert len(s["packed"]) == (T + 1) * stride + s["guard"]
    assert np.array_equal(s["value"][:T * R].view(np.float32), s["v_old"].numpy()) and len(s["value"]) == (T + 1) * R
    assert (s["grad"] == ref.SENT).all() and len(s["grad"]) == s["n_params"] + s["guard"] and len(s["stats"]) == 6 + s["guard"]
    assert sorted(s["index"].tolist()) == list(range(s["n"])) and s["index"].dtype == torch.int32
    again = ref.synth(net, s["shape"], M, 2)
    assert all(torch.equal(s[k], again[k]) for k in ("obs", "actions", "logp_old", "v_old", "adv", "ret", "index")) and np.array_equal(s["packed"], again["packed"])


# ---- K -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net,M,seed", ref.K_CASES, ids=[f"{n}-M{m}-s{s}" for n, m, s in ref.K_CASES])
def test_two_float32_evaluations_are_inside_k(net, M, seed):
    """torch float32 autograd on the whole batch and the float32 manual backward accumulated over 64-row tiles, against the float64 backward:
    every tensor inside K_CPU 2^-24 S_n, every statistic inside K_CPU 2^-24 of its scale (ppo_ref's docstring holds the measured table)"""
    _, _, args = case(net, M, seed)
    g64, st64, S, ss = ref.manual(*args)
    ga, sta = ref.autograd(*args, torch.float32)
    gm, stm, _, _ = ref.manual(*args, torch.float32, tile=64)
    ra, na = ref.ratio_to_bound(ga, g64, S)
    rm, nm = ref.ratio_to_bound(gm, g64, S)
    sa, sm = ref.stats_ratio(sta, st64, ss), ref.stats_ratio(stm, st64, ss)
    print(f"ppo_k {net} M={M} seed={seed}: autograd {ra:.2f} ({na}) tiled {rm:.2f} ({nm}) stats {sa:.2f} {sm:.2f}")
    assert max(ra, rm, sa, sm) <= ref.K_CPU


@pytest.mark.parametrize("net", ["tanh64x64", "relu128x3", "relu17x5"])
def test_wrong_gradients_are_far_outside(net):
    M = 1000
    _, _, args = case(net, M, 0)
    g64, _, S, _ = ref.manual(*args)
    for variant in ("gate_ignored", "no_inv_m", "entropy_sign", "value_clip_ignored", "z_no_inv"):
        bad, _, _, _ = ref.manual(*args, torch.float32, tile=64, variant=variant)
        r, at = ref.ratio_to_bound(bad, g64, S)
        print(f"ppo_wrong {net} {variant}: {r:.3g} x 2^-24 S at {at} = {r / ref.K_GPU:.0f} x the GPU bound")
        assert r > 100 * ref.K_GPU, variant


# ---- Adam ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_norm", [None, 0.5], ids=["noclip", "clip"])
def test_adam_reference_is_torch_adam_behind_clip_grad_norm(max_norm):
    gen = torch.Generator().manual_seed(3)
    p0 = torch.randn(257, generator=gen, dtype=torch.float64)
    grads = [torch.randn(257, generator=gen, dtype=torch.float64) * (0.1 + k) for k in range(5)]
    par = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([par], lr=3e-3, betas=(0.9, 0.999), eps=1e-8)
    p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    for k, g in enumerate(grads):
        par.grad = g.clone()
        if max_norm is not None:
            total = torch.nn.utils.clip_grad_norm_([par], max_norm)
        opt.step()
        p, m, v, norm = ref.adam(p, m, v, g, k + 1, 3e-3, max_norm=max_norm, f32_args=False)
        if max_norm is not None:
            assert abs(norm - float(total)) <= 1e-12 * norm
        assert float((p - par.detach()).abs().max()) <= 1e-12 * float(p.abs().max())
    st = opt.state[par]
    assert float((m - st["exp_avg"]).abs().max()) <= 1e-12 * float(m.abs().max())
    assert float((v - st["exp_avg_sq"]).abs().max()) <= 1e-12 * float(v.abs().max())


@pytest.mark.parametrize("step", [1, 7, 1000])
@pytest.mark.parametrize("max_norm", [None, 0.5], ids=["noclip", "clip"])
def test_float32_adam_meets_the_derived_bound(max_norm, step):
    gen = torch.Generator().manual_seed(10 + step)
    n = 4099
    p, g = torch.randn(n, generator=gen), torch.randn(n, generator=gen) * 0.3
    m, v = torch.randn(n, generator=gen) * 0.1, torch.rand(n, generator=gen) * 0.05
    v[:7] = 0.0                                                 # denominators down at eps
    g[:3] = 0.0
    p64, m64, v64, _ = ref.adam(p, m, v, g, step, 1e-3, max_norm=max_norm)
    p32, m32, v32, _ = ref.adam(p, m, v, g, step, 1e-3, max_norm=max_norm, dtype=torch.float32)
    tol_p, tol_m, tol_v = ref.adam_tolerances(p, m, v, g, step, 1e-3, max_norm=max_norm)
    for name, a, b64, tol in (("p", p32, p64, tol_p), ("m", m32, m64, tol_m), ("v", v32, v64, tol_v)):
        worst = float(((a.double() - b64).abs() / tol).max())
        print(f"ppo_adam_f32 step={step} clip={max_norm} {name}: {worst:.3f} of the bound")
        assert worst <= 1.0, name
    wrong = ref.adam(p, m, v, g, step + 1 if step < 1000 else 1, 1e-3, max_norm=max_norm, dtype=torch.float32)[0]      # another bias correction
    assert float(((wrong.double() - p64).abs() / tol_p).max()) > 100


# ---- kernel resources ------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not (os.path.isfile(LIB_PATH) and all(os.path.isfile(os.path.join(LLVM, t)) for t in TOOLS)),
                    reason="needs the built HIP engine and the ROCm LLVM tools")
def test_ppo_kernels_use_no_scratch(tmp_path):
    fat, co = str(tmp_path / "fat.bin"), str(tmp_path / "dev.co")
    subprocess.check_call([f"{LLVM}/llvm-objcopy", "--dump-section", f".hip_fatbin={fat}", LIB_PATH, str(tmp_path / "stripped.so")])
    subprocess.check_call([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"])
    notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True, check=True).stdout
    mine = []
    for blk in notes.split("- .agpr_count:")[1:]:
        f = dict(re.findall(r"\.(\w+):\s*(\S+)", ".agpr_count:" + blk))
        if re.match(r"_Z\d+k_ppo_", f.get("name", "")):
            mine.append(f)
    names = sorted(f["name"] for f in mine)
    assert len(names) == 5 and sum("k_ppo_grad" in n for n in names) == 2, names      # k_ppo_grad at 64 and 32 rows, k_ppo_reduce, k_ppo_norm, k_ppo_adam
    for f in mine:
        print(f["name"], "vgpr", f["vgpr_count"], "sgpr", f["sgpr_count"], "spills", f["vgpr_spill_count"], f["sgpr_spill_count"], "scratch",
              f["private_segment_fixed_size"], "static lds", f.get("group_segment_fixed_size", 0))
        assert int(f["private_segment_fixed_size"]) == 0 and int(f["vgpr_spill_count"]) == 0, f
        assert int(f.get("group_segment_fixed_size", 0)) <= 160 * 1024
        if "k_ppo_grad" in f["name"]:
            assert int(f["vgpr_count"]) <= 128, "1024 threads per workgroup: 128 registers each"


def test_lds_of_every_accepted_shape_fits():
    """k_ppo_grad's dynamic LDS: (D + the larger network's hidden widths + 4) rows of tile + 1 floats and the tile's 64-bit sample numbers;
    64-row tiles wherever they fit 160 KiB -- two 64 x 64 and 128 x 128 x 128 networks do -- else 32 rows, which holds the widest stack"""
    def lds(D, hidden, rt):
        return ((D + sum(hidden) + 4) * (rt + 1) + 2 + 128) * 4
    assert lds(16, (64, 64), 64) <= 160 * 1024 and lds(abi.ACTOR_MAX_OBS, (128, 128, 128), 64) <= 160 * 1024
    widest = (abi.ACTOR_MAX_HIDDEN,) * (abi.ACTOR_MAX_LAYERS - 1)
    assert lds(16, widest, 64) > 160 * 1024 and lds(abi.ACTOR_MAX_OBS, widest, 32) <= 160 * 1024


# ---- the oracle-backed env ---------------------------------------------------------------------------------------------------------------
def test_oracle_backed_env_refuses_by_name(gate_wrapper):  # noqa: F811
    w = gate_wrapper
    with pytest.raises(NotImplementedError, match="HipEngine"):
        w.ppo_update(None, epochs=1, minibatches=2, lr=1e-3)
    with pytest.raises(NotImplementedError, match="HipEngine"):
        w.pull_actor()
