"""The joint-ratio and dual-clip PPO losses on a CPU-only host (mqe_ppo_grad with MQE_PPO_JOINT / MQE_PPO_DUAL_CLIP; csrc/kernels_ppo.hpp;
tests/joint_ref.py): the constants and the struct in their three statements, the manual backward against float64 autograd of the stated loss, the
reference at A' = 1 and at c_d = 1e30 against ppo_ref.manual bit for bit, the generator's regions, the measured K, wrong gradients far outside the
GPU bound, the recurrent twin likewise, and the new kernel's resources."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import joint_ref as ref
import ppo_ref
from mqe.engine import abi
from mqe.engine.hip_engine import LIB_PATH
from test_rollout import HEADER, LLVM, TOOLS, _header_code

CSRC = os.path.join(os.path.dirname(LIB_PATH), "kernels_ppo.hpp")
_SYNTH = {}


def synth(net, Aw, seed, cd=ref.DUAL):
    """500 groups of A' agents (N = 10, T = 50, D = 16): every minibatch of a case is a slice of its seeded group permutation"""
    key = (net, Aw, seed, cd)
    if key not in _SYNTH:
        _SYNTH[key] = ref.synth(net, (10, Aw, 50, 16), seed, cd)
    return _SYNTH[key]


def case(net, G, Aw, loss, seed, cd=ref.DUAL, **over):
    s = synth(net, Aw, seed, cd)
    cfg = dict(ref.CFG, **ref.LOSSES[loss], **over)
    if cfg["dual_clip"] is not None:
        cfg["dual_clip"] = cd
    return s, (s["params"], s["a_dims"], s["c_dims"], s["act"], ref.batch(s, s["gindex"][:G]), cfg, Aw)


# ---- the three statements of the constants -------------------------------------------------------------------------------------------------------
def test_constants_and_struct_in_header_csrc_and_abi():
    assert (abi.PPO_JOINT, abi.PPO_DUAL_CLIP) == (64, 128)
    comment = " ".join(re.findall(r"/\*.*?\*/", open(HEADER).read(), flags=re.S))
    assert re.search(r"MQE_PPO_JOINT = 64\b", comment) and re.search(r"MQE_PPO_DUAL_CLIP = 128\b", comment)
    src = open(CSRC).read()
    assert re.search(r"^#define MQE_PPO_JOINT 64\b", src, re.M) and re.search(r"^#define MQE_PPO_DUAL_CLIP 128\b", src, re.M)
    code = re.sub(r"\s+", " ", _header_code())
    assert "typedef struct { float clip_ratio, value_coef, entropy_coef, value_clip, dual_clip, reserved[3]; } mqe_ppo_loss_ex;" in code
    assert not re.search(r"#define MQE_PPO_(JOINT|DUAL_CLIP)", code), "stated in the comment, not defined: the header's define set is pinned"
    assert C.sizeof(abi.PpoLossEx) == 32 and C.sizeof(abi.PpoLoss) == 16
    assert abi.PpoLossEx._fields_[:4] == abi.PpoLoss._fields_ and [f[0] for f in abi.PpoLossEx._fields_[4:]] == ["dual_clip", "reserved"]
    assert abi.PpoLossEx.dual_clip.offset == 16 and abi.PpoLossEx.reserved.offset == 20
    assert abi.SIGNATURES["mqe_ppo_grad"][1][12] is C.POINTER(abi.PpoLoss), "the prototype stays"
    assert abi.ABI_VERSION == 17 and re.search(r"#define MQE_ABI_VERSION 17\b", code)


# ---- the float64 reference ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", list(ref.LOSSES))
@pytest.mark.parametrize("net,Aw", [("tanh64x64", 2), ("relu17x5", 4), ("tanh7", 4), ("relu128x3", 2)])
def test_manual_float64_backward_is_autograd_of_the_stated_loss(net, Aw, loss):
    _, args = case(net, 65, Aw, loss, 1, entropy_coef=0.03)
    g, st, S, _ = ref.manual(*args)
    ga, sta = ref.autograd(*args, torch.float64)
    for name in g:
        scale = max(float(ga[name].abs().max()), 1e-300)
        assert float((g[name] - ga[name]).abs().max()) <= 1e-12 * scale, name
        assert S[name] >= float(g[name].abs().max()) * (1 - 1e-12), name
    assert float((st - sta).abs().max()) <= 1e-12 * float(sta.abs().max())
    gt = ref.manual(*args, tile=64)[0]                       # the tiled accumulation is the same sum
    assert all(float((gt[n] - g[n]).abs().max()) <= 1e-12 * max(float(g[n].abs().max()), 1e-300) for n in g)


@pytest.mark.parametrize("net", ["tanh64x64", "relu17x5"])
def test_one_agent_and_an_unreachable_dual_clip_are_ppo_ref_bit_for_bit(net):
    """at A' = 1 the joint loss, and at c_d = 1e30 the dual clip, are the plain loss: the float64 reference has ppo_ref.manual's bits"""
    s = ppo_ref.synth(net, (7, 1, 19, 16), 133, 5)
    b = ppo_ref.batch(s, s["index"][:130])
    cfg = dict(clip=ref.CLIP, value_coef=0.7, entropy_coef=0.01, value_clip=ref.VALUE_CLIP)
    want = ppo_ref.manual(s["params"], s["a_dims"], s["c_dims"], s["act"], b, cfg)
    for Aw, extra in ((1, dict(joint=True, dual_clip=None)), (1, dict(joint=True, dual_clip=1e30)), (2, dict(joint=False, dual_clip=1e30))):
        got = ref.manual(s["params"], s["a_dims"], s["c_dims"], s["act"], b, dict(cfg, **extra), Aw)
        assert all(torch.equal(got[0][n], want[0][n]) for n in want[0]), extra
        assert torch.equal(got[1], want[1]) and got[2] == want[2] and torch.equal(got[3], want[3]), extra


# ---- the generator --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net,Aw,cd", [("tanh64x64", 2, 1.5), ("relu17x5", 4, 1.5), ("tanh7", 2, 3.0), ("relu128x3", 4, 1.5)])
def test_every_region_holds_five_percent_and_no_group_is_near_a_kink(net, Aw, cd):
    s = synth(net, Aw, 0, cd)
    shares = ref.shares_of(s)
    print(f"joint_regions {net} A'={Aw} c_d={cd}: " + ", ".join(f"{n} {100 * x:.1f} %" for n, x in zip(ref.REGIONS, shares)) + f"; {s['group_redraws']} groups drawn again")
    assert min(shares) >= 0.05, shares
    d = (ref.logp64_of(s) - s["logp_old"].double()).reshape(-1, Aw)
    assert not bool(ref.group_kinks(d, s["adv"].double().reshape(-1, Aw), Aw, cd).any())
    assert s["n_groups"] == 500 and sorted(s["gindex"].tolist()) == list(range(500)) and s["gindex"].dtype == torch.int32
    full = ppo_ref.batch(s, slice(None))                     # the value head and the relus stay kink-free as ppo_ref.synth left them
    bad = ppo_ref.kinks(s["params"], s["a_dims"], s["c_dims"], s["act"], dict(full, logp_old=full["logp_old"] * 0 + 50.0, adv=full["adv"] * 0 + 1.0),
                        dict(clip=ref.CLIP, value_clip=ref.VALUE_CLIP))
    assert not bool(bad.any())
    if cd == 1.5:                                            # without the joint ratio the samples' own ratios reach every branch too
        r, a = torch.exp(d).reshape(-1), s["adv"].double()
        for m in ((a < 0) & (r > cd), (a < 0) & (r < 0.8), (a > 0) & (r > 1.2), (r - 1).abs() < 0.2, (a < 0) & (r > 1.2) & (r < cd)):
            assert float(m.double().mean()) >= 0.02
    again = ref.synth(net, (10, Aw, 50, 16), 0, cd)
    assert all(torch.equal(s[k], again[k]) for k in ("logp_old", "adv", "gindex", "region"))


# ---- K --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net,G,Aw,loss,seed", ref.K_CASES, ids=[f"{n}-G{g}-A{a}-{l}-s{s}" for n, g, a, l, s in ref.K_CASES])
def test_two_float32_evaluations_are_inside_k(net, G, Aw, loss, seed):
    _, args = case(net, G, Aw, loss, seed)
    g64, st64, S, ss = ref.manual(*args)
    ra, na, sa, threads = 0.0, None, 0.0, torch.get_num_threads()
    try:
        for nt in sorted({1, threads}):                      # torch's float32 sums depend on how many threads share them: both orders count
            torch.set_num_threads(nt)
            ga, sta = ref.autograd(*args, torch.float32)
            ra, na = max((ra, na), ref.ratio_to_bound(ga, g64, S), key=lambda x: x[0])
            sa = max(sa, ref.stats_ratio(sta, st64, ss))
    finally:
        torch.set_num_threads(threads)
    gm, stm, _, _ = ref.manual(*args, torch.float32, tile=64)
    rm, nm = ref.ratio_to_bound(gm, g64, S)
    sm = ref.stats_ratio(stm, st64, ss)
    print(f"joint_k {net} G={G} A'={Aw} {loss} seed={seed}: autograd {ra:.2f} ({na}) tiled {rm:.2f} ({nm}) stats {sa:.2f} {sm:.2f}")
    assert max(ra, rm, sa, sm) <= ref.K["mlp"]


@pytest.mark.parametrize("net,G,Aw,loss,seed", ref.K_CASES_LN, ids=[f"{n}-G{g}-A{a}-{l}-s{s}" for n, g, a, l, s in ref.K_CASES_LN])
def test_two_float32_evaluations_with_the_norms_are_inside_k(net, G, Aw, loss, seed):
    """the same with a LayerNorm on the observation and behind every hidden activation (k_ln_grad's networks): its own table entry"""
    key = (net, Aw, seed, "ln")
    if key not in _SYNTH:
        _SYNTH[key] = ref.synth(net, (10, Aw, 50, 16), seed, hidden=True, feat=True)
    s = _SYNTH[key]
    args = (s["params"], s["a_dims"], s["c_dims"], s["act"], ref.batch(s, s["gindex"][:G]), dict(ref.CFG, **ref.LOSSES[loss]), Aw)
    norms = dict(hidden=True, feat=True)
    g64, st64, S, ss = ref.manual(*args, **norms)
    ga, sta = ref.autograd(*args, torch.float32, **norms)
    gm, stm, _, _ = ref.manual(*args, torch.float32, tile=64, **norms)
    ra, na = ref.ratio_to_bound(ga, g64, S)
    rm, nm = ref.ratio_to_bound(gm, g64, S)
    sa, sm = ref.stats_ratio(sta, st64, ss), ref.stats_ratio(stm, st64, ss)
    print(f"joint_k_ln {net} G={G} A'={Aw} {loss} seed={seed}: autograd {ra:.2f} ({na}) tiled {rm:.2f} ({nm}) stats {sa:.2f} {sm:.2f}")
    assert max(ra, rm, sa, sm) <= ref.K["ln"]


@pytest.mark.parametrize("Aw", [2, 4])
@pytest.mark.parametrize("net", ["tanh64x64", "relu128x3", "relu17x5"])
def test_wrong_gradients_are_outside_the_gpu_bound(net, Aw):
    _, args = case(net, 500, Aw, "joint+dual", 0)
    g64, _, S, _ = ref.manual(*args)
    for variant in ref.WRONG:
        bad = ref.manual(*args, torch.float32, tile=64, variant=variant)[0]
        r, at = ref.ratio_to_bound(bad, g64, S)
        print(f"joint_wrong {net} A'={Aw} {variant}: {r:.3g} x 2^-24 S at {at} = {r / ref.K_GPU['mlp']:.0f} x the GPU bound")
        assert r > 100 * ref.K_GPU["mlp"], variant


# ---- the recurrent twin ---------------------------------------------------------------------------------------------------------------------------
_BPTT = {}


def bptt_synth(name):
    if name not in _BPTT:
        _BPTT[name] = ref.bptt_synth(name, 5, 8, 4)
    return _BPTT[name]


@pytest.mark.parametrize("name,count,loss", ref.K_CASES_BPTT, ids=[f"{n}-{c}-{l}" for n, c, l in ref.K_CASES_BPTT])
def test_recurrent_twin_manual_is_autograd_and_float32_is_inside_k(name, count, loss):
    s = bptt_synth(name)
    cfg = dict(ref.CFG, **ref.LOSSES[loss])
    groups = s["gindex"][:count].numpy()
    g64, st64, S = ref.bptt_manual(s, groups, 4, cfg)
    ga, sta = ref.bptt_autograd(s, groups, 4, cfg)
    for n in g64:
        assert float(np.abs(g64[n] - ga[n].numpy()).max()) <= 1e-11 * max(float(ga[n].abs().max()), 1e-300), n
    assert float(np.abs(st64 - sta.numpy()).max()) <= 1e-12 * float(np.abs(st64).max())
    ra, na, threads = 0.0, None, torch.get_num_threads()
    try:
        for nt in sorted({1, threads}):
            torch.set_num_threads(nt)
            g32a = ref.bptt_autograd(s, groups, 4, cfg, torch.float32)[0]
            ra, na = max((ra, na), ref.bptt_ref.ratio_to_bound({k: v.numpy() for k, v in g32a.items()}, g64, S), key=lambda x: x[0])
    finally:
        torch.set_num_threads(threads)
    g32m = ref.bptt_manual(s, groups, 4, cfg, np.float32, tile=64)[0]
    rm, nm = ref.bptt_ref.ratio_to_bound(g32m, g64, S)
    print(f"joint_k_bptt {name} groups={count} {loss}: autograd {ra:.2f} ({na}) tiled {rm:.2f} ({nm})")
    assert max(ra, rm) <= ref.K["bptt"]
    if count == 10 and loss == "joint+dual":
        for variant in ref.WRONG:
            r, at = ref.bptt_ref.ratio_to_bound(ref.bptt_manual(s, groups, 4, dict(ref.CFG, **ref.LOSSES["joint+dual"]), np.float32, variant=variant)[0],
                                                *ref.bptt_manual(s, groups, 4, dict(ref.CFG, **ref.LOSSES["joint+dual"]))[::2])
            print(f"joint_wrong_bptt {name} {variant}: {r:.3g} x 2^-24 S at {at} = {r / ref.K_GPU['bptt']:.1f} x the GPU bound")
            assert r > ref.K_GPU["bptt"], variant


def test_recurrent_generator_regions():
    s = bptt_synth("tanh64x64_both")
    d = (s["logp64"] - s["logp_old"].double()).reshape(-1, 2)
    shares = ref.region_shares(d, s["adv"].double().reshape(-1, 2), 2, s["cd"])
    print("joint_regions_bptt: " + ", ".join(f"{n} {100 * x:.1f} %" for n, x in zip(ref.REGIONS, shares)))
    assert min(shares) >= 0.05 and not bool(ref.group_kinks(d, s["adv"].double().reshape(-1, 2), 2, s["cd"]).any())
    assert s["n_groups"] == 10 and sorted(s["gindex"].tolist()) == list(range(10))


# ---- kernel resources -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not (os.path.isfile(LIB_PATH) and all(os.path.isfile(os.path.join(LLVM, t)) for t in TOOLS)),
                    reason="needs the built HIP engine and the ROCm LLVM tools")
def test_expand_kernel_uses_no_scratch(tmp_path):
    fat, co = str(tmp_path / "fat.bin"), str(tmp_path / "dev.co")
    subprocess.check_call([f"{LLVM}/llvm-objcopy", "--dump-section", f".hip_fatbin={fat}", LIB_PATH, str(tmp_path / "stripped.so")])
    subprocess.check_call([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"])
    notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True, check=True).stdout
    mine = [f for f in (dict(re.findall(r"\.(\w+):\s*(\S+)", ".agpr_count:" + blk)) for blk in notes.split("- .agpr_count:")[1:])
            if re.match(r"_Z\d+k_joint_", f.get("name", ""))]
    assert [f["name"] for f in mine] == ["_Z14k_joint_expandPKixxxiPi"], "one kernel, outside the pinned k_ppo_ / k_bptt_ / k_ln_grad / k_actor patterns"
    f = mine[0]
    print(f["name"], "vgpr", f["vgpr_count"], "sgpr", f["sgpr_count"], "spills", f["vgpr_spill_count"], f["sgpr_spill_count"], "scratch", f["private_segment_fixed_size"])
    assert int(f["private_segment_fixed_size"]) == 0 and int(f["vgpr_spill_count"]) == 0 and int(f["sgpr_spill_count"]) == 0
