"""Layer normalisation in the engine's actor-critic on a CPU-only host (MQE_ACTOR_LAYER_NORM, MQE_ACTOR_FEATURE_NORM; csrc/kernels_ln.hpp;
abi.actor_param_layout, mqe.utils.actor_net.mlp_spec, FusedTaskWrapper.set_actor): the layout for the four switch combinations, the constants
stated alike in header, engine and abi.py, what mlp_spec accepts and refuses, the twin of tests/layer_norm_ref.py against torch (norm and
gradient, float64), the measured constant K_LN_CPU holds two float32 evaluations and rejects wrong norms by > 100x, the new kernels' resources,
and the documented LDS rule for every accepted shape."""
import itertools
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import layer_norm_ref as ref
import ppo_ref
from mqe.engine import abi
from mqe.engine.hip_engine import LIB_PATH
from mqe.utils.actor_net import mlp_spec
from test_rollout import HEADER, LLVM, TOOLS, ROOT, _header_code, gate_wrapper  # noqa: F401  (the oracle-backed go1gate wrapper fixture)

KERNELS = os.path.join(ROOT, "multiagent-quadruped-environment_amd", "csrc", "kernels_ln.hpp")
CFG = dict(clip=ref.CLIP, value_coef=1.0, entropy_coef=0.01, value_clip=ref.VALUE_CLIP)
_SYNTH = {}


def case(name, M, seed, **kw):
    key = (name, M, seed, tuple(kw.items()))
    if key not in _SYNTH:
        _SYNTH[key] = ref.synth(name, ppo_ref.shape_for(M), M, seed, **kw)
    s = _SYNTH[key]
    return (s, *ref.args_of(s, s["index"][:M], CFG))


# ---- layout and constants ---------------------------------------------------------------------------------------------------------------------
def test_layout_of_the_four_switch_combinations():
    a, c = [16, 7, 5, 3], [16, 6, 1]

    def plain(dims_a, dims_c):             # the layout before the switches existed, restated
        out, off = {}, 0
        for who, dims in (("actor", dims_a), ("critic", dims_c)):
            for l in range(len(dims) - 1):
                out[f"{who}.{l}.weight"] = (off, (dims[l + 1], dims[l]))
                out[f"{who}.{l}.bias"] = (off + dims[l] * dims[l + 1], (dims[l + 1],))
                off += dims[l] * dims[l + 1] + dims[l + 1]
        out["log_std"] = (off, (3,))
        return out
    off_ = abi.actor_param_layout(a, c, layer_norm=False, feature_norm=False)
    assert off_ == plain(a, c) == abi.actor_param_layout(a, c) and list(off_) == list(plain(a, c))
    assert abi.actor_param_count(a, c, False, False, False) == abi.actor_param_count(a, c) == 16 * 7 + 7 + 7 * 5 + 5 + 5 * 3 + 3 + 16 * 6 + 6 + 6 + 1 + 3
    names = {(False, False): [], (True, False): ["actor.0.norm", "actor.1.norm", "critic.0.norm"], (False, True): ["actor.norm_in", "critic.norm_in"],
             (True, True): ["actor.norm_in", "actor.0.norm", "actor.1.norm", "critic.norm_in", "critic.0.norm"]}
    widths = {"actor.norm_in": 16, "critic.norm_in": 16, "actor.0.norm": 7, "actor.1.norm": 5, "critic.0.norm": 6}
    for (hidden, feat), norms in names.items():
        lay = abi.actor_param_layout(a, c, False, hidden, feat)
        got = [n[:-len(".weight")] for n in lay if "norm" in n and n.endswith(".weight")]
        assert got == norms, (hidden, feat, got)
        # contiguous, in order, nothing overlapping; a norm's bias follows its weight; the Linear shapes are the plain ones
        off = 0
        for name, (o, shape) in lay.items():
            assert o == off, (name, o, off)
            off += int(np.prod(shape))
            if "norm" in name:
                assert shape == (widths[name.rsplit(".", 1)[0]],)
            else:
                assert shape == off_[name][1]
        assert off == abi.actor_param_count(a, c, False, hidden, feat) == abi.actor_param_count(a, c) + 2 * sum(widths[n] for n in norms)
        order = list(lay)
        if feat:
            assert order[:3] == ["actor.norm_in.weight", "actor.norm_in.bias", "actor.0.weight"]
            assert order[order.index("critic.0.weight") - 1] == "critic.norm_in.bias"
        if hidden:
            assert order[order.index("actor.0.bias") + 1:][:3] == ["actor.0.norm.weight", "actor.0.norm.bias", "actor.1.weight"]
            assert "actor.2.norm.weight" not in lay and "critic.1.norm.weight" not in lay, "never behind the output layer"
        vn = abi.actor_param_layout(a, c, True, hidden, feat)
        assert list(vn)[:-1] == list(lay) and vn["value_norm"] == (off, (abi.VALUE_NORM_STATE,))
    single = abi.actor_param_layout([16, 3], [16, 1], False, True, True)
    assert list(single) == ["actor.norm_in.weight", "actor.norm_in.bias", "actor.0.weight", "actor.0.bias", "critic.norm_in.weight", "critic.norm_in.bias",
                            "critic.0.weight", "critic.0.bias", "log_std"]


def test_constants_are_stated_alike_in_header_engine_and_abi():
    header = open(HEADER).read()
    stated = {k: int(v) for k, v in re.findall(r"\b(MQE_ACTOR_(?:LAYER|FEATURE)_NORM) = (\d+)\b", header)}
    defined = {k: int(v) for k, v in re.findall(r"^#define (MQE_[A-Z_]+) (\d+)\b", open(KERNELS).read(), re.M)}
    mirror = dict(MQE_ACTOR_LAYER_NORM=abi.ACTOR_LAYER_NORM, MQE_ACTOR_FEATURE_NORM=abi.ACTOR_FEATURE_NORM)
    assert stated == defined == mirror == dict(MQE_ACTOR_LAYER_NORM=2, MQE_ACTOR_FEATURE_NORM=4)
    assert (abi.ACTOR_LAYER_NORM | abi.ACTOR_FEATURE_NORM) & (abi.ACTOR_TANH | abi.ACTOR_RELU | abi.ACTOR_VALUE_NORM | 512) == 0
    hdr = {k: int(v, 0) for k, v in re.findall(r"^#define (MQE_ACTOR_[A-Z_]+) (\w+)", _header_code(), re.M)}
    assert hdr == dict(MQE_ACTOR_MAX_LAYERS=4, MQE_ACTOR_MAX_HIDDEN=256, MQE_ACTOR_MAX_OBS=128, MQE_ACTOR_TANH=0, MQE_ACTOR_RELU=1), "the header's own set is unchanged"
    assert re.search(r"#define MQE_ABI_VERSION 17\b", header) and abi.ABI_VERSION == 17
    src = open(KERNELS).read()
    assert re.search(r"#define LN_EPS 1e-5f\b", src) and ref.LN_EPS == 1e-5
    actor_src = open(os.path.join(os.path.dirname(KERNELS), "kernels_actor.hpp")).read()
    assert re.search(rf"#define ACT_THREADS {64 * ref.WAVES}\b", actor_src), "the twin splits the features over the kernel's wavefronts"


# ---- mlp_spec --------------------------------------------------------------------------------------------------------------------------------------
def _openrl(out, D=16, h=(64, 64), act=torch.nn.Tanh, feature=True, hidden=True):
    nn = torch.nn
    layers = [nn.LayerNorm(D)] if feature else []
    k = D
    for n in h:
        layers += [nn.Linear(k, n), act()] + ([nn.LayerNorm(n)] if hidden else [])
        k = n
    return nn.Sequential(*layers, nn.Linear(k, out))


def test_mlp_spec_accepts_the_openrl_stack_and_refuses_by_layer_name():
    nn = torch.nn
    m = _openrl(3)
    dims, act, lin, norms = mlp_spec(m, "actor", 16, 3, layer_norm=True)
    assert dims == [16, 64, 64, 3] and act == "tanh" and lin == [m[1], m[4], m[7]] and norms == {"feature": m[0], "hidden": [m[3], m[6]]}
    for feature, hidden in ((False, True), (True, False), (False, False)):
        m = _openrl(1, act=nn.ReLU, feature=feature, hidden=hidden)
        dims, act, lin, norms = mlp_spec(m, "critic", 16, 1, layer_norm=True)
        assert dims == [16, 64, 64, 1] and act == "relu" and (norms["feature"] is not None) == feature and len(norms["hidden"]) == (2 if hidden else 0)
    m = nn.Sequential(nn.LayerNorm(16), nn.Linear(16, 3))
    assert mlp_spec(m, "actor", 16, 3, layer_norm=True)[3] == {"feature": m[0], "hidden": []}
    # the default call: three values, and a LayerNorm is refused with the message it always had
    assert len(mlp_spec(_openrl(3, feature=False, hidden=False), "actor", 16, 3)) == 3
    with pytest.raises(ValueError, match=r"actor\[2\] \(LayerNorm\): only Linear, Tanh and ReLU"):
        mlp_spec(nn.Sequential(nn.Linear(16, 8), nn.Tanh(), nn.LayerNorm(8), nn.Linear(8, 3)), "actor", 16, 3)
    with pytest.raises(ValueError, match=r"actor\[0\] \(LayerNorm\)"):
        mlp_spec(_openrl(3), "actor", 16, 3)
    spec = lambda *layers: mlp_spec(nn.Sequential(*layers), "actor", 16, 3, layer_norm=True)
    with pytest.raises(ValueError, match=r"actor\[4\] \(Tanh\): no LayerNorm behind this hidden activation, but one behind actor\[2\]"):
        spec(nn.Linear(16, 8), nn.Tanh(), nn.LayerNorm(8), nn.Linear(8, 8), nn.Tanh(), nn.Linear(8, 3))
    with pytest.raises(ValueError, match=r"actor\[1\] \(Tanh\): no LayerNorm behind"):
        spec(nn.Linear(16, 8), nn.Tanh(), nn.Linear(8, 8), nn.Tanh(), nn.LayerNorm(8), nn.Linear(8, 3))
    with pytest.raises(ValueError, match=r"actor\[4\] \(LayerNorm\): a LayerNorm directly behind a Linear layer \(behind the output"):
        spec(nn.Linear(16, 8), nn.Tanh(), nn.LayerNorm(8), nn.Linear(8, 3), nn.LayerNorm(3))
    with pytest.raises(ValueError, match=r"actor\[1\] \(LayerNorm\): a LayerNorm directly behind a Linear"):
        spec(nn.Linear(16, 8), nn.LayerNorm(8), nn.Tanh(), nn.Linear(8, 3))
    with pytest.raises(ValueError, match=r"actor\[2\] \(LayerNorm\): eps 1e-06"):
        spec(nn.Linear(16, 8), nn.Tanh(), nn.LayerNorm(8, eps=1e-6), nn.Linear(8, 3))
    with pytest.raises(ValueError, match=r"actor\[0\] \(LayerNorm\): elementwise_affine=False"):
        spec(nn.LayerNorm(16, elementwise_affine=False), nn.Linear(16, 3))
    with pytest.raises(ValueError, match=r"actor\[2\] \(LayerNorm\): normalized_shape \(4, 8\) is not the preceding width \(8,\)"):
        spec(nn.Linear(16, 8), nn.Tanh(), nn.LayerNorm((4, 8)), nn.Linear(8, 3))
    with pytest.raises(ValueError, match=r"actor\[0\] \(LayerNorm\): normalized_shape \(8,\) is not the preceding width \(16,\)"):
        spec(nn.LayerNorm(8), nn.Linear(16, 3))
    with pytest.raises(ValueError, match=r"actor\[1\] \(LayerNorm\): two LayerNorm layers in a row"):
        spec(nn.LayerNorm(16), nn.LayerNorm(16), nn.Linear(16, 3))
    with pytest.raises(ValueError, match=r"actor\[1\] \(ELU\)"):
        spec(nn.Linear(16, 8), nn.ELU(), nn.Linear(8, 3))


def test_set_actor_refuses_networks_that_differ_and_the_oracle_env_by_name(gate_wrapper):  # noqa: F811
    w = gate_wrapper
    with pytest.raises(ValueError, match="critic: the feature norm"):
        w.set_actor(_openrl(3), _openrl(1, feature=False), layer_norm=True)
    with pytest.raises(ValueError, match="critic: the hidden norm"):
        w.set_actor(_openrl(3), _openrl(1, hidden=False), layer_norm=True)
    with pytest.raises(ValueError, match=r"actor\[0\] \(LayerNorm\): only Linear, Tanh and ReLU"):
        w.set_actor(_openrl(3), _openrl(1))
    with pytest.raises(NotImplementedError, match="HipEngine"):
        w.set_actor(_openrl(3), _openrl(1), layer_norm=True)


# ---- the twin against torch -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 7, 16, 17, 64, 255, 256])
def test_float64_norm_is_torch_layer_norm_and_the_float32_twin_is_near(n):
    g = torch.Generator().manual_seed(n)
    a = (torch.randn(66, n, generator=g) * 3 + 5).double()
    gam, bet = torch.rand(n, generator=g).double() + 0.5, torch.rand(n, generator=g).double() - 0.5
    u, xhat, rstd = ref.layer_norm(a, gam, bet)
    want = torch.nn.functional.layer_norm(a, (n,), gam, bet, 1e-5)
    assert float((u - want).abs().max()) <= 1e-12
    assert float((xhat * gam + bet - u).abs().max()) <= 1e-12 and rstd.shape == (66, 1)
    # the kernel-order float32 twin: a mean of magnitude 5 under a spread of 3 -- the centred second pass keeps the variance's digits
    u32 = ref.layer_norm(a.float(), gam.float(), bet.float(), kernel_order=True)[0]
    t32 = torch.nn.functional.layer_norm(a.float(), (n,), gam.float(), bet.float(), 1e-5)
    yard = max(float((t32.double() - want).abs().max()), 2.0 ** -24)
    assert float((u32.double() - want).abs().max()) <= 4 * yard, "the twin's order stays inside what the GPU is allowed"


@pytest.mark.parametrize("name", list(ref.CASES))
def test_manual_float64_backward_is_autograd_of_the_stated_loss(name):
    cfg = dict(CFG, entropy_coef=0.03, value_coef=0.7)
    s, args, norms = case(name, 130, 1)
    args = args[:-1] + (cfg,)
    g, st, S, _ = ppo_ref.manual(*args, **norms)
    ga, sta = ppo_ref.autograd(*args, torch.float64, **norms)
    assert set(g) == set(ga) == set(ref.layout(s["a_dims"], s["c_dims"], s["hidden"], s["feat"]))
    for n in g:
        scale = max(float(ga[n].abs().max()), 1e-300)
        assert float((g[n] - ga[n]).abs().max()) <= 1e-11 * scale, n
        assert S[n] >= float(g[n].abs().max()) * (1 - 1e-12), n
        if "norm" in n:
            assert float(ga[n].abs().max()) > 0, f"{n}: the case exercises this norm"
    assert float((st - sta).abs().max()) <= 1e-12 * float(sta.abs().max())
    gt = ppo_ref.manual(*args, tile=64, **norms)[0]
    assert all(float((gt[n] - g[n]).abs().max()) <= 1e-11 * max(float(g[n].abs().max()), 1e-300) for n in g)
    full = ppo_ref.batch(s, slice(None))
    assert not bool(ppo_ref.kinks(s["params"], s["a_dims"], s["c_dims"], s["act"], full, CFG, **norms).any()), "kink-free by the redraw rule"


# ---- K ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,M,seed", ref.K_CASES, ids=[f"{n}-M{m}-s{s}" for n, m, s in ref.K_CASES])
def test_two_float32_evaluations_are_inside_k(name, M, seed):
    """torch float32 autograd on the whole batch and the float32 manual backward (the norm in the kernel's order) over 64-row tiles, against the
    float64 backward: every tensor inside K_LN_CPU 2^-24 S_n, every statistic inside K_LN_CPU 2^-24 of its scale; and the forward of the
    kernel-order twin inside 4x torch's float32 error (layer_norm_ref's docstring holds the measured table)"""
    s, args, norms = case(name, M, seed)
    g64, st64, S, ss = ppo_ref.manual(*args, **norms)
    ga, sta = ppo_ref.autograd(*args, torch.float32, **norms)
    gm, stm, _, _ = ppo_ref.manual(*args, torch.float32, tile=64, **norms)
    ra, na = ppo_ref.ratio_to_bound(ga, g64, S)
    rm, nm = ppo_ref.ratio_to_bound(gm, g64, S)
    sa, sm = ppo_ref.stats_ratio(sta, st64, ss), ppo_ref.stats_ratio(stm, st64, ss)
    print(f"ln_k {name} M={M} seed={seed}: autograd {ra:.2f} ({na}) tiled {rm:.2f} ({nm}) stats {sa:.2f} {sm:.2f}")
    assert max(ra, rm, sa, sm) <= ref.K_LN_CPU
    assert ref.K_LN_GPU == 4 * ref.K_LN_CPU
    if M >= 63:
        obs = args[4]["obs"]
        e = ref.forward_errors(s["params"], s["a_dims"], s["c_dims"], s["act"], s["hidden"], s["feat"], obs)
        p32 = {k: v.float() for k, v in s["params"].items()}
        for who, dims, key in (("actor", s["a_dims"], "mean"), ("critic", s["c_dims"], "value")):
            y = ref.forward(p32, who, dims, s["act"], obs.float(), kernel_order=True, **norms)[0].double()
            y = y if key == "mean" else y[..., 0]
            assert float((y - e[key + "64"]).abs().max()) <= 4 * e["yard_" + key], (who, "the kernel-order twin against the forward yardstick")


@pytest.mark.parametrize("variant", ref.VARIANTS_FORWARD + ref.VARIANTS_BACKWARD)
def test_wrong_norms_are_far_outside(variant):
    """16 -> 7 / 17 with the hidden norm, layer 0 scaled by 0.01 so that a row's variance is of the size of eps (where `eps outside the root`
    differs), M = 1000: each wrong variant misses K_LN_GPU 2^-24 S_n by more than 100x in at least one tensor"""
    s, args, norms = case("tanh7_17", 1000, 0, weight_scale=0.01)
    g64, _, S, _ = ppo_ref.manual(*args, **norms)
    ok = ppo_ref.manual(*args, torch.float32, tile=64, **norms)[0]
    assert ppo_ref.ratio_to_bound(ok, g64, S)[0] <= ref.K_LN_CPU, "the right float32 evaluation of these inputs is inside"
    if variant in ref.VARIANTS_FORWARD:
        bad = ppo_ref.autograd(*args, torch.float32, variant=variant, **norms)[0]
    else:
        bad = ppo_ref.manual(*args, torch.float32, tile=64, variant=variant, **norms)[0]
    r, at = ppo_ref.ratio_to_bound(bad, g64, S)
    print(f"ln_wrong {variant}: {r:.3g} x 2^-24 S at {at} = {r / ref.K_LN_GPU:.0f} x the GPU bound")
    assert r > 100 * ref.K_LN_GPU, variant


# ---- kernel resources and the LDS rule -------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not (os.path.isfile(LIB_PATH) and all(os.path.isfile(os.path.join(LLVM, t)) for t in TOOLS)),
                    reason="needs the built HIP engine and the ROCm LLVM tools")
def test_ln_kernels_use_no_scratch(tmp_path):
    fat, co = str(tmp_path / "fat.bin"), str(tmp_path / "dev.co")
    subprocess.check_call([f"{LLVM}/llvm-objcopy", "--dump-section", f".hip_fatbin={fat}", LIB_PATH, str(tmp_path / "stripped.so")])
    subprocess.check_call([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"])
    notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True, check=True).stdout
    mine = []
    for blk in notes.split("- .agpr_count:")[1:]:
        f = dict(re.findall(r"\.(\w+):\s*(\S+)", ".agpr_count:" + blk))
        if re.match(r"_Z\d+k_(actor|ln_grad|ppo_grad)", f.get("name", "")):      # the two new kernels, and the two re-instantiated around shared device functions
            mine.append(f)
    short = sorted(re.sub(r"^_Z\d+(k_[a-z_]+?)(ILi(\d+)E.*|\d.*)$", r"\1\3", f["name"]) for f in mine)
    assert short == ["k_actor", "k_actor_ln", "k_ln_grad32", "k_ln_grad64", "k_ppo_grad32", "k_ppo_grad64"], short
    for f in mine:
        print(f["name"], "vgpr", f["vgpr_count"], "sgpr", f["sgpr_count"], "spills", f["vgpr_spill_count"], f["sgpr_spill_count"], "scratch",
              f["private_segment_fixed_size"], "static lds", f.get("group_segment_fixed_size", 0))
        assert int(f["private_segment_fixed_size"]) == 0 and int(f["vgpr_spill_count"]) == 0, f
        assert int(f["vgpr_count"]) <= 128, "1024 threads per workgroup: 128 registers each"
        assert int(f.get("group_segment_fixed_size", 0)) == 0, "all LDS is dynamic: the rule below is the whole footprint"


def _lds_bytes(a_hidden, c_hidden, D, hidden, feat, rt):
    """k_ln_grad's documented rule (csrc/kernels_ln.hpp)"""
    uw = max([D] if feat else [0]) if not hidden else max([D if feat else 0, *a_hidden, *c_hidden])
    rows = D + max(sum(a_hidden), sum(c_hidden)) + uw + 8 + 32 + 4
    return (rows * (rt + 1) + 2 + 2 * 64) * 4


def test_lds_rule_fits_every_accepted_shape_with_both_switches():
    src = open(KERNELS).read()
    assert "return ppo_lds_rows(a, c, D) + uw + LN_STAT + LN_PART;" in src and "#define LN_PART (2 * ACT_WAVES)" in src
    assert "#define LN_STAT (2 * MQE_ACTOR_MAX_LAYERS)" in src and (2 * ref.WAVES, 2 * abi.ACTOR_MAX_LAYERS) == (32, 8)
    limit = 160 * 1024
    widths = (1, 7, 64, 128, abi.ACTOR_MAX_HIDDEN)
    worst = 0
    stacks = [h for depth in range(abi.ACTOR_MAX_LAYERS) for h in itertools.product(widths, repeat=depth)]
    for D in (1, 16, abi.ACTOR_MAX_OBS):
        for ah in stacks:                                   # every pair, the two networks unlike: Uw is taken over both, the hidden sum over the larger
            for ch in stacks:
                worst = max(worst, _lds_bytes(ah, ch, D, True, True, 32))
    assert worst == _lds_bytes((256,) * 3, (256,) * 3, 128, True, True, 32) == (1196 * 33 + 130) * 4 <= limit
    # the `either network` clause: the widest norm in the network with the SMALLER hidden sum still sets Uw, and the other's sum the outputs
    assert _lds_bytes((256,) * 3, (256,), 128, True, True, 32) == _lds_bytes((256,), (256,) * 3, 128, True, True, 32) == worst
    assert _lds_bytes((64,) * 3, (256,), 16, True, True, 32) == _lds_bytes((256,), (64,) * 3, 16, True, True, 32) == ((16 + 256 + 256 + 44) * 33 + 130) * 4
    assert _lds_bytes((7,), (), 16, True, False, 32) == _lds_bytes((), (7,), 16, True, False, 32) == ((16 + 7 + 7 + 44) * 33 + 130) * 4
    # 64-row tiles: the headline shape keeps them; 3 x 128 at D = 16 does, at D = 128 it takes 32 rows where the plain rule (D + H + 4) keeps 64
    assert _lds_bytes((64, 64), (64, 64), 16, True, True, 64) <= limit
    assert _lds_bytes((128,) * 3, (128,) * 3, 16, True, True, 64) <= limit < _lds_bytes((128,) * 3, (128,) * 3, 128, True, True, 64)
    assert ((128 + 384 + 4) * 65 + 130) * 4 <= limit
    # k_actor_ln: two ping-pong buffers of the widest input, 4 output rows, the 32 partial rows, stride 65
    assert "(size_t)(2 * ldh + 4 + LN_PART) * ACT_LD * sizeof(float)" in src
    assert (2 * abi.ACTOR_MAX_HIDDEN + 4 + 32) * 65 * 4 <= limit
