"""The recurrent PPO update on a CPU-only host (MQE_PPO_BPTT; csrc/kernels_bptt.hpp; HipEngine.ppo_grad / ppo_update(chunk_length=)): the three
constants stated alike in header, kernels_bptt.hpp and abi.py and disjoint from every other flag, the LDS rule in Python against the C
expressions, the new kernels' resources, the manual backward of tests/bptt_ref.py against torch autograd in float64, K_CPU, the wrong variants
far outside the bound, and the Python refusals that need no GPU."""
import itertools
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

import bptt_ref as ref
from mqe.engine import abi
from mqe.engine.hip_engine import HipEngine, LIB_PATH
from test_rollout import HEADER, LLVM, TOOLS, ROOT

CSRC = os.path.join(ROOT, "multiagent-quadruped-environment_amd", "csrc")
KERNELS = os.path.join(CSRC, "kernels_bptt.hpp")
_SYNTH = {}


def synth(name, N, T, L, seed=0):
    key = (name, N, T, L, seed)
    if key not in _SYNTH:
        _SYNTH[key] = ref.synth(name, N, T, L, seed=seed)
    return _SYNTH[key]


# ---- constants -----------------------------------------------------------------------------------------------------------------------------------------
def test_constants_are_stated_alike_in_header_kernels_and_abi():
    header = open(HEADER).read()
    names = ("MQE_PPO_BPTT", "MQE_PPO_CHUNK_SHIFT", "MQE_PPO_MAX_CHUNK")
    stated = {k: int(v) for k, v in re.findall(r"\b(MQE_PPO_BPTT|MQE_PPO_CHUNK_SHIFT|MQE_PPO_MAX_CHUNK) = (\d+)\b", header)}
    defined = {k: int(v) for k, v in re.findall(r"^#define (MQE_[A-Z_]+) (\d+)\b", open(KERNELS).read(), re.M)}
    mirror = dict(MQE_PPO_BPTT=abi.PPO_BPTT, MQE_PPO_CHUNK_SHIFT=abi.PPO_CHUNK_SHIFT, MQE_PPO_MAX_CHUNK=abi.PPO_MAX_CHUNK)
    assert stated == defined == mirror == dict(zip(names, (32, 8, 64)))
    assert not re.search(r"^#define MQE_PPO_(BPTT|CHUNK_SHIFT|MAX_CHUNK)\b", header, re.M), "stated in words: the header's define sets are pinned"
    known = abi.PPO_CLIP_VALUE | abi.PPO_VALUE_NORM | abi.PPO_VALUE_NORM_UPDATE | 2 | 4
    field = 0xff << abi.PPO_CHUNK_SHIFT
    assert abi.PPO_BPTT & (known | field) == 0 and field & known == 0 and abi.PPO_MAX_CHUNK << abi.PPO_CHUNK_SHIFT & ~field == 0
    assert "back-propagation through time" in header and "MQE_PPO_BPTT" in header


# ---- the LDS rule --------------------------------------------------------------------------------------------------------------------------------------
def _c_rules():
    src = open(KERNELS).read()
    rows = re.search(r"static inline int bptt_lds_rows\(int base, int Hm, bool ln\) \{ return (.*?); \}", src)
    size = re.search(r"static inline size_t bptt_lds_bytes\(int rows, int rt\) \{ return (.*?); \}", src)
    assert rows and size, "the LDS rule is two host functions"
    consts = dict(BPTT_CELL_ROWS=int(re.search(r"#define BPTT_CELL_ROWS (\d+)", src).group(1)))
    assert re.search(r"#define BPTT_LDS_LIMIT \(160 \* 1024\)", src) and abi.BPTT_LDS_LIMIT == 160 * 1024 and abi.BPTT_CELL_ROWS == consts["BPTT_CELL_ROWS"]
    assert "#define LN_STAT (2 * MQE_ACTOR_MAX_LAYERS)" in open(os.path.join(CSRC, "kernels_ln.hpp")).read() and abi.LN_STAT == 2 * abi.ACTOR_MAX_LAYERS
    r = rows.group(1).replace("(ln ? 2 : 0)", "(2 if ln else 0)")
    b = size.group(1).replace("(size_t)", "").replace("sizeof(float)", "4")
    return (lambda base, Hm, ln: eval(r, {}, dict(consts, base=base, Hm=Hm, ln=ln))), (lambda rows, rt: eval(b, {}, dict(rows=rows, rt=rt)))


def _base_rows(a_dims, c_dims, hidden, feat):
    """ppo_lds_rows / ln_lds_rows of csrc/kernels_ppo.hpp and kernels_ln.hpp, restated"""
    D = a_dims[0]
    rows = D + max(sum(a_dims[1:-1]), sum(c_dims[1:-1])) + 4
    if hidden or feat:
        rows += max([D if feat else 0] + (list(a_dims[1:-1]) + list(c_dims[1:-1]) if hidden else [])) + 8 + 32
    return rows


def test_lds_rule_in_python_is_the_c_rule_and_every_shape_up_to_64_fits():
    c_rows, c_bytes = _c_rules()
    widths = (1, 7, 33, 64)
    stacks = [h for depth in (1, 2, 3) for h in itertools.product(widths, repeat=depth)]
    worst64 = 0
    for D in (1, 16, abi.ACTOR_MAX_OBS):
        for ah in stacks:
            for ch in stacks[::5]:
                for hidden, feat in itertools.product((False, True), repeat=2):
                    a_dims, c_dims = [D, *ah, 3], [D, *ch, 1]
                    rows = abi.bptt_lds_rows(a_dims, c_dims, hidden, feat)
                    assert rows == c_rows(_base_rows(a_dims, c_dims, hidden, feat), max(ah[-1], ch[-1]), hidden or feat)
                    for rt in (64, 32):
                        assert abi.bptt_lds_bytes(rows, rt) == c_bytes(rows, rt)
                    rt = abi.bptt_row_tile(a_dims, c_dims, hidden, feat)
                    assert rt in (64, 32), "every recurrent shape with all widths <= 64 and D <= 128 fits"
                    assert (rt == 64) == (c_bytes(rows, 64) <= abi.BPTT_LDS_LIMIT)
                    worst64 = max(worst64, rows)
    assert worst64 == 128 + 192 + 7 * 64 + 128 + 8 + 32 + 2 + 4 and abi.bptt_lds_bytes(worst64, 32) <= abi.BPTT_LDS_LIMIT
    # the flagship shapes: 64-row tiles without the norms, 32-row tiles with both; the widest accepted cell
    assert abi.bptt_row_tile([16, 64, 64, 3], [16, 64, 64, 1]) == 64 and abi.bptt_row_tile([16, 64, 64, 3], [16, 64, 64, 1], True, True) == 32
    assert abi.bptt_row_tile([16, 147, 3], [16, 147, 1]) == 32 and abi.bptt_row_tile([16, 148, 3], [16, 148, 1]) is None


# ---- kernel resources ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not (os.path.isfile(LIB_PATH) and all(os.path.isfile(os.path.join(LLVM, t)) for t in TOOLS)),
                    reason="needs the built HIP engine and the ROCm LLVM tools")
def test_bptt_kernels_use_no_scratch(tmp_path):
    fat, co = str(tmp_path / "fat.bin"), str(tmp_path / "dev.co")
    subprocess.check_call([f"{LLVM}/llvm-objcopy", "--dump-section", f".hip_fatbin={fat}", LIB_PATH, str(tmp_path / "stripped.so")])
    subprocess.check_call([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"])
    notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True, check=True).stdout
    mine = []
    for blk in notes.split("- .agpr_count:")[1:]:
        f = dict(re.findall(r"\.(\w+):\s*(\S+)", ".agpr_count:" + blk))
        if "k_bptt_" in f.get("name", ""):
            mine.append(f)
    assert sorted(re.sub(r"^_Z\d+|P.*$", "", f["name"]) for f in mine) == ["k_bptt_expand", "k_bptt_gradILi32EEv", "k_bptt_gradILi64EEv", "k_bptt_ln_gradILi32EEv",
                                                                          "k_bptt_ln_gradILi64EEv"]
    for f in mine:
        print(f["name"][:28], "vgpr", f["vgpr_count"], "sgpr", f["sgpr_count"], "spills", f["vgpr_spill_count"], f["sgpr_spill_count"], "scratch",
              f["private_segment_fixed_size"])
        assert int(f["private_segment_fixed_size"]) == 0 and int(f["vgpr_spill_count"]) == 0, f
        assert int(f["vgpr_count"]) <= 128, "1024 threads per workgroup: 128 registers each"
        assert int(f.get("group_segment_fixed_size", 0)) == 0, "all LDS is dynamic: the rule above is the whole footprint"


# ---- the manual backward, K_CPU, the wrong variants ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ref.SHAPES))
def test_manual_backward_is_autograd_in_float64(name):
    N, T, L = 3, 10, 5
    s = synth(name, N, T, L)
    chunks = s["index"][:9].numpy()
    ga, sa, _ = ref.autograd(s, chunks, L, ref.CFG)
    gm, sm, S = ref.manual(s, chunks, L, ref.CFG)
    r, at = ref.ratio_to_bound({k: v.numpy() for k, v in ga.items()}, gm, S)
    print(f"bptt_manual {name}: autograd64 - manual64 = {r:.2e} x 2^-24 S at {at}")
    assert r <= 1e-6, (r, at)
    assert float(np.abs(sa.numpy() - sm).max()) <= 1e-12
    inside, at0 = ref.resets_inside(s, np.arange(s["n_chunks"]), L)
    assert inside >= 0.25 and at0 > 0, "at least a quarter of the chunks hold a reset inside, some at their first step"


def test_k_cpu_holds_both_float32_evaluations():
    worst, table, threads = 0.0, {}, torch.get_num_threads()
    for group, cases in ref.CASES.items():
        for name, N, T, L, calls in cases:
            s = synth(name, N, T, L)
            for first, count, use_index, vclip in calls:
                chunks = ref.selection(s, first, count, use_index)
                cfg = dict(ref.CFG, value_clip=ref.VALUE_CLIP if vclip else None)
                g64, _, S = ref.manual(s, chunks, L, cfg)
                ra = 0.0
                for nt in (1, threads):              # torch's float32 sums depend on how many threads share them: both orders count
                    torch.set_num_threads(nt)
                    ga, _, _ = ref.autograd(s, chunks, L, cfg, torch.float32)
                    ra = max(ra, ref.ratio_to_bound({k: v.numpy() for k, v in ga.items()}, g64, S)[0])
                gt, _, _ = ref.manual(s, chunks, L, cfg, np.float32, tile=64)
                rt = ref.ratio_to_bound(gt, g64, S)[0]
                table[(group, name)] = max(table.get((group, name), 0.0), ra, rt)
                worst = max(worst, ra, rt)
    for group in ref.CASES:
        print(f"bptt_k {group:8s}" + "".join(f"  {n}: {v:.1f}" for (g, n), v in table.items() if g == group))
    print(f"bptt_k max {worst:.2f} (K_CPU {ref.K_CPU})")
    assert worst <= ref.K_CPU


@pytest.mark.parametrize("name,L", [("tanh9x5_6x7_both", 5), ("tanh7_5", 5), ("tanh64x64_both", 2)])
def test_wrong_variants_lie_far_outside_the_bound(name, L):
    N, T = 4, 10
    s = synth(name, N, T, L)
    chunks = np.arange(s["n_chunks"])                   # every chunk: the variant that carries across chunks needs the chunk in front
    g64, _, S = ref.manual(s, chunks, L, ref.CFG)
    for variant in ref.WRONG:
        if variant == "no_gru_norm_grad" and not s["hidden"]:
            continue
        gw, _, _ = ref.manual(s, chunks, L, ref.CFG, variant=variant)
        r, at = ref.ratio_to_bound(gw, g64, S)
        print(f"bptt_wrong {name} L={L} {variant}: {r / ref.K_GPU:.1f} x the bound at {at}")
        assert r >= 100 * ref.K_GPU, (variant, r, at)


# ---- the Python surface without a GPU ------------------------------------------------------------------------------------------------------------------------
def _engine(recurrent):
    eng = HipEngine.__new__(HipEngine)
    eng._actor = dict(recurrent=recurrent, critic_dims=[16, 5, 1], actor_dims=[16, 7, 3], value_norm=False)
    return eng


def test_chunk_length_refusals_need_no_gpu():
    traj = types.SimpleNamespace(T=10, hidden=object())
    rec, plain = _engine(True), _engine(False)
    for who in ("ppo_grad", "ppo_update"):
        with pytest.raises(NotImplementedError, match="back-propagation through time"):
            rec._chunks(who, traj, None)
        with pytest.raises(ValueError, match="chunk_length= needs a recurrent actor"):
            plain._chunks(who, traj, 5)
        with pytest.raises(ValueError, match="not a multiple of chunk_length"):
            rec._chunks(who, traj, 3)
        with pytest.raises(ValueError, match="traj.hidden is None"):
            rec._chunks(who, types.SimpleNamespace(T=10, hidden=None), 5)
        with pytest.raises(ValueError, match="chunk_length must be 1 .. 64"):
            rec._chunks(who, types.SimpleNamespace(T=130, hidden=object()), 65)
    assert rec._chunks("ppo_grad", traj, 5) == 5 and plain._chunks("ppo_grad", traj, None) == 0
    with pytest.raises(NotImplementedError, match="back-propagation through time"):
        HipEngine.ppo_grad(rec, traj)
    with pytest.raises(NotImplementedError, match="back-propagation through time"):
        HipEngine.ppo_update(rec, traj, epochs=1, minibatches=1, lr=1e-3)
    with pytest.raises(ValueError, match="chunk_length= needs a recurrent actor"):
        HipEngine.ppo_grad(plain, traj, chunk_length=5)
