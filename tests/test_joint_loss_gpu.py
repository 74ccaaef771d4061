"""-m gpu: the joint-ratio and dual-clip losses of mqe_ppo_grad (MQE_PPO_JOINT, MQE_PPO_DUAL_CLIP; csrc/kernels_ppo.hpp; HipEngine.ppo_grad /
ppo_update(joint=, dual_clip=)) against tests/joint_ref.py: (1) gradient and statistics against float64 within 4 x the K measured on the CPU; (3) the
same bits as the plain call where the switch cannot act; (4) a layer-norm handle; (5) a recurrent handle; (6) determinism, guards, inputs; (7) value
normalisation; (8) more tiles than workgroups; (9) every new refusal; (10) the public surface.

THE HANDLES WITH A' = 4 AND A' = 1.  Among the stock tasks only go1football-2vs2 has four agents and only go1plane one, and both carry the stub wrapper
(no task observation), which mqe_actor_create refuses.  Nothing ties a task observation to an agent count, though: (2) and the A' = 1 case of (3) run
on those two scenes with the descriptor's task kind set to the seesaw wrapper's -- its observation (the agent's one-hot, its own and its mirror
partner's base state: D = 12 + A') and reward loop over the agents and touch no NPC.  The gradient tests read synthetic trajectories and never step
the scene, so what the wrapper means there does not matter; A' and D are taken from the tensor's shape.

Measured on an MI355X (the largest figure each test printed, x 2^-24 S_n; bounds 88, layer norm 124, recurrent 160): see DESIGN 3.10."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import bptt_ref
import gru_ref
import joint_ref as ref
import ppo_ref
import test_bptt_gpu as B
import test_ppo_gpu as P
from helpers import make_desc, hip_engine
from mqe.engine import abi
from test_rollout_gpu import same_bits, _gate_env, _modules, gate_cfg_restored  # noqa: F401

pytestmark = pytest.mark.gpu

EPS32 = ppo_ref.EPS32
JOINT, DUAL, CLIPV = abi.PPO_JOINT, abi.PPO_DUAL_CLIP, abi.PPO_CLIP_VALUE
_SYNTH = {}


def synth(net, N, T, cd=ref.DUAL, **norms):
    """the shared synthetic go1gate trajectory (A' = 2, D = 16; host side: made once, never changed)"""
    key = (net, N, T, cd, tuple(sorted(norms.items())))
    if key not in _SYNTH:
        _SYNTH[key] = ref.synth(net, (N, 2, T, 16), 40 + 7 * N + T + len(net), cd, **norms)
    return _SYNTH[key]


def scene_handle(task, N):
    """a stock scene with the seesaw wrapper's task observation (the module docstring): -> (engine, A', D)"""
    key = ("seesaw wrapper", task, N)
    if key not in _SYNTH:
        d, k, _ = make_desc(task, N)
        d.task = abi.TASK["seesaw"]
        _SYNTH[key] = hip_engine(d, k)
    eng = _SYNTH[key]
    n, Aw, D = (int(x) for x in eng.tensor(abi.T_WRAPPER_OBS).shape)
    assert n == N
    return eng, Aw, D


def upload(s, dev):
    t = P.upload(s, dev)
    t["gindex"] = s["gindex"].to(dev).contiguous()
    return t


def flags_of(cfg):
    return (CLIPV if cfg["value_clip"] is not None else 0) | (JOINT if cfg["joint"] else 0) | (DUAL if cfg["dual_clip"] is not None else 0)


def call(eng, s, t, first, count, use_index, cfg, loss=None, **kw):
    """mqe_ppo_grad with an mqe_ppo_loss_ex; the index list is the group permutation under the joint loss, the sample permutation otherwise"""
    if loss is None:
        loss = abi.PpoLossEx(cfg["clip"], cfg["value_coef"], cfg["entropy_coef"], cfg["value_clip"] if cfg["value_clip"] is not None else 0.0,
                             cfg["dual_clip"] if cfg["dual_clip"] is not None else 0.0)
    index = t["gindex" if cfg["joint"] else "index"].data_ptr() if use_index else None
    a = dict(T=s["T"], stride=s["stride"], index=index, flags=flags_of(cfg), grad=t["grad"].data_ptr(), stats=t["stats"].data_ptr(), ret=t["ret"].data_ptr())
    a.update(kw)
    rc = eng.lib.mqe_ppo_grad(eng.h, a["T"], t["packed"].data_ptr(), a["stride"], t["actions"].data_ptr(), t["logp_old"].data_ptr(), t["value"].data_ptr(),
                              t["adv"].data_ptr(), a["ret"], a["index"], first, count, C.cast(C.pointer(loss), C.POINTER(abi.PpoLoss)), a["flags"], a["grad"], a["stats"],
                              eng._stream())
    torch.cuda.synchronize()
    return rc


def selection(s, first, count, use_index, cfg):
    """the minibatch as ref.manual takes it: the group-major batch of the groups, or the samples themselves"""
    if cfg["joint"]:
        return ref.batch(s, s["gindex"][first:first + count] if use_index else torch.arange(first, first + count))
    return ppo_ref.batch(s, s["index"][first:first + count] if use_index else torch.arange(first, first + count))


def check(s, t, b, cfg, what, k="mlp"):
    grad, stats = P.outputs(s, t)
    norms = dict(hidden=s["hidden"], feat=s["feat"])
    g64, st64, S, ss = ref.manual(s["params"], s["a_dims"], s["c_dims"], s["act"], b, cfg, s["Aw"], **norms)
    flat = lambda g: ppo_ref.flat_grad(g, s["a_dims"], s["c_dims"], **norms)
    bound = flat({n: torch.full_like(g64[n], S[n]) for n in g64}) * EPS32
    assert bool(torch.isfinite(grad).all()) and bool(torch.isfinite(stats).all()), what
    dev, zero = (grad.double() - flat(g64)).abs(), bound == 0
    worst = float((dev[~zero] / bound[~zero]).max())
    sworst = float(((stats.double() - st64).abs() / (ss * EPS32)).max())
    print(f"joint_kernel {what}: gradient {worst:.2f} x 2^-24 S (bound {ref.K_GPU[k]:.0f}), statistics {sworst:.2f} x 2^-24 scale")
    assert bool((grad[zero] == 0).all()), f"{what}: a tensor without any contribution must be exactly 0"
    assert worst <= ref.K_GPU[k] and sworst <= ref.K_GPU[k], what
    return worst, sworst


# ---- 1. gradient and statistics against float64 ------------------------------------------------------------------------------------------------
# (count, first, index list?): groups under the joint loss -- 32 groups fill a 64-row tile, 16 a 32-row tile -- and samples without it
GROUPS = {64: ((1, 0, False), (31, 0, False), (32, 3, False), (33, 0, False), (65, 11, True)), 32: ((15, 0, False), (16, 3, False), (17, 5, True))}
SAMPLES = {64: ((1, 0, False), (63, 0, False), (64, 5, False), (65, 0, False), (130, 17, True)), 32: ((31, 0, False), (32, 5, False), (33, 17, True))}


@pytest.mark.parametrize("loss", list(ref.LOSSES))
@pytest.mark.parametrize("net", ["tanh64x64", "tanh7", "tanh256x3"])
def test_gradient_and_statistics_against_float64(net, loss):
    """go1gate (A' = 2, D = 16), N = 5, T = 24: 120 groups, every region of the generator with a seventh of them; value clipping on; c_d = 1.5.
    tanh256x3 takes 32-row tiles (lanes 32 .. 63 mirror rows 0 .. 31)"""
    s = synth(net, 5, 24)
    eng = P.handle("go1gate", 5)
    P.install(eng, s)
    rt = 32 if net == "tanh256x3" else 64
    cfg = dict(ref.CFG, **ref.LOSSES[loss])
    for count, first, use_index in (GROUPS if cfg["joint"] else SAMPLES)[rt]:
        t = upload(s, eng.torch_device)
        assert call(eng, s, t, first, count, use_index, cfg) == 0, eng.lib.mqe_last_error().decode()
        check(s, t, selection(s, first, count, use_index, cfg), cfg, f"{net} {loss} count={count} first={first} index={use_index}")


def test_the_reference_coefficient_and_no_value_clip():
    """c_d = 3.0 (dppo.yaml) on a trajectory whose dual-clipped region lies beyond 3; and the joint loss without value clipping"""
    s = synth("tanh64x64", 5, 24, cd=3.0)
    eng = P.handle("go1gate", 5)
    P.install(eng, s)
    for cfg in (dict(ref.CFG, joint=True, dual_clip=3.0), dict(ref.CFG, joint=False, dual_clip=3.0), dict(ref.CFG, joint=True, dual_clip=3.0, value_clip=None)):
        t = upload(s, eng.torch_device)
        count = 65 if cfg["joint"] else 130
        assert call(eng, s, t, 7, count, True, cfg) == 0, eng.lib.mqe_last_error().decode()
        check(s, t, selection(s, 7, count, True, cfg), cfg, f"tanh64x64 c_d=3 joint={cfg['joint']} vclip={cfg['value_clip']}")


# ---- 2. four agents: both steps of the butterfly -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", ["joint", "joint+dual"])
@pytest.mark.parametrize("net", ["tanh64x64", "tanh256x3"])
def test_four_agents(net, loss):
    """go1football-2vs2's four robots, N = 3, T = 24: 72 groups of four.  16 groups fill a 64-row tile (tanh64x64) and two 32-row tiles (tanh256x3);
    15, 16 from first > 0, 17 through the shuffled index"""
    eng, Aw, D = scene_handle("go1football-2vs2", 3)
    assert Aw == 4, "the scene with four agents"
    key = (net, "A4")
    if key not in _SYNTH:
        _SYNTH[key] = ref.synth(net, (3, Aw, 24, D), 77 + len(net))
    s = _SYNTH[key]
    P.install(eng, s)
    cfg = dict(ref.CFG, **ref.LOSSES[loss])
    for count, first, use_index in ((15, 0, False), (16, 3, False), (17, 5, True)):
        t = upload(s, eng.torch_device)
        assert call(eng, s, t, first, count, use_index, cfg) == 0, eng.lib.mqe_last_error().decode()
        check(s, t, selection(s, first, count, use_index, cfg), cfg, f"A'=4 D={D} {net} {loss} count={count} first={first} index={use_index}")


# ---- 3. the same bits as the plain call ----------------------------------------------------------------------------------------------------------
def test_one_agent_has_the_plain_call_bits():
    """go1plane's single robot: a group is a sample, and MQE_PPO_JOINT (with and without a dual clip that cannot act) returns the plain call's bits"""
    eng, Aw, D = scene_handle("go1plane", 5)
    assert Aw == 1, "the scene with one agent"
    s = _SYNTH.setdefault(("tanh64x64", "A1"), ref.synth("tanh64x64", (5, Aw, 40, D), 91))
    P.install(eng, s)
    dev = eng.torch_device
    for first, count, use_index in ((17, 130, True), (3, 65, False)):
        plain, joint, both = (upload(s, dev) for _ in range(3))
        for t in (joint, both):
            t["gindex"] = t["index"]                                                # a group is a sample: the same list
        assert P.call(eng, s, plain, first, count, use_index, ref.CFG) == 0
        assert call(eng, s, joint, first, count, use_index, dict(ref.CFG, joint=True)) == 0, eng.lib.mqe_last_error().decode()
        assert call(eng, s, both, first, count, use_index, dict(ref.CFG, joint=True, dual_clip=1e30)) == 0, eng.lib.mqe_last_error().decode()
        torch.cuda.synchronize()
        for t in (joint, both):
            assert torch.equal(plain["grad"], t["grad"]) and torch.equal(plain["stats"], t["stats"])
    check(s, both, ppo_ref.batch(s, torch.arange(3, 68)), dict(ref.CFG, joint=True, dual_clip=1e30), f"A'=1 D={D} tanh64x64 joint")


def test_an_unreachable_dual_clip_has_the_plain_call_bits():
    s = synth("tanh64x64", 5, 24)
    eng = P.handle("go1gate", 5)
    P.install(eng, s)
    plain, dual = upload(s, eng.torch_device), upload(s, eng.torch_device)
    assert P.call(eng, s, plain, 17, 130, True, ref.CFG) == 0                      # test_ppo_gpu's call: an mqe_ppo_loss of 16 bytes, no new bit
    assert call(eng, s, dual, 17, 130, True, dict(ref.CFG, joint=False, dual_clip=1e30)) == 0, eng.lib.mqe_last_error().decode()
    torch.cuda.synchronize()
    assert torch.equal(plain["grad"], dual["grad"]) and torch.equal(plain["stats"], dual["stats"])


# ---- 4. a layer-norm handle ------------------------------------------------------------------------------------------------------------------------
def test_layer_norm_handle():
    """k_ln_grad (both norms, 64 x 64): the same loss head behind another walk; its K is measured on the same networks (joint_ref.K["ln"])"""
    s = synth("tanh64x64", 5, 24, hidden=True, feat=True)
    eng = P.handle("go1gate", 5)
    eng.create_actor(s["a_dims"], s["c_dims"], activation=s["act"], layer_norm=True, feature_norm=True)
    views = eng.actor_params()
    for n, v in s["params"].items():
        views[n].copy_(v)
    cfg = dict(ref.CFG, **ref.LOSSES["joint+dual"])
    for count, first, use_index in ((1, 0, False), (33, 2, True), (65, 11, True)):
        t = upload(s, eng.torch_device)
        assert call(eng, s, t, first, count, use_index, cfg) == 0, eng.lib.mqe_last_error().decode()
        check(s, t, selection(s, first, count, use_index, cfg), cfg, f"layer norm joint+dual count={count}", k="ln")


# ---- 5. a recurrent handle -------------------------------------------------------------------------------------------------------------------------
def recurrent_call(eng, s, L, cfg, gindex, count, groups, what):
    """mqe_ppo_grad(MQE_PPO_BPTT | MQE_PPO_JOINT ...) over gindex[0 .. count) on a recurrent handle, against the float64 twin over the chunk groups `groups`;
    the statistics as test_bptt_gpu bounds them, with a group's A' log-probabilities"""
    t = B.upload(dict(s, index=gindex), eng.torch_device)
    lx = abi.PpoLossEx(cfg["clip"], cfg["value_coef"], cfg["entropy_coef"], cfg["value_clip"], cfg["dual_clip"] or 0.0)
    rc = eng.lib.mqe_ppo_grad(eng.h, s["T"], t["packed"].data_ptr(), s["stride"], t["actions"].data_ptr(), t["logp_old"].data_ptr(), t["value"].data_ptr(),
                              t["adv"].data_ptr(), t["ret"].data_ptr(), t["index"].data_ptr(), 0, count, C.cast(C.pointer(lx), C.POINTER(abi.PpoLoss)),
                              flags_of(cfg) | abi.PPO_BPTT | L << abi.PPO_CHUNK_SHIFT, t["grad"].data_ptr(), t["stats"].data_ptr(), eng._stream())
    torch.cuda.synchronize()
    assert rc == 0, eng.lib.mqe_last_error().decode()
    grad, stats = B.outputs(s, t)
    g64, st64, S = ref.bptt_manual(s, groups, L, cfg)
    got = {n: grad[o:o + int(np.prod(shp))].reshape(shp).numpy() for n, (o, shp) in
           abi.actor_param_layout(s["a_dims"], s["c_dims"], False, s["hidden"], s["feat"], recurrent=True).items()}
    worst, at = bptt_ref.ratio_to_bound(got, g64, S)
    chunks = ref.chunks_of(groups, 2)
    with torch.no_grad():
        a32, c32, ls = s["nets"]
        a64, c64 = gru_ref.doubles(a32, c32)
        m64, v64 = bptt_ref.twin_outputs(a64, c64, s, chunks, L, torch.float64)
        m32, v32 = bptt_ref.twin_outputs(a32, c32, s, chunks, L, torch.float32)
    b = bptt_ref.sample_data(s, chunks, L)
    logp = lambda m: ((-0.5 * ((b["actions"] - m.double()) * torch.exp(-ls.double())) ** 2 - ls.double()).sum(-1) - 1.5 * ref.LN2PI)
    e_p = 2 * (4 * float((logp(m32) - logp(m64)).abs().max()) + 2.0 ** -22)           # a group's Delta adds two of them
    e_v = 4 * float((v32.double() - v64).abs().max()) + 2.0 ** -22
    d = (logp(m64) - b["logp_old"]).reshape(-1)
    rho, A = torch.exp(ref.pair(d, 2)), ref.pair(b["adv"].reshape(-1), 2) * 0.5
    dv = torch.maximum((v64 - b["ret"]).abs(), (b["v_old"] - b["ret"]).abs() + cfg["value_clip"])
    tol = [float((A.abs() * rho).mean()) * math.expm1(e_p), float((2 * dv + e_v).mean()) * e_v, 0.0, 0.0, e_p, 0.0]
    tol[3] = tol[0] + cfg["value_coef"] * tol[1]
    tol = [x + 2.0 ** -22 * (1 + abs(float(st64[i]))) for i, x in enumerate(tol)]
    dev_s = np.abs(stats.double().numpy() - st64)
    print(f"joint_kernel_bptt {what}: gradient {worst:.2f} x 2^-24 S at {at} (bound {ref.K_GPU['bptt']:.0f}); statistics / their bounds " +
          " ".join(f"{x / y:.2f}" for x, y in zip(dev_s[:5], tol[:5])))
    assert worst <= ref.K_GPU["bptt"], (worst, at)
    assert stats[5].item() == np.float32(st64[5]), "kink-free groups: the same clip count"
    assert all(dev_s[i] <= tol[i] for i in range(5)), (dev_s, tol)


@pytest.mark.parametrize("name", ["tanh64x64_both", "tanh7_5"])
def test_recurrent_handle(name):
    """64-unit cells with both norms (k_bptt_ln_grad) and the smallest plain pair (k_bptt_grad): L = 4, T = 8, N = 5, so 10 chunk groups of two chunks;
    1 and all 10 through the seeded index, joint alone and with the dual clip; the statistics as test_bptt_gpu bounds them, with a group's A' log-probabilities"""
    L = 4
    s = _SYNTH.setdefault(("bptt", name), ref.bptt_synth(name, 5, 8, L))
    eng = B.handle(5)
    B.install(eng, s)
    for loss in ("joint", "joint+dual"):
        cfg = dict(ref.CFG, **ref.LOSSES[loss])
        for count in (1, 10):
            recurrent_call(eng, s, L, cfg, s["gindex"], count, s["gindex"][:count].numpy(), f"{name} {loss} chunk groups={count}")


def test_recurrent_handle_clamps_chunk_group_numbers():
    """chunk-group numbers outside [0, (T / L) N) are clamped, not followed (k_joint_expand, with (T / L) N as its range), and a group may come twice: the
    smallest recurrent shape, N = 4, T = 10, L = 5, so 8 chunk groups.  design() makes every group kink-free on its own, so any list of existing groups is"""
    L = 5
    s = _SYNTH.setdefault(("bptt", "tanh9x5_6x7_both", 4), ref.bptt_synth("tanh9x5_6x7_both", 4, 10, L))
    eng = B.handle(4)
    B.install(eng, s)
    gindex = torch.tensor([-4, 3, 8, 3, 2 ** 31 - 1, 6, -2 ** 31, 1], dtype=torch.int32)
    groups = np.clip(gindex.numpy().astype(np.int64), 0, s["n_groups"] - 1)
    assert s["n_groups"] == 8 and groups.min() == 0 and groups.max() == 7
    recurrent_call(eng, s, L, dict(ref.CFG, **ref.LOSSES["joint+dual"]), gindex, len(gindex), groups, "tanh9x5_6x7_both joint+dual clamped chunk groups")


# ---- 6. determinism, guards, inputs ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net", ["tanh64x64", "tanh256x3"])
def test_same_bits_identity_index_guards_and_inputs(net):
    s = synth(net, 5, 24)
    eng = P.handle("go1gate", 5)
    P.install(eng, s)
    cfg = dict(ref.CFG, **ref.LOSSES["joint+dual"])
    first, count = 3, s["n_groups"] - 7
    a, b, c = (upload(s, eng.torch_device) for _ in range(3))
    c["gindex"] = torch.arange(0, s["n_groups"], dtype=torch.int32, device=eng.torch_device)
    image = {k: v.clone() for k, v in a.items()}
    assert call(eng, s, a, first, count, False, cfg) == 0 and call(eng, s, b, first, count, False, cfg) == 0 and call(eng, s, c, first, count, True, cfg) == 0
    for name in ("grad", "stats"):
        assert torch.equal(a[name], b[name]), f"{name}: two calls on the same inputs differ"
        assert torch.equal(a[name], c[name]), f"{name}: the identity index list differs from the contiguous range"
    n = s["n_params"]
    assert bool((a["grad"][n:] == ppo_ref.SENT).all()) and bool((a["stats"][6:] == ppo_ref.SENT).all()), "guard words touched"
    assert not bool((a["grad"][:n] == ppo_ref.SENT).any()) and not bool((a["stats"][:6] == ppo_ref.SENT).any()), "an element was left unwritten"
    for k in ("packed", "value", "actions", "logp_old", "adv", "ret", "index", "gindex"):
        assert torch.equal(a[k].view(torch.uint8), image[k].view(torch.uint8)), f"{k} changed"
    d = upload(s, eng.torch_device)
    assert call(eng, s, d, first, count, True, cfg) == 0            # the shuffled list: other groups in other tiles
    assert not torch.equal(a["grad"], d["grad"])
    u = upload(s, eng.torch_device)                                 # group numbers outside [0, T N) are clamped, not followed
    u["gindex"][:3] = torch.tensor([-5, s["n_groups"] + 1000, 2 ** 31 - 1], dtype=torch.int32, device=eng.torch_device)
    assert call(eng, s, u, 0, 40, True, cfg) == 0
    sel = s["gindex"][:40].clone()
    sel[:3] = torch.tensor([0, s["n_groups"] - 1, s["n_groups"] - 1], dtype=torch.int32)
    check(s, u, ref.batch(s, sel), cfg, f"{net} clamped group numbers")


# ---- 7. value normalisation -------------------------------------------------------------------------------------------------------------------------
def test_value_normalisation_reads_the_expanded_list():
    """the five state floats after an updating joint call == after the plain call over the groups' samples, g A' + a group-major: k_vn_moments and
    k_vn_apply read the list k_joint_expand wrote"""
    s = synth("tanh7", 5, 24)
    eng = P.handle("go1gate", 5)
    VN = abi.PPO_VALUE_NORM | abi.PPO_VALUE_NORM_UPDATE
    cfg = dict(ref.CFG, **ref.LOSSES["joint+dual"])
    states = []
    for joint in (True, False):
        eng.create_actor(s["a_dims"], s["c_dims"], activation=s["act"], value_norm=True)
        views = eng.actor_params()
        for n, v in s["params"].items():
            views[n].copy_(v)
        before = views["value_norm"].clone()
        t = upload(s, eng.torch_device)
        first, count = 5, 47
        if joint:
            rc = call(eng, s, t, first, count, True, cfg, flags=flags_of(cfg) | VN)
        else:
            t["index"] = ref.samples_of(s["gindex"][first:first + count], 2).to(torch.int32).to(eng.torch_device)
            rc = call(eng, s, t, 0, 2 * count, True, dict(cfg, joint=False), flags=flags_of(dict(cfg, joint=False)) | VN)
        assert rc == 0, eng.lib.mqe_last_error().decode()
        after = eng.actor_params()["value_norm"].clone()
        assert not same_bits(before, after), "the call folds the returns into the statistics"
        states.append((after, t["stats"][1].clone()))
    assert same_bits(states[0][0], states[1][0]), (states[0][0], states[1][0])
    assert torch.equal(states[0][1], states[1][1]), "mean L_v: the same normalised targets, the same critic"


# ---- 8. more tiles than workgroups ---------------------------------------------------------------------------------------------------------------------
def test_more_tiles_than_workgroups():
    """9 900 contiguous groups (N = 33, T = 300; test_ppo_gpu's shape): 19 800 rows = 310 tiles of 64 for at most 256 workgroups"""
    s = synth("tanh64x64", 33, 300)
    eng = P.handle("go1gate", 33)
    P.install(eng, s)
    cfg = dict(ref.CFG, **ref.LOSSES["joint+dual"])
    t = upload(s, eng.torch_device)
    assert s["n_groups"] == 9900 and call(eng, s, t, 0, 9900, False, cfg) == 0, eng.lib.mqe_last_error().decode()
    check(s, t, ref.batch(s, torch.arange(9900)), cfg, "tanh64x64 joint+dual 9900 groups")


# ---- 9. refusals --------------------------------------------------------------------------------------------------------------------------------------
def test_new_refusals_and_old_callers():
    s = synth("tanh7", 5, 24)
    eng = P.handle("go1gate", 5)
    P.install(eng, s)
    t = upload(s, eng.torch_device)
    image = {k: v.clone() for k, v in t.items()}
    cfg = dict(ref.CFG, **ref.LOSSES["joint+dual"])

    def refused(word, first=0, count=20, use_index=True, cfg=cfg, **kw):
        rc = call(eng, s, t, first, count, use_index, cfg, **kw)
        msg = eng.lib.mqe_last_error().decode()
        assert rc == -6 and word in msg, (kw, rc, msg)
        for k in t:
            assert torch.equal(t[k].view(torch.uint8), image[k].view(torch.uint8)), (kw, k, "a refused call wrote into the buffers")

    for bad in (float("nan"), float("inf"), 1.2, 1.0, 0.0, -3.0):                  # c_d must exceed 1 + c = 1.2
        refused("dual_clip", cfg=dict(cfg, dual_clip=bad))
    for word in range(3):
        lx = abi.PpoLossEx(cfg["clip"], cfg["value_coef"], cfg["entropy_coef"], cfg["value_clip"], 1.5)
        lx.reserved[word] = 1e-45                                                   # one bit
        refused("reserved", loss=lx)
        lx.reserved[word] = -0.0                                                    # the sign bit alone
        refused("reserved", loss=lx)
    refused("first + count", first=s["n_groups"] - 19, count=20, use_index=False)       # the range is over groups: T N, not T N A'
    refused("flags", flags=flags_of(cfg) | 2)
    refused("flags", flags=flags_of(cfg) | 4)
    refused("MQE_PPO_BPTT", flags=flags_of(cfg) | abi.PPO_BPTT | 4 << abi.PPO_CHUNK_SHIFT)      # the new bits do not hide an old refusal
    refused("MQE_PPO_VALUE_NORM", flags=flags_of(cfg) | abi.PPO_VALUE_NORM)
    # without the new bits nothing beyond the first 16 bytes is read: a 16-byte mqe_ppo_loss at the very end of an allocation, garbage behind it in a 32-byte one
    plain_cfg = dict(ref.CFG, joint=False)
    garbage = abi.PpoLossEx(cfg["clip"], cfg["value_coef"], cfg["entropy_coef"], cfg["value_clip"], float("nan"))
    for word in range(3):
        garbage.reserved[word] = float("nan")
    a, b = upload(s, eng.torch_device), upload(s, eng.torch_device)
    assert call(eng, s, a, 0, 50, True, plain_cfg, loss=garbage) == 0, eng.lib.mqe_last_error().decode()
    assert P.call(eng, s, b, 0, 50, True, ref.CFG) == 0
    torch.cuda.synchronize()
    assert torch.equal(a["grad"], b["grad"]) and torch.equal(a["stats"], b["stats"])
    # the same calls with nothing wrong then succeed
    assert call(eng, s, t, 0, 20, True, cfg) == 0, eng.lib.mqe_last_error().decode()
    check(s, t, ref.batch(s, s["gindex"][:20]), cfg, "after the refusals")


# ---- 10. the public surface -------------------------------------------------------------------------------------------------------------------------------
def test_public_surface(gate_cfg_restored):  # noqa: F811
    N, T = 8, 8
    finals = []
    for _ in range(2):
        env = _gate_env(N)
        actor, critic, log_std = _modules(5)
        env.set_actor(actor, critic, log_std=log_std)
        env.reset()
        eng = env.env.engine
        traj = env.rollout(T, gamma=0.99, lam=0.95)
        p0 = eng.actor_params()["flat"].clone()
        stats = env.ppo_update(traj, epochs=2, minibatches=2, lr=1e-3, joint=True, dual_clip=3.0, generator=torch.Generator(device="cuda").manual_seed(4))
        torch.cuda.synchronize()
        assert stats.shape == (2, 2, abi.PPO_STATS) and bool(torch.isfinite(stats).all()) and eng.ppo_step == 4
        assert not same_bits(p0, eng.actor_params()["flat"]), "the parameters change"
        with pytest.raises(ValueError, match="groups"):
            env.ppo_update(traj, epochs=1, minibatches=T * N + 1, lr=1e-3, joint=True)      # bounded by the T N groups, not the T N A' samples
        with pytest.raises(RuntimeError, match="dual_clip"):
            eng.ppo_grad(traj, dual_clip=1.1)
        g_idx = torch.arange(T * N, dtype=torch.int32, device="cuda")
        ga, sa = eng.ppo_grad(traj, joint=True, dual_clip=3.0)
        gb, sb = eng.ppo_grad(traj, index=g_idx, joint=True, dual_clip=3.0)
        torch.cuda.synchronize()
        assert torch.equal(ga, gb) and torch.equal(sa, sb)
        finals.append((eng.actor_params()["flat"].clone(), stats.clone()))
    assert same_bits(finals[0][0], finals[1][0]) and same_bits(finals[0][1], finals[1][1]), "two engines, the same generator seed: the same bits"
