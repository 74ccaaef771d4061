"""-m gpu: the transformer's on-device PPO gradient (mqe_ppo_grad with MQE_PPO_TRANSFORMER; csrc/kernels_mat_grad.hpp: k_mat_grad, k_mat_reduce;
HipEngine.ppo_grad / ppo_update(transformer=True)) against tests/mat_grad_ref.py.  Every case compares every gradient tensor and the six statistics to
float64 autograd within K_MAT_GPU_OF[E] 2^-24 S_n (4 x the K measured on the CPU at that width), requires the guard words behind grad and stats
untouched and every gradient element written.  (1) go1gate 37 x 2, T = 3 at every width: the whole range, a slice of a permutation with a partial last
tile, one group; value clip on and off; (2) the joint ratio, the dual clip, value normalisation; (3) A' = 4 and A' = 1; (4) more tiles than workgroups,
an out-of-range index; (5) determinism and purity; (6) refusals; (7) end to end on a real rollout, the wrapper and the OpenRL adapter.
The trajectories are synthetic (mat_grad_ref.synth, written into mqe_rollout's layout) except (7)'s.  The handles with A' = 4 and A' = 1 are
tests/test_mat_gpu.py's (go1football-2vs2 and go1plane with the seesaw task kind).
WHAT THE WIDTHS PROTECT.  The bound is per width.  At E = 4 it is 20 796 x 2^-24 = 1.2e-3 of S_n, about 200 times what the kernel shows there (65 .. 112):
those cases catch gross errors and little else.  The per-tensor protection comes from E = 12 (bound 468, kernel 53 .. 322) and E = 64 (984, 36 .. 184)."""
import ctypes as C

import numpy as np
import pytest
import torch

import mat_grad_ref as ref
import mat_ref
import ppo_ref
import value_norm_ref as vref
from helpers import make_desc, hip_engine
from mqe.engine import abi
from test_mat_gpu import install as install_net, one_step
from test_rollout_gpu import _gate_env, engine, gate_cfg_restored, same_bits  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

EPS32, SENT = ppo_ref.EPS32, ppo_ref.SENT
MAT, JOINT, DUAL, CLIPV, VN, UPD = abi.PPO_TRANSFORMER, abi.PPO_JOINT, abi.PPO_DUAL_CLIP, abi.PPO_CLIP_VALUE, abi.PPO_VALUE_NORM, abi.PPO_VALUE_NORM_UPDATE
_HANDLES = {}


def handle(what):
    """the engine of mat_grad_ref.GPU_SHAPES[what]: go1gate, or a stock scene with the seesaw wrapper's task observation (tests/test_mat_gpu.py)"""
    if what not in _HANDLES:
        (N, Aw, _, D), _ = ref.GPU_SHAPES[what]
        task = {"gate": "go1gate", "many": "go1gate", "football": "go1football-2vs2", "plane": "go1plane", "sheep": "go1sheep-hard", "seesaw": "go1seesaw",
                "defender": "go1football-defender"}[what]
        d, k, _ = make_desc(task, N)
        if what in ("football", "plane"):                         # every other scene keeps its own task kind
            d.task = abi.TASK["seesaw"]
        eng = hip_engine(d, k)
        assert tuple(int(x) for x in eng.tensor(abi.T_WRAPPER_OBS).shape) == (N, Aw, D)
        _HANDLES[what] = eng
    return _HANDLES[what]


def install(eng, s, **kw):
    """a new transformer actor with the trajectory's parameters (scratch and moments of the old one are dropped); -> the views"""
    eng.create_actor([s["D"], s["E"], 3], None, transformer=True, **kw)
    views = eng.actor_params()
    views["flat"].copy_(mat_ref.flat_params(s["net"]))
    return views


def upload(s, dev):
    """fresh device images: packed / value / grad / stats carry sentinels and guards; the others are the logical tensors"""
    t = {k: torch.from_numpy(s[k].copy()).to(dev) for k in ("packed", "value", "grad", "stats")}
    t.update({k: s[k].to(dev).contiguous() for k in ("actions", "logp_old", "adv", "ret", "gindex")})
    return t


def flags_of(cfg):
    return MAT | (CLIPV if cfg["value_clip"] is not None else 0) | (JOINT if cfg["joint"] else 0) | (DUAL if cfg["dual_clip"] is not None else 0)


def call(eng, s, t, first, count, use_index, cfg, **kw):
    loss = abi.PpoLossEx(cfg["clip"], cfg["value_coef"], cfg["entropy_coef"], cfg["value_clip"] if cfg["value_clip"] is not None else 0.0,
                         cfg["dual_clip"] if cfg["dual_clip"] is not None else 0.0)
    a = dict(T=s["T"], stride=s["stride"], index=t["gindex"].data_ptr() if use_index else None, flags=flags_of(cfg), grad=t["grad"].data_ptr(),
             stats=t["stats"].data_ptr())
    a.update(kw)
    rc = eng.lib.mqe_ppo_grad(eng.h, a["T"], t["packed"].data_ptr(), a["stride"], t["actions"].data_ptr(), t["logp_old"].data_ptr(), t["value"].data_ptr(),
                              t["adv"].data_ptr(), t["ret"].data_ptr(), a["index"], first, count, C.cast(C.pointer(loss), C.POINTER(abi.PpoLoss)), a["flags"],
                              a["grad"], a["stats"], eng._stream())
    torch.cuda.synchronize()
    return rc


def groups_of(s, first, count, use_index):
    return s["gindex"][first:first + count].long() if use_index else torch.arange(first, first + count)


def check(s, t, b, cfg, what, kg=None):
    """gradient and statistics against float64 autograd within K_MAT_GPU_OF[E] (kg: the bound of an edge shape, K_MAT_GPU_AT[(E, D)]); guards; every
    gradient element written"""
    n, E = s["n_params"], s["E"]
    kg = ref.K_MAT_GPU_OF[E] if kg is None else kg
    gi, si = t["grad"].cpu(), t["stats"].cpu()
    assert bool((gi[n:] == SENT).all()) and bool((si[6:] == SENT).all()), f"{what}: a guard word was written"
    assert not bool((gi[:n] == SENT).any()) and not bool((si[:6] == SENT).any()), f"{what}: an output element was not written"
    grad, stats = gi[:n].view(torch.float32), si[:6].view(torch.float32)
    assert bool(torch.isfinite(grad).all()) and bool(torch.isfinite(stats).all()), what
    g64, st64, S, ss = ref.reference(s["net"], b, cfg)
    bound = ref.flat_bound(S, s["net"]) * EPS32
    dev, zero = (grad.double() - ref.flat(g64, s["net"])).abs(), bound == 0
    worst = float((dev[~zero] / bound[~zero]).max())
    sworst = float(((stats.double() - st64).abs() / (ss * EPS32)).max())
    print(f"mat_grad_kernel {what}: gradient {worst:.2f} x 2^-24 S (bound {kg:.0f}), statistics {sworst:.2f} x 2^-24 scale")
    assert bool((grad[zero] == 0).all()), f"{what}: a tensor without any contribution must be exactly 0"
    assert worst <= kg and sworst <= kg, what
    return grad, stats


# ---- 1. go1gate, every width ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vclip", [ref.VALUE_CLIP, None], ids=["vclip", "plain"])
@pytest.mark.parametrize("name", list(mat_ref.SHAPES))
def test_gradient_and_statistics_against_float64(name, vclip):
    """111 groups = 222 samples = 3 full tiles and one of 30 rows; 45 groups from first = 5 of the permutation: 90 samples, a partial last tile; one group"""
    E = mat_ref.SHAPES[name]
    s = ref.gpu_synth("gate", E)
    eng = handle("gate")
    install(eng, s)
    cfg = dict(ref.CFG, value_clip=vclip)
    for count, first, use_index in ((111, 0, False), (45, 5, True), (1, 7, True)):
        t = upload(s, eng.torch_device)
        assert call(eng, s, t, first, count, use_index, cfg) == 0, eng.lib.mqe_last_error().decode()
        check(s, t, ref.batch(s, groups_of(s, first, count, use_index)), cfg, f"{name} vclip={vclip} count={count} first={first} index={use_index}")


# ---- 2. the joint ratio, the dual clip, value normalisation ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", ["joint", "joint+dual"])
def test_joint_ratio_and_dual_clip(loss):
    s = ref.gpu_synth("gate", 12)
    eng = handle("gate")
    install(eng, s)
    cfg = dict(ref.CFG, joint=True, dual_clip=ref.DUAL if loss == "joint+dual" else None)
    t = upload(s, eng.torch_device)
    assert call(eng, s, t, 3, 70, True, cfg) == 0, eng.lib.mqe_last_error().decode()
    b = ref.batch(s, groups_of(s, 3, 70, True))
    grad, _ = check(s, t, b, cfg, f"e12 {loss} count=70 first=3")
    # the flags act: the per-sample loss on the same groups is another gradient
    g_plain, _, S, _ = ref.reference(s["net"], b, ref.CFG)
    assert float((grad.double() - ref.flat(g_plain, s["net"])).abs().max()) > 1e-4


def test_value_normalisation_follows_the_reference_state():
    """MQE_PPO_VALUE_NORM | MQE_PPO_VALUE_NORM_UPDATE: the minibatch's returns are folded into the state first (value_norm_ref.update, over the expanded
    sample list), the value loss compares with the returns normalised by the new (mu, sigma); the rest of the parameter buffer stays untouched"""
    s = ref.gpu_synth("gate", 12)
    eng = handle("gate")
    views = install(eng, s, value_norm=True)
    st = vref.k_state()
    views["value_norm"].copy_(torch.from_numpy(st))
    x = vref.raw_returns(s, st)                                  # reward units: normalised, they are the kink-free targets again
    t = upload(s, eng.torch_device)
    t["ret"] = torch.from_numpy(x).to(eng.torch_device)
    before = views["flat"].clone()
    first, count = 5, 45
    cfg = dict(ref.CFG)
    assert call(eng, s, t, first, count, True, cfg, flags=flags_of(cfg) | VN | UPD) == 0, eng.lib.mqe_last_error().decode()
    groups = groups_of(s, first, count, True)
    xs = x.reshape(s["n_groups"], s["Aw"])[groups.numpy()]
    after = views["value_norm"].cpu().numpy().copy()
    want, tol = vref.update(st, xs), vref.tol_update(st, xs)
    for name, g, w, tl in zip("mqd", after[:3], want, tol):
        assert abs(float(g) - w) <= tl, (name, float(g), w, tl)
    (mu, sg), (tmu, tsg) = vref.derive(*after[:3]), vref.tol_derived(*after[:3])
    assert abs(float(after[3]) - mu) <= tmu and abs(float(after[4]) - sg) <= tsg
    assert torch.equal(views["flat"], before), "the trainable parameters are inputs"
    b = ref.batch(s, groups)
    b["ret"] = torch.from_numpy(vref.normalise(xs, after[3], after[4]))      # float64 targets from the stored (mu, sigma)
    check(s, t, b, cfg, "e12 value normalisation count=45 first=5")


# ---- 3. A' = 4 and A' = 1 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [12, 64])
@pytest.mark.parametrize("what", ["football", "plane"])
def test_other_agent_counts(what, E):
    """17 envs x 4 agents = 68 rows a step: a tile holds 16 groups; 70 envs x 1 agent: every row its own group, nothing to attend to but itself"""
    s = ref.gpu_synth(what, E)
    eng = handle(what)
    install(eng, s)
    G = s["n_groups"]
    for cfg, (count, first, use_index) in ((dict(ref.CFG), (G, 0, False)), (dict(ref.CFG, joint=True, dual_clip=ref.DUAL), (G // 2 + 1, 3, True))):
        t = upload(s, eng.torch_device)
        assert call(eng, s, t, first, count, use_index, cfg) == 0, eng.lib.mqe_last_error().decode()
        check(s, t, ref.batch(s, groups_of(s, first, count, use_index)), cfg, f"{what} A'={s['Aw']} E={E} joint={cfg['joint']} count={count} first={first}")


# ---- 3b. the edges: E > 64, the widest width the gradient serves, the real tasks' observation sizes ----------------------------------------------------------
EDGES = [(what, E) for what, widths in ref.EDGE_WIDTHS.items() for E in widths]


@pytest.mark.parametrize("what,E", EDGES, ids=[f"{what}-e{E}" for what, E in EDGES])
def test_gradient_and_statistics_at_the_edges(what, E):
    """E = 68 and 72: a second, partial pass of the GELU loops and of actor_layer (4 and 8 outputs), norm chunks of 5 with empty wavefronts; E = 72: the largest
    LDS image (619 rows) and tape (2 D + 2900 rows); D = 14, 20, 34: the observation off the 16-byte grid beside aligned E x E matrices, T = max(D, E) = D at
    E = 12, G = E + D at E = 4 (the observation's gradient slot over slabs B1 .. REP).  The three selections of test 1 with the value clip on, held to
    K_MAT_GPU_AT[(E, D)]"""
    s = ref.gpu_synth(what, E)
    eng = handle(what)
    install(eng, s)
    kg = ref.K_MAT_GPU_AT[(E, s["D"])]
    cfg = dict(ref.CFG)
    assert cfg["value_clip"] == ref.VALUE_CLIP
    for count, first, use_index in ((s["n_groups"], 0, False), (45, 5, True), (1, 7, True)):
        t = upload(s, eng.torch_device)
        assert call(eng, s, t, first, count, use_index, cfg) == 0, eng.lib.mqe_last_error().decode()
        check(s, t, ref.batch(s, groups_of(s, first, count, use_index)), cfg, f"{what} E={E} D={s['D']} A'={s['Aw']} count={count} first={first} index={use_index}", kg)


@pytest.mark.parametrize("what,E", [("football", 72), ("sheep", 4)])
def test_joint_ratio_and_dual_clip_at_the_edges(what, E):
    s = ref.gpu_synth(what, E)
    eng = handle(what)
    install(eng, s)
    cfg = dict(ref.CFG, joint=True, dual_clip=ref.DUAL)
    first, count = 3, s["n_groups"] // 2 + 1
    t = upload(s, eng.torch_device)
    assert call(eng, s, t, first, count, True, cfg) == 0, eng.lib.mqe_last_error().decode()
    check(s, t, ref.batch(s, groups_of(s, first, count, True)), cfg, f"{what} E={E} D={s['D']} A'={s['Aw']} joint+dual count={count} first={first}",
          ref.K_MAT_GPU_AT[(E, s["D"])])


@pytest.mark.parametrize("what", ["gate", "sheep"])
def test_the_widest_width_and_the_first_refused(what):
    """D = 16 and D = 34: E = 72 is served; E = 76, which mqe_actor_create accepts, is refused with -5 naming the width and the bytes of the rule, and writes
    nothing; a plain actor created afterwards produces the gradient bits it produced before"""
    import test_ppo_gpu as P
    sp = P.synth("tanh7", "go1gate", 5, 24)
    plain_eng = P.handle("go1gate", 5)
    P.install(plain_eng, sp)
    tp = P.upload(sp, plain_eng.torch_device)
    assert P.call(plain_eng, sp, tp, 3, 100, True) == 0
    torch.cuda.synchronize()
    plain_bits = tp["grad"].clone()
    s = ref.gpu_synth(what, 72)
    D = s["D"]
    assert abi.mat_grad_lds_bytes(D, 72) <= abi.MATG_LDS_LIMIT < abi.mat_grad_lds_bytes(D, 76) and abi.actor_mat_lds_bytes(D, 76) <= abi.MAT_LDS_LIMIT
    eng = handle(what)
    install(eng, s)
    cfg = dict(ref.CFG)
    t = upload(s, eng.torch_device)
    assert call(eng, s, t, 0, 10, False, cfg) == 0, eng.lib.mqe_last_error().decode()
    check(s, t, ref.batch(s, torch.arange(10)), cfg, f"{what} E=72 D={D} in front of the refusal", ref.K_MAT_GPU_AT[(72, D)])
    eng.create_actor([D, 76, 3], None, transformer=True)
    n76 = mat_ref.param_count(D, 76)
    wide = dict(s, E=76, n_params=n76, grad=np.full(n76 + 64, SENT, np.int32))
    tw = upload(wide, eng.torch_device)
    rc = call(eng, wide, tw, 0, 10, False, cfg)
    msg = eng.lib.mqe_last_error().decode()
    assert rc == -5 and "E = 76" in msg and str(abi.mat_grad_lds_bytes(D, 76)) in msg, (rc, msg)
    assert bool((tw["grad"] == SENT).all()) and bool((tw["stats"] == SENT).all()), "a refused call wrote something"
    P.install(plain_eng, sp)
    tp3 = P.upload(sp, plain_eng.torch_device)
    assert P.call(plain_eng, sp, tp3, 3, 100, True) == 0
    torch.cuda.synchronize()
    assert torch.equal(tp3["grad"], plain_bits)


def test_widths_in_ascending_order_on_one_handle():
    """E = 12, then E = 72, then E = 12 again on one handle: tape and partials are the actor's and are released with it, so the wide actor gets its own
    (11.2 times the rows) and the second narrow gradient has the bits of the first.  Every other test installs a set's widths in descending order"""
    eng = handle("gate")
    cfg = dict(ref.CFG, joint=True, dual_clip=ref.DUAL)
    grads = []
    for E in (12, 72, 12):
        s = ref.gpu_synth("gate", E)
        install(eng, s)
        t = upload(s, eng.torch_device)
        assert call(eng, s, t, 2, 100, True, cfg) == 0, eng.lib.mqe_last_error().decode()
        kg = ref.K_MAT_GPU_AT[(72, 16)] if E == 72 else None
        check(s, t, ref.batch(s, groups_of(s, 2, 100, True)), cfg, f"gate E={E} in the order 12, 72, 12", kg)
        grads.append((t["grad"].clone(), t["stats"].clone()))
    assert torch.equal(grads[0][0], grads[2][0]) and torch.equal(grads[0][1], grads[2][1]), "the same bits behind a wider actor on the same handle"


# ---- 4. more tiles than workgroups ------------------------------------------------------------------------------------------------------------------------------
def test_more_tiles_than_workgroups_and_a_clamped_index():
    """go1gate N = 129, T = 64: 8256 groups = 16512 samples = 258 tiles > 256 workgroups, so workgroups 0 and 1 continue their chains over a second tile;
    then the same minibatch through an index list with a value beyond the groups and a negative one: clamped to the last group and to group 0"""
    s = ref.gpu_synth("many", 12)
    eng = handle("many")
    install(eng, s)
    G = s["n_groups"]
    assert (G * s["Aw"] + 63) // 64 == 258 > abi.PPO_MAX_WG
    cfg = dict(ref.CFG)
    t = upload(s, eng.torch_device)
    assert call(eng, s, t, 0, G, False, cfg) == 0, eng.lib.mqe_last_error().decode()
    check(s, t, ref.batch(s, torch.arange(G)), cfg, "e12 258 tiles")
    odd = s["gindex"].clone()
    odd[1], odd[2] = G + 1000, -5
    t = upload(s, eng.torch_device)
    t["gindex"] = odd.to(eng.torch_device)
    assert call(eng, s, t, 0, 130, True, cfg) == 0, eng.lib.mqe_last_error().decode()
    check(s, t, ref.batch(s, odd[:130].long().clamp(0, G - 1)), cfg, "e12 clamped index")


# ---- 5. determinism and purity --------------------------------------------------------------------------------------------------------------------------------------
def test_two_calls_give_equal_bits_and_inputs_stay():
    s = ref.gpu_synth("gate", 64)
    eng = handle("gate")
    views = install(eng, s)
    before = views["flat"].clone()
    cfg = dict(ref.CFG, joint=True, dual_clip=ref.DUAL)
    a, b = upload(s, eng.torch_device), upload(s, eng.torch_device)
    assert call(eng, s, a, 2, 100, True, cfg) == 0 and call(eng, s, b, 2, 100, True, cfg) == 0, eng.lib.mqe_last_error().decode()
    assert torch.equal(a["grad"], b["grad"]) and torch.equal(a["stats"], b["stats"]), "the same bits on every run"
    assert torch.equal(views["flat"], before), "the parameters are inputs"
    assert np.array_equal(a["packed"].cpu().numpy(), s["packed"]) and np.array_equal(a["value"].cpu().numpy(), s["value"])
    for k in ("actions", "logp_old", "adv", "ret"):
        assert same_bits(a[k].cpu(), s[k]), k
    assert torch.equal(a["gindex"].cpu(), s["gindex"])


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing_and_the_plain_path_keeps_its_bits():
    import test_ppo_gpu as P
    sp = P.synth("tanh7", "go1gate", 5, 24)
    plain_eng = P.handle("go1gate", 5)
    P.install(plain_eng, sp)
    tp = P.upload(sp, plain_eng.torch_device)
    assert P.call(plain_eng, sp, tp, 3, 100, True) == 0
    torch.cuda.synchronize()
    plain_bits = tp["grad"].clone()

    def refused(eng, s, t, first, count, use_index, cfg, word, **kw):
        rc = call(eng, s, t, first, count, use_index, cfg, **kw)
        msg = eng.lib.mqe_last_error().decode()
        assert rc == -6 and word in msg, (rc, msg)
        assert bool((t["grad"] == SENT).all()) and bool((t["stats"] == SENT).all()), "a refused call wrote something"
        return msg
    # the bit on a handle without MQE_ACTOR_TRANSFORMER
    tp2 = P.upload(sp, plain_eng.torch_device)
    rc = P.call(plain_eng, sp, tp2, 0, 10, False, flags=MAT)
    torch.cuda.synchronize()
    assert rc == -6 and "flags" in plain_eng.lib.mqe_last_error().decode() and "MQE_ACTOR_TRANSFORMER" in plain_eng.lib.mqe_last_error().decode()
    assert bool((tp2["grad"] == SENT).all()) and bool((tp2["stats"] == SENT).all())
    with pytest.raises(ValueError, match="transformer=True needs the transformer actor"):
        plain_eng.ppo_grad(None, transformer=True)
    s = ref.gpu_synth("gate", 12)
    eng = handle("gate")
    install(eng, s)
    cfg = dict(ref.CFG)
    t = upload(s, eng.torch_device)
    refused(eng, s, t, 0, 10, False, cfg, "flags", flags=flags_of(cfg) | abi.PPO_BPTT | 3 << abi.PPO_CHUNK_SHIFT)
    refused(eng, s, t, 0, 10, False, cfg, "flags", flags=flags_of(cfg) | 3 << abi.PPO_CHUNK_SHIFT)
    msg = refused(eng, s, t, 100, 12, False, cfg, "first + count")            # 112 > 111 groups
    assert "groups" in msg
    for unknown in (2, 4):
        refused(eng, s, t, 0, 10, False, cfg, "unknown bits", flags=flags_of(cfg) | unknown)
    msg = refused(eng, s, t, 0, 10, False, cfg, "gradient through the attention is not in the engine yet", flags=CLIPV)      # without the bit: as before
    assert "MATNet.evaluate" in msg
    # a width mqe_actor_create accepts and the gradient cannot serve: -5 naming E, nothing written
    eng.create_actor([16, 92, 3], None, transformer=True)
    wide = dict(s, E=92, n_params=mat_ref.param_count(16, 92), grad=np.full(mat_ref.param_count(16, 92) + 64, SENT, np.int32))
    tw = upload(wide, eng.torch_device)
    rc = call(eng, wide, tw, 0, 10, False, cfg)
    assert rc == -5 and "E = 92" in eng.lib.mqe_last_error().decode(), eng.lib.mqe_last_error().decode()
    assert bool((tw["grad"] == SENT).all()) and bool((tw["stats"] == SENT).all())
    # a plain actor created afterwards produces the gradient bits it produced before
    P.install(plain_eng, sp)
    tp3 = P.upload(sp, plain_eng.torch_device)
    assert P.call(plain_eng, sp, tp3, 3, 100, True) == 0
    torch.cuda.synchronize()
    assert torch.equal(tp3["grad"], plain_bits)


# ---- 7. end to end ------------------------------------------------------------------------------------------------------------------------------------------------------
def _traj_batch(traj, groups, ret):
    T, (N, Aw) = traj.T, traj.actions.shape[1:3]
    g = lambda x, *tail: x.cpu().reshape(T * N, Aw, *tail)[groups]
    return dict(obs=g(traj.obs[:T], traj.obs.shape[-1]), actions=g(traj.actions, 3), logp_old=g(traj.logp), v_old=g(traj.value[:T]), adv=g(traj.advantages),
                ret=ret.reshape(T * N, Aw)[groups])


def test_update_on_a_real_rollout():
    """rollout -> gae -> ppo_update(transformer=True), one minibatch of all T N groups under value normalisation: the parameters against ppo_ref.adam on the
    float64 gradient of that minibatch.  The bound: ppo_ref.adam_tolerances for the step's own roundings, plus what the first Adam step makes of a gradient
    deviation dg = K_MAT_GPU_OF 2^-24 S_n (tests/test_ppo_gpu.py's propagation:  step_size ((1 - b1) dg / denom + |m'| sqrt((1 - b2)(2 |g| dg + dg^2)) /
    (bc2s denom^2))).  Then a deterministic step follows the moved twin, and the first statistics' KL and clip share are the float64 values"""
    update_on_a_real_rollout("go1gate", 16, ref.K_MAT_GPU_OF[12])


def test_update_on_a_real_rollout_of_a_scene_with_npcs():
    """the same on go1sheep-hard: D = 34 > E = 12, the observations the scene itself produces, held to K_MAT_GPU_AT[(12, 34)]"""
    update_on_a_real_rollout("go1sheep-hard", 34, ref.K_MAT_GPU_AT[(12, 34)])


def update_on_a_real_rollout(task, D, kg):
    N, T, E, lr = 37, 6, 12, 1e-3
    eng = engine(task, N, seed=3, max_episode_length=5)
    assert tuple(int(x) for x in eng.tensor(abi.T_WRAPPER_OBS).shape) == (N, 2, D)
    net = install_net(eng, E, seed=9, value_norm=True)
    eng.reset_all()
    views = eng.actor_params()
    traj = eng.rollout(T, time_outs=True)
    eng.gae(traj, 0.99)
    torch.cuda.synchronize()
    p0 = views["flat"].cpu().clone()
    with pytest.raises(NotImplementedError, match="not in the\\s+engine yet"):
        eng.ppo_update(traj, epochs=1, minibatches=1, lr=lr)
    seed = lambda: torch.Generator(device=eng.torch_device).manual_seed(17)
    cfg = dict(clip=0.2, value_coef=0.5, entropy_coef=0.01, value_clip=0.2, joint=False, dual_clip=None)
    stats = eng.ppo_update(traj, epochs=1, minibatches=1, lr=lr, clip=0.2, value_coef=0.5, entropy_coef=0.01, value_clip=0.2, transformer=True, generator=seed())
    torch.cuda.synchronize()
    assert stats.shape == (1, 1, 6) and eng.ppo_step == 1
    perm = torch.randperm(T * N, device=eng.torch_device, generator=seed()).cpu()
    st = views["value_norm"].cpu().numpy()
    ret = torch.from_numpy(vref.normalise(traj.returns.cpu().numpy(), st[3], st[4]))      # the targets the update saw: its own new (mu, sigma)
    b = _traj_batch(traj, perm, ret)
    g64, st64, S, ss = ref.reference(net, b, cfg)
    for q in (4, 5):                                             # approximate KL, clip share
        assert abs(float(stats[0, 0, q]) - float(st64[q])) <= kg * EPS32 * float(ss[q]), (q, float(stats[0, 0, q]), float(st64[q]))
    g, dg = ref.flat(g64, net), ref.flat_bound(S, net) * (kg * EPS32) * 1.01
    zeros = torch.zeros_like(p0)
    p64, m64, v64, _ = ppo_ref.adam(p0, zeros, zeros, g, 1, lr)
    tol_p = ppo_ref.adam_tolerances(p0, zeros, zeros, g, 1, lr)[0]
    b1, b2, eps = (float(np.float32(x)) for x in (0.9, 0.999, 1e-8))
    step_size, bc2s = lr / (1 - b1), (1 - b2) ** 0.5
    vlow = torch.clamp(v64 - (1 - b2) * (2 * g.abs() * dg + dg * dg), min=0.0)
    denom = torch.sqrt(vlow) / bc2s + eps
    bound = tol_p + step_size * ((1 - b1) * dg / denom + (m64.abs() + (1 - b1) * dg) * torch.sqrt((1 - b2) * (2 * g.abs() * dg + dg * dg)) / (bc2s * denom * denom))
    moved = views["flat"].cpu().double()
    worst = float(((moved - p64).abs() / bound).max())
    sure = g.abs() > 100 * dg                                    # where the gradient's sign is beyond doubt the first step is lr against it
    print(f"mat_update {task}: parameters at {worst:.3f} of the propagated bound; {int(sure.sum())} of {g.numel()} elements with a sure sign")
    assert worst <= 1.0
    assert int(sure.sum()) > g.numel() // 4 and float(((moved - p0.double())[sure] + lr * torch.sign(g[sure])).abs().max()) <= 0.01 * lr
    # a deterministic step afterwards follows the moved twin
    with torch.no_grad():
        torch.nn.utils.vector_to_parameters(views["flat"].cpu().clone(), list(net.parameters()))
    one_step(eng, net, N, 2, D, 5, f"{task} after ppo_update(transformer=True)")
    eng.close()


def test_wrapper_and_openrl_adapter_run_the_update(gate_cfg_restored):  # noqa: F811
    n, T = 4, 6
    env = _gate_env(n)
    net = mat_ref.make_net(16, 12, seed=5).cuda()
    env.set_actor(net, value_norm=True)
    env.reset()
    traj = env.rollout(T, gamma=0.99, normalize_advantages=True)
    views = env.env.engine.actor_params()
    before = views["flat"].clone()
    with pytest.raises(NotImplementedError, match="not in the\\s+engine yet"):
        env.ppo_update(traj, epochs=1, minibatches=1, lr=1e-3)
    with pytest.raises(ValueError, match=f"minibatches <= {T * n} groups"):
        env.ppo_update(traj, epochs=1, minibatches=T * n + 1, lr=1e-3, transformer=True)
    stats = env.ppo_update(traj, epochs=2, minibatches=3, lr=1e-3, value_clip=0.2, joint=True, dual_clip=3.0, transformer=True)
    torch.cuda.synchronize()
    assert stats.shape == (2, 3, 6) and bool(torch.isfinite(stats).all()) and env.env.engine.ppo_step == 6
    assert float((views["flat"] - before).abs().max()) > 1e-4, "the engine's buffer moved"
    env.pull_actor()
    assert torch.equal(views["flat"], mat_ref.flat_params(net)), "pull_actor brings the result into the module"
    from openrl_ws.utils import mqe_openrl_wrapper
    w = mqe_openrl_wrapper(env)
    w.set_actor(net)
    tr = w.rollout_torch(T, gamma=0.99)
    st = w.ppo_update_torch(tr, epochs=1, minibatches=2, lr=1e-3, transformer=True)
    torch.cuda.synchronize()
    assert st.shape == (1, 2, 6) and bool(torch.isfinite(st).all())
    env.close()
