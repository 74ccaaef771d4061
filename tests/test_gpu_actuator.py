"""-m gpu: the actuator network inside the HIP engine, in both of its arithmetic forms -- layer 2 on split-f16 operands (default) and the
exact f32 MFMA chain (MQE_ACT_F32=1, or a network whose layer-2 weights do not fit the f16 planes) -- against the float64 reference of
tests/actuator_ref.py, the staged kernel (k_compute_torques_mfma) against the fused one (k_substeps) for every compiled variant, and the
f32 variants against the oracle; the P / V / T law likewise, fused against staged.  Every engine is built under MQE_VERBOSE, and the variant line of mqe_sim_create says which kernel ran."""
import numpy as np
import pytest
import torch

import actuator_ref as ar
from helpers import make_desc, hip_engine, oracle_engine
from mqe.engine import abi
from test_gpu_parity import _record          # measured deviations and variant lines: the parity tests' measurement log

pytestmark = pytest.mark.gpu


def variant_engine(monkeypatch, capfd, task, N, env=None, act_f32=False, tweak=None, oracle=False, **kw):
    """(HIP engine, desc, variant) built under the switches `env` (+ MQE_ACT_F32=1 if act_f32); variant = the fields of the line
    `mqe: variant shape=.. epw=.. actuator=.. post=..` that mqe_sim_create prints under MQE_VERBOSE.  oracle: an oracle engine on an
    equal desc as well (the switches that build_desc reads apply to both)."""
    env = dict(env or {})
    if act_f32:
        env["MQE_ACT_F32"] = "1"
    monkeypatch.delenv("MQE_ACT_F32", raising=False)
    for k, v in dict(env, MQE_VERBOSE="1").items():
        monkeypatch.setenv(k, v)
    capfd.readouterr()
    try:
        def desc():
            d, keep, _ = make_desc(task, N, max_episode_length=100000, **kw)
            if tweak:
                tweak(d)
            return d, keep
        d, keep = desc()
        e = hip_engine(d, keep)
        eo = oracle_engine(*desc()) if oracle else None
    finally:
        for k in dict(env, MQE_VERBOSE="1"):
            monkeypatch.delenv(k)
    err = capfd.readouterr().err
    lines = [ln for ln in err.splitlines() if ln.startswith("mqe: variant ")]
    assert len(lines) == 1, err
    var = dict(f.split("=", 1) for f in lines[0].split()[2:])
    _record("actuator_variant", {"task": task, "N": N, "env": env, "line": lines[0]})
    if act_f32:
        assert var["actuator"] == "f32", var
    return (e, d, var) if not oracle else (e, eo, d, var)


def _joints(d):
    """per joint of the batch (R * 12, robot-major): rest angle (f32), torque limit, hip flag"""
    R = d.num_envs * d.num_agents
    j = np.tile(np.arange(12), R)
    ddp = np.array([d.default_dof_pos[k] for k in range(12)], np.float32)[j]
    lim = np.array([d.torque_limits[k] for k in range(12)], np.float64)[j]
    return ddp, lim, j % 3 == 0


def _target(d, a, ddp, hip):
    """the joint target as both kernels compute it in f32: a * action_scale (* hip_scale_reduction on hips) + default angle"""
    s = np.asarray(a, np.float32) * np.float32(d.action_scale)
    s = np.where(hip, s * np.float32(d.hip_scale_reduction), s).astype(np.float32)
    return (s + ddp).astype(np.float32)


def check_tau(tau, x, lim, net=(None, None), what=""):
    """torques after the limit against the float64 network on the inputs the kernel saw: |tau - clip(tau64)| <= tau_bound everywhere,
    exactly +-limit where |tau64| exceeds the limit by more than the bound.  Returns the worst |tau - tau64| / bound off the limit."""
    ref, bnd = ar.tau64(x, *net), ar.tau_bound(x, *net)
    tau = np.asarray(tau, np.float64)
    dev = np.abs(tau - np.clip(ref, -lim, lim))
    i = int(np.argmax(dev / bnd))
    assert (dev <= bnd).all(), f"{what}: row {i}: tau {tau[i]!r}, tau64 {ref[i]!r}, bound {bnd[i]:.3e}, inputs {x[i].tolist()}"
    sat = np.abs(ref) > lim + bnd
    assert np.array_equal(tau[sat], np.sign(ref[sat]) * lim[sat]), f"{what}: a saturated torque is not exactly at its limit"
    free = np.abs(ref) <= lim - bnd
    return float((dev / bnd)[free].max()) if free.any() else 0.0


def staged_torques(e, d, x, a):
    """one compute_torques() with the actuator inputs of rows x (R * 12, 6: err, err_last, err_last_last, qd, qd_last, qd_last_last)
    made real: the joint angle is the target of the actions a (R * 12, dyadic: an exact target whatever the compiler contracts) plus
    the row's err.  Returns the torques, the inputs as the kernel sees them and the actuator history after the call [4][R * 12]."""
    N, A = d.num_envs, d.num_agents
    ddp, lim, hip = _joints(d)
    tgt = _target(d, a, ddp, hip)
    q = (tgt + x[:, 0]).astype(np.float32)
    xin = x.copy()
    xin[:, 0] = q - tgt                                     # f32, as the kernel forms err
    dof = e.tensor(abi.T_DOF_STATE)
    dof[:, :12 * A].copy_(torch.from_numpy(np.stack([q, x[:, 3]], -1).reshape(N, 12 * A, 2)))     # robots' joints only (seesaw rows stay)
    e.tensor(abi.T_ACT_HIST).copy_(torch.from_numpy(np.ascontiguousarray(x[:, [1, 2, 4, 5]].T).reshape(4, N * A, 12)))
    e.tensor(abi.T_ACTIONS).copy_(torch.from_numpy(np.asarray(a, np.float32).reshape(N, 12 * A)))
    e.compute_torques()
    torch.cuda.synchronize()
    return e.tensor(abi.T_TORQUES).cpu().numpy().reshape(-1), xin, e.tensor(abi.T_ACT_HIST).cpu().numpy().reshape(4, -1)


@pytest.mark.parametrize("task,N", [("go1plane", 1), ("go1gate", 37), ("go1football-defender", 3), ("go1football-2vs2", 5)])
def test_staged_kernel_against_float64(monkeypatch, capfd, task, N):
    """k_compute_torques_mfma in both forms on every input grid, at batches whose joint count fills no 32-joint tile (12, 888, 108, 240
    joints): torques within the float64 bound (exactly at the limit where saturated), the history shifted bit for bit"""
    x_all = np.concatenate([ar.grid(k, seed=i) for i, k in enumerate(ar.GRIDS)])
    taus, worst = {}, {}
    for f32 in (False, True):
        e, d, var = variant_engine(monkeypatch, capfd, task, N, act_f32=f32)
        assert var["actuator"] == ("f32" if f32 else "f16"), var
        e.reset_all()
        n = d.num_envs * d.num_agents * 12
        _, lim, _ = _joints(d)
        rs = np.random.RandomState(7)
        out, w = [], 0.0
        for c0 in range(0, len(x_all), n):
            x = x_all[np.arange(c0, c0 + n) % len(x_all)]
            a = rs.randint(-64, 65, n).astype(np.float32) / 16       # +-4 in 1/16 steps
            tau, xin, hist = staged_torques(e, d, x, a)
            w = max(w, check_tau(tau, xin, lim, what=f"{task} N={N} {var['actuator']}"))
            want = np.stack([xin[:, 0], x[:, 1], x[:, 3], x[:, 4]])
            assert np.array_equal(hist.view(np.int32), want.view(np.int32)), "actuator history after the call"
            out.append(tau[:max(0, min(n, len(x_all) - c0))])
        taus[f32], worst[var["actuator"]] = np.concatenate(out), w
        e.close()
    _record("actuator_staged", {"task": task, "N": N, "worst_dev_over_bound": worst})
    assert not np.array_equal(taus[False], taus[True]), "MQE_ACT_F32 did not reach the engine: both forms gave the same torques"


# the compiled k_substeps variants (mqe_engine.hip pick_shape / the shape table): (id, task, N, switches, shape, envs per wavefront, desc tweak)
def _lag(d):
    d.lag_timesteps = 6                   # the action lag of test_gpu_parity.py::test_domain_randomisation_matches_oracle


VARIANTS = [
    ("SH_A2-epw1", "go1gate", 32, {}, "SH_A2", 1, None),
    ("SH_A2-epw2", "go1gate", 37, {"MQE_ENVS_PER_WAVE": "2"}, "SH_A2", 2, None),
    ("SH_A1-epw1", "go1plane", 33, {}, "SH_A1", 1, None),
    ("SH_A1-epw2", "go1plane", 65, {"MQE_ENVS_PER_WAVE": "2"}, "SH_A1", 2, None),
    ("SH_A2_NOPAD", "go1gate", 32, {"MQE_COLLISION_MODEL": "exact"}, "SH_A2_NOPAD", 1, None),
    ("SH_A2_LINK", "go1seesaw", 16, {}, "SH_A2_LINK", 1, None),
    ("SH_A2_LINK-door", "go1revolvingdoor", 16, {}, "SH_A2_LINK", 1, None),
    ("SH_A2_NPC_FEW", "go1football-1vs1", 16, {}, "SH_A2_NPC_FEW", 1, None),
    ("SH_A2_BOX_FEW", "go1pushbox", 16, {}, "SH_A2_BOX_FEW", 1, None),
    ("SH_A2_STATIC_FEW", "go1bridge", 16, {}, "SH_A2_STATIC_FEW", 1, None),
    ("SH_A3_NPC_ROW", "go1football-defender", 16, {}, "SH_A3_NPC_ROW", 1, None),
    ("SH_A2_NPC", "go1sheep-hard", 14, {}, "SH_A2_NPC", 1, None),
    ("SH_A4_NPC", "go1football-2vs2", 8, {}, "SH_A4_NPC", 1, None),
    ("SH_A2_GEN", "go1gate", 32, {"MQE_LANE_SWEEP": "1"}, "SH_A2_GEN", 1, None),
    ("SH_GEN", "go1football-defender", 16, {"MQE_LANE_SWEEP": "1"}, "SH_GEN", 1, None),
    ("lagged", "go1gate", 32, {}, "SH_A2", 1, _lag),
]


def _controlled_state(d, state, seed=0):
    """(dof rows of the robots' joints [N, 12 A, 2], actuator history [4, R, 12]) written into both engines after the reset.
    standing: None (the seeded reset itself).  wide: joint angles +-0.6 rad around the rest pose inside the joint range, speeds +-30 rad/s,
    a history from the wide grid (+-3 rad, +-40 rad/s)"""
    if state == "standing":
        return None
    N, A = d.num_envs, d.num_agents
    rs = np.random.RandomState(seed)
    ddp, _, _ = _joints(d)
    lo = np.tile([d.robot.dof_lower[k] + 0.02 for k in range(12)], N * A)
    hi = np.tile([d.robot.dof_upper[k] - 0.02 for k in range(12)], N * A)
    q = np.clip(ddp + rs.uniform(-0.6, 0.6, ddp.shape), lo, hi).astype(np.float32)
    qd = rs.uniform(-30.0, 30.0, ddp.shape).astype(np.float32)
    x = ar.grid("wide", N * A * 12, seed)
    return np.stack([q, qd], -1).reshape(N, 12 * A, 2), np.ascontiguousarray(x[:, [1, 2, 4, 5]].T).reshape(4, N * A, 12)


def fused_and_staged(monkeypatch, capfd, task, N, env, act_f32, state, tweak=None, actuator=None):
    """engine A: step_command(cmd) -- substep 0 of k_substeps; engine B: policy_step(cmd), compute_torques() -- k_compute_torques_mfma;
    both from one desc and one controlled state.  Asserts A's substep-0 torques == B's torques bit for bit in the envs A did not reset
    (>= 90 % of them) and B's torques within the float64 bound (not under action lag: the target is then the lag ring's).  Returns
    (variant, A's substep-0 torques, B's torques, envs compared)."""
    kw = {} if actuator is None else {"actuator": actuator}
    eA, d, var = variant_engine(monkeypatch, capfd, task, N, env, act_f32, tweak, **kw)
    eB, _, varB = variant_engine(monkeypatch, capfd, task, N, env, act_f32, tweak, **kw)
    assert var == varB
    A = d.num_agents
    st = _controlled_state(d, state)
    for e in (eA, eB):
        e.reset_all()
        if st is not None:
            e.tensor(abi.T_DOF_STATE)[:, :12 * A].copy_(torch.from_numpy(st[0]))
            e.tensor(abi.T_ACT_HIST).copy_(torch.from_numpy(st[1]))
    g = torch.Generator().manual_seed(3)
    cmd = ((torch.rand(N * A, d.num_command_dims, generator=g) * 2 - 1) * 0.8).cuda().contiguous()
    eA.step_command(cmd)
    eB.policy_step(cmd)
    torch.cuda.synchronize()
    dof, hist, act = (eB.tensor(k).cpu().numpy() for k in (abi.T_DOF_STATE, abi.T_ACT_HIST, abi.T_ACTIONS))
    eB.compute_torques()
    torch.cuda.synchronize()
    keep = (eA.tensor(abi.T_RESET_BUF) == 0).cpu().numpy()
    assert keep.mean() >= 0.9, f"{task}: only {int(keep.sum())} of {N} envs stayed un-reset"
    assert np.array_equal(eA.tensor(abi.T_ACTIONS).cpu().numpy()[keep], act[keep]), "the two engines' policies disagree"
    fused = eA.tensor(abi.T_SUBSTEP_TORQUES)[:, 0].cpu().numpy()
    staged = eB.tensor(abi.T_TORQUES).cpu().numpy()
    diff = fused[keep].view(np.int32) != staged[keep].view(np.int32)
    assert not diff.any(), (f"{task} {var}: fused substep-0 torques differ from the staged kernel's in {int(diff.sum())} joints, "
                            f"max |diff| {np.abs(fused[keep] - staged[keep]).max():.3e}")
    if tweak is None:
        ddp, lim, hip = _joints(d)
        q = dof[:, :12 * A].reshape(-1, 2)
        tgt = _target(d, act.reshape(-1), ddp, hip)
        h = hist.reshape(4, -1)
        x = np.stack([q[:, 0] - tgt, h[0], h[1], q[:, 1], h[2], h[3]], -1)
        w = check_tau(staged.reshape(-1), x, lim, net=actuator or (None, None), what=f"{task} {var} staged")
        _record("actuator_fused_staged", {"task": task, "N": N, "env": env, "state": state, "variant": var, "worst_dev_over_bound": w})
    eA.close(); eB.close()
    return var, fused, staged, keep


@pytest.mark.parametrize("act_f32", [False, True], ids=["f16", "f32"])
@pytest.mark.parametrize("vid,task,N,env,shape,epw,tweak", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_fused_equals_staged_bit_for_bit(monkeypatch, capfd, vid, task, N, env, shape, epw, tweak, act_f32):
    """both copies of the network -- inside k_substeps and in k_compute_torques_mfma -- run the same instructions on the same bits:
    substep 0 of a fused step equals the staged kernel after the same policy step, for every compiled k_substeps variant and both forms"""
    for state in ("wide", "standing"):
        var, _, _, _ = fused_and_staged(monkeypatch, capfd, task, N, env, act_f32, state, tweak)
        assert (var["shape"], int(var["epw"]), var["actuator"]) == (shape, epw, "f32" if act_f32 else "f16"), var
        if epw == 2:           # the post-physics epilogue fused into the two-envs-per-wavefront kernel
            assert var["post"] == "fused", var


PD_SHAPES = [("go1gate", 5, {}, 1),                                    # 24 joints per env: one pass of the 64-lane joint loop
             ("go1football-2vs2", 3, {}, 1),                           # 48 joints per env, the generic shape
             ("go1plane", 3, {"MQE_ENVS_PER_WAVE": "2"}, 2)]           # the odd batch leaves a half-wave without an env


@pytest.mark.parametrize("ctrl", ["P", "V", "T"])
@pytest.mark.parametrize("task,N,env,epw", PD_SHAPES, ids=[s[0] for s in PD_SHAPES])
def test_fused_pd_law_equals_staged_bit_for_bit(monkeypatch, capfd, task, N, env, epw, ctrl):
    """control types P / V / T are one function (kernels_step.hpp joint_pd_torque) with two callers: engine A runs step_joint(a) -- the head
    of k_substeps' substep 0; engine B, from the same desc and the same controlled "wide" state, gets A's clipped actions and runs
    compute_torques() -- k_compute_torques.  A's substep-0 torques == B's torques bit for bit in the envs A did not reset (>= 90 %)."""
    def tweak(d):
        d.control_type = abi.CTRL[ctrl]
    # V once more with the wide state's speeds / 256: the D term on (qd - 0) / dt puts all but ~1 % of the wide state's torques at the limit
    for state, qd_scale in (("wide", 1.0),) + ((("wide-slow", 2.0 ** -8),) if ctrl == "V" else ()):
        eA, d, var = variant_engine(monkeypatch, capfd, task, N, env, tweak=tweak)
        eB, _, varB = variant_engine(monkeypatch, capfd, task, N, env, tweak=tweak)
        assert var == varB and int(var["epw"]) == epw, (var, varB)
        A = d.num_agents
        dof = _controlled_state(d, "wide")[0].copy()
        dof[..., 1] *= np.float32(qd_scale)
        for e in (eA, eB):
            e.reset_all()
            e.tensor(abi.T_DOF_STATE)[:, :12 * A].copy_(torch.from_numpy(dof))
        g = torch.Generator().manual_seed(3)
        a = ((torch.rand(N * A, 12, generator=g) * 2 - 1) * (1.0 if ctrl != "T" else 8.0)).cuda().contiguous()
        eA.step_joint(a)
        torch.cuda.synchronize()
        eB.tensor(abi.T_ACTIONS).copy_(eA.tensor(abi.T_ACTIONS))
        eB.compute_torques()
        torch.cuda.synchronize()
        keep = (eA.tensor(abi.T_RESET_BUF) == 0).cpu().numpy()
        assert keep.mean() >= 0.9, f"{task} {ctrl} {state}: only {int(keep.sum())} of {N} envs stayed un-reset"
        fused = eA.tensor(abi.T_SUBSTEP_TORQUES)[:, 0].cpu().numpy()[keep]
        staged = eB.tensor(abi.T_TORQUES).cpu().numpy()[keep]
        diff = fused.view(np.int32) != staged.view(np.int32)
        assert not diff.any(), (f"{task} {ctrl} {state} {var}: fused substep-0 torques differ from k_compute_torques' in {int(diff.sum())} joints, "
                                f"max |diff| {np.abs(fused - staged).max():.3e}")
        _, lim, _ = _joints(d)
        inside = float((np.abs(staged.reshape(-1)) < lim.reshape(N, -1)[keep].reshape(-1)).mean())
        _record("pd_fused_staged", {"task": task, "N": N, "env": env, "ctrl": ctrl, "state": state, "variant": var, "envs_compared": int(keep.sum()),
                                    "torques_inside_limit": inside})
        eA.close(); eB.close()


@pytest.mark.parametrize("vid,task,N,env,shape,epw,tweak", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_f32_variants_match_oracle(monkeypatch, capfd, vid, task, N, env, shape, epw, tweak):
    """the k_substeps<..., ACT32 = true> twins against the oracle: 5 fused steps from the seeded reset distribution, base-position
    deviation within the step-5 bounds of test_gpu_parity.py::test_fused_rollout_matches_oracle, reset flags identical"""
    eh, eo, d, var = variant_engine(monkeypatch, capfd, task, N, env, True, tweak, oracle=True)
    assert (var["shape"], int(var["epw"]), var["actuator"]) == (shape, epw, "f32"), var
    eh.reset_all(); eo.reset_all()
    A = d.num_agents
    Aw = eo.tensor(abi.T_WRAPPER_OBS).shape[1]
    g = torch.Generator().manual_seed(11)
    mism = 0
    for t in range(5):
        a = torch.rand(N, Aw, 3, generator=g) * 2 - 1
        eh.step(a.cuda().contiguous()); eo.step(a)
        torch.cuda.synchronize()
        mism += int((eh.tensor(abi.T_RESET_BUF).cpu() != eo.tensor(abi.T_RESET_BUF)).sum())
    rh, ro = eh.tensor(abi.T_ROOT_STATE).cpu(), eo.tensor(abi.T_ROOT_STATE)
    dev = (rh[:, :A, :3] - ro[:, :A, :3]).abs().amax(dim=(1, 2))
    assert torch.isfinite(dev).all()
    got = (float(dev.median()), float(dev.quantile(0.99)), float(dev.max()))
    _record("actuator_f32_rollout", {"variant": vid, "task": task, "N": N, "dev_step5": got, "flag_mismatches": mism})
    assert got[0] < 5e-7 and got[1] < 1e-5 and got[2] < 2e-5, f"{vid}: base position deviation after 5 steps (median, p99, max) = {got}"
    assert mism == 0, f"{vid}: {mism} reset-flag mismatches"
    eh.close(); eo.close()


def test_weight_range_fallback_and_its_threshold(monkeypatch, capfd):
    """A network whose layer-2 weights do not fit the f16 planes (2^14 |w| > 65504: max |W1| >= 3.99) runs the f32 chain without being
    asked: at max |W1| = 4.5 its fused and staged torques are those of MQE_ACT_F32=1 bit for bit; at 3.98 the planes are at their edge
    and the split-f16 form runs (other bits), both within the float64 bound of the scaled network"""
    for w1max, form in ((4.5, "f32"), (3.98, "f16")):
        net = ar.scaled_net(w1max)
        runs = {}
        for f32 in (False, True):
            var, fused, staged, keep = fused_and_staged(monkeypatch, capfd, "go1gate", 16, {}, f32, "wide", actuator=net)
            assert var["actuator"] == ("f32" if f32 else form), (w1max, var)
            runs[f32] = (fused[keep], staged)
        same = np.array_equal(runs[False][1].view(np.int32), runs[True][1].view(np.int32))
        if form == "f32":
            assert same and np.array_equal(runs[False][0].view(np.int32), runs[True][0].view(np.int32)), w1max
        else:
            assert not same, "the split-f16 form at max |W1| = 3.98 gave the f32 chain's bits"
