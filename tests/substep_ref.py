"""Host side of the fast-free-flight substep tests (tests/test_substep_ref.py on the CPU, tests/test_substep_gpu.py on the GPU): seeded state
grids in which nothing touches anything, a driver that runs EXACTLY ONE substep through either path of an engine, and the metric that holds
the result to the float64 oracle with the float32 oracle's own error as the yardstick.

WHY.  Without contacts a substep is a continuous function of the state: forward kinematics, the mass matrix and its inverse, the velocity-product
(Coriolis, centripetal, gyroscopic) bias, the Gauss-Seidel pass over the joint limits, the integrator.  No LCP branch excuses a difference, so
every env is held, and at base rates of 15 rad/s and joint rates of several rad/s a wrong velocity-product term stands hundreds of float32
errors above the right one (the defect builds of the oracle, oracle/Makefile `defects`, are how tests/test_substep_ref.py proves that).

THE DRIVER.  fused=False writes the torques into T_TORQUES and calls simulate(): k_simulate, the run-time-shape instantiation.  fused=True
reaches the kernels a training step runs, k_substeps<TA, TP, EPW>: control type T, decimation 1, no termination, no time-out, no pushes, no
action lag, action_scale 16, then ONE step_joint(actions): the torque is clip(16 clip(action, clip_actions), torque_limits), the post-physics
step resets nothing and leaves root and dof state as the substep wrote them.  tests/test_substep_ref.py asserts on the oracle that both paths
give the same bits, with one exception: the sheep's script rewrites the SHEEP rows after the substep, so a flock's NPC rows are compared
through simulate() only (case k_simulate-flock).

THE GRIDS.  (name: q placement, sigma(qd) rad/s, sigma(v) m/s, sigma(w) rad/s, torque amplitude N m, domain randomisation).  Base orientations
are uniformly random unit quaternions; the robots and free NPCs (ball, sheep, box) of an env are stacked 5 m apart from z = 50 m up, at the x, y
the reset gave them; articulated scenery stays where the reset put it.  `mid`: joints uniform in the middle 80 % of their range.  `stops`: every
joint 0.2 % of its range inside one of its stops (either, at random) and moving into it at 8 rad/s (+-10 %).  `overspeed`: sigma(qd) = 60 rad/s against
velocity limits of 28 and 50.  `torque`: actions of +-(40 .. 100) N m on every joint, beyond every torque limit (20 / 25 N m).  A calf under 25 N m gains
4 .. 41 rad/s in one substep (the float64 oracle, 64 envs of go1gate; hip -8 .. 41, thigh -9 .. 24) against a 28 rad/s limit, so this grid alone starts every
joint AGAINST its torque, at TORQUE_QD = 12 .. 16 (hip), 4 .. 10 (thigh), 18 .. 24 rad/s (calf): the middle of what it gains, so that the substep ends inside the limits.  `domain`: `spin` with added base mass and CoM shift.
FAST_QD, the sigma of `fastjoints`: 5 rad/s.  15 rad/s against the 28 rad/s limit of 16 of a robot's 24 .. 48 joints per env leaves a joint beyond it in
most envs; at 5 rad/s the limit is 5.6 sigma away.

THE METRIC.  Classes: the robots' joint velocity, (q' - q) / dt, base w, base v, quaternion, position; for free NPCs w, v, quaternion, position;
on the limit grids `on` (below).  err(engine) = max over the kept envs and all components of |x - x_f64|; ratio = err(engine) / max(err(f32 oracle), floor),
floor = the rounding of the float64 oracle's float32 output: half an ulp of the largest |x_f64| of the class (/ dt for (q' - q) / dt).
EXCLUSION on the smooth grids (a condition on the float64 result, not a measurement): an env is left out when any joint's velocity after the substep
lies within NEAR = 1 % of a bound of the limit pass (lo = max((lower - q) / dt, -vmax), hi likewise), or beyond it.  At most EXCLUDE_CAP = 2 % of a
grid's envs may be left out -- with 16 or 33 envs: none.  Spinning at 15 rad/s a thin link gains up to ~20 rad/s from the gyroscopic term alone and about
one joint in 1000 ends near its limit, so the SEEDS are chosen on the float64 oracle: good_seeds() walks seeds 0, 1, 2, .. and keeps those
whose float64 result stays within the cap; nothing an engine under test computes enters the choice.
LIMIT GRIDS (`stops`, `overspeed`): the limit pass is what is tested, in every env.  It is continuous (each impulse is a projection), so all classes are held
as on a smooth grid.  A joint is ON a bound when its velocity is within ON_TOL = 1e-5 of it, relative (a joint the pass put on its bound carries the rounding of
v + (bound - v): 2 * 2^-24 |bound - v| / |bound| < 1.2e-6 in float32 at 200 rad/s against 21).  The set of ON joints must be the float64 oracle's in every env
in which the float64 result has no joint between ON_TOL / 10 and 10 ON_TOL of a bound (where rounding decides the side).  The joints the float64 oracle left
EXACTLY on a bound (within EXACT = 2^-22, relative: its float32 output is the bound's own float32 value or a neighbour) are compared with THE BOUND'S OWN VALUE in the
class `on` and taken out of `qd`; the others, a real distance inside their bound, stay in `qd`.

THE CONSTANTS.  K_CPU is MEASURED ON THE CPU, never on a kernel: the float32 oracle's largest ratio against itself across seeds -- three good seeds per
grid and case, the second and third against the first one's yardstick, at the batch sizes of the GPU test (16 and 33 envs) -- that is, how far the largest
float32 error of one draw of 16 envs lies above that of another.  K_GPU = 4 K_CPU (policy_ref.py's rule: the kernel sums in another order, CRBA + Schur
complement instead of per-body Jacobian sums + Cholesky, and divides with the 2.5-ulp hardware sequence).
Measured with `python -m pytest tests/test_substep_ref.py -s` (prints every case and grid) on a host whose oracle runs 8 OpenMP threads (torch: 8); the
oracle's arithmetic is per env and does not depend on the thread count.  Worst ratio per grid over the 14 host scenes of CASES:
    calm 2.00   spin 2.79   fastjoints 2.38   torque 2.00   stops 2.18   overspeed 4.35   domain 2.81
K_CPU = 4.5 is the maximum, 4.35 (go1plane, 33 envs, `overspeed`, class `on`), rounded up; K_GPU = 18.  K_CPU is NOT taken from anything a kernel computes.

SELF-CONTACTS.  The descriptor switches self_collision off.  With it on, joints drawn across 80 % of their range fold legs into each other in about one
env of 100, the float32 and float64 oracles then differ by a contact branch (measured: 1.8 rad/s on a joint, 0.6 rad/s on the base, against 3e-5 rad/s
in the median env), and the cross-seed ratio above reached 199 at 16 envs and 899 at 1024: the states were not in free flight.

THE DEFECT BUILDS at the final grids (16 envs, first good seed; ratio per class qd / (q' - q)/dt / w / v / quat / pos; go1gate | go1football-2vs2):
    spin        1  gyroscopic, all bodies   30400 28100 13700  5540  9190  59 | 16000 16000 10900  1770 12400  24
                2  centripetal             103000 95500 34700 25200 29000 268 | 51400 51400 28900 11800 30300 162
                3  w x (a qd)                9070  8370  3060  1940  2590  20 |  6390  6400  1150  1230  1180  17
                4  gyroscopic, body 3       15200 14000   969   763   649   8 |  7500  7500   669   542   657   8
    fastjoints  1                            2850  2860   929   946   906   6 |  1660  1590   736   518   516   2
                2                           11800 11900  2610  3010  2130  14 |  9430  9060  2750  3360  2270   9
                3                            3330  3350   904  2260   521  10 |  2720  2610  1090  2190   850   6
                4                            2410  2420   300   345   209   2 |   820   788   193   175   118   2
    domain      1                           35800 38300 22200  6420 19900  94 | 10200 10100  7240  2170  6350  53
                2                           67600 72400 60300 21200 46000 312 | 47000 46800 29900  9690 27600 236
                3                            6810  7290  3230  2580  2400  38 |  2790  2780   583   477   538  12
                4                           13200 14200  2000   974  1500  14 |  5480  5460   561   369   444   9
The correct build on the next good seed against the same yardstick: at most 2.64.  2 K_GPU = 36: the weakest defect stands 22 x above it.

ON THE MI355X (tests/test_substep_gpu.py, both solvers): the worst ratio of every shape row is 1.07 .. 2.00 (the 2.00s are one float32 ulp of an NPC's quaternion
component against half an ulp; the largest of a robot's classes is 1.63, `on`); in the velocity classes of the fast grids 0.87 .. 1.11.  The kernel's joint velocities lie 0.05 .. 1.3 (median 0.23)
yardsticks from the float32 oracle's: most of either one's distance to float64 is common to both (presumably the float32 rotations and joint geometry that enter both),
which is why the ratios sit so close to 1."""
import contextlib
import os

import numpy as np
import torch

from helpers import make_desc, to_dev
from mqe.engine import abi

FAST_QD = 5.0
#        name          q placement, sigma(qd), sigma(v), sigma(w), torque amplitude, domain randomisation
GRIDS = {"calm":       ("mid",   1.0,     0.3, 0.3,  5.0,   False),
         "spin":       ("mid",   3.0,     1.0, 15.0, 5.0,   False),
         "fastjoints": ("mid",   FAST_QD, 0.3, 2.0,  5.0,   False),
         "torque":     ("mid",   None,    0.3, 0.3,  100.0, False),
         "stops":      ("stops", 8.0,     0.3, 0.3,  5.0,   False),
         "overspeed":  ("mid",   60.0,    0.3, 0.3,  5.0,   False),
         "domain":     ("mid",   3.0,     1.0, 15.0, 5.0,   True)}
SMOOTH = ("calm", "spin", "fastjoints", "torque", "domain")
LIMIT = ("stops", "overspeed")
FAST = ("spin", "fastjoints", "domain")
LIFT_Z, APART = 50.0, 5.0
ACTION_SCALE = 16.0            # torque = ACTION_SCALE * action: a power of two, so that 100 N m pass the action clip (10 in some tasks) exactly
TORQUE_QD = ((12.0, 16.0), (4.0, 10.0), (18.0, 24.0))     # `torque`: |qd| of hip, thigh, calf before the substep, against the torque's sign
NEAR, ON_TOL, EXACT, EXCLUDE_CAP = 1e-2, 1e-5, 2.0 ** -22, 0.02
SEEDS_TRIED = 20

K_CPU = 4.5                      # measured 4.35 (go1plane, 33 envs, `overspeed`, class `on`), rounded up; see the table above
K_GPU = 4 * K_CPU

# the GPU test's cases, shared with the CPU test that measures K_CPU on them: (id, task, N, switches, shape, envs per wavefront, fused)
CASES = [
    ("SH_A2-epw1", "go1gate", 16, {"MQE_ENVS_PER_WAVE": "1"}, "SH_A2", 1, True),
    ("SH_A2-epw2", "go1gate", 33, {"MQE_ENVS_PER_WAVE": "2"}, "SH_A2", 2, True),
    ("SH_A1-epw1", "go1plane", 16, {"MQE_ENVS_PER_WAVE": "1"}, "SH_A1", 1, True),
    ("SH_A1-epw2", "go1plane", 33, {"MQE_ENVS_PER_WAVE": "2"}, "SH_A1", 2, True),
    ("SH_A2_NOPAD", "go1gate", 16, {"MQE_COLLISION_MODEL": "exact"}, "SH_A2_NOPAD", 1, True),
    ("SH_A2_LINK-seesaw", "go1seesaw", 16, {}, "SH_A2_LINK", 1, True),
    ("SH_A2_LINK-door", "go1revolvingdoor", 16, {}, "SH_A2_LINK", 1, True),
    ("SH_A2_LINK-tug", "go1tug", 16, {}, "SH_A2_LINK", 1, True),
    ("SH_A2_NPC_FEW", "go1football-1vs1", 16, {}, "SH_A2_NPC_FEW", 1, True),
    ("SH_A2_BOX_FEW", "go1pushbox", 16, {}, "SH_A2_BOX_FEW", 1, True),
    ("SH_A2_STATIC_FEW", "go1bridge", 16, {}, "SH_A2_STATIC_FEW", 1, True),
    ("SH_A3_NPC_ROW", "go1football-defender", 16, {}, "SH_A3_NPC_ROW", 1, True),
    ("SH_A2_NPC", "go1sheep-hard", 16, {}, "SH_A2_NPC", 1, True),
    ("SH_A4_NPC", "go1football-2vs2", 16, {}, "SH_A4_NPC", 1, True),
    ("SH_A2_GEN", "go1gate", 16, {"MQE_LANE_SWEEP": "1"}, "SH_A2_GEN", 1, True),
    ("SH_GEN", "go1football-defender", 16, {"MQE_LANE_SWEEP": "1"}, "SH_GEN", 1, True),
    ("k_simulate", "go1gate", 16, {}, "SH_A2", 1, False),
    ("k_simulate-flock", "go1sheep-hard", 16, {}, "SH_A2_NPC", 1, False),
]


def host_scenes():
    """the cases as the host oracles tell them apart: (task, N, switches build_desc reads, fused) -- the kernel-selecting switches do not reach the oracle"""
    seen = []
    for _, task, N, env, _, _, fused in CASES:
        key = (task, N, {k: v for k, v in env.items() if k == "MQE_COLLISION_MODEL"}, fused)
        if key not in seen:
            seen.append(key)
    return seen


@contextlib.contextmanager
def under(env):
    """the switches of a case in os.environ while its descriptors and engines are built"""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# ---- descriptor and engines ---------------------------------------------------------------------------------------------------------------
def substep_desc(task, N, domain=False):
    """the task's scene with the controller reduced to `torque = clip(16 action)` and everything after the substep switched off"""
    d, keep, _ = make_desc(task, N, max_episode_length=10 ** 6)
    d.control_type, d.decimation, d.action_scale = abi.CTRL["T"], 1, ACTION_SCALE
    d.termination_flags = d.terminate_on_base_contact = 0
    d.push_interval, d.lag_timesteps = 0, 0
    d.self_collision = 0        # joints across their whole range fold the legs into each other: contacts between a robot's own links are contacts
    if domain:       # tests/test_gpu_parity.py::test_two_envs_per_wavefront_is_bit_identical's ranges
        d.rand_base_mass, d.added_mass_lo, d.added_mass_hi = 1, -1.0, 3.0
        d.rand_com = 1
        for c, (lo, hi) in enumerate(((-0.05, 0.15), (-0.1, 0.1), (-0.05, 0.05))):
            d.com_lo[c], d.com_hi[c] = lo, hi
    return d, keep


def make_engine(engine_factory, task, N, domain=False):
    return engine_factory(*substep_desc(task, N, domain))


def free_npcs(d):
    """root rows behind the robots that are free bodies"""
    return int(d.num_npcs) if d.npc_kind in (abi.NPC["ball"], abi.NPC["sheep"], abi.NPC["box"]) else 0


def joint_model(d):
    """(lower, upper, velocity limit, torque limit) of the 12 joints, float64"""
    r = d.robot
    return tuple(np.array([x[j] for j in range(12)], np.float64) for x in (r.dof_lower, r.dof_upper, r.dof_vel_limit, d.torque_limits))


# ---- states ------------------------------------------------------------------------------------------------------------------------------------
class State:
    """one seeded state of a grid: root [N, actors, 13], dof [N, ND, 2], actions [N A, 12] and the torques they mean [N, 12 A], float32"""

    def __init__(self, grid, seed, root, dof, actions, torques):
        self.grid, self.seed, self.root, self.dof, self.actions, self.torques = grid, seed, root, dof, actions, torques


def make_state(engine, grid, seed):
    """`engine`: any engine of the case's descriptor (it is reset; its reset state supplies x, y and the scenery's rows)"""
    place, s_qd, s_v, s_w, amp, _ = GRIDS[grid]
    d = engine.desc
    N, A, P = d.num_envs, d.num_agents, free_npcs(d)
    engine.reset_all()
    root = engine.tensor(abi.T_ROOT_STATE).cpu().numpy().copy()
    dof = engine.tensor(abi.T_DOF_STATE).cpu().numpy().copy()
    rs = np.random.RandomState(1000 * list(GRIDS).index(grid) + seed)
    lo, hi, _, tl = joint_model(d)
    n = A + P
    q4 = rs.standard_normal((N, n, 4))
    root[:, :n, 3:7] = q4 / np.linalg.norm(q4, axis=-1, keepdims=True)
    root[:, :n, 2] = LIFT_Z + APART * np.arange(n)
    root[:, :n, 7:10] = rs.standard_normal((N, n, 3)) * s_v
    root[:, :n, 10:13] = rs.standard_normal((N, n, 3)) * s_w
    u = rs.uniform(0.1, 0.9, (N, A, 12))
    a = rs.uniform(-amp, amp, (N, A, 12))
    if grid == "torque":
        a = np.where(rs.randint(0, 2, a.shape) == 1, 1.0, -1.0) * rs.uniform(0.4 * amp, amp, a.shape)
        lo_hi = np.tile(np.array(TORQUE_QD), (4, 1))
        qd = -np.sign(a) * rs.uniform(lo_hi[:, 0], lo_hi[:, 1], a.shape)
    elif place == "stops":
        side = rs.randint(0, 2, (N, A, 12))
        u = np.where(side == 1, 0.998, 0.002)
        qd = np.where(side == 1, 1.0, -1.0) * s_qd * rs.uniform(0.9, 1.1, (N, A, 12))
    else:
        qd = rs.standard_normal((N, A, 12)) * s_qd
    dof[:, :12 * A, 0] = (lo + u * (hi - lo)).reshape(N, 12 * A)
    dof[:, :12 * A, 1] = qd.reshape(N, 12 * A)
    a = (a / ACTION_SCALE).astype(np.float32).reshape(N * A, 12)
    assert np.abs(a).max() <= d.clip_actions, "the actions must pass the action clip unchanged"
    tl = tl.astype(np.float32)
    tau = np.clip(a * np.float32(d.action_scale), -tl, tl).astype(np.float32)
    if grid == "torque":
        assert (np.abs(tau) == tl).all(), "every torque of the `torque` grid sits on its limit"
    assert np.isfinite(root).all() and np.isfinite(dof).all()
    return State(grid, seed, root.astype(np.float32), dof.astype(np.float32), a, tau.reshape(N, 12 * A))


def run_substep(engine, st, fused):
    """write the state, run exactly one substep, -> (root, dof) after it as float32 numpy arrays"""
    engine.reset_all()
    engine.tensor(abi.T_ROOT_STATE).copy_(torch.from_numpy(st.root))
    engine.tensor(abi.T_DOF_STATE).copy_(torch.from_numpy(st.dof))
    if fused:
        engine.step_joint(to_dev(engine, st.actions))
        assert int(engine.tensor(abi.T_RESET_BUF).sum()) == 0, "the one-substep recipe must not reset anything"
    else:
        engine.tensor(abi.T_TORQUES).copy_(torch.from_numpy(st.torques))
        engine.simulate()
    return engine.tensor(abi.T_ROOT_STATE).cpu().numpy().copy(), engine.tensor(abi.T_DOF_STATE).cpu().numpy().copy()


def one_substep(engine_factory, task, N, grid, seed, *, fused):
    """a fresh engine of `task`, the seeded state of `grid`, one substep -> (desc, state, (root, dof))"""
    e = make_engine(engine_factory, task, N, GRIDS[grid][5])
    st = make_state(e, grid, seed)
    out = run_substep(e, st, fused)
    e.close()
    return e.desc, st, out


# ---- the limit pass, seen from outside --------------------------------------------------------------------------------------------------------------
def limit_bounds(d, st):
    """(lo, hi) [N, 12 A] of the limit pass in float64: the joint stops as a speed over one dt, cut at the velocity limit"""
    A, dt = d.num_agents, float(d.dt)
    lower, upper, vmax, _ = (np.tile(x, A) for x in joint_model(d))
    q = st.dof[:, :12 * A, 0].astype(np.float64)
    lo, hi = (lower - q) / dt, (upper - q) / dt
    return np.where(vmax > 0, np.maximum(lo, -vmax), lo), np.where(vmax > 0, np.minimum(hi, vmax), hi)


def bound_distance(d, st, dof):
    """-> (relative distance of every joint's velocity to its nearer bound [N, 12 A], negative beyond it; that bound's value)"""
    lo, hi = limit_bounds(d, st)
    v = dof[:, :12 * d.num_agents, 1].astype(np.float64)
    dl, dh = (v - lo) / np.abs(lo), (hi - v) / np.abs(hi)
    return np.minimum(dl, dh), np.where(dl <= dh, lo, hi)


def on_bound(d, st, dof):
    """[N, 12 A] bool: the joint's velocity sits on a bound of the limit pass"""
    return np.abs(bound_distance(d, st, dof)[0]) <= ON_TOL


def kept_envs(d, st, dof64):
    """the exclusion rule, from the float64 result alone: [N] bool.  Smooth grids: no joint within NEAR of a bound or beyond it.  Limit grids: all"""
    if st.grid in LIMIT:
        return np.ones(d.num_envs, bool)
    return ~(bound_distance(d, st, dof64)[0] <= NEAR).any(axis=1)


def good_seeds(e64, grid, count, fused, first=0, make=None, run=None, kept=None):
    """the first `count` seeds from `first` up whose float64 result stays within the exclusion cap -> [(state, float64 result, kept envs)].
    make(e64, grid, seed), run(e64, st, fused) and kept(d, st, float64 dof state) default to this module's free-flight ones
    (tests/contact_substep_ref.py passes its own: states in contact, a result with the contact forces, the contact list's stability added to the rule)"""
    d, out = e64.desc, []
    make, run, kept = make or make_state, run or run_substep, kept or kept_envs
    for seed in range(first, first + SEEDS_TRIED):
        st = make(e64, grid, seed)
        r64 = run(e64, st, fused)
        keep = kept(d, st, r64[1])
        if (~keep).sum() <= EXCLUDE_CAP * d.num_envs:
            out.append((st, r64, keep))
            if len(out) == count:
                return out
    raise AssertionError(f"{grid}: only {len(out)} of the seeds {first} .. {first + SEEDS_TRIED - 1} keep the float64 oracle within the exclusion cap")


# ---- metric ------------------------------------------------------------------------------------------------------------------------------------
def _half_ulp32(x):
    return 0.5 * float(np.spacing(np.float32(np.abs(x).max())))


def classes(d, st, root, dof, npc=True):
    """class -> float64 array [N, ...] of one result"""
    A, P, dt = d.num_agents, free_npcs(d) if npc else 0, float(d.dt)
    r, q = root.astype(np.float64), dof.astype(np.float64)
    out = {"qd": q[:, :12 * A, 1], "dq/dt": (q[:, :12 * A, 0] - st.dof[:, :12 * A, 0].astype(np.float64)) / dt,
           "w": r[:, :A, 10:13], "v": r[:, :A, 7:10], "quat": r[:, :A, 3:7], "pos": r[:, :A, 0:3]}
    if P:
        out.update({"npc_w": r[:, A:A + P, 10:13], "npc_v": r[:, A:A + P, 7:10], "npc_quat": r[:, A:A + P, 3:7], "npc_pos": r[:, A:A + P, 0:3]})
    return out


def errors(d, st, got, ref64, keep, npc=True):
    """-> (class -> max over the kept envs of |x - x_f64|, class -> floor)"""
    a, b = classes(d, st, *got, npc=npc), classes(d, st, *ref64, npc=npc)
    err = {k: np.abs(a[k] - b[k]) for k in b}
    fl = {k: _half_ulp32(b[k][keep]) for k in b}
    fl["dq/dt"] = _half_ulp32(ref64[1][keep][:, :12 * d.num_agents, 0]) / float(d.dt)
    if st.grid in LIMIT:        # the joints the float64 oracle left on a bound: against the bound's own value
        dist, bound = bound_distance(d, st, ref64[1])
        on = np.abs(dist) <= EXACT
        err["on"] = np.where(on, np.abs(a["qd"] - bound), 0.0)
        err["qd"] = np.where(on, 0.0, err["qd"])
        fl["on"] = _half_ulp32(bound[on]) if on.any() else 1.0
    return {k: float(e[keep].max()) for k, e in err.items()}, fl


def ratios(d, st, got, f32, ref64, keep, npc=True):
    """class -> err(engine) / max(err(f32 oracle), floor)"""
    (eg, fl), (ey, _) = errors(d, st, got, ref64, keep, npc), errors(d, st, f32, ref64, keep, npc)
    return {k: eg[k] / max(ey[k], fl[k]) for k in eg}


def check_on_set(d, st, got, ref64, what=""):
    """limit grids: the joints on a bound are the float64 oracle's, in every env where rounding cannot decide the side -> (joints on a bound, envs checked)"""
    dist = np.abs(bound_distance(d, st, ref64[1])[0])
    clear = ~((dist > ON_TOL / 10) & (dist < ON_TOL * 10)).any(axis=1)
    want, have = on_bound(d, st, ref64[1]), on_bound(d, st, got[1])
    diff = (want != have) & clear[:, None]
    assert not diff.any(), f"{what}: {int(diff.sum())} joints sit on a bound in one result and not in the other (first: env, joint {np.argwhere(diff)[0].tolist()})"
    return int(want[clear].sum()), int(clear.sum())
