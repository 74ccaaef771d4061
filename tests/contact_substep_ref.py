"""Host side of the one-substep tests IN CONTACT (tests/test_contact_substep_ref.py on the CPU, tests/test_contact_substep_gpu.py on the GPU): the contact
analogue of tests/substep_ref.py, built on it -- State, run_substep, substep_desc, classes and errors, the NEAR rule, good_seeds, CASES, under and host_scenes are
that module's; `ratios` here is its three lines over this module's errors().

WHY.  For a FIXED contact list a substep is as continuous a function of the state as in free flight: the normal rows, the friction box, the temporal
solver's re-evaluated separations, its push-out cap and voff are projections and sums.  So the free-flight machinery carries over: every env is held,
no absolute tolerance, the float32 oracle's own error against float64 is the yardstick.

BASE STATES.  Per (task, N, solver) the float64 oracle settles the scene under the PD law of tests/contact_rich.py (control type P, kp 40, kd 1) towards
joint targets SETTLE_AMP = +-0.15 rad around the default stance, seeded per robot, for SETTLE_STEPS = 160 substeps from the reset pose at rest.  The state
tensors are float32, so the result is one float32 state that goes to every engine.  Free NPCs (ball, box, sheep) settle with it and stay where they came to
rest.  The substep under test runs under substep_ref.substep_desc (control T, decimation 1, no termination, self_collision = 0).

THE GRIDS.  (name: sigma(v) m/s, sigma(w) rad/s, sigma(qd) rad/s, torque amplitude N m, vertical shift m, vertical speed m/s, randomised friction, pair)
on the base state, seeded.
    stick     friction below its bound                                  slide     every foot on the friction box (1.5 m/s)
    closing   +3 mm, -1.5 m/s: a gap that closes inside the substep     shallow   -0.5 mm: push-out below the 1 m/s cap
    deep      -30 mm: push-out on the cap, and voff                     belly     -200 mm: more feature points per robot than the bounded list keeps
    friction  `slide` with rand_friction, 0.3 .. 1.2: the per-env bucket and the averaged coefficient
    pair      the two-actor coupling blocks alone: every robot and free NPC stacked from z = 50 m up as substep_ref.make_state does, robot 1 at robot 0's
              height, 0.07 +- 0.03 m ahead of it (seeded), brought towards it along y by bisection on the float64 oracle's debug_dynamics list until the env's deepest
              two-actor separation lies in -6 .. -2 mm; the two close in at 0.5 m/s; nothing touches the ground.  Run on every row with two robots or
              more; SH_A1 (go1plane) has one robot and no two-actor block.
`belly`: MQE_T_CONTACT_OVERFLOW is positive in the float64 oracle in a third of the envs or more (11 of 33 .. 16 of 16: a robot lies on 7 to 9 points against a
share of 8), and on every grid it must be equal in every engine.

THE METRIC is substep_ref's (six robot classes, four NPC classes, half-ulp floors) plus the class `cf`: MQE_T_CONTACT_FORCE, all reported bodies, floor
half a float32 ulp of the largest |cf_f64| kept.
EXCLUSION, from the float64 oracle alone: an env is left out if the id columns of its float64 debug_dynamics contact list differ between
contact_offset (1 - 1e-3) and contact_offset (1 + 1e-3), or if substep_ref's NEAR rule on the joint-limit pass fires.  At most EXCLUDE_CAP = 2 % -- with
16 or 33 envs: none -- and substep_ref.good_seeds picks the seeds.

THE CONSTANTS.  KC_CPU is measured on the CPU as K_CPU is: the float32 oracle's worst class ratio on the second and third good seed against the first
one's yardstick, over all host scenes of CASES, all grids, both solvers -- and the same with the float32 oracle built with -ffp-contract=fast
(oracle/Makefile `contract`; every other build has it off): a CPU-side reading of what a legitimate change of rounding costs, the kernel solving in contact
space with CRBA + Schur where the oracle solves in velocity space with Cholesky.  KC_GPU = 4 KC_CPU (policy_ref.py's rule).  Nothing a kernel
computes enters either constant.
Measured with `python -m pytest tests/test_contact_substep_ref.py -s` (prints every solver, case and grid).  Worst ratio per grid over the 14 host scenes of
CASES (16 and 33 envs), the correct build across seeds and the -ffp-contract=fast build together:
    projected Gauss-Seidel   stick 2.09  slide 2.50  closing 2.00  shallow 2.86  deep 2.08  belly 2.06  pair 10.95  friction 2.67
    temporal Gauss-Seidel    stick 7.94  slide 8.55  closing 2.57  shallow 9.32  deep 2.28  belly 3.28  pair  4.01  friction 2.89
KC_CPU = 11.0 is the maximum, 10.95 (go1revolvingdoor, 16 envs, projected Gauss-Seidel, `pair`, class v), rounded up; KC_GPU = 44.  The ratios above 3.5 are
`pair` under the velocity-level solver (3.9 .. 10.95: an env's two to ten contacts between two free-floating robots, the largest float32 error of 16 envs differs
that much from draw to draw) and `stick` / `slide` / `shallow` under the temporal solver (6.4 .. 9.3, where a float32 error in a re-evaluated separation enters the
next sub-step's bias divided by dt / 4); the contracted build stays within 1.5 x the correct build's own reading on every row (worst: 9.32 against 7.65).

WALLS.  A robot whose calf comes to rest against the wall behind the start block (it happens: one env of 16 in go1pushbox and in go1seesaw) is placed 0.3 m further
along the contact's normal and the scene settles again: with that wall contact the float32 oracle's own error in that env was 40 x the other envs', and walls
belong to the parity tests.  tests/test_contact_substep_ref.py asserts that off `pair` and `belly` every contact of a robot is one with the ground.

THE POWER OF THE BOUND (16 envs, first good seed; ratio per class qd / (q' - q)/dt / w / v / quat / pos / cf; go1gate, projected | temporal Gauss-Seidel;
2 KC_GPU = 88):
    friction x 0.99                    stick     1170  1440   466  1060    79   10  1270 |   2410    929    828   2120    59    7   5140
                                       slide     2950  3110  2160  1140   629   34  4910 |   1860   1780   4700   1340   691   36   4130
                                       closing    745   758   383   582    70    9  1190 |    347    231    497    437    37    3    607
    max_depenetration_velocity x 0.99  deep      6740  4580   923  1530   460   16  9520 |   9530   3860   1360   1110   235   15   6350
                                       belly     8820  5820  6550 12100  2600  226 14400 |   4210   4200   4110  14700  1440  312  10500
                                       stick     1 in every class (the cap is never reached), and so is contact_offset x 0.5 (every foot touches)
    defect 5  temporal separation without the accumulated motion    closing   - | 136000 202000 179000  98300 28000  949 122000   shallow - | 86700 49100 81100 47400 6630 381 115000
                                                                    deep      - | 1 in every class: 30 mm deep the bias sits on the cap in every sub-step
    defect 6  voff left out of the quaternion integration           deep      - | quat 628, every other class 1                    belly   - | quat 34900
    defect 7  second tangent row bounded by the first row's impulse slide     130000 138000 17700 16500 5150 495 207000 | 52900 72700 28400 15900 4720 522 144000
                                                                    friction  108000 111000  3930 30400 2280 456 189000 | 108000 156000 8870 25700 1270 514 300000
    defect 8  two-actor rows without the second actor's angular part pair      5660 5750 9070 3200 9120 332 3060 | 784 2570 2970 1180 4280 600 1150
go1football-2vs2: the weakest outside reading is 534 (friction x 0.99 on `stick`, temporal solver), 6 x the 88.  The correct build on the next good seed against the same
yardstick: at most 10.9 (`pair`, go1gate, projected Gauss-Seidel), then 6.4 (`stick`, go1gate, temporal) and 2.3 or less on every other grid.

ON THE MI355X (tests/test_contact_substep_gpu.py, both solvers, 18 cases): no class of any shape row is outside KC_GPU; worst ratio per grid
    projected Gauss-Seidel   stick 1.50  slide 2.00  closing 1.44  shallow 2.00  deep 2.00  belly 2.00  pair 3.81  friction 2.00
    temporal Gauss-Seidel    stick 2.66  slide 2.00  closing 2.00  shallow 6.38  deep 2.00  belly 3.08  pair 1.03  friction 2.00
and per shape row in profiles/contact_substep.txt; MQE_T_CONTACT_OVERFLOW equal in every env of every grid.  Nothing in the kernel was changed.
"""
import os

import numpy as np
import torch

import substep_ref as sr
from helpers import oracle_engine
from mqe.engine import abi

#           sigma(v), sigma(w), sigma(qd), torque amplitude, vertical shift, vertical speed, rand_friction, pair
GRIDS = {"stick":    (0.1, 0.3, 1.0, 10.0, 0.0,     0.0,  False, False),
         "slide":    (1.5, 0.5, 1.0, 10.0, 0.0,     0.0,  False, False),
         "closing":  (0.1, 0.3, 1.0, 10.0, 3e-3,    -1.5, False, False),
         "shallow":  (0.1, 0.3, 1.0, 10.0, -0.5e-3, 0.0,  False, False),
         "deep":     (0.1, 0.3, 1.0, 10.0, -30e-3,  0.0,  False, False),
         "belly":    (0.1, 0.3, 1.0, 10.0, -200e-3, 0.0,  False, False),
         "friction": (1.5, 0.5, 1.0, 10.0, 0.0,     0.0,  True,  False),
         "pair":     (0.1, 0.3, 1.0, 10.0, 0.0,     0.0,  False, True)}
FRICTION_LO, FRICTION_HI = 0.3, 1.2
SETTLE_KP, SETTLE_KD, SETTLE_AMP, SETTLE_STEPS, SETTLE_SEED = 40.0, 1.0, 0.15, 160, 777
SETTLE_TRIES, WALL_CLEAR = 4, 0.3
OFFSET_BAND = 1e-3                       # the exclusion rule's relative change of contact_offset
PAIR_X, PAIR_JITTER, PAIR_SPEED, PAIR_SD = 0.07, 0.03, 0.5, (-6e-3, -2e-3)
PAIR_GAP = (0.05, 1.0)                   # bisection bracket of robot 1's y offset: overlapping trunks .. out of reach

KC_CPU = 11.0                    # measured 10.95 (go1revolvingdoor, 16 envs, projected Gauss-Seidel, `pair`, class v), rounded up; see the table above
KC_GPU = 4 * KC_CPU


def grids_of(d):
    """the grids a descriptor's scene takes: `pair` needs two robots"""
    return [g for g in GRIDS if not GRIDS[g][7] or d.num_agents >= 2]


def _f64(d, keep):
    return oracle_engine(d, keep, f64=True)


# ---- descriptors -----------------------------------------------------------------------------------------------------------------------------
_DESCS = {}


def _substep_desc(task, N):
    """a copy of substep_ref.substep_desc(task, N) under the switches now in force; the scene behind it (terrain, maps: seconds for a flock's track) is built once"""
    key = (task, N, tuple(sorted((k, v) for k, v in os.environ.items() if k.startswith("MQE_") and k not in ("MQE_VERBOSE", "MQE_ORACLE_LIB"))))
    if key not in _DESCS:
        _DESCS[key] = sr.substep_desc(task, N)
    d, keep = _DESCS[key]
    return type(d).from_buffer_copy(d), keep


def contact_desc(task, N, rand_friction=False, offset_scale=1.0):
    d, keep = _substep_desc(task, N)
    if rand_friction:
        d.rand_friction, d.friction_lo, d.friction_hi = 1, FRICTION_LO, FRICTION_HI
    d.contact_offset = d.contact_offset * offset_scale
    return d, keep


def make_engine(engine_factory, task, N, rand_friction=False, **change):
    """an engine of the substep's descriptor; `change`: descriptor fields multiplied by a factor (the descriptor defects of the CPU test)"""
    d, keep = contact_desc(task, N, rand_friction)
    for k, f in change.items():
        setattr(d, k, getattr(d, k) * f)
    return engine_factory(d, keep)


def settle(task, N):
    """-> (root, dof) float32: the scene after SETTLE_STEPS substeps of the float64 oracle under PD control, from the reset pose at rest.
    Walls are not this test's matter (tests/test_gpu_parity.py has them): a robot that comes to rest with a one-sided contact whose normal is not
    vertical -- a calf against the wall behind the start block -- starts WALL_CLEAR further along that normal and the scene settles again."""
    d, keep = _substep_desc(task, N)
    d.control_type, d.kp, d.kd, d.action_scale = abi.CTRL["P"], SETTLE_KP, SETTLE_KD, 1.0
    N, A = d.num_envs, d.num_agents
    target = np.random.RandomState(SETTLE_SEED).uniform(-SETTLE_AMP, SETTLE_AMP, (N, 12 * A)).astype(np.float32)
    shift = np.zeros((N, A, 2), np.float32)
    for _ in range(SETTLE_TRIES):
        e = _f64(d, keep)          # a fresh engine: the reset draws x, y from the env's reset count
        e.reset_all()
        root, dof = e.tensor(abi.T_ROOT_STATE), e.tensor(abi.T_DOF_STATE)
        dof[:, :12 * A, 0] = torch.tensor([d.default_dof_pos[j] for j in range(12)] * A)
        dof[..., 1] = 0
        root[..., 7:] = 0
        root[:, :A, :2] += torch.from_numpy(shift)
        e.tensor(abi.T_ACTIONS).copy_(torch.from_numpy(target).reshape(e.tensor(abi.T_ACTIONS).shape))
        for _ in range(SETTLE_STEPS):
            e.compute_torques()
            e.simulate()
        walls = [(env, int(c[0]), c[5:7]) for env in range(N) for c in e.debug_dynamics(env, 0)[2] if c[0] < A and c[2] < 0 and abs(c[7]) < 0.99]
        out = root.numpy().copy(), dof.numpy().copy()
        e.close()
        if not walls:
            break
        for env, r, n in walls:
            shift[env, r] += WALL_CLEAR * n / np.linalg.norm(n) / sum(1 for w in walls if w[:2] == (env, r))
    else:
        raise AssertionError(f"{task}: robots still rest against a wall after {SETTLE_TRIES} placements: {[(w[0], w[1]) for w in walls]}")
    assert np.isfinite(out[0]).all() and np.isfinite(out[1]).all()
    return out


class Scene:
    """the float64 side of one (task, N) under the switches in force when it is built: the settled base state, the float64 oracle of the substep's
    descriptor (with and without randomised friction), and for the exclusion rule the same with contact_offset (1 -+ OFFSET_BAND).
    good_seeds(grid, ..) -> [(state, float64 result, kept envs)] as substep_ref.good_seeds gives them"""

    def __init__(self, task, N):
        self.task, self.N = task, N
        self.base = settle(task, N)
        self._e = {}
        self.desc = self.e64(False).desc
        self._pairs = {}

    def e64(self, rand_friction, offset_scale=1.0):
        key = (bool(rand_friction), offset_scale)
        if key not in self._e:
            self._e[key] = _f64(*contact_desc(self.task, self.N, rand_friction, offset_scale))
        return self._e[key]

    def good_seeds(self, grid, count, fused, first=0):
        return sr.good_seeds(self.e64(GRIDS[grid][6]), grid, count, fused, first,
                             make=lambda e, g, seed: make_state(self, g, seed), run=run_substep,
                             kept=lambda d, st, dof64: kept_envs(self, st, dof64))


_SCENES = {}


def scene(task, N, solver, env=()):
    """the Scene of a case, built once per (task, N, solver, switches the oracle reads) and shared; call it under those switches"""
    key = (task, N, solver, tuple(sorted(dict(env).items())))
    if key not in _SCENES:
        _SCENES[key] = Scene(task, N)
    return _SCENES[key]


# ---- contact lists ------------------------------------------------------------------------------------------------------------------------------
def contact_lists(e, st):
    """the engine's debug_dynamics contact list of every env at the state's pose: [N] arrays [nc, 8] (actor A, body A, actor B, body B, sd, normal)"""
    e.reset_all()
    e.tensor(abi.T_ROOT_STATE).copy_(torch.from_numpy(st.root))
    e.tensor(abi.T_DOF_STATE).copy_(torch.from_numpy(st.dof))
    return [np.array(e.debug_dynamics(env, 0)[2], np.float64) for env in range(e.desc.num_envs)]


def two_actor(con):
    """rows of a contact list between two actors (actor B >= 0, another one than actor A)"""
    return con[(con[:, 2] >= 0) & (con[:, 2] != con[:, 0])] if len(con) else con


def kept_envs(sc, st, dof64):
    """the exclusion rule, from the float64 oracle alone: [N] bool"""
    rf = GRIDS[st.grid][6]
    lo, hi = (contact_lists(sc.e64(rf, s), st) for s in (1 - OFFSET_BAND, 1 + OFFSET_BAND))
    same = np.array([a.shape == b.shape and np.array_equal(a[:, :4], b[:, :4]) for a, b in zip(lo, hi)])
    return same & sr.kept_envs(sc.desc, st, dof64)


# ---- states ---------------------------------------------------------------------------------------------------------------------------------------
def _pair_placement(sc, root, dof, ahead):
    """root with every robot and free NPC stacked from LIFT_Z up, robot 1 `ahead` [N] of robot 0 and beside it at the y offset the bisection finds per env"""
    d, N = sc.desc, sc.N
    n = d.num_agents + sr.free_npcs(d)
    root = root.copy()
    root[:, :n, 2] = sr.LIFT_Z + sr.APART * np.arange(n)
    root[:, 1, 2] = root[:, 0, 2]
    root[:, 1, 0] = (root[:, 0, 0] + ahead).astype(np.float32)
    e = sc.e64(False)
    lo, hi = np.full(N, PAIR_GAP[0]), np.full(N, PAIR_GAP[1])
    probe = sr.State("pair", -1, root, dof, None, None)
    for _ in range(40):
        gap = 0.5 * (lo + hi)
        root[:, 1, 1] = (root[:, 0, 1] + gap).astype(np.float32)
        lists = contact_lists(e, probe)
        deepest = np.array([two_actor(c)[:, 4].min() if len(two_actor(c)) else np.inf for c in lists])
        inside, deep = (deepest >= PAIR_SD[0]) & (deepest <= PAIR_SD[1]), deepest < PAIR_SD[0]
        if inside.all():
            return root
        lo, hi = np.where(inside | deep, gap, lo), np.where(inside | ~deep, gap, hi)      # an env inside the window keeps its offset
    raise AssertionError(f"pair: the bisection left envs {np.flatnonzero(~inside).tolist()} outside {PAIR_SD} (deepest separations {deepest})")


def make_state(sc, grid, seed):
    s_v, s_w, s_qd, amp, dz, vz, _, pair = GRIDS[grid]
    d = sc.desc
    N, A = d.num_envs, d.num_agents
    root, dof = sc.base[0].copy(), sc.base[1].copy()
    rs = np.random.RandomState(100000 + 1000 * list(GRIDS).index(grid) + seed)
    if pair:
        ahead = PAIR_X + rs.uniform(-PAIR_JITTER, PAIR_JITTER, N)      # the placement is the seed's too: another seed, other pairs of feature points in reach
        if seed not in sc._pairs:
            sc._pairs[seed] = _pair_placement(sc, root, dof, ahead)
        root = sc._pairs[seed].copy()
    root[:, :A, 2] += np.float32(dz)
    v = rs.standard_normal((N, A, 3)) * s_v
    v[..., 2] += vz
    if pair:
        v[:, 0, 1] += 0.5 * PAIR_SPEED
        v[:, 1, 1] -= 0.5 * PAIR_SPEED
    root[:, :A, 7:10] = v
    root[:, :A, 10:13] = rs.standard_normal((N, A, 3)) * s_w
    dof[:, :12 * A, 1] = rs.standard_normal((N, 12 * A)) * s_qd
    a = (rs.uniform(-amp, amp, (N * A, 12)) / sr.ACTION_SCALE).astype(np.float32)
    assert np.abs(a).max() <= d.clip_actions, "the actions must pass the action clip unchanged"
    tl = sr.joint_model(d)[3].astype(np.float32)
    tau = np.clip(a * np.float32(d.action_scale), -tl, tl).astype(np.float32)
    return sr.State(grid, seed, root.astype(np.float32), dof.astype(np.float32), a, tau.reshape(N, 12 * A))


def run_substep(engine, st, fused):
    """substep_ref.run_substep with the contact side of the result: -> (root, dof, contact forces [N, ..], overflow count [N] of this substep)"""
    engine.tensor(abi.T_CONTACT_OVERFLOW).zero_()
    root, dof = sr.run_substep(engine, st, fused)
    return root, dof, engine.tensor(abi.T_CONTACT_FORCE).cpu().numpy().copy().reshape(root.shape[0], -1), engine.tensor(abi.T_CONTACT_OVERFLOW).cpu().numpy().copy()


# ---- metric -----------------------------------------------------------------------------------------------------------------------------------------
def errors(d, st, got, ref64, keep, npc=True):
    """substep_ref.errors plus the class `cf` -> (class -> max over the kept envs of |x - x_f64|, class -> floor)"""
    err, fl = sr.errors(d, st, got[:2], ref64[:2], keep, npc)
    c64 = ref64[2].astype(np.float64)
    err["cf"] = float(np.abs(got[2].astype(np.float64) - c64)[keep].max())
    fl["cf"] = sr._half_ulp32(c64[keep])
    return err, fl


def ratios(d, st, got, f32, ref64, keep, npc=True):
    """class -> err(engine) / max(err(f32 oracle), floor)"""
    (eg, fl), (ey, _) = errors(d, st, got, ref64, keep, npc), errors(d, st, f32, ref64, keep, npc)
    return {k: eg[k] / max(ey[k], fl[k]) for k in eg}
