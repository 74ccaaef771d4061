"""CPU: the one-substep bound IN CONTACT of tests/contact_substep_ref.py before any kernel meets it -- the exclusion cap on the float64 oracle alone, the
one-substep recipe on the oracle, KC_CPU as measured here (the float32 oracle and its -ffp-contract=fast build, oracle/Makefile `contract`), and the
power of the bound: descriptor defects (friction, max_depenetration_velocity, contact_offset) and the defect builds 5 .. 8 of the oracle
(oracle/Makefile `defects`: one wrong line of the contact solver each), every one of which must stand outside 2 KC_GPU where the correct build stands inside KC_GPU."""
import os
import subprocess

import numpy as np
import pytest

import contact_substep_ref as cr
import substep_ref as sr
from helpers import ROOT, oracle_engine

SOLVERS = ("pgs", "tgs")


def _f32(d, keep):
    return oracle_engine(d, keep)


def _build(target):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "-s", target])


def _lib_engine(lib, task, N, rand_friction=False):
    """the float32 oracle of another build (library selected through oracle_engine.load_library's MQE_ORACLE_LIB switch)"""
    with sr.under({"MQE_ORACLE_LIB": lib}):
        return cr.make_engine(_f32, task, N, rand_friction)


_MEASURED = {}


def measured():
    """per solver, host scene and grid: three good seeds, each with (state, float64 result, kept envs, float32 result, -ffp-contract=fast float32 result)"""
    if not _MEASURED:
        _build("contract")
        for solver in SOLVERS:
            for task, N, env, fused in sr.host_scenes():
                with sr.under(dict(env, MQE_SOLVER=solver)):
                    sc = cr.scene(task, N, solver, env)
                    for rf in (False, True):
                        e32, e32c = cr.make_engine(_f32, task, N, rf), _lib_engine("libmqe_oracle_contract.so", task, N, rf)
                        for grid in (g for g in cr.grids_of(sc.desc) if cr.GRIDS[g][6] == rf):
                            runs = [(st, r64, keep, cr.run_substep(e32, st, fused), cr.run_substep(e32c, st, fused)) for st, r64, keep in sc.good_seeds(grid, 3, fused)]
                            _MEASURED[(solver, task, N, tuple(env), fused, grid)] = (sc, runs)
                        e32.close(); e32c.close()
    return _MEASURED


def test_exclusion_cap_holds_on_the_float64_oracle_alone():
    """every solver, case and grid: three seeds among the first 20 keep the float64 result within the exclusion cap (no env of 16 or 33 whose contact list
    changes with contact_offset (1 -+ 1e-3), none with a joint within 1 % of a bound of the limit pass).  The states are what the grids say they are: off `pair` and `belly`
    every contact of a robot is one with the ground (normal vertical, no second actor); `belly` overflows the bounded list in the float64 oracle in at least a third of the envs
    (measured: 11 of 33 .. 16 of 16; 20 cm down a robot lies on 7 to 9 feature points against a share of 8, so every robot's share is full or one short of it); `pair`: every env has a contact between robots 0 and 1
    with its deepest separation in -6 .. -2 mm, and no contact with anything else; the float32 oracles count the same overflow as the float64 one"""
    print()
    for (solver, task, N, env, fused, grid), (sc, runs) in measured().items():
        A, rf = sc.desc.num_agents, cr.GRIDS[grid][6]
        for st, r64, keep, r32, r32c in runs:
            assert (~keep).sum() <= sr.EXCLUDE_CAP * N, (solver, task, grid, st.seed)
            assert np.array_equal(r32[3], r64[3]) and np.array_equal(r32c[3], r64[3]), (solver, task, grid, st.seed, "overflow")
            lists = cr.contact_lists(sc.e64(rf), st)
            for c in lists:
                two = cr.two_actor(c)
                if grid == "pair":
                    assert len(two) == len(c) > 0 and set(two[:, 0]) | set(two[:, 2]) == {0.0, 1.0}, (solver, task, st.seed, "pair: contacts between robots 0 and 1 only")
                    assert cr.PAIR_SD[0] <= two[:, 4].min() <= cr.PAIR_SD[1], (solver, task, st.seed, two[:, 4].min())
                elif grid != "belly":      # 20 cm down a robot on the bridge meets the deck's sides too
                    rob = c[c[:, 0] < A]
                    assert len(rob) > 0 and (rob[:, 2] < 0).all() and (np.abs(rob[:, 7]) > 0.99).all(), (solver, task, grid, st.seed, "a robot's contacts are with the ground")
            if grid == "belly":
                assert (r64[3] > 0).sum() >= N / 3 and min(map(len, lists)) >= 7 * A, (solver, task, st.seed, "belly must overflow the bounded list")
        ovf = runs[0][1][3]
        print(f"    {solver} {task:22s} N={N:3d} {'fused' if fused else 'simulate'} {' '.join(env) or '-':20s} {grid:9s} seeds {[r[0].seed for r in runs]}  contacts {min(map(len, lists))} .. {max(map(len, lists))}  envs in overflow {int((ovf > 0).sum())}")


def test_one_substep_recipe_on_the_oracle(solver):
    """step_joint under the recipe's descriptor IS one simulate() with the clipped torques, in contact too: same bits in root state, dof state, contact forces
    and overflow count (the float32 oracle, seed 0 of `stick` and `deep`); in a flock the sheep's script rewrites the sheep's rows, the robots' rows keep the
    substep's bits"""
    for task in ("go1gate", "go1plane", "go1football-defender", "go1football-2vs2", "go1seesaw", "go1pushbox", "go1sheep-hard"):
        sc = cr.scene(task, 8, solver)
        e = cr.make_engine(_f32, task, 8)
        A = e.desc.num_agents
        for grid in ("stick", "deep"):
            st = cr.make_state(sc, grid, 0)
            f, u = cr.run_substep(e, st, True), cr.run_substep(e, st, False)
            assert not np.array_equal(u[1], st.dof) and np.abs(u[2]).max() > 0, (task, grid)
            rows = slice(0, A) if task == "go1sheep-hard" else slice(None)
            assert np.array_equal(f[0][:, rows].view(np.int32), u[0][:, rows].view(np.int32)), (task, grid, "root")
            for k, what in ((1, "dof"), (2, "contact force"), (3, "overflow")):
                assert np.array_equal(f[k].view(np.int32), u[k].view(np.int32)), (task, grid, what)
        e.close()


def test_kc_cpu_is_the_measured_constant():
    """KC_CPU: the float32 oracle's largest ratio against itself across seeds (the second and third good seed against the first one's yardstick) over every
    solver, host scene and grid, and the same for its -ffp-contract=fast build against the same yardstick (all three seeds: another rounding of the same state)"""
    print("\n    solver / case / grid: worst ratio of seeds 2, 3 against seed 1's yardstick (class) | -ffp-contract=fast build, seeds 1, 2, 3 (class)")
    worst, per_grid, where = 0.0, {}, None
    for (solver, task, N, env, fused, grid), (sc, runs) in measured().items():
        d, npc = sc.desc, not (task == "go1sheep-hard" and fused)        # the sheep's script rewrites the sheep's rows after a fused step
        st0, r64, keep, r32, _ = runs[0]
        e0, fl0 = cr.errors(d, st0, r32, r64, keep, npc)
        yard = {k: max(e0[k], fl0[k]) for k in e0}
        k_own, c_own, k_fma, c_fma = 0.0, "-", 0.0, "-"
        for i, (st, r64, keep, r32, r32c) in enumerate(runs):
            e, _ = cr.errors(d, st, r32, r64, keep, npc)
            ec, _ = cr.errors(d, st, r32c, r64, keep, npc)
            for k in e:
                if i > 0 and e[k] / yard[k] > k_own:
                    k_own, c_own = e[k] / yard[k], k
                if ec[k] / yard[k] > k_fma:
                    k_fma, c_fma = ec[k] / yard[k], k
        k_here = max(k_own, k_fma)
        per_grid[(solver, grid)] = max(per_grid.get((solver, grid), 0.0), k_here)
        if k_here > worst:
            worst, where = k_here, (solver, task, N, grid, c_own if k_own >= k_fma else c_fma + ", -ffp-contract=fast")
        print(f"    {solver} {task:22s} N={N:3d} {'fused' if fused else 'simulate'} {' '.join(env) or '-':20s} {grid:9s} {k_own:6.2f} ({c_own:8s}) | {k_fma:6.2f} ({c_fma})")
    for solver in SOLVERS:
        print(f"    per grid, {solver}: " + "  ".join(f"{g} {v:.2f}" for (s, g), v in per_grid.items() if s == solver))
    print(f"    worst {worst:.3f} {where}  ->  KC_CPU = {cr.KC_CPU}, KC_GPU = {cr.KC_GPU}")
    assert worst <= cr.KC_CPU, worst
    assert worst > cr.KC_CPU / 2, "KC_CPU is not the measured constant any more: measure it again (contact_substep_ref.py)"
    assert cr.KC_GPU == 4 * cr.KC_CPU


def _yardstick(sc, task, N, grid):
    """first good seed of a grid: (state, float64 result, kept envs, float32 result, yardstick per class), and the correct build's worst ratio on the NEXT good seed"""
    rf = cr.GRIDS[grid][6]
    e32 = cr.make_engine(_f32, task, N, rf)
    (st, r64, keep), (st1, r64b, keep1) = sc.good_seeds(grid, 2, True)
    r32 = cr.run_substep(e32, st, True)
    e0, fl = cr.errors(sc.desc, st, r32, r64, keep)
    yard = {k: max(e0[k], fl[k]) for k in e0}
    e1, _ = cr.errors(sc.desc, st1, cr.run_substep(e32, st1, True), r64b, keep1)
    e32.close()
    return (st, r64, keep, r32), max(e1[k] / yard[k] for k in e1)


def _fmt(r):
    return "  ".join(f"{k} {v:.3g}" for k, v in r.items() if not k.startswith("npc"))


#                    descriptor field,             factor, grids on which it must stand outside 2 KC_GPU, grids on which it must stay inside KC_GPU
DESC_DEFECTS = [("friction",                   0.99, ("stick", "slide", "closing"), ()),
                ("max_depenetration_velocity", 0.99, ("deep", "belly"),             ("stick",)),
                ("contact_offset",             0.5,  (),                            ("stick",))]


@pytest.mark.parametrize("task,N", [("go1gate", 16), ("go1football-2vs2", 16)])
def test_descriptor_defects_stand_outside_the_bound(solver, task, N):
    """a float32 oracle whose descriptor is wrong by 1 %: friction on `stick`, `slide` and `closing`, the push-out cap on `deep` and `belly` -- and NOT on `stick`, which
    never reaches the cap; half the contact margin changes nothing on `stick`, where every foot touches"""
    sc = cr.scene(task, N, solver)
    print()
    for field, factor, outside, inside in DESC_DEFECTS:
        for grid in outside + inside:
            (st, r64, keep, r32), own = _yardstick(sc, task, N, grid)
            assert own <= cr.KC_GPU, (grid, own)
            ed = cr.make_engine(_f32, task, N, cr.GRIDS[grid][6], **{field: factor})
            r = cr.ratios(sc.desc, st, cr.run_substep(ed, st, True), r32, r64, keep)
            ed.close()
            print(f"    {solver} {task:18s} {grid:9s} {field} x {factor}: {_fmt(r)}   (correct build, next seed: {own:.2f})")
            if grid in outside:
                assert max(r.values()) > 2 * cr.KC_GPU, (field, grid, r)
            else:
                assert max(r.values()) <= cr.KC_GPU, (field, grid, r)


#          n: (what, solvers it exists in, named grids)
DEFECTS = {5: ("temporal separation without the accumulated motion", ("tgs",), ("closing", "shallow", "deep")),
           6: ("voff left out of the quaternion integration", ("tgs",), ("deep", "belly")),
           7: ("second tangent row bounded by the first row's impulse", SOLVERS, ("slide", "friction")),
           8: ("two-actor rows without the second actor's angular part", SOLVERS, ("pair",))}


@pytest.mark.parametrize("task,N", [("go1gate", 16), ("go1football-2vs2", 16)])
def test_every_defect_build_stands_outside_the_bound(solver, task, N):
    """each defect build of the contact solver exceeds 2 KC_GPU in at least one class on at least one of its named grids, where the correct float32 oracle on the
    next good seed, against the same yardstick, exceeds KC_GPU in none.  Defects 5 and 6 are lines of the temporal solver and do not exist under the other"""
    _build("defects")
    sc = cr.scene(task, N, solver)
    print()
    for n, (what, solvers, grids) in DEFECTS.items():
        if solver not in solvers:
            continue
        best = 0.0
        for grid in grids:
            (st, r64, keep, r32), own = _yardstick(sc, task, N, grid)
            assert own <= cr.KC_GPU, (grid, own)
            ed = _lib_engine(f"libmqe_oracle_defect{n}.so", task, N, cr.GRIDS[grid][6])
            r = cr.ratios(sc.desc, st, cr.run_substep(ed, st, True), r32, r64, keep)
            ed.close()
            best = max(best, max(r.values()))
            print(f"    {solver} {task:18s} {grid:9s} defect {n} ({what}): {_fmt(r)}   (correct build, next seed: {own:.2f})")
        assert best > 2 * cr.KC_GPU, (n, what, best)
