"""CPU: the fast-free-flight bound of tests/substep_ref.py before any kernel meets it -- the exclusion cap on the float64 oracle alone, the one-substep
recipe on the oracle, K_CPU as measured here, and the defect builds of the oracle (oracle/Makefile `defects`: one wrong velocity-product line each),
every one of which must stand outside 2 K_GPU where the correct build stands inside."""
import os
import subprocess

import numpy as np
import pytest

import substep_ref as sr
from helpers import ROOT, oracle_engine


def _f32(d, keep):
    return oracle_engine(d, keep)


def _f64(d, keep):
    return oracle_engine(d, keep, f64=True)


_MEASURED = {}


def measured():
    """per host scene and grid: three good seeds, each with (state, float64 result, kept envs, float32 result); computed once for the module"""
    if not _MEASURED:
        for task, N, env, fused in sr.host_scenes():
            with sr.under(env):
                for domain in (False, True):
                    e32, e64 = sr.make_engine(_f32, task, N, domain), sr.make_engine(_f64, task, N, domain)
                    for grid in sr.GRIDS:
                        if sr.GRIDS[grid][5] != domain:
                            continue
                        runs = [(st, r64, keep, sr.run_substep(e32, st, fused)) for st, r64, keep in sr.good_seeds(e64, grid, 3, fused)]
                        _MEASURED[(task, N, tuple(env), fused, grid)] = (e32.desc, runs)
                    e32.close(); e64.close()
    return _MEASURED


def test_exclusion_cap_holds_on_the_float64_oracle_alone():
    """every case, every grid: three seeds among the first 20 keep the float64 result within the exclusion cap (smooth grids: no env of 16 or 33
    has a joint within 1 % of a bound of the limit pass); on the limit grids the pass is active in every env and leaves at least a twentieth of all joints on either bound"""
    print()
    for (task, N, env, fused, grid), (d, runs) in measured().items():
        seeds = [st.seed for st, _, _, _ in runs]
        for st, r64, keep, _ in runs:
            assert (~keep).sum() <= sr.EXCLUDE_CAP * N, (task, grid, st.seed)
            if grid in sr.LIMIT:
                lo, hi = sr.limit_bounds(d, st)
                v, on = r64[1][:, :12 * d.num_agents, 1], sr.on_bound(d, st, r64[1])
                at_lo, at_hi = on & (np.abs(v - lo) < np.abs(v - hi)), on & (np.abs(v - lo) >= np.abs(v - hi))
                assert at_lo.mean() >= 0.05 and at_hi.mean() >= 0.05 and on.any(axis=1).all(), (task, grid, st.seed, "a limit grid must leave a twentieth of the joints on either bound")
        print(f"    {task:22s} N={N:3d} {'fused' if fused else 'simulate'} {' '.join(env) or '-':20s} {grid:10s} seeds {seeds}")


def test_one_substep_recipe_on_the_oracle():
    """step_joint under the recipe's descriptor IS one simulate() with the clipped torques: same bits in root and dof state (the float32 oracle, seed 0 of
    `spin` and `torque`); in a flock the sheep's script rewrites the sheep's rows, the robots' rows keep the substep's bits"""
    for task in ("go1gate", "go1plane", "go1football-defender", "go1football-2vs2", "go1seesaw", "go1pushbox", "go1sheep-hard"):
        e = sr.make_engine(_f32, task, 8)
        A = e.desc.num_agents
        for grid in ("spin", "torque"):
            st = sr.make_state(e, grid, 0)
            (rf, qf), (ru, qu) = sr.run_substep(e, st, True), sr.run_substep(e, st, False)
            assert not np.array_equal(qu, st.dof) and np.array_equal(qf.view(np.int32), qu.view(np.int32)), (task, grid)
            rows = slice(0, A) if task == "go1sheep-hard" else slice(None)
            assert np.array_equal(rf[:, rows].view(np.int32), ru[:, rows].view(np.int32)), (task, grid)
        e.close()


def test_k_cpu_is_the_measured_constant():
    """K_CPU: the float32 oracle's largest ratio against itself across seeds (the second and third good seed against the first one's yardstick), over every
    case and grid; and the float32 oracle passes the limit grids' set check against the float64 one"""
    print("\n    case / grid: worst ratio of seeds 2, 3 against seed 1's yardstick (class)")
    worst, per_grid = 0.0, {}
    for (task, N, env, fused, grid), (d, runs) in measured().items():
        npc = not (task == "go1sheep-hard" and fused)        # the sheep's script rewrites the sheep's rows after a fused step
        st0, r64, keep, r32 = runs[0]
        e0, fl0 = sr.errors(d, st0, r32, r64, keep, npc)
        yard = {k: max(e0[k], fl0[k]) for k in e0}
        k_here, cls = 0.0, "-"
        for st, r64, keep, r32 in runs:
            if grid in sr.LIMIT:
                sr.check_on_set(d, st, r32, r64, what=f"{task} {grid} seed {st.seed} f32 oracle")
            e, _ = sr.errors(d, st, r32, r64, keep, npc)
            for k in e:
                if e[k] / yard[k] > k_here:
                    k_here, cls = e[k] / yard[k], k
        per_grid[grid] = max(per_grid.get(grid, 0.0), k_here)
        worst = max(worst, k_here)
        print(f"    {task:22s} N={N:3d} {'fused' if fused else 'simulate'} {grid:10s} {k_here:6.2f} ({cls})")
    print("    per grid: " + "  ".join(f"{g} {v:.2f}" for g, v in per_grid.items()))
    print(f"    worst {worst:.3f}  ->  K_CPU = {sr.K_CPU}, K_GPU = {sr.K_GPU}")
    assert worst <= sr.K_CPU, worst
    assert worst > sr.K_CPU / 2, "K_CPU is not the measured constant any more: measure it again (substep_ref.py)"
    assert sr.K_GPU == 4 * sr.K_CPU


DEFECTS = {1: "no gyroscopic term w x I w, any body", 2: "no centripetal term w x (w x d) of the joint offsets",
           3: "no w x (a qd) in the link's angular bias", 4: "no gyroscopic term on one link (body 3)"}


@pytest.fixture(scope="module")
def defect_engines():
    """(task, N, domain) -> engine of defect build n; the libraries are built here and loaded through oracle_engine.load_library's MQE_ORACLE_LIB switch"""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "-s", "defects"])

    def make(n, task, N, domain):
        with sr.under({"MQE_ORACLE_LIB": f"libmqe_oracle_defect{n}.so"}):
            return sr.make_engine(_f32, task, N, domain)
    return make


@pytest.mark.parametrize("task,N", [("go1gate", 16), ("go1football-2vs2", 16)])
def test_every_defect_build_stands_outside_the_bound(defect_engines, task, N):
    """on every fast grid each defect build exceeds 2 K_GPU in at least one class and the correct float32 oracle exceeds K_GPU in none, at the GPU test's
    batch size, on a seed the yardstick was not taken from twice: the ratio of the correct build against its own yardstick is 1 by construction, so the
    correct build is ALSO held on the next good seed against this one's yardstick"""
    print()
    for grid in sr.FAST:
        domain = sr.GRIDS[grid][5]
        e32, e64 = sr.make_engine(_f32, task, N, domain), sr.make_engine(_f64, task, N, domain)
        d = e32.desc
        (st, r64, keep), (st1, r64b, keep1) = sr.good_seeds(e64, grid, 2, True)
        r32 = sr.run_substep(e32, st, True)
        e0, fl = sr.errors(d, st, r32, r64, keep)
        yard = {k: max(e0[k], fl[k]) for k in e0}
        e1, _ = sr.errors(d, st1, sr.run_substep(e32, st1, True), r64b, keep1)
        own = max(e1[k] / yard[k] for k in e1)
        print(f"    {task:18s} {grid:10s} correct build, next seed: worst {own:6.2f}")
        assert own <= sr.K_GPU, (grid, own)
        for n, what in DEFECTS.items():
            ed = defect_engines(n, task, N, domain)
            r = sr.ratios(d, st, sr.run_substep(ed, st, True), r32, r64, keep)
            ed.close()
            print(f"    {task:18s} {grid:10s} defect {n} ({what}): " + "  ".join(f"{k} {v:.3g}" for k, v in r.items() if not k.startswith("npc")))
            assert max(r.values()) > 2 * sr.K_GPU, (grid, n, r)
        e32.close(); e64.close()
