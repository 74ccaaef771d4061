"""-m gpu: ONE substep IN CONTACT, every compiled k_substeps shape row (both envs-per-wavefront forms) and k_simulate against the float64 oracle, with the
float32 oracle on the same states as the yardstick (tests/contact_substep_ref.py: base states, grids, exclusion rule, metric, KC_GPU; the cases are
substep_ref.CASES).  The parity tests meet contacts through k_simulate under absolute tolerances, or through 20-step fused rollouts held to a
distribution of base-position deviation; here the normal rows of both solvers, the friction box, the temporal solver's re-evaluated separations, its
push-out cap and voff, the bounded list's truncation and the two-actor blocks of every shape row -- its own LDS layout and lane assignment -- are held
within KC_GPU float32-oracle errors of float64, where a friction coefficient or a push-out cap wrong by 1 % stands hundreds of those errors out
(tests/test_contact_substep_ref.py proves it, and on the defect builds of the oracle).  Every engine is built under MQE_VERBOSE and the variant line of
mqe_sim_create says which kernel ran."""
import numpy as np
import pytest

import contact_substep_ref as cr
import substep_ref as sr
from test_gpu_parity import _record
from test_substep_gpu import _engines

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("solver")]


@pytest.mark.parametrize("cid,task,N,env,shape,epw,fused", sr.CASES, ids=[c[0] for c in sr.CASES])
def test_one_substep_in_contact_against_float64(monkeypatch, capfd, solver, cid, task, N, env, shape, epw, fused):
    """every grid of contact_substep_ref.GRIDS on the first good seed: the result is finite, MQE_T_CONTACT_OVERFLOW is the float64 oracle's in every env, each
    class ratio <= KC_GPU; free NPCs' root rows under the same rule (a flock's through k_simulate only: the sheep's script rewrites them after a fused step)"""
    npc = not (task.startswith("go1sheep") and fused)
    with sr.under(env):
        sc = cr.scene(task, N, solver, {k: v for k, v in env.items() if k == "MQE_COLLISION_MODEL"})
    worst, outside, lines = {}, [], []
    for rf in (False, True):
        eh, e32, e64, var, line = _engines(monkeypatch, capfd, task, N, env, rf, make=cr.make_engine)
        e64.close()             # the scene has its own float64 oracles
        assert (var["shape"], int(var["epw"])) == (shape, epw), line
        d = eh.desc
        for grid in (g for g in cr.grids_of(d) if cr.GRIDS[g][6] == rf):
            with sr.under(env):
                (st, r64, keep), = sc.good_seeds(grid, 1, fused)
            r32, got = cr.run_substep(e32, st, fused), cr.run_substep(eh, st, fused)
            assert all(np.isfinite(x).all() for x in got[:3]), (cid, grid)
            assert np.array_equal(got[3], r64[3]), (cid, grid, "MQE_T_CONTACT_OVERFLOW", got[3].tolist(), r64[3].tolist())
            r = cr.ratios(d, st, got, r32, r64, keep, npc)
            worst[grid] = max(r.values())
            outside += [(grid, k, round(v, 2)) for k, v in r.items() if v > cr.KC_GPU]
            lines.append(f"    {solver} {cid:18s} {line[13:]}  {grid:9s} seed {st.seed}  " + "  ".join(f"{k} {v:.2f}" for k, v in r.items()) + f"   envs in overflow {int((r64[3] > 0).sum())}")
        eh.close(); e32.close()
    with capfd.disabled():
        print("\n" + "\n".join(lines))
        print(f"    {solver} {cid:18s} worst per grid: " + "  ".join(f"{g} {v:.2f}" for g, v in worst.items()) + f"   (KC_GPU = {cr.KC_GPU})")
    _record("contact_substep_f64", {"case": cid, "task": task, "N": N, "env": env, "fused": fused, "solver": solver, "worst_ratio": worst})
    assert not outside, f"{cid}: ratios above KC_GPU = {cr.KC_GPU}: {outside}"
