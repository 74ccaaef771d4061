"""-m gpu: ONE substep in fast free flight, every compiled k_substeps shape row (both envs-per-wavefront forms) and k_simulate against the float64
oracle, with the float32 oracle on the same states as the yardstick (tests/substep_ref.py: grids, driver, metric, K_GPU).  The parity tests see the
specialised instantiations only through whole fused steps in mild states and against absolute tolerances a missing velocity-product term moves by a
few units; here each of them -- its own LDS layout, padding and pointer handling around phys_substep<TA, TP> -- is held within K_GPU float32-oracle
errors of float64 at base rates of 15 rad/s, where such a term stands thousands of those errors out (tests/test_substep_ref.py proves it on the
defect builds of the oracle).  Every engine is built under MQE_VERBOSE and the variant line of mqe_sim_create says which kernel ran.
SH_A2_GEN and SH_GEN are reached with MQE_LANE_SWEEP=1, as in tests/test_gpu_actuator.py."""
import numpy as np
import pytest

import substep_ref as sr
from helpers import hip_engine, oracle_engine
from test_gpu_parity import _record

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("solver")]


def _f32(d, keep):
    return oracle_engine(d, keep)


def _f64(d, keep):
    return oracle_engine(d, keep, f64=True)


def _engines(monkeypatch, capfd, task, N, env, domain, make=sr.make_engine):
    """(HIP engine, float32 oracle, float64 oracle, variant fields) of one descriptor, built under the case's switches by make(factory, task, N, domain)
    (tests/test_contact_substep_gpu.py passes contact_substep_ref.make_engine, whose flag is the randomised friction)"""
    for k, v in dict(env, MQE_VERBOSE="1").items():
        monkeypatch.setenv(k, v)
    capfd.readouterr()
    try:
        eh = make(hip_engine, task, N, domain)
        e32, e64 = make(_f32, task, N, domain), make(_f64, task, N, domain)
    finally:
        for k in dict(env, MQE_VERBOSE="1"):
            monkeypatch.delenv(k)
    lines = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("mqe: variant ")]
    assert len(lines) == 1, lines
    return eh, e32, e64, dict(f.split("=", 1) for f in lines[0].split()[2:]), lines[0]


@pytest.mark.parametrize("cid,task,N,env,shape,epw,fused", sr.CASES, ids=[c[0] for c in sr.CASES])
def test_one_substep_against_float64(monkeypatch, capfd, cid, task, N, env, shape, epw, fused):
    """every grid of substep_ref.GRIDS on the first good seed: each class ratio <= K_GPU; on `stops` and `overspeed` the joints on a bound are the
    float64 oracle's and sit on the bound's own value; free NPCs' root rows under the same rule (a flock's through k_simulate only: the sheep's
    script rewrites them after a fused step)"""
    npc = not (task.startswith("go1sheep") and fused)
    worst, outside, lines = {}, [], []
    for domain in (False, True):
        eh, e32, e64, var, line = _engines(monkeypatch, capfd, task, N, env, domain)
        assert (var["shape"], int(var["epw"])) == (shape, epw), line
        d = eh.desc
        for grid in (g for g in sr.GRIDS if sr.GRIDS[g][5] == domain):
            (st, r64, keep), = sr.good_seeds(e64, grid, 1, fused)
            r32, got = sr.run_substep(e32, st, fused), sr.run_substep(eh, st, fused)
            assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all(), (cid, grid)
            if grid in sr.LIMIT:
                sr.check_on_set(d, st, got, r64, what=f"{cid} {grid}")
            r = sr.ratios(d, st, got, r32, r64, keep, npc)
            worst[grid] = max(r.values())
            outside += [(grid, k, round(v, 2)) for k, v in r.items() if v > sr.K_GPU]
            apart = sr.errors(d, st, got, r32, keep, npc)[0]["qd"] / max(sr.errors(d, st, r32, r64, keep, npc)[0]["qd"], 1e-30)     # reported, not asserted
            lines.append(f"    {cid:18s} {line[13:]}  {grid:10s} seed {st.seed}  " + "  ".join(f"{k} {v:.2f}" for k, v in r.items()) + f"   |qd - qd_f32| / yardstick {apart:.2f}")
        for e in (eh, e32, e64):
            e.close()
    with capfd.disabled():
        print("\n" + "\n".join(lines))
        print(f"    {cid:18s} worst per grid: " + "  ".join(f"{g} {v:.2f}" for g, v in worst.items()) + f"   (K_GPU = {sr.K_GPU})")
    _record("substep_f64", {"case": cid, "task": task, "N": N, "env": env, "fused": fused, "worst_ratio": worst})
    assert not outside, f"{cid}: ratios above K_GPU = {sr.K_GPU}: {outside}"
