"""CPU: the float64 reference of the locomotion policy (tests/policy_ref.py) against the torch modules, the two float32 evaluations that its
constant K_CPU is measured with, and the emulated split-f16 design with its deliberately wrong variants: the bound tests/test_policy_gpu.py holds
the kernels to must pass a right design and fail every wrong one.  Run with -s to see the measured tables."""
import numpy as np
import pytest
import torch

import policy_ref as pr
from helpers import make_desc, oracle_engine
from mqe.utils import policy_weights as pw

R_CAL = 64          # rows per grid of the calibration (policy_ref.py: THE CONSTANTS)


@pytest.fixture(scope="module")
def nets():
    """the shipped adaptation module, the synthetic body, the scene's constant columns and an oracle engine on those networks"""
    d, keep, _ = make_desc("go1gate", 1)
    ada = pw.load_adaptation_module()
    Wb, bb, _ = pw.load_body(None, seed=0)
    return dict(ada=ada, body=(Wb, bb), cobs=pr.command_obs(d), oracle=oracle_engine(d, keep))


def _hist(nets, g, R=R_CAL):
    return pr.grid(g, R, nets["cobs"], pr.GRIDS.index(g)).reshape(R, -1)


@pytest.mark.parametrize("g", pr.GRIDS)
def test_grids_are_valid_for_the_compact_operand(nets, g):
    f = pr.grid(g, R_CAL, nets["cobs"], pr.GRIDS.index(g))
    assert f.dtype == np.float32 and f.shape == (R_CAL, pr.HIST, pr.FRAME)
    assert np.array_equal(f, pr.grid(g, R_CAL, nets["cobs"], pr.GRIDS.index(g))), "not seeded"
    live = (f != 0).any(2)
    assert np.array_equal(f[:, :, 6:18][live], np.broadcast_to(nets["cobs"], f[:, :, 6:18].shape)[live])
    assert np.abs(f[:, :, 42:66]).max() <= 1023.0
    small = np.setdiff1d(np.arange(pr.FRAME), pr.BIG_COLS)
    assert np.abs(f[:, :, small]).max() <= 200.0                      # large magnitudes only where a clamp means a clamp
    rows = f.reshape(R_CAL, -1)
    rows = rows[rows.any(1)]                                          # (`zeros`, and the rows of `resets` with all 30 frames zeroed, have no content)
    assert len(np.unique(rows, axis=0)) == len(rows), "two rows are equal: a row mix-up would not show"
    if g == "continuing":
        assert np.array_equal(f[:, 1:, 54:66].view(np.int32), f[:, :-1, 42:54].view(np.int32))
    if g == "irregular":
        brk = (f[:, 1:, 54:66].view(np.int32) != f[:, :-1, 42:54].view(np.int32)).any(2)
        assert brk[0, 0] and brk[1, 17] and brk[2, 28] and brk[3, 9] and brk[3, 10] and not f[4, 15].any() and (brk.sum(1) <= 2).all()
    if g == "resets":
        for r in range(len(pr.RESET_KS)):
            k = pr.RESET_KS[r]
            assert not f[r, :k + 1].any() and (k == 29 or f[r, k + 1].any())
    if g == "edge1023":
        assert (np.abs(f) == 1023.0).any() and np.abs(f).max() == 1023.0
    if g == "oldest":
        assert np.abs(f[:, 0, 54:66]).min() >= 100.0


def test_forward64_agrees_with_the_torch_modules(nets, tmp_path):
    """forward64 == the TorchScript-style modules in float64 (adaptation module as shipped, a scripted body of another shape), to 1e-12 of
    each row's largest output"""
    from test_models_oracle import scripted_body, torch_adaptation
    net, Ws, bs = scripted_body(tmp_path)
    ada_t, net = torch_adaptation().double(), net.double()
    for g in ("unit", "wide", "over"):
        h = _hist(nets, g, 16)
        out, lat, _ = pr.forward64(h, nets["ada"], (Ws, bs))
        with torch.no_grad():
            x = torch.from_numpy(h).double()
            lt = ada_t(x)
            ot = net(torch.cat([x, lt], 1))
        for got, want in ((lat, lt.numpy()), (out, ot.numpy())):
            assert (np.abs(got - want) <= 1e-12 * np.abs(want).max(1, keepdims=True)).all(), (g, np.abs(got - want).max())


def test_the_bound_is_the_first_order_effect_of_a_perturbation(nets):
    """bound64's Jacobians are the float64 pass's own: perturbing one layer's bias by delta moves the outputs by G_l delta to first order,
    so with delta = 2^-24 (|W| |x| + |b| + c_elu) s, s a random sign per unit, the outputs move by no more than that layer's share of the
    bound, and the layers' shares together by no more than the whole (and by more than a hundredth of it: the bound is not slack by orders)"""
    h = _hist(nets, "wide", 8)
    ada, body = nets["ada"], nets["body"]
    out, _, tr = pr.forward64(h, ada, body)
    bnd = pr.bound64(tr)
    rs = np.random.RandomState(0)
    moved = np.zeros_like(out)
    # a per-row bias perturbation is a per-row input perturbation of the next evaluation: evaluate row by row
    for r in range(len(h)):
        bs_a = [np.asarray(b, np.float64) + pr.EPS32 * (np.abs(L["x"][r]) @ np.abs(L["W"]).T + np.abs(L["b"]) + pr.C_ELU) * rs.choice([-1.0, 1.0], len(b))
                for b, L in zip(ada[1], tr["ada"])]
        bs_b = [np.asarray(b, np.float64) + pr.EPS32 * (np.abs(L["x"][r]) @ np.abs(L["W"]).T + np.abs(L["b"]) + pr.C_ELU) * rs.choice([-1.0, 1.0], len(b))
                for b, L in zip(body[1], tr["body"])]
        moved[r] = pr.forward64(h[r:r + 1], (ada[0], bs_a), (body[0], bs_b))[0][0] - out[r]
    assert (np.abs(moved) <= 1.001 * bnd).all(), (np.abs(moved) / bnd).max()
    assert (np.abs(moved) / bnd).max() > 0.01


def test_float32_evaluations_stay_within_the_bound(nets):
    """K_CPU: on every grid the oracle's fmaf chain and the numpy float32 forward are within K_CPU bound64 of forward64 (no clamps: the float32
    evaluations have none).  Prints the table policy_ref.py quotes."""
    worst = {}
    print("\n    grid          oracle   numpy32   max |out|   max bound")
    for g in pr.GRIDS:
        h = _hist(nets, g)
        ref, lat, tr = pr.forward64(h, nets["ada"], nets["body"])
        bnd = pr.bound64(tr)
        assert np.isfinite(bnd).all() and (bnd > 0).all()
        ro = pr.ratio(pr.oracle_forward(nets["oracle"], h)[0], ref, bnd)
        rn = pr.ratio(pr.forward32(h, nets["ada"], nets["body"])[0], ref, bnd)
        worst[g] = (float(ro.max()), float(rn.max()))
        print(f"    {g:12s} {ro.max():7.3f}   {rn.max():7.3f}   {np.abs(ref).max():9.3g}   {bnd.max():9.3g}")
    k = max(max(v) for v in worst.values())
    print(f"    worst {k:.3f}  ->  K_CPU = {pr.K_CPU}, K_GPU = {pr.K_GPU}")
    assert k <= pr.K_CPU, worst
    assert k > pr.K_CPU / 4, "K_CPU is not the measured constant any more: measure it again (policy_ref.py)"
    assert pr.K_GPU == 4 * pr.K_CPU


def _emulated_ratio(nets, g, body=None, **kw):
    h = _hist(nets, g)
    body = body or nets["body"]
    ref, _, tr = pr.forward64(h, nets["ada"], body, clamp0=True, clamp_tail=True)
    out, _ = pr.emulate_split(h, nets["ada"], body, nets["cobs"], **kw)
    return pr.ratio(out, ref, pr.bound64(tr))


def test_the_bound_has_teeth(nets):
    """the emulated design (split layer 0 + fused tail, against the saturating reference) stays below K_GPU bound64 on unit / wide / edge1023 /
    irregular; each wrong variant exceeds 2 K_GPU bound64 on at least one row of every grid it is listed with"""
    print()
    for g in ("unit", "wide", "edge1023", "irregular", "over"):
        r = _emulated_ratio(nets, g)
        print(f"    design      {g:10s} worst ratio {r.max():8.3f}")
        assert r.max() <= pr.K_GPU, (g, r.max())
    for name, grids, kw in pr.MUTANTS:
        for g in grids:
            r = _emulated_ratio(nets, g, **kw)
            print(f"    {name:28s} {g:10s} worst ratio {r.max():8.3g}   rows outside 2 K_GPU: {int((r.max(1) > 2 * pr.K_GPU).sum())} of {len(r)}")
            assert (r.max(1) > 2 * pr.K_GPU).any(), (name, g, r.max())


def test_saturation_edge(nets):
    """the fused tail's clamp is inactive on unit / wide / tiny (forward64 identical with and without clamp_tail) and active on edge1023 and
    over -- inside layer 0's documented input range in the first case.  Prints the largest hidden activations per grid."""
    print("\n    grid         max |h0|   max |h1|   max |b0|   max |b1|   max |b2|")
    for g in pr.GRIDS:
        h = _hist(nets, g)
        out, _, tr = pr.forward64(h, nets["ada"], nets["body"])
        sat, _, _ = pr.forward64(h, nets["ada"], nets["body"], clamp_tail=True)
        m = pr.hidden_max(tr)
        print(f"    {g:12s}" + "".join(f" {m[k]:10.4g}" for k in ("h0", "h1", "b0", "b1", "b2")))
        if g in ("unit", "wide", "tiny"):
            assert np.array_equal(out, sat) and max(m.values()) < pr.LIMT, g
        if g in ("edge1023", "over"):
            assert m["h1"] > pr.LIMT and not np.array_equal(out, sat), g
            assert m["h1"] >= m["h0"]                      # h1 is the activation that saturates first
    h = _hist(nets, "edge1023")
    assert np.abs(h).max() <= 1023.0                        # every entry inside layer 0's range: clamp0 changes nothing there
    assert np.array_equal(pr.forward64(h, nets["ada"], nets["body"], clamp0=True)[0], pr.forward64(h, nets["ada"], nets["body"])[0])


def test_design_holds_on_a_wide_weight_range(nets):
    """the heavy-tailed body of tests/test_policy_gpu.py (weights of 0.05 next to a few of 20 .. 50: low planes of the small ones in the f16
    subnormals): the emulated design stays below K_GPU bound64 on unit and tiny, so a kernel outside it there is wrong, not the design"""
    body = pr.heavy_tailed_body(0)
    for W in body[0]:
        s = pr._wscale(W)
        lo = pr._split2(W, s)[1]
        assert 20.0 <= np.abs(W).max() <= 50.0 and (np.abs(lo[lo != 0]) < 2.0 ** -14).any(), "no low-plane subnormals: the weight set lost its point"
    print()
    for g in ("unit", "tiny"):
        r = _emulated_ratio(nets, g, body=body)
        print(f"    heavy-tailed body  {g:6s} worst ratio {r.max():.3f}")
        assert r.max() <= pr.K_GPU, (g, r.max())
