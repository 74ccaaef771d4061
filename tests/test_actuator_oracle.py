"""The actuator network (6-32-32-1 softsign) against its float64 reference with a derived rounding bound (tests/actuator_ref.py), on
the CPU: the oracle's f32 fmaf chain on every input grid, the engine's split-f16 layer as a numpy emulation, and -- so that the bound
cannot pass by being vacuous -- the layout errors a kernel could make, each of which must exceed it."""
import ctypes as C

import numpy as np
import pytest

import actuator_ref as ar
from helpers import make_desc, oracle_engine


def _oracle_net(actuator=None):
    d, k, _ = make_desc("go1gate", 1, actuator=actuator)
    e = oracle_engine(d, k)
    f = e.lib.mqo_actuator_net
    f.argtypes, f.restype = [C.c_void_p, C.c_void_p], C.c_float

    def run(x):
        rows = [np.ascontiguousarray(r, np.float32) for r in x]          # keep alive across the foreign calls
        return np.array([f(e.h, r.ctypes.data) for r in rows], np.float64)
    return run


@pytest.mark.parametrize("kind", ar.GRIDS)
def test_oracle_actuator_net_within_the_float64_bound(kind):
    x = ar.grid(kind)
    got = _oracle_net()(x)
    ref, bnd = ar.tau64(x), ar.tau_bound(x)
    ratio = np.abs(got - ref) / bnd
    assert ratio.max() <= 1.0, f"{kind}: row {int(ratio.argmax())}: |oracle - tau64| = {ratio.max():.3f} x the bound"
    # the bound is first order and worst case, not loose by orders of magnitude: a few 1e-5 .. 1e-4 Nm
    assert 2e-5 < bnd.min() and bnd.max() < 2e-3, (bnd.min(), bnd.max())


def test_grids_reach_the_regimes_they_are_named_for():
    """wide: hip and thigh torques beyond the 20 Nm limit; saturating: layer-0 units deep in the softsign's tails"""
    W, b = ar.net()
    t = ar.tau64(ar.grid("wide"))
    assert (np.abs(t) > 20.0).mean() > 0.05
    p1 = ar.grid("saturating").astype(np.float64) @ W[0].T + b[0]
    assert (np.abs(p1) > 10.0).mean() > 0.8          # softsign slope < 1 / 121
    x = ar.grid("exact")
    assert (x == 0).all(axis=1).sum() == 1 and ((x != 0).sum(axis=1) == 1).sum() == 36
    assert np.array_equal(x[-64:], -x[-128:-64])


@pytest.mark.parametrize("kind", ar.GRIDS)
def test_split_f16_layer_emulation_within_the_bound(kind):
    """the engine's default arithmetic for layer 1 (two f16 planes per operand, three products) stays well inside the bound"""
    x = ar.grid(kind)
    ratio = np.abs(ar.tau_split_f16(x) - ar.tau64(x)) / ar.tau_bound(x)
    assert ratio.max() < 0.25, ratio.max()


def _swap_units(i, j):
    W, b = ar.load_actuator_net()
    perm = np.arange(32)
    perm[[i, j]] = perm[[j, i]]
    return [W[0], W[1][:, perm], W[2]], b


def _swap_inputs(x, i, j):
    x = x.copy()
    x[:, [i, j]] = x[:, [j, i]]
    return x


# layout errors, emulated: (name, evaluation on rows x, smallest fraction of the ordinary grid on which it must exceed the bound)
MISTAKES = [
    # hidden units of layer 1 swapped in W1's columns: u(r, h) = (r & 3) + 8 (r >> 2) + 4 h read with h and r >> 2 exchanged, or two neighbours
    ("W1 columns 4 <-> 8", lambda x: ar.tau64(x, *_swap_units(4, 8)), 0.95),
    ("W1 columns 0 <-> 1", lambda x: ar.tau64(x, *_swap_units(0, 1)), 0.95),
    # inputs of layer 0 swapped: the k pairing of a1[s2] = W0[j32 * 6 + 2 s2 + h] against the B operands (h ? x[2 s2 + 1] : x[2 s2])
    ("inputs err_last <-> err_last_last", lambda x: ar.tau64(_swap_inputs(x, 1, 2)), 0.95),
    ("inputs err <-> err_last", lambda x: ar.tau64(_swap_inputs(x, 0, 1)), 0.95),
    ("inputs qd <-> qd_last", lambda x: ar.tau64(_swap_inputs(x, 3, 4)), 0.95),
    # the split-f16 layer with one of its two cross products missing (measured on this grid: 87 % and 39 % of the rows)
    ("split-f16 layer without hl", lambda x: ar.tau_split_f16(x, drop=("hl",)), 0.6),
    ("split-f16 layer without lh", lambda x: ar.tau_split_f16(x, drop=("lh",)), 0.25),
]


@pytest.mark.parametrize("name,wrong,frac", MISTAKES, ids=[m[0] for m in MISTAKES])
def test_bound_catches_layout_errors(name, wrong, frac):
    x = ar.grid("ordinary")
    out = np.abs(wrong(x) - ar.tau64(x)) > ar.tau_bound(x)
    assert out.mean() >= frac, f"{name}: exceeds the bound on only {out.mean():.1%} of the ordinary grid"


@pytest.mark.parametrize("w1max", [3.98, 4.5])
def test_scaled_networks_of_the_fallback_test(w1max):
    """the two layer-1 scalings the GPU test of the f16-plane range check uses: the oracle's f32 chain stays within the bound of the
    scaled network, and so does the split-f16 form at 3.98 (2^14 w still inside f16); at 4.5 the f16 planes clamp and the form breaks"""
    W, b = ar.scaled_net(w1max)
    assert np.float32(np.abs(W[1]).max()) == np.float32(w1max)
    x = np.concatenate([ar.grid("ordinary", 256), ar.grid("wide", 256)])
    ref, bnd = ar.tau64(x, W, b), ar.tau_bound(x, W, b)
    assert (np.abs(_oracle_net((W, b))(x) - ref) <= bnd).all()
    split = np.abs(ar.tau_split_f16(x, W, b) - ref) <= bnd
    if w1max < 3.99:
        assert split.all()
    else:
        assert not split.all()
