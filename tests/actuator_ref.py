"""Float64 reference of the actuator network (6-32-32-1 softsign, unitree_go1.pt; go1.py:367-382), a first-order bound on the rounding
error of any f32 evaluation of it, and the input grids the actuator tests sweep.  CPU only: no GPU, no oracle.

A row of inputs is (err, err_last, err_last_last, qd, qd_last, qd_last_last) -- the order of go1.py:347-350 and of the engines'
actuator history (MQE_T_ACT_HIST = [e1, e2, v1, v2]).  Weights are (out, in) as torch.nn.Linear stores them."""
import numpy as np

from mqe.utils.policy_weights import load_actuator_net

U = 2.0 ** -24                  # unit roundoff of f32 (round to nearest)
C_LAYER = (8.0, 48.0, 34.0)     # rounding constants of the three layers, in units of U (tau_bound)
C_SOFTSIGN = 4.0                # ... and of one softsign, relative to its output


def net(W=None, b=None):
    """(Ws, bs) in float64: the shipped network, or the one passed in"""
    if W is None:
        W, b = load_actuator_net()
    return [np.asarray(w, np.float64) for w in W], [np.asarray(v, np.float64) for v in b]


def _softsign(p):
    return p / (1.0 + np.abs(p))


def tau64(x, W=None, b=None):
    """the network in float64 on rows x (n, 6): one torque per row, before the torque limit"""
    W, b = net(W, b)
    x = np.asarray(x, np.float64)
    h1 = _softsign(x @ W[0].T + b[0])
    h2 = _softsign(h1 @ W[1].T + b[1])
    return h2 @ W[2][0] + b[2][0]


def tau_bound(x, W=None, b=None):
    """First-order bound on |tau_f32 - tau64| for an f32 evaluation of the network on the f32 inputs x (n, 6), in float64.

    Layer l of K products and a bias rounds its result by at most c_l U (sum_k |w_k x_k| + |bias|); the error carried in from the layer
    before is propagated through |W| and, behind each softsign, through its slope 1 / (1 + |p|)^2; each softsign adds C_SOFTSIGN U |h|:
    1 + |p| rounded (U), the reciprocal (v_rcp_f32: 1 ulp = 2 U relative; a correctly rounded division: U), the product (U).
    The constants count the roundings an evaluation order can put on the path of one term, with margin:

      layer 0 (6 products), c_0 = 8:   the engine loads the bias into the accumulator and runs three v_mfma_f32_32x32x2f32 of two
                                       products each (<= 2 roundings per instruction: 6); the oracle's fmaf chain adds the bias last (7).
      layer 1 (32 products), c_1 = 48: f32 chain: 16 MFMAs of two products (32), oracle 33.  Split-f16 (act_layer2_f16): each operand is
                                       held as two f16 planes to 22 significand bits (2^-22 = 4 U relative per operand, 8 U per product),
                                       the dropped low x low product is <= 2^-22 of a product (4 U), and six v_mfma_f32_32x32x16_f16 add
                                       16 exact products each -- at most log2(16) + 1 = 5 roundings deep per instruction (30): 42.
      layer 2 (32 products), c_2 = 34: engine: two 16-term fmaf chains (16), their join and the output bias (18); oracle: a 32-term fmaf
                                       chain and the bias (33).

    None of the constants is a measurement.  Inputs are taken as exact: they are the f32 values both engines read."""
    W, b = net(W, b)
    x = np.asarray(x, np.float64)
    c0, c1, c2 = C_LAYER
    p1 = x @ W[0].T + b[0]
    h1 = _softsign(p1)
    e1 = c0 * U * (np.abs(x) @ np.abs(W[0]).T + np.abs(b[0]))
    eh1 = e1 / (1.0 + np.abs(p1)) ** 2 + C_SOFTSIGN * U * np.abs(h1)
    p2 = h1 @ W[1].T + b[1]
    h2 = _softsign(p2)
    e2 = eh1 @ np.abs(W[1]).T + c1 * U * (np.abs(h1) @ np.abs(W[1]).T + np.abs(b[1]))
    eh2 = e2 / (1.0 + np.abs(p2)) ** 2 + C_SOFTSIGN * U * np.abs(h2)
    return eh2 @ np.abs(W[2][0]) + c2 * U * (np.abs(h2) @ np.abs(W[2][0]) + abs(b[2][0]))


# ---- input grids ---------------------------------------------------------------------------------------------------------------------
GRIDS = ("ordinary", "wide", "saturating", "exact")
_RANGE = {"ordinary": (0.3, 5.0), "wide": (3.0, 40.0), "saturating": (50.0, 1e3)}     # |err| [rad], |qd| [rad/s]


def grid(kind, n=1024, seed=0):
    """(n', 6) float32 rows.  ordinary / wide / saturating: uniform in +-|err| on the three errors and +-|qd| on the three velocities;
    exact: zeros, rows where one input alone is non-zero (at every range's scale, both signs), and sign-mirrored pairs"""
    if kind == "exact":
        rows = [np.zeros(6)]
        for i in range(6):
            for e, v in _RANGE.values():
                for s in (1.0, -1.0):
                    r = np.zeros(6)
                    r[i] = s * (e if i < 3 else v)
                    rows.append(r)
        half = grid("wide", 64, seed + 1).astype(np.float64)
        rows = np.concatenate([np.asarray(rows), half, -half])
        return rows.astype(np.float32)
    e, v = _RANGE[kind]
    rs = np.random.RandomState(seed)
    x = rs.uniform(-1.0, 1.0, (n, 6)) * np.array([e, e, e, v, v, v])
    return x.astype(np.float32)


# ---- numpy emulation of the split-f16 layer (mqe_common.hpp act_layer2_f16), for the tests that the bound is not vacuous -------------
def _planes(x, scale):
    """f32 x -> two f16 planes of scale * x (mqe_common.hpp split2): h + l == scale * x to 22 significand bits"""
    y = np.clip(np.asarray(x, np.float32) * np.float32(scale), -65504.0, 65504.0).astype(np.float32)
    h = y.astype(np.float16)
    lo = (y - h.astype(np.float32)).astype(np.float16)
    return h.astype(np.float64), lo.astype(np.float64)


def tau_split_f16(x, W=None, b=None, drop=()):
    """the network with layer 1 in the engine's split-f16 form: f32 activations of layer 0, weights and activations as two f16 planes
    of 2^14 x, the products hh + hl + lh (first letter: weight plane, second: activation plane) summed exactly and rounded to f32 once,
    the rest in float64.  drop: products to leave out ("hl", "lh") -- the errors the bound must catch."""
    W32, b32 = load_actuator_net() if W is None else (W, b)
    W64, b64 = net(W32, b32)
    x = np.asarray(x, np.float64)
    h1 = _softsign(x @ W64[0].T + b64[0]).astype(np.float32)
    wh, wl = _planes(W32[1], 16384.0)
    sh, sl = _planes(h1, 16384.0)
    acc = np.asarray(b32[1], np.float32).astype(np.float64) * 2.0 ** 28
    acc = acc + sh @ wh.T
    if "hl" not in drop:
        acc = acc + sl @ wh.T
    if "lh" not in drop:
        acc = acc + sh @ wl.T
    p2 = acc.astype(np.float32).astype(np.float64) * 2.0 ** -28
    h2 = _softsign(p2)
    return h2 @ W64[2][0] + b64[2][0]


def scaled_net(w1max):
    """the shipped network with layer 1's weights scaled so that max |W1| = w1max (the engine's f16-plane range check: < 3.99)"""
    W, b = load_actuator_net()
    W = [w.copy() for w in W]
    W[1] = (W[1].astype(np.float64) * (w1max / np.abs(W[1]).max())).astype(np.float32)
    return W, [v.copy() for v in b]
