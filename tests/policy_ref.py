"""Host side of the locomotion-policy tests (k_gemm_h2 / k_gemm_h2_mix / k_gemm_f32 / k_policy_tail and the general chain; csrc/kernels_gemm.hpp,
kernels_tail.hpp): the float64 reference of the policy in plain numpy, its first-order error bound, two float32 evaluations that calibrate the
bound, a numpy emulation of the split-f16 design with deliberately wrong variants, and the seeded history grids the CPU and GPU tests share.

THE POLICY.  hist [R, 2100] is the 30 x 70 history in time order (HipEngine.history()).  adaptation: 2100 -> 256 -> 128 -> 2 (ELU between the
layers), body: cat(hist, latent) 2102 -> ... -> 12 (ELU between the layers, the last one linear).  forward64 evaluates that in float64 and keeps,
per layer l, its input x_l and pre-activation z_l.  Two switches state what the kernels do OUTSIDE the range they represent: clamp0 clamps the
history operand at +-1023.5 = 65504 / 64 (split2 under MQE_H2_ASCALE: the split layer 0 only), clamp_tail clamps every activation that
k_policy_tail stores as f16 planes (h0, h1, b0, b1, b2) at +-65504 (split2 under TL_ASCALE = 1: the fused tail only).  The latent is never
clamped: it enters body layer 0 in f32 through w_lat0 / w_lat1.

THE BOUND.  A float32 evaluation of z_l = W_l x_l + b_l, in whatever order, differs from the exact value by at most gamma (|W_l| |x_l| + |b_l|)
per unit, gamma = (number of roundings a term passes) * 2^-24; rounding the stored activation costs another 2^-24 |h_l|, which layer l + 1's
|W| |x| term contains; the ELU adds the absolute error of its exponential (1.2e-7 for the kernels' __expf form, <= 1 ulp for expm1f).  To first
order these errors reach the 12 joint targets through G_l = d out / d z_l, the Jacobian of the float64 pass itself (backpropagated through the
body, from the body's two latent columns on into the adaptation module; ELU' = 1 or exp(z), 0 through a clamp that is active).  Hence, per row
and output,

    bound64 = 2^-24 * sum_l |G_l| (|W_l| |x_l| + |b_l| + c_elu),        c_elu = 1.2e-7 / 2^-24 = 2.01 (the ELU's absolute error in units of 2^-24)

and the statement tested is |out - out64| <= K * bound64, where K stands for gamma / 2^-24 and for what first order leaves out.  The true
Jacobian matters: the chained norm bound (products of |W_l|) is about 1e5 times looser on these networks and passes every wrong kernel.

THE CONSTANTS.  K_CPU is MEASURED ON THE CPU, never on a kernel: the worst |f32 - f64| / bound64 over every grid of GRIDS (R = 64 rows each,
seed = the grid's index, the shipped adaptation module and the synthetic body, no clamps: the float32 evaluations have none), reached by two
independent float32 evaluations -- the oracle's own fmaf chain (mqo_policy_forward) and a numpy float32 forward (forward32: BLAS sgemm, another
summation order).  K_GPU = 4 K_CPU (ppo_ref.py's rule, for the same reason: the kernels sum in yet another order -- 32 x 32 x 16 MFMA blocks, a
per-block rotated k order -- and a split product carries 3 * 2^-22 instead of 2^-24).
Measured with `python -m pytest tests/test_policy_ref.py -s -k within_the_bound` (prints this table), worst ratio per grid:
    grid          oracle   numpy32   max |out|   max bound     max |h0|   max |h1|
    unit           0.062     0.028       0.659    1.05e-05          865       1493
    wide           0.207     0.070        19.6    0.000194         1988     1.41e4
    tiny           0.060     0.042       0.317    6.37e-06          798        149
    dyadic         0.186     0.091         101    0.000933         3635     4.18e4
    edge1023       0.454     0.259         990     0.00493       6.67e4     2.84e5
    over           0.536     0.211    4.24e+03      0.0214       5.27e5     2.92e6
    zeros          0.019     0.026       0.114     4.2e-06          8.1       53.4
    resets         0.056     0.032       0.445    1.03e-05          832        998
    continuing     0.049     0.033       0.583    1.05e-05          874       1118
    irregular      0.064     0.032       0.581    1.05e-05          898       1305
    oldest         0.273     0.145        8.95    6.52e-05         3154     1.02e4
K_CPU = 0.6 is the maximum, 0.536, rounded up; K_GPU = 2.4.  tests/test_policy_ref.py asserts that both evaluations stay inside K_CPU, that
the emulated design stays inside K_GPU (it reaches 0.028 / 0.070 / 0.198 / 0.031 / 0.227 on unit / wide / edge1023 / irregular / over, 0.36 with
the heavy-tailed body) and that every emulated defect exceeds 2 K_GPU on some row (MUTANTS: layer 0 without its lh product 7.8 .. 30.6, the
tail without hl 28 .. 126, a single plane 34 .. 211, a split2 without its clamp: not finite).

SATURATION.  The two right-hand columns are the largest hidden activations of the adaptation module in the float64 pass.  h1 (128 wide,
after the ELU) is the activation that leaves the f16 range first: N(0, 0.3) histories reach 1.5e3, N(0, 3) 1.4e4, multiples of 1 / 64 within
+-15 4.2e4, and a history with 0.2 % of its entries at +-1023 -- every entry inside layer 0's documented range -- 2.8e5, so the fused tail's
planes saturate at 65504 (h0 as well, at 6.7e4) and the joint targets differ from the unclamped network's by up to 54 on outputs of 990.
What the kernels compute there is forward64(clamp0=True, clamp_tail=True): a clamp, which the GPU tests hold them to."""
import numpy as np

EPS32 = 2.0 ** -24
C_ELU = 1.2e-7 / EPS32
LIM0 = 65504.0 / 64.0                  # split2 under MQE_H2_ASCALE
LIMT = 65504.0                         # split2 under TL_ASCALE
HIST, FRAME = 30, 70
BIG_COLS = np.r_[0:6, 18:42, 66:70]    # where a grid may put large magnitudes (not the constants 6..17, not the action columns 42..65)

K_CPU = 0.6                            # measured 0.536 (the oracle's chain on `over`), rounded up; see the table above
K_GPU = 4 * K_CPU                      # 2.4

GRIDS = ("unit", "wide", "tiny", "dyadic", "edge1023", "over", "zeros", "resets", "continuing", "irregular", "oldest")
RESET_KS = (0, 1, 17, 28, 29)
IRREGULAR = ((1,), (18,), (29,), (10, 11), "zero15")


# ---- the float64 reference ----------------------------------------------------------------------------------------------------------------
def _elu(z):
    return np.where(z > 0, z, np.expm1(np.minimum(z, 0)))


def _delu(z):
    return np.where(z > 0, 1.0, np.exp(np.minimum(z, 0)))


def _mlp64(x, Ws, bs, clamp, extra=None):
    """-> (output, [layer records]); extra: columns appended to layer 0's input (the latent)"""
    recs = []
    n = len(Ws)
    for l in range(n):
        W, b = np.asarray(Ws[l], np.float64), np.asarray(bs[l], np.float64)
        xin = np.concatenate([x, extra], 1) if (l == 0 and extra is not None) else x
        z = xin @ W.T + b
        rec = dict(W=W, b=b, x=xin, z=z, keep=None)
        recs.append(rec)
        if l + 1 < n:
            h = _elu(z)
            if clamp:
                rec["keep"] = (np.abs(h) <= LIMT).astype(np.float64)
                h = np.clip(h, -LIMT, LIMT)
            x = h
        else:
            x = z
    return x, recs


def forward64(hist, ada, body, clamp0=False, clamp_tail=False):
    """-> (joint targets [R, 12], latent [R, 2], trace) in float64; trace = {"ada": [...], "body": [...]} with per layer W, b, the input x, the
    pre-activation z and keep (1 where the clamp on the layer's activation is inactive; None without clamp_tail): what bound64 needs"""
    x = np.asarray(hist, np.float64)
    assert x.ndim == 2 and x.shape[1] == HIST * FRAME
    if clamp0:
        x = np.clip(x, -LIM0, LIM0)
    lat, ra = _mlp64(x, ada[0], ada[1], clamp_tail)
    out, rb = _mlp64(x, body[0], body[1], clamp_tail, extra=lat)
    return out, lat, {"ada": ra, "body": rb}


def hidden_max(trace):
    """{name: max |activation|} of the hidden activations of the float64 pass (before any clamp): h0, h1, ... / b0, b1, ..."""
    out = {}
    for net, tag in (("ada", "h"), ("body", "b")):
        for l, r in enumerate(trace[net][:-1]):
            out[f"{tag}{l}"] = float(np.abs(_elu(r["z"])).max())
    return out


def bound64(trace):
    """the first-order running bound of the module docstring, [R, 12]"""
    body, ada = trace["body"], trace["ada"]
    R, n_out = body[-1]["z"].shape
    G = np.broadcast_to(np.eye(n_out), (R, n_out, n_out))
    total = np.zeros((R, n_out))

    def back(recs, G, total):
        for l in range(len(recs) - 1, -1, -1):
            L = recs[l]
            t = np.abs(L["x"]) @ np.abs(L["W"]).T + np.abs(L["b"]) + C_ELU
            total += np.einsum("roj,rj->ro", np.abs(G), t)
            Gx = G @ L["W"]                                   # d out / d x_l
            if l == 0:
                return Gx
            P = recs[l - 1]
            d = _delu(P["z"])
            if P["keep"] is not None:
                d = d * P["keep"]
            G = Gx * d[:, None, :]

    Gx = back(body, G, total)
    back(ada, Gx[:, :, HIST * FRAME:], total)                 # the body's sensitivity to the latent carries on into the adaptation module
    return EPS32 * total


# ---- float32 evaluations (the yardsticks K_CPU is measured with) -----------------------------------------------------------------------------
def forward32(hist, ada, body):
    """numpy float32 forward (sgemm summation order, expm1 in float32) -> (joint targets, latent)"""
    f = np.float32
    x = np.asarray(hist, f)

    def mlp(x, Ws, bs):
        for l, (W, b) in enumerate(zip(Ws, bs)):
            x = x @ np.asarray(W, f).T + np.asarray(b, f)
            if l + 1 < len(Ws):
                x = np.where(x > 0, x, np.expm1(np.minimum(x, f(0)))).astype(f)
        return x
    lat = mlp(x, *ada)
    return mlp(np.concatenate([x, lat], 1), *body), lat


def oracle_forward(e, hist):
    """the oracle's own fmaf chain, row by row (mqo_policy_forward of an oracle engine built on the same networks) -> (joint targets, latent)"""
    import ctypes as C
    f = e.lib.mqo_policy_forward
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    hist = np.ascontiguousarray(hist, np.float32)
    out, lat = np.zeros((len(hist), 12), np.float32), np.zeros((len(hist), 2), np.float32)
    for i in range(len(hist)):
        f(e.h, hist[i].ctypes.data, lat[i].ctypes.data, out[i].ctypes.data)
    return out, lat


def ratio(out, ref, bnd):
    """|out - ref| / bound per row and output; a non-finite result counts as infinitely far"""
    with np.errstate(invalid="ignore"):
        r = np.abs(np.asarray(out, np.float64) - ref) / bnd
    return np.where(np.isfinite(r), r, np.inf)


# ---- the split-f16 design, emulated (NOT a second reference: only to show that the bound tells a right design from a wrong one) ---------------
def _split2(x, scale, clamp=True):
    """mqe_common.hpp split2 -> (h, l) as float32 values of the two f16 planes"""
    f = np.float32
    y = np.asarray(x, f) * f(scale)
    if clamp:
        y = np.clip(y, f(-65504.0), f(65504.0))
    with np.errstate(over="ignore", invalid="ignore"):
        h = y.astype(np.float16).astype(f)
        l = (y - h).astype(np.float16).astype(f)
    return h, l


def _wscale(W):
    """mqe_engine.hip weight_scale: the power of two that puts max |w| into [16384, 32768]"""
    wmax = np.float32(np.abs(W).max())
    e = int(np.floor(np.log2(np.float32(32768.0) / wmax))) if wmax > 0 else 0
    return float(2.0 ** min(max(e, -100), 100))


def _prod(a, w, terms, single):
    """sum of the plane products (activation plane x weight plane): every f16 x f16 product is exact in float32, the accumulation is float32"""
    (ah, al), (wh, wl) = a, w
    acc = np.zeros((ah.shape[0], wh.shape[0]), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in (("hh",) if single else terms):
            acc = acc + {"hh": ah, "hl": ah, "lh": al}[t] @ {"hh": wh, "hl": wl, "lh": wh}[t].T
    return acc


def _elu32(v):
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(v > 0, v, np.expm1(np.minimum(v, np.float32(0)))).astype(np.float32)


def _compact_maps(cobs):
    """input k of layer 0 -> (column of the compact operand, factor): mqe_engine.hip k2row / k2scale (mqe_common.hpp MQE_H2_FRAME)"""
    k = np.arange(HIST * FRAME)
    f, c = k // FRAME, k % FRAME
    row = np.where(c < 6, f * 48 + c, np.where(c < 18, f * 48 + 46, np.where(c < 54, f * 48 + c - 12, np.where(c < 66, 0, f * 48 + c - 24))))
    a2 = (c >= 54) & (c < 66)
    row = np.where(a2, np.where(f > 0, (f - 1) * 48 + c - 24, (18 + c - 54) * 48 + 47), row)
    scale = np.ones(len(k))
    const = (c >= 6) & (c < 18)
    scale[const] = np.asarray(cobs, np.float32)[c[const] - 6]
    return row, scale


def emulate_split(hist, ada, body, cobs, split_l0=True, fused_tail=True, l0_terms=("hh", "hl", "lh"), tail_terms=("hh", "hl", "lh"),
                  single_plane=False, clamp0=True, clamp_tail=True):
    """numpy emulation of the policy's arithmetic for the fused shape -> (joint targets, latent).  split_l0: layer 0 as k_gemm_h2 (compact
    operand scaled by 64, per-layer weight scale, hh + hl + lh, the f32 residual of frames that do not continue their predecessor), else plain
    float32.  fused_tail: the rest as k_policy_tail (unscaled planes), else plain float32.  The switches make it wrong on purpose: l0_terms /
    tail_terms leave a plane product out, single_plane keeps hh alone, clamp0 / clamp_tail = False drop split2's clamp (the f16 conversion then
    overflows).  cobs: desc.command_obs[6:18]."""
    f = np.float32
    x = np.ascontiguousarray(hist, f)
    R = len(x)
    (Wa, ba), (Wb, bb) = ada, body
    n_a0 = Wa[0].shape[0]
    W0 = np.concatenate([np.asarray(Wa[0], f), np.asarray(Wb[0], f)[:, :HIST * FRAME]], 0)
    b0 = np.concatenate([np.asarray(ba[0], f), np.asarray(bb[0], f)])
    if split_l0:
        row, scale = _compact_maps(cobs)
        Wc = np.zeros((W0.shape[0], HIST * 48))
        np.add.at(Wc.T, row, (W0.astype(np.float64) * scale).T)
        Wc = Wc.astype(f)
        fr = x.reshape(R, HIST, FRAME)
        A = np.zeros((R, HIST, 48), f)
        for c in range(FRAME):
            cc = c if c < 6 else (c - 12 if 18 <= c < 54 else (c - 24 if c >= 66 else -1))
            if cc >= 0:
                A[:, :, cc] = fr[:, :, c]
        A[:, :, 46] = (fr != 0).any(2)
        A[:, 18:30, 47] = fr[:, 0, 54:66]
        ws = _wscale(Wc)
        acc = _prod(_split2(A.reshape(R, -1), 64.0, clamp0), _split2(Wc, ws), l0_terms, single_plane)
        P = acc * f(1.0 / (64.0 * ws)) + b0
        a2, a1 = fr[:, 1:, 54:66], fr[:, :-1, 42:54]
        irr = (a2.view(np.int32) != a1.view(np.int32)).any(2)                      # [R, 29]: frame p = 1 + index does not continue p - 1
        res = np.where(irr[:, :, None], a2 - a1, f(0))
        Wr = W0.reshape(-1, HIST, FRAME)[:, 1:, 54:66]
        P = P + np.einsum("rpj,opj->ro", res, Wr).astype(f)
    else:
        P = x @ W0.T + b0
    h0, pre0 = _elu32(P[:, :n_a0]), P[:, n_a0:]
    wl = np.asarray(Wb[0], f)[:, HIST * FRAME:]

    def layer(a, W, b, last):
        W, b = np.asarray(W, f), np.asarray(b, f)
        if fused_tail:
            s = _wscale(W)
            v = _prod(_split2(a, 1.0, clamp_tail), _split2(W, s), tail_terms, single_plane) * f(1.0 / s) + b
        else:
            v = a @ W.T + b
        return v if last else _elu32(v)
    h1 = layer(h0, Wa[1], ba[1], False)
    lat = layer(h1, Wa[2], ba[2], True)
    with np.errstate(invalid="ignore", over="ignore"):
        a = _elu32(pre0 + lat[:, :1] * wl[:, 0] + lat[:, 1:2] * wl[:, 1])
    for l in range(1, len(Wb)):
        a = layer(a, Wb[l], bb[l], l + 1 == len(Wb))
    return a, lat


# (name, grids on which it must show, emulate_split switches): every one must exceed 2 K_GPU bound64 on at least one row of one of its grids
MUTANTS = [("layer 0 without lh", ("unit", "wide", "edge1023", "irregular"), dict(l0_terms=("hh", "hl"))),
           ("tail without hl", ("unit", "wide", "edge1023", "irregular"), dict(tail_terms=("hh", "lh"))),
           ("single plane", ("unit", "wide", "edge1023", "irregular"), dict(single_plane=True)),
           ("layer 0 without the clamp", ("over",), dict(clamp0=False)),
           ("tail without the clamp", ("edge1023", "over"), dict(clamp_tail=False))]


# ---- the grids ----------------------------------------------------------------------------------------------------------------------------
def grid(name, R, cobs, seed=0):
    """[R, 30, 70] float32 frames, seeded, every row distinct (`zeros` apart), valid for the compact operand: in every non-zero frame columns
    6..17 are the scene's constants cobs = desc.command_obs[6:18], the action columns 42..65 stay within +-1023, large magnitudes only in
    BIG_COLS.
      unit N(0, 0.3) | wide N(0, 3) | tiny N(0, 1e-6): low planes underflow | dyadic: multiples of 1/64 within +-15, layer-0 planes exact
      edge1023: unit with 0.2 % of the BIG_COLS entries at exactly +-1023 | over: unit with +-3000 and 2e4 in three entries per row
      zeros | resets: frames 0..k zero, k = RESET_KS[row % 5], as a reset leaves the ring
      continuing: frame p's columns 54..65 are frame p-1's 42..53 bit for bit | irregular: continuing, broken per row as IRREGULAR[row % 5]
      says (at p = 1, 18, 29, at two adjacent p, by a zero frame in the middle) | oldest: unit with +-(100..200) in frame 0's columns 54..65
      (the carrier columns)"""
    rs = np.random.RandomState(1000 + seed)
    cobs = np.asarray(cobs, np.float32)

    def base(sigma=0.3):
        return rs.normal(0.0, sigma, (R, HIST, FRAME))

    def chain(f):
        for p in range(1, HIST):
            f[:, p, 54:66] = f[:, p - 1, 42:54]
        return f
    if name == "unit":
        f = base()
    elif name == "wide":
        f = base(3.0)
    elif name == "tiny":
        f = base(1e-6)
    elif name == "dyadic":
        f = rs.randint(-960, 961, (R, HIST, FRAME)) / 64.0
    elif name == "edge1023":
        f = base()
        sub = f[:, :, BIG_COLS]
        hit = rs.rand(*sub.shape) < 0.002
        sub[hit] = np.where(rs.rand(int(hit.sum())) < 0.5, -1023.0, 1023.0)
        f[:, :, BIG_COLS] = sub
    elif name == "over":
        f = base()
        for r in range(R):
            for v in (3000.0, -3000.0, 2.0e4):
                f[r, rs.randint(HIST), BIG_COLS[rs.randint(len(BIG_COLS))]] = v
    elif name == "zeros":
        return np.zeros((R, HIST, FRAME), np.float32)
    elif name == "resets":
        f = base()
        for r in range(R):
            f[r, :RESET_KS[r % len(RESET_KS)] + 1] = 0.0
    elif name == "continuing":
        f = chain(base())
    elif name == "irregular":
        f = chain(base())
        for r in range(R):
            pat = IRREGULAR[r % len(IRREGULAR)]
            if pat == "zero15":
                f[r, 15] = 0.0
            else:
                for p in pat:
                    f[r, p, 54:66] = rs.normal(0.0, 0.3, 12)
    elif name == "oldest":
        f = base()
        f[:, 0, 54:66] = np.where(rs.rand(R, 12) < 0.5, -100.0, 100.0) * (1.0 + rs.rand(R, 12))
    else:
        raise KeyError(name)
    f = f.astype(np.float32)
    live = (f != 0).any(2)
    f[:, :, 6:18] = np.where(live[:, :, None], cobs, np.float32(0))
    return f


def registers(frames):
    """(last_locomotion_action, last_two_locomotion_action) a GPU test writes next to a grid: the newest grid frame's action columns, so that
    the frame the step itself pushes continues the written history exactly where the grid's newest frame did (or, for `irregular`, did not)"""
    return np.ascontiguousarray(frames[:, -1, 42:54]), np.ascontiguousarray(frames[:, -1, 54:66])


# ---- bodies of other shapes and weight ranges -------------------------------------------------------------------------------------------------
def general_body(hidden, seed):
    """seeded body 2102 -> hidden ... -> 12: N(0, 1.5^2 / fan_in) weights, biases uniform in +-0.3"""
    rs = np.random.RandomState(seed)
    dims = (HIST * FRAME + 2,) + tuple(hidden) + (12,)
    Ws = [(rs.standard_normal((dims[i + 1], dims[i])) * (1.5 / np.sqrt(dims[i]))).astype(np.float32) for i in range(len(dims) - 1)]
    bs = [rs.uniform(-0.3, 0.3, dims[i + 1]).astype(np.float32) for i in range(len(dims) - 1)]
    return Ws, bs


def heavy_tailed_body(seed=0):
    """2102-512-256-128-12 (the shape the fused tail runs) with a wide weight range: N(0, 0.05^2) weights, and per layer eight of them at
    +-(20 .. 50).  The per-layer weight scale (max |w| -> [16384, 32768]) is then 2^9, and the low planes of the weights below 2.4e-4 fall
    into the f16 subnormals; biases uniform in +-0.3."""
    rs = np.random.RandomState(seed)
    dims = (HIST * FRAME + 2, 512, 256, 128, 12)
    Ws, bs = [], []
    for i in range(len(dims) - 1):
        W = rs.normal(0.0, 0.05, (dims[i + 1], dims[i]))
        o, k = rs.randint(dims[i + 1], size=8), rs.randint(dims[i], size=8)
        W[o, k] = rs.uniform(20.0, 50.0, 8) * np.where(rs.rand(8) < 0.5, -1.0, 1.0)
        Ws.append(W.astype(np.float32))
        bs.append(rs.uniform(-0.3, 0.3, dims[i + 1]).astype(np.float32))
    return Ws, bs


def command_obs(d):
    """desc.command_obs[6:18]: the constant columns of a written frame"""
    return np.array([d.command_obs[k] for k in range(6, 18)], np.float32)
