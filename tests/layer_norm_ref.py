"""Host side of the layer-normalisation tests (MQE_ACTOR_LAYER_NORM, MQE_ACTOR_FEATURE_NORM; csrc/kernels_ln.hpp): the norm's twin -- float64,
and float32 in the kernel's own summation order --, the networks with norms as a torch expression (torch.nn.functional.layer_norm: for autograd,
THE reference) and as a manual backward at any dtype (float64: what the GPU test compares against, held to autograd by tests/test_layer_norm.py),
deliberately wrong variants, seeded parameters and the kink-free synthetic trajectory in ppo_ref.synth's format, and the tolerances.

THE BOUNDS follow tests/ppo_ref.py.  Gradient: |g - g64| <= K 2^-24 S_n for every entry of tensor n, exactly 0 where S_n = 0; S_n = the largest
entry of the summed ABSOLUTE per-sample contributions (for a norm: sum |du xhat| for its weight, sum |du| for its bias).  K is MEASURED ON THE
CPU, never on the kernel: the largest ratio reached over K_CASES by two float32 evaluations -- torch autograd on the whole batch, and the manual
backward with the kernel-order norm accumulated over tiles of 64 rows.  The GPU gets K_LN_GPU = 4 K_LN_CPU.  Forward: the yardstick is torch's
float32 CPU evaluation against float64 on the same inputs (forward_errors), the GPU gets 4x.

Measured with this file (tests/test_layer_norm.py prints every case; 36 cases: 4 networks x M in {1, 63, 130} x 3 seeds, value clipping on,
entropy_coef 0.01; the larger of the two float32 evaluations, gradient tensors and statistics together), largest ratio per network and M.  torch's
float32 CPU kernels differ between hosts (another BLAS path, another thread count), and with M = 1 nothing averages, so the table holds two hosts:
                   M = 1     63    130   |  M = 1     63    130      (a second host)
    tanh7_17       13.7    3.9    6.0   |   15.0    3.1    4.0
    relu64x64      23.7   11.2   18.1   |   29.6    9.6   18.6
    tanh256x3      20.3   16.2   10.0   |   46.0    7.8    7.6
    linear         28.6    2.9    4.5   |   19.1    6.9    4.8
The left table is a host whose torch runs 8 CPU threads (torch.get_num_threads()), the right one a host with 16, the kind that also carries the
GPU; tests/test_layer_norm.py runs on both, prints every case, and is expected to reproduce the column of the host it runs on to the printed
digits (left: maximum 28.56, linear, M = 1; right: maximum 46.00, tanh256x3, M = 1, seed 1, the tiled evaluation).  One constant has to hold on
both, since the same test asserts it on both, so K_LN_CPU = 47 is the larger maximum rounded up to the next integer.  A single-host K would be
29 on the left host; the GPU bound 4 K is therefore up to 1.6x wider than that host alone would give, which is the price of one test for both.
From M = 63 up nothing exceeds 18.6 on either.  K_LN_CPU is NOT taken from anything the kernel computes."""
import math

import numpy as np
import torch

from mqe.engine import abi
import ppo_ref

EPS32 = ppo_ref.EPS32
SENT = ppo_ref.SENT
LN2PI = ppo_ref.LN2PI
CLIP, VALUE_CLIP = ppo_ref.CLIP, ppo_ref.VALUE_CLIP
LN_EPS = 1e-5
WAVES = 16                     # csrc/kernels_actor.hpp ACT_WAVES: the norm's features are split over them in consecutive chunks
K_LN_CPU = 47.0
K_LN_GPU = 4 * K_LN_CPU

# name: (activation, the actor's hidden widths, the critic's, hidden norm, feature norm) -- the GPU test's four shapes
CASES = {"tanh7_17": ("tanh", (7,), (17,), True, False), "relu64x64": ("relu", (64, 64), (64, 64), True, True),
         "tanh256x3": ("tanh", (256, 256, 256), (256, 256, 256), True, True), "linear": ("tanh", (), (), False, True)}
K_MS = (1, 63, 130)
K_CASES = [(case, M, seed) for case in CASES for M in K_MS for seed in (0, 1, 2)]
VARIANTS_FORWARD = ("unbiased", "eps_outside", "norm_before_act")       # wrong networks: their float32 autograd gradient is the wrong answer
VARIANTS_BACKWARD = ("no_gamma", "no_xhat_term")                       # wrong backward passes of the right network


def dims_of(case, D):
    act, ah, ch, hidden, feat = CASES[case]
    return [D, *ah, 3], [D, *ch, 1], act, hidden, feat


def layout(a_dims, c_dims, hidden, feat):
    return abi.actor_param_layout(a_dims, c_dims, False, hidden, feat)


def seeded_params(a_dims, c_dims, hidden, feat, seed, weight_scale=1.0):
    """{name: float32 tensor} in the layout's names: Linear weights and biases uniform in +-1 / sqrt(fan_in) (rollout_ref.seeded_params'),
    log_std uniform in [-1, 0.5], a norm's weight uniform in [0.5, 1.5] and its bias in [-0.5, 0.5].  weight_scale multiplies the weight
    and the bias of layer 0, so that the activations of a row differ little: a variance near eps"""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for name, (_, shape) in layout(a_dims, c_dims, hidden, feat).items():
        part = name.split(".")
        if name == "log_std":
            out[name] = torch.rand(3, generator=g) * 1.5 - 1.0
        elif "norm" in part[1] or part[2] == "norm":
            out[name] = torch.rand(*shape, generator=g) + (0.5 if part[-1] == "weight" else -0.5)
        else:
            fan_in = (a_dims if part[0] == "actor" else c_dims)[int(part[1])]
            out[name] = (torch.rand(*shape, generator=g) * 2 - 1) / math.sqrt(fan_in)
            if part[1] == "0":
                out[name] = out[name] * weight_scale
    return out


# ---- the norm ---------------------------------------------------------------------------------------------------------------------------------
def _fma32(a, b, c):
    """fmaf on float32 tensors: the product of two float32 is exact in float64"""
    return (a.double() * b.double() + c.double()).float()


def layer_norm(a, g, b, kernel_order=False, variant=None):
    """The norm of the last axis: -> (u, xhat, rstd).  float64 (or any dtype) by the definition; kernel_order: float32 with the chains of
    csrc/kernels_ln.hpp -- per-wave partials over consecutive chunks of ceil(n / 16) features, added in wave order, 1 / n rounded once, a
    centred second pass with fmaf, eps inside the root.  variant "unbiased": n - 1; "eps_outside": 1 / (sqrt(var) + eps)."""
    n = a.shape[-1]
    if kernel_order:
        assert a.dtype == torch.float32 and variant is None
        c = -(-n // WAVES)
        inv_n = torch.tensor(1.0 / n, dtype=torch.float64).float()

        def sweep(term):
            t = torch.zeros(a.shape[:-1])
            for w in range(WAVES):
                s = torch.zeros(a.shape[:-1])
                for k in range(min(w * c, n), min(w * c + c, n)):
                    s = term(s, k)
                t = t + s
            return t
        mu = (sweep(lambda s, k: s + a[..., k]) * inv_n)[..., None]
        d = a - mu
        var = sweep(lambda s, k: _fma32(d[..., k], d[..., k], s)) * inv_n
        rstd = (1.0 / torch.sqrt(var + torch.tensor(LN_EPS, dtype=torch.float32)))[..., None]
        xhat = d * rstd
        return _fma32(g, xhat, b), xhat, rstd
    mu = a.mean(-1, keepdim=True)
    d = a - mu
    var = (d * d).sum(-1, keepdim=True) / (n - 1 if variant == "unbiased" else n)
    rstd = 1.0 / (torch.sqrt(var) + LN_EPS) if variant == "eps_outside" else 1.0 / torch.sqrt(var + LN_EPS)
    xhat = d * rstd
    return g * xhat + b, xhat, rstd


def norm_name(who, l):
    """the norm in front of Linear l: the feature norm, or the one behind hidden layer l - 1"""
    return f"{who}.norm_in" if l == 0 else f"{who}.{l - 1}.norm"


def forward(p, who, dims, act, hidden, feat, x, kernel_order=False, variant=None, functional=False):
    """-> (out, xs, norms, pres): xs[l] the input of Linear l; norms[l] = (name, a, xhat, rstd) of the norm in front of it or None; pres the
    hidden pre-activations.  functional: the norm is torch.nn.functional.layer_norm (autograd's reference).  variant "norm_before_act": the
    hidden norm in front of the activation instead of behind it."""
    f = torch.tanh if act == "tanh" else torch.relu
    L = len(dims) - 1
    xs, norms, pres = [], [], []
    h = x
    for l in range(L):
        normed = (feat if l == 0 else hidden) and not (variant == "norm_before_act" and l > 0)
        if normed:
            name = norm_name(who, l)
            if functional:
                u, xhat, rstd = torch.nn.functional.layer_norm(h, (h.shape[-1],), p[name + ".weight"], p[name + ".bias"], LN_EPS), None, None
            else:
                u, xhat, rstd = layer_norm(h, p[name + ".weight"], p[name + ".bias"], kernel_order, variant)
            norms.append((name, h, xhat, rstd))
            h = u
        else:
            norms.append(None)
        xs.append(h)
        h = h @ p[f"{who}.{l}.weight"].T + p[f"{who}.{l}.bias"]
        if l + 1 < L:
            pres.append(h)
            if variant == "norm_before_act" and hidden:
                h = layer_norm(h, p[norm_name(who, l + 1) + ".weight"], p[norm_name(who, l + 1) + ".bias"])[0]
            h = f(h)
    return h, xs, norms, pres


def forward_errors(params, a_dims, c_dims, act, hidden, feat, obs):
    """float64 mean / value on obs (the twin), and the yardstick: max |torch float32 CPU - float64| of each"""
    out = {}
    for who, dims, key in (("actor", a_dims, "mean"), ("critic", c_dims, "value")):
        if not dims:
            continue
        p64, p32 = {k: v.double() for k, v in params.items()}, {k: v.float() for k, v in params.items()}
        y64 = forward(p64, who, dims, act, hidden, feat, obs.double())[0]
        y32 = forward(p32, who, dims, act, hidden, feat, obs.float(), functional=True)[0]
        if key == "value":
            y64, y32 = y64[..., 0], y32[..., 0]
        out[key + "64"], out["yard_" + key] = y64, float((y32.double() - y64).abs().max())
    return out


# ---- the loss and its gradient ------------------------------------------------------------------------------------------------------------------
def loss_torch(params, a_dims, c_dims, act, hidden, feat, b, cfg, variant=None):
    """ppo_ref.loss_torch on the networks with norms (torch.nn.functional.layer_norm unless a wrong variant is asked for): -> (L, stats[6])"""
    c, vc, ec, cv = cfg["clip"], cfg["value_coef"], cfg["entropy_coef"], cfg["value_clip"]
    ls = params["log_std"]
    fn = variant is None
    mean = forward(params, "actor", a_dims, act, hidden, feat, b["obs"], variant=variant, functional=fn)[0]
    v = forward(params, "critic", c_dims, act, hidden, feat, b["obs"], variant=variant, functional=fn)[0][:, 0]
    z = (b["actions"] - mean) * torch.exp(-ls)
    logp = (-0.5 * z * z - ls).sum(-1) - 1.5 * LN2PI
    ratio = torch.exp(logp - b["logp_old"])
    Lpi = -torch.minimum(ratio * b["adv"], torch.clamp(ratio, 1 - c, 1 + c) * b["adv"])
    Lv = (v - b["ret"]) ** 2
    if cv is not None:
        v_c = b["v_old"] + torch.clamp(v - b["v_old"], -cv, cv)
        Lv = torch.maximum(Lv, (v_c - b["ret"]) ** 2)
    H = ls.sum() + 1.5 * (1 + LN2PI)
    L = Lpi.mean() + vc * Lv.mean() - ec * H
    stats = torch.stack([Lpi.mean(), Lv.mean(), H, L, (b["logp_old"] - logp).mean(), ((ratio - 1).abs() > c).to(L.dtype).mean()])
    return L, stats


def autograd(params, a_dims, c_dims, act, hidden, feat, b, cfg, dtype, variant=None):
    """torch autograd of loss_torch at `dtype` on the whole batch: -> ({name: grad}, stats)"""
    p = {k: v.to(dtype).clone().requires_grad_(True) for k, v in params.items()}
    bb = {k: v.to(dtype) for k, v in b.items()}
    L, stats = loss_torch(p, a_dims, c_dims, act, hidden, feat, bb, cfg, variant)
    L.backward()
    return {k: (v.grad if v.grad is not None else torch.zeros_like(v)).detach() for k, v in p.items()}, stats.detach()


def manual(params, a_dims, c_dims, act, hidden, feat, b, cfg, dtype=torch.float64, tile=None, variant=None):
    """ppo_ref.manual with the norms' backward as csrc/kernels_ln.hpp states it; float32: the norm in the kernel's order.  -> (grads, stats[6], S,
    stat_scales).  variant "no_gamma": dxhat = du; "no_xhat_term": the xhat * mean(dxhat xhat) term dropped."""
    c, vc, ec, cv = cfg["clip"], cfg["value_coef"], cfg["entropy_coef"], cfg["value_clip"]
    p = {k: v.to(dtype) for k, v in params.items()}
    b = {k: v.to(dtype) for k, v in b.items()}
    M = b["obs"].shape[0]
    inv_m = 1.0 / M
    ls = p["log_std"]
    inv = torch.exp(-ls)
    g = {k: torch.zeros_like(v) for k, v in p.items()}
    S = {k: torch.zeros_like(v) for k, v in p.items()}
    sums, sc = torch.zeros(4, dtype=dtype), torch.zeros(3, dtype=dtype)
    order = dtype == torch.float32
    tile = tile or M
    for r0 in range(0, M, tile):
        sl = slice(r0, min(r0 + tile, M))
        obs = b["obs"][sl]
        fa = forward(p, "actor", a_dims, act, hidden, feat, obs, kernel_order=order)
        fc = forward(p, "critic", c_dims, act, hidden, feat, obs, kernel_order=order)
        mean, v = fa[0], fc[0][:, 0]
        z = (b["actions"][sl] - mean) * inv
        logp = (-0.5 * z * z - ls).sum(-1) - 1.5 * LN2PI
        lpo, adv, ret = b["logp_old"][sl], b["adv"][sl], b["ret"][sl]
        ratio = torch.exp(logp - lpo)
        Lpi = -torch.minimum(ratio * adv, torch.clamp(ratio, 1 - c, 1 + c) * adv)
        gate = ((adv > 0) & (ratio > 1 + c)) | ((adv < 0) & (ratio < 1 - c))
        dlp = torch.where(gate, torch.zeros_like(adv), -adv * ratio * inv_m)
        g["log_std"] += (dlp[:, None] * (z * z - 1)).sum(0)
        S["log_std"] += (dlp[:, None] * (z * z - 1)).abs().sum(0)
        d1 = v - ret
        Lv, dv = d1 * d1, 2 * d1
        if cv is not None:
            vo = b["v_old"][sl]
            d2 = vo + torch.clamp(v - vo, -cv, cv) - ret
            Lv = torch.maximum(d1 * d1, d2 * d2)
            dv = torch.where(d1 * d1 >= d2 * d2, 2 * d1, torch.where((v - vo).abs() < cv, 2 * d2, torch.zeros_like(d1)))
        sums += torch.stack([Lpi.sum(), Lv.sum(), (lpo - logp).sum(), ((ratio - 1).abs() > c).to(dtype).sum()])
        mag = lambda who, dims, f: f[1][-1].abs() @ p[f"{who}.{len(dims) - 2}.weight"].abs().T + p[f"{who}.{len(dims) - 2}.bias"].abs()
        A = (0.5 * z * z + ls.abs()).sum(-1) + 1.5 * LN2PI + lpo.abs() + (z.abs() * inv * mag("actor", a_dims, fa)).sum(-1)
        vmag = mag("critic", c_dims, fc)[:, 0] + ret.abs() + (b["v_old"][sl].abs() if cv is not None else 0)
        sc += torch.stack([(adv.abs() * ratio * (1 + A)).sum(), (vmag * vmag).sum(), A.sum()])
        for who, dims, f, delta in (("actor", a_dims, fa, dlp[:, None] * z * inv), ("critic", c_dims, fc, (vc * inv_m * dv)[:, None])):
            _, xs, norms, _ = f
            for l in range(len(dims) - 2, -1, -1):
                W = p[f"{who}.{l}.weight"]
                g[f"{who}.{l}.weight"] += delta.T @ xs[l]
                g[f"{who}.{l}.bias"] += delta.sum(0)
                S[f"{who}.{l}.weight"] += delta.abs().T @ xs[l].abs()
                S[f"{who}.{l}.bias"] += delta.abs().sum(0)
                if l == 0 and norms[0] is None:
                    break
                da, y = delta @ W, xs[l]
                if norms[l] is not None:
                    name, y, xhat, rstd = norms[l]
                    g[name + ".weight"] += (da * xhat).sum(0)
                    g[name + ".bias"] += da.sum(0)
                    S[name + ".weight"] += (da * xhat).abs().sum(0)
                    S[name + ".bias"] += da.abs().sum(0)
                    if l == 0:
                        break
                    dxh = da if variant == "no_gamma" else da * p[name + ".weight"]
                    m2 = (dxh * xhat).mean(-1, keepdim=True)
                    da = rstd * (dxh - dxh.mean(-1, keepdim=True) - (0 if variant == "no_xhat_term" else xhat * m2))
                delta = da * ((1 - y * y) if act == "tanh" else (y > 0).to(dtype))
    g["log_std"] = g["log_std"] - ec
    S["log_std"] = S["log_std"] + ec
    H = ls.sum() + 1.5 * (1 + LN2PI)
    Lpi, Lv = sums[0] / M, sums[1] / M
    stats = torch.stack([Lpi, Lv, H, Lpi + vc * Lv - ec * H, sums[2] / M, sums[3] / M])
    Hs = ls.abs().sum() + 1.5 * (1 + LN2PI)
    stat_scales = torch.stack([sc[0] / M, sc[1] / M, Hs, sc[0] / M + vc * sc[1] / M + ec * Hs, sc[2] / M, torch.ones((), dtype=dtype)]).double()
    return g, stats, {k: float(v.max()) for k, v in S.items()}, stat_scales


# ---- the synthetic trajectory (ppo_ref.synth's, for networks with norms) ------------------------------------------------------------------------
def kinks(params, a_dims, c_dims, act, hidden, feat, b, cfg):
    """ppo_ref.kinks: bool per row (float64), the row is within the margins of a kink of the loss"""
    p = {k: v.double() for k, v in params.items()}
    c, cv = cfg["clip"], cfg["value_clip"]
    obs = b["obs"].double()
    bad = torch.zeros(obs.shape[0], dtype=torch.bool)
    outs = {}
    for who, dims in (("actor", a_dims), ("critic", c_dims)):
        outs[who], _, _, pres = forward(p, who, dims, act, hidden, feat, obs)
        if act == "relu":
            for pre in pres:
                bad |= (pre.abs() < 1e-4).any(-1)
    ls = p["log_std"]
    z = (b["actions"].double() - outs["actor"]) * torch.exp(-ls)
    ratio = torch.exp((-0.5 * z * z - ls).sum(-1) - 1.5 * LN2PI - b["logp_old"].double())
    bad |= ((ratio - (1 + c)).abs() < 1e-3) | ((ratio - (1 - c)).abs() < 1e-3) | (b["adv"].double().abs() < 1e-3)
    v, vo, ret = outs["critic"][:, 0], b["v_old"].double(), b["ret"].double()
    bad |= ((v - vo).abs() - cv).abs() < 1e-3
    v_c = vo + torch.clamp(v - vo, -cv, cv)
    bad |= ((v - vo).abs() > cv) & (((v - ret) ** 2 - (v_c - ret) ** 2).abs() < 1e-3)
    return bad


def synth(case, shape, M, seed, extra_stride=8, guard=64, weight_scale=1.0):
    """ppo_ref.synth for CASES[case]: a seeded kink-free trajectory of `shape` = (N, A', T, D) in mqe_ppo_grad's buffers (the same keys), with
    the norms' parameters in `params`, `hidden` and `feat`.  Rows inside a kink margin are drawn again (ppo_ref's redraw rule)."""
    N, Aw, T, D = shape
    R = N * Aw
    n = T * R
    assert n >= M
    a_dims, c_dims, act, hidden, feat = dims_of(case, D)
    params = seeded_params(a_dims, c_dims, hidden, feat, 500 + seed, weight_scale)
    cfg = dict(clip=CLIP, value_clip=VALUE_CLIP)
    g = torch.Generator().manual_seed(seed)
    p64 = {k: v.double() for k, v in params.items()}
    ls = p64["log_std"]

    def draw(k):
        obs = torch.randn(k, D, generator=g).float()
        mean = forward(p64, "actor", a_dims, act, hidden, feat, obs.double())[0]
        v = forward(p64, "critic", c_dims, act, hidden, feat, obs.double())[0][:, 0]
        actions = (mean + torch.exp(ls) * torch.randn(k, 3, generator=g).double()).float()
        z = (actions.double() - mean) * torch.exp(-ls)
        logp = (-0.5 * z * z - ls).sum(-1) - 1.5 * LN2PI
        return dict(obs=obs, actions=actions, logp_old=(logp + 0.25 * torch.randn(k, generator=g).double()).float(),
                    adv=torch.randn(k, generator=g).float(), v_old=(v + 0.3 * torch.randn(k, generator=g).double()).float(),
                    ret=(v + torch.randn(k, generator=g).double()).float())

    b = draw(n)
    redraws = 0
    for _ in range(200):
        bad = torch.nonzero(kinks(params, a_dims, c_dims, act, hidden, feat, b, cfg))[:, 0]
        if len(bad) == 0:
            break
        redraws += len(bad)
        fresh = draw(len(bad))
        for k in b:
            b[k][bad] = fresh[k]
    else:
        raise RuntimeError("synth: rows inside a kink margin remain")
    nobs = R * D
    pf = nobs + R + (N + 3) // 4
    stride = (pf + 3) // 4 * 4 + extra_stride
    packed = np.full((T + 1) * stride + guard, SENT, np.int32)
    rows = packed[:(T + 1) * stride].reshape(T + 1, stride)
    rows[:T, :nobs] = b["obs"].numpy().reshape(T, nobs).view(np.int32)
    rows[T, :nobs] = torch.randn(nobs, generator=g).float().numpy().view(np.int32)
    value = np.concatenate([b["v_old"].numpy(), torch.randn(R, generator=g).float().numpy()]).view(np.int32).copy()
    n_params = abi.actor_param_count(a_dims, c_dims, False, hidden, feat)
    out = lambda k: np.full(k + guard, SENT, np.int32)
    index = torch.randperm(n, generator=g).to(torch.int32)
    return dict(net=case, shape=shape, N=N, Aw=Aw, T=T, D=D, R=R, n=n, nobs=nobs, pf=pf, stride=stride, guard=guard, params=params, a_dims=a_dims,
                c_dims=c_dims, act=act, hidden=hidden, feat=feat, n_params=n_params, index=index, redraws=redraws, packed=packed, value=value,
                grad=out(n_params), stats=out(abi.PPO_STATS), **b)


def args_of(s, sel, cfg):
    """the positional arguments of manual() / autograd() for the minibatch `sel` of a synthetic trajectory"""
    return s["params"], s["a_dims"], s["c_dims"], s["act"], s["hidden"], s["feat"], ppo_ref.batch(s, sel), cfg


def flat_grad(g, s):
    """{name: tensor} -> the engine's flat layout (float64)"""
    flat = torch.zeros(s["n_params"], dtype=torch.float64)
    for name, (off, shape) in layout(s["a_dims"], s["c_dims"], s["hidden"], s["feat"]).items():
        flat[off:off + int(np.prod(shape))] = g[name].reshape(-1).double()
    return flat
