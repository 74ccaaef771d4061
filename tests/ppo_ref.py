"""Host side of the PPO tests (mqe_ppo_grad, mqe_ppo_adam; csrc/kernels_ppo.hpp): the loss in torch (for autograd), a manual backward at any
dtype (float64 is the reference; float32, whole batch or tile by tile, is the yardstick), deliberately wrong variants, Adam with the norm
clip, the seeded kink-free trajectory in mqe_rollout's layout that the CPU and the GPU tests share, and the tolerances.  Every loss function
takes hidden= and feat=, the two layer-norm switches (csrc/kernels_ln.hpp; tests/layer_norm_ref.py holds its cases and its K): one statement
of the loss and of its backward for the plain networks and for those with norms, on the one walk rollout_ref.forward.

THE GRADIENT BOUND.  For every parameter tensor n the float64 backward also yields S_n, the largest entry of the sum over the samples of the
ABSOLUTE per-sample contributions (|Delta|^T |X| for a weight, sum |Delta| for a bias, sum |dlogp (z^2 - 1)| + entropy_coef for log_std):
the magnitude that the roundings of any summation order act on.  The bound is |g - g64| <= K 2^-24 S_n for every entry of tensor n, and an
exactly zero gradient where S_n = 0.  The statistics use the same K with the scales of `stat_scales`.  K is MEASURED ON THE CPU, never on
the kernel: the largest ratio |g32 - g64| / (2^-24 S_n) reached over K_CASES by two float32 evaluations -- torch autograd on the whole batch,
and the manual backward accumulated serially over tiles of 64 rows.  tests/test_ppo.py asserts that both stay inside K_CPU; the GPU test
allows K_GPU = 4 K_CPU (the project's margin for k_actor: the kernel differs from the CPU by its tanhf / expf).

Measured with this file (tests/test_ppo.py prints every case; 75 cases: 5 networks x M in {1, 63, 130, 1000, 4099} x 3 seeds; value clipping
on, entropy_coef 0.01; the larger of the two float32 evaluations, gradient tensors and statistics together), largest ratio per network and M:
                   M = 1     63    130   1000   4099
    tanh64x64        5.7    6.3   11.3    1.4    0.8
    tanh7           11.4    2.9    5.8    1.3    0.8
    relu128x3       21.3    4.4    8.7    1.6    3.2
    tanh256x3        7.8    5.9    8.5    2.1    0.9
    relu17x5        20.0    3.0    6.5    2.0    1.7
The maximum is 21.33 (relu128x3, M = 1, actor.1.weight: with one sample nothing averages and the scale is a single product); from M = 1000
up the gradient ratio stays under 2.1 (the 3.2 is a statistic).  Rejected rows: 1.5 - 2.5 % for the tanh networks and relu17x5, 37 - 40 %
for relu128x3.  K_CPU = 22 is that maximum rounded up to the next integer; it is NOT taken from anything the kernel computes."""
import math

import numpy as np
import torch

from mqe.engine import abi
import rollout_ref
from rollout_ref import forward

EPS32 = 2.0 ** -24
SENT = 0x7FC12345
LN2PI = math.log(2 * math.pi)
CLIP, VALUE_CLIP = 0.2, 0.2                  # the constants the generator's kink margins are built around
K_CPU = 22.0
K_GPU = 4 * K_CPU

NETS = {"tanh64x64": ("tanh", (64, 64)), "tanh7": ("tanh", (7,)), "relu128x3": ("relu", (128, 128, 128)), "tanh256x3": ("tanh", (256, 256, 256)),
        "relu17x5": ("relu", (17, 5))}
K_MS = (1, 63, 130, 1000, 4099)
K_CASES = [(net, M, seed) for net in NETS for M in K_MS for seed in (0, 1, 2)]


def dims_of(net, D):
    act, hidden = NETS[net]
    return [D, *hidden, 3], [D, *hidden, 1], act


def shape_for(M, D=16):
    """the smallest (N, A' = 2, T, D) used for an M-sample CPU case"""
    T = 1 if M < 8 else (7 if M < 200 else 63)
    N = -(-M // (2 * T))
    return (N, 2, T, D)


# ---- the loss ---------------------------------------------------------------------------------------------------------------------------
def loss_torch(params, a_dims, c_dims, act, b, cfg, variant=None, hidden=False, feat=False):
    """the stated loss as a torch expression (for autograd) in the dtype of params: -> (L, stats[6]).  A norm is torch.nn.functional.layer_norm
    unless a wrong network is asked for (variant: layer_norm_ref.VARIANTS_FORWARD)"""
    c, vc, ec, cv = cfg["clip"], cfg["value_coef"], cfg["entropy_coef"], cfg["value_clip"]
    ls = params["log_std"]
    net = dict(hidden=hidden, feat=feat, variant=variant, functional=variant is None)
    mean = forward(params, "actor", a_dims, act, b["obs"], **net)[0]
    v = forward(params, "critic", c_dims, act, b["obs"], **net)[0][:, 0]
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


def autograd(params, a_dims, c_dims, act, b, cfg, dtype, variant=None, hidden=False, feat=False):
    """torch autograd of loss_torch at `dtype` on the whole batch: -> ({name: grad}, stats)"""
    p = {k: v.to(dtype).clone().requires_grad_(True) for k, v in params.items()}
    bb = {k: v.to(dtype) for k, v in b.items()}
    L, stats = loss_torch(p, a_dims, c_dims, act, bb, cfg, variant, hidden, feat)
    L.backward()
    return {k: (v.grad if v.grad is not None else torch.zeros_like(v)).detach() for k, v in p.items()}, stats.detach()


def manual(params, a_dims, c_dims, act, b, cfg, dtype=torch.float64, tile=None, variant=None, hidden=False, feat=False):
    """The manual backward at `dtype`: the gradient as csrc/kernels_ppo.hpp states it (selects at the kinks) and the norms' backward as
    csrc/kernels_ln.hpp does (float32: the norm in the kernel's order), accumulated over tiles of `tile` rows in order (None: the whole batch
    at once).  -> (grads, stats[6], S, stat_scales): S[name] = the scale S_n of the module docstring (for a norm: sum |du xhat| for its weight,
    sum |du| for its bias).  variant, each a wrong gradient: "gate_ignored", "no_inv_m", "entropy_sign", "value_clip_ignored", "z_no_inv"; of
    the norm's backward: "no_gamma" (dxhat = du), "no_xhat_term" (the xhat * mean(dxhat xhat) term dropped)."""
    c, vc, ec, cv = cfg["clip"], cfg["value_coef"], cfg["entropy_coef"], cfg["value_clip"]
    if variant == "value_clip_ignored":
        cv = None
    p = {k: v.to(dtype) for k, v in params.items()}
    b = {k: v.to(dtype) for k, v in b.items()}
    M = b["obs"].shape[0]
    inv_m = 1.0 if variant == "no_inv_m" else 1.0 / M
    ls = p["log_std"]
    inv = torch.exp(-ls) if variant != "z_no_inv" else torch.ones_like(ls)
    g = {k: torch.zeros_like(v) for k, v in p.items()}
    S = {k: torch.zeros_like(v) for k, v in p.items()}
    sums = torch.zeros(4, dtype=dtype)           # L_pi, L_v, logp_old - logp, clipped
    sc = torch.zeros(3, dtype=dtype)             # scales of L_pi, L_v, KL sums
    net = dict(hidden=hidden, feat=feat, kernel_order=dtype == torch.float32)
    tile = tile or M
    for r0 in range(0, M, tile):
        sl = slice(r0, min(r0 + tile, M))
        obs = b["obs"][sl]
        fa = forward(p, "actor", a_dims, act, obs, **net)
        fc = forward(p, "critic", c_dims, act, obs, **net)
        # actor head
        mean, v = fa[0], fc[0][:, 0]
        z = (b["actions"][sl] - mean) * inv
        logp = (-0.5 * z * z - ls).sum(-1) - 1.5 * LN2PI
        lpo, adv, ret = b["logp_old"][sl], b["adv"][sl], b["ret"][sl]
        ratio = torch.exp(logp - lpo)
        Lpi = -torch.minimum(ratio * adv, torch.clamp(ratio, 1 - c, 1 + c) * adv)
        gate = ((adv > 0) & (ratio > 1 + c)) | ((adv < 0) & (ratio < 1 - c))
        dlp = -adv * ratio * inv_m
        if variant != "gate_ignored":
            dlp = torch.where(gate, torch.zeros_like(dlp), dlp)
        g["log_std"] += (dlp[:, None] * (z * z - 1)).sum(0)
        S["log_std"] += (dlp[:, None] * (z * z - 1)).abs().sum(0)
        # critic head
        d1 = v - ret
        Lv, dv = d1 * d1, 2 * d1
        if cv is not None:
            vo = b["v_old"][sl]
            d2 = vo + torch.clamp(v - vo, -cv, cv) - ret
            Lv = torch.maximum(d1 * d1, d2 * d2)
            dv = torch.where(d1 * d1 >= d2 * d2, 2 * d1, torch.where((v - vo).abs() < cv, 2 * d2, torch.zeros_like(d1)))
        sums += torch.stack([Lpi.sum(), Lv.sum(), (lpo - logp).sum(), ((ratio - 1).abs() > c).to(dtype).sum()])
        # the magnitudes that the last layers' sums act on, for the statistics' scales
        mag = lambda who, dims, f: f[1][-1].abs() @ p[f"{who}.{len(dims) - 2}.weight"].abs().T + p[f"{who}.{len(dims) - 2}.bias"].abs()
        A = (0.5 * z * z + ls.abs()).sum(-1) + 1.5 * LN2PI + lpo.abs() + (z.abs() * inv * mag("actor", a_dims, fa)).sum(-1)
        vmag = mag("critic", c_dims, fc)[:, 0] + ret.abs() + (b["v_old"][sl].abs() if cv is not None else 0)
        sc += torch.stack([(adv.abs() * ratio * (1 + A)).sum(), (vmag * vmag).sum(), A.sum()])
        # the two networks, top layer down
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
    g["log_std"] = g["log_std"] + (ec if variant == "entropy_sign" else -ec)
    S["log_std"] = S["log_std"] + ec
    H = ls.sum() + 1.5 * (1 + LN2PI)
    Lpi, Lv = sums[0] / M, sums[1] / M
    stats = torch.stack([Lpi, Lv, H, Lpi + vc * Lv - ec * H, sums[2] / M, sums[3] / M])
    Hs = ls.abs().sum() + 1.5 * (1 + LN2PI)
    stat_scales = torch.stack([sc[0] / M, sc[1] / M, Hs, sc[0] / M + vc * sc[1] / M + ec * Hs, sc[2] / M, torch.ones((), dtype=dtype)]).double()
    return g, stats, {k: float(v.max()) for k, v in S.items()}, stat_scales


def ratio_to_bound(g, g64, S):
    """max over the tensors of max |g - g64| / (2^-24 S_n); a tensor with S_n = 0 must be exactly 0 (ratio inf otherwise) -> (ratio, name)"""
    worst, at = 0.0, None
    for name, s in S.items():
        d = float((g[name].double() - g64[name].double()).abs().max())
        r = (0.0 if d == 0.0 else math.inf) if s == 0.0 else d / (EPS32 * s)
        if r >= worst:
            worst, at = r, name
    return worst, at


def stats_ratio(stats, stats64, scales):
    """the same for the six statistics (entry 5, the clip share, has scale 1: kink-free inputs give the same count)"""
    return float(((stats.double() - stats64.double()).abs() / (EPS32 * scales)).max())


# ---- Adam ---------------------------------------------------------------------------------------------------------------------------------
def adam(p, m, v, g, step, lr, b1=0.9, b2=0.999, eps=1e-8, max_norm=None, dtype=torch.float64, f32_args=True):
    """one step of torch.optim.Adam (no weight decay, no amsgrad) behind clip_grad_norm_, as include/mqe_hip.h states it: -> (p, m, v, norm).
    f32_args: lr, b1, b2, eps and max_norm are first rounded to float32 -- mqe_ppo_adam takes them as floats, so THOSE are the inputs (1 -
    float32(0.999) differs from 0.001 by 2^-15 relative: an input, not an error).  float32: the kernel's chain -- the derived constants formed in
    float64 and rounded once, fmaf where the kernel has one."""
    f32 = dtype == torch.float32
    if f32_args:
        lr, b1, b2, eps = (float(np.float32(x)) for x in (lr, b1, b2, eps))
        max_norm = float(np.float32(max_norm)) if max_norm is not None else None
    g64 = g.double()
    norm = torch.sqrt((g64 * g64).sum())
    cast = (lambda x: torch.tensor(x, dtype=torch.float64).float()) if f32 else (lambda x: torch.tensor(x, dtype=torch.float64))
    p, m, v, g = p.to(dtype), m.to(dtype), v.to(dtype), g.to(dtype)
    if max_norm is not None and max_norm > 0:
        scale = torch.clamp(cast(max_norm) / (norm.to(dtype) + cast(1e-6)), max=1.0)
        g = g * scale
    omb1, omb2 = cast(1.0 - b1), cast(1.0 - b2)
    step_size, bc2s = cast(lr / (1.0 - b1 ** step)), cast(math.sqrt(1.0 - b2 ** step))
    if f32:
        fma = lambda a, x, y: (a.double() * x.double() + y.double()).float()
        m = fma(cast(b1), m, omb1 * g)
        v = fma(cast(b2), v, (omb2 * g) * g)
    else:
        m = b1 * m + omb1 * g
        v = b2 * v + omb2 * g * g
    p = p - (step_size * m) / (torch.sqrt(v) / bc2s + cast(eps))
    return p, m, v, float(norm)


def adam_tolerances(p, m, v, g, step, lr, b1=0.9, b2=0.999, eps=1e-8, max_norm=None):
    """(tol_p, tol_m, tol_v) per element, DERIVED from the chain of csrc/kernels_ppo.hpp by counting roundings of relative size e = 2^-24
    (the 2.5-ulp division and square root count 2.5), from the float64 step of the float32 inputs (hyperparameters included: adam(f32_args=True)):
      scale  = min(1, max_norm / ((float) norm + 1e-6)): the f32 store of the f64 norm, the sum, the division: 4.5 e;   g' = g scale: 5.5 e, <= 6 e
             (without clipping g' = g exactly; the bound is kept)
      m'     = fmaf(b1, m, omb1 g'): omb1 = 1 - b1 rounded to f32 (1 e), the product (1 e), g' (6 e), the fmaf (1 e of the result, itself at most the
               sum of the magnitudes): |dm| <= 9 e (b1 |m| + (1 - b1) |g|) =: em
      v'     = fmaf(b2, v, (omb2 g') g'): all terms positive: <= (1 + 2 x 6 + 2 + 1) e = 16 e relative
      denom  = sqrt(v') / bc2s + eps: half of v's 16 e, sqrt 2.5, bc2s 1, the division 2.5, the sum 1 (eps as f32: 1 e of a term below the sum): 16 e
      upd    = (step_size m') / denom: step_size 1 e, product 1 e, division 2.5 e, denom 16 e: |d upd| <= step_size em / denom + 20.5 e |upd|
      p'     = p - upd: one rounding of the result: e max(|p|, |p'|)."""
    e = EPS32
    p64, m64, v64, _ = adam(p, m, v, g, step, lr, b1, b2, eps, max_norm)
    lr, b1, b2, eps = (float(np.float32(x)) for x in (lr, b1, b2, eps))
    gs = g.double()
    if max_norm is not None and max_norm > 0:
        gs = gs * min(1.0, max_norm / (float(torch.sqrt((gs * gs).sum())) + 1e-6))
    em = 9 * e * (b1 * m.double().abs() + (1 - b1) * gs.abs())
    ev = 16 * e * v64
    step_size = lr / (1.0 - b1 ** step)
    denom = torch.sqrt(v64) / math.sqrt(1.0 - b2 ** step) + eps
    upd = step_size * m64.abs() / denom
    tol_p = abs(step_size) * em / denom + 20.5 * e * upd + e * torch.maximum(p.double().abs(), p64.abs())
    return tol_p, em + 1e-45, ev + 1e-45


# ---- the synthetic trajectory -----------------------------------------------------------------------------------------------------------
def kinks(params, a_dims, c_dims, act, b, cfg, hidden=False, feat=False):
    """bool per row (float64): the row is within the margins of a kink of the loss"""
    p = {k: v.double() for k, v in params.items()}
    c, cv = cfg["clip"], cfg["value_clip"]
    obs = b["obs"].double()
    bad = torch.zeros(obs.shape[0], dtype=torch.bool)
    outs = {}
    for who, dims in (("actor", a_dims), ("critic", c_dims)):
        outs[who], _, _, pres = forward(p, who, dims, act, obs, hidden, feat)
        if act == "relu":
            for pre in pres:
                bad |= (pre.abs() < 1e-4).any(-1)
    ls = p["log_std"]
    z = (b["actions"].double() - outs["actor"]) * torch.exp(-ls)
    ratio = torch.exp((-0.5 * z * z - ls).sum(-1) - 1.5 * LN2PI - b["logp_old"].double())
    bad |= ((ratio - (1 + c)).abs() < 1e-3) | ((ratio - (1 - c)).abs() < 1e-3) | (b["adv"].double().abs() < 1e-3)
    if cv is not None:
        v, vo, ret = outs["critic"][:, 0], b["v_old"].double(), b["ret"].double()
        bad |= ((v - vo).abs() - cv).abs() < 1e-3
        v_c = vo + torch.clamp(v - vo, -cv, cv)
        bad |= ((v - vo).abs() > cv) & (((v - ret) ** 2 - (v_c - ret) ** 2).abs() < 1e-3)
    return bad


def synth(net, shape, M, seed, pseed=None, extra_stride=8, guard=64, dims=None, hidden=False, feat=False, weight_scale=1.0):
    """A seeded kink-free trajectory of `shape` = (N, A', T, D) for the network NETS[net], in mqe_ppo_grad's buffers, with at least M samples.
    Every one of the n = T N A' rows is drawn -- observation N(0, 1); action = mean64 + exp(log_std) N(0, 1); logp_old = logp64 + 0.25 N(0, 1)
    (ratios on both sides of 1 +- CLIP); adv N(0, 1); v_old = v64 + 0.3 N(0, 1) (both sides of VALUE_CLIP); ret = v64 + N(0, 1) -- and
    every row inside a kink margin (kinks(), with CLIP and VALUE_CLIP) is drawn again until none is left, so that ANY minibatch of it is
    kink-free.  dims: (a_dims, c_dims, act) of a network that NETS does not hold; hidden, feat: with the norms, whose parameters join `params`;
    weight_scale: rollout_ref.seeded_params'.  -> dict: params (float32 tensors), a_dims, c_dims, act, the logical float32 tensors obs (n, D), actions (n, 3), logp_old, v_old,
    adv, ret (n), index (a seeded int32 permutation of n), redraws (rows drawn again, in all), and the flat int32 images: `packed` ((T + 1)
    stride + guard words: the observations of rows 0 .. T in place, everything else the sentinel), `value` ((T + 1) R': v_old, then a filler
    row), `grad` (n_params + guard) and `stats` (6 + guard), both all sentinel."""
    N, Aw, T, D = shape
    R = N * Aw
    n = T * R
    assert n >= M
    a_dims, c_dims, act = dims or dims_of(net, D)
    norms = dict(hidden=hidden, feat=feat)
    params = rollout_ref.seeded_params(a_dims, c_dims, 500 + seed if pseed is None else pseed, hidden, feat, weight_scale)
    cfg = dict(clip=CLIP, value_clip=VALUE_CLIP)
    g = torch.Generator().manual_seed(seed)
    p64 = {k: v.double() for k, v in params.items()}
    ls = p64["log_std"]

    def draw(k):
        obs = torch.randn(k, D, generator=g).float()
        mean = forward(p64, "actor", a_dims, act, obs.double(), **norms)[0]
        v = forward(p64, "critic", c_dims, act, obs.double(), **norms)[0][:, 0]
        actions = (mean + torch.exp(ls) * torch.randn(k, 3, generator=g).double()).float()
        z = (actions.double() - mean) * torch.exp(-ls)
        logp = (-0.5 * z * z - ls).sum(-1) - 1.5 * LN2PI
        return dict(obs=obs, actions=actions, logp_old=(logp + 0.25 * torch.randn(k, generator=g).double()).float(),
                    adv=torch.randn(k, generator=g).float(), v_old=(v + 0.3 * torch.randn(k, generator=g).double()).float(),
                    ret=(v + torch.randn(k, generator=g).double()).float())

    b = draw(n)
    redraws = 0
    for _ in range(200):
        bad = torch.nonzero(kinks(params, a_dims, c_dims, act, b, cfg, **norms))[:, 0]
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
    return dict(net=net, shape=shape, N=N, Aw=Aw, T=T, D=D, R=R, n=n, nobs=nobs, pf=pf, stride=stride, guard=guard, params=params, a_dims=a_dims,
                c_dims=c_dims, act=act, **norms, n_params=n_params, index=index, redraws=redraws, packed=packed, value=value, grad=out(n_params),
                stats=out(abi.PPO_STATS), **b)


def batch(s, sel):
    """the minibatch `sel` (a tensor or slice of sample numbers) of a synthetic trajectory, as manual() / autograd() take it"""
    if isinstance(sel, torch.Tensor):
        sel = sel.long()
    return {k: s[k][sel] for k in ("obs", "actions", "logp_old", "v_old", "adv", "ret")}


def flat_grad(g, a_dims, c_dims, hidden=False, feat=False):
    """{name: tensor} -> the engine's flat layout (float64)"""
    flat = torch.zeros(abi.actor_param_count(a_dims, c_dims, False, hidden, feat), dtype=torch.float64)
    for name, (off, shape) in abi.actor_param_layout(a_dims, c_dims, False, hidden, feat).items():
        flat[off:off + int(np.prod(shape))] = g[name].reshape(-1).double()
    return flat


def split_flat(flat, a_dims, c_dims, hidden=False, feat=False):
    """the engine's flat layout -> {name: tensor}"""
    layout = abi.actor_param_layout(a_dims, c_dims, False, hidden, feat)
    return {name: flat[off:off + int(np.prod(shape))].reshape(shape) for name, (off, shape) in layout.items()}
