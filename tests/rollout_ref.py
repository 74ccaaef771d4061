"""Host restatements for the on-device rollout's tests (mqe_rollout, csrc/kernels_actor.hpp): the counter RNG's N(0, 1) draws
(mqe_hash -> mqe_u01 -> the Box-Muller statement of kernels_step.hpp) in float64, seeded network parameters in the engine's layout, and
the networks in torch at any precision: `mlp`, the rollout tests' plain twin, and `forward`, the one walk of the PPO and layer-normalisation
references (ppo_ref.py, layer_norm_ref.py) with the norm's twin `layer_norm` (csrc/kernels_ln.hpp) in front of it."""
import math

import numpy as np
import torch

from mqe.engine import abi

M32 = 0xFFFFFFFF
LN_EPS = 1e-5
WAVES = 16                     # csrc/kernels_actor.hpp ACT_WAVES: the norm's features are split over them in consecutive chunks


def hash_u32(seed, genv, count, k):
    """mqe_hash (csrc/mqe_common.hpp) on numpy arrays / ints, uint32 arithmetic carried in uint64"""
    seed, genv, count, k = (np.asarray(v, np.uint64) & np.uint64(M32) for v in (seed, genv, count, k))
    m = lambda a, c: (a * np.uint64(c)) & np.uint64(M32)
    x = m(seed, 0x9E3779B1) ^ m(genv, 0x85EBCA77) ^ m(count, 0xC2B2AE3D) ^ m(k, 0x27D4EB2F)
    x ^= x >> np.uint64(16); x = m(x, 0x85EBCA6B); x ^= x >> np.uint64(13); x = m(x, 0xC2B2AE35); x ^= x >> np.uint64(16)
    return x


def u01(seed, genv, count, k):
    """mqe_u01: the top 24 bits / 2^24 -- exact in float32 and in float64"""
    return (hash_u32(seed, genv, count, k) >> np.uint64(8)).astype(np.float64) / 16777216.0


def randn(seed, genv, count, k):
    """mqe_randn_key in float64: sqrt(-2 log(1 - u1)) cos(6.2831855f u2), u1 / u2 = the draws 2k / 2k + 1.  1 - u1 is exact in float32 (a
    multiple of 2^-24 in (0, 1]); the angle is the float32 product the kernel forms, so the only differences from the kernel are its float32 logf, sqrtf, cosf and the
    two roundings of the products"""
    k = np.asarray(k, np.uint64)
    u1, u2 = u01(seed, genv, count, 2 * k), u01(seed, genv, count, 2 * k + 1)
    ang = (np.float32(6.2831855) * u2.astype(np.float32)).astype(np.float64)
    return np.sqrt(-2.0 * np.log(1.0 - u1)) * np.cos(ang)


def actor_draws(seed, env_offset, N, Aw, n0, T):
    """(T, N, Aw, 3) float64: z of rollout step t (the post-physics step counter stands at n0 + t when its k_actor is enqueued), env e,
    agent a, action column j -- key (seed, e + env_offset, RNG_ACTOR + n0 + t, a * 3 + j)"""
    t = np.arange(T).reshape(T, 1, 1, 1)
    e = np.arange(N).reshape(1, N, 1, 1) + env_offset
    a = np.arange(Aw).reshape(1, 1, Aw, 1)
    j = np.arange(3).reshape(1, 1, 1, 3)
    return randn(seed, e, abi.RNG_ACTOR + n0 + t, a * 3 + j)


def seeded_params(actor_dims, critic_dims, seed, hidden=False, feat=False, weight_scale=1.0):
    """{name: float32 tensor} in abi.actor_param_layout's names: Linear weights and biases uniform in +-1 / sqrt(fan_in) (activations O(1), tanh
    not saturated everywhere), log_std uniform in [-1, 0.5], a norm's weight uniform in [0.5, 1.5] and its bias in [-0.5, 0.5].  weight_scale
    multiplies the weight and the bias of layer 0, so that the activations of a row differ little: a variance near eps"""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for name, (_, shape) in abi.actor_param_layout(actor_dims, critic_dims, False, hidden, feat).items():
        part = name.split(".")
        if name == "log_std":
            out[name] = torch.rand(3, generator=g) * 1.5 - 1.0
        elif "norm" in part[1] or part[2] == "norm":
            out[name] = torch.rand(*shape, generator=g) + (0.5 if part[-1] == "weight" else -0.5)
        else:
            fan_in = (actor_dims if part[0] == "actor" else critic_dims)[int(part[1])]
            out[name] = (torch.rand(*shape, generator=g) * 2 - 1) / math.sqrt(fan_in)
            if part[1] == "0":
                out[name] = out[name] * weight_scale
    return out


def flat_params(params, actor_dims, critic_dims):
    """the dict above as the engine's flat buffer"""
    flat = torch.zeros(abi.actor_param_count(actor_dims, critic_dims))
    for name, (off, shape) in abi.actor_param_layout(actor_dims, critic_dims).items():
        flat[off:off + int(np.prod(shape))] = params[name].reshape(-1).float()
    return flat


def mlp(params, who, n_layers, activation, x):
    """the network `who` on x (..., D) in x's dtype: Linear, activation, ..., Linear"""
    for l in range(n_layers):
        x = x @ params[f"{who}.{l}.weight"].to(x.dtype).T + params[f"{who}.{l}.bias"].to(x.dtype)
        if l + 1 < n_layers:
            x = torch.tanh(x) if activation == "tanh" else torch.relu(x)
    return x


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


def forward(p, who, dims, act, x, hidden=False, feat=False, kernel_order=False, variant=None, functional=False):
    """The network `who` in the dtype of p and x, with the hidden and the feature norm or without: -> (out, xs, norms, pres): xs[l] the input
    of Linear l; norms[l] = (name, a, xhat, rstd) of the norm in front of it or None; pres the hidden pre-activations.  functional: the norm
    is torch.nn.functional.layer_norm (autograd's reference).  variant "norm_before_act": the hidden norm in front of the activation instead
    of behind it."""
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


def gaussian_logp(a, mean, log_std):
    """sum_j of log N(a_j; mean_j, exp(log_std_j)^2), in the arguments' dtype"""
    z = (a - mean) / torch.exp(log_std)
    return (-0.5 * z * z - log_std - 0.5 * math.log(2 * math.pi)).sum(-1)
