"""Host restatements for the on-device rollout's tests (mqe_rollout, csrc/kernels_actor.hpp): the counter RNG's N(0, 1) draws
(mqe_hash -> mqe_u01 -> the Box-Muller statement of kernels_step.hpp) in float64, seeded network parameters in the engine's layout, and
the networks in torch at any precision."""
import math

import numpy as np
import torch

from mqe.engine import abi

M32 = 0xFFFFFFFF


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


def seeded_params(actor_dims, critic_dims, seed):
    """{name: float32 tensor} in abi.actor_param_layout's names: weights and biases uniform in +-1 / sqrt(fan_in) (activations O(1), tanh not
    saturated everywhere), log_std uniform in [-1, 0.5]"""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for name, (_, shape) in abi.actor_param_layout(actor_dims, critic_dims).items():
        if name == "log_std":
            out[name] = torch.rand(3, generator=g) * 1.5 - 1.0
        else:
            who, l, _ = name.split(".")
            fan_in = (actor_dims if who == "actor" else critic_dims)[int(l)]
            out[name] = (torch.rand(*shape, generator=g) * 2 - 1) / math.sqrt(fan_in)
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


def gaussian_logp(a, mean, log_std):
    """sum_j of log N(a_j; mean_j, exp(log_std_j)^2), in the arguments' dtype"""
    z = (a - mean) / torch.exp(log_std)
    return (-0.5 * z * z - log_std - 0.5 * math.log(2 * math.pi)).sum(-1)
