"""Host side of the tests of the transformer's on-device PPO gradient (mqe_ppo_grad with MQE_PPO_TRANSFORMER; csrc/kernels_mat_grad.hpp: k_mat_grad):
the loss as a torch expression on MATNet.evaluate -- its float64 autograd is THE reference --, a manual float64 backward written from the formulas the
kernel file states, the scales S_n from hooks on the float64 twin, deliberately wrong variants of the backward, and the synthetic trajectory.  No GPU, no
engine.  ppo_ref, joint_ref and mat_ref are imported and unchanged: the loss head (joint_ref.policy_head), the value head, the buffers and the seeded
networks are theirs.

THE UNIT is the env-step group: every batch here is (G, A', ...) -- G groups of the A' agents of one env-step, the layout MATNet.evaluate takes.  cfg
holds ppo_ref's keys and "joint" (bool), "dual_clip" (None or c_d).  THE LOSS (csrc/kernels_mat_grad.hpp):
    mean, value = MATNet.evaluate(obs, actions)            sigma_j = 0.5 sigmoid(log_std_j);  z_j = (a_j - mean_j) / sigma_j
    logp = sum_j (-0.5 z_j^2 - ln sigma_j) - 1.5 ln(2 pi);  H = sum_j ln sigma_j + 1.5 (1 + ln(2 pi))
    L = mean(L_pi) + value_coef mean(L_v) - entropy_coef H      with L_pi, L_v and the six statistics of csrc/kernels_ppo.hpp

THE BOUND has ppo_ref's form: |g - g64| <= K 2^-24 S_n for every entry of parameter tensor n, S_n the largest entry of the sum over the samples of the
ABSOLUTE per-sample contributions, taken from forward and full-backward hooks on the float64 twin (scales()): |Delta|^T |X| for a Linear weight, sum
|Delta| for a bias, sum |du xhat| and sum |du| for a norm's weight and bias, sum |dL/dlogp (z_j^2 - 1)| (1 - sigmoid) + entropy_coef (1 - sigmoid) for
log_std.  The statistics' scales are ppo_ref's (joint_ref's under the joint ratio) with ln sigma in the place of log_std.

K IS MEASURED ON THE CPU, never on the kernel: the largest ratio |g32 - g64| / (2^-24 S_n), gradient tensors and statistics together, reached by two
float32 evaluations -- torch autograd on the whole batch, and autograd accumulated serially over tiles of 64 rows -- over K_CASES: E in {64, 12, 4} x A'
in {1, 2, 4} x count in {1, 31, 65, 520} groups x 3 seeds x (plain; joint + dual clip + value clip), D = 16.  tests/test_mat_grad.py prints every case
and asserts the table.  Largest ratio per E and count (both losses, the three A', the three seeds, the larger of the two evaluations):
                 count = 1       31       65      520
    e64  (E = 64)     243.6    245.0    222.6     51.5
    e12  (E = 12)      78.9    116.8     71.3     26.0
    e4   (E = 4)     1154.5   2316.2   1461.9   5198.9
(the same with torch running 1, 4, 16 and its default number of threads, but e12 at 520 groups: 25.7 .. 26.0).  The maximum is 5198.9 (e4, A' = 2, 520
groups, joint + dual + value clip, seed 0, autograd on the whole batch, mat.dec.act_fc.weight): K_MAT_CPU, rounded up to the next integer, is 5199.
WHY SO LARGE, AND WHY K IS KEPT PER WIDTH.  S_n is made of the deltas that ARRIVE at a tensor; a LayerNorm's backward subtracts two means from its incoming
gradient, and over E = 4 features (and with ten norms in a row) what remains is a small difference of large terms whose roundings S_n does not see.  One
constant for all widths would let E = 64 and E = 12 pass with 20 and 40 times the error a float32 evaluation of THEM shows.  So the bound a width is held to
is the maximum of ITS row, rounded up (K_MAT_CPU_OF; never above K_MAT_CPU, so no test asks less than the one constant would), and K_MAT_GPU_OF = 4 x that:
the project's margin for a kernel that differs from the CPU by its expf / erff.  None of them is taken from anything the kernel computes.
BEYOND D = 16 AND E = 64 the same measurement per (E, D) (K_CASES_AT: the A' the GPU cases run at that pair, the four counts, both losses, three seeds,
both evaluations); largest ratio per pair and count:
                           count = 1       31       65      520
    (68, 16)  A' in {2, 4}     162.0    120.0    106.4     44.1
    (72, 16)  A' in {2, 4}     190.6    243.6    200.9     28.8
    (72, 13)  A' = 1            85.1     54.6     57.1     21.8
    (72, 34)  A' = 2            81.4    155.5     82.1     34.1
    (12, 34)  A' = 2            65.8    188.5    127.7    184.2
    (4, 34)   A' = 2           353.6    249.9    243.1   6798.2
    (12, 14)  A' = 2          2016.1    100.4     66.3     51.7
    (12, 20)  A' = 2           959.7     77.4    135.7     23.1
(the same with torch running 1, 16 and its default number of threads, but (72, 13) at 520 groups: 21.5 .. 21.8, and (12, 34) at one group: 65.8 .. 66.0).
K_MAT_CPU_AT is each row's maximum rounded up, K_MAT_GPU_AT = 4 x that.  The two one-group maxima, (12, 14) seed 2 at mat.dec.attn1.query.weight and
(12, 20) seed 1 at mat.enc.attn.query.weight, are the E = 4 effect in one group: S_n of a query weight is made of ds, which a single group's softmax
leaves small, and the roundings behind it are not.  (4, 34): mat.enc.obs_fc.weight, 520 groups, seed 2, plain, autograd on the whole batch.

THE WRONG VARIANTS (manual(variant=...)), each the float64 backward with one thing wrong: "no_r" the softmax Jacobian's - r_i term dropped; "mask_ignored"
dv and dk summed with the UNMASKED probabilities; "no_scale" c missing from dq and dk; "no_res_rep" the decoder's residual path into rep dropped;
"no_query_rep" attn2's query path into rep dropped; "enc_value_only" the encoder receiving the value head's gradient alone; "tanh_gelu" the derivative of
the tanh approximation; "no_one_minus_sigmoid" dlogp/dlog_std without (1 - sigmoid).  Gradient flowing into s is not listed: s is data in every
statement of the backward, there is no term to get wrong.  tests/test_mat_grad.py holds each outside 2 K_MAT_GPU_OF 2^-24 S_n at every width and A'
where it can differ (tanh_gelu at E = 4 on TANH_GELU_AT_E4's inputs); the weakest factor is recorded there."""
import copy
import math

import numpy as np
import torch

import joint_ref
import mat_ref
import ppo_ref
from joint_ref import pair, spread
from mqe.engine import abi
from ppo_ref import EPS32, LN2PI, SENT

CLIP, VALUE_CLIP, DUAL = ppo_ref.CLIP, ppo_ref.VALUE_CLIP, joint_ref.DUAL
K_MAT_CPU_OF = {64: 246.0, 12: 117.0, 4: 5199.0}          # per n_embd: the rows of the table above, rounded up
K_MAT_CPU = max(K_MAT_CPU_OF.values())
K_MAT_GPU_OF = {E: 4 * k for E, k in K_MAT_CPU_OF.items()}
K_MAT_GPU = 4 * K_MAT_CPU
LOSSES = {"plain": dict(joint=False, dual_clip=None, value_clip=None), "joint+dual+vclip": dict(joint=True, dual_clip=DUAL, value_clip=VALUE_CLIP)}
CFG = dict(clip=CLIP, value_coef=0.7, entropy_coef=0.01, value_clip=VALUE_CLIP, joint=False, dual_clip=None)
K_COUNTS = (1, 31, 65, 520)
K_CASES = [(name, Aw, count, loss, seed) for name in mat_ref.SHAPES for Aw in (1, 2, 4) for count in K_COUNTS for loss in LOSSES for seed in (0, 1, 2)]
# beyond D = 16 and E = 64: per (n_embd, D) the A' measured (those the GPU cases run there) and the row of the second table above, rounded up
K_AT_AGENTS = {(68, 16): (2, 4), (72, 16): (2, 4), (72, 13): (1,), (72, 34): (2,), (12, 34): (2,), (4, 34): (2,), (12, 14): (2,), (12, 20): (2,)}
K_MAT_CPU_AT = {(68, 16): 163.0, (72, 16): 244.0, (72, 13): 86.0, (72, 34): 156.0, (12, 34): 189.0, (4, 34): 6799.0, (12, 14): 2017.0, (12, 20): 960.0}
K_MAT_GPU_AT = {at: 4 * k for at, k in K_MAT_CPU_AT.items()}
K_CASES_AT = [(at, Aw, count, loss, seed) for at, agents in K_AT_AGENTS.items() for Aw in agents for count in K_COUNTS for loss in LOSSES for seed in (0, 1, 2)]
# the trajectories of tests/test_mat_grad_gpu.py: (N, A', T, D) and the widths; tests/test_mat_grad.py checks the generator's condition at every one
GPU_SHAPES = {"gate": ((37, 2, 3, 16), (64, 12, 4, 68, 72)), "football": ((17, 4, 4, 16), (12, 64, 72)), "plane": ((70, 1, 2, 13), (12, 64, 72)),
              "many": ((129, 2, 64, 16), (12,)),
              # the real tasks' own observations (go1sheep-hard, go1seesaw, go1football-defender)
              "sheep": ((37, 2, 3, 34), (72, 12, 4)), "seesaw": ((37, 2, 3, 14), (12,)), "defender": ((37, 2, 3, 20), (12,))}
# the widths of a set held to K_MAT_GPU_AT[(E, D)]; every other to K_MAT_GPU_OF[E], as before
EDGE_WIDTHS = {"gate": (68, 72), "football": (72,), "plane": (72,), "sheep": (72, 12, 4), "seesaw": (12,), "defender": (12,)}
_SYNTH, _POOL = {}, {}


def gpu_synth(what, E, **kw):
    """the shared trajectory of GPU_SHAPES[what] at width E (made once, never changed)"""
    key = (what, E, tuple(sorted(kw.items())))
    if key not in _SYNTH:
        shape, widths = GPU_SHAPES[what]
        assert E in widths
        _SYNTH[key] = synth(E, shape, 31 * len(what) + E, **kw)
    return _SYNTH[key]


def k_case(name, Aw, count, seed, D=16):
    """(net, batch) of a K case: the first `count` of 520 kink-free groups of (E, A', seed)"""
    key = (name, Aw, seed)
    if key not in _POOL:
        net = mat_ref.make_net(D, mat_ref.SHAPES[name], 500 + seed)
        _POOL[key] = (net, kink_free(net, max(K_COUNTS), Aw, D, 100 * seed + Aw)[0])
    net, b = _POOL[key]
    return net, {k: v[:count] for k, v in b.items()}


def k_case_at(E, D, Aw, count, seed):
    """k_case at a pair of K_MAT_CPU_AT: the same seeds, the width and the observation size given"""
    key = (E, D, Aw, seed)
    if key not in _POOL:
        net = mat_ref.make_net(D, E, 500 + seed)
        _POOL[key] = (net, kink_free(net, max(K_COUNTS), Aw, D, 100 * seed + Aw)[0])
    net, b = _POOL[key]
    return net, {k: v[:count] for k, v in b.items()}


WRONG = ("no_r", "mask_ignored", "no_scale", "no_res_rep", "no_query_rep", "enc_value_only", "tanh_gelu", "no_one_minus_sigmoid")
# cannot differ at A' = 1: one row, nothing masked; and p = 1 there, so ds = 0 and dq = dk = 0 -- with or without the scale, and nothing reaches rep through
# attn2's query
NEEDS_AGENTS = ("mask_ignored", "no_scale", "no_query_rep")
# the inputs on which the tanh_gelu variant is held to the bound at E = 4, per A': (groups, seed) of k_case.  With many groups S_n (a sum of absolute
# contributions) outgrows the variant's error, whose sign varies; with a few it does not
TANH_GELU_AT_E4 = {1: (4, 0), 2: (1, 3), 4: (8, 0)}
# the same at the pairs of K_MAT_CPU_AT whose bound is as loose, (E, D) -> A' -> (groups, seed) of k_case_at: E = 4 keeps its rule; at (12, 14) the row's
# maximum is a one-group case (2016; with 31 groups and more the pair stays below 101), and with 65 groups the variant reads 0.28 of the doubled bound
TANH_GELU_AT = {(4, 34): {2: TANH_GELU_AT_E4[2]}, (12, 14): {2: (1, 0)}}
KEYS = ("obs", "actions", "logp_old", "v_old", "adv", "ret")


def names(net):
    """the parameter names in the engine's order (MATNet.named_parameters), as abi.actor_param_layout(transformer=True) spells them"""
    return [("mat." + n) if n != "log_std" else n for n, _ in net.named_parameters()]


def flat(g, net):
    """{engine name: tensor} -> the engine's flat layout (float64)"""
    return torch.cat([g[n].reshape(-1).double() for n in names(net)])


def flat_bound(S, net):
    """S_n on every element of tensor n, flat"""
    return torch.cat([torch.full((p.numel(),), S[n], dtype=torch.float64) for n, (_, p) in zip(names(net), net.named_parameters())])


# ---- the loss ----------------------------------------------------------------------------------------------------------------------------------------
def _heads(net, mean, value, b, cfg, inv_m, inv_g, variant=None):
    """the two loss heads behind (mean, value), group-major flat: -> (L_pi, dL/dlogp, -Delta, rho, L_v, dL_v/dv, z, 1 / sigma, ln sigma) per sample"""
    Aw = mean.shape[-2]
    sig = torch.sigmoid(net.log_std)
    lsg, inv = torch.log(0.5 * sig), 1.0 / (0.5 * sig)
    z = ((b["actions"] - mean) * inv).reshape(-1, 3)
    logp = (-0.5 * z * z - lsg).sum(-1) - 1.5 * LN2PI
    Lpi, dlp, nd, rho = joint_ref.policy_head(torch, logp - b["logp_old"].reshape(-1), b["adv"].reshape(-1), cfg, Aw, inv_g, variant)
    v, ret, cv = value.reshape(-1), b["ret"].reshape(-1), cfg["value_clip"]
    d1 = v - ret
    Lv, dv = d1 * d1, 2 * d1
    if cv is not None:
        vo = b["v_old"].reshape(-1)
        d2 = vo + torch.clamp(v - vo, -cv, cv) - ret
        Lv = torch.maximum(d1 * d1, d2 * d2)
        dv = torch.where(d1 * d1 >= d2 * d2, 2 * d1, torch.where((v - vo).abs() < cv, 2 * d2, torch.zeros_like(d1)))
    return Lpi, dlp, nd, rho, Lv, dv, z, inv, lsg


def loss_torch(net, b, cfg, M=None, entropy=True):
    """the stated loss on MATNet.evaluate in the dtype of net: -> (L, sums[4]: L_pi, L_v, -Delta, clipped -- SUMS over the batch's samples).  M: the
    minibatch's samples when b is one tile of it (the means' divisors stay the minibatch's); entropy: the tile carries the - entropy_coef H term"""
    Aw = b["obs"].shape[-2]
    n = b["obs"].shape[0] * Aw
    M = M or n
    mean, _, value = net.evaluate(b["obs"], b["actions"])
    Lpi, _, nd, rho, Lv, _, _, _, lsg = _heads(net, mean, value, b, cfg, 1.0, 1.0)
    G = M // Aw if cfg["joint"] else M
    step = Aw if cfg["joint"] else 1                          # one value a group under the joint ratio
    L = Lpi[::step].sum() / G + cfg["value_coef"] * Lv.sum() / M
    if entropy:
        L = L - cfg["entropy_coef"] * (lsg.sum() + 1.5 * (1 + LN2PI))
    clipped = ((rho - 1).abs() > cfg["clip"]).to(L.dtype)
    # every sample adds its group's statistics (csrc/kernels_ppo.hpp), so the sums are over samples and the means divide by M
    return L, torch.stack([Lpi.sum(), Lv.sum(), nd.sum(), clipped.sum()]).detach()


def _stats(net, sums, M, cfg):
    H = float(torch.log(0.5 * torch.sigmoid(net.log_std.detach().double())).sum()) + 1.5 * (1 + LN2PI)
    Lpi, Lv = float(sums[0]) / M, float(sums[1]) / M
    return torch.tensor([Lpi, Lv, H, Lpi + cfg["value_coef"] * Lv - cfg["entropy_coef"] * H, float(sums[2]) / M, float(sums[3]) / M], dtype=torch.float64)


def autograd(net, b, cfg, dtype, tile=None):
    """torch autograd of loss_torch at `dtype`: on the whole batch, or accumulated serially over tiles of `tile` rows (a multiple of A'), as the kernel's
    workgroup walks them.  -> ({engine name: grad}, stats[6])"""
    n = copy.deepcopy(net).to(dtype)
    bb = {k: b[k].to(dtype) for k in KEYS}
    G, Aw = bb["obs"].shape[:2]
    M = G * Aw
    per = G if tile is None else tile // Aw
    sums = torch.zeros(4, dtype=dtype)
    for g0 in range(0, G, per):
        L, s = loss_torch(n, {k: v[g0:g0 + per] for k, v in bb.items()}, cfg, M, entropy=g0 == 0)
        L.backward()                                          # .grad accumulates in `dtype`, tile after tile
        sums = sums + s
    g = {name: (p.grad if p.grad is not None else torch.zeros_like(p)).detach() for name, (_, p) in zip(names(n), n.named_parameters())}
    return g, _stats(net, sums.double(), M, cfg)


# ---- the scales S_n: hooks on the float64 twin ---------------------------------------------------------------------------------------------------------
def reference(net, b, cfg):
    """float64 autograd on the whole batch with hooks: -> (g64 {engine name: grad}, stats64[6], S {engine name: S_n}, stat_scales[6])"""
    n = mat_ref.doubles(net)
    bb = {k: b[k].double() for k in KEYS}
    G, Aw = bb["obs"].shape[:2]
    M = G * Aw
    seen, S, hooks = {}, {}, []

    def fwd(name):
        def f(mod, inp, out):
            seen[name] = inp[0].detach()
        return f

    def bwd(name):
        def f(mod, gin, gout):
            d, x = gout[0].detach().abs(), seen[name]
            if isinstance(mod, torch.nn.Linear):
                S[f"mat.{name}.weight"] = float((d.reshape(-1, d.shape[-1]).T @ x.abs().reshape(-1, x.shape[-1])).max())
            else:
                mu = x.mean(-1, keepdim=True)
                xhat = (x - mu) / torch.sqrt(((x - mu) ** 2).mean(-1, keepdim=True) + mod.eps)
                S[f"mat.{name}.weight"] = float((d * xhat.abs()).reshape(-1, d.shape[-1]).sum(0).max())
            S[f"mat.{name}.bias"] = float(d.reshape(-1, d.shape[-1]).sum(0).max())
        return f

    for name, mod in n.named_modules():
        if isinstance(mod, (torch.nn.Linear, torch.nn.LayerNorm)):
            hooks += [mod.register_forward_hook(fwd(name)), mod.register_full_backward_hook(bwd(name))]
    obs = bb["obs"].clone().requires_grad_(True)               # so that the first norm has a full backward as well
    L, sums = loss_torch(n, dict(bb, obs=obs), cfg)
    L.backward()
    for h in hooks:
        h.remove()
    g64 = {name: p.grad.detach() for name, (_, p) in zip(names(n), n.named_parameters())}
    # log_std and the statistics: the heads' own magnitudes
    with torch.no_grad():
        mean, _, value = n.evaluate(bb["obs"], bb["actions"])
        inv_m = 1.0 / M
        inv_g = 1.0 / G if cfg["joint"] else inv_m
        Lpi, dlp, nd, rho, Lv, dv, z, inv, lsg = _heads(n, mean, value, bb, cfg, inv_m, inv_g)
        om = 1 - torch.sigmoid(n.log_std)
        S["log_std"] = float((((dlp[:, None] * (z * z - 1)).abs().sum(0) + cfg["entropy_coef"]) * om).max())
        mag = lambda lin, x: x.abs() @ lin.weight.abs().T + lin.bias.abs()
        lpo, adv, ret = bb["logp_old"].reshape(-1), bb["adv"].reshape(-1), bb["ret"].reshape(-1)
        A = (0.5 * z * z + lsg.abs()).sum(-1) + 1.5 * LN2PI + lpo.abs() + (z.abs() * inv * mag(n.mean_out, seen["mean_out"]).reshape(-1, 3)).sum(-1)
        Ag, advg = A, adv
        if cfg["joint"] and Aw > 1:
            Ag, advg = spread(pair(A, Aw), Aw), spread(pair(adv.abs(), Aw) * (1.0 / Aw), Aw)
        vmag = mag(n.value_out, seen["value_out"]).reshape(-1) + ret.abs() + (bb["v_old"].reshape(-1).abs() if cfg["value_clip"] is not None else 0)
        sc = torch.stack([(advg.abs() * rho * (1 + Ag)).sum(), (vmag * vmag).sum(), Ag.sum()])
        Hs = float(lsg.abs().sum()) + 1.5 * (1 + LN2PI)
        vc, ec = cfg["value_coef"], cfg["entropy_coef"]
        scales = torch.stack([sc[0] / M, sc[1] / M, torch.tensor(Hs, dtype=torch.float64), sc[0] / M + vc * sc[1] / M + ec * Hs, sc[2] / M,
                              torch.ones((), dtype=torch.float64)])
    return g64, _stats(n, sums, M, cfg), S, scales


def ratio_to_bound(g, g64, S):
    """max over the tensors of max |g - g64| / (2^-24 S_n) -> (ratio, name): ppo_ref's"""
    return ppo_ref.ratio_to_bound(g, g64, S)


# ---- the manual backward: the formulas csrc/kernels_mat_grad.hpp states ------------------------------------------------------------------------------------
def _gelu(x):
    return 0.5 * x * (1 + torch.erf(x / math.sqrt(2.0)))


def _dgelu(x, variant=None):
    if variant == "tanh_gelu":                                # d/dx of 0.5 x (1 + tanh(u)), u = sqrt(2 / pi) (x + 0.044715 x^3)
        k = math.sqrt(2.0 / math.pi)
        t = torch.tanh(k * (x + 0.044715 * x ** 3))
        return 0.5 * (1 + t) + 0.5 * x * (1 - t * t) * k * (1 + 3 * 0.044715 * x * x)
    return 0.5 * (1 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)


class _Walk:
    """forward with every slab the backward needs kept, and the operators' backward; g: {engine name: gradient}"""

    def __init__(self, net, variant=None):
        self.net, self.variant = net, variant
        self.g = {n: torch.zeros_like(p) for n, (_, p) in zip(names(net), net.named_parameters())}
        self.kept = {}

    def lin(self, name, x):
        m = self.net.get_submodule(name)
        self.kept[name] = x
        return x @ m.weight.T + m.bias

    def lin_back(self, name, d):
        m, x = self.net.get_submodule(name), self.kept[name]
        self.g[f"mat.{name}.weight"] += d.reshape(-1, d.shape[-1]).T @ x.reshape(-1, x.shape[-1])
        self.g[f"mat.{name}.bias"] += d.reshape(-1, d.shape[-1]).sum(0)
        return d @ m.weight

    def ln(self, name, a):
        m = self.net.get_submodule(name)
        mu = a.mean(-1, keepdim=True)
        rstd = 1.0 / torch.sqrt(((a - mu) ** 2).mean(-1, keepdim=True) + m.eps)
        xhat = (a - mu) * rstd
        self.kept[name] = (xhat, rstd)
        return m.weight * xhat + m.bias

    def ln_back(self, name, du):
        m, (xhat, rstd) = self.net.get_submodule(name), self.kept[name]
        self.g[f"mat.{name}.weight"] += (du * xhat).reshape(-1, du.shape[-1]).sum(0)
        self.g[f"mat.{name}.bias"] += du.reshape(-1, du.shape[-1]).sum(0)
        dxh = du * m.weight
        return rstd * (dxh - dxh.mean(-1, keepdim=True) - xhat * (dxh * xhat).mean(-1, keepdim=True))

    def gelu(self, name, pre):
        self.kept[name + ":pre"] = pre
        return _gelu(pre)

    def gelu_back(self, name, d):
        return d * _dgelu(self.kept[name + ":pre"], self.variant)

    def attn(self, name, key, value, query, masked):
        k, v, q = self.lin(name + ".key", key), self.lin(name + ".value", value), self.lin(name + ".query", query)
        c = 1.0 / math.sqrt(k.shape[-1])
        s = q @ k.transpose(-1, -2) * c
        A = s.shape[-1]
        inJ = torch.tril(torch.ones(A, A, dtype=torch.bool)) if masked else torch.ones(A, A, dtype=torch.bool)
        p = torch.softmax(s.masked_fill(~inJ, float("-inf")), dim=-1)
        self.kept[name] = (k, v, q, p, torch.softmax(s, dim=-1), c)
        return self.lin(name + ".proj", p @ v)

    def attn_back(self, name, dout):
        """-> (d key input, d value input, d query input)"""
        k, v, q, p, p_all, c = self.kept[name]
        dY = self.lin_back(name + ".proj", dout)
        dp = dY @ v.transpose(-1, -2)                          # dp_ij = dY_i . v_j
        r = (p * dp).sum(-1, keepdim=True)                     # over J(i): p is 0 outside
        ds = p * dp if self.variant == "no_r" else p * (dp - r)
        pc, dsc = p, ds
        if self.variant == "mask_ignored":                     # the column sums over ALL rows, with the probabilities no mask shaped
            pc = p_all
            dsc = p_all * (dp - (p_all * dp).sum(-1, keepdim=True))
        cs = 1.0 if self.variant == "no_scale" else c
        dv = pc.transpose(-1, -2) @ dY
        dq = cs * (ds @ k)
        dk = cs * (dsc.transpose(-1, -2) @ q)
        return self.lin_back(name + ".key", dk), self.lin_back(name + ".value", dv), self.lin_back(name + ".query", dq)


def manual(net, b, cfg, variant=None):
    """The manual backward in the dtype of net (float64 for the comparison with autograd): csrc/kernels_mat_grad.hpp's walk -- the decoder in reverse, then
    the encoder once with the sum that reached rep -- with the sums where gradients meet in the kernel's order.  -> ({engine name: grad}, stats[6])"""
    w = _Walk(net, variant)
    bb = {k: b[k].to(net.log_std.dtype) for k in KEYS}
    G, Aw = bb["obs"].shape[:2]
    M = G * Aw
    with torch.no_grad():
        # forward: MATNet.encode / decode, written out
        x = w.ln("enc.ln", w.gelu("enc.obs_fc", w.lin("enc.obs_fc", w.ln("enc.obs_norm", bb["obs"]))))
        x = w.ln("enc.ln1", x + w.attn("enc.attn", x, x, x, False))
        rep = w.ln("enc.ln2", x + w.lin("enc.mlp1", w.gelu("enc.mlp0", w.lin("enc.mlp0", x))))
        value = w.lin("value_out", w.ln("enc.head_ln", w.gelu("enc.head0", w.lin("enc.head0", rep))))[..., 0]
        s = torch.cat([torch.zeros_like(bb["actions"][..., :1, :]), bb["actions"][..., :-1, :]], dim=-2)
        x = w.ln("dec.ln", w.gelu("dec.act_fc", w.lin("dec.act_fc", s)))
        x = w.ln("dec.ln1", x + w.attn("dec.attn1", x, x, x, True))
        x = w.ln("dec.ln2", rep + w.attn("dec.attn2", x, x, rep, True))
        x = w.ln("dec.ln3", x + w.lin("dec.mlp1", w.gelu("dec.mlp0", w.lin("dec.mlp0", x))))
        mean = w.lin("mean_out", w.ln("dec.head_ln", w.gelu("dec.head0", w.lin("dec.head0", x))))
        # the heads
        inv_m = 1.0 / M
        inv_g = 1.0 / G if cfg["joint"] else inv_m
        Lpi, dlp, nd, rho, Lv, dv, z, inv, lsg = _heads(net, mean, value, bb, cfg, inv_m, inv_g)
        om = torch.ones(3, dtype=z.dtype) if variant == "no_one_minus_sigmoid" else 1 - torch.sigmoid(net.log_std)
        w.g["log_std"] += ((dlp[:, None] * (z * z - 1)).sum(0) - cfg["entropy_coef"]) * om
        dmean = (dlp[:, None] * z * inv).reshape(G, Aw, 3)
        dvalue = (cfg["value_coef"] * inv_m * dv).reshape(G, Aw, 1)
        # the decoder, in reverse
        d = w.gelu_back("dec.head0", w.ln_back("dec.head_ln", w.lin_back("mean_out", dmean)))
        d = w.ln_back("dec.ln3", w.lin_back("dec.head0", d))
        d = d + w.lin_back("dec.mlp0", w.gelu_back("dec.mlp0", w.lin_back("dec.mlp1", d)))      # the residual, + dx of mlp0
        d = w.ln_back("dec.ln2", d)
        drep = torch.zeros_like(d) if variant == "no_res_rep" else d                               # the decoder's residual: rep + attn2
        dkey, dval, dqry = w.attn_back("dec.attn2", d)
        if variant != "no_query_rep":
            drep = drep + dqry                                                                     # + dx of attn2.query
        d = w.ln_back("dec.ln1", dval + dkey)                                                      # dx of attn2.value, + dx of attn2.key
        dkey, dval, dqry = w.attn_back("dec.attn1", d)
        d = w.ln_back("dec.ln", ((d + dval) + dqry) + dkey)                                        # the residual, + value, + query, + key
        w.lin_back("dec.act_fc", w.gelu_back("dec.act_fc", d))                                      # a weight gradient only: s is data
        # the encoder, once, with the sum that reached rep
        d = w.gelu_back("enc.head0", w.ln_back("enc.head_ln", w.lin_back("value_out", dvalue)))
        d = w.lin_back("enc.head0", d)
        d = w.ln_back("enc.ln2", d if variant == "enc_value_only" else drep + d)
        d = d + w.lin_back("enc.mlp0", w.gelu_back("enc.mlp0", w.lin_back("enc.mlp1", d)))
        d = w.ln_back("enc.ln1", d)
        dkey, dval, dqry = w.attn_back("enc.attn", d)
        d = w.ln_back("enc.ln", ((d + dval) + dqry) + dkey)
        w.ln_back("enc.obs_norm", w.lin_back("enc.obs_fc", w.gelu_back("enc.obs_fc", d)))        # dgamma and dbeta: nothing lies below the observation
        clipped = ((rho - 1).abs() > cfg["clip"]).to(z.dtype)
        sums = torch.stack([Lpi.sum(), Lv.sum(), nd.sum(), clipped.sum()])
    return w.g, _stats(net, sums.double(), M, cfg)


# ---- the synthetic trajectory ---------------------------------------------------------------------------------------------------------------------------
def group_kinks(n64, b, c=CLIP, cv=VALUE_CLIP, cd=DUAL):
    """bool per GROUP (float64): a sample of it, or the group's joint ratio or mean advantage, lies within ppo_ref.kinks' margins of a kink of ANY of the
    losses -- 1 - c, 1 + c, c_d, a zero advantage, the value clip's two kinks -- so that every flag combination reads the same kink-free trajectory"""
    bb = {k: b[k].double() for k in KEYS}
    G, Aw = bb["obs"].shape[:2]
    with torch.no_grad():
        _, logp, v = n64.evaluate(bb["obs"], bb["actions"])
    bad = joint_ref.group_kinks(logp - bb["logp_old"], bb["adv"], Aw, cd, c)
    vo, ret = bb["v_old"], bb["ret"]
    vk = ((v - vo).abs() - cv).abs() < 1e-3
    v_c = vo + torch.clamp(v - vo, -cv, cv)
    vk |= ((v - vo).abs() > cv) & (((v - ret) ** 2 - (v_c - ret) ** 2).abs() < 1e-3)
    return bad | vk.any(-1)


def draw_groups(n64, G, Aw, D, gen):
    """ppo_ref.synth's draws with MAT's head, per group: observation N(0, 1); action = mean64 + sigma N(0, 1) with the decoder conditioned on the drawn
    actions (MATNet.act); logp_old = logp64 + 0.25 N(0, 1); adv N(0, 1); v_old = v64 + 0.3 N(0, 1); ret = v64 + N(0, 1).  float32 tensors (G, A', ...)"""
    obs = torch.randn(G, Aw, D, generator=gen).float()
    with torch.no_grad():
        actions, _, v = n64.act(obs.double(), z=torch.randn(G, Aw, 3, generator=gen).double())
        actions = actions.float()
        _, logp, _ = n64.evaluate(obs.double(), actions.double())
    return dict(obs=obs, actions=actions, logp_old=(logp + 0.25 * torch.randn(G, Aw, generator=gen).double()).float(),
                adv=torch.randn(G, Aw, generator=gen).float(), v_old=(v + 0.3 * torch.randn(G, Aw, generator=gen).double()).float(),
                ret=(v + torch.randn(G, Aw, generator=gen).double()).float())


def kink_free(net, G, Aw, D, seed):
    """G kink-free groups: a group inside a margin is drawn again -- the whole group, since a row's observation reaches all of it -- until none is left.
    The groups drawn again stay below 15 % of the groups (four times the project's measured 2.5 % of rows at A' = 4, rounded up): asserted.
    -> (batch, share drawn again)"""
    n64 = mat_ref.doubles(net)
    gen = torch.Generator().manual_seed(seed)
    b = draw_groups(n64, G, Aw, D, gen)
    redraws = 0
    for _ in range(200):
        bad = torch.nonzero(group_kinks(n64, b))[:, 0]
        if len(bad) == 0:
            break
        redraws += len(bad)
        fresh = draw_groups(n64, len(bad), Aw, D, gen)
        for k in b:
            b[k][bad] = fresh[k]
    else:
        raise RuntimeError("kink_free: groups inside a kink margin remain")
    share = redraws / G
    assert share < 0.15, f"{redraws} of {G} groups drawn again"
    return b, share


def synth(E, shape, seed, pseed=None, extra_stride=8, guard=64, value_norm=False):
    """A seeded kink-free trajectory of `shape` = (N, A', T, D) for the MATNet mat_ref.make_net(D, E, pseed), in mqe_ppo_grad's buffers (ppo_ref.synth's
    images: `packed` with the observations of rows 0 .. T - 1 in place, a filler row T and sentinels elsewhere, `value`, `grad`, `stats` with guards).
    Logical tensors are flat over the n = T N A' samples, sample s = (t N + env) A' + a: group g = t N + env.  gindex: a seeded int32 permutation of the
    T N groups.  -> dict"""
    N, Aw, T, D = shape
    R, G = N * Aw, T * N
    n = T * R
    net = mat_ref.make_net(D, E, 500 + seed if pseed is None else pseed)
    b, share = kink_free(net, G, Aw, D, seed)
    g = torch.Generator().manual_seed(7000 + seed)
    nobs = R * D
    pf = nobs + R + (N + 3) // 4
    stride = (pf + 3) // 4 * 4 + extra_stride
    packed = np.full((T + 1) * stride + guard, SENT, np.int32)
    rows = packed[:(T + 1) * stride].reshape(T + 1, stride)
    rows[:T, :nobs] = b["obs"].numpy().reshape(T, nobs).view(np.int32)
    rows[T, :nobs] = torch.randn(nobs, generator=g).float().numpy().view(np.int32)
    value = np.concatenate([b["v_old"].reshape(-1).numpy(), torch.randn(R, generator=g).float().numpy()]).view(np.int32).copy()
    n_params = mat_ref.param_count(D, E)
    out = lambda k: np.full(k + guard, SENT, np.int32)
    flatb = {k: b[k].reshape(n, *b[k].shape[2:]) for k in KEYS}
    return dict(E=E, shape=shape, N=N, Aw=Aw, T=T, D=D, R=R, n=n, n_groups=G, stride=stride, guard=guard, net=net, n_params=n_params, redrawn=share,
                gindex=torch.randperm(G, generator=g).to(torch.int32), packed=packed, value=value, grad=out(n_params + (abi.VALUE_NORM_STATE if value_norm else 0)),
                stats=out(abi.PPO_STATS), groups=b, **flatb)


def batch(s, groups):
    """the minibatch of the group numbers `groups` (tensor, list or slice), (G, A', ...)"""
    if isinstance(groups, torch.Tensor):
        groups = groups.long()
    return {k: s["groups"][k][groups] for k in KEYS}
