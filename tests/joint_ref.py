"""Host side of the joint-ratio and dual-clip tests (mqe_ppo_grad with MQE_PPO_JOINT / MQE_PPO_DUAL_CLIP; csrc/kernels_ppo.hpp states the loss): the
loss in torch (float64 autograd is the truth), the manual backward tile by tile in float32 and float64 with the pairwise order of the kernel's xor
butterfly, deliberately wrong variants, the recurrent twin on bptt_ref's walk, and the synthetic trajectories.  ppo_ref and bptt_ref are imported
and unchanged: the networks' walk, the value head, the scales' form and the buffers are theirs.

THE UNIT.  A minibatch is G groups; a group is the A' samples g A' + a of one env-step, so every batch here is GROUP-MAJOR: row i of a batch is
agent i % A' of group i // A' (batch(), samples_of()).  cfg holds ppo_ref's keys and "joint" (bool), "dual_clip" (None or c_d).

THE BOUND has ppo_ref's form, |g - g64| <= K 2^-24 S_n per tensor with S_n the sum over the SAMPLES of the absolute per-sample contributions, and
exactly 0 where S_n = 0; the statistics use the scales of manual().  K IS MEASURED ON THE CPU, never on the kernel: the largest ratio reached by two
float32 evaluations (torch autograd on the whole batch; manual() accumulated over 64-row tiles) against float64, over K_CASES: the five networks of
ppo_ref.NETS x G in {1, 16, 33, 65, 500} x A' in {2, 4} x (joint, joint + dual) x three seeds, value clipping on, c = 0.2, c_d = 1.5.
tests/test_joint_loss.py prints every case and asserts the table; the GPU is allowed 4 x (the project's margin for the kernel's expf / tanhf).

THE RULE.  Every case is evaluated with torch running one thread and with its default number of threads (torch's float32 sums depend on how many
threads share them), and on every kind of host the suite runs on; K is the largest ratio of all of them, rounded up to the next integer
(tests/layer_norm_ref.py's rule: the same test asserts one constant everywhere).  Largest ratio per network and G (the larger of the two float32
evaluations, gradient tensors and statistics together):
                     G = 1     16     33     65    500
    tanh64x64         11.0    9.4    7.9    7.9    5.2
    tanh7              9.0   15.0   14.6    8.0    2.8
    relu128x3         21.6   15.6   13.7    9.9    4.2
    tanh256x3         13.1   11.1   11.9    7.7    3.9
    relu17x5          11.3   15.0   11.8   11.0    5.2
The maximum is 21.57 (relu128x3, one group of four agents, joint and joint + dual, seed 0, actor.2.weight, both evaluations; with 8 torch threads the
largest is 15.04, relu17x5 at 16 groups), so K_CPU_JOINT = 22 -- measured here, not ppo_ref's 22 reused.
THE RECURRENT TWIN (K_CASES_BPTT: three of bptt_ref's shapes at L = 4, T = 8, N = 5, A' = 2, chunk-group counts 1 and 10 through the seeded index,
joint and joint + dual; torch autograd and the manual backward in float32 over 64-chunk tiles against the float64 manual backward), per shape
tanh7_5, tanh9x5_6x7_both, tanh64x64_both: 18.3, 39.4, 19.7 (39.41: 10 chunk groups, joint, torch autograd, actor.norm_in.weight; 29.48 with 8
threads, there the manual backward at one chunk group), so K_CPU_JOINT_BPTT = 40.
WITH THE NORMS (K_CASES_LN: a LayerNorm on the observation and behind every hidden activation; tanh64x64 and tanh7, G in {1, 33, 65}, both A', both
losses, three seeds), per network: 30.8 and 26.6 (30.77: tanh64x64, one group of four agents, seed 2, the tiled manual backward, actor.1.weight), so
K_CPU_JOINT_LN = 31.
None of the three is taken from anything the kernel computes."""
import contextlib
import math

import numpy as np
import torch

import bptt_ref
import ppo_ref
from ppo_ref import EPS32, LN2PI, forward

CLIP, VALUE_CLIP, DUAL = ppo_ref.CLIP, ppo_ref.VALUE_CLIP, 1.5
K = {"mlp": 22.0, "ln": 31.0, "bptt": 40.0}  # K_CPU_JOINT, K_CPU_JOINT_LN, K_CPU_JOINT_BPTT: measured, the docstring above
K_GPU = {k: 4 * v for k, v in K.items()}
CFG = dict(clip=CLIP, value_coef=0.7, entropy_coef=0.01, value_clip=VALUE_CLIP, joint=True, dual_clip=None)
LOSSES = {"joint": dict(joint=True, dual_clip=None), "dual": dict(joint=False, dual_clip=DUAL), "joint+dual": dict(joint=True, dual_clip=DUAL)}
K_GS = (1, 16, 33, 65, 500)
K_CASES = [(net, G, Aw, loss, seed) for net in ppo_ref.NETS for G in K_GS for Aw in (2, 4) for loss in ("joint", "joint+dual") for seed in (0, 1, 2)]
K_CASES_LN = [(net, G, Aw, loss, seed) for net in ("tanh64x64", "tanh7") for G in (1, 33, 65) for Aw in (2, 4) for loss in ("joint", "joint+dual") for seed in (0, 1, 2)]
K_CASES_BPTT = [(name, count, loss) for name in ("tanh7_5", "tanh9x5_6x7_both", "tanh64x64_both") for count in (1, 10) for loss in ("joint", "joint+dual")]
WRONG = ("per_agent_ratio", "adv_not_averaged", "inv_m", "dual_ignored", "dual_where_positive", "no_gate_at_cd")
REGIONS = ("unclipped", "high, A > 0", "low, A < 0", "dual-clipped")


# ---- the groups ----------------------------------------------------------------------------------------------------------------------------------
def pair(x, Aw):
    """the sum over the A' agents of every group in the xor butterfly's order: x (G A', ...) group-major -> (G, ...); torch or numpy"""
    x = x.reshape(-1, Aw, *x.shape[1:])
    while x.shape[1] > 1:
        x = x[:, 0::2] + x[:, 1::2]
    return x[:, 0]


def spread(x, Aw):
    """a group's value on each of its A' samples: (G, ...) -> (G A', ...)"""
    return x.repeat_interleave(Aw, 0) if isinstance(x, torch.Tensor) else np.repeat(x, Aw, 0)


def samples_of(groups, Aw):
    """group numbers -> the flat sample numbers g A' + a, group-major (what k_joint_expand writes)"""
    g = torch.as_tensor(np.asarray(groups), dtype=torch.int64)
    return (g[:, None] * Aw + torch.arange(Aw)[None, :]).reshape(-1)


def batch(s, groups):
    return ppo_ref.batch(s, samples_of(groups, s["Aw"]))


def policy_head(xp, d, adv, cfg, Aw, inv_g, variant=None):
    """THE LOSS HEAD of csrc/kernels_ppo.hpp behind d = logp - logp_old, per sample (a group's values on each of its samples): ->
    (L_pi, dL/dlogp, -Delta, rho).  xp: torch or numpy; selects at the kinks.  variant: one of WRONG."""
    c, cd = cfg["clip"], cfg["dual_clip"]
    where, minimum, maximum = (torch.where, torch.minimum, torch.maximum) if xp is torch else (np.where, np.minimum, np.maximum)
    clamp = (lambda v: torch.clamp(v, 1 - c, 1 + c)) if xp is torch else (lambda v: np.clip(v, 1 - c, 1 + c))
    if cfg["joint"] and Aw > 1:
        A = pair(adv, Aw)
        A = spread(A if variant == "adv_not_averaged" else A * (1.0 / Aw), Aw)
        D = d if variant == "per_agent_ratio" else spread(pair(d, Aw), Aw)
    else:
        A, D = adv, d
    rho = xp.exp(D)
    surr = minimum(rho * A, clamp(rho) * A)
    gate = ((A > 0) & (rho > 1 + c)) | ((A < 0) & (rho < 1 - c))
    if cd is not None and variant != "dual_ignored":
        neg = (A < 0) | (variant == "dual_where_positive")
        surr = where(neg, maximum(surr, cd * A), surr)
        if variant != "no_gate_at_cd":
            gate = gate | (neg & (rho > cd))
        if variant == "dual_where_positive":             # max(., c_d A) is c_d A for every A > 0: no gradient there
            gate = gate | (A > 0)
    dlp = -A * rho * inv_g
    return -surr, where(gate, 0 * dlp, dlp), -D, rho


# ---- the feed-forward networks: ppo_ref's loss with the head above -----------------------------------------------------------------------------------
def loss_torch(params, a_dims, c_dims, act, b, cfg, Aw, hidden=False, feat=False):
    """the stated loss as a torch expression in the dtype of params, on a group-major batch: the policy term is the mean over GROUPS -> (L, stats[6])"""
    c, vc, ec, cv = cfg["clip"], cfg["value_coef"], cfg["entropy_coef"], cfg["value_clip"]
    ls = params["log_std"]
    mean = forward(params, "actor", a_dims, act, b["obs"], hidden=hidden, feat=feat)[0]
    v = forward(params, "critic", c_dims, act, b["obs"], hidden=hidden, feat=feat)[0][:, 0]
    z = (b["actions"] - mean) * torch.exp(-ls)
    logp = (-0.5 * z * z - ls).sum(-1) - 1.5 * LN2PI
    Lpi, _, nd, rho = policy_head(torch, logp - b["logp_old"], b["adv"], cfg, Aw, 1.0)
    if cfg["joint"]:
        Lpi, nd, rho = Lpi[::Aw], nd[::Aw], rho[::Aw]           # one value a group
    Lv = (v - b["ret"]) ** 2
    if cv is not None:
        v_c = b["v_old"] + torch.clamp(v - b["v_old"], -cv, cv)
        Lv = torch.maximum(Lv, (v_c - b["ret"]) ** 2)
    H = ls.sum() + 1.5 * (1 + LN2PI)
    L = Lpi.mean() + vc * Lv.mean() - ec * H
    return L, torch.stack([Lpi.mean(), Lv.mean(), H, L, nd.mean(), ((rho - 1).abs() > c).to(L.dtype).mean()])


def autograd(params, a_dims, c_dims, act, b, cfg, Aw, dtype, hidden=False, feat=False):
    p = {k: v.to(dtype).clone().requires_grad_(True) for k, v in params.items()}
    L, stats = loss_torch(p, a_dims, c_dims, act, {k: v.to(dtype) for k, v in b.items()}, cfg, Aw, hidden, feat)
    L.backward()
    return {k: (v.grad if v.grad is not None else torch.zeros_like(v)).detach() for k, v in p.items()}, stats.detach()


def manual(params, a_dims, c_dims, act, b, cfg, Aw, dtype=torch.float64, tile=None, variant=None, hidden=False, feat=False):
    """ppo_ref.manual with the head above: the backward at `dtype` over tiles of `tile` rows (a multiple of A'; None: the whole batch), 1 / G on the
    policy term and 1 / M on the value term, every sample adding its GROUP's statistics.  -> (grads, stats[6], S, stat_scales) as ppo_ref.manual.
    With joint off (or A' = 1) and without a dual clip every expression is ppo_ref.manual's, in its order: the same float64 bits."""
    c, vc, ec, cv = cfg["clip"], cfg["value_coef"], cfg["entropy_coef"], cfg["value_clip"]
    p = {k: v.to(dtype) for k, v in params.items()}
    b = {k: v.to(dtype) for k, v in b.items()}
    M = b["obs"].shape[0]
    inv_m = 1.0 / M
    inv_g = inv_m if (variant == "inv_m" or not cfg["joint"]) else 1.0 / (M // Aw)
    ls = p["log_std"]
    inv = torch.exp(-ls)
    g = {k: torch.zeros_like(v) for k, v in p.items()}
    S = {k: torch.zeros_like(v) for k, v in p.items()}
    sums, sc = torch.zeros(4, dtype=dtype), torch.zeros(3, dtype=dtype)
    net = dict(hidden=hidden, feat=feat, kernel_order=dtype == torch.float32)
    tile = tile or M
    assert not cfg["joint"] or (tile % Aw == 0 and M % Aw == 0), "a group lies inside one tile"
    for r0 in range(0, M, tile):
        sl = slice(r0, min(r0 + tile, M))
        obs = b["obs"][sl]
        fa = forward(p, "actor", a_dims, act, obs, **net)
        fc = forward(p, "critic", c_dims, act, obs, **net)
        mean, v = fa[0], fc[0][:, 0]
        z = (b["actions"][sl] - mean) * inv
        logp = (-0.5 * z * z - ls).sum(-1) - 1.5 * LN2PI
        lpo, adv, ret = b["logp_old"][sl], b["adv"][sl], b["ret"][sl]
        Lpi, dlp, nd, rho = policy_head(torch, logp - lpo, adv, cfg, Aw, inv_g, variant)
        g["log_std"] += (dlp[:, None] * (z * z - 1)).sum(0)
        S["log_std"] += (dlp[:, None] * (z * z - 1)).abs().sum(0)
        d1 = v - ret
        Lv, dv = d1 * d1, 2 * d1
        if cv is not None:
            vo = b["v_old"][sl]
            d2 = vo + torch.clamp(v - vo, -cv, cv) - ret
            Lv = torch.maximum(d1 * d1, d2 * d2)
            dv = torch.where(d1 * d1 >= d2 * d2, 2 * d1, torch.where((v - vo).abs() < cv, 2 * d2, torch.zeros_like(d1)))
        sums += torch.stack([Lpi.sum(), Lv.sum(), nd.sum(), ((rho - 1).abs() > c).to(dtype).sum()])
        mag = lambda who, dims, f: f[1][-1].abs() @ p[f"{who}.{len(dims) - 2}.weight"].abs().T + p[f"{who}.{len(dims) - 2}.bias"].abs()
        A = (0.5 * z * z + ls.abs()).sum(-1) + 1.5 * LN2PI + lpo.abs() + (z.abs() * inv * mag("actor", a_dims, fa)).sum(-1)
        Ag, advg = A, adv                                        # the magnitudes behind a GROUP's Delta and advantage
        if cfg["joint"] and Aw > 1:
            Ag, advg = spread(pair(A, Aw), Aw), spread(pair(adv.abs(), Aw) * (1.0 / Aw), Aw)
        vmag = mag("critic", c_dims, fc)[:, 0] + ret.abs() + (b["v_old"][sl].abs() if cv is not None else 0)
        sc += torch.stack([(advg.abs() * rho * (1 + Ag)).sum(), (vmag * vmag).sum(), Ag.sum()])
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
                    dxh = da * p[name + ".weight"]
                    da = rstd * (dxh - dxh.mean(-1, keepdim=True) - xhat * (dxh * xhat).mean(-1, keepdim=True))
                delta = da * ((1 - y * y) if act == "tanh" else (y > 0).to(dtype))
    g["log_std"] = g["log_std"] - ec
    S["log_std"] = S["log_std"] + ec
    H = ls.sum() + 1.5 * (1 + LN2PI)
    Lpi, Lv = sums[0] / M, sums[1] / M
    stats = torch.stack([Lpi, Lv, H, Lpi + vc * Lv - ec * H, sums[2] / M, sums[3] / M])
    Hs = ls.abs().sum() + 1.5 * (1 + LN2PI)
    stat_scales = torch.stack([sc[0] / M, sc[1] / M, Hs, sc[0] / M + vc * sc[1] / M + ec * Hs, sc[2] / M, torch.ones((), dtype=dtype)]).double()
    return g, stats, {k: float(v.max()) for k, v in S.items()}, stat_scales


# ---- the synthetic trajectory ---------------------------------------------------------------------------------------------------------------------
# (region, sign of the group's advantage, rho from, rho to): dealt to the groups in turn over a seeded order, so each holds a seventh of them
def _deal(cd, c=CLIP):
    return (("unclipped", 1, 1 - c + 0.02, 1 + c - 0.02), ("unclipped", -1, 1 - c + 0.02, 1 + c - 0.02), ("high, A > 0", 1, 1 + c + 0.02, 1 + c + 0.7),
            ("low, A < 0", -1, 0.45, 1 - c - 0.02), ("dual-clipped", -1, cd + 0.02, cd + 0.7), ("low, A > 0", 1, 0.45, 1 - c - 0.02),
            ("between 1 + c and c_d, A < 0", -1, 1 + c + 0.02, cd - 0.02))


def group_kinks(d, adv, Aw, cd, c=CLIP):
    """float64 d = logp - logp_old and adv, (G, A'): bool per GROUP -- its rho or a sample's ratio within 1e-3 of 1 - c, 1 + c or c_d, its advantage or a
    sample's within 1e-3 of 0"""
    D, A = pair(d.reshape(-1), Aw), pair(adv.reshape(-1), Aw) * (1.0 / Aw)
    bad = A.abs() < 1e-3
    for x in (torch.exp(D)[:, None], torch.exp(d)):
        for k in (1 - c, 1 + c, cd):
            bad |= ((x - k).abs() < 1e-3).any(-1)
    return bad | (adv.abs() < 1e-3).any(-1)


def design(logp64, adv, Aw, gen, cd):
    """logp_old and adv of a trajectory so that the JOINT log-ratio has spread.  logp64, adv: (G, A') per group (an env-step).  Every group is dealt a
    region of _deal: its advantages change sign together where the region asks for the other sign of their mean, its rho is uniform in the region's
    interval, and logp_old_a = logp_a - (ln rho / A' + e_a) with e = 0.3 N(0, 1) less its mean over the group (the agents' own ratios differ and land on
    both sides of the kinks).  A group inside group_kinks' margins is drawn again (advantages N(0, 1), rho, e) until none is left: nothing is excluded.
    -> (logp_old float32 (G, A'), adv float32 (G, A'), region number per group, groups drawn again)"""
    G = logp64.shape[0]
    deal = _deal(cd)
    region = torch.empty(G, dtype=torch.int64)
    region[torch.randperm(G, generator=gen)] = torch.arange(G) % len(deal)
    sign = torch.tensor([r[1] for r in deal], dtype=torch.float64)[region]
    lo, hi = (torch.tensor([r[k] for r in deal], dtype=torch.float64)[region] for k in (2, 3))
    adv = adv.clone().double()
    lpo = torch.zeros(G, Aw)
    todo, redraws = torch.arange(G), 0
    for it in range(200):
        n = len(todo)
        if it:
            adv[todo] = torch.randn(n, Aw, generator=gen).double()
        a = adv[todo].float().double()
        flip = torch.where(pair(a.reshape(-1), Aw) * sign[todo] < 0, -1.0, 1.0)
        adv[todo] = a * flip[:, None]
        rho = lo[todo] + (hi[todo] - lo[todo]) * torch.rand(n, generator=gen).double()
        e = 0.3 * torch.randn(n, Aw, generator=gen).double()
        d = torch.log(rho)[:, None] / Aw + e - e.mean(-1, keepdim=True)
        lpo[todo] = (logp64[todo] - d).float()
        bad = group_kinks(logp64[todo] - lpo[todo].double(), adv[todo], Aw, cd)
        todo = todo[bad]
        if len(todo) == 0:
            break
        redraws += len(todo)
    else:
        raise RuntimeError("design: groups inside a kink margin remain")
    return lpo, adv.float(), region, redraws


def region_shares(d, adv, Aw, cd, c=CLIP):
    """the share of the groups in each of REGIONS (float64 d = logp - logp_old, adv: (G, A'))"""
    rho, A = torch.exp(pair(d.reshape(-1), Aw)), pair(adv.reshape(-1), Aw) * (1.0 / Aw)
    masks = ((rho - 1).abs() <= c, (A > 0) & (rho > 1 + c), (A < 0) & (rho < 1 - c), (A < 0) & (rho > cd))
    return [float(m.double().mean()) for m in masks]


def logp64_of(s):
    p64 = {k: v.double() for k, v in s["params"].items()}
    mean = forward(p64, "actor", s["a_dims"], s["act"], s["obs"].double(), hidden=s["hidden"], feat=s["feat"])[0]
    z = (s["actions"].double() - mean) * torch.exp(-p64["log_std"])
    return (-0.5 * z * z - p64["log_std"]).sum(-1) - 1.5 * LN2PI


def synth(net, shape, seed, cd=DUAL, **kw):
    """ppo_ref.synth(net, shape = (N, A', T, D)) -- kink-free per sample in the value head and the relus -- with logp_old and adv from design(): kink-free
    per GROUP and per sample against 1 - c, 1 + c, c_d and a zero advantage, every region of _deal holding a seventh of the groups.  Adds n_groups = T N,
    gindex (a seeded int32 permutation of the groups), region, cd."""
    s = ppo_ref.synth(net, shape, shape[0] * shape[1] * shape[2], seed, **kw)
    Aw, G = s["Aw"], s["n"] // s["Aw"]
    gen = torch.Generator().manual_seed(9000 + seed)
    lpo, adv, region, redraws = design(logp64_of(s).reshape(G, Aw), s["adv"].reshape(G, Aw), Aw, gen, cd)
    s.update(logp_old=lpo.reshape(-1), adv=adv.reshape(-1), region=region, group_redraws=redraws, n_groups=G, cd=cd,
             gindex=torch.randperm(G, generator=gen).to(torch.int32))
    return s


def shares_of(s):
    Aw = s["Aw"]
    return region_shares((logp64_of(s) - s["logp_old"].double()).reshape(-1, Aw), s["adv"].double().reshape(-1, Aw), Aw, s["cd"])


ratio_to_bound, stats_ratio = ppo_ref.ratio_to_bound, ppo_ref.stats_ratio


# ---- the recurrent twin: bptt_ref's walk with the head above ----------------------------------------------------------------------------------------------
# A minibatch is chunk groups cg = (t0 / L) N + n; its chunks are cg A' + a, group-major, so the A' neighbours of every step's rows are a group.
def chunks_of(chunk_groups, Aw):
    return samples_of(chunk_groups, Aw).numpy()


def _loss_of(cfg, Aw):
    def loss_of(mean, v, ls, b, _cfg, M):
        c, vc, ec, cv = cfg["clip"], cfg["value_coef"], cfg["entropy_coef"], cfg["value_clip"]
        z = (b["actions"] - mean) * torch.exp(-ls)
        logp = (-0.5 * z * z - ls).sum(-1) - 1.5 * LN2PI                     # (L, C): a step's C rows are group-major
        L_, C = logp.shape
        flat = lambda x: x.reshape(L_ * C)
        Lpi, _, nd, rho = policy_head(torch, flat(logp - b["logp_old"]), flat(b["adv"]), cfg, Aw, 1.0)
        Lv = (v - b["ret"]) ** 2
        if cv is not None:
            v_c = b["v_old"] + torch.clamp(v - b["v_old"], -cv, cv)
            Lv = torch.maximum(Lv, (v_c - b["ret"]) ** 2)
        H = ls.sum() + 1.5 * (1 + LN2PI)
        Lpi_m, Lv_m = Lpi.sum() / M, Lv.sum() / M                            # every sample adds its group's value: the mean over groups
        L = Lpi_m + vc * Lv_m - ec * H
        return L, torch.stack([Lpi_m, Lv_m, H, L, nd.sum() / M, ((rho - 1).abs() > c).to(L.dtype).sum() / M]), logp
    return loss_of


def _heads_of(cfg, Aw, variant):
    def heads(p, mean, v, b, _cfg, inv_m):
        c, vc, cv = cfg["clip"], cfg["value_coef"], cfg["value_clip"]
        ls = p["log_std"]
        inv = np.exp(-ls)
        z = (b["actions"] - mean) * inv
        logp = (-0.5 * z * z - ls).sum(-1) - 1.5 * LN2PI
        inv_g = inv_m * (Aw if cfg["joint"] and variant != "inv_m" else 1)     # A' is a power of two: exact
        Lpi, dlp, nd, rho = policy_head(np, logp - b["logp_old"], b["adv"], cfg, Aw, inv_g, variant)
        dlp = dlp.astype(mean.dtype)
        d1 = v - b["ret"]
        Lv, dv = d1 * d1, 2 * d1
        if cv is not None:
            vo = b["v_old"]
            d2 = vo + np.clip(v - vo, -cv, cv) - b["ret"]
            Lv = np.maximum(d1 * d1, d2 * d2)
            dv = np.where(d1 * d1 >= d2 * d2, 2 * d1, np.where(np.abs(v - vo) < cv, 2 * d2, 0))
        sums = np.array([Lpi.sum(), Lv.sum(), nd.sum(), (np.abs(rho - 1) > c).sum()], dtype=np.float64)
        return dlp[:, None] * z * inv, (vc * inv_m * dv)[:, None].astype(mean.dtype), dlp[:, None] * (z * z - 1), sums
    return heads


@contextlib.contextmanager
def _heads_in_bptt_ref(cfg, Aw, variant=None):
    """bptt_ref's walk looks its two loss heads up by name when it runs: for the length of the block they are the ones above (the file is unchanged)"""
    keep = bptt_ref.loss_of, bptt_ref._heads
    bptt_ref.loss_of, bptt_ref._heads = _loss_of(cfg, Aw), _heads_of(cfg, Aw, variant)
    try:
        yield
    finally:
        bptt_ref.loss_of, bptt_ref._heads = keep


def bptt_autograd(s, chunk_groups, L, cfg, dtype=torch.float64):
    with _heads_in_bptt_ref(cfg, s["Aw"]):
        return bptt_ref.autograd(s, chunks_of(chunk_groups, s["Aw"]), L, cfg, dtype)[:2]


def bptt_manual(s, chunk_groups, L, cfg, dtype=np.float64, tile=None, variant=None):
    with _heads_in_bptt_ref(cfg, s["Aw"], variant):
        return bptt_ref.manual(s, chunks_of(chunk_groups, s["Aw"]), L, cfg, dtype, tile)


def bptt_synth(name, N, T, L, seed=0, Aw=2, cd=DUAL, D=16):
    """bptt_ref.synth with logp_old and adv from design() over the env-steps (t, n); adds n_groups = (T / L) N chunk groups, gindex, cd.  The packed image
    holds observations, done bytes and tails only, so it stays as it is"""
    s = bptt_ref.synth(name, N, T, L, D=D, seed=seed, Aw=Aw)
    allc = np.arange(s["n_chunks"])
    t, r = bptt_ref.chunk_steps(s, allc, L)
    a64, c64 = bptt_ref.gru_ref.doubles(*s["nets"][:2])
    with torch.no_grad():
        mean, _ = bptt_ref.twin_outputs(a64, c64, s, allc, L, torch.float64)
    ls = s["nets"][2].double()
    z = (s["actions"][t, r[None, :]].double() - mean) * torch.exp(-ls)
    logp = torch.zeros(T, s["R"], dtype=torch.float64)
    logp[t, r[None, :]] = ((-0.5 * z * z - ls).sum(-1) - 1.5 * LN2PI).detach()
    gen = torch.Generator().manual_seed(9100 + seed)
    lpo, adv, region, redraws = design(logp.reshape(T * N, Aw), s["adv"].reshape(T * N, Aw), Aw, gen, cd)
    s.update(logp_old=lpo.reshape(T, s["R"]), adv=adv.reshape(T, s["R"]), region=region, n_groups=(T // L) * N, cd=cd, logp64=logp)
    s["gindex"] = torch.randperm(s["n_groups"], generator=gen).to(torch.int32)
    return s
