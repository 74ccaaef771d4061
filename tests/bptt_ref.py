"""Host side of the recurrent PPO tests (mqe_ppo_grad with MQE_PPO_BPTT; csrc/kernels_bptt.hpp): truncated back-propagation through time over chunks
of L steps.  THE REFERENCE is the float64 twin: mqe.utils.actor_net.RecurrentMLP.double().evaluate over each chunk from the recorded state (the
mask of the chunk's first step among its masks), the loss of tests/ppo_ref.py on the chunks' samples, and torch autograd (autograd()).  manual() is
the backward written out (numpy, batched over the chunks): the cell's backward as include/mqe_hip.h and csrc/kernels_bptt.hpp state it, the norms'
as csrc/kernels_ln.hpp does; in float64 it equals autograd to rounding (tests/test_bptt.py), it yields the scales S_n, and it takes deliberately
wrong variants.  synth() makes the seeded kink-free trajectory in mqe_rollout's layout with recorded tails that the CPU and the GPU tests share.

THE BOUND has ppo_ref's form: for every parameter tensor n, |g - g64| <= K 2^-24 S_n for every entry, S_n the largest entry of the sum over the
CHUNKS of the absolute per-chunk gradient (float64, manual()), and an exactly zero gradient where S_n = 0.  K is MEASURED ON THE CPU, never on the
kernel: the largest ratio reached over CASES by two float32 evaluations -- torch autograd on the whole minibatch (with one thread and with the
host's default number: its sums depend on it), and manual() in float32 accumulated over tiles of 64 chunks in order.  The GPU is allowed K_GPU = 4 K_CPU (the project's margin for another summation order and libm).

Measured with this file over CASES, the very minibatches the GPU test runs (tests/test_bptt.py prints every case; entropy_coef 0.01; the larger of the
two float32 evaluations over the gradient tensors), largest ratio per group and shape, on the two hosts the suite runs on (torch's float32 kernels
differ between them):
                                       an Intel Xeon host                                   an AMD EPYC 9575F host
    shapes    tanh7_5                  4.7                                                  4.7
              tanh9x5_6x7_both         34.3 (one thread; 32.6 on eight)                     91.3 (any number of threads)
              tanh16_12_hidden         8.4                                                  8.4
              relu17x16_8_feat         4.1                                                  5.2
              tanh64_48                14.6                                                 14.6
              tanh64x64_both           10.9                                                 10.1
    lengths   tanh7_5, tanh64x64_both  5.0, 10.8                                            5.0, 11.2
    counts    tanh7_5, tanh64_48, tanh64x64_both   5.5, 11.0, 19.9                          5.5, 11.0, 25.3
    tiles     tanh7_5                  0.6                                                  1.0
The maximum is 91.28 (tanh9x5_6x7_both, all 16 chunks, torch autograd; the manual backward in float32 reaches 11.5 on the Xeon: with 16 chunks nothing
averages, and the scale of a chunk whose value error v - ret is small is small with it).  The same test asserts K_CPU on both hosts, so K_CPU = 92 is the larger
maximum rounded up to the next integer (tests/layer_norm_ref.py's rule); it is NOT taken from anything the kernel computes."""
import math

import numpy as np
import torch

import gru_ref
from mqe.engine import abi

EPS32 = 2.0 ** -24
SENT = 0x7FC12345
LN2PI = math.log(2 * math.pi)
CLIP, VALUE_CLIP = 0.2, 0.2
LN_EPS = 1e-5
K_CPU = 92.0
K_GPU = 4 * K_CPU
CFG = dict(clip=CLIP, value_coef=0.7, entropy_coef=0.01, value_clip=VALUE_CLIP)

# (hidden widths of the actor, of the critic, activation, hidden norm, feature norm)
SHAPES = {
    "tanh7_5": ((7,), (5,), "tanh", False, False),                          # dword weight loads, Ha != Hc
    "tanh9x5_6x7_both": ((9, 5), (6, 7), "tanh", True, True),               # three Linear layers, both norms, odd widths
    "tanh16_12_hidden": ((16,), (12,), "tanh", True, False),
    "relu17x16_8_feat": ((17, 16), (8,), "relu", False, True),
    "tanh64_48": ((64,), (48,), "tanh", False, False),
    "tanh64x64_both": ((64, 64), (64, 64), "tanh", True, True),             # the learner's configuration
}
# THE CASES the GPU test runs and K_CPU is measured over, on the same minibatches: (shape, N, T, L, ((first, count, index list?, value clipping?), ...));
# go1gate: D = 16, A' = 2, so N = 4 is 8 rows
def _all(n):
    return ((0, n, False, True), (1, n - 2, True, True))


CASES = {
    # every shape at L = 5 (16 chunks): all chunks by an index list, a range with first > 0, and one call without value clipping
    "shapes": [(name, 4, 10, 5, ((0, 16, True, True), (3, 11, False, True), (2, 9, True, False))) for name in SHAPES],
    # L = 1 (no carried gradient), L = 2, L = T (one chunk per row)
    "lengths": [(name, 4, 10, L, _all(80 // L)) for name in ("tanh7_5", "tanh64x64_both") for L in (1, 2, 10)],
    # the edges of a 64-chunk tile and of two and four 32-chunk tiles
    "counts": [(name, 4, 34, 2, ((0, 1, False, True), (0, 63, True, True), (5, 64, False, True), (0, 65, True, True), (6, 130, True, True)))
               for name in ("tanh7_5", "tanh64_48", "tanh64x64_both")],
    # 18 432 chunks = 288 tiles of 64 for 256 workgroups: a workgroup walks a second tile.  The smallest networks
    "tiles": [("tanh7_5", 1024, 18, 2, ((0, 18432, False, True),))],
}
WRONG = ("mask_ignored_in_carry", "state_unmasked_step0", "carry_across_first_step", "stale_state", "dghn_no_r", "inv_m_count", "no_gru_norm_grad")


def dims_of(name, D):
    a_h, c_h, act, hidden, feat = SHAPES[name]
    return [D, *a_h, 3], [D, *c_h, 1], act, hidden, feat


def named(actor, critic, log_std, a_dims, c_dims, hidden, feat):
    """{engine name: float32 tensor} of a RecurrentMLP pair (abi.actor_param_layout(recurrent=True) over gru_ref.flat_params)"""
    flat = gru_ref.flat_params(actor, critic, log_std)
    lay = abi.actor_param_layout(a_dims, c_dims, False, hidden, feat, recurrent=True)
    return {n: flat[o:o + int(np.prod(shp))].reshape(shp).clone() for n, (o, shp) in lay.items()}


def flat_of(g, s):
    lay = abi.actor_param_layout(s["a_dims"], s["c_dims"], False, s["hidden"], s["feat"], recurrent=True)
    flat = torch.zeros(s["n_params"], dtype=torch.float64)
    for n, (o, shp) in lay.items():
        flat[o:o + int(np.prod(shp))] = torch.as_tensor(np.asarray(g[n], dtype=np.float64)).reshape(-1)
    return flat


def selection(s, first, count, use_index):
    """the chunk numbers of a minibatch: a slice of the trajectory's seeded permutation, or the range"""
    return s["index"][first:first + count].numpy() if use_index else np.arange(first, first + count)


def chunk_steps(s, chunks, L):
    """chunk numbers -> (t (L, C), r (C,)): the steps and the row of every chunk"""
    c = np.asarray(chunks, dtype=np.int64)
    tc, r = c // s["R"], c % s["R"]
    return tc[None, :] * L + np.arange(L)[:, None], r


# ---- the float64 twin ------------------------------------------------------------------------------------------------------------------------------
def loss_of(mean, v, ls, b, cfg, M):
    """ppo_ref's loss on given network outputs: mean (S, 3), v (S,), the samples' data b -> (L, stats[6]); sums / M"""
    c, vc, ec, cv = cfg["clip"], cfg["value_coef"], cfg["entropy_coef"], cfg["value_clip"]
    z = (b["actions"] - mean) * torch.exp(-ls)
    logp = (-0.5 * z * z - ls).sum(-1) - 1.5 * LN2PI
    ratio = torch.exp(logp - b["logp_old"])
    Lpi = -torch.minimum(ratio * b["adv"], torch.clamp(ratio, 1 - c, 1 + c) * b["adv"])
    Lv = (v - b["ret"]) ** 2
    if cv is not None:
        v_c = b["v_old"] + torch.clamp(v - b["v_old"], -cv, cv)
        Lv = torch.maximum(Lv, (v_c - b["ret"]) ** 2)
    H = ls.sum() + 1.5 * (1 + LN2PI)
    Lpi_m, Lv_m = Lpi.sum() / M, Lv.sum() / M
    L = Lpi_m + vc * Lv_m - ec * H
    return L, torch.stack([Lpi_m, Lv_m, H, L, (b["logp_old"] - logp).sum() / M, ((ratio - 1).abs() > c).to(L.dtype).sum() / M]), logp


def twin_outputs(actor, critic, s, chunks, L, dtype):
    """RecurrentMLP.evaluate of both networks over the chunks: -> (mean (L, C, 3), v (L, C)) in `dtype`, differentiable"""
    t, r = chunk_steps(s, chunks, L)
    obs = s["obs"][t, r[None, :]].to(dtype)                                    # (L, C, D)
    masks = (1 - s["done"][t, r[None, :] // s["Aw"]].to(dtype))[..., None]
    h0 = s["tails"][t[0], r].to(dtype)
    Ha = s["a_dims"][-2]
    mean, _ = actor.evaluate(obs, h0[:, :Ha], masks)
    v, _ = critic.evaluate(obs, h0[:, Ha:], masks)
    return mean, v[..., 0]


def sample_data(s, chunks, L, dtype=torch.float64):
    t, r = chunk_steps(s, chunks, L)
    return {k: s[k][t, r[None, :]].to(dtype) for k in ("actions", "logp_old", "adv", "v_old", "ret")}


def autograd(s, chunks, L, cfg, dtype=torch.float64, nets=None):
    """torch autograd of the loss over the chunks at `dtype`: -> ({name: grad}, stats, logp (L, C))"""
    actor, critic, log_std = nets or s["nets"]
    import copy
    actor, critic = copy.deepcopy(actor).to(dtype), copy.deepcopy(critic).to(dtype)
    ls = log_std.detach().to(dtype).clone().requires_grad_(True)
    mean, v = twin_outputs(actor, critic, s, chunks, L, dtype)
    b = sample_data(s, chunks, L, dtype)
    loss, stats, logp = loss_of(mean, v, ls, b, cfg, len(chunks) * L)
    loss.backward()
    ps = list(actor.parameters()) + list(critic.parameters()) + [ls]
    flat = torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1) for p in ps]).detach()
    lay = abi.actor_param_layout(s["a_dims"], s["c_dims"], False, s["hidden"], s["feat"], recurrent=True)
    return {n: flat[o:o + int(np.prod(shp))].reshape(shp) for n, (o, shp) in lay.items()}, stats.detach(), logp.detach()


# ---- the manual backward -----------------------------------------------------------------------------------------------------------------------------
def _ln(a, g, b):
    mu = a.mean(-1, keepdims=True)
    xc = a - mu
    rstd = 1 / np.sqrt((xc * xc).mean(-1, keepdims=True) + a.dtype.type(LN_EPS))
    xh = xc * rstd
    return g * xh + b, xh, rstd


def _ln_back(du, xh, rstd, g):
    dxh = du * g
    return rstd * (dxh - dxh.mean(-1, keepdims=True) - xh * (dxh * xh).mean(-1, keepdims=True))


def _sig(v):
    return 1 / (1 + np.exp(-v))


class _Net:
    """one network's forward of one step with everything the backward needs, and that backward: numpy, rows = chunks"""

    def __init__(self, p, who, dims, act, hidden, feat, variant):
        self.p, self.who, self.dims, self.act, self.hidden, self.feat, self.variant = p, who, dims, act, hidden, feat, variant
        self.nl = len(dims) - 1

    def w(self, name):
        return self.p[f"{self.who}.{name}"]

    def forward(self, obs, hin):
        k = dict(hin=hin)
        x = obs
        if self.feat:
            x, k["fxh"], k["frstd"] = _ln(obs, self.w("norm_in.weight"), self.w("norm_in.bias"))
        k["xs"], k["acts"], k["norms"], k["pres"] = [], [], [], []
        for l in range(self.nl - 1):
            k["xs"].append(x)
            pre = x @ self.w(f"{l}.weight").T + self.w(f"{l}.bias")
            a = np.tanh(pre) if self.act == "tanh" else np.maximum(pre, 0)
            k["pres"].append(pre)
            k["acts"].append(a)
            if self.hidden:
                x, xh, rstd = _ln(a, self.w(f"{l}.norm.weight"), self.w(f"{l}.norm.bias"))
                k["norms"].append((xh, rstd))
            else:
                x = a
        H = self.dims[-2]
        gi = x @ self.w("gru.weight_ih").T + self.w("gru.bias_ih")
        gh = hin @ self.w("gru.weight_hh").T + self.w("gru.bias_hh")
        r, z = _sig(gi[:, :H] + gh[:, :H]), _sig(gi[:, H:2 * H] + gh[:, H:2 * H])
        n = np.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
        hp = (1 - z) * n + z * hin
        k.update(x=x, r=r, z=z, n=n, ghn=gh[:, 2 * H:], hp=hp)
        xo = hp
        if self.hidden:
            xo, k["gxh"], k["grstd"] = _ln(hp, self.w("gru.norm.weight"), self.w("gru.norm.bias"))
        k["xo"] = xo
        k["out"] = xo @ self.w(f"{self.nl - 1}.weight").T + self.w(f"{self.nl - 1}.bias")
        return k

    def backward(self, k, dout, carry, G):
        """dout (C, out): the head's delta; carry (C, H): the state gradient from the step behind, already masked.  Adds the step's per-chunk
        gradients to G[name] (C, ...) and -> dh (C, H), the gradient with respect to the step's (masked) input state"""
        who, nl, H = self.who, self.nl, self.dims[-2]
        add = lambda name, v: G.__setitem__(f"{who}.{name}", G.get(f"{who}.{name}", 0) + v)
        outer = lambda d, x: d[:, :, None] * x[:, None, :]
        add(f"{nl - 1}.weight", outer(dout, k["xo"]))
        add(f"{nl - 1}.bias", dout)
        dhp = dout @ self.w(f"{nl - 1}.weight")
        if self.hidden:
            add("gru.norm.weight", dhp * k["gxh"])
            add("gru.norm.bias", dhp)
            if self.variant != "no_gru_norm_grad":
                dhp = _ln_back(dhp, k["gxh"], k["grstd"], self.w("gru.norm.weight"))
        dhp = dhp + carry
        r, z, n, ghn, hin = k["r"], k["z"], k["n"], k["ghn"], k["hin"]
        dn, dz, dh = dhp * (1 - z), dhp * (hin - n), dhp * z
        dan = dn * (1 - n * n)
        dar = (dan * ghn) * r * (1 - r)
        daz = dz * z * (1 - z)
        dgi = np.concatenate([dar, daz, dan], -1)
        dgh = np.concatenate([dar, daz, dan if self.variant == "dghn_no_r" else dan * r], -1)
        add("gru.weight_ih", outer(dgi, k["x"]))
        add("gru.bias_ih", dgi)
        add("gru.weight_hh", outer(dgh, hin))
        add("gru.bias_hh", dgh)
        dh = dh + dgh @ self.w("gru.weight_hh")
        da = dgi @ self.w("gru.weight_ih")
        for l in range(nl - 2, -1, -1):
            a = k["acts"][l]
            if self.hidden:
                xh, rstd = k["norms"][l]
                add(f"{l}.norm.weight", da * xh)
                add(f"{l}.norm.bias", da)
                da = _ln_back(da, xh, rstd, self.w(f"{l}.norm.weight"))
            delta = da * ((1 - a * a) if self.act == "tanh" else (a > 0).astype(a.dtype))
            add(f"{l}.weight", outer(delta, k["xs"][l]))
            add(f"{l}.bias", delta)
            da = delta @ self.w(f"{l}.weight")
        if self.feat:
            add("norm_in.weight", da * k["fxh"])
            add("norm_in.bias", da)
        return dh


def _heads(p, mean, v, b, cfg, inv_m):
    """the loss heads of csrc/kernels_ppo.hpp (selects at the kinks): -> (dmean (C, 3), dv (C, 1), dlog_std per chunk (C, 3), sums[4])"""
    c, vc, cv = cfg["clip"], cfg["value_coef"], cfg["value_clip"]
    ls = p["log_std"]
    inv = np.exp(-ls)
    z = (b["actions"] - mean) * inv
    logp = (-0.5 * z * z - ls).sum(-1) - 1.5 * LN2PI
    ratio = np.exp(logp - b["logp_old"])
    adv = b["adv"]
    Lpi = -np.minimum(ratio * adv, np.clip(ratio, 1 - c, 1 + c) * adv)
    gate = ((adv > 0) & (ratio > 1 + c)) | ((adv < 0) & (ratio < 1 - c))
    dlp = np.where(gate, 0, -adv * ratio * inv_m).astype(mean.dtype)
    d1 = v - b["ret"]
    Lv, dv = d1 * d1, 2 * d1
    if cv is not None:
        vo = b["v_old"]
        d2 = vo + np.clip(v - vo, -cv, cv) - b["ret"]
        Lv = np.maximum(d1 * d1, d2 * d2)
        dv = np.where(d1 * d1 >= d2 * d2, 2 * d1, np.where(np.abs(v - vo) < cv, 2 * d2, 0))
    sums = np.array([Lpi.sum(), Lv.sum(), (b["logp_old"] - logp).sum(), (np.abs(ratio - 1) > c).sum()], dtype=np.float64)
    return dlp[:, None] * z * inv, (vc * inv_m * dv)[:, None].astype(mean.dtype), dlp[:, None] * (z * z - 1), sums


def _chunks_backward(s, p, nets, chunks, L, cfg, inv_m, dtype, variant, extra=None):
    """forward and backward of a set of chunks: -> (G {name: per-chunk gradient (C, ...)}, sums[4], dh0 {who: (C, H)} the masked state gradient
    of the chunks' first step).  extra {who: (C, H)}: a state gradient entering behind the last step (the wrong variant that carries across chunks)"""
    t, r = chunk_steps(s, chunks, L)
    C = len(r)
    np_of = lambda k: s[k].numpy()[t, r[None, :]].astype(dtype)
    obs = np_of("obs")
    mask = (1 - s["done"].numpy()[t, r[None, :] // s["Aw"]]).astype(dtype)[..., None]      # (L, C, 1)
    b = {k: np_of(k) for k in ("actions", "logp_old", "adv", "v_old", "ret")}
    tails = s["tails"].numpy()[t, r[None, :]].astype(dtype)                             # (L, C, Hs)
    Ha = s["a_dims"][-2]
    kept = {"actor": [], "critic": []}
    for who, net in nets.items():
        sl = slice(0, Ha) if who == "actor" else slice(Ha, None)
        h = None
        for j in range(L):
            if j == 0:
                hin = tails[0][:, sl] * (1 if variant == "state_unmasked_step0" else mask[0])
            elif variant == "stale_state":
                hin = tails[j][:, sl] * mask[j]
            else:
                hin = h * mask[j]
            k = net.forward(obs[j], hin)
            h = k["hp"]
            kept[who].append(k)
    G = {"log_std": np.zeros((C, 3), dtype)}
    sums = np.zeros(4)
    carry = {who: (extra[who].astype(dtype) if extra is not None else np.zeros((C, net.dims[-2]), dtype)) for who, net in nets.items()}
    for j in range(L - 1, -1, -1):
        bj = {k: v[j] for k, v in b.items()}
        dmean, dv, dls, sm = _heads(p, kept["actor"][j]["out"], kept["critic"][j]["out"][:, 0], bj, cfg, inv_m)
        G["log_std"] += dls
        sums += sm
        for who, net in nets.items():
            dh = net.backward(kept[who][j], dmean if who == "actor" else dv, carry[who], G)
            if variant == "stale_state":
                dh = np.zeros_like(dh)
            carry[who] = dh * (1 if variant == "mask_ignored_in_carry" else mask[j])
    return G, sums, carry


def manual(s, chunks, L, cfg, dtype=np.float64, tile=None, variant=None):
    """The manual backward at `dtype` over the minibatch `chunks`, accumulated over tiles of `tile` chunks in order (None: all at once):
    -> (grads {name: array}, stats[6] float64, S {name: float}).  variant: one of WRONG, each a wrong gradient (or a wrong forward)."""
    a_dims, c_dims, act, hidden, feat = s["a_dims"], s["c_dims"], s["act"], s["hidden"], s["feat"]
    p = {k: v.numpy().astype(dtype) for k, v in s["params"].items()}
    nets = {"actor": _Net(p, "actor", a_dims, act, hidden, feat, variant), "critic": _Net(p, "critic", c_dims, act, hidden, feat, variant)}
    chunks = np.asarray(chunks, dtype=np.int64)
    M = len(chunks) * (1 if variant == "inv_m_count" else L)
    inv_m = dtype(1.0 / M)
    g = {k: np.zeros(v.shape, dtype) for k, v in p.items()}
    S = {k: np.zeros(v.shape, np.float64) for k, v in p.items()}
    sums = np.zeros(4)

    def take(G, sm):
        nonlocal sums
        for name, v in G.items():
            g[name] += v.sum(0)
            S[name] += np.abs(v.astype(np.float64)).sum(0)
        sums += sm

    if variant == "carry_across_first_step":
        # the state gradient of a chunk's first step enters the chunk in front of it (same row) behind its last step, as if the recorded state
        # were the computed one: time blocks from the last down
        tc = chunks // s["R"]
        dh0 = {}
        for blk in sorted(set(tc.tolist()), reverse=True):
            sel = chunks[tc == blk]
            extra = {who: np.stack([dh0.get((who, int(c) + s["R"]), np.zeros(net.dims[-2])) for c in sel]) for who, net in nets.items()}
            G, sm, carry = _chunks_backward(s, p, nets, sel, L, cfg, inv_m, dtype, variant, extra)
            take(G, sm)
            for who in nets:
                for i, c in enumerate(sel):
                    dh0[(who, int(c))] = carry[who][i]
    else:
        tile = tile or len(chunks)
        for c0 in range(0, len(chunks), tile):
            take(*_chunks_backward(s, p, nets, chunks[c0:c0 + tile], L, cfg, inv_m, dtype, variant)[:2])
    ec = cfg["entropy_coef"]
    g["log_std"] = g["log_std"] - dtype(ec)
    S["log_std"] = S["log_std"] + ec
    n = len(chunks) * L
    ls = p["log_std"].astype(np.float64)
    H = ls.sum() + 1.5 * (1 + LN2PI)
    Lpi, Lv = sums[0] / n, sums[1] / n
    stats = np.array([Lpi, Lv, H, Lpi + cfg["value_coef"] * Lv - ec * H, sums[2] / n, sums[3] / n])
    return g, stats, {k: float(v.max()) for k, v in S.items()}


def ratio_to_bound(g, g64, S):
    """max over the tensors of max |g - g64| / (2^-24 S_n); a tensor with S_n = 0 must be exactly 0 (ratio inf otherwise) -> (ratio, name)"""
    worst, at = 0.0, None
    for name, sc in S.items():
        d = float(np.abs(np.asarray(g[name], dtype=np.float64) - np.asarray(g64[name], dtype=np.float64)).max())
        r = (0.0 if d == 0.0 else math.inf) if sc == 0.0 else d / (EPS32 * sc)
        if r >= worst:
            worst, at = r, name
    return worst, at


# ---- the synthetic trajectory ---------------------------------------------------------------------------------------------------------------------------
def _kinked(s, nets64, chunks, L, cfg):
    """bool per chunk: a step of it lies within ppo_ref's distances of a kink of the loss (float64)"""
    actor, critic, log_std = nets64
    t, r = chunk_steps(s, chunks, L)
    with torch.no_grad():
        mean, v = twin_outputs(actor, critic, s, chunks, L, torch.float64)
    b = sample_data(s, chunks, L)
    c, cv = cfg["clip"], cfg["value_clip"]
    ls = log_std.double()
    z = (b["actions"] - mean) * torch.exp(-ls)
    ratio = torch.exp((-0.5 * z * z - ls).sum(-1) - 1.5 * LN2PI - b["logp_old"])
    bad = ((ratio - (1 + c)).abs() < 1e-3) | ((ratio - (1 - c)).abs() < 1e-3) | (b["adv"].abs() < 1e-3)
    vo, ret = b["v_old"], b["ret"]
    bad |= ((v - vo).abs() - cv).abs() < 1e-3
    v_c = vo + torch.clamp(v - vo, -cv, cv)
    bad |= ((v - vo).abs() > cv) & (((v - ret) ** 2 - (v_c - ret) ** 2).abs() < 1e-3)
    if s["act"] == "relu":                        # a hidden pre-activation near 0: the base sees the observation alone
        obs = s["obs"][t, r[None, :]].double()
        for net in (actor, critic):
            x = obs
            for m in net.base:
                x = m(x)
                if isinstance(m, torch.nn.Linear):
                    bad |= (x.abs() < 1e-4).any(-1)
    return bad.any(0), mean, v


def synth(name, N, T, L, D=16, seed=0, Aw=2, extra_stride=8, guard=64):
    """A seeded kink-free trajectory of T steps over R = N Aw rows for the recurrent pair SHAPES[name], in mqe_ppo_grad's buffers, for chunk length
    L.  Observations N(0, 1); recorded tails 0.5 N(0, 1) on every row (data: NOT what the current parameters would compute); done bytes with
    probability 0.3 per (row of the trajectory, env), row 0 included; per sample action = mean64 + exp(log_std) N(0, 1), logp_old = logp64 + 0.25
    N(0, 1), adv N(0, 1), v_old = v64 + 0.3 N(0, 1), ret = v64 + N(0, 1) with mean64 / v64 the float64 twin's over the sample's chunk.  Every chunk
    with a step inside a kink margin gets fresh observations and samples until none is left.  -> dict: nets (actor, critic, log_std), params
    {name: float32}, the logical tensors obs (T + 1, R, D), done (T + 1, N) uint8, tails (T + 1, R, Hs), actions (T, R, 3), logp_old, adv, v_old,
    ret (T, R), index (a seeded int32 permutation of the chunks), and the flat int32 images packed / value / grad / stats with sentinels and guards."""
    a_dims, c_dims, act, hidden, feat = dims_of(name, D)
    assert T % L == 0
    R = N * Aw
    Hs = a_dims[-2] + c_dims[-2]
    actor, critic, log_std = gru_ref.make_nets(D, tuple(a_dims[1:-1]), tuple(c_dims[1:-1]), act, hidden, feat, seed=700 + seed)
    a64, c64 = gru_ref.doubles(actor, critic)
    g = torch.Generator().manual_seed(seed)
    s = dict(name=name, N=N, Aw=Aw, T=T, D=D, R=R, L=L, Hs=Hs, n=T * R, n_chunks=(T // L) * R, a_dims=a_dims, c_dims=c_dims, act=act, hidden=hidden, feat=feat,
             nets=(actor, critic, log_std), params=named(actor, critic, log_std, a_dims, c_dims, hidden, feat))
    s["n_params"] = abi.actor_param_count(a_dims, c_dims, False, hidden, feat, recurrent=True)
    s["obs"] = torch.randn(T + 1, R, D, generator=g)
    s["done"] = (torch.rand(T + 1, N, generator=g) < 0.3).to(torch.uint8)
    s["tails"] = 0.5 * torch.randn(T + 1, R, Hs, generator=g)
    for k, shp in (("actions", (T, R, 3)), ("logp_old", (T, R)), ("adv", (T, R)), ("v_old", (T, R)), ("ret", (T, R))):
        s[k] = torch.zeros(shp)
    todo = np.arange(s["n_chunks"])
    redraws = 0
    nets64 = (a64, c64, log_std)
    ls = log_std.double()
    for it in range(200):
        t, r = chunk_steps(s, todo, L)
        if it:
            s["obs"][t, r[None, :]] = torch.randn(L, len(todo), D, generator=g)
        with torch.no_grad():
            mean, v = twin_outputs(a64, c64, s, todo, L, torch.float64)
        act_ = mean + torch.exp(ls) * torch.randn(L, len(todo), 3, generator=g).double()
        zz = (act_.float().double() - mean) * torch.exp(-ls)
        logp = (-0.5 * zz * zz - ls).sum(-1) - 1.5 * LN2PI
        s["actions"][t, r[None, :]] = act_.float()
        s["logp_old"][t, r[None, :]] = (logp + 0.25 * torch.randn(L, len(todo), generator=g).double()).float()
        s["adv"][t, r[None, :]] = torch.randn(L, len(todo), generator=g)
        s["v_old"][t, r[None, :]] = (v + 0.3 * torch.randn(L, len(todo), generator=g).double()).float()
        s["ret"][t, r[None, :]] = (v + torch.randn(L, len(todo), generator=g).double()).float()
        bad = _kinked(s, nets64, todo, L, dict(clip=CLIP, value_clip=VALUE_CLIP))[0].numpy()
        todo = todo[bad]
        if len(todo) == 0:
            break
        redraws += len(todo)
    else:
        raise RuntimeError("synth: chunks inside a kink margin remain")
    s["redraws"] = redraws
    s["index"] = torch.randperm(s["n_chunks"], generator=g).to(torch.int32)
    nobs = R * D
    pf = nobs + R + (N + 3) // 4
    p4 = (pf + 3) // 4 * 4
    stride = (p4 + R * Hs + 3) // 4 * 4 + extra_stride
    packed = np.full((T + 1) * stride + guard, SENT, np.int32)
    rows = packed[:(T + 1) * stride].reshape(T + 1, stride)
    rows[:, :nobs] = s["obs"].numpy().reshape(T + 1, nobs).view(np.int32)
    rows[:, nobs + R:nobs + R + (N + 3) // 4] = 0
    rows.view(np.uint8).reshape(T + 1, stride * 4)[:, (nobs + R) * 4:(nobs + R) * 4 + N] = s["done"].numpy()
    rows[:, p4:p4 + R * Hs] = s["tails"].numpy().reshape(T + 1, R * Hs).view(np.int32)
    value = np.concatenate([s["v_old"].numpy().reshape(-1), torch.randn(R, generator=g).numpy()]).view(np.int32).copy()
    out = lambda k: np.full(k + guard, SENT, np.int32)
    s.update(nobs=nobs, pf=pf, p4=p4, stride=stride, guard=guard, packed=packed, value=value, grad=out(s["n_params"]), stats=out(abi.PPO_STATS))
    return s


def resets_inside(s, chunks, L):
    """(share of the chunks with a reset at a step j >= 1, share with one at step 0)"""
    t, r = chunk_steps(s, chunks, L)
    d = s["done"].numpy()[t, r[None, :] // s["Aw"]] != 0
    return (float(d[1:].any(0).mean()) if L > 1 else 0.0), float(d[0].mean())
