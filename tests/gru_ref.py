"""Host reference of the engine's recurrent actor-critic (MQE_ACTOR_RECURRENT; csrc/kernels_gru.hpp): the GRU cell by its definition in any dtype
(float64: the reference), the float32 twin that restates the kernel's rounding points, seeded mqe.utils.actor_net.RecurrentMLP pairs in the engine's
layout, and one rollout step of such a pair on the host.  No GPU, no engine."""
import copy

import torch

from mqe.utils.actor_net import RecurrentMLP

# the shapes the GPU test holds the kernel to (hidden widths of the actor, of the critic or None, activation, hidden norm, feature norm)
SHAPES = {
    "a_tanh7_5": ((7,), (5,), "tanh", False, False),                       # dword path, short unit blocks, Ha != Hc
    "b_tanh64x64_norms": ((64, 64), (64, 64), "tanh", True, True),
    "c_relu128x3_hidden": ((128, 128, 128), (128, 128, 128), "relu", True, False),
    "d_tanh16_alone": ((16,), None, "tanh", False, False),                 # the actor alone
}


def gru_cell(x, h, w_ih, w_hh, b_ih, b_hh):
    """torch.nn.GRU's cell by its definition, gate order r, z, n, in the arguments' dtype: -> h'"""
    H = h.shape[-1]
    gi, gh = x @ w_ih.T + b_ih, h @ w_hh.T + b_hh
    r = torch.sigmoid(gi[..., :H] + gh[..., :H])
    z = torch.sigmoid(gi[..., H:2 * H] + gh[..., H:2 * H])
    n = torch.tanh(gi[..., 2 * H:] + r * gh[..., 2 * H:])
    return (1 - z) * n + z * h


def _fma32(a, b, c):
    """fmaf on float32 tensors: the product of two float32 is exact in float64"""
    return (a.double() * b.double() + c.double()).float()


def _chain32(W, b, v):
    """acc = b[o]; k ascending: acc = fmaf(W[o][k], v[k], acc) -- actor_layer's chain, for rows v (..., K) -> (..., O)"""
    acc = b.expand(*v.shape[:-1], b.shape[0]).clone()
    for k in range(W.shape[1]):
        acc = _fma32(W[:, k], v[..., k:k + 1], acc)
    return acc


def gru_cell_f32(x, h, w_ih, w_hh, b_ih, b_hh):
    """the kernel's cell restated in float32 (csrc/kernels_gru.hpp): every gi / gh entry the ascending-k fmaf chain from its bias;
    sigmoid(v) = 1 / (1 + expf(-v)); n = tanhf(fmaf(r, gh_n, gi_n)); h' = fmaf(z, h - n, n).  libm and the division are the host's."""
    H = h.shape[-1]
    x, h, w_ih, w_hh, b_ih, b_hh = (t.float() for t in (x, h, w_ih, w_hh, b_ih, b_hh))
    gi, gh = _chain32(w_ih, b_ih, x), _chain32(w_hh, b_hh, h)
    one = torch.ones((), dtype=torch.float32)
    sig = lambda v: one / (one + torch.exp(-v))
    r, z = sig(gi[..., :H] + gh[..., :H]), sig(gi[..., H:2 * H] + gh[..., H:2 * H])
    n = torch.tanh(_fma32(r, gh[..., 2 * H:], gi[..., 2 * H:]))
    return _fma32(z, h - n, n)


def base_of(D, hidden, act, hidden_norm, feat_norm):
    nn = torch.nn
    layers = [nn.LayerNorm(D)] if feat_norm else []
    k = D
    for n in hidden:
        layers += [nn.Linear(k, n), nn.Tanh() if act == "tanh" else nn.ReLU()] + ([nn.LayerNorm(n)] if hidden_norm else [])
        k = n
    return nn.Sequential(*layers)


def make_nets(D, a_hidden, c_hidden, act="tanh", hidden_norm=False, feat_norm=False, seed=0):
    """seeded float32 (actor, critic or None, log_std): torch's own initialisation, every norm's weight in [0.5, 1.5] and bias in [-0.5, 0.5],
    log_std in [-1, 0.5]"""
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    nets = [RecurrentMLP(base_of(D, a_hidden, act, hidden_norm, feat_norm), 3)]
    if c_hidden is not None:
        nets.append(RecurrentMLP(base_of(D, c_hidden, act, hidden_norm, feat_norm), 1))
    with torch.no_grad():
        for net in nets:
            for m in net.modules():
                if isinstance(m, torch.nn.LayerNorm):
                    m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
                    m.bias.copy_(torch.rand(m.bias.shape, generator=g) - 0.5)
    log_std = torch.rand(3, generator=g) * 1.5 - 1.0
    return nets[0], (nets[1] if c_hidden is not None else None), log_std


def nets_of(name, D, seed=0):
    a_h, c_h, act, hidden, feat = SHAPES[name]
    return make_nets(D, a_h, c_h, act, hidden, feat, seed), dict(actor_dims=[D, *a_h, 3], critic_dims=[D, *c_h, 1] if c_h is not None else None, activation=act,
                                                                 layer_norm=hidden, feature_norm=feat, recurrent=True)


def flat_params(actor, critic, log_std):
    """the engine's flat parameter buffer of the pair: parameters_to_vector in module order (tests/test_gru.py holds abi.actor_param_layout to it)"""
    ps = list(actor.parameters()) + (list(critic.parameters()) if critic is not None else []) + [log_std]
    return torch.nn.utils.parameters_to_vector([p.detach() for p in ps])


def split_hidden(hidden, actor, critic):
    Ha = actor.rnn.hidden_size
    return hidden[..., :Ha], (hidden[..., Ha:] if critic is not None else None)


def step(actor, critic, obs, hidden, done_prev):
    """one rollout step on the host in the modules' dtype: obs (N, A', D), hidden (N, A', Hs) UNMASKED, done_prev (N,) bool or None (no mask) ->
    (mean (N, A', 3), value (N, A') or None, hidden_next (N, A', Hs))"""
    dt = next(actor.parameters()).dtype
    obs, hidden = obs.to(dt), hidden.to(dt)
    mask = torch.ones(obs.shape[:-1] + (1,), dtype=dt) if done_prev is None else (~done_prev.bool()).to(dt)[:, None, None].expand(*obs.shape[:-1], 1)
    ha, hc = split_hidden(hidden, actor, critic)
    with torch.no_grad():
        mean, na = actor(obs, ha, mask)
        if critic is None:
            return mean, None, na
        value, nc = critic(obs, hc, mask)
    return mean, value[..., 0], torch.cat([na, nc], -1)


def yardstick(a32, c32, a64, c64, obs, hidden, done_prev):
    """float64 step and the yardstick: max |float32 CPU step - float64 step| of the mean, the value and the next state"""
    m64, v64, h64 = step(a64, c64, obs, hidden, done_prev)
    m32, v32, h32 = step(a32, c32, obs, hidden, done_prev)
    dev = lambda x32, x64: float((x32.double() - x64).abs().max())
    out = dict(mean64=m64, hidden64=h64, yard_mean=dev(m32, m64), yard_hidden=dev(h32, h64))
    if c64 is not None:
        out.update(value64=v64, yard_value=dev(v32, v64))
    return out


def doubles(actor, critic):
    return copy.deepcopy(actor).double(), (copy.deepcopy(critic).double() if critic is not None else None)


def lds_bytes_c_rule(ldh, Ha, Hc, ln):
    """csrc/kernels_gru.hpp actor_gru_lds_bytes, restated: (2 ldh + 4 + (ln ? 32 : 0) + Ha + Hc) rows of 65 floats"""
    return (2 * ldh + 4 + (32 if ln else 0) + Ha + Hc) * 65 * 4

