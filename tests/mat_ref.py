"""Host reference of the engine's Multi-Agent Transformer policy (MQE_ACTOR_TRANSFORMER; csrc/kernels_mat.hpp): the shapes the tests hold the kernel
to, seeded mqe.utils.actor_net.MATNet twins at a scale where the attention matters, the inputs of the one-step tests, the yardstick (what a
float32 CPU evaluation of the twin deviates from its float64 evaluation on the same inputs), and the WRONG variants a bound must tell apart.
No GPU, no engine."""
import copy
import math

import torch

from mqe.utils.actor_net import MATNet

# n_embd of the shapes: the reference's width; a width that is neither a power of two nor a multiple of 8; the smallest the engine accepts
SHAPES = {"e64": 64, "e12": 12, "e4": 4}
VARIANTS = ("no_mask", "s_zero", "no_scale", "exp_sigma", "tanh_gelu")
# the edges of what the engine accepts, for the rollout: (scene, A', D, E).  NOT part of SHAPES: every test parametrised over SHAPES keeps its cases.
#   E = 68: a second, partial pass of actor_layer's 16 x 4 outputs (4 left), norm chunks of 5 with the last three wavefronts empty
#   E = 92: the largest width mqe_actor_create accepts; 28 outputs in the second pass; norm chunks of 6, the last wavefront with 2
#   go1plane with the seesaw task kind: A' = 1, D = 13 -- nothing on the 16-byte grid
#   go1sheep-hard: D = 34 (629 rows of LDS at E = 92, 300 bytes under the limit; D > E at E = 12; D > 5 E at E = 4), a scene with NPCs
#   go1seesaw D = 14, go1football-defender D = 20: the real tasks' own observations; at D = 14 and 34 obs_fc loads dwords, every E x E matrix 16 bytes
EDGE_SHAPES = {"gate-e68": ("go1gate", 2, 16, 68), "gate-e92": ("go1gate", 2, 16, 92), "plane-e92": ("go1plane", 1, 13, 92),
               "sheep-e92": ("go1sheep-hard", 2, 34, 92), "sheep-e12": ("go1sheep-hard", 2, 34, 12), "sheep-e4": ("go1sheep-hard", 2, 34, 4),
               "seesaw-e64": ("go1seesaw", 2, 14, 64), "defender-e12": ("go1football-defender", 2, 20, 12)}
# envs of a scene in the GPU tests: 74 rows = one full tile and one partial; 70 rows at A' = 1
EDGE_ENVS = {"go1gate": 37, "go1plane": 70, "go1sheep-hard": 37, "go1seesaw": 37, "go1football-defender": 37}
# (make_net's seed, inputs' seed) of an edge shape's one-step test: SHAPES' rule (the name's length, E) unless a wrong variant missed the factor there
EDGE_SEEDS = {}
# with one agent nothing is masked, nothing conditions and the one probability is 1 with or without the scale: these cannot differ at A' = 1
NEED_AGENTS = ("no_mask", "s_zero", "no_scale")


def edge_seeds(name):
    return EDGE_SEEDS.get(name, (len(name), EDGE_SHAPES[name][3]))


def make_net(D, E, seed=0):
    """a seeded float32 MATNet: weights ~ N(0, 1 / fan_in), Linear biases in [-0.1, 0.1], every norm's weight in [0.5, 1.5] and bias in [-0.5, 0.5],
    log_std = three different nonzero values in [-1, 0.5]"""
    g = torch.Generator().manual_seed(seed)
    net = MATNet(D, E)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.Linear):
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) / math.sqrt(m.in_features))
                m.bias.copy_(torch.rand(m.bias.shape, generator=g) * 0.2 - 0.1)
            elif isinstance(m, torch.nn.LayerNorm):
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
                m.bias.copy_(torch.rand(m.bias.shape, generator=g) - 0.5)
        net.log_std.copy_(torch.tensor([-1.0, -0.3, 0.5]) + 0.1 * torch.rand(3, generator=g))
    return net


def flat_params(net):
    """the engine's flat parameter buffer: parameters_to_vector in the module's own order (tests/test_mat.py holds abi.actor_param_layout to it)"""
    return torch.nn.utils.parameters_to_vector([p.detach() for p in net.parameters()])


def doubles(net):
    return copy.deepcopy(net).double()


def inputs(n_envs, A, D, seed=0):
    """(obs (n_envs, A, D) float32 ~ N(0, 1), z (n_envs, A, 3) float32 ~ N(0, 1)): the inputs of the one-step tests, on the CPU and on the GPU"""
    g = torch.Generator().manual_seed(1000 + seed)
    return torch.randn(n_envs, A, D, generator=g), torch.randn(n_envs, A, 3, generator=g)


def _dev(x32, x64):
    return float((x32.double() - x64).abs().max())


def yardstick(n32, n64, obs, actions):
    """float64 evaluation of (obs, actions) and the yardstick: max |float32 CPU evaluation - float64 evaluation| of the mean, logp and the value"""
    with torch.no_grad():
        m64, lp64, v64 = n64.evaluate(obs.double(), actions.double())
        m32, lp32, v32 = n32.evaluate(obs.float(), actions.float())
    return dict(mean64=m64, logp64=lp64, value64=v64, yard_mean=_dev(m32, m64), yard_logp=_dev(lp32, lp64), yard_value=_dev(v32, v64))


def _attn(at, key, value, query, masked, scaled):
    k, v, q = at.key(key), at.value(value), at.query(query)
    s = q @ k.transpose(-1, -2)
    if scaled:
        s = s * (1.0 / math.sqrt(k.shape[-1]))
    if masked:
        n = s.shape[-1]
        s = s.masked_fill(~torch.tril(torch.ones(n, n, dtype=torch.bool)), float("-inf"))
    return at.proj(torch.softmax(s, dim=-1) @ v)


def wrong_evaluate(net, obs, actions, variant):
    """MATNet.evaluate with ONE thing wrong: "no_mask" the decoder's attentions unmasked, "s_zero" the decoder never sees an action, "no_scale" no
    1 / sqrt(E) on the scores, "exp_sigma" sigma = exp(log_std), "tanh_gelu" the tanh approximation of GELU.  variant=None: the network itself,
    written out (tests/test_mat.py holds it to MATNet.evaluate)."""
    assert variant is None or variant in VARIANTS
    F = torch.nn.functional
    gelu = (lambda x: F.gelu(x, approximate="tanh")) if variant == "tanh_gelu" else F.gelu
    masked, scaled = variant != "no_mask", variant != "no_scale"
    e, d = net.enc, net.dec
    x = e.ln(gelu(e.obs_fc(e.obs_norm(obs))))
    x = e.ln1(x + _attn(e.attn, x, x, x, False, scaled))
    rep = e.ln2(x + e.mlp1(gelu(e.mlp0(x))))
    value = net.value_out(e.head_ln(gelu(e.head0(rep))))[..., 0]
    s = torch.cat([torch.zeros_like(actions[..., :1, :]), actions[..., :-1, :]], dim=-2)
    if variant == "s_zero":
        s = torch.zeros_like(s)
    x = d.ln(gelu(d.act_fc(s)))
    x = d.ln1(x + _attn(d.attn1, x, x, x, masked, scaled))
    x = d.ln2(rep + _attn(d.attn2, x, x, rep, masked, scaled))
    x = d.ln3(x + d.mlp1(gelu(d.mlp0(x))))
    mean = net.mean_out(d.head_ln(gelu(d.head0(x))))
    sigma = torch.exp(net.log_std) if variant == "exp_sigma" else 0.5 * torch.sigmoid(net.log_std)
    z = (actions - mean) / sigma
    logp = (-0.5 * z * z - torch.log(sigma)).sum(-1) - 1.5 * math.log(2.0 * math.pi)
    return mean, logp, value


def param_count(D, E):
    """the closed count of abi.actor_param_layout(transformer=True)'s docstring"""
    return 2 * D + D * E + 18 * E * E + 45 * E + 7
