"""The nine forms of an actor that FusedTaskWrapper.set_actor accepts, at D = 16 with hidden widths (8,) and (7, 5): shared by tests/test_actor_tensors.py
(the ordered tensor list of mqe.utils.actor_net.actor_tensors against abi.actor_param_layout) and tests/test_actor_handle_gpu.py (the round trip through
the engine's buffer).  7 and 5 are no multiple of 4 (the kernels' dword path) and give Ha != Hc."""
import torch

from gru_ref import base_of, flat_params  # noqa: F401  (flat_params: parameters_to_vector in module order, then log_std -- the engine's buffer)
from mqe.utils.actor_net import RecurrentMLP

D = 16
# name: (actor's hidden widths, critic's or None, feature norm, hidden norm, recurrent)
VARIANTS = {
    "plain": ((7, 5), (8,), False, False, False),
    "feature_norm": ((8,), (7, 5), True, False, False),
    "hidden_norm": ((7, 5), (8,), False, True, False),
    "both_norms": ((8,), (7, 5), True, True, False),
    "single_linear": ((), (8,), True, True, False),         # the actor is one Linear layer: it has the feature norm and no hidden norm
    "actor_alone": ((7, 5), None, False, False, False),
    "recurrent": ((7, 5), (8,), False, False, True),
    "recurrent_hidden_norm": ((8,), (7, 5), False, True, True),
    "recurrent_both_norms": ((7, 5), (8,), True, True, True),
}


def modules(name, seed):
    """(actor, critic or None, log_std) of a variant (its name, or a tuple in VARIANTS' form), float32 on the host, EVERY parameter drawn from the
    seed (no gamma left at 1, no bias at 0)"""
    a_h, c_h, feat, hidden, recurrent = VARIANTS.get(name, name)
    nn = torch.nn

    def net(widths, out):
        base = base_of(D, widths, "tanh", hidden, feat)
        return RecurrentMLP(base, out) if recurrent else nn.Sequential(*base, nn.Linear(widths[-1] if widths else D, out))
    nets = [net(a_h, 3)] + ([net(c_h, 1)] if c_h is not None else [])
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in nets:
            for p in m.parameters():
                p.copy_(torch.rand(p.shape, generator=g) - 0.5)
    return nets[0], (nets[1] if c_h is not None else None), torch.rand(3, generator=g) - 1.0


def set_actor_kw(name):
    _, _, feat, hidden, recurrent = VARIANTS.get(name, name)
    return dict(layer_norm=feat or hidden, recurrent=recurrent)


def layout_kw(name):
    a_h, c_h, feat, hidden, recurrent = VARIANTS.get(name, name)
    return dict(actor_dims=[D, *a_h, 3], critic_dims=[D, *c_h, 1] if c_h is not None else None, layer_norm=hidden, feature_norm=feat, recurrent=recurrent)
