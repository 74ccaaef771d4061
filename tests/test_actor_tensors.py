"""mqe.utils.actor_net.actor_tensors, the one ordered list FusedTaskWrapper.sync_actor and pull_actor walk: for every form of an actor that set_actor
accepts (tests/actor_variants.py) its names are abi.actor_param_layout's in the layout's order, its tensors have the layout's shapes, and its
concatenation is the modules' own parameter vector -- the engine's flat buffer."""
import pytest
import torch

import actor_variants as av
from mqe.engine import abi
from mqe.utils.actor_net import actor_tensors, mlp_spec, recurrent_spec


def tensors_of(name, actor, critic):
    recurrent = av.VARIANTS[name][4]
    out = []
    for who, module, width in (("actor", actor, 3), ("critic", critic, 1)):
        if module is None:
            continue
        if recurrent:
            _, _, linears, norms, rnn = recurrent_spec(module, who, av.D, width, layer_norm=True)
        else:
            (_, _, linears, norms), rnn = mlp_spec(module, who, av.D, width, layer_norm=True), None
        out += actor_tensors(who, linears, norms, rnn)
    return out


@pytest.mark.parametrize("name", list(av.VARIANTS))
def test_the_list_is_the_layout(name):
    actor, critic, log_std = av.modules(name, seed=1)
    listed = tensors_of(name, actor, critic) + [("log_std", log_std)]
    layout = abi.actor_param_layout(value_norm=critic is not None, **av.layout_kw(name))
    if critic is not None:
        assert list(layout)[-1] == "value_norm"
    layout.pop("value_norm", None)
    assert [n for n, _ in listed] == list(layout)
    for n, t in listed:
        assert tuple(t.shape) == layout[n][1], n
    assert len({t.data_ptr() for _, t in listed}) == len(listed), "every tensor once"
    flat = torch.cat([t.detach().reshape(-1) for _, t in listed])
    assert torch.equal(flat, av.flat_params(actor, critic, log_std))
    assert flat.numel() == abi.actor_param_count(**av.layout_kw(name))
    # the layout's offsets are where the concatenation puts each tensor
    for n, t in listed:
        off = layout[n][0]
        assert torch.equal(flat[off:off + t.numel()], t.detach().reshape(-1)), n


def test_plain_networks_through_the_three_value_form():
    """set_actor without layer_norm reads mlp_spec's three values and no norms: the same list"""
    actor, critic, _ = av.modules("plain", seed=2)
    no_norms = {"feature": None, "hidden": []}
    listed = []
    for who, module, width in (("actor", actor, 3), ("critic", critic, 1)):
        found = mlp_spec(module, who, av.D, width)
        assert len(found) == 3
        listed += actor_tensors(who, found[2], no_norms)
    assert [n for n, _ in listed] == [n for n, _ in tensors_of("plain", actor, critic)]
    assert all(a is b for (_, a), (_, b) in zip(listed, tensors_of("plain", actor, critic)))
