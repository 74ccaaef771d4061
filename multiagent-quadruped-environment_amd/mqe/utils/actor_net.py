"""torch modules -> the engine's actor (mqe_actor_create): which torch.nn.Sequential stacks k_actor can evaluate, and their shapes."""
import torch


def mlp_spec(module, what, in_dim, out_dim):
    """(dims, activation, linears) of a torch.nn.Sequential of Linear / Tanh / ReLU: Linear layers with a bias, one activation -- the same
    kind everywhere -- between two of them, a linear output; dims = [in_dim, hidden ..., out_dim], activation "tanh" / "relu" (None for a
    single Linear).  Anything else raises ValueError and names the offending layer."""
    nn = torch.nn
    if not isinstance(module, nn.Sequential):
        raise ValueError(f"{what}: expected a torch.nn.Sequential of Linear / Tanh / ReLU, got {type(module).__name__}")
    linears, acts = [], []
    expect_linear = True
    for name, layer in module.named_children():
        where = f"{what}[{name}] ({type(layer).__name__})"
        if isinstance(layer, nn.Linear):
            if not expect_linear:
                raise ValueError(f"{where}: two Linear layers with no activation between them")
            if layer.bias is None:
                raise ValueError(f"{where}: Linear without a bias")
            if linears and layer.in_features != linears[-1].out_features:
                raise ValueError(f"{where}: in_features {layer.in_features} does not follow out_features {linears[-1].out_features}")
            linears.append(layer)
            expect_linear = False
        elif isinstance(layer, (nn.Tanh, nn.ReLU)):
            if expect_linear:
                raise ValueError(f"{where}: an activation must follow a Linear layer")
            acts.append((where, "tanh" if isinstance(layer, nn.Tanh) else "relu"))
            expect_linear = True
        else:
            raise ValueError(f"{where}: only Linear, Tanh and ReLU layers can run inside the engine")
    if not linears:
        raise ValueError(f"{what}: no Linear layer")
    if expect_linear:
        raise ValueError(f"{acts[-1][0]}: the output layer must be linear (an activation is the last layer)")
    kinds = {k for _, k in acts}
    if len(kinds) > 1:
        odd = next(w for w, k in acts if k != acts[0][1])
        raise ValueError(f"{odd}: mixed activations; the engine applies one kind ({acts[0][1]} here, from {acts[0][0]}) to every hidden layer")
    if linears[0].in_features != in_dim:
        raise ValueError(f"{what}: the first Linear takes {linears[0].in_features} inputs, the task observation has {in_dim}")
    if linears[-1].out_features != out_dim:
        raise ValueError(f"{what}: the last Linear gives {linears[-1].out_features} outputs, {out_dim} wanted")
    dims = [linears[0].in_features] + [l.out_features for l in linears]
    return dims, (acts[0][1] if acts else None), linears
