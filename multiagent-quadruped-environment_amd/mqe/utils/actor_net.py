"""torch modules -> the engine's actor (mqe_actor_create): which torch.nn.Sequential stacks k_actor can evaluate, and their shapes."""
import torch

LN_EPS = 1e-5          # the only eps the engine's norm has (csrc/kernels_ln.hpp LN_EPS)


def mlp_spec(module, what, in_dim, out_dim, layer_norm=False):
    """(dims, activation, linears) of a torch.nn.Sequential of Linear / Tanh / ReLU: Linear layers with a bias, one activation -- the same
    kind everywhere -- between two of them, a linear output; dims = [in_dim, hidden ..., out_dim], activation "tanh" / "relu" (None for a
    single Linear).  Anything else raises ValueError and names the offending layer.
    layer_norm=True: -> (dims, activation, linears, norms) and torch.nn.LayerNorm(n, eps=1e-5, elementwise_affine=True) is accepted in exactly
    two positions: first of all, on the in_dim observation floats (the feature norm), and directly behind a hidden activation -- behind every
    one or behind none (the hidden norm).  norms = {"feature": LayerNorm or None, "hidden": [LayerNorm per hidden layer] or []}."""
    nn = torch.nn
    if not isinstance(module, nn.Sequential):
        raise ValueError(f"{what}: expected a torch.nn.Sequential of Linear / Tanh / ReLU, got {type(module).__name__}")
    linears, acts = [], []
    feature, hidden = None, {}             # hidden: {index of the hidden layer: (where, LayerNorm)}
    expect_linear = True
    prev = None                            # the kind of the layer before: None, "linear", "act", "norm"
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
            prev = "linear"
        elif isinstance(layer, (nn.Tanh, nn.ReLU)):
            if expect_linear:
                raise ValueError(f"{where}: an activation must follow a Linear layer")
            acts.append((where, "tanh" if isinstance(layer, nn.Tanh) else "relu"))
            expect_linear = True
            prev = "act"
        elif layer_norm and isinstance(layer, nn.LayerNorm):
            if prev is None:
                width = in_dim
            elif prev == "act":
                width = linears[-1].out_features
            elif prev == "linear":
                raise ValueError(f"{where}: a LayerNorm directly behind a Linear layer (behind the output, or in front of the activation); the engine's "
                                 f"norm sits behind a hidden activation or on the observation")
            else:
                raise ValueError(f"{where}: two LayerNorm layers in a row")
            if not layer.elementwise_affine or layer.weight is None or layer.bias is None:
                raise ValueError(f"{where}: elementwise_affine=False (or no bias); the engine's norm has a weight and a bias")
            if float(layer.eps) != LN_EPS:
                raise ValueError(f"{where}: eps {layer.eps!r}; the engine's norm has eps = 1e-5 only")
            if tuple(layer.normalized_shape) != (width,):
                raise ValueError(f"{where}: normalized_shape {tuple(layer.normalized_shape)} is not the preceding width ({width},)")
            if prev is None:
                feature = layer
            else:
                hidden[len(linears) - 1] = (where, layer)
            prev = "norm"
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
    act = acts[0][1] if acts else None
    if not layer_norm:
        return dims, act, linears
    if hidden and len(hidden) != len(acts):
        bare = next(w for i, (w, _) in enumerate(acts) if i not in hidden)
        raise ValueError(f"{bare}: no LayerNorm behind this hidden activation, but one behind {next(iter(hidden.values()))[0]}; the engine's hidden "
                         f"norm is on every hidden layer or on none")
    return dims, act, linears, {"feature": feature, "hidden": [hidden[i][1] for i in sorted(hidden)]}
