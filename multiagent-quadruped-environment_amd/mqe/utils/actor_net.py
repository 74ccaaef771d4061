"""torch modules -> the engine's actor (mqe_actor_create): which torch.nn.Sequential stacks k_actor can evaluate, and their shapes; RecurrentMLP,
the torch twin of a network with the engine's GRU cell (k_actor_gru), and what of it the engine accepts; MATNet, the torch twin of the engine's
Multi-Agent Transformer policy (k_actor_mat), and mat_spec, what of it the engine accepts."""
import math

import torch

LN_EPS = 1e-5          # the only eps the engine's norm has (csrc/kernels_ln.hpp LN_EPS)


class RecurrentMLP(torch.nn.Module):
    """The torch twin of one network of the engine's recurrent actor-critic (abi.ACTOR_RECURRENT; csrc/kernels_gru.hpp), OpenRL's MLP base +
    RNNLayer + head: `base`, a Sequential in the form mlp_spec accepts minus the output layer (it ends in a hidden activation, or in that
    activation's LayerNorm); `rnn`, torch.nn.GRU(H, H, num_layers=1); `norm`, LayerNorm(H) or None (with the hidden norm); `head`, Linear(H, out).
    parameters() come in the engine's order.  Works in float32 and, after .double(), as the float64 reference."""

    def __init__(self, base, out_dim, norm=None):
        super().__init__()
        nn = torch.nn
        widths = [m.out_features for m in base if isinstance(m, nn.Linear)] if isinstance(base, nn.Sequential) else []
        if not widths:
            raise ValueError("RecurrentMLP: base must be a torch.nn.Sequential with at least one Linear layer")
        H = widths[-1]
        self.base = base
        self.rnn = nn.GRU(H, H, num_layers=1)
        if norm is None:                       # as the base: with the hidden norm it ends in a LayerNorm
            norm = isinstance(list(base)[-1], nn.LayerNorm)
        self.norm = nn.LayerNorm(H, eps=LN_EPS) if norm is True else None if norm is False else norm
        self.head = nn.Linear(H, int(out_dim))

    def forward(self, obs, h, mask):
        """one step: obs (..., D), h (..., H), mask (..., 1) or (...) = 1 - done of the step before -> (out (..., out_dim), h_next (..., H));
        the cell starts from h * mask, and h_next is not masked"""
        mask = mask.to(h.dtype)
        if mask.dim() == h.dim() - 1:
            mask = mask.unsqueeze(-1)
        x = self.base(obs)
        H = h.shape[-1]
        y, _ = self.rnn(x.reshape(1, -1, H), (h * mask).reshape(1, -1, H).contiguous())
        h_next = y.reshape(h.shape)
        return self.head(self.norm(h_next) if self.norm is not None else h_next), h_next

    def evaluate(self, obs_seq, h0, masks):
        """a chunk: obs_seq (L, ..., D), h0 (..., H), masks (L, ..., 1) or (L, ...) -> (outs (L, ..., out_dim), the state behind the chunk);
        back-propagation through time runs through the L steps"""
        outs, h = [], h0
        for t in range(obs_seq.shape[0]):
            o, h = self.forward(obs_seq[t], h, masks[t])
            outs.append(o)
        return torch.stack(outs), h


class _MATAttention(torch.nn.Module):
    """one head of MAT's SelfAttention: key, query, value, proj (Linear E -> E each); masked: row i attends to rows j <= i"""

    def __init__(self, E):
        super().__init__()
        nn = torch.nn
        self.key, self.query, self.value, self.proj = nn.Linear(E, E), nn.Linear(E, E), nn.Linear(E, E), nn.Linear(E, E)

    def forward(self, key, value, query, masked):
        k, v, q = self.key(key), self.value(value), self.query(query)
        s = q @ k.transpose(-1, -2) * (1.0 / math.sqrt(k.shape[-1]))
        if masked:
            n = s.shape[-1]
            s = s.masked_fill(~torch.tril(torch.ones(n, n, dtype=torch.bool, device=s.device)), float("-inf"))
        return self.proj(torch.softmax(s, dim=-1) @ v)


class _MATEncoder(torch.nn.Module):
    def __init__(self, D, E):
        super().__init__()
        nn = torch.nn
        ln = lambda n: nn.LayerNorm(n, eps=LN_EPS)
        self.obs_norm, self.obs_fc, self.ln = ln(D), nn.Linear(D, E), ln(E)
        self.attn, self.ln1 = _MATAttention(E), ln(E)
        self.mlp0, self.mlp1, self.ln2 = nn.Linear(E, E), nn.Linear(E, E), ln(E)
        self.head0, self.head_ln = nn.Linear(E, E), ln(E)


class _MATDecoder(torch.nn.Module):
    def __init__(self, E):
        super().__init__()
        nn = torch.nn
        ln = lambda n: nn.LayerNorm(n, eps=LN_EPS)
        self.act_fc, self.ln = nn.Linear(3, E), ln(E)
        self.attn1, self.ln1 = _MATAttention(E), ln(E)
        self.attn2, self.ln2 = _MATAttention(E), ln(E)
        self.mlp0, self.mlp1, self.ln3 = nn.Linear(E, E), nn.Linear(E, E), ln(E)
        self.head0, self.head_ln = nn.Linear(E, E), ln(E)


class MATNet(torch.nn.Module):
    """The torch twin of the engine's Multi-Agent Transformer policy (abi.ACTOR_TRANSFORMER; csrc/kernels_mat.hpp states the network): MAT as
    published for continuous actions at n_block = 1, n_head = 1, dec_actor = False -- an encoder that attends over the A' agents of an env and
    carries the value head, a decoder that emits the agents' actions one after the other, each conditioned on the sampled actions before it, and
    sigma = 0.5 * sigmoid(log_std).  obs is (..., A', D): the second-last dimension is the agents of ONE env.  parameters() come in the engine's
    order: enc.*, dec.*, value_out, mean_out (the two narrow output layers behind everything else), log_std.  Works in float32 and, after
    .double(), as the float64 reference."""
    n_block, n_head = 1, 1

    def __init__(self, obs_dim, n_embd=64):
        super().__init__()
        nn = torch.nn
        self.obs_dim, self.n_embd = int(obs_dim), int(n_embd)
        self.enc, self.dec = _MATEncoder(self.obs_dim, self.n_embd), _MATDecoder(self.n_embd)
        self.value_out, self.mean_out = nn.Linear(self.n_embd, 1), nn.Linear(self.n_embd, 3)
        self.log_std = nn.Parameter(torch.zeros(3))

    def named_parameters(self, prefix="", recurse=True, remove_duplicate=True):
        """torch lists a module's own parameters in front of its children's; log_std goes behind them, where the engine has it (parameters() follows)"""
        own = prefix + ("." if prefix else "") + "log_std"
        last = []
        for name, p in super().named_parameters(prefix=prefix, recurse=recurse, remove_duplicate=remove_duplicate):
            if name == own:
                last.append((name, p))
            else:
                yield name, p
        yield from last

    def encode(self, obs):
        """obs (..., A', D) -> (rep (..., A', E), value (..., A'))"""
        e, gelu = self.enc, torch.nn.functional.gelu
        x = e.ln(gelu(e.obs_fc(e.obs_norm(obs))))
        x = e.ln1(x + e.attn(x, x, x, False))
        rep = e.ln2(x + e.mlp1(gelu(e.mlp0(x))))
        return rep, self.value_out(e.head_ln(gelu(e.head0(rep))))[..., 0]

    def decode(self, s, rep):
        """s (..., A', 3): row a holds the raw action of agent a - 1 (row 0: zeros); -> the means (..., A', 3).  Row a depends on rows <= a of s"""
        d, gelu = self.dec, torch.nn.functional.gelu
        x = d.ln(gelu(d.act_fc(s)))
        x = d.ln1(x + d.attn1(x, x, x, True))
        x = d.ln2(rep + d.attn2(x, x, rep, True))
        x = d.ln3(x + d.mlp1(gelu(d.mlp0(x))))
        return self.mean_out(d.head_ln(gelu(d.head0(x))))

    def sigma(self):
        return 0.5 * torch.sigmoid(self.log_std)

    def logp_of(self, z):
        return (-0.5 * z * z - torch.log(self.sigma())).sum(-1) - 1.5 * math.log(2.0 * math.pi)

    def act(self, obs, z=None, deterministic=False):
        """the autoregressive loop: agent a's mean from the actions of agents 0 .. a - 1 AS SAMPLED; z (..., A', 3): the N(0, 1) draws to use (None:
        torch.randn); deterministic: a = mean, logp at z = 0.  -> (actions (..., A', 3) raw, logp (..., A'), value (..., A'))"""
        rep, value = self.encode(obs)
        A = obs.shape[-2]
        if deterministic:
            z = torch.zeros(*obs.shape[:-1], 3, dtype=obs.dtype, device=obs.device)
        elif z is None:
            z = torch.randn(*obs.shape[:-1], 3, dtype=obs.dtype, device=obs.device)
        sigma = self.sigma()
        s = torch.zeros(*obs.shape[:-1], 3, dtype=obs.dtype, device=obs.device)
        acts = []
        for a in range(A):
            acts.append(self.decode(s, rep)[..., a, :] + sigma * z[..., a, :])
            if a + 1 < A:
                s = torch.cat([s[..., :a + 1, :], acts[-1].unsqueeze(-2), s[..., a + 2:, :]], dim=-2)
        return torch.stack(acts, dim=-2), self.logp_of(z), value

    def evaluate(self, obs, actions):
        """what a learner differentiates: ONE parallel decoder pass with s_a = actions[a - 1]; through the causal mask the same function as act.
        -> (mean (..., A', 3), logp of `actions` (..., A'), value (..., A'))"""
        rep, value = self.encode(obs)
        s = torch.cat([torch.zeros_like(actions[..., :1, :]), actions[..., :-1, :]], dim=-2)
        mean = self.decode(s, rep)
        return mean, self.logp_of((actions - mean) / self.sigma()), value


def mat_spec(module, in_dim):
    """(D, E) of a MATNet for the engine, after holding every layer to what k_actor_mat evaluates: LayerNorm(n, eps=1e-5) with weight and bias,
    Linear with a bias, the widths that follow from (D, E), one head, one block.  Refusals name the layer."""
    nn = torch.nn
    if not isinstance(module, MATNet):
        raise ValueError(f"mat: expected a mqe.utils.actor_net.MATNet, got {type(module).__name__}")
    if int(getattr(module, "n_head", 1)) != 1:
        raise ValueError(f"mat.n_head = {module.n_head}: the engine's attention has one head (n_head = 1)")
    if int(getattr(module, "n_block", 1)) != 1:
        raise ValueError(f"mat.n_block = {module.n_block}: the engine evaluates one encoder block and one decoder block (n_block = 1)")
    D, E = int(in_dim), int(module.n_embd)
    attn = lambda at: [(f"{at}.{n}", "lin", E, E) for n in ("key", "query", "value", "proj")]
    want = ([("enc.obs_norm", "ln", D), ("enc.obs_fc", "lin", D, E), ("enc.ln", "ln", E)] + attn("enc.attn") +
            [("enc.ln1", "ln", E), ("enc.mlp0", "lin", E, E), ("enc.mlp1", "lin", E, E), ("enc.ln2", "ln", E), ("enc.head0", "lin", E, E), ("enc.head_ln", "ln", E),
             ("dec.act_fc", "lin", 3, E), ("dec.ln", "ln", E)] + attn("dec.attn1") + [("dec.ln1", "ln", E)] + attn("dec.attn2") +
            [("dec.ln2", "ln", E), ("dec.mlp0", "lin", E, E), ("dec.mlp1", "lin", E, E), ("dec.ln3", "ln", E), ("dec.head0", "lin", E, E), ("dec.head_ln", "ln", E),
             ("value_out", "lin", E, 1), ("mean_out", "lin", E, 3)])
    for name, kind, *shape in want:
        layer = module.get_submodule(name)
        where = f"mat.{name} ({type(layer).__name__})"
        if kind == "ln":
            if not isinstance(layer, nn.LayerNorm):
                raise ValueError(f"{where}: expected LayerNorm({shape[0]}, eps=1e-5)")
            if not layer.elementwise_affine or layer.weight is None or layer.bias is None:
                raise ValueError(f"{where}: elementwise_affine=False (or no bias); the engine's norm has a weight and a bias")
            if float(layer.eps) != LN_EPS:
                raise ValueError(f"{where}: eps {layer.eps!r}; the engine's norm has eps = 1e-5 only")
            if tuple(layer.normalized_shape) != (shape[0],):
                raise ValueError(f"{where}: normalized_shape {tuple(layer.normalized_shape)} is not ({shape[0]},)")
        else:
            if not isinstance(layer, nn.Linear):
                raise ValueError(f"{where}: expected Linear({shape[0]}, {shape[1]})")
            if layer.bias is None:
                raise ValueError(f"{where}: Linear without a bias")
            if (layer.in_features, layer.out_features) != tuple(shape):
                raise ValueError(f"{where}: Linear({layer.in_features}, {layer.out_features}) where the network has Linear({shape[0]}, {shape[1]})")
    if not isinstance(module.log_std, torch.nn.Parameter) or module.log_std.numel() != 3:
        raise ValueError("mat.log_std: expected a Parameter of 3 values (one per action column)")
    return D, E


def recurrent_spec(module, what, in_dim, out_dim, layer_norm=False):
    """(dims, activation, linears, norms, module) of a RecurrentMLP for the engine: base through mlp_spec (with a stand-in output layer), then the
    cell, its norm and the head against the base.  dims = [in_dim, hidden ..., out_dim]; `linears` ends with the head.  Refusals name the layer."""
    nn = torch.nn
    if not isinstance(module, RecurrentMLP):
        raise ValueError(f"{what}: recurrent=True takes mqe.utils.actor_net.RecurrentMLP networks, got {type(module).__name__}")
    base = module.base
    if not isinstance(base, nn.Sequential) or len(base) == 0:
        raise ValueError(f"{what}.base: expected a torch.nn.Sequential of Linear / Tanh / ReLU that ends in a hidden activation")
    last_name, last = list(base.named_children())[-1]
    if isinstance(last, nn.Linear):
        raise ValueError(f"{what}.base[{last_name}] (Linear): the base ends in a Linear layer; the GRU cell reads a hidden ACTIVATION (the output layer is `head`)")
    H = next(m.out_features for m in reversed(list(base)) if isinstance(m, nn.Linear)) if any(isinstance(m, nn.Linear) for m in base) else 0
    stand_in = nn.Sequential(*base, nn.Linear(max(H, 1), out_dim))          # names 0 .. n - 1 as in base: the refusals of mlp_spec name its layers
    spec = mlp_spec(stand_in, f"{what}.base", in_dim, out_dim, layer_norm=layer_norm)
    dims, act, linears = spec[:3]
    norms = spec[3] if layer_norm else {"feature": None, "hidden": []}
    rnn = module.rnn
    if not isinstance(rnn, nn.GRU):
        raise ValueError(f"{what}.rnn ({type(rnn).__name__}): the engine's cell is torch.nn.GRU")
    if (rnn.input_size, rnn.hidden_size, rnn.num_layers, rnn.bias, rnn.bidirectional) != (H, H, 1, True, False) or getattr(rnn, "proj_size", 0):
        raise ValueError(f"{what}.rnn (GRU): expected GRU({H}, {H}, num_layers=1) with biases, one direction; got GRU({rnn.input_size}, {rnn.hidden_size}, "
                         f"num_layers={rnn.num_layers}, bias={rnn.bias}, bidirectional={rnn.bidirectional})")
    norm = module.norm
    if norm is not None:
        if not layer_norm:
            raise ValueError(f"{what}.norm (LayerNorm): only Linear, Tanh and ReLU layers can run inside the engine (set_actor(layer_norm=True) admits the norms)")
        if not isinstance(norm, nn.LayerNorm) or tuple(norm.normalized_shape) != (H,) or float(norm.eps) != LN_EPS or not norm.elementwise_affine or norm.bias is None:
            raise ValueError(f"{what}.norm ({type(norm).__name__}): expected LayerNorm({H}, eps=1e-5) with a weight and a bias")
    if (norm is not None) != bool(norms["hidden"]):
        raise ValueError(f"{what}.norm: the LayerNorm behind the GRU cell goes with the hidden norm (a LayerNorm behind every hidden activation of base): both or neither")
    head = module.head
    if not isinstance(head, nn.Linear) or head.bias is None or head.in_features != H:
        raise ValueError(f"{what}.head ({type(head).__name__}): expected Linear({H}, {out_dim}) with a bias")
    if head.out_features != out_dim:
        raise ValueError(f"{what}.head (Linear): the last Linear gives {head.out_features} outputs, {out_dim} wanted")
    return dims, act, linears[:-1] + [head], norms, module


def actor_tensors(who, linears=(), norms=None, rnn=None, mat=None):
    """[(the engine's name, the torch tensor)] of one network, "actor" or "critic", from what mlp_spec / recurrent_spec found for it (its Linear
    layers, its norms, its RecurrentMLP or None): the names and the order of abi.actor_param_layout, which is the module's own parameters() order.
    mat (a MATNet that mat_spec accepted; who = "mat"): every tensor of the transformer but log_std, as mat.<the module's own parameter name>."""
    if mat is not None:
        return [(f"{who}.{name}", p) for name, p in mat.named_parameters() if name != "log_std"]
    def both(name, m):
        return [(f"{who}.{name}weight", m.weight), (f"{who}.{name}bias", m.bias)]
    out = both("norm_in.", norms["feature"]) if norms["feature"] is not None else []
    for l, layer in enumerate(linears):
        if rnn is not None and l + 1 == len(linears):          # the cell's block in front of the output layer
            out += [(f"{who}.gru.{name}", getattr(rnn.rnn, name + "_l0")) for name in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
            if rnn.norm is not None:
                out += both("gru.norm.", rnn.norm)
        out += both(f"{l}.", layer)
        if l < len(norms["hidden"]):
            out += both(f"{l}.norm.", norms["hidden"][l])
    return out


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
