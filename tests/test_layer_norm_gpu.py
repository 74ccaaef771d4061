"""-m gpu: layer normalisation in the engine's actor-critic (MQE_ACTOR_LAYER_NORM, MQE_ACTOR_FEATURE_NORM; csrc/kernels_ln.hpp: k_actor_ln,
k_ln_grad) on go1gate (D = 16, A' = 2) at N = 33 -- 66 rows: a second workgroup of k_actor_ln with two live rows, so clamped loads and masked
stores run.  The four networks of layer_norm_ref.CASES: 16 -> 7 -> 3 with 16 -> 17 -> 1 (tanh, hidden norm: unaligned weight rows, short last
blocks), two 16 -> 64 -> 64 (relu, both switches: 16-byte loads), two 16 -> 256 -> 256 -> 256 (tanh, both: the widest norm, 32-row tiles), a
single Linear per network with the feature norm alone.  The reference is the float64 twin of tests/layer_norm_ref.py, which
tests/test_layer_norm.py holds to torch; the bounds are that file's (forward: 4x torch's float32 CPU error; gradient: K_LN_GPU 2^-24 S_n)."""
import copy
import ctypes as C
import math

import numpy as np
import pytest
import torch

import layer_norm_ref as ref
import ppo_ref
import rollout_ref
from helpers import make_desc, hip_engine
from mqe.engine import abi
from test_rollout_gpu import same_bits, engine, sampling_tolerances, _gate_env, gate_cfg_restored  # noqa: F401
from test_ppo_gpu import upload, call, outputs

pytestmark = pytest.mark.gpu

EPS32 = ppo_ref.EPS32
TASK, N, D, AW, T = "go1gate", 33, 16, 2, 2
CFG = dict(clip=ref.CLIP, value_coef=0.7, entropy_coef=0.01, value_clip=ref.VALUE_CLIP)
_HANDLE, _SYNTH, _REF = [], {}, {}


def handle():
    if not _HANDLE:
        d, k, _ = make_desc(TASK, N)
        _HANDLE.append(hip_engine(d, k))
    return _HANDLE[0]


def synth(case):
    """the shared synthetic trajectory of a case: T = 2 steps of 66 rows = 132 samples (host side: made once, never changed)"""
    if case not in _SYNTH:
        _SYNTH[case] = ref.synth(case, (N, AW, T, D), N * AW * T, seed=40 + len(case))
    return _SYNTH[case]


def install(eng, s, **kw):
    eng.create_actor(s["a_dims"], s["c_dims"], activation=s["act"], layer_norm=s["hidden"], feature_norm=s["feat"], **kw)
    views = eng.actor_params()
    assert views["flat"].numel() == s["n_params"]
    for n, v in s["params"].items():
        views[n].copy_(v)
    return views


def reference(s, sel, key):
    """float64 gradient (flat), statistics and their bounds K_LN_GPU 2^-24 S_n / scale of a minibatch"""
    if key not in _REF:
        args, norms = ref.args_of(s, sel, CFG)
        g64, st64, S, ss = ppo_ref.manual(*args, **norms)
        flat = lambda g: ppo_ref.flat_grad(g, s["a_dims"], s["c_dims"], **norms)
        bound = flat({n: torch.full_like(g64[n], S[n]) for n in g64}) * (ref.K_LN_GPU * EPS32)
        _REF[key] = (flat(g64), st64, bound, ss * (ref.K_LN_GPU * EPS32))
    return _REF[key]


# ---- 1. the forward pass --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(ref.CASES))
def test_rollouts_against_the_float64_twin(case):
    """A sampled and a deterministic rollout(T = 2) of a fresh handle.  Means and values: at most 4x the deviation of torch's float32 CPU
    evaluation from the float64 twin on the same observations.  The sampled actions and log-probabilities: the counter RNG's draws within
    test_rollout_gpu.sampling_tolerances, which are derived from that 4x yardstick; the deterministic log-probability is a constant."""
    s = synth(case)
    seed = 7
    eng = engine(TASK, N, seed=seed)
    install(eng, s)
    eng.reset_all()
    p = s["params"]
    ls = p["log_std"].double()
    std = torch.exp(ls)
    sampled = eng.rollout(T)
    det = eng.rollout(T, deterministic=True)
    torch.cuda.synchronize()
    for name, traj in (("sampled", sampled), ("deterministic", det)):
        obs = traj.obs.cpu()
        assert obs.shape == (T + 1, N, AW, D) and bool(torch.isfinite(obs).all())
        e = ref.forward_errors(p, s["a_dims"], s["c_dims"], s["act"], s["hidden"], s["feat"], obs)
        dev_value = float((traj.value.cpu().double() - e["value64"]).abs().max())
        a = traj.actions.cpu().double()
        if name == "deterministic":
            dev_mean = float((a - e["mean64"][:T]).abs().max())
            want = -float(ls.sum()) - 1.5 * math.log(2 * math.pi)
            assert float((traj.logp.cpu().double() - want).abs().max()) <= 4 * 8 * EPS32
        else:
            twin = rollout_ref.actor_draws(seed, 0, N, AW, 0, T)
            tol_z, tol_lp = sampling_tolerances(e["yard_mean"], float(a.abs().max()), float(std.min()), float(np.abs(twin).max()))
            z = ((a - e["mean64"][:T]) / std).numpy()
            dev_mean = float(np.abs(z - twin).max()) * float(std.min())
            assert float(np.abs(z - twin).max()) <= tol_z, (name, float(np.abs(z - twin).max()), tol_z)
            dev_lp = float((traj.logp.cpu().double() - rollout_ref.gaussian_logp(a, e["mean64"][:T], ls)).abs().max())
            assert dev_lp <= tol_lp, (dev_lp, tol_lp)
        print(f"layer_norm_forward {case} {name}: mean {dev_mean:.3e} (torch-f32 {e['yard_mean']:.3e}) value {dev_value:.3e} (torch-f32 {e['yard_value']:.3e})")
        assert dev_value <= 4 * e["yard_value"], (name, dev_value, e["yard_value"])
        if name == "deterministic":
            assert dev_mean <= 4 * e["yard_mean"], (dev_mean, e["yard_mean"])
    assert not same_bits(sampled.actions, det.actions)
    eng.close()


# ---- 2. the gradient ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(ref.CASES))
def test_gradient_against_float64_and_same_bits(case):
    """mqe_ppo_grad at M = 1, 63, 130 and through a shuffled index slice with first > 0: every tensor, the norms' weights and biases included,
    within K_LN_GPU 2^-24 S_n of the float64 backward and exactly 0 where S_n = 0; the statistics likewise with their scales; the same call
    twice gives the same bits."""
    s = synth(case)
    eng = handle()
    install(eng, s)
    for M, first, use_index in ((1, 0, False), (63, 0, False), (130, 0, False), (100, 17, True)):
        t, u = upload(s, eng.torch_device), upload(s, eng.torch_device)
        assert call(eng, s, t, first, M, use_index, CFG) == 0, eng.lib.mqe_last_error().decode()
        assert call(eng, s, u, first, M, use_index, CFG) == 0
        torch.cuda.synchronize()
        assert torch.equal(t["grad"], u["grad"]) and torch.equal(t["stats"], u["stats"]), "two calls on the same inputs differ"
        n = s["n_params"]
        assert bool((t["grad"][n:] == ppo_ref.SENT).all()) and not bool((t["grad"][:n] == ppo_ref.SENT).any()), "guard touched or an element unwritten"
        sel = s["index"][first:first + M] if use_index else torch.arange(first, first + M)
        grad, stats = outputs(s, t)
        g64, st64, bound, sbound = reference(s, sel, (case, M, first, use_index))
        assert bool(torch.isfinite(grad).all()) and bool(torch.isfinite(stats).all())
        dev = (grad.double() - g64).abs()
        zero = bound == 0
        worst = float((dev[~zero] / bound[~zero]).max()) * ref.K_LN_GPU
        sworst = float(((stats.double() - st64).abs() / sbound).max()) * ref.K_LN_GPU
        names = [nm for nm, (off, shape) in ref.layout(s["a_dims"], s["c_dims"], s["hidden"], s["feat"]).items() if "norm" in nm]
        print(f"layer_norm_grad {case} M={M} index={use_index}: gradient {worst:.2f} x 2^-24 S (bound {ref.K_LN_GPU:.0f}), statistics {sworst:.2f}; "
              f"{len(names)} norm tensors")
        assert bool((grad[zero] == 0).all()), "a tensor without any contribution must be exactly 0"
        assert worst <= ref.K_LN_GPU and sworst <= ref.K_LN_GPU, (case, M, worst, sworst)


# ---- 3. Adam moves the norms' parameters --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(ref.CASES))
def test_one_ppo_update_step_moves_gamma_and_beta_as_adam_says(case):
    """ppo_update(epochs=1, minibatches=1) on a real trajectory: the gradient of the same permutation, taken before the step (the same bits),
    through ppo_ref.adam in float64 -- every parameter, gamma and beta among them, within ppo_ref.adam_tolerances"""
    s = synth(case)
    eng = handle()
    views = install(eng, s)
    eng.reset_all()
    traj = eng.gae(eng.rollout(T, time_outs=True), 0.99, 0.95)
    kw = dict(clip=0.2, value_coef=0.5, entropy_coef=0.01, value_clip=0.2)
    total = T * N * AW
    perm = torch.randperm(total, device=eng.torch_device, generator=torch.Generator(device="cuda").manual_seed(5)).to(torch.int32)
    grad, _ = eng.ppo_grad(traj, index=perm, **kw)
    p0 = views["flat"].clone()
    eng.ppo_update(traj, epochs=1, minibatches=1, lr=1e-2, max_grad_norm=0.5, generator=torch.Generator(device="cuda").manual_seed(5), **kw)
    torch.cuda.synchronize()
    assert eng.ppo_step == 1
    p0, g, p1 = p0.cpu(), grad.cpu(), views["flat"].cpu()
    zeros = torch.zeros_like(p0)
    p64 = ppo_ref.adam(p0, zeros, zeros, g, 1, 1e-2, max_norm=0.5)[0]
    tol_p = ppo_ref.adam_tolerances(p0, zeros, zeros, g, 1, 1e-2, max_norm=0.5)[0]
    worst = float(((p1.double() - p64).abs() / tol_p).max())
    moved = 0
    for name, (off, shape) in ref.layout(s["a_dims"], s["c_dims"], s["hidden"], s["feat"]).items():
        if "norm" in name:
            sl = slice(off, off + int(np.prod(shape)))
            assert bool((g[sl] != 0).any()) and not torch.equal(p1[sl], p0[sl]), f"{name} did not move"
            moved += 1
    print(f"layer_norm_adam {case}: parameters at {worst:.3f} of the Adam bound; {moved} norm tensors moved")
    assert worst <= 1.0 and moved > 0


# ---- 4. the public surface ----------------------------------------------------------------------------------------------------------------------
def test_set_actor_round_trip_with_value_norm(gate_cfg_restored):  # noqa: F811
    """set_actor(layer_norm=True, value_norm=True) -> rollout -> ppo_update -> pull_actor: the engine evaluated the torch modules (float64 torch
    on the stored observations, 4x the float32 yardstick), and afterwards the modules hold the buffer's values bit for bit"""
    nn = torch.nn
    torch.manual_seed(4)
    mk = lambda out: nn.Sequential(nn.LayerNorm(16), nn.Linear(16, 32), nn.Tanh(), nn.LayerNorm(32), nn.Linear(32, 24), nn.Tanh(), nn.LayerNorm(24),
                                   nn.Linear(24, out)).cuda()
    actor, critic, log_std = mk(3), mk(1), torch.tensor([-0.7, -0.2, 0.1])
    with torch.no_grad():
        for m in list(actor) + list(critic):
            if isinstance(m, nn.LayerNorm):
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.5, 0.5)
    twin = copy.deepcopy(actor).cpu()
    env = _gate_env(N)
    env.set_actor(actor, critic, log_std=log_std, value_norm=True, layer_norm=True)
    env.reset()
    eng = env.env.engine
    assert eng._actor["layer_norm"] and eng._actor["feature_norm"] and eng._actor["value_norm"]
    views = eng.actor_params()
    assert same_bits(views["actor.norm_in.weight"], actor[0].weight.detach()) and same_bits(views["critic.1.norm.bias"], critic[6].bias.detach())
    traj = env.rollout(4, deterministic=True, gamma=0.99)
    torch.cuda.synchronize()
    with torch.no_grad():
        obs = traj.obs[:4].cpu()
        a64, a32 = twin.double()(obs.double()), twin.float()(obs)
    yard = float((a32.double() - a64).abs().max())
    dev = float((traj.actions.cpu().double() - a64).abs().max())
    print(f"layer_norm_surface: mean {dev:.3e} (torch-f32 {yard:.3e})")
    assert dev <= 4 * yard
    before = views["flat"].clone()
    st = env.ppo_update(traj, epochs=1, minibatches=2, lr=1e-3, value_clip=0.2, entropy_coef=0.01, max_grad_norm=1.0)
    env.pull_actor()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(st).all()) and not same_bits(before, views["flat"])
    for who, mod in (("actor", actor), ("critic", critic)):
        assert same_bits(mod[0].weight.detach(), views[f"{who}.norm_in.weight"]) and same_bits(mod[0].bias.detach(), views[f"{who}.norm_in.bias"])
        for l, (lin, norm) in enumerate(((1, 3), (4, 6), (7, None))):
            assert same_bits(mod[lin].weight.detach(), views[f"{who}.{l}.weight"]) and same_bits(mod[lin].bias.detach(), views[f"{who}.{l}.bias"])
            if norm is not None:
                assert same_bits(mod[norm].weight.detach(), views[f"{who}.{l}.norm.weight"]) and same_bits(mod[norm].bias.detach(), views[f"{who}.{l}.norm.bias"])
    assert float(views["value_norm"][2]) > 0.0, "the value-normalisation state was updated"
    env.close()


def test_kind_bits_of_mqe_actor_create():
    """bits 2 and 4 of the kind byte are the two switches, alone and together with the kind and MQE_ACTOR_VALUE_NORM; every gamma starts at 1 and
    the rest of the buffer at 0; bit 512 is still refused"""
    eng = handle()

    def create(activation):
        sh = abi.ActorShape()
        sh.obs_dim, sh.act_dim, sh.actor_layers, sh.critic_layers = D, 3, 2, 2
        for i, v in enumerate((D, 8, 3)):
            sh.actor_dims[i] = v
        for i, v in enumerate((D, 5, 1)):
            sh.critic_dims[i] = v
        sh.activation, sh.action_gain = activation, 1.0
        return eng.lib.mqe_actor_create(eng.h, C.byref(sh))
    for bits, hidden, feat in ((2, True, False), (4, False, True), (6, True, True), (abi.ACTOR_RELU | 6 | abi.ACTOR_VALUE_NORM, True, True)):
        assert (abi.ACTOR_LAYER_NORM, abi.ACTOR_FEATURE_NORM) == (2, 4)
        assert create(bits) == 0, eng.lib.mqe_last_error().decode()
        v = abi.TensorView()
        assert eng.lib.mqe_actor_params(eng.h, C.byref(v)) == 0
        lay = abi.actor_param_layout([D, 8, 3], [D, 5, 1], bool(bits & abi.ACTOR_VALUE_NORM), hidden, feat)
        n = abi.actor_param_count([D, 8, 3], [D, 5, 1], bool(bits & abi.ACTOR_VALUE_NORM), hidden, feat)
        assert int(v.shape[0]) == n
        flat = eng._wrap(v.ptr, [n], v.dtype).cpu()
        for name, (off, shape) in lay.items():
            want = 1.0 if name.endswith("norm.weight") or name.endswith("norm_in.weight") else 0.0
            if name != "value_norm":
                assert bool((flat[off:off + int(np.prod(shape))] == want).all()), name
    assert create(512) == -6 and create(abi.ACTOR_TANH | 8) == -6
    eng._actor = eng._actor_views = None
