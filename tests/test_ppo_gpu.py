"""-m gpu: the on-device PPO update (mqe_ppo_grad, mqe_ppo_optimizer, mqe_ppo_adam; csrc/kernels_ppo.hpp; HipEngine.ppo_grad / adam_step /
ppo_update, FusedTaskWrapper.ppo_update / pull_actor): (1) gradient and statistics against float64 within K_GPU 2^-24 S_n; (2) determinism,
index list == contiguous range; (3) every element written, nothing beyond, inputs untouched; (4) shards; (5) Adam; (6) every refusal;
(7) the public surface."""
import ctypes as C

import numpy as np
import pytest
import torch

import ppo_ref as ref
from helpers import make_desc, hip_engine
from mqe.engine import abi
from test_rollout_gpu import same_bits, _gate_env, _modules, gate_cfg_restored  # noqa: F401

pytestmark = pytest.mark.gpu

EPS32 = ref.EPS32
TASKS = {"go1gate": 16, "go1sheep-hard": 34, "go1seesaw": 14}
_HANDLES, _SYNTH, _REF = {}, {}, {}
CFG = dict(clip=ref.CLIP, value_coef=0.7, entropy_coef=0.01, value_clip=ref.VALUE_CLIP)


def handle(task, N):
    if (task, N) not in _HANDLES:
        d, k, _ = make_desc(task, N)
        _HANDLES[(task, N)] = hip_engine(d, k)
    return _HANDLES[(task, N)]


def synth(net, task, N, T):
    """the shared synthetic trajectory of (net, task, N, T) (host side: made once, never changed)"""
    key = (net, task, N, T)
    if key not in _SYNTH:
        _SYNTH[key] = ref.synth(net, (N, 2, T, TASKS[task]), N * 2 * T, seed=100 + 7 * N + T + len(net))
    return _SYNTH[key]


def install(eng, s):
    """the engine's actor with the trajectory's network and parameters (a new actor: scratch and moments of the old one are dropped)"""
    eng.create_actor(s["a_dims"], s["c_dims"], activation=s["act"])
    views = eng.actor_params()
    for n, v in s["params"].items():
        views[n].copy_(v)
    assert tuple(eng.tensor(abi.T_WRAPPER_OBS).shape) == (s["N"], s["Aw"], s["D"])
    return views


def upload(s, dev):
    """fresh device images: packed / value / grad / stats carry sentinels and guards; the others are the logical tensors"""
    t = {k: torch.from_numpy(s[k].copy()).to(dev) for k in ("packed", "value", "grad", "stats")}
    t.update({k: s[k].to(dev).contiguous() for k in ("actions", "logp_old", "adv", "ret", "index")})
    return t


def call(eng, s, t, first, count, use_index, cfg=CFG, want_stats=True, **kw):
    loss = abi.PpoLoss(cfg["clip"], cfg["value_coef"], cfg["entropy_coef"], cfg["value_clip"] if cfg["value_clip"] is not None else 0.0)
    a = dict(h=eng.h, T=s["T"], packed=t["packed"].data_ptr(), stride=s["stride"], actions=t["actions"].data_ptr(), logp=t["logp_old"].data_ptr(),
             value=t["value"].data_ptr(), adv=t["adv"].data_ptr(), ret=t["ret"].data_ptr(), index=t["index"].data_ptr() if use_index else None,
             first=first, count=count, loss=C.byref(loss), flags=abi.PPO_CLIP_VALUE if cfg["value_clip"] is not None else 0,
             grad=t["grad"].data_ptr(), stats=t["stats"].data_ptr() if want_stats else None)
    a.update(kw)
    return eng.lib.mqe_ppo_grad(a["h"], a["T"], a["packed"], a["stride"], a["actions"], a["logp"], a["value"], a["adv"], a["ret"], a["index"], a["first"],
                         a["count"], a["loss"], a["flags"], a["grad"], a["stats"], eng._stream())


def outputs(s, t):
    return t["grad"][:s["n_params"]].view(torch.float32).cpu(), t["stats"][:6].view(torch.float32).cpu()


def reference(s, sel, cfg, key=None):
    """float64 gradient (flat), statistics, the per-entry bound K_GPU 2^-24 S_n (flat) and the statistics' bound of a minibatch"""
    if key is not None and key in _REF:
        return _REF[key]
    g64, st64, S, ss = ref.manual(s["params"], s["a_dims"], s["c_dims"], s["act"], ref.batch(s, sel), cfg)
    bound = ref.flat_grad({n: torch.full_like(g64[n], S[n]) for n in g64}, s["a_dims"], s["c_dims"]) * (ref.K_GPU * EPS32)
    out = (ref.flat_grad(g64, s["a_dims"], s["c_dims"]), st64, bound, ss * (ref.K_GPU * EPS32))
    if key is not None:
        _REF[key] = out
    return out


def check(s, t, sel, cfg, what):
    grad, stats = outputs(s, t)
    g64, st64, bound, sbound = reference(s, sel, cfg)
    assert bool(torch.isfinite(grad).all()) and bool(torch.isfinite(stats).all()), what
    dev = (grad.double() - g64).abs()
    zero = bound == 0
    worst = float((dev[~zero] / bound[~zero]).max()) * ref.K_GPU
    sworst = float(((stats.double() - st64).abs() / sbound).max()) * ref.K_GPU
    print(f"ppo_kernel {what}: gradient {worst:.2f} x 2^-24 S (bound {ref.K_GPU:.0f}), statistics {sworst:.2f} x 2^-24 scale")
    assert bool((grad[zero] == 0).all()), f"{what}: a tensor without any contribution must be exactly 0"
    assert worst <= ref.K_GPU and sworst <= ref.K_GPU, what


# ---- 1. gradient and statistics against float64 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("task,N", [("go1gate", 5), ("go1sheep-hard", 5), ("go1seesaw", 3)])
@pytest.mark.parametrize("net", ["tanh64x64", "tanh7", "relu128x3", "tanh256x3"])
def test_gradient_and_statistics_against_float64(net, task, N):
    """|g - g64| <= K_GPU 2^-24 S_n per tensor, statistics likewise with their scales (tests/ppo_ref.py: K_GPU = 4 K_CPU, K_CPU measured on two
    float32 CPU evaluations).  M = 1, 63, 64, 65 are the edges of a 64-row tile (two tiles of the 32-row kernel that tanh256x3, the widest
    accepted stack, takes); 130 goes through a shuffled index slice with first > 0; value clipping on and off.  go1seesaw's D = 14 leaves
    the first layer's weight rows unaligned (dword loads); go1sheep-hard is D = 34."""
    T = 24 if N == 5 else 40                 # 240 samples either way
    s = synth(net, task, N, T)
    eng = handle(task, N)
    install(eng, s)
    for vclip in (ref.VALUE_CLIP, None):
        cfg = dict(CFG, value_clip=vclip)
        for M, first, use_index in ((1, 0, False), (63, 0, False), (64, 5, False), (65, 0, False), (130, 17, True)):
            t = upload(s, eng.torch_device)
            rc = call(eng, s, t, first, M, use_index, cfg)
            torch.cuda.synchronize()
            assert rc == 0, eng.lib.mqe_last_error().decode()
            sel = s["index"][first:first + M] if use_index else torch.arange(first, first + M)
            check(s, t, sel, cfg, f"{net} {task} M={M} vclip={vclip}")


@pytest.mark.parametrize("net", ["tanh64x64", "relu128x3", "tanh256x3"])
def test_more_tiles_than_workgroups(net):
    """19 800 contiguous samples (N = 33, T = 300): 310 tiles of 64 rows (619 of 32) for at most 256 workgroups, so the persistent loop runs and
    a workgroup's partial gradient continues its chains through scratch"""
    s = synth(net, "go1gate", 33, 300)
    eng = handle("go1gate", 33)
    install(eng, s)
    t = upload(s, eng.torch_device)
    rc = call(eng, s, t, 0, s["n"], False)
    torch.cuda.synchronize()
    assert rc == 0 and s["n"] == 19800, eng.lib.mqe_last_error().decode()
    check(s, t, slice(None), CFG, f"{net} go1gate M=19800")


# ---- 2. determinism and equivalence ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net,N,T", [("tanh64x64", 33, 300), ("tanh256x3", 5, 24)])
def test_same_bits_and_index_equals_range(net, N, T):
    s = synth(net, "go1gate", N, T)
    eng = handle("go1gate", N)
    install(eng, s)
    first, count = 7, s["n"] - 11
    a, b, c = (upload(s, eng.torch_device) for _ in range(3))
    c["index"] = torch.arange(0, s["n"], dtype=torch.int32, device=eng.torch_device)
    assert call(eng, s, a, first, count, False) == 0 and call(eng, s, b, first, count, False) == 0 and call(eng, s, c, first, count, True) == 0
    torch.cuda.synchronize()
    for name in ("grad", "stats"):
        assert torch.equal(a[name], b[name]), f"{name}: two calls on the same inputs differ"
        assert torch.equal(a[name], c[name]), f"{name}: index = arange(first, first + count) differs from the contiguous call"
    d = upload(s, eng.torch_device)
    assert call(eng, s, d, first, count, True) == 0                  # the shuffled list: other samples in other tiles
    torch.cuda.synchronize()
    assert not torch.equal(a["grad"], d["grad"])


# ---- 3. memory discipline ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net,task,N", [("tanh64x64", "go1gate", 5), ("relu128x3", "go1seesaw", 3), ("tanh256x3", "go1sheep-hard", 5)])
def test_every_element_written_nothing_beyond(net, task, N):
    s = synth(net, task, N, 24)
    eng = handle(task, N)
    views = install(eng, s)
    opt = eng.optimizer_state()
    opt["exp_avg"].uniform_(-1, 1)
    opt["exp_avg_sq"].uniform_(0, 1)
    before = [views["flat"].clone(), opt["exp_avg"].clone(), opt["exp_avg_sq"].clone()]
    t = upload(s, eng.torch_device)
    image = {k: v.clone() for k, v in t.items()}
    assert call(eng, s, t, 3, 130, True) == 0, eng.lib.mqe_last_error().decode()
    torch.cuda.synchronize()
    n = s["n_params"]
    assert bool((t["grad"][n:] == ref.SENT).all()) and bool((t["stats"][6:] == ref.SENT).all()), "guard elements touched"
    assert not bool((t["grad"][:n] == ref.SENT).any()) and not bool((t["stats"][:6] == ref.SENT).any()), "an element was left unwritten"
    for k in ("packed", "value", "actions", "logp_old", "adv", "ret", "index"):
        assert torch.equal(t[k].view(torch.uint8), image[k].view(torch.uint8)), f"{k} changed"
    for was, now in zip(before, (views["flat"], opt["exp_avg"], opt["exp_avg_sq"])):
        assert same_bits(was, now), "parameters or moments changed"
    u = upload(s, eng.torch_device)
    assert call(eng, s, u, 3, 130, True, want_stats=False) == 0
    torch.cuda.synchronize()
    assert torch.equal(u["grad"], t["grad"]) and bool((u["stats"] == ref.SENT).all()), "stats_dev = NULL: the same gradient, nothing else"


# ---- 4. shards ---------------------------------------------------------------------------------------------------------------------------------
def test_row_weighted_mean_of_two_shards_is_the_whole_batch():
    s = synth("tanh64x64", "go1gate", 5, 24)
    eng = handle("go1gate", 5)
    install(eng, s)
    M, m1 = 200, 77
    parts = []
    for first, count in ((0, M), (0, m1), (m1, M - m1)):
        t = upload(s, eng.torch_device)
        assert call(eng, s, t, first, count, True) == 0
        torch.cuda.synchronize()
        parts.append((outputs(s, t)[0].double(), reference(s, s["index"][first:first + count], CFG)[2]))
    (whole, b0), (g1, b1), (g2, b2) = parts
    w1, w2 = m1 / M, (M - m1) / M
    mix = w1 * g1 + w2 * g2
    worst = float(((mix - whole).abs() / (b0 + w1 * b1 + w2 * b2)).max())
    print(f"ppo_shards: the weighted mean of two shards at {worst:.3f} of the sum of the bounds")
    assert worst <= 1.0
    assert float((g1 - g2).abs().max()) > 1e-3, "the shards are different minibatches"


# ---- 5. Adam -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_norm", [None, 0.5], ids=["noclip", "clip"])
@pytest.mark.parametrize("net", ["tanh64x64", "tanh256x3"])
def test_adam_steps_against_float64(net, max_norm):
    """every step from the engine's own float32 state against the float64 step of that state, within ppo_ref.adam_tolerances (derived by
    counting the roundings of the kernel's chain); 5 steps with step = 1 .. 5, then one with step = 1000: the bias corrections follow `step`"""
    s = synth(net, "go1gate", 5, 24)
    eng = handle("go1gate", 5)
    views = install(eng, s)
    opt = eng.optimizer_state()
    n, dev = s["n_params"], eng.torch_device
    assert opt["exp_avg"].shape == opt["exp_avg_sq"].shape == (n,)
    assert not bool(opt["exp_avg"].any()) and not bool(opt["exp_avg_sq"].any()), "the moments start at zero"
    gen = torch.Generator().manual_seed(9)
    opt["exp_avg"].copy_(torch.randn(n, generator=gen) * 0.1)
    opt["exp_avg_sq"].copy_(torch.rand(n, generator=gen) * 0.05)
    norm_dev = torch.full((3,), 7.0, device=dev)
    for step in (1, 2, 3, 4, 5, 1000):
        g = torch.randn(n, generator=gen) * 0.3
        g[:5] = 0.0
        p0, m0, v0 = views["flat"].cpu(), opt["exp_avg"].cpu(), opt["exp_avg_sq"].cpu()
        gd = g.to(dev)
        eng.adam_step(gd, step, 1e-3, max_grad_norm=max_norm, norm_out=norm_dev[1:2])
        torch.cuda.synchronize()
        p64, m64, v64, norm = ref.adam(p0, m0, v0, g, step, 1e-3, max_norm=max_norm)
        tol_p, tol_m, tol_v = ref.adam_tolerances(p0, m0, v0, g, step, 1e-3, max_norm=max_norm)
        worst = [float(((a.cpu().double() - b).abs() / tol).max()) for a, b, tol in
                 ((views["flat"], p64, tol_p), (opt["exp_avg"], m64, tol_m), (opt["exp_avg_sq"], v64, tol_v))]
        print(f"ppo_adam {net} clip={max_norm} step={step}: p {worst[0]:.3f} m {worst[1]:.3f} v {worst[2]:.3f} of the bound")
        assert max(worst) <= 1.0, (step, worst)
        assert abs(float(norm_dev[1]) - norm) <= 2 * EPS32 * norm and float(norm_dev[0]) == 7.0 and float(norm_dev[2]) == 7.0
        assert same_bits(gd.cpu(), g), "the gradient is an input"
        other = ref.adam(p0, m0, v0, g, step + 1 if step < 1000 else 1, 1e-3, max_norm=max_norm)[0]
        assert float(((views["flat"].cpu().double() - other).abs() / tol_p).max()) > 1.0, "step is honoured"
    # the views are live: what adam_step wrote is what they show, and a new actor starts from zero again
    install(eng, s)
    assert not bool(eng.optimizer_state()["exp_avg_sq"].any())


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refusals_of_mqe_ppo_grad():
    s = synth("tanh7", "go1gate", 3, 24)
    eng = handle("go1gate", 3)
    dev = eng.torch_device
    t = upload(s, dev)
    image = {k: v.clone() for k, v in t.items()}
    n = s["n"]

    def refused(code, word, first=0, count=50, use_index=True, cfg=CFG, **kw):
        rc = call(eng, s, t, first, count, use_index, cfg, **kw)
        msg = eng.lib.mqe_last_error().decode()
        torch.cuda.synchronize()
        assert rc == code and msg and word in msg, (kw, rc, msg)
        for k in t:
            assert torch.equal(t[k].view(torch.uint8), image[k].view(torch.uint8)), (kw, k, "a refused call wrote into the buffers")

    # no actor; an actor without a critic
    d, k, _ = make_desc("go1gate", 3)
    bare = hip_engine(d, k)
    rc = call(bare, s, t, 0, 50, True)
    assert rc == -6 and "no actor" in bare.lib.mqe_last_error().decode()
    bare.create_actor(s["a_dims"], None, activation=s["act"])
    rc = call(bare, s, t, 0, 50, True)
    assert rc == -6 and "critic" in bare.lib.mqe_last_error().decode()
    bare.close()
    views = install(eng, s)
    p = lambda name, off=0: t[name].data_ptr() + off
    refused(-1, "null", h=None)
    for name in ("packed", "actions", "logp", "value", "adv", "ret", "loss", "grad"):
        refused(-1, "required", **{name: None})
    for T in (0, -2, abi.ROLLOUT_MAX_STEPS + 1):
        refused(-6, "T must", T=T)
    refused(-6, "row_stride", stride=(s["pf"] + 3) // 4 * 4 - 4)
    refused(-6, "row_stride", stride=s["stride"] + 1)
    for name, key in (("packed", "packed"), ("actions", "actions"), ("logp", "logp_old"), ("value", "value"), ("adv", "adv"), ("ret", "ret"),
                      ("index", "index"), ("grad", "grad"), ("stats", "stats")):
        refused(-6, "misaligned", **{name: p(key, 2)})
    refused(-6, "misaligned", packed=p("packed", 4))                        # 4-byte aligned is not enough for packed_dev
    refused(-6, "count", count=0)
    refused(-6, "count", count=-3)
    refused(-6, "first", first=-1)
    refused(-6, "first + count", first=n - 49, count=50, use_index=False)
    for field in ("clip", "value_coef", "entropy_coef", "value_clip"):
        for bad in (-0.01, float("nan"), float("inf")):
            refused(-6, {"clip": "clip_ratio"}.get(field, field), cfg=dict(CFG, **{field: bad}))
    refused(-6, "flags", flags=2)
    refused(-6, "flags", flags=abi.PPO_CLIP_VALUE | 4)
    for name in ("packed", "actions", "logp_old", "value", "adv", "ret", "index"):
        refused(-6, "grad_dev", grad=p(name, 16))
        refused(-6, "stats_dev", stats=p(name, 16))
    refused(-6, "grad_dev", grad=views["flat"].data_ptr())
    refused(-6, "stats_dev", stats=views["flat"].data_ptr() + 4 * (s["n_params"] - 1))
    refused(-6, "stats_dev", stats=p("grad", 4 * (s["n_params"] - 1)))
    # the same call with nothing wrong then succeeds, and an index value outside the trajectory is clamped, not followed
    assert call(eng, s, t, 0, 50, True) == 0, eng.lib.mqe_last_error().decode()
    torch.cuda.synchronize()
    check(s, t, s["index"][:50], CFG, "after the refusals")
    u = upload(s, dev)
    u["index"][:3] = torch.tensor([-5, n + 1000, 2 ** 31 - 1], dtype=torch.int32, device=dev)
    assert call(eng, s, u, 0, 50, True) == 0
    torch.cuda.synchronize()
    sel = s["index"][:50].clone()
    sel[:3] = torch.tensor([0, n - 1, n - 1], dtype=torch.int32)
    check(s, u, sel, CFG, "clamped index values")


def test_refusals_of_mqe_ppo_adam():
    s = synth("tanh7", "go1gate", 3, 24)
    eng = handle("go1gate", 3)
    views = install(eng, s)
    opt = eng.optimizer_state()
    n, dev = s["n_params"], eng.torch_device
    g = torch.full((n + 8,), 0.25, device=dev)
    norm = torch.full((2,), 7.0, device=dev)
    before = [x.clone() for x in (views["flat"], opt["exp_avg"], opt["exp_avg_sq"])]
    f = eng.lib.mqe_ppo_adam

    def refused(code, word, **kw):
        a = dict(h=eng.h, grad=g.data_ptr(), step=1, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, max_norm=0.5, norm=norm.data_ptr())
        a.update(kw)
        rc = f(a["h"], a["grad"], a["step"], a["lr"], a["b1"], a["b2"], a["eps"], a["max_norm"], a["norm"], eng._stream())
        msg = eng.lib.mqe_last_error().decode()
        torch.cuda.synchronize()
        assert rc == code and word in msg, (kw, rc, msg)
        for was, now in zip(before, (views["flat"], opt["exp_avg"], opt["exp_avg_sq"])):
            assert same_bits(was, now), (kw, "a refused call changed the optimiser")
        assert bool((norm == 7.0).all())

    refused(-1, "null", h=None)
    refused(-1, "grad_dev", grad=None)
    for step in (0, -1):
        refused(-6, "step", step=step)
    refused(-6, "misaligned", grad=g.data_ptr() + 2)
    refused(-6, "misaligned", norm=norm.data_ptr() + 1)
    refused(-6, "lr", lr=float("nan"))
    for bad in (-0.1, 1.0, float("nan")):
        refused(-6, "beta1", b1=bad)
        refused(-6, "beta2", b2=bad)
    for bad in (-1e-8, float("inf"), float("nan")):
        refused(-6, "eps", eps=bad)
    refused(-6, "max_grad_norm", max_norm=float("inf"))
    refused(-6, "grad_dev", grad=views["flat"].data_ptr())
    refused(-6, "grad_dev", grad=opt["exp_avg_sq"].data_ptr())
    refused(-6, "norm_dev", norm=opt["exp_avg"].data_ptr() + 8)
    refused(-6, "norm_dev", norm=g.data_ptr() + 4)
    with pytest.raises(ValueError, match="grad"):
        eng.adam_step(g, 1, 1e-3)                                      # n + 8 elements


# ---- 7. the public surface ---------------------------------------------------------------------------------------------------------------------
def _torch_loss_inputs(traj, sel):
    flat = lambda x, *tail: x.reshape(-1, *tail)[sel].double().cpu()
    T = traj.T
    return dict(obs=flat(traj.obs[:T], traj.obs.shape[-1]), actions=flat(traj.actions, 3), logp_old=flat(traj.logp), v_old=flat(traj.value[:T]),
                adv=flat(traj.advantages), ret=flat(traj.returns))


def test_public_surface(gate_cfg_restored):  # noqa: F811
    """rollout(gamma) -> ppo_update(epochs=1, minibatches=2) on a real go1gate env; the parameters against a float64 torch replay (autograd +
    torch.optim.Adam + clip_grad_norm_) that draws the same permutation.  The bound of step k: the gradient may deviate by dg = K_GPU 2^-24 S_n
    (+ for step 2 the change of the float64 gradient under a parameter perturbation of the size of step 1's bound, measured on the REFERENCE
    with four random sign patterns and doubled), and an Adam step maps a gradient deviation dg to at most
        step_size ((1 - b1) dg / denom + |m'| sqrt((1 - b2) (2 |g| dg + dg^2)) / (bc2s denom^2))      (|sqrt a - sqrt b| <= sqrt |a - b|)
    plus ppo_ref.adam_tolerances for the step's own roundings."""
    N, T = 8, 16
    env = _gate_env(N)
    actor, critic, log_std = _modules(3)
    env.set_actor(actor, critic, log_std=log_std)
    env.reset()
    eng = env.env.engine
    traj = env.rollout(T, gamma=0.99, lam=0.95)
    p0 = eng.actor_params()["flat"].clone()
    a_dims, c_dims = eng._actor["actor_dims"], eng._actor["critic_dims"]
    kw = dict(epochs=1, minibatches=2, lr=1e-3, clip=0.2, value_coef=0.5, entropy_coef=0.01, value_clip=0.2, max_grad_norm=1.0)
    stats = env.ppo_update(traj, generator=torch.Generator(device="cuda").manual_seed(11), **kw)
    torch.cuda.synchronize()
    assert stats.shape == (1, 2, abi.PPO_STATS) and bool(torch.isfinite(stats).all()) and eng.ppo_step == 2
    p_gpu = eng.actor_params()["flat"].cpu().double()
    assert not same_bits(p0, eng.actor_params()["flat"])
    # the float64 replay
    total = T * N * 2
    perm = torch.randperm(total, device="cuda", generator=torch.Generator(device="cuda").manual_seed(11)).cpu()
    cfg = dict(clip=0.2, value_coef=0.5, entropy_coef=0.01, value_clip=0.2)
    p, m, v = p0.cpu().double(), torch.zeros(len(p0), dtype=torch.float64), torch.zeros(len(p0), dtype=torch.float64)
    bound = torch.zeros_like(p)
    b1, b2, lr, eps = (float(np.float32(x)) for x in (0.9, 0.999, 1e-3, 1e-8))
    for k in range(2):
        sel = perm[k * (total // 2):(k + 1) * (total // 2)]
        batch = _torch_loss_inputs(traj, sel)
        grad_at = lambda q: ref.manual(ref.split_flat(q, a_dims, c_dims), a_dims, c_dims, "tanh", batch, cfg)
        g, st64, S, ss = grad_at(p)
        g = ref.flat_grad(g, a_dims, c_dims)
        dg = ref.flat_grad({n: torch.full(shape, S[n], dtype=torch.float64) for n, (_, shape) in abi.actor_param_layout(a_dims, c_dims).items()},
                           a_dims, c_dims) * (ref.K_GPU * EPS32)
        if k == 0:                       # the statistics of the first minibatch are taken at the parameters the replay starts from
            assert float(((stats[0, 0].cpu().double() - st64).abs() / (ss * ref.K_GPU * EPS32)).max()) <= 1.0
        else:
            gsign = torch.Generator().manual_seed(1)
            for _ in range(4):
                sign = (torch.randint(0, 2, p.shape, generator=gsign) * 2 - 1).double()
                dg = torch.maximum(dg, dg + 2 * (ref.flat_grad(grad_at(p + sign * bound)[0], a_dims, c_dims) - g).abs())
        pn, mn, vn, norm = ref.adam(p, m, v, g, k + 1, 1e-3, max_norm=1.0)
        tol_p = ref.adam_tolerances(p, m, v, g, k + 1, 1e-3, max_norm=1.0)[0]
        scale = min(1.0, 1.0 / (norm + 1e-6))
        gs, dgs = g.abs() * scale, dg * scale * 1.01
        step_size, bc2s = lr / (1 - b1 ** (k + 1)), (1 - b2 ** (k + 1)) ** 0.5
        vlow = torch.clamp(vn - (1 - b2) * (2 * gs * dgs + dgs * dgs), min=0.0)
        denom = torch.sqrt(vlow) / bc2s + eps
        bound = bound + tol_p + step_size * ((1 - b1) * dgs / denom + (mn.abs() + (1 - b1) * dgs) * torch.sqrt((1 - b2) * (2 * gs * dgs + dgs * dgs)) / (bc2s * denom * denom))
        p, m, v = pn, mn, vn
    worst = float(((p_gpu - p).abs() / bound).max())
    print(f"ppo_update replay: parameters at {worst:.3f} of the propagated bound; largest change {float((p - p0.cpu().double()).abs().max()):.2e}")
    assert worst <= 1.0
    # pull_actor: the torch modules equal the engine's buffer bit for bit
    env.pull_actor()
    torch.cuda.synchronize()
    views = eng.actor_params()
    lin = [l for l in actor if isinstance(l, torch.nn.Linear)]
    for l, layer in enumerate(lin):
        assert same_bits(layer.weight.detach(), views[f"actor.{l}.weight"]) and same_bits(layer.bias.detach(), views[f"actor.{l}.bias"])
    clin = [l for l in critic if isinstance(l, torch.nn.Linear)]
    assert same_bits(clin[-1].weight.detach(), views[f"critic.{len(clin) - 1}.weight"])
    assert same_bits(log_std.to("cuda"), views["log_std"])
    # a following rollout continues the trajectory with the new parameters
    nxt = env.rollout(4)
    torch.cuda.synchronize()
    assert same_bits(nxt.obs[0], traj.obs[T])
    with torch.no_grad():
        mean64 = actor.double()(nxt.obs[:1].double())
        z = (nxt.actions[:1].double() - mean64) / torch.exp(views["log_std"].double())
        assert float(z.abs().max()) < 6.5, "the rollout's actions are samples around the UPDATED actor's mean"
        actor.float()
    # ten full-batch steps on one fixed trajectory lower the loss
    losses = [float(env.ppo_update(traj, epochs=1, minibatches=1, lr=1e-3, entropy_coef=0.0, value_coef=0.5)[0, 0, 3]) for _ in range(10)]
    print("ppo_update ten full-batch steps: L =", " ".join(f"{x:.5f}" for x in losses))
    assert losses[-1] < losses[0]
    with pytest.raises(ValueError, match="minibatches"):
        env.ppo_update(traj, epochs=1, minibatches=0, lr=1e-3)
    env.close()


def test_openrl_ppo_update_torch_passes_through(gate_cfg_restored):  # noqa: F811
    from openrl_ws.utils import mqe_openrl_wrapper
    N, T = 4, 6
    actor, critic, log_std = _modules(2)
    w = mqe_openrl_wrapper(_gate_env(N))
    w.set_actor(actor, critic, log_std=log_std)
    w.env.reset()
    traj = w.rollout_torch(T, gamma=0.98)
    st = w.ppo_update_torch(traj, epochs=2, minibatches=3, lr=5e-4, generator=torch.Generator(device="cuda").manual_seed(1))
    torch.cuda.synchronize()
    assert st.shape == (2, 3, 6) and bool(torch.isfinite(st).all()) and w.env.env.engine.ppo_step == 6
    w.close()
