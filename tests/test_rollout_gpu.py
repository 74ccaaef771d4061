"""-m gpu: on-device rollouts (mqe_actor_create / mqe_actor_params / mqe_rollout, csrc/kernels_actor.hpp; HipEngine.rollout,
FusedTaskWrapper.set_actor / rollout): (1) the networks against float64, held to 4x the error of a torch float32 CPU evaluation; (2) the
samples against the host twin of the counter RNG, their log-density and moments; (3) a rollout is T steps, bit for bit; (4) continuation,
checkpoint, the observation a wrapper rollout starts from; (5) shards; (6) every element written, nothing beyond; (7) no side effects on
the step, live parameters; (8) every refusal; (9) the public surface."""
import ctypes as C
import math
import types

import numpy as np
import pytest
import torch

import rollout_ref as ref
from helpers import make_desc, hip_engine
from mqe.engine import abi
from mqe.engine.hip_engine import Rollout

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -24
NETS = {"tanh64x64": ("tanh", (64, 64)), "tanh7": ("tanh", (7,)), "relu128x3": ("relu", (128, 128, 128))}
_ENGINES = {}


def bits(t):
    return t.contiguous().view(torch.uint8) if t.dtype == torch.bool else t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def engine(task, N, seed=None, **kw):
    d, k, _ = make_desc(task, N, **kw)
    if seed is not None:
        d.seed = seed
    return hip_engine(d, k)


def shared_engine(task, N):
    if (task, N) not in _ENGINES:
        _ENGINES[(task, N)] = engine(task, N)
    return _ENGINES[(task, N)]


def install(eng, net, critic, pseed, gain=1.0):
    """create the engine's actor with seeded parameters; -> (params, actor_dims, critic_dims, activation)"""
    act, hidden = NETS[net]
    D = int(eng.tensor(abi.T_WRAPPER_OBS).shape[-1])
    a_dims, c_dims = [D, *hidden, 3], ([D, *hidden, 1] if critic else None)
    eng.create_actor(a_dims, c_dims, activation=act, action_gain=gain)
    params = ref.seeded_params(a_dims, c_dims, pseed)
    views = eng.actor_params()
    for n, v in params.items():
        views[n].copy_(v)
    assert views["flat"].numel() == abi.actor_param_count(a_dims, c_dims)
    return params, a_dims, c_dims, act


def net_errors(params, a_dims, c_dims, act, obs):
    """float64 mean / value on obs, and the yardstick: max |float32 CPU torch - float64| of each"""
    o64 = obs.double()
    m64, m32 = ref.mlp(params, "actor", len(a_dims) - 1, act, o64), ref.mlp(params, "actor", len(a_dims) - 1, act, obs.float())
    out = dict(mean64=m64, yard_mean=float((m32.double() - m64).abs().max()))
    if c_dims:
        v64 = ref.mlp(params, "critic", len(c_dims) - 1, act, o64)[..., 0]
        v32 = ref.mlp(params, "critic", len(c_dims) - 1, act, obs.float())[..., 0]
        out.update(value64=v64, yard_value=float((v32.double() - v64).abs().max()))
    return out


def sampling_tolerances(yard_mean, amax, min_std, zmax):
    """(tol_z, tol_logp) of a sampled rollout; the derivation is in test_samples_are_the_counter_rng_draws.  Every term is an UPPER BOUND
    worked out from the formats, not a measurement: 4 x yardstick is what test 1 allows the mean (its measured error is 1-2x), and the
    libm allowance is a worst case; the observed deviations are ~7x (z) and ~60x (logp) below these, which still catch a wrong term,
    constant or key (a wrong draw is off by O(1))."""
    tol_z = (4 * yard_mean + EPS32 * amax) / min_std + 5.77 * 10 * EPS32
    return tol_z, 3 * zmax * tol_z + 8 * 64 * EPS32


# ---- 1. the networks against float64 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("critic", [False, True], ids=["nocritic", "critic"])
@pytest.mark.parametrize("net", list(NETS))
@pytest.mark.parametrize("task,N,D,Aw", [("go1gate", 3, 16, 2), ("go1sheep-hard", 5, 34, 2), ("go1football-defender", 4, 20, 2), ("go1seesaw", 3, 14, 2)])
def test_networks_against_float64(task, N, D, Aw, net, critic):
    """Deterministic rollouts: actions == mean, value, logp == -sum log_std - 1.5 ln 2 pi.  The kernel's maximum deviation from the
    float64 network may be at most 4x the maximum deviation of a torch float32 CPU evaluation of the same network on the same
    observations (another summation order and libm: the same size class, not the same bits).  Measured maxima: profiles/rollout.txt."""
    eng = shared_engine(task, N)
    assert tuple(eng.tensor(abi.T_WRAPPER_OBS).shape) == (N, Aw, D)
    params, a_dims, c_dims, act = install(eng, net, critic, pseed=1000 + len(net) + 7 * critic)
    eng.reset_all()
    T = 6
    traj = eng.rollout(T, deterministic=True)
    torch.cuda.synchronize()
    assert traj.obs.shape == (T + 1, N, Aw, D) and traj.actions.shape == (T, N, Aw, 3) and traj.logp.shape == (T, N, Aw)
    obs = traj.obs.cpu()
    assert torch.isfinite(obs).all()
    e = net_errors(params, a_dims, c_dims, act, obs)
    dev_mean = float((traj.actions.cpu().double() - e["mean64"][:T]).abs().max())
    print(f"rollout_net task={task} net={net} critic={int(critic)} mean: kernel {dev_mean:.3e} torch-f32 {e['yard_mean']:.3e}", end="")
    if critic:
        assert traj.value.shape == (T + 1, N, Aw)
        dev_value = float((traj.value.cpu().double() - e["value64"]).abs().max())
        print(f" value: kernel {dev_value:.3e} torch-f32 {e['yard_value']:.3e}")
        assert dev_value <= 4 * e["yard_value"], (dev_value, e["yard_value"])
    else:
        print()
        assert traj.value is None
    assert dev_mean <= 4 * e["yard_mean"], (dev_mean, e["yard_mean"])
    # logp at z = 0: three subtractions of log_std and one of the constant, partial sums below 8 in magnitude: 4 roundings of <= 8 * 2^-24
    want = -float(params["log_std"].double().sum()) - 1.5 * math.log(2 * math.pi)
    assert float((traj.logp.cpu().double() - want).abs().max()) <= 4 * 8 * EPS32


# ---- 2. sampling ---------------------------------------------------------------------------------------------------------------------------
def test_samples_are_the_counter_rng_draws():
    """z recovered from the stored action, z = (a - mean64) / exp(log_std), against the host twin's draw for the key (seed, global env,
    MQE_RNG_ACTOR + post-step ordinal, agent * 3 + j).  Tolerance, derived:
      * the kernel's mean may deviate from mean64 by 4x the torch-float32 yardstick (what test 1 holds it to) -> / min exp(log_std);
      * a is one float32 rounding of mean + std z (an fmaf): 2^-24 max|a| -> / min exp(log_std);
      * the draw itself: the kernel's float32 logf, sqrtf (2.5 ulp form), cosf, expf and two product roundings against the float64 twin --
        under 10 ulp in all, relative to r = sqrt(-2 log(1 - u1)) <= 5.77 (cos near 0 has an ABSOLUTE error of an ulp of 1): 5.77 * 10 * 2^-24.
    logp against the float64 Gaussian density of the stored action: |d logp / d z_j| = |z_j|, three columns -> 3 max|z| tol_z, plus the
    float32 rounding of a sum of <= 8 terms below 64 in magnitude.  Moments over the 12 288 draws: 4 sigma bounds (tests/test_rollout.py
    checks that the twin alone meets them for this seed)."""
    N, T, Aw, seed = 64, 32, 2, 7
    eng = engine("go1gate", N, seed=seed)
    params, a_dims, c_dims, act = install(eng, "tanh64x64", True, pseed=21)
    eng.reset_all()
    traj = eng.rollout(T)
    torch.cuda.synchronize()
    obs, a = traj.obs.cpu(), traj.actions.cpu().double()
    e = net_errors(params, a_dims, c_dims, act, obs[:T])
    ls = params["log_std"].double()
    std = torch.exp(ls)
    z = ((a - e["mean64"]) / std).numpy()
    twin = ref.actor_draws(seed, 0, N, Aw, 0, T)
    tol_z, tol_lp = sampling_tolerances(e["yard_mean"], float(a.abs().max()), float(std.min()), float(np.abs(twin).max()))
    dev = float(np.abs(z - twin).max())
    print(f"rollout_sampling z: kernel-vs-twin {dev:.3e} tol {tol_z:.3e} (yardstick mean {e['yard_mean']:.3e}, min std {float(std.min()):.3f})")
    assert dev <= tol_z
    logp64 = ref.gaussian_logp(a, e["mean64"], ls)
    dev_lp = float((traj.logp.cpu().double() - logp64).abs().max())
    print(f"rollout_sampling logp: dev {dev_lp:.3e} tol {tol_lp:.3e}")
    assert dev_lp <= tol_lp
    n = z.size
    assert n == 12288
    print(f"rollout_sampling moments: mean {z.mean():.4f} (<= {4 / math.sqrt(n):.4f}) var {z.var():.4f} (|.-1| <= {4 * math.sqrt(2 / n):.4f})")
    assert abs(z.mean()) <= 4 / math.sqrt(n) and abs(z.var() - 1) <= 4 * math.sqrt(2 / n)
    # another seed, other draws (same scene, same parameters)
    outs = []
    for s in (0, 7):
        e2 = engine("go1gate", 4, seed=s)
        install(e2, "tanh64x64", False, pseed=21)
        e2.reset_all()
        outs.append(e2.rollout(1).actions.cpu())
        e2.close()
    assert not torch.equal(outs[0], outs[1])
    eng.close()


# ---- 3. a rollout is T steps --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("task,N", [("go1gate", 5), ("go1sheep-hard", 3)])
def test_rollout_is_T_steps(task, N):
    """handle A rolls out 12 steps with every env timing out inside the window; handle B (same scene, same seed) is stepped with
    gain * traj.actions[t]: observation, reward and done bytes agree bit for bit at every t.  go1sheep-hard's NPC script draws N(0, 1) from
    the same step counter: the actor's stream collides with none of the old ones."""
    T = 12
    A, B = engine(task, N, max_episode_length=5), engine(task, N, max_episode_length=5)
    install(A, "tanh64x64", True, pseed=5)
    A.reset_all(); B.reset_all()
    traj = A.rollout(T)
    assert same_bits(traj.obs[0], B.tensor(abi.T_WRAPPER_OBS))
    seen = 0
    for t in range(T):
        B.step(traj.actions[t].contiguous())          # action_gain = 1
        assert same_bits(traj.obs[t + 1], B.tensor(abi.T_WRAPPER_OBS)), t
        assert same_bits(traj.reward[t], B.tensor(abi.T_WRAPPER_REWARD)), t
        assert torch.equal(traj.done[t].view(torch.uint8), B.tensor(abi.T_RESET_BUF)), t
        seen += int(traj.done[t].sum())
    assert bool(traj.done.any(dim=0).all()), "every env times out at least once inside the window"
    assert seen >= N
    assert same_bits(A.tensor(abi.T_ROOT_STATE), B.tensor(abi.T_ROOT_STATE))
    A.close(); B.close()


# ---- 4. continuation and checkpoint ------------------------------------------------------------------------------------------------------
def _traj_equal(a, b):
    return (same_bits(a.obs, b.obs) and same_bits(a.reward, b.reward) and same_bits(a.done, b.done) and same_bits(a.actions, b.actions)
            and same_bits(a.logp, b.logp) and same_bits(a.value, b.value))


def test_continuation_and_checkpoint():
    N = 6
    A, B = engine("go1sheep-hard", N, max_episode_length=9), engine("go1sheep-hard", N, max_episode_length=9)
    for e in (A, B):
        install(e, "tanh64x64", True, pseed=8)
        e.reset_all()
    r1 = A.rollout(6)
    assert same_bits(A.tensor(abi.T_WRAPPER_OBS), r1.obs[6]) and same_bits(A.tensor(abi.T_WRAPPER_REWARD), r1.reward[5])
    assert torch.equal(A.tensor(abi.T_WRAPPER_PACKED)[-((N + 3) // 4):].view(torch.uint8)[:N], r1.done[5].view(torch.uint8))
    r2 = A.rollout(6)                      # obs0 = None: the engine's own buffer was brought to row T of the first rollout
    whole = B.rollout(12)
    for name in ("obs", "reward", "done", "actions", "logp", "value"):
        w = getattr(whole, name)
        first, second = getattr(r1, name), getattr(r2, name)
        if name in ("obs", "value"):       # T + 1 entries: entry 6 is shared
            assert same_bits(first, w[:7]) and same_bits(second, w[6:]), name
        else:
            assert same_bits(first, w[:6]) and same_bits(second, w[6:]), name
    # save -> rollout(8) -> load -> rollout(8): the same trajectory twice
    blob = A.save_state()                  # the blob holds the engine's own return buffer, which is current after a rollout
    x = A.rollout(8)
    A.load_state(blob)
    y = A.rollout(8)
    assert same_bits(x.obs[0], r2.obs[6])
    assert _traj_equal(x, y)
    assert bool(x.done.any())
    A.close(); B.close()


def test_widest_network_and_caller_buffers():
    """hidden width 256 (MQE_ACTOR_MAX_HIDDEN: 134 kB of LDS per workgroup) with 4 Linear layers, held to test 1's bound; and what
    rollout(out=...) refuses before it hands raw pointers to the library"""
    eng = shared_engine("go1gate", 3)
    NETS["tanh256x3"] = ("tanh", (256, 256, 256))
    try:
        params, a_dims, c_dims, act = install(eng, "tanh256x3", True, pseed=77)
    finally:
        del NETS["tanh256x3"]
    eng.reset_all()
    T = 3
    traj = eng.rollout(T, deterministic=True)
    e = net_errors(params, a_dims, c_dims, act, traj.obs.cpu())
    dev_mean = float((traj.actions.cpu().double() - e["mean64"][:T]).abs().max())
    dev_value = float((traj.value.cpu().double() - e["value64"]).abs().max())
    print(f"rollout_net task=go1gate net=tanh256x3 critic=1 mean: kernel {dev_mean:.3e} torch-f32 {e['yard_mean']:.3e} value: kernel {dev_value:.3e} torch-f32 {e['yard_value']:.3e}")
    assert dev_mean <= 4 * e["yard_mean"] and dev_value <= 4 * e["yard_value"]
    good, _ = _buffers(eng, T)
    for field, bad in (("actions", good.actions.transpose(1, 2)), ("logp", good.logp[:, :, :1]), ("value", good.value.double())):
        r, _ = _buffers(eng, T)
        setattr(r, field, bad)
        with pytest.raises(ValueError, match=f"out.{field}"):
            eng.rollout(T, out=r)
    with pytest.raises(ValueError, match="3 steps, not 2"):
        eng.rollout(2, out=good)
    assert eng.rollout(T, out=good) is good


# ---- 5. shards ---------------------------------------------------------------------------------------------------------------------------------
def test_a_shard_reproduces_its_rows():
    T = 8
    full, part = engine("go1gate", 4, max_episode_length=5), engine("go1gate", 2, max_episode_length=5, env_id_offset=2)
    for e in (full, part):
        install(e, "tanh64x64", True, pseed=13)
        e.reset_all()
    f, p = full.rollout(T), part.rollout(T)
    assert same_bits(f.obs[:, 2:4], p.obs) and same_bits(f.actions[:, 2:4], p.actions) and same_bits(f.logp[:, 2:4], p.logp)
    assert same_bits(f.value[:, 2:4], p.value) and same_bits(f.reward[:, 2:4], p.reward) and same_bits(f.done[:, 2:4], p.done)
    assert not same_bits(f.actions[:, 0:2], p.actions)
    full.close(); part.close()


# ---- 6. every element is written, nothing beyond ------------------------------------------------------------------------------------------
SENT = 0x7FC12345          # a NaN pattern none of whose bytes is 0 or 1


def _sentinel(n, dev):
    return torch.full((n,), SENT, dtype=torch.int32, device=dev).view(torch.float32)


def _is_sent(t):
    return t.contiguous().view(torch.int32) == SENT


def _buffers(eng, T, extra_stride=8, guard=64):
    """(Rollout over sentinel-filled buffers with `guard` elements behind each, the flat tensors)"""
    N, Aw, D = (int(x) for x in eng.tensor(abi.T_WRAPPER_OBS).shape)
    dev = eng.torch_device
    stride = eng.rollout_row_stride() + extra_stride
    flat = dict(packed=_sentinel((T + 1) * stride + guard, dev), actions=_sentinel(T * N * Aw * 3 + guard, dev),
                logp=_sentinel(T * N * Aw + guard, dev), value=_sentinel((T + 1) * N * Aw + guard, dev))
    r = Rollout(flat["packed"][:(T + 1) * stride].view(T + 1, stride), flat["actions"][:T * N * Aw * 3].view(T, N, Aw, 3),
                flat["logp"][:T * N * Aw].view(T, N, Aw), flat["value"][:(T + 1) * N * Aw].view(T + 1, N, Aw), (N, Aw, D))
    return r, flat


@pytest.mark.parametrize("N", [3, 5])          # R' = 6 and 10 rows: no multiple of a workgroup's 64
def test_every_element_written_nothing_beyond(N):
    T = 5
    eng = shared_engine("go1gate", N)
    install(eng, "tanh7", True, pseed=3)
    eng.reset_all()
    r, flat = _buffers(eng, T)
    out = eng.rollout(T, out=r)
    torch.cuda.synchronize()
    assert out is r
    Aw, D = 2, 16
    n, nr = N * Aw * D, N * Aw
    pf = n + nr + (N + 3) // 4
    for name, used in (("packed", r.packed.numel()), ("actions", r.actions.numel()), ("logp", r.logp.numel()), ("value", r.value.numel())):
        assert _is_sent(flat[name][used:]).all(), f"{name}: guard elements touched"
    assert _is_sent(r.packed[:, pf:]).all(), "stride padding touched"
    assert not _is_sent(r.packed[:, :n + nr]).any(), "an observation / reward element was left unwritten"
    done_bytes = r.packed[:, n + nr:pf].contiguous().view(torch.uint8)
    assert bool((done_bytes[:, :N] <= 1).all()), "done bytes are 0 / 1"
    assert bool((done_bytes[0, :N] == 0).all()) and bool((r.packed[0, n:n + nr] == 0).all()), "row 0: reward and done zeroed"
    pad = done_bytes[:, N:]
    want = torch.tensor(list(SENT.to_bytes(4, "little")), dtype=torch.uint8, device=pad.device)[N % 4:] if N % 4 else pad[:, :0]
    assert pad.numel() == 0 or bool((pad == want).all()), "pad bytes of the last done word are never written"
    assert torch.isfinite(r.actions).all() and torch.isfinite(r.logp).all() and torch.isfinite(r.value).all()
    assert torch.isfinite(r.value[T]).all(), "value[T]: the bootstrap value"
    assert r.done.dtype == torch.bool and r.done.shape == (T, N)


# ---- 7. no side effects on the step; live parameters --------------------------------------------------------------------------------------
def test_no_side_effects_and_live_parameters():
    N = 4
    X, Y = engine("go1gate", N), engine("go1gate", N)
    params, a_dims, c_dims, act = install(X, "tanh64x64", True, pseed=2)
    X.reset_all(); Y.reset_all()
    g = torch.Generator().manual_seed(4)
    for t in range(8):
        a = (torch.rand(N, 2, 3, generator=g) * 2 - 1).cuda()
        X.step(a); Y.step(a)
    for kind in (abi.T_WRAPPER_PACKED, abi.T_ROOT_STATE, abi.T_DOF_STATE, abi.T_HISTORY):
        assert same_bits(X.tensor(kind), Y.tensor(kind)), kind
    # parameters are live: a second rollout follows what was written between the two
    r1 = X.rollout(3, deterministic=True)
    e1 = net_errors(params, a_dims, c_dims, act, r1.obs.cpu())
    assert float((r1.actions.cpu().double() - e1["mean64"][:3]).abs().max()) <= 4 * e1["yard_mean"]
    new = ref.seeded_params(a_dims, c_dims, 99)
    views = X.actor_params()
    for n_, v in new.items():
        views[n_].copy_(v)
    r2 = X.rollout(3, obs0=r1.obs[3].contiguous(), deterministic=True)
    e2 = net_errors(new, a_dims, c_dims, act, r2.obs.cpu())
    old_on_new_obs = ref.mlp(params, "actor", len(a_dims) - 1, act, r2.obs.cpu().double())[:3]
    assert float((r2.actions.cpu().double() - e2["mean64"][:3]).abs().max()) <= 4 * e2["yard_mean"]
    assert float((r2.actions.cpu().double() - old_on_new_obs).abs().max()) > 1e-2
    # every weight zero: mean = output bias, value = the critic's output bias, exactly
    for n_, v in views.items():
        if n_.endswith(".weight"):
            v.zero_()
    r3 = X.rollout(2, obs0=r2.obs[3].contiguous(), deterministic=True)
    assert torch.equal(r3.actions.cpu(), new["actor.2.bias"].expand(2, N, 2, 3))
    assert torch.equal(r3.value.cpu(), new["critic.2.bias"].expand(3, N, 2))
    X.close(); Y.close()


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    N, T = 3, 2
    eng = engine("go1gate", N)
    eng.reset_all()
    f = eng.lib.mqe_rollout
    r, flat = _buffers(eng, T)
    p = lambda t, off=0: C.c_void_p((t.data_ptr() + off) if t is not None else None)
    stride = int(r.packed.stride(0))
    pf = eng.tensor(abi.T_WRAPPER_PACKED).numel()

    def refused(code, **kw):
        a = dict(h=eng.h, T=T, obs0=p(None), packed=p(r.packed), stride=stride, actions=p(r.actions), logp=p(r.logp), value=p(r.value), flags=0)
        a.update(kw)
        rc = f(a["h"], a["T"], a["obs0"], a["packed"], a["stride"], a["actions"], a["logp"], a["value"], a["flags"], eng._stream())
        msg = eng.lib.mqe_last_error().decode()
        torch.cuda.synchronize()
        assert rc == code and msg, (kw, rc, msg)
        for name, t in flat.items():
            assert _is_sent(t).all(), (kw, name, "a refused call wrote into the buffers")
        return msg

    assert "no actor" in refused(-6)                                   # no actor yet
    install(eng, "tanh7", False, pseed=1)
    assert "critic" in refused(-6)                                     # value given without a critic
    install(eng, "tanh7", True, pseed=1)
    refused(-1, h=None)
    refused(-6, T=0)
    refused(-6, T=-3)
    refused(-6, T=abi.ROLLOUT_MAX_STEPS + 1)
    refused(-1, packed=p(None))
    refused(-1, actions=p(None))
    refused(-6, stride=pf - 1 if (pf - 1) % 4 == 0 else (pf // 4) * 4 - 4)      # a multiple of 4, too small
    refused(-6, stride=stride + 1)                                     # large enough, not a multiple of 4
    refused(-6, packed=p(r.packed, 4))                                 # 4-byte aligned only
    refused(-6, actions=p(r.actions, 2))
    refused(-6, logp=p(r.logp, 1))
    refused(-6, value=p(r.value, 2))
    refused(-6, obs0=p(eng.tensor(abi.T_WRAPPER_OBS), 2))
    seen = []
    eng.step(torch.zeros(N, 2, 3, device=eng.torch_device), between=lambda: seen.append(refused(-8)))
    assert seen and "open step" in seen[0]

    # mqe_actor_create
    def create_refused(e, *a, **kw):
        with pytest.raises(RuntimeError, match=r"mqe_actor_create failed \(-6\)") as ei:
            e.create_actor(*a, **kw)
        return str(ei.value)
    assert "obs_dim" in create_refused(eng, [17, 8, 3])
    assert "hidden width" in create_refused(eng, [16, 257, 3])
    assert "hidden width" in create_refused(eng, [16, 8, 3], [16, 257, 1])
    with pytest.raises(ValueError, match="5 Linear layers, at most 4"):       # mqe_actor_shape cannot even hold them: the binding's own refusal
        eng.create_actor([16, 8, 8, 8, 8, 3])
    sh = abi.ActorShape(obs_dim=16, act_dim=3, actor_layers=5, activation=0, action_gain=1.0)      # the same through the C entry point itself
    for i, v in enumerate([16, 8, 8, 8, 8]):
        sh.actor_dims[i] = v
    assert eng.lib.mqe_actor_create(eng.h, C.byref(sh)) == -6 and "Linear layers" in eng.lib.mqe_last_error().decode()
    stub = engine("go1football-1vs1", 2)
    assert "no task observation" in create_refused(stub, [int(stub.tensor(abi.T_WRAPPER_OBS).shape[-1]), 8, 3])
    stub.close()
    from replay import CMD_FLAGS
    cmd = engine("go1gate", 2, command_flags=CMD_FLAGS)
    assert cmd.desc.num_command_dims != 3
    assert "num_command_dims" in create_refused(cmd, [16, 8, 3])
    cmd.close()
    # a refused create leaves the actor that was there; the same call with nothing wrong succeeds
    rc = f(eng.h, T, p(None), p(r.packed), stride, p(r.actions), p(r.logp), p(r.value), 0, eng._stream())
    torch.cuda.synchronize()
    assert rc == 0, eng.lib.mqe_last_error().decode()
    assert not _is_sent(r.actions).any() and not _is_sent(r.value).any() and torch.isfinite(r.logp).all()
    eng.close()


# ---- 9. the public surface ------------------------------------------------------------------------------------------------------------------
def _gate_env(n, record_video=False):
    from mqe.envs.utils import make_mqe_env, custom_cfg
    from mqe.utils.helpers import finish_args
    a = finish_args(types.SimpleNamespace(task="go1gate", num_envs=n, seed=1, headless=True, record_video=record_video, sim_device="cuda:0", pipeline="gpu",
                                          subscenes=0, num_threads=0))
    return make_mqe_env("go1gate", a, custom_cfg(a))[0]


@pytest.fixture
def gate_cfg_restored():
    from mqe.envs.utils import ENV_DICT
    c = ENV_DICT["go1gate"]["config"]
    saved = (c.env.num_envs, c.env.record_video)
    yield
    c.env.num_envs, c.env.record_video = saved


def _modules(seed):
    nn = torch.nn
    torch.manual_seed(seed)
    actor = nn.Sequential(nn.Linear(16, 32), nn.Tanh(), nn.Linear(32, 32), nn.Tanh(), nn.Linear(32, 3))
    critic = nn.Sequential(nn.Linear(16, 32), nn.Tanh(), nn.Linear(32, 1))
    return actor.cuda(), critic.cuda(), torch.tensor([-0.7, -0.2, 0.1])


def test_public_surface(gate_cfg_restored):
    N, T = 4, 8
    env = _gate_env(N)
    actor, critic, log_std = _modules(0)
    env.set_actor(actor, critic, log_std=log_std)
    env.reset()
    g = torch.Generator().manual_seed(6)
    obs, _, _, _ = env.step((torch.rand(N, 2, 3, generator=g) * 2 - 1).cuda())      # leaves the engine's own return buffer stale
    count0 = env.reward_buffer["step count"]
    steps0, common0 = env.env._steps_policy, env.env.common_step_counter
    traj = env.rollout(T)
    assert same_bits(traj.obs[0], obs), "the rollout starts from the observation the last step returned"
    assert traj.obs.shape == (T + 1, N, 2, 16) and traj.reward.shape == (T, N, 2) and traj.done.shape == (T, N) and traj.done.dtype == torch.bool
    assert traj.actions.shape == (T, N, 2, 3) and traj.logp.shape == (T, N, 2) and traj.value.shape == (T + 1, N, 2)
    assert env.reward_buffer["step count"] == count0 + T
    assert env.env._steps_policy == steps0 + T and env.env.common_step_counter == common0 + T
    # the engine evaluated the modules: float64 mean of the torch actor at the stored observations, 4x the float32 yardstick as in test 1
    with torch.no_grad():
        o = traj.obs[:T].cpu()
        a64, a32 = actor.cpu().double()(o.double()), actor.float()(o)
        yard = float((a32.double() - a64).abs().max())
        z = (traj.actions.cpu().double() - a64) / torch.exp(log_std.double())
        lp = traj.logp.cpu().double()
        _, tol_lp = sampling_tolerances(yard, float(traj.actions.abs().max()), float(torch.exp(log_std).min()), 5.77)
        assert float((lp - ref.gaussian_logp(traj.actions.cpu().double(), a64, log_std.double())).abs().max()) <= tol_lp
        assert float(z.abs().max()) < 6.0
    # this wrapper's get_state / set_state carry the observation a rollout starts from: the same trajectory twice
    ck = env.get_state()
    assert same_bits(ck["last_obs"].cuda(), traj.obs[T])
    again1 = env.rollout(4)
    env.set_state(ck)
    again2 = env.rollout(4)
    assert _traj_equal(again1, again2) and same_bits(again1.obs[0], traj.obs[T])
    assert env.returned_batch.numel() == env.env.engine.tensor(abi.T_WRAPPER_PACKED).numel()      # one row, not a view of the trajectory
    keep = [t.clone() for t in (traj.obs, traj.reward, traj.done, traj.actions, traj.logp, traj.value)]
    obs2, _, _, _ = env.step(torch.zeros(N, 2, 3, device="cuda"))
    torch.cuda.synchronize()
    for k, t in zip(keep, (traj.obs, traj.reward, traj.done, traj.actions, traj.logp, traj.value)):
        assert same_bits(k, t), "a following step changed the returned tensors"
    assert obs2.data_ptr() != traj.packed.data_ptr()
    # a reset BELOW the wrapper: the observation the wrapper holds is not used, the rollout starts from the engine's own buffer
    env.env.reset()
    fresh = env.env.engine.tensor(abi.T_WRAPPER_OBS).clone()
    assert not same_bits(fresh, obs2)
    assert same_bits(env.rollout(2).obs[0], fresh)
    env.close()


def test_rollout_refused_while_recording(gate_cfg_restored):
    env = _gate_env(2, record_video=True)
    actor, critic, log_std = _modules(1)
    env.set_actor(actor, critic, log_std=log_std)
    env.reset()
    env.start_recording()
    with pytest.raises(NotImplementedError, match="recording"):
        env.rollout(2)
    env.pause_recording()
    assert env.rollout(2).actions.shape == (2, 2, 2, 3)
    env.close()


def test_openrl_rollout_torch_has_gain_one_half(gate_cfg_restored):
    from openrl_ws.utils import mqe_openrl_wrapper
    N, T = 4, 6
    actor, critic, log_std = _modules(2)
    log_std = log_std + 1.0                  # wide enough that 0.5 * a leaves [-1, 1] now and then: the clip is part of the check
    w = mqe_openrl_wrapper(_gate_env(N))
    w.set_actor(actor, critic, log_std=log_std)
    w.env.reset()
    t1 = w.rollout_torch(T)
    twin = _gate_env(N)
    twin.set_actor(actor, critic, log_std=log_std, action_gain=0.5)
    twin.reset()
    t2 = twin.rollout(T)
    assert _traj_equal(t1, t2)
    assert bool((t1.actions.abs() > 2).any())
    # and it is what step_torch does with the same actions
    ws = mqe_openrl_wrapper(_gate_env(N))
    assert same_bits(ws.env.reset(), t1.obs[0])
    for t in range(T):
        o, rew, done = ws.step_torch(t1.actions[t])
        assert same_bits(o, t1.obs[t + 1]) and same_bits(rew[..., 0], t1.reward[t]) and torch.equal(done[:, 0], t1.done[t]), t
    for e in (w, twin, ws):
        e.close()
