"""-m gpu: on-device GAE (mqe_rollout_time_outs, mqe_gae; csrc/kernels_gae.hpp; HipEngine.rollout(time_outs=True) / gae,
FusedTaskWrapper.rollout(gamma=...)): (1) k_gae on synthetic trajectories against float64 within the derived bounds; (2) every element
written, nothing beyond, inputs untouched; (3) normalisation; (4) the time-out record of a real rollout; (5) shards; (6) every refusal;
(7) the public surface."""
import ctypes as C

import numpy as np
import pytest
import torch

import gae_ref as ref
from helpers import make_desc, hip_engine
from mqe.engine import abi
from test_rollout_gpu import (bits, same_bits, engine, install, _traj_equal, _gate_env, _modules, gate_cfg_restored)  # noqa: F401

pytestmark = pytest.mark.gpu

EPS32 = ref.EPS32
_HANDLES, _SYNTH = {}, {}


def handle(N):
    """any small go1gate engine with this N (A' = 2, D = 16): mqe_gae takes the shapes from it and nothing else"""
    if N not in _HANDLES:
        d, k, _ = make_desc("go1gate", N)
        _HANDLES[N] = hip_engine(d, k)
    return _HANDLES[N]


def synth(shape):
    """the shared synthetic trajectory of a shape (host side: made once, never changed)"""
    if shape not in _SYNTH:
        N, Aw, T = shape
        _SYNTH[shape] = ref.synth(N, Aw, T, 16, seed=1000 + 7 * N + T)
    return _SYNTH[shape]


def upload(s, dev):
    """fresh device images of a synthetic trajectory: {name: tensor}; packed / adv / ret / stats carry their guards"""
    t = {k: torch.from_numpy(s[k].copy()).to(dev) for k in ("packed", "adv", "ret", "stats", "value", "time_outs")}
    t["value"] = t["value"].contiguous()
    return t


def call(eng, s, t, gamma, lam, with_to, flags=0, want_stats=False, **kw):
    a = dict(h=eng.h, T=s["T"], packed=t["packed"].data_ptr(), stride=s["stride"], value=t["value"].data_ptr(),
             to=t["time_outs"].data_ptr() if with_to else None, gamma=gamma, lam=lam, flags=flags, adv=t["adv"].data_ptr(), ret=t["ret"].data_ptr(),
             stats=t["stats"].data_ptr() if want_stats else None)
    a.update(kw)
    return eng.lib.mqe_gae(a["h"], a["T"], a["packed"], a["stride"], a["value"], a["to"], a["gamma"], a["lam"], a["flags"], a["adv"], a["ret"], a["stats"],
                        eng._stream())


def outputs(s, t):
    n = s["T"] * s["R"]
    f = lambda x: x[:n].view(torch.float32).cpu().numpy().reshape(s["T"], s["N"], s["Aw"])
    return f(t["adv"]), f(t["ret"])


def reference(s, gamma, lam, with_to):
    adv64, ret64 = ref.gae(s["reward"], s["value"], s["done"], s["time_outs"] if with_to else None, gamma, lam)
    return adv64, ret64, ref.tolerances(s["reward"], s["value"], adv64, gamma, lam)


# ---- 1. synthetic against float64 -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_to", [True, False], ids=["to", "noto"])
@pytest.mark.parametrize("gamma,lam", ref.GAMMA_LAM)
@pytest.mark.parametrize("shape", ref.SHAPES, ids=str)
def test_synthetic_against_float64(shape, gamma, lam, with_to):
    """|adv - adv64| <= tol_adv, |ret - ret64| <= tol_ret with the bounds DERIVED in gae_ref.tolerances: a step has four float32 roundings
    (rr, the inner fmaf, the subtraction, the fmaf into adv), each at most 2^-24 times the magnitude it rounds, all bounded by B = max over
    (t, r) of |reward| + 2 gamma |v| + gamma |vn| + |v| + gamma lam |adv64[t+1]| + |adv64[t]| from the float64 run; an error made at step t
    reaches step t - k scaled by (gamma lam)^k: tol_adv = 4 2^-24 B sum_{k<T} (gamma lam)^k, tol_ret = tol_adv + 2^-24 max(|adv64| + |v|).
    tests/test_gae.py shows that a float32 numpy evaluation meets them and that wrong recursions miss them by > 100x.  Shapes: 66 rows = one
    wavefront and two lanes, 128 = two full ones, T = 12 / 300 wrap the 8-step batches with a remainder, T = 16 is two exact batches,
    T < 8 is a single partial one.  Measured maxima: profiles/gae.txt."""
    s = synth(shape)
    eng = handle(shape[0])
    t = upload(s, eng.torch_device)
    rc = call(eng, s, t, gamma, lam, with_to)
    torch.cuda.synchronize()
    assert rc == 0, eng.lib.mqe_last_error().decode()
    adv, ret = outputs(s, t)
    adv64, ret64, (tol_adv, tol_ret) = reference(s, gamma, lam, with_to)
    dev_adv, dev_ret = float(np.abs(adv - adv64).max()), float(np.abs(ret - ret64).max())
    print(f"gae_kernel {shape} gamma {gamma} lam {lam} to {int(with_to)}: adv {dev_adv:.3e} (tol {tol_adv:.3e}) ret {dev_ret:.3e} (tol {tol_ret:.3e})")
    assert np.isfinite(adv).all() and np.isfinite(ret).all()
    assert dev_adv <= tol_adv and dev_ret <= tol_ret


# ---- 2. every element written, nothing beyond -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, abi.GAE_NORMALIZE], ids=["plain", "normalize"])
@pytest.mark.parametrize("shape", [(3, 2, 5), (33, 2, 7), (64, 2, 9), (2, 2, 300)], ids=str)
def test_every_element_written_nothing_beyond(shape, flags):
    s = synth(shape)
    eng = handle(shape[0])
    t = upload(s, eng.torch_device)
    rc = call(eng, s, t, 0.99, 0.95, True, flags=flags, want_stats=bool(flags))
    torch.cuda.synchronize()
    assert rc == 0, eng.lib.mqe_last_error().decode()
    n = s["T"] * s["R"]
    for name in ("adv", "ret"):
        assert bool((t[name][n:] == ref.SENT).all()), f"{name}: guard elements touched"
        assert not bool((t[name][:n] == ref.SENT).any()), f"{name}: an element was left unwritten"
        assert bool(torch.isfinite(t[name][:n].view(torch.float32)).all())
    assert bool((t["stats"][2:] == ref.SENT).all())
    assert bool((t["stats"][:2] == ref.SENT).all()) == (flags == 0), "stats: written by normalising calls only"
    # inputs bit-identical afterwards; the image holds the stride padding and the guard behind the last row
    assert np.array_equal(t["packed"].cpu().numpy(), s["packed"]), "packed (padding and guard included) changed"
    assert np.array_equal(t["value"].cpu().numpy().view(np.int32), s["value"].view(np.int32))
    assert np.array_equal(t["time_outs"].cpu().numpy(), s["time_outs"])


# ---- 3. normalisation ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 2, 1), (3, 2, 5), (33, 2, 7), (64, 2, 9), (2, 2, 300)], ids=str)
def test_normalisation(shape):
    """stats = (mean, std) of the advantages: the moments are accumulated in f64 from the float32 advantages, so against float64 numpy
    moments (unbiased std) of those float32 values what remains is the f32 store: held to 2^-20 relative.  Against the float64 recursion the
    mean may differ by the mean of the advantages' errors, <= tol_adv, plus its store, and the std by the errors' own std, <=
    sqrt(n / (n - 1)) tol_adv <= sqrt(2) tol_adv, plus its store.  Normalised advantages against (adv64 - mean64) /
    (std64 + 1e-8): tol_adv / std64 plus two roundings of the normalised value.  ret: bit for bit the un-normalised call's; two calls: the
    same bits.  (1, 2, 1) is T x R' = 2, the smallest batch a std exists for."""
    gamma, lam = 0.99, 0.95
    s = synth(shape)
    eng = handle(shape[0])
    plain, a, b = (upload(s, eng.torch_device) for _ in range(3))
    assert call(eng, s, plain, gamma, lam, True) == 0
    assert call(eng, s, a, gamma, lam, True, flags=abi.GAE_NORMALIZE, want_stats=True) == 0, eng.lib.mqe_last_error().decode()
    assert call(eng, s, b, gamma, lam, True, flags=abi.GAE_NORMALIZE, want_stats=True) == 0
    torch.cuda.synchronize()
    for name in ("adv", "ret", "stats"):
        assert torch.equal(a[name], b[name]), f"{name}: two normalising calls differ"
    assert torch.equal(a["ret"], plain["ret"]), "ret must come from the un-normalised advantage"
    adv32, _ = outputs(s, plain)
    norm, _ = outputs(s, a)
    mean, std = (float(x) for x in a["stats"][:2].view(torch.float32).cpu())
    m32, s32 = float(adv32.astype(np.float64).mean()), float(adv32.astype(np.float64).std(ddof=1))
    adv64, _, (tol_adv, _) = reference(s, gamma, lam, True)
    m64, s64 = float(adv64.mean()), float(adv64.std(ddof=1))
    want = (adv64 - m64) / (s64 + 1e-8)
    tol_norm = tol_adv / s64 + 2 * EPS32 * float(np.abs(want).max())
    dev = float(np.abs(norm - want).max())
    print(f"gae_normalize {shape}: mean {mean:.8g} (f64 of f32 adv {m32:.8g}, f64 {m64:.8g}) std {std:.8g} ({s32:.8g}, {s64:.8g}) "
          f"normalised adv dev {dev:.3e} (tol {tol_norm:.3e})")
    assert abs(mean - m32) <= 2.0 ** -20 * abs(m32) and abs(std - s32) <= 2.0 ** -20 * s32
    assert abs(mean - m64) <= tol_adv + EPS32 * abs(m64)
    assert abs(std - s64) <= 2 ** 0.5 * tol_adv + EPS32 * s64
    assert dev <= tol_norm


# ---- 4. the time-out record on a real rollout ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("task,N", [("go1gate", 5), ("go1sheep-hard", 3)])
def test_time_out_record_of_a_real_rollout(task, N):
    T = 12
    A, B, Cc = (engine(task, N, max_episode_length=5) for _ in range(3))
    install(A, "tanh64x64", True, pseed=5)
    install(Cc, "tanh64x64", True, pseed=5)
    for e in (A, B, Cc):
        e.reset_all()
    traj = A.rollout(T, time_outs=True)
    assert traj.time_outs.shape == (T, N) and traj.time_outs.dtype == torch.bool
    for t in range(T):
        B.step(traj.actions[t].contiguous())
        assert torch.equal(traj.time_outs[t].view(torch.uint8), B.tensor(abi.T_TIME_OUT_BUF)), t
    assert bool((traj.time_outs.view(torch.uint8) <= traj.done.view(torch.uint8)).all()), "a time-out is a done"
    assert bool(traj.time_outs.any(dim=0).all()), "every env times out at least once inside the window"
    bare = Cc.rollout(T)
    assert bare.time_outs is None and bare.advantages is None and bare.returns is None and bare.adv_stats is None
    assert _traj_equal(traj, bare), "recording the time-outs changed the trajectory"
    # nothing stays registered: a following rollout without the record leaves the tensor alone
    keep = traj.time_outs.clone()
    A.rollout(T)
    assert torch.equal(keep, traj.time_outs)
    # GAE of the recorded trajectory against float64 from its own tensors
    assert A.gae(traj, 0.99, 0.95) is traj
    torch.cuda.synchronize()
    assert traj.advantages.shape == traj.returns.shape == (T, N, 2) and traj.adv_stats is None
    rew, val = traj.reward.cpu().numpy(), traj.value.cpu().numpy()
    done, to = traj.done.view(torch.uint8).cpu().numpy(), traj.time_outs.view(torch.uint8).cpu().numpy()
    adv64, ret64 = ref.gae(rew, val, done, to, 0.99, 0.95)
    tol_adv, tol_ret = ref.tolerances(rew, val, adv64, 0.99, 0.95)
    dev_adv = float(np.abs(traj.advantages.cpu().numpy() - adv64).max())
    dev_ret = float(np.abs(traj.returns.cpu().numpy() - ret64).max())
    print(f"gae_rollout {task}: adv {dev_adv:.3e} (tol {tol_adv:.3e}) ret {dev_ret:.3e} (tol {tol_ret:.3e})")
    assert dev_adv <= tol_adv and dev_ret <= tol_ret
    for e in (A, B, Cc):
        e.close()


# ---- 5. shards -------------------------------------------------------------------------------------------------------------------------------
def test_a_shard_reproduces_its_rows():
    T = 8
    full, part = engine("go1gate", 4, max_episode_length=5), engine("go1gate", 2, max_episode_length=5, env_id_offset=2)
    for e in (full, part):
        install(e, "tanh64x64", True, pseed=13)
        e.reset_all()
    f, p = full.gae(full.rollout(T, time_outs=True), 0.99, 0.95), part.gae(part.rollout(T, time_outs=True), 0.99, 0.95)
    assert same_bits(f.time_outs[:, 2:4], p.time_outs) and bool(p.time_outs.any())
    assert same_bits(f.advantages[:, 2:4], p.advantages) and same_bits(f.returns[:, 2:4], p.returns)
    assert not same_bits(f.advantages[:, 0:2], p.advantages)
    full.close(); part.close()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_of_mqe_gae():
    shape = (3, 2, 5)
    s = synth(shape)
    eng = handle(3)
    t = upload(s, eng.torch_device)
    image = {k: v.clone() for k, v in t.items()}
    n4 = s["T"] * s["R"] * 4

    def refused(code, word, **kw):
        rc = call(eng, s, t, kw.pop("gamma", 0.99), kw.pop("lam", 0.95), True, want_stats=True, **kw)
        msg = eng.lib.mqe_last_error().decode()
        torch.cuda.synchronize()
        assert rc == code and msg and word in msg, (kw, rc, msg)
        for k in t:
            assert torch.equal(t[k].view(torch.uint8), image[k].view(torch.uint8)), (kw, k, "a refused call wrote into the buffers")

    p = lambda name, off=0: t[name].data_ptr() + off
    refused(-1, "null", h=None)
    for name in ("packed", "value", "adv", "ret"):
        refused(-1, "required", **{name: None})
    for T in (0, -2, abi.ROLLOUT_MAX_STEPS + 1):
        refused(-6, "T must", T=T)
    refused(-6, "row_stride", stride=(s["pf"] + 3) // 4 * 4 - 4)          # a multiple of 4, too small
    refused(-6, "row_stride", stride=s["stride"] + 1)                      # large enough, not a multiple of 4
    for name in ("packed", "value", "adv", "ret", "stats"):
        refused(-6, "misaligned", **{name: p(name, 2)})
    for bad in (-0.01, 1.01, float("nan")):
        refused(-6, "gamma", gamma=bad)
        refused(-6, "lam", lam=bad)
    refused(-6, "flags", flags=2)
    refused(-6, "flags", flags=abi.GAE_NORMALIZE | 4)
    refused(-6, "adv_dev", adv=p("value", 4))                              # an output inside an input
    refused(-6, "ret_dev", ret=p("packed", 4 * s["stride"]))
    refused(-6, "adv_dev", adv=p("time_outs") & ~3)
    refused(-6, "adv_dev", adv=p("ret", n4 - 4))                           # the two outputs share one element
    refused(-6, "stats_dev", stats=p("value"))
    refused(-6, "ret_dev", ret=p("stats") - n4 + 4)                        # ret's last element is stats[0]
    one = handle(1)                                                        # R' = 2: T = 1 is 2 values (test 3), nothing smaller exists at A' = 2
    rc = call(one, synth((1, 2, 1)), upload(synth((1, 2, 1)), one.torch_device), 0.99, 0.95, True, flags=abi.GAE_NORMALIZE)
    assert rc == 0
    # the same call with nothing wrong then succeeds
    assert call(eng, s, t, 0.99, 0.95, True, want_stats=True) == 0, eng.lib.mqe_last_error().decode()
    torch.cuda.synchronize()
    assert not bool((t["adv"][:n4 // 4] == ref.SENT).any()) and bool((t["stats"] == ref.SENT).all())


def test_normalize_needs_two_values():
    """T x R' < 2 needs a scene with one agent row: go1plane's N = 1 has R' = 1"""
    d, k, _ = make_desc("go1plane", 1)
    eng = hip_engine(d, k)
    N, Aw, D = (int(x) for x in eng.tensor(abi.T_WRAPPER_OBS).shape)
    assert N * Aw == 1
    s = ref.synth(1, 1, 1, D, seed=3)
    t = upload(s, eng.torch_device)
    assert call(eng, s, t, 0.99, 0.95, True, flags=abi.GAE_NORMALIZE, want_stats=True) == -6
    assert "T x R'" in eng.lib.mqe_last_error().decode()
    torch.cuda.synchronize()
    assert bool((t["adv"] == ref.SENT).all()) and bool((t["ret"] == ref.SENT).all()) and bool((t["stats"] == ref.SENT).all())
    assert call(eng, s, t, 0.99, 0.95, True) == 0
    torch.cuda.synchronize()
    adv64, _ = ref.gae(s["reward"], s["value"], s["done"], s["time_outs"], 0.99, 0.95)
    assert abs(float(t["adv"][:1].view(torch.float32)) - float(adv64.ravel()[0])) <= 1e-5
    eng.close()


def test_refusals_of_the_time_out_record():
    from test_rollout_gpu import _buffers, _is_sent
    N, T = 3, 4
    eng = engine("go1gate", N)
    install(eng, "tanh7", True, pseed=1)
    eng.reset_all()
    reg = eng.lib.mqe_rollout_time_outs
    rec = torch.full((T * N + 64,), 0x5A, dtype=torch.uint8, device=eng.torch_device)
    assert reg(None, rec.data_ptr(), T) == -1 and eng.lib.mqe_last_error().decode()
    for cap in (0, -1):
        assert reg(eng.h, rec.data_ptr(), cap) == -6 and "capacity_steps" in eng.lib.mqe_last_error().decode()
    assert reg(eng.h, rec.data_ptr(), T - 1) == 0
    f = eng.lib.mqe_rollout
    r, flat = _buffers(eng, T)
    p = lambda x: C.c_void_p(x.data_ptr())
    args = (eng.h, T, None, p(r.packed), int(r.packed.stride(0)), p(r.actions), p(r.logp), p(r.value), 0)
    before = eng.tensor(abi.T_ROOT_STATE).clone()
    assert f(*args, eng._stream()) == -6 and "capacity_steps" in eng.lib.mqe_last_error().decode()
    torch.cuda.synchronize()
    assert all(bool(_is_sent(x).all()) for x in flat.values()) and bool((rec == 0x5A).all()), "a refused rollout wrote something"
    assert same_bits(before, eng.tensor(abi.T_ROOT_STATE)), "a refused rollout stepped"
    assert reg(eng.h, rec.data_ptr(), T) == 0
    assert f(*args, eng._stream()) == 0, eng.lib.mqe_last_error().decode()
    torch.cuda.synchronize()
    assert bool((rec[:T * N] <= 1).all()) and bool((rec[T * N:] == 0x5A).all()), "the record is T x N flags, nothing beyond"
    assert reg(eng.h, None, 0) == 0                                        # removed: the next rollout leaves the record alone
    rec.fill_(0x5A)
    assert f(*args, eng._stream()) == 0
    torch.cuda.synchronize()
    assert bool((rec == 0x5A).all())
    # HipEngine.rollout unregisters its record when the library refuses the call too (here: inside an open step)
    r2, _ = _buffers(eng, T)
    r2.time_outs = rec[:T * N].view(T, N)

    def inside():
        with pytest.raises(RuntimeError, match=r"mqe_rollout failed \(-8\)"):
            eng.rollout(T, out=r2, time_outs=True)
    eng.step(torch.zeros(N, 2, 3, device=eng.torch_device), between=inside)
    assert eng.rollout(T).time_outs is None
    torch.cuda.synchronize()
    assert bool((rec == 0x5A).all()), "the record of a refused call stayed registered"
    assert eng.rollout(T, out=r2, time_outs=True) is r2
    torch.cuda.synchronize()
    assert bool((rec[:T * N] <= 1).all()) and bool((rec[T * N:] == 0x5A).all())
    eng.close()


# ---- 7. the public surface ------------------------------------------------------------------------------------------------------------------
def test_public_surface(gate_cfg_restored):  # noqa: F811
    N, T = 4, 8
    env = _gate_env(N)
    actor, critic, log_std = _modules(0)
    env.set_actor(actor, critic, log_std=log_std)
    env.reset()
    bare = env.rollout(T)
    assert bare.time_outs is None and bare.advantages is None and bare.returns is None and bare.adv_stats is None
    traj = env.rollout(T, gamma=0.99, lam=0.95, normalize_advantages=True)
    torch.cuda.synchronize()
    assert traj.time_outs.shape == (T, N) and traj.time_outs.dtype == torch.bool
    assert traj.advantages.shape == traj.returns.shape == (T, N, 2) and traj.advantages.dtype == torch.float32
    assert traj.adv_stats.shape == (2,) and same_bits(traj.obs[0], bare.obs[T])
    rew, val = traj.reward.cpu().numpy(), traj.value.cpu().numpy()
    done, to = traj.done.view(torch.uint8).cpu().numpy(), traj.time_outs.view(torch.uint8).cpu().numpy()
    adv64, ret64 = ref.gae(rew, val, done, to, 0.99, 0.95)
    tol_adv, tol_ret = ref.tolerances(rew, val, adv64, 0.99, 0.95)
    assert float(np.abs(traj.returns.cpu().numpy() - ret64).max()) <= tol_ret
    mean, std = (float(x) for x in traj.adv_stats.cpu())
    assert abs(mean - adv64.mean()) <= tol_adv + EPS32 * abs(adv64.mean())
    want = (adv64 - adv64.mean()) / (adv64.std(ddof=1) + 1e-8)
    assert float(np.abs(traj.advantages.cpu().numpy() - want).max()) <= tol_adv / adv64.std(ddof=1) + 2 * EPS32 * float(np.abs(want).max())
    # HipEngine.gae: what it refuses before it hands raw pointers to the library
    eng = env.env.engine
    good = eng.gae(traj, 0.99)
    assert good is traj and traj.adv_stats is None
    for field, bad in (("advantages", traj.advantages.transpose(1, 2)), ("returns", traj.returns.double()), ("advantages", traj.advantages[:, :, :1])):
        holder = type("Out", (), dict(advantages=traj.advantages, returns=traj.returns, adv_stats=None))()
        setattr(holder, field, bad)
        with pytest.raises(ValueError, match=f"out.{field}"):
            eng.gae(traj, 0.99, out=holder)
    adv_ptr = traj.advantages.data_ptr()
    assert eng.gae(traj, 0.99, out=traj).advantages.data_ptr() == adv_ptr
    value, traj.value = traj.value, None
    with pytest.raises(ValueError, match="traj.value is None"):
        eng.gae(traj, 0.99)
    traj.value = value
    # an actor without a critic: refused before anything is enqueued
    env.set_actor(actor, None, log_std=log_std)
    count0, steps0, common0 = env.reward_buffer["step count"], env.env._steps_policy, env.env.common_step_counter
    root0 = eng.tensor(abi.T_ROOT_STATE).clone()
    with pytest.raises(ValueError, match="critic"):
        env.rollout(T, gamma=0.99)
    assert (env.reward_buffer["step count"], env.env._steps_policy, env.env.common_step_counter) == (count0, steps0, common0)
    assert same_bits(root0, eng.tensor(abi.T_ROOT_STATE))
    assert env.rollout(2).value is None
    env.close()


def test_openrl_rollout_torch_passes_the_keywords(gate_cfg_restored):  # noqa: F811
    from openrl_ws.utils import mqe_openrl_wrapper
    N, T = 4, 6
    actor, critic, log_std = _modules(2)
    w = mqe_openrl_wrapper(_gate_env(N))
    w.set_actor(actor, critic, log_std=log_std)
    w.env.reset()
    t1 = w.rollout_torch(T, gamma=0.98, lam=0.9, normalize_advantages=True)
    twin = _gate_env(N)
    twin.set_actor(actor, critic, log_std=log_std, action_gain=0.5)
    twin.reset()
    t2 = twin.rollout(T, gamma=0.98, lam=0.9, normalize_advantages=True)
    assert _traj_equal(t1, t2)
    for name in ("time_outs", "advantages", "returns", "adv_stats"):
        assert same_bits(getattr(t1, name), getattr(t2, name)), name
    t3 = w.rollout_torch(T)
    assert t3.advantages is None and t3.time_outs is None
    for e in (w, twin):
        e.close()
