"""-m gpu: the recurrent actor-critic inside the engine's rollout (MQE_ACTOR_RECURRENT, MQE_ROLLOUT_HIDDEN_IN / _RECORD; csrc/kernels_gru.hpp:
k_actor_gru, k_actor_gru_ln; HipEngine.create_actor(recurrent=True) / rollout(hidden=, record_hidden=)): (1) one step against float64, held to
4x the error of a float32 CPU evaluation of the same RecurrentMLP; (2) twelve recorded stochastic steps: every step from the engine's own
state, the draws, logp over chunks, the reset on done; (3) continuation, checkpoint, determinism, shards; (4) memory; (5) refusals; (6) the task wrapper's surface.
go1gate with 37 envs = 74 rows: one full workgroup and one partial; max_episode_length=5: every env resets inside a 12-step window."""
import ctypes as C
import types

import pytest
import torch

import gru_ref as ref
import rollout_ref
from mqe.engine import abi
from mqe.engine.hip_engine import Rollout
from test_rollout_gpu import _gate_env, _is_sent, _sentinel, engine, gate_cfg_restored, same_bits, sampling_tolerances  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

N, AW, D = 37, 2, 16
_CACHE = {}


def install(eng, name, seed=0):
    """create the recurrent actor of shape `name` with seeded parameters; -> (actor, critic or None, log_std) float32 on the host"""
    (actor, critic, log_std), kw = ref.nets_of(name, D, seed)
    eng.create_actor(kw.pop("actor_dims"), kw.pop("critic_dims"), **kw)
    flat = ref.flat_params(actor, critic, log_std)
    views = eng.actor_params()
    assert views["flat"].numel() == flat.numel()
    views["flat"].copy_(flat)
    return actor, critic, log_std


def hidden_width(actor, critic):
    return actor.rnn.hidden_size + (critic.rnn.hidden_size if critic is not None else 0)


# ---- 1. one step against float64 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ref.SHAPES))
def test_one_step_against_float64(name):
    """A deterministic step from a random state given through hidden=: the means, the value and row 1's tail may deviate from the float64
    RecurrentMLP by at most 4x the maximum deviation of its float32 CPU evaluation on the same inputs (tests/test_rollout_gpu.py test 1's form)."""
    eng = engine("go1gate", N, max_episode_length=5)
    actor, critic, _ = install(eng, name, seed=len(name))
    a64, c64 = ref.doubles(actor, critic)
    eng.reset_all()
    Hs = hidden_width(actor, critic)
    assert eng.hidden_width() == Hs
    h0 = torch.randn(N, AW, Hs, generator=torch.Generator().manual_seed(5))
    traj = eng.rollout(1, deterministic=True, hidden=h0.cuda(), record_hidden=True)
    torch.cuda.synchronize()
    assert traj.hidden.shape == (2, N, AW, Hs) and torch.equal(traj.hidden[0].cpu(), h0), "row 0's tail is the state the call started from"
    e = ref.yardstick(actor, critic, a64, c64, traj.obs[0].cpu(), h0, None)
    dev_mean = float((traj.actions[0].cpu().double() - e["mean64"]).abs().max())
    dev_hid = float((traj.hidden[1].cpu().double() - e["hidden64"]).abs().max())
    print(f"gru_step {name} mean: kernel {dev_mean:.3e} torch-f32 {e['yard_mean']:.3e} hidden: kernel {dev_hid:.3e} torch-f32 {e['yard_hidden']:.3e}", end="")
    if critic is not None:
        dev_value = float((traj.value[0].cpu().double() - e["value64"]).abs().max())
        print(f" value: kernel {dev_value:.3e} torch-f32 {e['yard_value']:.3e}")
        assert dev_value <= 4 * e["yard_value"], (dev_value, e["yard_value"])
    else:
        print()
        assert traj.value is None
    assert dev_mean <= 4 * e["yard_mean"], (dev_mean, e["yard_mean"])
    assert dev_hid <= 4 * e["yard_hidden"], (dev_hid, e["yard_hidden"])
    eng.close()


# ---- 2. twelve steps, recorded, stochastic --------------------------------------------------------------------------------------------------------------
def recorded(name="b_tanh64x64_norms", seed=11, T=12):
    """one recorded stochastic rollout per shape, shared by the tests that read it: host copies only"""
    key = (name, seed, T)
    if key not in _CACHE:
        eng = engine("go1gate", N, seed=seed, max_episode_length=5)
        actor, critic, log_std = install(eng, name, seed=3)
        eng.reset_all()
        traj = eng.rollout(T, record_hidden=True)
        torch.cuda.synchronize()
        _CACHE[key] = dict(actor=actor, critic=critic, log_std=log_std, obs=traj.obs.cpu(), done=traj.done.cpu(), hidden=traj.hidden.cpu(), actions=traj.actions.cpu(),
                           logp=traj.logp.cpu(), value=traj.value.cpu() if traj.value is not None else None, next_hidden=traj.next_hidden().cpu(), seed=seed, T=T)
        eng.close()
    return _CACHE[key]


@pytest.mark.parametrize("name", ["b_tanh64x64_norms", "a_tanh7_5"])
def test_twelve_recorded_steps(name):
    r = recorded(name)
    T, actor, critic = r["T"], r["actor"], r["critic"]
    a64, c64 = ref.doubles(actor, critic)
    done = r["done"]
    assert bool(done.any(dim=0).all()), "every env resets at least once inside the window"
    assert torch.equal(r["hidden"][0], torch.zeros_like(r["hidden"][0])), "a fresh actor starts from the zero state"
    mean64 = []
    worst = dict(mean=0.0, hidden=0.0, value=0.0)
    for t in range(T):
        # every step from the engine's own hidden[t], done bytes and observation: nothing compounds
        prev = done[t - 1] if t > 0 else None
        e = ref.yardstick(actor, critic, a64, c64, r["obs"][t], r["hidden"][t], prev)
        mean64.append(e["mean64"])
        dev_h = float((r["hidden"][t + 1].double() - e["hidden64"]).abs().max())
        dev_v = float((r["value"][t].double() - e["value64"]).abs().max())
        worst = dict(mean=max(worst["mean"], e["yard_mean"]), hidden=max(worst["hidden"], dev_h / e["yard_hidden"]), value=max(worst["value"], dev_v / e["yard_value"]))
        assert dev_h <= 4 * e["yard_hidden"], (t, dev_h, e["yard_hidden"])
        assert dev_v <= 4 * e["yard_value"], (t, dev_v, e["yard_value"])
        if prev is not None and bool(prev.any()):
            # rows whose env was done enter the step from a state that is bitwise zero: the reference step from zero gives the same result as the
            # reference step from the masked state, and the kernel's next state is inside its bound of it
            zero = r["hidden"][t].clone()
            zero[prev] = 0.0
            z = ref.step(a64, c64, r["obs"][t], zero, None)
            assert float((z[2][prev] - e["hidden64"][prev]).abs().max()) <= 1e-12 and float((z[0][prev] - e["mean64"][prev]).abs().max()) <= 1e-12
            assert float((r["hidden"][t + 1][prev].double() - z[2][prev]).abs().max()) <= 4 * e["yard_hidden"]
            assert float(r["hidden"][t][prev].abs().max()) > 0, "the recorded state is unmasked: the mask is in the row's done bytes"
    # value[T]: the critic from the masked state of row T
    eT = ref.yardstick(actor, critic, a64, c64, r["obs"][T], r["hidden"][T], done[T - 1])
    assert float((r["value"][T].double() - eT["value64"]).abs().max()) <= 4 * eT["yard_value"]
    want_next = r["hidden"][T].clone()
    want_next[done[T - 1]] = 0.0                     # exactly 0.0f, never -0.0f
    assert same_bits(r["next_hidden"], want_next)
    # the draws: actions - mean = exp(log_std) z with z from the host twin of the counter RNG (tests/test_rollout_gpu.py derives the tolerance)
    mean64 = torch.stack(mean64)
    a = r["actions"].double()
    std = torch.exp(r["log_std"].double())
    z = ((a - mean64) / std).numpy()
    twin = rollout_ref.actor_draws(r["seed"], 0, N, AW, 0, T)
    tol_z, tol_lp = sampling_tolerances(worst["mean"], float(a.abs().max()), float(std.min()), float(abs(twin).max()))
    dev_z = float(abs(z - twin).max())
    print(f"gru_rollout {name}: z kernel-vs-twin {dev_z:.3e} tol {tol_z:.3e}; hidden {worst['hidden']:.2f} x yardstick, value {worst['value']:.2f} x")
    assert dev_z <= tol_z
    # logp against RecurrentMLP.evaluate walked over chunks of 4 from hidden[0], hidden[4], hidden[8] with the recorded masks: a learner's
    # first-epoch ratio is 1
    Ha = actor.rnn.hidden_size
    masks = torch.cat([torch.ones(1, N), (~done[:-1]).double()])[:, :, None, None].expand(T, N, AW, 1)
    lp = []
    for t0 in (0, 4, 8):
        with torch.no_grad():
            m, _ = a64.evaluate(r["obs"][t0:t0 + 4].double(), r["hidden"][t0][..., :Ha].double(), masks[t0:t0 + 4])
        lp.append(rollout_ref.gaussian_logp(a[t0:t0 + 4], m, r["log_std"].double()))
    dev_lp = float((r["logp"].double() - torch.cat(lp)).abs().max())
    print(f"gru_rollout {name}: logp over chunks dev {dev_lp:.3e} tol {tol_lp:.3e}")
    assert dev_lp <= tol_lp


# ---- 3. continuation, checkpoint, determinism, shards ---------------------------------------------------------------------------------------------------
def _same(a, b, rows=slice(None)):
    return (same_bits(a.actions[:, rows], b.actions) and same_bits(a.logp[:, rows], b.logp) and same_bits(a.value[:, rows], b.value)
            and same_bits(a.hidden[:, rows], b.hidden) and same_bits(a.obs[:, rows], b.obs) and same_bits(a.done[:, rows], b.done))


def _cat(x, y):
    """two consecutive trajectories as one: row 0 of the second repeats row T of the first (its tail: masked, where the first holds it unmasked)"""
    c = lambda a, b: torch.cat([a, b])
    return types.SimpleNamespace(actions=c(x.actions, y.actions), logp=c(x.logp, y.logp), done=c(x.done, y.done), value=c(x.value[:-1], y.value),
                                 obs=c(x.obs[:-1], y.obs), hidden=c(x.hidden, y.hidden[1:]))


def test_continuation_checkpoint_and_determinism():
    name, T = "b_tanh64x64_norms", 12
    A, B, Cc = (engine("go1gate", N, seed=4, max_episode_length=5) for _ in range(3))
    for e in (A, B, Cc):
        install(e, name, seed=2)
        e.reset_all()
    whole, again = A.rollout(T, record_hidden=True), Cc.rollout(T, record_hidden=True)
    assert _same(whole, again), "two runs give the same bits"
    first = B.rollout(6, record_hidden=True)
    # the live state behind a call is row T's tail, masked: the second half starts from it without hidden=
    second = B.rollout(6, record_hidden=True)
    assert same_bits(second.hidden[0], first.next_hidden())
    assert _same(whole, _cat(first, second)), "rollout(6) + rollout(6) is rollout(12), bit for bit"
    # the same with the cut behind the first step that ended an episode, so that the call boundary masks: the live state of a done env is bitwise +0.0f
    k = int(whole.done.any(dim=1).nonzero()[0]) + 1
    assert 1 <= k < T, "an episode ends inside the window, before its last step"
    G = engine("go1gate", N, seed=4, max_episode_length=5)
    install(G, name, seed=2)
    G.reset_all()
    g1, g2 = G.rollout(k, record_hidden=True), G.rollout(T - k, record_hidden=True)
    ended = g1.done[k - 1]
    assert bool(ended.any()), "the check below bites"
    assert bool((g2.hidden[0][ended].view(torch.int32) == 0).all()) and bool((g1.hidden[k][ended] != 0).any())
    assert same_bits(g2.hidden[0][~ended], g1.hidden[k][~ended]) and same_bits(g2.hidden[0], g1.next_hidden())
    assert _same(whole, _cat(g1, g2))
    G.close()
    # the same after save_state / load_state into a fresh handle with hidden=traj.next_hidden()
    Dd, E = engine("go1gate", N, seed=4, max_episode_length=5), engine("go1gate", N, seed=4, max_episode_length=5)
    install(Dd, name, seed=2); install(E, name, seed=2)
    Dd.reset_all()
    size_before = int(E.lib.mqe_state_size(E.h))
    half = Dd.rollout(6, record_hidden=True)
    blob = Dd.save_state()
    E.load_state(blob)
    rest = E.rollout(6, obs0=half.obs[6].contiguous(), hidden=half.next_hidden().contiguous(), record_hidden=True)
    assert same_bits(rest.hidden[0], half.next_hidden())
    assert _same(whole, _cat(half, rest)), "a checkpointed rollout continues bit for bit in a fresh handle"
    assert int(E.lib.mqe_state_size(E.h)) == size_before
    # an unrecorded run leaves the same live state and the same samples
    F = engine("go1gate", N, seed=4, max_episode_length=5)
    install(F, name, seed=2)
    F.reset_all()
    plain = F.rollout(T)
    assert plain.hidden is None and same_bits(plain.actions, whole.actions) and same_bits(plain.value, whole.value)
    nxt_f, nxt_a = F.rollout(1, record_hidden=True), A.rollout(1, record_hidden=True)
    assert same_bits(nxt_f.hidden, nxt_a.hidden) and same_bits(nxt_f.hidden[0], whole.next_hidden())
    for e in (A, B, Cc, Dd, E, F):
        e.close()


def test_a_shard_reproduces_its_rows():
    T = 8
    full, part = engine("go1gate", 4, max_episode_length=5), engine("go1gate", 2, max_episode_length=5, env_id_offset=2)
    for e in (full, part):
        install(e, "a_tanh7_5", seed=13)
        e.reset_all()
    f, p = full.rollout(T, record_hidden=True), part.rollout(T, record_hidden=True)
    assert _same(f, p, rows=slice(2, 4))
    assert not same_bits(f.actions[:, 0:2], p.actions)
    full.close(); part.close()


# ---- 4. memory ------------------------------------------------------------------------------------------------------------------------------------------------
def _buffers(eng, T, width, guard=64):
    dev = eng.torch_device
    flat = dict(packed=_sentinel((T + 1) * width + guard, dev), actions=_sentinel(T * N * AW * 3 + guard, dev), logp=_sentinel(T * N * AW + guard, dev),
                value=_sentinel((T + 1) * N * AW + guard, dev))
    return flat


@pytest.mark.parametrize("record", [False, True])
def test_memory_written(record):
    T = 3
    eng = engine("go1gate", N, max_episode_length=5)
    size0 = int(eng.lib.mqe_state_size(eng.h))
    actor, critic, _ = install(eng, "a_tanh7_5", seed=1)
    assert int(eng.lib.mqe_state_size(eng.h)) == size0, "the recurrent state is the actor's, not the simulation's"
    eng.reset_all()
    Hs = hidden_width(actor, critic)
    p4 = eng.rollout_row_stride()
    n, nr = N * AW * D, N * AW
    pf = n + nr + (N + 3) // 4
    width = p4 + nr * Hs + 8                        # 8 floats of padding behind the tail
    flat = _buffers(eng, T, width)
    r = Rollout(flat["packed"][:(T + 1) * width].view(T + 1, width), flat["actions"][:T * nr * 3].view(T, N, AW, 3), flat["logp"][:T * nr].view(T, N, AW),
                flat["value"][:(T + 1) * nr].view(T + 1, N, AW), (N, AW, D), hidden_width=Hs if record else 0)
    out = eng.rollout(T, out=r, record_hidden=record)
    torch.cuda.synchronize()
    assert out is r
    for name, used in (("packed", r.packed.numel()), ("actions", r.actions.numel()), ("logp", r.logp.numel()), ("value", r.value.numel())):
        assert _is_sent(flat[name][used:]).all(), f"{name}: guard elements touched"
    assert not _is_sent(r.packed[:, :n + nr]).any()
    if not record:
        assert _is_sent(r.packed[:, pf:]).all(), "without record_hidden nothing beyond the packed layout is touched"
    else:
        assert _is_sent(r.packed[:, pf:p4]).all() and _is_sent(r.packed[:, p4 + nr * Hs:]).all(), "the padding in front of and behind the tail is intact"
        tail = r.packed[:, p4:p4 + nr * Hs]
        assert not _is_sent(tail).any() and torch.isfinite(tail).all(), "exactly R' Hs floats per row at offset P4 are written, rows 0 .. T"
        assert r.hidden.shape == (T + 1, N, AW, Hs) and bool((r.hidden[0] == 0).all()) and bool((r.hidden[1:].abs() > 0).any())
    assert int(eng.lib.mqe_state_size(eng.h)) == size0
    eng.close()


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    T = 2
    eng = engine("go1gate", N, max_episode_length=5)
    eng.reset_all()
    p4 = eng.rollout_row_stride()
    nr = N * AW
    Hs = 12
    width = p4 + nr * Hs
    flat = _buffers(eng, T, width)
    flat.update(adv=_sentinel(T * nr, eng.torch_device), ret=_sentinel(T * nr, eng.torch_device), grad=_sentinel(4096, eng.torch_device))
    p = lambda t: C.c_void_p(t.data_ptr() if t is not None else None)

    def refused(code, stride=width, flags=0):
        rc = eng.lib.mqe_rollout(eng.h, T, p(None), p(flat["packed"]), stride, p(flat["actions"]), p(flat["logp"]), p(flat["value"]), flags, eng._stream())
        msg = eng.lib.mqe_last_error().decode()
        torch.cuda.synchronize()
        assert rc == code and msg, (stride, flags, rc, msg)
        for name, t in flat.items():
            assert _is_sent(t).all(), (name, "a refused call wrote into the buffers")
        return msg

    # either flag on a plain handle
    eng.create_actor([D, 7, 3], [D, 5, 1])
    for fl in (abi.ROLLOUT_HIDDEN_IN, abi.ROLLOUT_HIDDEN_RECORD, abi.ROLLOUT_HIDDEN_IN | abi.ROLLOUT_HIDDEN_RECORD | abi.ROLLOUT_DETERMINISTIC):
        assert "flags" in refused(-6, flags=fl)
    with pytest.raises(ValueError, match="need a recurrent actor"):
        eng.rollout(T, record_hidden=True)

    # mqe_actor_create: a one-layer network with the bit, a shape over the LDS rule, bits 8 and 512
    def create_refused(*a, **kw):
        with pytest.raises(RuntimeError, match=r"mqe_actor_create failed \(-6\)") as ei:
            eng.create_actor(*a, **kw)
        return str(ei.value)
    assert "actor_layers" in create_refused([D, 3], [D, 5, 1], recurrent=True)
    assert "critic_layers" in create_refused([D, 7, 3], [D, 1], recurrent=True)
    assert abi.actor_gru_lds_bytes([D, 256, 256, 3], [D, 256, 256, 1]) > abi.GRU_LDS_LIMIT
    assert "width" in create_refused([D, 256, 256, 3], [D, 256, 256, 1], recurrent=True)
    for bit in (8, 512):
        sh = abi.ActorShape(obs_dim=D, act_dim=3, actor_layers=2, activation=bit | abi.ACTOR_RECURRENT, action_gain=1.0)
        for i, v in enumerate([D, 7, 3]):
            sh.actor_dims[i] = v
        assert eng.lib.mqe_actor_create(eng.h, C.byref(sh)) == -6 and "activation" in eng.lib.mqe_last_error().decode()
    # a refused create leaves the plain actor that was there
    assert "flags" in refused(-6, flags=abi.ROLLOUT_HIDDEN_RECORD)

    # a recurrent handle: too small a row_stride with either flag; the old rule without
    eng.create_actor([D, 7, 3], [D, 5, 1], recurrent=True)
    assert eng.hidden_width() == Hs
    for fl in (abi.ROLLOUT_HIDDEN_IN, abi.ROLLOUT_HIDDEN_RECORD):
        assert "row_stride" in refused(-6, stride=width - 4, flags=fl)
        assert "row_stride" in refused(-6, stride=p4, flags=fl)
    narrow = Rollout(torch.zeros(T + 1, p4, device=eng.torch_device), torch.zeros(T, N, AW, 3, device=eng.torch_device), torch.zeros(T, N, AW, device=eng.torch_device),
                     torch.zeros(T + 1, N, AW, device=eng.torch_device), (N, AW, D))
    with pytest.raises(ValueError, match="out.packed rows hold"):
        eng.rollout(T, out=narrow, record_hidden=True)
    # mqe_ppo_grad on a recurrent handle: refused with the reason, nothing written
    loss = abi.PpoLoss(0.2, 1.0, 0.0, 0.0)
    rc = eng.lib.mqe_ppo_grad(eng.h, T, p(flat["packed"]), width, p(flat["actions"]), p(flat["logp"]), p(flat["value"]), p(flat["adv"]), p(flat["ret"]), p(None), 0,
                              T * nr, C.byref(loss), 0, p(flat["grad"]), p(None), eng._stream())
    msg = eng.lib.mqe_last_error().decode()
    torch.cuda.synchronize()
    assert rc == -6 and "back-propagation through time" in msg
    assert all(_is_sent(t).all() for t in flat.values())
    traj = eng.rollout(T, record_hidden=True)
    with pytest.raises(NotImplementedError, match="back-propagation through time"):
        eng.ppo_grad(traj)
    with pytest.raises(NotImplementedError, match="back-propagation through time"):
        eng.ppo_update(traj, epochs=1, minibatches=1, lr=1e-3)
    # gae on a recurrent trajectory works, and so does the optimiser on the cell's parameters
    eng.gae(traj, 0.99)
    torch.cuda.synchronize()
    assert torch.isfinite(traj.advantages).all() and torch.isfinite(traj.returns).all()
    views = eng.actor_params()
    n_params = views["flat"].numel()
    assert n_params == abi.actor_param_count([D, 7, 3], [D, 5, 1], recurrent=True) and eng.optimizer_state()["exp_avg"].numel() == n_params
    before = views["actor.gru.weight_hh"].clone()
    eng.adam_step(torch.ones(n_params, device=eng.torch_device), 1, 1e-2)
    torch.cuda.synchronize()
    assert float((views["actor.gru.weight_hh"] - before).abs().min()) > 0, "a torch learner's gradient in this layout reaches the cell"
    eng.close()


# ---- 6. the public surface: FusedTaskWrapper -------------------------------------------------------------------------------------------------------------------
def test_wrapper_set_actor_rollout_and_state(gate_cfg_restored):  # noqa: F811
    n, T = 4, 6
    env = _gate_env(n)
    actor, critic, log_std = ref.make_nets(D, (32, 24), (16,), "tanh", True, True, seed=5)
    actor, critic = actor.cuda(), critic.cuda()
    env.set_actor(actor, critic, log_std=log_std, layer_norm=True, recurrent=True)
    eng = env.env.engine
    views = eng.actor_params()
    assert torch.equal(views["flat"].cpu(), ref.flat_params(actor.cpu(), critic.cpu(), log_std)), "sync_actor copies the cells and their norms too"
    actor, critic = actor.cuda(), critic.cuda()
    env.reset()
    traj = env.rollout(T, gamma=0.99, record_hidden=True)
    assert traj.hidden.shape == (T + 1, n, 2, 24 + 16) and bool((traj.hidden[0] == 0).all()) and traj.advantages.shape == (T, n, 2)
    # the recorded trajectory is the torch twin's: value[t] from hidden[t], masks and obs[t], chunk by chunk
    a64, c64 = ref.doubles(actor.cpu(), critic.cpu())
    actor, critic = actor.cuda(), critic.cuda()
    masks = torch.cat([torch.ones(1, n), (~traj.done[:-1]).cpu().double()])[:, :, None, None].expand(T, n, 2, 1)
    with torch.no_grad():
        v64, _ = c64.evaluate(traj.obs[:3].cpu().double(), traj.hidden[0][..., 24:].cpu().double(), masks[:3])
    assert float((traj.value[:3].cpu().double() - v64[..., 0]).abs().max()) <= 1e-4
    with pytest.raises(NotImplementedError, match="back-propagation through time"):
        env.ppo_update(traj, epochs=1, minibatches=1, lr=1e-3)
    # get_state / set_state carry next_hidden() of the last recorded rollout: the same continuation twice
    ck = env.get_state()
    assert same_bits(ck["last_hidden"].cuda(), traj.next_hidden())
    one = env.rollout(4, record_hidden=True)
    assert same_bits(one.hidden[0], traj.next_hidden()), "a following rollout continues from the live state"
    env.set_state(ck)
    two = env.rollout(4, record_hidden=True)
    assert same_bits(one.hidden, two.hidden) and same_bits(one.actions, two.actions) and same_bits(one.value, two.value)
    # after an unrecorded rollout the live state cannot be read back: get_state says so
    env.rollout(2)
    with pytest.raises(RuntimeError, match="did not record its state"):
        env.get_state()
    # a reset (of the wrapper, or below it) starts the cells from zero
    env.reset()
    assert bool((env.rollout(2, record_hidden=True).hidden[0] == 0).all())
    env.env.reset()
    assert bool((env.rollout(2, record_hidden=True).hidden[0] == 0).all())
    # pull_actor brings the engine's cell back into the modules
    views["actor.gru.weight_hh"].mul_(0.5)
    before = actor.rnn.weight_hh_l0.detach().clone()
    env.pull_actor()
    torch.cuda.synchronize()
    assert torch.equal(actor.rnn.weight_hh_l0.detach(), before * 0.5)
    env.close()
