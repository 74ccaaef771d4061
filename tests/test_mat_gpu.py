"""-m gpu: the Multi-Agent Transformer policy inside the engine's rollout (MQE_ACTOR_TRANSFORMER; csrc/kernels_mat.hpp: k_actor_mat;
HipEngine.create_actor(transformer=True)): (1) one deterministic step against float64, held to 4x the error of a float32 CPU evaluation of the same
MATNet; (2) twelve recorded stochastic steps: the conditioning on the SAMPLED actions, the draws, logp, value; (3) the acting pass against the parallel
pass; (4) continuation, checkpoint, determinism, shards; (5) A' = 4 and A' = 1; (6) gae under value normalisation and Adam on a torch gradient;
(7) refusals; (8) the task wrapper's surface.  go1gate with 37 envs = 74 rows: one full workgroup and one partial; max_episode_length=5: every env
resets inside a 12-step window.  (1) and (2) run again at mat_ref.EDGE_SHAPES -- E = 68 and 92, D = 13, 14, 20 and 34, the real tasks' own scenes -- and (7)
has the refusal boundary at D = 34.

THE HANDLES WITH A' = 4 AND A' = 1 are tests/test_joint_loss_gpu.py's: go1football-2vs2 and go1plane with the descriptor's task kind set to the
seesaw wrapper's.  Those tests never step such a handle; a rollout does.  What a step of it runs that the stock scenes do not: the seesaw branch of
wrapper_env_dev (csrc/kernels_step.hpp), the only code keyed on that task kind -- the sizes (A', D = 12 + A') apart.  Its observation reads the
agents' own rows of the observation bag (one-hot, own and mirror partner's base state); its reward reads w_last / w_have_last (per env, MQE_MAX_AGENTS
wide, allocated for every scene), collide_buf, r_term, p_term and reset_buf.  No NPC state, no dof beyond the robots', no scene geometry: nothing those
two scenes lack.  The NPC physics is keyed on npc_kind, which stays the scene's own."""
import ctypes as C
import math
import types

import numpy as np
import pytest
import torch

import gae_ref
import mat_ref as ref
import rollout_ref
import value_norm_ref as vref
from helpers import make_desc, hip_engine
from mqe.engine import abi
from test_rollout_gpu import _gate_env, engine, gate_cfg_restored, same_bits, sampling_tolerances  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

N, AW, D = 37, 2, 16
EPS32 = 2.0 ** -24
_CACHE = {}


def install(eng, E, seed=0, **kw):
    """create the transformer actor of width E with seeded parameters; -> the float32 MATNet on the host"""
    Dd = int(eng.tensor(abi.T_WRAPPER_OBS).shape[-1])
    net = ref.make_net(Dd, E, seed)
    eng.create_actor([Dd, E, 3], None, transformer=True, **kw)
    views = eng.actor_params()
    flat = ref.flat_params(net)
    assert views["flat"].numel() == flat.numel() == ref.param_count(Dd, E)
    views["flat"].copy_(flat)
    return net


def one_step(eng, net, n, A, Dd, seed, what):
    """a deterministic step from the seeded inputs of mat_ref: means and values within 4x the yardstick; -> the trajectory"""
    n64 = ref.doubles(net)
    obs0, _ = ref.inputs(n, A, Dd, seed=seed)
    traj = eng.rollout(1, obs0=obs0.to(eng.torch_device), deterministic=True)
    torch.cuda.synchronize()
    assert torch.equal(traj.obs[0].cpu(), obs0)
    act = traj.actions[0].cpu()
    y = ref.yardstick(net, n64, obs0, act)
    dev_mean = float((act.double() - y["mean64"]).abs().max())
    dev_value = float((traj.value[0].cpu().double() - y["value64"]).abs().max())
    print(f"mat_step {what} mean: kernel {dev_mean:.3e} torch-f32 {y['yard_mean']:.3e} value: kernel {dev_value:.3e} torch-f32 {y['yard_value']:.3e}")
    assert dev_mean <= 4 * y["yard_mean"], (dev_mean, y["yard_mean"])
    assert dev_value <= 4 * y["yard_value"], (dev_value, y["yard_value"])
    # logp at z = 0: -sum ln sigma - 1.5 ln 2 pi; three f32 logarithms and four subtractions of partial sums below 8 in magnitude
    want = -float(torch.log(n64.sigma().detach()).sum()) - 1.5 * math.log(2 * math.pi)
    assert float((traj.logp.cpu().double() - want).abs().max()) <= 8 * 8 * EPS32
    return traj, y, obs0


# ---- 1. one step against float64 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ref.SHAPES))
def test_one_step_against_float64(name):
    """tests/test_mat.py holds the five wrong variants to at least 100x this bound on these very inputs, seeds and shapes"""
    E = ref.SHAPES[name]
    eng = engine("go1gate", N, max_episode_length=5)
    net = install(eng, E, seed=len(name))
    eng.reset_all()
    one_step(eng, net, N, AW, D, E, name)
    eng.close()


def edge_engine(task):
    """the cached handle of a scene of mat_ref.EDGE_SHAPES: its own task kind, but go1plane, which takes the seesaw wrapper's (the module docstring)"""
    if ("edge", task) not in _CACHE:
        n = ref.EDGE_ENVS[task]
        if task == "go1plane":
            d, k, _ = make_desc(task, n)
            d.task = abi.TASK["seesaw"]
            _CACHE["edge", task] = hip_engine(d, k)
        else:
            _CACHE["edge", task] = engine(task, n, max_episode_length=5)
        _CACHE["edge", task].reset_all()
    return _CACHE["edge", task]


@pytest.mark.parametrize("name", list(ref.EDGE_SHAPES))
def test_one_step_at_the_edge_shapes(name):
    """mat_ref.EDGE_SHAPES: a second, partial output pass (E = 68, 92), the largest LDS image (E = 92 at D = 34), D off the 16-byte grid beside aligned
    E x E matrices (D = 14, 34; nothing aligned at D = 13), D > E and D > 5 E, a scene with NPCs.  tests/test_mat.py holds the wrong variants to at least
    100x this bound on these inputs, seeds and shapes"""
    task, A, Dd, E = ref.EDGE_SHAPES[name]
    eng, n = edge_engine(task), ref.EDGE_ENVS[task]
    assert tuple(int(x) for x in eng.tensor(abi.T_WRAPPER_OBS).shape) == (n, A, Dd)
    assert abi.actor_mat_lds_bytes(Dd, E) <= abi.MAT_LDS_LIMIT
    pseed, iseed = ref.edge_seeds(name)
    net = install(eng, E, seed=pseed)
    one_step(eng, net, n, A, Dd, iseed, name)


# ---- 2. twelve steps, recorded, stochastic --------------------------------------------------------------------------------------------------------------
def recorded(name, seed=11, T=12, task="go1gate"):
    """name: a key of mat_ref.SHAPES on go1gate, or the width itself"""
    key = (name, seed, T, task)
    if key not in _CACHE:
        eng = engine(task, N, seed=seed, max_episode_length=5)
        net = install(eng, ref.SHAPES[name] if name in ref.SHAPES else name, seed=3)
        eng.reset_all()
        traj = eng.rollout(T)
        torch.cuda.synchronize()
        _CACHE[key] = dict(net=net, obs=traj.obs.cpu(), done=traj.done.cpu(), actions=traj.actions.cpu(), logp=traj.logp.cpu(), value=traj.value.cpu(), seed=seed, T=T)
        eng.close()
    return _CACHE[key]


@pytest.mark.parametrize("name", ["e64", "e12"])
def test_twelve_recorded_steps(name):
    check_recorded(recorded(name), name)


@pytest.mark.parametrize("task,E", [("go1sheep-hard", 12), ("go1gate", 92)])
def test_six_recorded_steps_at_the_edges(task, E):
    """the same window, six steps with every env reset inside it: D = 34 > E in a scene with NPCs; the largest width"""
    r = recorded(E, T=6, task=task)
    assert r["obs"].shape == (7, N, AW, ref.EDGE_SHAPES["sheep-e12" if task == "go1sheep-hard" else "gate-e92"][2])
    check_recorded(r, f"{task} E={E}")


def check_recorded(r, name):
    T, net = r["T"], r["net"]
    n64 = ref.doubles(net)
    assert bool(r["done"].any(dim=0).all()), "every env resets at least once inside the window"
    sigma = n64.sigma().detach()
    twin = rollout_ref.actor_draws(r["seed"], 0, N, AW, 0, T)
    a = r["actions"].double()
    worst = dict(z=0.0, lp=0.0, value=0.0, implied=0.0)
    for t in range(T):
        # MATNet.evaluate on the engine's own observation and RECORDED actions: nothing compounds
        y = ref.yardstick(net, n64, r["obs"][t], r["actions"][t])
        tol_z, tol_lp = sampling_tolerances(y["yard_mean"], float(a[t].abs().max()), float(sigma.min()), float(abs(twin[t]).max()))
        # the engine's implied mean, a - sigma z of the host twin's draw, is the twin's mean conditioned on the sampled actions ...
        implied = a[t] - sigma * torch.from_numpy(twin[t])
        dev_implied = float((implied - y["mean64"]).abs().max())
        z = ((a[t] - y["mean64"]) / sigma).numpy()
        dev_z = float(abs(z - twin[t]).max())
        assert dev_z <= tol_z, (t, dev_z, tol_z)
        assert dev_implied <= tol_z * float(sigma.max()), (t, dev_implied)
        # ... and not the one a decoder that never saw agent 0's action would give: agent 1 misses the bound, agent 0 (s_0 = 0 either way) keeps it
        with torch.no_grad():
            m0, _, _ = ref.wrong_evaluate(n64, r["obs"][t].double(), a[t], "s_zero")
        assert float((implied[:, 1] - m0[:, 1]).abs().max()) > 100 * tol_z * float(sigma.max())
        assert float((implied[:, 0] - m0[:, 0]).abs().max()) <= tol_z * float(sigma.max())
        dev_lp = float((r["logp"][t].double() - y["logp64"]).abs().max())
        dev_v = float((r["value"][t].double() - y["value64"]).abs().max())
        assert dev_lp <= tol_lp, (t, dev_lp, tol_lp)
        assert dev_v <= 4 * y["yard_value"], (t, dev_v, y["yard_value"])
        worst = dict(z=max(worst["z"], dev_z / tol_z), lp=max(worst["lp"], dev_lp / tol_lp), value=max(worst["value"], dev_v / y["yard_value"]),
                     implied=max(worst["implied"], dev_implied))
    # value[T]: the encoder on the last observation
    with torch.no_grad():
        vT64 = n64.encode(r["obs"][T].double())[1]
        vT32 = net.encode(r["obs"][T])[1]
    assert float((r["value"][T].double() - vT64).abs().max()) <= 4 * float((vT32.double() - vT64).abs().max())
    print(f"mat_rollout {name}: z {worst['z']:.3f} of its tolerance, logp {worst['lp']:.3f} of its tolerance, value {worst['value']:.2f} x yardstick, implied mean {worst['implied']:.3e}")


# ---- 3. the acting pass against the parallel pass ---------------------------------------------------------------------------------------------------------
def test_acting_pass_is_the_parallel_pass():
    """a deterministic rollout's agent-1 mean is the twin's with agent 0's MEAN as s_1 (test 1 holds it to the bound; here: and not with s_1 = 0);
    a stochastic step from the same observation has the same value bits and, at agent 0, the same mean up to the rounding of the draw"""
    E = 64
    A, B = engine("go1gate", N, seed=5, max_episode_length=5), engine("go1gate", N, seed=5, max_episode_length=5)
    net = install(A, E, seed=7)
    install(B, E, seed=7)
    A.reset_all(); B.reset_all()
    det, y, obs0 = one_step(A, net, N, AW, D, 77, "acting-vs-parallel")
    n64 = ref.doubles(net)
    with torch.no_grad():
        m0, _, _ = ref.wrong_evaluate(n64, obs0.double(), det.actions[0].cpu().double(), "s_zero")
    assert float((det.actions[0, :, 1].cpu().double() - m0[:, 1]).abs().max()) > 400 * y["yard_mean"]
    sto = B.rollout(1, obs0=obs0.cuda())
    torch.cuda.synchronize()
    assert same_bits(sto.value[0], det.value[0]), "the value does not depend on the draw"
    sigma = n64.sigma().detach()
    z = torch.from_numpy(rollout_ref.actor_draws(5, 0, N, AW, 0, 1)[0])
    tol_z, _ = sampling_tolerances(0.0, float(sto.actions.abs().max()), float(sigma.min()), float(z.abs().max()))
    implied0 = sto.actions[0, :, 0].cpu().double() - sigma * z[:, 0]
    assert float((implied0 - det.actions[0, :, 0].cpu().double()).abs().max()) <= tol_z * float(sigma.max()), "agent 0: the same mean in both modes"
    assert float((sto.actions[0, :, 1].cpu() - det.actions[0, :, 1].cpu()).abs().max()) > 1e-3
    A.close(); B.close()


# ---- 4. continuation, checkpoint, determinism, shards ---------------------------------------------------------------------------------------------------
def _same(a, b, rows=slice(None)):
    return (same_bits(a.actions[:, rows], b.actions) and same_bits(a.logp[:, rows], b.logp) and same_bits(a.value[:, rows], b.value)
            and same_bits(a.obs[:, rows], b.obs) and same_bits(a.done[:, rows], b.done))


def _cat(x, y):
    c = lambda a, b: torch.cat([a, b])
    return types.SimpleNamespace(actions=c(x.actions, y.actions), logp=c(x.logp, y.logp), done=c(x.done, y.done), value=c(x.value[:-1], y.value), obs=c(x.obs[:-1], y.obs))


def test_continuation_checkpoint_and_determinism():
    E, T = 12, 12
    engs = [engine("go1gate", N, seed=4, max_episode_length=5) for _ in range(5)]
    for e in engs:
        install(e, E, seed=2)
        e.reset_all()
    Aa, Bb, Cc, Dd, Ee = engs
    whole, again = Aa.rollout(T), Cc.rollout(T)
    assert _same(whole, again), "two runs give the same bits"
    assert bool(whole.done.any()), "episodes end inside the window"
    first = Bb.rollout(6)
    second = Bb.rollout(6)
    assert _same(whole, _cat(first, second)), "rollout(6) + rollout(6) is rollout(12), bit for bit"
    half = Dd.rollout(6)
    Ee.load_state(Dd.save_state())
    rest = Ee.rollout(6, obs0=half.obs[6].contiguous())
    assert _same(whole, _cat(half, rest)), "a checkpointed rollout continues bit for bit in a fresh handle"
    for e in engs:
        e.close()


def test_a_shard_reproduces_its_rows():
    T = 8
    full, low, part = engine("go1gate", 4, max_episode_length=5), engine("go1gate", 2, max_episode_length=5), engine("go1gate", 2, max_episode_length=5, env_id_offset=2)
    for e in (full, low, part):
        install(e, 12, seed=13)
        e.reset_all()
    f, l, p = full.rollout(T), low.rollout(T), part.rollout(T)
    assert _same(f, l, rows=slice(0, 2)) and _same(f, p, rows=slice(2, 4)), "the two shards' union is the whole batch"
    assert not same_bits(f.actions[:, 0:2], p.actions)
    full.close(); low.close(); part.close()


# ---- 5. A' = 4 and A' = 1 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("task,n,A", [("go1football-2vs2", 17, 4), ("go1plane", 70, 1)])
def test_other_agent_counts(task, n, A):
    """17 envs x 4 agents = 68 rows: a group ends at the tile's edge and one begins the next tile; 70 envs x 1 agent: nothing to attend to but itself.
    The handles are the module docstring's."""
    d, k, _ = make_desc(task, n)
    d.task = abi.TASK["seesaw"]
    eng = hip_engine(d, k)
    nn, Aw, Dd = (int(x) for x in eng.tensor(abi.T_WRAPPER_OBS).shape)
    assert (nn, Aw, Dd) == (n, A, 12 + A)
    eng.reset_all()
    for name in ("e64", "e12"):
        net = install(eng, ref.SHAPES[name], seed=A)
        one_step(eng, net, n, A, Dd, 10 * A + len(name), f"{task} {name}")
    eng.close()


# ---- 6. gae under value normalisation; Adam on a torch gradient ----------------------------------------------------------------------------------------------
def test_gae_with_value_norm_and_adam_on_a_torch_gradient():
    T, gamma, E = 6, 0.99, 12
    eng = engine("go1gate", N, seed=3, max_episode_length=5)
    net = install(eng, E, seed=9, value_norm=True)
    eng.reset_all()
    views = eng.actor_params()
    st = views["value_norm"].cpu().numpy()
    traj = eng.rollout(T, time_outs=True)
    eng.gae(traj, gamma)
    torch.cuda.synchronize()
    rew, val = traj.reward.cpu().numpy(), traj.value.cpu().numpy()
    done, to = traj.done.view(torch.uint8).cpu().numpy(), traj.time_outs.view(torch.uint8).cpu().numpy()
    adv64, ret64 = gae_ref.gae(rew, vref.denormalise(val, st[3], st[4]), done, to, gamma, 0.95)
    tol_adv, tol_ret = vref.tol_gae(rew, val, adv64, gamma, 0.95, st[3], st[4])
    assert float(np.abs(traj.advantages.cpu().numpy() - adv64).max()) <= tol_adv and float(np.abs(traj.returns.cpu().numpy() - ret64).max()) <= tol_ret
    # a torch learner: the gradient of a loss on MATNet.evaluate(traj.obs, traj.actions) in "flat"'s layout, stepped by the engine's Adam
    obs, act = traj.obs[:T].cpu(), traj.actions.cpu()
    mean, logp, value = net.evaluate(obs, act)
    loss = -(logp * traj.advantages.cpu()).mean() + 0.5 * ((value - traj.returns.cpu()) ** 2).mean()
    grads = torch.autograd.grad(loss, list(net.parameters()))
    g = torch.nn.utils.parameters_to_vector(grads)
    assert g.numel() == views["flat"].numel() and float(g.abs().min()) >= 0 and int((g != 0).sum()) > 0.9 * g.numel()
    before = views["flat"].clone()
    lr = 1e-2
    eng.adam_step(g.to(eng.torch_device), 1, lr)
    torch.cuda.synchronize()
    moved = views["flat"] - before
    # Adam's first step is lr g / (|g| + eps): about lr wherever |g| is far above eps = 1e-8 (a key bias, which the softmax cancels, has a gradient of rounding size)
    assert float(moved[g.to(moved.device).abs() > 1e-6].abs().min()) > 0.5 * lr, "the first Adam step moves every parameter with a gradient by about lr"
    assert np.array_equal(views["value_norm"].cpu().numpy(), st), "Adam leaves the value-normalisation state alone"
    # the next deterministic rollout follows the moved twin
    opt = torch.optim.Adam(net.parameters(), lr=lr)
    for p, gp in zip(net.parameters(), grads):
        p.grad = gp
    opt.step()
    assert float((ref.flat_params(net) - views["flat"].cpu()).abs().max()) <= 1e-6
    views["flat"].copy_(ref.flat_params(net))
    one_step(eng, net, N, AW, D, 5, "after adam_step")
    eng.close()


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    eng = engine("go1gate", 3, max_episode_length=5)
    eng.reset_all()
    eng.create_actor([D, 7, 3], [D, 5, 1])

    def create_refused(*a, **kw):
        with pytest.raises(RuntimeError, match=r"mqe_actor_create failed \(-6\)") as ei:
            eng.create_actor(*a, **kw)
        return str(ei.value)
    for bad in ("layer_norm", "feature_norm", "recurrent"):
        assert "activation" in create_refused([D, 64, 3], [D, 64, 1], transformer=True, **{bad: True})
    assert "critic_dims" in create_refused([D, 64, 3], [D, 32, 1], transformer=True)
    assert "activation" in create_refused([D, 64, 3], [D, 64, 1], activation="relu", transformer=True)
    assert "multiple of 4" in create_refused([D, 10, 3], None, transformer=True)
    assert "multiple of 4" in create_refused([D, 2, 3], None, transformer=True)
    assert abi.actor_mat_lds_bytes(D, 96) > abi.MAT_LDS_LIMIT >= abi.actor_mat_lds_bytes(D, 92)
    msg = create_refused([D, 96, 3], None, transformer=True)
    assert "E = 96" in msg and "actor_dims" in msg
    assert "actor_layers" in create_refused([D, 64, 64, 3], [D, 64, 1], transformer=True)
    # critic_layers = 0: through the struct, as a C caller would
    sh = abi.ActorShape(obs_dim=D, act_dim=3, actor_layers=2, critic_layers=0, activation=abi.ACTOR_TRANSFORMER, action_gain=1.0)
    for i, v in enumerate([D, 64, 3]):
        sh.actor_dims[i] = v
    assert eng.lib.mqe_actor_create(eng.h, C.byref(sh)) == -6 and "critic_layers" in eng.lib.mqe_last_error().decode()
    # a refused create leaves the plain actor that was there
    assert eng.actor_params()["flat"].numel() == abi.actor_param_count([D, 7, 3], [D, 5, 1])
    plain = eng.rollout(2)
    # the accepted edges: E = 92 at D = 16, E = 4
    for E in (92, 4):
        eng.create_actor([D, E, 3], None, transformer=True)
        assert eng.actor_params()["flat"].numel() == ref.param_count(D, E)
    # every norm weight starts at 1, everything else at 0
    views = eng.actor_params()
    for name, v in views.items():
        if name.startswith("mat."):
            want = 1.0 if (".ln" in name or "_ln" in name or "obs_norm" in name) and name.endswith(".weight") else 0.0
            assert bool((v == want).all()), name
    install(eng, 12, seed=1)
    traj = eng.rollout(2, time_outs=True)
    eng.gae(traj, 0.99)
    with pytest.raises(NotImplementedError, match="gradient through the attention is not in the\\s+engine yet"):
        eng.ppo_grad(traj)
    with pytest.raises(NotImplementedError, match="MATNet.evaluate"):
        eng.ppo_update(traj, epochs=1, minibatches=1, lr=1e-3)
    # the library itself: -6, nothing written
    SENT = 0x7FC12345
    grad = torch.full((ref.param_count(D, 12),), SENT, dtype=torch.int32, device=eng.torch_device).view(torch.float32)
    p = lambda t: C.c_void_p(t.data_ptr() if t is not None else None)
    loss = abi.PpoLoss(0.2, 1.0, 0.0, 0.0)
    rc = eng.lib.mqe_ppo_grad(eng.h, 2, p(traj.packed), int(traj.packed.stride(0)), p(traj.actions), p(traj.logp), p(traj.value), p(traj.advantages), p(traj.returns),
                              p(None), 0, 2 * 3 * AW, C.byref(loss), 0, p(grad), p(None), eng._stream())
    msg = eng.lib.mqe_last_error().decode()
    torch.cuda.synchronize()
    assert rc == -6 and "gradient through the attention is not in the engine yet" in msg and "MATNet.evaluate" in msg
    assert bool((grad.view(torch.int32) == SENT).all())
    # a plain actor created afterwards runs the plain kernel again, with the bits it had
    eng2 = engine("go1gate", 3, max_episode_length=5)
    eng2.reset_all()
    eng2.create_actor([D, 7, 3], [D, 5, 1])
    assert same_bits(eng2.rollout(2).actions, plain.actions)
    eng.close(); eng2.close()


def test_refusal_boundary_at_the_widest_observation():
    """go1sheep-hard, D = 34: E = 92 (629 LDS rows, 300 bytes under the limit) is created and steps; E = 96 is refused by name, and the actor that was there
    keeps its parameters and produces the bits it produced"""
    eng, Dd = edge_engine("go1sheep-hard"), 34
    n = ref.EDGE_ENVS["go1sheep-hard"]
    assert abi.actor_mat_lds_bytes(Dd, 92) <= abi.MAT_LDS_LIMIT < abi.actor_mat_lds_bytes(Dd, 96)
    net = install(eng, 92, seed=4)
    before, _, obs0 = one_step(eng, net, n, AW, Dd, 92, "D = 34, E = 92 in front of the refusal")
    with pytest.raises(RuntimeError, match=r"mqe_actor_create failed \(-6\)") as ei:
        eng.create_actor([Dd, 96, 3], None, transformer=True)
    assert "E = 96" in str(ei.value) and "actor_dims" in str(ei.value)
    views = eng.actor_params()
    assert views["flat"].numel() == ref.param_count(Dd, 92) and torch.equal(views["flat"].cpu(), ref.flat_params(net))
    after = eng.rollout(1, obs0=obs0.to(eng.torch_device), deterministic=True)
    torch.cuda.synchronize()
    assert same_bits(after.actions, before.actions) and same_bits(after.value[0], before.value[0]) and same_bits(after.logp, before.logp)


# ---- 8. the public surface: FusedTaskWrapper ------------------------------------------------------------------------------------------------------------------
def test_wrapper_set_actor_rollout_learner_step_and_round_trip(gate_cfg_restored):  # noqa: F811
    n, T = 4, 6
    env = _gate_env(n)
    net = ref.make_net(D, 12, seed=5).cuda()
    with pytest.raises(ValueError, match="the transformer is the whole policy"):
        env.set_actor(net, torch.nn.Sequential(torch.nn.Linear(D, 1)))
    env.set_actor(net, value_norm=True)
    eng = env.env.engine
    views = eng.actor_params()
    assert torch.equal(views["flat"].cpu(), ref.flat_params(net).cpu()), "sync_actor copies every tensor, log_std from the module"
    env.reset()
    traj = env.rollout(T, gamma=0.99, normalize_advantages=True)
    assert traj.advantages.shape == (T, n, 2) and traj.value.shape == (T + 1, n, 2) and torch.isfinite(traj.advantages).all()
    # the learner loop of INTEGRATION: a torch loss on MATNet.evaluate(traj.obs, traj.actions), the optimiser, sync_actor()
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    mean, logp, value = net.evaluate(traj.obs[:T], traj.actions)
    assert float((logp.detach() - traj.logp).abs().max()) <= 1e-3, "the first-epoch ratio is 1"
    ratio = torch.exp(logp - traj.logp)
    loss = -(ratio * traj.advantages).mean() + 0.5 * ((value - traj.value[:T]) ** 2).mean()
    opt.zero_grad()
    loss.backward()
    opt.step()
    env.sync_actor()
    assert torch.equal(views["flat"], ref.flat_params(net)), "bit for bit"
    views["mat.dec.attn2.query.weight"].mul_(0.5)
    views["log_std"].add_(0.25)
    before, ls = net.dec.attn2.query.weight.detach().clone(), net.log_std.detach().clone()
    env.pull_actor()
    torch.cuda.synchronize()
    assert torch.equal(net.dec.attn2.query.weight.detach(), before * 0.5) and torch.equal(net.log_std.detach(), ls + 0.25)
    assert torch.equal(views["flat"], ref.flat_params(net))
    with pytest.raises(NotImplementedError, match="not in the\\s+engine yet"):
        env.ppo_update(traj, epochs=1, minibatches=1, lr=1e-3)
    env.rollout(2, deterministic=True)
    ck = env.get_state()
    env.set_state(ck)
    # the OpenRL adapter passes the module through
    from openrl_ws.utils import mqe_openrl_wrapper
    w = mqe_openrl_wrapper(env)
    w.set_actor(net)
    assert float(w.rollout_torch(2).actions.abs().max()) > 0
    env.close()
