"""-m gpu: the host side of the engine's actor (csrc/mqe_engine.hip: mqe_actor_create in stages, one kernel row and one device image of the shapes per
actor; FusedTaskWrapper's one ordered tensor list).  (1) Four actors created one after the other on ONE handle: each computes what a fresh handle
computes -- nothing of the actor before it survives a create.  (2) set_actor / pull_actor / sync_actor carry every tensor of every form of an actor
(tests/actor_variants.py) both ways, bit for bit.  go1gate with 5 envs = 10 rows, T = 3."""
import pytest
import torch

import actor_variants as av
from mqe.engine import abi
from test_rollout_gpu import _gate_env, engine, same_bits

pytestmark = pytest.mark.gpu

N, T = 5, 3
LOSS = dict(clip=0.2, value_coef=0.5, entropy_coef=0.01, value_clip=0.2)
# in VARIANTS' form: plain; both norms with widths off the dword path; recurrent with the hidden norm and Ha != Hc; plain again, another width
SEQUENCE = [((8,), (8,), False, False, False), ((7, 5), (7, 5), True, True, False), ((8,), (7, 5), False, True, True), ((5,), (5,), False, False, False)]


def results(eng, spec, seed, blob):
    """create the actor `spec` with seeded parameters on `eng`, bring the scene to `blob`, roll out T steps [and take one gradient]: host copies"""
    actor, critic, log_std = av.modules(spec, seed)
    kw = av.layout_kw(spec)
    eng.create_actor(kw.pop("actor_dims"), kw.pop("critic_dims"), activation="tanh", **kw)
    eng.actor_params()["flat"].copy_(av.flat_params(actor, critic, log_std))
    eng.load_state(blob)
    recurrent = spec[4]
    traj = eng.rollout(T, time_outs=True, **({"record_hidden": True} if recurrent else {}))
    out = dict(obs=traj.obs, actions=traj.actions, logp=traj.logp, value=traj.value)
    if recurrent:
        out["hidden"] = traj.hidden
    else:
        eng.gae(traj, 0.99)
        out["grad"], out["stats"] = eng.ppo_grad(traj, **LOSS)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def test_a_second_create_leaves_nothing_of_the_first():
    one = engine("go1gate", N)
    one.reset_all()
    blob = one.save_state()
    for i, spec in enumerate(SEQUENCE):
        got = results(one, spec, seed=20 + i, blob=blob)
        fresh = engine("go1gate", N)
        fresh.reset_all()
        want = results(fresh, spec, seed=20 + i, blob=blob)
        fresh.close()
        assert set(got) == set(want)
        for name in want:
            assert same_bits(got[name], want[name]), (i, spec, name)
        assert bool(torch.isfinite(got["actions"]).all()) and float(got["actions"].abs().max()) > 0
        if "grad" in got:
            assert float(got["grad"].abs().max()) > 0, "the gradient kernels read the shapes of THIS actor"
    one.close()


@pytest.fixture(scope="module")
def gate_env():
    from mqe.envs.utils import ENV_DICT
    c = ENV_DICT["go1gate"]["config"]
    saved = (c.env.num_envs, c.env.record_video)
    env = _gate_env(N)
    yield env
    env.close()
    c.env.num_envs, c.env.record_video = saved


@pytest.mark.parametrize("name", list(av.VARIANTS))
def test_every_tensor_both_ways(gate_env, name):
    """one env for all nine: every set_actor replaces the actor before it"""
    env = gate_env
    cuda = lambda mods: tuple(m.cuda() if m is not None else None for m in mods)
    actor, critic, log_std = cuda(av.modules(name, seed=1))
    env.set_actor(actor, critic, log_std=log_std, **av.set_actor_kw(name))
    views = env.env.engine.actor_params()
    assert same_bits(views["flat"], av.flat_params(actor, critic, log_std)), "set_actor copies every tensor"
    # the engine's buffer changes, view by view under the engine's names: pull_actor brings every value into the modules
    second = cuda(av.modules(name, seed=2))
    flat2 = av.flat_params(*second)
    layout = abi.actor_param_layout(**av.layout_kw(name))
    assert flat2.numel() == views["flat"].numel()
    for n, (off, shape) in layout.items():
        views[n].copy_(flat2[off:off + views[n].numel()].view(shape))
    env.pull_actor()
    torch.cuda.synchronize()
    for mine, theirs in zip((actor, critic), second[:2]):
        if mine is not None:
            for (n, p), q in zip(mine.named_parameters(), theirs.parameters()):
                assert same_bits(p.detach(), q.detach()), n
    assert same_bits(log_std, second[2])
    # the modules change: sync_actor brings every value into the engine's buffer
    third = cuda(av.modules(name, seed=3))
    with torch.no_grad():
        for mine, theirs in zip((actor, critic), third[:2]):
            if mine is not None:
                for p, q in zip(mine.parameters(), theirs.parameters()):
                    p.copy_(q)
        log_std.copy_(third[2])
    env.sync_actor()
    torch.cuda.synchronize()
    assert same_bits(views["flat"], av.flat_params(*third))
    assert not same_bits(av.flat_params(*third), flat2)
