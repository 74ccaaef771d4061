"""-m gpu: the BASELINE.json configurations at their FULL sizes on the HIP engine.

  config 2  go1gate               4096 envs x 2 agents                      (also tests/test_gpu_parity.py::test_full_size_invariants)
  config 3  go1sheep-hard         2048 envs x (2 agents + 9 sheep), tracks assigned by randint as legged_robot.py:980-993
  config 4  go1seesaw             4096 envs x (2 agents + articulated seesaw)
  config 5  go1football-defender  4096 envs x (3 agents + ball) = the per-GPU shard of the 32768-env, 8-GPU configuration

Until the end of round 5 the oracle could not run these sizes in seconds (its policy layers' fmaf chain was a libm call per multiply-add, and
libgomp oversubscribed the 16 CPUs of the GPU box's container with 256 threads); it can now, and test_full_size_rollout_matches_oracle holds the
four configurations to it directly.  What tied them to the small batches before, and still does, is SIZE INDEPENDENCE: envs
[g0, g0 + NS) of the full batch and the same GLOBAL env ids run alone (env_id_offset, same track assignment) must agree bit for
bit over a fused rollout -- every kernel treats a row / an env independently of its neighbours and every random draw is keyed by
the global env id.  Plus invariants that need no oracle: finite state, unit quaternions, bodies inside the arena, joint limits,
no truncated contact list."""
import numpy as np
import pytest
import torch

from helpers import make_desc, hip_engine, oracle_engine, task_cfg
from mqe.engine import abi

pytestmark = pytest.mark.gpu


def _log(**kw):
    """measured deviations, appended to gpurun_out/test_measurements.jsonl when that directory exists (what the bounds are set from)"""
    import json, os
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out")
    if os.path.isdir(out):
        with open(os.path.join(out, "test_measurements.jsonl"), "a") as f:
            f.write(json.dumps(kw) + "\n")

FULL = [("go1gate", 4096), ("go1sheep-hard", 2048), ("go1seesaw", 4096), ("go1football-defender", 4096)]


def assign_tracks(task, NF, seed=0):
    """terrain_levels / terrain_types of the GLOBAL batch as Go1._create_scene draws them (reference legged_robot.py:980-993):
    levels = randint(0, max_init_level + 1), types = env id mod num_cols"""
    cfg = task_cfg(task)
    rows, cols = cfg.terrain.num_rows, cfg.terrain.num_cols
    max_level = cfg.terrain.max_init_terrain_level if cfg.terrain.curriculum else rows - 1
    g = torch.Generator().manual_seed(seed)
    levels = torch.randint(0, max_level + 1, (NF,), generator=g).numpy()
    types = np.arange(NF) % cols
    return levels, types


def shard_desc(task, NF, g0, n, levels, types):
    return make_desc(task, n, levels=levels[g0:g0 + n], types=types[g0:g0 + n], env_id_offset=g0)


@pytest.mark.parametrize("task,NF", FULL)
def test_full_size_invariants(task, NF):
    levels, types = assign_tracks(task, NF)
    d, k, ctx = shard_desc(task, NF, 0, NF, levels, types)
    if task == "go1sheep-hard":
        assert len(set(zip(levels.tolist(), types.tolist()))) == 35, "all 5 x 7 tracks must be in use"
    e = hip_engine(d, k)
    e.reset_all()
    A, P = d.num_agents, d.num_npcs
    Aw = e.tensor(abi.T_WRAPPER_OBS).shape[1]
    g = torch.Generator(device="cuda").manual_seed(1234)
    for t in range(40):
        e.step(torch.rand(NF, Aw, 3, device="cuda", generator=g) * 2 - 1)
    torch.cuda.synchronize()
    root, dof = e.tensor(abi.T_ROOT_STATE), e.tensor(abi.T_DOF_STATE)
    assert torch.isfinite(root).all() and torch.isfinite(dof).all()
    assert torch.isfinite(e.tensor(abi.T_WRAPPER_OBS)).all() and torch.isfinite(e.tensor(abi.T_WRAPPER_REWARD)).all()
    assert torch.isfinite(e.tensor(abi.T_CONTACT_FORCE)).all()
    rob = root[:, :A]
    assert ((rob[..., 3:7].norm(dim=-1) - 1).abs() < 1e-4).all()                           # unit quaternions
    zmax = 2.0 if task == "go1seesaw" else 1.0                                             # the seesaw's far end is 1.3 m up
    assert rob[..., 2].min() > 0.0 and rob[..., 2].max() < zmax                            # nobody fell through the ground / flew away
    eo = torch.as_tensor(ctx["env_origins"], device="cuda")[:, None, :2]
    assert (root[:, :, :2] - eo).abs().max() < 30.0                                        # nothing left its track
    q = dof[:, :12 * A, 0].reshape(NF, A, 12)
    lo = torch.tensor([d.robot.dof_lower[j] for j in range(12)], device="cuda")
    hi = torch.tensor([d.robot.dof_upper[j] for j in range(12)], device="cuda")
    assert (q > lo - 0.05).all() and (q < hi + 0.05).all()                                 # joint limits, to solver tolerance
    vl = torch.tensor([d.robot.dof_vel_limit[j] for j in range(12)], device="cuda")
    assert (dof[:, :12 * A, 1].reshape(NF, A, 12).abs() <= vl * 1.0001).all()               # URDF joint velocity limits (go1.urdf:115,157,185)
    sv = e.tensor(abi.T_SUBSTEP_DOF_VEL).reshape(NF, 4, A, 12)
    assert (sv.abs() <= vl * 1.0001).all() and torch.equal(sv[:, 3].reshape(NF, -1), dof[:, :12 * A, 1])
    obs = e.tensor(abi.T_WRAPPER_OBS)
    assert obs.shape[:2] == (NF, Aw)
    if task not in ("go1football-defender",):
        ids = obs[:, :, :Aw]
        assert torch.equal(ids, torch.eye(Aw, device="cuda").expand(NF, Aw, Aw))            # one-hot agent ids
    if P and task == "go1sheep-hard":
        sheep = root[:, A:]
        assert (sheep[..., 7:9].abs() <= 2.0).all() and (sheep[..., 2] >= 0).all() and (sheep[..., 2] <= 0.3 + 0.05).all()   # go1_sheep.py:59-60
    # how often did a bounded contact list drop a touching pair?  (per env and substep; 0 expected on these scenes)
    ov = e.tensor(abi.T_CONTACT_OVERFLOW)
    assert int(ov.sum()) <= NF * 40 * 4 // 1000, f"contact lists truncated in {int(ov.sum())} env-substeps"
    assert int(e.tensor(abi.T_RESET_COUNT).min()) >= 1
    e.close()


def test_soak_two_full_episodes_at_full_size():
    """go1gate, 4096 envs x 2 agents, 1100 fused steps with random commands = what bench.py measures, twice over: two waves of
    time-outs of ALL envs (max_episode_length 500), the history ring turned over 36 times, thousands of falls.  No oracle at this
    size and length; what must hold: finite state all along, unit quaternions, joint limits, robots on their tracks, episode
    counters inside the episode length, every env reset at least twice, (almost) no truncated contact list, and a policy that is
    still alive (the robots' mean speed does not collapse to zero or blow up)."""
    NF = 4096
    levels, types = assign_tracks("go1gate", NF)
    d, k, ctx = shard_desc("go1gate", NF, 0, NF, levels, types)
    e = hip_engine(d, k)
    e.reset_all()
    A = d.num_agents
    g = torch.Generator(device="cuda").manual_seed(77)
    root, dof = e.tensor(abi.T_ROOT_STATE), e.tensor(abi.T_DOF_STATE)
    lo = torch.tensor([d.robot.dof_lower[j] for j in range(12)], device="cuda")
    hi = torch.tensor([d.robot.dof_upper[j] for j in range(12)], device="cuda")
    eo = torch.as_tensor(ctx["env_origins"], device="cuda")[:, None, :2]
    n_time_out = 0
    for t in range(1100):
        e.step(torch.rand(NF, A, 3, device="cuda", generator=g) * 2 - 1)
        if t % 50 == 49 or t in (500, 501, 1001, 1002):
            torch.cuda.synchronize()
            assert torch.isfinite(root).all() and torch.isfinite(dof).all() and torch.isfinite(e.tensor(abi.T_WRAPPER_OBS)).all(), t
            assert ((root[:, :A, 3:7].norm(dim=-1) - 1).abs() < 1e-4).all(), t
            assert root[:, :A, 2].min() > 0.0 and root[:, :A, 2].max() < 1.5, t
            assert (root[:, :A, :2] - eo).abs().max() < 30.0, t
            q = dof[:, :12 * A, 0].reshape(NF, A, 12)
            assert (q > lo - 0.05).all() and (q < hi + 0.05).all(), t
            assert int(e.tensor(abi.T_EPISODE_LENGTH).max()) <= d.max_episode_length + 1, t
        n_time_out += int(e.tensor(abi.T_TIME_OUT_BUF).sum()) if t in (500, 1001) or t % 97 == 0 else 0
    torch.cuda.synchronize()
    assert int(e.tensor(abi.T_RESET_COUNT).min()) >= 3                      # the reset at the start + two time-outs at least
    assert int(e.tensor(abi.T_CONTACT_OVERFLOW).sum()) <= NF * 1100 * 4 // 1000
    speed = root[:, :A, 7:9].norm(dim=-1).mean()
    assert 0.01 < float(speed) < 3.0, float(speed)
    act = e.tensor(abi.T_ACTIONS)
    assert float(act.abs().mean()) > 0.01 and float(act.abs().max()) <= d.clip_actions + 1e-6
    e.close()


@pytest.mark.parametrize("task,NF", FULL)
def test_full_size_batch_is_the_union_of_its_shards(monkeypatch, task, NF):
    """20 fused steps: envs [g0, g0 + 32) of the full batch == the same global env ids run as a 32-env batch of their own (the size
    the oracle parity tests cover), BIT FOR BIT -- state, returned batch, reset flags, episode counters.  The layer-0 kernel is
    pinned to the split-f16 one, which the small batch would not pick by itself."""
    monkeypatch.setenv("MQE_GEMM_SPLIT", "1")
    NS = 32
    levels, types = assign_tracks(task, NF)
    df, kf, _ = shard_desc(task, NF, 0, NF, levels, types)
    ef = hip_engine(df, kf)
    ef.reset_all()
    small = []
    # shard starts are multiples of 32 envs: the policy tail's per-workgroup k rotation is keyed by the GLOBAL 32-row block, so a
    # shard that starts inside a block would sum its dot products in another (equally valid) order -- last-bit differences
    for g0 in (0, (NF // 2 // NS) * NS - NS, NF - NS):
        d, k, _ = shard_desc(task, NF, g0, NS, levels, types)
        e = hip_engine(d, k)
        e.reset_all()
        small.append((g0, e))
    Aw = ef.tensor(abi.T_WRAPPER_OBS).shape[1]
    g = torch.Generator().manual_seed(11)
    kinds = (abi.T_ROOT_STATE, abi.T_DOF_STATE, abi.T_WRAPPER_OBS, abi.T_WRAPPER_REWARD, abi.T_RESET_BUF, abi.T_EPISODE_LENGTH,
             abi.T_CONTACT_FORCE, abi.T_SUBSTEP_TORQUES)
    for t in range(-1, 20):
        if t >= 0:
            a = torch.rand(NF, Aw, 3, generator=g) * 2 - 1
            ef.step(a.cuda().contiguous())
            for g0, e in small:
                e.step(a[g0:g0 + NS].cuda().contiguous())
        torch.cuda.synchronize()
        for g0, e in small:
            for kind in kinds:
                full = ef.tensor(kind)
                per = full.shape[0] // NF
                assert torch.equal(full[g0 * per:(g0 + NS) * per], e.tensor(kind)), f"{task}: step {t}, envs from {g0}, tensor kind {kind}"
    ef.close()
    for _, e in small:
        e.close()


# step-20 deviations (median, 99th percentile, worst env [m]) of these four at the final round-6 physics; bounds = 3 x these (floors 1e-6 / 2e-5 / 1e-3)
FULL_MEASURED = {"go1gate": (2.4e-07, 7.2e-06, 8.8e-04), "go1sheep-hard": (6.0e-08, 3.2e-04, 6.0e-03),
                 "go1seesaw": (2.4e-07, 4.1e-05, 2.5e-03), "go1football-defender": (2.4e-07, 1.1e-06, 1.2e-05)}


@pytest.mark.parametrize("task,NF", FULL)
def test_full_size_rollout_matches_oracle(task, NF):
    """BASELINE.json's single-GPU configurations at their full sizes, HIP engine against the CPU oracle: 20 fused steps from the seeded reset distribution
    with the same random wrapper actions.  Bounds = 3 x what the final round-6 physics measures at step 20 (FULL_MEASURED; both engines are deterministic,
    so the figures reproduce on any box), no reset flag may differ."""
    levels, types = assign_tracks(task, NF)
    d1, k1, _ = shard_desc(task, NF, 0, NF, levels, types)
    d2, k2, _ = shard_desc(task, NF, 0, NF, levels, types)
    eh, eo = hip_engine(d1, k1), oracle_engine(d2, k2)
    eh.reset_all(); eo.reset_all()
    A = d1.num_agents
    Aw = eo.tensor(abi.T_WRAPPER_OBS).shape[1]
    g = torch.Generator().manual_seed(7)
    flags = 0
    for t in range(20):
        a = torch.rand(NF, Aw, 3, generator=g) * 2 - 1
        eh.step(a.cuda().contiguous()); eo.step(a)
        flags += int((eh.tensor(abi.T_RESET_BUF).cpu() != eo.tensor(abi.T_RESET_BUF)).sum())
        if t == 0:
            assert (eh.tensor(abi.T_ACTIONS).cpu() - eo.tensor(abi.T_ACTIONS)).abs().max() < 5e-6          # the policy's joint targets (measured 1.8e-7)
    rh, ro = eh.tensor(abi.T_ROOT_STATE).cpu(), eo.tensor(abi.T_ROOT_STATE)
    assert torch.isfinite(rh).all() and torch.isfinite(ro).all()
    dev = (rh[:, :A, :3] - ro[:, :A, :3]).abs().amax(dim=(1, 2))
    got = (float(dev.median()), float(dev.quantile(0.99)), float(dev.max()))
    _log(kind="full_size_rollout", task=task, N=NF, dev=got, flags=flags)
    med, p99, worst = FULL_MEASURED[task]
    assert got[0] < max(3 * med, 1e-6) and got[1] < max(3 * p99, 2e-5) and got[2] < max(3 * worst, 1e-3), got
    assert flags == 0, flags
    assert (eh.tensor(abi.T_WRAPPER_OBS).cpu() - eo.tensor(abi.T_WRAPPER_OBS)).abs().median() < 1e-5
    assert int(eh.tensor(abi.T_CONTACT_OVERFLOW).sum()) == int(eo.tensor(abi.T_CONTACT_OVERFLOW).sum()) == 0
    eh.close(); eo.close()


# step-20 deviations (median, 99th percentile, worst env [m]) of what bench.py labels strict_f32 -- MQE_GEMM_SPLIT=0 (k_gemm_f32 for layer 0),
# MQE_NO_FUSED_TAIL=1 (the separate f32 policy tail), MQE_ACT_F32=1 (the actuator's f32 MFMA chain) -- on go1gate at 4096 envs, measured once on
# the MI355X; bounds = 3 x these with the floors of the test above
STRICT_MEASURED = (2.4e-07, 7.5e-06, 8.8e-04)


def test_strict_f32_configuration_at_full_size_matches_oracle(monkeypatch):
    """bench.py's strict-precision line runs these kernels and nothing else checks them at the headline size: go1gate, 4096 envs, all three
    switches together, 20 fused steps against the oracle with the protocol of test_full_size_rollout_matches_oracle"""
    for k, v in (("MQE_GEMM_SPLIT", "0"), ("MQE_NO_FUSED_TAIL", "1"), ("MQE_ACT_F32", "1")):
        monkeypatch.setenv(k, v)
    NF = 4096
    levels, types = assign_tracks("go1gate", NF)
    d1, k1, _ = shard_desc("go1gate", NF, 0, NF, levels, types)
    d2, k2, _ = shard_desc("go1gate", NF, 0, NF, levels, types)
    eh, eo = hip_engine(d1, k1), oracle_engine(d2, k2)
    eh.reset_all(); eo.reset_all()
    A = d1.num_agents
    g = torch.Generator().manual_seed(7)
    flags = 0
    for t in range(20):
        a = torch.rand(NF, A, 3, generator=g) * 2 - 1
        eh.step(a.cuda().contiguous()); eo.step(a)
        flags += int((eh.tensor(abi.T_RESET_BUF).cpu() != eo.tensor(abi.T_RESET_BUF)).sum())
        if t == 0:
            assert (eh.tensor(abi.T_ACTIONS).cpu() - eo.tensor(abi.T_ACTIONS)).abs().max() < 5e-6          # the policy's joint targets
    rh, ro = eh.tensor(abi.T_ROOT_STATE).cpu(), eo.tensor(abi.T_ROOT_STATE)
    assert torch.isfinite(rh).all() and torch.isfinite(ro).all()
    dev = (rh[:, :A, :3] - ro[:, :A, :3]).abs().amax(dim=(1, 2))
    got = (float(dev.median()), float(dev.quantile(0.99)), float(dev.max()))
    _log(kind="strict_f32_full_size", task="go1gate", N=NF, dev=got, flags=flags)
    med, p99, worst = STRICT_MEASURED
    assert got[0] < max(3 * med, 1e-6) and got[1] < max(3 * p99, 2e-5) and got[2] < max(3 * worst, 1e-3), got
    assert flags == 0, flags
    eh.close(); eo.close()


# the other nine tasks of ENV_DICT at 4096 envs (go1football-2vs2: four robots per env): step-20 deviations measured at the final round-6 physics
# (median, 99th percentile, worst env [m]; gpurun_out/test_measurements.jsonl -> profiles/r06_full_size_measurements.jsonl); the bounds below are 3 x these with
# floors of 1e-6 / 2e-5 / 1e-3 (they were 10 x with floors ten times higher), and no reset flag may differ (none did in 5.2 M).  go1revolvingdoor's door contact is
# the one place where two correct rollouts part by a centimetre within 20 steps (a robot leaning on the moving wing)
OTHER = {"go1bridge": (2.4e-07, 1.9e-06, 1.0e-05), "go1football-1vs1": (8.9e-08, 9.5e-07, 9.2e-06), "go1football-2vs2": (2.7e-07, 1.4e-06, 3.2e-05),
         "go1plane": (6.0e-08, 3.9e-06, 1.0e-03), "go1pushbox": (2.4e-07, 4.1e-05, 2.2e-03), "go1revolvingdoor": (7.2e-07, 6.6e-04, 1.1e-02),
         "go1sheep-easy": (2.4e-07, 5.7e-05, 2.7e-03), "go1tug": (2.4e-07, 6.3e-05, 9.4e-04), "go1wrestling": (9.5e-07, 4.1e-05, 2.6e-04)}


@pytest.mark.parametrize("task", sorted(OTHER))
def test_every_other_task_at_4096_envs_matches_oracle(task):
    NF = 4096
    d1, k1, _ = make_desc(task, NF)
    d2, k2, _ = make_desc(task, NF)
    eh, eo = hip_engine(d1, k1), oracle_engine(d2, k2)
    eh.reset_all(); eo.reset_all()
    A = d1.num_agents
    Aw = eo.tensor(abi.T_WRAPPER_OBS).shape[1]
    g = torch.Generator().manual_seed(7)
    flags = 0
    for t in range(20):
        a = torch.rand(NF, Aw, 3, generator=g) * 2 - 1
        eh.step(a.cuda().contiguous()); eo.step(a)
        flags += int((eh.tensor(abi.T_RESET_BUF).cpu() != eo.tensor(abi.T_RESET_BUF)).sum())
    rh, ro = eh.tensor(abi.T_ROOT_STATE).cpu(), eo.tensor(abi.T_ROOT_STATE)
    assert torch.isfinite(rh).all() and torch.isfinite(ro).all()
    dev = (rh[:, :A, :3] - ro[:, :A, :3]).abs().amax(dim=(1, 2))
    med, p99, worst = OTHER[task]
    got = (float(dev.median()), float(dev.quantile(0.99)), float(dev.max()))
    _log(kind="full_size_rollout", task=task, N=NF, dev=got, flags=flags)
    assert got[0] < max(3 * med, 1e-6) and got[1] < max(3 * p99, 2e-5) and got[2] < max(3 * worst, 1e-3), got
    assert flags == 0, flags
    assert int(eh.tensor(abi.T_CONTACT_OVERFLOW).sum()) == int(eo.tensor(abi.T_CONTACT_OVERFLOW).sum()) == 0
    eh.close(); eo.close()
