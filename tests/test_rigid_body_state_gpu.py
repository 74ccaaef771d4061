"""-m gpu: the rigid-body state tensor (MQE_T_RIGID_BODY_STATE; mqe_refresh_rigid_body_state, mqe_set_rigid_body_refresh; reference
legged_robot_field.py:117-119,196-197).  Robot rows against float64 forward kinematics and central differences of it (tests/rigid_ref.py),
the row order against the contact forces, the terminal pose of envs reset in the step, bit-identity of everything else with the per-step
refresh on, the NPC rows of every scene class, and the Go1-level view a plugin-point override sees."""
import json
import os
import types

import numpy as np
import pytest
import torch

import rigid_ref
from helpers import make_desc, hip_engine
from mqe.engine import abi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACTS = json.load(open(os.path.join(ROOT, "tests", "golden", "go1_urdf_facts.json")))
FOOT_OFF = np.asarray(FACTS["joints"]["FL_foot_fixed"]["xyz"], np.float64)


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _quat_R(q):
    """(..., 4) xyzw -> (..., 3, 3), float64, normalised"""
    q = q / np.linalg.norm(q, axis=-1, keepdims=True)
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], -1),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], -1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1)], -2)


def _robot_rows_f64(m, p0, R0, q):
    """world origin and rotation of the 17 reported bodies of one robot (base, then per leg hip, thigh, calf, foot)"""
    R, p = rigid_ref.fk(m, p0, R0, q)
    out_p, out_R = [p[0]], [R[0]]
    for leg in range(4):
        for j in range(3):
            out_p.append(p[1 + 3 * leg + j]); out_R.append(R[1 + 3 * leg + j])
        c = 3 + 3 * leg
        out_p.append(p[c] + R[c] @ FOOT_OFF); out_R.append(R[c])
    return np.array(out_p), np.array(out_R)


def test_robot_rows_against_float64_kinematics():
    """go1gate 4096 envs x 2 robots, random joint angles (inside the limits), joint speeds, root orientations and root velocities written into
    the live state, one refresh.  Base rows are the root rows bit for bit; every other row's origin relative to its base, rotation, linear
    and angular velocity agree with float64 forward kinematics and central differences of it along the state's generalized velocity."""
    N, A = 4096, 2
    d, k, _ = make_desc("go1gate", N)
    e = hip_engine(d, k)
    e.reset_all()
    g = torch.Generator().manual_seed(7)
    lo = torch.tensor([d.robot.dof_lower[j] for j in range(12)]).repeat(A)
    hi = torch.tensor([d.robot.dof_upper[j] for j in range(12)]).repeat(A)
    root, dof = e.tensor(abi.T_ROOT_STATE), e.tensor(abi.T_DOF_STATE)
    q = lo + (hi - lo) * torch.rand(N, 12 * A, generator=g)
    qd = (torch.rand(N, 12 * A, generator=g) * 2 - 1) * 10.0
    quat = torch.randn(N, A, 4, generator=g)
    quat = quat / quat.norm(dim=-1, keepdim=True)
    vel = (torch.rand(N, A, 6, generator=g) * 2 - 1) * torch.tensor([2.0, 2.0, 2.0, 3.0, 3.0, 3.0])
    torch.cuda.synchronize()
    dof[:, :12 * A, 0] = q.cuda(); dof[:, :12 * A, 1] = qd.cuda()
    root[:, :A, 3:7] = quat.cuda(); root[:, :A, 7:13] = vel.cuda()
    e.refresh_rigid_body_state()
    torch.cuda.synchronize()
    rbs = e.tensor(abi.T_RIGID_BODY_STATE)
    assert rbs.shape == (N, 17 * A, 13)
    assert torch.equal(rbs[:, 0::17][:, :A], root[:, :A]), "base rows must be the root rows bit for bit"
    got, rt, dq = _np(rbs), _np(root), _np(dof)
    qn = np.linalg.norm(got[..., 3:7], axis=-1)
    assert np.abs(qn - 1.0).max() <= 1e-6, np.abs(qn - 1.0).max()
    m = rigid_ref.load_model()
    err = dict(p=0.0, R=0.0, v=0.0, w=0.0)
    eps = 1e-6
    for env in range(N):
        for a in range(A):
            r13 = rt[env, a]
            p0, R0, q12, gv = rigid_ref.split_state(r13, dq[env, 12 * a:12 * a + 12, 0], dq[env, 12 * a:12 * a + 12, 1])
            P, Rm = _robot_rows_f64(m, np.zeros(3), R0, q12)
            Pp, Rp = _robot_rows_f64(m, *rigid_ref._advance(np.zeros(3), R0, q12, gv, +eps))
            Pm, Rmm = _robot_rows_f64(m, *rigid_ref._advance(np.zeros(3), R0, q12, gv, -eps))
            V = (Pp - Pm) / (2 * eps)
            Wm = np.einsum("bij,bkj->bik", (Rp - Rmm) / (2 * eps), Rm)
            W = np.stack([Wm[:, 2, 1] - Wm[:, 1, 2], Wm[:, 0, 2] - Wm[:, 2, 0], Wm[:, 1, 0] - Wm[:, 0, 1]], -1) / 2
            rows = got[env, 17 * a:17 * a + 17]
            err["p"] = max(err["p"], np.abs((rows[:, :3] - r13[:3]) - P).max())
            err["R"] = max(err["R"], np.abs(_quat_R(rows[:, 3:7]) - Rm).max())
            err["v"] = max(err["v"], (np.abs(rows[:, 7:10] - V) / (1 + np.linalg.norm(V, axis=-1, keepdims=True))).max())
            err["w"] = max(err["w"], (np.abs(rows[:, 10:13] - W) / (1 + np.linalg.norm(W, axis=-1, keepdims=True))).max())
    print("rigid-body rows vs float64:", {k: float("%.3g" % v) for k, v in err.items()})
    # measured on an MI355X (8192 robots): p 5.9e-7 m, R 6.8e-7, v 7.5e-7, w 6.2e-7 (relative to 1 + |.|); bounds about 5 x that
    assert err["p"] <= 3e-6 and err["R"] <= 3e-6, err
    assert err["v"] <= 4e-6 and err["w"] <= 4e-6, err
    e.close()


def test_foot_rows_in_contact_sit_on_the_ground():
    """the row order ties to the contact forces: on the flat slab, 50 steps with random commands, every foot row whose net contact force
    pushes up by more than 1 N has its origin (the foot sphere's centre) within 5 mm of [ground, ground + foot radius + contact_offset]"""
    N = 256
    d, k, _ = make_desc("go1plane", N)
    assert not d.ground_height and d.npc_kind == abi.NPC["none"]
    e = hip_engine(d, k)
    e.set_rigid_body_refresh(True)
    e.reset_all()
    A = d.num_agents
    feet = torch.tensor([17 * a + f for a in range(A) for f in (4, 8, 12, 16)])
    r_foot = d.robot.sphere_radius[0]
    lo, hi = d.ground_z - 0.005, d.ground_z + r_foot + d.contact_offset + 0.005
    g = torch.Generator().manual_seed(11)
    n_touch = 0
    for t in range(50):
        cmd = ((torch.rand(N * A, 3, generator=g) * 2 - 1) * torch.tensor([1.5, 0.5, 1.0])).cuda().contiguous()
        e.step_command(cmd)
        torch.cuda.synchronize()
        fz = e.tensor(abi.T_CONTACT_FORCE)[:, feet, 2]
        z = e.tensor(abi.T_RIGID_BODY_STATE)[:, feet, 2]
        touch = fz > 1.0
        n_touch += int(touch.sum())
        bad = touch & ((z < lo) | (z > hi))
        assert not bad.any(), (t, z[bad][:8].tolist(), fz[bad][:8].tolist(), (lo, hi))
    assert n_touch > N * A * 50, n_touch          # robots stand on about two feet or more on average
    e.close()


def test_envs_reset_in_the_step_show_their_terminal_pose():
    """episodes of 5 steps with random start lengths: time-outs land on every step.  The fused handle (refresh on) against a twin loaded with
    the same state before every step and stepped in the staged form: envs that did not reset show their new root rows; envs that did show
    the rows the twin had between POST_NPC and POST_RESET, i.e. after the physics and before the reset (as upstream's refresh in
    post_physics_step)."""
    N = 96
    d1, k1, _ = make_desc("go1gate", N, max_episode_length=5)
    d2, k2, _ = make_desc("go1gate", N, max_episode_length=5)
    ea, eb = hip_engine(d1, k1), hip_engine(d2, k2)
    ea.set_rigid_body_refresh(True)
    ea.reset_all()
    A = d1.num_agents
    g = torch.Generator().manual_seed(5)
    ea.tensor(abi.T_EPISODE_LENGTH).copy_(torch.randint(0, 5, (N,), generator=g, dtype=torch.int32).cuda())
    n_reset = n_kept = 0
    for t in range(8):
        cmd = ((torch.rand(N * A, 3, generator=g) * 2 - 1) * torch.tensor([1.5, 0.5, 1.0])).cuda().contiguous()
        eb.load_state(ea.save_state())
        ea.step_command(cmd)
        eb.policy_step(cmd)
        for k in range(d2.decimation):
            eb.compute_torques(); eb.simulate(); eb.post_decimation_step(k)
        eb.post_physics_stage(abi.POST_FRAME)
        eb.post_physics_stage(abi.POST_NPC)
        terminal = eb.tensor(abi.T_ROOT_STATE)[:, :A].clone()
        eb.post_physics_stage(abi.POST_RESET)
        eb.post_physics_stage(abi.POST_OBS)
        eb.post_physics_stage(abi.POST_WRAPPER)
        torch.cuda.synchronize()
        reset = ea.tensor(abi.T_RESET_BUF).bool()
        assert torch.equal(reset, eb.tensor(abi.T_RESET_BUF).bool()), t
        base = ea.tensor(abi.T_RIGID_BODY_STATE)[:, 0::17][:, :A]
        assert torch.equal(base[~reset], ea.tensor(abi.T_ROOT_STATE)[:, :A][~reset]), t
        assert torch.allclose(base[reset], terminal[reset], rtol=0, atol=1e-6), (t, (base[reset] - terminal[reset]).abs().max().item())
        if reset.any():                                   # the reset moved them
            assert not torch.allclose(base[reset][..., :3], ea.tensor(abi.T_ROOT_STATE)[:, :A][reset][..., :3]), t
        n_reset += int(reset.sum()); n_kept += int((~reset).sum())
    assert n_reset > N and n_kept > N, (n_reset, n_kept)
    ea.close(); eb.close()


_FLAGS = (abi.T_RESET_BUF, abi.T_TIME_OUT_BUF, abi.T_COLLIDE_BUF, abi.T_R_TERM, abi.T_P_TERM, abi.T_Z_HIGH_TERM, abi.T_EPISODE_LENGTH,
          abi.T_RESET_COUNT, abi.T_CONTACT_OVERFLOW)
_VALUES = (abi.T_WRAPPER_OBS, abi.T_WRAPPER_REWARD, abi.T_ROOT_STATE, abi.T_DOF_STATE, abi.T_OBS_BAG)


@pytest.mark.parametrize("task", ["go1gate", "go1sheep-hard", "go1seesaw", "go1football-defender"])
def test_refresh_changes_nothing_else(task):
    """two handles of one scene and seed, the per-step refresh on in one of them, 100 fused wrapper-level steps: flags, counters, the
    returned observation / reward and the root, joint and observation state are bit-identical at every step.  With the refresh on, a scene
    whose post-physics step is the physics kernel's epilogue (go1gate, go1sheep-hard, go1seesaw) runs it as the separate launch; the
    defender scene runs the separate launch either way."""
    N = 512
    d1, k1, _ = make_desc(task, N)
    d2, k2, _ = make_desc(task, N)
    on, off = hip_engine(d1, k1), hip_engine(d2, k2)
    on.set_rigid_body_refresh(True)
    on.reset_all(); off.reset_all()
    Aw = on.tensor(abi.T_WRAPPER_OBS).shape[1]
    g = torch.Generator().manual_seed(13)
    for t in range(100):
        a = (torch.rand(N, Aw, 3, generator=g) * 2 - 1).cuda()
        on.step(a); off.step(a)
        torch.cuda.synchronize()
        for kind in _FLAGS + _VALUES:
            assert torch.equal(on.tensor(kind), off.tensor(kind)), (task, t, kind)
    rbs = on.tensor(abi.T_RIGID_BODY_STATE)
    assert torch.isfinite(rbs).all() and rbs.abs().sum() > 0
    on.close(); off.close()


def _refreshed(task, N=32, steps=3, seed=17):
    d, k, _ = make_desc(task, N)
    e = hip_engine(d, k)
    e.set_rigid_body_refresh(True)
    e.reset_all()
    Aw = e.tensor(abi.T_WRAPPER_OBS).shape[1]
    g = torch.Generator().manual_seed(seed)
    for t in range(steps):
        e.step((torch.rand(N, Aw, 3, generator=g) * 2 - 1).cuda())
    torch.cuda.synchronize()
    return d, e, g


@pytest.mark.parametrize("task", ["go1sheep-hard", "go1pushbox"])
def test_free_npc_rows_are_their_root_rows(task):
    """a free NPC's row is its root row.  The per-step refresh runs before the NPC script (the sheep's walk moves them afterwards, as
    upstream's _step_npc follows its refresh), so the rows are compared after a refresh from the current state"""
    d, e, _ = _refreshed(task)
    A, P = d.num_agents, d.num_npcs
    e.refresh_rigid_body_state()
    torch.cuda.synchronize()
    rbs = e.tensor(abi.T_RIGID_BODY_STATE)
    assert rbs.shape[1] == 17 * A + P
    assert torch.equal(rbs[:, 17 * A:], e.tensor(abi.T_ROOT_STATE)[:, A:])
    e.close()


@pytest.mark.parametrize("task,axis", [("go1seesaw", 1), ("go1revolvingdoor", 2), ("go1tug", 3)])
def test_one_dof_link_rows_follow_the_npc_dof(task, axis):
    """the fixed base's row is its root row; the link's row: base origin + seesaw_joint_offset, then a rotation about +y (seesaw plank) /
    +z (revolving door) by the dof angle with w = R axis theta_dot, or a slide along +y (tug cylinder) with velocity s_dot"""
    d, e, g = _refreshed(task)
    A, N = d.num_agents, d.num_envs
    assert d.seesaw_axis == axis
    dof, root = e.tensor(abi.T_DOF_STATE), e.tensor(abi.T_ROOT_STATE)
    th = (torch.rand(N, generator=g) * 2 - 1) * 0.4
    thd = (torch.rand(N, generator=g) * 2 - 1) * 2.0
    dof[:, 12 * A, 0] = th.cuda(); dof[:, 12 * A, 1] = thd.cuda()
    e.refresh_rigid_body_state()
    torch.cuda.synchronize()
    rbs = e.tensor(abi.T_RIGID_BODY_STATE)
    assert rbs.shape[1] == 17 * A + 2
    assert torch.equal(rbs[:, 17 * A], root[:, A])
    link, base = _np(rbs[:, 17 * A + 1]), _np(root[:, A])
    th, thd = th.double().numpy(), thd.double().numpy()
    p = base[:, :3] + np.asarray(list(d.seesaw_joint_offset), np.float64)
    R = np.tile(np.eye(3), (N, 1, 1))
    v, w = np.zeros((N, 3)), np.zeros((N, 3))
    if axis == 3:
        p[:, 1] += th
        v[:, 1] = thd
    else:
        ax = np.array([0.0, 1.0, 0.0]) if axis == 1 else np.array([0.0, 0.0, 1.0])
        R = np.array([rigid_ref.rodrigues(ax, a) for a in th])
        w = np.einsum("nij,j->ni", R, ax) * thd[:, None]
    assert np.abs(link[:, :3] - p).max() <= 1e-5
    assert np.abs(_quat_R(link[:, 3:7]) - R).max() <= 1e-6
    assert np.abs(np.linalg.norm(link[:, 3:7], axis=-1) - 1).max() <= 1e-6
    assert np.abs(link[:, 7:10] - v).max() <= 1e-6 and np.abs(link[:, 10:13] - w).max() <= 1e-6
    e.close()


def test_static_scenery_rows_are_the_actor_pose_at_rest():
    d, e, _ = _refreshed("go1bridge")
    A = d.num_agents
    rbs, root = e.tensor(abi.T_RIGID_BODY_STATE), e.tensor(abi.T_ROOT_STATE)
    nrb = d.npc_reported_bodies * d.num_npcs
    assert nrb >= 2 and rbs.shape[1] == 17 * A + nrb
    for j in range(nrb):
        assert torch.equal(rbs[:, 17 * A + j, :7], root[:, A, :7]), j
        assert (rbs[:, 17 * A + j, 7:] == 0).all(), j
    e.close()


def test_go1_override_sees_the_rows_of_this_step():
    """a Go1 subclass whose compute_reward reads self.all_rigid_body_states (the staged Go1-level path): the base rows equal root_states at
    that point of every step, the view is the same object across steps, and its contents move"""
    from mqe.envs.configs.go1_gate_config import Go1GateCfg
    from mqe.envs.go1.go1 import Go1
    N = 16

    class Probe(Go1):
        def compute_reward(self):
            rbs = self.all_rigid_body_states
            A = self.num_agents
            self.seen.append((rbs, rbs.view(self.num_envs, -1, 13)[:, 0:17 * A:17].clone(), self.root_states.view(self.num_envs, A, 13).clone(), rbs.clone()))
            self.rew_buf.zero_()

    cfg = type("Go1GateProbe", (Go1GateCfg,), {"env": type("env", (Go1GateCfg.env,), {"num_envs": N})})
    env = Probe(cfg, types.SimpleNamespace(dt=cfg.sim.dt, use_gpu_pipeline=True), None, "cuda:0", True)
    env.seen = []
    env.reset()
    A = env.num_agents
    g = torch.Generator().manual_seed(19)
    for t in range(4):
        env.step(((torch.rand(N * A, 3, generator=g) * 2 - 1) * torch.tensor([1.5, 0.5, 1.0])).cuda())
    torch.cuda.synchronize()
    assert len(env.seen) == 4
    assert all(s[0] is env.seen[0][0] for s in env.seen) and env.all_rigid_body_states is env.seen[0][0]
    assert env.seen[0][0].shape == (N * (17 * A), 13)
    for t, (_, base, root, _) in enumerate(env.seen):
        assert torch.equal(base, root), t
    assert not torch.equal(env.seen[0][3], env.seen[-1][3])
    assert env.feet_indices.device.type == "cuda" and env.feet_indices.tolist() == [4, 8, 12, 16]
    env.close()
