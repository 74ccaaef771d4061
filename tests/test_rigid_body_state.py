"""The rigid-body state tensor's surface on a CPU-only host: the two entry points are declared and exported, the tensor kind agrees between
the header and the Python mirror, the body index lists follow upstream's substring rule (legged_robot.py:804-813,897-907), and
Go1.all_rigid_body_states refuses an engine that has no such tensor (the oracle-backed one)."""
import ctypes as C
import os
import re
import types

import pytest
import torch

from mqe.engine import abi
from mqe.engine.hip_engine import LIB_PATH
from mqe.envs.go1.go1 import Go1

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mqe_hip.h")


def _header_code():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_entry_points_declared_and_exported():
    code = _header_code()
    assert re.search(r"\bint mqe_refresh_rigid_body_state\(mqe_sim\* s, void\* stream\);", code)
    assert re.search(r"\bint mqe_set_rigid_body_refresh\(mqe_sim\* s, int on\);", code)
    assert os.path.isfile(LIB_PATH), "run __graft_entry__.build() first"
    lib = C.CDLL(LIB_PATH)
    assert hasattr(lib, "mqe_refresh_rigid_body_state") and hasattr(lib, "mqe_set_rigid_body_refresh")
    assert lib.mqe_abi_version() == abi.ABI_VERSION == 17


def test_tensor_kind_matches_header_enum():
    code = _header_code()
    body = code[code.index("MQE_T_ROOT_STATE = 0"):code.index("MQE_T_COUNT")]
    kinds = re.findall(r"\b(MQE_T_[A-Z_0-9]+)\b", body)
    assert kinds[-1] == "MQE_T_RIGID_BODY_STATE"
    assert kinds.index("MQE_T_RIGID_BODY_STATE") == abi.T_RIGID_BODY_STATE == abi.T_COUNT - 1


def _oracle_factory(desc, keep, device):
    from oracle_engine import OracleEngine
    return OracleEngine(desc, keep)


def _go1(monkeypatch, cfg):
    from mqe.envs.utils import ENV_DICT  # noqa: F401  (registers the task configs' classes)
    monkeypatch.setattr(Go1, "engine_factory", staticmethod(_oracle_factory))
    monkeypatch.setattr(Go1, "shard", None)
    env_cfg = type("env", (cfg.env,), {"num_envs": 2})
    cfg = type(cfg.__name__ + "Small", (cfg,), {"env": env_cfg})
    sim = types.SimpleNamespace(dt=cfg.sim.dt, use_gpu_pipeline=False)
    return Go1(cfg, sim, None, "cpu", True)


def test_body_indices_on_oracle_backed_go1(monkeypatch):
    from mqe.envs.configs.go1_gate_config import Go1GateCfg
    env = _go1(monkeypatch, Go1GateCfg)
    try:
        for name, want in (("feet_indices", [4, 8, 12, 16]), ("penalised_contact_indices", [0, 2, 6, 10, 14]), ("termination_contact_indices", [0])):
            t = getattr(env, name)
            assert isinstance(t, torch.Tensor) and t.dtype == torch.long, name
            assert t.tolist() == want, (name, t.tolist())
        # they index the robot rows of contact_forces: the feet rows of robot 0 are the rows of a contact-force view
        assert env.contact_forces[:, env.feet_indices].shape == (2, 4, 3)
    finally:
        env.close()


def test_body_indices_empty_without_feet_name(monkeypatch):
    from mqe.envs.configs.go1_gate_config import Go1GateCfg
    asset = type("asset", (Go1GateCfg.asset,), {"foot_name": "None", "penalize_contacts_on": [], "terminate_after_contacts_on": []})
    env = _go1(monkeypatch, type("NoFeetCfg", (Go1GateCfg,), {"asset": asset}))
    try:
        for name in ("feet_indices", "penalised_contact_indices", "termination_contact_indices"):
            t = getattr(env, name)
            assert t.dtype == torch.long and t.numel() == 0, name
    finally:
        env.close()


def test_all_rigid_body_states_refuses_the_oracle_engine(monkeypatch):
    from mqe.envs.configs.go1_gate_config import Go1GateCfg
    env = _go1(monkeypatch, Go1GateCfg)
    try:
        with pytest.raises(NotImplementedError, match="HipEngine"):
            env.all_rigid_body_states
    finally:
        env.close()
