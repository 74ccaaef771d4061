"""Which kernels does mqe_sim_create choose?  For every task at six batch sizes, and for three tasks under each engine switch, creates the
engine under MQE_VERBOSE, takes two steps and prints the creation's `mqe: physics LDS`, `mqe: k_substeps runs` and `mqe: variant` lines.
Two builds of the engine choose alike iff their outputs are equal line by line AND, run under `rocprofv3 --kernel-trace --stats -- python
tools/engine_variants.py`, their kernel-name -> calls tables are equal (the lines do not name the layer-0 and policy-tail kernels).
MQE_HIP_LIB=<other libmqe_hip.so> runs another build.  Run on the GPU box:  python tools/engine_variants.py > variants.txt"""
import os, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "multiagent-quadruped-environment_amd"), os.path.join(ROOT, "tests")]
import torch
from helpers import make_desc, hip_engine
from mqe.engine import abi

TASKS = ["go1plane", "go1gate", "go1sheep-easy", "go1sheep-hard", "go1football-defender", "go1football-1vs1", "go1football-2vs2", "go1seesaw",
         "go1pushbox", "go1revolvingdoor", "go1tug", "go1bridge", "go1wrestling"]
SIZES = [8, 500, 771, 772, 4096, 4097]
SWITCHES = [{"MQE_NO_FUSE_POST": "1"}, {"MQE_NO_FUSE_SUBSTEPS": "1"}, {"MQE_NO_FUSED_TAIL": "1"}, {"MQE_GEMM_SPLIT": "0"}, {"MQE_GEMM_SPLIT": "1"},
            {"MQE_GEMM_HALF": "0"}, {"MQE_ENVS_PER_WAVE": "1"}, {"MQE_ENVS_PER_WAVE": "2"}, {"MQE_LANE_SWEEP": "1"}, {"MQE_ACT_F32": "1"},
            {"MQE_COLLISION_MODEL": "exact"}]
SWITCHED_TASKS = ["go1gate", "go1plane", "go1sheep-hard"]
KEEP = ("mqe: physics LDS", "mqe: k_substeps runs", "mqe: variant")
DESCS = {}       # scene descriptors, built once per (task, batch size, collision model)


def run(task, N, env):
    """the kept stderr lines of one creation (the library writes to the C stderr: caught at the descriptor)"""
    os.environ.update(env, MQE_VERBOSE="1")
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            key = (task, N, env.get("MQE_COLLISION_MODEL"))      # (read by the descriptor builder; every other switch by the engine)
            if key not in DESCS:
                DESCS[key] = make_desc(task, N)[:2]
            e = hip_engine(*DESCS[key])
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            for k in dict(env, MQE_VERBOSE="1"):
                del os.environ[k]
        tmp.seek(0)
        err = tmp.read().decode(errors="replace")
    e.reset_all()
    actions = torch.zeros(N, e.tensor(abi.T_WRAPPER_OBS).shape[1], 3, device=e.torch_device)
    for _ in range(2):
        e.step(actions)
    torch.cuda.synchronize()
    e.close()
    return [ln for ln in err.splitlines() if ln.startswith(KEEP)]


if __name__ == "__main__":
    configs = [(t, n, {}) for t in TASKS for n in SIZES] + [(t, n, sw) for t in SWITCHED_TASKS for sw in SWITCHES for n in SIZES]
    for task, N, env in configs:
        print("== %s num_envs=%d %s" % (task, N, " ".join("%s=%s" % kv for kv in env.items()) or "-"), flush=True)
        for ln in run(task, N, env):
            print("   " + ln, flush=True)
