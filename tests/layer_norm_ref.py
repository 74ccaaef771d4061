"""Host side of the layer-normalisation tests (MQE_ACTOR_LAYER_NORM, MQE_ACTOR_FEATURE_NORM; csrc/kernels_ln.hpp): what is about the norm alone.
The norm's twin -- float64, and float32 in the kernel's own summation order -- and the network walk with norms are rollout_ref.layer_norm and
rollout_ref.forward (below ppo_ref, which walks with them; named here again for the tests); the loss, its autograd (torch.nn.functional.layer_norm:
THE reference), the manual backward at any dtype and the kink-free trajectory are ppo_ref's, called with hidden= and feat=.  Here: the four
networks of the tests, the names of the deliberately wrong variants, the forward yardstick, and the tolerances.

THE BOUNDS follow tests/ppo_ref.py.  Gradient: |g - g64| <= K 2^-24 S_n for every entry of tensor n, exactly 0 where S_n = 0; S_n = the largest
entry of the summed ABSOLUTE per-sample contributions (for a norm: sum |du xhat| for its weight, sum |du| for its bias).  K is MEASURED ON THE
CPU, never on the kernel: the largest ratio reached over K_CASES by two float32 evaluations -- torch autograd on the whole batch, and the manual
backward with the kernel-order norm accumulated over tiles of 64 rows.  The GPU gets K_LN_GPU = 4 K_LN_CPU.  Forward: the yardstick is torch's
float32 CPU evaluation against float64 on the same inputs (forward_errors), the GPU gets 4x.

Measured with this file (tests/test_layer_norm.py prints every case; 36 cases: 4 networks x M in {1, 63, 130} x 3 seeds, value clipping on,
entropy_coef 0.01; the larger of the two float32 evaluations, gradient tensors and statistics together), largest ratio per network and M.  torch's
float32 CPU kernels differ between hosts (another BLAS path, another thread count), and with M = 1 nothing averages, so the table holds two hosts:
                   M = 1     63    130   |  M = 1     63    130      (a second host)
    tanh7_17       13.7    3.9    6.0   |   15.0    3.1    4.0
    relu64x64      23.7   11.2   18.1   |   29.6    9.6   18.6
    tanh256x3      20.3   16.2   10.0   |   46.0    7.8    7.6
    linear         28.6    2.9    4.5   |   19.1    6.9    4.8
The left table is a host whose torch runs 8 CPU threads (torch.get_num_threads()), the right one a host with 16, the kind that also carries the
GPU; tests/test_layer_norm.py runs on both, prints every case, and is expected to reproduce the column of the host it runs on to the printed
digits (left: maximum 28.56, linear, M = 1; right: maximum 46.00, tanh256x3, M = 1, seed 1, the tiled evaluation).  One constant has to hold on
both, since the same test asserts it on both, so K_LN_CPU = 47 is the larger maximum rounded up to the next integer.  A single-host K would be
29 on the left host; the GPU bound 4 K is therefore up to 1.6x wider than that host alone would give, which is the price of one test for both.
From M = 63 up nothing exceeds 18.6 on either.  K_LN_CPU is NOT taken from anything the kernel computes."""
from mqe.engine import abi
import ppo_ref
from rollout_ref import LN_EPS, WAVES, forward, layer_norm, norm_name  # noqa: F401  (the norm's twin and the walk: tests name them through this module)

CLIP, VALUE_CLIP = ppo_ref.CLIP, ppo_ref.VALUE_CLIP
K_LN_CPU = 47.0
K_LN_GPU = 4 * K_LN_CPU

# name: (activation, the actor's hidden widths, the critic's, hidden norm, feature norm) -- the GPU test's four shapes
CASES = {"tanh7_17": ("tanh", (7,), (17,), True, False), "relu64x64": ("relu", (64, 64), (64, 64), True, True),
         "tanh256x3": ("tanh", (256, 256, 256), (256, 256, 256), True, True), "linear": ("tanh", (), (), False, True)}
K_MS = (1, 63, 130)
K_CASES = [(case, M, seed) for case in CASES for M in K_MS for seed in (0, 1, 2)]
VARIANTS_FORWARD = ("unbiased", "eps_outside", "norm_before_act")       # wrong networks: their float32 autograd gradient is the wrong answer
VARIANTS_BACKWARD = ("no_gamma", "no_xhat_term")                       # wrong backward passes of the right network


def dims_of(case, D):
    act, ah, ch, hidden, feat = CASES[case]
    return [D, *ah, 3], [D, *ch, 1], act, hidden, feat


def layout(a_dims, c_dims, hidden, feat):
    return abi.actor_param_layout(a_dims, c_dims, False, hidden, feat)


# ---- the forward yardstick --------------------------------------------------------------------------------------------------------------
def forward_errors(params, a_dims, c_dims, act, hidden, feat, obs):
    """float64 mean / value on obs (the twin), and the yardstick: max |torch float32 CPU - float64| of each"""
    out = {}
    for who, dims, key in (("actor", a_dims, "mean"), ("critic", c_dims, "value")):
        if not dims:
            continue
        p64, p32 = {k: v.double() for k, v in params.items()}, {k: v.float() for k, v in params.items()}
        y64 = forward(p64, who, dims, act, obs.double(), hidden, feat)[0]
        y32 = forward(p32, who, dims, act, obs.float(), hidden, feat, functional=True)[0]
        if key == "value":
            y64, y32 = y64[..., 0], y32[..., 0]
        out[key + "64"], out["yard_" + key] = y64, float((y32.double() - y64).abs().max())
    return out


# ---- the synthetic trajectory and the arguments of ppo_ref's loss functions -----------------------------------------------------------------------
def synth(case, shape, M, seed, weight_scale=1.0):
    """ppo_ref.synth for CASES[case]: the norms' parameters in `params`, and `hidden` and `feat`"""
    a_dims, c_dims, act, hidden, feat = dims_of(case, shape[3])
    return ppo_ref.synth(case, shape, M, seed, dims=(a_dims, c_dims, act), hidden=hidden, feat=feat, weight_scale=weight_scale)


def args_of(s, sel, cfg):
    """(positional, keyword) arguments of ppo_ref.manual / autograd for the minibatch `sel` of a synthetic trajectory"""
    return (s["params"], s["a_dims"], s["c_dims"], s["act"], ppo_ref.batch(s, sel), cfg), dict(hidden=s["hidden"], feat=s["feat"])
