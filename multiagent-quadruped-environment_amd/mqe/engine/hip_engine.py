"""Loader of the HIP engine (csrc/ -> libmqe_hip.so).  There is NO CPU fallback: without the built library or
without a GPU this raises -- the product path never silently runs anything else."""
import ctypes as C
import os

import numpy as np
import torch

from . import abi
from .base import EngineBase, _DevArray, _TORCH_DT

_LIB = None
LIB_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "csrc", "libmqe_hip.so")


def load_library():
    """the process-wide CDLL, every function of include/mqe_hip.h bound to its abi.SIGNATURES entry (once, here: no caller sets a signature)"""
    global _LIB
    if _LIB is None:
        path = os.environ.get("MQE_HIP_LIB", LIB_PATH)       # experiments: an alternative build of the same ABI
        if path != LIB_PATH:
            import sys
            print(f"mqe: override in effect: MQE_HIP_LIB={path} (not the in-tree build)", file=sys.stderr)      # never silent
        elif not os.path.isfile(LIB_PATH):
            raise RuntimeError(f"HIP engine not built: {LIB_PATH} missing (run `python -c 'import __graft_entry__ as g; g.build()'`)")
        lib = C.CDLL(path)
        abi.bind(lib)
        _LIB = lib
    return _LIB


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _need_f32(what, t, shape):
    if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == shape):
        raise ValueError(f"{what} must be a contiguous float32 device tensor of shape {shape}")


def _need_flags(what, t, shape):
    if not (t.is_cuda and t.dtype in (torch.bool, torch.uint8) and t.is_contiguous() and tuple(t.shape) == shape):
        raise ValueError(f"{what} must be a contiguous bool or uint8 device tensor of shape {shape}")


def _need_packed(traj):
    if traj.packed.dtype != torch.float32 or not traj.packed.is_cuda or traj.packed.stride(1) != 1:
        raise ValueError("traj.packed must be a float32 device tensor (T + 1, row_stride) with unit stride along a row")


class Rollout:
    """A trajectory of HipEngine.rollout: `packed` (T+1, row_stride) is the one tensor the steps wrote -- row 0 the starting observation, row
    t + 1 what step t returned (obs | reward | done bytes) -- and obs / reward / done are views of it; actions are the UNCLIPPED samples,
    logp their log-density, value[t] the critic at obs[t] (value[T]: the bootstrap value), None without a critic.  None unless asked for:
    time_outs (T, N) bool, the time-out flags of every step (rollout(time_outs=True)); advantages / returns (T, N, A') and adv_stats
    (float32 [2]: mean, std of the advantages before normalisation; normalising calls only), filled by HipEngine.gae.  hidden (T + 1, N, A', Hs):
    the recurrent state of a recurrent actor, a view of the rows' tails (rollout(record_hidden=True); None otherwise) -- hidden[t] is the
    UNMASKED state step t starts from (row 0: the state the call started from), the actor's Ha floats, then the critic's Hc; step t evaluates
    from hidden[t] * (1 - done[t - 1]) (t = 0: unmasked), OpenRL's (rnn_states[t], masks[t])."""

    def __init__(self, packed, actions, logp, value, shape, time_outs=None, advantages=None, returns=None, adv_stats=None, hidden_width=0):
        N, Aw, D = shape
        n, nr = N * Aw * D, N * Aw
        self.packed, self.actions, self.logp, self.value = packed, actions, logp, value
        self.T = packed.shape[0] - 1
        self.obs = packed[:, :n].view(self.T + 1, N, Aw, D)
        self.reward = packed[1:, n:n + nr].view(self.T, N, Aw)
        self.done = packed[1:, n + nr:].view(torch.uint8)[:, :N].view(torch.bool)      # the byte tail of every row, seen as bool in place
        self.time_outs = time_outs.view(torch.bool) if time_outs is not None and time_outs.dtype == torch.uint8 else time_outs
        self.advantages, self.returns, self.adv_stats = advantages, returns, adv_stats
        p4 = (n + nr + (N + 3) // 4 + 3) // 4 * 4
        self.hidden = packed[:, p4:p4 + nr * hidden_width].view(self.T + 1, N, Aw, hidden_width) if hidden_width else None

    def next_hidden(self):
        """the state a following rollout(hidden=...) continues from: hidden[T], zero where the last step ended its env's episode"""
        if self.hidden is None:
            raise ValueError("next_hidden: the trajectory holds no recurrent state (rollout(record_hidden=True) on a recurrent actor)")
        h = self.hidden[self.T]
        return torch.where(self.done[self.T - 1][:, None, None], torch.zeros((), dtype=h.dtype, device=h.device), h)      # exactly 0.0f, as the engine masks


class HipEngine(EngineBase):
    prefix = "mqe_"
    device = "cuda"

    def __init__(self, desc, keepalive, device="cuda:0"):
        if not torch.cuda.is_available():
            raise RuntimeError("mqe HIP engine needs an AMD GPU (torch.cuda.is_available() is False); there is no CPU path")
        self.torch_device = torch.device(device)
        torch.cuda.set_device(self.torch_device)
        super().__init__(load_library(), desc, keepalive)
        self._actor = self._actor_views = self._height_live = None
        self._n_policy = 0          # policy steps so far: the slot of T_HISTORY's ring (history())
        self.ppo_step = 0           # Adam steps taken by ppo_update

    def _invoke(self, name, *args):
        """mqe_<name>(handle, *args) for the entry points whose refusals callers tell apart by name and code"""
        rc = getattr(self.lib, "mqe_" + name)(self.h, *args)
        if rc != 0:
            raise RuntimeError(f"mqe_{name} failed ({rc}): {self.lib.mqe_last_error().decode()}")

    def _need_actor(self):
        if self._actor is None:
            raise RuntimeError("no actor: call create_actor first")

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.torch_device).cuda_stream)

    def _wrap(self, ptr, shape, dtype):
        typestr = {0: "<f4", 1: "<i4", 2: "|u1"}[dtype]
        return torch.as_tensor(_DevArray(ptr, shape, typestr), device=self.torch_device)

    def policy_step(self, command):
        assert command.is_cuda and command.dtype == torch.float32 and command.is_contiguous()
        self._call("policy_step", C.c_void_p(command.data_ptr()), self._stream())
        self._n_policy += 1

    def compute_torques(self):
        self._call("compute_torques", self._stream())

    def simulate(self):
        self._call("simulate", self._stream())

    def post_decimation_step(self, i):
        self._call("post_decimation_step", int(i), self._stream())

    def post_physics_step(self):
        self._call("post_physics_step", self._stream())

    def post_physics_stage(self, stages):
        """mqe_post_physics_stage: an OR of abi.POST_* (post_physics_step in the stages the reference's method has)"""
        self._call("post_physics_stage", int(stages), self._stream())

    def reset_all(self):
        self._call("reset_all", self._stream())

    def step_command(self, command):
        """Fused Go1.step for control type C (mqe_step_command): (R, num_command_dims) per-robot command rows on the device."""
        assert command.is_cuda and command.dtype == torch.float32 and command.is_contiguous()
        self._call("step_command", C.c_void_p(command.data_ptr()), self._stream())
        self._n_policy += 1

    def step_joint(self, actions12):
        """Fused step for control types P / V / T: (R, 12) joint-space actions on the device."""
        assert actions12.is_cuda and actions12.dtype == torch.float32 and actions12.is_contiguous()
        self._call("step_joint", C.c_void_p(actions12.data_ptr()), self._stream())

    def step(self, actions, between=None, before_tail=None):
        """mqe_step; with `between` (a callable) the two halves mqe_step_begin / mqe_step_end with the callable's own
        launches placed after the policy kernels and before the physics kernel; with `before_tail` as well the policy itself in two
        parts, mqe_step_head / mqe_step_tail, with that callable's launches after layer 0 (see include/mqe_hip.h)."""
        assert actions.is_cuda and actions.dtype == torch.float32 and actions.is_contiguous()
        if between is None and before_tail is None:
            self._call("step", C.c_void_p(actions.data_ptr()), self._stream())
        elif before_tail is not None:
            self._call("step_head", C.c_void_p(actions.data_ptr()), self._stream())
            try:
                before_tail()
            finally:
                self._call("step_tail", self._stream())
                try:
                    if between is not None:
                        between()
                finally:
                    self._call("step_end", self._stream())
        else:
            self._call("step_begin", C.c_void_p(actions.data_ptr()), self._stream())
            try:
                between()
            finally:
                self._call("step_end", self._stream())
        self._n_policy += 1

    def set_return_buffer(self, packed):
        """mqe_set_return_buffer: the following launches write obs | reward | done into `packed` (None: the engine's own buffer)"""
        if packed is not None:
            assert packed.is_cuda and packed.dtype == torch.float32 and packed.is_contiguous()
            assert packed.numel() >= self.tensor(abi.T_WRAPPER_PACKED).numel()
        self._call("set_return_buffer", C.c_void_p(packed.data_ptr() if packed is not None else None))

    # ---- on-device rollouts (mqe_actor_create / mqe_actor_params / mqe_rollout) -------------------------------------------------------
    def create_actor(self, actor_dims, critic_dims=None, activation="tanh", action_gain=1.0, value_norm=False, layer_norm=False, feature_norm=False,
                     recurrent=False, transformer=False):
        """The engine's actor (and critic): MLPs on the task observation.  actor_dims = (D, hidden ..., 3), critic_dims = (D, hidden ..., 1)
        or None; activation "tanh" / "relu" on every hidden layer; the step receives action_gain * a.  Parameters start at zero: fill the
        views of actor_params().  A second call replaces the first.  value_norm (needs a critic): the engine keeps OpenRL's ValueNorm beside
        the parameters (abi.ACTOR_VALUE_NORM; csrc/kernels_vn.hpp states the arithmetic): the critic's outputs are in units of the running
        (mu, sigma) of the returns, and gae / ppo_grad / ppo_update follow (their value_norm=None).  layer_norm / feature_norm
        (abi.ACTOR_LAYER_NORM / ACTOR_FEATURE_NORM; csrc/kernels_ln.hpp states the arithmetic): torch.nn.LayerNorm(n, eps=1e-5) behind every
        hidden activation / on the observation in front of layer 0, in both networks; their weights start at 1, and rollout, gae, ppo_grad,
        adam_step and ppo_update work unchanged on such an actor.  recurrent (abi.ACTOR_RECURRENT; csrc/kernels_gru.hpp states the arithmetic): a
        torch.nn.GRU cell H -> H (H = the last hidden width; every network needs a hidden layer) in front of the output layer of both networks,
        followed by a LayerNorm(H) under layer_norm; the engine carries the state across rollout calls, zeroed here and reset wherever a step ended
        an episode.  rollout, gae and adam_step work on such an actor; ppo_grad and ppo_update take it with chunk_length= (back-propagation through time over
        chunks of a trajectory recorded with rollout(record_hidden=True)) and refuse it without.  transformer (abi.ACTOR_TRANSFORMER;
        csrc/kernels_mat.hpp states the network): MAT, the Multi-Agent Transformer -- actor_dims = (D, E, 3), critic_dims = (D, E, 1) or None for
        the same; the parameters are mqe.utils.actor_net.MATNet's (abi.mat_param_blocks).  rollout, gae and adam_step work on such an actor;
        ppo_grad and ppo_update refuse it: the gradient through the attention is not in the engine yet."""
        actor_dims = [int(x) for x in actor_dims]
        if transformer and critic_dims is None and len(actor_dims) == 3:
            critic_dims = [actor_dims[0], actor_dims[1], 1]          # the encoder always carries the value head
        critic_dims = [int(x) for x in critic_dims] if critic_dims is not None else []
        for who, dims in (("actor", actor_dims), ("critic", critic_dims)):
            if len(dims) - 1 > abi.ACTOR_MAX_LAYERS:         # mqe_actor_shape has no room for them: never reaches the library
                raise ValueError(f"create_actor: {who}: {len(dims) - 1} Linear layers, at most {abi.ACTOR_MAX_LAYERS} (abi.ACTOR_MAX_LAYERS)")
        if activation not in ("tanh", "relu"):
            raise ValueError(f"activation must be 'tanh' or 'relu', got {activation!r}")
        sh = abi.ActorShape()
        sh.obs_dim, sh.act_dim = actor_dims[0], 3
        sh.actor_layers, sh.critic_layers = len(actor_dims) - 1, max(len(critic_dims) - 1, 0)
        for i, v in enumerate(actor_dims):
            sh.actor_dims[i] = v
        for i, v in enumerate(critic_dims):
            sh.critic_dims[i] = v
        sh.activation = ((abi.ACTOR_RELU if activation == "relu" else abi.ACTOR_TANH) | (abi.ACTOR_VALUE_NORM if value_norm else 0)
                         | (abi.ACTOR_LAYER_NORM if layer_norm else 0) | (abi.ACTOR_FEATURE_NORM if feature_norm else 0)
                         | (abi.ACTOR_RECURRENT if recurrent else 0) | (abi.ACTOR_TRANSFORMER if transformer else 0))
        sh.action_gain = float(action_gain)
        self._invoke("actor_create", C.byref(sh))
        self._actor = dict(actor_dims=actor_dims, critic_dims=critic_dims or None, activation=activation, action_gain=float(action_gain),
                           value_norm=bool(value_norm), layer_norm=bool(layer_norm), feature_norm=bool(feature_norm), recurrent=bool(recurrent),
                           transformer=bool(transformer))
        self._actor_views = None
        self.ppo_step = 0            # the library dropped Adam's moments with the old actor

    def actor_params(self):
        """{name: zero-copy view} of the engine's parameter buffer (abi.actor_param_layout: actor.0.weight, actor.0.bias, ..., critic.0.weight,
        ..., log_std) + "flat", the trainable parameters (what ppo_grad, adam_step and optimizer_state size against).  Live device memory: copy_
        into the views; later launches on the stream see the values.  An actor created with value_norm also has "value_norm", the five
        state floats (m, q, d, mu, sigma) behind log_std, and "all", the whole buffer = a learner checkpoint's parameter part."""
        self._need_actor()
        if self._actor_views is None:
            v = abi.TensorView()
            self._call("actor_params", C.byref(v))
            flat = self._wrap(v.ptr, [int(v.shape[0])], v.dtype)
            vn = self._actor["value_norm"]
            layout = abi.actor_param_layout(self._actor["actor_dims"], self._actor["critic_dims"], vn, self._actor["layer_norm"], self._actor["feature_norm"],
                                            self._actor["recurrent"], self._actor.get("transformer", False))
            views = {n: flat[o:o + int(np.prod(shp))].view(shp) for n, (o, shp) in layout.items()}
            if vn:
                views["all"] = flat
                flat = flat[:layout["value_norm"][0]]
            views["flat"] = flat
            self._actor_views = views
        return self._actor_views

    def rollout_row_stride(self):
        """floats of one row of a trajectory's packed tensor: the T_WRAPPER_PACKED length rounded up to a multiple of 4"""
        return (self.tensor(abi.T_WRAPPER_PACKED).numel() + 3) // 4 * 4

    def hidden_width(self):
        """Hs = Ha + Hc: the floats of a row's recurrent state (the last hidden widths of the actor and the critic); 0 unless the actor is recurrent"""
        a = self._actor
        if a is None or not a["recurrent"]:
            return 0
        return a["actor_dims"][-2] + (a["critic_dims"][-2] if a["critic_dims"] else 0)

    def _chunks(self, who, traj, chunk_length, transformer=False):
        """chunk_length of ppo_grad / ppo_update against the actor and the trajectory: -> L (0: a plain actor, samples), or the refusal.
        transformer: the caller asked for the transformer's on-device gradient (abi.PPO_TRANSFORMER)"""
        rec = self._actor is not None and self._actor["recurrent"]
        mat = self._actor is not None and self._actor.get("transformer", False)
        if transformer:
            if not mat:
                raise ValueError(f"{who}: transformer=True needs the transformer actor (create_actor(transformer=True)); this actor's gradient needs no such switch")
            if chunk_length is not None:
                raise ValueError(f"{who}: transformer=True does not combine with chunk_length= (the transformer carries no state)")
            return 0
        if mat:
            raise NotImplementedError(f"{who}: the actor is the transformer (create_actor(transformer=True)): the gradient through the attention is not in the "
                                      f"engine yet; differentiate the torch twin -- MATNet.evaluate(traj.obs, traj.actions) -- and sync_actor() the result, or "
                                      f"step the engine's buffer with adam_step")
        if chunk_length is None:
            if rec:
                raise NotImplementedError(f"{who}: the actor is recurrent: its gradient is back-propagation through time over chunks of the trajectory, which "
                                          f"the engine runs when asked for: pass chunk_length=L (T a multiple of L; rollout(record_hidden=True))")
            return 0
        L = int(chunk_length)
        if not rec:
            raise ValueError(f"{who}: chunk_length= needs a recurrent actor (create_actor(recurrent=True)); a plain actor's minibatches are samples")
        if not 1 <= L <= abi.PPO_MAX_CHUNK:
            raise ValueError(f"{who}: chunk_length must be 1 .. {abi.PPO_MAX_CHUNK} (abi.PPO_MAX_CHUNK), got {L}")
        if traj.hidden is None:
            raise ValueError(f"{who}: traj.hidden is None: the chunks start from the recorded state (rollout(record_hidden=True))")
        if int(traj.T) % L != 0:
            raise ValueError(f"{who}: the trajectory's T = {int(traj.T)} steps are not a multiple of chunk_length = {L}")
        return L

    def rollout(self, T, obs0=None, deterministic=False, out=None, time_outs=False, hidden=None, record_hidden=False):
        """T steps of actor -> step inside the engine, one host call, no synchronisation (mqe_rollout).  obs0: the (N, A', D) observation to
        start from (None: the engine's own T_WRAPPER_OBS, which a reset, a step without a return buffer of the caller's, and every rollout
        leave current -- NOT a step that was given its own return buffer, as the task wrappers' step() does).  out: a Rollout of the same T whose tensors are written again instead of fresh
        ones.  Returns a Rollout: views of the one packed tensor (obs (T+1, N, A', D), reward (T, N, A'), done (T, N) bool) + actions
        (T, N, A', 3), logp (T, N, A'), value (T+1, N, A') or None without a critic.  time_outs=True: the call also records T_TIME_OUT_BUF as
        every step left it (mqe_rollout_time_outs: one N-byte device copy per step) into Rollout.time_outs, (T, N) bool -- a fresh tensor,
        or out.time_outs; without it the call enqueues what it always did and Rollout.time_outs stays as it was (None on a fresh one).
        A recurrent actor (create_actor(recurrent=True)) continues from the engine's live state; hidden: an (N, A', Hs) float32 device tensor to
        start from instead (copied into row 0's tail; abi.ROLLOUT_HIDDEN_IN); record_hidden: the rows are R' Hs floats wider and Rollout.hidden
        (T + 1, N, A', Hs) views the recorded states (abi.ROLLOUT_HIDDEN_RECORD).  out= needs a packed tensor of that width."""
        self._need_actor()
        T = int(T)
        N, Aw, D = (int(x) for x in self.tensor(abi.T_WRAPPER_OBS).shape)
        dev = self.torch_device
        critic = self._actor["critic_dims"] is not None
        hs = self.hidden_width()
        wide = hidden is not None or record_hidden
        if wide and not hs:
            raise ValueError("rollout: hidden= / record_hidden=True need a recurrent actor (create_actor(recurrent=True))")
        if hidden is not None:
            _need_f32("hidden", hidden, (N, Aw, hs))
        p4 = self.rollout_row_stride()
        need = p4 + N * Aw * hs if wide else 0
        if out is None:
            stride = (need + 3) // 4 * 4 if wide else p4
            out = Rollout(torch.zeros(max(T, 0) + 1, stride, dtype=torch.float32, device=dev), torch.empty(max(T, 0), N, Aw, 3, dtype=torch.float32, device=dev),
                          torch.empty(max(T, 0), N, Aw, dtype=torch.float32, device=dev),
                          torch.empty(max(T, 0) + 1, N, Aw, dtype=torch.float32, device=dev) if critic else None, (N, Aw, D),
                          hidden_width=hs if record_hidden else 0)
        else:
            if out.T != T:
                raise ValueError(f"out holds a trajectory of {out.T} steps, not {T}")
            if out.packed.stride(1) != 1 or out.packed.stride(0) < out.packed.shape[1]:
                raise ValueError("out.packed must be (T + 1, row_stride) with unit stride along a row")
            for name, t, shape in (("actions", out.actions, (T, N, Aw, 3)), ("logp", out.logp, (T, N, Aw)), ("value", out.value, (T + 1, N, Aw))):
                if t is not None:
                    _need_f32(f"out.{name}", t, shape)
            if out.actions is None or out.packed.dtype != torch.float32 or not out.packed.is_cuda:
                raise ValueError("out.packed and out.actions must be float32 device tensors")
            if wide and (out.packed.shape[1] < need or (record_hidden and out.hidden is None)):
                raise ValueError(f"out.packed rows hold {out.packed.shape[1]} floats; with hidden= / record_hidden=True a row takes {need} "
                                 "(the packed length rounded up to a multiple of 4 + N A' Hs state floats): pass a Rollout of rollout(record_hidden=True)")
        if time_outs:
            if out.time_outs is None:
                out.time_outs = torch.zeros(max(T, 0), N, dtype=torch.uint8, device=dev).view(torch.bool)
            _need_flags("out.time_outs", out.time_outs, (T, N))
        if obs0 is not None:
            assert obs0.is_cuda and obs0.dtype == torch.float32 and obs0.is_contiguous() and tuple(obs0.shape) == (N, Aw, D)
        if hidden is not None and T >= 1:
            out.packed[0, p4:p4 + N * Aw * hs].copy_(hidden.reshape(-1))
        if time_outs:
            self._call("rollout_time_outs", _ptr(out.time_outs), max(T, 1))       # T <= 0: mqe_rollout itself refuses
        try:
            self._invoke("rollout", T, _ptr(obs0), _ptr(out.packed), int(out.packed.stride(0)), _ptr(out.actions), _ptr(out.logp), _ptr(out.value),
                         (abi.ROLLOUT_DETERMINISTIC if deterministic else 0) | (abi.ROLLOUT_HIDDEN_IN if hidden is not None else 0)
                         | (abi.ROLLOUT_HIDDEN_RECORD if record_hidden else 0), self._stream())
        finally:
            if time_outs:
                self.lib.mqe_rollout_time_outs(self.h, None, 0)         # the record belongs to this call alone, refused or not
        self._n_policy += T
        return out

    def _value_norm(self, who, value_norm):
        """value_norm=None follows the actor; True on an actor without the state is refused here as the library would"""
        have = self._actor is not None and self._actor["value_norm"]
        if value_norm is None:
            return have
        if value_norm and not have:
            raise ValueError(f"{who}: value_norm=True needs an actor created with value_norm=True")
        return bool(value_norm)

    def gae(self, traj, gamma, lam=0.95, normalize=False, out=None, value_norm=None):
        """GAE(lambda) advantages and returns of a Rollout on the device (mqe_gae; csrc/kernels_gae.hpp states the arithmetic): one launch,
        two with normalize, no synchronisation (the first normalising call of an engine allocates its scratch and synchronises once).
        traj.value is required ((T+1, N, A'); it may have been written by a torch critic); traj.time_outs, when recorded, bootstraps
        timed-out steps with gamma * value (rsl_rl); without it every done is a failure.  normalize: advantages become (adv - mean) /
        (std + 1e-8) over all T x N x A' values of THIS engine's rows (unbiased std), returns stay un-normalised, and traj.adv_stats holds
        (mean, std).  out: a Rollout whose advantages / returns (/ adv_stats) tensors are written instead of fresh ones.  Fills
        traj.advantages, traj.returns (T, N, A') and traj.adv_stats (float32 [2], None without normalize); returns traj.  value_norm (None:
        as the actor was created): traj.value is in NORMALISED units -- what a value-normalising critic predicts -- and the engine
        de-normalises it with the current (mu, sigma) first (abi.GAE_VALUE_NORM: one more launch); advantages and returns are in reward units."""
        vn = self._value_norm("gae", value_norm)
        if traj.value is None:
            raise ValueError("gae: the trajectory has no values (traj.value is None): create the actor with a critic, or fill traj.value")
        T = int(traj.T)
        N, Aw, D = (int(x) for x in self.tensor(abi.T_WRAPPER_OBS).shape)
        dev = self.torch_device
        shape = (T, N, Aw)
        _need_f32("traj.value", traj.value, (T + 1, N, Aw))
        _need_packed(traj)
        rec = traj.time_outs
        if rec is not None:
            _need_flags("traj.time_outs", rec, (T, N))
        adv, ret, stats = (out.advantages, out.returns, out.adv_stats) if out is not None else (None, None, None)
        for name, t, shp in (("advantages", adv, shape), ("returns", ret, shape), ("adv_stats", stats, (2,))):
            if t is not None:
                _need_f32(f"out.{name}", t, shp)
        adv = adv if adv is not None else torch.empty(shape, dtype=torch.float32, device=dev)
        ret = ret if ret is not None else torch.empty(shape, dtype=torch.float32, device=dev)
        if normalize and stats is None:
            stats = torch.empty(2, dtype=torch.float32, device=dev)
        self._invoke("gae", T, _ptr(traj.packed), int(traj.packed.stride(0)), _ptr(traj.value), _ptr(rec), float(gamma), float(lam),
                     (abi.GAE_NORMALIZE if normalize else 0) | (abi.GAE_VALUE_NORM if vn else 0), _ptr(adv), _ptr(ret), _ptr(stats if normalize else None), self._stream())
        traj.advantages, traj.returns, traj.adv_stats = adv, ret, (stats if normalize else None)
        return traj

    # ---- the PPO update on the engine's own parameters (mqe_ppo_grad / mqe_ppo_optimizer / mqe_ppo_adam; csrc/kernels_ppo.hpp) ---------------
    def _ppo_units(self, T, L, joint):
        """(how many, their noun): the units a minibatch of this trajectory is made of -- what index / first / count number (csrc/kernels_ppo.hpp).
        joint: the units are groups (the joint ratio, or the transformer's gradient)"""
        N, Aw, _ = (int(x) for x in self.tensor(abi.T_WRAPPER_OBS).shape)
        return T * N * (1 if joint else Aw) // max(L, 1), ("chunk groups" if L else "groups") if joint else ("chunks" if L else "samples")

    def ppo_grad(self, traj, index=None, first=0, count=None, clip=0.2, value_coef=1.0, entropy_coef=0.0, value_clip=None, out=None, value_norm=None,
                 update_value_norm=False, chunk_length=None, joint=False, dual_clip=None, transformer=False):
        """Gradient of rsl_rl's clipped-surrogate PPO loss over one minibatch of a Rollout that HipEngine.gae has filled, with respect to the
        engine's actor-critic parameters (mqe_ppo_grad; csrc/kernels_ppo.hpp states the loss): two launches, no synchronisation (the first
        call after create_actor allocates its scratch and synchronises once), the same bits on every run.  The minibatch is
        index[first:first + count] (an int32 device tensor of flat sample numbers t * N * A' + row, e.g. a slice of torch.randperm) or, without
        an index, the samples first .. first + count; count=None: everything from `first` on.  value_clip: None (plain squared error) or the
        clamp c_v of the clipped value loss.  out: (grad, stats) tensors to write instead of fresh ones.  -> (grad, stats): grad float32
        [n_params] in actor_params()["flat"]'s layout, stats float32 [6]: mean L_pi, mean L_v, entropy H, L, approximate KL, clip share.
        value_norm (None: as the actor was created): the value loss compares against the minibatch's returns normalised with the current
        (mu, sigma) (abi.PPO_VALUE_NORM: one more launch; mean L_v is then in normalised units, traj.returns stays as it is);
        update_value_norm: the minibatch's returns are folded into the statistics first (abi.PPO_VALUE_NORM_UPDATE: one more launch) -- the
        only call that changes actor_params()["value_norm"].
        chunk_length=L (a recurrent actor, which is refused without it; abi.PPO_BPTT, csrc/kernels_bptt.hpp): truncated back-propagation through
        time, OpenRL's recurrent generator at data_chunk_length = L.  The trajectory (rollout(record_hidden=True), T a multiple of L) is cut into
        (T / L) * N * A' chunks, chunk c = (t0 / L) * N * A' + row covering steps t0 .. t0 + L - 1 of that row; index / first / count are CHUNK
        numbers, the loss averages over the count * L samples, and a chunk starts from the masked recorded state traj.hidden[t0] (data, no
        gradient) and carries the state it computes with the current parameters through its steps, reset where traj.done says so.
        joint=True (abi.PPO_JOINT; OpenRL's use_joint_action_loss): one importance ratio -- the product of the agents' -- and one advantage -- their
        mean -- per env-step; index / first / count are then GROUP numbers t * N + env (with chunk_length: chunk groups (t0 / L) * N + env), each
        standing for the A' samples (chunks) of that env-step, and the policy term averages over the groups; one more small launch.
        dual_clip=c_d (abi.PPO_DUAL_CLIP; OpenRL's dual_clip_ppo / dual_clip_coeff; None: off): where the advantage is negative the surrogate is
        additionally bounded by c_d * adv; c_d > 1 + clip.  csrc/kernels_ppo.hpp states both.
        transformer=True (the transformer actor, which is refused without it; abi.PPO_TRANSFORMER, csrc/kernels_mat_grad.hpp: k_mat_grad): the gradient
        through MAT's encoder, decoder and attention on the device.  index / first / count are GROUP numbers t * N + env whether or not joint is set (the
        attention needs all A' agents of an env-step); the loss is the one above with sigma = 0.5 sigmoid(log_std); joint, dual_clip, value_clip and the
        value normalisation combine with it.  The first such call allocates the activation tapes (abi.mat_grad_scratch_bytes) and synchronises once; a
        width whose working set does not fit the LDS (abi.mat_grad_lds_bytes) is refused there."""
        self._need_actor()
        L = self._chunks("ppo_grad", traj, chunk_length, transformer)
        vn = self._value_norm("ppo_grad", value_norm)
        if update_value_norm and not vn:
            raise ValueError("ppo_grad: update_value_norm=True needs value normalisation (an actor created with value_norm=True)")
        if self._actor["critic_dims"] is None:
            raise ValueError("ppo_grad: the loss has a value term and the actor was created without a critic")
        for name in ("value", "logp", "advantages", "returns"):
            if getattr(traj, name) is None:
                raise ValueError(f"ppo_grad: traj.{name} is None (rollout with a critic, then gae)")
        T = int(traj.T)
        N, Aw, D = (int(x) for x in self.tensor(abi.T_WRAPPER_OBS).shape)
        dev = self.torch_device
        for name, shp in (("actions", (T, N, Aw, 3)), ("logp", (T, N, Aw)), ("value", (T + 1, N, Aw)), ("advantages", (T, N, Aw)), ("returns", (T, N, Aw))):
            _need_f32(f"traj.{name}", getattr(traj, name), shp)
        _need_packed(traj)
        n_params = self.actor_params()["flat"].numel()
        total, what = self._ppo_units(T, L, joint or transformer)
        if index is not None:
            if not (index.is_cuda and index.dtype == torch.int32 and index.is_contiguous() and index.dim() == 1):
                raise ValueError("index must be a contiguous one-dimensional int32 device tensor")
            total = int(index.numel())
        first = int(first)
        count = total - first if count is None else int(count)
        if index is not None and (first < 0 or count < 1 or first + count > total):
            raise ValueError(f"index holds {total} {what}: first={first}, count={count} reach outside it")
        grad, stats = out if out is not None else (None, None)
        for what, t, shp in (("out[0] (grad)", grad, (n_params,)), ("out[1] (stats)", stats, (abi.PPO_STATS,))):
            if t is not None:
                _need_f32(what, t, shp)
        grad = grad if grad is not None else torch.empty(n_params, dtype=torch.float32, device=dev)
        stats = stats if stats is not None else torch.empty(abi.PPO_STATS, dtype=torch.float32, device=dev)
        loss = abi.PpoLossEx(float(clip), float(value_coef), float(entropy_coef), float(value_clip) if value_clip is not None else 0.0,
                             float(dual_clip) if dual_clip is not None else 0.0)
        self._invoke("ppo_grad", T, _ptr(traj.packed), int(traj.packed.stride(0)), _ptr(traj.actions), _ptr(traj.logp), _ptr(traj.value),
                     _ptr(traj.advantages), _ptr(traj.returns), _ptr(index), first, count, C.cast(C.pointer(loss), C.POINTER(abi.PpoLoss)),
                     (abi.PPO_CLIP_VALUE if value_clip is not None else 0) | (abi.PPO_VALUE_NORM if vn else 0) |
                     (abi.PPO_VALUE_NORM_UPDATE if update_value_norm else 0) | ((abi.PPO_BPTT | L << abi.PPO_CHUNK_SHIFT) if L else 0) |
                     (abi.PPO_JOINT if joint else 0) | (abi.PPO_DUAL_CLIP if dual_clip is not None else 0) | (abi.PPO_TRANSFORMER if transformer else 0),
                     _ptr(grad), _ptr(stats), self._stream())
        return grad, stats

    def optimizer_state(self):
        """{"exp_avg", "exp_avg_sq"}: zero-copy views of Adam's two moment buffers (mqe_ppo_optimizer), float32 [n_params] in the layout of
        actor_params()["flat"], zero until the first adam_step; a new create_actor drops them.  With actor_params()["flat"] and the step count
        (HipEngine.ppo_step) they are the whole optimiser checkpoint."""
        self._need_actor()
        m, v = abi.TensorView(), abi.TensorView()
        self._call("ppo_optimizer", C.byref(m), C.byref(v))
        return {"exp_avg": self._wrap(m.ptr, [int(m.shape[0])], m.dtype), "exp_avg_sq": self._wrap(v.ptr, [int(v.shape[0])], v.dtype)}

    def adam_step(self, grad, step, lr, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=None, norm_out=None):
        """One torch.optim.Adam step (no weight decay, no amsgrad) on the engine's parameters, in place, ordered on the stream (mqe_ppo_adam).
        step >= 1 is the caller's count.  max_grad_norm: clip_grad_norm_ over all parameters first (None: off); norm_out: a float32 [1] device
        tensor that receives the unscaled gradient norm."""
        n_params = self.actor_params()["flat"].numel()
        if not (grad.is_cuda and grad.dtype == torch.float32 and grad.is_contiguous() and grad.numel() == n_params):
            raise ValueError(f"grad must be a contiguous float32 device tensor of {n_params} elements")
        if norm_out is not None and not (norm_out.is_cuda and norm_out.dtype == torch.float32 and norm_out.numel() >= 1):
            raise ValueError("norm_out must be a float32 device tensor")
        self._invoke("ppo_adam", grad.data_ptr(), int(step), float(lr), float(betas[0]), float(betas[1]), float(eps),
                     float(max_grad_norm) if max_grad_norm is not None else 0.0, _ptr(norm_out), self._stream())

    def ppo_update(self, traj, epochs, minibatches, lr, clip=0.2, value_coef=1.0, entropy_coef=0.0, value_clip=None, betas=(0.9, 0.999), eps=1e-8,
                   max_grad_norm=None, generator=None, value_norm=None, chunk_length=None, joint=False, dual_clip=None, transformer=False):
        """The PPO update of one trajectory inside the engine: per epoch one device permutation of the T x N x A' samples
        (torch.randperm(..., device=..., generator=generator)), cut into `minibatches` equal slices (the last takes the remainder), and per
        slice ppo_grad + adam_step -- 2 to 4 launches, no synchronisation, no copy.  The step count lives on this object (ppo_step) and carries
        over between calls.  -> the (epochs, minibatches, 6) statistics tensor (ppo_grad's, before each step).  Afterwards the engine's buffer
        is the master copy of the parameters.  value_norm (None: as the actor was created): every minibatch first folds its returns into
        the running statistics, then normalises them with the new (mu, sigma) -- OpenRL's ValueNorm order; 1 or 2 more launches a slice.
        chunk_length=L (a recurrent actor, refused without it; ppo_grad's): what is permuted and cut into minibatches are the (T / L) * N * A'
        chunks, and `minibatches` is bounded by their number; one launch more a slice under value normalisation.
        joint, dual_clip: ppo_grad's (OpenRL's use_joint_action_loss; dual_clip_ppo with dual_clip_coeff).  With joint what is permuted and cut are
        the T * N groups (the (T / L) * N chunk groups), `minibatches` is bounded by their number, and a slice costs one launch more.
        transformer=True (the transformer actor, refused without it; ppo_grad's): the update through k_mat_grad -- rollout, gae and this call, and the
        parameters never leave the buffer the actor reads.  What is permuted and cut are the T * N groups, and `minibatches` is bounded by their number."""
        self._need_actor()
        L = self._chunks("ppo_update", traj, chunk_length, transformer)
        vn = self._value_norm("ppo_update", value_norm)
        epochs, minibatches = int(epochs), int(minibatches)
        total, what = self._ppo_units(int(traj.T), L, joint or transformer)
        if epochs < 1 or minibatches < 1 or minibatches > total:
            raise ValueError(f"ppo_update: epochs >= 1 and 1 <= minibatches <= {total} {what}")
        dev = self.torch_device
        stats = torch.empty(epochs, minibatches, abi.PPO_STATS, dtype=torch.float32, device=dev)
        grad = torch.empty(self.actor_params()["flat"].numel(), dtype=torch.float32, device=dev)
        per = total // minibatches
        for e in range(epochs):
            perm = torch.randperm(total, device=dev, generator=generator).to(torch.int32)
            for b in range(minibatches):
                first = b * per
                count = per if b + 1 < minibatches else total - first
                self.ppo_grad(traj, index=perm, first=first, count=count, clip=clip, value_coef=value_coef, entropy_coef=entropy_coef,
                              value_clip=value_clip, out=(grad, stats[e, b]), value_norm=vn, update_value_norm=vn, chunk_length=chunk_length, joint=joint,
                              dual_clip=dual_clip, transformer=transformer)
                self.ppo_step += 1
                self.adam_step(grad, self.ppo_step, lr, betas=betas, eps=eps, max_grad_norm=max_grad_norm)
        return stats

    def defender_command(self, out):
        self._call("defender_command", C.c_void_p(out.data_ptr()), self._stream())

    def wrapper_eval(self, is_reset):
        self._call("wrapper_eval", int(is_reset), self._stream())

    def save_state(self):
        """Checkpoint: every state buffer of the handle + its ring positions as one host blob (numpy uint8); see mqe_state_save.
        Not part of it: a caller-owned return buffer (mqe_set_return_buffer) and the wrappers' host-side counters."""
        blob = np.empty(int(self.lib.mqe_state_size(self.h)) + 8, np.uint8)
        self._call("state_save", C.c_void_p(blob.ctypes.data), self._stream())
        blob[-8:] = np.frombuffer(np.int64(self._n_policy).tobytes(), np.uint8)      # host-side frame counter of history()
        return blob

    def load_state(self, blob):
        blob = np.ascontiguousarray(blob, np.uint8)
        want = int(self.lib.mqe_state_size(self.h)) + 8
        if blob.nbytes != want:     # the C side checks the header against the handle, not the length of the caller's buffer
            raise ValueError(f"checkpoint blob has {blob.nbytes} bytes, this handle's state takes {want} (truncated file or another scene shape)")
        self._call("state_load", C.c_void_p(blob.ctypes.data), self._stream())
        self._n_policy = int(np.frombuffer(blob[-8:].tobytes(), np.int64)[0])

    def render_depth(self, height, width, hfov_deg, pos, rpy, far=20.0, out=None):
        """forward depth images of every robot from the current state: (R, height, width) device tensor, negative depth along the optical
        axis, -inf = nothing within `far` (mqe_render_depth)"""
        R = self.desc.num_envs * self.desc.num_agents
        if out is None:
            out = torch.empty(R, int(height), int(width), dtype=torch.float32, device=self.torch_device)
        p3, r3 = (C.c_float * 3)(*[float(x) for x in pos]), (C.c_float * 3)(*[float(x) for x in rpy])
        self._invoke("render_depth", out.data_ptr(), int(height), int(width), float(hfov_deg), p3, r3, float(far), self._stream())
        return out

    def render_view(self, env, height, width, hfov_deg, eye, lookat, far=60.0, rgba=None, geom=False, ids=False):
        """one image of env `env` from a free camera at the world point `eye` looking at `lookat`, from the current state (mqe_render_view;
        include/mqe_hip.h is the specification): the (H, W, 4) uint8 colour image, Isaac Gym's IMAGE_COLOR layout, as a device tensor
        (`rgba`: a tensor to fill instead of a fresh one).  geom / ids: a tuple that adds the (H, W, 4) float tensor (negative axial depth,
        -inf on a miss; world normal facing the eye) and / or the (H, W) int32 id words (abi.VIEW_*).  One launch, no synchronisation."""
        H, W = int(height), int(width)
        if H <= 0 or W <= 0 or H * W > abi.VIEW_MAX_PIXELS:
            raise ValueError(f"render_view: resolution {H} x {W} out of range (height * width <= {abi.VIEW_MAX_PIXELS})")
        dev = self.torch_device
        if rgba is None:
            rgba = torch.empty(H, W, 4, dtype=torch.uint8, device=dev)
        assert rgba.is_cuda and rgba.dtype == torch.uint8 and rgba.is_contiguous() and rgba.numel() == H * W * 4
        g = torch.empty(H, W, 4, dtype=torch.float32, device=dev) if geom else None
        i = torch.empty(H, W, dtype=torch.int32, device=dev) if ids else None
        e3, l3 = (C.c_float * 3)(*[float(x) for x in eye]), (C.c_float * 3)(*[float(x) for x in lookat])
        self._invoke("render_view", int(env), rgba.data_ptr(), _ptr(g), _ptr(i), H, W, float(hfov_deg), e3, l3, float(far), self._stream())
        out = (rgba,) + ((g,) if geom else ()) + ((i,) if ids else ())
        return out if len(out) > 1 else rgba

    def refresh_rigid_body_state(self):
        """gym.refresh_rigid_body_state_tensor: tensor(T_RIGID_BODY_STATE) from the current root and dof state (mqe_refresh_rigid_body_state)"""
        self._call("refresh_rigid_body_state", self._stream())

    def set_rigid_body_refresh(self, on):
        """on: every post-physics step refreshes tensor(T_RIGID_BODY_STATE) first, after the physics and before termination and resets
        (mqe_set_rigid_body_refresh); off (the default): no step touches it"""
        self._call("set_rigid_body_refresh", int(bool(on)))

    def _height_grid(self, points_xy):
        """(P, 2) base-frame offsets -> contiguous float32 host array (mqe_measure_heights' points_xy)"""
        if isinstance(points_xy, torch.Tensor):
            points_xy = points_xy.detach().cpu().numpy()
        pts = np.ascontiguousarray(points_xy, np.float32)
        if pts.ndim != 2 or pts.shape[1] != 2:
            raise ValueError(f"points_xy must be (P, 2) base-frame offsets, got {pts.shape}")
        return pts

    def _height_call(self, name, out, pts, scenery, *tail):
        self._invoke(name, _ptr(out), pts.ctypes.data if pts is not None else None, int(pts.shape[0]) if pts is not None else 0,
                     abi.HSCAN_SCENERY if scenery else 0, *tail)

    def measure_heights(self, points_xy, out=None, scenery=False):
        """(R, P) device tensor: the height of the static surface under the yaw-aligned grid `points_xy` ((P, 2) base-frame offsets) around
        every robot, from the current root state, absolute world z (mqe_measure_heights).  scenery: the static scenery boxes' tops count.
        `out`: a float32 device tensor of R * P contiguous elements to fill (4-byte alignment suffices)"""
        pts = self._height_grid(points_xy)
        R = self.desc.num_envs * self.desc.num_agents
        if out is None:
            out = torch.empty(R, pts.shape[0], dtype=torch.float32, device=self.torch_device)
        assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == R * pts.shape[0]
        self._height_call("measure_heights", out, pts, scenery, self._stream())
        return out

    def set_height_refresh(self, points_xy, scenery=False):
        """registers the scan every post-physics step refreshes first -- after the physics, before termination and resets
        (mqe_set_height_refresh) -- and returns the live (R, P) tensor the engine object owns; None drops it (no step launches it: the default)"""
        if points_xy is None:
            self._height_call("set_height_refresh", None, None, False)
            self._height_live = None
            return None
        pts = self._height_grid(points_xy)
        R = self.desc.num_envs * self.desc.num_agents
        live = self._height_live
        if live is None or live.shape != (R, pts.shape[0]):
            live = torch.zeros(R, pts.shape[0], dtype=torch.float32, device=self.torch_device)
        self._height_call("set_height_refresh", live, pts, scenery)
        self._height_live = live
        return live

    def history_sync(self):
        """after writing tensor(T_HISTORY): the compact layer-0 operand is rebuilt from the ring (mqe_history_sync)"""
        self._call("history_sync", self._stream())

    def history(self):
        """(R, 2100) time-ordered locomotion history gathered from the ring (host-side bookkeeping of the slot)."""
        h = self.tensor(abi.T_HISTORY)
        pos = self._n_policy % abi.HIST
        idx = (torch.arange(abi.HIST, device=h.device) + pos) % abi.HIST
        return h[:, idx, :70].reshape(h.shape[0], -1)

    def debug_dynamics(self, env, robot):
        minv = np.zeros((18, 18), np.float32)
        nc = C.c_int(0)
        con = np.zeros((64, 8), np.float32)
        torch.cuda.synchronize()
        self._call("debug_dynamics", int(env), int(robot), C.c_void_p(minv.ctypes.data), C.byref(nc), C.c_void_p(con.ctypes.data))
        return minv, con[:nc.value]

    def profile_enable(self, on=True):
        """on: False/0 = off, True/1 = bracket every fused step with HIP events, k > 1 = one fused step per period of k (the THIRD of each
        period, so that a run's first steps -- allocator and clock warm-up -- are never the sample; a run shorter than three steps with k > 2
        records nothing: profile_read() then returns cnt == 0 and callers must handle that)."""
        self._call("profile_enable", int(on))

    def profile_read(self, n=16):
        buf = (C.c_float * n)()
        cnt = C.c_int(0)
        self._call("profile_read", buf, n, C.byref(cnt))
        return list(buf), cnt.value
