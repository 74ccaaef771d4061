"""Base task wrapper (reference mqe/envs/wrappers/empty_wrapper.py:4-18) + the device-resident reward log."""
import torch

from mqe.engine import abi
from mqe.engine.desc import REWARD_TERMS
from .spaces import Wrapper, Box  # noqa: F401


class RewardBuffer(dict):
    """`reward_buffer` of the reference wrappers: per-term reward sums + "step count".  The reference adds
    `torch.sum(term).cpu()` every step (a host sync per term, e.g. go1_sheep_wrapper.py:77,83,93,105,112); here the
    sums live on the device ([N, terms], accumulated in-kernel) and are reduced only when somebody reads a value
    (mqe_openrl_wrapper.batch_rewards, openrl_ws/utils.py:76-90).  Assigning 0 to a key clears its column."""

    def __init__(self, names, sums):
        super().__init__()
        self._col = {n: i for i, n in enumerate(names) if n is not None}
        self._sums = sums
        for n in names:
            if n is not None:
                dict.__setitem__(self, n, 0)
        dict.__setitem__(self, "step count", 0)

    def __getitem__(self, k):
        if k in self._col:
            return self._sums[:, self._col[k]].sum()
        return dict.__getitem__(self, k)

    def __setitem__(self, k, v):
        if k in self._col:
            self._sums[:, self._col[k]] = v
        else:
            dict.__setitem__(self, k, v)

    def items(self):
        return [(k, self[k]) for k in self.keys()]

    def values(self):
        return [self[k] for k in self.keys()]


class EmptyWrapper(Wrapper):
    def __init__(self, env):
        super().__init__(env)
        self.num_envs = env.num_envs
        self.num_agents = env.num_agents
        if hasattr(env.cfg.terrain, "BarrierTrack_kwargs"):
            self.BarrierTrack_kwargs = env.cfg.terrain.BarrierTrack_kwargs
        for key in dir(env.cfg.rewards.scales):
            if key[0] != "_" and "scale" in key:
                setattr(self, key, getattr(env.cfg.rewards.scales, key))
        self.obs_ids = torch.eye(self.num_agents, dtype=torch.float32, device=env.device).repeat(self.num_envs, 1).reshape(self.num_envs, self.num_agents, -1)


class FusedTaskWrapper(EmptyWrapper):
    """Shared by the four task wrappers: observation / reward come out of the engine's fused step."""
    task = "plain"
    obs_dim = 0
    wrapper_agents = None

    def __init__(self, env):
        super().__init__(env)
        if self.wrapper_agents is not None:
            self.num_agents = self.wrapper_agents
            self.obs_ids = torch.eye(self.num_agents, dtype=torch.float32, device=env.device).repeat(self.num_envs, 1).reshape(self.num_envs, self.num_agents, -1)
        assert env.task == self.task, f"{type(self).__name__} wraps task '{self.task}', env was built for '{env.task}'"
        dsc = env.engine.desc
        if dsc.num_command_dims != 3 or [dsc.command_src[c] for c in range(18)] != [-1] * 3 + [0, 1, 2] + [-1] * 12:
            # upstream's task wrappers multiply the (N, A, 3) action by a (1, 1, 3) scale (go1_*_wrapper.py step()): there is no room for the
            # action columns that command.cfg.{body_height, gait_freq, ...} add (go1.py:64-93); such a config runs behind EmptyWrapper / Go1.step
            raise NotImplementedError("command.cfg flags beyond the velocity command: the task wrappers carry exactly (x, y, yaw) per agent, "
                                      "as upstream; step the Go1 env itself (EmptyWrapper, e.g. go1plane)")
        self.observation_space = Box(low=-float("inf"), high=float("inf"), shape=(self._obs_dim(),), dtype=float)
        self.action_space = Box(low=-1, high=1, shape=(3,), dtype=float)
        self.action_scale = torch.tensor([[[2, 0.5, 0.5]]], device=env.device).repeat(self.num_envs, self.num_agents, 1)
        self._wobs = env.engine.tensor(abi.T_WRAPPER_OBS)
        self._wrew = env.engine.tensor(abi.T_WRAPPER_REWARD)
        self._wpack = env.engine.tensor(abi.T_WRAPPER_PACKED)        # obs | reward | done (N bytes) in one buffer
        assert self._wobs.shape[-1] == self.observation_space.shape[0]
        self.reward_buffer = RewardBuffer([n for _, n in REWARD_TERMS[self.task]], env.engine.tensor(abi.T_REWARD_SUMS))
        # a recurrent actor (set_actor(recurrent=True)): what the next rollout() starts its cells from -- "live" (the engine's own state), "zeros" or
        # a tensor -- and what get_state() can save of the state behind the last rollout: "zeros", a tensor, or None (not recorded: unknown)
        self._recurrent, self._hidden_next, self._hidden_saved = False, "live", "zeros"

    def _obs_dim(self):
        raise NotImplementedError

    def reset(self):
        self.env.reset()
        self._hidden_next = self._hidden_saved = "zeros"          # every episode starts anew
        self._hold_obs(self._wobs.clone())
        return self._last_obs

    def _hold_obs(self, obs):
        """the observation a following rollout() starts from, with the env's observation epoch: Go1.reset() and Go1.set_state() called
        below this wrapper advance the epoch, and the held observation is then not used"""
        self._last_obs, self._last_obs_epoch = obs, getattr(self.env, "_obs_epoch", 0)

    def get_state(self):
        """Go1.get_state() + the observation this wrapper last returned: the engine's blob does not hold it when the step wrote it into a
        tensor of the caller's (as step() does), and a rollout() after set_state() starts from it.  With a recurrent actor
        (set_actor(recurrent=True)) also "last_hidden": the cells' state behind the last rollout(record_hidden=True), which set_state() hands
        the next rollout(); after an unrecorded rollout it raises RuntimeError and says why"""
        state = dict(self.env.get_state())
        obs = getattr(self, "_last_obs", None)
        current = obs is not None and getattr(self, "_last_obs_epoch", None) == getattr(self.env, "_obs_epoch", 0)
        state["last_obs"] = obs.detach().cpu().clone() if current else None
        if self._recurrent:
            # the engine's live recurrent state has no export of its own: what the wrapper can save is next_hidden() of the last RECORDED rollout
            h = self._hidden_saved
            if h is None:
                raise RuntimeError("get_state: the actor is recurrent and the last rollout() did not record its state (record_hidden=False): the "
                                   "engine's live state cannot be read back; roll out with record_hidden=True before a checkpoint")
            state["last_hidden"] = h.detach().cpu().clone() if isinstance(h, torch.Tensor) and current else None      # None: zeros
        return state

    def set_state(self, state):
        self.env.set_state(state)
        obs = state.get("last_obs")
        self._hold_obs(obs.to(self._wobs.device).contiguous() if obs is not None else None)
        h = state.get("last_hidden")                 # the next rollout() starts from it (zeros when the state held none)
        self._hidden_next = self._hidden_saved = h.to(self._wobs.device).contiguous() if h is not None else "zeros"

    def step(self, action):
        # fresh tensors every step, like the reference: the HIP engine writes obs | reward | done of this step straight into a
        # new tensor (mqe_set_return_buffer; the engine's own MQE_T_WRAPPER_* buffer then keeps the previous contents); an
        # engine without that entry point is snapshotted with one copy
        eng = self.env.engine
        direct = hasattr(eng, "set_return_buffer")
        if direct:
            snap = torch.empty_like(self._wpack)
            eng.set_return_buffer(snap)
        try:
            self.env.step_fused(action.reshape(self.num_envs, self.num_agents, 3))
        finally:
            if direct:
                eng.set_return_buffer(None)
        dict.__setitem__(self.reward_buffer, "step count", dict.__getitem__(self.reward_buffer, "step count") + 1)
        if not direct:
            snap = self._wpack.clone()
        n, nr = self._wobs.numel(), self._wrew.numel()
        self.returned_batch = snap                                     # obs | reward | done (0/1): what a sharded runner all-gathers
        # all three returned tensors belong to this step alone (the reference builds a new reset_buf every step; env.reset_buf
        # is a live view of engine memory that the next step overwrites) and all three are VIEWS of the one buffer the step wrote:
        # the done flags are its byte tail, seen as torch.bool in place -- no torch kernel runs in a step
        done = snap[n + nr:].view(torch.uint8)[:self.num_envs].view(torch.bool)
        self._hold_obs(snap[:n].view(self._wobs.shape))                # what a following rollout() starts from
        return self._last_obs, snap[n:n + nr].view(self._wrew.shape), done, self.env.extras

    # ---- on-device rollouts (mqe_rollout): the actor runs inside the engine, T steps per call ---------------------------------------
    def _rollout_engine(self, what):
        eng = self.env.engine
        if not hasattr(eng, "rollout"):
            raise NotImplementedError(f"{what} runs inside the HIP engine (mqe.engine.hip_engine.HipEngine, mqe_rollout); "
                                      f"{type(eng).__name__} has no on-device actor")
        return eng

    def set_actor(self, actor_module, critic_module=None, log_std=None, action_gain=1.0, value_norm=False, layer_norm=False, recurrent=False):
        """The policy a following rollout() evaluates inside the engine: torch.nn.Sequential stacks of Linear / Tanh / ReLU -- actor
        (obs_dim -> ... -> 3, the mean), optional critic (obs_dim -> ... -> 1) with the same activation -- and log_std (3 values; a tensor
        or Parameter is read again by every sync_actor(); None: zeros).  Anything else raises ValueError naming the offending layer.
        Creates the engine's actor and copies the parameters (on the device when the modules live there).  value_norm (needs a critic):
        the engine keeps OpenRL's ValueNorm beside the parameters (HipEngine.create_actor) -- the critic predicts returns in units of
        their running mean and standard deviation; rollout(gamma=...) and ppo_update() follow it.  The statistics start at (mu, sigma) =
        (0, 0.1) with every set_actor; sync_actor() and pull_actor() never touch them.  layer_norm=True: the stacks may hold OpenRL's
        torch.nn.LayerNorm(n, eps=1e-5) layers -- one on the observation in front of the first Linear (the feature norm), one behind every
        hidden activation (the hidden norm), either, both or none, the same choice in actor and critic (mqe.utils.actor_net.mlp_spec names
        what it refuses); sync_actor() and pull_actor() copy their weights and biases too.  Without it a LayerNorm is refused like any
        other layer.  recurrent=True: both networks are mqe.utils.actor_net.RecurrentMLP (base -> GRU cell -> [LayerNorm] -> head; OpenRL's
        use_recurrent_policy), or the actor alone; a plain Sequential beside a RecurrentMLP is refused.  The engine carries the cells' state
        across rollout() calls and zeroes it wherever a step ended an episode; sync_actor() / pull_actor() copy the cells too.  ppo_update()
        trains such an actor with chunk_length=L: back-propagation through time over chunks of a trajectory of rollout(record_hidden=True),
        inside the engine; without the keyword it refuses it (a learner may still differentiate the torch twins -- RecurrentMLP.evaluate
        from traj.hidden -- and sync_actor() the result).  actor_module may instead be ONE mqe.utils.actor_net.MATNet, the Multi-Agent
        Transformer (OpenRL's --algo mat): the whole policy, with no critic_module (its encoder carries the value head) and no log_std (the
        module's own Parameter); value_norm= applies, layer_norm= / recurrent= do not.  rollout() evaluates it inside the engine; ppo_update(...,
        transformer=True) updates it inside the engine too, and without the keyword refuses it (a learner may still differentiate
        MATNet.evaluate(traj.obs, traj.actions) in torch and sync_actor() every tensor back)."""
        from mqe.utils.actor_net import MATNet, RecurrentMLP, actor_tensors, mat_spec, mlp_spec, recurrent_spec
        D = self.observation_space.shape[0]
        if isinstance(actor_module, MATNet):
            # the Multi-Agent Transformer (OpenRL's --algo mat): one module is the whole policy -- its encoder carries the value head, log_std is its
            # own Parameter.  rollout() / gae work as for any actor; ppo_update(transformer=True) runs the engine's own backward; without the keyword it
            # refuses, and a learner differentiates MATNet.evaluate(traj.obs, traj.actions) in torch and sync_actor() copies the result back
            # (HipEngine.create_actor(transformer=True))
            if critic_module is not None or log_std is not None or layer_norm or recurrent:
                raise ValueError("set_actor(MATNet): the transformer is the whole policy: no separate critic (its encoder carries the value head), no log_std "
                                 "(it is the module's own Parameter), no layer_norm= / recurrent= (it has its own norms and no state)")
            _, E = mat_spec(actor_module, D)
            self._rollout_engine("set_actor").create_actor([D, E, 3], [D, E, 1], activation="tanh", action_gain=action_gain, value_norm=value_norm, transformer=True)
            self._actor = (actor_tensors("mat", mat=actor_module), actor_module.log_std, True)
            self._recurrent, self._hidden_next, self._hidden_saved = False, "live", "zeros"
            self.sync_actor()
            return
        no_norms = {"feature": None, "hidden": []}

        def spec(module, what, out):           # (dims, activation, linears, norms) of a network, whichever of the three forms it comes in
            if recurrent:
                return recurrent_spec(module, what, D, out, layer_norm=layer_norm)[:4]
            found = mlp_spec(module, what, D, out, layer_norm=layer_norm)
            return found if layer_norm else (*found, no_norms)
        if not recurrent:
            for what, m in (("actor", actor_module), ("critic", critic_module)):
                if isinstance(m, RecurrentMLP):
                    raise ValueError(f"{what}: a RecurrentMLP without recurrent=True; the engine evaluates both networks recurrent (set_actor(..., recurrent=True)) or neither")
        a_dims, a_act, a_lin, a_norm = spec(actor_module, "actor", 3)
        c_dims, c_act, c_lin, c_norm = (None, None, [], no_norms)
        if critic_module is not None:
            c_dims, c_act, c_lin, c_norm = spec(critic_module, "critic", 1)
            if a_act is not None and c_act is not None and a_act != c_act:
                raise ValueError(f"critic: mixed activations; the actor uses {a_act}, the critic {c_act}: the engine applies one kind to both networks")
            if (a_norm["feature"] is None) != (c_norm["feature"] is None):
                raise ValueError("critic: the feature norm (a LayerNorm in front of the first Linear) is in one network and not in the other: "
                                 "the engine applies one choice to both")
            if len(a_dims) > 2 and len(c_dims) > 2 and bool(a_norm["hidden"]) != bool(c_norm["hidden"]):
                raise ValueError("critic: the hidden norm (a LayerNorm behind every hidden activation) is in one network and not in the other: "
                                 "the engine applies one choice to both")
        if log_std is not None and int(torch.as_tensor(log_std).numel()) != 3:
            raise ValueError(f"log_std must hold 3 values (one per action column), got {tuple(torch.as_tensor(log_std).shape)}")
        if value_norm and critic_module is None:
            raise ValueError("set_actor(value_norm=True): value normalisation is that of a critic's targets, and no critic was given")
        eng = self._rollout_engine("set_actor")
        norm_kw = {}
        if layer_norm:                     # an engine without the keywords is never asked for them
            norm_kw = dict(layer_norm=bool(a_norm["hidden"] or c_norm["hidden"]), feature_norm=a_norm["feature"] is not None)
        if recurrent:
            norm_kw["recurrent"] = True
        eng.create_actor(a_dims, c_dims, activation=a_act or c_act or "tanh", action_gain=action_gain, value_norm=value_norm, **norm_kw)
        a_rnn, c_rnn = (actor_module, critic_module) if recurrent else (None, None)
        # every tensor the modules share with the engine under the engine's name, the actor's then the critic's; log_std; whether there is a critic
        self._actor = (actor_tensors("actor", a_lin, a_norm, a_rnn) + actor_tensors("critic", c_lin, c_norm, c_rnn), log_std, critic_module is not None)
        self._recurrent, self._hidden_next, self._hidden_saved = bool(recurrent), "live", "zeros"       # create_actor zeroed the engine's state
        self.sync_actor()

    def sync_actor(self):
        """copies the modules' current parameters into the engine's buffer again (after an optimiser step); device to device when the
        modules live on the engine's device, no synchronisation"""
        if getattr(self, "_actor", None) is None:
            raise RuntimeError("sync_actor: no actor (set_actor first)")
        tensors, log_std, _ = self._actor
        views = self._rollout_engine("sync_actor").actor_params()
        with torch.no_grad():
            for name, t in tensors:
                views[name].copy_(t.detach(), non_blocking=True)
            if log_std is None:
                views["log_std"].zero_()
            else:
                views["log_std"].copy_(torch.as_tensor(log_std).detach().reshape(3).to(torch.float32), non_blocking=True)

    def pull_actor(self):
        """the reverse of sync_actor(): the engine's parameter buffer -> the torch modules and log_std given to set_actor, device to device
        when they live on the engine's device, no synchronisation.  After ppo_update() the ENGINE holds the master copy of the parameters:
        pull_actor() brings the modules up to date, and a sync_actor() before it would overwrite the update with the modules' old values"""
        eng = self._rollout_engine("pull_actor")
        if getattr(self, "_actor", None) is None:
            raise RuntimeError("pull_actor: no actor (set_actor first)")
        tensors, log_std, _ = self._actor
        views = eng.actor_params()
        with torch.no_grad():
            for name, t in tensors:
                t.copy_(views[name], non_blocking=True)
            if isinstance(log_std, torch.Tensor):
                log_std.copy_(views["log_std"].reshape(log_std.shape), non_blocking=True)

    def ppo_update(self, traj, **kw):
        """The PPO update of a trajectory of rollout(gamma=...) inside the engine (HipEngine.ppo_update: epochs, minibatches, lr, clip,
        value_coef, entropy_coef, value_clip, betas, eps, max_grad_norm, generator): per minibatch the clipped-surrogate gradient and one Adam
        step on the engine's own parameter buffer, no copy and no synchronisation; -> the (epochs, minibatches, 6) statistics tensor.
        Afterwards the engine holds the master copy: the following rollout() uses it as it is, pull_actor() copies it into the torch
        modules, and sync_actor() would overwrite it with the modules' values.  After set_actor(value_norm=True) every minibatch first folds
        its returns (reward units) into the running statistics and the value loss compares the critic with the returns normalised by the new
        (mu, sigma): statistics entry 1 (mean L_v) is in normalised units.  After set_actor(recurrent=True): chunk_length=L is required --
        the trajectory (rollout(record_hidden=True), T a multiple of L) is cut into chunks of L steps per row, the minibatches are sets of chunks
        and the gradient runs through the GRU cells over each chunk's steps (OpenRL's data_chunk_length; HipEngine.ppo_grad states the rule).
        joint=True is OpenRL's use_joint_action_loss (jrpo.yaml): one ratio and one advantage per env-step, the minibatches are sets of env-steps;
        dual_clip=c_d is dual_clip_ppo with dual_clip_coeff = c_d (dppo.yaml).  After set_actor(MATNet): transformer=True is required -- the update
        runs through the engine's own backward of the transformer (HipEngine.ppo_grad states it), the minibatches are sets of env-steps, and
        pull_actor() brings the result back into the module; without the keyword the call is refused as before and the learner stays in torch."""
        eng = self._rollout_engine("ppo_update")
        if getattr(self, "_actor", None) is None:
            raise RuntimeError("ppo_update: no actor (set_actor first)")
        if not self._actor[2]:
            raise ValueError("ppo_update: the loss has a value term, and the actor was set without a critic (set_actor(actor, critic))")
        return eng.ppo_update(traj, **kw)

    def rollout(self, T, deterministic=False, gamma=None, lam=0.95, normalize_advantages=False, record_hidden=False):
        """T steps with the engine's own actor (set_actor) in one call: a Rollout (mqe.engine.hip_engine) whose tensors -- obs (T+1, N, A', D),
        reward (T, N, A'), done (T, N) bool, actions (T, N, A', 3) unclipped, logp (T, N, A'), value (T+1, N, A') or None -- are fresh memory
        that belongs to the caller.  Starts from the observation the last step() / reset() / rollout() returned (set_state() of this
        wrapper restores it; after a Go1-level reset() or set_state() below the wrapper: from the engine's own observation buffer).
        With a gamma (the actor needs a critic: ValueError otherwise, before anything is enqueued) the rollout also records the time-out
        flags of every step and the engine computes GAE(lam) on the device (HipEngine.gae): time_outs (T, N) bool, advantages and returns
        (T, N, A'), adv_stats (mean, std; with normalize_advantages, which normalises over this env's own rows) are filled; with
        gamma=None they are None and the call enqueues nothing more than it always did.  After set_actor(value_norm=True) traj.value is in
        NORMALISED units (what the critic predicts); the engine de-normalises it with the current (mu, sigma) for the recursion, and
        traj.returns / traj.advantages are in reward units.  After set_actor(recurrent=True) the cells continue from the engine's live state
        (zeros after a reset or set_state() of the env below this wrapper; after this wrapper's set_state(): the state it restored);
        record_hidden=True: traj.hidden (T + 1, N, A', Hs) holds the state every step started from, for back-propagation through time on the
        torch twins, and get_state() can checkpoint the state behind the trajectory."""
        env = self.env
        eng = self._rollout_engine("rollout")
        if type(self).step is not FusedTaskWrapper.step:
            raise NotImplementedError(f"{type(self).__name__}.step transforms the actions in Python before the engine sees them; the engine's actor "
                                      "feeds the step directly: roll this task out with step()")
        if getattr(env, "record_now", False):
            raise NotImplementedError("rollout while recording is live: a frame is due after every step, and the T steps of a rollout are enqueued "
                                      "as one; pause_recording() first, or step()")
        if getattr(env, "between_policy_and_physics", None) is not None or getattr(env, "before_policy_tail", None) is not None:
            raise NotImplementedError("rollout with the sharded runner's hooks set (between_policy_and_physics / before_policy_tail): its "
                                      "all-gather sits inside every step; each shard rolls out its own envs without them")
        if env.has_overrides:
            raise NotImplementedError("rollout runs entirely inside the engine: a Go1 subclass that overrides any of "
                                      + " / ".join(env._PLUGIN_POINTS) + " is stepped through Go1.step()")
        if getattr(self, "_actor", None) is None:
            raise RuntimeError("rollout: no actor (set_actor first)")
        if gamma is not None and not self._actor[2]:
            raise ValueError("rollout(gamma=...): advantages need values, and the actor was set without a critic (set_actor(actor, critic))")
        obs0 = getattr(self, "_last_obs", None)
        if getattr(self, "_last_obs_epoch", None) != getattr(env, "_obs_epoch", 0):
            obs0 = None       # the env was reset or restored below this wrapper: the engine's own buffer is what there is
        rec_kw = {}
        if self._recurrent:
            src = self._hidden_next if obs0 is not None else "zeros"       # reset or restored below this wrapper: zeros
            if isinstance(src, str):
                src = None if src == "live" else torch.zeros(self.num_envs, self.num_agents, eng.hidden_width(), dtype=torch.float32, device=self._wobs.device)
            rec_kw = dict(hidden=src, record_hidden=record_hidden)
        elif record_hidden:
            raise ValueError("rollout(record_hidden=True): the actor is not recurrent (set_actor(..., recurrent=True))")
        traj = eng.rollout(T, obs0=obs0.contiguous() if obs0 is not None else None, deterministic=deterministic, time_outs=gamma is not None, **rec_kw)
        if rec_kw:
            self._hidden_next, self._hidden_saved = "live", (traj.next_hidden() if record_hidden else None)
        if gamma is not None:
            eng.gae(traj, gamma, lam=lam, normalize=normalize_advantages)
        T = traj.T
        dict.__setitem__(self.reward_buffer, "step count", dict.__getitem__(self.reward_buffer, "step count") + T)
        env._steps_policy = getattr(env, "_steps_policy", 0) + T
        env.common_step_counter += T
        env._refresh_extras()
        self.returned_batch = traj.packed[T, :self._wpack.numel()].clone()      # step()'s layout and length; a copy: a view would keep all T + 1 rows alive after the caller drops the trajectory
        self._hold_obs(self.returned_batch[:self._wobs.numel()].view(self._wobs.shape))
        return traj
