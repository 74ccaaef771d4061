"""ctypes mirror of include/mqe_hip.h: constants, structs and SIGNATURES, the signature of every function the header declares
(tests/test_abi.py holds the struct sizes against the built library and SIGNATURES against the header's prototypes)."""
import ctypes as C

ABI_VERSION = 17
MAX_SPHERES, NBODY, NREP, NDOF = 64, 13, 17, 12
MAX_SELF_PAIRS = 384
MAX_PRIMS = 20
PRIM_SPHERE, PRIM_CAPSULE, PRIM_BOX = 0, 1, 2
MAX_AGENTS, MAX_NPCS, FRAME, HIST, MAX_LAYERS, MAX_REWARD_TERMS = 4, 16, 72, 30, 6, 12
OBS_BAG = 74
MAX_HEIGHT_POINTS, HSCAN_SCENERY = 1024, 1      # mqe_measure_heights: grid points per robot, the scenery flag

# mqe_render_view (include/mqe_hip.h): the id word's classes and bit fields, and the constants of the colour formula
VIEW_MAX_PIXELS = 1 << 20
VIEW_NONE, VIEW_GROUND, VIEW_WALL, VIEW_ROBOT, VIEW_NPC, VIEW_LINK_SCENE, VIEW_SCENERY = range(7)
VIEW_CHECKER_BIT = 1 << 24
VIEW_AMBIENT, VIEW_DIFFUSE, VIEW_CHECKER = 0.35, 0.65, 0.08
VIEW_LIGHT = (0.36, 0.48, 0.80)
VIEW_SKY = (135, 190, 235)
VIEW_PALETTE = ((0.55, 0.58, 0.50), (0.72, 0.68, 0.60), (0.85, 0.25, 0.20), (0.20, 0.40, 0.85), (0.95, 0.75, 0.15),      # ground, wall, robots 0-3,
                (0.25, 0.70, 0.35), (0.92, 0.90, 0.82), (0.60, 0.42, 0.25), (0.50, 0.50, 0.58))                          # free NPC, 1-dof scene, scenery box


def view_palette_row(cls, index):
    """row of VIEW_PALETTE that holds the albedo of class `cls` (robot `index`: one of four)"""
    return {VIEW_GROUND: 0, VIEW_WALL: 1, VIEW_ROBOT: 2 + index % 4}.get(cls, cls + 2)


TASK = dict(plain=0, gate=1, sheep=2, seesaw=3, football_defender=4, pushbox=5, rotation=6, bridge=7, wrestling=8, tug=9)
NPC = dict(none=0, ball=1, sheep=2, seesaw=3, box=4, rotation=3, bridge=5, wrestling=5, circular=3)     # the revolving door shares the seesaw's fixed-base + 1-dof-link structure
CTRL = dict(C=0, P=1, V=2, T=3)
TERM = dict(roll=1, pitch=2, z_low=4, z_high=8)
POST_FRAME, POST_NPC, POST_RESET, POST_OBS, POST_WRAPPER, POST_ALL, POST_WRAPPER_LEVEL = 1, 2, 4, 8, 16, 31, 32      # mqe_post_physics_stage

(T_ROOT_STATE, T_DOF_STATE, T_CONTACT_FORCE, T_TORQUES, T_ACTIONS, T_LAST_ACTIONS, T_LOCOMOTION_OBS, T_HISTORY,
 T_LAST_LOCO_ACTION, T_LAST_TWO_LOCO_ACTION, T_ACT_HIST, T_GAIT_INDICES, T_CLOCK_INPUTS, T_BASE_LIN_VEL,
 T_BASE_ANG_VEL, T_PROJECTED_GRAVITY, T_BASE_QUAT, T_EPISODE_LENGTH, T_RESET_BUF, T_COLLIDE_BUF, T_TIME_OUT_BUF,
 T_R_TERM, T_P_TERM, T_Z_HIGH_TERM, T_OBS_BAG, T_WRAPPER_OBS, T_WRAPPER_REWARD, T_REWARD_SUMS, T_SHEEP_POS_AVG,
 T_SHEEP_POS_VAR, T_RESET_COUNT, T_SUBSTEP_TORQUES, T_NPC_NOISE, T_WRAPPER_PACKED, T_DOMAIN_PARAMS, T_SUBSTEP_DOF_VEL,
 T_SUBSTEP_EXCEED_DOF_POS_LIMITS, T_CONTACT_OVERFLOW, T_ENV_ORIGINS, T_TERRAIN_LEVELS, T_CONTACT_REDUCED, T_RIGID_BODY_STATE,
 T_COUNT) = range(43)

# slices of one OBS_BAG row (compute_observations, reference go1.py:153-196)
BAG = dict(base_pos=(0, 3), base_rpy=(3, 6), dof_pos=(6, 18), dof_vel=(18, 30), lin_vel=(30, 33), ang_vel=(33, 36),
           last_action=(36, 48), last_last_action=(48, 60), projected_gravity=(60, 63), clock_inputs=(63, 67),
           base_quat=(67, 71))

f32, i32 = C.c_float, C.c_int32
FP = C.POINTER(C.c_float)


class Mlp(C.Structure):
    _fields_ = [("n_layers", i32), ("dims", i32 * (MAX_LAYERS + 1)), ("W", FP * MAX_LAYERS), ("b", FP * MAX_LAYERS)]


class RobotModel(C.Structure):
    _fields_ = [
        ("mass", f32 * NBODY), ("com", (f32 * 3) * NBODY), ("inertia", (f32 * 6) * NBODY),
        ("joint_offset", (f32 * 3) * NBODY), ("joint_axis", (f32 * 3) * NBODY),
        ("dof_lower", f32 * NDOF), ("dof_upper", f32 * NDOF), ("dof_vel_limit", f32 * NDOF),
        ("n_spheres", i32), ("sphere_body", i32 * MAX_SPHERES), ("sphere_reported", i32 * MAX_SPHERES), ("sphere_prim", i32 * MAX_SPHERES),
        ("sphere_center", (f32 * 3) * MAX_SPHERES), ("sphere_radius", f32 * MAX_SPHERES),
        ("n_prims", i32), ("prim_type", i32 * MAX_PRIMS), ("prim_body", i32 * MAX_PRIMS), ("prim_reported", i32 * MAX_PRIMS),
        ("prim_center", (f32 * 3) * MAX_PRIMS), ("prim_axis", (f32 * 3) * MAX_PRIMS), ("prim_half", (f32 * 3) * MAX_PRIMS),
        ("prim_bound", f32 * MAX_PRIMS), ("feature_reach", f32),
        ("n_self_pairs", i32), ("self_pair", C.c_uint16 * MAX_SELF_PAIRS),
        ("self_safe_lo", f32 * NDOF), ("self_safe_hi", f32 * NDOF),
    ]


class SimDesc(C.Structure):
    _fields_ = [
        ("abi_version", i32),
        ("num_envs", i32), ("num_agents", i32), ("num_npcs", i32), ("npc_kind", i32), ("task", i32),
        ("env_id_offset", i32), ("seed", i32),
        ("dt", f32), ("decimation", i32), ("gravity_z", f32), ("solver_iterations", i32),
        ("contact_offset", f32), ("max_depenetration_velocity", f32), ("friction", f32), ("erp", f32), ("solver_type", i32), ("velocity_iterations", i32),
        ("robot", RobotModel),
        ("npc_mass", f32), ("npc_inertia", f32), ("npc_n_spheres", i32),
        ("npc_sphere_center", (f32 * 3) * 8), ("npc_sphere_radius", f32 * 8), ("npc_box_half", f32 * 3), ("npc_contact_cap", i32),
        ("seesaw_joint_offset", f32 * 3), ("seesaw_plank_center", f32 * 3), ("seesaw_plank_half", f32 * 3),
        ("seesaw_base_half", f32 * 3),
        ("seesaw_plank_mass", f32), ("seesaw_plank_inertia_yy", f32), ("seesaw_vel_limit", f32), ("seesaw_default_angle", f32),
        ("seesaw_column_radius", f32), ("seesaw_column_length", f32), ("seesaw_theta_lo", f32), ("seesaw_theta_hi", f32),
        ("n_static_boxes", i32), ("npc_reported_bodies", i32), ("self_collision", i32), ("static_box_center", (f32 * 3) * 4), ("static_box_half", (f32 * 3) * 4),
        ("seesaw_axis", i32), ("seesaw_link_cylinder", i32),
        ("control_type", i32), ("action_scale", f32), ("hip_scale_reduction", f32), ("clip_actions", f32),
        ("torque_limits", f32 * NDOF), ("kp", f32), ("kd", f32), ("default_dof_pos", f32 * NDOF),
        ("command_obs", f32 * 70), ("cmd_lin_scale", f32), ("cmd_ang_scale", f32), ("clip_command", i32),
        ("num_command_dims", i32), ("command_src", i32 * 18), ("command_scale", f32 * 18),
        ("wall_sdf", FP), ("sdf_nx", i32), ("sdf_ny", i32),
        ("horizontal_scale", f32), ("wall_height", f32), ("ground_z", f32), ("ground_height", FP), ("wall_top", FP), ("edge_contacts", i32), ("wall_corner", FP), ("soft_dof_pos_limit", f32),
        ("env_origins", FP), ("agent_origins", FP), ("base_init_state", FP), ("npc_init_state", FP), ("gate_pos", FP),
        ("terrain_curriculum", i32), ("terrain_num_rows", i32), ("terrain_num_cols", i32), ("terrain_env_length", f32),
        ("terrain_origins", FP), ("terrain_levels", C.POINTER(i32)), ("terrain_types", C.POINTER(i32)),
        ("termination_flags", i32), ("terminate_on_base_contact", i32), ("max_episode_length", i32),
        ("roll_threshold", f32), ("pitch_threshold", f32), ("z_low_threshold", f32), ("z_high_threshold", f32),
        ("noise_mode", i32), ("dof_ratio_lo", f32), ("dof_ratio_hi", f32),
        ("has_base_pos_range", i32), ("has_npc_pos_range", i32),
        ("base_pos_x_lo", f32), ("base_pos_x_hi", f32), ("base_pos_y_lo", f32), ("base_pos_y_hi", f32),
        ("npc_pos_x_lo", f32), ("npc_pos_x_hi", f32), ("npc_pos_y_lo", f32), ("npc_pos_y_hi", f32),
        ("base_vel_lo", f32), ("base_vel_hi", f32),
        ("rand_friction", i32), ("friction_lo", f32), ("friction_hi", f32),
        ("rand_base_mass", i32), ("added_mass_lo", f32), ("added_mass_hi", f32),
        ("rand_com", i32), ("com_lo", f32 * 3), ("com_hi", f32 * 3),
        ("lag_timesteps", i32), ("push_interval", i32), ("max_push_vel_xy", f32),
        ("sheep_movement_scale", f32), ("sheep_movement_randomness", f32),
        ("reward_scale", f32 * MAX_REWARD_TERMS), ("wrapper_param", f32 * 8),
        ("actuator", Mlp), ("adaptation", Mlp), ("body", Mlp),
    ]


# on-device rollouts (include/mqe_hip.h: mqe_actor_create, mqe_actor_params, mqe_rollout)
ACTOR_MAX_LAYERS, ACTOR_MAX_HIDDEN, ACTOR_MAX_OBS = 4, 256, 128
ACTOR_TANH, ACTOR_RELU = 0, 1
ROLLOUT_MAX_STEPS, ROLLOUT_DETERMINISTIC = 4096, 1
GAE_NORMALIZE = 1            # mqe_gae flags bit 0
PPO_CLIP_VALUE, PPO_STATS = 1, 6      # mqe_ppo_grad: flags bit 0; floats of stats_dev (mean L_pi, mean L_v, H, L, approximate KL, clip share)
# value normalisation (include/mqe_hip.h states the values, csrc/kernels_vn.hpp defines them): a bit of mqe_actor_shape.activation above the kind
# byte; the state floats (m, q, d, mu, sigma) behind log_std; mqe_gae flags bit 3; mqe_ppo_grad flags bits 3 and 4 (the update needs bit 3)
ACTOR_VALUE_NORM, VALUE_NORM_STATE = 256, 5
GAE_VALUE_NORM = 8
PPO_VALUE_NORM, PPO_VALUE_NORM_UPDATE = 8, 16
# layer normalisation (include/mqe_hip.h states the values, csrc/kernels_ln.hpp defines them): two bits of the kind byte of
# mqe_actor_shape.activation, or-ed with ACTOR_TANH / ACTOR_RELU -- a LayerNorm behind every hidden activation / on the observation
ACTOR_LAYER_NORM, ACTOR_FEATURE_NORM = 2, 4
# the recurrent actor-critic (include/mqe_hip.h states the values, csrc/kernels_gru.hpp defines them): a bit of the kind byte of
# mqe_actor_shape.activation -- a GRU cell in front of the output layer of both networks -- and mqe_rollout flags bits 1 and 2: the start state is
# read from the tail of packed row 0 / the tails of rows 0 .. T are written
ACTOR_RECURRENT = 16
ROLLOUT_HIDDEN_IN, ROLLOUT_HIDDEN_RECORD = 2, 4
ACT_LD, LN_PART, GRU_LDS_LIMIT = 65, 32, 160 * 1024      # csrc/kernels_actor.hpp, kernels_ln.hpp, kernels_gru.hpp: what the LDS rule below is made of
# the recurrent gradient (include/mqe_hip.h states the values, csrc/kernels_bptt.hpp defines them): mqe_ppo_grad flags bit 5 -- back-propagation through
# time over chunks; index / first / count are chunks --, the shift of the chunk length L in flags (bits 8 .. 15) and the largest L
PPO_BPTT, PPO_CHUNK_SHIFT, PPO_MAX_CHUNK = 32, 8, 64
# the joint-ratio and dual-clip losses (include/mqe_hip.h states the values, csrc/kernels_ppo.hpp defines them): mqe_ppo_grad flags bits 6 and 7 -- index /
# first / count number the groups of A' samples of one env-step; `loss` points at a PpoLossEx
PPO_JOINT, PPO_DUAL_CLIP = 64, 128
LN_STAT, BPTT_CELL_ROWS, BPTT_LDS_LIMIT = 8, 7, 160 * 1024      # csrc/kernels_ln.hpp, kernels_bptt.hpp: what the LDS rule of the recurrent gradient is made of
# the Multi-Agent Transformer policy (include/mqe_hip.h states the value, csrc/kernels_mat.hpp defines it): a bit of the kind byte of
# mqe_actor_shape.activation -- actor_dims = (D, E, 3) and critic_dims = (D, E, 1) then describe MAT's encoder and decoder --, and what its LDS rule is made of
ACTOR_TRANSFORMER = 32
MAT_SLABS, MAT_FIXED_ROWS, MAT_LDS_LIMIT = 6, 3 + 4 + 4 + LN_PART, 160 * 1024
# the transformer's on-device gradient (include/mqe_hip.h states the value, csrc/kernels_mat_grad.hpp defines it): mqe_ppo_grad flags bit 16, the first above
# the chunk-length byte -- index / first / count number the env-step groups --, and what the two rules below are made of
PPO_TRANSFORMER = 65536
PPO_MAX_WG, MATG_FIXED_ROWS, MATG_HEAD_BYTES, MATG_LDS_LIMIT = 256, 2 + 3 + 4 + LN_PART, 64 * 8 + 16, 160 * 1024
RNG_ACTOR = 0x70000000          # csrc/mqe_common.hpp MQE_RNG_ACTOR: `count` of the actor's draws = RNG_ACTOR + post-physics steps so far


class ActorShape(C.Structure):
    _fields_ = [("obs_dim", i32), ("act_dim", i32), ("actor_layers", i32), ("actor_dims", i32 * (ACTOR_MAX_LAYERS + 1)),
                ("critic_layers", i32), ("critic_dims", i32 * (ACTOR_MAX_LAYERS + 1)), ("activation", i32), ("action_gain", f32)]


class PpoLoss(C.Structure):
    """mqe_ppo_loss"""
    _fields_ = [("clip_ratio", f32), ("value_coef", f32), ("entropy_coef", f32), ("value_clip", f32)]


class PpoLossEx(C.Structure):
    """mqe_ppo_loss_ex: what mqe_ppo_grad's `loss` points at under PPO_DUAL_CLIP (passed through ctypes.cast to POINTER(PpoLoss): the prototype stays)"""
    _fields_ = PpoLoss._fields_ + [("dual_clip", f32), ("reserved", f32 * 3)]


def actor_gru_lds_bytes(actor_dims, critic_dims=None, layer_norm=False, feature_norm=False):
    """LDS of k_actor_gru / k_actor_gru_ln for a recurrent shape (csrc/kernels_gru.hpp actor_gru_lds_bytes): two buffers of the widest layer input,
    the 4 output rows, the norms' 32 partial rows, the state of both cells, in rows of 65 floats.  mqe_actor_create refuses above GRU_LDS_LIMIT."""
    nets = [list(actor_dims)] + ([list(critic_dims)] if critic_dims else [])
    ldh = max(int(d) for dims in nets for d in dims[:-1])
    hs = sum(int(dims[-2]) for dims in nets)
    return (2 * ldh + 4 + (LN_PART if layer_norm or feature_norm else 0) + hs) * ACT_LD * 4


def bptt_lds_rows(actor_dims, critic_dims, layer_norm=False, feature_norm=False):
    """LDS rows of k_bptt_grad / k_bptt_ln_grad for a recurrent shape (csrc/kernels_bptt.hpp, THE RULE): the observation, every hidden output of the
    larger network and 4 output rows (ppo_lds_rows); with a norm the widest normalised vector, LN_STAT statistics and LN_PART partial rows
    (ln_lds_rows) and 2 rows for the norm behind the cell; BPTT_CELL_ROWS rows per unit of the wider cell."""
    nets = [[int(d) for d in actor_dims], [int(d) for d in critic_dims]]
    D = nets[0][0]
    rows = D + max(sum(dims[1:-1]) for dims in nets) + 4
    if layer_norm or feature_norm:
        uw = max([D if feature_norm else 0] + ([w for dims in nets for w in dims[1:-1]] if layer_norm else []))
        rows += uw + LN_STAT + LN_PART + 2
    return rows + BPTT_CELL_ROWS * max(dims[-2] for dims in nets)


def bptt_lds_bytes(rows, rt):
    """csrc/kernels_bptt.hpp bptt_lds_bytes: rows of rt + 1 floats, the sample numbers of the step and of the chunks, the done bytes of two steps, the running statistics"""
    return (rows * (rt + 1) + 2 + 20 * 64) * 4


def bptt_row_tile(actor_dims, critic_dims, layer_norm=False, feature_norm=False):
    """the chunks a workgroup of the recurrent gradient kernel walks at a time: 64 where the LDS rule fits BPTT_LDS_LIMIT, else 32; None where the
    shape does not fit at 32 either (the first ppo_grad(chunk_length=...) refuses it, naming the cell's width)"""
    rows = bptt_lds_rows(actor_dims, critic_dims, layer_norm, feature_norm)
    return next((rt for rt in (64, 32) if bptt_lds_bytes(rows, rt) <= BPTT_LDS_LIMIT), None)


def actor_mat_lds_bytes(obs_dim, n_embd):
    """LDS of k_actor_mat (csrc/kernels_mat.hpp actor_mat_lds_bytes): the observation's D rows, MAT_SLABS slabs of E rows, the rows of s, the
    outputs, the kept results and the norm's partials, in rows of 65 floats.  mqe_actor_create refuses above MAT_LDS_LIMIT."""
    return (int(obs_dim) + MAT_SLABS * int(n_embd) + MAT_FIXED_ROWS) * ACT_LD * 4


def mat_grad_lds_bytes(obs_dim, n_embd):
    """LDS of k_mat_grad (csrc/kernels_mat_grad.hpp mat_grad_lds_bytes, LDS RULE): max(D, E) + 2 rows of popped inputs, max(6 E, E + D) rows of slabs and
    their gradients, E rows of a dx to be added, the fixed rows, in rows of 65 floats, behind the tile's sample numbers.  The first
    ppo_grad(transformer=True) refuses above MATG_LDS_LIMIT (-5, naming E)."""
    D, E = int(obs_dim), int(n_embd)
    return (max(D, E) + 2 + max(MAT_SLABS * E, E + D) + E + MATG_FIXED_ROWS) * ACT_LD * 4 + MATG_HEAD_BYTES


def mat_grad_scratch_bytes(obs_dim, n_embd):
    """the workgroups' tapes (csrc/kernels_mat_grad.hpp mat_grad_scratch_bytes, THE TAPE): PPO_MAX_WG x (2 D + 40 E + 20) rows of 64 floats, allocated by
    the first ppo_grad(transformer=True) of an actor and released with it"""
    return PPO_MAX_WG * (2 * int(obs_dim) + 40 * int(n_embd) + 20) * 64 * 4


def mat_param_blocks(obs_dim, n_embd):
    """[(name, shape)] of the transformer's tensors in the engine's order -- mqe.utils.actor_net.MATNet's parameters() without log_std: the
    encoder and the decoder in the order their operators run, then the two narrow output layers (csrc/kernels_mat.hpp, PARAMETERS)"""
    D, E = int(obs_dim), int(n_embd)
    ln = lambda name, n: [(f"mat.{name}.weight", (n,)), (f"mat.{name}.bias", (n,))]
    lin = lambda name, k, n: [(f"mat.{name}.weight", (n, k)), (f"mat.{name}.bias", (n,))]
    attn = lambda name: [b for part in ("key", "query", "value", "proj") for b in lin(f"{name}.{part}", E, E)]
    return (ln("enc.obs_norm", D) + lin("enc.obs_fc", D, E) + ln("enc.ln", E) + attn("enc.attn") + ln("enc.ln1", E) + lin("enc.mlp0", E, E) +
            lin("enc.mlp1", E, E) + ln("enc.ln2", E) + lin("enc.head0", E, E) + ln("enc.head_ln", E) +
            lin("dec.act_fc", 3, E) + ln("dec.ln", E) + attn("dec.attn1") + ln("dec.ln1", E) + attn("dec.attn2") + ln("dec.ln2", E) +
            lin("dec.mlp0", E, E) + lin("dec.mlp1", E, E) + ln("dec.ln3", E) + lin("dec.head0", E, E) + ln("dec.head_ln", E) +
            lin("value_out", E, 1) + lin("mean_out", E, 3))


def actor_param_layout(actor_dims, critic_dims=None, value_norm=False, layer_norm=False, feature_norm=False, recurrent=False, transformer=False):
    """The flat parameter buffer of mqe_actor_params as an ordered {name: (offset, shape)}: per layer W (out, in) row-major as
    torch.nn.Linear.weight, then b; the actor's layers, then the critic's, then log_std[3].  Names: actor.<layer>.weight / .bias,
    critic.<layer>.weight / .bias, log_std.  value_norm (an actor created with ACTOR_VALUE_NORM): + "value_norm", the VALUE_NORM_STATE
    floats (m, q, d, mu, sigma) behind log_std -- state of the normaliser, not a trainable parameter.  feature_norm (ACTOR_FEATURE_NORM):
    <who>.norm_in.weight / .bias (D each) in front of a network's layer 0; layer_norm (ACTOR_LAYER_NORM): <who>.<layer>.norm.weight / .bias
    (n each) behind the bias of every hidden layer.  With both off the layout is the plain one.  recurrent (ACTOR_RECURRENT; every network needs
    a hidden layer, H = the last one's width): <who>.gru.weight_ih / .weight_hh (3H, H), .bias_ih / .bias_hh (3H) and, with layer_norm,
    <who>.gru.norm.weight / .bias (H) in front of the output layer's weight -- torch.nn.GRU's own tensors and order.
    transformer (ACTOR_TRANSFORMER; actor_dims = (D, E, 3), critic_dims = (D, E, 1) or None for the same): mat_param_blocks' names, mat.enc.*, mat.dec.*,
    mat.value_out.*, mat.mean_out.*, in MATNet's parameters() order; log_std and value_norm behind them as always.  The trainable count is
    2 D + D E + 18 E^2 + 45 E + 7:  the encoder 2 D + D E + 7 E^2 + 16 E, the decoder 11 E^2 + 25 E, value_out E + 1, mean_out 3 E + 3, log_std 3."""
    out, off = {}, 0
    if transformer:
        dims = [int(d) for d in actor_dims]
        if len(dims) != 3 or dims[2] != 3 or (critic_dims and [int(d) for d in critic_dims] != [dims[0], dims[1], 1]):
            raise ValueError("transformer: actor_dims = (D, E, 3) and critic_dims = (D, E, 1) with the same E (the encoder carries the value head)")
        if layer_norm or feature_norm or recurrent:
            raise ValueError("transformer: the transformer has its own norms and no state (no layer_norm, feature_norm or recurrent)")
        for name, shape in mat_param_blocks(dims[0], dims[1]):
            out[name] = (off, shape)
            off += shape[0] * (shape[1] if len(shape) > 1 else 1)
        actor_dims, critic_dims = (), ()
    for who, dims in (("actor", actor_dims), ("critic", critic_dims or ())):
        if feature_norm and len(dims) > 1:
            d = int(dims[0])
            out[f"{who}.norm_in.weight"] = (off, (d,))
            out[f"{who}.norm_in.bias"] = (off + d, (d,))
            off += 2 * d
        for l in range(len(dims) - 1):
            k, n = int(dims[l]), int(dims[l + 1])
            if recurrent and l + 2 == len(dims):
                if l == 0:
                    raise ValueError(f"{who}: a recurrent network needs at least 2 Linear layers (the GRU cell sits behind the last hidden layer)")
                for name, shape in (("weight_ih", (3 * k, k)), ("weight_hh", (3 * k, k)), ("bias_ih", (3 * k,)), ("bias_hh", (3 * k,)),
                                    *((("norm.weight", (k,)), ("norm.bias", (k,))) if layer_norm else ())):
                    out[f"{who}.gru.{name}"] = (off, shape)
                    off += shape[0] * (shape[1] if len(shape) > 1 else 1)
            out[f"{who}.{l}.weight"] = (off, (n, k))
            out[f"{who}.{l}.bias"] = (off + n * k, (n,))
            off += n * k + n
            if layer_norm and l + 2 < len(dims):
                out[f"{who}.{l}.norm.weight"] = (off, (n,))
                out[f"{who}.{l}.norm.bias"] = (off + n, (n,))
                off += 2 * n
    out["log_std"] = (off, (3,))
    if value_norm:
        out["value_norm"] = (off + 3, (VALUE_NORM_STATE,))
    return out


def actor_param_count(actor_dims, critic_dims=None, value_norm=False, layer_norm=False, feature_norm=False, recurrent=False, transformer=False):
    """floats of the buffer: the trainable parameters, + VALUE_NORM_STATE with value_norm"""
    off, shape = list(actor_param_layout(actor_dims, critic_dims, value_norm, layer_norm, feature_norm, recurrent, transformer).values())[-1]
    return off + shape[0]


class TensorView(C.Structure):
    _fields_ = [("ptr", C.c_void_p), ("ndim", i32), ("shape", C.c_int64 * 4), ("dtype", i32)]


# The signature of EVERY function include/mqe_hip.h declares, {name: (restype, argtypes)}, stated here and nowhere else: load_library()
# applies the table to the CDLL once and no caller assigns argtypes / restype.  One type rule (tests/test_abi.py holds every entry to the
# header's prototype under it): int / long long / float -> c_int / c_longlong / c_float; mqe_sim* -> c_void_p, mqe_sim** -> POINTER(c_void_p);
# a pointer to mqe_sim_desc / mqe_tensor_view / mqe_actor_shape / mqe_ppo_loss -> POINTER of its mirror; every other pointer (device or host
# data, the stream) -> c_void_p, which takes None, an integer address, a ctypes array and byref(...).
_H = _P = _STREAM = C.c_void_p            # the handle; a data pointer; the hipStream_t
_I, _L, _F = C.c_int, C.c_longlong, C.c_float
_VIEW = C.POINTER(TensorView)


def _sig(*argtypes, res=C.c_int):
    return res, argtypes


SIGNATURES = {
    "mqe_last_error": _sig(res=C.c_char_p),
    "mqe_abi_limits": _sig(_P, _I),
    "mqe_sim_create": _sig(C.POINTER(SimDesc), C.POINTER(_H)),
    "mqe_sim_destroy": _sig(_H),
    "mqe_sim_tensor": _sig(_H, _I, _VIEW),
    "mqe_actor_create": _sig(_H, C.POINTER(ActorShape)),
    "mqe_actor_params": _sig(_H, _VIEW),
    "mqe_rollout": _sig(_H, _I, _P, _P, _L, _P, _P, _P, _I, _STREAM),
    "mqe_rollout_time_outs": _sig(_H, _P, _I),
    "mqe_gae": _sig(_H, _I, _P, _L, _P, _P, _F, _F, _I, _P, _P, _P, _STREAM),
    "mqe_ppo_grad": _sig(_H, _I, _P, _L, _P, _P, _P, _P, _P, _P, _L, _L, C.POINTER(PpoLoss), _I, _P, _P, _STREAM),
    "mqe_ppo_optimizer": _sig(_H, _VIEW, _VIEW),
    "mqe_ppo_adam": _sig(_H, _P, _L, _F, _F, _F, _F, _F, _P, _STREAM),
    "mqe_render_depth": _sig(_H, _P, _I, _I, _F, _P, _P, _F, _STREAM),
    "mqe_render_view": _sig(_H, _I, _P, _P, _P, _I, _I, _F, _P, _P, _F, _STREAM),
    "mqe_measure_heights": _sig(_H, _P, _P, _I, _I, _STREAM),
    "mqe_set_height_refresh": _sig(_H, _P, _P, _I, _I),
    "mqe_debug_dynamics": _sig(_H, _I, _I, _P, _P, _P),
    "mqe_debug_times": _sig(_P),
    "mqe_state_size": _sig(_H, res=_L),
    "mqe_profile_read": _sig(_H, _P, _I, _P),
}
for _names, _s in (("abi_version sizeof_desc", _sig()),          # the families that share a signature
                   ("compute_torques simulate post_physics_step reset_all step_end step_tail refresh_rigid_body_state history_sync", _sig(_H, _STREAM)),
                   ("policy_step defender_command step step_begin step_head step_command step_joint state_save state_load", _sig(_H, _P, _STREAM)),
                   ("post_decimation_step post_physics_stage wrapper_eval", _sig(_H, _I, _STREAM)),
                   ("set_actor_root_state_indexed set_dof_state_indexed", _sig(_H, _P, _I, _STREAM)),
                   ("set_rigid_body_refresh debug_stop_phase profile_enable", _sig(_H, _I)),
                   ("set_return_buffer debug_wave_times debug_tail_times debug_phase_times debug_epilogue_times", _sig(_H, _P))):
    SIGNATURES.update({"mqe_" + _n: _s for _n in _names.split()})
SHARED = ("last_error", "sim_create", "sim_destroy", "sim_tensor")      # what the CPU oracle exports as well (mqo_*), with these signatures


def bind(lib, prefix="mqe_", names=None):
    """Puts SIGNATURES on the functions of a loaded library, where it is loaded: all of them (libmqe_hip.so), or the `names` (without prefix)
    that a library exporting part of the ABI under another prefix shares (the oracle: SHARED as mqo_*)."""
    for name in names or [n[4:] for n in SIGNATURES]:
        f = getattr(lib, prefix + name)
        f.restype, f.argtypes = SIGNATURES["mqe_" + name]
