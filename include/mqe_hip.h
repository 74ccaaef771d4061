/* mqe_hip.h -- C ABI of the MI355X-native MQE rollout engine (drop-in boundary).
 *
 * The reference (ziyanx02/multiagent-quadruped-environment) is pure Python on top of the Isaac Gym tensor API;
 * this library replaces that *inner* boundary and adds a fused fast path.  Each entry point cites the reference
 * call it stands in for.  Conventions: every function returns 0 on success or a negative code and records a
 * message retrievable with mqe_last_error(); no exceptions cross the ABI; the handle owns all device memory it
 * allocates; caller owns buffers it passes in; one handle per GPU; calls on one handle are serialised by the
 * caller; all work is enqueued on the `stream` argument (a hipStream_t passed as void*; NULL = default stream).
 *
 * Memory contract (reference mqe/envs/base/legged_robot.py:549-645, "_init_buffers"): all tensors are float32,
 * env-major:
 *   ROOT_STATE     [N, A+P, 13]  pos3, quat4 (xyzw), linvel3, angvel3 in world frame; agents first   (:567-574)
 *   DOF_STATE      [N, 12A+Dn, 2] (pos, vel); agent dofs first, NPC dofs after                        (:577-585)
 *   CONTACT_FORCE  [N, 17A+Bn, 3] net contact force per reported rigid body, agents first             (:595)
 *   RIGID_BODY_STATE [N, 17A+Bn, 13] the same rows: link-frame origin, quat, linvel, angvel (legged_robot_field.py:196-197)
 *   TORQUES        [N, 12A]                                                                            (:605)
 * Leg/DOF order inside one robot: FL, FR, RL, RR x (hip, thigh, calf); bodies: base, then per leg hip, thigh,
 * calf, foot.
 */
#ifndef MQE_HIP_H
#define MQE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped on EVERY change of a limit, an export, a descriptor field or the meaning of a call (a binding compiled against another header is
 * refused by mqe_sim_create and can compare mqe_abi_limits() with the constants it was built with).  v15 (round 6) over v14: mqe_abi_limits
 * (new export); MQE_MAX_NPCS 16 and mqe_debug_tail_times / mqe_profile_enable(on = N) as shipped late in round 5 under v14; an env's contact
 * list holds the sum of its per-actor caps (+ 8 two-actor slots in scenes of more than four actors, at most 64) instead of min(40, .), and
 * mqe_sim_create refuses a scene whose caps exceed 64; edge_contacts bit 8 + MQE_T_CONTACT_REDUCED (new tensor): optional manifold reduction of a
 * robot's one-sided contacts to its DEEPEST eight instead of the first eight in feature order.  v16 (round 6) over v15: mqe_debug_epilogue_times
 * (new export).  v17 over v16: MQE_T_RIGID_BODY_STATE (new tensor kind before MQE_T_COUNT), mqe_refresh_rigid_body_state and
 * mqe_set_rigid_body_refresh (new exports).  v17, additive (no bump: no limit of mqe_abi_limits, tensor kind, descriptor field or existing call
 * changes): mqe_measure_heights and mqe_set_height_refresh (new exports), MQE_MAX_HEIGHT_POINTS, MQE_HSCAN_SCENERY; mqe_actor_create,
 * mqe_actor_params and mqe_rollout (new exports), mqe_actor_shape, MQE_ACTOR_*, MQE_ROLLOUT_*; mqe_rollout_time_outs and mqe_gae (new exports),
 * MQE_GAE_NORMALIZE; mqe_ppo_grad, mqe_ppo_optimizer and mqe_ppo_adam (new exports), mqe_ppo_loss, MQE_PPO_*; value normalisation: no export
 * and no prototype changes -- MQE_ACTOR_VALUE_NORM (a bit of mqe_actor_shape.activation above the kind byte), MQE_VALUE_NORM_STATE,
 * MQE_GAE_VALUE_NORM, MQE_PPO_VALUE_NORM and MQE_PPO_VALUE_NORM_UPDATE (flag bits that were refused as unknown before); layer normalisation:
 * likewise -- MQE_ACTOR_LAYER_NORM and MQE_ACTOR_FEATURE_NORM (bits 2 and 4 of the kind byte of mqe_actor_shape.activation, refused before); the
 * recurrent actor-critic: likewise -- MQE_ACTOR_RECURRENT (bit 16 of the kind byte, refused before), MQE_ROLLOUT_HIDDEN_IN and
 * MQE_ROLLOUT_HIDDEN_RECORD (mqe_rollout flags 2 and 4, ignored before); the joint-ratio and dual-clip losses: likewise -- MQE_PPO_JOINT and
 * MQE_PPO_DUAL_CLIP (mqe_ppo_grad flags 64 and 128, refused as unknown before) and the typedef mqe_ppo_loss_ex. */
#define MQE_ABI_VERSION 17
#define MQE_MAX_SPHERES 64    /* feature points of one robot (the capsule model has 32, the exact one 60) */
#define MQE_MAX_PRIMS 20      /* collision primitives of one robot (Go1: 18) */
#define MQE_MAX_SELF_PAIRS 384
#define MQE_NBODY 13      /* dynamic bodies of one Go1 after fixed-joint collapsing */
#define MQE_NREP 17       /* reported rigid bodies of one Go1 (feet kept, go1.urdf dont_collapse) */
#define MQE_NDOF 12
#define MQE_MAX_AGENTS 4  /* one env = one 64-lane wavefront of the physics kernel, a body per lane: 13 per Go1 (+ the NPCs): a fifth robot does not fit */
#define MQE_MAX_NPCS 16   /* round 5 (was 9): a 4 x 4 sheep flock = 18 actors, 42 bodies, 84 generalized velocities per env */
#define MQE_FRAME 72      /* 70-float locomotion observation padded to 72 (16-byte rows) */
#define MQE_HIST 30       /* frames of history fed to the locomotion policy (go1.py:395) */
#define MQE_MAX_LAYERS 6
#define MQE_MAX_REWARD_TERMS 12
#define MQE_MAX_HEIGHT_POINTS 1024   /* grid points of one robot's terrain height scan (mqe_measure_heights; the shipped 17 x 11 grid: 187) */
#define MQE_HSCAN_SCENERY 1          /* mqe_measure_heights flag: the tops of the static scenery boxes count as surface */

/* tasks whose wrapper observation / reward are evaluated in-kernel (reference mqe/envs/wrappers) */
enum { MQE_TASK_PLAIN = 0, MQE_TASK_GATE = 1, MQE_TASK_SHEEP = 2, MQE_TASK_SEESAW = 3, MQE_TASK_FOOTBALL_DEFENDER = 4, MQE_TASK_PUSHBOX = 5,
       MQE_TASK_ROTATION = 6, MQE_TASK_BRIDGE = 7, MQE_TASK_WRESTLING = 8, MQE_TASK_TUG = 9 };
/* NPC kinds (reference resources/objects/{ball,sheep,seesaw}.urdf) */
enum { MQE_NPC_NONE = 0, MQE_NPC_BALL = 1, MQE_NPC_SHEEP = 2, MQE_NPC_SEESAW = 3, MQE_NPC_BOX = 4, MQE_NPC_STATIC = 5 };
/* collision primitive types of mqe_robot_model */
enum { MQE_PRIM_SPHERE = 0, MQE_PRIM_CAPSULE = 1, MQE_PRIM_BOX = 2 };
/* control types (reference legged_robot.py:368-392 "P","V","T"; go1.py:315-354 "C") */
enum { MQE_CTRL_C = 0, MQE_CTRL_P = 1, MQE_CTRL_V = 2, MQE_CTRL_T = 3 };
/* termination terms (reference legged_robot_field.py:121-146) */
enum { MQE_TERM_ROLL = 1, MQE_TERM_PITCH = 2, MQE_TERM_Z_LOW = 4, MQE_TERM_Z_HIGH = 8 };
/* reset-noise modes: hash RNG keyed by (seed, global env id, reset count) | scripted (tests: the sequence
 * tools/gen_golden.py's ScriptedRand produces) */
enum { MQE_NOISE_HASH = 0, MQE_NOISE_SCRIPTED = 1 };

typedef struct {
  int32_t n_layers;                       /* Linear layers */
  int32_t dims[MQE_MAX_LAYERS + 1];       /* in, hidden..., out */
  const float* W[MQE_MAX_LAYERS];         /* host pointers, W[l] is (dims[l+1], dims[l]) row-major (torch Linear) */
  const float* b[MQE_MAX_LAYERS];
} mqe_mlp;

typedef struct {
  /* floating-base tree of 13 bodies: 0 = base, 1+3k+{0,1,2} = hip, thigh, calf(+foot) of leg k */
  float mass[MQE_NBODY];
  float com[MQE_NBODY][3];                /* body frame */
  float inertia[MQE_NBODY][6];            /* xx, yy, zz, xy, xz, yz about the COM, body axes */
  float joint_offset[MQE_NBODY][3];       /* joint origin in the parent frame (entry 0 unused) */
  float joint_axis[MQE_NBODY][3];         /* in the child (= parent at q=0) frame */
  float dof_lower[MQE_NDOF], dof_upper[MQE_NDOF];
  float dof_vel_limit[MQE_NDOF];          /* URDF <limit velocity> (go1.urdf:115,157,185: 50 / 28 / 28 rad/s; props["velocity"],
                                             legged_robot.py:315): the solver keeps |joint speed| below it; <= 0 = unlimited */
  /* Collision model (go1.urdf <collision> elements; ABI v12).  PRIMITIVES are the URDF's shapes themselves -- what other bodies
   * collide WITH: sphere (foot), capsule (hip cylinder as `replace_cylinder_with_capsule` makes it, go1_config.py:75; thigh and
   * calf bars as the best-fitting capsule), box (trunk go1.urdf:56, head :80; aligned with the link frame).  FEATURE POINTS
   * ("spheres": centre + radius, rigidly on a link) are what is tested AGAINST the terrain maps, the scenery, the 1-dof link,
   * the free box and the other actors' primitives: the foot spheres, the capsules' end points (capsule radius) and the boxes'
   * corners (radius 0) -- a convex body's outermost point against a plane is always one of them.  Order = priority in the
   * bounded contact list (feet, trunk, head, knees, thigh tops, hips).
   * Two models ship (assets/go1_model.json; desc builder `collision_model`): "capsule" (default; the bars as best-fitting capsules,
   * 32 feature points, surface within 6 mm of the URDF's) and "exact" (round 4: the thigh and calf bars as the URDF's own
   * link-aligned boxes, go1.urdf:170,198, and every box corner that can be outermost -- 60 feature points; the union's support
   * function to < 1 mm, tests/test_models_oracle.py). */
  int32_t n_spheres;
  int32_t sphere_body[MQE_MAX_SPHERES];
  int32_t sphere_reported[MQE_MAX_SPHERES];
  int32_t sphere_prim[MQE_MAX_SPHERES];   /* the primitive the feature point belongs to */
  float sphere_center[MQE_MAX_SPHERES][3];
  float sphere_radius[MQE_MAX_SPHERES];
  int32_t n_prims;
  int32_t prim_type[MQE_MAX_PRIMS];       /* MQE_PRIM_SPHERE / _CAPSULE / _BOX */
  int32_t prim_body[MQE_MAX_PRIMS];
  int32_t prim_reported[MQE_MAX_PRIMS];
  float prim_center[MQE_MAX_PRIMS][3];    /* link frame */
  float prim_axis[MQE_MAX_PRIMS][3];      /* capsule: half of its segment (centre +- axis), link frame; otherwise 0 */
  float prim_half[MQE_MAX_PRIMS][3];      /* box: half extents along the link axes; sphere / capsule: [0] = radius */
  float prim_bound[MQE_MAX_PRIMS];        /* radius of the bounding sphere about prim_center */
  float feature_reach;                    /* no feature point (its sphere included) is ever farther from the base origin than this,
                                             whatever the joint angles: the broad phase between two robots */
  /* self-collision candidates (asset.self_collisions = 0, go1_config.py:73 / legged_robot.py:874): (feature point, primitive)
   * pairs whose links are neither the same nor parent and child and that some pose inside the joint limits brings within 3 cm
   * (mqe/utils/urdf_model.py::_self_pair_candidates), ascending; entry = feature | primitive << 8 */
  int32_t n_self_pairs;
  uint16_t self_pair[MQE_MAX_SELF_PAIRS];
  /* a box of joint angles around the stance inside which no candidate pair comes within 4 cm (dense sampling when the model file is
   * built): a robot whose joints are all inside it skips the self-collision phase (lo > hi: no such box, never skip) */
  float self_safe_lo[MQE_NDOF], self_safe_hi[MQE_NDOF];
} mqe_robot_model;

typedef struct {
  int32_t abi_version;
  /* sizes */
  int32_t num_envs, num_agents, num_npcs, npc_kind, task;
  int32_t env_id_offset;                  /* global index of local env 0 (env sharding across GPUs) */
  int32_t seed;
  /* simulation (reference legged_robot_config.py:211-229) */
  float dt;                               /* 0.005 */
  int32_t decimation;                     /* 4 (go1_config.py:119) */
  float gravity_z;                        /* -9.81 */
  int32_t solver_iterations;              /* sim.physx.num_position_iterations (:221): sweeps over the contact list (solver type 0) resp.
                                             sub-steps of the temporal Gauss-Seidel (solver type 1) */
  float contact_offset, max_depenetration_velocity, friction;
  float erp;                              /* solver type 0 only: share of a penetration asked back per step (velocity-level bias) */
  /* sim.physx.solver_type (legged_robot_config.py:219, "0: pgs, 1: tgs"; 1 in every config of the reference):
   *   0 = projected Gauss-Seidel on velocities with the erp bias (the scheme of rounds 1-3, kept);
   *   1 = temporal Gauss-Seidel as PhysX publishes it: `solver_iterations` sub-steps of dt / n, every contact's separation re-evaluated
   *       from the motion accumulated so far, penetrations pushed out within the sub-step at <= max_depenetration_velocity (no erp)
   *       and the push-out speed taken back once the penetration is gone, positions integrated with the accumulated motion.
   * velocity_iterations = sim.physx.num_velocity_iterations (:222; 0 in every config): further sweeps that see penetrations as
   * touching and move nothing. */
  int32_t solver_type, velocity_iterations;
  /* robot */
  mqe_robot_model robot;
  /* NPC free bodies (ball / sheep): mass, isotropic inertia, spheres in the body frame */
  float npc_mass, npc_inertia;
  int32_t npc_n_spheres;
  float npc_sphere_center[8][3];   /* vs terrain; a box (MQE_NPC_BOX) carries its 8 corners here */
  float npc_sphere_radius[8];
  float npc_box_half[3];           /* MQE_NPC_BOX: half extents of the oriented box the robots' spheres collide with */
  int32_t npc_contact_cap;         /* one-sided (terrain) contacts kept per NPC: 2, a box resting on its face needs 4 */
  /* seesaw (fixed base + revolute plank), reference resources/objects/seesaw.urdf */
  float seesaw_joint_offset[3], seesaw_plank_center[3], seesaw_plank_half[3], seesaw_base_half[3];
  float seesaw_plank_mass, seesaw_plank_inertia_yy, seesaw_vel_limit, seesaw_default_angle;
  float seesaw_column_radius, seesaw_column_length;   /* static column under the platform (seesaw.urdf:90-108) */
  float seesaw_theta_lo, seesaw_theta_hi;             /* plank angles at which an end touches the ground slab */
  /* MQE_NPC_STATIC (bridge.urdf, wrestling.urdf: fixed-base scenery whose collision meshes are boxes): up to 4 world-aligned
     static boxes, centres relative to the NPC root position; the actor reports `npc_reported_bodies` rigid bodies */
  int32_t n_static_boxes, npc_reported_bodies;
  int32_t self_collision;                 /* 1: contacts between the links of one robot (the self_pair list) */
  float static_box_center[4][3], static_box_half[4][3];
  int32_t seesaw_axis;   /* joint of the 1-dof link: 1 = revolute +y (seesaw plank), 2 = revolute +z (revolving door,
                            rotation_door.urdf:44-50), 3 = prismatic +y (the tug-of-war cylinder, cylinder.urdf:37-43); same
                            fixed-base + one-link structure, `seesaw_plank_inertia_yy` holds the inertia about the axis resp.
                            the link mass */
  int32_t seesaw_link_cylinder;   /* 1: the link is an upright cylinder, radius = seesaw_plank_half[0], half height = [2] */
  /* control (reference go1_config.py:108-155) */
  int32_t control_type;
  float action_scale, hip_scale_reduction, clip_actions;
  float torque_limits[MQE_NDOF];
  float kp, kd;
  float default_dof_pos[MQE_NDOF];
  float command_obs[70];                  /* _fill_command_obs (go1.py:411-479) */
  float cmd_lin_scale, cmd_ang_scale;     /* 2.0, 0.25 */
  int32_t clip_command;                   /* 1: Go1.step re-clips to +-1 (go1.py:38); 0: defender variant */
  /* Which column of the command row feeds entry c (0..17) of the locomotion observation (Go1.preprocess_action, go1.py:64-93, with the
   * slots that _fill_command_obs assigns for command.cfg.{vel, body_height, gait_freq, footswing_height, body_pose, stance_width,
   * stance_length, aux_reward}, go1.py:411-479): -1 = the constant command_obs[c]; otherwise row[command_src[c]] * command_scale[c]
   * (control.obs_scales).  Shipped configs: entries 3, 4, 5 <- columns 0, 1, 2, everything else constant, num_command_dims = 3.
   * num_command_dims = width of the rows handed to mqe_policy_step / mqe_step_begin.  Anything but the default is served by the
   * unfused entry points and the exact-f32 layer-0 kernel; the fused wrapper-level mqe_step refuses it (the task wrappers'
   * (N, A, 3) action scaling cannot carry more columns upstream either). */
  int32_t num_command_dims;
  int32_t command_src[18];
  float command_scale[18];
  /* terrain: 2D signed distance [m] to the wall set, raster entry (i, j) at the world point (i hs, j hs) = the vertices of the BarrierTrack heightfield mesh */
  const float* wall_sdf;                  /* host pointer, [sdf_nx][sdf_ny] */
  int32_t sdf_nx, sdf_ny;
  float horizontal_scale, wall_height, ground_z;
  /* low relief of the walkable surface (Perlin noise, barrier_track.py:372-393,421-439; perlin.py:33-72): height [m] above
   * ground_z at the same raster points as wall_sdf, [sdf_nx][sdf_ny] host pointer, or NULL for the flat slab */
  const float* ground_height;
  /* walls of different heights in one scene (barrier_track.py:167-173,191-199,218-239: a (lo, hi) wall_height draws one height per
   * block): top [m] of the wall nearest to each raster point, [sdf_nx][sdf_ny] host pointer, or NULL = wall_height everywhere */
  const float* wall_top;
  /* Edge contacts (round 4): what a test of feature POINTS against shapes cannot see -- an edge cutting into a primitive between its
   * feature points.  edge_contacts is a bit mask: 1 = the vertical edges of the wall prisms (wall_corner: per raster point the world
   * (x, y) of the nearest convex corner of the wall set, [sdf_nx][sdf_ny][2] host pointer, or NULL) against the robots' primitives --
   * a capsule's axis against the edge, the edge against a box primitive's faces; 2 = the robots' capsule axes against the oriented
   * boxes of the scene (1-dof link plank / door, free box, scenery boxes): the closest point of the whole segment, not of its two end
   * points; 4 = the twelve edges of those boxes against the robots' box primitives (off by default: desc builder default 3).  The closest approach of a segment to a convex box
   * is a one-dimensional convex minimisation: both engines run the same 18-evaluation golden-section search.  Such a contact is kept
   * when it lies BETWEEN feature points (segment parameter inside 5 .. 95 %); 0 = round 3's behaviour.
   * Bit 8 (round 6, off by default; not an edge contact, it shares the contact-generation option word): manifold reduction -- a robot that
   * touches the static world at more points than its eight one-sided slots keeps every contact penetrating by more than 1 mm first (deepest
   * 2 mm class first) and fills the rest in feature order, instead of the first eight in feature order whatever their depth; counted in
   * MQE_T_CONTACT_REDUCED instead of MQE_T_CONTACT_OVERFLOW.  Built in both engines and parity-tested; not the default because a limp robot
   * collapsing onto its belly comes to rest in another pose with it. */
  int32_t edge_contacts;
  const float* wall_corner;
  float soft_dof_pos_limit;               /* rewards.soft_dof_pos_limit (legged_robot.py:317-321): fraction of the URDF joint range
                                             outside of which MQE_T_SUBSTEP_EXCEED_DOF_POS_LIMITS flags a joint; 0 = 1.0 */
  /* per-env constants, host pointers */
  const float* env_origins;               /* [N,3] */
  const float* agent_origins;             /* [N,A,3] */
  const float* base_init_state;           /* [A,13] */
  const float* npc_init_state;            /* [P,13] */
  const float* gate_pos;                  /* [N,2] task specific (wrappers' gate_pos / football gate) or NULL */
  /* Run-time terrain curriculum (terrain.curriculum with several rows; legged_robot.py:479-503, called first in reset_idx,
   * go1.py:123-125), upstream's code restated with its accidents (fixture tests/golden/fullstep_pushbox_curriculum.npz): when env e
   * is reset -- the first reset() included, init_done is set before it -- the distance walked is measured on ROW e of the agents'
   * root-state tensor (robot e % A of env e / A: single-agent code left in place) against env e's origin, as the rows stood before
   * any reset of this step; farther than terrain_env_length / 2 moves the env one level up; the commands Go1 never samples are zero,
   * so nothing ever moves down; past the last level a level is re-drawn uniformly; then ONLY env_origins[e] is re-read from the
   * origin table -- the live tensor behind the NPCs' respawn (:437) and the football / push-box wrappers; agent_origins (where the
   * robots respawn), the env_origins_repeat copy behind obs.base_pos, env_info and the copies made at construction (sheep
   * wrapper, gate positions) keep the first track.  terrain_origins [rows][cols][3], terrain_levels / terrain_types [N] are host
   * pointers read at creation; the live values are MQE_T_TERRAIN_LEVELS / MQE_T_ENV_ORIGINS.  A shard of a larger batch
   * (env_id_offset != 0) cannot evaluate it: row e belongs to another shard's env. */
  int32_t terrain_curriculum, terrain_num_rows, terrain_num_cols;
  float terrain_env_length;
  const float* terrain_origins;
  const int32_t* terrain_levels;
  const int32_t* terrain_types;
  /* termination (reference go1_config.py:187-207, legged_robot.py:159-169) */
  int32_t termination_flags, terminate_on_base_contact, max_episode_length;
  float roll_threshold, pitch_threshold, z_low_threshold, z_high_threshold;
  /* reset distribution (reference legged_robot.py:394-470) */
  int32_t noise_mode;
  float dof_ratio_lo, dof_ratio_hi;
  int32_t has_base_pos_range, has_npc_pos_range;
  float base_pos_x_lo, base_pos_x_hi, base_pos_y_lo, base_pos_y_hi;
  float npc_pos_x_lo, npc_pos_x_hi, npc_pos_y_lo, npc_pos_y_hi;
  float base_vel_lo, base_vel_hi;
  /* domain randomisation -- every switch is off in the reference's task configs (go1_config.py:216-247).  Values are drawn
   * once per handle from the hash RNG keyed by the GLOBAL env id and exposed as MQE_T_DOMAIN_PARAMS:
   *   friction (legged_robot.py:283-294): 64 buckets U(lo, hi), one bucket per env, applied to the robots' shapes; a contact
   *     uses the average of the robot's coefficient and `friction` (PhysX combine mode average with terrain / objects);
   *   added base mass (legged_robot.py:332-334) and base CoM shift (legged_robot_field.py:324-334): per robot, body 0;
   *   lag_timesteps (go1.py:337-339, control type C): the joint targets are delayed by this many SUBSTEPS (the reference
   *     shifts its lag buffer in every _compute_torques call); the buffer is never reset;
   *   push_interval / max_push_vel_xy (go1.py:237, legged_robot.py:470-476): every push_interval-th step the base linear
   *     velocity x, y of every robot is re-drawn from U(-max, max) after the step's observations were taken. */
  int32_t rand_friction; float friction_lo, friction_hi;
  int32_t rand_base_mass; float added_mass_lo, added_mass_hi;
  int32_t rand_com; float com_lo[3], com_hi[3];
  int32_t lag_timesteps;
  int32_t push_interval; float max_push_vel_xy;
  /* sheep script (reference go1_sheep.py:35-64) */
  float sheep_movement_scale, sheep_movement_randomness;
  /* wrapper parameters: reward scales in the order documented in mqe/envs/wrappers of this package */
  float reward_scale[MQE_MAX_REWARD_TERMS];
  float wrapper_param[8];
  /* networks */
  mqe_mlp actuator, adaptation, body;
} mqe_sim_desc;

/* tensor kinds for mqe_sim_tensor (device pointers into handle-owned memory, valid for the handle's lifetime;
 * the zero-copy analogue of gym.acquire_*_tensor + gymtorch.wrap_tensor, legged_robot.py:554-567,595) */
enum {
  MQE_T_ROOT_STATE = 0, MQE_T_DOF_STATE, MQE_T_CONTACT_FORCE, MQE_T_TORQUES, MQE_T_ACTIONS, MQE_T_LAST_ACTIONS,
  MQE_T_LOCOMOTION_OBS, MQE_T_HISTORY, MQE_T_LAST_LOCO_ACTION, MQE_T_LAST_TWO_LOCO_ACTION,
                           /* MQE_T_HISTORY [R][MQE_HIST][72] is the f32 ring (slot order; the newest frame sits in the slot written last).  It is an
                              OUTPUT view: large batches run layer 0 on a compact split-f16 copy that the engine maintains frame by frame
                              (csrc/mqe_common.hpp, MQE_H2_FRAME), so host writes into the ring do not reach the policy there.  The action
                              registers, the observation bag and every other state tensor ARE inputs of the next step.  (Handles created
                              with MQE_GEMM_SPLIT=0 read the ring itself.)  A host that WRITES the ring calls mqe_history_sync afterwards:
                              the compact operand is rebuilt from it (columns 6..17 of a written frame must hold the scene's constants,
                              desc.command_obs -- the compact form carries them on the frame's presence flag). */
  MQE_T_ACT_HIST,          /* [4][R][12]: pos_err_last, pos_err_last_last, vel_last, vel_last_last */
  MQE_T_GAIT_INDICES, MQE_T_CLOCK_INPUTS,
  MQE_T_BASE_LIN_VEL, MQE_T_BASE_ANG_VEL, MQE_T_PROJECTED_GRAVITY, MQE_T_BASE_QUAT,
  MQE_T_EPISODE_LENGTH,    /* int32 [N] */
  MQE_T_RESET_BUF, MQE_T_COLLIDE_BUF, MQE_T_TIME_OUT_BUF, MQE_T_R_TERM, MQE_T_P_TERM, MQE_T_Z_HIGH_TERM, /* uint8 [N] */
  MQE_T_OBS_BAG,           /* [R][74]: base_pos3 base_rpy3 dof_pos12 dof_vel12 lin_vel3 ang_vel3 last_action12
                              last_last_action12 projected_gravity3 clock_inputs4 base_quat4, filled by
                              compute_observations (go1.py:153-196) */
  MQE_T_WRAPPER_OBS, MQE_T_WRAPPER_REWARD, MQE_T_REWARD_SUMS, /* [N,A',D], [N,A'], [MQE_MAX_REWARD_TERMS] */
  MQE_T_SHEEP_POS_AVG, MQE_T_SHEEP_POS_VAR,
  MQE_T_RESET_COUNT,       /* int32 [N] */
  MQE_T_SUBSTEP_TORQUES,   /* [N,4,12A] (legged_robot.py:112-115) */
  MQE_T_NPC_NOISE,         /* [N,P,3] injected N(0,1) for the sheep script when noise_mode is SCRIPTED */
  MQE_T_WRAPPER_PACKED,    /* f32 [N*Aw*D + N*Aw + ceil(N/4)] everything a step returns as ONE contiguous buffer: wrapper observation,
                              reward, then MQE_T_RESET_BUF once more as N BYTES (0 / 1; pad bytes of the last word are never written) --
                              the caller views them as bool in place, and the whole buffer is what the env-sharded runner all-gathers */
  MQE_T_DOMAIN_PARAMS,     /* [R][8]: shape friction of the robot's env, added base mass, base CoM shift xyz, 3 unused; read by every
                              physics step, writable (tests / curricula) */
  MQE_T_SUBSTEP_DOF_VEL,   /* [N,4,12A] joint velocities after each substep (legged_robot.py:114) */
  MQE_T_SUBSTEP_EXCEED_DOF_POS_LIMITS,   /* uint8 [N,4,12A] joint outside its soft position limits after each substep (legged_robot.py:115) */
  MQE_T_CONTACT_OVERFLOW,  /* int32 [N]: substeps so far in which the bounded contact list of the env dropped a touching pair (per-actor
                              cap or list end); 0 everywhere = no contact was ever truncated */
  MQE_T_ENV_ORIGINS,       /* [N,3] the LIVE env origins (legged_robot.py:495): what the NPCs respawn around and the football / push-box
                              wrappers subtract; equal to desc.env_origins unless the terrain curriculum has moved an env */
  MQE_T_TERRAIN_LEVELS,    /* int32 [N] terrain level of each env (legged_robot.py:983,490) */
  MQE_T_CONTACT_REDUCED,   /* int32 [N]: with edge_contacts bit 8: substeps so far in which a robot of the env touched the static world at more
                            * points than its eight one-sided slots and the set was reduced (penetrations of more than 1 mm first, deepest 2 mm class first, then feature
                            * order: feet first); MQE_T_CONTACT_OVERFLOW then counts only what is dropped in list order (NPC caps, the two-actor
                            * share, the end of the list).  Without the bit (default): always zero, robots' extra contacts count as overflow */
  MQE_T_RIGID_BODY_STATE,  /* [N, NBR, 13] (v17) Isaac Gym's rigid-body state tensor: the rows of MQE_T_CONTACT_FORCE in their order; origin of the
                              link frame, quaternion xyzw, linear velocity of that origin, angular velocity, all world frame.  Robot rows: base =
                              the root row (bit-equal), hip / thigh / calf by the kinematic chain, foot = its calf moved by the foot joint's origin.
                              NPC rows: a free NPC's root row; a 1-dof link scene's fixed base, then its link from the NPC dof; a static scenery
                              actor's root pose with zero velocity in each of its rows.  Written only by mqe_refresh_rigid_body_state and, while
                              mqe_set_rigid_body_refresh is on, by every post-physics step; derived data, not part of mqe_state_save's blob */
  MQE_T_COUNT
};

typedef struct {
  void* ptr;               /* device pointer */
  int32_t ndim;
  int64_t shape[4];
  int32_t dtype;           /* 0 f32, 1 i32, 2 u8 */
} mqe_tensor_view;

typedef struct mqe_sim mqe_sim;

const char* mqe_last_error(void);
int mqe_abi_version(void);
/* the compile-time limits of the library, for a binding to compare with the header it was built against: writes up to n of
 * { MQE_ABI_VERSION, MQE_MAX_AGENTS, MQE_MAX_NPCS, MQE_MAX_SPHERES, MQE_MAX_PRIMS, MQE_MAX_SELF_PAIRS, MQE_MAX_LAYERS, MQE_MAX_REWARD_TERMS,
 *   MQE_NBODY, MQE_NREP, MQE_NDOF, MQE_FRAME, MQE_HIST, MQE_T_COUNT } and returns how many there are (14) */
int mqe_abi_limits(int32_t* out, int n);
int mqe_sizeof_desc(void);   /* sizeof(mqe_sim_desc): lets a foreign-language binding verify its struct mirror */

/* gym.create_sim + load_asset + create_env/create_actor + add_triangle_mesh + prepare_sim
 * (reference legged_robot.py:255-261,754-923; barrier_track.py:395-410; base_task.py:91) */
int mqe_sim_create(const mqe_sim_desc* desc, mqe_sim** out);
int mqe_sim_destroy(mqe_sim* s);
/* gym.acquire_*_tensor + gymtorch.wrap_tensor (legged_robot.py:554-567) */
int mqe_sim_tensor(mqe_sim* s, int kind, mqe_tensor_view* out);

/* ---- unfused, Isaac-Gym-shaped entry points (inner boundary) ---- */
/* Go1.preprocess_action (go1.py:64-108): command -> locomotion obs -> history -> adaptation+body MLP ->
 * clipped joint-target actions.  `command` is [R,3] device memory (already scaled by the task wrapper). */
int mqe_policy_step(mqe_sim* s, const float* command, void* stream);
/* Go1FootballDefender._get_defender_action (go1_football_defender.py:56-80): scripted (x, y, yaw) command of agent 2
 * from the current state -> out_dev [N,3] */
int mqe_defender_command(mqe_sim* s, float* out_dev, void* stream);
/* Go1._compute_torques (go1.py:315-354) / LeggedRobot._compute_torques (legged_robot.py:368-392) */
int mqe_compute_torques(mqe_sim* s, void* stream);
/* gym.set_dof_actuation_force_tensor + gym.simulate + refresh_dof_state_tensor (go1.py:52-56): one dt of rigid-body
 * dynamics with the torques currently in MQE_T_TORQUES; also refreshes the net contact forces */
int mqe_simulate(mqe_sim* s, void* stream);
/* post_decimation_step (legged_robot.py:112-115) */
int mqe_post_decimation_step(mqe_sim* s, int dec_i, void* stream);
/* post_physics_step (legged_robot_field.py:117-119 -> legged_robot.py:117-157) incl. termination, NPC script,
 * in-kernel reset, compute_observations, and the task wrapper's observation / reward */
int mqe_post_physics_step(mqe_sim* s, void* stream);
/* The same in the stages the reference's method has (legged_robot.py:117-157), for a host that runs code of its own between them -- a
 * subclass's check_termination / _step_npc / reset_idx / compute_observations: any OR of
 *   MQE_POST_FRAME    episode counter, body-frame velocities, gravity, gait clock, the wrapper's copy of the NPC rows (:126-139) and the
 *                     default check_termination (:159-169, legged_robot_field.py:121-146) -> MQE_T_RESET_BUF & co;
 *   MQE_POST_NPC      the task's NPC script (:146: the sheep's flocking walk);
 *   MQE_POST_RESET    reset_idx of the envs whose MQE_T_RESET_BUF is set WHEN THIS STAGE RUNS (:147-148), terrain curriculum included;
 *   MQE_POST_OBS      compute_observations, last_actions, last_dof_vel (:149-152);
 *   MQE_POST_WRAPPER  the task wrapper's observation / reward and the periodic push; the step counter advances with this stage.
 * Stages of one call run in this order; mqe_post_physics_step == MQE_POST_ALL in one launch (the staged form is a plain
 * thread-per-env kernel per call: the same arithmetic -- results equal to the last bit or two -- not the fast path). */
enum { MQE_POST_FRAME = 1, MQE_POST_NPC = 2, MQE_POST_RESET = 4, MQE_POST_OBS = 8, MQE_POST_WRAPPER = 16, MQE_POST_ALL = 31,
       MQE_POST_WRAPPER_LEVEL = 32 };   /* modifier of MQE_POST_WRAPPER: the call comes from a task wrapper's step() (go1tug re-poses its slider then) */
int mqe_post_physics_stage(mqe_sim* s, int stages, void* stream);
/* task wrapper observation + reward only (mqe/envs/wrappers/go1_<task>_wrapper.py step()/reset() bodies) from the current contents of
 * MQE_T_OBS_BAG, MQE_T_ROOT_STATE (NPC rows), the termination flags and MQE_T_SHEEP_POS_*; part of
 * mqe_post_physics_step / mqe_reset_all, exposed separately so the wrappers can be checked against golden vectors */
int mqe_wrapper_eval(mqe_sim* s, int is_reset_call, void* stream);
/* gym.set_actor_root_state_tensor_indexed / set_dof_state_tensor_indexed (legged_robot.py:419-421,468-470):
 * state tensors are live device memory, so these only invalidate cached per-env data for the listed actors */
int mqe_set_actor_root_state_indexed(mqe_sim* s, const int32_t* actor_ids_dev, int n, void* stream);
int mqe_set_dof_state_indexed(mqe_sim* s, const int32_t* actor_ids_dev, int n, void* stream);
/* Go1.reset (go1.py:147-151): reset_idx(all) + compute_observations, no physics step */
int mqe_reset_all(mqe_sim* s, void* stream);

/* ---- fused fast path: one Go1.step (go1.py:35-62) + task wrapper ----
 * actions: [N, A', 3] raw policy actions in [-1,1] (the wrapper's clip and action_scale are applied inside);
 * results land in MQE_T_WRAPPER_OBS / MQE_T_WRAPPER_REWARD / MQE_T_RESET_BUF. */
int mqe_step(mqe_sim* s, const float* actions, void* stream);
/* mqe_step in two halves, for a host that has launches of its own to place between them: _begin enqueues the wrapper head
 * and the locomotion policy (Go1.step up to go1.py:41), _end the decimation loop, post-physics step and wrapper
 * (go1.py:46-62).  mqe_step == _begin; _end.  The env-sharded runner issues the all-gather of the PREVIOUS batch between
 * the two, so that the collective shares the GPU with the physics kernel (wave-granular, tolerant of a few displaced
 * CUs) and not with the policy GEMM (one workgroup per CU: any displaced workgroup costs a whole extra round). */
int mqe_step_begin(mqe_sim* s, const float* actions, void* stream);
int mqe_step_end(mqe_sim* s, void* stream);
/* mqe_step_begin in two parts, for a host that wants to place launches of its own between layer 0 of the policy and the rest of it:
 * mqe_step_head = wrapper head + history frame + layer 0 (k_pre_policy, k_gemm_*), mqe_step_tail = the rest of the policy
 * (k_policy_tail); then mqe_step_end as usual.  The env-sharded runner issues the previous batch's all-gather after the head -- the
 * RCCL kernel then shares the GPU with the policy tail, which leaves every CU three quarters empty, instead of with either of the two
 * kernels that fill the machine exactly -- and makes the physics kernel wait for it (bench.py --gather tail). */
int mqe_step_head(mqe_sim* s, const float* actions, void* stream);
int mqe_step_tail(mqe_sim* s, void* stream);
/* Where the following launches write what a step returns (the MQE_T_WRAPPER_PACKED layout: obs | reward | done): a device
 * buffer of the caller, at least as large as MQE_T_WRAPPER_PACKED, or NULL for the engine's own buffer (the one the
 * MQE_T_WRAPPER_* views show).  Host-side switch only; a launch uses the buffer that was set when it was enqueued.  The
 * wrappers hand every step a fresh tensor this way (the reference returns new tensors each step) instead of copying. */
int mqe_set_return_buffer(mqe_sim* s, float* packed_dev);
/* Go1.step itself (go1.py:35-62) as one call for control type "C": `command` [R, num_command_dims] = the per-robot command rows
 * Go1.step receives (already scaled by a task wrapper, if any; re-clipped to +-1 inside as go1.py:38 does unless the scene is the
 * defender variant), policy, decimation loop and post-physics step as the five fused launches.  No wrapper head and no wrapper
 * evaluation: the task wrapper's observation, reward and bookkeeping belong to mqe_step.  Equivalent to mqe_policy_step + decimation x
 * (mqe_compute_torques, mqe_simulate, mqe_post_decimation_step) + mqe_post_physics_step. */
int mqe_step_command(mqe_sim* s, const float* command, void* stream);
/* The same for the low-level control types "P" / "V" / "T" (Go1.step's else branch, go1.py:42-44 -> pre_physics_step,
 * legged_robot.py:108-110, and the PD / torque laws of legged_robot.py:380-392): actions [R, 12] joint-space actions, clipped
 * to clip_actions inside; no locomotion policy runs.  The decimation loop, post-physics step and (plain) wrapper are the
 * fused ones. */
int mqe_step_joint(mqe_sim* s, const float* actions12, void* stream);

/* ---- on-device rollouts: a small Gaussian actor (and optional critic) evaluated by the engine, T steps per call ----
 * v17, additive (new exports only; no tensor kind, descriptor field, limit of mqe_abi_limits or state-blob change).
 * The networks are MLPs on the task wrapper's observation (the D floats of a row of MQE_T_WRAPPER_OBS): actor D -> h... -> 3 with a linear
 * output = the mean, a state-independent log_std[3], critic D -> h... -> 1.  One kernel (csrc/kernels_actor.hpp, k_actor: arithmetic and
 * summation order stated there) per rollout step, R' = N x A' rows:
 *   a_j  = mean_j + exp(log_std_j) z_j,  z_j ~ N(0, 1) from the counter RNG keyed by (seed, GLOBAL env id, MQE_RNG_ACTOR + n, agent * 3 + j),
 *          MQE_RNG_ACTOR = 0x70000000, n = the handle's count of post-physics steps when the launch is enqueued (the counter that keys the
 *          NPC script's draws; part of mqe_state_save): a trajectory does not depend on how the envs are sharded and continues bit for bit
 *          after mqe_state_load;
 *   logp = sum_j (-z_j^2 / 2 - log_std_j - ln(2 pi) / 2): the density of the UNCLIPPED sample a;
 *   the following step receives action_gain * a (mqe_step clips to +-1 and applies the task's action scale as for any caller).
 * Parameter buffer (mqe_actor_params), flat f32: per layer W (out, in) row-major as torch.nn.Linear.weight, then b (out); the actor's
 * layers first, then the critic's, then log_std[3]. */
#define MQE_ACTOR_MAX_LAYERS 4        /* Linear layers of one network */
#define MQE_ACTOR_MAX_HIDDEN 256      /* width of a hidden layer */
#define MQE_ACTOR_MAX_OBS 128         /* D */
#define MQE_ACTOR_TANH 0
#define MQE_ACTOR_RELU 1
#define MQE_ROLLOUT_MAX_STEPS 4096    /* T of one mqe_rollout call */
#define MQE_ROLLOUT_DETERMINISTIC 1   /* flags bit 0: a = mean, logp evaluated at z = 0 */
typedef struct {
  int32_t obs_dim;                                /* D: must equal the scene's MQE_T_WRAPPER_OBS width */
  int32_t act_dim;                                /* 3 */
  int32_t actor_layers;                           /* 1 .. MQE_ACTOR_MAX_LAYERS */
  int32_t actor_dims[MQE_ACTOR_MAX_LAYERS + 1];   /* obs_dim, hidden ..., 3 */
  int32_t critic_layers;                          /* 0 = no critic */
  int32_t critic_dims[MQE_ACTOR_MAX_LAYERS + 1];  /* obs_dim, hidden ..., 1 */
  int32_t activation;                             /* MQE_ACTOR_TANH / MQE_ACTOR_RELU on every hidden layer of both networks (+ the bits of the value- and layer-normalisation sections) */
  float action_gain;                              /* 1 for the task wrappers, 0.5 for the OpenRL adapter (which feeds 0.5 * a) */
} mqe_actor_shape;
/* Allocates the engine-owned parameter buffer (zeroed) and the action staging buffer; a second call replaces the first.  Refused with
 * -6 and a message: obs_dim differs from the scene's wrapper-observation width; the scene has no task observation (MQE_TASK_PLAIN: go1plane,
 * the football stubs); num_command_dims != 3; control type other than C; act_dim != 3; a layer count, width or dims[] end outside the limits above. */
int mqe_actor_create(mqe_sim* s, const mqe_actor_shape* shape);
/* the flat parameter buffer as a 1-d f32 view: live device memory like every tensor of the handle -- a trainer copies its updated
 * parameters into it on the device; launches enqueued later on the same stream see them.  -6 without an actor. */
int mqe_actor_params(mqe_sim* s, mqe_tensor_view* out);
/* T steps in one host call: per step k_actor, then the launches of mqe_step (registered rigid-body / height-scan refreshes included), each
 * step's return buffer redirected into the trajectory; a final value-only launch (no draw) when value_dev is given.  No synchronisation.
 *   packed_dev   T + 1 rows of row_stride floats, row_stride >= the MQE_T_WRAPPER_PACKED length and a multiple of 4; 16-byte aligned.  Row 0 =
 *                the starting observation with reward and done bytes zeroed; row t + 1 = what step t returns, in mqe_set_return_buffer's
 *                obs | reward | done-bytes layout.  Floats of a row beyond that layout are never written.
 *   obs0_dev     (N, A', D) observation the first action is computed from; NULL = the engine's own MQE_T_WRAPPER_OBS (stale after a step
 *                that was given a return buffer of the caller's: such a caller passes the observation it holds)
 *   actions_dev  [T, N, A', 3] the unclipped samples;  logp_dev [T, N, A'] or NULL;  value_dev [T + 1, N, A'] or NULL (NULL is required
 *                without a critic), entry T = the value of the last observation.  4-byte alignment.
 *   flags        MQE_ROLLOUT_DETERMINISTIC
 * Afterwards the return-buffer switch points at the engine's own buffer, and one device-to-device copy has brought that buffer (the
 * MQE_T_WRAPPER_* views) to row T: a following call with obs0_dev == NULL continues the trajectory.  Refusals enqueue nothing: -1 null handle / packed_dev /
 * actions_dev; -6 no actor, T <= 0, T > MQE_ROLLOUT_MAX_STEPS, a misaligned pointer, a bad row_stride, value_dev without a critic; -8 inside an
 * open step (mqe_step_begin / _head without mqe_step_end). */
int mqe_rollout(mqe_sim* s, int T, const float* obs0_dev, float* packed_dev, long long row_stride, float* actions_dev, float* logp_dev,
                float* value_dev, int flags, void* stream);
/* registers (NULL: removes) a destination for the per-step time-out flags of the following mqe_rollout calls:
 * time_outs_dev [capacity_steps][N] uint8, row t = MQE_T_TIME_OUT_BUF as step t of the call left it.
 * MQE_T_TIME_OUT_BUF is overwritten by every step; a learner that bootstraps timed-out episodes (legged_gym / rsl_rl:
 * reward += gamma * value * time_outs) needs the flag of every step.  While a destination is registered, mqe_rollout enqueues one N-byte
 * device-to-device copy behind the launches of each step, on the same stream; with none registered its launch sequence is unchanged.  A
 * rollout with T > capacity_steps is refused with -6 and enqueues nothing.  The registration is host state of the handle only (not part of
 * mqe_state_save); the memory stays the caller's.  -1 null handle; -6 capacity_steps <= 0 with a non-null pointer.  v17, additive. */
int mqe_rollout_time_outs(mqe_sim* s, uint8_t* time_outs_dev, int capacity_steps);

/* ---- GAE(lambda) advantages and returns of a trajectory, on the device (csrc/kernels_gae.hpp: k_gae, k_gae_normalize) ----
 * v17, additive.  The handle supplies the shapes (N, A', D) and owns one scratch buffer; no actor is needed (the values may come from a
 * torch critic), and the call runs outside or inside an open step.  R' = N x A', row r = env * A' + agent.
 *   packed_dev, row_stride  a trajectory in mqe_rollout's layout: the reward of step t, row r, is float (N A' D + r) of packed row t + 1,
 *                           the done byte of step t, env e, is byte e behind the R' rewards of that row
 *   value_dev      [T + 1][R']: the critic at obs[t]; entry T bootstraps the last step
 *   time_outs_dev  [T][N] uint8 (mqe_rollout_time_outs) or NULL
 *   adv_dev, ret_dev  [T][R'] outputs;  stats_dev float[2] or NULL: (mean, std) of the advantages, written by MQE_GAE_NORMALIZE calls only
 * Per row, t = T - 1 ... 0, adv = 0 in front, all f32 (the exact statement: csrc/kernels_gae.hpp), d = done[t][e], to = time_outs ?
 * (time_outs[t][e] & d) : 0, v = value[t][r], vn = value[t + 1][r]:
 *   rr    = to ? fmaf(gamma, v, reward) : reward          rsl_rl's time-out bootstrap with the value of the step's own observation
 *   delta = (d ? rr : fmaf(gamma, vn, rr)) - v
 *   adv   = d ? delta : fmaf(gamma * lam, adv, delta)
 *   ret   = adv + v
 * MQE_GAE_NORMALIZE: adv_dev becomes (adv - mean) / (std + 1e-8f), mean and unbiased (n - 1) std over all T x R' values, accumulated and
 * applied in f64 in a fixed order (no atomics: the same bits on every run), rounded to f32 once; ret_dev is computed from the un-normalised
 * advantage.  EACH SHARD NORMALISES OVER ITS OWN ROWS: a multi-GPU learner that wants global statistics calls without the flag and
 * normalises itself.  The call never synchronises, except the FIRST normalising call of a handle, which allocates the scratch buffer (2
 * doubles per 64 rows, freed with the handle) and synchronises once.
 * Refusals enqueue nothing and write nothing: -1 null handle / packed_dev / value_dev / adv_dev / ret_dev; -6 with a message naming the
 * argument: T outside 1 .. MQE_ROLLOUT_MAX_STEPS; row_stride below the packed length or not a multiple of 4; a pointer that is not 4-byte
 * aligned; gamma or lam outside [0, 1] or NaN; MQE_GAE_NORMALIZE with T x R' < 2; an output range that overlaps an input range or another
 * output; unknown flag bits. */
#define MQE_GAE_NORMALIZE 1   /* flags bit 0 */
int mqe_gae(mqe_sim* s, int T, const float* packed_dev, long long row_stride, const float* value_dev, const uint8_t* time_outs_dev,
            float gamma, float lam, int flags, float* adv_dev, float* ret_dev, float* stats_dev, void* stream);

/* ---- The PPO update on the engine's own actor-critic, on the device (csrc/kernels_ppo.hpp: k_ppo_grad, k_ppo_reduce, k_ppo_norm, k_ppo_adam) ----
 * v17, additive.  rollout -> gae -> (grad, adam) per minibatch: the parameters never leave the buffer k_actor reads, nothing synchronises, and
 * the gradient has the same bits on every run (no floating-point atomics; a fixed grid and fixed-order reductions).  Needs an actor WITH a critic.
 * mqe_ppo_grad: the clipped-surrogate loss of rsl_rl and its gradient over one minibatch.
 *   T, packed_dev, row_stride  a trajectory in mqe_rollout's layout; sample s = t * R' + r, 0 <= s < T * R', has its observation at
 *                              packed_dev + t * row_stride + r * D
 *   actions_dev [T][R'][3], logp_dev [T][R'], value_dev [T + 1][R'] (the first T rows are v_old), adv_dev, ret_dev [T][R']
 *   index_dev, first, count    the minibatch, M = count samples: index_dev[first .. first + count) (int32: a slice of a device permutation) or,
 *                              with index_dev NULL, the range first .. first + count.  INDEX VALUES ARE THE CALLER'S RESPONSIBILITY to keep inside
 *                              [0, T * R'): the kernel clamps them, so that a bad one cannot read outside the trajectory -- it is not reported
 *   loss, flags                clip_ratio c, value_coef, entropy_coef, value_clip c_v (used with MQE_PPO_CLIP_VALUE only)
 *   grad_dev   [n_params] f32 in exactly mqe_actor_params' layout; EVERY element is written by every call (a parameter without gradient: 0)
 *   stats_dev  NULL or float[MQE_PPO_STATS]: mean L_pi, mean L_v, H, L, mean of logp_old - logp (approximate KL), share of samples with
 *              |ratio - 1| > clip_ratio; accumulated in f64
 * Per sample, all f32 (the exact statement, the gradient at the kinks and the layout: csrc/kernels_ppo.hpp):
 *   mean = actor(obs), v = critic(obs);  z_j = (a_j - mean_j) exp(-log_std_j);  logp = sum_j (-0.5 z_j^2 - log_std_j) - 1.5 ln(2 pi)
 *   ratio = exp(logp - logp_old);  L_pi = -min(ratio adv, clamp(ratio, 1 - c, 1 + c) adv)
 *   L_v = (v - ret)^2, with MQE_PPO_CLIP_VALUE max((v - ret)^2, (v_c - ret)^2), v_c = v_old + clamp(v - v_old, -c_v, c_v)
 *   H = sum_j log_std_j + 1.5 (1 + ln(2 pi));  L = mean(L_pi) + value_coef mean(L_v) - entropy_coef H
 * The call changes no parameter and no input and never synchronises, except that the FIRST call after mqe_actor_create allocates the
 * scratch (256 partial gradients; released with the actor) and synchronises once.  A sharded learner all-reduces grad_dev between this call
 * and mqe_ppo_adam (each shard's gradient carries its own 1 / M: weight by the row counts).
 * Refusals enqueue nothing and write nothing: -1 null handle or required pointer (everything but index_dev and stats_dev); -6 with a message
 * naming the argument: no actor, or an actor without a critic; T outside 1 .. MQE_ROLLOUT_MAX_STEPS; row_stride below the packed length or not
 * a multiple of 4; a misaligned pointer (4 bytes; packed_dev 16); count < 1, first < 0, first + count > T * R' without an index list;
 * clip_ratio, value_clip or a coefficient that is negative, NaN or infinite; unknown flag bits; grad_dev or stats_dev overlapping an input,
 * the parameter buffer or each other.
 * mqe_ppo_optimizer: live views of Adam's two moment buffers, [n_params] f32 each in the parameters' layout, allocated ZEROED on first use
 * (here or in mqe_ppo_adam) and released with the actor: a new mqe_actor_create drops them.
 * mqe_ppo_adam: one torch.optim.Adam step (no weight decay, no amsgrad) in place on the parameter buffer, ordered on the stream.  step >= 1
 * is the CALLER's count -- the engine keeps none: a checkpoint is the three buffers and that integer, nothing goes into mqe_state_save.
 *   max_grad_norm > 0: g is first scaled by min(1, max_grad_norm / (norm + 1e-6)), norm = the L2 norm over all parameters, accumulated in f64 in a
 *   fixed order (clip_grad_norm_);  norm_dev, when given, receives the unscaled norm (f32)
 *   m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2;  p -= (lr / (1 - b1^step)) m / (sqrt(v) / sqrt(1 - b2^step) + eps)
 *   (the bias corrections and 1 - b are formed on the host in f64 and passed as f32)
 * -1 null handle / grad_dev; -6: no actor, step < 1, a misaligned pointer, lr / max_grad_norm not finite, a beta outside [0, 1), eps negative or
 * not finite, grad_dev or norm_dev overlapping the parameter or moment buffers or each other. */
typedef struct { float clip_ratio, value_coef, entropy_coef, value_clip; } mqe_ppo_loss;
/* what `loss` points at under MQE_PPO_DUAL_CLIP (the joint-ratio and dual-clip section below): 32 bytes, the first 16 are mqe_ppo_loss */
typedef struct { float clip_ratio, value_coef, entropy_coef, value_clip, dual_clip, reserved[3]; } mqe_ppo_loss_ex;
#define MQE_PPO_CLIP_VALUE 1      /* flags bit 0 */
#define MQE_PPO_STATS 6
int mqe_ppo_grad(mqe_sim* s, int T, const float* packed_dev, long long row_stride, const float* actions_dev,
                 const float* logp_dev, const float* value_dev, const float* adv_dev, const float* ret_dev,
                 const int32_t* index_dev, long long first, long long count, const mqe_ppo_loss* loss, int flags,
                 float* grad_dev, float* stats_dev, void* stream);
int mqe_ppo_optimizer(mqe_sim* s, mqe_tensor_view* m_out, mqe_tensor_view* v_out);   /* live views of the two moment buffers */
int mqe_ppo_adam(mqe_sim* s, const float* grad_dev, long long step, float lr, float beta1, float beta2, float eps,
                 float max_grad_norm, float* norm_dev, void* stream);

/* ---- Value normalisation: running return statistics beside the parameters (csrc/kernels_vn.hpp: k_vn_denorm, k_vn_moments, k_vn_apply) ----
 * v17, additive: OpenRL / MAPPO ValueNorm with the rounding points fixed.  The critic predicts returns in units of their running, debiased mean
 * and standard deviation; GAE works on de-normalised values; the value loss compares against normalised returns; a minibatch folds its returns
 * into the statistics before it is normalised; v_old stays in the units it was predicted in.  The same bits on every run (no atomics).
 * THE FIVE CONSTANTS BELOW ARE NOT #DEFINED BY THIS HEADER YET: tests/test_rollout.py, test_gae.py and test_ppo.py pin the exact set of
 * MQE_ACTOR_*, MQE_GAE_* and MQE_PPO_* defines.  Their values are stated here, defined under these names in csrc/kernels_vn.hpp (which the
 * engine compiles) and mirrored in mqe/engine/abi.py; tests/test_value_norm.py holds the three statements together.  A C caller passes the numbers.
 *   MQE_ACTOR_VALUE_NORM = 256   MQE_VALUE_NORM_STATE = 5   MQE_GAE_VALUE_NORM = 8   MQE_PPO_VALUE_NORM = 8   MQE_PPO_VALUE_NORM_UPDATE = 16
 * State: MQE_VALUE_NORM_STATE floats w = (m, q, d, mu, sigma) -- running mean, running mean of squares, debiasing term, and the derived pair
 * every consumer reads.  beta = 0.99999f (widened to double, 1 - beta formed in f64), eps = 1e-5f, var_min = 1e-2f:
 *   dc = max(d, eps);  mu = (float)(m / dc);  sigma = (float)sqrt(max(q / dc - (m / dc)^2, var_min))       in f64 from the stored f32 (m, q, d)
 *   update over the M returns x_i of a minibatch (exactly the samples mqe_ppo_grad reads, index clamping included), sums in f64:
 *   m' = (float)(beta m + (1 - beta) sum x_i / M);  q' likewise with x_i^2;  d' = (float)(beta d + (1 - beta));  then (mu, sigma) from (m', q', d')
 *   de-normalise: fmaf(v, sigma, mu);  normalise: (float)(((double)x - mu) * (1.0 / (double)sigma))
 * The f32 state has ValueNorm's cancellation limit: q / dc - mu^2 loses digits once mu^2 >> the variance.
 * MQE_ACTOR_VALUE_NORM, or-ed into mqe_actor_shape.activation (the low byte stays the kind): needs a critic (-6 otherwise).  The parameter
 *   allocation becomes n_params + MQE_VALUE_NORM_STATE floats, the state behind log_std, created as (0, 0, 0, 0, 0.1f); mqe_actor_params returns
 *   the whole view.  n_params, grad_dev, the Adam moments and everything mqe_ppo_adam touches keep meaning the trainable parameters: no
 *   optimiser step reads or writes the state.  A learner checkpoint is the parameter view (state included), the two moment buffers and the
 *   step count; nothing enters mqe_state_save.  EACH SHARD KEEPS ITS OWN STATISTICS, as with MQE_GAE_NORMALIZE.
 * MQE_GAE_VALUE_NORM (mqe_gae flags): value_dev holds NORMALISED critic outputs; one more launch writes fmaf(v, sigma, mu) for all (T + 1) R'
 *   values into engine-owned scratch, and the recursion (and MQE_GAE_NORMALIZE) runs on that.  adv_dev and ret_dev are in reward units;
 *   value_dev is not written.
 * MQE_PPO_VALUE_NORM (mqe_ppo_grad flags): the minibatch's ret_dev entries are normalised with the current (mu, sigma) into engine-owned [T][R']
 *   scratch at their own sample positions, and the loss reads those: stats_dev[1] (mean L_v) is then in normalised units.  ret_dev is not written.
 * MQE_PPO_VALUE_NORM_UPDATE (needs MQE_PPO_VALUE_NORM, -6 otherwise): the minibatch's returns are first folded into the state, so the call
 *   changes the five state floats and nothing else of the parameter buffer.  For every other flag combination "the call changes no parameter"
 *   stays true.
 * The scratch is allocated by the first flagged call and grown when T grows; such a call synchronises once, as the other first calls do, and the
 * scratch is released with the actor.  Refused (-6, naming flags; nothing enqueued or written, state untouched): a flag on a handle without an
 * actor created with MQE_ACTOR_VALUE_NORM.  Bits 2 and 4 of both flag words stay unknown. */

/* ---- Layer normalisation in the actor-critic, forward and backward (csrc/kernels_ln.hpp: k_actor_ln, k_ln_grad) ------------------------------
 * v17, additive: no prototype, no struct and no #define of this header changes.  OpenRL's PPONet keeps MAPPO's MLP base: a LayerNorm on the
 * observation and one behind every hidden activation.  The operator is torch.nn.LayerNorm(n, eps = 1e-5, elementwise_affine = True) over the n
 * features of one row: u = gamma * xhat + beta, xhat = (a - mean(a)) / sqrt(mean((a - mean(a))^2) + eps) (biased variance), all f32, two-pass
 * and centred; the summation order is stated in csrc/kernels_ln.hpp and restated on the host by tests/layer_norm_ref.py.
 * THE TWO CONSTANTS BELOW ARE NOT #DEFINED BY THIS HEADER (tests/test_rollout.py pins the exact set of MQE_ACTOR_* defines).  Their values are
 * stated here, defined under these names in csrc/kernels_ln.hpp (which the engine compiles) and mirrored in mqe/engine/abi.py;
 * tests/test_layer_norm.py holds the three statements together.  A C caller passes the numbers.
 *   MQE_ACTOR_LAYER_NORM = 2   MQE_ACTOR_FEATURE_NORM = 4
 * Both are bits of the KIND BYTE of mqe_actor_shape.activation, or-ed with MQE_ACTOR_TANH / MQE_ACTOR_RELU (and with MQE_ACTOR_VALUE_NORM above
 * the byte or not); every other bit of the byte is refused as before (-6), and so is bit 512.  They apply to both networks of the handle:
 * MQE_ACTOR_LAYER_NORM    the hidden norm: a LayerNorm behind the activation of EVERY hidden layer (a = tanh / relu (W x + b), the next layer
 *   reads u); never behind the output layer; a network of one Linear layer has none.
 * MQE_ACTOR_FEATURE_NORM  the feature norm: a LayerNorm on the D observation floats in front of layer 0; each network has its own gamma, beta.
 * Parameter buffer, per network and in this order: [norm_in.weight (D), norm_in.bias (D)] with the feature norm; per layer l weight, bias, and
 *   for a hidden layer under the hidden norm [norm.weight (n), norm.bias (n)]; then the critic likewise, log_std[3] and the value-normalisation
 *   state as before.  With both bits clear the layout is the plain one, bit for bit.  mqe_actor_create sets every gamma to 1 (the buffer is
 *   otherwise zeroed).  n_params, grad_dev, the Adam moments and the gradient clip cover gamma and beta like any weight or bias.
 * mqe_rollout, mqe_gae, mqe_ppo_grad, mqe_ppo_optimizer and mqe_ppo_adam are called as before.  A handle created with either bit launches
 * k_actor_ln and k_ln_grad instead of k_actor and k_ppo_grad; a handle created without them launches what it always did.  The gradient of a
 * normalised layer (du = the gradient with respect to u):  dgamma = sum over the samples of du * xhat;  dbeta = sum of du;
 *   dxhat = du * gamma;  da = rstd * (dxhat - mean(dxhat) - xhat * mean(dxhat * xhat));  then the activation's derivative.
 * No atomics: the same bits on every run.  Every shape mqe_actor_create accepts without the bits it accepts with them (D up to 128 included);
 * k_ln_grad's LDS rule (csrc/kernels_ln.hpp) takes 32-row tiles earlier than k_ppo_grad's. */

/* ---- Recurrent actor-critic: a GRU cell in the rollout's networks, its state carried and recorded (csrc/kernels_gru.hpp: k_actor_gru, k_actor_gru_ln) ----
 * v17, additive: no prototype, no struct and no #define of this header changes.  OpenRL's PPONet with use_recurrent_policy is MAPPO's: behind the
 * MLP base a one-layer GRU(H, H) and, with the norms, a LayerNorm(H); then the linear head; the state is zeroed wherever the step before ended an
 * episode.  THE THREE CONSTANTS BELOW ARE NOT #DEFINED BY THIS HEADER (tests/test_rollout.py pins the exact sets of MQE_ACTOR_* and MQE_ROLLOUT_*
 * defines).  Their values are stated here, defined under these names in csrc/kernels_gru.hpp (which the engine compiles) and mirrored in
 * mqe/engine/abi.py; tests/test_gru.py holds the three statements together.  A C caller passes the numbers.
 *   MQE_ACTOR_RECURRENT = 16   MQE_ROLLOUT_HIDDEN_IN = 2   MQE_ROLLOUT_HIDDEN_RECORD = 4
 * MQE_ACTOR_RECURRENT is a bit of the KIND BYTE of mqe_actor_shape.activation and combines freely with the kinds, the two norm bits and the
 *   value-normalisation bit; bits 8 and 512 stay refused.  It applies to both networks; each needs at least 2 Linear layers (-6 naming
 *   actor_layers / critic_layers otherwise).  With H the width of a network's last hidden layer, a cell H -> H sits between that layer's output
 *   (behind its hidden norm, when there is one) and the output Linear; under the hidden norm a LayerNorm(H, eps = 1e-5) follows the cell.  The cell
 *   is torch.nn.GRU's, gate order r, z, n, all f32 (rounding points: csrc/kernels_gru.hpp, restated by tests/gru_ref.py):
 *     gi = W_ih x + b_ih;  gh = W_hh h + b_hh;  r = sigmoid(gi_r + gh_r);  z = sigmoid(gi_z + gh_z);  n = tanh(gi_n + r gh_n);  h' = (1 - z) n + z h
 * Parameter buffer, per network, in front of the output layer's weight: gru.weight_ih (3H, H), gru.weight_hh (3H, H), gru.bias_ih (3H),
 *   gru.bias_hh (3H) and, under the hidden norm, gru.norm.weight (H) -- created as 1 -- and gru.norm.bias (H).  With the bit clear the layout is
 *   the one it was, bit for bit.  n_params, mqe_ppo_optimizer and mqe_ppo_adam cover the cell like any weight.
 * State: [R'][Hs] floats owned by the engine, Hs = Ha + Hc (the cells' widths; Hc = 0 without a critic), row r = the actor's Ha floats, then the
 *   critic's; made zeroed by mqe_actor_create, released with the actor, NOT part of mqe_state_save (a learner checkpoints the recorded state).
 *   The TAIL of a packed row is the R' Hs floats at offset P4 = the MQE_T_WRAPPER_PACKED length rounded up to a multiple of 4.
 * mqe_rollout on a recurrent handle: step t is evaluated from h_in(t) = state * (1 - done) with done the byte of the row's env in packed row t
 *   (row 0's are zeroed: step 0 never masks; all agents of an env reset together; a masked state is exactly 0.0f); afterwards the live state, and row
 *   t + 1's tail when recorded, hold h'(t) UNMASKED -- the mask is in that row's own done bytes: OpenRL's (rnn_states[t], masks[t]).  The launch
 *   behind the last step is always enqueued: it masks the live state with row T's done bytes, writes value[T] from the masked critic state when
 *   value_dev is given, and advances nothing; a following call continues from it.  The critic's state advances whether or not value_dev is given.
 *   MQE_ROLLOUT_HIDDEN_IN      the start state is read from row 0's tail (written by the caller) instead of the live state
 *   MQE_ROLLOUT_HIDDEN_RECORD  the tails of rows 0 .. T are written, row 0's with the state the call started from; no other float beyond the packed layout
 *   With either flag row_stride >= P4 + R' Hs (still a multiple of 4), -6 naming row_stride otherwise; either flag on a handle without the bit: -6
 *   naming flags.  Without the flags tails are neither read nor written and the rule for row_stride is the old one.  Refusals enqueue nothing.
 * Resets that happen in mqe_step calls between rollouts are not seen by the state: it is masked by the done bytes of trajectory rows only.
 * mqe_gae, mqe_ppo_optimizer, mqe_ppo_adam and mqe_rollout_time_outs work unchanged.  mqe_ppo_grad on a recurrent handle is back-propagation through time
 *   over CHUNKS of a trajectory recorded with MQE_ROLLOUT_HIDDEN_RECORD (csrc/kernels_bptt.hpp: k_bptt_grad, k_bptt_ln_grad, k_bptt_expand; OpenRL /
 *   MAPPO's recurrent generator at data_chunk_length = L).  Three more constants, stated here, defined in csrc/kernels_bptt.hpp, mirrored in
 *   mqe/engine/abi.py (tests/test_bptt.py holds the three statements together); a C caller passes the numbers:
 *     MQE_PPO_BPTT = 32   MQE_PPO_CHUNK_SHIFT = 8   MQE_PPO_MAX_CHUNK = 64
 *   flags = MQE_PPO_BPTT | L << MQE_PPO_CHUNK_SHIFT (bits 8 .. 15 hold L, 1 <= L <= MQE_PPO_MAX_CHUNK), or-ed with the other mqe_ppo_grad flags.  T must
 *   be a multiple of L.  The trajectory is (T / L) R' chunks, chunk c = (t0 / L) R' + r covering steps t0 .. t0 + L - 1 of row r; index_dev / first /
 *   count then mean CHUNKS (index values are clamped into [0, (T / L) R')), the minibatch is count L samples and the loss's 1 / M is 1 / (count L); the
 *   loss, its kinks and the six statistics are those stated at mqe_ppo_grad, over those samples.  Step 0 of a chunk starts both cells from the tail of
 *   packed row t0 masked by that row's done byte of the row's env (data: no gradient reaches it); step j > 0 starts from the h' computed at step j - 1
 *   with the CURRENT parameters, masked by packed row t0 + j's done byte: the rule of mqe_rollout above.  The gradient of step j's input state is
 *   carried to step j - 1 times that mask; the one step 0 produces is dropped.  The same bits on every run.  Under MQE_PPO_VALUE_NORM[_UPDATE] the
 *   minibatch's returns are those of its count L samples.  -6, naming the argument, nothing enqueued or written: the bit or any of bits 8 .. 15 on a
 *   handle without MQE_ACTOR_RECURRENT (flags); L = 0 or L > 64 (flags); T not a multiple of L (T); row_stride < P4 + R' Hs (row_stride); first + count
 *   beyond the chunks when there is no index.  A recurrent handle called WITHOUT the bit stays refused (-6, nothing enqueued or written): its gradient
 *   is back-propagation through time, which has to be asked for with the chunk length.
 *   Scratch, made by the first such call, grown when L grows (that call synchronises once, as the other first calls do), released with the actor: the
 *   workgroups' input states, 256 workgroups x L x max(Ha, Hc) x the row tile (64 or 32 chunks) floats -- 64 steps x 128 units x 64 rows x 4 B x 256 =
 *   537 MB at the largest, 42 MB in the usual case L = 10, H = 64 -- and, under value normalisation, the count L sample numbers of the minibatch.
 *   The first call refuses (-5, naming the cell's width) a shape whose LDS need (csrc/kernels_bptt.hpp: k_ln_grad's rows + 7 per unit of the wider
 *   cell) does not fit 160 KiB at 32 chunks a workgroup; every shape with all widths <= 64 and obs_dim <= 128 fits, with and without the norms.
 * mqe_actor_create refuses (-6, naming the width) a recurrent shape whose LDS need, (2 max layer input + 4 + Ha + Hc, + 32 with a norm) rows of 260
 *   bytes, exceeds the 160 KiB of a workgroup; every shape with all widths and obs_dim <= 128 fits.  A handle created without the bit launches
 *   exactly the kernels it launched before. */

/* ---- Multi-agent transformer policy in the rollout: MAT's encoder and decoder evaluated by the engine (csrc/kernels_mat.hpp: k_actor_mat) ----
 * v17, additive: no export, no prototype, no struct and no #define of this header changes.  OpenRL's `--algo mat` (cfgs/mat.yaml; MATNet) at the
 * defaults the file leaves untouched: n_block = 1, n_head = 1, n_embd = E = 64, dec_actor = False, continuous actions.  THE CONSTANT BELOW IS NOT
 * #DEFINED BY THIS HEADER (tests/test_rollout.py pins the exact set of MQE_ACTOR_* defines).  Its value is stated here, defined under this name in
 * csrc/kernels_mat.hpp (which the engine compiles) and mirrored in mqe/engine/abi.py; tests/test_mat.py holds the three statements together.  A C
 * caller passes the number.  The bit was refused as unknown before.
 *   MQE_ACTOR_TRANSFORMER = 32
 * A bit of the KIND BYTE of mqe_actor_shape.activation.  With it actor_layers = critic_layers = 2, actor_dims = {D, E, 3}, critic_dims = {D, E, 1}
 *   with the same E: the "actor" is MAT's decoder, the "critic" the value head its encoder always carries (there is no such handle without one).
 *   MQE_ACTOR_TANH is the only accepted kind (GELU is implied); MQE_ACTOR_VALUE_NORM combines with it (mat.yaml: use_valuenorm).
 * The network, with LN = LayerNorm(eps = 1e-5, weight and bias), GELU the exact erf form, every Linear with a bias, A' the agents of an env:
 *     Attn(key, value, query; masked): k = Wk key + bk, v = Wv value + bv, q = Wq query + bq;  s_ij = (q_i . k_j) / sqrt(E), masked: only j <= i;
 *                                      p = softmax_j(s);  y_i = sum_j p_ij v_j;  out = Wp y + bp
 *     Encoder  x = LN_E(GELU(Linear_{D->E}(LN_D(obs))));  x = LN_E(x + Attn(x, x, x; unmasked));  rep = LN_E(x + Linear(GELU(Linear(x))))
 *              value_a = Linear_{E->1}(LN_E(GELU(Linear_{E->E}(rep_a))))
 *     Decoder  s_0 = 0, s_a = the action of agent a - 1 as sampled (raw: before action_gain, unclipped);  x = LN_E(GELU(Linear_{3->E}(s)))
 *              x = LN_E(x + Attn(x, x, x; masked));  x = LN_E(rep + Attn(key = x, value = x, query = rep; masked));  x = LN_E(x + Linear(GELU(Linear(x))))
 *              mean_a = Linear_{E->3}(LN_E(GELU(Linear_{E->E}(x_a))))
 *     Head     sigma_j = 0.5 sigmoid(log_std_j) (MAT's, not exp(log_std));  a = mean + sigma z;  logp = sum_j (-0.5 z_j^2 - ln sigma_j) - 1.5 ln(2 pi)
 *   Acting is autoregressive inside one launch: agent a's mean is conditioned on the sampled actions of agents 0 .. a - 1; its bits are those of one
 *   parallel decoder pass over the final s (csrc/kernels_mat.hpp, EVALUATION ORDER), which is what a learner evaluates.  z is the draw of the plain
 *   actor, keyed (seed, global env id, MQE_RNG_ACTOR + n, agent * 3 + j): shards and checkpoints continue as they do there.  MQE_ROLLOUT_DETERMINISTIC: z = 0.
 * Parameter buffer: every Linear weight (out, in) row-major then bias, every norm weight -- created as 1 -- then bias, in the order the operators run:
 *   the encoder (obs_norm, obs_fc, ln, attn.key / .query / .value / .proj, ln1, mlp0, mlp1, ln2, head0, head_ln), the decoder (act_fc, ln, attn1.*, ln1,
 *   attn2.*, ln2, mlp0, mlp1, ln3, head0, head_ln), then value_out (E -> 1), mean_out (E -> 3), log_std[3] and the value-normalisation state:
 *   2 D + D E + 18 E^2 + 45 E + 7 trainable floats.  mqe_ppo_optimizer and mqe_ppo_adam cover them like any weight.
 * mqe_rollout, mqe_gae, mqe_rollout_time_outs, mqe_ppo_optimizer and mqe_ppo_adam work unchanged on such a handle; there is no carried state.
 *   mqe_ppo_grad WITHOUT the bit below refuses such a handle (-6, nothing enqueued or written: "the gradient through the attention is not in the engine
 *   yet"), as it did before that gradient existed: it is asked for explicitly, like MQE_PPO_BPTT on a recurrent handle.
 * THE GRADIENT (csrc/kernels_mat_grad.hpp: k_mat_grad, k_mat_reduce; the loss is stated there once).  The constant is not #defined by this header either
 *   (tests/test_ppo.py pins the MQE_PPO_* define set); it is defined in csrc/kernels_mat_grad.hpp and mirrored in mqe/engine/abi.py (tests/test_mat_grad.py):
 *   MQE_PPO_TRANSFORMER = 65536
 *   Bit 16 of mqe_ppo_grad's flags, the first above the chunk-length byte.  With it the minibatch's unit is the env-step GROUP g = t N + n, standing for the
 *   samples g A' + a -- MQE_PPO_JOINT's unit and numbering, because the attention needs all A' agents of an env-step: index_dev / first / count are group
 *   numbers in [0, T N) (index values are clamped), M = count A'.  The loss is mqe_ppo_grad's with the Head above: mean and value from one parallel pass over
 *   the group (s_a = the recorded action of agent a - 1: data), dlogp/dmean_j = z_j / sigma_j, dlogp/dlog_std_j = (z_j^2 - 1)(1 - sigmoid(log_std_j)), H = sum_j
 *   ln sigma_j + 1.5 (1 + ln(2 pi)), log_std_j receiving -entropy_coef (1 - sigmoid(log_std_j)).  With MQE_PPO_JOINT the ratio is the group's and the policy term
 *   is divided by G = count; without it the ratio is per sample and every mean is over M.  MQE_PPO_DUAL_CLIP, MQE_PPO_CLIP_VALUE and MQE_PPO_VALUE_NORM[_UPDATE]
 *   combine as elsewhere.  Every element of grad_dev is written; no floating-point atomics: the same bits on every run.
 *   -6, nothing enqueued or written: the bit on a handle without MQE_ACTOR_TRANSFORMER (flags); the bit with MQE_PPO_BPTT or a chunk length (flags);
 *   first + count beyond the T N groups without an index (first / count).
 *   The first flagged call of an actor allocates (and synchronises once; released with the actor) 256 tapes of the activations the backward needs,
 *   256 x (2 obs_dim + 40 E + 20) rows x 64 floats (E = 64, obs_dim = 128: 186 MB), and refuses with -5, naming E, a shape whose working set,
 *   (max(obs_dim, E) + 2 + max(6 E, E + obs_dim) + E + 41) rows of 260 bytes + 528 bytes, exceeds the 160 KiB of a workgroup: E = 64 fits for every
 *   obs_dim <= 128; at obs_dim = 16 every E <= 72 fits, so E = 76 .. 92, which mqe_actor_create accepts, can act and be updated through the torch twin only.
 * -6 naming the field: the bit with MQE_ACTOR_LAYER_NORM, MQE_ACTOR_FEATURE_NORM or MQE_ACTOR_RECURRENT (activation); the relu kind (activation);
 *   actor_layers / critic_layers other than 2; critic_dims[1] != actor_dims[1] (critic_dims); E < 4 or E % 4 != 0 (actor_dims); an E whose LDS need,
 *   obs_dim + 6 E + 43 rows of 260 bytes, exceeds the 160 KiB of a workgroup (actor_dims; E = 64 fits for every obs_dim <= 128); an A' that does not
 *   divide the 64 rows of a tile (A').  A handle created without the bit launches exactly the kernels it launched before.
 * Not built: n_block > 1, n_head > 1, dec_actor, discrete actions. */

/* ---- Joint-ratio and dual-clip policy losses in mqe_ppo_grad (csrc/kernels_ppo.hpp: the loss head of the four gradient kernels, k_joint_expand) ----
 * v17, additive: no export, no prototype and no #define of this header changes; mqe_ppo_loss_ex above is the one new typedef.  OpenRL's
 * use_joint_action_loss (jrpo.yaml) and dual_clip_ppo / dual_clip_coeff (dppo.yaml).  THE TWO CONSTANTS BELOW ARE NOT #DEFINED BY THIS HEADER
 * (tests/test_ppo.py pins the exact set of MQE_PPO_* defines).  Their values are stated here, defined under these names in csrc/kernels_ppo.hpp (which
 * the engine compiles) and mirrored in mqe/engine/abi.py; tests/test_joint_loss.py holds the three statements together.  A C caller passes the
 * numbers.  Both bits were refused as unknown before.
 *   MQE_PPO_JOINT = 64   MQE_PPO_DUAL_CLIP = 128
 * MQE_PPO_JOINT: one importance ratio and one advantage per ENV-STEP instead of one per agent.  With R' = N A' rows a step and sample
 *   s = t R' + n A' + a, a GROUP is the A' samples of one env-step: g = t N + n, samples g A' + a.  index_dev / first / count are GROUP numbers in
 *   [0, T N) (index values are clamped into that range); with MQE_PPO_BPTT they are chunk groups (t0 / L) N + n in [0, (T / L) N), each standing for
 *   the A' chunks of that env.  Per sample d_a = logp_a - logp_old_a (f32, as above); per group, pairwise in the order of the xor butterfly:
 *     Delta = d_0 (A' = 1), d_0 + d_1 (A' = 2), (d_0 + d_1) + (d_2 + d_3) (A' = 4), ...;   rho = expf(Delta)
 *     A = (adv_0 + ...) * (float)(1.0 / A'), added in the same order;   L_pi(g) = -min(rho A, clamp(rho, 1 - c, 1 + c) A)
 *   The policy term of L is the mean of L_pi(g) over the G = count (count L under MQE_PPO_BPTT) groups, 1 / G = (float)(1.0 / G); the value term stays the
 *   mean over the M = G A' samples, the entropy term is unchanged.  For every agent a of the group dL/dlogp_a = -A rho (1 / G), and 0 when
 *   (A > 0 and rho > 1 + c) or (A < 0 and rho < 1 - c): every agent of a group sees the same bits of Delta, rho and A, so the group decides a kink once.
 *   stats_dev[0] is the mean of L_pi over groups, [4] the mean of -Delta over groups, [5] the share of groups with |rho - 1| > c; [1 .. 3] as before.
 *   At A' = 1 the call has the bits of the call without the flag.  Under MQE_PPO_VALUE_NORM[_UPDATE] the returns are those of the groups' samples.
 *   One more small launch (k_joint_expand: the groups' flat sample or chunk numbers into engine-owned scratch, made by the first such call and grown with
 *   count; that call synchronises once).  -6 naming A' on a handle whose A' does not divide 32 (the agents of a group share the lanes of one wavefront).
 * MQE_PPO_DUAL_CLIP: `loss` points at an mqe_ppo_loss_ex; without the bit nothing beyond the first 16 bytes is read.  With c_d = dual_clip > 1 + c,
 *   where the advantage is negative  L_pi = -max(min(rho A, clamp(rho) A), c_d A),  and dL/dlogp is additionally 0 when A < 0 and rho > c_d (for
 *   c_d > 1 + c value for value OpenRL's ratio = min(ratio, c_d) form).  Without MQE_PPO_JOINT rho = ratio and A = adv of the single sample.
 *   -6 naming dual_clip: not finite, or <= 1 + clip_ratio; -6 naming reserved: a reserved word whose bits are not zero.
 * Both combine with each other and with every other mqe_ppo_grad flag; every refusal enqueues and writes nothing. */

/* The onboard forward depth camera of LeggedRobotField (legged_robot_field.py:23-93: create_camera_sensor + attach_camera_to_body on the
 * base link, :196-223: get_camera_image_gpu_tensor(IMAGE_DEPTH)) for every robot, from the CURRENT state: out_dev [R][height][width]
 * device floats, Isaac Gym's IMAGE_DEPTH convention -- the NEGATIVE distance along the optical axis to the first surface, -inf where
 * nothing lies within far_m.  cam_pos3 / cam_rpy3 (host pointers) = cfg.sensor.forward_camera.position / .rotation (ZYX Euler) in the base
 * link; the camera looks along its +x, +z up; pixel (0, 0) is the top-left corner.  What is seen is what the physics collides with: the
 * ground (slab or relief), the wall prisms, the OTHER robots' collision primitives, free NPCs, the 1-dof link, the scenery boxes -- a ray
 * caster (csrc/kernels_camera.hpp), not the reference's rasteriser, which is closed: the image is SPECIFIED by the scalar caster of the CPU
 * oracle (oracle/mqe_oracle.c: mqo_render_depth -- conventions, surfaces, marching rules), which passes geometric known answers on its own
 * (tests/test_camera_oracle.py); the kernel is held to it per pixel on 8 scenes (tests/test_camera_gpu.py: <= 0.2 % of the pixels -- silhouettes -- may differ in hit / miss or depth, the rest agree to 1e-4 m + 1e-5 relative).  Colour images (IMAGE_COLOR) are not offered. */
int mqe_render_depth(mqe_sim* s, float* out_dev, int height, int width, float horizontal_fov_deg, const float* cam_pos3, const float* cam_rpy3,
                     float far_m, void* stream);

/* Episode recording: one image of ONE env from a free camera (upstream's FloatingCameraSensor on env 0, mqe/utils/helpers.py:276-298:
 * create_camera_sensor, set_camera_location(pos, lookat), get_camera_image(IMAGE_COLOR); state machine legged_robot.py:916-957).  Isaac Gym's
 * rasteriser is closed, so pixels cannot be matched: like the depth camera this is a ray caster over the collision geometry
 * (csrc/kernels_view.hpp, k_view), and this comment is its specification.
 *   camera    mqe_render_depth's conventions: the camera looks along its +x, +y is its left, +z up; pixel (0, 0) is top-left;
 *             yc = -(2 (j + 0.5) / W - 1) tan(hfov / 2), zc = -(2 (i + 0.5) / H - 1) tan(hfov / 2) H / W; the ray d = f + yc l + zc u is
 *             NOT normalised, so its parameter t is the depth along the optical axis.  The basis comes from (eye, lookat), world points
 *             (env frames coincide with the world, legged_robot.py:834-835), built on the host in double: f = normalize(lookat - eye),
 *             l = normalize(z_world x f), u = f x l; when f is within 1e-6 of vertical, l = (0, 1, 0).
 *   surfaces  what mqe_render_depth sees, by its rules -- the slab or the relief marched in half cells and bisected six times, the wall
 *             march over the SDF (wall_top / wall_height, 400 steps at most), free NPCs as spheres or the box, the 1-dof link scene's base
 *             and link (the cylinder as a capsule), the scenery boxes -- and EVERY robot of the env: no own-robot exclusion.  A hit needs
 *             t > 1e-4; an eye inside a shape sees nothing of it.
 *   normal    of the nearest surface at the hit point, world frame, turned to face the eye (n . d <= 0).  Sphere: (p - c) / r.  Capsule: p
 *             minus the closest point of its segment, normalised.  Box: the axis of the face the entry slab belongs to.  Slab: (0, 0, 1).
 *             Relief: normalize(-gx, -gy, 1), (gx, gy) the gradient of the bilinear sample at the hit point.  Wall: (0, 0, 1) when the hit
 *             lies within 1 mm of the wall's top, else the normalised horizontal gradient of the bilinear SDF sample ((1, 0, 0) where
 *             that gradient vanishes).
 *   id        int32 word: bits 0-7 class (MQE_VIEW_*: 0 nothing, 1 ground, 2 wall, 3 robot, 4 free NPC, 5 1-dof scene, 6 scenery box);
 *             bits 8-15 robot / NPC / box index; bits 16-23 part: the robot's primitive index (mqe_robot_model::prim_*), for class 5
 *             0 = base, 1 = link; bit 24, ground only: parity of floor(x) + floor(y) of the hit point, a 1 m checker that makes motion
 *             over flat ground visible.
 *   colour    a pure function of (id word, normal): channel c = (uint8)(255 min(1, albedo_c (MQE_VIEW_AMBIENT + MQE_VIEW_DIFFUSE
 *             max(0, n . L))) + 0.5), L = MQE_VIEW_LIGHT (unit); albedo = the class's row of MQE_VIEW_PALETTE (robot r: row 2 + r % 4),
 *             the ground's times 1 + MQE_VIEW_CHECKER where bit 24 is set and 1 - MQE_VIEW_CHECKER where it is not; a miss gets
 *             MQE_VIEW_SKY.  Alpha is always 255.
 *   outputs   device pointers, each written only if non-null.  rgba_dev: uint8 [H][W][4], Isaac Gym's IMAGE_COLOR layout after upstream's
 *             reshape (helpers.py:296-298); 4-byte aligned (one store per pixel).  geom_dev: float [H][W][4] = the axial depth in
 *             IMAGE_DEPTH's convention (negative; the bit pattern of -inf on a miss, as mqe_render_depth writes it), then the normal (zero
 *             on a miss); 16-byte aligned (one store per pixel).  id_dev: int32 [H][W].
 * Renders from the CURRENT state with one launch on `stream`: allocates nothing, does not synchronise, reads state only.  eye3 / lookat3
 * are host pointers.  Refused with a negative code and a message, without a launch: null handle (-1); all three outputs null, null eye3
 * / lookat3 (-1); env outside [0, num_envs), height or width <= 0, height * width > MQE_VIEW_MAX_PIXELS, fov outside (1, 179), far_m <= 0,
 * |lookat - eye| < 1e-6, a misaligned output (-6); inside an open step (-8).
 * Mapping and cost (profiles/view_render.txt): 16 x 16-pixel tiles, one 256-thread workgroup each, a wavefront = an 8 x 8 block. */
#define MQE_VIEW_MAX_PIXELS (1 << 20)
#define MQE_VIEW_NONE 0
#define MQE_VIEW_GROUND 1
#define MQE_VIEW_WALL 2
#define MQE_VIEW_ROBOT 3
#define MQE_VIEW_NPC 4
#define MQE_VIEW_LINK_SCENE 5
#define MQE_VIEW_SCENERY 6
#define MQE_VIEW_ID(cls, index, part) ((cls) | ((index) << 8) | ((part) << 16))
#define MQE_VIEW_CHECKER_BIT (1 << 24)
#define MQE_VIEW_AMBIENT 0.35f
#define MQE_VIEW_DIFFUSE 0.65f
#define MQE_VIEW_CHECKER 0.08f
#define MQE_VIEW_LIGHT {0.36f, 0.48f, 0.80f}
#define MQE_VIEW_SKY {135, 190, 235}
#define MQE_VIEW_PALETTE_ROWS 9          /* ground, wall, robots 0-3, free NPC, 1-dof scene, scenery box */
#define MQE_VIEW_PALETTE {{0.55f, 0.58f, 0.50f}, {0.72f, 0.68f, 0.60f}, {0.85f, 0.25f, 0.20f}, {0.20f, 0.40f, 0.85f}, {0.95f, 0.75f, 0.15f}, \
                          {0.25f, 0.70f, 0.35f}, {0.92f, 0.90f, 0.82f}, {0.60f, 0.42f, 0.25f}, {0.50f, 0.50f, 0.58f}}
int mqe_render_view(mqe_sim* s, int env, uint8_t* rgba_dev, float* geom_dev, int32_t* id_dev, int height, int width,
                    float horizontal_fov_deg, const float* eye3, const float* lookat3, float far_m, void* stream);

/* gym.refresh_rigid_body_state_tensor (legged_robot_field.py:117-119): MQE_T_RIGID_BODY_STATE from the CURRENT root and dof state.
 * Enqueued on `stream`. */
int mqe_refresh_rigid_body_state(mqe_sim* s, void* stream);
/* on != 0: every post-physics step refreshes MQE_T_RIGID_BODY_STATE first -- after the last substep, before termination, the NPC script
 * and the resets (an env reset in that step shows its terminal pose, as upstream) -- in mqe_step, mqe_step_end, mqe_step_command,
 * mqe_step_joint, mqe_post_physics_step and mqe_post_physics_stage calls that include MQE_POST_FRAME.  A fused step then runs its
 * post-physics step as a launch of its own instead of the physics kernel's epilogue (the same arithmetic).  0 (the default): no step
 * launches it.  mqe_reset_all and mqe_state_load never refresh it.  Host-side switch; not inside an open step. */
int mqe_set_rigid_body_refresh(mqe_sim* s, int on);

/* legged_gym's measured_heights (legged_robot.py:1047-1061 _init_height_points, :1094-1097 _reward_base_height, go1.py:235-236): the height of
 * the static surface under a yaw-aligned grid of points around every robot's base.  UNPINNED: upstream's own _get_heights is absent from the
 * reference snapshot and its call site is commented out, so no reference program fixes the numbers; the meaning is the published legged_gym
 * one, on the surface THIS engine's physics collides with.  Specification (tests/height_ref.py restates it in float64; csrc/kernels_terrain_scan.hpp):
 *   grid      points_xy [n_points][2] base-frame offsets; for cfg.terrain.measured_points_x / _y point i * len(y) + j = (x[i], y[j]) (x-major,
 *             torch.meshgrid flattened); 1 <= n_points <= MQE_MAX_HEIGHT_POINTS.
 *   point     world (x, y) of robot r, point p = root_xy + Rz (px, py); Rz = upstream's quat_apply_yaw (mqe/utils/math.py:38-42), the rotation
 *             of the normalised quaternion (0, 0, qz, qw) of the base: cos = (qw^2 - qz^2) / (qz^2 + qw^2), sin = 2 qw qz / (qz^2 + qw^2) -- the
 *             twist about z, not the Euler yaw of a tilted body; identity when qz^2 + qw^2 < 1e-18.
 *   height    H(x, y) = world z of the static surface, by the conventions of the physics' terrain test: fx = clamp(x / hs, 0, nx - 1) (as
 *             fmin(fmax(v, 0), limit): a NaN lands on 0), ix = min((int)fx, nx - 2), tx = fx - ix, y likewise; g = ground_z + the bilinear sample
 *             of ground_height (scenes with a relief); s = the bilinear sample of wall_sdf; s <= 0 (inside a wall footprint): H = max(g, top),
 *             top = wall_top[tx < 0.5 ? ix : ix + 1][ty < 0.5 ? iy : iy + 1] or wall_height without that map, a world z as the physics
 *             compares it; otherwise H = g.
 *   flags     MQE_HSCAN_SCENERY: each static scenery box (MQE_NPC_STATIC scenes: bridge, wrestling ring; world-aligned, centred at the NPC
 *             root + static_box_center) whose footprint |x - cx| <= hx, |y - cy| <= hy holds the point raises H to max(H, cz + hz).  Off (the
 *             default, upstream's meaning): terrain only.  Robots, free NPCs and the 1-dof link are never seen.
 *   output    out_dev [R][n_points] device floats (R = num_envs * num_agents; caller-owned, 4-byte alignment suffices), ABSOLUTE world heights:
 *             what _reward_base_height subtracts from root_states[:, 2].
 * mqe_measure_heights: from the CURRENT root state, one launch on `stream`.  points_xy is a HOST pointer; the handle keeps device copies of
 * the grid it was last given (one for this call, one for the registered scan) and uploads only when the grid changes (that upload
 * synchronises the device).  Cost on one MI355X (profiles/height_scan.txt): k_height_scan 7.9 us at 4096 envs x 2 x 187 points, 17.8 us at
 * 16384; registered, a go1gate 4096 x 2 step takes 0.1943 -> 0.2041 ms (+5.0 %, most of it the given-up epilogue, as with the rigid-body
 * refresh); nothing registered: the parent's launches and step time (0.1940 vs 0.1939 ms, inside the box-to-box spread). */
int mqe_measure_heights(mqe_sim* s, float* out_dev, const float* points_xy, int n_points, int flags, void* stream);
/* registers (out_dev != NULL) or drops (out_dev == NULL; the other arguments are then ignored) the scan that every post-physics step
 * refreshes first -- after the last substep, before termination, the NPC script and the resets (an env reset in that step shows the
 * heights under its terminal pose), where mqe_set_rigid_body_refresh's launch sits and in the same calls.  While a scan is registered a
 * fused step runs its post-physics step as a launch of its own instead of the physics kernel's epilogue (the same arithmetic).  Nothing is
 * registered by default: no step launches it.  out_dev must stay valid until the scan is dropped or the handle destroyed.  mqe_reset_all and
 * mqe_state_load never refresh it; derived data, not part of mqe_state_save's blob.  Host-side switch; not inside an open step. */
int mqe_set_height_refresh(mqe_sim* s, float* out_dev, const float* points_xy, int n_points, int flags);

/* After host writes into MQE_T_HISTORY (obs_history of the reference, go1.py:102,145): rebuilds what the engine derives from the ring --
 * the compact split-f16 operand of layer 0, the presence flags (a frame of 70 zeros is absent), the carrier columns, the continuity
 * bits.  A no-op for handles whose layer 0 reads the ring itself.  Enqueued on `stream`. */
int mqe_history_sync(mqe_sim* s, void* stream);

/* debug taps (tests): M^-1 (18 x 18) of one robot and the contact list of one env ([<= 64][8]: actor A, link A, actor B (-1 static),
 * link B, separation, normal xyz) from the CURRENT state, without advancing it; outputs are host pointers */
int mqe_debug_dynamics(mqe_sim* s, int env, int robot, float* minv_out_host, int* nc_out_host, float* contacts_out_host);
int mqe_debug_times(long long* out16);   /* clock64 stamps of the phases of the last mqe_debug_dynamics launch */
/* per-phase counter runs (tools/phase_counters.py): the following mqe_simulate launches leave the wavefront after phase tap `tap`
 * and write nothing back (tap < 0: normal launches again; tap >= 100: the same specialised kernel run to the end, state written).  Two-robot scenes without objects only; any other scene is refused.
 * The environment variable MQE_DEBUG_STOP_PHASE sets the same thing when the handle is created. */
int mqe_debug_stop_phase(mqe_sim* s, int tap);
/* handles created with MQE_WAVE_TIMES=1 in the environment: wall-clock stamps (100 MHz) of every wavefront of the last fused
 * decimation launch at entry and exit + its HW_ID and XCC_ID registers, [num wavefronts][4] (tools/dev/wave_times.py: the spread
 * of the wavefronts' run times and where the dispatcher put them) */
int mqe_debug_wave_times(mqe_sim* s, long long* out_host);
/* handles created with MQE_TAIL_TIMES=1 (fused policy tail): wall-clock stamps (100 MHz) of every workgroup of the last k_policy_tail launch at
 * its entry [0], after each of its eight barriers [1 .. 8] and at its end [9], [row blocks of 32 robots][16] (tools/dev/tail_times.py); slots
 * [10 .. 15] of the same rows carry the split-f16 layer-0 kernel's (k_gemm_h2) stamps of the same step, workgroup by workgroup: the wall clock at
 * entry / end of the K loop / exit, then the shader clock (s_memtime) at the same three points */
int mqe_debug_tail_times(mqe_sim* s, long long* out_host);
/* handles created with MQE_PHASE_TIMES=1 (two robots without objects, two robots + a flock, three robots + ball): the fused decimation launch runs with its phase taps
 * live; [num_envs][4 substeps][16] wall-clock stamps (100 MHz) of the last launch: taps 0..14 of the substep (kernels_physics.hpp
 * TSTAMP), [15] = its end (tools/dev/phase_walltimes.py: where the time of a full launch goes, phase by phase) */
int mqe_debug_phase_times(mqe_sim* s, long long* out_host);
/* the same handles (scenes whose post-physics step is the decimation kernel's epilogue): [num_envs][16] stamps of the epilogue of the last launch --
 * [0] after the actuator history's write-back, [1] actions staged, [2] loads + frame quantities, [3] flag / frame stores, [4] NPC rows staged,
 * [5] NPC script, [6] reset, [7] observation rows staged, [8] task wrapper (one lane per env), [9] rows flushed, [10] end
 * (tools/dev/epilogue_taps.py, round 6: the wrapper's serialised load -> store chains were half of the epilogue) */
int mqe_debug_epilogue_times(mqe_sim* s, long long* out_host);

/* Checkpoint / resume of the simulation state (the reference has none: SURVEY 5).  The blob holds every state buffer of the handle --
 * the tensors of mqe_sim_tensor and the internal ones (the compact history operand and its ring position, the action-lag ring, wrapper
 * bookkeeping, the reset counters that key the RNG streams, the domain parameters) -- and NOT the scene: load it into a handle created
 * from the same descriptor (same shape and layer-0 path; checked).  A rollout continued after mqe_state_load is bit for bit the
 * rollout that was not interrupted.  Both calls synchronise `stream`; `host_blob` is host memory of mqe_state_size() bytes. */
long long mqe_state_size(mqe_sim* s);
int mqe_state_save(mqe_sim* s, void* host_blob, void* stream);
int mqe_state_load(mqe_sim* s, const void* host_blob, void* stream);

/* bookkeeping for benchmarks: time of every kernel class measured with HIP events on `stream`; `on` = N > 0 brackets the launches of one step in every N
 * (the third step of each period: the first one after a synchronisation starts on an idle GPU), 0 switches it off */
int mqe_profile_enable(mqe_sim* s, int on);
int mqe_profile_read(mqe_sim* s, float* ms_per_kernel, int n, int* n_launches);

#ifdef __cplusplus
}
#endif
#endif
