/*
 * tds_hip.h — C ABI of libtds_hip.so, the MI355X-native many-instance stepper.
 *
 * This is the drop-in boundary for ONE path of tiny-differentiable-simulator (TDS):
 * the per-environment simulation step
 *     PD -> forward_dynamics (ABA) -> integrate_euler_qdd -> World::step -> integrate_euler
 * (reference: examples/environments/locomotion_contact_simulation.h:151-304) replayed over
 * N independent environments.  Everything in this header is plain C: pointers, sizes,
 * ints.  No torch / STL types cross it.
 *
 * Two layers are exported:
 *
 *  (1) The handle API  tds_hip_*  — resident device state, explicit stream, status codes.
 *      It replaces  VectorizedEnvironment::CustomForwardDynamicsStepper::step
 *      (reference: examples/ars/ars_vectorized_environment.h:75-85) without the
 *      host<->device copy per step that the reference CUDA stepper performs
 *      (reference: examples/ars/ars_train_policy_cuda.cpp:246-308).
 *
 *  (2) The legacy  <model>_forward_zero{,_meta,_allocate,_deallocate}  symbols, exactly as the
 *      reference's generated CUDA libraries export them and as CudaModel<double> dlopen()s
 *      them (reference: examples/ars/ars_train_policy_cuda.cpp:220-229, 345-359; emitter
 *      src/utils/cuda_codegen.hpp:146-262).  They live in the thin shim libraries
 *      cuda_model_ant.so / cuda_model_laikago.so (csrc/legacy_shim.cpp) and forward to (1).
 *
 * The model description (tds_model_t) is a POD "flattened MultiBody + World": it is what
 * include/tds_hip_stepper.hpp::flatten_model() produces from an intact tds::MultiBody /
 * tds::World built by TDS's own URDF loader, so that every loader quirk is inherited.
 */
#ifndef TDS_HIP_H
#define TDS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TDS_HIP_ABI_VERSION 5

#define TDS_MAX_LINKS 64   /* links of the model as the reference builds it; the kernels take <= 32 lanes: one per
                              moving link (fixed links are folded into their parents when lanes run short), six for
                              a floating base, three per spherical joint */
#define TDS_MAX_GEOMS 32
#define TDS_MAX_VISUALS 64
#define TDS_MAX_ACTIONS 32
#define TDS_MAX_DOF 32
/* contact points per environment: sphere 1, capsule 2, box 8 (contact_point.hpp:96-198) */
#define TDS_MAX_CONTACTS 64
/* articulated bodies of one world (World::multi_bodies_ without the plane; src/world.hpp:206-282 pairs them all) */
#define TDS_MAX_BODIES 4
/* contact points between the geometries of the articulated bodies of a world, summed over all body pairs
   (sphere-sphere 1, capsule-sphere 2: contact_point.hpp:43-94, 405-438), per environment */
#define TDS_MAX_PAIR_CONTACTS 160

/* status codes returned by every tds_hip_* function */
enum {
  TDS_OK = 0,
  TDS_ERR_INVALID_ARG = 1,
  TDS_ERR_UNSUPPORTED = 2, /* model uses a feature the HIP path does not implement */
  TDS_ERR_HIP = 3,         /* a HIP runtime call failed; see tds_hip_last_error() */
  TDS_ERR_NO_DEVICE = 4
};

/* joint types — numeric values identical to tds::JointType (src/link.hpp:9-21) */
enum {
  TDS_JOINT_FIXED = -1,
  TDS_JOINT_PRISMATIC_X = 0,
  TDS_JOINT_PRISMATIC_Y = 1,
  TDS_JOINT_PRISMATIC_Z = 2,
  TDS_JOINT_PRISMATIC_AXIS = 3,
  TDS_JOINT_REVOLUTE_X = 4,
  TDS_JOINT_REVOLUTE_Y = 5,
  TDS_JOINT_REVOLUTE_Z = 6,
  TDS_JOINT_REVOLUTE_AXIS = 7,
  TDS_JOINT_SPHERICAL = 8
};

/* geometry types — numeric values identical to tds::GeometryTypes (src/geometry.hpp:30-38) */
enum {
  TDS_GEOM_SPHERE = 0,
  TDS_GEOM_PLANE = 1,
  TDS_GEOM_CAPSULE = 2,
  TDS_GEOM_MESH = 3,
  TDS_GEOM_BOX = 4
};

/* which call sequence one "step" replays */
enum {
  /* PD -> ABA -> integrate_euler_qdd -> contacts + MLCP/PGS -> integrate_euler -> pack
     (locomotion_contact_simulation.h:151-304).  x = [q | qd | action | kp kd max_force] */
  TDS_STEP_LOCOMOTION = 0,
  /* joint torques given directly, no PD:              x = [q | qd | tau]
       has_plane == 0:  ABA -> clear_forces -> integrate_euler   (cartpole_environment.h:88-94)
       has_plane == 1:  ABA -> clear_forces -> integrate_euler_qdd -> World::step -> integrate_euler
                        (examples/soft_contact_example.cpp:107-115)                     */
  TDS_STEP_TAU = 1
};

/* reward / termination rule written into the observation record (tds_hip_step_obs) */
enum {
  TDS_REWARD_NONE = 0,
  /* reward = (x_t - x_{t-1})/dt, done = z < 0.26 (reward 0 when done)
     (examples/environments/ant_environment2.h:75-106) */
  TDS_REWARD_ANT = 1,
  /* reward = x, done = up_dot_world_z < 0.6 || z < 0.2, up from rpy = q[3..5]
     (examples/environments/laikago_environment2.h:130-171) */
  TDS_REWARD_LAIKAGO = 2,
  /* reward = x, done = up_dot_world_z < 0.6 || z < 0.8, up from the quaternion q[3..6] of the spherical root joint
     (examples/environments/humanoid_environment.h:155-197, fixed-base branch) */
  TDS_REWARD_HUMANOID = 3
};

/* scalar types: what the kernels compute in / what the records in HBM (x, y, actions, obs, policy) are stored in.
   F64        double / double — the reference's arithmetic; parity-gated at 1e-6 (measured <= 4e-11 per step)
   F32        float / float   — pure single precision; measured, NOT gated: the mass-matrix factorisation loses the
                                1e-6 contract in float (8e-6 without contacts, 1e-3 with), as does the reference's own
                                TinyAlgebra<float> instantiation (tests/test_f32.py)
   F64_REC32  double / float  — the reference's FLOAT record ABI (BASELINE config 2; half the bytes per env-step) with
                                the arithmetic kept in double registers: parity-gated at 1e-6 on float inputs */
enum { TDS_DTYPE_F64 = 0, TDS_DTYPE_F32 = 1, TDS_DTYPE_F64_REC32 = 2 };

/* All 3x3 matrices are row-major: m[3*r+c].  Transforms are TDS "right-associative":
   X.rot maps child-frame vectors into the parent frame, X.trans is the child origin in the
   parent frame (src/math/transform.hpp:123-137). */
typedef struct tds_link {
  int32_t joint_type; /* TDS_JOINT_* */
  int32_t parent;     /* parent link index, -1 = base */
  int32_t q_index;    /* index into q,  -2 for fixed joints (multi_body.hpp:324-349); a spherical joint owns 4 */
  int32_t qd_index;   /* index into qd, -2 for fixed joints; a spherical joint owns 3 */
  double X_T_rot[9];  /* parent link -> joint frame (link.hpp:39) */
  double X_T_trans[3];
  double S[6];        /* motion subspace [angular | linear], NOT normalised (link.hpp:125-193) */
  double mass;        /* RigidBodyInertia (src/math/inertia.hpp:9-37) */
  double com[3];
  double inertia[9];
  double stiffness;   /* link.hpp:88-89 (always 0 from the URDF loader) */
  double damping;
} tds_link_t;

typedef struct tds_geom {
  int32_t link; /* owning link (index into tds_model_t::links, i.e. global over all bodies of a multi-body world);
                   -1 - b = base of body b (-1 for a single body) */
  int32_t type; /* TDS_GEOM_SPHERE / CAPSULE / BOX */
  double radius;
  double length;     /* capsule */
  double extents[3]; /* box full extents */
  double X_rot[9];   /* X_collision: geometry frame in link frame (link.hpp:75) */
  double X_trans[3];
} tds_geom_t;

typedef struct tds_visual {
  int32_t link; /* owning link (>= 0; base visuals are not packed by the reference) */
  int32_t pad_;
  double X_rot[9]; /* X_visual (link.hpp:78-79) */
  double X_trans[3];
} tds_visual_t;

/* body b >= 1 of a world with several articulated bodies (tds_model_t::bodies) */
typedef struct tds_body {
  int32_t first_link;  /* index of the body's first link in tds_model_t::links */
  int32_t first_geom;  /* index of the body's first geometry in tds_model_t::geoms */
  int32_t is_floating; /* multi_body.hpp:66-78 */
  int32_t pad_;
  double base_X_world_rot[9];
  double base_X_world_trans[3];
  double base_mass; /* mb.base_rbi(), used only when is_floating */
  double base_com[3];
  double base_inertia[9];
} tds_body_t;

typedef struct tds_model {
  int32_t abi_version; /* TDS_HIP_ABI_VERSION */
  int32_t step_mode;   /* TDS_STEP_* */
  int32_t num_links;
  int32_t dof_q;       /* mb.dof()    */
  int32_t dof_qd;      /* mb.dof_qd() */
  int32_t is_floating; /* 1: floating base — q = [quat xyzw | pos | joints] (dof_q = 7 + n), qd = [omega | v | joints]
                          (multi_body.hpp:324-349, kinematics.hpp:35-62) */
  int32_t num_geoms;
  int32_t num_visuals;
  int32_t action_dim;    /* LOCOMOTION: #PD targets; TAU: dof_qd */
  int32_t pd_start_link; /* first link the PD loop visits (base_dof_=6, locomotion_contact_simulation.h:180) */
  int32_t has_plane;     /* 1: multi_bodies_[0] is the implicit plane (plane first!) */
  int32_t pgs_iterations;
  int32_t input_dim;  /* doubles per env in the reference record x */
  int32_t output_dim; /* doubles per env in the reference record y */
  int32_t pack_visuals; /* 1: y carries 7 doubles per visual + up_dot_z */
  int32_t reward_mode;  /* TDS_REWARD_*: which env's compute_reward_done the obs record mirrors */
  double dt;
  double gravity[3];
  double base_X_world_rot[9];
  double base_X_world_trans[3];
  double plane_normal[3]; /* unit */
  double plane_constant;
  double cfm;         /* mb_constraint_solver.hpp:64-67 */
  double erp;
  double friction;    /* World::default_friction   (world.hpp:68) */
  double restitution; /* World::default_restitution (world.hpp:69) */
  double action_limit; /* 0.4 (locomotion_contact_simulation.h:234) */
  double initial_poses[TDS_MAX_ACTIONS];
  /* environment reset (examples/environments/ant_environment2.h:109-165,
     laikago_environment2.h:63-116): q = reset_q + reset_noise * U(-1,1) per coordinate, qd = 0,
     followed by settle_steps steps with zero action.  The reference draws U from std::rand();
     the device uses a counter-based generator keyed by (seed, env, reset count, coordinate). */
  double reset_q[TDS_MAX_DOF];
  double reset_noise[TDS_MAX_DOF];
  int32_t settle_steps;
  /* 1: the observation tds_hip_reset hands out keeps the raw base x, y — what LaikagoContactSimulation::reset and
     HumanoidContactSimulation::reset return (laikago_environment2.h:63-116); 0: obs[0] = obs[1] = 0 as
     AntContactSimulation2::reset does (ant_environment2.h:162-163).  The STEP's observation always zeroes them
     (ars_vectorized_environment.h:283-288).  (Occupies the former padding slot: layout unchanged.) */
  int32_t reset_obs_raw_xy;
  /* rigid-body inertia of the base link, mb.base_rbi() (multi_body.hpp:78); used only when is_floating */
  double base_mass;
  double base_com[3];
  double base_inertia[9];
  /* Worlds with SEVERAL articulated bodies (World::step over multi_bodies_ = [plane,] body 0, 1, ...:
     src/world.hpp:206-282, 293-366).  num_bodies = B in 2..TDS_MAX_BODIES: body 0 is described by the fields above
     (base frame, is_floating, base inertia) and owns links [0, bodies[1].first_link) and geoms [0, bodies[1].first_geom);
     body b >= 1 is bodies[b] and owns links / geoms from its first_link / first_geom up to those of body b + 1 (or the
     end).  A link's parent is -1 (its own body's base) or a link of the same body; q / qd indices are dense over all
     bodies: q = [q_0 | q_1 | ...], qd = [qd_0 | qd_1 | ...] (a floating body's share is [quat xyzw | pos | joints] /
     [omega | v | joints]), in TAU mode x = [q | qd | tau_0 | tau_1 | ...] with dof_actuated entries per body; a geometry
     on the base of body b has link = -1 - b; geoms in the reference's order (base first, then link by link).  Each body is
     stepped by its own forward dynamics; contacts: every body against the plane (if any), then every pair of bodies
     i < j in the reference's order — sphere-sphere and capsule-sphere in either order, as the reference's dispatcher
     knows them — solved pair by pair (plane-0, plane-1, ..., 0-1, 0-2, ..., 1-2, ...) with both Jacobian blocks and both
     inverse mass matrices (mb_constraint_solver.hpp:191-498).  num_bodies 0 / 1: one body.  1-dof joints; step_mode TAU. */
  int32_t num_bodies;
  int32_t pad3_[3];
  tds_body_t bodies[TDS_MAX_BODIES]; /* entries 1 .. num_bodies - 1 (entry 0 is not read) */
  tds_link_t links[TDS_MAX_LINKS];
  tds_geom_t geoms[TDS_MAX_GEOMS];
  tds_visual_t visuals[TDS_MAX_VISUALS];
  char name[32];
} tds_model_t;

typedef struct tds_hip_sim tds_hip_sim_t; /* opaque */

/* Human-readable text of the last failure on the calling thread ("" if none). */
const char *tds_hip_last_error(void);

/* Library/ABI introspection. */
int tds_hip_abi_version(void);
int tds_hip_device_count(void);

/* Validate a model against what the HIP path implements (joint/geometry coverage,
   sizes).  TDS_OK or TDS_ERR_UNSUPPORTED / TDS_ERR_INVALID_ARG. */
int tds_hip_model_check(const tds_model_t *model);

/* Create a simulation of num_envs independent copies of `model` on HIP device `device`.
   dtype = TDS_DTYPE_*.  Device buffers owned by the handle: x [N][input_dim], y [N][output_dim] (both in the
   record dtype).  Every entry point selects the handle's device for the duration of the call and restores the
   caller's current device: one process may hold handles on several GPUs. */
int tds_hip_create(const tds_model_t *model, int num_envs, int device, int dtype,
                   tds_hip_sim_t **out);
int tds_hip_destroy(tds_hip_sim_t *sim);

/* All launches / copies of this handle are enqueued on `hip_stream` (a hipStream_t;
   NULL = the default stream).  The library never synchronises unless documented. */
int tds_hip_set_stream(tds_hip_sim_t *sim, void *hip_stream);

int tds_hip_num_envs(const tds_hip_sim_t *sim);
int tds_hip_input_dim(const tds_hip_sim_t *sim);
int tds_hip_output_dim(const tds_hip_sim_t *sim);
int tds_hip_dtype(const tds_hip_sim_t *sim);
int tds_hip_device(const tds_hip_sim_t *sim);
int tds_hip_record_bytes(const tds_hip_sim_t *sim); /* bytes per scalar of the records: 8 (F64) or 4 */
/* wait for everything enqueued on the handle's stream */
int tds_hip_sync(tds_hip_sim_t *sim);

/* Device pointers of the resident records, for zero-copy consumers (e.g. a torch tensor
   wrapping them).  Layout: env-major [N][dim], compute dtype. */
void *tds_hip_x_device(tds_hip_sim_t *sim);
void *tds_hip_y_device(tds_hip_sim_t *sim);

/* Host <-> resident record transfers (double on the host side, converted to the compute
   dtype).  These synchronise the handle's stream. */
int tds_hip_set_inputs(tds_hip_sim_t *sim, const double *x_host /* [N*input_dim] */);
int tds_hip_get_inputs(tds_hip_sim_t *sim, double *x_host /* [N*input_dim] */);
int tds_hip_get_outputs(tds_hip_sim_t *sim, double *y_host /* [N*output_dim] */);

/* y = f(x) on caller-provided DEVICE buffers in the compute dtype (pure function, the
   reference's forward_zero semantics).  Asynchronous on the handle's stream. */
int tds_hip_forward_zero_device(tds_hip_sim_t *sim, const void *x_dev, void *y_dev);

/* One closed-loop environment step on the resident records, asynchronous:
     - if actions_dev != NULL, x[:, dof_q+dof_qd : +action_dim] <- actions_dev [N][action_dim]
     - y = f(x)
     - x[:, 0 : dof_q+dof_qd] <- y[:, 0 : dof_q+dof_qd]     (what VectorizedEnvironment::step
       does on the host, ars_vectorized_environment.h:240-289, minus reward/reset)
   Repeated `substeps` times with the same action. */
int tds_hip_step(tds_hip_sim_t *sim, const void *actions_dev, int substeps);

/* tds_hip_step plus the per-env observation record the vectorised env hands to the policy
   (ars_vectorized_environment.h:250-289), written by the same kernel launch:
     obs_dev [N][obs_dim + 2] = [ q | qd  with obs[0] = obs[1] = 0 | reward | done ]   (compute dtype)
   obs_dim = dof_q + dof_qd.  reward/done follow model->reward_mode for the LAST substep (what
   repeated VectorizedEnvironment::step calls would report).  This record is what a multi-GPU
   job all-gathers. */
int tds_hip_step_obs(tds_hip_sim_t *sim, const void *actions_dev, int substeps, void *obs_dev);
int tds_hip_obs_dim(const tds_hip_sim_t *sim);

/* The same step for a caller whose actions and observations are HOST arrays of doubles — the signature the reference's
   VectorizedEnvironment::step works on (ars_vectorized_environment.h:213-291) — with the STATE resident on the device:
   per call only actions_host [N][action_dim] travel up and obs_host [N][obs_dim + 2] = [obs | reward | done]
   (and y_host [N][output_dim] = sim_states_with_graphics_, optional) travel down, through pinned staging memory owned
   by the handle.  Blocking.  With tds_hip_set_auto_reset on, done environments are reset inside the call.
   tds_hip_reset_host: tds_hip_reset with a host mask ([N] bytes, NULL = all) and the observations back on the host.
   tds_hip_set_states: overwrite [q | qd] of every environment from qqd_host [N][dof_q + dof_qd] (actions and the PD
   variables of the x records stay) — how a caller that resets with the REFERENCE's own reset() hands the states over.
   Used by tds_hip::VectorizedEnv (include/tds_hip_stepper.hpp). */
int tds_hip_step_host(tds_hip_sim_t *sim, const double *actions_host, int substeps, double *obs_host, double *y_host);
int tds_hip_reset_host(tds_hip_sim_t *sim, const unsigned char *mask_host, double *obs_host);
int tds_hip_set_states(tds_hip_sim_t *sim, const double *qqd_host);
/* Device memory on the handle's device for callers without HIP headers (action pools, record rings, policies handed to
   tds_hip_step_many_rings / tds_hip_rollout): alloc zero-fills; upload / download block on the handle's stream. */
int tds_hip_device_alloc(tds_hip_sim_t *sim, size_t bytes, void **out);
int tds_hip_device_free(tds_hip_sim_t *sim, void *ptr);
int tds_hip_device_upload(tds_hip_sim_t *sim, void *dst_dev, const void *src_host, size_t bytes);
int tds_hip_device_download(tds_hip_sim_t *sim, void *dst_host, const void *src_dev, size_t bytes);

/* n_steps closed-loop steps (tds_hip_step_obs with substeps = 1) per host call, replayed from a
   captured hipGraph: ONE graph launch instead of n_steps kernel launches, which removes the host-side launch gaps
   that cost a double-digit share of short runs at ~20 us per step.
     actions_dev  [action_blocks][N][action_dim] (record dtype) or NULL; step k uses block (first_block + k) % action_blocks
     obs_dev      optional [N][obs_dim + 2], overwritten by every step (holds the last step's record afterwards)
   The graph is cached on the handle (keyed by all arguments); _prepare builds it without running anything, so that a
   timed region holds the launch only.  n_steps <= 4096.

   Environment chains.  The environments are independent and the call holds n_steps steps of each, so the batch need
   not move in lockstep: the library splits it into C contiguous environment ranges ("chains"), captures one linear
   graph per chain and replays them concurrently on C streams forked from / joined to the handle's stream.  While one
   chain sits at a kernel boundary (launch latency, workgroup dispatch ramp, the wait for its slowest workgroup: ~3 us
   of a 20 us Ant x 4096 step) the other chains' workgroups have the compute units to themselves.  Records are bit
   for bit those of whole-batch launches.  C: tds_hip_set_graph_chains (0 = library default: 2 for models with
   contact points, 1 otherwise; environment TDS_HIP_GRAPH_CHAINS overrides), or measured on the spot by
   tds_hip_step_many_tune, which runs probe_steps steps (advancing the simulation) once untimed and once timed for
   C = 1, 2, 3, keeps the fastest and returns it in *chains. */
int tds_hip_step_many_prepare(tds_hip_sim_t *sim, const void *actions_dev, int action_blocks, int first_block,
                              int n_steps, void *obs_dev);
int tds_hip_step_many(tds_hip_sim_t *sim, const void *actions_dev, int action_blocks, int first_block, int n_steps,
                      void *obs_dev);
int tds_hip_set_graph_chains(tds_hip_sim_t *sim, int chains);

/* Run-time options.  Every switch of the library — kernel forms, launch forms, reset-pool geometry, exchange forms — is a
   named integer option (table: csrc/tds_options.h; tds_hip_option_count / _name enumerate it).  When a handle is
   CREATED each option takes, in this order: the value of tds_hip_default_option in this process, the environment
   variable TDS_HIP_<KEY> (upper case), or "unset" = the library's own rule.  The handle keeps that snapshot; afterwards
   only tds_hip_set_option changes it — the environment is never read while a handle is in use and nothing is latched
   per process, so one process can hold handles with different forms (how the tests select kernel builds).
   Create-time options (lanes_per_env, na_cap, w2, gram, no_chain, no_rootjoint, no_kinchain, no_eulerroot, no_legscan,
   fold_fixed) shape the device model / LDS layout: tds_hip_set_option refuses them, set them with
   tds_hip_default_option before tds_hip_create.  Setting an option that cached graphs or the reset pool depend on
   drops those (they are rebuilt by the next call).  The options of a shard are those of its sim handle
   (tds_hip_shard_sim).  Unknown key: TDS_ERR_INVALID_ARG. */
int tds_hip_default_option(const char *key, long long value);
int tds_hip_set_option(tds_hip_sim_t *sim, const char *key, long long value);
/* *is_set (optional) = 0: the option is unset (library rule), *value = 0 */
int tds_hip_get_option(const tds_hip_sim_t *sim, const char *key, long long *value, int *is_set);
int tds_hip_option_count(void);
const char *tds_hip_option_name(int index);
/* 1 if tds_hip_step_many(sim, ..., n_steps, ...) runs as ONE launch of the step-loop kernel instead of graphs: worlds
   without contact points (pendulums, the cartpole), fixed-base kernels up to 16 dof with contacts (the Ant) while
   the batch is at most three rounds of workgroups; the star-shaped legged robots of tds_hip_single_step_kernel take their
   own kernels' step-loop forms: the 16-lane kernel (Laikago) while every workgroup of the launch is resident at once —
   computed from the device's compute-unit count and LDS size, hipDeviceProp_t: in one-wavefront workgroups up to 6144
   environments on an MI355X, in workgroups of eight wavefronts around one constant table (a workgroup per compute unit:
   option quad_wide, default on) up to 8192 — and the chained graphs of its straight-line form beyond; the 8-lane kernel (the Ant) always — beyond one round of resident
   two-wavefront workgroups (8192 environments) as environment ranges of that size one after the other, each a launch of all the
   call's steps (the environments are independent; single steps and the exchange's launches stay whole).  No kernel boundaries; the state stays in
   LDS (in the compute scalar) for the n_steps steps, every step takes its own action block, y / obs / x are written
   once at the end — what the graph form leaves behind too, whose obs_dev is overwritten by every step.  With float
   records the state is rounded to float once per call instead of once per step.
   (TDS_HIP_STEP_MANY_LOOP=0 / 1 forbids / forces the form).

   With tds_hip_set_auto_reset on, every one of the n_steps steps resets the environments it ends with done
   (ars_vectorized_environment.h:262-277), through the reset pool: where _is_loop holds (then for the Ant at every
   batch size: the alternative is single steps, not graphs), as step-loop launches of up to
   128 steps in which a done environment copies its next pre-settled state from its ring into LDS and carries on, the
   rings being topped up between the launches on a side stream; elsewhere as n_steps single steps.  Same stream of
   random numbers and same records as n_steps calls of tds_hip_step_obs. */
int tds_hip_step_many_is_loop(const tds_hip_sim_t *sim, int n_steps);

/* tds_hip_step_many with PER-STEP RECORDS: every one of the n_steps steps produces what one call of the reference's
   VectorizedEnvironment::step produces (ars_vectorized_environment.h:240-289 on top of step_forward_original's output
   packing, locomotion_contact_simulation.h:273-303) — the [obs | reward | done] record and, if asked for, the whole y
   record (q, qd, visual poses, up.z, padding) — and stores it into the step's slot of a caller-owned ring in HBM:
     obs_ring  [obs_slots][N][obs_dim + 2]   step k of the call -> slot (obs_first + k) % obs_slots
     y_ring    [y_slots][N][y_stride]        step k of the call -> slot (y_first + k) % y_slots        (either may be NULL)
   in the record dtype; obs_f32 != 0: the obs ring holds FLOATS whatever the record dtype (the wire format of the
   multi-GPU exchange).  Where tds_hip_step_many_is_loop holds the n_steps steps are ONE launch of the step-loop kernel
   that packs and stores the records of every step (write-back stores; the state itself never leaves LDS between the
   steps); elsewhere they are the chained graphs of single-step launches with each launch pointed at its slots.  With
   auto-reset on, a step that ends with done leaves reward / done of the terminal step and the observation of the fresh
   environment in its slot, as the reference does.  Afterwards the handle's y record holds the last step's (a device
   copy of its slot).  This is the form bench.py times: all of step_forward_original's work, every step.
     progress  optional, step-loop form only, not with auto-reset (those calls are cut into several launches): an array
               of obs_slots device counters, one per slot of the obs ring.  Every workgroup adds 1 to the counter of
               step k's slot once its OBS-RING record of that step is visible device-wide (signalled while step k + 1
               runs; not for the last step of the call: stream order covers it): the slot's counter has grown by
               tds_hip_step_many_rings_blocks exactly when EVERY workgroup has stored that step — what
               tds_hip_shard_step_many polls to exchange slot k while the launch carries on (a single running total
               would be reached by the average workgroup while the slowest is steps behind).  It covers the obs ring
               only: the y ring is written with ordinary stores that become visible to other agents at the end of the
               launch (nothing exchanges y records; read them behind the launch in stream order).
               tds_hip_step_many_rings_blocks = increments of a slot's counter per use of the slot.
     y_stride  scalars between consecutive y records of the y ring (0: output_dim, i.e. packed).  A stride that is a
               multiple of the 128-byte line (Ant, f64: 160 instead of 155) lets every record start on a line boundary:
               the ring launch then writes whole lines only (measured: HBM write traffic per step down to the payload).
     obs_slot_envs  see the field.
   A slot is overwritten `slots` steps later: the ring's depth is the lag the consumer may have. */
typedef struct tds_hip_rings {
  void *obs_ring;
  int32_t obs_slots, obs_first, obs_f32, y_stride;
  void *y_ring;
  int32_t y_slots, y_first;
  unsigned long long *progress;
  int32_t obs_slot_envs; /* environments per SLOT of the obs ring (0: the handle's own N).  Larger than N: a slot laid out
                            for the environments of all ranks of a multi-GPU run — obs_ring then points at this rank's
                            block of slot 0, and the launch stores its records straight into the receive buffer of an
                            in-place all-gather (no copy of the local block on any rank) */
  int32_t pad1_;
} tds_hip_rings_t;
int tds_hip_step_many_rings(tds_hip_sim_t *sim, const void *actions_dev, int action_blocks, int first_block, int n_steps,
                            const tds_hip_rings_t *rings);
/* builds the graphs of the next tds_hip_step_many_rings with the same arguments (graph form; a no-op for the loop form) */
int tds_hip_step_many_rings_prepare(tds_hip_sim_t *sim, const void *actions_dev, int action_blocks, int first_block,
                                    int n_steps, const tds_hip_rings_t *rings);
int tds_hip_step_many_rings_blocks(const tds_hip_sim_t *sim);
int tds_hip_step_many_tune(tds_hip_sim_t *sim, const void *actions_dev, int action_blocks, int probe_steps,
                           void *obs_dev, int *chains);

/* On-device environment reset — replaces the host loop of VectorizedEnvironment::reset / the
   auto-reset branch of VectorizedEnvironment::step (ars_vectorized_environment.h:196-211, 262-277).
   tds_hip_reset: re-initialise the environments selected by mask_dev (uint8 [N], NULL = all) from
     the model's reset distribution, run model->settle_steps zero-action steps, write the new state
     into the resident x record and, if obs_dev != NULL, the observation part of their obs record
     (reward / done slots are left untouched).  One kernel launch, asynchronous.
   tds_hip_set_auto_reset(enable): tds_hip_step / tds_hip_step_obs then reset every environment whose
     step ends with done (model->reward_mode) inside the same launch: y, reward and done describe
     the terminal step, x and the observation describe the freshly reset + settled environment —
     exactly what the reference's auto_reset_when_done does.
   seed selects the random stream (counter-based: deterministic for a given seed, environment
   index and per-environment reset count, independent of launch geometry). */
int tds_hip_set_auto_reset(tds_hip_sim_t *sim, int enable, unsigned long long seed);
int tds_hip_reset(tds_hip_sim_t *sim, const unsigned char *mask_dev, void *obs_dev);

/* Policy rollout entirely on device: n_steps times { action = W obs + b with the
   environment's OWN parameters; step; reward / done; return bookkeeping } in ONE launch, on the
   resident records.  It is Worker::rollouts + VectorizedEnvironment::policy/step of the reference
   (examples/ars/ars_vectorized_worker.h:51-140, ars_vectorized_environment.h:213-300) for the linear
   policy those build (one linear layer obs_dim -> action_dim with bias, identity activation):
     policy_dev        [num_envs][action_dim*obs_dim + action_dim] in the compute dtype, NeuralNetwork
                       parameter order: weights row-major (row = action), then biases
                       (src/math/neural_network.hpp:406-415); obs_dim = dof_q + dof_qd
     obs               [q | qd] with obs[0] = obs[1] = 0 (ars_vectorized_environment.h:283-288);
                       flags bit 0: the FIRST step sees the raw base x, y, as it does right after
                       VectorizedEnvironment::reset (:196-211)
     return_sum_dev    [num_envs] compute dtype: sum of (reward - shift) over the steps taken while the
                       environment was not done; return_steps_dev [num_envs] int: their number
                       (total_rewards / vec_steps of Worker::rollouts); either may be NULL
     obs_dev           optional [num_envs][obs_dim + 2]: final observation | last reward | done
     flags             bit 0: see obs.  The rollout runs as ONE launch of the step-loop kernel; bit 1 forces one
                       launch of the straight-line step kernel per step with a small policy + bookkeeping kernel in
                       between (same results to round-off; slower at every batch size measured; no auto-reset).
   With tds_hip_set_auto_reset a done environment is re-initialised + settled and keeps collecting;
   without it, it stays done (the state keeps stepping, as under the reference's custom stepper). */
int tds_hip_rollout(tds_hip_sim_t *sim, const void *policy_dev, int n_steps, double shift, int flags,
                    void *return_sum_dev, int *return_steps_dev, void *obs_dev);

/* tds_hip_rollout plus the by-products Worker::rollouts produces alongside the returns
   (examples/ars/ars_vectorized_worker.h:88-135), each optional (NULL):
     stats_dev     [num_envs][obs_dim][3] record dtype, UPDATED in place (zero it for a fresh filter): RunningStat
                   (examples/ars/running_stat.h, Knuth's recurrence) of every observation component the policy was
                   evaluated on — (count, mean, S); variance = S / (count - 1).  Pushed every step, done or not.
     traj_dev      [num_envs][n_steps][output_dim] record dtype + traj_len_dev [num_envs] int: per environment the y
                   record (sim_states_with_graphics_) of every step taken while not done; a step that ends with done
                   repeats the previous entry if there is one — the trajectories vector of Worker::rollouts.
   Asking for either selects the per-step-launch form of the rollout (the bookkeeping kernel between the step
   launches produces them); auto-reset then goes through the reset pool. */
int tds_hip_rollout_ex(tds_hip_sim_t *sim, const void *policy_dev, int n_steps, double shift, int flags,
                       void *return_sum_dev, int *return_steps_dev, void *obs_dev, void *stats_dev, void *traj_dev,
                       int *traj_len_dev);

/* Policies with hidden layers (the reference's NeuralNetworkSpecification / NeuralNetwork::compute,
   src/math/neural_network.hpp:93-160, 223-300 — the vectorised ARS environment builds one linear layer and keeps its
   two ReLU layers commented out, examples/ars/ars_vectorized_environment.h:170-178).  num_layers entries, the input
   included: layer_sizes[0] = obs_dim = dof_q + dof_qd, layer_sizes[num_layers - 1] = action_dim, each
   <= TDS_NN_MAX_UNITS; activations[i - 1] (TDS_NN_ACT_*) is applied to layer i >= 1; use_bias[i] != 0 gives layer i a
   bias (use_bias[0]: a bias added to the observation, set_input_dim).  Afterwards the policy_dev argument of
   tds_hip_rollout(_ex) holds, per environment, tds_hip_policy_num_parameters() scalars in NeuralNetwork parameter order
   (set_parameters, :406-415): all weights layer by layer, each row-major [unit of layer i][unit of layer i - 1], then all
   biases layer by layer — and rollouts run as one straight-line step launch per step with the network evaluated by a
   kernel of its own in between (one wavefront per environment, activations in LDS).  num_layers = 0 restores the
   default (the linear policy inside the step-loop launch). */
enum {
  TDS_NN_ACT_IDENTITY = -1,
  TDS_NN_ACT_TANH = 0,
  TDS_NN_ACT_SIN = 1,
  TDS_NN_ACT_RELU = 2,
  TDS_NN_ACT_SOFT_RELU = 3,
  TDS_NN_ACT_ELU = 4,
  TDS_NN_ACT_SIGMOID = 5,
  TDS_NN_ACT_SOFTSIGN = 6
};
#define TDS_NN_MAX_LAYERS 8
#define TDS_NN_MAX_UNITS 256
int tds_hip_set_policy_network(tds_hip_sim_t *sim, int num_layers, const int *layer_sizes, const int *activations,
                               const int *use_bias);
int tds_hip_policy_num_parameters(const tds_hip_sim_t *sim);

/* Blocking convenience with HOST buffers in double, any N <= num_envs:
   H2D(x) -> kernel -> D2H(y), i.e. exactly what the reference's <model>_forward_zero does. */
int tds_hip_forward_zero_host(tds_hip_sim_t *sim, int n, const double *x_host, double *y_host);
/* The same call in two halves (F64 records only): _begin enqueues H2D -> kernel -> D2H on the handle's stream and
   returns, _end waits.  A host that drives several devices enqueues every device's share before it waits
   (include/tds_hip_stepper.hpp: HipStepper with a device list). */
int tds_hip_forward_zero_host_begin(tds_hip_sim_t *sim, int n, const double *x_host, double *y_host);
int tds_hip_forward_zero_host_end(tds_hip_sim_t *sim);

/* The same call split the way the reference's newer generated-library ABI splits it
   (src/utils/cuda/cuda_function.hpp:11-20, 78-99: <fn>_send_local, then <fn>):
   send_local uploads the first n input records; forward_zero_fetch runs the kernel on the
   first n resident records and downloads their outputs. Both block. */
int tds_hip_send_local(tds_hip_sim_t *sim, int n, const double *x_host);
int tds_hip_forward_zero_fetch(tds_hip_sim_t *sim, int n, double *y_host);

/* Step Jacobians (tiny-differentiable-simulator's CudaModel::sparse_jacobian, src/utils/cuda/cuda_model.hpp:14-25,
   cuda_codegen.hpp:303-426).  J = d y / d x of forward_zero per environment, x [input_dim] the reference record,
   y [output_dim], taken through the algorithm as executed: clamps, PGS projections, friction boxes and the activation
   of contacts follow the branch the primal takes; quaternion entries of x are differentiated raw (no projection onto
   the unit sphere).  Forward mode (dual numbers), a kernel of its own; f64 handles only.  In scope: one articulated
   body, fixed or floating base, 1-DoF and fixed joints, PD or torque actuation, plane contacts with spheres, capsules
   and boxes; spherical joints, worlds of several bodies and f32 / float-record handles give TDS_ERR_UNSUPPORTED with
   a tds_hip_last_error() message.  An environment whose joint-space inertia is not positive definite gets NaN
   outputs (device) or TDS_ERR_INVALID_ARG (host). */
enum { TDS_JAC_ACCUMULATE_NONE = 0, TDS_JAC_ACCUMULATE_SUM = 1, TDS_JAC_ACCUMULATE_MEAN = 2 }; /* CudaAccumulationMethod */
/* Directional derivatives: jv[n][k][output_dim] = J v for v [n][k][input_dim]; y [n][output_dim] (optional, may be
   NULL) = forward_zero's output.  All device pointers, n environments (any n >= 1, independent of num_envs).
   Enqueued on the handle's stream; the host waits for that stream only when the handle's work buffer has to grow.
   Work buffer: one work object per lane (the step's state in dual form: 54 KB (cartpole, pendulum5, cube_floating),
   76 KB (ant), 69 KB (laikago)) for min(n * ceil(k / K), 16384) lanes, K = tds_hip_jacobian_tangents; it is kept by
   the handle for the next call and freed with it. */
int tds_hip_jvp(tds_hip_sim_t *sim, int n, const void *x_dev, int k, const void *v_dev, void *y_dev, void *jv_dev);
/* Jacobian rows x columns (set_jac_output_sparsity / set_jac_local_input_sparsity): rows_host [n_rows] indices into y,
   cols_host [n_cols] into x, host arrays, NULL = dense (the count is then ignored).  accumulate NONE: jac_dev
   [n][n_rows][n_cols]; SUM / MEAN: [n_rows][n_cols] summed / averaged over the n environments in environment order.
   y_dev optional.  Enqueued on the handle's stream (work buffer as for tds_hip_jvp, with k = n_cols, plus
   n * n_rows * n_cols doubles for SUM / MEAN); the host waits for that stream first where a row or column selection
   is given (it is copied into the work buffer with a blocking copy) or the work buffer has to grow. */
int tds_hip_jacobian(tds_hip_sim_t *sim, int n, const void *x_dev, int n_rows, const int *rows_host, int n_cols,
                     const int *cols_host, int accumulate, void *y_dev, void *jac_dev);
/* The same template on the CPU (checker and CPU fallback; needs no GPU): host arrays, y (optional) from the double
   instantiation of the step, jac (optional) as tds_hip_jacobian lays it out. */
int tds_hip_jacobian_host(const tds_model_t *model, int n, const double *x, int n_rows, const int *rows, int n_cols,
                          const int *cols, int accumulate, double *y, double *jac);
/* Tangents one device lane carries for this model (the K of TdsDual<K>); 0 if the model is refused. */
int tds_hip_jacobian_tangents(const tds_model_t *model);

/* Step VJPs: reverse mode of the same derivative (the branch of the primal, quaternions raw), one tape per
   environment swept back once per cotangent.  wj[n][k][input_dim] = w^T J(x) for w [n][k][output_dim], per environment
   and cotangent; y [n][output_dim] (optional, may be NULL) = forward_zero's output.  Entries of w past the step's
   written outputs (q | qd | visuals | up . z) contribute nothing.  All device pointers, any n >= 1, f64 handles only;
   scope and refusals as for tds_hip_jacobian.  An environment whose joint-space inertia is not positive definite gets
   NaN outputs.  The tape of an environment holds at most a bound per model class (18 to 28 % above the longest tape
   counted for the class's models): an environment that would exceed it gets NaN outputs and the call returns
   TDS_ERR_UNSUPPORTED.  Enqueued on the handle's stream (a recording and a sweep kernel per 4096 environments); the call
   waits for them (it reads back the overflow flag).
   Work buffer (shared with tds_hip_jvp / tds_hip_jacobian, grown as needed and kept by the handle): for
   min(ceil(n / 64) * 64, 4096) lanes, the lane's work object plus 32 B per tape entry of the bound (10.9 GB for Ant
   x 4096). */
int tds_hip_vjp(tds_hip_sim_t *sim, int n, const void *x_dev, int k, const void *w_dev, void *y_dev, void *wj_dev);
/* The same on the CPU (host arrays, needs no GPU); a joint-space inertia that is not positive definite gives NaN
   outputs and TDS_ERR_INVALID_ARG, an overflowing tape NaN outputs and TDS_ERR_UNSUPPORTED. */
int tds_hip_vjp_host(const tds_model_t *model, int n, const double *x, int k, const double *w, double *y, double *wj);
/* tds_hip_vjp_host with the tape capacity tape_cap (<= 0: the class's bound, as tds_hip_vjp_host) and, where
   tape_len [n] is given, the number of entries each environment recorded (-1 where it overflowed). */
int tds_hip_vjp_host_tape(const tds_model_t *model, int n, const double *x, int k, const double *w, double *y,
                          double *wj, int tape_cap, int *tape_len);

/* Parameter derivatives: the step derivatives above taken in [x | theta], theta [n][p] f64 per environment, the model
   scalars a selection params[p] names, in that order (system identification: examples/pendulum_sys_id.cpp).  The step
   reads theta_i in place of the blob's values for environment i; every other scalar comes from the blob.  Derivative,
   scope, refusals and error handling as for tds_hip_jacobian / tds_hip_vjp.  A selection with an unknown kind, a link
   or comp out of range, a duplicate entry or a base kind on a fixed base gives TDS_ERR_INVALID_ARG.
   The contact model is selectable too (kinds 16..21; 12..15 are unknown kinds): the solver's cfm and erp, and per
   collision shape — `link` is then the GEOM index — its radius, a capsule's length, a box's extents and the translation
   of its frame X_trans.  A geom index or comp out of range, a length on anything but a capsule, an extent on anything
   but a box, a radius on a shape that is none of sphere, capsule, box: TDS_ERR_INVALID_ARG.  A geom of a model without a plane is selectable, its derivative is exactly zero.
   A box's contact points use rad = radius > 1e-2 ? radius : 1e-2, a branch of the primal: at or below 1e-2 the
   derivative along the radius is exactly zero.
   dt, the plane (normal, constant), the shapes' rotations, visuals and the rigid-body worlds (tds_rb_*: their radii
   and erp) are not selectable. */
enum {
  TDS_PARAM_LINK_MASS = 0,       /* links[link].mass */
  TDS_PARAM_LINK_COM = 1,        /* links[link].com[comp], comp 0..2 */
  TDS_PARAM_LINK_INERTIA = 2,    /* links[link].inertia, comp 0..5 = xx, yy, zz, xy, xz, yz (an off-diagonal comp sets
                                    both mirror entries) */
  TDS_PARAM_LINK_XT_TRANS = 3,   /* links[link].X_T_trans[comp], comp 0..2 */
  TDS_PARAM_LINK_STIFFNESS = 4,  /* links[link].stiffness */
  TDS_PARAM_LINK_DAMPING = 5,    /* links[link].damping */
  TDS_PARAM_BASE_MASS = 6,       /* base_mass (floating base only; link 0) */
  TDS_PARAM_BASE_COM = 7,        /* base_com[comp] (floating base only) */
  TDS_PARAM_BASE_INERTIA = 8,    /* base_inertia, comp as for links (floating base only) */
  TDS_PARAM_GRAVITY = 9,         /* gravity[comp] (link 0) */
  TDS_PARAM_FRICTION = 10,       /* friction (link 0, comp 0) */
  TDS_PARAM_RESTITUTION = 11,    /* restitution (link 0, comp 0) */
  /* 12..15: unknown kinds */
  TDS_PARAM_CFM = 16,            /* cfm (link 0, comp 0) */
  TDS_PARAM_ERP = 17,            /* erp (link 0, comp 0) */
  TDS_PARAM_GEOM_RADIUS = 18,    /* geoms[link].radius (sphere, capsule, box; link = geom index, here and below) */
  TDS_PARAM_GEOM_LENGTH = 19,    /* geoms[link].length (capsule only) */
  TDS_PARAM_GEOM_EXTENT = 20,    /* geoms[link].extents[comp], comp 0..2 (box only) */
  TDS_PARAM_GEOM_TRANS = 21      /* geoms[link].X_trans[comp], comp 0..2 */
};
typedef struct tds_param {
  int32_t kind, link, comp, pad_; /* TDS_PARAM_*; link 0 and comp 0 where the kind has none */
} tds_param_t;
/* theta [p] = the blob's values of the selection (host arrays); checks the selection. */
int tds_hip_params_get(const tds_model_t *model, int p, const tds_param_t *params, double *theta);
/* The inverse: *out_model = the blob with the selected scalars set to theta [p] (host arrays; out_model may be model
   itself).  Same checks and refusals as tds_hip_params_get; an off-diagonal inertia comp sets both mirror entries.
   This is the definition of "the model of variant v" below. */
int tds_hip_params_apply(const tds_model_t *model, int p, const tds_param_t *params, const double *theta,
                         tds_model_t *out_model);

/* Per-environment model variants: STEPPING a batch whose environments differ in the scalars a selection names (domain
   randomisation, sampling-based system identification).  Variant v is tds_hip_params_apply(the handle's blob, params,
   theta_host [v]) built into a device model of its own, so every derived quantity follows; environment e steps under
   variant env_variant_host [e] (int32 [num_envs]; NULL where n_variants == num_envs: the identity).  While variants are
   installed EVERY stepping path of the handle — forward_zero, step, step_many, the record rings, the rollout, forced
   resets through tds_hip_reset (re-initialised and settled under the environment's own variant) — runs the general step
   kernel's variant builds, one wavefront per workgroup (tds_hip_single_step_kernel and tds_hip_kernel_info report
   that); the 8-lane, 16-lane and serial-chain kernels decline.  n_variants == 0 clears: the handle is back on its own
   kernel and computes bit for bit what it computed before.  The derivative and query entry points (tds_hip_jvp*,
   tds_hip_vjp*, tds_hip_trajectory_*, tds_hip_policy_trajectory_*, tds_hip_dynamics, tds_hip_contacts, ...) take theta
   explicitly or read the handle's own blob: they IGNORE installed variants.
   Every variant must have the base model's STRUCTURE: outside the fields a selection can change (X_T, mass, centre of
   mass, inertia, joint springs, gravity, friction, restitution, cfm, erp, and the frames and radii of contact points —
   which is where a shape's radius, length, extents and X_trans go — and the frames of visuals) its
   device model equals the base's — a mass on a massless root link, for instance, changes how the root chain is
   treated; such a variant is TDS_ERR_INVALID_ARG, the message names the variant and the field.  A map entry outside
   [0, n_variants), n_variants > num_envs, n_variants != num_envs with a NULL map, or a bad selection:
   TDS_ERR_INVALID_ARG.  Models with spherical joints and worlds of several bodies: TDS_ERR_UNSUPPORTED with the
   parameter derivatives' message.  A handle with auto-reset on: TDS_ERR_UNSUPPORTED, as is tds_hip_set_auto_reset(1)
   while variants are installed (the reset pool's entries are settled under one model), the handle of a multi-GPU
   shard, phase stamps and option alt_build.  Memory: n_variants * sizeof(device model), 40.5 KB each in double
   arithmetic, 23.8 KB in float.  The call waits for the handle's stream, then replaces the arrays and drops every
   captured step_many graph and prepared launch. */
int tds_hip_set_model_variants(tds_hip_sim_t *sim, int n_variants, int p, const tds_param_t *params_host,
                               const double *theta_host /* [n_variants][p] */, const int32_t *env_variant_host);
/* variants installed on the handle (0: none) */
int tds_hip_model_variants(const tds_hip_sim_t *sim);
/* The checks of tds_hip_set_model_variants on the CPU, for a handle of num_envs environments of `dtype` (needs no GPU);
   *bytes (optional) receives the size of the device array of the variants' models. */
int tds_hip_model_variants_host(const tds_model_t *model, int dtype, int num_envs, int n_variants, int p,
                                const tds_param_t *params, const double *theta, const int32_t *env_variant,
                                int64_t *bytes);
/* Forward mode in [x | theta]: jv[n][k][output_dim] = J v for v [n][k][input_dim + p]; k = 0 computes y only (v, jv
   may then be NULL).  x_dev [n][input_dim], theta_dev [n][p], y_dev (optional) [n][output_dim]: device pointers;
   params_host: host array.  Enqueued on the handle's stream (the selection is copied into the work buffer with a
   blocking copy).  Work buffer as for tds_hip_jvp, each lane's work object holding the overlay of parameters. */
int tds_hip_jvp_params(tds_hip_sim_t *sim, int n, const void *x_dev, int p, const tds_param_t *params_host,
                       const void *theta_dev, int k, const void *v_dev, void *y_dev, void *jv_dev);
/* Reverse mode in [x | theta]: wj[n][k][input_dim + p] = w^T J for w [n][k][output_dim], the x part first.  As
   tds_hip_vjp (tape bound per class for parameter mode; the call waits for its kernels). */
int tds_hip_vjp_params(tds_hip_sim_t *sim, int n, const void *x_dev, int p, const tds_param_t *params_host,
                       const void *theta_dev, int k, const void *w_dev, void *y_dev, void *wj_dev);
/* The same templates on the CPU (host arrays, needs no GPU); jv / wj as above, y optional. */
int tds_hip_jvp_params_host(const tds_model_t *model, int n, const double *x, int p, const tds_param_t *params,
                            const double *theta, int k, const double *v, double *y, double *jv);
int tds_hip_vjp_params_host(const tds_model_t *model, int n, const double *x, int p, const tds_param_t *params,
                            const double *theta, int k, const double *w, double *y, double *wj, int tape_cap,
                            int *tape_len);

/* Forward-mode derivatives of articulated-body trajectories: forward_zero chained over `steps` steps (the derivatives'
   statement of the step, as tds_hip_jvp_params), the states s recorded after steps every, 2 every, .., steps, and
   js = (d s / d [x0 | theta]) v.  Step 0 reads x0 [n][input_dim] as forward_zero reads it; step t >= 1 reads
   [y_{t-1}'s q | qd | u[t-1] | x0's gains (LOCOMOTION: kp kd max_force)], u [n][steps - 1][n_act] with
   n_act = input_dim - dof_q - dof_qd - (3 for LOCOMOTION, else 0); u NULL holds x0's action slots every step.  The
   actions of u are inputs, not differentiated.  theta [n][p]: the scalars a selection params[p] names (kinds and checks
   as tds_hip_jvp_params), for the whole trajectory; NULL: the model's values.  s [n][n_rec][dof_q + dof_qd] with
   n_rec = steps / every, v [n][k][input_dim + p] (x0's columns, then theta's), js [n][k][n_rec][dof_q + dof_qd].
   k = 0 computes s only (the double step; v, js may then be NULL); with k > 0 s may be NULL.  The derivative is that of
   the algorithm as executed (the primal's branch at clamps, PGS projections, friction boxes and contact activation,
   quaternions raw).  An environment whose joint-space inertia is not positive definite at some step gets NaN for that
   record and every later one.  steps < 1, an `every` that does not divide steps or a bad selection gives
   TDS_ERR_INVALID_ARG; scope and refusals are those of tds_hip_jacobian, f64 handles only.  Any n >= 1, independent of
   num_envs; the handle's resident state is not touched.  Device pointers (params_host: host array); enqueued on the
   handle's stream as launches of at most option traj_steps steps each (the host waits only where the work buffer grows
   or the selection is copied).  Work buffer (shared with the step derivatives): min(n ceil(k / K), 16384) lane work
   objects plus (dof_q + dof_qd) (K + 1) + 1 doubles per (environment, block of K directions), K of
   tds_hip_jacobian_tangents (k = 0: K = 0). */
int tds_hip_trajectory_jvp(tds_hip_sim_t *sim, int n, int steps, int every, const void *x0_dev, const void *u_dev,
                           int p, const tds_param_t *params_host, const void *theta_dev, int k, const void *v_dev,
                           void *s_dev, void *js_dev);
/* The same per-step function on the CPU (host arrays, needs no GPU; s required): the checker of
   tds_hip_trajectory_jvp.  Returns TDS_ERR_INVALID_ARG where some environment's inertia was not positive definite,
   after writing every record. */
int tds_hip_trajectory_jvp_host(const tds_model_t *model, int n, int steps, int every, const double *x0,
                                const double *u, int p, const tds_param_t *params, const double *theta, int k,
                                const double *v, double *s, double *js);

/* Reverse-mode derivatives of the same trajectories: one cotangent gs [n][n_rec][dof_q + dof_qd] on the recorded states
   of tds_hip_trajectory_jvp's trajectory (step 0's record, step t's record, u, theta, every and n_rec, scope, refusals
   and the f64-only rule as there), and its gradients
     gx0 [n][input_dim] = sum_r gs_r^T d s_r / d x0, the linear map of js' x0 columns: x0's action slots feed step 0
                          only where u is given and every step where u is NULL, the LOCOMOTION gains every step;
     gu [n][steps - 1][n_act], in the actions of steps 1 .. steps - 1: required where u is given and n_act > 0,
                          ignored where u is NULL;
     gtheta [n][p], where p > 0;
   s [n][n_rec][dof_q + dof_qd] (optional, may be NULL) is bit for bit the k = 0 result of tds_hip_trajectory_jvp.  A
   slot that several steps feed is accumulated with t descending, on host and device alike.  Derivative conventions as
   above (the primal's branch, quaternions raw).  Per environment: a joint-space inertia that is not positive definite at
   some step gives NaN in s from that record on and NaN in all of the environment's gradients; a tape past the class's
   bound of parameter mode (tds_hip_vjp_params) gives NaN in all of its gradients and the call returns
   TDS_ERR_UNSUPPORTED.  Argument errors as tds_hip_trajectory_jvp.
   Device pointers (params_host: host array).  A primal pass stores the state after every step (n steps (dof_q + dof_qd)
   doubles of the work buffer); then, per chunk of environments and window of W consecutive steps, last window first,
   one launch records the W steps' tapes side by side and one launch sweeps them back in turn.  Option traj_vjp_lanes
   (a multiple of 64 in [64, 16384]; unset: 4096) is the lanes of a recording launch: chunk = min(ceil(n / 64) 64,
   traj_vjp_lanes) environments, W = max(1, min(traj_vjp_lanes / chunk, traj_steps, steps)); the results do not depend
   on either.  Enqueued back to back on the handle's stream (the host waits where the work buffer grows and the
   selection is copied); the call then waits for its kernels (it reads back the overflow flag).  Work buffer (shared
   with the step derivatives): the state store, and per lane of a recording launch the parameter-mode lane's work
   object plus 24 B per tape entry of the bound, plus 8 B per entry and environment of a chunk (11.5 GB for the Ant at
   the unset 4096 lanes, 46 GB at 16384). */
int tds_hip_trajectory_vjp(tds_hip_sim_t *sim, int n, int steps, int every, const void *x0_dev, const void *u_dev,
                           int p, const tds_param_t *params_host, const void *theta_dev, const void *gs_dev,
                           void *s_dev, void *gx0_dev, void *gu_dev, void *gtheta_dev);
/* The same on the CPU (host arrays, needs no GPU; one tape at a time): the checker of tds_hip_trajectory_vjp.  tape_cap
   (<= 0: the class's bound) and tape_len [n][steps] (optional: the entries each step recorded, -1 where it overflowed,
   0 for an environment whose inertia was not positive definite) as for tds_hip_vjp_host_tape.  Returns
   TDS_ERR_UNSUPPORTED where a tape overflowed, else TDS_ERR_INVALID_ARG where some environment's inertia was not
   positive definite, after writing every output. */
int tds_hip_trajectory_vjp_host(const tds_model_t *model, int n, int steps, int every, const double *x0,
                                const double *u, int p, const tds_param_t *params, const double *theta,
                                const double *gs, double *s, double *gx0, double *gu, double *gtheta,
                                int tape_cap, int *tape_len /* [n][steps], optional */);

/* Closed-loop policy gradients: the trajectory of tds_hip_trajectory_jvp (records, gains, theta, every, n_rec, scope,
   refusals and the f64-only rule as there) with EVERY step t = 0 .. steps - 1 taking its action from a policy network
   evaluated on the state that enters the step, u_t = pi_W(obs_t), and the gradients of a loss on the recorded states
   and on the actions through the dynamics AND the policy.
     obs_t   [q | qd] entering step t (x0's for t = 0, the state after step t - 1 otherwise) with obs[0] = obs[1] = 0,
             as the rollouts' policy kernels have it.  flags bit 0: step 0 sees the two entries raw (as tds_hip_rollout);
             flags bit 1: every step does (fixed-base models, whose q[0], q[1] are joints).  Other bits: INVALID_ARG.
     policy  [n][P] f64, per-environment parameters of the network num_layers, layer_sizes, activations, use_bias:
             checks, limits and parameter order of tds_hip_set_policy_network, P as tds_hip_policy_num_parameters counts
             it; num_layers = 0 is the default linear policy (action_dim x obs_dim weights, then biases).  The network
             is an argument: the handle's own (tds_hip_set_policy_network) is neither read nor changed.
   x0's action slots are not read.  A model with action_dim < 1 or whose record's action slots are not its actions
   (n_act != action_dim) gives TDS_ERR_INVALID_ARG.
   Cotangents: gs [n][n_rec][dof_q + dof_qd] on the recorded states and ga [n][steps][n_act] on the actions taken, each
   optional; both NULL computes the primal only (s required; no tapes are recorded, no gradient is written).
   Outputs: s [n][n_rec][dof_q + dof_qd] (optional where a cotangent is given), u [n][steps][n_act] the actions taken
   (optional), gpolicy [n][P], gx0 [n][input_dim] (its action slots are returned as zero), gtheta [n][p] (where p > 0).
   lambda_T = 0 and, t descending: the step's VJP as tds_hip_trajectory_vjp has it gives lambda_t's physical part and
   ubar_t; ubar_t += ga_t; gpolicy += (d pi / d W)^T ubar_t; lambda_t += mask^T (d pi / d obs)^T ubar_t, the layers'
   activations recomputed at obs_t.  The derivative is that of the algorithm as executed: ReLU and ELU take the
   primal's branch, masked observation entries pass nothing back.  NaN and overflow rules per environment as
   tds_hip_trajectory_vjp, gpolicy included.
   Device pointers (params_host, the network's arrays: host).  The primal runs one step per launch with the policy's
   forward kernel (one wavefront per environment) in front of each; backward, per chunk and window as
   tds_hip_trajectory_vjp, one launch records the window's tapes, then each step is swept by a launch of its own with
   the policy's backward kernel behind it.  Options traj_steps and traj_vjp_lanes apply as there and do not change the
   results.  Work buffer: tds_hip_trajectory_vjp's plus the x0 copy, the action store and its adjoints
   (n (input_dim + 2 (steps - 1) n_act) doubles); the primal-only call needs the state store, the primal lanes and the
   x0 copy and action store alone. */
int tds_hip_policy_trajectory_vjp(tds_hip_sim_t *sim, int n, int steps, int every, int flags, const void *x0_dev,
                                  const void *policy_dev, int num_layers, const int *layer_sizes,
                                  const int *activations, const int *use_bias, int p, const tds_param_t *params_host,
                                  const void *theta_dev, const void *gs_dev, const void *ga_dev, void *s_dev,
                                  void *u_dev, void *gpolicy_dev, void *gx0_dev, void *gtheta_dev);
/* The same on the CPU (host arrays, needs no GPU; one tape at a time): the checker.  The network's arithmetic is the
   device's statement with the device's summation tree (csrc/tds_policy.h).  tape_cap, tape_len and the return codes as
   tds_hip_trajectory_vjp_host (tape_len is written only where a cotangent is given). */
int tds_hip_policy_trajectory_vjp_host(const tds_model_t *model, int n, int steps, int every, int flags,
                                       const double *x0, const double *policy, int num_layers, const int *layer_sizes,
                                       const int *activations, const int *use_bias, int p, const tds_param_t *params,
                                       const double *theta, const double *gs, const double *ga, double *s, double *u,
                                       double *gpolicy, double *gx0, double *gtheta, int tape_cap,
                                       int *tape_len /* [n][steps], optional */);

/* Batched dynamics queries (the reference's forward_kinematics, mass_matrix, forward_dynamics, point_jacobian of
   python/pytinydiffsim.inl:629-668 and inverse_dynamics of src/dynamics/inverse_dynamics.hpp, for n states at once).
   State q [n][dof_q], qd [n][dof_qd] (NULL: zero), f64 device pointers.  Scope and refusals are those of
   tds_hip_jacobian (one articulated body, 1-DoF and fixed joints, f64 handles; the same messages).  Any n >= 1,
   independent of num_envs; the handle's resident state is not touched.  Enqueued on the handle's stream with no host
   wait except where the work buffer (shared with tds_hip_jvp, grown as needed: 8 (75 num_links + 2 dof_qd^2 + 9 dof_qd
   + 55) bytes for each of min(n, 16384) lanes) grows.  Only the outputs whose pointers are non-NULL are computed and
   written:
     x_world      [n][num_links][12]     rotation (9, row-major) and translation (3) of every link
     mass_matrix  [n][dof_qd][dof_qd]    the joint-space inertia (CRBA), both triangles
     bias         [n][dof_qd]            ID(q, qd, 0): gravity, Coriolis and centrifugal terms (no springs or dampers);
                                         fixed base only (TDS_ERR_UNSUPPORTED on a floating base: the reference has no
                                         floating-base inverse dynamics)
     qdd          [n][dof_qd]            unconstrained forward dynamics (no contacts, no PD): M = L L^T and a solve
                                         against tau - K q - D qd - bias (joint stiffness K and damping D as the
                                         reference's forward_dynamics has them); NaN for an environment whose M is not
                                         positive definite
   tau [n][dof_qd - (6 on a floating base)]: the torques of the actuated dofs, in the order the torque-actuated step
   reads its action slots; NULL: zero. */
typedef struct {  /* device pointers (tds_hip_dynamics) or host pointers (tds_hip_dynamics_host), each may be NULL */
  void *x_world;
  void *mass_matrix;
  void *bias;
  void *qdd;
} tds_dyn_out_t;
int tds_hip_dynamics(tds_hip_sim_t *sim, int n, const void *q_dev, const void *qd_dev, const void *tau_dev,
                     const tds_dyn_out_t *out);
/* tau [n][dof_qd] = ID(q, qd, qdd) (RNEA; qd, qdd NULL: zero): the torques that produce qdd without springs or dampers,
   M qdd + bias to round-off.  Fixed base only (TDS_ERR_UNSUPPORTED on a floating base). */
int tds_hip_inverse_dynamics(tds_hip_sim_t *sim, int n, const void *q_dev, const void *qd_dev, const void *qdd_dev,
                             void *tau_dev);
/* jac [n][3][dof_qd]: the world-frame Jacobian of a point on link `link` (one value per call; -1: the base), the point
   [n][3] given in world coordinates or, with is_local, in the link's own frame (taken to the world with X_world).  A
   link outside [-1, num_links) gives TDS_ERR_INVALID_ARG. */
int tds_hip_point_jacobian(tds_hip_sim_t *sim, int n, const void *q_dev, int link, const void *point_dev, int is_local,
                           void *jac_dev);
/* The same templates on the CPU (host arrays, need no GPU): the checkers of the three calls above.
   tds_hip_dynamics_host returns TDS_ERR_INVALID_ARG where some environment's M was not positive definite, after writing
   every output (that environment's qdd NaN). */
int tds_hip_dynamics_host(const tds_model_t *model, int n, const double *q, const double *qd, const double *tau,
                          const tds_dyn_out_t *out);
int tds_hip_inverse_dynamics_host(const tds_model_t *model, int n, const double *q, const double *qd, const double *qdd,
                                  double *tau);
int tds_hip_point_jacobian_host(const tds_model_t *model, int n, const double *q, int link, const double *point,
                                int is_local, double *jac);

/* Forward-mode derivatives of tds_hip_dynamics and tds_hip_inverse_dynamics in their inputs and in model parameters.
   The input of the dynamics call is  z = [q (dof_q) | qd (dof_qd) | tau (dof_qd - (6 on a floating base)) | theta (p)],
   that of the inverse-dynamics call  z = [q (dof_q) | qd (dof_qd) | qdd (dof_qd) | theta (p)].  For directions
   v [n][k][z] the tangents of every output `dout` names are written as [n][k][...the output's shape...]
   (dtau [n][k][dof_qd]), and (optionally, in the same call) the primal outputs `out` names (tau_dev), at
   theta_dev [n][p]: the selection params_host [p] of tds_hip_jvp_params, every kind tds_hip_params_get accepts;
   theta_dev NULL: the model's values.  k = 0 gives the primal at per-environment theta only (dout / dtau_dev and v_dev
   may then be NULL).  A NULL qd, tau or qdd stands for zeros in value; its columns of v still seed tangents.
   Convention: the derivative of the statement as executed (tds_hip_jvp's); quaternion entries of a floating base's q
   are differentiated raw.  The kinds the unconstrained dynamics do not read (friction, restitution, cfm, erp, the
   collision shapes) give exactly zero tangents.  An environment whose M is not positive definite has NaN in qdd and in
   qdd's tangents, and nowhere else.  Scope, refusals and messages: those of tds_hip_dynamics / tds_hip_inverse_dynamics
   (bias and inverse dynamics need a fixed base); selection errors: tds_hip_params_get's.
   Enqueued on the handle's stream as one launch.  The host waits only where the work buffer (shared with every other
   derivative and query call: calls on the stream use it in turn) grows, or, with p > 0, where the selection is copied
   into it (a blocking copy after a wait for the stream, as in tds_hip_jvp_params).  Work items are (environment,
   block of K directions), K = tds_hip_dynamics_jvp_tangents(model); at most 16384 lanes per launch, more items are
   walked with the grid's stride.  The primal is written by the items of the first block. */
int tds_hip_dynamics_jvp(tds_hip_sim_t *sim, int n, const void *q_dev, const void *qd_dev, const void *tau_dev, int p,
                         const tds_param_t *params_host, const void *theta_dev, int k, const void *v_dev,
                         const tds_dyn_out_t *out, const tds_dyn_out_t *dout);
int tds_hip_inverse_dynamics_jvp(tds_hip_sim_t *sim, int n, const void *q_dev, const void *qd_dev, const void *qdd_dev,
                                 int p, const tds_param_t *params_host, const void *theta_dev, int k, const void *v_dev,
                                 void *tau_dev, void *dtau_dev);
/* The same template on the CPU (host arrays, need no GPU): the checkers.  tds_hip_dynamics_jvp_host returns
   TDS_ERR_INVALID_ARG where some environment's M was not positive definite, after writing every output. */
int tds_hip_dynamics_jvp_host(const tds_model_t *model, int n, const double *q, const double *qd, const double *tau,
                              int p, const tds_param_t *params, const double *theta, int k, const double *v,
                              const tds_dyn_out_t *out, const tds_dyn_out_t *dout);
int tds_hip_inverse_dynamics_jvp_host(const tds_model_t *model, int n, const double *q, const double *qd,
                                      const double *qdd, int p, const tds_param_t *params, const double *theta, int k,
                                      const double *v, double *tau, double *dtau);
/* K: the tangents a work item of the two device calls carries for this model's class; a refused model gives minus its
   TDS_ERR_* code. */
int tds_hip_dynamics_jvp_tangents(const tds_model_t *model);

/* Batched contact query: what the step forward_zero(x) does about its plane contacts, for n records x [n][input_dim]
   (f64, the record of tds_hip_jvp / tds_hip_jacobian / tds_hip_step_host), per environment.  n_c is the model's number
   of plane contact points, a constant of the model: every point of every geometry (sphere 1, capsule 2, box 8, in
   the order of the model's geometries; the reference keeps all points), 0 without a plane: tds_hip_contact_layout.
   Scope and refusals are those of tds_hip_jacobian (one articulated body, 1-DoF and fixed joints, f64 handles; the
   same messages).  Any n >= 1, independent of num_envs; the handle's resident state is not touched.  Enqueued on the
   handle's stream as one launch with no host wait except where the work buffer (shared with tds_hip_jvp and
   tds_hip_dynamics) grows.  Only the outputs whose pointers are non-NULL are computed and written:
     contacts  [n][n_c][10]          world_normal_on_b (3) | world_point_on_b (3) | world_point_on_a (3) | distance
                                     (the plane is body a, the robot body b; world.hpp:206-282)
     jac       [n][n_c][3][dof_qd]   point_jacobian2(robot, link_b, world_point_on_b) (jacobian.hpp:13-90)
     rows      [n][3 n_c][dof_qd]    the solver's J: normal rows, friction-1 rows, friction-2 rows
                                     (mb_constraint_solver.hpp:278-388); exactly zero for a separated point
                                     (distance >= 0)
     rhs       [n][3 n_c]            the solver's b, at the velocities qd_pre
     delassus  [n][3 n_c][3 n_c]     A = J M^-1 J^T + cfm 1, both triangles
     impulse   [n][3 n_c]            p after the model's pgs_iterations sweeps of PGS, in row order
     force     [n][n_c][3]           the world-frame force on the robot at world_point_on_b:
                                     -(N p_n + t1 p_f1 + t2 p_f2) / dt, N, t1, t2 as tds_hip_contact_layout gives them
     qd_pre    [n][dof_qd]           the velocities the solver reads: qd + dt qdd after PD or torque actuation and
                                     forward dynamics
     qd_post   [n][dof_qd]           qd_pre - M^-1 J^T p: the qd part of forward_zero(x)
   An environment whose M is not positive definite has NaN in rows .. qd_post (contacts and jac stay valid).  With
   n_c = 0 only qd_pre and qd_post have any extent. */
typedef struct {  /* device pointers (tds_hip_contacts) or host pointers (tds_hip_contacts_host), each may be NULL */
  void *contacts;
  void *jac;
  void *rows;
  void *rhs;
  void *delassus;
  void *impulse;
  void *force;
  void *qd_pre;
  void *qd_post;
} tds_contact_out_t;
int tds_hip_contacts(tds_hip_sim_t *sim, int n, const void *x_dev, const tds_contact_out_t *out);
/* The same template on the CPU (host arrays, needs no GPU): the checker.  Returns TDS_ERR_INVALID_ARG where some
   environment's M was not positive definite, after writing every output. */
int tds_hip_contacts_host(const tds_model_t *model, int n, const double *x, const tds_contact_out_t *out);
/* n_c, and per contact point its link (-1: the base) and the index of its geometry; dirs [9]: the contact normal
   N = world_normal_on_b and the two friction directions t1, t2 of the rows (the same for every point: they follow
   from the plane's normal).  Each pointer may be NULL.  A refused model gives minus its TDS_ERR_* code (and
   tds_hip_last_error). */
int tds_hip_contact_layout(const tds_model_t *model, int32_t *link, int32_t *geom, double *dirs);

/* Forward-mode derivatives of the contact query in [x | theta]: for directions v [n][k][input_dim + p] the tangents
   of every output `dout` names, [n][k][...the output's shape...], and (optionally) the primal outputs `out` names, at
   theta_dev [n][p] (the selection params_host [p] of tds_hip_jvp_params, the contact kinds included; theta_dev NULL:
   the model's values).  k = 0 gives the primal at per-environment theta only (dout, v_dev may then be NULL).
   Convention: the derivative of the algorithm as executed (tds_hip_jvp's): the primal takes every branch — contact
   activation distance < 0, the [0, 1e5] clamp of the normal rows, the friction box, the action and max_force clamps —
   by value, and the tangent is that of the taken branch; a separated point has exactly zero tangents in rows, rhs,
   impulse and force; quaternion entries of x are differentiated raw.  An environment whose M is not positive definite
   has NaN in rows .. qd_post and in their tangents.  delassus and its tangent are computed only where one of them is
   asked for.  Scope, refusals and messages: those of tds_hip_jvp_params; selection errors: tds_hip_params_get's.
   Enqueued on the handle's stream as one launch.  The host waits only where the work buffer (shared with every other
   derivative and query call: calls on the stream use it in turn) grows, or, with p > 0, where the selection is copied
   into it (a blocking copy after a wait for the stream, as in tds_hip_jvp_params).  Work items are (environment,
   block of K directions), K = tds_hip_contacts_jvp_tangents(model); at most 16384 lanes per launch, more items are
   walked with the grid's stride.  The primal is written by the items of the first block. */
int tds_hip_contacts_jvp(tds_hip_sim_t *sim, int n, const void *x_dev, int p, const tds_param_t *params_host,
                         const void *theta_dev, int k, const void *v_dev, const tds_contact_out_t *out,
                         const tds_contact_out_t *dout);
/* The same template on the CPU (host arrays, needs no GPU): the checker.  Returns TDS_ERR_INVALID_ARG where some
   environment's M was not positive definite, after writing every output. */
int tds_hip_contacts_jvp_host(const tds_model_t *model, int n, const double *x, int p, const tds_param_t *params,
                              const double *theta, int k, const double *v, const tds_contact_out_t *out,
                              const tds_contact_out_t *dout);
/* K: the tangents a work item of tds_hip_contacts_jvp carries for this model's class; a refused model gives minus its
   TDS_ERR_* code. */
int tds_hip_contacts_jvp_tangents(const tds_model_t *model);

/* Batched inverse kinematics (the reference's TinyInverseKinematics::compute of src/tiny_inverse_kinematics.h:140-247,
   for n environments at once): from q_init [n][dof_q], move the actuated coordinates until the k body points (link
   links[j], point body_points[j][3] in the link's own frame; the same for every environment) reach
   targets [n][k][3] (world coordinates).  Each iteration: kinematics of q, J [3k][dof_qd] (a floating base's six
   columns zeroed) and e [3k] = target - actual, residual = |e|; residual < target_tolerance stops with REACHED;
   otherwise delta = J^T e (TRANSPOSE), J^+ e (PINV, the Moore-Penrose inverse: rank-deficient J is served) or
   J^T (J J^T + lambda^2 I)^-1 e (DAMPED_LM, lambda != 0), q_i += alpha delta_i and, with q_ref,
   q_i += weight_reference (q_ref_i - q_i) on the actuated coordinates (all of a fixed base's, q[7:] of a floating
   base's: the base pose is returned as given); sum delta_i^2 < step_tolerance^2 stops with CONVERGED; after
   max_iterations the status is FAILED.  An environment whose q stops being finite is FAILED with iterations =
   max_iterations, the others are not affected.  Outputs: q [n][dof_q] (f64), iterations [n], status [n] (int32) and
   residual [n] (f64; -1 for an environment that never iterated); the last three may be NULL.
   Scope and refusals are those of tds_hip_jacobian (the same messages); 1 <= k <= TDS_IK_MAX_TARGETS, links in
   [0, num_links), max_iterations >= 0, a known method, lambda != 0 with DAMPED_LM: otherwise TDS_ERR_INVALID_ARG.
   links, body_points (NULL: the links' origins) and opt (NULL: the defaults) are host pointers, read before the call
   returns.  Any n >= 1; enqueued on the handle's stream as ONE launch, no host wait except where the work buffer
   shared with tds_hip_jvp and tds_hip_dynamics grows. */
#define TDS_IK_MAX_TARGETS 4
enum { TDS_IK_TRANSPOSE = 0, TDS_IK_PINV = 1, TDS_IK_DAMPED_LM = 2 };    /* the reference's TinyIKMethod */
enum { TDS_IK_FAILED = 0, TDS_IK_CONVERGED = 1, TDS_IK_REACHED = 2 };    /* the reference's TinyIKStatus */
typedef struct {
  int32_t method;          /* TDS_IK_*; tds_hip_ik_default_options: TDS_IK_PINV */
  int32_t max_iterations;  /* 20 */
  double lambda;           /* 0.02   damping of DAMPED_LM */
  double target_tolerance; /* 1e-3   |e| below which the targets count as reached */
  double step_tolerance;   /* 1e-8   |delta| below which the iteration counts as converged */
  double alpha;            /* 5      step size */
  double weight_reference; /* 0.2    pull towards q_ref (used only where q_ref is given) */
} tds_ik_options_t;
void tds_hip_ik_default_options(tds_ik_options_t *opt);
int tds_hip_inverse_kinematics(tds_hip_sim_t *sim, int n, const void *q_init_dev, int k, const int32_t *links,
                               const double *body_points, const void *targets_dev, const void *q_ref_dev,
                               const tds_ik_options_t *opt, void *q_dev, void *iter_dev, void *status_dev,
                               void *residual_dev);
/* The same statement on the CPU (host arrays, needs no GPU): the checker of tds_hip_inverse_kinematics. */
int tds_hip_inverse_kinematics_host(const tds_model_t *model, int n, const double *q_init, int k, const int32_t *links,
                                    const double *body_points, const double *targets, const double *q_ref,
                                    const tds_ik_options_t *opt, double *q, int32_t *iterations, int32_t *status,
                                    double *residual);

/* Batched iLQR, part 1: the backward pass of n time-varying LQ problems of horizon T (csrc/tds_lqr.hip).  All arrays
   f64, row-major: A [n][T][nx][nx], B [n][T][nx][nu], lx [n][T+1][nx], lu [n][T][nu], lxx [n][T+1][nx][nx],
   luu [n][T][nu][nu], lux [n][T][nu][nx] (entry T of lx and lxx: the terminal cost), mu [n] (the regularisation of
   each problem).  From V_x = lx[T], V_xx = lxx[T], for t = T-1 .. 0:
       Q_x  = lx + A^T V_x           Q_u  = lu + B^T V_x
       Q_xx = lxx + A^T V_xx A       Q_ux = lux + B^T V_xx A
       Q_uu = luu + B^T V_xx B       Q_uu + mu I = L L^T   (Cholesky)
       k = -(Q_uu + mu I)^-1 Q_u     K = -(Q_uu + mu I)^-1 Q_ux
       V_x  = Q_x  + K^T Q_uu k + K^T Q_u  + Q_ux^T k
       V_xx = Q_xx + K^T Q_uu K + K^T Q_ux + Q_ux^T K,   then V_xx <- (V_xx + V_xx^T) / 2
       dV1 += k^T Q_u                dV2 += k^T Q_uu k / 2
   Outputs: k [n][T][nu], K [n][T][nu][nx], dv [n][2] = (dV1, dV2), status [n] (int32).  A problem whose Cholesky meets
   a pivot that is not positive at step t gets status t + 1, k = K = 0 over the whole horizon and dv = 0; the other
   problems are not affected; otherwise status 0.  Every element of every product and solve is one sequential sum in
   index order, the same on the device and in the host checker (the unit is built without FP contraction).
   1 <= nx <= TDS_LQR_MAX_NX, 1 <= nu <= TDS_LQR_MAX_NU: larger dimensions give TDS_ERR_UNSUPPORTED.  The handle
   supplies device, stream and error text; its model is not read.  ONE launch on the handle's stream, no host wait. */
#define TDS_LQR_MAX_NX 40
#define TDS_LQR_MAX_NU 16
int tds_hip_lqr_backward(tds_hip_sim_t *sim, int n, int T, int nx, int nu, const void *A_dev, const void *B_dev,
                         const void *lx_dev, const void *lu_dev, const void *lxx_dev, const void *luu_dev,
                         const void *lux_dev, const void *mu_dev, void *k_dev, void *K_dev, void *dv_dev,
                         void *status_dev);
/* The same statement with plain loops on the CPU (host arrays, needs no GPU): the checker. */
int tds_hip_lqr_backward_host(int n, int T, int nx, int nu, const double *A, const double *B, const double *lx,
                              const double *lu, const double *lxx, const double *luu, const double *lux,
                              const double *mu, double *k, double *K, double *dv, int32_t *status);

/* Batched iLQR, part 2: closed-loop rollout under time-varying affine feedback.  With nsd = dof_q + dof_qd and n_act
   the action slots of a step's record (input_dim - nsd, less the three gains of a locomotion model): x0
   [rows][input_dim], s_nom [P][T+1][nsd], u_nom [P][T][n_act], k [P][T][n_act], K [P][T][n_act][nsd], alpha [rows],
   problem_of_row [rows] (int32, entries in [0, P) -- the caller's promise; NULL: p = row).  s_0 = x0[:nsd], then
       u_t     = (u_nom[p,t] + alpha k[p,t]) + K[p,t] (s_t - s_nom[p,t])      (the last sum: index order)
       s_{t+1} = forward_zero([s_t | u_t | the rest of x0's record])[:nsd]
   Outputs s_out [rows][T+1][nsd], u_out [rows][T][n_act].  Actions are not clamped here (the step's own clamps apply).
   The step is the handle's forward_zero launch, rows served num_envs at a time; between the steps one small kernel
   forms u_t, assembles the next records and stores s_t, u_t.  Scope and refusals are those of tds_hip_jacobian (the
   same messages); a handle with model variants installed is refused.  Any rows >= 1, T >= 1; enqueued on the handle's
   stream, no host wait except where the work buffer shared with tds_hip_jvp grows. */
int tds_hip_feedback_rollout(tds_hip_sim_t *sim, int rows, int T, const void *x0_dev, const void *s_nom_dev,
                             const void *u_nom_dev, const void *k_dev, const void *K_dev, const void *alpha_dev,
                             const void *problem_of_row_dev, void *s_out_dev, void *u_out_dev);
/* The same statement over the host step (tds_hip_jacobian_host's y): the checker; num_problems bounds problem_of_row
   (TDS_ERR_INVALID_ARG outside).  Returns TDS_ERR_INVALID_ARG where some row's inertia was not positive definite. */
int tds_hip_feedback_rollout_host(const tds_model_t *model, int rows, int T, int num_problems, const double *x0,
                                  const double *s_nom, const double *u_nom, const double *k, const double *K,
                                  const double *alpha, const int32_t *problem_of_row, double *s_out, double *u_out);

/* Batched iLQR under control limits (box-DDP: Tassa, Mansard, Todorov, ICRA 2014), part 1: the backward pass of
   tds_hip_lqr_backward with bounds dlo <= dhi [n][T][nu] on the step k_t (lo - u_nom, hi - u_nom of the nominal controls;
   +-inf where a control has no limit).  Products, Q_x .. Q_uu, the V update, dv and the symmetrisation are the plain
   pass's; in place of the unconstrained solve, step t solves
       min_x  f(x) = x^T H x / 2 + q^T x   over dlo <= x <= dhi,     H = Q_uu + mu I,  q = Q_u
   by projected Newton from x = clamp(k_{t+1}, dlo, dhi) (clamp(0) at t = T-1).  For i = 1 .. 100:
     1. g = q + H x; control a is CLAMPED if (x_a == dlo_a and g_a > 0) or (x_a == dhi_a and g_a < 0), otherwise FREE
     2. no control free: stop
     3. first iteration, or the clamped set changed: H_ff = L L^T, as the Cholesky of H with the clamped rows and columns
        replaced by the identity's (a pivot that is not positive: status t + 1, as in the plain pass)
     4. |g_f|_2 < 1e-8: stop
     5. y_c = x_c, y_f = -H_ff^-1 (q_f + H_fc x_c); sd = (y - x)^T g; sd >= 0: stop
     6. line search: the candidate at step 1 is clamp(y) itself, at step < 1 clamp(x + step (y - x)); the first with
        (f(cand) - f(x)) / (step sd) >= 0.1 is taken, else step *= 0.6; step < 1e-22: stop and keep x
     7. x = cand
   then k_t = x, and K_t = -H_ff^-1 Q_ux,f on the free rows of the last factorisation's set, zero on its clamped rows,
   zero everywhere if the loop stopped with nothing free.  V and dv use the unregularised Q_uu, as in the plain pass.
   The constants (100, 1e-8, 0.1, 0.6, 1e-22) are the paper's.  With dlo = -inf, dhi = +inf, k, K, dv and status are
   tds_hip_lqr_backward's bit for bit (the first Newton point is the plain k by the same sums; the second iteration's
   test 4 ends the loop).  Further outputs: clamped [n][T] (int32; bit a set: control a clamped in the final set),
   qp_iterations [n][T] (int32; iterations begun, at most 100); both zero over the horizon of a problem whose status is
   not 0.  dlo <= dhi without NaN is the caller's promise on the device (the host checker returns TDS_ERR_INVALID_ARG).
   Bounds, refusals and messages otherwise as tds_hip_lqr_backward; ONE launch on the handle's stream, no host wait. */
int tds_hip_lqr_backward_box(tds_hip_sim_t *sim, int n, int T, int nx, int nu, const void *A_dev, const void *B_dev,
                             const void *lx_dev, const void *lu_dev, const void *lxx_dev, const void *luu_dev,
                             const void *lux_dev, const void *mu_dev, const void *dlo_dev, const void *dhi_dev,
                             void *k_dev, void *K_dev, void *dv_dev, void *status_dev, void *clamped_dev,
                             void *qp_iterations_dev);
/* The same statement with plain loops on the CPU: the checker.  dlo > dhi anywhere, or a NaN bound:
   TDS_ERR_INVALID_ARG. */
int tds_hip_lqr_backward_box_host(int n, int T, int nx, int nu, const double *A, const double *B, const double *lx,
                                  const double *lu, const double *lxx, const double *luu, const double *lux,
                                  const double *mu, const double *dlo, const double *dhi, double *k, double *K,
                                  double *dv, int32_t *status, int32_t *clamped, int32_t *qp_iterations);

/* Batched iLQR under control limits, part 2: tds_hip_feedback_rollout with
       u_t = min(max((u_nom[p,t] + alpha k[p,t]) + K[p,t] (s_t - s_nom[p,t]), u_lo[p,t]), u_hi[p,t])
   u_lo, u_hi [P][T][n_act] absolute bounds, indexed by the row's problem and the step; u_out and the record that enters
   the step both hold the clamped value.  u_lo = u_hi = NULL is tds_hip_feedback_rollout itself; one of them NULL is
   TDS_ERR_INVALID_ARG.  u_lo <= u_hi without NaN is the caller's promise on the device (the host checker returns
   TDS_ERR_INVALID_ARG).  Everything else as tds_hip_feedback_rollout. */
int tds_hip_feedback_rollout_box(tds_hip_sim_t *sim, int rows, int T, const void *x0_dev, const void *s_nom_dev,
                                 const void *u_nom_dev, const void *k_dev, const void *K_dev, const void *alpha_dev,
                                 const void *problem_of_row_dev, const void *u_lo_dev, const void *u_hi_dev,
                                 void *s_out_dev, void *u_out_dev);
int tds_hip_feedback_rollout_box_host(const tds_model_t *model, int rows, int T, int num_problems, const double *x0,
                                      const double *s_nom, const double *u_nom, const double *k, const double *K,
                                      const double *alpha, const int32_t *problem_of_row, const double *u_lo,
                                      const double *u_hi, double *s_out, double *u_out);

/* Batched system identification: one damped Gauss-Newton (Levenberg-Marquardt) step of n least-squares problems
   (csrc/tds_lm.hip).  Problem i owns the contiguous rows row_start[i] .. row_start[i+1]-1 of `rows` trajectories; a row
   has m = n_rec (nq + nd) residual entries; the rows of a problem share its p parameters.  All arrays row-major, f64
   where not said: row_start [n+1] (int32, non-decreasing from 0 to rows), s and s_obs [rows][m] (the simulated and the
   observed states), w [rows][m] or NULL (every weight 1), js [rows][p][m] (tds_hip_trajectory_jvp's js [n][k][n_rec][nsd]
   with k = p unit directions on theta, as it comes), dlo <= dhi [n][p] (bounds on the STEP; both NULL: none; +-inf where
   a parameter has none), lambda [n][n_lambda] (> 0: the damping of each candidate).
     Sums, over the entries of the problem's rows: an entry with w == 0 is skipped (its s_obs may be NaN: a missing
   measurement); otherwise a = w (s - s_obs), c_i = w js_i, and
       cost = sum a^2 / 2        g_i = sum c_i a        H_ij = sum c_i c_j
   each ONE sequential sum in the order (row ascending, entry ascending), products not contracted.
     Damping and the step, for each candidate l:
       D_i = min(max(H_ii, 1e-6), 1e32)                     (Ceres's min_lm_diagonal, max_lm_diagonal)
       A = H + lambda_l diag(D)
       delta_l = argmin  delta^T A delta / 2 + g^T delta   over dlo <= delta <= dhi
   by the projected-Newton box QP of tds_hip_lqr_backward_box (its rules 1-7 and constants, with H = A, q = g) from
   delta = clamp(0, dlo, dhi); with infinite bounds delta_l is the plain damped Gauss-Newton step -A^-1 g (zero where
   |g|_2 < 1e-8: rule 4).  pred_l = -(g^T delta_l + delta_l^T H delta_l / 2) with the undamped H.
     Outputs: cost [n], g [n][p], H [n][p][p] (symmetric), delta [n][n_lambda][p], pred [n][n_lambda], and int32
   [n][n_lambda] each: clamped (bit a set: parameter a in the QP's final clamped set), qp_iterations, status:
       0  the candidate is valid
       1  a pivot of that candidate's factorisation was not positive: delta_l = 0, pred_l = 0 (clamped, qp_iterations 0)
       2  the problem's cost or a diagonal entry of its H is not finite -- a counted entry that is not finite (the NaN
          records of an inertia that is not positive definite) always makes one so, as does an entry whose square
          overflows --: every candidate of that problem; cost = +inf, and g, H, delta, pred, clamped, qp_iterations zero
   The other problems are not affected, bit for bit as if run alone.  A problem without rows is legal (H = g = 0,
   delta = 0).  p = 0 is the cost-only mode: js, bounds, lambda and every output but cost may be NULL and only cost is
   written (+inf where it is not finite), whatever n_lambda.
     n >= 1, rows >= 0, m >= 1, 0 <= p <= TDS_LM_MAX_P, 0 <= n_lambda <= TDS_LM_MAX_LAMBDA: beyond the two bounds
   TDS_ERR_UNSUPPORTED.  A row_start that is not non-decreasing from 0 to rows, dlo > dhi, a NaN bound, a lambda that is
   not positive and finite: the caller's promise on the device (row_start is clipped to [0, rows], so that nothing
   outside the arrays is read), TDS_ERR_INVALID_ARG in the host checker.  Every sum and solve is the same sequence of
   operations on the device and in the host checker (the unit is built without FP contraction).  The handle supplies
   device, stream and error text; its model is not read.  ONE launch on the handle's stream, one wavefront per problem,
   no host wait. */
#define TDS_LM_MAX_P 16
#define TDS_LM_MAX_LAMBDA 8
int tds_hip_lm_step(tds_hip_sim_t *sim, int n, int rows, int m, int p, int n_lambda, const void *row_start_dev,
                    const void *s_dev, const void *s_obs_dev, const void *w_dev, const void *js_dev, const void *dlo_dev,
                    const void *dhi_dev, const void *lambda_dev, void *cost_dev, void *g_dev, void *H_dev,
                    void *delta_dev, void *pred_dev, void *clamped_dev, void *qp_iterations_dev, void *status_dev);
/* The same statement with plain loops on the CPU (host arrays, needs no GPU): the checker. */
int tds_hip_lm_step_host(int n, int rows, int m, int p, int n_lambda, const int32_t *row_start, const double *s,
                         const double *s_obs, const double *w, const double *js, const double *dlo, const double *dhi,
                         const double *lambda, double *cost, double *g, double *H, double *delta, double *pred,
                         int32_t *clamped, int32_t *qp_iterations, int32_t *status);

/* Duration of the most recent stepping CALL (all of its launches: one for a plain step, two for the split
   auto-reset step, 2 n + 1 for a per-step-launch rollout, the whole graph for tds_hip_step_many) measured with HIP
   events on the handle's stream, in milliseconds (enabled by tds_hip_set_timing(sim, 1); synchronises). */
int tds_hip_set_timing(tds_hip_sim_t *sim, int enable);
int tds_hip_last_kernel_ms(tds_hip_sim_t *sim, float *ms);

/* Diagnostic: run y = f(x) once on the resident records with the instrumented kernel build and
   return 14 shader-clock timestamps taken by workgroup 0 at the phase boundaries
   (A load + PD, B jcalc, C kinematics sweep, I narrowphase + visuals + D inertias, E composite
    inertia / bias force sweep, G mass matrix, H LDL^T, F forward-dynamics solve, (sync), J Jacobian rows,
    K row solves, L PGS, M pack, end).
   With n >= 28 and a grid the two-wavefront workgroups serve, THAT form is profiled: 0..13 are the main
   wavefront's stamps (3 -> 4, 7 -> 8 and 8 -> 9 contain the three workgroup barriers), 14..22 the helper's (start,
   constants loaded = before barrier 1, after barrier 1, narrowphase, visual poses + y tail, Jacobian rows = before
   barrier 2, after barrier 2, row solves = before barrier 3, after barrier 3).  Synchronises the stream. */
int tds_hip_profile_phases(tds_hip_sim_t *sim, long long *cycles_host, int n);

/* Host-side counterpart of the reference's SubmitProfileTiming hook (src/base.hpp:39; World::submit_profile_timing,
   world.hpp:82-86, called around "compute multi body contacts", "solve constraints", "integrate" ..., and
   MultiBodyConstraintSolver's "inverse_mass_matrix_a", "lcpA", "solve_pgs", mb_constraint_solver.hpp:225-439): runs ONE
   step of the resident state with the instrumented kernel build and calls fn(zone, microseconds, user) once per zone —
   the reference's zone names where a phase group of the kernel corresponds to one, "forward_dynamics/..." and
   "solve constraints/..." sub-zones for the kernel's own phases, "step" for the whole.  Durations are those of workgroup
   0's instruction stream (shader clock / the device's clock rate).  Synchronises the stream. */
typedef void (*tds_hip_profile_zone_fn)(const char *zone, double microseconds, void *user);
int tds_hip_profile_zones(tds_hip_sim_t *sim, tds_hip_profile_zone_fn fn, void *user);

/* Test aid: fills the LDS of every compute unit of the handle's device with a byte pattern (0xFF = NaN in every
   scalar type) by running workgroups that own a whole CU's LDS.  The step kernels never clear LDS, so a read of a slot
   nobody wrote normally sees benign leftovers; after this call it sees the pattern — a forgotten initialisation or a
   "0 x whatever" on an unwritten slot shows up as NaN deterministically instead of once in a blue moon
   (tests/test_hip_parity.py::test_no_step_reads_stale_lds).  Synchronises. */
int tds_hip_debug_poison_lds(tds_hip_sim_t *sim, int byte_pattern);

/* Static resource usage of the step kernel for this handle (for DESIGN.md / bench). */
int tds_hip_kernel_info(const tds_hip_sim_t *sim, int *lds_bytes_per_env, int *threads_per_env,
                        int *envs_per_block);

/* Which kernel a plain single step of this handle runs (tds_hip_step / _step_obs with substeps = 1, tds_hip_forward_zero_*,
   the launches of the tds_hip_step_many graphs): 0 the general kernel (csrc/tds_kernels.hip: lanes per environment as
   tds_hip_kernel_info reports), 1 the 16-lane kernel of the star-shaped legged robots with four-link legs (csrc/tds_quad.hip:
   a root body on the reference's six virtual links + four legs of three 1-dof joints and a fixed toe — Laikago, BASELINE
   config 4; create-time option quad = 0 keeps such a model on the general kernel), 2 the 8-lane kernel of the stars with
   two-link legs (csrc/tds_oct.hip: four legs of hip + ankle, a capsule on every leg link, a sphere on the root body — the gym
   Ant, BASELINE configs 3 and 5; create-time option oct = 0).  Both take models stepped with PD control on the leg joints
   only.  3 the kernel of the fixed-base serial chains without contacts (csrc/tds_chain.hip: 2 .. 8 links, link i the child of
   link i - 1, 1-dof joints, torques given directly — cartpole and pendulum5, BASELINE configs 1 and 2; create-time option
   chain = 0).  Optional outputs: that kernel's lanes and LDS bytes per environment. */
int tds_hip_single_step_kernel(const tds_hip_sim_t *sim, int *lanes_per_env, int *lds_bytes_per_env);

/* Which kernel and build a launch takes, asked on the CPU (no device needed): the plan launch() follows for a handle of
   `model` / `dtype` / `num_envs` on a device of `num_cus` compute units with `lds_per_cu` bytes of LDS each, under the
   process's default options (tds_hip_default_option).  req[TDS_PLAN_REQ_INTS]: environments in the launch, environments
   resident at the same time (0: the same), steps, reset mode (0 none, 1 auto, 2 forced), policy rollout, record rings,
   ... with progress counters, ... with peer stores, reset states from the pool, refill pass of the reset pool, phase stamps
   (0 none, 1 room for one wavefront's, 2 for the two-wavefront form's), auto-reset on.  out[TDS_PLAN_OUT_INTS]: kernel (as
   tds_hip_single_step_kernel), general kernel kind (0 .. 4), the kernel's build, the general kernel's build, its LDS layout
   (0 one-wave, 1 two-wavefront, 2 reset pool), environments and threads per workgroup, workgroups, refused (option
   loop_occ), and for a request over all num_envs environments: step-loop launch (1) or chained graphs (0), environment
   range of the 8-lane kernel's calls (0: one launch), exchange after the launch (ring launch with progress counters).
   Returns TDS_PLAN_OUT_INTS, or an error code. */
#define TDS_PLAN_REQ_INTS 12
#define TDS_PLAN_OUT_INTS 12
int tds_hip_launch_plan_host(const tds_model_t *model, int dtype, int num_envs, int num_cus, int lds_per_cu, const int *req,
                             int n_req, int *out, int n_out);

/* The window barriers of one step of the 8-lane kernel's two-wavefront builds, asked on the CPU (csrc/tds_oct_windows.h: the
   rule both wavefronts' loops follow), for a wavefront whose environments have at most `max_contacts` contacts, under
   `pgs_iterations` Gauss-Seidel iterations and option oct_long_window = `long_window_option`.  out[TDS_OCT_WINDOW_PLAN_INTS]:
   barriers the main wavefront takes, barriers the helper takes (a workgroup hangs where they differ), 1 if the first
   window of the first iteration runs on through the second window's rows.  Returns TDS_OCT_WINDOW_PLAN_INTS, or an error
   code. */
#define TDS_OCT_WINDOW_PLAN_INTS 3
int tds_hip_oct_window_plan_host(int max_contacts, int pgs_iterations, int long_window_option, int *out, int n_out);
/* The same walk with the main wavefront's first sweep in the instantiation specialised for the contact count where option
   oct_sweep_na = `sweep_na_option` sends it there (step-loop build for one wavefront per SIMD).  out[TDS_OCT_SWEEP_NA_PLAN_INTS]:
   barriers the main wavefront takes, barriers the helper takes, 1 if the first sweep is a specialised one. */
#define TDS_OCT_SWEEP_NA_PLAN_INTS 3
int tds_hip_oct_sweep_na_plan_host(int max_contacts, int pgs_iterations, int long_window_option, int sweep_na_option, int *out,
                                   int n_out);

/* ======================================================================================
 * Multi-GPU: the global batch of environments is cut into equal contiguous shards, one per rank /
 * GPU (rank r owns environments [r N/G, (r+1) N/G)); each shard is an ordinary tds_hip_sim on its own device, the
 * model constants are replicated, and there is NO collective inside the step.  The one exchange is an all-gather of
 * the [obs | reward | done] records, once per policy step, over RCCL / xGMI — called from here (librccl is loaded
 * with dlopen at first use), on a private communication stream, overlapped with the following steps.  New
 * functionality: the reference has no multi-device path.
 *
 *   one process per GPU:   rank 0: tds_hip_shard_unique_id(id) -> ship the 128 bytes to the other ranks by any
 *                          means (MPI, a file, torch.distributed) -> every rank: tds_hip_shard_create(..., id, ...)
 *   one process, G GPUs:   tds_hip_shard_create_all(model, N, G, devices, ...) and tds_hip_shard_group_step
 *   then per policy step:  tds_hip_shard_step(shard, actions_of_my_shard, substeps)
 *   consumer:              tds_hip_shard_gathered(shard, consumer_stream, &records, &steps_in_block): the gathered
 *                          records of the most recently submitted exchange, [world][block][n_local][obs_dim + 2]
 *                          in the wire dtype (block = 1: [N][obs_dim + 2] in global environment order); the
 *                          consumer's stream is made to wait for the exchange, the host never blocks.
 * ====================================================================================== */
#define TDS_SHARD_ID_BYTES 128 /* sizeof(ncclUniqueId) */
typedef struct tds_hip_shard tds_hip_shard_t;

/* version of the RCCL library found at run time (ncclGetVersion), 0 if none can be loaded */
int tds_hip_shard_rccl_version(void);
int tds_hip_shard_unique_id(void *id_out /* TDS_SHARD_ID_BYTES */);
/* This rank's shard of `global_envs` environments (a multiple of `world`) on HIP device `device`.
   dtype: TDS_DTYPE_* of the shard's sim.  wire_dtype: TDS_DTYPE_F32 (4 bytes per scalar on the wire, as SURVEY 8e
   sizes the exchange; F64 records are converted on the communication stream) or TDS_DTYPE_F64 (as computed).
   unique_id NULL is allowed for world == 1 only: the "exchange" is then a device copy (no RCCL needed).
   Collective: every rank of the communicator must call it. */
int tds_hip_shard_create(const tds_model_t *model, int global_envs, int rank, int world, int device, int dtype,
                         const void *unique_id, int wire_dtype, tds_hip_shard_t **out);
/* One process driving n_devices GPUs (ncclCommInitAll): out[i] = shard of rank i on devices[i]. */
int tds_hip_shard_create_all(const tds_model_t *model, int global_envs, int n_devices, const int *devices, int dtype,
                             int wire_dtype, tds_hip_shard_t **out /* [n_devices] */);
int tds_hip_shard_destroy(tds_hip_shard_t *shard);
/* the shard's simulation: every tds_hip_* call (state upload, reset, auto-reset, streams ...) applies to it */
tds_hip_sim_t *tds_hip_shard_sim(tds_hip_shard_t *shard);
int tds_hip_shard_rank(const tds_hip_shard_t *shard);
int tds_hip_shard_world(const tds_hip_shard_t *shard);
int tds_hip_shard_local_envs(const tds_hip_shard_t *shard);
int tds_hip_shard_first_env(const tds_hip_shard_t *shard); /* global index of the shard's first environment */
int tds_hip_shard_wire_bytes(const tds_hip_shard_t *shard);
/* Records of `steps_per_exchange` consecutive steps travel in ONE all-gather (default 1 = SURVEY 8e's protocol:
   one exchange per policy step).  Larger blocks trade observation latency for fewer collectives.  Flushes. */
int tds_hip_shard_set_block(tds_hip_shard_t *shard, int steps_per_exchange);
/* One closed-loop step of the shard (tds_hip_step_obs into the ring's record block) and, when the block is complete,
   its all-gather on the communication stream.  Asynchronous. */
int tds_hip_shard_step(tds_hip_shard_t *shard, const void *actions_dev, int substeps);
/* The same for all shards of one process (tds_hip_shard_create_all): the steps are enqueued device by device, the
   all-gathers go out as one RCCL group. */
int tds_hip_shard_group_step(tds_hip_shard_t **shards, int n, const void *const *actions_dev, int substeps);
/* n_steps steps of the shard INCLUDING their exchanges as one hipGraph launch (the two-stream pattern of
   tds_hip_shard_step captured once, RCCL all-gathers as graph nodes): one host call per n_steps instead of ~8 per
   step — the eager form is host-bound at ~20 us per step.  actions_dev [action_blocks][n_local][action_dim], step k
   uses block (first_block + k) % action_blocks.  n_steps: a multiple of the exchange block, <= 4096.  Collective:
   every rank makes the same call.  Falls back to eager stepping if the capture is refused (TDS_HIP_SHARD_NO_GRAPH=1
   forces that), and steps eagerly when auto-reset is on (the refill passes of the reset pool are host-driven).

   RING EXCHANGE.  Where tds_hip_step_many_is_loop holds for the shard's simulation (and the exchange block is 1) the
   n_steps steps are step-loop launches of up to 256 steps (option shard_chunk) — the very launches of
   tds_hip_step_many_rings, storing every step's record straight into this rank's block of that step's gathered slot (in-
   place all-gather; the obs ring in the wire dtype) and a y ring, i.e. the same work per step as a single GPU does — with
   one ncclAllGather per policy step on the communication stream, no kernel boundary per step, nothing the step needs
   waiting for the exchange.  WHEN a slot travels depends on the build of the launch (option exchange_w2):
     1 (default)  the two-wavefront build N = 1 runs: it fills every SIMD's register file, so nothing of the exchange
                  could run beside it — the launch runs exactly as at N = 1 and the communication stream sends its slots
                  as ONE RCCL group as soon as it has completed (beside the NEXT launch; launch j + 2 waits for the
                  exchanges of launch j);
     0            the one-wave build: every workgroup counts itself in on the slot's own device counter once its records
                  of step k are visible device-wide, and the communication stream — one bounded one-lane wait kernel (or
                  hipStreamWaitValue64: option shard_wait) + one all-gather per step — sends slot k while the launch runs
                  step k + 1, as soon as the SLOWEST workgroup has stored it.
   PEER-STORE EXCHANGE (round 5; option shard_peer, default on where every rank can set it up).  The all-gather without a
   collective: at the first tds_hip_shard_step_many every rank maps the other ranks' gathered rings and flag arrays into its
   address space (hipIpcGetMemHandle / hipIpcOpenMemHandle, the handles exchanged once over the communicator; a token round
   trip over the mapped memory checks the mapping) and from then on the step-loop launch itself — the N = 1 two-wavefront
   build — stores every step's record into its own block of the slot on EVERY rank (system-scope write-through stores over
   xGMI, issued by the helper wavefront that stores the record anyway) and raises the slot's flag on every rank when its
   last workgroup has stored it.  The transfer of step k lies inside step k + 1 of the same launch; no kernel of the
   exchange needs a compute unit beside the launch, no host call per step.  Around a LAUNCH: a one-wave credit kernel in
   front of it (ranks drift apart by at most one launch: launch m waits until every peer has started launch m - 1) and a
   one-wave arrival check behind it on the communication stream (what tds_hip_shard_gathered / _flush wait for).  If IPC
   cannot be set up on ANY rank, every rank uses the RCCL forms above (shard_peer = 2: an error instead; = 0: never
   tried).  Option exchange_fields = 1 sends only [reward | done] to the peers (8 instead of 120 bytes per Ant
   environment and step on the float wire: for runs whose policy lives on the device, tds_hip_rollout).
   Option shard_peer_copy = 1 (round 6) is the STAGED form of the same exchange: the launch stores into this rank's block
   only and raises this rank's own flags; behind it the communication stream copies the launch's slots into every peer's ring
   (one strided device-to-device copy per peer: the runtime's copy engines) and a one-wave kernel raises the flags there —
   no store over the fabric from inside the kernel, full records only.  Option shard_peer_release = 1 puts system-scope
   release fences in front of the arrival counts and the flag stores of the in-kernel form (default: s_waitcnt vmcnt(0) +
   relaxed stores): the ordering assumption of the protocol can be A/B-ed on a fabric in one run.
   tds_hip_shard_exchange_form tells which form the most recent call ran.
   Option shard_graph = 1 replays each launch + its exchanges from one hipGraph instead (cached by arguments; slower on
   ROCm 7: a chain of dependent graph nodes pays a node-to-node latency a stream does not).  tds_hip_shard_gathered then
   returns the slot of the last step, [world][n_local][obs_dim + 2].  Option shard_ring = 0 forces the per-step-launch
   form. */
int tds_hip_shard_step_many(tds_hip_shard_t *shard, const void *actions_dev, int action_blocks, int first_block,
                            int n_steps);
/* which exchange the most recent tds_hip_shard_step / _step_many of the shard ran (0: none yet) */
enum {
  TDS_EXCHANGE_NONE = 0,
  TDS_EXCHANGE_RCCL_PER_STEP = 1,     /* one kernel launch + one ncclAllGather per step (eager or from one hipGraph) */
  TDS_EXCHANGE_RCCL_AFTER_LAUNCH = 2, /* ring exchange, two-wavefront build: the launch's slots as ONE RCCL group behind it */
  TDS_EXCHANGE_RCCL_PER_SLOT = 3,     /* ring exchange, one-wave build: wait kernel + ncclAllGather per slot beside the launch */
  TDS_EXCHANGE_PEER_STORES = 4,       /* ring exchange by peer stores: no collective, the launch writes every rank's ring */
  TDS_EXCHANGE_PEER_COPY = 5          /* the same rings, flags and credit protocol, STAGED (option shard_peer_copy = 1): the launch
                                         writes this rank's ring only; behind it the communication stream copies the launch's
                                         slots into every peer's ring (one strided device-to-device copy per peer: the runtime's
                                         copy engines) and raises the flags — no collective, no fabric store from the kernel */
};
int tds_hip_shard_exchange_form(const tds_hip_shard_t *shard);
/* ranks this shard stores its records to under the peer-store exchange (0 on one rank; -1: the exchange is not in use) */
int tds_hip_shard_peer_count(const tds_hip_shard_t *shard);
/* capture + instantiate the graph of the next tds_hip_shard_step_many with the same arguments; nothing executes */
int tds_hip_shard_step_many_prepare(tds_hip_shard_t *shard, const void *actions_dev, int action_blocks,
                                    int first_block, int n_steps);
/* Introspection of the ring exchange's host arithmetic (no device needed; csrc/tds_shard_plan.h): the step-loop launches
   ("chunks", here of up to 64 steps each; a shard takes its option shard_chunk, default 256) a tds_hip_shard_step_many call of n_steps steps is cut into after chunks_done earlier
   chunks, 6 ints per chunk in out [6 * cap]: ring half | steps | first step of the call | action block of its first
   step | ring slot of its first step | progress count the communication stream waits for before it sends that slot
   (n_blocks workgroups per step; 0 = "the launch's completion").  Returns the number of chunks, -1 on bad arguments.
   tds_hip_shard_gathered_offset: scalar offset of global environment e's record in a gathered block-1 slot. */
int tds_hip_shard_ring_plan(long long chunks_done, int n_steps, int act_first, int act_blocks, int n_blocks, int *out,
                            int cap);
long long tds_hip_shard_gathered_offset(int global_env, int n_local, int width);
/* Exchange a partially filled block, then wait (host) until every exchange in flight has completed. */
int tds_hip_shard_flush(tds_hip_shard_t *shard);
int tds_hip_shard_gathered(tds_hip_shard_t *shard, void *consumer_stream, void **records_dev, int *steps_in_block);
/* Ring exchange only: the gathered records [world][n_local][obs_dim + 2] of the step `steps_back` steps before the most
   recently submitted one (0: what tds_hip_shard_gathered returns), as long as it lies inside the most recently submitted
   step-loop launch (its slots are still in the ring); the consumer's stream waits for that launch's exchanges. */
int tds_hip_shard_gathered_step(tds_hip_shard_t *shard, int steps_back, void *consumer_stream, void **records_dev);

/* ======================================================================================
 * Free rigid bodies: World::step for worlds that hold tds::RigidBody
 * objects — apply gravity, pairwise narrowphase, RigidBodyConstraintSolver (sequential impulses
 * with Baumgarte stabilisation and Coulomb friction), integrate.
 * Reference: src/world.hpp:293-366 (step), :163-204 (pairs), src/rigid_body.hpp:26-123,
 * src/rb_constraint_solver.hpp:65-168, src/contact_point.hpp:43-198,405-506: every pair the
 * reference's CollisionDispatcher knows — sphere-sphere, plane-sphere, plane-capsule (2 end spheres),
 * plane-box (8 corner spheres), capsule-sphere, each also in the swapped order; any other pair
 * produces no contact, as in the reference.  N independent worlds of the same bodies, one launch.
 * ====================================================================================== */
#define TDS_RB_MAX_BODIES 16
#define TDS_RB_STATE 13 /* per body: position(3) | orientation quaternion x y z w (4) | linear velocity(3) | angular velocity(3) */

typedef struct tds_rb_body {
  double mass;          /* 0: static (inv_mass = 0, inv_inertia = 0; rigid_body.hpp:49-53), else inv_inertia = 1 */
  int32_t geom_type;    /* TDS_GEOM_SPHERE / PLANE / CAPSULE / BOX */
  int32_t pad_;
  double radius;        /* sphere, capsule (box: radius of the rounded corners, normally 0) */
  double length;        /* capsule: distance of the end-sphere centres along local z */
  double extents[3];    /* box: full edge lengths */
  double plane_normal[3];
  double plane_constant;
} tds_rb_body_t;

typedef struct tds_rb_model {
  int32_t abi_version;  /* TDS_HIP_ABI_VERSION */
  int32_t num_bodies;   /* <= TDS_RB_MAX_BODIES */
  int32_t solver_iterations; /* World::num_solver_iterations (default 1) */
  int32_t pad_;
  double dt;
  double gravity[3];    /* World::gravity_acceleration_ (default 0 0 -9.81) */
  double restitution;   /* World::default_restitution (0) */
  double friction;      /* World::default_friction (0.5) */
  double erp;           /* RigidBodyConstraintSolver::erp_ (0.1) */
  tds_rb_body_t bodies[TDS_RB_MAX_BODIES];
} tds_rb_model_t;

typedef struct tds_rb_sim tds_rb_sim_t;

const char *tds_rb_last_error(void);
int tds_rb_create(const tds_rb_model_t *model, int num_worlds, int device, int dtype, tds_rb_sim_t **out);
int tds_rb_destroy(tds_rb_sim_t *sim);
int tds_rb_set_stream(tds_rb_sim_t *sim, void *hip_stream);
/* resident state, world-major [num_worlds][num_bodies][TDS_RB_STATE] in the compute dtype */
void *tds_rb_state_device(tds_rb_sim_t *sim);
int tds_rb_set_state(tds_rb_sim_t *sim, const double *state_host);
int tds_rb_get_state(tds_rb_sim_t *sim, double *state_host);
/* `steps` World::step calls on every world, one launch (async on the stream) */
int tds_rb_step(tds_rb_sim_t *sim, int steps);

/* Forward-mode derivatives of rollouts: s_T after `steps` World::steps from s0, and jv = (d s_T / d [s0 | theta]) v.
   The derivative is that of the algorithm as executed (contact activation, the nrv / impulse tests, the friction clamp
   and the lateral-speed test follow the primal's branch; quaternion entries raw).  theta [n][p] per world: the scalars a
   selection params[p] names, of these kinds only: TDS_PARAM_LINK_MASS (link = body index, dynamic bodies; inv_mass =
   1 / theta, the inverse inertia stays eye3), TDS_PARAM_GRAVITY (comp 0..2), TDS_PARAM_FRICTION, TDS_PARAM_RESTITUTION.
   Any other kind, a body out of range, a static body's mass or a duplicate gives TDS_ERR_INVALID_ARG.
   s0 [n][num_bodies][TDS_RB_STATE], v [n][k][num_bodies * TDS_RB_STATE + p] (columns in the order of the state, then
   theta), sT [n][num_bodies][TDS_RB_STATE], jv [n][k][num_bodies * TDS_RB_STATE].  k = 0 computes sT only (v, jv may then
   be NULL); with k > 0 sT may be NULL.  theta NULL: the model's values.  Any n >= 1, independent of num_worlds; the
   handle's resident state is not touched.  Device pointers (params_host: host array), f64 handles only (an f32 handle
   gives TDS_ERR_UNSUPPORTED); enqueued on the handle's stream.  Work buffer (kept by the handle, grown as needed):
   num_bodies * 15 * 2 doubles per lane of a launch, min(n * ceil(k / 2), 262144) lanes. */
int tds_rb_jvp(tds_rb_sim_t *sim, int n, int steps, const void *s0_dev, int p, const tds_param_t *params_host,
               const void *theta_dev, int k, const void *v_dev, void *sT_dev, void *jv_dev);
/* The same template on the CPU (host arrays, needs no GPU): the checker of tds_rb_jvp. */
int tds_rb_jvp_host(const tds_rb_model_t *model, int n, int steps, const double *s0, int p, const tds_param_t *params,
                    const double *theta, int k, const double *v, double *sT, double *jv);
/* theta [p] = the model's values of the selection (host arrays); checks the selection. */
int tds_rb_params_get(const tds_rb_model_t *model, int p, const tds_param_t *params, double *theta);

/* Reverse-mode derivatives of rollouts: the rollout of tds_rb_jvp, the state after every `every`-th step recorded in
   s [n][n_rec][num_bodies][TDS_RB_STATE] (n_rec = steps / every; every must divide steps, every = steps gives s_T alone),
   one cotangent gs [n][n_rec][num_bodies * TDS_RB_STATE] on the recorded states, and its gradients gs0
   [n][num_bodies * TDS_RB_STATE] in s0 and gtheta [n][p] in theta: sum over the records of (d s_r / d [s0 | theta])^T gs_r.
   s may be NULL; gs0 or gtheta may be NULL where not wanted; gtheta is not touched when p = 0.  The convention, the
   selections, theta (NULL: the model's values), the checks and the scope are tds_rb_jvp's: the derivative of the
   algorithm as executed, quaternion entries raw, f64 handles only (an f32 handle gives TDS_ERR_UNSUPPORTED), any
   n >= 1, the resident state untouched, enqueued on the handle's stream (the call waits for its launches: it reports
   overflows).
   A primal pass keeps the state after every step; the steps' tapes are then recorded a window of W steps at a time,
   one lane per (step, world), and swept back once; only the state cotangent crosses window boundaries.
   tape_cap: the entries one step's tape of one world may hold; 0: a bound derived from the model (collision spheres of
   the pairs the dispatcher accepts x solver_iterations x the entries of one narrowphase + solve, plus gravity and
   integrate), capped by what work_bytes leaves for one step of 64 worlds.  A world one of whose steps overflows gets NaN
   in gs0 and gtheta and the call returns TDS_ERR_UNSUPPORTED ("tape exceeds the capacity"); the other worlds' results
   stand.  A collision sphere that ends without an impulse leaves no entries, so a scene whose contacts are few next to
   its pairs (billiards: 350 to 11 765 entries per step against a bound of 336 448) is served far better by an explicit
   tape_cap: the tapes' strides, hence W, follow the capacity.
   work_bytes: the upper bound on the handle's work buffer for this call (0: 8 GiB); it decides W and the worlds per
   pass (whole wavefronts), never the results.  One that cannot hold one step of 64 worlds gives TDS_ERR_INVALID_ARG; the
   message names the size needed.  tds_rb_vjp_plan tells what a call would choose, without a device:
   plan[4] = tape capacity | worlds per pass | W | bytes of work buffer. */
int tds_rb_vjp(tds_rb_sim_t *sim, int n, int steps, int every, const void *s0_dev, int p,
               const tds_param_t *params_host, const void *theta_dev, const void *gs_dev, void *s_dev, void *gs0_dev,
               void *gtheta_dev, int tape_cap, size_t work_bytes);
/* The same templates on the CPU (host arrays, needs no GPU), one world and one tape at a time: the checker of
   tds_rb_vjp. */
int tds_rb_vjp_host(const tds_rb_model_t *model, int n, int steps, int every, const double *s0, int p,
                    const tds_param_t *params, const double *theta, const double *gs, double *s, double *gs0,
                    double *gtheta, int tape_cap);
int tds_rb_vjp_plan(const tds_rb_model_t *model, int n, int steps, int p, int tape_cap, size_t work_bytes,
                    long long *plan);

#ifdef __cplusplus
}
#endif
#endif /* TDS_HIP_H */
