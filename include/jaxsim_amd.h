/* jaxsim_amd -- C ABI of the MI355X-native batched rigid-body step.
 *
 * Drop-in boundary for the hot path of ami-iit/jaxsim.  The reference has no FFI seam: the
 * path sits behind plain Python functions taking (model, data) pytrees.  Each entry point
 * below names the reference function it replaces (paths relative to the reference root).
 * A Python maintainer binds these with ctypes (INTEGRATION.md shows the stub); the in-tree
 * binding is jaxsim_amd/_lib.py.
 *
 * Conventions
 *  - plain C types only; no torch / HIP types in signatures (streams are `void*`
 *    = hipStream_t, NULL = default stream);
 *  - every batched array is a *device* pointer, struct-of-arrays with the batch index fastest,
 *    tile-interleaved: written below as [rows][N], stored as [ceil(N/T)][rows][T] where
 *    T = jxs_layout.tile environments (the environments one wavefront processes; T = 2 for the
 *    24-link humanoid).  Element (row, env) lives at ((env/T)*rows + row)*T + env%T; arrays are
 *    allocated in whole tiles.  dtype = the model's dtype (float or double);
 *  - state block rows (reference `JaxSimModelData`, src/jaxsim/api/data.py:46-63; the base
 *    velocity is stored inertial-fixed like the reference, :151-156,187-188):
 *        base_position[3] base_quaternion[4] (wxyz) joint_positions[n]
 *        base_linear_velocity[3] base_angular_velocity[3] joint_velocities[n]
 *        tangential_deformation[n_cp][3]
 *    row offsets are reported by jxs_model_layout();
 *  - all kernels are asynchronous on the given stream; the caller synchronises;
 *  - functions return 0 on success, a negative JXS_E* code otherwise, and
 *    jxs_last_error() returns a thread-local message.  No exceptions cross the ABI.
 */
#ifndef JAXSIM_AMD_H
#define JAXSIM_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define JXS_OK 0
#define JXS_EINVAL (-1)      /* bad argument / unsupported model                     */
#define JXS_ENODEVICE (-2)   /* no HIP device / HIP runtime error                    */
#define JXS_ENOMEM (-3)
#define JXS_ECOMM (-4)       /* RCCL error                                           */

#define JXS_F32 0
#define JXS_F64 1

/* Velocity / force representations: src/jaxsim/api/common.py:39-47 */
#define JXS_REPR_INERTIAL 0
#define JXS_REPR_BODY 1
#define JXS_REPR_MIXED 2

/* IntegratorType: src/jaxsim/api/model.py:32-40.  RungeKutta4Fast (api/integrators.py:170-276) only with
 * the rigid contact models: the reference's version corrupts the SoftContacts state and fails without
 * collidable points. */
#define JXS_INTEGRATOR_SEMI_IMPLICIT_EULER 0
#define JXS_INTEGRATOR_RUNGE_KUTTA4 1
#define JXS_INTEGRATOR_RUNGE_KUTTA4_FAST 2

/* Contact models: src/jaxsim/rbda/contacts/{soft,rigid,relaxed_rigid}.py */
#define JXS_CONTACT_SOFT 0
#define JXS_CONTACT_RIGID 1
#define JXS_CONTACT_RELAXED_RIGID 2

/* Host description of one model: the static tables of `KinDynParameters`
 * (src/jaxsim/api/kin_dyn_parameters.py:86-284) plus the model-level constants of
 * `JaxSimModel` (src/jaxsim/api/model.py:52-82).  All arrays are host pointers, indexed by
 * the reference link index (entry 0 of the per-joint arrays is unused: joint i moves link i).
 */
typedef struct jxs_model_desc {
  int32_t n_links;
  int32_t floating_base;
  int32_t dtype; /* JXS_F32 | JXS_F64 */
  const int32_t* parent;        /* [nL]   parent_array, parent[0] = -1                      */
  const int32_t* joint_type;    /* [nL]   1 revolute, 2 prismatic (math/joint_model.py)     */
  const double* joint_axis;     /* [nL][3]                                                  */
  const double* lambda_H_pre;   /* [nL][16] row-major 4x4                                   */
  const double* suc_H_i;        /* [nL][16]                                                 */
  const double* link_mass;      /* [nL]                                                     */
  const double* link_com;       /* [nL][3]                                                  */
  const double* link_inertia;   /* [nL][9] I_CoM row-major                                  */
  const double* friction_static;       /* [nL] */
  const double* friction_viscous;      /* [nL] */
  const double* position_limit_min;    /* [nL] */
  const double* position_limit_max;    /* [nL] */
  const double* position_limit_spring; /* [nL] */
  const double* position_limit_damper; /* [nL] */
  int32_t n_points;               /* collidable points (ContactParameters, :765-840)        */
  const int32_t* point_body;      /* [n_points]                                             */
  const double* point_position;   /* [n_points][3]                                          */
  const uint8_t* point_enabled;   /* [n_points]                                             */
  double time_step;               /* api/model.py:54-56                                     */
  double gravity;                 /* signed z acceleration (-9.81)                          */
  double K, D, mu, p, q;          /* SoftContactsParams, rbda/contacts/soft.py:24-46        */
  double terrain_height;          /* Flat/PlaneTerrain height over the origin, terrain/terrain.py:65-238 */
  double torque_max, omega_th, omega_max; /* ActuationParams, rbda/actuation/common.py:16-19 */
  int32_t enable_friction;
  double terrain_normal[3];       /* PlaneTerrain unit normal (terrain/terrain.py:127-238); (0,0,1) = FlatTerrain */
  int32_t integrator;             /* JXS_INTEGRATOR_*: model.integrator, api/model.py:2665-2678 */
  int32_t contact_model;          /* JXS_CONTACT_*; with JXS_CONTACT_RIGID K, D, mu are RigidContactsParams
                                     (rbda/contacts/rigid.py:28-42) and p, q are ignored */
  double regularization_delassus; /* RigidContacts.regularization_delassus (rigid.py:99-101), 1e-6 */
  double solver_tol;              /* RigidContacts solver_options["solver_tol"] (rigid.py:103-108), 1e-3 */
  /* JXS_CONTACT_RELAXED_RIGID: RelaxedRigidContactsParams (rbda/contacts/relaxed_rigid.py:29-75); mu above is
     its friction coefficient, K and D are ignored exactly as the reference ignores them (:567-568) */
  double rr_time_constant, rr_damping_coefficient, rr_d_min, rr_d_max, rr_width, rr_midpoint, rr_power;
  /* [round 6] Height-field terrain: the reference's generic `Terrain` (terrain/terrain.py:15-62: any height(x, y), the
     normal by central differences with delta = 0.01) in the form a C ABI can carry -- heights sampled on a regular
     grid, sample [ix][iy] at (origin + (ix dx, iy dy)), row-major with x outer; height(x, y) is the BILINEAR
     interpolant (clamped to the border samples outside the grid) and the normal is
     n = [(h(x-d,y) - h(x+d,y)) / 2d, (h(x,y-d) - h(x,y+d)) / 2d, 1] / |.| of THAT function, d = terrain_delta
     (terrain.py:52-62).  NULL: the flat / plane terrain above.  With a grid `terrain_height` / `terrain_normal` are
     not used.  All three contact models.                                                                           */
  const double* terrain_grid;     /* [terrain_nx][terrain_ny] or NULL                                               */
  int32_t terrain_nx, terrain_ny; /* >= 2 each                                                                      */
  double terrain_origin[2];       /* (x, y) of sample [0][0]                                                        */
  double terrain_spacing[2];      /* (dx, dy), both > 0                                                             */
  double terrain_delta;           /* step of the central difference (Terrain.delta = 0.010, terrain.py:23); 0 = 0.01 */
} jxs_model_desc;

typedef struct jxs_model jxs_model; /* opaque, immutable after creation, shareable */

typedef struct jxs_layout {
  int32_t n_links, n_joints, n_points, n_rows;
  int32_t row_pos, row_quat, row_s, row_vlin, row_vang, row_sd, row_m;
  int32_t group; /* lanes per environment chosen for this model */
  int32_t tile;  /* T = 64 / group: environments per tile of every batched array */
  int32_t dtype;
  int32_t row_mode; /* 1: ABA passes run row-distributed (8 lanes per active link), 0: link per lane */
} jxs_layout;

/* ---- library / device ---------------------------------------------------------------- */
const char* jxs_last_error(void);
int jxs_device_count(int* count);
int jxs_set_device(int device);
int jxs_malloc(void** dptr, uint64_t bytes);
int jxs_free(void* dptr);
int jxs_memcpy_h2d(void* dst, const void* src, uint64_t bytes, void* stream);
int jxs_memcpy_d2h(void* dst, const void* src, uint64_t bytes, void* stream);
int jxs_memcpy_d2d(void* dst, const void* src, uint64_t bytes, void* stream);
int jxs_memset(void* dst, int value, uint64_t bytes, void* stream);
int jxs_stream_create(void** stream);
int jxs_stream_destroy(void* stream);
int jxs_stream_synchronize(void* stream);
/* Same completion guarantee, waited for by polling from the calling thread (microsecond-scale wake-up;
 * for timing short regions).                                                                   */
int jxs_stream_wait_spin(void* stream);
int jxs_device_synchronize(void);
/* HIP events on a stream (bench.py times the step kernel with these). */
int jxs_event_create(void** event);
int jxs_event_destroy(void* event);
int jxs_event_record(void* event, void* stream);
int jxs_event_elapsed_ms(void* start, void* stop, float* ms);

/* ---- model ----------------------------------------------------------------------------
 * Replaces JaxSimModel.build / KinDynParameters.build as far as the device is concerned:
 * uploads the constant tables (src/jaxsim/api/model.py:225-330).                        */
int jxs_model_create(const jxs_model_desc* desc, jxs_model** out);
int jxs_model_destroy(jxs_model* model);
int jxs_model_layout(const jxs_model* model, jxs_layout* out);

/* ---- model-specialised kernels ----------------------------------------------------------
 * The reference compiles `step` per model: the kinematic tree (parent array, joint types, ...) is static
 * under jax.jit (src/jaxsim/api/model.py:36-120, `static_field`s of KinDynParameters) and XLA folds it into
 * the program.  The generic kernels of this library read the same facts as wave-uniform flags at run time
 * and branch on them, which costs a lone wave ~20 % of the step.  A specialised
 * kernel is the SAME hand-written kernel source compiled with those integer flags as constants
 * (jaxsim_amd/csrc/jxs_spec.hip, built by jaxsim_amd/specialize.py with hipcc); physical parameters
 * (masses, gains, time step, contact parameters) stay run-time data.
 *
 * jxs_kernel_spec: the canonical description of the flags a kernel of `mode` (JXS_MODE_* below) would be
 *   specialised on, as text "T=float;G=32;MODE=0;P.n_chunks=1,P.seg_steps=4,...".  Host-only (no device
 *   needed).  Returns the length written (excluding the terminator) or a negative error code.
 * jxs_model_attach_specialized: loads a shared object built for exactly that description (checked) and
 *   routes the launches of `mode` for this model through it.  Cached launch graphs are dropped.     */
enum { JXS_MODE_STEP = 0, JXS_MODE_STEP_RIGID = 6 };
int jxs_kernel_spec(const jxs_model_desc* desc, int mode, char* buf, int capacity);
int jxs_model_attach_specialized(jxs_model* model, int mode, const char* shared_object_path);
/* bit `mode` set: launches of that mode use a specialised kernel */
int jxs_model_specialized_modes(const jxs_model* model, unsigned* mask);

/* ---- hot path ------------------------------------------------------------------------- */

/* js.model.step (src/jaxsim/api/model.py:2601-2681): actuation model -> soft contacts ->
 * ABA -> semi-implicit Euler.  state_out may alias state_in (in-place).  `tau` =
 * joint_force_references [n][N] or NULL (zeros); `link_forces` = [nL*6][N] or NULL,
 * expressed in `force_repr` (the data's velocity representation, api/model.py:2641-2646). */
int jxs_step(jxs_model* model, const void* state_in, void* state_out, const void* tau,
             const void* link_forces, int force_repr, int N, void* stream);

/* `n_launches` back-to-back in-place jxs_step launches enqueued from one call (no fusion: one kernel
 * launch per step, exactly what a host loop over jxs_step enqueues, without the per-call cost of the
 * host language).  On a created stream blocks of 250 and of 50 launches are captured once into hipGraphs
 * and replayed while the arguments stay the same; a remainder below 50 is launched plainly (faster to get
 * going than a graph of that size: tools/region_overhead.py).                                   */
int jxs_step_repeat(jxs_model* model, void* state, const void* tau, const void* link_forces,
                    int force_repr, int N, int n_launches, void* stream);

/* jxs_step_repeat bracketed by stream synchronisations on both sides (polling waits) and a host wall clock,
 * all inside one call: the timed region of a benchmark without the interpreter's call overhead inside it
 * (bench.py times its regions of exactly --steps launches with this).  *seconds = wall time of the region. */
int jxs_step_repeat_timed(jxs_model* model, void* state, const void* tau, const void* link_forces,
                          int force_repr, int N, int n_launches, void* stream, double* seconds);

/* `n_steps` consecutive steps with constant inputs in ONE launch sequence (what a
 * `jax.lax.fori_loop` over `step` does in the reference's notebooks); in place.           */
int jxs_rollout(jxs_model* model, void* state, const void* tau, const void* link_forces,
                int force_repr, int N, int n_steps, void* stream);

/* [round 4] `n_steps` consecutive steps with a SEQUENCE of joint torques -- what a `jax.lax.scan` of `step` over
 * precomputed `joint_force_references` does (open-loop rollouts: trajectory sampling, MPPI); in place.
 * `tau_seq` = [n_steps * n][N] in the usual [row][N] convention: rows k*n .. (k+1)*n-1 are the torques of step k
 * (the actuation model is applied to them at every step, like `step`).  `link_forces` stay constant.  Where the
 * steps fuse (semi-implicit Euler, SoftContacts, one chunk of collidable points) this is ONE launch with the state in
 * registers and one torque load per step; otherwise one launch per step, the step's torques gathered by a strided
 * device copy into a scratch block the MODEL owns: unfused controlled rollouts of one model are not re-entrant
 * across streams (use one model handle per stream, as for every call that carries per-model device state).   */
int jxs_rollout_controlled(jxs_model* model, void* state, const void* tau_seq, const void* link_forces,
                           int force_repr, int N, int n_steps, void* stream);

/* [round 4] A rollout that RECORDS: the state block after every step goes to `out_states` = [n_steps * n_rows][N]
 * (rows k*n_rows .. (k+1)*n_rows-1 = the state after step k, the layout of `state`), what `jax.lax.scan` over `step`
 * returns as its stacked outputs; `state` is advanced in place as by jxs_rollout.  `tau`: constant [n][N] or NULL, or
 * -- `tau_per_step` != 0 -- a sequence [n_steps * n][N] as in jxs_rollout_controlled.  Fused into one launch where the
 * steps fuse (one store of the state per step from registers); otherwise one launch and one strided device copy
 * per step.                                                                                     */
int jxs_rollout_recorded(jxs_model* model, void* state, const void* tau, int tau_per_step, const void* link_forces,
                         int force_repr, int N, int n_steps, void* out_states, void* stream);

/* forward_dynamics_aba (src/jaxsim/api/model.py:1269-1406) in inertial representation:
 * out_acc = [6+n][N] = inertial-fixed base acceleration then joint accelerations.
 * `joint_forces` are applied as given (no actuation model), no contact forces.          */
int jxs_forward_dynamics_aba(jxs_model* model, const void* state, const void* joint_forces,
                             const void* link_forces, int force_repr, void* out_acc, int N,
                             void* stream);

/* [round 6] system_dynamics / system_acceleration (src/jaxsim/api/ode.py:16-131,174-225) and link_contact_forces
 * (src/jaxsim/api/contact.py:514-603) -- what the reference's contact-model benchmarks time
 * (tests/test_benchmark.py:103-139) -- in ONE launch: contact forces of the model's contact model (SoftContacts,
 * RigidContacts, RelaxedRigidContacts), summed per link, plus the external `link_forces`, through ABA.  No actuation
 * model (`joint_torques` are applied as given, api/ode.py:117-122), no integrator, no impact.
 *   out_xdot  = [n_rows][N], the layout of the state block, every row holding the time derivative of the state row
 *               it stands for, inertial-fixed like the state: pdot_B = v_W + w x p_B, Qdot (Quaternion.derivative of
 *               the normalised quaternion with the Baumgarte gain `baumgarte`, api/ode.py:136-169; the reference's
 *               default is 1.0), sdot, W_vdot_WB (linear, angular), sddot, and the rate of the tangential deformation
 *               of the enabled points (zero for disabled points and for the rigid contact models).  May be NULL
 *               when only the link wrenches are wanted (SoftContacts then stops before ABA).
 *   out_link_contact_forces = [nL * 6][N] or NULL: the 6D contact wrench of every link, inertial representation
 *               ([f; p_W x f] summed over the link's enabled points, api/contact.py:592-601), rows 6 l .. 6 l + 5.
 * `link_forces` / `force_repr` as in jxs_step.                                                              */
int jxs_system_dynamics(jxs_model* model, const void* state, const void* joint_torques, const void* link_forces,
                        int force_repr, double baumgarte, void* out_xdot, void* out_link_contact_forces, int N,
                        void* stream);
/* link_contact_forces alone (api/contact.py:514-555): jxs_system_dynamics with out_xdot = NULL; `out_mdot`
 * ([3 * n_points][N] or NULL) receives the `m_dot` entry of the reference's aux dictionary for SoftContacts (rows
 * 3 c .. 3 c + 2 = point c; zeros for disabled points and for the rigid contact models).                        */
int jxs_link_contact_forces(jxs_model* model, const void* state, const void* joint_torques, const void* link_forces,
                            int force_repr, void* out_link_contact_forces, void* out_mdot, int N, void* stream);

/* inverse_dynamics / RNEA (src/jaxsim/api/model.py:1746-1894, rbda/rnea.py:12-238) in
 * inertial representation: in_acc = [6+n][N] (base acceleration, joint accelerations) or
 * NULL (zeros => free_floating_bias_forces, :1934-1978); out = [6+n][N] = base wrench then
 * joint torques.                                                                        */
int jxs_inverse_dynamics(jxs_model* model, const void* state, const void* in_acc,
                         const void* link_forces, int force_repr, void* out_forces, int N,
                         void* stream);

/* Layout conversion on the device between an environment-major array `[N][rows]` (row-major, what the
 * reference's vmapped arrays, a NumPy upload or a DLPack / __cuda_array_interface__ buffer of another
 * framework hold) and the tile-interleaved storage every batched argument of this library uses
 * (`jxs_layout.tile`).  The tiled buffer must hold ceil(N / tile) * rows * tile elements.      */
int jxs_tile_from_env_major(const void* src, void* dst, int rows, int N, int tile, int dtype, void* stream);
int jxs_tile_to_env_major(const void* src, void* dst, int rows, int N, int tile, int dtype, void* stream);

/* Value checks of a state block, the counterpart of the host callbacks the reference enables with
 * JAXSIM_ENABLE_EXCEPTIONS (src/jaxsim/exceptions.py:6-60, rbda/utils.py:135-146).  Synchronous.
 * counts3[0] = environments whose base quaternion contains NaN, [1] = environments whose quaternion is
 * not normalised (jnp.allclose(q.q, 1)), [2] = environments with any non-finite state entry.      */
int jxs_validate_state(jxs_model* model, const void* state, int N, int* counts3, void* stream);

/* ---- the episode loop around `step`: reset, pick and flag environments on the device ----------------
 * All three work on the tiled storage [ceil(N / tile)][rows][tile] of any batched argument, are asynchronous on
 * `stream` and neither allocate, synchronise nor read anything on the host: they can sit between two jxs_step
 * launches of a stream in flight.  `dtype` is JXS_F32 or JXS_F64; words are copied as bits.
 *
 * jxs_env_select: out[:, e] = mask[e] ? a[:, e] : b[:, e] for every environment e < N -- the reference's
 *   `jax.tree.map(lambda x, y: jnp.where(done, x, y), fresh, data)` under vmap.  `mask` = N bytes on the device in
 *   environment order, any non-zero byte is true (what a bool array of another framework holds); it is never read
 *   at or beyond N.  The padding columns of the last tile take b's words.  out == b (in-place reset), out == a and
 *   a == b are allowed; any other overlap is not.  In place, a tile whose mask bytes are all zero costs the read
 *   of those bytes only.                                                                                        */
int jxs_env_select(const uint8_t* mask, const void* a, const void* b, void* out, int rows, int N, int tile, int dtype,
                   void* stream);

/* jxs_env_copy: for k < K, environment src_idx[k] of `src` (src_N environments, tiling src_tile) is copied to
 *   environment dst_idx[k] of `dst` (dst_N, dst_tile); a null index array means k itself.  A tiling of 1 IS the
 *   environment-major layout [N][rows], so this one call is the reference's `jax.tree.map(lambda x: x[idx], data)`
 *   (gather into a smaller batch), `x.at[idx].set(y)` (scatter fresh states into a running batch) and both
 *   directions of an exchange with another framework's (K, rows) tensor.  The index arrays live on the device:
 *   every index is checked against src_N / dst_N in the kernel and an entry with either index out of range is
 *   skipped entirely -- nothing outside the two blocks is read or written.  Duplicate destinations leave that one
 *   environment unspecified (one of the sources, or a mixture of their rows) and affect nothing else.  `src` and
 *   `dst` must not overlap.                                                                                      */
int jxs_env_copy(const void* src, int src_N, int src_tile, const int32_t* src_idx, void* dst, int dst_N, int dst_tile,
                 const int32_t* dst_idx, int rows, int K, int dtype, void* stream);

/* jxs_env_flags: one byte per environment into `out_flags` (N bytes on the device), the per-environment form of
 *   jxs_validate_state -- the reference's `jnp.isfinite(x).all()` per vmapped instance, without a download:
 *   bit 0 (JXS_ENV_NONFINITE): some word of the environment is NaN or infinite (the rule of counts3[2]);
 *   bit 1 (JXS_ENV_QUAT_NOT_UNIT): the quaternion holds no NaN and is not of unit norm (the rule of counts3[1]).
 *   A NaN quaternion sets bit 0 only.  The bytes can be handed to jxs_env_select as its mask.                */
enum { JXS_ENV_NONFINITE = 1, JXS_ENV_QUAT_NOT_UNIT = 2 };
int jxs_env_flags(jxs_model* model, const void* state, int N, uint8_t* out_flags, void* stream);

/* jxs_env_randomize: a freshly sampled state into exactly the environments `mask` names (N bytes on the device, any
 *   non-zero byte is true, never read at or beyond N; NULL = every environment), in place on the tile-interleaved block
 *   of `model`'s layout and dtype -- the reference's `jnp.where(done, random_model_data(model, key=k), data)` under vmap
 *   without a `fresh` block.  The other environments and the padding columns of the last tile keep every bit.
 *   `bounds` = [2][12 + 2 n_joints] words of the state's dtype on the device, the row of lower and the row of upper
 *   bounds of the variables: 0-2 base position, 3-5 XYZ Euler angles, 6.. joint positions, then 3 linear and 3 angular
 *   base-velocity components in `velocity_representation` (JXS_REPR_*; stored inertial-fixed; zeros for a fixed base),
 *   then the joint velocities.  The rows behind the joint velocities (tangential deformation) are written as zero.
 *   A value is a function of (seed, draw, first_env + e, variable) alone -- Philox4x32-10 with key = seed and counter =
 *   (first_env + e, variable, draw), csrc/jxs_env_random.h --, never of N, the tiling, the mask or the split of a batch
 *   over processes: a shard passes the global index of its first environment as `first_env` and draws what one big
 *   batch would.  Asynchronous on `stream`; no allocation, synchronisation or host read (legal between two jxs_step
 *   launches and inside a stream capture: a captured graph replays the same `draw`).  JXS_EINVAL: a null model, state
 *   or bounds, N <= 0, first_env < 0, first_env + N > 2^32, an unknown representation, a misaligned block.          */
int jxs_env_randomize(jxs_model* model, const uint8_t* mask, void* state, int N, const void* bounds, uint64_t seed,
                      uint64_t draw, int64_t first_env, int velocity_representation, void* stream);

/* jxs_env_observe: the input of a policy network, an environment-major tensor `out` = [N][out_ld], assembled on the
 *   device from the tiled state block and up to four further tiled blocks [rows_s][N] of the state's dtype and tile (the
 *   centroidal record, frame records, gravity torques, link contact wrenches, last step's torques ...) -- what the
 *   reference's user gets from `jnp.concatenate` of `data.joint_positions`, `data.base_orientation`, `data.base_velocity`
 *   ... under vmap (src/jaxsim/api/data.py:267-312, inertial_to_other_representation of api/common.py:100-158).
 *   The observation is described once per model by an immutable table of D slots (1 <= D <= JXS_OBS_MAX_WIDTH), slot d =
 *   {kind, source, index} with `offset[d]` and `scale[d]` (NULL: zeros / ones; rounded to the model's dtype): word d of
 *   environment e is (x - offset[d]) * scale[d], two roundings in the state's dtype, with x by kind:
 *     JXS_OBS_STATE_ROW          word `index` of the environment's state rows (jxs_layout order)
 *     JXS_OBS_SOURCE_ROW         row `index` of block `source` (0 .. 3), which has `source_rows[source]` rows
 *     JXS_OBS_BASE_QUAT_UNIT     component `index` (w x y z) of q / |q|; a zero quaternion stays as it is
 *     JXS_OBS_BASE_ROTATION      entry `index` (0 .. 8, row-major) of the rotation matrix of q / |q|
 *     JXS_OBS_BASE_VELOCITY      component `index` (0-2 linear, 3-5 angular) of the base velocity in the launch's
 *                                `velocity_representation` (JXS_REPR_*; the state stores it inertial-fixed)
 *     JXS_OBS_PROJECTED_GRAVITY  component `index` of R^T (0, 0, -1)
 *   jxs_observation_create refuses with JXS_EINVAL: D outside its range, an unknown kind, a row, component or source out
 *   of range (a source whose `source_rows` entry is <= 0 does not exist; NULL `source_rows`: none does), an offset or
 *   scale that is not finite in the model's dtype.  A table may be used with every model of the same state layout and dtype.
 *   jxs_env_observe writes columns < D of rows < N of `out` and nothing else: with out_ld > D a caller fills a slice of a
 *   wider tensor.  `out_dtype` is JXS_F32 or the model's dtype (an fp64 state is rounded once, at the store).  The four
 *   source pointers travel by value; one the table does not use may be NULL.  Padding columns of the last tile are
 *   never read as environments and no source is read beyond its storage.  Asynchronous on `stream`; no allocation,
 *   synchronisation, memset or host read (legal between two jxs_step launches and inside a stream capture).  JXS_EINVAL:
 *   a null model, table, state or out, N <= 0, out_ld < D, an unknown representation or out_dtype, a used source whose
 *   pointer is NULL, a table of another layout or dtype, a misaligned block.                                            */
#define JXS_OBS_MAX_WIDTH 4096
enum {
  JXS_OBS_STATE_ROW = 0,
  JXS_OBS_SOURCE_ROW = 1,
  JXS_OBS_BASE_QUAT_UNIT = 2,
  JXS_OBS_BASE_ROTATION = 3,
  JXS_OBS_BASE_VELOCITY = 4,
  JXS_OBS_PROJECTED_GRAVITY = 5
};
typedef struct jxs_observation jxs_observation;
int jxs_observation_create(jxs_model* model, int D, const int32_t* slots /* [D][3] */, const double* offset,
                           const double* scale, const int32_t source_rows[4], jxs_observation** out);
int jxs_observation_destroy(jxs_observation* observation);
int jxs_env_observe(jxs_model* model, const jxs_observation* observation, const void* state,
                    const void* const sources[4], int N, int velocity_representation, void* out, int out_dtype,
                    int64_t out_ld, void* stream);

/* jxs_env_act: the joint torques of a policy's action, the tiled [n][N] block `out_tau` that jxs_step reads as `tau`,
 *   computed on the device from the environment-major action tensor `actions` = [N][act_ld] and the joint positions and
 *   velocities of the tiled state block -- what the reference's user writes as the controller that a `jax.lax.scan` of
 *   `step` carries under `vmap`: scaled position or velocity targets turned into torques by a PD law at the physics rate,
 *   from the q and qdot of every sub-step between two policy evaluations.
 *   The law is described once per model by an immutable table of n entries, one per joint in the order of the state's
 *   joint rows: `joints` [n][2] = {mode, column} and `params` [n][8] = {scale, offset, kp, kd, action_clip, target_lo,
 *   target_hi, torque_limit} (rounded to the model's dtype).  With clamp(x, lo, hi) = x < lo ? lo : (hi < x ? hi : x) --
 *   a NaN x passes through -- the word of joint j of environment e is, every operation rounded in the model's dtype:
 *     a   = column < 0 ? 0 : actions[e][column]
 *     u   = clamp(a, -action_clip, action_clip) * scale + offset
 *     t   = JXS_ACT_OFF       0
 *           JXS_ACT_TORQUE    u
 *           JXS_ACT_POSITION  kp * (clamp(u, target_lo, target_hi) - q_j) - kd * qdot_j
 *           JXS_ACT_VELOCITY  kd * (u - qdot_j)
 *     t   = feed_forward ? t + feed_forward[j][e] : t
 *     tau = clamp(t, -torque_limit, torque_limit)
 *   JXS_ACT_POSITION with column -1 holds `offset`.  `feed_forward` is NULL or a tiled [n][N] block of the model's dtype
 *   and tile (what jxs_gravity_torques writes).
 *   jxs_action_create refuses with JXS_EINVAL: a model without joints, A outside [0, JXS_ACT_MAX_WIDTH], an unknown mode, a
 *   column outside [-1, A), a scale, offset, kp or kd that is not finite in the model's dtype, an action_clip or
 *   torque_limit that is negative, NaN or finite but not in the model's dtype (+inf: no limit), target_lo > target_hi or
 *   NaN (infinities allowed).  A table may be used with every model of the same state layout and dtype.
 *   jxs_env_act: `act_ld` >= A; `act_dtype` is JXS_F32 or the model's dtype; `actions` may be NULL exactly when no joint
 *   has a column.  Every word of `out_tau` of an environment < N is written, the padding columns of the last tile are
 *   written as zero, nothing else is written.  Action columns the table does not name and the gap A .. act_ld-1 may hold
 *   anything; no action row at or beyond N is read; padding columns of the state and of `feed_forward` never reach a
 *   word of a real environment.  Asynchronous on `stream`; no allocation, synchronisation, memset or host read (legal
 *   between two jxs_step launches).  JXS_EINVAL: a null model, table, state or out_tau, N <= 0, act_ld < A, an unknown
 *   act_dtype, NULL actions while a column is used, a table of another layout or dtype, a misaligned block.            */
#define JXS_ACT_MAX_WIDTH 4096
enum { JXS_ACT_OFF = 0, JXS_ACT_TORQUE = 1, JXS_ACT_POSITION = 2, JXS_ACT_VELOCITY = 3 };
typedef struct jxs_action jxs_action;
int jxs_action_create(jxs_model* model, int A, const int32_t* joints /* [n][2] = mode, column */,
                      const double* params /* [n][8] */, jxs_action** out);
int jxs_action_destroy(jxs_action* action);
int jxs_env_act(jxs_model* model, const jxs_action* action, const void* state, const void* actions, int act_dtype,
                int64_t act_ld, const void* feed_forward, void* out_tau, int N, void* stream);

/* jxs_env_evaluate: the reward and the termination flags of a policy step, one launch that writes per environment e < N
 *   `reward[e]` (one word of `reward_dtype`, contiguous) and `done[e]` (one byte: bit 0 JXS_DONE_TERMINATED, bit 1
 *   JXS_DONE_TRUNCATED -- directly the `mask` of jxs_env_select and jxs_env_randomize), and optionally `fired[e]` (uint32,
 *   bit c: condition c fired), `terms` = [N][terms_ld] (the K per-term contributions, environment-major, of `terms_dtype`)
 *   and the in/out episode counter `steps[e]` (int32) -- what the reference's user writes as a reward function and a done
 *   predicate over `data.base_position`, `data.joint_positions`, `data.base_velocity` ... under vmap.  With it
 *   act -> step x k -> evaluate -> jxs_env_randomize(done) -> observe needs no host trip.
 *   The law is described once per model by an immutable table (jxs_evaluation_desc).  It has D slots (1 <= D <=
 *   JXS_EVAL_MAX_SLOTS), each {kind, source, index} with `offset[d]` and `scale[d]` exactly as a slot of jxs_env_observe
 *   (NULL: zeros / ones), and each optionally with a target {source, row} in `targets` [D][2] (source -1, or NULL
 *   `targets`: none), the commanded value of the environment, read from a source block.  Every operation is rounded on its
 *   own in the model's dtype:
 *     x_d = target ? raw_d - source[row][e] : raw_d
 *     y_d = (x_d - offset[d]) * scale[d]
 *   Every slot belongs to exactly one term or one condition.  Term t (0 <= K <= JXS_EVAL_MAX_TERMS), `terms` [K][4] =
 *   {first, count, inner, outer} and `term_params` [K][3] = {weight, lo, hi}, owns the slots first .. first + count - 1:
 *     v_d = JXS_EVAL_IDENTITY y_d | JXS_EVAL_ABS |y_d| | JXS_EVAL_SQUARE y_d * y_d | JXS_EVAL_EXCESS max(|y_d| - 1, 0)
 *     s_t = v_first, then s_t = s_t + v_d in slot order
 *     o_t = JXS_EVAL_OUTER_IDENTITY s_t | JXS_EVAL_OUTER_EXP exp(-s_t)       (the accurate exponential of the dtype)
 *     p_t = clamp(weight * o_t, lo, hi)       (clamp(x, lo, hi) = x < lo ? lo : (hi < x ? hi : x): a NaN stays a NaN)
 *   (JXS_EVAL_EXCESS with offset = the centre and scale = 1 / half-width of a window measures how far a value lies outside
 *   it, in half-widths: joint limits.)  Then r = p_0, r = r + p_t in term order (K = 0: r = 0), r = clamp(r, reward_lo,
 *   reward_hi).  Condition c (0 <= C <= JXS_EVAL_MAX_CONDITIONS), `conditions` [C][2] = {slot, kind} and
 *   `condition_limits` [C][2] = {lo, hi}, fires when !(lo <= y && y <= hi) -- a NaN fires; either limit may be infinite --
 *   and sets the bit of its kind (JXS_EVAL_TERMINATED, JXS_EVAL_TRUNCATED) in `done` and bit c in `fired`.  With `steps`
 *   non-NULL (then max_steps > 0): n = steps[e] + 1; n >= max_steps sets JXS_DONE_TRUNCATED (and no bit of `fired`);
 *   steps[e] = done ? 0 : n -- an environment flagged done starts its next episode at zero, since the caller resets it
 *   with that same mask.  Last, bit 0 of done adds `termination_reward` to r.
 *   jxs_evaluation_create refuses with JXS_EINVAL: D, K or C outside their ranges, an unknown kind, inner, outer or
 *   condition kind, a row, component, source or target out of range (`source_rows` as for jxs_observation_create), an
 *   empty term, overlapping slot ranges, a slot of no term and no condition or of two, an offset, scale, weight or
 *   termination_reward that is not finite in the model's dtype, lo > hi or a NaN limit (infinities allowed).  A table may
 *   be used with every model of the same state layout and dtype.
 *   jxs_env_evaluate writes reward[0 .. N), done[0 .. N), fired[0 .. N), steps[0 .. N) and columns < K of rows < N of
 *   `terms`, each only when its pointer is non-NULL, and nothing else; at least one of `reward` and `done` is non-NULL.
 *   `reward_dtype` and `terms_dtype` are JXS_F32 or the model's dtype.  Padding columns of the last tile are never read
 *   and no source is read beyond its storage.  Asynchronous on `stream`; no allocation, synchronisation, memset or host
 *   read (legal between two jxs_step launches and inside a stream capture).  JXS_EINVAL: a null model, table or state,
 *   NULL reward and done, N <= 0, terms_ld < K, an unknown representation or dtype, `steps` with max_steps <= 0, a used
 *   source whose pointer is NULL, a table of another layout or dtype, a misaligned block.                             */
#define JXS_EVAL_MAX_SLOTS 1024
#define JXS_EVAL_MAX_TERMS 32
#define JXS_EVAL_MAX_CONDITIONS 32
#define JXS_DONE_TERMINATED 1
#define JXS_DONE_TRUNCATED 2
enum { JXS_EVAL_IDENTITY = 0, JXS_EVAL_ABS = 1, JXS_EVAL_SQUARE = 2, JXS_EVAL_EXCESS = 3 };
enum { JXS_EVAL_OUTER_IDENTITY = 0, JXS_EVAL_OUTER_EXP = 1 };
enum { JXS_EVAL_TERMINATED = 0, JXS_EVAL_TRUNCATED = 1 };
typedef struct jxs_evaluation_desc {
  int32_t D, K, C;
  const int32_t* slots;           /* [D][3] = kind, source, index (JXS_OBS_*) */
  const int32_t* targets;         /* [D][2] = source, row; source -1: none; may be NULL */
  const double* offset;           /* [D], may be NULL */
  const double* scale;            /* [D], may be NULL */
  const int32_t* terms;           /* [K][4] = first, count, inner, outer */
  const double* term_params;      /* [K][3] = weight, lo, hi */
  const int32_t* conditions;      /* [C][2] = slot, kind */
  const double* condition_limits; /* [C][2] = lo, hi */
  double reward_lo, reward_hi, termination_reward;
  int32_t source_rows[4];
} jxs_evaluation_desc;
typedef struct jxs_evaluation jxs_evaluation;
int jxs_evaluation_create(jxs_model* model, const jxs_evaluation_desc* desc, jxs_evaluation** out);
int jxs_evaluation_destroy(jxs_evaluation* evaluation);
int jxs_env_evaluate(jxs_model* model, const jxs_evaluation* evaluation, const void* state,
                     const void* const sources[4], int N, int velocity_representation, void* reward, int reward_dtype,
                     uint8_t* done, uint32_t* fired, void* terms, int terms_dtype, int64_t terms_ld, int32_t* steps,
                     int max_steps, void* stream);

/* jxs_env_contacts: contact sensors of a legged robot, one launch that turns the link kinematics of jxs_refresh_kinematics
 *   (`link_transforms` [nL*12][N], `link_velocities` [nL*6][N], tiled) into a tiled record `out_record` [G*8][N] per group of
 *   points -- foot contact, clearance, slip, air time -- laid out as a source block of jxs_env_observe and jxs_env_evaluate,
 *   so that contact flags in the observation, a feet-air-time reward, a foot-slip penalty and a "trunk touched the ground"
 *   termination need no host trip.  The reference's user writes these over `js.contact.in_contact` and
 *   `js.contact.collidable_point_kinematics` under vmap.
 *   The sensors are described once per model by an immutable table (jxs_contact_sensors_create): P entries (1 <= P <=
 *   JXS_CONTACT_MAX_POINTS), entry k = {parent_link[k], L_p[k][3]}, in G groups (1 <= G <= JXS_CONTACT_MAX_GROUPS), `groups`
 *   [G][2] = {first, count >= 1}, whose ranges are disjoint and cover every entry; a point wanted in two groups is listed
 *   twice.  Per environment and entry, with [R|t] and (v, w) of its parent link, every operation rounded on its own in the
 *   model's dtype:
 *     p  = ((R[:,0] x + R[:,1] y) + R[:,2] z) + t,  pd = v + w x p     (src/jaxsim/api/contact.py:18-45,
 *                                                                       src/jaxsim/rbda/collidable_points.py:9-65)
 *     h  = height(p_x, p_y) of the model's own terrain, with the operations of the step kernel: flat `terrain_height`; plane
 *          terrain_height - (n_x p_x + n_y p_y) * (1 / n_z); height field the bilinear interpolant clamped to the border
 *          samples (src/jaxsim/terrain/terrain.py:15-238)
 *     c  = p_z - h; the point is in contact when c <= 0 (src/jaxsim/api/contact.py:92-145); a NaN clearance is no contact
 *     s  = |pd - (pd . n) n|^2 with n the terrain normal (flat: pd_x^2 + pd_y^2; height field: the central-difference
 *          normal of src/jaxsim/terrain/terrain.py:40-62, the one place with a reciprocal square root); 0 with NULL
 *          `link_velocities`
 *   Group g owns rows 8 g + JXS_CONTACT_* of the record:
 *     FLAG 1 if any point of the group is in contact, else 0;  COUNT the number of points in contact;
 *     CLEARANCE m = c_first, then m = c_k < m ? c_k : m in entry order;  SLIP_SQ the largest s_k over the points in
 *     contact, 0 if none;  AIR_TIME a';  CONTACT_TIME b';  TOUCHDOWN 1 if in contact now and a > 0;  FLIGHT_TIME a if
 *     touchdown, else 0: the length of the flight that just ended.
 *   `timers` [G*2][N] (tiled, in/out; a of group g at row 2 g, b at 2 g + 1): an environment whose `reset_mask` byte is
 *   non-zero takes a = b = 0 first -- the mask is the `done` of jxs_env_evaluate as it is --, then a' = contact ? 0 : a + dt
 *   and b' = contact ? b + dt : 0.  With NULL `timers` rows 4-7 are 0 and nothing is carried.  The feet-air-time reward
 *   sum (flight - 0.5) touchdown is two terms of jxs_env_evaluate over source rows: weight * sum FLIGHT_TIME and
 *   -0.5 weight * sum TOUCHDOWN.
 *   jxs_contact_sensors_create refuses with JXS_EINVAL: G or P outside their ranges, an empty group, one outside the table
 *   or overlapping an earlier one, an entry of no group, a parent link outside [0, nL), an L_p that is not finite in the
 *   model's dtype.  A table may be used with every model of the same layout, link count and dtype.
 *   jxs_env_contacts writes every word of `out_record` of an environment < N, the padding columns of its last tile as zero,
 *   and `timers` for environments < N only; the mask and the blocks are never read for padding columns.  Asynchronous on
 *   `stream`; no allocation, synchronisation, memset or host read (legal inside a stream capture).  JXS_EINVAL: a null
 *   model, table, link_transforms or out_record, N <= 0, dt negative or not finite, a table of another model layout or
 *   dtype, a misaligned block.                                                                                          */
#define JXS_CONTACT_MAX_POINTS 1024
#define JXS_CONTACT_MAX_GROUPS 32
#define JXS_CONTACT_ROWS 8
#define JXS_CONTACT_TIMER_ROWS 2
enum {
  JXS_CONTACT_FLAG = 0,
  JXS_CONTACT_COUNT = 1,
  JXS_CONTACT_CLEARANCE = 2,
  JXS_CONTACT_SLIP_SQ = 3,
  JXS_CONTACT_AIR_TIME = 4,
  JXS_CONTACT_CONTACT_TIME = 5,
  JXS_CONTACT_TOUCHDOWN = 6,
  JXS_CONTACT_FLIGHT_TIME = 7
};
typedef struct jxs_contact_sensors jxs_contact_sensors;
int jxs_contact_sensors_create(jxs_model* model, int G, const int32_t* groups /* [G][2] */, int P,
                               const int32_t* parent_link /* [P] */, const double* L_p /* [P][3] */,
                               jxs_contact_sensors** out);
int jxs_contact_sensors_destroy(jxs_contact_sensors* sensors);
int jxs_env_contacts(jxs_model* model, const jxs_contact_sensors* sensors, const void* link_transforms,
                     const void* link_velocities, int N, double dt, const uint8_t* reset_mask, void* timers,
                     void* out_record, void* stream);

/* RigidContacts only.  A contact-force QP or an impact solve whose result is not finite (fp32 on a numerically
 * singular stance) is DISCARDED -- that environment takes the step without contact forces / without the
 * velocity reset instead of poisoning its state -- where the reference would propagate NaN
 * (src/jaxsim/rbda/contacts/rigid.py:331-379).  The discards are counted per model: counts2[0] = contact-force
 * solves, counts2[1] = impact solves, in environments, since the last reset.  Synchronous.          */
int jxs_solver_fault_counts(jxs_model* model, int* counts2, int reset, void* stream);

/* [round 4] jxs_step with tau_ref + g(q): the joint part of free_floating_gravity_forces (src/jaxsim/api/model.py:1897-1931)
 * of the INPUT state is added to the joint force references inside the step kernel -- the controller loop
 *     tau = js.model.free_floating_gravity_forces(model, data)[6:] (+ tau_user);  data = js.model.step(model, data, joint_force_references=tau)
 * (BASELINE config 5) in one launch instead of two.  `tau` may be null (pure gravity compensation) or hold tau_user.
 * Models with a rigid contact model (RigidContacts / RelaxedRigidContacts and enabled points) only: JXS_EINVAL otherwise.      */
int jxs_step_gravity_compensated(jxs_model* model, const void* state_in, void* state_out, const void* tau,
                                 const void* link_forces, int force_repr, int N, void* stream);

/* Developer knobs of the launcher (JXS_DUO, JXS_DUO_MAX_BLOCKS, JXS_NO_MFMA, JXS_DISABLE_COMMON_VARIANT: A/B switches
 * between kernel variants that compute the same thing) are read from the environment once per process, at the first
 * launch.  This call reads them again -- for test programs that switch variants between launches.  No reference
 * counterpart (XLA flags are read once too).                                                          */
int jxs_debug_reload_env(void);

/* Gravity compensation torques: the joint part of free_floating_gravity_forces
 * (src/jaxsim/api/model.py:1897-1931: RNEA at zero velocity, zero acceleration, no external forces),
 * written as [n][N] -- the layout jxs_step reads `tau` in, so a controller loop
 * "tau = g(q); step(tau)" (BASELINE.json config 5) stays on the device.                     */
int jxs_gravity_torques(jxs_model* model, const void* state, void* out_tau, int N, void* stream);

/* free_floating_mass_matrix (src/jaxsim/api/model.py:1553-1590, rbda/crba.py:10-170): the composite-rigid-body
 * algorithm, one launch.  out_M = [(6+n)*(6+n)][N], row-major (row r, column c at row index r*(6+n)+c), in
 * MIXED velocity representation (base block about the base position, world axes); the Body / Inertial forms
 * are the 6x6 block congruence of api/model.py:1529-1551 applied by the caller.                  */
int jxs_mass_matrix(jxs_model* model, const void* state, void* out_M, int N, void* stream);

/* free_floating_mass_matrix_inverse (src/jaxsim/api/model.py:1593-1631, rbda/mass_inverse.py:11-233): the columns
 * are the responses of the articulated-body factorisation to unit generalized forces, one launch.  Same
 * layout and representation (MIXED) as jxs_mass_matrix; the six base rows / columns of a fixed-base model are
 * zero (a fixed base does not accelerate).                                                       */
int jxs_mass_matrix_inverse(jxs_model* model, const void* state, void* out_Minv, int N, void* stream);

/* Centroidal momentum, CoM and energies, one launch (jaxsim.api.com: com_position, com_linear_velocity,
 * centroidal_momentum, centroidal_momentum_jacobian, locked_centroidal_spatial_inertia, average_centroidal_velocity
 * (_jacobian), src/jaxsim/api/com.py; jaxsim.api.model: total_momentum(_jacobian), locked_spatial_inertia,
 * average_velocity(_jacobian), kinetic_energy, potential_energy, mechanical_energy, src/jaxsim/api/model.py:1988-2175,
 * 2397-2453).  One leaves-to-root sweep of the composite inertia, subtree momentum and subtree kinetic energy
 * (rbda/crba.py:10-170).  G[W] = (W_p_CoM, world axes); the generalized velocity is the stored one, the base velocity of
 * a fixed-base model included (like the reference's).
 *   out_record = [JXS_CENTROIDAL_ROWS][N]:
 *     rows  0.. 2  JXS_CENTROIDAL_COM        W_p_CoM (as the cached link transforms place the links)
 *     rows  3.. 8  JXS_CENTROIDAL_MOMENTUM   centroidal momentum h_G in G[W]: linear; angular about the CoM
 *     rows  9..14  JXS_CENTROIDAL_INERTIA    rotational inertia I_G about the CoM, world axes: xx, xy, xz, yy, yz, zz.
 *                                            The locked centroidal inertia in G[W] is diag(m 1, I_G) -- for a model
 *                                            whose base link has a translated pose (suc_H_i[0] = (1, d)) the CoM of
 *                                            the dynamics sits at W_p_CoM - R_B d: blocks m S(e)^T, I_G + m S(e) S(e)^T
 *                                            with e = -R_B d, as the reference's congruence gives
 *     rows 15..20  JXS_CENTROIDAL_AVG_VEL    average centroidal velocity in G[W]: linear (= CoM velocity); angular
 *     row  21      JXS_CENTROIDAL_KINETIC    kinetic energy 1/2 nu^T M nu
 *     row  22      JXS_CENTROIDAL_POTENTIAL  potential energy AS THE REFERENCE COMPUTES IT: m z_CoM gravity with
 *                                            gravity = -9.81, i.e. -m g z (so K - U, not K + U, is conserved)
 *     row  23      JXS_CENTROIDAL_MASS       total mass
 *   out_cmm = [6*(6+n)][N] or NULL: the centroidal momentum matrix A_G in G[W] (row r, column c at row index
 *     r*(6+n)+c), for the generalized velocity in MIXED representation; the other representations are the 6x6
 *     input / output transforms of api/com.py applied by the caller.
 * Every entry of both outputs is written by the kernel: no allocation, no memset, no host synchronisation (legal
 * inside a stream capture).                                                                         */
#define JXS_CENTROIDAL_COM 0
#define JXS_CENTROIDAL_MOMENTUM 3
#define JXS_CENTROIDAL_INERTIA 9
#define JXS_CENTROIDAL_AVG_VEL 15
#define JXS_CENTROIDAL_KINETIC 21
#define JXS_CENTROIDAL_POTENTIAL 22
#define JXS_CENTROIDAL_MASS 23
#define JXS_CENTROIDAL_ROWS 24
int jxs_centroidal(jxs_model* model, const void* state, void* out_record, void* out_cmm, int N, void* stream);

/* free_floating_coriolis_matrix (src/jaxsim/api/model.py:1634-1745): C(q, nu) with C nu = h - g and Mdot - 2C
 * skew-symmetric, equal entry by entry to the reference's sum over the links, one launch (a leaves-to-root sweep of the
 * composite inertia and of sum (v_L x*) M_L).  out_C = [(6+n)*(6+n)][N], row-major (the layout of
 * jxs_mass_matrix), in MIXED velocity representation; out_M = NULL or the Mixed mass matrix of the same launch, equal to
 * jxs_mass_matrix's.  As in the reference the generalized velocity of a fixed-base model includes its stored base
 * velocity.  Body / Inertial are T^T (M Tdot + C T) with T = diag(X, 1), v_mixed = X v_repr, applied by the caller.
 * Refused with JXS_EINVAL: a null out_C, model or state, N <= 0.  Both outputs are zeroed with hipMemsetAsync, nothing
 * is allocated and the host does not wait (legal inside a stream capture).                               */
int jxs_coriolis(jxs_model* model, const void* state, void* out_C, void* out_M, int N, void* stream);

/* forward_dynamics_crb (src/jaxsim/api/model.py:1409-1498): same arguments, layout and meaning as
 * jxs_forward_dynamics_aba; M nu_dot = B tau - h + J^T f solved by CRBA + tree-sparse LtDL, one launch.  M (the
 * composite-inertia sweep of jxs_mass_matrix) and its factor stay in the LDS, the right-hand side is one RNEA pass at zero
 * acceleration with the link wrenches applied (h as free_floating_bias_forces: a fixed base drops its stored base
 * velocity).  Like the reference's CRB path the link wrenches act through the link Jacobians: for a model whose base link
 * has a pose offset, Body / Mixed wrenches are applied at the link frame of the dynamics, not of the cached kinematics
 * (where jxs_forward_dynamics_aba converts them).  out_acc = [6+n][N]: inertial-fixed base acceleration (exactly zero for
 * a fixed base), then the joint accelerations; every entry is written by the kernel -- no memset, nothing is allocated
 * and the host does not wait (legal inside a stream capture).  Refused with JXS_EINVAL: a null out_acc, model or state,
 * N <= 0.                                                                                                              */
int jxs_forward_dynamics_crb(jxs_model* model, const void* state, const void* joint_forces, const void* link_forces,
                             int force_repr, void* out_acc, int N, void* stream);

/* Frames: poses, velocities, bias accelerations and Jacobians of frames rigidly attached to links, one launch
 * (jaxsim.api.link: transform, velocity, jacobian, bias_acceleration; jaxsim.api.frame: transform, velocity, jacobian;
 * jaxsim.api.model.link_bias_accelerations, src/jaxsim/api/model.py:2179-2395).  A target is (parent link L, L_H_F); a
 * link is the target (L, identity).  The link bias accelerations are one ancestor prefix sum of v_i x vJ_i at zero joint
 * acceleration, started from the zero base acceleration of the INPUT representation converted to inertial-fixed.
 * jxs_frames_create uploads an immutable target table (refused with JXS_EINVAL: n < 1, n > JXS_FRAME_MAX_TARGETS, a
 * parent outside [0, nL), a last row of L_H_F other than [0 0 0 1]); one table serves every launch and stream of its
 * model, and one specialised MODE_FRAMES kernel serves every table.
 * jxs_frame_kinematics, for the generalized velocity in representation in_repr (I) and outputs in out_repr (O), both
 * JXS_REPR_* (0 Inertial, 1 Body, 2 Mixed):
 *   out_record = [n * JXS_FRAME_ROWS][N], target t at rows t * JXS_FRAME_ROWS + ...:
 *     rows  0..11  JXS_FRAME_POSE  W_H_F as [R|p], 3 x 4 row-major (the pose of the cached link kinematics)
 *     rows 12..17  JXS_FRAME_VEL   O_v_WF = O_J_WF_I I_nu
 *     rows 18..23  JXS_FRAME_BIAS  O_vdot_bias_WF = O_Jdot_WF_I I_nu (for a link and I = O: link_bias_accelerations)
 *   out_J = [n * 6 * (6+n_joints)][N] or NULL: O_J_WF_I of target t, row r, column c at row index
 *     (t * 6 + r) * (6+n_joints) + c; exact zeros in the columns of the joints that do not support L.
 * As in the reference, the stored base velocity of a fixed-base model is part of the generalized velocity.  Every entry of
 * both outputs is written by the kernel: no allocation, no memset, no host synchronisation (legal inside a stream
 * capture).                                                                                        */
#define JXS_FRAME_POSE 0
#define JXS_FRAME_VEL 12
#define JXS_FRAME_BIAS 18
#define JXS_FRAME_ROWS 24
#define JXS_FRAME_MAX_TARGETS 4096
typedef struct jxs_frames jxs_frames;
int jxs_frames_create(jxs_model* model, int n, const int32_t* parent_link, const double* L_H_F /* [n][16] */, jxs_frames** out);
int jxs_frames_destroy(jxs_frames* frames);
int jxs_frame_kinematics(jxs_model* model, const jxs_frames* frames, const void* state, int in_repr, int out_repr,
                         void* out_record, void* out_J, int N, void* stream);

/* jacobian_full_doubly_left + jacobian_derivative_full_doubly_left (src/jaxsim/rbda/jacobian.py:128-339), one
 * launch: out_J = [2*6*(6+n)][N] = B_J_full_WX_B (6 x (6+n), row-major) followed by B_Jdot_full_WX_B, both with
 * input and output in the base frame ("doubly left"); out_B_H_L = [nL*12][N] rows of [R|p] of every link
 * relative to the base, or NULL.  The link Jacobians / their derivatives in any pair of representations are
 * the column masks and 6x6 transforms of api/model.py:925-1228 applied by the caller.             */
int jxs_jacobian_full(jxs_model* model, const void* state, void* out_J, void* out_B_H_L, int N, void* stream);

/* The cached kinematics of JaxSimModelData.replace (src/jaxsim/api/data.py:405-523,
 * rbda/forward_kinematics.py:12-113): link transforms [nL*12][N] (rows of [R|p]) and
 * inertial-fixed link velocities [nL*6][N]; either output may be NULL.                  */
int jxs_refresh_kinematics(jxs_model* model, const void* state, void* out_link_transforms,
                           void* out_link_velocities, int N, void* stream);

/* ---- multi-GPU: one process per GPU, batch sharded, no per-step communication ---------
 * One RCCL all-gather over xGMI concatenates the final state shards (SURVEY.md section
 * 8(e)); the reference has no counterpart (single-device JAX).  The 128-byte unique id is
 * created on rank 0 and distributed by the host launcher (torch.distributed / MPI / file). */
int jxs_comm_unique_id(char id[128]);
int jxs_comm_init(void** comm, const char id[128], int rank, int world_size);
int jxs_comm_destroy(void* comm);
/* [round 5] what a scaling record must be able to say about its communicator: the version of the RCCL library the
 * ranks talk through (ncclGetVersion: e.g. 22107) and the PCI bus id of the device a rank runs on ("0000:05:00.0";
 * buf of at least 16 bytes) -- bench.py puts both into its line and refuses a run whose communicator is not RCCL
 * when asked to (--require-rccl).  */
int jxs_comm_version(int* version);
int jxs_device_pci_bus_id(char* buf, int len);
/* recv[world][rows][n_local]  <-  send[rows][n_local] of every rank */
int jxs_allgather(void* comm, const void* send, void* recv, uint64_t count, int dtype,
                  void* stream);

#ifdef __cplusplus
}
#endif
#endif /* JAXSIM_AMD_H */
