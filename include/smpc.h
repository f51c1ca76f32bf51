/*
 * smpc.h -- C ABI of the MI355X batched safe-MPC engine.
 *
 * This is the drop-in boundary for ONE path of idra-lab/safe-mpc: everything at and below
 * AbstractController.solve() (reference src/safe_mpc/controller.py:136-167), i.e. what the reference
 * reaches through acados_template.AcadosOcpSolver (controller.py:247) -- batched over independent OCP
 * instances.  Plain pointers and sizes only; no torch / numpy types.  The same structs are mirrored with
 * ctypes in safe_mpc_amd/problem.py and are also read by the test oracle (oracle/), which shares this
 * interface and nothing else with the product.
 *
 * Conventions
 *   - all arrays are row-major and laid out exactly like the reference's numpy arrays:
 *       x0 [B][nx], x_guess [B][N+1][nx], u_guess [B][N][nu], p [B][N+1][5]   (guess_acados.py:236,
 *       controller.py:147-156); nx = 2*nq, nu = nq, p = [ee_ref(3), alpha, flag] (controller.py:27-31).
 *   - every entry point returns 0 on success and a negative SMPC_E* code on API misuse / HIP failure.
 *     The numerical outcome of each instance is reported only through status[B], using the acados codes the
 *     reference tests against (0 ok, 1 NaN, 2 max-iter, 3 min-step, 4 QP failure; controller.py:125,158).
 *   - a handle is bound to one device and one stream, owns all device scratch, and is not thread-safe.  Scratch grows in
 *     eager calls: a call that would grow it while the handle's stream is being captured into a hipGraph returns SMPC_ESTATE.
 */
#ifndef SMPC_H_
#define SMPC_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SMPC_ABI_VERSION 5

#define SMPC_MAX_NQ 7
#define SMPC_MAX_NX 14
#define SMPC_MAX_POINTS 12
#define SMPC_MAX_ROWS 12
#define SMPC_MAX_LAYERS 6
#define SMPC_MAX_N 63
#define SMPC_NP 5 /* per-node parameter vector length */

/* bounds with |value| >= SMPC_INF are treated as absent (the reference writes 1e6 for "no upper bound",
 * env_model.py:265-266, safe_set.py:104) */
#define SMPC_INF 1.0e5

/* error codes */
#define SMPC_OK 0
#define SMPC_EINVAL (-1)
#define SMPC_ENOMEM (-2)
#define SMPC_EHIP (-3)
#define SMPC_ESTATE (-4)

/* acados status codes reproduced per instance */
#define SMPC_STATUS_SUCCESS 0
#define SMPC_STATUS_NAN 1
#define SMPC_STATUS_MAXITER 2
#define SMPC_STATUS_MINSTEP 3
#define SMPC_STATUS_QP_FAILURE 4

/* One actuated revolute joint and the (lumped) link it moves.  Replaces the adam KinDynComputations model the
 * reference builds from the URDF (env_model.py:40-45).  Links reached through fixed / locked joints are lumped
 * into `mass, com, inertia` by the host (safe_mpc_amd/urdf.py). */
typedef struct {
    double R0[9];      /* parent-link frame -> joint frame rotation at q = 0, row-major (URDF origin rpy) */
    double p0[3];      /* ... and translation (URDF origin xyz) */
    double axis[3];    /* unit axis in the joint (= child link) frame */
    double mass;       /* lumped mass of the child link */
    double com[3];     /* lumped centre of mass, child-link frame */
    double inertia[6]; /* ixx ixy ixz iyy iyz izz about the COM, child-link axes */
    double q_min, q_max, v_max, tau_max; /* URDF <limit> (env_model.py:107-114) */
} smpc_joint;

/* A point rigidly attached to the child link of actuated joint `link` (link = -1: fixed in the world). */
typedef struct {
    int32_t link;
    int32_t reserved;
    double local[3];
} smpc_point;

/* kinds of collision rows (env_model.py:263-316) */
#define SMPC_ROW_SEG_FIXEDSEG 0 /* capsule-capsule, second capsule fixed (utils.py:94-113) */
#define SMPC_ROW_SEG_SEG 1      /* capsule-capsule, both on the robot */
#define SMPC_ROW_SEG_POINT 2    /* capsule-sphere (utils.py:115-118) */
#define SMPC_ROW_POINT_POINT 3  /* sphere-sphere on the EE point (env_model.py:300-301) */
#define SMPC_ROW_COORD 4        /* plane: coordinate of a robot point (env_model.py:286-287, utils.py:123-124) */

typedef struct {
    int32_t kind;
    int32_t pa, pb; /* robot points: segment A-B, or the single point pa */
    int32_t pc, pd; /* second robot segment (SEG_SEG) */
    int32_t axis;   /* COORD: 0/1/2 */
    double C[3];    /* fixed segment start / fixed point */
    double D[3];    /* fixed segment end */
    double len2;    /* SEG_POINT: capsule_length**2 used as denominator (utils.py:116) */
    double offset;  /* COORD: value = P[axis] - offset */
    double lb, ub;  /* lh, uh of this row */
} smpc_row;

#define SMPC_COST_ZERO 0  /* ZeroCost (cost_definition.py:34-46) */
#define SMPC_COST_REACH 1 /* ReachTargetEXT / ReachTargetNLS (cost_definition.py:61-100) */

#define SMPC_HESS_GAUSS_NEWTON 0 /* NONLINEAR_LS */
#define SMPC_HESS_EXACT 1        /* EXTERNAL + hessian_approx EXACT (cost_definition.py:18,100) */

#define SMPC_NN_NONE 0
#define SMPC_NN_TERMINAL 1 /* ST / HTWA / RealReceding: node N only (controller.py:332-357) */
#define SMPC_NN_ALL 2      /* Receding / constraint_everywhere: nodes 1..N, switched by p[4] (controller.py:411-442) */

typedef struct {
    int32_t abi_version;
    int32_t nq;
    int32_t N;
    int32_t n_points;
    int32_t n_rows;
    int32_t ee_point;          /* index of the EE point (env_model.py:92-95) */
    int32_t cost_kind;
    int32_t hessian;
    int32_t nn_mode;
    int32_t nn_dof;            /* n_dof_safe_set (config.yaml:11) */
    int32_t qp_max_iter;       /* qp_solver_iter_max (config.yaml:18) */
    int32_t rows_at_node0;     /* != 0: the collision rows are kept at node 0, as the reference does when --noise == 0
                                * (controller.py:77-79; removed for noisy runs, :69-73).  x_0 is pinned, so they are
                                * constants of the QP: a violated one makes the QP infeasible and the instance reports
                                * SMPC_STATUS_QP_FAILURE (the iterate is still returned, as acados does) */
    int32_t qp_stall_iters;    /* > 0: the IPM gives up (SMPC_STATUS_QP_FAILURE, the iterate is still returned) after this many
                                * CONSECUTIVE stalled iterations -- step length below 1/2 AND the complementarity not halved
                                * either (an iterate that meets the exit test is never a stall) -- or after 7/6 of that many in
                                * total (round 5: 24 -> 28; infeasible QPs whose complementarity falls in bursts reset the run
                                * and took up to 52 iterations, now 31, with no feasible QP more given up).  0 = off: an infeasible QP then runs
                                * until its step length underflows (40-90 iterations: what RealReceding's +-1e-3 tubes,
                                * controller.py:531-532, produce in about 1 % of its solves).  A stall is not a proof of
                                * infeasibility -- a feasible, degenerate QP can crawl for 20 iterations before it converges
                                * (tests/golden/c4_degenerate_start.npz) -- hence an option with a generous default where it is
                                * switched on (24 for 'real_receding' and for the backup OCP, problem.py) and none elsewhere */
    int32_t reserved_i0;
    double dt;                 /* config.yaml:7 */
    double Q, R;               /* config.yaml:35,39 */
    double cost_scale_stage;   /* factor on the cost Q|ee-ref|^2 + R|u|^2 whose derivatives smpc_node_eval reports: acados
                                * multiplies stage costs by dt and the terminal one by 1 [EXT-UNVERIFIED]; a NONLINEAR_LS cost
                                * is 1/2 |y|^2_W (cost_definition.py:61-81), i.e. a further factor 1/2 on both */
    double cost_scale_term;
    double lm_stage;           /* Levenberg-Marquardt added to every diagonal of the stage Hessian */
    double lm_term;
    double nn_eps;             /* config.yaml:48 */
    double nn_soft_e;          /* L1 slack weight on the terminal NN row (zl_e, controller.py:348-354); < 0 = hard */
    double nn_soft_run;        /* same for running nodes; < 0 = hard */
    double qp_tol;             /* IPM exit tolerance on the complementarity (mean lambda t) */
    double qp_tol_res;         /* ... and on the linear residuals (stationarity, dynamics, slack definitions); 0 = qp_tol.
                                * HPIPM's BALANCE mode (config.yaml:15) asks 1e-6 of the stationarity residual and 1e-8 of the
                                * others [EXT-UNVERIFIED]; the engine's default is 1e-8 for both */
    double qp_mu0;             /* IPM initial barrier */
    double gravity[3];
    double nn_mean[SMPC_MAX_NQ];
    double nn_std[SMPC_MAX_NQ];
    double x_lo[SMPC_MAX_NX];   /* lbx / ubx of nodes 1..N-1 (controller.py:49-51) */
    double x_hi[SMPC_MAX_NX];
    double x_lo_e[SMPC_MAX_NX]; /* lbx_e / ubx_e (controller.py:53-55, 300-306) */
    double x_hi_e[SMPC_MAX_NX];
    smpc_joint joints[SMPC_MAX_NQ];
    smpc_point points[SMPC_MAX_POINTS];
    smpc_row rows[SMPC_MAX_ROWS];
} smpc_problem_desc;

/* Per-(instance, node) linearisation record returned by smpc_eval_nodes; one per node k = 0..N.
 * Exposes what acados evaluates through the CasADi-generated functions (N2 in SURVEY section 2) so that each piece
 * can be compared with the oracle separately. */
typedef struct {
    double tau[SMPC_MAX_NQ];                       /* M(q)u + h(q,qd) (env_model.py:80-83) */
    double M[SMPC_MAX_NQ * SMPC_MAX_NQ];           /* dtau/du, row-major nq x nq (leading dim nq) */
    double dtau_dq[SMPC_MAX_NQ * SMPC_MAX_NQ];
    double dtau_dv[SMPC_MAX_NQ * SMPC_MAX_NQ];
    double ee[3];                                  /* t_glob (env_model.py:92-95) */
    double cost_grad_q[SMPC_MAX_NQ];               /* d/dq of Q*|ee - ref|^2 (unscaled) */
    double cost_hess_qq[SMPC_MAX_NQ * SMPC_MAX_NQ];/* exact or Gauss-Newton, unscaled, row-major */
    double row_val[SMPC_MAX_ROWS];                 /* collision rows */
    double row_grad[SMPC_MAX_ROWS * SMPC_MAX_NQ];  /* d row / dq, row-major n_rows x nq */
    double nn_val;                                 /* g(x,p) (safe_set.py:94), 0 if not evaluated */
    double nn_grad[SMPC_MAX_NX];                   /* dg/dx */
} smpc_node_eval;

typedef struct smpc_handle smpc_handle;

/* ---- lifetime ------------------------------------------------------------------------------------------------- */
/* replaces AcadosOcpSolver(ocp, json_file, generate, build) (controller.py:247); device = HIP device ordinal */
int smpc_create(const smpc_problem_desc* desc, int device, smpc_handle** out);
void smpc_destroy(smpc_handle* h);
int smpc_abi_version(void);
/* last error text of this handle (or of the failed smpc_create when h == NULL) */
const char* smpc_last_error(const smpc_handle* h);

/* replaces l4c.L4CasADi(model_net, device='cpu') + model_external_shared_lib_* (safe_set.py:89-94,
 * controller.py:344-346): fp32 weights W[l] is [dims[l+1]][dims[l]] row-major (torch nn.Linear.weight), b[l] is
 * [dims[l+1]]; activation between layers is GELU(tanh) (parser.py:99), none after the last.  Pointers may be host or
 * device memory (on_device != 0: e.g. torch.Tensor.data_ptr() of a ROCm tensor); the handle keeps its own copy. */
int smpc_set_mlp(smpc_handle* h, int nlayers, const int32_t* dims, const float* const* W, const float* const* b,
                 int on_device);
/* the activation between the layers: parser.py:95-102 (`act_fun` of config.yaml:67); GELU(tanh) unless set */
enum { SMPC_ACT_GELU_TANH = 0, SMPC_ACT_RELU = 1, SMPC_ACT_ELU = 2, SMPC_ACT_TANH = 3, SMPC_ACT_SILU = 4 };
int smpc_set_mlp_activation(smpc_handle* h, int act);

/* replaces ocp_solver.set_new_time_steps + update_qp_solver_cond_N (controller.py:208-209): change N without
 * re-creating; N <= SMPC_MAX_N */
int smpc_set_horizon(smpc_handle* h, int N);

/* Which form of the QP solve a handle launches -- the engine's counterpart of the reference's choice of QP back-end
 * (`ocp.solver_options.qp_solver`, controller.py:100-101: partial- or full-condensing HPIPM; `qp_solver_cond_N`, controller.py:209).
 * Same algorithm and the same result to rounding either way; only the mapping onto the GPU differs:
 *   SMPC_QP_AUTO (default)  by batch size: the latency form for small batches, the throughput form otherwise
 *   SMPC_QP_THROUGHPUT      k_qp_ipm: one wavefront per pair of instances
 *   SMPC_QP_LATENCY         k_qp_ipm_wg: one workgroup per instance, stage-parallel row work, recursions through LDS
 *                           (falls back to the throughput form when a horizon's factor blocks do not fit one CU's LDS)
 * (added in round 6; ABI version unchanged: no existing entry point or structure changed) */
enum { SMPC_QP_AUTO = -1, SMPC_QP_THROUGHPUT = 0, SMPC_QP_LATENCY = 1 };
int smpc_set_qp_mode(smpc_handle* h, int mode);

/* The crew of the throughput form: a k_qp_ipm launch over P = ceil(B / 2) pairs of instances runs G = ceil(fraction * P) wavefronts,
 * which take the pairs longest-expected-first from a ticket -- the first G at once, the others as wavefronts come free.  fraction = 1
 * is a wavefront per pair.  waves > 0 fixes G itself (clamped to P) and fraction is ignored.  Scheduling only: every instance's
 * arithmetic, and so every result, is the same for every crew.  The latency form is not affected. */
int smpc_set_qp_crew(smpc_handle* h, double fraction, int waves);

/* replaces ocp_solver.constraints_set(k,'lbx'/'ubx',v) for k >= 1 (controller.py:531-536).  lo/hi are [N+1][nx]
 * shared by all instances, or NULL to restore the descriptor's bounds. */
int smpc_set_stage_bounds(smpc_handle* h, const double* lo, const double* hi);

/* Per-instance variant for RealReceding's state tube (controller.py:530-536: node r of instance b is boxed to
 * x_guess[b][r+1] +- 1e-3 with its own r): lo/hi are [B][N+1][nx]; they apply to the next smpc_solve_batch calls with the
 * same B until cleared with lo = hi = NULL.  Pointers follow on_device like smpc_solve_batch; the handle keeps a copy. */
int smpc_set_instance_bounds(smpc_handle* h, int B, const double* lo, const double* hi, int on_device);

/* A scene of its own for every instance: where each collision row's FIXED obstacle sits in the world, per instance.  Geometry only:
 * the rows themselves stay shared -- kinds, robot points, len2, bounds lb / ub and every check bound come from the descriptor
 * (the bounds lb / ub have a slot of their own: smpc_set_instance_row_bounds).
 * geom is [B][n_rows][SMPC_SCENE_ROW] doubles, one 64-byte record {C[3], D[3], offset, 0} per (instance, row), of which a row
 * reads by kind
 *   SMPC_ROW_SEG_FIXEDSEG  C, D (the fixed capsule's end points)      SMPC_ROW_SEG_POINT, _POINT_POINT  C (the fixed point)
 *   SMPC_ROW_COORD         offset (value = P[axis] - offset)          SMPC_ROW_SEG_SEG                  nothing
 * and the rest is ignored.  The handle keeps a copy (stream-ordered; with host pointers the call waits for it like
 * smpc_set_instance_bounds), geom == NULL clears the scene.
 * While a scene is set, every entry point that evaluates collision rows uses it: smpc_solve_batch, smpc_eval_nodes,
 * smpc_merit_terms, smpc_sqp_batch, smpc_check_guess, smpc_ik_batch, smpc_check_trajectory, smpc_score_rollout, smpc_policy_step
 * (kinds 0-4) and smpc_loop_post.  The scene belongs to ITS batch size: a call of these with another B returns SMPC_EINVAL and names both sizes --
 * it never falls back to the descriptor's obstacles, which would solve in the wrong world without a word.  Clear the scene (or set
 * one of the new size) first.  SMPC_POLICY_PARALLEL (its candidate slots are not instances) and smpc_rollout_batch (its worker
 * handles hold no scene) return SMPC_ESTATE while a scene is set.  Without a scene every entry point launches the kernels it
 * launched before the scene existed.
 * SMPC_EINVAL: B <= 0, a descriptor without rows, or (host pointers only) a non-finite value in a field that is read.
 * SMPC_ESTATE: the copy would have to grow while the stream is being captured.
 * (ABI version unchanged: no existing entry point or structure changed) */
#define SMPC_SCENE_ROW 8   /* doubles per (instance, row): C[3], D[3], offset, 0 */
int smpc_set_instance_scene(smpc_handle* h, int B, const double* geom, int on_device);

/* Obstacles that move along the horizon: a TRACK of scenes per instance.  geom is [B][T][n_rows][SMPC_SCENE_ROW] doubles, one scene
 * record (as above) per (instance, time column, row); memory 64 * n_rows * T * B bytes.  What a scene does not carry, a track does
 * not carry either.  THE column rule: the scene at time c is column
 *     col(c) = clamp(c, 0, T - 1)
 * -- before the track's first column the world stands as in column 0, behind its last as in column T - 1.  With t = the value of
 * the scene clock when a kernel runs (smpc_set_scene_clock; 0 without one):
 *   smpc_solve_batch, smpc_eval_nodes, smpc_merit_terms, smpc_sqp_batch, smpc_check_guess, smpc_check_trajectory,
 *   smpc_debug_stage_records, and the solve and the x_temp test of smpc_policy_step (kinds 0-4):   node k in column col(t + k)
 *   smpc_loop_post (its one node is the plant's NEXT state):                                       column col(t + 1)
 *     (of the WORLD, with the world's T, while one is set: smpc_set_instance_world_track below)
 *   smpc_ik_batch:                                                                                 column col(t)
 *   smpc_score_rollout (the log starts at time 0, the clock is not read):                          state j of the log in col(j)
 * A track and a scene are ONE slot of the handle: setting one replaces the other, smpc_set_instance_scene(h, B, geom, ..) is exactly
 * a track with T = 1, and smpc_set_instance_scene(h, 0, NULL, 0) clears a track too (as geom == NULL does here).  Everything said
 * of a scene holds: the copy is stream-ordered and a call with host pointers checks the fields that the row kinds read for
 * non-finite values and waits; the track belongs to its batch size (another B: SMPC_EINVAL naming both); SMPC_POLICY_PARALLEL and
 * smpc_rollout_batch return SMPC_ESTATE.  SMPC_EINVAL also for T < 1.  SMPC_ESTATE: the copy would have to grow while the stream is
 * being captured (the old contents stay).
 * (ABI version unchanged: no existing entry point or structure changed) */
int smpc_set_instance_scene_track(smpc_handle* h, int B, int64_t T, const double* geom, int on_device);

/* The time of node 0, for a track: d_clock is a DEVICE pointer to ONE int64 that the caller owns and keeps alive; NULL = time 0.
 * The cell is read on the device when a kernel runs -- no host synchronisation, and a captured graph replays with whatever the cell
 * holds then; smpc_loop_state.step is the intended cell.  It is read by the kernels that read a scene track with T > 1 and by the
 * network pass of a context track with T > 1 (smpc_set_instance_context_track); without either, or with T = 1, the clock is not
 * read.  The clock stays set across smpc_set_instance_scene / _track and smpc_set_instance_context / _track calls until it is
 * replaced or cleared here. */
int smpc_set_scene_clock(smpc_handle* h, const int64_t* d_clock);

/* The WORLD: a track that only the plant meets.  geom is [B][T][n_rows][SMPC_SCENE_ROW], exactly a scene
 * track's layout and validation (host pointers are checked for non-finite values in the fields the row kinds read and the call
 * waits for the copy, device pointers are taken as they are).  It is a slot of the handle under the one slot rule: it belongs to its
 * batch size, the same (B, T) is overwritten in place, growth while the stream is being captured is SMPC_ESTATE with the old contents
 * kept, and geom == NULL clears it.  Clearing the world also clears a scene slot that holds a forecast and a context the forecast
 * wrote, and the observed track (below): a forecast or an observation without its world is stale.
 * Who reads the world: smpc_forecast_scene and smpc_forecast_scene_fit (below; in the modes HOLD and CV and in the fit only while
 * no observed track is set, see smpc_set_instance_observed_track), and smpc_loop_post, whose one node -- the plant's NEXT state --
 * is tested in column col(t + 1) of the WORLD instead of the scene slot while a world is set (col with the world's T, t the scene
 * clock).
 * smpc_loop_post with another B: SMPC_EINVAL naming both sizes.  Nothing else reads it; in particular the x_temp test of
 * smpc_policy_step keeps reading the scene slot, which is what the controller believes.
 * SMPC_EINVAL: B <= 0, T < 1, a descriptor without rows, or (host pointers only) a non-finite value in a field that is read.
 * (ABI version unchanged: no existing entry point or structure changed) */
int smpc_set_instance_world_track(smpc_handle* h, int B, int64_t T, const double* geom, int on_device);

/* A FORECAST of the horizon's N + 1 scenes, formed on the device from what the world has shown up to the clock, into the scene
 * slot.  Enqueue-only on the handle's stream once its buffers exist.  With W the world (in the modes HOLD and CV: the observed
 * track of smpc_set_instance_observed_track while one is set -- what the controller has seen of the world), T its columns, t the scene clock's cell when
 * the kernel runs (0 without a clock, held to +-2^62), col THE column rule with W's T, c0 = col(t), c1 = col(t - 1) and N the
 * handle's horizon, for every instance b, row r and all eight slots s of the record:
 *   SMPC_FORECAST_HOLD  F[b][k][r][s] = W[b][c0][r][s], k = 0..N                      (the frozen world)
 *   SMPC_FORECAST_CV    d = W[b][c0][r][s] - W[b][c1][r][s];  F[b][0] = W[b][c0],  F[b][k] = F[b][k-1] + d, k = 1..N
 *                       -- repeated addition in this order, no multiplication; c0 == c1 (t <= 0, t >= T, T = 1) gives d = 0
 *   SMPC_FORECAST_TRUE  F[b][k] = W[b][col(t + k)]                                    (the clairvoyant arm of a study)
 * F replaces whatever the scene slot held, as a track of N + 1 columns for B instances.  While the slot holds a forecast it is read
 * FROM TIME 0, whatever the clock says (the launchers hand the kernels no clock, as for T = 1): node k of the solves and tests of
 * the scene track's table reads column clamp(k, 0, N), smpc_ik_batch column 0, smpc_score_rollout column col(j) as for any track
 * (re-set the slot to the world before scoring a log).  smpc_set_instance_scene / _track replace the forecast and return the slot to
 * clocked reading; smpc_set_horizon drops a forecast (it is laid out by N); SMPC_POLICY_PARALLEL and smpc_rollout_batch refuse
 * the slot as they refuse any scene.
 * Context rows: select is n_sel HOST pairs (row, slot) -- which number of the scene each context input of the network is.  With
 * n_sel > 0 the call also writes the context slot, [B][N+1][n_ctx] fp32, from the same F:
 *   ctx[b][k][i] = (float)((F[b][k][row_i][slot_i] - ctx_mean[i]) / ctx_std[i])
 * read from time 0 like the forecast scene, replaced and re-clocked by smpc_set_instance_context / _track, dropped with the
 * forecast.  The pairs travel with the launch (no device copy is kept, so a captured call carries its own).  With n_sel == 0 the
 * context slot is left alone.
 * SMPC_EINVAL (the message names the call and, where sizes disagree, both): B differs from the world's; unknown mode; an observed
 * track whose (B, T) is not the world's; n_sel > 0 with
 * a network without context columns or with n_sel != n_ctx; a pair outside n_rows x SMPC_SCENE_ROW; n_sel > 0 with select == NULL.
 * SMPC_ESTATE: no world set, or the scene or context buffer would have to grow while the stream is being captured.
 * A refused call leaves the slot contents in force.
 * (ABI version unchanged: no existing entry point or structure changed) */
enum { SMPC_FORECAST_HOLD = 0, SMPC_FORECAST_CV = 1, SMPC_FORECAST_TRUE = 2 };
int smpc_forecast_scene(smpc_handle* h, int B, int mode, int n_sel, const int32_t* select);

/* What the controller OBSERVES of the world: geom is [B][T][n_rows][SMPC_SCENE_ROW], and layout, validation,
 * the slot rule, host and device pointers and growth under capture (SMPC_ESTATE, the old contents kept) are exactly the world
 * track's.  A slot of its own; geom == NULL clears it, and so does clearing the world (an observation without its world is stale).
 * Who reads it, while it is set: smpc_forecast_scene in the modes HOLD and CV, INSTEAD of the world (same column rule, same clock),
 * smpc_forecast_scene_fit and smpc_forecast_scene_poly.  SMPC_FORECAST_TRUE and smpc_loop_post keep reading the world; nothing else
 * reads the observed track.
 * Call the table those forecasts read S, "what was seen": the observed track while one is set, else the world.
 * A forecast call while an observed track is set needs its (B, T) to equal the world's: SMPC_EINVAL naming both otherwise.
 * (ABI version unchanged: no existing entry point or structure changed) */
int smpc_set_instance_observed_track(smpc_handle* h, int B, int64_t T, const double* geom, int on_device);

/* A forecast by a LINE FIT over the last `window` samples of S.  Every rule of smpc_forecast_scene holds (enqueue-only once its
 * buffers exist; needs a world, of B instances; F replaces the scene slot as a track of N + 1 columns read from time 0; n_sel and
 * select mean and are refused the same, and write the context rows; the slot then "holds a forecast" exactly as after
 * smpc_forecast_scene; a refused call changes nothing), and SMPC_EINVAL also for window < 1 or window > SMPC_FIT_MAX, naming it.
 * With t the scene clock's cell when the kernel runs (0 without a clock, held to +-2^62), col THE column rule with S's T,
 * m = min(window, max(t, 0) + 1) -- nothing has been seen before time 0 -- and y_j = S[b][col(t - j)][r][s], j = 0..m-1, for every
 * instance b, row r and all eight slots s:
 *   u_j = (double)(4m - 2 - 6j)    / (double)(m (m + 1))
 *   w_j = (double)(6(m - 1) - 12j) / (double)(m (m^2 - 1))                               (m = 1: w_0 = 0)
 *   a = u_0 y_0;  a = a + u_j y_j   (j = 1..m-1, in this order, every product rounded before its sum)
 *   d = w_0 y_0;  d = d + w_j y_j   (likewise)
 *   F[b][0] = a,  F[b][k] = F[b][k-1] + d,  k = 1..N                                     (repeated addition, as SMPC_FORECAST_CV)
 * a is the least-squares line's value now and d its slope per column.  window = 1 is SMPC_FORECAST_HOLD; window = 2 gives
 * u = (1, 0), w = (1, -1), hence a = y_0, d = y_0 - y_1: SMPC_FORECAST_CV bit for bit at every clock.  Behind the track's last
 * column the clamped samples make the slope decay to zero within `window` steps.
 * (ABI version unchanged: no existing entry point or structure changed) */
#define SMPC_FIT_MAX 32
int smpc_forecast_scene_fit(smpc_handle* h, int B, int window, int n_sel, const int32_t* select);

/* A forecast by a least-squares POLYNOMIAL of degree 0, 1 or 2 over the last `window` samples of S.  Every
 * rule, refusal, flag and state of smpc_forecast_scene_fit holds -- it is the same code, with this call's name in the message -- and
 * SMPC_EINVAL also for degree < 0 or degree > 2, naming it.  t, col, m = min(window, max(t, 0) + 1) and y_j = S[b][col(t - j)][r][s]
 * as there; the effective degree is p = min(degree, m - 1): nothing was seen before time 0, so one sample gives a constant and two
 * give a line.  The model is y(tau) = a + b tau + c tau^2 at tau = -j.  For every instance b, row r and all eight slots s:
 *   p = 0   u_j = 1.0 / (double)m;  a = u_0 y_0;  a = a + u_j y_j  (j = 1..m-1, every product rounded before its sum)
 *           F[b][k] = a, k = 0..N                 (stored, not added: a -0.0 stays one).  The window mean; m = 1: SMPC_FORECAST_HOLD
 *   p = 1   smpc_forecast_scene_fit with window m, bit for bit: degree == 1 launches that call's kernel
 *   p = 2   ua_j = (double)(3(3m^2 - 3m + 2) - 18(2m - 1) j + 30 j^2)                         / (double)(m (m + 1)(m + 2))
 *           uv_j = (double)((36m^3 - 96m^2 + 36m + 24) + (-192m^2 + 180m + 48) j + 180 m j^2) / (double)(m (m^2 - 1)(m^2 - 4))
 *           ue_j = (double)(60 ((m - 1)(m - 2) - 6(m - 1) j + 6 j^2))                         / (double)(m (m^2 - 1)(m^2 - 4))
 *           (integers formed in 64 bits, ONE correctly rounded division each; m = 3: ua = (1, 0, 0), uv = (2, -3, 1), ue = (1, -2, 1))
 *           a, v, e each  x = u_0 y_0;  x = x + u_j y_j   (in increasing j, every product rounded before its sum)
 *           F[b][0] = a;  for k = 1..N:  F[b][k] = F[b][k-1] + v;  v = v + e              (in that order; repeated addition)
 * a is the parabola's value now, v = b + c its first step F[1] - F[0] and e = 2c the step of the step: a constant-acceleration
 * model.  degree 2 with window 2 is SMPC_FORECAST_CV and degree 0 with window 1 SMPC_FORECAST_HOLD, bit for bit at every clock.
 * (ABI version unchanged: no existing entry point or structure changed) */
int smpc_forecast_scene_poly(smpc_handle* h, int B, int window, int degree, int n_sel, const int32_t* select);

/* Row bounds per instance and node: how much room a collision row leaves, along the horizon (obstacle inflation).  lo and hi are
 * [B][N+1][n_rows] doubles, N the handle's horizon at the call; entry (b, k, r) REPLACES rows[r].lb / .ub of the descriptor for node k
 * of instance b wherever the OCP's own row bounds are read: the row's lo = lb - v and hi = ub - v of the QP, the rows_at_node0
 * infeasibility test (the only reader of node 0) and the rows' l1 violation of the merit.  A value with |v| >= SMPC_INF is an
 * absent side, as in the descriptor.  The table is read along the horizon from node 0, like a forecast in the scene slot: it needs no
 * clock, and it is independent of the scene, world, observed and context slots (smpc_forecast_scene leaves it in force).
 *   reads it, and guards its B (another B: SMPC_EINVAL naming the call, both sizes and this setter):
 *       smpc_solve_batch, smpc_sqp_batch, smpc_merit_terms, smpc_policy_step kinds 0-4 (the solve only), smpc_debug_stage_records
 *   does not read it -- what counts as a collision stays physical, the caller's check bounds:
 *       smpc_check_trajectory, smpc_check_guess, smpc_score_rollout, smpc_loop_post, smpc_ik_batch, the x_temp test of smpc_policy_step
 *   refuses it (SMPC_ESTATE while it is set, whatever its B): SMPC_POLICY_PARALLEL and smpc_rollout_batch
 * The handle keeps a copy (stream-ordered; with host pointers the call waits for it, device pointers are taken as they are).  The
 * same B is overwritten in place, so a captured solve keeps seeing the buffer and replays with the new table; lo == hi == NULL clears
 * it; smpc_set_horizon drops it (it is laid out by N), as it drops the instance bounds.  A refused call changes nothing.
 * SMPC_EINVAL: B <= 0, a descriptor without rows, exactly one of the two pointers NULL, or (host pointers only) a NaN, or lo > hi
 * where both sides are present -- the message names (b, k, r).
 * SMPC_ESTATE: the copy would have to grow while the stream is being captured (the old table stays in force).
 * (ABI version unchanged: no existing entry point or structure changed) */
int smpc_set_instance_row_bounds(smpc_handle* h, int B, const double* lo, const double* hi, int on_device);

/* The row-bounds table formed ON THE DEVICE from the residuals of a fit: a prediction interval per instance, row and node (DESIGN.md
 * section 9r).  Enqueue-only once the slot's buffer has its size.  Reads S ("what was seen": the observed track while one is set, else
 * the world) and the scene clock exactly as smpc_forecast_scene_poly does -- t, col, m = min(window, max(t, 0) + 1),
 * p = min(degree, m - 1), y_j = S[b][col(t - j)][r][s] and a, v, e are that call's, the same operations in the same order -- and is
 * meant to follow a forecast with the same window and degree; it neither needs nor touches the scene slot.  For instance b and row r:
 *   moving slots  SMPC_ROW_SEG_FIXEDSEG: 0..5;  SMPC_ROW_SEG_POINT, _POINT_POINT: 0..2;  SMPC_ROW_COORD: 6;  SMPC_ROW_SEG_SEG: none (d = 0)
 *   nu = m - p - 1.   nu >= 1:  per moving slot, in increasing j:  f_j = a  |  a - j v  |  (a - j v) + (j (j + 1) / 2) e   (p = 0 | 1 | 2)
 *                               res = y_j - f_j;   q = res res at j = 0,  q = q + res res afterwards;   rss = the largest q over the
 *                               moving slots, a NaN winning;   s2 = rss / (double)nu,  raised to sigma_prior^2 where it is below it
 *                               (a NaN stays)
 *                     nu == 0:  s2 = sigma_prior^2  (nothing can be estimated)
 *   h_k = sum_j c_kj^2  (increasing j from the j = 0 term),  c_kj = 1.0 / (double)m  |  u_j + k w_j  |  (ua_j + k uv_j) + (k (k - 1) / 2) ue_j
 *         with the weights of smpc_forecast_scene_fit / _poly: no "+ 1" under the root, the true obstacle carries no noise
 *   d_k = (base_a + base_b k) + (z sqrt(s2)) sqrt(h_k),   d_k = d_k <= d_max ? d_k : d_max       (a NaN in the window gives the cap)
 * every product rounded before its sum.  The table is what smpc_set_instance_row_bounds would be handed for these margins: a plane row
 * gets lb + d_k and ub - d_k, any other row (sqrt(lb) + d_k)^2, a side with |v| >= SMPC_INF stays absent, and where d_k == 0.0 the
 * descriptor's own lb and ub.  It fills the slot of smpc_set_instance_row_bounds for B under that slot's rules: the same size is
 * overwritten in place, so a captured [forecast; margin; solve] replays with the clock; smpc_set_horizon drops it;
 * SMPC_POLICY_PARALLEL and smpc_rollout_batch keep refusing the slot.  A refused call changes nothing.
 * SMPC_ESTATE: no world is set; the buffer would have to grow while the stream is being captured.
 * SMPC_EINVAL: B is not the world's; an observed track of another shape than the world's; window outside 1..SMPC_FIT_MAX; degree
 * outside 0..2; z, sigma_prior, base_a, base_b or d_max negative or not finite (the message names it); a d_max with which a plane
 * row's two sides would cross, lb + d_max > ub - d_max (the message names the row); a descriptor without rows.
 * (ABI version unchanged: no existing entry point or structure changed) */
int smpc_forecast_row_margin(smpc_handle* h, int B, int window, int degree, double z, double sigma_prior, double base_a, double base_b,
                             double d_max);

/* The row-bounds table as the slot holds it: lo and hi receive [B][N+1][n_rows] doubles each.  Stream-ordered with device pointers;
 * with host pointers the call waits for the copy.  SMPC_ESTATE while no table is set, SMPC_EINVAL for another B than the table's or a
 * NULL pointer.  What a test or a study reads the margins of a step with. */
int smpc_get_instance_row_bounds(smpc_handle* h, int B, double* lo, double* hi, int on_device);

/* Obstacle forecasts from a Kalman filter.  One filter per (instance, row) RECORD over all eight slots of a scene
 * record with the record's gains; time is in columns.  The model: degree p in 0..2 (constant, constant velocity, constant acceleration;
 * only components 0..p of a record are used), q >= 0 the process noise, r > 0 the sensor noise in metres, v0, a0 >= 0 the prior standard
 * deviations of velocity and acceleration, beta in [0, 1] the rate of the innovation scale.
 *   transition   pos' = (pos + vel) + 0.5 acc,  vel' = vel + acc,  acc' = acc;   Phi = ((1, 1, 1/2), (0, 1, 1), (0, 0, 1))
 *   process      Q = q^2 G G',  G = (1) | (1/2, 1) | (1/6, 1/2, 1);  formed on the host as gq_i = q G_i, Q_ij = gq_i gq_j
 * The state lives in CALLER-OWNED device memory, [B][n_rows][SMPC_KALMAN_REC] doubles (the engine keeps no filter state, as it keeps no
 * policy or loop state), a record being  pos[8] | vel[8] | acc[8] | P00 P01 P02 P11 P12 P22 | s2 | n;  all zero means "nothing seen".
 * A record is OBSERVED at a step when none of the moving slots of its row kind (smpc_forecast_row_margin lists them) holds a NaN in
 * S[b][col(t)][r]; a SMPC_ROW_SEG_SEG row always is.
 *   advance, n < 1    observed: pos = y, vel = acc = 0, P = diag(r^2, v0^2, a0^2), s2 = 1, n = 1;   unobserved: the record stays
 *   advance, n >= 1   predict x- = Phi x, P- = Phi P Phi' + Q (first the rows of Phi P, then times Phi', then + Q);
 *                     observed: S = P-00 + r^2, inv = 1.0 / S (the one division), K_i = P-0i inv; per slot nu = y - pos-, x_i = x-_i + K_i nu;
 *                       P_ij = P-ij - K_i P-0j (i <= j); nis = the largest (nu nu) inv over the moving slots from 0, a NaN winning;
 *                       s2 = s2 + beta (nis - s2), then 1 where it is below 1;  n = n + 1
 *                     unobserved: x = x-, P = P-; s2 and n stay
 *   forecast          p = 0: F[k] = pos (stored);  p = 1: F[0] = pos, F[k] = F[k-1] + vel;
 *                     p = 2: v = vel + 0.5 acc, F[0] = pos, then F[k] = F[k-1] + v; v = v + acc
 * every product rounded before its sum: problem.kalman_statement is the definition, and the kernel repeats it bit for bit. */
#define SMPC_KALMAN_REC 32
typedef struct {
    int32_t degree, reserved;
    double q, r, v0, a0, beta;
} smpc_kalman_params;

/* One step of the filter (advance != 0) and its forecast over the handle's horizon, written into the scene slot -- and the context slot
 * with n_sel > 0 -- under every rule of smpc_forecast_scene: room first and launch last, growth under capture is SMPC_ESTATE with nothing
 * changed, the slot then holds a forecast (read from time 0).  Enqueue-only, so [kalman; margin; solve] can be captured: a replay is
 * one more advance.  state: DEVICE [B][n_rows][SMPC_KALMAN_REC], updated in place.
 *   advance != 0   reads S (the observed track while one is set, else the world) at the scene clock: needs the world, B the world's
 *                  and an observed track of the world's shape, as smpc_forecast_scene_fit does.
 *   advance == 0   forecasts from the state as it is: reads no table, needs no world and takes any B > 0 -- what a second handle with
 *                  another horizon calls on rows of the controller's state.
 * SMPC_EINVAL, naming the argument: degree outside 0..2; r not finite or <= 0; q, v0 or a0 negative or not finite; beta outside [0, 1];
 * par or state NULL; B <= 0; a descriptor without rows; n_sel / select as for smpc_forecast_scene.  A refused call changes nothing, the
 * state included.  (ABI version unchanged: no existing entry point or structure changed) */
int smpc_forecast_scene_kalman(smpc_handle* h, int B, const smpc_kalman_params* par, double* state, int advance, int n_sel,
                               const int32_t* select);

/* The row-bounds table from the filter's covariance: reads P and s2 of state (DEVICE [B][n_rows][SMPC_KALMAN_REC]) and nothing else --
 * no world, no clock, not the scene slot.  Pi_0 = P, Pi_k = Phi Pi_{k-1} Phi' + Q, g_k = sqrt(Pi_k[0][0]) (no + r^2: the true obstacle
 * carries no noise);  d_k = (base_a + base_b k) + (z sqrt(s2)) g_k,  d_k = d_k <= d_max ? d_k : d_max  (a NaN gives the cap);  d = 0 for
 * a row without a moving slot.  The table is what smpc_forecast_row_margin writes for these d, and it fills the slot of
 * smpc_set_instance_row_bounds under that slot's rules.  problem.kalman_margin_statement is the definition.
 * SMPC_EINVAL: the model as above; z, base_a, base_b or d_max negative or not finite; a d_max with which a plane row's sides would
 * cross; a descriptor without rows; B <= 0; par or state NULL.  SMPC_ESTATE: the buffer would have to grow under capture. */
int smpc_kalman_row_margin(smpc_handle* h, int B, const smpc_kalman_params* par, const double* state, double z, double base_a,
                           double base_b, double d_max);

/* A reference curve of its own for every instance of the tracking task.  curves is [B][3][L] doubles: curves[b] has exactly the
 * layout of the shared table smpc_policy_state.traj / smpc_score_params.traj ([3][L], L = n_steps + 1 + N columns).  The handle
 * keeps a copy like a scene (stream-ordered; with host pointers the call checks every entry for finiteness and waits for the
 * copy; device pointers are taken as they are), curves == NULL clears them.  A call with the same (B, L) overwrites the handle's
 * buffer in place, so a step captured in a hipGraph keeps seeing it.
 * While curves are set
 *   smpc_policy_step (all six kinds, SMPC_POLICY_PARALLEL included): before the solve, for the stepping instances,
 *       p[b][i][0:3] = curves[b][:, clamp(current_step[b] + i, 0, L - 1)]
 *     -- what a non-NULL st->traj does from the shared table; instances that do not step keep their p.  A non-NULL st->traj is
 *     SMPC_EINVAL (two sources for one input).
 *   smpc_score_rollout with par->traj == NULL and par->ee_ref == NULL: ref_j of instance b is column min(j, L - 1) of curves[b].
 *     With either pointer given the call does not read the curves.
 * The curves belong to THEIR batch size: these two calls with another B return SMPC_EINVAL and name both sizes; the engine never
 * falls back to the shared reference.  Nothing else reads them: smpc_solve_batch, smpc_sqp_batch, smpc_merit_terms and
 * smpc_check_guess take p from the caller, smpc_rollout_batch has no reference trajectory.
 * Memory: 24 bytes x L x B.  The shipped n_steps_tracking = 5000 with N = 30 gives L = 5031: 121 KB per instance, 495 MB at 4096.
 * SMPC_EINVAL: B <= 0, L < 1, or (host pointers only) a non-finite entry.
 * SMPC_ESTATE: the copy would have to grow while the stream is being captured.
 * (ABI version unchanged: no existing entry point or structure changed) */
int smpc_set_instance_curves(smpc_handle* h, int B, int64_t L, const double* curves, int on_device);

/* A controller model of its own for every instance: the link inertials the OCP's dynamics are formed with.  joints is [B][nq]
 * smpc_joint, the records smpc_plant_step takes as joints_noisy; of every record the engine reads mass, com[3] and inertia[6] and
 * nothing else.  Kinematics (R0, p0, axis) and the limits (q_min, q_max, v_max, tau_max) stay the descriptor's, and with them the EE
 * point, the collision rows, inverse kinematics, the bounds and the torque limits.
 * The handle keeps the 232-byte records as they are -- the caller's inertials with the descriptor's other seven fields in every
 * record -- so that a record stands wherever the kernels read a joint of the descriptor; 232 x nq x B bytes (1392 per instance at
 * nq = 6, 5.7 MB at 4096), of which the kernels touch the 80 bytes of inertials per joint (and the torque kernels of the
 * thread-per-node path the kinematics beside them).  The copy is stream-ordered; with host pointers the call checks that the seven
 * fields equal the descriptor's bit for bit, that mass is finite and >= 0 and that com and inertia are finite, and waits for the
 * copy; device pointers are taken as they are (the seven fields are then not read at all: the handle's records get the
 * descriptor's).  joints == NULL clears the table.  A call with the same B overwrites the handle's buffer in place, so a step
 * captured in a hipGraph keeps seeing it; smpc_set_horizon does not drop it.
 * While a table is set, these form the torque row, its Jacobians, the merit's torque term and the torque margin with instance b's
 * inertials: smpc_solve_batch, smpc_eval_nodes, smpc_merit_terms, smpc_sqp_batch, smpc_check_guess, smpc_policy_step (kinds 0-4)
 * and smpc_debug_stage_records (both paths).  The table belongs to ITS batch size: a call of these with another B returns
 * SMPC_EINVAL and names both sizes -- it never falls back to the descriptor's robot.  SMPC_POLICY_PARALLEL and smpc_rollout_batch
 * return SMPC_ESTATE while a table is set, for the reasons they refuse a scene.  Not read by: smpc_plant_step and the plant inside
 * smpc_loop_post (their own joints_noisy argument), smpc_check_trajectory, smpc_score_rollout, smpc_ik_batch (no dynamics),
 * smpc_ray_update.  Without a table every entry point launches exactly the kernels it launched before the table existed.
 * SMPC_EINVAL: B <= 0, or (host pointers only) a record that fails the checks above; the message names instance, joint and field
 * and the previous table stays in force.
 * SMPC_ESTATE: the copy would have to grow while the stream is being captured (the old contents stay).
 * (ABI version unchanged: no existing entry point or structure changed) */
int smpc_set_instance_models(smpc_handle* h, int B, const smpc_joint* joints, int on_device);

/* A safe-set network that knows its scene: n_ctx extra inputs (a CONTEXT, numbers of the instance's scene) behind the 2 n_dof_safe_set
 * state features.  The network's first layer is W0 = [Ws | Wc], Ws [H][2 nd] handed over by smpc_set_mlp and Wc [H][n_ctx] (row-major,
 * H = dims[1]) here; for an instance with context c the row's value and gradient are those of the plain network with first-layer
 * weights Ws and first-layer bias b0 + Wc ((c - ctx_mean) / ctx_std).  No derivative with respect to the context is formed.
 * Call it after smpc_set_mlp.  ctx_default[n_ctx] is the context every row gets while no instance context is set (the shared scene's).
 * n_ctx = 0 or Wc == NULL clears the context columns; smpc_set_mlp drops them too (new weights mean no context).  Setting or clearing
 * also drops an instance context.  on_device != 0: all four pointers are device memory.  The call synchronises the stream.
 * The input of layer 0 is padded to 16 columns, so n_ctx <= 16 - 2 n_dof_safe_set (4 for six joints, 2 for seven).
 * SMPC_EINVAL (the message names the limit): n_ctx outside that range, a non-finite value, a ctx_std <= 0.
 * SMPC_ESTATE: no network (smpc_set_mlp was not called).
 * (ABI version unchanged: no existing entry point or structure changed) */
int smpc_set_mlp_context(smpc_handle* h, int n_ctx, const float* Wc, const double* ctx_mean, const double* ctx_std,
                         const double* ctx_default, int on_device);

/* The context of every instance: ctx is [B][n_ctx] doubles; the handle keeps a normalised fp32 copy.  The copy is stream-ordered;
 * with host pointers the call checks for non-finite values and waits, with device pointers a small kernel normalises.  NULL clears it
 * (every row then gets ctx_default again).  The context is a slot of its own: the engine does not derive it from the instance scene.
 * It belongs to ITS batch size: smpc_solve_batch, smpc_eval_nodes, smpc_merit_terms, smpc_sqp_batch, smpc_check_guess,
 * smpc_check_trajectory, smpc_score_rollout, smpc_policy_step and smpc_debug_stage_records with another B return SMPC_EINVAL and name
 * both sizes.  SMPC_POLICY_PARALLEL and smpc_rollout_batch return SMPC_ESTATE while it is set (candidate slots and worker handles are
 * not instances); both run with the default context.
 * Which instance a network row belongs to: node / (N + 1) on the [B][N+1] node arrays, node / n_nodes in smpc_check_trajectory,
 * row % B in the step-major log of smpc_score_rollout.
 * SMPC_EINVAL: no context columns, B <= 0, or (host pointers only) a non-finite entry.
 * SMPC_ESTATE: the copy would have to grow while the stream is being captured (the old contents stay).
 * (ABI version unchanged: no existing entry point or structure changed) */
int smpc_set_instance_context(smpc_handle* h, int B, const double* ctx, int on_device);

/* A context that follows a scene track: ctx is [B][T][n_ctx] doubles, the raw numbers of instance b's scene in time column j; the
 * handle keeps a normalised fp32 copy of 4 * n_ctx * T * B bytes.  The meaning is quasi-static: the network is one trained on
 * standing scenes, and at node k it is asked about the scene as it will stand at time t + k.
 * The column rule is THE column rule of smpc_set_instance_scene_track above and its table, not restated here: t = the cell of
 * smpc_set_scene_clock (0 without one), and col(.) clamps with THIS table's T, which may differ from the scene track's (each
 * table clamps by its own).  Which network row reads which column:
 *   smpc_solve_batch, smpc_eval_nodes, smpc_merit_terms, smpc_sqp_batch, smpc_check_guess (its safe_node included),
 *   smpc_debug_stage_records, and the solve and the x_temp / viable-state tests of smpc_policy_step (kinds 0-4):
 *                                                              the network row of node k of the [B][N+1] arrays: col(t + k)
 *   smpc_check_trajectory:                                     node k of the [B][n_nodes] arrays: col(t + k)
 *   smpc_score_rollout (the clock is not read):                state j of the log: col(j)
 * A context and a context track are ONE slot of the handle, as a scene and a scene track are: setting one replaces the other,
 * smpc_set_instance_context(h, B, ctx, ..) is exactly a track with T = 1, and ctx == NULL in either setter clears both.  Everything
 * said of the instance context holds: the copy is stream-ordered; a call with host pointers checks for non-finite values (the message
 * names instance, column and number, and the previous table stays in force) and waits, device pointers go through the normalising
 * kernel; the table belongs to its batch size (another B: SMPC_EINVAL naming both); the same (B, T) overwrites the buffer in place, so
 * a captured step keeps seeing it; smpc_set_mlp and smpc_set_mlp_context drop it; SMPC_POLICY_PARALLEL and smpc_rollout_batch return
 * SMPC_ESTATE while it is set.  With T = 1 the clock is not read.
 * SMPC_EINVAL: no context columns, B <= 0, T < 1, or (host pointers only) a non-finite entry.
 * SMPC_ESTATE: the copy would have to grow while the stream is being captured (the old contents stay).
 * (ABI version unchanged: no existing entry point or structure changed) */
int smpc_set_instance_context_track(smpc_handle* h, int B, int64_t T, const double* ctx, int on_device);

/* replaces ocp_solver.cost_set(k,'zl'/'zu',v) (controller.py:455-468, 526-527): L1 penalty of the slack on the safe-set row of
 * node k, for the nodes where the formulation made that row soft (nn_soft_e / nn_soft_run >= 0; a hard row has no slack and
 * acados' arrays for it are empty).  zl is [N+1] host doubles shared by all instances (entry 0 unused); NULL restores the
 * descriptor's weights. */
int smpc_set_slack_weights(smpc_handle* h, const double* zl);

/* ---- the hot path --------------------------------------------------------------------------------------------- */
/* One SQP-RTI solve of B independent OCPs: replaces reset / constraints_set(0,lbx|ubx,x0) / set(i,x|u|p) / solve /
 * get(i,x|u) of controller.py:141-164 for B instances in one call.
 *   x0 [B][nx], xg [B][N+1][nx], ug [B][N][nu], p [B][N+1][5]        inputs
 *   x_out [B][N+1][nx], u_out [B][N][nu], status [B], qp_iter [B]    outputs (qp_iter may be NULL)
 * on_device != 0: all pointers are device pointers (resident in HBM); the call only enqueues work on the handle's
 * stream (use smpc_sync to wait).  on_device == 0: host pointers; the call copies in, runs, copies out and waits. */
int smpc_solve_batch(smpc_handle* h, int B, const double* x0, const double* xg, const double* ug, const double* p,
                     double* x_out, double* u_out, int32_t* status, int32_t* qp_iter, int on_device);

/* Linearisation only (HOT LOOP A of SURVEY 3.2): evaluates every node of every instance at (xg, ug, p) and writes
 * out[B][N+1] records.  Used by the parity tests; pointers follow on_device like smpc_solve_batch. */
int smpc_eval_nodes(smpc_handle* h, int B, const double* xg, const double* ug, const double* p, smpc_node_eval* out,
                    int on_device);

/* ---- full SQP with merit backtracking (the warm starts of scripts/guess_acados.py) ------------ */
/* The two terms of the l1 merit function  f + mu |c|_1  of B trajectories, evaluated forward-only at the trial points
 * (x + alpha[b] dx, u + alpha[b] du):  out[B][3] = {f, viol, gd}.
 *   f     the cost as acados sums it: cost_scale_stage / cost_scale_term times Q |ee - p[0:3]|^2 (+ R |u|^2 on nodes 0..N-1);
 *         0 for SMPC_COST_ZERO
 *   viol  the l1 norm of every constraint's violation: |x_0 - x0|, the defects of the double integrator, the state box of nodes
 *         1..N, max(|tau| - tau_max, 0) on nodes 0..N-1, the collision rows on nodes 1..N (a bound with |value| >= SMPC_INF is
 *         absent), the safe-set row max(-g, 0) on the nodes where the formulation has it and p[4] > 0 (never on node 0)
 *   gd    grad f . (dx, du), for the instances with alpha[b] == 0 (or alpha == NULL) when dx / du are given; 0 otherwise
 * dx / du / alpha may be NULL (the point is (x, u), gd = 0).  mask[B] (bytes, may be NULL): instances with mask[b] == 0 are
 * skipped and their out[b] left as it is (so out is read as well as written on the host path).  Sums are formed in a fixed order:
 * two calls give the same bits.  Pointers follow on_device like smpc_solve_batch. */
int smpc_merit_terms(smpc_handle* h, int B, const double* x0, const double* x, const double* u, const double* p, const double* dx,
                     const double* du, const double* alpha, const uint8_t* mask, double* out, int on_device);

typedef struct {
    int32_t max_iter;        /* SQP iterations of this call at most (nlp_solver_max_iter, parser.py:139) */
    int32_t reserved0;
    double tol;              /* an instance is done once alpha * |step|_inf < tol (1e-6) */
    double armijo;           /* sufficient-decrease factor of the line search (1e-4) */
    double alpha_reduction;  /* step-length factor per rejected trial (0.7) */
    double alpha_min;        /* floor at which the step is taken regardless (0.05) */
    double mu0;              /* start value of the penalty (10): the caller fills the state's mu[B] with it before the first call;
                              * the call itself reads and writes mu[B] only */
    double mu_max;           /* cap of the penalty (1e8) */
} smpc_sqp_opts;

typedef struct {             /* per-instance arrays [B], read AND written: a call resumes where the previous one stopped */
    double* mu;              /* penalty of the l1 merit function */
    uint8_t* done;           /* converged (or failed): skipped by every kernel of later iterations */
    int32_t* status;         /* acados status of the last QP the instance took part in */
    double* alpha;           /* last iteration the instance took part in: accepted step length (0: step not taken) */
    double* merit_before;    /* ... merit at the iterate before the step */
    double* merit;           /* ... merit after it (= merit_before where the step was not taken) */
    double* violation;       /* ... l1 violation after it */
    uint8_t* updated;        /* ... the iterate moved */
    int32_t* iters;          /* SQP iterations the instance took part in (accumulates) */
    int32_t* qp_iter_total;  /* interior-point iterations of those solves (accumulates) */
} smpc_sqp_state;

/* SQP with l1-merit backtracking for B instances, in place on (x_guess, u_guess): replaces ocp_solver.solve() with
 * nlp_solver_type 'SQP' and globalization 'MERIT_BACKTRACKING' (parser.py:115-117, guess_acados.py:115).  Per iteration: the
 * stage QP at the iterate (instances that are done are masked out of the stage builder and the QP), penalty update so that the QP
 * step is a descent direction of the merit, backtracking over the step lengths 1, r, r^2, .. down to alpha_min with the Armijo test
 *   merit(alpha) <= merit(0) + armijo alpha min(grad f . d - mu |c|_1, 0) + 1e-12 (1 + |merit(0)|),
 * commit of the accepted point, done |= alpha |step|_inf < tol or status != 0.  max_iter = 1 called k times equals one call with
 * max_iter = k, bit for bit.  The call stops early once no instance is open; that 4-byte count is the only per-iteration host read
 * (skipped while the stream is being captured).  on_device != 0: every array, the state's included, is a device pointer; 0: host
 * pointers, copied in and out. */
int smpc_sqp_batch(smpc_handle* h, int B, const smpc_sqp_opts* opts, const double* x0, double* x_guess, double* u_guess,
                   const double* p, const smpc_sqp_state* state, int on_device);

/* The acceptance test of a warm start, AbstractController.checkGuess (guess_acados.py:118: `status in (0, 2) and checkGuess()`),
 * per instance and forward-only, so that a device-resident SQP batch can be asked between two smpc_sqp_batch calls which of its
 * instances are acceptable.  flags[B]: bit i set = predicate i FAILS (a NaN fails); worst[B][5]: the value each predicate tests.
 *   0  state box on nodes 0..N (env_model.py:170-172): max over nodes, components of max(x_min - x, x - x_max)   passes: <= tol_x
 *   1  collision rows (env_model.py:236-243), on node 0 only when collision_first_node != 0, on every node otherwise: max over the
 *      tested nodes and rows of max(row_lb_chk - v, v - row_ub_chk); -inf without rows                            passes: <= 0
 *   2  torque on nodes 0..N-1 (env_model.py:179-182): max of max(tau_min - tau, tau - tau_max)                    passes: <= tol_tau
 *   3  dynamics (env_model.py:226-234, the controller's own model: what smpc_guess_correction rolls out from node 0):
 *      |x - x_sim|_2 over the whole trajectory                                                     passes: < tol_dyn sqrt(N + 1)
 *   4  safe set at node safe_node (safe_set.py:61-68): -g(x, alpha); safe_node < 0: not tested, bit clear, -inf
 *                                                                         passes: g >= -tol_safe && g <= 1e6 + tol_safe */
typedef struct {
    double tol_x, tol_tau, tol_dyn, tol_safe, alpha;
    int32_t collision_first_node;   /* as smpc_policy_params */
    int32_t safe_node;              /* node of the safe-set test (N for the terminal-set controllers), < 0: none */
    const double *x_min, *x_max;            /* HOST [nx]   */
    const double *tau_min, *tau_max;        /* HOST [nq]   */
    const double *row_lb_chk, *row_ub_chk;  /* HOST [n_rows] */
} smpc_guess_check;

/* x [B][N+1][nx], u [B][N][nu]; mask[B] (bytes, may be NULL): instances with mask[b] == 0 are skipped and their flags[b] /
 * worst[b] left as they are (so both are read as well as written on the host path).  Sums are formed in a fixed order: two calls
 * give the same bits.  x, u, mask, flags, worst follow on_device like smpc_merit_terms; with device pointers the call only
 * enqueues.  The small host arrays of `par` are kept in a device block of the handle and uploaded only when they change.
 * SMPC_ESTATE: safe_node >= 0 without a network, or scratch / the bounds block would have to change while the stream is being
 * captured.  SMPC_EINVAL: safe_node > N.  (ABI version unchanged: no existing entry point or structure changed) */
int smpc_check_guess(smpc_handle* h, int B, const double* x, const double* u, const smpc_guess_check* par,
                     const uint8_t* mask, int32_t* flags, double* worst, int on_device);

/* ---- training data of the safe set: the bookkeeping of ray labelling ------------------------------------------------ */
/* What NetSafeSet learns (safe_set.py:71-104) is, for a configuration q and a unit direction d, the largest speed s such that
 * (q, s d) can still be brought to rest inside the state box, the torque limits and the free space.  A ray (q, d) is labelled by
 * trials of the backup OCP from x0 = (q, s d), each started from the constant guess with a fresh SQP state: trial 0 at s = 0, trial 1
 * at s = hi (the velocity box along d, set by the caller), trials 2 .. bisect + 1 at s = (lo + hi) / 2.  Between rounds of
 * smpc_sqp_batch + smpc_check_guess this entry point takes one look at every open ray.  Its trial is
 *   feasible    if status == 0, flags[b] == 0, max |v_N| <= tol_term, |x_guess[b][0] - x0[b]|_inf <= 1e-12 and no NaN is in the iterate;
 *   infeasible  if not feasible and the instance is done, has used `budget` SQP iterations, or holds a NaN;
 *   pending     otherwise: the ray is left untouched, bit for bit -- as is a ray with open[b] == 0.
 * A feasible trial copies the iterate into (x_cert, u_cert) and sets lo = s, an infeasible one sets hi = s; either adds the trial's SQP
 * iterations to iters_total and 1 to trial.  Then trial 0 infeasible ends the ray as SMPC_RAY_DEAD, trial 1 feasible as
 * SMPC_RAY_SATURATED, trial bisect + 1 as SMPC_RAY_BRACKETED (kind set, open = 0, the SQP state's done = 1: the ray costs nothing
 * further; its label is lo); otherwise the next trial starts: s, x0[b] = (q, s d), x_guess[b] = x0[b] on every node, u_guess[b] = 0,
 * every field of the SQP state reset (mu = mu0, the rest 0).  The statement is safe_mpc_amd/safe_set_data.py::ray_update_statement. */
#define SMPC_RAY_OPEN 0
#define SMPC_RAY_DEAD 1
#define SMPC_RAY_SATURATED 2
#define SMPC_RAY_BRACKETED 3
typedef struct {
    int32_t bisect;          /* bisection steps after the two end-point trials (>= 0) */
    int32_t budget;          /* SQP iterations of a trial at most (>= 1); looked at between rounds only */
    double tol_term;         /* largest terminal velocity component of a feasible trial (tol_x) */
    double mu0;              /* start value of the SQP penalty of a new trial (smpc_sqp_opts.mu0) */
} smpc_ray_opts;

typedef struct {             /* per-ray arrays, read AND written except q and d */
    const double *q, *d;     /* [B][nq] configuration and unit direction */
    double *lo, *hi, *s;     /* [B] bracket and the speed of the trial in flight */
    int32_t *trial;          /* [B] trials completed = index of the one in flight */
    int32_t *kind;           /* [B] SMPC_RAY_* */
    uint8_t *open;           /* [B] 1 while the ray is in flight: the mask of the next smpc_check_guess */
    double *x_cert, *u_cert; /* [B][N+1][nx], [B][N][nu]: the iterate of the last feasible trial, the proof of the label lo */
    int32_t *iters_total;    /* [B] SQP iterations of the completed trials */
} smpc_ray_state;

/* flags [B] (of smpc_check_guess with mask = rays->open), x0 [B][nx], x_guess [B][N+1][nx], u_guess [B][N][nu]; *n_open (one int32):
 * the rays still open after the call, the only value a labelling loop reads per round.  Nothing is summed across rays and no
 * floating-point atomics are used: two calls give the same bits and a ray's result does not depend on B or on its neighbours.  Every
 * array, those of both structs and n_open included, follows on_device like smpc_sqp_batch; with device pointers the call only
 * enqueues (capturable, no scratch).  SMPC_EINVAL: B <= 0, bisect < 0, budget < 1 or a NULL array.
 * (ABI version unchanged: no existing entry point or structure changed) */
int smpc_ray_update(smpc_handle* h, int B, const smpc_ray_opts* opts, const smpc_ray_state* rays, const smpc_sqp_state* sqp,
                    const int32_t* flags, double* x0, double* x_guess, double* u_guess, int32_t* n_open, int on_device);

/* ---- start states at a chosen end-effector position: batched multi-start inverse kinematics ------------------------- */
/* Per instance b: a joint configuration q in [q_lo, q_hi] whose end-effector point (the descriptor's ee_point) sits at target[b]
 * and whose collision rows meet row_lb <= v_r(q) <= row_ub (a bound with |value| >= SMPC_INF is absent) -- the problem of the
 * reference's InverseKinematicsOCP (ocp.py:321-326, solved there by IPOPT per instance; guess_acados.py:179-183 takes the start
 * state of a tracking run from it).  The caller appends the zero velocity.
 * S starts per instance (q_start[b][s], supplied by the caller: no sampler runs on the device) each run max_iter iterations of a
 * projected Levenberg-Marquardt method on the stacked residual r(q) = {ee(q) - target; w (lb' - v_r) for the rows below their
 * pushed bound lb' = lb + push |lb|; w (v_r - ub') for those above ub' = ub - push |ub|}, w = 1 / max(sqrt|bound|, 1e-3):
 *   dq = -(J^T J + lam I)^-1 J^T r,  q' = clip(q + dq, q_lo, q_hi),  accepted when |r(q')|^2 < |r(q)|^2;
 *   lam *= damping_accept (floor damping_min) on accept, *= damping_reject (cap damping_max) on reject, lam = damping at the start.
 * A start succeeds when at its final point |ee - target|_inf <= tol_ee and every row is within its UNPUSHED bounds.  The winner
 * is the successful start with the lowest index; if none succeeds, the start with the least final |r|^2 (ties: lowest index).
 * The statement is safe_mpc_amd/ik.py::ik_batch_host. */
typedef struct {
    int32_t max_iter;               /* iterations of every start, exactly (40) */
    int32_t reserved0;
    double tol_ee;                  /* success: |ee - target|_inf <= tol_ee (1e-6, constr_viol_tol of ocp.py:338) */
    double push;                    /* relative distance the rows are pushed inside their bounds (1e-2) */
    double damping;                 /* lam at the start (1e-2) */
    double damping_accept, damping_reject;  /* factors on lam after an accepted / rejected step (0.3, 4) */
    double damping_min, damping_max;        /* floor and cap of lam (1e-9, 1e6) */
    const double *q_lo, *q_hi;      /* HOST [nq] */
    const double *row_lb, *row_ub;  /* HOST [n_rows] */
} smpc_ik_params;

/* target [B][3], q_start [B][S][nq] with 1 <= S <= 64; mask[B] (bytes, may be NULL): instances with mask[b] == 0 are skipped and
 * their outputs left as they are (so the outputs are read as well as written on the host path).
 *   q_out [B][nq]   the winner's final point: always finite and inside the box (a non-finite start component starts from the
 *                   middle of its interval)
 *   info  [B][2]    {index of the winning start, number of starts that succeeded (0 = no solution)}
 *   resid [B][2]    {|ee - target|_inf, worst row margin max(lb - v, v - ub) over the present bounds; -inf without one}, both at
 *                   q_out from a final forward-only evaluation
 * Nothing is summed across starts or instances and no atomics are used: two calls give the same bits, and an instance's result
 * does not depend on B or on the rest of the batch.  While a scene is set (smpc_set_instance_scene) the rows are formed in the
 * instance's scene, and a call with another B returns SMPC_EINVAL.  target, q_start, mask, q_out, info, resid follow on_device
 * like smpc_check_guess; with device pointers the call only enqueues.  The small host arrays of `par` are kept in a device block
 * of the handle and uploaded only when they change.  SMPC_EINVAL: S outside 1..64, max_iter < 1, missing bounds.  SMPC_ESTATE: the
 * bounds block would have to change while the stream is being captured.
 * (ABI version unchanged: no existing entry point or structure changed) */
int smpc_ik_batch(smpc_handle* h, int B, int S, const double* target, const double* q_start, const smpc_ik_params* par,
                  const uint8_t* mask, double* q_out, int32_t* info, double* resid, int on_device);

/* ---- scoring a closed-loop run where its logs are ------------------------------------------------------------------ */
/* The last step of the experiment: the closed-loop cost of every instance (metrics_count_fails.py:19-28), the distance the
 * convergence test compares with tol_conv (mpc.py:273) and how close the run came to the obstacles, the state box
 * (env_model.py:170-172,236-243) and the learned safe set (safe_set.py:61-68), from the step-major logs of smpc_loop_state, per
 * instance and forward-only.  out[B][SMPC_SCORE_ND] doubles and outi[B][SMPC_SCORE_NI] int32:
 *   d0  cost = Q d1 + R d2 with the descriptor's Q and R (no cost_scale_*, no dt): for a complete log the reference's metric
 *   d1  sum over j <= last_x of |ee(x_j) - ref_j|^2; ref_j = ee_ref, or column min(j, traj_len - 1) of traj (the convention of
 *       smpc_policy_state.traj)
 *   d2  sum over j <= last_u of |u_j|^2
 *   d3  |ee(x_j) - ref_j|_2 at j = last_x
 *   d4  worst collision margin: max over j <= last_x and the rows of max(row_lb_chk - v, v - row_ub_chk), v as smpc_merit_terms forms
 *       the rows; <= 0 means free; -inf without rows.                                        i0, i1: its step and row (-1, -1)
 *   d5  worst state-box margin: max over j <= last_x and components of max(x_min - x, x - x_max)           i2: its step
 *   d6  least safe-set value: min over j <= last_x of g(x_j, alpha), g as smpc_check_guess forms it (fp32-accurate: it passes
 *       through the network); +inf when want_safe == 0                                                 i3: its step (-1)
 * last_x[B] / last_u[B]: last valid row of each log, inclusive (last_u = -1: no valid control; last_x >= max(last_u, 0)); NULL: the
 * logs are complete.  Rows past them may hold anything, NaN included, and affect nothing.  Ties go to the earliest step, then the
 * lowest row; a maximum or minimum that has seen a NaN in a valid row stays NaN (placed at the first one), and so do the sums. */
#define SMPC_SCORE_ND 7
#define SMPC_SCORE_NI 4
typedef struct {
    double alpha, tol_safe;         /* as smpc_guess_check; tol_safe is carried for the caller's own test of d6 and read by no kernel */
    int32_t want_safe;              /* != 0: fill d6 / i3 (needs smpc_set_mlp) */
    int32_t reserved0;
    const double *x_min, *x_max;            /* HOST [nx] */
    const double *row_lb_chk, *row_ub_chk;  /* HOST [n_rows] */
    const double *ee_ref;                   /* HOST [3], used when traj == NULL; both NULL: the handle's curves (smpc_set_instance_curves) */
    const double *traj; int64_t traj_len;   /* [3][traj_len], follows on_device; or NULL */
} smpc_score_params;

/* x_log [n_steps+1][B][nx], u_log [n_steps][B][nu]; mask[B] (bytes, may be NULL): instances with mask[b] == 0 are skipped and their
 * out[b] / outi[b] left as they are (so both are read as well as written on the host path).  Sums are formed in a fixed order and
 * without floating-point atomics: steps ascending inside segments of 32 steps cut by absolute step index, then the segments
 * ascending -- two calls give the same bits, and d0..d5 / i0..i2 of an instance do not depend on B or on the rest of the batch (d6
 * may: the row count selects the network kernel).  The network runs over the log in passes of a bounded row count, so scratch does
 * not grow with n_steps * B beyond 64 bytes per instance and 32 steps.  x_log, u_log, last_x, last_u, traj, mask, out, outi follow
 * on_device like smpc_check_guess; with device pointers the call only enqueues.  The small host arrays of `par` are kept in a device
 * block of the handle and uploaded only when they change.  SMPC_ESTATE: want_safe without a network, or scratch / the bounds block
 * would have to change while the stream is being captured.  SMPC_EINVAL: n_steps < 1, missing bounds, traj with traj_len < 1.
 * (ABI version unchanged: no existing entry point or structure changed) */
int smpc_score_rollout(smpc_handle* h, int B, int n_steps, const double* x_log, const double* u_log,
                       const int64_t* last_x, const int64_t* last_u, const smpc_score_params* par,
                       const uint8_t* mask, double* out, int32_t* outi, int on_device);

/* ---- callers on either side of the solve ------------------------------------------- */
/* guessCorrection (controller.py:226-231): x_guess[k+1] = f(x_guess[k], u_guess[k]) in place. */
int smpc_guess_correction(smpc_handle* h, int B, double* xg, const double* ug, int on_device);

/* provideControl (controller.py:169-184): per instance, take (x_temp,u_temp) if accept[b] != 0 else keep the old
 * guess; write u_apply = row 0; shift by one and duplicate the last row. */
int smpc_provide_control(smpc_handle* h, int B, const int32_t* accept, const double* x_temp, const double* u_temp,
                         double* xg, double* ug, double* u_apply, int on_device);

/* checkStateConstraints over a trajectory (env_model.py:170-173, 236-243): ok[b] = all nodes within
 * [x_min - tol_x, x_max + tol_x] (the margin-widened model bounds passed here) and collision rows within
 * [lb_chk, ub_chk]; nn_ok[b][k] = g(x_k, alpha) >= -tol_safe (safe_set.py:61-68) if nn_ok != NULL. */
int smpc_check_trajectory(smpc_handle* h, int B, int n_nodes, const double* x, const double* x_min,
                          const double* x_max, double tol_x, const double* row_lb_chk, const double* row_ub_chk,
                          double alpha, double tol_safe, int32_t* state_ok, int32_t* nn_ok, int on_device);

/* plant step AdamModel.integrate (env_model.py:192-206): tau = RNEA_noisy(x,u) + noise, clip, qdd = M^-1(tau - h),
 * double-integrator step.  joints_noisy is [B][nq] smpc_joint (per-instance perturbed inertials) or NULL for the
 * nominal model; tau_noise [B][nq] additive torque noise or NULL. */
int smpc_plant_step(smpc_handle* h, int B, const double* x, const double* u, const smpc_joint* joints_noisy,
                    const double* tau_noise, double* x_next, double* u_eff, int on_device);

/* Closed-loop rollout of the plain RTI policy for n_steps, without a host round trip per step: NaiveController.step
 * (controller.py:274-284: guessCorrection, solve, fails = status == 0 ? 0 : fails + 1, provideControl(fails == 0)) followed
 * by the plant step of scripts/mpc.py:151,240 (smpc_plant_step semantics, optional per-instance model and per-step torque
 * noise).  x_guess / u_guess are the warm start on entry and the shifted guess of the last step on return.
 * Trajectories are STEP-major: x_traj[n_steps+1][B][nx] (x_traj[0] = x0), u_traj[n_steps][B][nu], status_traj[n_steps][B],
 * iter_traj[n_steps][B] (may be NULL), tau_noise[n_steps][B][nq] or NULL, joints_noisy[B][nq] or NULL.
 * Large batches are split into two (B >= 1024) or three (B >= 3072) sub-batches that advance on their own streams inside the
 * engine (worker handles sharing the network weights): the long tail of one sub-batch's QP launch overlaps the bulk of the
 * others'.  The
 * environment variable SMPC_ROLLOUT_STREAMS overrides the number of sub-batches; results do not depend on it. */
int smpc_rollout_batch(smpc_handle* h, int B, int n_steps, const double* x0, double* x_guess, double* u_guess,
                       const double* p, const smpc_joint* joints_noisy, const double* tau_noise, double* x_traj,
                       double* u_traj, int32_t* status_traj, int32_t* iter_traj, int on_device);

/* ---- the policy layer with all state in HBM ------------------------------------------------- */
/* The reference walks its instances one at a time through <Controller>.step (controller.py:274-284, 375-388, 448-498,
 * 524-565, 651-661) and the safe-abort loop of scripts/mpc.py:125-264.  These three entry points are those two pieces of code
 * for B instances at once, state resident on the device, enqueue-only on the handle's stream (no host synchronisation, so a
 * caller can capture a whole closed-loop step in a hipGraph once an eager step of the same batch size has grown the handle's
 * buffers; a call that would grow one while the stream is being captured returns SMPC_ESTATE).  All pointers inside the structs
 * and all array arguments are DEVICE pointers unless stated otherwise; flags are one byte per instance (0 / 1). */
enum {
    SMPC_POLICY_NAIVE = 0,          /* NaiveController / TerminalZeroVelocity / STController                      :274-284 */
    SMPC_POLICY_STATE_CHECK = 1,    /* ControllerSafeSetEverywhere: success also needs checkStateConstraints       :651-661 */
    SMPC_POLICY_STWA = 2,           /* STWAController / HTWAController: viable state, abort after N - 1 failures   :375-388 */
    SMPC_POLICY_RECEDING = 3,       /* RecedingController: receding index r, row switched on at node r             :448-498 */
    SMPC_POLICY_REAL_RECEDING = 4,  /* RealReceding: node r boxed to the planned state +- tube                     :524-565 */
    SMPC_POLICY_PARALLEL = 5        /* ParallelController: N candidate OCPs, row on at node n = N..1, best kept    :567-644 */
};

typedef struct {
    int32_t kind;                   /* SMPC_POLICY_* */
    int32_t abort_flag;             /* params.abort_flag (controller.py:471-478) */
    int32_t collision_first_node;   /* != 0: trajectories are collision-tested at their first node only, as the reference's
                                       checkCollision does (env_model.py:238-243); 0: at every node */
    int32_t reserved0;
    double tol_x, alpha, tol_safe;  /* checkStateConstraints / checkSafeConstraints tolerances (env_model.py:170, safe_set.py:61) */
    double tube;                    /* RealReceding: half-width of the box at node r (1e-3, controller.py:531-532) */
    const double *x_min, *x_max;            /* HOST [nx]: model bounds of the state test */
    const double *row_lb_chk, *row_ub_chk;  /* HOST [n_rows]: check bounds of the collision rows */
    const double *stage_lo, *stage_hi;      /* DEVICE [N+1][nx]: RealReceding's bounds away from node r (NULL otherwise) */
} smpc_policy_params;

typedef struct {                    /* what a controller object holds per instance (controller.py:112-131) */
    double *x_guess, *u_guess;      /* [B][N+1][nx], [B][N][nu] */
    double *x_temp, *u_temp;        /* the iterate of the last solve */
    double *p;                      /* [B][N+1][5] */
    double *x_viable;               /* [B][nx] */
    int64_t *fails, *current_step;  /* [B] */
    int64_t *r;                     /* [B] receding index (NULL for the policies without one) */
    int32_t *status, *qp_iter;      /* [B] of the last solve */
    const double* traj;             /* [3][traj_len] reference trajectory of the cost (cost.traj, cost_definition.py:30-31,89), or NULL.
                                       Not NULL: before the solve, p[b][i][0:3] = traj[:, current_step[b] + i] for every node i of the
                                       stepping instances -- what solve() does through ocp_solver.set(i, 'p', .) at
                                       controller.py:153-156 (column index clamped to traj_len - 1).  NULL: p[:, :, 0:3] is left as the
                                       caller set it (the constant ee_ref of the ReachTarget costs) -- unless the handle holds curves
                                       (smpc_set_instance_curves), which then feed p the same way and with which traj must be NULL. */
    int64_t traj_len;
} smpc_policy_state;

/* <Controller>.step(x) for the instances with stepping[b] != 0 (NULL: all): guessCorrection, the policy's flags / bounds,
 * the RTI solve, the acceptance tests, the fails / r / viable-state automaton, provideControl.  Instances that do not step are
 * left untouched and skipped by the QP kernels.  u_out[b] = the policy's control, u_guess[b][0] for an instance that raises
 * abort, u_other[b] for one that did not step (u_other may be NULL when stepping is).  abort_out[b] = the step's second return
 * value; *any_abort (one int32) is set to 1 if any instance aborted, 0 otherwise. */
/* SMPC_POLICY_PARALLEL needs st->r and a network with the row on every node (SMPC_NN_ALL), like the receding kinds need r.  Its
 * step solves candidate n = N for every stepping instance, then candidates N - 1 .. 1 for the instances whose first candidate did
 * not reach node N, as one launch over a dense list of candidate slots (which slots are live is only known on the device).  That
 * second launch runs on candidate scratch of up to B * (N - 1) extra instances, allocated on the first parallel step of a batch
 * size and reused: the QP workspace of B * (N - 1) instances, the network pass's per-row buffers for their B * (N - 1) * N nodes,
 * and the candidates' inputs and outputs.  For nq = 6, 6 rows, N = 30, B = 4096 (computed from the layouts, not measured):
 * 19.8 GB + 10.9 GB + 1.6 GB.  When it cannot be allocated the call returns SMPC_ENOMEM and says how much it asked for. */
int smpc_policy_step(smpc_handle* h, int B, const smpc_policy_params* par, const smpc_policy_state* st, const double* x,
                     const uint8_t* stepping, const double* u_other, double* u_out, uint8_t* abort_out, int32_t* any_abort);

typedef struct {                    /* the driver's per-instance state (scripts/mpc.py:102-124) */
    double* x_cur;                  /* [B][nx] */
    uint8_t *alive, *sa, *collided; /* [B]: still simulated / following a backup trajectory / failed */
    int64_t *ja, *last_x, *last_u;  /* [B]: abort clock; last valid row of the state / input logs */
    double *x_abort, *u_abort;      /* [B][Nb+1][nx], [B][Nb][nu]: backup trajectories */
    int64_t* step;                  /* [1]: the step counter j */
    double *x_log, *u_log;          /* step-major logs [n_steps+1][B][nx], [n_steps][B][nu] */
    int64_t* r_log;                 /* [n_steps][B] receding index used at each step, -1 where none (or NULL) */
    uint8_t* resumed;               /* [B]: written by smpc_loop_pre -- the instance left its backup trajectory at THIS step and
                                       steps its controller again (scripts/mpc.py:137-141); may be NULL */
} smpc_loop_state;

/* scripts/mpc.py:130-151 before the controller's step: PD tracking of the backup trajectory / hold / resume for the instances
 * in safe abort -> u_other[B][nu]; stepping[b] = alive and not in abort; logs r (may be NULL) of the stepping instances. */
int smpc_loop_pre(smpc_handle* h, int B, int Nb, const smpc_loop_state* ls, const int64_t* r, const uint8_t* pending,
                  double* u_other, uint8_t* stepping);

/* What the driver makes of the aborts the controllers raised in this step (abort[B] = smpc_policy_step's abort_out, updated
 * in place).  An abort raised by an instance that stepped normally is an abort EVENT (scripts/mpc.py:161-190: viable state
 * recorded, backup OCP solved): it stays set.  An abort raised on the very step an instance resumed MPC after a backup
 * trajectory (ls->resumed) happens inside the `if sa_flag:` branch of the reference (mpc.py:137-141), where no event is
 * opened: the instance simply is in safe abort again -- old backup trajectory, abort clock still running -- and re-tests its
 * velocity next step.  With reference_quirks != 0 that is what happens here (sa[b] = 1, abort[b] = 0); with 0 every abort is an
 * event.  *any_event (one int32) = 1 if an event remains, else 0. */
int smpc_loop_classify_aborts(smpc_handle* h, int B, const smpc_loop_state* ls, int reference_quirks, uint8_t* abort,
                              int32_t* any_event);

/* scripts/mpc.py:161-190, second half: the n_c abort events of the previous step, applied once their backup OCPs (solved as a
 * compact batch, possibly on another handle / stream that the caller has ordered before this call) are known.  rows[n_c] =
 * instance of each event, status_c[n_c] / x_c[n_c][Nb+1][nx] / u_c[n_c][Nb][nu] = the backup solves.  Solved: the instance
 * follows its backup trajectory from this step on (u[b] = PD law on its first node, clock 1), viable[b] += 1 (a saturating
 * count: mpc.py:189 appends the instance to viable_idx once per event and :277-278 removes it once); failed: lost at
 * the step of the event.  pending[b] (the flag smpc_loop_pre reads) is cleared.  Between the event and this call an instance
 * only has to be kept from stepping, which is what lets the backup solve overlap the next step's solve. */
int smpc_loop_apply_backup(smpc_handle* h, int B, int Nb, const smpc_loop_state* ls, int n_c, const int64_t* rows,
                           const int32_t* status_c, const double* x_c, const double* u_c, uint8_t* viable, double* u,
                           uint8_t* pending);

/* scripts/mpc.py:240-264 after it: logs u, plant step (smpc_plant_step semantics), state test of the new state
 * (par: x_min / x_max / tol_x / row check bounds), logs, outcome flags, next current state, j += 1. */
int smpc_loop_post(smpc_handle* h, int B, const smpc_policy_params* par, const smpc_loop_state* ls, const double* u,
                   const smpc_joint* joints_noisy, const double* tau_noise);

/* wait for the handle's stream */
int smpc_sync(smpc_handle* h);
/* the hipStream_t the handle enqueues on (for event timing by the caller) */
void* smpc_stream(smpc_handle* h);
/* device time of the kernels of the last smpc_solve_batch, measured with HIP events on the handle's stream:
 * ms[0] linearise (since round 4: the stage builder -- linearisation AND the set-up of the QP's stage records, one kernel),
 * ms[1] MLP, ms[2] QP (the interior point), ms[3] total.
 * Mirrors ocp_solver.get_stats('time_lin'|'time_qp'|'time_tot')
 * (controller.py:123-124,192-193).  Only valid when timing was enabled.  on = 1: HIP events + the in-kernel load-balance probe of
 * smpc_get_qp_wave_stats; on = 2: HIP events only (what a running loop can afford); 0: off. */
int smpc_enable_timing(smpc_handle* h, int on);
int smpc_get_timing(smpc_handle* h, float* ms4);
/* Split of ms[2] of smpc_get_timing: ms2[0] = the QP set-up (stage records + initial point; ~0, the stage builder has already
 * written them), ms2[1] = k_qp_ipm (the interior-point iterations) -- the per-kernel durations rocprofv3
 * --kernel-trace reports (acados: time_qp_solver_call). */
int smpc_get_qp_timing(smpc_handle* h, float* ms2);
/* The same durations for the solve `back` solves before the last one (0 = the last; the handle keeps the events of its last 64
 * timed solves), without waiting: ms6 = {linearise, MLP, k_qp_setup, k_qp_ipm, total, valid}.  valid = 0 (and the rest 0) when
 * there is no such solve or it has not finished yet.  Lets a loop that enqueues far ahead of the GPU collect per-kernel times of
 * its own launches afterwards (bench.py: kernel_ms_in_loop). */
int smpc_get_timing_history(smpc_handle* h, int back, float* ms6);
/* acc3[0] += sum of qp_iter[B], acc3[1] += number of status[b] != 0, acc3[2] += B -- device-side counters of a closed loop
 * (DEVICE pointers; qp_iter may be NULL), enqueued on the handle's stream. */
int smpc_accumulate_stats(smpc_handle* h, int B, const int32_t* status, const int32_t* qp_iter, unsigned long long* acc3);
/* Load balance of the last timed k_qp_ipm launch: out3[0] = mean busy time of a half-wavefront (= one instance), out3[1] =
 * first start to last end of any half-wavefront, both in microseconds of the constant 100 MHz clock, out3[2] = half-waves
 * counted.  out3[1] / out3[0] is the share of the launch spent waiting for its slowest instances. */
int smpc_get_qp_wave_stats(smpc_handle* h, double* out3);

#ifdef __cplusplus
}
#endif
#endif /* SMPC_H_ */
