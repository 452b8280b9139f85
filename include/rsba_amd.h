/* rsba_amd — C ABI of the MI355X-native bundle-adjustment hot path.
 *
 * Drop-in boundary for the path rsba runs through Ceres-Solver today.  Every entry
 * point cites the reference interface it replaces; paths are relative to /root/reference/src/rsba/.
 * Plain pointers and sizes only; no C++ / torch types.  All functions return an rsba_status (0 = OK),
 * never throw, and — like ceres::Problem — are not re-entrant on one handle.
 *
 * The C++ facade in include/rsba/ceres_facade.hpp maps rsba's CostFunction / Problem / Solve usage
 * onto these calls; INTEGRATION.md shows the reference-side binding.
 */
#ifndef RSBA_AMD_H_
#define RSBA_AMD_H_
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RSBA_AMD_ABI_VERSION 4

typedef enum rsba_status {
  RSBA_OK = 0,
  RSBA_ERR_INVALID_ARGUMENT = 1,
  RSBA_ERR_NO_DEVICE = 2,        /* no gfx950 device / HIP runtime unusable: there is NO CPU fallback */
  RSBA_ERR_HIP = 3,              /* a HIP call failed: see rsba_last_error() */
  RSBA_ERR_EVALUATION_FAILED = 4,/* some functor returned false (point behind camera, mat/cam.h:410-412) */
  RSBA_ERR_OUT_OF_MEMORY = 5,
  RSBA_ERR_UNSUPPORTED = 6,
  RSBA_ERR_COMM = 7
} rsba_status;

/* mat/cam.h:37-41 */
enum { RSBA_SHUTTER_GLOBAL = 0, RSBA_SHUTTER_HORIZONTAL = 1, RSBA_SHUTTER_VERTICAL = 2 };

/* The residual blocks CeresHandler::Add (CeresHandler.h:94-390) creates from a Session
 * (sfm.thrift:13-74), flattened: one block per observation over caller-owned parameter arrays.
 *   poses_per_frame == 2 -> RsBundleAdjustment (VideoSfmBaRs.h:15-84; CeresHandler.h:245-265)
 *   poses_per_frame == 1 -> ReprojectionError  (video_bundler_free.h:17-101; CeresHandler.h:266-280)
 *   calibrated != 0      -> intrinsics are data (Create(cam,obs) / Create(sess,opt,obs))
 *   calibrated == 0      -> intrinsics are a parameter block (CreateWithCam / Create(obs)),
 *                           shared sess.cam or per frame f.cam via frame_intrinsics (CeresHandler.h:260,277)
 * Parameter arrays are written back by rsba_solve / rsba_download_parameters, as ceres::Solve
 * mutates the blocks it was given (CeresHandler.h:253-255). */
typedef struct rsba_problem_desc {
  int32_t shutter;               /* sess.rs */
  int32_t scanlines[2];          /* sess.scanlines */
  int32_t interpolate_rotation;  /* opt.model.interpolateRotation (SfmOptions.h:25) */
  int32_t calibrated;            /* opt.model.calibrated (SfmOptions.h:27) */
  int32_t poses_per_frame;       /* f.poses.size(): 1 or 2 */
  int32_t num_frames, num_points, num_intrinsics;
  int64_t num_observations;
  double* poses;                 /* [F][P][6]  angle-axis world->camera, camera centre (mat/cam.h:354-366) */
  double* points;                /* [M][3] */
  double* intrinsics;            /* [NI][9] {fx,fy,k1,k2,p1,p2,k3,cx,cy} (mat/cam.h:23-34) */
  const int32_t* frame_intrinsics; /* [F] or NULL (= every frame uses intrinsics[0]) */
  const double* obs_xy;          /* [N][2] */
  const int32_t* obs_frame;      /* [N] */
  const int32_t* obs_point;      /* [N] */
  const uint8_t* pose_fixed_mask;   /* [F][P]: bit i set = coordinate i held fixed (SubsetParameterization,
                                       CeresHandler.h:350-382); 0x3f = SetParameterBlockConstant (:342-348); NULL = free */
  const uint8_t* point_constant;    /* [M] SetParameterBlockConstant on points (CeresHandler.h:288-300); NULL = free */
  const uint8_t* intrinsics_constant; /* [NI] (CeresHandler.h:284,347); NULL = free */
  double huber_a;                /* opt.ceres.huberLoss: > 0 -> one shared ceres::HuberLoss(a) (CeresHandler.h:85-90); any other loss: rsba_set_loss */
} rsba_problem_desc;

typedef struct rsba_handle rsba_handle;   /* stands for the ceres::Problem member of CeresHandler (CeresHandler.h:78) */

/* ceres::Solver::Options fields rsba writes (CeresHandler.h:403-412, VideoSfMHandler.cc:579-583)
 * plus the Ceres 1.9 defaults the LM loop depends on. */
typedef struct rsba_solver_options {
  int32_t max_num_iterations;               /* 50 (CeresHandler.h:405) / 20 (VideoSfMHandler.h:63) */
  int32_t jacobi_scaling;                   /* 1 */
  int32_t max_num_consecutive_invalid_steps;/* 5 */
  int32_t minimizer_progress_to_stdout;     /* CeresHandler.h:404 */
  double initial_trust_region_radius;       /* 1e4 */
  double max_trust_region_radius;           /* 1e16 */
  double min_trust_region_radius;           /* 1e-32 */
  double min_relative_decrease;             /* 1e-3 */
  double min_lm_diagonal, max_lm_diagonal;  /* 1e-6, 1e32 */
  double function_tolerance;                /* 1e-6 */
  double gradient_tolerance;                /* 1e-10 */
  double parameter_tolerance;               /* 1e-8 */
  int32_t level_scheduled_cholesky;         /* 0.  1 = factor the reduced camera system with one launch per elimination
                                             * level instead of the persistent task-DAG kernel (same arithmetic, same results,
                                             * no communication between workgroups inside a launch; slower) */
  int32_t profile_phases;                   /* 0.  1 = time the phases of every LM iteration with HIP events on the solver's
                                             * stream; read with rsba_get_phase_times after the solve */
} rsba_solver_options;

enum { RSBA_CONVERGENCE = 0, RSBA_NO_CONVERGENCE = 1, RSBA_FAILURE = 2 };   /* ceres::TerminationType subset */

/* ceres::IterationSummary subset (what minimizer_progress_to_stdout prints) */
typedef struct rsba_iteration {
  int32_t iteration, step_is_valid, step_is_successful, reserved;
  double cost, cost_change, gradient_max_norm, step_norm, relative_decrease, trust_region_radius, model_cost_change;
} rsba_iteration;

/* ceres::Solver::Summary subset rsba reads (VideoSfMHandler.cc:593-596,627-630) + phase times that
 * FullReport() prints */
typedef struct rsba_solver_summary {
  int32_t termination_type, num_successful_steps, num_unsuccessful_steps, num_iterations;
  int32_t num_residual_blocks, num_residual_blocks_reduced, num_parameters_reduced, is_solution_usable;
  double initial_cost, final_cost, fixed_cost;
  double total_time_s, residual_jacobian_time_s, linear_solver_time_s;
  int32_t num_dag_fallbacks;     /* linear solves of the persistent Cholesky driver whose residual check failed and that were
                                  * repeated on the level schedule (0 in every run so far) */
  int32_t reserved;
} rsba_solver_summary;

/* Pointers into HBM for callers that keep results on the device.  All fp64, tiled component-major:
 * observations (INTERNAL frame-major order; order_host[i] = caller's index of internal observation i)
 * are grouped in tiles of `tile` = 256; component c of observation i lives at
 *   base[(i / tile) * ncomp * tile + c * tile + (i % tile)]
 * with ncomp = 2 for residuals and 2*K for jacobians (component r*K + c = row r, column c; columns
 * ordered [cam 9]? [pose0 6] [pose1 6]? [point 3]). */
typedef struct rsba_device_view {
  double* residuals;
  double* jacobians;        /* NULL until an evaluation WITH Jacobians has run on the handle (the buffer — 16 K bytes per observation — is allocated then, not by the view) */
  int64_t tile;
  int32_t jacobian_cols;    /* K */
  int32_t reserved;
  const int64_t* order_host;/* host array [N] */
  double* poses; double* points; double* intrinsics;   /* device parameter arrays */
} rsba_device_view;

int32_t rsba_abi_version(void);
const char* rsba_status_string(int32_t status);
const char* rsba_last_error(void);                 /* thread-local detail for the last non-OK status */
int32_t rsba_device_count(int32_t* count);         /* RSBA_ERR_NO_DEVICE when none: callers must fail, not fall back */

/* == ceres::Problem construction + the AddResidualBlock loop (CeresHandler.h:78, 208-301): uploads the
 * flat problem once; `device` is the HIP device ordinal (one process per GPU). */
int32_t rsba_create(const rsba_problem_desc* desc, int32_t device, rsba_handle** out);
void rsba_destroy(rsba_handle* h);                 /* == ~Problem: frees every device buffer exactly once */

/* Run on a caller-owned HIP stream (hipStream_t as void*), e.g. torch's current stream; NULL = the
 * handle's own stream. */
int32_t rsba_set_stream(rsba_handle* h, void* hip_stream);

/* Parameter blocks are caller-owned in Ceres; these move them between the caller's arrays and HBM. */
int32_t rsba_upload_parameters(rsba_handle* h, const double* poses, const double* points, const double* intrinsics);
int32_t rsba_download_parameters(rsba_handle* h, double* poses, double* points, double* intrinsics);

/* The metric's "residual + Jacobian evaluation": == CostFunction::Evaluate over every residual block
 * (VideoSfmBaRs.h:53-80 / video_bundler_free.h:70-91 through AutoDiffCostFunction).  Asynchronous on the
 * handle's stream; results stay in HBM (rsba_get_device_view).  with_jacobians == 0 is the T=double path. */
int32_t rsba_evaluate_device(rsba_handle* h, int32_t with_jacobians);

/* == ceres::Problem::Evaluate(EvaluateOptions(), &cost, &residuals, &gradient, &jacobian)
 * (CeresHandler.h:386-387 uses the cost-only form).  Host outputs in the CALLER's observation order:
 * residuals [N][2]; jacobians [N][2][K] raw CostFunction blocks (no loss, no masks); gradient
 * [F*P*6 | M*3 | NI*9] = loss-corrected J^T r with zeros at fixed coordinates; cost = 1/2 sum rho(|r|^2).
 * Any output may be NULL.  num_failed receives the number of blocks whose functor returned false;
 * the status is then RSBA_ERR_EVALUATION_FAILED.  Motion prior blocks (rsba_set_motion_priors) count in cost, gradient
 * and num_failed; residuals / jacobians cover the observation blocks only. */
int32_t rsba_evaluate(rsba_handle* h, double* cost, double* residuals, double* jacobians, double* gradient, int64_t* num_failed);

/* Loss-corrected, masked normal-equation blocks at the current parameters (no damping, no Jacobi
 * scaling) — what Ceres' SchurEliminator consumes: U [F][CD][CD], gc [F][CD] with
 * CD = 6*poses_per_frame, V [M][3][3], gp [M][3]; host arrays, any may be NULL.  These per-camera blocks
 * are also the payload of the multi-GPU exchange.  Calibrated problems only.  Motion prior blocks contribute their
 * share of U and gc; the (f, f-1) blocks they add to the reduced camera system are not part of this output. */
int32_t rsba_normal_equations(rsba_handle* h, double* U, double* gc, double* V, double* gp);

int32_t rsba_get_device_view(rsba_handle* h, rsba_device_view* view);

/* Average device time of one evaluation launch, measured with hipEvents on the handle's stream
 * around `iters` back-to-back launches (after `warmup` untimed ones). */
int32_t rsba_time_evaluate(rsba_handle* h, int32_t with_jacobians, int32_t warmup, int32_t iters, double* avg_ms);

/* == ceres::Solve(options, &problem, &summary) with linear_solver_type = SPARSE_SCHUR
 * (CeresHandler.h:394-426): LM trust region, Schur elimination of the points, Cholesky of the reduced
 * camera system, all on the device; parameters are written back to the arrays given to rsba_create.
 * trace (may be NULL) receives up to trace_capacity iteration records.
 * The trust-region decisions themselves (TrustRegionMinimizer's accept / reject, radius, convergence tests) are taken by a device kernel
 * for every problem this call takes (calibrated, one shared or several intrinsics blocks; with or without motion priors — interFrameRatio
 * known or free —, GoodPosePrior blocks and the SphericalPrior; one rank or several) — the host then waits once per iteration for the
 * state, never inside one; the same rules on the host with options.profile_phases, when a rank of a sharded solve asks for it (no
 * observations) and under RSBA_DEVICE_LM=0.  The two forms produce the same iteration records bit for bit. */
void rsba_default_solver_options(rsba_solver_options* opt);
int32_t rsba_solve(rsba_handle* h, const rsba_solver_options* opt, rsba_solver_summary* summary,
                   rsba_iteration* trace, int32_t trace_capacity);

/* == the choice ceres::Solver::Options::linear_solver_type makes between the exact reduced solve (SPARSE_SCHUR / DENSE_SCHUR)
 * and ITERATIVE_SCHUR, the solver VideoSfMHandler::BA's min_linear_solver_iterations = 3 is meant for (VideoSfMHandler.cc:579-583:
 * the option is read by Ceres' iterative Schur solver only).  Mirrors linear_solver_type, min_linear_solver_iterations,
 * max_linear_solver_iterations and eta of ceres::Solver::Options.  Ceres is not part of the reference tree; the rules below are
 * THIS library's definition of the iterative solve:
 *   type 1 solves the reduced camera system S y = rhs of every LM iteration (S explicit, in its packed 48 x 48 tiles, after the
 *   same Schur elimination and damping as the exact solve) by conjugate gradients preconditioned with the block diagonal M of S:
 *   one CD x CD block per frame (CD = 6 * poses_per_frame), one 9 x 9 block per intrinsics parameter block, each Cholesky-factored
 *   once per linear solve.  From y_0 = 0: r_0 = rhs, z = M^-1 r, p = z; then q = S p, alpha = r.z / p.q, y += alpha p,
 *   r -= alpha q, z = M^-1 r, beta = r.z_new / r.z_old, p = z + beta p.  After iteration k >= min_iterations the solve stops when
 *     r_tolerance >= 0 and |r_k|_2 <= r_tolerance * |rhs|_2, or
 *     eta > 0 and k (Q_k - Q_k-1) / Q_k < eta with Q_k = -1/2 y_k.(rhs + r_k), Q_0 = 0 (the model's decrease has levelled off),
 *   and always at k = max_iterations: reaching the cap is no failure, the step is used as it is.  (eta <= 0 and r_tolerance < 0
 *   switch their test off.)  A block of M that is not positive definite, or a p.q that is not positive and finite, fails the linear
 *   solve: the LM step is invalid, as after a failed pivot of the exact solve.  Every sum has a fixed order: two solves of the same
 *   problem agree bit for bit.
 * rsba_set_linear_solver is valid between solves and takes effect at the next rsba_solve.  With type 1 the trust-region decisions
 * are taken by the host (once per chunk of CG iterations it reads the convergence flag), the time of the iterations counts in
 * RSBA_PHASE_CHOLESKY, rsba_pose_covariance keeps using the exact factorisation, and rsba_solve returns RSBA_ERR_UNSUPPORTED
 * (the handle stays usable) for a free interFrameRatio, for a handle with an exchange attached and together with
 * options.level_scheduled_cholesky.  Type 0 (the default) is the exact solve, bit for bit what it was.
 * rsba_get_linear_solver_stats: the counts of the last rsba_solve (all zero after one with type 0) and, of its last linear solve,
 * the iterations and |r|_2 / |rhs|_2 at the end. */
enum { RSBA_LINEAR_SOLVER_EXACT = 0, RSBA_LINEAR_SOLVER_PCG = 1 };
typedef struct rsba_linear_solver_options {
  int32_t type;                  /* 0: RSBA_LINEAR_SOLVER_EXACT (linear_solver_type SPARSE_SCHUR), 1: RSBA_LINEAR_SOLVER_PCG (ITERATIVE_SCHUR, JACOBI) */
  int32_t min_iterations;        /* 1    min_linear_solver_iterations (VideoSfMHandler.cc:583 sets 3) */
  int32_t max_iterations;        /* 500  max_linear_solver_iterations */
  int32_t reserved;
  double eta;                    /* 0.1  eta */
  double r_tolerance;            /* -1: off */
} rsba_linear_solver_options;
typedef struct rsba_linear_solver_stats {
  int64_t num_linear_solves, total_iterations;            /* of the last rsba_solve */
  int32_t max_iterations, num_solves_at_cap, num_failed_solves;
  int32_t last_iterations;                                /* of its last linear solve */
  double last_relative_residual;
} rsba_linear_solver_stats;
void rsba_default_linear_solver_options(rsba_linear_solver_options* opt);
int32_t rsba_set_linear_solver(rsba_handle* h, const rsba_linear_solver_options* opt);
int32_t rsba_get_linear_solver_stats(rsba_handle* h, rsba_linear_solver_stats* out);

/* == the loss function CeresHandler passes to every reprojection block and to the motion-prior blocks, beyond the one HuberLoss that
 * rsba_problem_desc::huber_a describes: the losses of ceres/loss_function.h (Ceres-Solver 1.9.0), one for the whole problem.  Ceres is
 * not part of the tree; the text below is THIS library's definition.
 * With s = |r|^2 of a residual block a loss returns rho = {rho(s), rho'(s), rho''(s)}; min = DBL_MIN; every form is evaluated as written:
 *   TRIVIAL                 rho = {s, 1, 0}
 *   HUBER(a)      b = a^2;  s <= b: {s, 1, 0};  s > b: with r = sqrt(s)  {2 a r - b, max(min, a / r), -rho1 / (2 s)}
 *   SOFT_L_ONE(a) b = a^2, c = 1 / b, sum = 1 + s c, t = sqrt(sum):      {2 b (t - 1), max(min, 1 / t), -(c rho1) / (2 sum)}
 *   CAUCHY(a)     b = a^2, c = 1 / b, sum = 1 + s c, inv = 1 / sum:      {b log(sum), max(min, inv), -c inv^2}
 *   ARCTAN(a)     b = 1 / a^2, sum = 1 + s^2 b, inv = 1 / sum:           {a atan2(s, a), max(min, inv), -2 s b inv^2}
 *   TOLERANT(a, b) c = b log(1 + exp(-a / b)), x = (s - a) / b;  x > 36.7: {s - a - c, 1, 0};
 *                 otherwise with e = exp(x)                              {b log(1 + e) - c, max(min, e / (1 + e)), 0.5 / (b (1 + cosh x))}
 * and scale > 0 multiplies all three (ceres::ScaledLoss; 1 = no scaling).
 * The corrector (ceres corrector.cc) is the same for every loss.  If s == 0 or rho2 <= 0: r~ = sqrt(rho1) r, J~ = sqrt(rho1) J.
 * Otherwise D = 1 + 2 s rho2 / rho1, alpha = 1 - sqrt(D), r~ = sqrt(rho1) / (1 - alpha) r, J~ = sqrt(rho1) (J - (alpha / s) r (r^T J)).
 * The cost of a block is rho0 / 2 of the UNcorrected residual.  Of the set only TOLERANT has rho2 > 0.
 * The loss applies exactly where huber_a applies: reprojection blocks and motion-prior blocks; never to GoodPosePrior / SphericalPrior
 * blocks, PnP, the filter or track creation.
 * rsba_set_loss is valid between calls and takes effect at the next rsba_evaluate / rsba_gradient / rsba_solve / rsba_pose_covariance.
 * A handle created with huber_a > 0 reports {HUBER, a, scale 1}, one created without {TRIVIAL, scale 1}; rsba_set_loss({HUBER, a, scale 1})
 * gives the bits of a handle created with huber_a = a, and TRIVIAL at scale 1 those of one created without a loss: both run the code
 * they ran before this call existed.  RSBA_ERR_INVALID_ARGUMENT (the handle keeps its loss) for a, TOLERANT's b or scale that is not
 * positive and finite (a and b are ignored where the type does not use them), and for an unknown type.
 * Several ranks (rsba_set_exchange): every rank sets the same loss before the collective call. */
enum { RSBA_LOSS_TRIVIAL = 0, RSBA_LOSS_HUBER = 1, RSBA_LOSS_SOFT_L_ONE = 2, RSBA_LOSS_CAUCHY = 3, RSBA_LOSS_ARCTAN = 4, RSBA_LOSS_TOLERANT = 5 };
typedef struct rsba_loss {
  int32_t type, reserved;
  double a, b, scale;
} rsba_loss;
void rsba_default_loss(rsba_loss* loss);                       /* TRIVIAL, a = b = 0, scale 1 */
int32_t rsba_set_loss(rsba_handle* h, const rsba_loss* loss);
int32_t rsba_get_loss(rsba_handle* h, rsba_loss* out);

/* Measurement aids: where an LM iteration spends its device time, and the sizes of the symbolic plan the
 * kernels' algorithmic bytes / flops follow from.  Phase p covers the launches listed; ms[p] is the HIP-event time summed
 * over the last rsba_solve that ran with options.profile_phases != 0, calls[p] how many times the phase ran. */
enum {
  RSBA_PHASE_EVAL_LM = 0,        /* eval_kernel<.., kLmJacobian> + cost reduction: r, J (loss-corrected, scaled) as per-wave camera blocks (point-major records only with several intrinsics blocks) */
  RSBA_PHASE_CAMERA_BLOCKS = 1,  /* per-frame J^T J / J^T r blocks (+ intrinsics border) from the per-wave partials */
  RSBA_PHASE_POINT_BLOCKS = 2,   /* V_j, g_p,j */
  RSBA_PHASE_POINT_FACTOR = 3,   /* (V_j + D^2)^-1 factors, z_j */
  RSBA_PHASE_PROJECT = 4,        /* P records (+ virtual intrinsics records) */
  RSBA_PHASE_SCHUR = 5,          /* clear + Schur tile products + merge: S, rhs */
  RSBA_PHASE_CHOLESKY = 6,       /* factor + forward / backward solve of the reduced camera system */
  RSBA_PHASE_BACK_SUBSTITUTE = 7,/* point steps + model cost change */
  RSBA_PHASE_CANDIDATE = 8,      /* x + delta, |step|, |x| */
  RSBA_PHASE_EVAL_TRIAL = 9,     /* evaluation of the candidate + cost reduction: in LM mode (the linearisation an accepted step re-uses) when the problem keeps no records, residual-only otherwise */
  RSBA_PHASE_PRIORS = 10,        /* motion-prior blocks, cost and model terms */
  RSBA_PHASE_EXCHANGE = 11,      /* multi-GPU all-reduces (pack / collective / unpack) */
  RSBA_PHASE_OTHER = 12,         /* diagonal clamp, gradient norm, scalar packing */
  RSBA_NUM_PHASES = 13
};
typedef struct rsba_phase_times { double ms[RSBA_NUM_PHASES]; int32_t calls[RSBA_NUM_PHASES]; int32_t reserved; } rsba_phase_times;
int32_t rsba_get_phase_times(rsba_handle* h, rsba_phase_times* out);
const char* rsba_phase_name(int32_t phase);
typedef struct rsba_plan_stats {
  int64_t tiles, factor_tiles, levels, tasks;       /* 48 x 48 tiles of S, tiles of its factor after fill, elimination levels, Cholesky tasks */
  int64_t schur_entries, schur_chunks;              /* (point, tile pair) entries of the Schur work list, workgroups */
  int64_t schur_block_products;                     /* CD x 3 by 3 x CD block products that are not structurally zero */
  int64_t cholesky_flops;                           /* of the tile factorisation incl. fill, forward and backward solve */
  int64_t exchange_doubles;                         /* payload (2) of the multi-GPU exchange: the structurally non-zero tiles of S + rhs */
  int64_t schur_groups;                             /* (point, frame tile) groups of P records */
  int64_t schur_mfma_issued, schur_launches;        /* fp64 MFMAs (2048 flop each) the Schur kernel issued so far — all-zero operand blocks are skipped — over so many launches */
  int64_t sharded_factorisation;                    /* 1: several ranks, each factoring its own part of the elimination tree (the points follow rsba_partition_points);
                                                     * exchange_doubles is then the separators' tiles | their rhs rows | the gather of the camera step */
  int64_t separator_tiles, separator_factor_tiles;  /* tile columns in the separators all ranks share, and tiles of the factor inside them (what exchange (2) carries) */
  int64_t local_tasks, separator_tasks;             /* Cholesky tasks of this rank's part (forward) / of the separators incl. both backward solves */
  int64_t local_levels, separator_levels;           /* the two dependency chains: elimination levels inside this rank's part / levels that hold a separator column */
  int64_t schur_group_bytes, schur_factored_groups; /* bytes of all groups: 3 x 48 doubles each in full form; 80 doubles for the groups stored FACTORED (two-pose frame tiles: the
                                                     * 6-row factor q = Jq^T Jp L^-T per frame + tau instead of the 12 rows (1 - tau) q | tau q), and how many those are */
  int64_t device_loop_solves, host_loop_solves;     /* rsba_solve calls on this plan whose trust-region loop ran without the host (decisions by device kernels: every problem rsba_solve takes,
                                                     * phase timing excepted) / with the host deciding */
} rsba_plan_stats;
int32_t rsba_get_plan_stats(rsba_handle* h, rsba_plan_stats* out);   /* runs the symbolic phase if it has not run yet */

/* ---- the steps either side of the solve: batched reprojection / validation filter ----
 * == vision::sfm::validate(sess, f, opt, pt, obs) for every observation of the problem
 * (struct/VideoSfM.cc:159-169 with getPose :103-133; callers: CeresHandler.h:239-243 revalidateReprojections,
 * VideoSfMHandler.cc evalTracks / createTracks): valid[i] = 1 iff |camera centre at the observation's scan
 * line - point| >= min_distance (opt.tracks.minDistanceToCamera) and the squared reprojection error <
 * sq_threshold (opt.tracks.sqrdThreshold).  Unlike the cost functor, tau is taken from the TRUE observation
 * (x for HORIZONTAL, y for VERTICAL).  valid is a host array [N] in the caller's observation order. */
int32_t rsba_validate_observations(rsba_handle* h, double sq_threshold, double min_distance, uint8_t* valid);
/* == vision::sfm::reproject(sess, f, opt, pt, obs) (struct/VideoSfM.cc:139-155) for n (frame, point) pairs:
 * fixed point on the scan-line time from the principal point, at most 49 projections, converged when the
 * projection moves <= 1e-3 px.  xy_out [n][2], ok_out [n] (host arrays). */
int32_t rsba_reproject(rsba_handle* h, const int32_t* frames, const int32_t* points, int64_t n, double* xy_out, uint8_t* ok_out);

/* The same two filters for ONE frame without a handle — the shape vision::sfm::validate / reproject are called in
 * (CeresHandler.h:220-243: the observations of the frame being added against the tracks' points): cam[9], poses
 * [num_poses][6], points [n][3], obs_xy [n][2]; valid / ok_out [n], xy_out [n][2]; all host arrays.  num_poses 1: that pose;
 * 2: interpolate_rs at the item's scan line; MORE ("fullDoF", a pose per scan line): the pose getPose picks for the item,
 * poses[round(clamp(line, 0, num_poses - 1))] with line = x for HORIZONTAL, y otherwise (struct/VideoSfM.cc:118-132) — reproject
 * re-picks it in every step of its fixed point, as the reference does.  Each host
 * thread keeps one device arena, pinned staging buffer and stream between calls, so a call is one upload, one launch and
 * one download. */
int32_t rsba_validate_frame(int32_t device, const double* cam, const double* poses, int32_t num_poses, int32_t shutter, const int32_t* scanlines,
                            int32_t interpolate_rotation, const double* points, const double* obs_xy, int64_t n, double sq_threshold,
                            double min_distance, uint8_t* valid);
int32_t rsba_reproject_frame(int32_t device, const double* cam, const double* poses, int32_t num_poses, int32_t shutter, const int32_t* scanlines,
                             int32_t interpolate_rotation, const double* points, int64_t n, double* xy_out, uint8_t* ok_out);

/* == the geometric predicates of VideoSfMHandler::createTracks / reprojectMatches (VideoSfMHandler.cc:231-372) for a batch of
 * candidates, without a handle.  A candidate is a pair (o = cand_a[c], o2 = cand_b[c]) of indices into the observations; its
 * request[c] holds RSBA_TRACK_* bits:
 *   RSBA_TRACK_TRIANGULATE: tri_ok[c] = 1 iff getPose(o) and getPose(o2) differ bitwise (memcmp, :321), both directions exist
 *     (undistortion converged, mat/cam.h:154-176), det(A) >= DBL_EPSILON in triangulate (mat/cam.h:188-231; the reference aborts
 *     there), neither camera centre is nearer than min_distance to the point, and vision::validate holds on both sides
 *     (:326-337).  tri_pt[c][3] is the triangulated point whenever the 3x3 solve ran, else 0.
 *   RSBA_TRACK_REPROJECT: reproj_ok[c] = vision::sfm::validate(sess, frame of o, opt, track_pt[c], o) (struct/VideoSfM.cc:159-169):
 *     the distance gate and the reprojection check of reprojectMatches (:250-262), both at getPose(o).
 * Frames: cams [num_cams][9] with frame_cam [F] (NULL when num_cams == 1); poses [pose_offset[F]][6] with pose_offset [F + 1]
 * (pose_offset[0] = 0, non-decreasing): a frame's 1 pose, 2 (interpolate_rs at the observation's scan line) or more (one per
 * scan line, struct/VideoSfM.cc:118-132).  Observations: obs_frame [num_obs] in [0, F), each of a frame with poses; obs_xy
 * [num_obs][2].  Outputs in the caller's candidate order; an output may be NULL only when no candidate asks for it
 * (track_pt likewise); a bit not asked for gives 0.  All host arrays.  The ray pass (getPose, undistortion, rotation) runs once
 * per observation and only when some candidate asks for a triangulation.  Each host thread keeps one device arena, pinned
 * staging buffer and stream between calls, as for rsba_validate_frame; there is no CPU fallback. */
enum { RSBA_TRACK_TRIANGULATE = 1, RSBA_TRACK_REPROJECT = 2 };
int32_t rsba_track_candidates(int32_t device, const double* cams, int32_t num_cams, const int32_t* frame_cam, int32_t num_frames,
                              const double* poses, const int64_t* pose_offset, int32_t shutter, const int32_t* scanlines, int32_t interpolate_rotation,
                              const int32_t* obs_frame, const double* obs_xy, int64_t num_obs, const int32_t* cand_a, const int32_t* cand_b,
                              const uint8_t* request, const double* track_pt, int64_t num_cand, double sq_threshold, double min_distance,
                              uint8_t* tri_ok, double* tri_pt, uint8_t* reproj_ok);

/* == the neighbour search of VideoSfMClient::Match (VideoSfMClient.cc:73-129: cv::BFMatcher().knnMatch, NORM_L2, no cross-check)
 * for a list of (query frame, train frame) pairs, as parseFrame forms them (:196-201), without a handle.  OpenCV is not part of
 * the reference tree; the rules below are THIS library's definition of the search:
 *   distance(i, j) = sqrtf(float(sum_c (q_ic - t_jc)^2)); for every query row i the k' = min(k, n_train) train rows with the
 *   smallest distance, ascending; TIES GO TO THE LOWER TRAIN INDEX.  A pair with n_train < 2 yields no neighbours (the
 *   reference reads ms[1] out of bounds there), a pair with n_query == 0 none either (the reference divides by zero).
 * desc [frame_offset[num_frames]][dim] holds every frame's descriptors, frame f's rows at frame_offset[f] .. frame_offset[f + 1]
 * (frame_offset[0] = 0, non-decreasing).  dim must be 128 (FEATURE_SIZE, struct/VideoSfM.cc:11-13): RSBA_ERR_UNSUPPORTED
 * otherwise.  k in [1, 5] (Match asks for 2, or 5 with `multiple`).  Pair p searches frame pair_query[p]'s rows among frame
 * pair_train[p]'s; a frame may serve in any number of pairs, as query and as train.  The descriptors must be FINITE: they are
 * not checked, and a NaN or an infinity gives an unspecified result for the queries it touches.
 * Outputs (host arrays): pair p's results start at slot out_offset[p] (a non-negative multiple of k; the pairs' ranges must not
 * overlap), k slots per query: nn_index (train row within its frame) and nn_dist, ordered by (distance, index); slots past k'
 * hold index -1 and distance +inf.  nn_count[out_offset[p] / k + i] = k' of pair p's query i, 0 for a pair with n_train < 2.
 * The arrays must reach the largest end = out_offset[p] + k * n_query(p), and the call writes ALL of [0, end): slots (and counts)
 * in gaps that the pairs' ranges leave come back as unused (-1, +inf, 0), whatever they held.
 * Exactness: the search runs in the GEMM form ||q||^2 + ||t||^2 - 2 q.t on the f32 matrix cores, the k' survivors' distances
 * are recomputed in the direct form above (an fmaf chain in c order).  For integer-valued descriptors in [0, 255] — what
 * OpenCV's SIFT emits — every intermediate is an integer below 2^24, so indices, counts and distances equal the integer
 * restatement bit for bit.  For general data the search may confuse neighbours whose squared distances differ by less than
 * ~130 * 2^-24 * (||q||^2 + ||t||^2 + 2 sum |q_c||t_c|); the reported distance is always the direct form's.
 * Each host thread keeps one device arena, pinned staging buffer and stream between calls, as for rsba_track_candidates; there
 * is no CPU fallback.
 * rsba_match_last_kernel_ms (a measurement aid for tools/match_time.py, no part of the matching itself): the HIP-event time of
 * the three kernel passes of the calling thread's last successful rsba_match_descriptors call that reached the device.
 * RSBA_ERR_INVALID_ARGUMENT when ms is NULL or this thread has made no such call yet. */
int32_t rsba_match_descriptors(int32_t device, const float* desc, int32_t dim, const int64_t* frame_offset, int32_t num_frames,
                               const int32_t* pair_query, const int32_t* pair_train, int64_t num_pairs, int32_t k,
                               const int64_t* out_offset, int32_t* nn_index, float* nn_dist, int32_t* nn_count);
int32_t rsba_match_last_kernel_ms(float* ms);

/* == the covariance blocks VideoSfMHandler::BA prints with opt.debug.calcCovariances (VideoSfMHandler.cc:602-621:
 * ceres::Covariance::Compute on (p0,p0), (p0,p1), (p1,p1) of a frame): cov [CD][CD] row-major,
 * CD = 6 * poses_per_frame, = the (frame, frame) block of (J^T J)^-1 at the current parameters, loss function applied,
 * zero rows / columns at fixed coordinates.  RSBA_ERR_UNSUPPORTED when J^T J is rank deficient (Compute returns false). */
int32_t rsba_pose_covariance(rsba_handle* h, int32_t frame, double* cov);

/* == the covariance of EVERY frame at once — and of pairs of frames, and of the intrinsics blocks — where rsba_pose_covariance
 * returns one (frame, frame) block for CD solves through the factorisation.  rsba_covariance_compute linearises and factors exactly
 * as rsba_pose_covariance does (same refusals: RSBA_ERR_UNSUPPORTED when J^T J is rank deficient, RSBA_ERR_EVALUATION_FAILED), then
 * forms Sigma = S^-1 of the reduced camera system on the tile pattern of its Cholesky factor (48 x 48 tiles, after fill) by the
 * Takahashi recurrence — about one more factorisation's worth of tile products — and keeps it on the device: two arrays of the
 * factor's size, allocated by the first compute and given back by rsba_covariance_release or rsba_destroy.  A block of Sigma is the
 * same block of (J^T J)^-1 (points, priorPoses blocks eliminated; the column of a free interFrameRatio added as the bordered inverse).
 * One rank only: a handle with an exchange attached (rsba_set_exchange) is refused with RSBA_ERR_UNSUPPORTED.
 *   rsba_covariance_frame_blocks: cov [n][CD][CD] row-major, block p = the (frame_a[p], frame_b[p]) block; (a, b) with a > b is the
 *     transpose of (b, a) bit for bit; zero rows / columns at fixed coordinates, at the data slot of a one-pose frame and at
 *     coordinates no residual touches.  Every (f, f) is available, and (f, g) where the two frames' tiles share a tile of the factor
 *     (co-visible frames, frames linked by a prior, and whatever fill adds); any other pair: RSBA_ERR_UNSUPPORTED naming the pair,
 *     nothing written, the handle and the computed covariance stay usable.
 *   rsba_covariance_intrinsics_block: cov [9][9] of intrinsics parameter block `block` (uncalibrated problems), zeros where constant.
 *   rsba_covariance_point_blocks: cov [n][3][3], block p = the (point, point) block of point points[p] (points == NULL: points 0 .. n - 1,
 *     n <= num_points) — V^-1 + V^-1 (sum over the point's pairs of observations W_o^T Sigma W_o') V^-1, plus the border's term.  The
 *     frames of one point always share tiles of the factor, so every point is available.  Exact zeros for a constant point and for a
 *     point without observations; a point whose frames and intrinsics are all constant gives V^-1.
 *   rsba_covariance_memory: the device memory the covariance holds on the handle at the moment (the two tile arrays, two vectors of the
 *     camera-side length, and the lists of the recurrence, which stay with the plan after a release), in bytes.
 * The getters return RSBA_ERR_INVALID_ARGUMENT ("no covariance computed") before the first compute, after rsba_covariance_release and
 * after any call that moves the parameters or changes the problem: rsba_solve, rsba_upload_parameters, rsba_set_loss,
 * rsba_set_linear_solver.  The calls leave the handle as they found it: a later rsba_solve or rsba_pose_covariance gives what it
 * gives on a fresh handle, bit for bit.  Cross blocks of a pose and a point, or of two points, are not part of this interface. */
int32_t rsba_covariance_compute(rsba_handle* h);
int32_t rsba_covariance_frame_blocks(rsba_handle* h, const int32_t* frame_a, const int32_t* frame_b, int64_t n, double* cov);
int32_t rsba_covariance_intrinsics_block(rsba_handle* h, int32_t block, double* cov);
int32_t rsba_covariance_point_blocks(rsba_handle* h, const int32_t* points, int64_t n, double* cov);
int32_t rsba_covariance_memory(rsba_handle* h, int64_t* bytes);
int32_t rsba_covariance_times(rsba_handle* h, double* ms5);   /* HIP-event times, ms: G, OFF, DIAG launches of the last compute; the last point getter's kernel; the last gather's — taken in a process started with RSBA_COV_TIMES=1 only, zeros otherwise */
int32_t rsba_covariance_release(rsba_handle* h);

/* == the frame-to-frame motion priors CeresHandler::Add attaches to a rolling-shutter frame (CeresHandler.h:147-185;
 * SURVEY §8f row f1): one 12-residual block per listed frame f >= 1 over (f.poses[0], f.poses[1], f-1.poses[0],
 * f-1.poses[1]) — RsConstVeloPrior (kind 1, video_bundler_rs_inter.h:55-108) or RsConstAccelerationPrior (kind 2,
 * :113-173) with weight `scale` (opt.ceres.constFrameVelocity / constFrameAcceleration), rotation rows down-scaled
 * by 0.01, under the problem's loss function (huber_a).  inter_frame_ratio is opt.ceres.interFrameRatio: a CONSTANT
 * block — the case the reference takes when the option is != 1 (CeresHandler.h:175-177) — unless
 * rsba_set_inter_frame_ratio_free (below) makes it the free, lower-bounded parameter of the reference's default.
 * The blocks count in cost, gradient, num_residual_blocks and the solve; their validity flag (ratio >= 0 resp.
 * >= DBL_EPSILON) fails the evaluation like any functor returning false.  Needs poses_per_frame == 2 and a calibrated
 * or shared-intrinsics problem.  frames strictly increasing; must precede the first solve / gradient call;
 * kind 0 or count 0 removes them.  With rsba_set_exchange every rank passes the same list (rank 0 contributes them). */
int32_t rsba_set_motion_priors(rsba_handle* h, int32_t kind, double scale, double inter_frame_ratio, const int32_t* frames, int32_t count);
/* The reference's DEFAULT for these priors (opt.ceres.interFrameRatio left at 1, CeresHandler.h:175): the ratio is a free
 * parameter block with a lower bound (0 for kind 1, DBL_EPSILON for kind 2; :161,:172).  is_free != 0 makes rsba_solve
 * treat it so: one more unknown of the LM (its column is a 1-wide dense border of the reduced camera system, served by a
 * second solve through the factorisation), the candidate projected onto the bound as Ceres' ParameterBlock::Plus does,
 * the gradient norm taken of the projected gradient.  Ceres' extra projected line search for bounded problems (>= 1.10)
 * is not restated: steps follow the plain trust-region rules.  rsba_get_inter_frame_ratio returns the current value
 * (the solved one after rsba_solve).  Must precede the first solve / gradient call; evaluate / gradient treat the ratio
 * as the constant it currently is; rsba_pose_covariance includes its column (the pose block of the bordered inverse). */
int32_t rsba_set_inter_frame_ratio_free(rsba_handle* h, int32_t is_free);
int32_t rsba_get_inter_frame_ratio(rsba_handle* h, double* ratio);

/* == the per-pose prior blocks of CeresHandler::Add, neither with a loss function (nullptr in the reference):
 *   GoodPosePrior (CeresHandler.h:52-73, attached at :188-204 when opt.ceres.trustPriorCamRotation / trustPriorCamPosition are set
 *     and the frame has priorPoses): 6 residuals W (prior - pose) over TWO parameter blocks — the frame's priorPoses[i], a FREE
 *     block like every block Ceres is handed, and poses[i]; rotation rows times `rotation`, position rows times `position`; the
 *     functor fails when residual[0] >= 1.  pose_blocks[k] = f * poses_per_frame + i, distinct; prior_values [count][6] are the
 *     caller's priorPoses blocks: rsba_solve writes the solved values back, rsba_upload_parameters re-reads them.
 *   SphericalPrior (:36-50, attached at :127-130 to poses[0] of frame 1 of a session that starts at the origin): residuals
 *     |rot|^2 and 1e20 (1 - |cx| - |cy| - |cz|); fails when |rot|^2 >= 1.  spherical_pose_block = its pose block, -1 = none.
 *     (A 1e20-weighted residual: once it is met, its value is rounding noise times 1e20 — the cost Ceres and this library
 *     report then carries that noise; see DESIGN.md.)
 * The blocks count in cost, gradient (pose coordinates), num_residual_blocks and the solve; the priorPoses blocks are eliminated
 * in closed form like points.  Must precede the first solve / gradient call.  With rsba_set_exchange every rank passes the same
 * blocks (rank 0 contributes them). */
int32_t rsba_set_pose_priors(rsba_handle* h, double rotation, double position, const int32_t* pose_blocks, double* prior_values, int32_t count,
                             int32_t spherical_pose_block);

/* Sessions that mix rolling-shutter frames (two poses) with one-pose frames: CeresHandler::Add picks the functor per frame by
 * f.poses.size() (CeresHandler.h:245-286) — RsBundleAdjustment over (poses[0], poses[1], point) or ReprojectionError over
 * (getPose(...), point).  Create the problem with poses_per_frame = 2 and flag the one-pose frames here: is_global [num_frames],
 * 1 = the frame's observations use poses[f][0] alone (tau = 0; the validation / reprojection filters follow: getPose returns the
 * single pose, struct/VideoSfM.cc:103-133); the second pose slot of such a frame is not a parameter block — it is held constant and
 * left untouched.  NULL clears the flags.  Call before the first evaluation / solve.
 * Frames with MORE than two poses ("fullDoF", a pose per scan line; struct/VideoSfM.cc:83-97, CeresHandler.h:266-285) are the same
 * case once more: an observation of such a frame is a ReprojectionError block over ONE pose block, getPose's pick
 * poses[round(clamp(line, 0, size - 1))].  Every pose block that some observation picks is a "frame" of the flat problem (one-pose
 * problem, or a flagged frame of a two-pose one), obs_frame names it, pose blocks nobody picks are not part of the problem — as in
 * Ceres, which never hears of them.  include/rsba/ceres_handler.hpp (getPose + the facade's block-address lowering) and
 * rsba_amd/problem.py::lower_scanline_poses do exactly this. */
int32_t rsba_set_global_shutter_frames(rsba_handle* h, const uint8_t* is_global);

/* The symbolic phase of a handle's first solve works in ~40 bytes of host memory per observation.  That scratch is kept by the
 * library between handles (a fresh handle per call is windowedBA's pattern, VideoSfMHandler.cc:185-214, and mapping / unmapping
 * it per call cost more than the passes that fill it), and so are the device blocks, streams, events and the small pinned block of
 * destroyed handles (rsba_amd/csrc/devmem.hpp; device blocks up to RSBA_DEVICE_CACHE_MB, default 2048); this call gives all of it
 * back.  Safe at any time; the next handle simply allocates again. */
void rsba_release_host_scratch(void);

/* == the RANSAC hypotheses of vision::solveRsPnPRansac (solveRSpnp.cpp:413-524), batched: task t is
 * what pnpTask (:265-335) does for the subset subsets[t][0..m) of the n float points —
 *   skipped (status 0, nothing else written) when drop_coincident != 0 and two of its 3-D points coincide (:283-293;
 *   the final refinement over the inliers, :496-502, is the same call with drop_coincident = 0);
 *   vision::solveRsPnP (:100-192) from init_poses: ceres::Solve over the two pose blocks of one rolling-shutter frame,
 *   one RsBA<float> residual block per point (:25-97; w2i without validation, tau from observed_x), max_num_iterations
 *   (the reference: 10), all other options Ceres defaults; poses_out[t] = the result if usable (status 1), else the
 *   initial poses (status 2);
 *   num_inliers[t] = points whose float-rounded projection at the scan line of the TRUE observation lies closer than
 *   reprojection_error (float distance) to the observation (:225-258, :304-310).
 * Poses are rsba's 6-vectors (angle-axis world->camera, camera centre): [pose, pose2]; the rvec/tvec conversions of
 * :119-128, :166-176 and the OpenCV GS initialisation (:111-117) stay with the caller.  init_stride 12 = one initial
 * pair per task, 0 = one shared pair.  All pointers are host arrays; final_cost / num_inliers may be NULL.
 * rsba_pnp_inliers returns the inlier flags [n] of one pose pair (the winning hypothesis' list, :312-326). */
int32_t rsba_pnp_tasks(int32_t device, const double* cam, int32_t shutter, const int32_t* scanlines, const float* object_points,
                       const float* image_points, int32_t n, const int32_t* subsets, int32_t m, int32_t num_tasks,
                       const double* init_poses, int32_t init_stride, int32_t max_num_iterations, int32_t drop_coincident, float reprojection_error,
                       double* poses_out, uint8_t* status, double* final_cost, int32_t* num_inliers);
int32_t rsba_pnp_inliers(int32_t device, const double* cam, int32_t shutter, const int32_t* scanlines, const float* object_points,
                         const float* image_points, int32_t n, const double* poses, float reprojection_error, uint8_t* inlier_mask);

/* == the start poses of the global-shutter RANSAC hypotheses (include/rsba/solve_rs_pnp.hpp: solveGsPnPRansac, what cv::solvePnPRansac
 * does at solveRSpnp.cpp:437-449 and VideoSfMHandler.cc:715-730): pnp_detail::dlt_pose for every subset, on the device.  The image points
 * are undistorted and normalised once per call (hyp_detail::normalised_point, include/rsba/hyp_host.hpp), then one lane per subset runs the whole of dlt_pose: the
 * collinear / planar tests on the 3 x 3 scatter, the homography of a planar target or the 12 x 12 Gram matrix with its two gap tests, the
 * nearest rotation, the pose.  m >= 6.  poses_out are rsba's 6-vectors.
 * status[t]: 0 declined (degenerate subset; poses_out[t] untouched), 1 general DLT, 2 planar branch. */
int32_t rsba_pnp_dlt(int32_t device, const double* cam, const float* object_points, const float* image_points, int32_t n,
                     const int32_t* subsets, int32_t m, int32_t num_tasks, double* poses_out /* [num_tasks][6] */, uint8_t* status);

/* the whole global-shutter hypothesis batch of solveGsPnPRansac in one call: normalise, DLT, the refinement of
 * rsba_pnp_tasks with shutter GLOBAL from each subset's DLT pose (both pose slots the same), inlier counts.
 * The start poses never leave the device. status[t]: 0 declined by the DLT, 1 refined and usable, 2 refinement
 * unusable (poses_out[t] = the DLT pose). final_cost / num_inliers may be NULL. */
int32_t rsba_pnp_gs_hypotheses(int32_t device, const double* cam, const float* object_points, const float* image_points, int32_t n,
                               const int32_t* subsets, int32_t m, int32_t num_tasks, int32_t max_num_iterations, float reprojection_error,
                               double* poses_out /* [num_tasks][6] */, uint8_t* status, double* final_cost, int32_t* num_inliers);

/* == the minimal solver of the global-shutter RANSAC (what cv::solvePnPRansac(..., CV_P3P) runs per sample, VideoSfMHandler.cc:726-731;
 * OpenCV is not in the reference tree, so this text is the definition; include/rsba/solve_rs_pnp.hpp: pnp_detail::p3p_pose is its host form).
 * A subset has four indices: the first three are solved, the fourth chooses among the solutions.
 *   Inputs.  Image points undistorted and normalised as hyp_detail::normalised_point does; bearings j_i = (x, y, 1) / |(x, y, 1)|.
 *   Solve.  Grunert's formulation: with depths s_i along j_i, sides a = |P2 P3|, b = |P1 P3|, c = |P1 P2| and the cosines of the angles
 *     between the bearings, s2 = u s1, s3 = v s1 turn the three cosine laws into u = N(v) / (2 D(v)), D(v) = j1.j2 - v j2.j3, and a
 *     quartic in v.  All of its roots with three positive depths are looked for, in t = v / (1 + v) in (0, 1): the four intervals between
 *     the roots of the derivative (found the same way from the second and third derivatives) are bisected 40 times each where the
 *     quartic changes sign, every root is polished by two Newton steps.  Every loop has a fixed bound.
 *     The quartic loses its leading coefficient when the angle under which the camera sees P2 P3 equals the triangle's angle at P1 or its
 *     supplement (the camera centre on the surface the circumcircle sweeps when turned about P2 P3): the lost root is v = infinity,
 *     s1 = 0 — the camera centre in P1, not a solution with positive depths.  In t that root is t = 1, outside the open interval, and
 *     nothing is divided by the leading coefficient: the remaining roots are found as everywhere else.
 *     u divides by D(v), which vanishes where s1 j1.j2 = s3 j2.j3 (P1 and P3 project onto the second ray at the same point); a root
 *     with |D| <= 1e-12 (in units of s1 + s3) is dropped.
 *   Pose per solution.  The rigid motion that takes the three world points onto s_i j_i: the two triangles are congruent, so it is
 *     F E^T for their orthonormal triads (first edge, normal, their cross product) and maps centroid to centroid; converted to
 *     rsba's 6-vector by hyp_detail::pose_from_rt.
 *   Choice.  A solution is admissible when its three depths are positive (above 1e-9 b: the camera centre in a world point, where the
 *     lost root ends up under rounding, is no solution) and it puts the fourth point in front of the camera (z > 0).
 *     Among the admissible ones the smallest distance between the fourth point's projection and its normalised image point wins; ties go to
 *     the solution found first, roots in ascending t (ascending s3 / s1).
 *   Declined (status 0, poses_out[t] untouched, num_solutions[t] = 0): two of the four indices coincide, or two of the three world points;
 *     the three world points are collinear (the smaller singular value of the centred triple not above 1e-4 of the larger: the number
 *     of the DLT's line test, which applies it to the scatter's eigenvalues); no admissible solution; a pose that is not finite.
 * subsets [num_tasks][4], n >= 4.  status[t]: 0 declined, 1 solved.  num_solutions (may be NULL) [num_tasks]: admissible solutions, 0..4.
 * One lane per subset, fp64, all in registers; a subset's result does not depend on where it sits in the call. */
int32_t rsba_pnp_p3p(int32_t device, const double* cam, const float* object_points, const float* image_points, int32_t n,
                     const int32_t* subsets /* [num_tasks][4] */, int32_t num_tasks, double* poses_out /* [num_tasks][6] */, uint8_t* status,
                     int32_t* num_solutions);

/* rsba_pnp_gs_hypotheses with the minimal solver in the DLT's place (solveGsPnPRansacP3P in one call): normalise, P3P, the refinement of
 * rsba_pnp_tasks with shutter GLOBAL and m = 4 from each subset's pose, inlier counts.  The start poses never leave the device.
 * status[t]: 0 declined by the minimal solver, 1 refined and usable, 2 refinement unusable (poses_out[t] = the P3P pose). */
int32_t rsba_pnp_gs_hypotheses_p3p(int32_t device, const double* cam, const float* object_points, const float* image_points, int32_t n,
                                   const int32_t* subsets /* [num_tasks][4] */, int32_t num_tasks, int32_t max_num_iterations, float reprojection_error,
                                   double* poses_out /* [num_tasks][6] */, uint8_t* status, double* final_cost, int32_t* num_inliers);

/* == the two-view bootstrap: essential-matrix hypotheses from 2-D / 2-D correspondences, for the first two frames of a video, which have no
 * poses for createTracks / PnP to start from.  The reference has no such step, so this text is the definition; include/rsba/two_view.hpp
 * (epi_detail::eight_point, decompose, score) is its host form and findEssentialRansac / initializeTwoView the callers.
 *   Inputs.  xy_a, xy_b [n][2] float: pixel coordinates of correspondence i in frame A and frame B; cam_a, cam_b the 9 sfm intrinsics of the two
 *     frames.  Both sides are undistorted and normalised once per call (hyp_detail::normalised_point): a = (xa, ya, 1), b = (xb, yb, 1).
 *     E is row-major, b^T E a = 0; camera A is the origin, camera B sees x_B = R x_A + t, E = [t]x R.
 *   Eight-point (m >= 8 indices per subset).  Hartley normalisation of each side's m points (centroid; mean distance scaled to sqrt 2); the
 *     9 x 9 Gram matrix of the rows (xb xa, xb ya, xb, yb xa, yb ya, yb, xa, ya, 1); its smallest eigenvector by cyclic Jacobi (60 sweeps at
 *     most) under the DLT's two gap tests — second-smallest eigenvalue above 1e-9 of the largest (where the largest counts the host form's
 *     idle unknowns, twice the trace), smallest below 0.05 of the second; the normalisation undone; the projection onto the essential
 *     manifold: V and the singular values s1 >= s2 from the Jacobi eigen-decomposition of E^T E, u_i = E v_i / s_i for the two largest,
 *     result u1 v1^T + u2 v2^T.  Sign: the entry of largest magnitude (the first such, row-major) is positive.
 *     Declined (status 0, E_out[t] untouched): a repeated index; a Hartley scale that is not positive (coincident points); a second null
 *     direction (coplanar scene points, a pure rotation); s2 not above 1e-6 s1; a result that is not finite.
 *   Pose recovery (of any given E).  With u3 = u1 x u2, v3 = v1 x v2: R1 = U W V^T, R2 = U W^T V^T (W the quarter turn about z), t = u3 / |u3|;
 *     candidates in the fixed order (R1, +t), (R1, -t), (R2, +t), (R2, -t).  s1 = s2 leaves the way round (v1, v2) runs in their plane to
 *     rounding, and the other way round swaps (R1, +t) with (R2, -t): the pair is taken so that the largest component of v3 is positive.  A correspondence is in front for a candidate when the
 *     least-squares depths of z_a R a + t = z_b b (2 x 2 normal equations, closed form) are both positive.
 *   Inlier rule.  Sampson distance in normalised coordinates, fp64: d^2 = (b^T E a)^2 / ((E a)_x^2 + (E a)_y^2 + (E^T b)_x^2 + (E^T b)_y^2);
 *     inlier iff d^2 f^2 <= threshold_px^2, f = (fx_a + fy_a + fx_b + fy_b) / 4.  Both deciding comparisons are evaluated with the host form's
 *     operations in the host form's order, every product and sum rounded on its own.
 *   Score.  num_inliers[t]; num_front[t][c] = the inliers in front for candidate c; the candidate with the most wins, ties go to the first;
 *     poses_out[t] = hyp_detail::pose_from_rt(R, t) of the winner — camera B in A's frame, rsba's 6-vector, unit baseline.
 *     Declined (status 0; the counts are zero, poses_out[t] untouched): s2 not above 1e-6 s1, or a pose that is not finite.
 * rsba_epipolar_eight_point: one lane per subset, fp64; a subset's result does not depend on where it sits in the call.
 * rsba_epipolar_score: scores the given matrices E [num_tasks][9], one wave per matrix; the counts are integer sums.
 * rsba_epipolar_hypotheses: the chain — normalise, eight-point, score; E never leaves the device between the two kernels.  status[t] 1: solved
 *   and scored; 0: declined by either step (zero counts, E_out[t] and poses_out[t] untouched).
 * rsba_epipolar_inliers: the inlier flags [n] of one E.
 * n >= 8, m >= 8, n >= m.  All pointers are host arrays. */
int32_t rsba_epipolar_eight_point(int32_t device, const double* cam_a, const double* cam_b, const float* xy_a, const float* xy_b, int32_t n,
                                  const int32_t* subsets /* [num_tasks][m] */, int32_t m, int32_t num_tasks, double* E_out /* [num_tasks][9] */,
                                  uint8_t* status);
int32_t rsba_epipolar_score(int32_t device, const double* cam_a, const double* cam_b, const float* xy_a, const float* xy_b, int32_t n,
                            const double* E /* [num_tasks][9] */, int32_t num_tasks, double threshold_px, int32_t* num_inliers,
                            int32_t* num_front /* [num_tasks][4] */, double* poses_out /* [num_tasks][6] */, uint8_t* status);
int32_t rsba_epipolar_hypotheses(int32_t device, const double* cam_a, const double* cam_b, const float* xy_a, const float* xy_b, int32_t n,
                                 const int32_t* subsets /* [num_tasks][m] */, int32_t m, int32_t num_tasks, double threshold_px,
                                 double* E_out /* [num_tasks][9] */, double* poses_out /* [num_tasks][6] */, uint8_t* status, int32_t* num_inliers,
                                 int32_t* num_front /* [num_tasks][4] */);
int32_t rsba_epipolar_inliers(int32_t device, const double* cam_a, const double* cam_b, const float* xy_a, const float* xy_b, int32_t n,
                              const double* E /* [9] */, double threshold_px, uint8_t* inlier_mask /* [n] */);

/* == the minimal solver of the two-view bootstrap: every essential matrix of five correspondences.  Beside the eight-point rule, not in its
 * place (TwoViewOptions::solver chooses; the default is the eight-point).  The reference has no such step, so this text is the definition;
 * epi_detail::five_point (include/rsba/two_view.hpp) is its host form.  Inputs and conventions as above: both sides undistorted and
 * normalised once per call, b^T E a = 0, E = [t]x R, row-major.
 *   Five-point (exactly five indices per subset).
 *     Null space.  The five rows (xb xa, xb ya, xb, yb xa, yb ya, yb, xa, ya, 1) as the columns of a 9 x 5 matrix, triangularised by five
 *       Householder reflections (no column exchange, no Gram matrix: the conditioning is that of the rows); the reflections applied to the
 *       unit vectors 5..8 give an orthonormal basis X, Y, Z, W of the null space.  E = x X + y Y + z Z + W.
 *     Cubics.  det E = 0 and (E E^T - 1/2 tr(E E^T) I) E = 0 expanded by polynomial arithmetic into a 10 x 20 matrix over the monomials
 *       x^3 y^3 x^2y xy^2 x^2z x^2 y^2z y^2 xyz xy | xz^2 xz x yz^2 yz y z^3 z^2 z 1, Gauss-Jordan on the first ten columns with row pivoting.
 *     Eliminant (Nister).  Rows (x^2z, x^2), (y^2z, y^2), (xyz, xy) of the result, each pair as <first> - z <second>, give B(z) (x, y, 1)^T = 0
 *       with B 3 x 3, its columns cubic, cubic and quartic in z; p(z) = det B(z) has degree 10.
 *     Roots.  Those with |z| <= 1 from p on [-1, 1], those with |z| > 1 as 1 / w from the reversed polynomial w^10 p(1 / w) on (-1, 1): no
 *       division by a leading coefficient.  On [-1, 1] the roots of each derivative bracket the roots of the polynomial above it (degree 1 up
 *       to 10); an interval whose ends differ in sign is bisected 40 times, a root of the polynomial itself then takes two Newton steps (a
 *       step is taken only while it stays in [-1, 1]).  55 intervals per pass, two passes: every loop has a fixed bound.
 *     Solutions.  Per root, (x, y) from the two rows of B(z) whose 2 x 2 minor in (x, y) is largest (the first such); then two Gauss-Newton
 *       steps in (x, y, z) on the ten cubics themselves, evaluated from X..W directly (3 x 3 normal equations by cofactors; a step that is
 *       not finite ends them) — the eliminant's coefficients went through the elimination and a determinant of polynomials, the cubics did
 *       not; E scaled to unit Frobenius norm and signed as the eight-point result (the entry of largest magnitude, the first such, positive).
 *     Order.  Ascending |sum_k (k + 1) E[k]|, k = 0..8 row-major: a fixed linear form with nine different weights, free of E's sign and of the
 *       basis X..W (which the roots z are not), and not equal for two solutions just because the motion runs along an axis; summed in the
 *       order of k, every product and sum rounded on its own.  Equal keys in the order found (the first pass ascending z, then the second ascending w).
 *     Declined (status 0, the task's outputs untouched, num_solutions 0): a repeated index; a Householder diagonal not above 1e-7 of the longest
 *       row (a null space of more than four dimensions: coincident correspondences); an elimination pivot not above 1e-7 of the largest entry
 *       of the 10 x 20 matrix (a pure rotation: the cubics then hold on a continuum); no real root; a solution that is not finite.  Coplanar
 *       scene points are NOT declined: five points of a plane have their (up to ten) essential matrices like any others.
 * rsba_epipolar_five_point: one lane per subset, fp64; a subset's bytes do not depend on where it sits in the call.  E_out[t][s] for
 *   s < num_solutions[t]; the other slots of an accepted task are untouched too.
 * rsba_epipolar_hypotheses_five_point: the chain — normalise, five-point, the score of rsba_epipolar_score for EVERY solution of every
 *   subset, then per subset the solution with the most inliers; ties go to the one with more inliers in front (of its winning candidate),
 *   then to the first in the order above.  The solutions never leave the device between the steps.  Outputs as rsba_epipolar_hypotheses, so a
 *   RANSAC loop can take either: status[t] 1 solved and scored; 0 declined, or no solution that the score accepts (zero counts, E_out[t] and
 *   poses_out[t] untouched).  num_solutions (may be NULL) as the first call's.
 * n >= 5.  All pointers are host arrays. */
int32_t rsba_epipolar_five_point(int32_t device, const double* cam_a, const double* cam_b, const float* xy_a, const float* xy_b, int32_t n,
                                 const int32_t* subsets /* [num_tasks][5] */, int32_t num_tasks, double* E_out /* [num_tasks][10][9] */,
                                 int32_t* num_solutions /* [num_tasks], 0..10 */, uint8_t* status);
int32_t rsba_epipolar_hypotheses_five_point(int32_t device, const double* cam_a, const double* cam_b, const float* xy_a, const float* xy_b, int32_t n,
                                            const int32_t* subsets /* [num_tasks][5] */, int32_t num_tasks, double threshold_px,
                                            double* E_out /* [num_tasks][9] */, double* poses_out /* [num_tasks][6] */, uint8_t* status,
                                            int32_t* num_inliers, int32_t* num_front /* [num_tasks][4] */, int32_t* num_solutions /* may be NULL */);

/* == geometric verification: the essential-matrix RANSAC of MANY frame pairs in one call — what checks a frame pair's matches against the
 * pair's epipolar geometry before they become tracks (include/rsba/two_view.hpp: findEssentialRansacPairs, verifyMatches).  The rules are
 * the ones above, unchanged; this text defines the loop around them, which is epi_detail::ransac per pair (what findEssentialRansac runs for
 * one pair with the calls above), kept on the device.
 *   Inputs.  cams [num_cams][9]; pair p has the cameras cams[pair_cam_a[p]], cams[pair_cam_b[p]] and the correspondences
 *     pair_offset[p] .. pair_offset[p + 1] of xy_a, xy_b [pair_offset[num_pairs]][2] (float pixels; pair_offset[0] = 0, not decreasing);
 *     n_p their number.  subsets [num_pairs][tasks_per_pair][m] with indices local to the pair (0 .. n_p - 1); m = 8: eight-point subsets,
 *     m = 5: five-point subsets.  Every side of every pair is undistorted and normalised once per call by the pair's own camera; the
 *     inlier rule takes the pair's own f.
 *   Per pair.  Hypotheses: rsba_epipolar_hypotheses (m = 8) or rsba_epipolar_hypotheses_five_point (m = 5) of the pair's subsets over the
 *     pair's correspondences.  Winner: the accepted task with the most inliers; for m = 5 a tie goes to the task with more inliers in front
 *     (the most over its four candidates); then the lowest task wins.  inlier_mask = rsba_epipolar_inliers of the winner's E.  Then up to
 *     `refits` rounds: the ascending indices of the current inliers; stop if they are fewer than 8; the eight-point fit over all of them
 *     as one task (m = their number) and its score over the pair; adopted iff the task is accepted and its count is not lower, else stop;
 *     an adopted refit replaces E, the pose, the counts and the mask and adds one to refits_adopted.
 *   Outputs per pair.  status 1: the pair has a winner; E_out[p], poses_out[p] (camera B in A's frame, unit baseline), winner_task[p],
 *     refits_adopted[p], num_inliers[p], num_front[p][4] (per candidate, as rsba_epipolar_score counts them) and inlier_mask over the pair's
 *     range are those of the final E.  status 0: n_p < 8, or no accepted hypothesis — zero counts, a zero mask, winner_task -1, E_out[p] and
 *     poses_out[p] untouched; the subsets of a pair with n_p < 8 are not read.  A repeated index in a subset is a declined task, not an error.
 *   Chunking.  Scratch grows with the tasks of a launch (five-point: ten slots per task), so the call works through the pairs in chunks of
 *     whole pairs of at most max_tasks_per_launch tasks (0: the library's default, 65 536); a pair with more tasks is a chunk of its own.
 *     One upload, a fixed sequence of launches per chunk with nothing read back between them, one download.  A pair's bytes depend neither
 *     on the chunking nor on which other pairs share the call: the arithmetic runs in the kernels of the single-pair calls (one compiled
 *     eight-point kernel for the subsets and the refits, one score kernel), the loop's own kernels move integers and copies, and nothing
 *     uses an atomic.
 *   A global-shutter rule.  E relates two central projections.  A pair of rolling-shutter frames has no single E (every scanline has its
 *     own pose); the rule treats it as the global-shutter pair at the frames' first pose slots, as the bootstrap above does, and the
 *     residual motion within a frame shows up as Sampson distance.  The threshold is the caller's to widen for such pairs.
 *   Errors (RSBA_ERR_INVALID_ARGUMENT, outputs untouched): a null pointer; num_cams, num_pairs or tasks_per_pair <= 0; refits or
 *     max_tasks_per_launch < 0; m not 5 or 8; pair_offset[0] != 0 or a decreasing pair_offset; a camera index out of range; a subset index
 *     outside 0 .. n_p - 1 of a pair with n_p >= 8.  All pointers are host arrays. */
int32_t rsba_epipolar_ransac_pairs(int32_t device, const double* cams /* [num_cams][9] */, int32_t num_cams, const int32_t* pair_cam_a /* [num_pairs] */,
                                   const int32_t* pair_cam_b /* [num_pairs] */, const int32_t* pair_offset /* [num_pairs + 1] */, int32_t num_pairs,
                                   const float* xy_a, const float* xy_b, const int32_t* subsets /* [num_pairs][tasks_per_pair][m] */, int32_t m,
                                   int32_t tasks_per_pair, double threshold_px, int32_t refits, int32_t max_tasks_per_launch,
                                   double* E_out /* [num_pairs][9] */, double* poses_out /* [num_pairs][6] */, uint8_t* status /* [num_pairs] */,
                                   int32_t* winner_task, int32_t* refits_adopted, int32_t* num_inliers, int32_t* num_front /* [num_pairs][4] */,
                                   uint8_t* inlier_mask /* [pair_offset[num_pairs]] */);

/* == two-view degeneracy: how well a homography explains a frame pair, and how much parallax its inliers have — the two measurements that
 * tell a pair fit to start a reconstruction from one that only turned, has a baseline of a per cent of the depth, or looks at a wall
 * (include/rsba/pair_geometry.hpp: findHomographyRansac, classifyPairs, classifyMatches, pickBootstrapPair with a geometry).  The reference
 * has no such step, so this text is the definition; homo_detail (dlt, invert, transfer_inlier, score, parallax_counts) is its host form.
 *   Inputs and conventions.  As for rsba_epipolar_*: xy_a, xy_b [n][2] float pixels, the 9 sfm intrinsics per side; both sides undistorted
 *     and normalised once per call, a = (xa, ya, 1), b = (xb, yb, 1).  H is row-major with b ~ H a.
 *   Four-point DLT (m >= 4 indices per subset; the minimal sample and the refit over all inliers alike).  Hartley normalisation of each
 *     side's m points (hyp_detail::hartley_side); the 9 x 9 Gram matrix of the 2 m rows (-a', 0, xb' a') and (0, -a', yb' a'); its smallest
 *     eigenvector by the cyclic Jacobi of the eight-point rule under the same two gap tests (hyp_detail::null_vector9: the largest eigenvalue
 *     counts the idle unknowns, twice the trace); the normalisation undone, H = Tb^-1 Hn Ta; scaled to unit Frobenius norm.  Sign: (H a)_z > 0
 *     for the subset's first index.
 *     Declined (status 0, H_out[t] untouched): a repeated index; a Hartley scale that is not positive; a second null direction (three of four
 *     points on a line, two coincident points); (H a)_z not of one sign over the subset — the orientation test; |det H| not above 1e-6 (with
 *     the Frobenius norm at 1); a result that is not finite.
 *   Inlier rule.  Transfer error in normalised coordinates, fp64, both ways: d_ab^2 = |b - pi(H a)|^2, d_ba^2 = |a - pi(H^-1 b)|^2, H^-1 the
 *     adjugate over the determinant, computed once per matrix.  Inlier iff (H a)_z > 0, (H^-1 b)_z > 0 and max(d_ab^2, d_ba^2) f^2 <=
 *     threshold_px^2, f the mean focal length of the epipolar rule.  The inverse and the deciding comparisons are evaluated with the host
 *     form's operations in the host form's order, every product and sum rounded on its own.
 *   Score.  num_inliers[t] of every given H.  Declined (status 0, a zero count): a determinant that is zero or not finite, an inverse that
 *     is not finite.
 *   Parallax rule.  Given a pair's E, its pose (camera B in A's frame, the 6-vector rsba_epipolar_score writes; R and t = -R c from it by
 *     hyp_detail::rotate) and a threshold angle: a correspondence counts as IN FRONT when it is a Sampson inlier of E (the epipolar rule, the
 *     same threshold_px) and in front for (R, t) (the epipolar rule's depths); as HAVING PARALLAX when, in addition, the angle between the rays
 *     a and R^T b is at least the threshold — decided without an inverse cosine, a . (R^T b) <= c sqrt(|a|^2 |R^T b|^2), c the cosine of the
 *     threshold, passed as a double.  Two integer counts per pair: "the median parallax reaches the angle" is 2 num_parallax > num_front.
 * rsba_homography_dlt: one lane per subset, fp64; a subset's result does not depend on where it sits in the call.
 * rsba_homography_score: scores the given matrices H [num_tasks][9], one wave per matrix; the counts are integer sums.
 * rsba_homography_hypotheses: the chain — normalise, DLT, score; H never leaves the device between the two kernels.  status[t] 1: solved and
 *   scored; 0: declined by either step (a zero count, H_out[t] untouched).
 * rsba_homography_inliers: the inlier flags [n] of one H (all zero for an H the score declines).
 * n >= 4, m >= 4, n >= m, num_tasks > 0; otherwise, and for a null pointer or a subset index outside 0 .. n - 1, RSBA_ERR_INVALID_ARGUMENT with
 * the outputs untouched.  All pointers are host arrays. */
int32_t rsba_homography_dlt(int32_t device, const double* cam_a, const double* cam_b, const float* xy_a, const float* xy_b, int32_t n,
                            const int32_t* subsets /* [num_tasks][m] */, int32_t m, int32_t num_tasks, double* H_out /* [num_tasks][9] */,
                            uint8_t* status);
int32_t rsba_homography_score(int32_t device, const double* cam_a, const double* cam_b, const float* xy_a, const float* xy_b, int32_t n,
                              const double* H /* [num_tasks][9] */, int32_t num_tasks, double threshold_px, int32_t* num_inliers, uint8_t* status);
int32_t rsba_homography_hypotheses(int32_t device, const double* cam_a, const double* cam_b, const float* xy_a, const float* xy_b, int32_t n,
                                   const int32_t* subsets /* [num_tasks][m] */, int32_t m, int32_t num_tasks, double threshold_px,
                                   double* H_out /* [num_tasks][9] */, uint8_t* status, int32_t* num_inliers);
int32_t rsba_homography_inliers(int32_t device, const double* cam_a, const double* cam_b, const float* xy_a, const float* xy_b, int32_t n,
                                const double* H /* [9] */, double threshold_px, uint8_t* inlier_mask /* [n] */);

/* The homography RANSAC and the parallax counts of MANY frame pairs in one call (classifyPairs).  Inputs as rsba_epipolar_ransac_pairs: cams,
 * pair_cam_a / pair_cam_b, pair_offset, xy_a / xy_b; subsets [num_pairs][tasks_per_pair][4] with indices local to the pair.  E [num_pairs][9],
 * poses [num_pairs][6] and pair_status [num_pairs] are the pairs' essential results (rsba_epipolar_ransac_pairs' E_out, poses_out, or the
 * caller's verdict in pair_status); where pair_status[p] is 0, E[p] and poses[p] are not used.
 *   Per pair.  Hypotheses: rsba_homography_hypotheses of the pair's subsets over the pair's correspondences.  Winner: the accepted task with
 *     the most inliers, then the lowest task.  h_inlier_mask = rsba_homography_inliers of the winner's H.  Then up to `refits` rounds: the
 *     ascending indices of the current inliers; stop if they are fewer than 5; the DLT over all of them as one task (m = their number) and
 *     its score over the pair; adopted iff the task is accepted and its count is not lower, else stop; an adopted refit replaces H, the
 *     count and the mask and adds one to h_refits_adopted.  For a pair with pair_status[p] != 0 the parallax rule with E[p], poses[p] gives
 *     num_front[p], num_parallax[p]; else both are 0.
 *   Outputs per pair.  h_status 1: the pair has a winner; H_out[p], h_winner_task[p], h_refits_adopted[p], num_h_inliers[p] and h_inlier_mask
 *     over the pair's range are those of the final H.  h_status 0: n_p < 4, or no accepted hypothesis — a zero count, a zero mask,
 *     h_winner_task -1, H_out[p] untouched; the subsets of a pair with n_p < 4 are not read.
 *   Chunking.  Whole pairs of at most max_tasks_per_launch tasks per launch (0: 65 536); a pair with more tasks is a chunk of its own.  One
 *     upload, a fixed sequence of launches per chunk with nothing read back between them, the parallax kernel once over all pairs, one
 *     download.  A pair's bytes depend neither on the chunking nor on which other pairs share the call: the arithmetic runs in the kernels of
 *     the single-pair calls (one compiled DLT kernel for the subsets and the refits, one score kernel), the loop's own kernels move integers
 *     and copies, and nothing uses an atomic.
 *   Errors (RSBA_ERR_INVALID_ARGUMENT, outputs untouched): a null pointer; num_cams, num_pairs or tasks_per_pair <= 0; refits or
 *     max_tasks_per_launch < 0; cos_min_parallax outside [-1, 1]; pair_offset[0] != 0 or a decreasing pair_offset; a camera index out of
 *     range; a subset index outside 0 .. n_p - 1 of a pair with n_p >= 4.  All pointers are host arrays. */
int32_t rsba_two_view_classify_pairs(int32_t device, const double* cams /* [num_cams][9] */, int32_t num_cams, const int32_t* pair_cam_a /* [num_pairs] */,
                                     const int32_t* pair_cam_b /* [num_pairs] */, const int32_t* pair_offset /* [num_pairs + 1] */, int32_t num_pairs,
                                     const float* xy_a, const float* xy_b, const double* E /* [num_pairs][9] */, const double* poses /* [num_pairs][6] */,
                                     const uint8_t* pair_status /* [num_pairs] */, const int32_t* subsets /* [num_pairs][tasks_per_pair][4] */,
                                     int32_t tasks_per_pair, double threshold_px, int32_t refits, double cos_min_parallax, int32_t max_tasks_per_launch,
                                     double* H_out /* [num_pairs][9] */, uint8_t* h_status /* [num_pairs] */, int32_t* h_winner_task, int32_t* h_refits_adopted,
                                     int32_t* num_h_inliers, uint8_t* h_inlier_mask /* [pair_offset[num_pairs]] */, int32_t* num_front /* [num_pairs] */,
                                     int32_t* num_parallax /* [num_pairs] */);

/* ---- multi-GPU: one process per GPU, observations partitioned BY POINT, cameras replicated ----
 * (the reference is single-process; this is the exchange step SURVEY §8e derives for the path).
 * Every rank creates a handle over its own observations (all frames / points arrays are full size, a rank
 * simply holds no observations of the points it does not own).  Per LM iteration the solver all-reduces
 *   (1) the per-camera gradient blocks g_c and diag(U)  + cost / failure scalars (+ a slot per rank: its gradient maximum)  [2*F*CD + 3 (+ world) doubles]
 *   (2) the packed non-zero tiles of its partial reduced camera system S and its rhs  [tile pairs*48*48 + F*CD] — or, when the points are cut along
 *       the top separators of the elimination tree (rsba_partition_points) and every rank factors its own part, (2') the separators' tiles only,
 *       between the two launches of the factorisation, and (4) the camera step, each rank its rows  [npad]
 *   (3) twelve step scalars (model decrease, |step|^2, |x|^2, gradient maximum, trial cost, failure flags, the factorisation's verification flag)
 * through RCCL directly (rsba_set_exchange_rccl, below) or through the callback below, for hosts that bring their own
 * transport (the tests stage it through gloo).
 * op: 0 = sum, 1 = max.  The buffer is device memory; the collective must be ordered after prior work
 * on `hip_stream` and complete (or be stream-ordered) before the callback returns.  Return 0 on success. */
typedef int32_t (*rsba_allreduce_fn)(void* ctx, double* device_buffer, int64_t count, int32_t op, void* hip_stream);
int32_t rsba_set_exchange(rsba_handle* h, rsba_allreduce_fn fn, void* ctx, int32_t rank, int32_t world);

/* Structure of the reduced camera system: mask[a*F + b] != 0 (a >= b) iff frames a and b share a point in
 * THIS rank's observations.  All ranks must install the same (union) structure before the first solve so
 * that their tile layouts — and therefore exchange buffer (2) — coincide; frame_obs_count [F] likewise
 * carries the per-frame observation count (summed over ranks before it is set back). */
int32_t rsba_get_block_structure(rsba_handle* h, uint8_t* mask, int64_t* frame_obs_count);
int32_t rsba_set_block_structure(rsba_handle* h, const uint8_t* mask, const int64_t* frame_obs_count);
/* The two calls above in one, over the installed exchange: every rank calls it after rsba_set_exchange[_rccl] and before
 * the first solve; the co-visibility masks are OR-ed and the per-frame counts summed through the all-reduce itself, and
 * the partition is checked (RSBA_ERR_INVALID_ARGUMENT when some point has observations on more than one rank). */
int32_t rsba_sync_block_structure(rsba_handle* h);

/* What the exchange of a sharded solve carried (a first multi-rank run should be diagnosable from its numbers alone): per kind of
 * collective the calls and fp64 elements since the handle was created, and — after an rsba_solve with options.profile_phases — the
 * HIP-event time of those of that solve, measured on the solver's stream around each collective. */
enum {
  RSBA_EXCHANGE_SETUP = 0,      /* co-visibility structure, problem-size counts, the form of the plan (once per handle / solve) */
  RSBA_EXCHANGE_CAMERA = 1,     /* (1) per-camera gradient blocks g_c | diag(U) | cost scalars | every rank's max |g_i| over its points, once per linearisation */
  RSBA_EXCHANGE_SYSTEM = 2,     /* (2) the reduced camera system: every structurally non-zero tile | rhs (replicated factorisation) or the
                                 *     separators' tiles | their rhs rows between the two launches of a sharded factorisation */
  RSBA_EXCHANGE_SCALARS = 3,    /* (3) step scalars and the verification flag: one sum of 12 doubles per iteration (the gradient max-norm rides in (1);
                                 *     with per-pose priors it still takes a MAX all-reduce of its own) */
  RSBA_EXCHANGE_STEP = 4,       /* (4) the gather of the camera step (sharded factorisation only) */
  RSBA_EXCHANGE_POINTS = 5,     /* the merge of the solved points at the end of a solve */
  RSBA_NUM_EXCHANGES = 6
};
typedef struct rsba_exchange_stats {
  int64_t calls[RSBA_NUM_EXCHANGES], doubles[RSBA_NUM_EXCHANGES];
  double ms[RSBA_NUM_EXCHANGES];
  int32_t rank, world;
} rsba_exchange_stats;
int32_t rsba_get_exchange_stats(rsba_handle* h, rsba_exchange_stats* out);
const char* rsba_exchange_name(int32_t kind);
/* == ncclGetVersion / ncclCommCount / ncclCommUserRank of a communicator, as the library's own RCCL sees it (-1 where the symbol is missing) */
int32_t rsba_rccl_describe(void* nccl_comm, int32_t* version, int32_t* nranks, int32_t* rank);

/* Which rank should own which point: owner [num_points] (host array), computed on the host from the WHOLE problem's description
 * (no device needed; every rank of a job computes the same answer from the same description).  Any by-point partition gives a
 * correct sharded solve; THIS one places the cut along the top separators of the nested dissection that orders the reduced camera
 * system's 48 x 48 tile columns: every rank's points then touch the tiles of its own subtree (and the separators) only, the columns
 * of its subtree are complete on that rank, and the solver factors them there — exchange (2) shrinks from every non-zero tile of S
 * to the separators' tiles, the factorisation's work is shared out (rsba_plan_stats.sharded_factorisation says whether the plan
 * took that form).  world == 1: all zero.  num_top_tiles (may be NULL): tile columns in the separators the ranks share.
 * RSBA_ERR_UNSUPPORTED when the co-visibility graph cannot be cut into `world` parts (a handful of frames, or not connected). */
int32_t rsba_partition_points(const rsba_problem_desc* desc, int32_t world, int32_t* owner, int32_t* num_top_tiles);

/* Native transport: RCCL's ncclAllReduce over xGMI, issued by the solver on its own HIP stream — nothing of the host
 * language runs inside an LM iteration.  librccl is resolved at run time (RSBA_RCCL_LIB, else an RCCL already loaded in
 * the process, else librccl.so.1); single-GPU users never load it.
 *   rsba_rccl_get_unique_id   one rank (usually 0) fills id[RSBA_RCCL_UNIQUE_ID_BYTES] (== ncclGetUniqueId); the host
 *                             hands the bytes to the other ranks by whatever means it has (MPI, a file, torch.distributed)
 *   rsba_rccl_comm_create     == ncclCommInitRank on `device`; collective over all ranks; *comm_out is an ncclComm_t
 *   rsba_set_exchange_rccl    installs the all-reduce over an ncclComm_t (one made above or the caller's own) on the
 *                             handle; must precede the first solve / gradient call, like rsba_set_exchange
 *   rsba_rccl_comm_destroy    == ncclCommDestroy (after the handles that use it)
 * After a sharded rsba_solve every rank holds the complete solved parameter arrays: the points are merged over the ranks
 * (each from the rank that owns its observations) before they are written back. */
#define RSBA_RCCL_UNIQUE_ID_BYTES 128
int32_t rsba_rccl_get_unique_id(void* id);
int32_t rsba_rccl_comm_create(const void* id, int32_t rank, int32_t world, int32_t device, void** comm_out);
void rsba_rccl_comm_destroy(void* comm);
int32_t rsba_set_exchange_rccl(rsba_handle* h, void* nccl_comm, int32_t rank, int32_t world);

#ifdef __cplusplus
}
#endif
#endif /* RSBA_AMD_H_ */
