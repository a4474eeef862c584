/*
 * uvs_solver.h -- C ABI of the MI355X-native sliding-window back-end.
 *
 * This header is the drop-in boundary for ONE path of url-kaist/UV-SLAM: the
 * nonlinear least-squares solve inside Estimator::optimization()
 * (reference vins_estimator/src/estimator.cpp:761-1233).  In the reference
 * that function builds a ceres::Problem and calls ceres::Solve; a maintainer
 * replaces that body by "fill a uvs_window, call uvs_solve_window()" -- see
 * INTEGRATION.md for the exact stub.
 *
 * Conventions (all taken from the reference, file:line cited per field):
 *   - every scalar is IEEE double (the reference path is FP64 end to end);
 *   - pose block = (px,py,pz, qx,qy,qz,qw)              estimator.cpp:530-537
 *   - speed/bias block = (v[3], ba[3], bg[3])            estimator.cpp:539-549
 *   - residual row order of an IMU block = (P,R,V,BA,BG) parameters.h:59-66
 *   - parameter blocks are addressed by INDEX (frame id, landmark id), not by
 *     pointer as in Ceres (SURVEY.md section 8b "Parameter memory").
 *
 * Plain pointers and sizes only; no C++ / torch types cross this boundary.
 * All pointers are HOST pointers unless a function says otherwise.
 */
#ifndef UVS_SOLVER_H
#define UVS_SOLVER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UVS_ABI_VERSION 7

#define UVS_WINDOW_SIZE 10                    /* parameters.h:12 WINDOW_SIZE  */
#define UVS_NUM_FRAMES (UVS_WINDOW_SIZE + 1)  /* frames 0..WINDOW_SIZE        */
#define UVS_SIZE_POSE 7                       /* parameters.h:51 SIZE_POSE    */
#define UVS_SIZE_SPEEDBIAS 9                  /* parameters.h:52              */
#define UVS_SIZE_LINE 4                       /* parameters.h:54              */
#define UVS_MAX_ITER 64                       /* capacity of the per-iteration trace */
#define UVS_MAX_PRIOR_BLOCKS 16               /* 10 poses + speedbias + ex + td (+slack) */
#define UVS_MAX_PRIOR_DIM 96                  /* n <= 76 in the reference (a9) */

/* ---- status codes (the reference has no error path: estimator.cpp:993-997
 *      discards ceres::Solver::Summary; we return one and never abort) ---- */
enum {
    UVS_OK = 0,
    UVS_ERR_INVALID_ARG = 1,    /* null pointer / index out of range / bad count */
    UVS_ERR_UNSUPPORTED = 2,    /* a combination this path does not take: relocalization blocks in a landmark-sharded solve over SEVERAL ranks;
                                 * RCCL not found for a multi-rank communicator */
    UVS_ERR_NO_DEVICE = 3,      /* no HIP device / extension cannot run (never falls back to CPU) */
    UVS_ERR_HIP = 4,            /* a HIP runtime call failed; see uvs_last_error() */
    UVS_ERR_CAPACITY = 5,       /* window larger than the handle was created for */
    UVS_ERR_NUMERIC = 6         /* non-finite cost / Cholesky breakdown reported by the device */
};

/* ---- termination reasons, named after Ceres ---- */
enum {
    UVS_TERM_NO_CONVERGENCE = 0,       /* max_num_iterations reached           */
    UVS_TERM_GRADIENT_TOL = 1,
    UVS_TERM_PARAMETER_TOL = 2,
    UVS_TERM_FUNCTION_TOL = 3,
    UVS_TERM_MIN_RADIUS = 4,
    UVS_TERM_INVALID_STEPS = 5,        /* max_num_consecutive_invalid_steps    */
    UVS_TERM_NUMERIC_FAILURE = 6,
    UVS_TERM_MAX_TIME = 7              /* max_solver_time_in_seconds reached (Ceres: NO_CONVERGENCE, "Maximum solver time reached") */
};

/* Solver options == the globals Estimator::optimization() reads
 * (parameters.h:11-47, estimator.cpp:982-991) plus the Ceres defaults it
 * relies on.  uvs_default_options() fills the EuRoC
 * values of config/euroc/euroc_config.yaml. */
typedef struct uvs_options {
    int32_t max_num_iterations;        /* NUM_ITERATIONS, euroc_config.yaml:56 (10)        */
    int32_t estimate_extrinsic;        /* ESTIMATE_EXTRINSIC (0): Ex_Pose constant; != 0: free 6-dof block (estimator.cpp:784-788) */
    int32_t estimate_td;               /* ESTIMATE_TD (0); 1: ProjectionTdFactor + para_Td (estimator.cpp:790-797,853-858) */
    int32_t function_tol_keeps_candidate; /* 0 = Ceres order: tolerance checks before accept (App. B.4) */
    double focal_length;               /* FOCAL_LENGTH = fx, parameters.cpp:60 (461.6)     */
    double point_sqrt_info;            /* FOCAL_LENGTH/1.6, estimator.cpp:17               */
    double line_factor;                /* LINE_FACTOR (300)  euroc_config.yaml:86          */
    double vp_factor;                  /* VP_FACTOR (10)     euroc_config.yaml:87          */
    double loss_point;                 /* CauchyLoss(1.0)  estimator.cpp:765               */
    double loss_line;                  /* CauchyLoss(0.1)  estimator.cpp:768               */
    double loss_vp;                    /* CauchyLoss(1.0)  estimator.cpp:772               */
    double gravity[3];                 /* G = (0,0,g_norm) parameters.cpp:12,79            */
    /* Ceres trust-region defaults (not set by the reference => defaults apply) */
    double initial_trust_region_radius;   /* 1e4  */
    double max_trust_region_radius;       /* 1e16 */
    double min_trust_region_radius;       /* 1e-32 */
    double min_relative_decrease;         /* 1e-3 */
    double min_lm_diagonal;               /* 1e-6 */
    double max_lm_diagonal;               /* 1e32 */
    double function_tolerance;            /* 1e-6 */
    double gradient_tolerance;            /* 1e-10 */
    double parameter_tolerance;           /* 1e-8 */
    int32_t max_consecutive_invalid_steps;/* 5 */
    int32_t jacobi_scaling;               /* 1 */
    double max_solver_time_in_seconds;    /* options.max_solver_time_in_seconds = SOLVER_TIME or 0.8 SOLVER_TIME (estimator.cpp:987-991); checked at the top of
                                           * every LM iteration with the GPU's 100 MHz wall clock.  0 (default) = no cap: the iteration count is then
                                           * deterministic, which the parity runs need */
} uvs_options;

/* One IMU pre-integration block == the fields of IntegrationBase that
 * IMUFactor::Evaluate reads (integration_base.h:188-203, imu_factor.h:19-182).
 * Links frame i = index, frame j = index+1 (estimator.cpp:811-818).
 * jacobian / covariance are 15x15 ROW-major here (Eigen's are column-major;
 * the host shim transposes on copy). */
typedef struct uvs_imu_block {
    double sum_dt;
    double delta_p[3];
    double delta_q[4];                 /* (x,y,z,w) */
    double delta_v[3];
    double linearized_ba[3];
    double linearized_bg[3];
    double jacobian[15 * 15];
    double covariance[15 * 15];
    int32_t frame_i;                   /* j = frame_i + 1 */
    int32_t skip;                      /* 1 when sum_dt > 10.0 (estimator.cpp:814) */
} uvs_imu_block;

/* Marginalization prior == what MarginalizationFactor::Evaluate reads from
 * MarginalizationInfo (marginalization_factor.cpp:333-381, .h:64-69).
 * n rows; kept block b has global size block_size[b] (7,9,1), column offset
 * block_idx[b] (already minus m), linearization point x0 at x0[x0_off[b]..].
 * linearized_jacobians is n x n ROW-major. */
enum { UVS_BLOCK_POSE = 0, UVS_BLOCK_SPEEDBIAS = 1, UVS_BLOCK_EX_POSE = 2, UVS_BLOCK_TD = 3 };
#define UVS_PRIOR_X0_LEN (UVS_MAX_PRIOR_BLOCKS * 9)
typedef struct uvs_prior {
    int32_t n;                         /* 0 => no prior (last_marginalization_info == nullptr) */
    int32_t n_blocks;
    int32_t block_kind[UVS_MAX_PRIOR_BLOCKS];   /* UVS_BLOCK_*                                */
    int32_t block_frame[UVS_MAX_PRIOR_BLOCKS];  /* frame index for POSE / SPEEDBIAS, else 0   */
    int32_t block_size[UVS_MAX_PRIOR_BLOCKS];   /* keep_block_size (global size 7/9/1)        */
    int32_t block_idx[UVS_MAX_PRIOR_BLOCKS];    /* keep_block_idx - m (local column offset)   */
    int32_t x0_off[UVS_MAX_PRIOR_BLOCKS];       /* offset of keep_block_data in x0[]          */
    double x0[UVS_PRIOR_X0_LEN];
    double linearized_residuals[UVS_MAX_PRIOR_DIM];
    double linearized_jacobians[UVS_MAX_PRIOR_DIM * UVS_MAX_PRIOR_DIM];  /* row-major, leading dim n */
} uvs_prior;

/* The sliding window handed to the solver: exactly what optimization() feeds
 * Ceres after vector2double() (estimator.cpp:800), flattened to SoA.
 *
 * Point residual blocks (estimator.cpp:823-866): one entry per
 * ProjectionFactor(pts_i, pts_j) with blocks Pose[fi], Pose[fj], Ex_Pose,
 * Feature[lm].  Entries of one landmark must be contiguous and lm must be
 * non-decreasing (this is the order the reference loop emits them in).
 *
 * Line residual blocks (estimator.cpp:868-927): one entry per
 * LineProjectionFactor(ric,tic,sp,ep) with blocks Pose[fj], Ortho[lm]; when
 * has_vp != 0 the same entry also carries VPProjectionFactor(...,vp)
 * (estimator.cpp:920-925, added iff vp(2)==1).  Same contiguity rule. */
typedef struct uvs_window {
    /* frame states: para_Pose / para_SpeedBias / para_Ex_Pose (estimator.h:114-121) */
    double pose[UVS_NUM_FRAMES][UVS_SIZE_POSE];
    double speedbias[UVS_NUM_FRAMES][UVS_SIZE_SPEEDBIAS];
    double ex_pose[UVS_SIZE_POSE];
    double td;                         /* para_Td (unused unless estimate_td) */

    /* point landmarks: para_Feature[l][0] = inverse depth (feature_manager.cpp:290-306) */
    int32_t n_points;
    int32_t n_point_obs;
    const double *inv_depth;           /* [n_points]            */
    const int32_t *pt_lm;              /* [n_point_obs] feature_index            */
    const int32_t *pt_fi;              /* [n_point_obs] imu_i (anchor frame)     */
    const int32_t *pt_fj;              /* [n_point_obs] imu_j                    */
    const double *pt_pi;               /* [n_point_obs][3] pts_i                 */
    const double *pt_pj;               /* [n_point_obs][3] pts_j                 */

    /* line landmarks: para_Ortho_plucker[l] = (psi_x,psi_y,psi_z,phi) (feature_manager.cpp:308-331) */
    int32_t n_lines;
    int32_t n_line_obs;
    const double *line_orth;           /* [n_lines][4]          */
    const int32_t *ln_lm;              /* [n_line_obs] line_feature_index        */
    const int32_t *ln_fj;              /* [n_line_obs] imu_j                     */
    const double *ln_sp;               /* [n_line_obs][3] start_point            */
    const double *ln_ep;               /* [n_line_obs][3] end_point              */
    const int32_t *ln_has_vp;          /* [n_line_obs] 1 iff vp(2)==1            */
    const double *ln_vp;               /* [n_line_obs][3] vp                     */

    /* IMU factors (estimator.cpp:811-818): up to WINDOW_SIZE blocks */
    int32_t n_imu;
    const uvs_imu_block *imu;          /* [n_imu] */

    /* marginalization prior (estimator.cpp:803-809); may be NULL / n==0 */
    const uvs_prior *prior;

    /* ProjectionTdFactor inputs (projection_td_factor.cpp:3-16,51-52), read only when options.estimate_td != 0, else may be NULL:
     * image-plane feature velocities of the anchor / current observation and their time offsets.  The rolling-shutter term is
     * folded in by the caller: pt_td_i = cur_td_i - TR / ROW * (row_i - ROW / 2), so that
     *   pts_i_td = pts_i - (td - pt_td_i) * (vel_i, 0)          (same for j). */
    const double *pt_vel_i;            /* [n_point_obs][2] */
    const double *pt_vel_j;            /* [n_point_obs][2] */
    const double *pt_td_i;             /* [n_point_obs]    */
    const double *pt_td_j;             /* [n_point_obs]    */

    /* Relocalization residual blocks (estimator.cpp:944-978), n_relo_obs == 0 when relocalization_info == 0.  One entry per matched
     * feature: ProjectionFactor(pts_i, pts_j) on the blocks Pose[start_frame], relo_Pose, Ex_Pose, Feature[lm] with pts_i = the
     * feature's FIRST observation (feature_per_frame[0].point) and pts_j = (match_point.x, match_point.y, 1).  relo_Pose is a free
     * 7-dof block with PoseLocalParameterization (estimator.cpp:947-948); it starts at para_Pose[relo_frame_local_index]
     * (Estimator::setReloFrame, estimator.cpp:1361-1379).  relo_lm must be strictly increasing and every such landmark needs at least
     * one ordinary observation (its anchor frame imu_i is taken from there).  With estimate_td the blocks stay plain ProjectionFactors (no
     * dependence on td, estimator.cpp:967-970).  With estimate_extrinsic the 6 + 6 (+ 1) free dofs beside the frames no longer fit the spare rows of
     * the reduced system: relo_Pose is then eliminated at a second level (same exact solve of the damped system) -- by uvs_solve_window, the batch
     * entry points and, on one rank, the uvs_large_* forms. */
    int32_t n_relo_obs;
    double relo_pose[UVS_SIZE_POSE];
    const int32_t *relo_lm;            /* [n_relo_obs] feature_index */
    const double *relo_pi;             /* [n_relo_obs][3] pts_i      */
    const double *relo_pj;             /* [n_relo_obs][3] pts_j      */
} uvs_window;

/* Solver output == the para_* arrays after ceres::Solve and BEFORE
 * double2vector() (estimator.cpp:999); caller allocates inv_depth[n_points]
 * and line_orth[n_lines*4]. */
typedef struct uvs_state {
    double pose[UVS_NUM_FRAMES][UVS_SIZE_POSE];
    double speedbias[UVS_NUM_FRAMES][UVS_SIZE_SPEEDBIAS];
    double ex_pose[UVS_SIZE_POSE];
    double td;
    double *inv_depth;                 /* [n_points]   */
    double *line_orth;                 /* [n_lines][4] */
    double relo_pose[UVS_SIZE_POSE];   /* relo_Pose after the solve (estimator.cpp:671-685 reads it); the input value when n_relo_obs == 0 */
} uvs_state;

/* Replaces ceres::Solver::Summary (discarded by the reference) with the trace
 * needed for parity diffing. Entry 0 of the arrays is
 * the initial evaluation; entry k>=1 is LM iteration k. */
typedef struct uvs_report {
    int32_t status;                    /* UVS_OK / UVS_ERR_NUMERIC */
    int32_t termination;               /* UVS_TERM_* */
    int32_t num_iterations;            /* LM iterations executed (successful or not) */
    int32_t num_successful;
    double initial_cost;
    double final_cost;
    double cost[UVS_MAX_ITER + 1];             /* cost of x after iteration k             */
    double candidate_cost[UVS_MAX_ITER + 1];
    double model_cost_change[UVS_MAX_ITER + 1];
    double relative_decrease[UVS_MAX_ITER + 1];
    double radius[UVS_MAX_ITER + 1];           /* trust region radius after iteration k   */
    double step_norm[UVS_MAX_ITER + 1];
    double gradient_max_norm[UVS_MAX_ITER + 1];
    int32_t accepted[UVS_MAX_ITER + 1];        /* 1 accepted, 0 rejected, -1 invalid step */
} uvs_report;

/* Per-residual-block evaluation dump (uvs_evaluate): what
 * cost_function->Evaluate + the Ceres corrector would hand the linear solver,
 * in LOCAL (tangent) column size.  Used by the parity tests to compare the
 * hand-derived HIP Jacobians element-wise with the oracle's Jets.
 *   point block : r[2], J = [d/dPose_i (2x6) | d/dPose_j (2x6) | d/dEx (2x6) | d/dlambda (2x1)]  -> 2x19 row-major
 *   line block  : r[2], J = [d/dPose_j (2x6) | d/dline (2x4)]                                  -> 2x10
 *   vp block    : r[1], J = [d/dPose_j (1x6) | d/dline (1x4)]                                  -> 1x10 (zeros when !has_vp)
 *   imu block   : r[15], J = [Pose_i (15x6) | SB_i (15x9) | Pose_j (15x6) | SB_j (15x9)]         -> 15x30
 *   prior       : r[n]  (J is the constant linearized_jacobians)
 * robust!=0 applies the Cauchy corrector (a10); cost = sum over blocks of 0.5*rho(s). */
typedef struct uvs_eval {
    double *pt_r;      /* [n_point_obs][2]   */
    double *pt_J;      /* [n_point_obs][2*19]*/
    double *ln_r;      /* [n_line_obs][2]    */
    double *ln_J;      /* [n_line_obs][2*10] */
    double *vp_r;      /* [n_line_obs][1]    */
    double *vp_J;      /* [n_line_obs][10]   */
    double *imu_r;     /* [n_imu][15]        */
    double *imu_J;     /* [n_imu][15*30]     */
    double *prior_r;   /* [prior n]          */
    double cost;       /* out */
    double *pt_Jtd;    /* [n_point_obs][2] d r / d td of ProjectionTdFactor (only with estimate_td; may be NULL) */
} uvs_eval;

typedef struct uvs_solver uvs_solver;  /* opaque: device buffers, stream, workspaces */

/* ---- lifecycle ---- */
int uvs_abi_version(void);
void uvs_default_options(uvs_options *opts);
/* device = HIP device ordinal. max_* size the per-window workspaces
 * (reference capacities NUM_OF_F = NUM_OF_LF = 1000, parameters.h:14-16).
 * Fails with UVS_ERR_NO_DEVICE when no GPU is present: there is no CPU path. */
int uvs_create(const uvs_options *opts, int device, int max_batch, int max_points, int max_point_obs,
               int max_lines, int max_line_obs, uvs_solver **out);
void uvs_destroy(uvs_solver *s);
const char *uvs_last_error(const uvs_solver *s);
const char *uvs_status_string(int status);

/* ---- the hot path: replaces problem build + ceres::Solve (estimator.cpp:763-997) ---- */
int uvs_solve_window(uvs_solver *s, const uvs_window *w, uvs_state *out, uvs_report *rep);

/* Batch of independent windows (BASELINE configs[2]). upload: host->HBM once;
 * solve: device-resident, re-runnable (reads the uploaded initial state, writes
 * separate outputs); elapsed_ms (may be NULL) = HIP-event time of the solve
 * kernels on the solver's stream; download: HBM->host. */
int uvs_batch_upload(uvs_solver *s, int n, const uvs_window *const *ws);
int uvs_batch_solve(uvs_solver *s, float *elapsed_ms);
int uvs_batch_download(uvs_solver *s, int n, uvs_state *states, uvs_report *reps);
/* A stream of n_batches batches of per_batch windows each (ws[k * per_batch + b] = window b of batch k), END TO END: host packing, upload, solve
 * and download of consecutive batches overlap on three buffer sets (no reference equivalent: offline replay of recorded windows, estimator.cpp:992
 * once per window).  states / reps: n_batches * per_batch entries (either may be NULL); wall_ms: wall time of the whole call.  Results are those
 * of uvs_batch_upload / uvs_batch_solve / uvs_batch_download batch by batch.  On an error in batch k (e.g. a malformed window) the batches before k have been
 * delivered, batch k and the later ones have not been touched, and the code of the first error is returned.  The call leaves NO resident batch behind:
 * uvs_batch_solve / uvs_batch_download after it need their own uvs_batch_upload. */
int uvs_batch_stream(uvs_solver *s, int n_batches, int per_batch, const uvs_window *const *ws, uvs_state *states, uvs_report *reps, double *wall_ms);

/* One evaluation of every residual block at the window's state (no solve).  Relocalization blocks (n_relo_obs) are solve-only: they are
 * neither evaluated here nor marginalized below (the reference's marginalization does not add them, estimator.cpp:1002-1228), and the
 * per-observation outputs keep the caller's numbering. */
int uvs_evaluate(uvs_solver *s, const uvs_window *w, int robust, uvs_eval *out);

/* Diagnostic (parity tests only): reduced system of the FIRST LM iteration of `w`:
 * S_lower[176*176] row-major = damped, landmark-Schur-reduced frame system in the padded index space
 * (16*frame + dof, dof 15 = dummy pivot), g/hd/dd/step[176], scal[UVS_DEBUG_SCAL_LEN] = {cost, gmax, chol_ok, model_cost_change,
 * step_norm^2, line chunks whose pass A ran under the previous gather walk, full linearizations (both counted over the whole solve), -, per-phase shader cycles[16], sub-timers[8], -...}: the caller's buffer must hold UVS_DEBUG_SCAL_LEN doubles. */
#define UVS_DEBUG_SCAL_LEN 40
int uvs_debug_first_iteration(uvs_solver *s, const uvs_window *w, double *S_lower, double *g, double *hd, double *dd,
                              double *step, double *scal);

/* Diagnostic (step tests only): the damped LM step of the FIRST linearization of `w`, solved at radii[0] with the first iteration's Jacobi scaling
 * and clamped Marquardt diagonal, then at radii[1], radii[2], ... each the way the selected kernels handle a rejected step.  form 0 = the persistent
 * k_solve of the handle's instantiation (UVS_KSOLVE_NT), which re-damps its stored linearization.  form 1 = the landmark-sharded kernels
 * (k_large_chunks -> k_large_reduce -> k_large_solve -> k_large_backsub of the handle's instantiations, UVS_LARGE_CHUNKS_NT / UVS_LARGE_SOLVE_NT) through the
 * step-wise calls below, which re-linearize at the same state with the new radius (uvs_large_decide keeps no linearization to re-damp); the landmark part
 * and the frame part (relo_Pose included) are what k_large_backsub itself holds, the scalars are formed by the code uvs_large_decide uses.  Per radius k:
 * step[k * n_step ...] = the FULL unscaled tangent step as the kernels hold it (not recovered from the candidate state):
 *   11 x 15 frame entries (dp, dtheta, dv, dba, dbg), 6 extrinsic entries if estimate_extrinsic, 1 td entry if estimate_td, 6 relo_Pose entries
 *   if n_relo_obs > 0, n_points inverse depths, 4 n_lines line parameters -- n_step must be exactly that length;
 * scal[k * UVS_DEBUG_SCAL_LEN ...] = {cost, gmax, chol_ok, model_cost_change, step_norm^2, 0...} as for uvs_debug_first_iteration.
 * UVS_ERR_INVALID_ARG: null pointer, n_radii < 1, an unknown form, a radius that is not finite or <= 0, or n_step not matching the layout.
 * UVS_ERR_UNSUPPORTED (form 1): relocalization blocks while uvs_large_set_nranks announced more than one rank, as uvs_large_begin.
 * Ordinary solves do not run this code: it is a separate instantiation of the kernel (k_solve_dstep, k_large_backsub_dstep). */
int uvs_debug_step(uvs_solver *s, const uvs_window *w, int form, int n_radii, const double *radii, int n_step, double *step, double *scal);

/* Diagnostic, host only (no device is touched): packs `w` the way uvs_batch_upload() does and reports the layout:
 * info[12] = {blob bytes, workspace doubles, landmark chunks, packed point observations (incl. relocalization blocks), relocalization
 * blocks, doubles per point record, extra Schur slots per point landmark, LDS doubles of the fullest chunk, LDS staging capacity,
 * largest split of a pose block, compact prior-image entries, pose blocks the prior touches}.  Same status codes as the upload. */
int uvs_debug_pack_layout(const uvs_options *opts, const uvs_window *w, int32_t *info);

/* ---- marginalization (estimator.cpp:1002-1228, marginalization_factor.cpp) ----
 * flag 0 = MARGIN_OLD, 1 = MARGIN_SECOND_NEW. `w` carries the POST-solve state
 * (the reference calls vector2double() again at :1004). Output prior is already
 * re-indexed for the next window (addr_shift, estimator.cpp:1139-1153). */
int uvs_marginalize(uvs_solver *s, const uvs_window *w, int flag, uvs_prior *out);
/* Same, for the usual sequence "solve window w, then marginalize it" (Estimator::optimization()): the caller promises that the
 * residual blocks of `w` are the ones of the LAST upload of this handle (uvs_solve_window / uvs_batch_upload with n = 1) and that
 * only the state fields (pose, speedbias, ex_pose, td, inv_depth, line_orth) changed; the resident factors are reused and only the
 * state is sent to the device.  Returns UVS_ERR_INVALID_ARG when the block counts do not match the resident window. */
int uvs_marginalize_resident(uvs_solver *s, const uvs_window *w, int flag, uvs_prior *out);
/* The same call in two halves (round 4): uvs_marginalize_resident_begin() hands the whole marginalization -- sub-window packing, the device linearization, the
 * elimination of the departing frame and the n x n factorization -- to a worker thread of the handle and returns at once; uvs_marginalize_wait() blocks until the
 * prior is there and returns what uvs_marginalize_resident() would have returned.  The prior is first needed by the NEXT uvs_solve_window(), so the caller's own
 * work between two frames (window slide, IMU integration, feature bookkeeping: estimator.cpp:123-222) runs beside it.  Contract: between begin and wait the handle
 * must not be used for anything else, and `w` as well as every array it points to (incl. w->prior) must stay valid and unchanged.  uvs_destroy() waits by itself. */
int uvs_marginalize_resident_begin(uvs_solver *s, const uvs_window *w, int flag);
int uvs_marginalize_wait(uvs_solver *s, uvs_prior *out);
/* The marginalization of a BATCH of independent windows (ABI v7, round 6): out[b] = what uvs_marginalize(s, ws[b], flags[b], &out[b]) returns, for b = 0 .. n - 1, with the
 * cubic work of all windows in two launches -- the sub-windows of the MARGIN_OLD windows (flag 0) are linearized by one launch (assembly A = sum J^T J, b = sum J^T r and elimination
 * of the dropped landmark blocks, marginalization_factor.cpp:232-276), then ONE launch eliminates every window's dropped frame block, forms the Schur complement and factors it
 * (J0 = sqrt(S) V^T, r0 = sqrt(S^-1) V^T b with the eps = 1e-8 cut, :278-291; a parallel cyclic Jacobi per window, csrc/uvs_marg_kernel.h).  MARGIN_SECOND_NEW windows (flag 1)
 * read their old prior only and join the second launch.  Host work per window (sub-window packing, the block tables) runs on the handle's packing threads.  status (may be NULL)
 * receives the per-window code; the return value is the first one that is not UVS_OK.  A window the device path does not take (a landmark or frame block the reference's eps cut
 * would touch, N = dropped + kept frame dofs > 96) is sent through uvs_marginalize() -- which, like every one-window call, may replace the handle's resident batch.  Synchronous; not
 * to be called while a uvs_marginalize_resident_begin() is in flight.  What a batched closed-loop replay calls between two uvs_batch_solve(). */
int uvs_marginalize_batch(uvs_solver *s, int n, const uvs_window *const *ws, const int *flags, uvs_prior *out, int *status);

/* ---- ONE large window spread over the GPU and, with an all-reduce between the steps, over several GPUs (BASELINE configs[3]) ----
 * Landmarks shard (rank r holds the landmarks k with k % G == r; frames / IMU / prior are replicated); the only exchanged data are
 * the pose-block partials returned by uvs_large_reduced() (SUM, except entry [n-7] which is a MAX) and the n = 6 scalars of
 * uvs_large_scalars() (SUM; the sixth is this rank's vote that options.max_solver_time_in_seconds is used up: reduced with the rest, so that
 * every rank ends the solve at the same iteration).  Both are DEVICE pointers so that RCCL can reduce them in place.  On one GPU skip the all-reduces
 * or call uvs_large_solve().  Loop: begin; while (!done) { if (need_linearize) { linearize; allreduce(reduced) } step; allreduce(scalars); decide } finish.
 * Relocalization blocks (n_relo_obs > 0) are taken on ONE rank only: a landmark shard cannot tell from its own observations whether relo_Pose is a
 * free block of the window, so in a solve over several ranks no rank may pass them (uvs_large_solve_fused answers UVS_ERR_UNSUPPORTED).
 * uvs_large_set_nranks(s, n) tells the step-wise form over how many ranks the caller all-reduces (default 1; UVS_ERR_INVALID_ARG for n < 1); with n > 1,
 * uvs_large_begin answers UVS_ERR_UNSUPPORTED for a shard with n_relo_obs > 0, as the fused form does.  A rank whose shard holds none of them is not
 * refused by its own call: the caller must spread the refusal to every rank before the first collective (api.py: Solver.large_solve).
 * uvs_large_solve (one process) ignores the count and leaves it set. */
int uvs_large_set_nranks(uvs_solver *s, int nranks);
int uvs_large_begin(uvs_solver *s, const uvs_window *w);
int uvs_large_need_linearize(const uvs_solver *s);
int uvs_large_linearize(uvs_solver *s);
double *uvs_large_reduced(uvs_solver *s, int *n);
int uvs_large_exchange_host(uvs_solver *s, int which, double *buf, int set);   /* host-staged get/set of the two vectors (no GPU-aware transport) */
int uvs_large_step(uvs_solver *s);
double *uvs_large_scalars(uvs_solver *s, int *n);
int uvs_large_decide(uvs_solver *s);
int uvs_large_done(const uvs_solver *s);
double uvs_large_local_x2(const uvs_solver *s);
void uvs_large_set_landmark_x2(uvs_solver *s, double all_ranks_x2);
int uvs_large_finish(uvs_solver *s, uvs_state *out, uvs_report *rep);
int uvs_large_solve(uvs_solver *s, const uvs_window *w, uvs_state *out, uvs_report *rep);

/* Diagnostic (step tests only): the step of a SHARD of the step-wise form, so that a test can drive several handles in one process and sum their
 * exchange vectors on the host.  uvs_large_set_debug_step(s, 1) makes every later uvs_large_step of the handle (uvs_debug_step form 1 does the same for
 * its own duration) run the storing instantiation of k_large_backsub; ordinary calls (flag 0, the default) run the product kernel and pay nothing.
 * uvs_large_debug_step(), called after uvs_large_step and after the caller has summed uvs_large_scalars() over the ranks, returns step[n_step] = the
 * unscaled tangent step of THIS shard's window in the layout of uvs_debug_step (frames, extrinsic, td, relo_Pose, the shard's own inverse depths and
 * lines in the shard's numbering) and scal[UVS_DEBUG_SCAL_LEN] = {cost, gmax, chol_ok, model_cost_change, step_norm^2, landmark chunks, chunk
 * workgroups of k_large_chunks (= partial rows of k_large_reduce), chunk workgroups of k_large_backsub, 0...} from the exchanged scalars and the
 * launches of this step (uvs_debug_step form 1 returns the same three figures).  next_radius > 0 then handles the step as a REJECTED one at that radius (re-linearization at the same state: need_linearize becomes 1) in
 * place of uvs_large_decide; next_radius == 0 leaves the run state alone.  UVS_ERR_INVALID_ARG: no step-wise solve in progress, the flag not set
 * before the last uvs_large_step (a step stored by an earlier solve is never handed out), n_step not matching the layout, a next radius that is
 * negative or not finite.
 * UVS_DEBUG_LARGE_GRID=<n> in the environment of uvs_create (step tests only; unset in production) caps the chunk workgroups of the handle's
 * large-window kernels at n (never above compute units - 1), so that a window of a thousand landmarks walks the persistent loops that only a
 * configs[3] window reaches on the full grid: the packing asks for a multiple of n chunks, k_large_chunks runs n workgroups, k_large_backsub 2 n.
 * It is the device-side twin of UVS_DEBUG_CHUNK_GRID, which sets the same grid for the host-only uvs_debug_pack_layout. */
int uvs_large_set_debug_step(uvs_solver *s, int on);
int uvs_large_debug_step(uvs_solver *s, double next_radius, int n_step, double *step, double *scal);

/* ---- fused multi-GPU loop: the library owns the RCCL communicator (SURVEY.md 8b "library owns ... RCCL comm") and keeps the
 * trust-region control on the device, so that one solve is one stream of launches with two in-place all-reduces per iteration and no
 * host round trip.  Usage on every rank (one process per GPU, one handle per process):
 *     rank 0: uvs_large_comm_unique_id(&id); broadcast `id` (128 bytes) to the other ranks by any host transport;
 *     uvs_large_comm_init(s, nranks, rank, &id);            (nranks <= 8; nranks == 1 needs no id and no RCCL)
 *     uvs_large_solve_fused(s, shard_of_this_rank, &state, &report, &ms);    w = the landmarks k with k % nranks == rank, frames / IMU /
 *                                                                            prior replicated; frames of `state` identical on all ranks
 *     uvs_large_comm_destroy(s);                             (also done by uvs_destroy)
 * RCCL is looked up at run time (a copy already loaded by the process is reused; UVS_RCCL_LIB overrides): UVS_ERR_UNSUPPORTED if absent.
 *
 * WITHOUT a communicator (no uvs_large_comm_init, or nranks == 1) uvs_large_solve_fused() is also the LOW-LATENCY form for ONE window of
 * any size on an otherwise idle GPU (the online case): the landmark chunks of every LM iteration run on many compute units, the frame
 * terms in a workgroup beside them, the reduced solve in one workgroup; one upload, one stream of launches, one download, one wait.
 * On MI355X a canonical 10-keyframe window takes 1.2 ms per call this way against 1.7 ms through uvs_solve_window() (which keeps the
 * whole solve on one compute unit and is what a BATCH of windows uses per window).  Same LM controller, same results to rounding
 * (tests/test_fused_single.py); relocalization blocks are taken on one rank (tests/test_relo.py). */
typedef struct uvs_rccl_id { char internal[128]; } uvs_rccl_id;      /* == ncclUniqueId */
int uvs_large_comm_unique_id(uvs_rccl_id *id);
int uvs_large_comm_init(uvs_solver *s, int nranks, int rank, const uvs_rccl_id *id);
void uvs_large_comm_destroy(uvs_solver *s);
int uvs_large_solve_fused(uvs_solver *s, const uvs_window *w, uvs_state *out, uvs_report *rep, float *loop_ms);

/* ---- size helpers for callers that serialise windows ---- */
int uvs_reduced_dim(const uvs_options *opts);  /* 165 (+6 if estimate_extrinsic) */

/* ---- 4-DoF pose graph of loop closure (reference pose_graph/src/pose_graph.cpp:403-579, PoseGraph::optimize4DoF) ----
 * The caller passes the keyframes of the solve in list order -- first_looped_index .. cur_index of the reference -- as local indices 0 .. n-1.
 * Each keyframe is (yaw in DEGREES, t); yaw, pitch and roll are Utility::R2ypr of q.  Pitch and roll are never variables.  Keyframe i is
 * constant when constant[i] != 0 (the reference: index == first_looped_index or sequence == 0).  The library builds the sequential edges
 * itself, exactly as the reference does: FourDOFError (i-j, i) for j = 1..4 when both have the same sequence, measured from the initial poses
 * (rel_t = R(q_{i-j})^T (t_i - t_{i-j}), rel_yaw = yaw_i - yaw_{i-j}, pitch / roll of i-j), no loss.  Loop edge l is
 * FourDOFWeightError (old, cur) with HuberLoss(0.1), yaw residual / 10, pitch / roll of the initial pose of `old`.  Solver: Ceres LM with
 * max_num_iterations = 5 and otherwise the defaults of uvs_default_options(), a direct solve of the damped normal
 * equations (banded Cholesky + Woodbury, one step of iterative refinement when loop edges have two free ends).  Edges whose two keyframes are both constant are not part of the problem (Ceres drops them from its reduced program): the costs
 * reported here are those of the other edges.  No CPU path: uvs_pg_create fails with UVS_ERR_NO_DEVICE without a GPU. */
#define UVS_PG_MAX_KEYFRAMES 65536            /* largest max_keyframes uvs_pg_create takes */
#define UVS_PG_MAX_LOOPS 256                  /* largest max_loops uvs_pg_create takes      */
typedef struct uvs_pose_graph uvs_pose_graph;  /* opaque: device buffers, stream */

typedef struct uvs_pg_loop {
    int32_t cur;                       /* local index of the keyframe that has the loop  (pose_graph.cpp:516-530) */
    int32_t old;                       /* local index of its loop_index keyframe, 0 <= old < cur */
    double rel_t[3];                   /* loop_info(0..2): t of cur in the frame of old    */
    double rel_yaw;                    /* loop_info(7), degrees                            */
} uvs_pg_loop;

typedef struct uvs_pg_problem {
    int32_t n;                         /* keyframes, >= 1 */
    int32_t n_loops;                   /* loop edges, >= 0 */
    const double *t;                   /* [n][3] initial (VIO) translation */
    const double *q;                   /* [n][4] initial (VIO) rotation, (x, y, z, w) */
    const int32_t *sequence;           /* [n] */
    const int32_t *constant;           /* [n] != 0: yaw and t held fixed */
    const uvs_pg_loop *loops;          /* [n_loops] */
} uvs_pg_problem;

/* Entry 0 of the arrays is the initial evaluation, entry k >= 1 LM iteration k (as in uvs_report). */
typedef struct uvs_pg_report {
    int32_t status;                    /* UVS_OK / UVS_ERR_NUMERIC */
    int32_t termination;               /* UVS_TERM_* */
    int32_t num_iterations;
    int32_t num_successful;
    int32_t n_free;                    /* keyframes that are variables */
    int32_t n_edges;                   /* sequential + loop edges in the problem */
    int32_t n_loop_columns;            /* 4 x loop edges with two free ends (the low-rank part of the normal equations) */
    int32_t reserved;
    double initial_cost;
    double final_cost;
    double cost[UVS_MAX_ITER + 1];
    double candidate_cost[UVS_MAX_ITER + 1];
    double model_cost_change[UVS_MAX_ITER + 1];
    double radius[UVS_MAX_ITER + 1];
    int32_t accepted[UVS_MAX_ITER + 1];        /* 1 accepted, 0 rejected, -1 invalid step */
} uvs_pg_report;

int uvs_pg_create(int device, int max_keyframes, int max_loops, uvs_pose_graph **out);
void uvs_pg_destroy(uvs_pose_graph *pg);
const char *uvs_pg_last_error(const uvs_pose_graph *pg);
/* out_yaw_t[n][4] = (yaw in degrees, tx, ty, tz) after the solve, every keyframe (constant ones unchanged).  UVS_ERR_INVALID_ARG: null pointer,
 * n < 1, or a loop outside 0 <= old < cur < n; UVS_ERR_CAPACITY: n or n_loops above the handle's capacity. */
int uvs_pg_optimize(uvs_pose_graph *pg, const uvs_pg_problem *problem, double *out_yaw_t, uvs_pg_report *report);

/* Diagnostic (tests only): ONE damped solve of the first LM iteration of uvs_pg_optimize, through the same kernels.  Linearizes at the
 * initial poses, computes the Jacobi scaling as the first linearization does and solves the damped system at `radius`:
 * delta[4 * n_free] = the unscaled step in free-keyframe order (yaw deg, t), scal[UVS_PG_DEBUG_SCAL_LEN] = {banded Cholesky fail flag,
 * capacitance Cholesky fail flag, n_loop_columns, n_free}.  UVS_ERR_INVALID_ARG also for a radius that is not finite or <= 0. */
#define UVS_PG_DEBUG_SCAL_LEN 4
int uvs_pg_debug_step(uvs_pose_graph *pg, const uvs_pg_problem *problem, double radius, double *delta, double *scal);

/* ---- loop verification of loop closure (reference pose_graph/src/keyframe.cpp:259-521, KeyFrame::findConnection) ----
 * Verifies a batch of candidate pairs (current keyframe, old keyframe as place recognition proposed it) in one call; a pair gives the same
 * bits alone or in a batch.  Per pair: each window point of the current keyframe is matched to the old keypoint of smallest Hamming distance
 * over its 256-bit BRIEF descriptor (ties: the first index; kept when the distance is < 80); with > 25 matches, a PnP-RANSAC (100 hypotheses
 * of 5 points, each an LM from the VIO prior, inlier threshold 10 / 460 in normalized coordinates, OpenCV's adaptive iteration rule) and an
 * LM refinement on the chosen hypothesis's inliers give the old keyframe's body pose; with > 25 inliers, loop_info as the reference builds it,
 * accepted when |relative yaw| < 30 deg and |relative t| < 20 m.  The numerics (sample generator, LM, selection) are spelled out in
 * csrc/uvs_loop_verify.hip and restated in tests/lc_ref.py; DESIGN.md 3.7 lists where they deviate from OpenCV.
 * No CPU path: uvs_lc_create fails with UVS_ERR_NO_DEVICE without a GPU. */
#define UVS_LC_MAX_PAIRS 4096                 /* largest max_pairs uvs_lc_create takes            */
#define UVS_LC_MAX_QUERY 1024                 /* largest max_query (window points of a keyframe)  */
#define UVS_LC_MAX_OLD 4096                   /* largest max_old (keypoints of an old keyframe)   */
#define UVS_LC_N_HYPOTHESES 100               /* solvePnPRansac iterationsCount (keyframe.cpp:232) */
typedef struct uvs_loop_verifier uvs_loop_verifier;  /* opaque: device buffers, pinned staging, stream */

enum {
    UVS_LC_ACCEPTED = 0,
    UVS_LC_NO_MATCHES = 1,         /* no window point matched (also n_query = 0 or n_old = 0) */
    UVS_LC_FEW_MATCHES = 2,        /* matches <= MIN_LOOP_NUM (25) */
    UVS_LC_RANSAC_FAILED = 3,      /* no hypothesis with >= 5 inliers */
    UVS_LC_FEW_INLIERS = 4,        /* inliers <= 25 */
    UVS_LC_YAW_GATE = 5,           /* |relative yaw| >= 30 deg */
    UVS_LC_T_GATE = 6              /* |relative t| >= 20 m */
};

typedef struct uvs_lc_pair {
    int32_t n_query;                   /* window points of the current keyframe, 0 .. max_query */
    int32_t n_old;                     /* keypoints of the old keyframe, 0 .. max_old */
    const double *p3d;                 /* [n_query][3] point_3d, in the current keyframe's VIO world frame */
    const uint64_t *desc;              /* [n_query][4] window_brief_descriptors */
    double vio_t[3];                   /* origin_vio_T of the current keyframe */
    double vio_q[4];                   /* origin_vio_R as a unit quaternion (x, y, z, w) */
    const double *old_uv_norm;         /* [n_old][2] keypoints_norm of the old keyframe */
    const uint64_t *old_desc;          /* [n_old][4] brief_descriptors of the old keyframe */
    uint64_t seed;                     /* keys the RANSAC sample generator */
} uvs_lc_pair;

typedef struct uvs_lc_result {
    int32_t accepted;                  /* 1: the loop passes every gate */
    int32_t reason;                    /* UVS_LC_* */
    int32_t n_matches;
    int32_t n_inliers;                 /* inliers of the chosen hypothesis (0 before RANSAC) */
    int32_t best_hypothesis;           /* -1: none */
    int32_t ransac_iters;              /* hypotheses the sequential adaptive rule examined */
    double loop_info[8];               /* relative t (3), relative q (w, x, y, z), relative yaw (deg): keyframe.cpp:485 order */
    double PnP_T_old[3];               /* body pose of the old keyframe from PnP */
    double PnP_q_old[4];               /* (x, y, z, w) */
    int32_t hyp_inliers[UVS_LC_N_HYPOTHESES];   /* inlier count of every hypothesis, -1 invalid (all -1 when RANSAC did not run) */
} uvs_lc_result;

int uvs_lc_create(int device, int max_pairs, int max_query, int max_old, uvs_loop_verifier **out);
void uvs_lc_destroy(uvs_loop_verifier *lc);
const char *uvs_lc_last_error(const uvs_loop_verifier *lc);
/* tic[3], qic_xyzw[4]: the camera-IMU extrinsic.  match_old[] and inlier[] hold one entry per window point, concatenated over the pairs in
 * order: the matched old keypoint index or -1, and 1 for a match that is an inlier of the chosen hypothesis.  results[n_pairs].
 * UVS_ERR_INVALID_ARG: null pointer, n_pairs < 1, a negative count, a null array behind a positive count, or qic / a vio_q that is not a
 * unit quaternion (|norm - 1| > 1e-6); UVS_ERR_CAPACITY: n_pairs, n_query or n_old above the handle's capacity.  A pair with n_query = 0
 * or n_old = 0 is rejected (UVS_LC_NO_MATCHES), not an error. */
int uvs_lc_verify(uvs_loop_verifier *lc, int n_pairs, const uvs_lc_pair *pairs, const double tic[3], const double qic_xyzw[4],
                  int32_t *match_old, uint8_t *inlier, uvs_lc_result *results);

/* Diagnostic (tests only): ONE pair through a second instantiation of the same kernel body, which also writes every intermediate value of
 * the PnP-RANSAC into trace[UVS_LC_TRACE_LEN] (doubles; integers and flags as 0.0 / 1.0 / counts; zeroed before the run, so what the kernel
 * did not reach stays 0).  match_old[n_query], inlier[n_query] and *result are bit for bit what uvs_lc_verify gives for the pair.
 *   record r = 0 .. 99 (hypothesis r) and r = 100 (the refinement) at trace + r * UVS_LC_TRACE_REC_LEN:
 *     [0..4] sample match indices (-1 where the draw failed; hypotheses only)   [5] valid (refinement: 1 once it ran)
 *     [6] iteration records written   [7] initial cost   [8..19] final R (row-major), t   [20] draw succeeded (hypotheses);
 *     [20..31] start R, t (refinement: the chosen hypothesis's final pose)
 *     iteration i at + UVS_LC_TRACE_HEAD_LEN + i * UVS_LC_TRACE_ITER_LEN:
 *       [0..11] start R, t   [12] lambda   [13..40] packed upper J^T J (21), J^T r (6), cost (the block sum in the refinement)
 *       [41] Cholesky succeeded   [42..47] delta   [48..59] candidate R, t   [60] candidate cost   [61] current cost   [62] accepted
 *       [63] stop (|delta| below the threshold).  After a failed Cholesky [42..63] stay 0.
 *   at trace + UVS_LC_TRACE_STAGE_OFF: [0] n matches, then X[UVS_LC_MAX_QUERY][3], uv[UVS_LC_MAX_QUERY][2] and the query index
 *     [UVS_LC_MAX_QUERY] of match m as the kernel staged them (the first n rows of each). */
#define UVS_LC_TRACE_HEAD_LEN 32
#define UVS_LC_TRACE_ITER_LEN 64
#define UVS_LC_TRACE_REC_LEN (UVS_LC_TRACE_HEAD_LEN + 20 * UVS_LC_TRACE_ITER_LEN)
#define UVS_LC_TRACE_STAGE_OFF ((UVS_LC_N_HYPOTHESES + 1) * UVS_LC_TRACE_REC_LEN)
#define UVS_LC_TRACE_LEN (UVS_LC_TRACE_STAGE_OFF + 1 + 6 * UVS_LC_MAX_QUERY)
int uvs_lc_debug_pair(uvs_loop_verifier *lc, const uvs_lc_pair *pair, const double tic[3], const double qic_xyzw[4],
                      int32_t *match_old, uint8_t *inlier, uvs_lc_result *result, double *trace);

/* ---- vanishing points of the line front end (reference feature_tracker/src/line_feature_tracker.cpp:1977-2299) ----
 * Estimates, for a batch of frames in one call, the three orthogonal vanishing points of each frame's line segments and tags every line with
 * the one it runs towards; a frame gives the same bits alone or in a batch, and from run to run.  Per frame: 105 line pairs (a counter-based
 * generator keyed by `seed`) x 360 rotations give 37 800 orthogonal-triple hypotheses; every line pair whose orientations differ by <= 60 deg
 * votes sqrt(len_i len_j) (sin(2 dev) + 0.2) into the cell of its intersection on a 90 x 360 one-degree latitude / longitude grid; the grid is
 * smoothed by its 3 x 3 window; the hypothesis whose three cells sum highest wins (the lowest index of the maximum); a line whose direction is
 * within th_angle of the direction to a vanishing point gets that point's tag.  The numerics (generator, cell rule, the order-independent sum)
 * are spelled out in csrc/uvs_vanishing_points.hip and restated in tests/vp_ref.py; DESIGN.md 3.8 lists the one place where they deviate from
 * the reference.  No CPU path: uvs_vp_create fails with UVS_ERR_NO_DEVICE without a GPU. */
#define UVS_VP_MAX_FRAMES 1024                /* largest max_frames uvs_vp_create takes */
#define UVS_VP_MAX_LINES 1024                 /* largest max_lines (segments of one frame) */
#define UVS_VP_MAX_COORD 1e7                  /* largest |coordinate| of a segment, pixels */
#define UVS_VP_N_SAMPLES 105                  /* int(log(1 - 0.9999) / log(1 - (1/3) * 0.5^2)), line_feature_tracker.cpp:1981-1985 */
#define UVS_VP_N_ROTATIONS 360
#define UVS_VP_N_HYPOTHESES 37800             /* UVS_VP_N_SAMPLES x UVS_VP_N_ROTATIONS */
#define UVS_VP_GRID_LA 90
#define UVS_VP_GRID_LO 360
typedef struct uvs_vp_estimator uvs_vp_estimator;  /* opaque: device buffers, pinned staging, stream */

enum {
    UVS_VP_OK = 0,
    UVS_VP_TOO_FEW_LINES = 1,      /* n_lines < 2: the reference skips the frame (line_feature_tracker.cpp:86) */
    UVS_VP_NO_HYPOTHESIS = 2       /* a sample found no pair of distinct, non-parallel lines in its bounded number of attempts */
};

typedef struct uvs_vp_frame {
    int32_t n_lines;                   /* 0 .. max_lines */
    int32_t reserved;
    const double *segments;            /* [n_lines][4] x1, y1, x2, y2 in pixels of the undistorted image */
    uint64_t seed;                     /* keys the sample generator */
} uvs_vp_frame;

typedef struct uvs_vp_camera {
    double fx, fy, cx, cy;
} uvs_vp_camera;

typedef struct uvs_vp_result {
    int32_t status;                    /* UVS_VP_* */
    int32_t best_hypothesis;           /* 360 * sample + rotation; -1 when status != UVS_VP_OK */
    double score;                      /* smoothed-grid sum of its three cells */
    double vps[3][3];                  /* unit vectors with z >= 0: tmp_vps of the reference (zero when status != UVS_VP_OK) */
    int32_t n_tagged[3];               /* lines per tag */
    int32_t reserved;
} uvs_vp_result;

int uvs_vp_create(int device, int max_frames, int max_lines, uvs_vp_estimator **out);
void uvs_vp_destroy(uvs_vp_estimator *vp);
const char *uvs_vp_last_error(const uvs_vp_estimator *vp);
/* th_angle: the tag threshold in radians (the reference: 1 degree).  tag[] (0..2, or 3 for "none") and line_vp[][3] (vps[tag] / vps[tag].z, or
 * zero for tag 3) hold one entry per line, concatenated over the frames in order; results[n_frames].  A frame whose status is not UVS_VP_OK
 * has every tag 3.  UVS_ERR_INVALID_ARG: null pointer, n_frames < 1, a negative count, a null array behind a positive count, a coordinate that
 * is not finite or beyond UVS_VP_MAX_COORD, a zero-length segment, fx / fy / th_angle not positive; UVS_ERR_CAPACITY: n_frames or n_lines
 * above the handle's capacity.  The handle stays usable after a rejected call. */
int uvs_vp_estimate(uvs_vp_estimator *vp, int n_frames, const uvs_vp_frame *frames, const uvs_vp_camera *camera, double th_angle,
                    int32_t *tag, double *line_vp, uvs_vp_result *results);
/* HIP-event time of the last successful uvs_vp_estimate: upload, the five kernels, download, on the handle's stream (milliseconds). */
double uvs_vp_last_device_ms(const uvs_vp_estimator *vp);
/* Diagnostic (tests only): ONE frame through the same kernels, with the intermediate results: hyp[37800][3][3], cells[37800][3] (latitude * 360
 * + longitude of each vanishing point), scores[37800], grid_raw / grid_smooth[90 * 360], pair_cell[n (n - 1) / 2] (pairs i < j row by row: the
 * cell the pair voted into, -1 when it did not vote).  All zero when the frame's status is not UVS_VP_OK. */
int uvs_vp_debug_frame(uvs_vp_estimator *vp, const uvs_vp_frame *frame, const uvs_vp_camera *camera, double th_angle, double *hyp,
                       int32_t *cells, double *scores, double *grid_raw, double *grid_smooth, int32_t *pair_cell, uvs_vp_result *result);

/* ---- keyframe features of loop closure (reference pose_graph/src/keyframe.cpp:14-41, 75-113; ThirdParty/DVision/BRIEF.cpp:39-106) ----
 * Extracts, for a batch of 8-bit grey images in one call, what a keyframe of the pose graph carries into uvs_lc_verify: FAST 9-16 corners
 * (threshold 20, non-maximum suppression) of the unblurred image in row-major order with their normalized coordinates (PinholeCamera::
 * liftProjective, FP64), their 256-bit BRIEF descriptors, and the BRIEF descriptors of the frame's window points (sub-pixel (u, v)); BRIEF
 * reads a 9 x 9 blur of the image.  A frame gives the same bits alone or in a batch, from run to run and on any machine: everything is integer
 * arithmetic except the float32 add of BRIEF's coordinates and the FP64 of liftProjective, which is IEEE multiplies and adds in a fixed order.
 *   blur     separable, taps {7, 17, 32, 46, 52, 46, 32, 17, 7} / 256 (exp(-k^2 / 8) normalized to 256 and rounded: sigma 2), border
 *            reflect-101, rows then columns without rounding in between, out = (sum + 32768) >> 16
 *   FAST     ring clockwise from the top: (0,-3) (1,-3) (2,-2) (3,-1) (3,0) (3,1) (2,2) (1,3) (0,3) (-1,3) (-2,2) (-3,1) (-3,0) (-3,-1) (-2,-2)
 *            (-1,-3); pixels with 3 <= x < W - 3, 3 <= y < H - 3; d_i = ring_i - centre, A = max over the 16 arcs of 9 contiguous ring pixels
 *            of min(d_i), B the same of -d_i; a corner iff max(A, B) > 20, score max(A, B) - 1 (OpenCV's cornerScore<16>), 0 otherwise; kept
 *            iff its score is strictly greater than the scores of its 8 neighbours
 *   BRIEF    test i: xa = (int)(float(u) + float(x1[i])) (float32 add, truncation toward zero; -0.5 becomes 0), ya, xb, yb alike; bit i is
 *            set iff the four are inside the image and blur[ya][xa] < blur[yb][xb]; bit i is bit (i & 63) of word (i >> 6), the layout of
 *            uvs_lc_pair.desc / old_desc
 *   lift     m = (u / fx - cx / fx, v / fy - cy / fy) through 1 / fx, -cx / fx, 1 / fy, -cy / fy; when a distortion coefficient is not zero,
 *            the recursive model with 8 evaluations of distortion() (PinholeCamera.cc:450-510, 678-694)
 * The numerics are restated in tests/kf_ref.py; DESIGN.md 3.9 lists the two deviations from the reference (the integer blur in place of
 * cv::GaussianBlur, the keypoint cap).  The library embeds no BRIEF pattern: the caller reads it (the reference's brief_pattern.yml) and
 * gives it to uvs_kf_create.  No CPU path: uvs_kf_create fails with UVS_ERR_NO_DEVICE without a GPU. */
#define UVS_KF_MAX_FRAMES 64                  /* largest max_frames uvs_kf_create takes */
#define UVS_KF_MIN_SIZE 9                     /* smallest width and height of an image (one reflection covers the blur's border) */
#define UVS_KF_MAX_WIDTH 4096                 /* largest max_width */
#define UVS_KF_MAX_HEIGHT 4096                /* largest max_height */
#define UVS_KF_PATTERN_BITS 256               /* tests of the BRIEF pattern = bits of a descriptor */
#define UVS_KF_MAX_PATTERN_OFFSET 1024        /* largest |x1|, |y1|, |x2|, |y2| of the pattern */
#define UVS_KF_MAX_COORD 1e6                  /* largest |u|, |v| of a window point, pixels */
typedef struct uvs_kf_extractor uvs_kf_extractor;  /* opaque: device buffers, pinned staging, stream */

enum {
    UVS_KF_OK = 0,
    UVS_KF_OVERFLOW = 1            /* more corners survive than max_keypoints: the first max_keypoints in row-major order are returned */
};

typedef struct uvs_kf_frame {
    const uint8_t *image;              /* [height][width] grey levels, row-major, stride = width */
    int32_t width;                     /* UVS_KF_MIN_SIZE .. max_width */
    int32_t height;                    /* UVS_KF_MIN_SIZE .. max_height */
    int32_t n_window;                  /* window points, 0 .. max_window */
    int32_t reserved;
    const float *window_uv;            /* [n_window][2] point_2d_uv, pixels */
} uvs_kf_frame;

typedef struct uvs_kf_camera {
    double fx, fy, cx, cy;             /* pinhole */
    double k1, k2, p1, p2;             /* radial-tangential distortion; all zero: none */
} uvs_kf_camera;

typedef struct uvs_kf_result {
    int32_t status;                    /* UVS_KF_OK / UVS_KF_OVERFLOW */
    int32_t n_keypoints;               /* corners that survive the suppression (the true count, also on overflow) */
    int32_t n_returned;                /* min(n_keypoints, max_keypoints) */
    int32_t n_corners_before_nms;      /* pixels with max(A, B) > 20 */
} uvs_kf_result;

/* x1, y1, x2, y2: the BRIEF pattern, UVS_KF_PATTERN_BITS offsets each.  max_keypoints <= UVS_LC_MAX_OLD and max_window <= UVS_LC_MAX_QUERY,
 * so that what uvs_kf_extract returns always fits uvs_lc_verify.  UVS_ERR_INVALID_ARG: null pointer, a capacity < 1, max_width or max_height
 * below UVS_KF_MIN_SIZE, a pattern offset beyond UVS_KF_MAX_PATTERN_OFFSET; UVS_ERR_CAPACITY: a capacity above its bound. */
int uvs_kf_create(int device, int max_frames, int max_width, int max_height, int max_keypoints, int max_window,
                  const int32_t *x1, const int32_t *y1, const int32_t *x2, const int32_t *y2, uvs_kf_extractor **out);
void uvs_kf_destroy(uvs_kf_extractor *kf);
const char *uvs_kf_last_error(const uvs_kf_extractor *kf);
/* Layout of the outputs.  The keypoint arrays are STRIDED: frame f owns entries f * max_keypoints .. f * max_keypoints + n_returned - 1 of
 * keypoints_xy[][2] (x, y), keypoint_score[], keypoints_norm[][2] and desc[][4]; entries past n_returned are not written.  window_desc[][4] is
 * PACKED: one entry per window point, concatenated over the frames in order (as match_old of uvs_lc_verify is).  results[n_frames].
 * The arrays of frame f go unchanged into uvs_lc_pair: window_desc -> desc (as the current keyframe), keypoints_norm -> old_uv_norm and
 * desc -> old_desc with n_old = n_returned (as an old keyframe).
 * UVS_ERR_INVALID_ARG: null pointer, n_frames < 1, a negative count, a null array behind a positive count, a width or height below
 * UVS_KF_MIN_SIZE, a window point that is not finite or beyond UVS_KF_MAX_COORD, a camera that is not finite or whose fx or fy is not positive;
 * UVS_ERR_CAPACITY: n_frames, a width, a height or n_window above the handle's capacity.  More corners than max_keypoints is not an error
 * (UVS_KF_OVERFLOW in the frame's result).  The handle stays usable after a rejected call. */
int uvs_kf_extract(uvs_kf_extractor *kf, int n_frames, const uvs_kf_frame *frames, const uvs_kf_camera *camera, int32_t *keypoints_xy,
                   uint8_t *keypoint_score, double *keypoints_norm, uint64_t *desc, uint64_t *window_desc, uvs_kf_result *results);
/* HIP-event time of the last successful uvs_kf_extract: upload, the kernels, download, on the handle's stream (milliseconds). */
double uvs_kf_last_device_ms(const uvs_kf_extractor *kf);
/* Diagnostic (tests only): ONE frame through the same kernels, with the whole blurred image blur[height][width] and the whole score map
 * score[height][width] (0 where the pixel is no corner or is not examined) next to the outputs of uvs_kf_extract for that frame
 * (keypoint arrays of max_keypoints entries, window_desc of n_window). */
int uvs_kf_debug_frame(uvs_kf_extractor *kf, const uvs_kf_frame *frame, const uvs_kf_camera *camera, uint8_t *blur, uint8_t *score,
                       int32_t *keypoints_xy, uint8_t *keypoint_score, double *keypoints_norm, uint64_t *desc, uint64_t *window_desc,
                       uvs_kf_result *result);

/* ---- point tracking of the point front end (reference feature_tracker/src/feature_tracker.cpp:54-147: cv::calcOpticalFlowPyrLK(cur_img,
 * forw_img, cur_pts, forw_pts, status, err, cv::Size(21, 21), 3) at :86, inBorder at :93-95 / utility.cpp:3-9, liftProjective of
 * undistortedPoints at :240-288) ----
 * A handle is a tracker with max_streams slots.  Each slot keeps the image pyramid of the last image it was given resident on the device (two
 * buffers per slot, swapped: an image is uploaded and reduced once).  One call takes a batch of items, at most one per slot: it builds the new
 * image's pyramid, tracks the item's points from the slot's stored pyramid into it with pyramidal Lucas-Kanade (21 x 21 window, at most 30
 * iterations per level), and makes the new pyramid the slot's stored one.  A slot that holds nothing (fresh, or after uvs_ft_reset) only stores
 * the pyramid.  An item gives the same bits alone or in a batch, from run to run and on any machine: every sum over the window is an integer
 * sum (exact in any order), and the FP64 operations of an iteration are the few below, in the order written (no fused multiply-add).
 *
 * Conventions: refl(i, n) is reflect-101 (-i for i < 0, 2 n - 2 - i for i >= n); >> is an arithmetic shift; rint rounds half to even.
 *   pyramid   level 0 is the image; level l + 1 has size ((W + 1) / 2, (H + 1) / 2);
 *             out(x, y) = (sum_{i, j = -2..2} k_i k_j in(refl(2 x + i), refl(2 y + j)) + 128) >> 8, k = {1, 4, 6, 4, 1}
 *   gradient  Scharr: Gx(x, y) = 3 (p(x+1, y-1) - p(x-1, y-1)) + 10 (p(x+1, y) - p(x-1, y)) + 3 (p(x+1, y+1) - p(x-1, y+1)), Gy the transpose;
 *             every read of p goes through refl, also where (x, y) itself lies outside the image (the gradient of the reflected image)
 *   window    sample of an image P (a level, its Gx or its Gy) at the FP64 position c:  u = c - 10, iu = floor(u), a = u.x - iu.x, b = u.y - iu.y,
 *             w00 = rint((1 - a) (1 - b) 16384), w01 = rint(a (1 - b) 16384), w10 = rint((1 - a) b 16384), w11 = 16384 - w00 - w01 - w10;
 *             for x, y = 0..20: S(x, y) = w00 P(iu.x + x, iu.y + y) + w01 P(iu.x + x + 1, iu.y + y) + w10 P(iu.x + x, iu.y + y + 1)
 *             + w11 P(iu.x + x + 1, iu.y + y + 1); grey levels: (S + 256) >> 9 (5 fractional bits); gradients: (S + 8192) >> 14
 *   a point p, levels l = levels - 1 .. 0, with p_l = p 2^-l and W_l x H_l the level's size:
 *             the estimate q starts at p_l on the coarsest level and is doubled on the way down.
 *             p_l outside [0, W_l - 1] x [0, H_l - 1]: LOST_OUTSIDE.
 *             I, Dx, Dy = the window samples of the previous pyramid's level, Gx and Gy at p_l.
 *             A11 = sum Dx^2, A12 = sum Dx Dy, A22 = sum Dy^2 as int64 (up to 441 x 4080^2 = 7.3e9); converted to FP64 and multiplied by 2^-20.
 *             D = A11 A22 - A12 A12;  minEig = (A22 + A11 - sqrt((A11 - A22) (A11 - A22) + 4 A12 A12)) / 882.
 *             minEig < 1e-4 or D < 1.1920929e-7: a level above 0 is skipped with q unchanged, at level 0 the point is LOST_FLAT.
 *             iterations j = 0..29:  q outside the level's image: LOST_OUTSIDE.  J = the window sample of the new pyramid's level at q;
 *               b1 = sum (J - I) Dx, b2 = sum (J - I) Dy as int64, times 2^-20;
 *               delta = ((A12 b2 - A22 b1) / D, (A12 b1 - A11 b2) / D);  q += delta;  stop if delta . delta <= 1e-4;
 *               if j > 0 and |delta.x + prev.x| < 0.01 and |delta.y + prev.y| < 0.01: q -= 0.5 delta, then stop (prev = the delta before).
 *             after level 0:  q outside the image: LOST_OUTSIDE;  xr = rint(q.x), yr = rint(q.y): TRACKED iff 1 <= xr < W - 1 and
 *             1 <= yr < H - 1 (the reference's inBorder), LOST_BORDER otherwise.
 *             next_xy is written for every status: the last q, scaled to level 0 (times 2^l where the point was lost at level l).
 * The numerics are restated in tests/ft_ref.py, which the device is held to bit for bit; DESIGN.md 3.10 lists the deviations from
 * cv::calcOpticalFlowPyrLK.  No CPU path: uvs_ft_create fails with UVS_ERR_NO_DEVICE without a GPU. */
#define UVS_FT_MAX_STREAMS 64                 /* largest max_streams uvs_ft_create takes */
#define UVS_FT_MAX_LEVELS 4                   /* levels: 1 .. 4 (the reference's maxLevel = 3 is 4 levels) */
#define UVS_FT_MIN_SIZE 24                    /* smallest width and height of the coarsest level: an image is at least 24 << (levels - 1) */
#define UVS_FT_MAX_POINTS 8192                /* largest max_points (points of one item) */
#define UVS_FT_WINDOW 21                      /* winSize */
#define UVS_FT_MAX_ITERATIONS 30              /* iterations per level */
#define UVS_FT_TRACE_HEADER 16                /* uvs_ft_debug_point: doubles at the head of a level's trace */
#define UVS_FT_TRACE_ITER 10                  /* ... of one iteration */
#define UVS_FT_TRACE_LEVEL 320                /* ... of one level: 16 + 30 x 10, padded */
typedef struct uvs_ft_tracker uvs_ft_tracker;      /* opaque: the slots' pyramids, device buffers, pinned staging, stream */

enum {
    UVS_FT_TRACKED = 0,
    UVS_FT_LOST_FLAT = 1,          /* no texture in the window at level 0 */
    UVS_FT_LOST_OUTSIDE = 2,       /* the point or its estimate left the image */
    UVS_FT_LOST_BORDER = 3         /* converged onto the outermost pixel ring (inBorder) */
};

typedef struct uvs_ft_item {
    const uint8_t *image;              /* [height][width] grey levels, row-major, stride = width: the slot's NEW image (raw, if the slot is equalized) */
    int32_t stream;                    /* the slot, 0 .. max_streams - 1; at most once per call */
    int32_t width;                     /* 24 << (levels - 1) .. max_width; fixed by the slot's first image until uvs_ft_reset */
    int32_t height;                    /* 24 << (levels - 1) .. max_height */
    int32_t n_points;                  /* 0 .. max_points; 0 for a slot that holds nothing */
    const double *points_xy;           /* [n_points][2] pixels in the slot's PREVIOUS image, finite and within UVS_KF_MAX_COORD */
} uvs_ft_item;

/* UVS_ERR_INVALID_ARG: null out, a capacity < 1, levels outside 1..4, max_width or max_height below 24 << (levels - 1);
 * UVS_ERR_CAPACITY: max_streams > UVS_FT_MAX_STREAMS, max_width > UVS_KF_MAX_WIDTH, max_height > UVS_KF_MAX_HEIGHT, max_points > UVS_FT_MAX_POINTS. */
int uvs_ft_create(int device, int max_streams, int max_width, int max_height, int levels, int max_points, uvs_ft_tracker **out);
void uvs_ft_destroy(uvs_ft_tracker *ft);
const char *uvs_ft_last_error(const uvs_ft_tracker *ft);
/* Empties a slot: its next image may have another size and must come without points.  Its mask and its equalization are cleared. */
int uvs_ft_reset(uvs_ft_tracker *ft, int stream);
/* The outputs are PACKED over the items in order (as window_desc of uvs_kf_extract is): next_xy[][2], status[] (UVS_FT_*), iterations[] (the
 * iterations run at level 0), next_norm[][2] (liftProjective of next_xy through `camera`, the uvs_kf_camera of uvs_kf_extract, for TRACKED
 * points; zero for the others); results[n_items] = the number of TRACKED points of each item.
 * UVS_ERR_INVALID_ARG: null pointer, n_items < 1, a negative count, a null array behind a positive count, a stream outside the handle's slots
 * or given twice, points for a slot that holds nothing, a size that differs from the slot's without a reset, a width or height below
 * 24 << (levels - 1), a point that is not finite or beyond UVS_KF_MAX_COORD, a camera that is not finite or whose fx or fy is not positive;
 * UVS_ERR_CAPACITY: n_items, a width, a height or n_points above the handle's capacity.  A rejected call changes no slot, and the handle
 * stays usable after it. */
int uvs_ft_track(uvs_ft_tracker *ft, int n_items, const uvs_ft_item *items, const uvs_kf_camera *camera, double *next_xy, int32_t *status,
                 int32_t *iterations, double *next_norm, int32_t *results);
/* HIP-event time of the last successful uvs_ft_track: upload, the kernels, download, on the handle's stream (milliseconds). */
double uvs_ft_last_device_ms(const uvs_ft_tracker *ft);
/* Diagnostic (tests only): the stored pyramid of a slot.  level_sizes[levels][2] = (width, height) of each level; pixels receives the levels
 * one after the other, each [height_l][width_l] with stride width_l (capacity: pixels_capacity bytes, UVS_ERR_CAPACITY when too small).
 * UVS_ERR_INVALID_ARG for a slot that holds nothing. */
int uvs_ft_debug_pyramid(uvs_ft_tracker *ft, int stream, int32_t *level_sizes, uint8_t *pixels, int64_t pixels_capacity);
/* Diagnostic (tests only): ONE item with ONE point through the same kernels as uvs_ft_track (the slot's state advances as it does there), with
 * every intermediate value: trace[UVS_FT_MAX_LEVELS][UVS_FT_TRACE_LEVEL], level l at trace[l]; entries of a level that was not visited are 0.
 *   [0] 1 when the level was visited   [1..2] p_l   [3..6] w00 w01 w10 w11 of the window at p_l   [7..9] A11 A12 A22 (the integer sums)
 *   [10] D   [11] minEig   [12] 1 when the level was flat   [13] iterations run   [14..15] q when the level was left
 *   [16 + 10 j ..] iteration j: w00 w01 w10 w11 of the window at q, b1 b2 (the integer sums), delta.x delta.y, q.x q.y after the step
 * next_xy[2], status, iterations, next_norm[2] as uvs_ft_track returns them. */
int uvs_ft_debug_point(uvs_ft_tracker *ft, const uvs_ft_item *item, const uvs_kf_camera *camera, double *trace, double *next_xy,
                       int32_t *status, int32_t *iterations, double *next_norm);

/* ---- new points of the point front end (reference feature_tracker/src/feature_tracker.cpp:9-42 setMask, :119-131
 * cv::goodFeaturesToTrack(forw_img, n_pts, MAX_CNT - forw_pts.size(), 0.01, MIN_DIST, mask), :44-52 addPoints) ----
 * uvs_ft_detect finds Shi-Tomasi corners in the image a slot already holds: level 0 of the pyramid that uvs_ft_track stored, so nothing is
 * uploaded but the occupied points.  Every window sum is an integer sum; the FP64 of a pixel is one conversion, one square root and one
 * subtraction, of the threshold one product.  An item gives the same bits alone or in a batch and from run to run, and the slot's pyramid is
 * not altered.  Conventions as above; p(x, y) is the slot's stored level-0 image, W x H.
 *   gradient    Sobel, at every pixel of the image, every read of p through refl:
 *               gx(x, y) = (p(x+1, y-1) - p(x-1, y-1)) + 2 (p(x+1, y) - p(x-1, y)) + (p(x+1, y+1) - p(x-1, y+1)), gy the transpose; |g| <= 1020
 *   sums        blockSize 3, the PRODUCTS reflected (not the image a second time):
 *               A(x, y) = sum_{i, j = -1..1} gx(refl(x+i, W), refl(y+j, H))^2, B the same sum of gx gy, C of gy^2; int32 (<= 9 x 1020^2)
 *   score       S = (A - C)^2 + 4 B^2 as int64 (<= 4.4e14, exact in FP64);  score = (double)(A + C) - sqrt((double)S) >= 0.
 *               cv::cornerMinEigenVal's value is score / (2 x 3060^2); neither the order nor the relative threshold depends on the factor
 *   allowed     a pixel is allowed iff the slot's resident mask (uvs_ft_set_mask) is absent or non-zero there, and for no occupied point
 *               (ox, oy) of the item, xr = rint(ox), yr = rint(oy), is (x - xr)^2 + (y - yr)^2 <= R^2, R = min_distance
 *   threshold   max_score = the largest score over ALL allowed pixels (the border ring too); threshold = quality_level * max_score.
 *               No allowed pixel, or max_score == 0: max_score = threshold = 0 and there are no candidates
 *   candidates  1 <= x <= W - 2, 1 <= y <= H - 2, allowed, score > threshold, and score >= each of the eight neighbours' scores (ties
 *               survive; neighbours that are not allowed still suppress).  n_candidates is their true count; beyond the handle's
 *               max_candidates only the first max_candidates in row-major order are ranked, and the status is UVS_FT_DETECT_OVERFLOW
 *   ranking     by score descending, equal scores by the pixel index y W + x descending
 *   selection   the ranking is walked in order; a candidate is taken iff dx^2 + dy^2 >= R^2 to every candidate taken before it (two points
 *               exactly R apart are both taken); the walk stops at max_new taken
 *   outputs     per taken point, in taking order: (x, y), its score, liftProjective(x, y) through `camera`.
 * The numerics are restated in tests/fd_ref.py, which the device is held to bit for bit; DESIGN.md 3.11 lists the deviations from OpenCV.
 * No CPU path. */
#define UVS_FT_DEFAULT_CANDIDATES 65536       /* max_candidates of a fresh handle */
#define UVS_FT_MAX_CANDIDATES (1 << 20)       /* largest max_candidates */
#define UVS_FT_MAX_MIN_DISTANCE 1024          /* largest min_distance */
enum { UVS_FT_DETECT_OK = 0, UVS_FT_DETECT_OVERFLOW = 1 };

typedef struct uvs_ft_detect_item {
    int32_t stream;                    /* a slot that holds an image */
    int32_t n_occupied;                /* 0 .. max_points */
    int32_t max_new;                   /* 0 .. max_points; 0: nothing is returned */
    int32_t reserved;
    const double *occupied_xy;         /* [n_occupied][2], finite, within UVS_KF_MAX_COORD */
} uvs_ft_detect_item;

typedef struct uvs_ft_detect_result {
    int32_t status;                    /* UVS_FT_DETECT_OK / UVS_FT_DETECT_OVERFLOW */
    int32_t n_new;                     /* points taken, <= max_new */
    int32_t n_candidates;              /* the true count, also on overflow */
    int32_t reserved;
    double max_score, threshold;
} uvs_ft_detect_result;

/* Candidates ranked per item: 1 .. UVS_FT_MAX_CANDIDATES (UVS_ERR_INVALID_ARG outside). */
int uvs_ft_set_max_candidates(uvs_ft_tracker *ft, int max_candidates);
/* mask[height][width], stride = width, of the size of the image the slot holds (UVS_ERR_INVALID_ARG otherwise, or when the slot holds nothing):
 * detection is allowed where it is non-zero.  NULL clears it.  It stays on the device until it is cleared or the slot is reset. */
int uvs_ft_set_mask(uvs_ft_tracker *ft, int stream, const uint8_t *mask, int width, int height);
/* The outputs are PACKED by max_new: item i owns entries off_i .. off_i + n_new_i - 1 of new_xy[][2], new_score[] and new_norm[][2], off_i =
 * the sum of max_new over the items before it; entries past n_new are not written.  results[n_items].
 * UVS_ERR_INVALID_ARG: null pointer, n_items < 1, a stream outside the handle's slots or given twice, a slot that holds nothing, a negative
 * count, a null array behind a positive count, an occupied point that is not finite or beyond UVS_KF_MAX_COORD, quality_level outside (0, 1],
 * min_distance outside 1 .. UVS_FT_MAX_MIN_DISTANCE, a camera that is not finite or whose fx or fy is not positive;
 * UVS_ERR_CAPACITY: n_items, n_occupied or max_new above the handle's capacity.  A rejected call changes nothing, and the handle stays usable. */
int uvs_ft_detect(uvs_ft_tracker *ft, int n_items, const uvs_ft_detect_item *items, double quality_level, int min_distance,
                  const uvs_kf_camera *camera, int32_t *new_xy, double *new_score, double *new_norm, uvs_ft_detect_result *results);
/* HIP-event time of the last successful uvs_ft_detect: upload, the kernels, download, on the handle's stream (milliseconds). */
double uvs_ft_last_detect_device_ms(const uvs_ft_tracker *ft);
/* Diagnostic (tests only): ONE item through the same kernels, with score[H][W], allowed[H][W] (0 or 1), the ranked candidates
 * cand_index[max_candidates] (y W + x) and cand_score[max_candidates] (the first min(n_candidates, max_candidates) entries are written), and
 * the outputs of uvs_ft_detect for the item (arrays of max_new entries). */
int uvs_ft_debug_detect(uvs_ft_tracker *ft, const uvs_ft_detect_item *item, double quality_level, int min_distance,
                        const uvs_kf_camera *camera, double *score, uint8_t *allowed, int32_t *cand_index, double *cand_score,
                        int32_t *new_xy, double *new_score, double *new_norm, uvs_ft_detect_result *result);

/* ---- outlier rejection of the point front end (reference feature_tracker/src/feature_tracker.cpp:149-182 rejectWithF:
 * cv::findFundamentalMat(un_cur_pts, un_forw_pts, cv::FM_RANSAC, F_THRESHOLD, 0.99, status)) ----
 * uvs_ft_reject fits a fundamental matrix to the tracks of a frame by RANSAC over 7-point samples and says which tracks to keep.  It works on
 * the NORMALIZED points (what uvs_ft_track returns as next_norm): the reference's virtual pinhole image, FOCAL_LENGTH x / z + COL / 2, is an
 * isotropic scale and a shift of that plane, so the epipolar distances there are FOCAL_LENGTH times these, and the caller passes
 * threshold = F_THRESHOLD / FOCAL_LENGTH.  It reads no image and alters no slot.  An item gives the same bits alone or in a batch and from run
 * to run.  Every FP64 operation below is one of + - * / sqrt, rounded once, in the order written (no fused multiply-add); the one log is in the
 * stopping rule.  Track i is (x1, y1) = prev_norm[i], (x2, y2) = next_norm[i]; F is row-major and x2' F x1 = 0.
 *   sample      hypothesis h = 0 .. UVS_FT_REJECT_HYPOTHESES - 1 draws with the generator of uvs_lc_verify: z = mix64(seed +
 *               0x9E3779B97F4A7C15 (1 + (h << 20) + a)) mod 2^64, mix64 = the splitmix64 finalizer, draw a = 0, 1, .. gives the track z % n; a
 *               duplicate of an earlier draw of the hypothesis is skipped; 7 distinct tracks within 64 draws or the hypothesis is invalid.  No
 *               collinearity test: a degenerate sample fails the pivot test
 *   null space  row k of the 7 x 9 matrix, from the k-th track drawn: [x2 x1, x2 y1, x2, y2 x1, y2 y1, y2, x1, y1, 1].  Gauss-Jordan with
 *               complete pivoting; no row or column is moved.  Step k = 0 .. 6: the pivot is the largest |a| over the rows and columns that
 *               hold no pivot yet, scanned rows ascending, then columns ascending, taken on a strict >, so ties go to the lowest row, then the
 *               lowest column.  A pivot p that is not |p| > 1e-10 |first pivot| makes the hypothesis invalid.  Over the columns c that hold no
 *               pivot (the pivot's own excluded): a[pr][c] = a[pr][c] / p, then for each of the other six rows r, f = a[r][pc],
 *               a[r][c] = a[r][c] - f a[pr][c].  With c1 < c2 the two columns left over: F1[c1] = 1, F1[c2] = 0, F1[pivot column of row r] =
 *               -a[r][c1]; F2[c1] = 0, F2[c2] = 1, F2[pivot column of row r] = -a[r][c2]
 *   cubic       det(F1 + l F2) = c0 + c1 l + c2 l^2 + c3 l^3.  A_j, B_j: column j of F1, F2;
 *               det3(u, v, w) = (u0 (v1 w2 - v2 w1) - u1 (v0 w2 - v2 w0)) + u2 (v0 w1 - v1 w0);  c0 = det3(A0, A1, A2),
 *               c1 = (det3(B0, A1, A2) + det3(A0, B1, A2)) + det3(A0, A1, B2), c2 = (det3(B0, B1, A2) + det3(B0, A1, B2)) + det3(A0, B1, B2),
 *               c3 = det3(B0, B1, B2);  p(x) = ((c3 x + c2) x + c1) x + c0
 *   roots       the hypothesis is invalid unless c0 .. c3 are finite, c3 != 0 and the Cauchy bound R = 1 + max(|c0|, |c1|, |c2|) / |c3| is
 *               finite.  D = c2 c2 - (3 c3) c1.  D > 0: s = sqrt(D), e1 = (-c2 - s) / (3 c3), e2 = (-c2 + s) / (3 c3), each clamped to [-R, R],
 *               lo = the smaller, hi = the larger, and the monotone intervals are [-R, lo], [lo, hi], [hi, R]; otherwise [-R, R] alone.  An
 *               interval [a, b] holds a root iff (p(a) <= 0 and p(b) > 0) or (p(a) >= 0 and p(b) < 0).  Then 60 bisections: m = 0.5 a + 0.5 b;
 *               b = m if p(m) is strictly on b's side of zero (> 0 in the first case, < 0 in the second), else a = m.  x = 0.5 a + 0.5 b, then
 *               4 Newton steps x' = x - p(x) / (((3 c3) x + 2 c2) x + c1), each taken iff a <= x' <= b.  The roots are numbered r = 0, 1, 2
 *               in ascending interval order; model (h, r) is F = F1 + l_r F2, entry by entry
 *   error       OpenCV's computeError: a = (F0 x1 + F1 y1) + F2, b = (F3 x1 + F4 y1) + F5, c = (F6 x1 + F7 y1) + F8, s2 = (x2 a + y2 b) + c,
 *               d2 = s2 s2 / (a a + b b);  a = (F0 x2 + F3 y2) + F6, b = (F1 x2 + F4 y2) + F7, c = (F2 x2 + F5 y2) + F8, s1 = (x1 a + y1 b) + c,
 *               d1 = s1 s1 / (a a + b b).  A track is an inlier iff d1 <= t t and d2 <= t t, t = threshold (a NaN is an outlier)
 *   selection   OpenCV's RANSACPointSetRegistrator::run replayed over the counts, h-major, then r: h >= niters ends the loop (niters = 1000 at
 *               first); count > max(best, 6) makes (h, r) the best and niters = RANSACUpdateNumIters(confidence, (n - count) / n, 7, niters),
 *               where (1 - ep)^7 is six multiplications, num = log(max(1 - confidence, DBL_MIN)), denom = log(1 - (1 - ep)^7) (niters = 0 if
 *               that argument is < DBL_MIN), and the result is niters if denom >= 0 or -num >= niters (-denom), else num / denom rounded half
 *               to even.  iterations = the hypotheses the loop examined.  The device evaluates the hypotheses in rounds and leaves as soon as
 *               niters <= the hypotheses done, which gives what evaluating all of them gives
 *   outcome     UVS_FT_REJECT_OK: a model was chosen; keep = its inlier mask, n_inliers = its count = the ones of keep, F = the model divided
 *               by its entry of largest magnitude (the first such).  UVS_FT_REJECT_SKIPPED: n < 8 (the reference's forw_pts.size() >= 8);
 *               UVS_FT_REJECT_NO_MODEL: no model reached 7 inliers (a camera at exact rest); in both keep is all ones, n_inliers = n,
 *               hypothesis = root = -1 and F = 0.
 * The numerics are restated in tests/fr_ref.py, which the device is held to bit for bit, except that `iterations` may differ where num / denom
 * lies within rounding of a half-integer, the log being the library's; DESIGN.md 3.12 lists the deviations from OpenCV.  No CPU path. */
#define UVS_FT_REJECT_HYPOTHESES 1000
enum { UVS_FT_REJECT_OK = 0, UVS_FT_REJECT_SKIPPED = 1, UVS_FT_REJECT_NO_MODEL = 2 };

typedef struct uvs_ft_reject_item {
    int32_t n_points;                  /* 0 .. max_points */
    int32_t reserved;
    uint64_t seed;                     /* of the item's samples */
    const double *prev_norm;           /* [n_points][2], finite */
    const double *next_norm;           /* [n_points][2], finite */
} uvs_ft_reject_item;

typedef struct uvs_ft_reject_result {
    int32_t status;                    /* UVS_FT_REJECT_* */
    int32_t n_inliers;                 /* the ones of the item's keep */
    int32_t hypothesis, root;          /* the chosen model, -1 if none */
    int32_t iterations;                /* hypotheses the selection examined */
    int32_t reserved;
    double F[9];                       /* row-major, largest |entry| = 1; 0 if none */
} uvs_ft_reject_result;

/* keep[] is PACKED over the items in order: item i owns n_points_i bytes (1 = keep the track, 0 = drop it).  results[n_items].
 * UVS_ERR_INVALID_ARG: null pointer, n_items outside 1 .. max_streams, n_points outside 0 .. max_points, a null array behind a positive count,
 * a threshold that is not finite and positive, a confidence outside (0, 1), a coordinate that is not finite.  A rejected call changes nothing,
 * and the handle stays usable. */
int uvs_ft_reject(uvs_ft_tracker *ft, int n_items, const uvs_ft_reject_item *items, double threshold, double confidence, uint8_t *keep,
                  uvs_ft_reject_result *results);
/* HIP-event time of the last successful uvs_ft_reject: upload, the kernel, download, on the handle's stream (milliseconds). */
double uvs_ft_last_reject_device_ms(const uvs_ft_tracker *ft);
/* Diagnostic (tests only): ONE item through the same kernel with every round evaluated, and every hypothesis's samples[1000][7] (-1 where the
 * draw failed), models[1000][3][9] (F1 + l_r F2, unscaled; 0 where there is none) and counts[1000][3] (-1 where there is none), besides
 * keep[n_points] and the result as uvs_ft_reject gives them. */
int uvs_ft_debug_reject(uvs_ft_tracker *ft, const uvs_ft_reject_item *item, double threshold, double confidence, int32_t *samples, double *models,
                        int32_t *counts, uint8_t *keep, uvs_ft_reject_result *result);

/* ---- equalization of the front ends' images (reference feature_tracker/src/feature_tracker.cpp:60-66: cv::createCLAHE(3.0, cv::Size(8, 8))
 * ->apply(_img, img) under EQUALIZE; line_feature_tracker.cpp:24-31 has it always on) ----
 * Contrast-limited adaptive histogram equalization of an 8-bit image W x H with clip_limit (FP64, >= 0) and tiles_x x tiles_y tiles (the
 * reference: 3.0, 8, 8).  uvs_ft_set_equalize switches it on for a slot: uvs_ft_track then takes the item's image as the RAW image, equalizes
 * it on the device into level 0 of the slot's new pyramid and builds the levels above from that, so that the tracker, uvs_ft_detect and the
 * next call see the equalized image and nothing else changes.  uvs_ft_equalize equalizes loose images (the line front end's, whose segments the
 * caller still extracts).  Histograms, clipping and the running sums are integers (exact in any order); the float32 operations are the few
 * below, each rounded once, in the order written (no fused multiply-add).  An image gives the same bits alone or in a batch, from run to run
 * and on any machine.  Conventions as above: refl is reflect-101, rint rounds half to even, sat_u8 clamps to 0 .. 255.
 *   padding     if W % tiles_x == 0 and H % tiles_y == 0: Wp = W, Hp = H.  Otherwise Wp = W + tiles_x - W % tiles_x and Hp = H + tiles_y -
 *               H % tiles_y: BOTH are padded, and a dimension that did divide gains a FULL extra tiles_x columns (tiles_y rows).  That is
 *               OpenCV's behaviour (its copyMakeBorder call) and is kept.  The padded image is ext(x, y) = img(refl(x, W), refl(y, H)); it is
 *               never materialized
 *   tile        tw = Wp / tiles_x, th = Hp / tiles_y, N = tw th;  lutScale = 255.0f / (float)N (float32);
 *               clip = 0 if clip_limit == 0, otherwise max((int)(clip_limit N / 256), 1): product and quotient in FP64, then truncated
 *   per tile    h[0 .. 255] = the histogram of ext over the tile.  If clip > 0: clipped = sum max(h[i] - clip, 0); h[i] = min(h[i], clip);
 *               batch = clipped / 256, residual = clipped - 256 batch; batch is added to every bin; if residual > 0, step =
 *               max(256 / residual, 1) and 1 is added to the bins 0, step, 2 step, .. until `residual` of them are done.  The bins still sum
 *               to N.  lut[i] = sat_u8(rint((float)(h[0] + .. + h[i]) lutScale)): the conversion rounds to nearest even, one float32 multiply
 *   per pixel   (x, y) of the original W x H:  txf = (float)x (1.0f / (float)tw) - 0.5f;  tx1 = floor(txf), xa = txf - (float)tx1,
 *               xa1 = 1.0f - xa;  then tx2 = min(tx1 + 1, tiles_x - 1) and tx1 = max(tx1, 0);  the same in y.  With v = img(x, y) and
 *               L(ty, tx) = (float)lut[ty][tx][v]:
 *               res = (L(ty1, tx1) xa1 + L(ty1, tx2) xa) ya1 + (L(ty2, tx1) xa1 + L(ty2, tx2) xa) ya;  out = sat_u8(rint(res)).
 * The numerics are restated in tests/cl_ref.py, which the device is held to bit for bit; DESIGN.md 3.13 has the kernel plan.  OpenCV's own
 * output could not be compared where this was written.  No CPU path. */
#define UVS_FT_CLAHE_MAX_TILES 16             /* largest tiles_x and tiles_y */

typedef struct uvs_ft_image {
    const uint8_t *image;              /* [height][width] grey levels, row-major, stride = width */
    int32_t width;                     /* 24 .. max_width: the reflection of up to 16 padding pixels always fits */
    int32_t height;                    /* 24 .. max_height */
} uvs_ft_image;

/* The equalization state of a slot, like its resident mask: it holds until it is changed or uvs_ft_reset empties the slot (which switches it
 * off).  tiles_x == 0 switches it off (the other arguments are not looked at).  While it is on, uvs_ft_track and uvs_ft_debug_point take the
 * item's image as the raw image.  A call that mixes equalized and plain slots gives every item the bits it gives alone; a call without an
 * equalized slot issues exactly the operations it issued before this existed.
 * UVS_ERR_INVALID_ARG: a stream outside the handle's slots, clip_limit not finite or outside 0 .. 256, tiles_x or tiles_y outside
 * 1 .. UVS_FT_CLAHE_MAX_TILES.  A rejected call changes nothing. */
int uvs_ft_set_equalize(uvs_ft_tracker *ft, int stream, double clip_limit, int tiles_x, int tiles_y);
/* Stateless: equalizes n_images images (1 .. max_streams) with one setting; it touches no slot.  out receives the images PACKED in order, each
 * [height][width] with stride = width.
 * UVS_ERR_INVALID_ARG: null pointer, n_images < 1, a width or height below 24, clip_limit or tiles as above;
 * UVS_ERR_CAPACITY: n_images, a width or a height above the handle's capacity.  A rejected call changes nothing, and the handle stays usable. */
int uvs_ft_equalize(uvs_ft_tracker *ft, int n_images, const uvs_ft_image *images, double clip_limit, int tiles_x, int tiles_y, uint8_t *out);
/* HIP-event time of the last successful uvs_ft_equalize: upload, the kernels, download, on the handle's stream (milliseconds). */
double uvs_ft_last_equalize_device_ms(const uvs_ft_tracker *ft);
/* Diagnostic (tests only): ONE image through the same kernels with every intermediate value: bins[tiles_y][tiles_x][256] (after clipping and
 * redistribution), luts[tiles_y][tiles_x][256], out[height][width] and info[4] = {Wp, Hp, N, clip}. */
int uvs_ft_debug_equalize(uvs_ft_tracker *ft, const uvs_ft_image *image, double clip_limit, int tiles_x, int tiles_y, int32_t *bins,
                          uint8_t *luts, uint8_t *out, int32_t *info);

/* ---- line tracking of the line front end (reference feature_tracker/src/line_feature_tracker.cpp: lineExtraction's lineBiDes->compute,
 * lineMatching, and the matches that readImage4Line :351-433 turns into ids) ----
 * A handle is a line tracker with max_streams slots.  The caller passes the segments of a frame (its own detector's, or uvs_lt_detect's
 * below; uvs_lt_detect_track does both steps) with the image they were found in.  One call takes a batch of items, at most one per slot: it computes one
 * 256-bit LBD descriptor per segment, matches the slot's previous lines (the queries) against the new ones (the train set), and makes the new
 * lines the slot's previous ones: descriptors and gate points stay resident on the device.  A slot that holds nothing (fresh, after
 * uvs_lt_reset, or after a frame without lines) matches nothing.  An item gives the same bits alone or in a batch, from run to run and on any
 * machine: positions, projections and row sums are integers (exact in any order), and the FP64 operations are the few below, each rounded
 * once, in the order written (no fused multiply-add).
 *
 * The rule is this project's own statement of LBD with the default parameters of OpenCV's BinaryDescriptor (9 bands of width 7, one octave);
 * OpenCV's own descriptors could not be compared where this was written.  Two deliberate deviations, both for order-independence and bit
 * equality: sample positions and gradient projections are fixed-point (Q10) where OpenCV keeps float32 running sums, and the direction comes
 * from dx / len, dy / len, not from cos / sin(atan2).  Conventions as above: refl, rint, >> arithmetic; (int) truncates towards zero.
 *   segment     (sx, sy, ex, ey); if sx > ex the ends are swapped (a tie keeps them).  dx = ex - sx, dy = ey - sy, len = sqrt(dx dx + dy dy),
 *               L = (int)len.  Status UVS_LT_SHORT if L < 2, UVS_LT_LONG if L > max_length: the descriptor is all zero, the line is never
 *               matched, and cq = sq = halfWidth = 0; otherwise UVS_LT_OK and cq = rint(1024 dx / len), sq = rint(1024 dy / len),
 *               halfWidth = (L - 1) / 2.  MX = rint(512 (sx + ex)), MY = rint(512 (sy + ey)).  The gate points are ((int)sx, (int)sy) and
 *               ((int)ex, (int)ey) of the ordered ends (the reference stores the truncated values, and getStartPoint() returns them)
 *   gradient    the Sobel gx, gy of uvs_ft_detect's rule over the item's image W x H, reflect-101, |g| <= 1020
 *   support     63 rows h, L columns w:  X = MX + (w - halfWidth) cq - (h - 31) sq,  Y = MY + (w - halfWidth) sq + (h - 31) cq  (int32);
 *               the pixel is x = clamp((X + 512) >> 10, 0, W - 1), y = clamp((Y + 512) >> 10, 0, H - 1)
 *   projections gDL = gx cq + gy sq,  gDO = -gx sq + gy cq  (int32, |.| < 1.5e6)
 *   row sums    S[h][0] = sum_w max(gDL, 0), S[h][1] = sum_w max(-gDL, 0), S[h][2] = sum_w max(gDO, 0), S[h][3] = sum_w max(-gDO, 0): 64-bit
 *               integers (below 2^32 for L <= 2048)
 *   tables      G[h] = exp(-(h - 31)^2 / (2 31^2)), h = 0 .. 62;  Lc[i] = exp(-(i - 10)^2 / (2 7^2)), i = 0 .. 20 (the local sigma is OpenCV's
 *               integer (2 7 + 1) / 2 = 7); computed once on the host with exp in FP64 (uvs_lt_gauss_tables)
 *   bands       for h = 0 .. 62 ascending and each k: r = G[h] (double)S[h][k], r2 = r r, b = h / 7, j = h % 7;
 *               BS[b][k] += Lc[7 + j] r, B2[b][k] += (Lc[7 + j] Lc[7 + j]) r2; if b >= 1 the same into band b - 1 with Lc[14 + j]; if b <= 7 the
 *               same into band b + 1 with Lc[j].  (An accumulator of band b so receives the rows 7 (b - 1) .. 7 (b + 1) + 6 that exist,
 *               ascending, row h with Lc[h - 7 b + 7].)  inv = 1.0 / 14 for the bands 0 and 8, 1.0 / 21 otherwise;  m = BS inv,
 *               sd = sqrt(max(B2 inv - m m, 0));  d[8 b + 2 k] = m, d[8 b + 2 k + 1] = sd
 *   normalise   tm = sum m^2, ts = sum sd^2, each from 0 with b ascending and k ascending within it.  If tm > 0 every m is multiplied by
 *               1 / sqrt(tm); likewise sd with ts.  Every entry above 0.4 becomes 0.4.  desc_float = d (1 / sqrt(sum d^2)), the sum from 0 in
 *               index order; all zero if the sum is 0
 *   bits        byte p = 0 .. 31 takes the p-th pair (a, b) of the lexicographic list (0, 1), (0, 2), .., (0, 8), (1, 2), ..; its bit 7 - i is
 *               d[8 a + i] > d[8 b + i] on the clamped values (the final scale changes no comparison; a tie gives 0)
 *   match       for each previous line q with status OK, t* is the OK current line with the smallest Hamming distance, ties to the lowest
 *               t.  The match is dropped iff the squared distance of the start gate points, or of the end gate points, is > 900 (integers:
 *               exactly 30 px apart passes).  match_of_prev[q] = t* or -1; distance[q] = the Hamming distance to t*, dropped or not, or -1
 *               if q is not OK or there is no OK current line;  prev_of_cur[t] = the LARGEST accepted q that chose t, else -1 (the
 *               reference walks the matches in query order and overwrites).
 * The numerics are restated in tests/lt_ref.py, which the device is held to bit for bit; DESIGN.md 3.14 has the kernel plan.  No CPU path:
 * uvs_lt_create fails with UVS_ERR_NO_DEVICE without a GPU (uvs_lt_gauss_tables needs none). */
#define UVS_LT_MAX_STREAMS 64                 /* largest max_streams uvs_lt_create takes */
#define UVS_LT_MAX_LINES 1024                 /* largest max_lines (segments of one item) = UVS_VP_MAX_LINES */
#define UVS_LT_MAX_LENGTH 2048                /* largest max_length (L of a described segment) */
#define UVS_LT_MIN_SIZE 8                     /* smallest width and height of an image */
#define UVS_LT_ROWS 63                        /* rows of the support region: 9 bands of width 7 */
#define UVS_LT_DESC_FLOATS 72                 /* desc_float: (mean, deviation) of 4 sums in 9 bands */
#define UVS_LT_DESC_BYTES 32
#define UVS_LT_GATE2 900                      /* squared gate of lineMatching: 30 px */
typedef struct uvs_lt_tracker uvs_lt_tracker;      /* opaque: the slots' previous lines, device buffers, pinned staging, stream */

enum { UVS_LT_OK = 0, UVS_LT_SHORT = 1, UVS_LT_LONG = 2 };

typedef struct uvs_lt_item {
    const uint8_t *image;              /* [height][width] grey levels, row-major, stride = width: the (undistorted) image of the segments */
    int32_t stream;                    /* the slot, 0 .. max_streams - 1; at most once per call */
    int32_t width;                     /* UVS_LT_MIN_SIZE .. max_width; it may differ from the slot's last frame */
    int32_t height;                    /* UVS_LT_MIN_SIZE .. max_height */
    int32_t n_lines;                   /* 0 .. max_lines; 0 empties the slot's previous set */
    const double *segments;            /* [n_lines][4]: sx, sy, ex, ey in pixels, finite and within UVS_KF_MAX_COORD; they may leave the image */
} uvs_lt_item;

typedef struct uvs_lt_result {
    int32_t n_described;               /* lines of the item with status UVS_LT_OK */
    int32_t n_matched;                 /* previous lines of the slot with an accepted match */
    int32_t status;                    /* 0 */
} uvs_lt_result;

/* UVS_ERR_INVALID_ARG: null out, a capacity < 1, max_width or max_height below UVS_LT_MIN_SIZE, max_length < 2;
 * UVS_ERR_CAPACITY: max_streams > UVS_LT_MAX_STREAMS, max_width > UVS_KF_MAX_WIDTH, max_height > UVS_KF_MAX_HEIGHT, max_lines >
 * UVS_LT_MAX_LINES, max_length > UVS_LT_MAX_LENGTH. */
int uvs_lt_create(int device, int max_streams, int max_width, int max_height, int max_lines, int max_length, uvs_lt_tracker **out);
void uvs_lt_destroy(uvs_lt_tracker *lt);
const char *uvs_lt_last_error(const uvs_lt_tracker *lt);
/* Empties a slot: its next frame matches nothing. */
int uvs_lt_reset(uvs_lt_tracker *lt, int stream);
/* The outputs are PACKED over the items' lines in order: desc[][32], line_status[] (UVS_LT_*), prev_index[] (prev_of_cur: the index, in the
 * slot's previous frame, of the line this one continues, or -1) and distance[] (the Hamming distance of that match, or -1);
 * results[n_items].
 * UVS_ERR_INVALID_ARG: null pointer, n_items < 1, a negative count, a null array behind a positive count, a null image, a stream outside the
 * handle's slots or given twice, a width or height below UVS_LT_MIN_SIZE, a coordinate that is not finite or beyond UVS_KF_MAX_COORD;
 * UVS_ERR_CAPACITY: n_items, a width, a height or n_lines above the handle's capacity.  A rejected call changes no slot, and the handle stays
 * usable after it. */
int uvs_lt_track(uvs_lt_tracker *lt, int n_items, const uvs_lt_item *items, uint8_t *desc, int32_t *line_status, int32_t *prev_index,
                 int32_t *distance, uvs_lt_result *results);
/* Stateless: the match kernel on the caller's descriptors prev_desc[n_prev][32], cur_desc[n_cur][32] and gate points prev_ends[n_prev][4],
 * cur_ends[n_cur][4] (int32: start x, y, end x, y); every line counts as UVS_LT_OK.  match_of_prev[n_prev], distance[n_prev],
 * prev_of_cur[n_cur].  It touches no slot.
 * UVS_ERR_INVALID_ARG: null pointer behind a positive count, a negative count; UVS_ERR_CAPACITY: n_prev or n_cur above max_lines. */
int uvs_lt_match(uvs_lt_tracker *lt, int n_prev, const uint8_t *prev_desc, const int32_t *prev_ends, int n_cur, const uint8_t *cur_desc,
                 const int32_t *cur_ends, int32_t *match_of_prev, int32_t *distance, int32_t *prev_of_cur);
/* HIP-event time of the last successful uvs_lt_track: upload, the kernels, download, on the handle's stream (milliseconds). */
double uvs_lt_last_device_ms(const uvs_lt_tracker *lt);
/* Diagnostic (tests only): ONE segment[4] of ONE image through the same kernels, with every intermediate value:
 * geom[8] = {L, cq, sq, MX, MY, halfWidth, status, 0}, row_sums[63][4], desc_float[72], desc[32].  It touches no slot. */
int uvs_lt_debug_line(uvs_lt_tracker *lt, const uint8_t *image, int width, int height, const double *segment, int32_t *geom,
                      int64_t *row_sums, double *desc_float, uint8_t *desc);
/* Host only, no GPU needed: the two coefficient tables a handle uploads, G[63] and Lc[21]. */
void uvs_lt_gauss_tables(double *G, double *Lc);

/* ---- segment detection of the line front end (the place of elsed.detect(forw_img) in the reference's lineExtraction) ----
 * Calls on the line tracker's handle.  ELSED's source is not in the reference tree, and a sequential edge walk is the wrong shape for a GPU;
 * this is the project's own statement of a detector, chosen so that every stage is order-independent and the device is held to a numpy
 * restatement (tests/ld_ref.py) bit for bit: Burns-style line-support regions, i.e. connected regions of like gradient orientation in two
 * overlapping orientation partitions, a vote between the partitions, and a weighted moment fit.  No comparison with ELSED or OpenCV output was
 * possible where this was written.  Out of scope: splitting curved regions, a straightness gate (width2 is returned so that a caller can
 * filter), sub-pixel refinement, merging collinear pieces.
 *
 * For one 8-bit image I[H][W] and the parameters grad_threshold T >= 1, min_pixels >= 2, min_length > 0 (conventions as above: refl is
 * reflect-101, >> arithmetic):
 *   1 blur      separable, taps {1, 4, 6, 4, 1}, reflect-101, rows then columns in integers, out = (sum + 128) >> 8
 *   2 gradient  the Sobel gx, gy of the tracking rule above (k_lt_gradient's, reflect-101) on the BLURRED image;  M = |gx| + |gy|;  a pixel is
 *               a support pixel iff M >= T
 *   3 sectors   integers only.  Quadrant q: (gx > 0, gy >= 0) -> 0, (gx <= 0, gy > 0) -> 1, (gx < 0, gy <= 0) -> 2, (gx >= 0, gy < 0) -> 3.  The
 *               vector turned back by q 90 degrees is (px, py) with px > 0, py >= 0: (gx, gy), (gy, -gx), (-gx, -gy), (-gy, gx).
 *               Partition A, boundaries at multiples of 45 degrees:  A = 2 q + (py >= px).
 *               Partition B, boundaries at 22.5 + 45 k degrees:      B = (2 q + (985 py >= 408 px) + (408 py >= 985 px)) mod 8.
 *   4 regions   in each partition two support pixels are linked iff they are 8-neighbours with the same sector; a region is a connected
 *               component, its NAME the smallest linear index y W + x among its pixels, its size n
 *   5 vote      a support pixel votes A iff n_A(its A region) >= n_B(its B region), else B.  A region's support s = the number of its pixels
 *               that voted for its partition.  A region is a candidate iff n >= min_pixels and 2 s > n
 *   6 fit       over ALL pixels of a candidate, relative to its name pixel (x0, y0):  dx = x - x0, dy = y - y0, w = M;  the int64 sums S0, Sx, Sy,
 *               Sxx, Sxy, Syy of w, w dx, w dy, w dx^2, w dx dy, w dy^2 (exact in any order), each converted to FP64 once.  Then, every FP64
 *               operation rounding as written (+ - x / sqrt only, no fused multiply-add):
 *                 mx = Sx / S0, my = Sy / S0;  a = Sxx / S0 - mx mx, c = Syy / S0 - my my, b = Sxy / S0 - mx my;
 *                 h = (a - c) 0.5, r = sqrt(h h + b b);  (ux, uy) = a >= c ? (h + r, b) : (b, r - h);  nrm = sqrt(ux ux + uy uy);
 *                 the region is rejected if nrm == 0;  ux /= nrm, uy /= nrm;  width2 = (a + c) 0.5 - r
 *   7 extent    per pixel t = (dx - mx) ux + (dy - my) uy;  tmin, tmax over the region's pixels (exact in any order);  length = tmax - tmin;
 *               the region is kept iff length >= min_length.  Start = ((x0 + mx) + tmin ux, (y0 + my) + tmin uy), end likewise with tmax
 *   8 output    the kept segments ranked by (length descending, name ascending, partition A before B); the first max_lines (of the handle)
 *               are returned.  Per segment: seg[4] = start x, y, end x, y; width2; info[4] = name, partition (0 = A, 1 = B), n, s.
 * The device equals tests/ld_ref.py bit for bit; DESIGN.md 3.15 has the kernel plan.  No CPU path. */
#define UVS_LT_DET_MAX_THRESHOLD 2040         /* largest grad_threshold: M never exceeds it */
enum { UVS_LT_DET_OK = 0, UVS_LT_DET_OVERFLOW = 1 };      /* OVERFLOW: n_found > max_lines; the first max_lines of the ranking are returned */

typedef struct uvs_lt_det_item {
    const uint8_t *image;              /* [height][width] grey levels, row-major, stride = width */
    int32_t stream;                    /* uvs_lt_detect_track: the slot, at most once per call; uvs_lt_detect ignores it */
    int32_t width;                     /* UVS_LT_MIN_SIZE .. max_width; in uvs_lt_detect_track, for a slot with a map (uvs_lt_set_undistort
                                          below): the RAW frame, of the map's source size */
    int32_t height;                    /* UVS_LT_MIN_SIZE .. max_height */
    int32_t reserved;                  /* 0 */
} uvs_lt_det_item;

typedef struct uvs_lt_det_params {
    int32_t grad_threshold;            /* T: 1 .. UVS_LT_DET_MAX_THRESHOLD */
    int32_t min_pixels;                /* >= 2 */
    double min_length;                 /* > 0, finite */
} uvs_lt_det_params;

typedef struct uvs_lt_det_result {
    int32_t status;                    /* UVS_LT_DET_* */
    int32_t n_found;                   /* all kept segments */
    int32_t n_returned;                /* min(n_found, max_lines) */
    int32_t n_support;                 /* support pixels */
    int32_t n_regions[2];              /* regions of partition A, of partition B (of every size) */
} uvs_lt_det_result;

/* Stateless: it touches no slot.  The outputs hold max_lines rows PER ITEM (item b's rows start at b max_lines; rows from n_returned on are
 * zero): seg[n_items max_lines][4], width2[n_items max_lines], info[n_items max_lines][4]; results[n_items].  An item gives the same bits
 * alone or in a batch.
 * UVS_ERR_INVALID_ARG: null pointer, n_items < 1, a null image, a width or height below UVS_LT_MIN_SIZE, a parameter outside the ranges above;
 * UVS_ERR_CAPACITY: n_items above max_streams, a width or a height above the handle's capacity.  A rejected call changes nothing, and the
 * handle stays usable after it.  The first call allocates the detection's work space (about 160 bytes per pixel of max_streams images of
 * max_width x max_height). */
int uvs_lt_detect(uvs_lt_tracker *lt, int n_items, const uvs_lt_det_item *items, const uvs_lt_det_params *params, double *seg, double *width2,
                  int32_t *info, uvs_lt_det_result *det_results);
/* uvs_lt_detect, then exactly what uvs_lt_track does with the returned segments of every item in the slot item.stream; the image is uploaded
 * once.  seg, width2, info, det_results as above;  desc, line_status, prev_index, distance, results as uvs_lt_track's, PACKED over the items'
 * n_returned lines in order.  The results and the slots afterwards equal uvs_lt_detect followed by uvs_lt_track on the same images, bit for
 * bit.  The checks are those of both calls (a stream outside the slots or given twice: UVS_ERR_INVALID_ARG); a rejected call changes no slot. */
int uvs_lt_detect_track(uvs_lt_tracker *lt, int n_items, const uvs_lt_det_item *items, const uvs_lt_det_params *params, double *seg,
                        double *width2, int32_t *info, uvs_lt_det_result *det_results, uint8_t *desc, int32_t *line_status,
                        int32_t *prev_index, int32_t *distance, uvs_lt_result *results);
/* HIP-event time of the last successful uvs_lt_detect or uvs_lt_detect_track: upload, the kernels, download, on the handle's stream
 * (milliseconds; for uvs_lt_detect_track the detection's and the tracking's added). */
double uvs_lt_last_detect_device_ms(const uvs_lt_tracker *lt);
/* Diagnostic (tests only): ONE image through the detection's kernels with the per-pixel stages, each [height][width]: blur, grad (gx in the
 * low, gy in the high 16 bits), sector_a and sector_b (255 = no support), name_a and name_b (-1 = none), vote (0 = A, 1 = B, 255 = no
 * support).  It touches no slot. */
int uvs_lt_debug_detect(uvs_lt_tracker *lt, const uint8_t *image, int width, int height, const uvs_lt_det_params *params, uint8_t *blur,
                        uint32_t *grad, uint8_t *sector_a, uint8_t *sector_b, int32_t *name_a, int32_t *name_b, uint8_t *vote);

/* ---- undistortion of the line front end's images (reference feature_tracker/src/line_feature_tracker.cpp:35-47 readImage4Line: imageUndistortion
 * :1161-1188 = cv::undistort with the pinhole matrix and k1, k2, p1, p2, then the crop by ROW_MARGIN / COL_MARGIN) ----
 * Calls on the line tracker's handle.  A slot may hold a MAP from the pixels of an undistorted, cropped image Wo x Ho to positions in the raw
 * image W x H; uvs_lt_detect_track then takes the item's image as the RAW frame, and everything it returns is in pixels of the undistorted
 * image.  cv::undistort is not in the reference tree and OpenCV's output could not be compared where this was written; the rule is this
 * project's own integer statement with OpenCV's structure: a fixed-point map with 5 fractional bits, a bilinear blend, a constant zero border.
 * One deliberate deviation: OpenCV rounds a float weight table to 15 bits, here the four weights are the exact products below (they sum to 1024);
 * the two differ by at most one grey level.  Conventions as above: rint rounds half to even, >> is arithmetic.
 *   map         camera = a uvs_kf_camera, margins cm, rm >= 0, Wo = W - 2 cm, Ho = H - 2 rm.  For output pixel (uo, vo): u = uo + cm, v = vo + rm as
 *               doubles, then in FP64, every operation rounded once in the order written (no fused multiply-add):
 *                 x = (u - cx) / fx, y = (v - cy) / fy;  x2 = x x, y2 = y y, xy = x y, r2 = x2 + y2;
 *                 kr = 1 + (k1 r2 + k2 (r2 r2));
 *                 xd = x kr + ((2 p1) xy + p2 (r2 + 2 x2)),  yd = y kr + (p1 (r2 + 2 y2) + (2 p2) xy);
 *                 mx = fx xd + cx, my = fy yd + cy;  X = rint(32 mx), Y = rint(32 my)
 *               X and Y are clamped to -2^24 .. 2^24, a value that is not finite becomes -2^24; both are stored as int32: map_xy[vo][uo] = (X, Y)
 *   remap       xi = X >> 5, ax = X & 31, yi = Y >> 5, ay = Y & 31;  the taps p00 = S(yi, xi), p01 = S(yi, xi + 1), p10 = S(yi + 1, xi),
 *               p11 = S(yi + 1, xi + 1) of the raw image S, a tap outside [0, H) x [0, W) being 0 (decided per tap);
 *               out = ((32 - ax)(32 - ay) p00 + ax (32 - ay) p01 + (32 - ax) ay p10 + ax ay p11 + 512) >> 10
 * With k1 = k2 = p1 = p2 = 0 the map is X = 32 u, Y = 32 v exactly and the output is the cropped input.  The rule is restated in
 * tests/ud_ref.py, which the device is held to word for word and byte for byte; DESIGN.md 3.17 has the kernel plan.  No CPU path.
 *
 * The map is the state of a slot like the camera it describes: it survives uvs_lt_reset (unlike uvs_ft_set_equalize's state, which uvs_ft_reset
 * switches off) and dies with the handle.  Its memory, 8 Wo Ho bytes, is allocated by the slot's first set call.  uvs_lt_detect (stateless, it
 * ignores `stream`) and uvs_lt_track (the segments and their image are the caller's) never look at it.  In uvs_lt_detect_track an item whose
 * slot holds a map must have the map's source size as width x height (else UVS_ERR_INVALID_ARG); after the one upload a kernel writes the
 * undistorted image into device memory, which the detection and the tracking both read.  A call that mixes slots with and without a map gives
 * every item the bits it gives alone; a call without a mapped slot issues exactly the operations it issued before this existed.
 *
 * uvs_lt_set_undistort builds the map of a rad-tan pinhole camera on the device; camera == NULL switches the slot's map off (the other
 * arguments are not looked at).  uvs_lt_set_remap uploads the caller's own map_xy[out_height][out_width][2] in the same convention (any other
 * camera model; values are clamped to -2^24 .. 2^24).  uvs_lt_get_remap returns the slot's sizes and, where map_xy is not NULL, the map.
 * UVS_ERR_INVALID_ARG: a null pointer, a stream outside the handle's slots, a camera that is not finite or with fx or fy <= 0, a negative
 * margin, a source or an output width or height below UVS_LT_MIN_SIZE, uvs_lt_get_remap on a slot without a map;  UVS_ERR_CAPACITY: a source or
 * output width or height above the handle's.  A rejected call changes nothing, and the handle stays usable after it. */
int uvs_lt_set_undistort(uvs_lt_tracker *lt, int stream, const uvs_kf_camera *camera, int width, int height, int col_margin, int row_margin);
int uvs_lt_set_remap(uvs_lt_tracker *lt, int stream, int src_width, int src_height, int out_width, int out_height, const int32_t *map_xy);
int uvs_lt_get_remap(uvs_lt_tracker *lt, int stream, int32_t *out_width, int32_t *out_height, int32_t *map_xy);
/* Undistorts n_images (1 .. max_streams) RAW images, image b through the map of the slot images[b].stream (two images may name one slot;
 * `reserved` is not looked at).  It touches no line state.  out receives the images PACKED in order, each [Ho][Wo] of its slot with stride = Wo.
 * UVS_ERR_INVALID_ARG: null pointer, n_images < 1, a null image, a stream outside the slots, a slot without a map, a width or height that is not
 * the map's source size;  UVS_ERR_CAPACITY: n_images above max_streams.  A rejected call changes nothing. */
int uvs_lt_undistort(uvs_lt_tracker *lt, int n_images, const uvs_lt_det_item *images, uint8_t *out);
/* HIP-event time of the last successful uvs_lt_undistort: upload, the kernel, download, on the handle's stream (milliseconds). */
double uvs_lt_last_undistort_device_ms(const uvs_lt_tracker *lt);

/* ---- camera models of the front ends: MEI and Kannala-Brandt beside the pinhole (reference camera_model/src/camera_models/CataCamera.cc
 * :556-659 liftProjective / spaceToPlane, :766-782 distortion; EquidistantCamera.cc:428-461 liftProjective / spaceToPlane, :716-818
 * backprojectSymmetric; CameraFactory::generateCameraFromYamlFile) ----
 * A uvs_kf_camera is a radial-tangential pinhole.  A uvs_camera_model is one of three models; csrc/uvs_camera_models.h states them once for
 * the device and the host, in FP64, every operation rounded once in the order written (no fused multiply-add); tests/cm_ref.py restates it.
 *   lift      pixel (x, y) -> ray (X, Y, Z) and the normalized point (X / Z, Y / Z), as undistortedPoints forms it.
 *   project   ray -> pixel (spaceToPlane).
 * Below, D(x, y) is the distortion both pinhole and MEI use: x2 = x x, y2 = y y, xy = x y, r2 = x2 + y2, rad = k1 r2 + (k2 r2) r2,
 *   dx = (x rad + ((2 p1) xy)) + p2 (r2 + 2 x2), dy = (y rad + ((2 p2) xy)) + p1 (r2 + 2 y2); and (xd, yd) = (iK11 x + iK13, iK22 y + iK23) with
 *   iK11 = 1 / sx, iK13 = -u0 / sx, iK22 = 1 / sy, iK23 = -v0 / sy for the model's scales (sx, sy) and centre (u0, v0).
 *   PINHOLE   p = fx fy cx cy k1 k2 p1 p2.  lift: uvs_kf_extract's liftProjective unchanged (the recursive model: (xu, yu) = (xd, yd), then 8 times
 *             (xu, yu) = (xd, yd) - D(xu, yu); none when k1 = k2 = p1 = p2 = 0), ray = (xu, yu, 1): the bits of the same camera given as a
 *             uvs_kf_camera.  project: x = X / Z, y = Y / Z, then the forward map of uvs_lt_set_undistort above (kr, xd, yd, mx, my).
 *   MEI       p = xi k1 k2 p1 p2 gamma1 gamma2 u0 v0.  lift: (xu, yu) as for the pinhole with (gamma1, gamma2, u0, v0) (none of the 8 passes when
 *             the four coefficients are 0), then Z = ((1 - xu xu) - yu yu) / 2 when xi == 1, else rho2 = xu xu + yu yu,
 *             Z = 1 - (xi (rho2 + 1)) / (xi + sqrt(1 + (1 - xi xi) rho2)); ray = (xu, yu, Z).  project: n = sqrt(X X + (Y Y + Z Z)), z = Z + xi n,
 *             x = X / z, y = Y / z, (x, y) += D(x, y) unless the four coefficients are 0, pixel = (gamma1 x + u0, gamma2 y + v0).  Multiplies, adds,
 *             divides and one correctly rounded sqrt: the device and the restatement agree bit for bit.
 *   KANNALA_BRANDT  p = k2 k3 k4 k5 mu mv u0 v0.  With t = th th:  r(th) = th + th (t (k2 + t (k3 + t (k4 + t k5)))),
 *             r'(th) = 1 + t (3 k2 + t (5 k3 + t (7 k4 + t (9 k5)))).  th_max: the first th in (0, pi] with r'(th) <= 0, found once per model on the
 *             host (a scan of r' at i pi / 4096, i = 1 .. 4096, then the bisection of that step down to neighbouring doubles; th_max is the
 *             lower one, where r' > 0), or pi if there is none; r_max = r(th_max).
 *             lift: (px, py) = (xd, yd) with (mu, mv, u0, v0), rr = sqrt(px px + py py).  th = rr when the four k are 0 or !(rr < r_max);
 *             otherwise the root of r(th) = rr on [0, th_max] by a safeguarded Newton iteration: lo = 0, hi = th_max, th = min(rr, th_max), then
 *             at most UVS_CAM_KB_ITERATIONS times: f = r(th) - rr; stop if f == 0; hi = th if f > 0 else lo = th; tn = th - f / r'(th); stop if
 *             tn == th or tn == the th of the step before (two neighbouring doubles straddle the root: the later one is kept);
 *             tn = (lo + hi) / 2 unless lo <= tn <= hi; th = tn.  ray = ((sin th px) / rr, (sin th py) / rr, cos th), and
 *             (sin th, 0, cos th) when rr < 1e-10 (the reference's phi = 0).
 *             project: h = sqrt(X X + Y Y), th = atan2(h, Z), q = r(th), pixel = (mu ((q X) / h) + u0, mv ((q Y) / h) + v0), and (mu q + u0, v0)
 *             when h == 0.  Neither direction forms phi.
 *             Deviation: the reference takes th as the smallest non-negative real eigenvalue of the polynomial's companion matrix, per pixel.
 *             On the first monotone branch [0, th_max] that is the root found here (tests/cm_ref.py holds both to a 60-digit evaluation of
 *             the reference's definition over the image rectangles of the shipped fisheye configurations).  For rr beyond the branch the
 *             reference would return a root of a later, physically meaningless branch if one exists; here th = rr, the reference's own
 *             fallback when it finds no root.  sin, cos and atan2 are the device library's: KB results are held to a tolerance, not to bits.
 *
 * uvs_ft_set_camera_model / uvs_kf_set_camera_model put a model on a handle (model == NULL takes it off).  While a tracker holds one,
 * uvs_ft_track, uvs_ft_detect, uvs_ft_debug_point and uvs_ft_debug_detect lift next_norm / new_norm through it; while an extractor holds one,
 * uvs_kf_extract and uvs_kf_debug_frame lift keypoints_norm through it.  Their `camera` argument may then be NULL and is not looked at.
 * Nothing else of those calls changes, and without a model they issue exactly the operations they issued before.  The model is the
 * handle's, not a slot's: it survives uvs_ft_reset.
 *
 * uvs_ft_lift / uvs_ft_project: n loose points through a model on the tracker's device and stream (the place of m_camera->liftProjective and
 * spaceToPlane for a caller with points of its own, e.g. in front of uvs_ft_reject); one thread per point, and a point gets the bits it gets
 * alone.  xy[n][2], ray[n][3], norm[n][2]; either output of uvs_ft_lift may be NULL.  n == 0 is a successful no-op.
 *
 * uvs_lt_set_undistort_model builds a slot's undistortion map for any model (camodocal's initUndistortRectifyMap with the identity rotation):
 * for output pixel (uo, vo), u = uo + cm, v = vo + rm, the ray ((u - cx_out) / fx_out, (v - cy_out) / fy_out, 1) of the output pinhole goes
 * through project of the model to the raw position (mx, my), which is quantised and stored exactly as uvs_lt_set_undistort does.  The slot's
 * state is the same, so uvs_lt_get_remap, uvs_lt_undistort and uvs_lt_detect_track work on it unchanged; a PINHOLE model whose output pinhole
 * is its own (fx, fy, cx, cy) gives uvs_lt_set_undistort's map.  model == NULL switches the slot's map off.
 *
 * UVS_ERR_INVALID_ARG: a null pointer, n < 0, an unknown model id, a parameter p[0 .. count) that is not finite, a scale (fx / fy, gamma1 /
 * gamma2, mu / mv, fx_out / fy_out) <= 0, xi < 0, and for the map the size and margin checks of uvs_lt_set_undistort (UVS_ERR_CAPACITY alike).
 * A rejected call changes nothing, and the handle stays usable after it.  DESIGN.md 3.18 has the kernel plan.  No CPU path. */
#define UVS_CAM_PINHOLE 0
#define UVS_CAM_MEI 1
#define UVS_CAM_KANNALA_BRANDT 2
#define UVS_CAM_KB_ITERATIONS 32              /* most Newton / bisection steps of the Kannala-Brandt root search */
typedef struct uvs_camera_model {
    int32_t model;      /* UVS_CAM_* */
    int32_t reserved;
    double  p[12];      /* PINHOLE: fx fy cx cy k1 k2 p1 p2 | MEI: xi k1 k2 p1 p2 gamma1 gamma2 u0 v0 | KANNALA_BRANDT: k2 k3 k4 k5 mu mv u0 v0 */
} uvs_camera_model;
int uvs_ft_set_camera_model(uvs_ft_tracker *ft, const uvs_camera_model *model);
int uvs_kf_set_camera_model(uvs_kf_extractor *kf, const uvs_camera_model *model);
int uvs_ft_lift(uvs_ft_tracker *ft, const uvs_camera_model *model, int n, const double *xy, double *ray, double *norm);
int uvs_ft_project(uvs_ft_tracker *ft, const uvs_camera_model *model, int n, const double *ray, double *xy);
int uvs_lt_set_undistort_model(uvs_lt_tracker *lt, int stream, const uvs_camera_model *model, int width, int height, int col_margin,
                               int row_margin, double fx_out, double fy_out, double cx_out, double cy_out);

/* ---- place recognition of loop closure (reference pose_graph/src/pose_graph.cpp:304-386 detectLoop; ThirdParty/DBoW/TemplatedVocabulary.h
 * transform, TemplatedDatabase.h add / queryL1, BowVector.cpp addWeight / normalize) ----
 * Which old keyframe to try: a vocabulary tree over 256-bit BRIEF descriptors, the tf-idf bag-of-words vector of a keyframe, and the L1 query
 * of an append-only database of such vectors.  Everything below is integer arithmetic or FP64 in a stated order, so a keyframe gives the same
 * bits alone or in a batch, from run to run and on any machine; tests/pr_ref.py restates it.
 *   vocabulary  the caller's, in the arrays of the reference's binary file (ThirdParty/VocabularyBinary.hpp: records {nodeId, parentId, weight,
 *               descriptor[4]} and {nodeId, wordId}); the root is node 0 and has no record; a node's children are in the order of their
 *               records.  Descriptor bit i is bit (i & 63) of word (i >> 6), the layout of uvs_kf_extract's desc.  Only weightingType 0
 *               (TF_IDF) and scoringType 0 (L1_NORM).
 *   transform   a descriptor descends from the root, at every inner node to the child of the smallest Hamming distance, a tie to the earlier
 *               child; the leaf it ends at gives (word id, weight).  The vector of a keyframe: words of weight <= 0 dropped; per word
 *               v = w, then v += w once per further occurrence; norm = the sum of |v| in ascending word id, one add after the other; every v
 *               divided by norm when norm > 0.  Sorted by word id.
 *   query       entry e of a database of n entries is eligible iff e < max_id || max_id == -1 || e == n - 1.  Its raw score is
 *               s(e) = sum over the words it shares with the query, in ascending word id, of |q - d| - |q| - |d|, starting from the first
 *               term; an entry that shares no word is no result.  Results in ascending s, a tie to the lower entry id (the reference's
 *               std::sort leaves ties open: this is the library's definition), cut to max_results (0: all), Score = -s / 2.
 *   detect      detectLoop: query(4, frame_index - 50), then add; a loop iff Score[0] > 0.05 and some i >= 1 has Score[i] > 0.015; when
 *               frame_index > 50 as well, the smallest id among result 0 (whatever its score) and the results i >= 1 with Score[i] > 0.015;
 *               otherwise -1.
 * No CPU path: uvs_pr_create fails with UVS_ERR_NO_DEVICE without a GPU (uvs_pr_check_vocabulary needs none). */
#define UVS_PR_MAX_K 16                       /* most children of a node: one lane of a 16-lane group each (DBoW2 vocabularies in use have k = 10) */
#define UVS_PR_MAX_L 16                       /* largest depth L */
#define UVS_PR_MAX_FRAMES 64                  /* most keyframes of one uvs_pr_transform / uvs_pr_add / uvs_pr_query call */
#define UVS_PR_DETECT_RESULTS 4               /* results detectLoop asks for */
typedef struct uvs_place_recognizer uvs_place_recognizer;  /* opaque: the vocabulary and the database on the device, staging, stream */

/* Host only.  node_id / parent_id / weight / descriptor[][4]: the n_nodes node records; word_node_id / word_id: the n_words word records.
 * UVS_ERR_UNSUPPORTED: a weighting or scoring other than 0.  UVS_ERR_INVALID_ARG with a text in message (message_capacity bytes, may be
 * NULL): a null array, k outside 1 .. UVS_PR_MAX_K, L outside 1 .. UVS_PR_MAX_L, a node id outside 1 .. n_nodes or given twice, a parent
 * outside 0 .. n_nodes, a cycle, a node deeper than L, more than UVS_PR_MAX_K children, a word id outside 0 .. n_words - 1 or given twice,
 * a node with two words, a leaf without a word, a word on an inner node, a root without children, a weight that is negative or not finite.
 * Leaves may sit above depth L, and ids need not be contiguous among siblings. */
int uvs_pr_check_vocabulary(int k, int L, int scoring_type, int weighting_type, int n_nodes, const int32_t *node_id, const int32_t *parent_id,
                            const double *weight, const uint64_t *descriptor, int n_words, const int32_t *word_node_id, const int32_t *word_id,
                            char *message, int message_capacity);
/* max_features: most descriptors of a keyframe, 1 .. UVS_LC_MAX_OLD (what uvs_kf_extract returns at most).  initial_entries >= 1: the
 * database's first capacity; it grows by doubling (a new buffer, a device-to-device copy, the old one freed).  The checks of
 * uvs_pr_check_vocabulary apply; UVS_ERR_CAPACITY: max_features above its bound. */
int uvs_pr_create(int device, int k, int L, int scoring_type, int weighting_type, int n_nodes, const int32_t *node_id, const int32_t *parent_id,
                  const double *weight, const uint64_t *descriptor, int n_words, const int32_t *word_node_id, const int32_t *word_id,
                  int max_features, int initial_entries, uvs_place_recognizer **out);
void uvs_pr_destroy(uvs_place_recognizer *pr);
const char *uvs_pr_last_error(const uvs_place_recognizer *pr);
/* Entries in the database / forget them all (the capacity stays). */
int uvs_pr_size(const uvs_place_recognizer *pr);
int uvs_pr_clear(uvs_place_recognizer *pr);
/* n_features[n_frames]; descriptors[][4] PACKED over the frames in order.  words_out[] / weights_out[]: one per descriptor, packed alike
 * (stop words included).  bow_n[n_frames]; bow_words / bow_values are STRIDED: frame f owns entries f * max_features .. + bow_n[f] - 1.
 * Changes no state.  UVS_ERR_INVALID_ARG: null pointer, n_frames < 1, a negative count; UVS_ERR_CAPACITY: n_frames > UVS_PR_MAX_FRAMES or
 * a count above max_features.  An empty frame (n_features 0) is valid everywhere below. */
int uvs_pr_transform(uvs_place_recognizer *pr, int n_frames, const int32_t *n_features, const uint64_t *descriptors, int32_t *words_out,
                     double *weights_out, int32_t *bow_n, int32_t *bow_words, double *bow_values);
/* Appends the vectors of n_frames keyframes in order; entry_ids[n_frames] = their entry ids (the order of addition since the last clear). */
int uvs_pr_add(uvs_place_recognizer *pr, int n_frames, const int32_t *n_features, const uint64_t *descriptors, int32_t *entry_ids);
/* n_frames queries against the database as it is; changes no state.  max_results >= 0 (0: all); max_id[n_frames].  n_results[n_frames];
 * ids / scores are STRIDED by (max_results > 0 ? max_results : uvs_pr_size()) per frame. */
int uvs_pr_query(uvs_place_recognizer *pr, int n_frames, const int32_t *n_features, const uint64_t *descriptors, int max_results,
                 const int32_t *max_id, int32_t *n_results, int32_t *ids, double *scores);
/* detectLoop for one keyframe: the query, the add (one transform serves both), the gates.  ids / scores: UVS_PR_DETECT_RESULTS entries. */
int uvs_pr_detect(uvs_place_recognizer *pr, int n_features, const uint64_t *descriptors, int frame_index, int32_t *loop_index,
                  int32_t *n_results, int32_t *ids, double *scores);
/* HIP-event time of the last successful call on the handle's stream (milliseconds): part 0 the whole call, 1 the transform (upload, descent,
 * vector), 2 the query (scoring, download); a part the call did not run is 0. */
double uvs_pr_last_device_ms(const uvs_place_recognizer *pr, int part);

/* ---- triangulation of landmarks: the state a solve starts from (uvs_tri_*, csrc/uvs_triangulate.hip; additions only, the ABI version stays 7) ----
 * FeatureManager::triangulate (feature_manager.cpp:427-481), triangulateLine (:504-589, calcPluckerLine :827-902), the validity rule of
 * setLineOrtho (:352-416) and the re-anchoring of removeBackShiftDepth (:627-634) for whole batches of landmarks, one lane per landmark, FP64.
 * The caller lists only the landmarks to be worked on: the reference's selection rules (used_num >= 2 && start_frame < WINDOW_SIZE - 2,
 * estimated_depth <= 0, orthonormal_vec[3] == 0 with at least two views) stay host bookkeeping.
 *   point       camera k of a track is frame pt_start + k, the start frame's own view included; its pose relative to the start camera gives
 *               P = [R^T | -R^T t]; with f = obs / |obs| the rows f0 P.row(2) - f2 P.row(0) and f1 P.row(2) - f2 P.row(1) make the 2n x 4 matrix
 *               svd_A; depth = V[2] / V[3] of its smallest right singular vector (of svd_A itself, never of svd_A^T svd_A).
 *               pt_flag 0: kept.  1: the value was < 0.1, init_depth is returned (:475-478).  2: the value was not finite, init_depth is
 *               returned -- a stated deviation, the reference lets a NaN through into para_Feature.
 *   line        a = sp_i x ep_i; b = (R_rel sp_j) x (R_rel ep_j); beta = -b . t_rel; d_l = b x a; n_l = a beta; d_w = R_left d_l;
 *               n_w = R_left n_l + t_left x d_w; U = [n_w / |n_w|, d_w / |d_w|, (n_w x d_w) / |n_w x d_w|];
 *               orth = (Eigen 3.3 eulerAngles(0, 1, 2) of U with the first angle in [0, pi], atan2(|d_w|, |n_w|)).
 *               ln_flag 0: ok.  2: |d_w|, |n_w| or |n_w x d_w| is zero or not finite; orth is four zeros ("no parameters yet" to the caller's
 *               own rule) -- the second stated deviation, the reference stores NaN.
 *   check       with orth_old, the line in the start camera, cut by the two planes through the first observation's end points (each spanned by
 *               the end point and the end point moved by (1, -(ep_x - sp_x) / (ep_y - sp_y)); the division and what follows from it are the
 *               reference's); flag 2 where D_s(2) / w_s < 0 or D_e(2) / w_e < 0, else 1.
 *   shift       depth_out = (new_R^T (marg_R (uv0 depth) + marg_P - new_P)).z, flag 0; where that is not > 0: the handle's init_depth, flag 1.
 * No CPU path: uvs_tri_create fails with UVS_ERR_NO_DEVICE without a GPU. */
#define UVS_TRI_MAX_WINDOWS 4096              /* largest max_windows uvs_tri_create takes */
#define UVS_TRI_MAX_LANDMARKS (1 << 22)       /* largest max_points / max_lines; max_point_obs up to UVS_NUM_FRAMES times as many */
typedef struct uvs_tri uvs_tri;               /* opaque: device buffers, pinned staging, stream */

typedef struct uvs_tri_batch {
    int32_t n_windows, n_points, n_lines, reserved;
    const double *pose;                /* [n_windows][UVS_NUM_FRAMES][7], as uvs_window.pose */
    const double *ex_pose;             /* [n_windows][7], as uvs_window.ex_pose */
    const int32_t *pt_window;          /* [n_points], non-decreasing */
    const int32_t *pt_start;           /* [n_points] start frame */
    const int32_t *pt_obs_begin;       /* [n_points + 1]: track k owns observations pt_obs_begin[k] .. pt_obs_begin[k + 1] - 1; [0] = 0 */
    const double *pt_obs;              /* [n_obs][3]: observation k of a track belongs to frame pt_start + k */
    const int32_t *ln_window;          /* [n_lines], non-decreasing */
    const int32_t *ln_fi, *ln_fj;      /* [n_lines] frame of the first / of the last observation */
    const double *ln_sp_i, *ln_ep_i;   /* [n_lines][3] end points of the first observation */
    const double *ln_sp_j, *ln_ep_j;   /* [n_lines][3] end points of the last observation */
} uvs_tri_batch;

/* UVS_ERR_INVALID_ARG: null out or a capacity < 1 (max_point_obs < 2); UVS_ERR_CAPACITY: a capacity above its bound. */
int uvs_tri_create(int device, int max_windows, int max_points, int max_point_obs, int max_lines, uvs_tri **out);
void uvs_tri_destroy(uvs_tri *t);
const char *uvs_tri_last_error(const uvs_tri *t);
/* The init_depth of uvs_tri_shift_depth (uvs_tri_triangulate takes its own as an argument): a setter, not a create argument.  A new
 * handle holds 5.0, INIT_DEPTH of the reference's configurations.  UVS_ERR_INVALID_ARG unless positive and finite. */
int uvs_tri_set_init_depth(uvs_tri *t, double init_depth);
/* One upload, the kernels, one download.  depth[n_points], pt_flag[n_points], orth[n_lines][4], ln_flag[n_lines].  n_points == 0, n_lines == 0
 * or both are valid (both: UVS_OK with nothing launched; the arrays of an empty kind may be NULL).  Every refusal is UVS_ERR_INVALID_ARG and
 * happens before anything is launched: a null pointer, a negative count, n_windows < 1, init_depth not positive and finite, a track with
 * fewer than 2 or more than UVS_NUM_FRAMES views, pt_start < 0 or pt_start + views > UVS_NUM_FRAMES, pt_obs_begin[0] != 0, ln_fi < 0,
 * ln_fj > UVS_WINDOW_SIZE or ln_fj <= ln_fi, a window index outside 0 .. n_windows - 1 or decreasing, or a count (windows, points,
 * observations, lines) above the handle's capacity.  A refused call changes nothing and the handle stays usable. */
int uvs_tri_triangulate(uvs_tri *t, const uvs_tri_batch *batch, double init_depth, double *depth, int32_t *pt_flag, double *orth,
                        int32_t *ln_flag);
/* pose / ex_pose / ln_window as in uvs_tri_batch; ln_start[n_lines] in 0 .. UVS_WINDOW_SIZE; ln_sp0 / ln_ep0 [n_lines][3] the first
 * observation; orth_old[n_lines][4]; flag[n_lines] = 1 (valid) or 2.  n_lines == 0: UVS_OK, nothing launched.  Refusals as above. */
int uvs_tri_check_lines(uvs_tri *t, int n_windows, const double *pose, const double *ex_pose, int n_lines, const int32_t *ln_window,
                        const int32_t *ln_start, const double *ln_sp0, const double *ln_ep0, const double *orth_old, int32_t *flag);
/* uv0[n_points][3], depth[n_points]; marg_R / new_R [3][3] row-major, marg_P / new_P [3]: the camera poses of the departed and of the new
 * oldest frame.  depth_out[n_points], flag[n_points].  n_points == 0: UVS_OK, nothing launched.  Refusals as above. */
int uvs_tri_shift_depth(uvs_tri *t, int n_points, const double *uv0, const double *depth, const double *marg_R, const double *marg_P,
                        const double *new_R, const double *new_P, double *depth_out, int32_t *flag);
/* HIP-event time of the kernels of the last successful call on the handle's stream, upload and download excluded (milliseconds). */
double uvs_tri_last_device_ms(const uvs_tri *t);

/* ---- IMU pre-integration for batches of intervals (uvs_imu_*, csrc/uvs_imu_preintegrate.hip; additions only, the ABI version stays 7) ----
 * IntegrationBase::push_back / propagate / midPointIntegration / repropagate (integration_base.h:30-158) for a batch of intervals in one
 * launch, one wavefront per interval, FP64.  Per sample (dt, acc_1, gyr_1), with R(q) Eigen's toRotationMatrix() polynomial:
 *   un_gyr = (gyr_0 + gyr_1) / 2 - bg;  rq = delta_q * (un_gyr dt / 2, 1), used UN-normalised in this step;
 *   un_acc = (R(delta_q) (acc_0 - ba) + R(rq) (acc_1 - ba)) / 2;  rp = delta_p + delta_v dt + un_acc dt^2 / 2;  rv = delta_v + un_acc dt;
 *   F (15 x 15) and V (15 x 18) as in midPointIntegration;  jacobian = F jacobian;  covariance = F covariance F^T + V noise V^T with
 *   noise = diag(acc_n, gyr_n, acc_n, gyr_n, acc_w, gyr_w)^2 (x) I3;  then delta_q = rq / |rq|, delta_p = rp, delta_v = rv, sum_dt += dt,
 *   (acc_0, gyr_0) = (acc_1, gyr_1).  skip = sum_dt > 10.0.  An interval without samples yields the empty pre-integration: identity delta and
 *   jacobian, zero covariance, sum_dt = 0.  Re-propagation is the same call with other biases.
 * Dead reckoning (state_p / state_R / state_v set): in the same walk, processIMU's prediction (estimator.cpp:104-117) from the state of frame i:
 *   R' = R R(deltaQ(un_gyr dt)) with deltaQ = (theta / 2, 1) not normalised, no re-normalisation of R;
 *   a = ((R (acc_0 - ba) - g) + (R' (acc_1 - ba) - g)) / 2;  P += dt V + dt^2 a / 2;  V += dt a.
 * No CPU path: uvs_imu_create fails with UVS_ERR_NO_DEVICE without a GPU. */
#define UVS_IMU_MAX_INTERVALS 65536           /* largest max_intervals uvs_imu_create takes */
#define UVS_IMU_MAX_SAMPLES (1 << 22)         /* largest max_samples */
#define UVS_IMU_STAGE_CHUNK 64                /* samples the kernel stages at a time (one per lane); of interest to tests only */
typedef struct uvs_imu uvs_imu;               /* opaque: device buffers, pinned staging, stream, the noise values */

typedef struct uvs_imu_batch {
    int32_t n_intervals;
    const int32_t *sample_begin;   /* [n_intervals + 1], [0] = 0, non-decreasing: interval k owns samples sample_begin[k] .. sample_begin[k+1]-1 */
    const double *acc_0, *gyr_0;   /* [n_intervals][3] the sample the interval starts from */
    const double *ba, *bg;         /* [n_intervals][3] linearized_ba / linearized_bg */
    const int32_t *frame_i;        /* [n_intervals] copied into the block; may be NULL (0) */
    const double *dt;              /* [n_samples] */
    const double *acc, *gyr;       /* [n_samples][3] */
    /* dead reckoning, all NULL or all set */
    const double *state_p, *state_R, *state_v;   /* [n_intervals][3], [9] (row-major), [3] */
    double gravity[3];
} uvs_imu_batch;

/* UVS_ERR_INVALID_ARG: null out or a capacity < 1; UVS_ERR_CAPACITY: a capacity above its bound. */
int uvs_imu_create(int device, int max_intervals, int max_samples, uvs_imu **out);
void uvs_imu_destroy(uvs_imu *h);
const char *uvs_imu_last_error(const uvs_imu *h);
/* The four noise densities of `noise`.  A new handle holds the EuRoC values 0.08, 0.004, 0.00004, 2.0e-6.  UVS_ERR_INVALID_ARG unless all
 * are positive and finite (the values then stay as they were). */
int uvs_imu_set_noise(uvs_imu *h, double acc_n, double gyr_n, double acc_w, double gyr_w);
/* One upload, the launch, one download.  blocks[n_intervals] (linearized_ba / bg and frame_i copied from the batch); with dead reckoning
 * pred_p[n_intervals][3], pred_R[n_intervals][9], pred_v[n_intervals][3], else the three are not touched and may be NULL.
 * n_intervals == 0: UVS_OK, nothing launched.  Every refusal happens before anything is launched, writes nothing and leaves the handle usable.
 * UVS_ERR_INVALID_ARG: a null pointer (the sample arrays may be NULL when there are no samples), a negative count, sample_begin[0] != 0 or
 * a decreasing sample_begin, a dt that is negative or not finite, a sample, bias, state or gravity that is not finite, a dead-reckoning trio
 * set only in part or its outputs missing.  UVS_ERR_CAPACITY: n_intervals or the sample count above the handle's capacity. */
int uvs_imu_preintegrate(uvs_imu *h, const uvs_imu_batch *b, uvs_imu_block *blocks, double *pred_p, double *pred_R, double *pred_v);
/* HIP-event time of the kernel of the last successful call, upload and download excluded (milliseconds). */
double uvs_imu_last_device_ms(const uvs_imu *h);

/* ---- relative pose of window pairs: the bootstrap's choice of its reference frame (uvs_rp_*, csrc/uvs_relative_pose.hip; additions only, the
 * ABI version stays 7) ----
 * Estimator::relativePose (estimator.cpp:448-477) with MotionEstimator::solveRelativeRT (initial/solve_5pts.cpp:193-227) and that file's
 * recoverPose / decomposeEssentialMat (:5-182), for a batch of frame pairs.  An item is the correspondences of one pair (frame_l, WINDOW_SIZE)
 * of one window (what FeatureManager::getCorresponding returns, host bookkeeping): left[i], right[i] the normalized points of track i in the
 * two frames.  The ten pairs of a window are ten items of one launch, many windows one batch; a window's answer is its first item with ok.
 * An item gives the same bits alone or in a batch and from run to run.  Every FP64 operation of steps 1 to 3 is one of + - * / sqrt, rounded
 * once, in the order written (no fused multiply-add): they are held bit for bit to tests/rp_ref.py and tests/fr_ref.py.  Steps 4 to 6 are
 * held to the 60-digit evaluation of tests/rp_ref.py: the counts, masks and the choice exactly, R and t within a bound.
 *   1 gate      n > min_corres, else status UVS_RP_FEW_CORRES.  average_parallax = (the sum over i = 0 .. n - 1, in that order, of
 *               sqrt(dx dx + dy dy), dx = left_x - right_x, dy = left_y - right_y on the points as given) / n;
 *               average_parallax focal_length > min_parallax_px, else UVS_RP_LOW_PARALLAX.  n >= min_ransac_points, else UVS_RP_FEW_POINTS.
 *               A gated item has ok = 0, runs no RANSAC (its workgroup leaves at once) and no recovery; its other fields are 0 (hypothesis
 *               = root = chosen = -1, ransac.status = UVS_FT_REJECT_SKIPPED, an all-zero mask); n = 0 gives average_parallax = 0
 *   2 rounding  solveRelativeRT turns the points into cv::Point2f: from here on every coordinate is rounded to float32 (to nearest even) and
 *               widened again
 *   3 RANSAC    uvs_ft_reject's rule, unchanged, on the rounded points (prev = left, next = right) with f_threshold, confidence and the
 *               item's seed; `ransac` is its result block.  UVS_FT_REJECT_NO_MODEL gives status UVS_RP_NO_MODEL, ok = 0 -- a stated
 *               deviation, the reference would hand an empty matrix to recoverPose
 *   4 decompose F = U diag(s) V^T with s0 >= s1 >= s2.  The signs, which the reference leaves to its SVD routine, are fixed here: each right
 *               singular vector v_k, k = 0, 1, 2, has its entry of largest magnitude (the first such) positive; u_k = F v_k / s_k for k = 0, 1;
 *               u_2 = u_0 x u_1 with the sign that makes ITS entry of largest magnitude positive.  Then U is negated if det(U) < 0, V^T if
 *               det(V^T) < 0.  W = [[0,1,0],[-1,0,0],[0,0,1]]; R1 = U W V^T, R2 = U W^T V^T, t = U[:,2]
 *               An F with s1 = 0 (rank < 2) or a singular value that is not finite has no such decomposition: UVS_RP_NO_MODEL, ok = 0,
 *               the fields behind `ransac` as for a gated item
 *   5 cheirality  for the candidates k = 0 .. 3 = (R1, t), (R2, t), (R1, -t), (R2, -t) and every point: the 4 x 4 matrix of OpenCV's
 *               triangulatePoints from P0 = [I | 0] and P = [R | t], rows x P0[2] - P0[0], y P0[2] - P0[1] with (x, y) = left, then
 *               x P[2] - P[0], y P[2] - P[1] with (x, y) = right; Q = its right singular vector of the smallest singular value;
 *               m = Q2 Q3 > 0; X = Q[0..2] / Q3, m &= X2 < max_depth; Y = R X + t, m &= Y2 > 0, m &= Y2 < max_depth; m &= the RANSAC mask.
 *               good[k] = the ones of m
 *   6 choice    the reference's chain (solve_5pts.cpp:152-181): k = 0 if good0 >= each of the others, else 1 if good1 >= each of the others,
 *               else 2 if good2 >= each of the others, else 3 -- ties go to the lower k.  R = the candidate's rotation, t its translation,
 *               mask = its m; inlier_cnt = good[chosen]; Rotation = R^T, Translation = -(R^T t); ok = inlier_cnt > min_inliers, else status
 *               UVS_RP_FEW_INLIERS
 * Kernels: k_rp_gate (a wavefront per item: step 1, step 2), k_ft_reject_run (step 3: the kernel of uvs_ft_reject, shared through
 * csrc/uvs_ft_reject_kernel.h; F and its mask stay on the device), k_rp_recover (a wavefront per item: the 3 x 3 SVD by one-sided Jacobi,
 * wave-uniform; lanes stride over the points, the four triangulations of a point in registers by Givens rotations and a one-sided Jacobi
 * SVD; the counts by ballots).  No CPU path: uvs_rp_create fails with UVS_ERR_NO_DEVICE without a GPU. */
#define UVS_RP_MAX_ITEMS 4096                 /* largest max_items uvs_rp_create takes; max_points up to UVS_FT_MAX_POINTS */
enum { UVS_RP_OK = 0, UVS_RP_FEW_CORRES = 1, UVS_RP_LOW_PARALLAX = 2, UVS_RP_FEW_POINTS = 3, UVS_RP_NO_MODEL = 4, UVS_RP_FEW_INLIERS = 5 };
typedef struct uvs_rp uvs_rp;                 /* opaque: device buffers, pinned staging, stream */

typedef struct uvs_rp_item {
    int32_t window;                    /* 0 .. n_windows - 1, non-decreasing over the items */
    int32_t frame_l;                   /* 0 .. UVS_WINDOW_SIZE - 1, strictly increasing within a window */
    int32_t n;                         /* correspondences, 0 .. max_points */
    int32_t reserved;
    uint64_t seed;                     /* of the item's RANSAC samples */
    const double *left;                /* [n][2] normalized points in frame_l, finite */
    const double *right;               /* [n][2] normalized points in the newest frame, finite */
} uvs_rp_item;

typedef struct uvs_rp_params {         /* uvs_rp_default_params: the reference's values */
    double focal_length;               /* 460     FOCAL_LENGTH */
    double min_parallax_px;            /* 30      average_parallax * FOCAL_LENGTH > 30 */
    double f_threshold;                /* 0.3 / 460 */
    double confidence;                 /* 0.99 */
    double max_depth;                  /* 50      recoverPose's dist */
    int32_t min_corres;                /* 20      corres.size() > 20 */
    int32_t min_ransac_points;         /* 15      corres.size() >= 15; at least 8 */
    int32_t min_inliers;               /* 12      inlier_cnt > 12 */
    int32_t reserved;
} uvs_rp_params;

typedef struct uvs_rp_item_result {
    int32_t status;                    /* UVS_RP_* */
    int32_t n;
    double average_parallax;
    uvs_ft_reject_result ransac;       /* of step 3 */
    int32_t good[4];
    int32_t chosen;                    /* 0 .. 3, -1 if the item did not get that far */
    int32_t inlier_cnt;
    int32_t ok;
    int32_t reserved;
    double R[9], t[3];                 /* as recoverPose returns them, row-major */
    double Rotation[9], Translation[3];/* as solveRelativeRT returns them: R^T, -(R^T t) */
} uvs_rp_item_result;

typedef struct uvs_rp_window_result {
    int32_t l;                         /* frame_l of the window's first item with ok, or -1 */
    int32_t reserved;
    double Rotation[9], Translation[3];/* of that item; 0 if none */
} uvs_rp_window_result;

/* UVS_ERR_INVALID_ARG: null out or a capacity < 1; UVS_ERR_CAPACITY: max_items > UVS_RP_MAX_ITEMS or max_points > UVS_FT_MAX_POINTS. */
int uvs_rp_create(int device, int max_items, int max_points, uvs_rp **out);
void uvs_rp_destroy(uvs_rp *rp);
const char *uvs_rp_last_error(const uvs_rp *rp);
void uvs_rp_default_params(uvs_rp_params *params);
/* One upload, the three kernels, one download.  mask[] is PACKED over the items in order: item i owns n_i bytes, the final recoverPose mask
 * (1 = the point passed every test of the chosen candidate).  item_results[n_items]; window_results[n_windows] (a window without items has
 * l = -1).  Every refusal is UVS_ERR_INVALID_ARG and happens before anything is launched: a null pointer (handle, items, params, mask, either
 * result array, or a point array behind a positive n), n_items outside 1 .. max_items, n_windows < 1, a window outside 0 .. n_windows - 1 or
 * decreasing, a frame_l outside 0 .. UVS_WINDOW_SIZE - 1 or not increasing within its window, n outside 0 .. max_points, a coordinate that
 * is not finite, a parameter that is not finite, focal_length, f_threshold or max_depth <= 0, confidence outside (0, 1), min_ransac_points
 * < 8, min_corres or min_inliers < 0.  A refused call changes nothing -- no output is written -- and the handle stays usable. */
int uvs_rp_relative_pose(uvs_rp *rp, int n_items, const uvs_rp_item *items, const uvs_rp_params *params, uint8_t *mask,
                         uvs_rp_item_result *item_results, int n_windows, uvs_rp_window_result *window_results);
/* HIP-event time of a part of the last successful call on the handle's stream, upload and download excluded (milliseconds):
 * part 0 k_rp_gate, 1 k_ft_reject_run, 2 k_rp_recover; any other part 0. */
double uvs_rp_last_device_ms(const uvs_rp *rp, int part);

#ifdef __cplusplus
}
#endif
#endif /* UVS_SOLVER_H */
