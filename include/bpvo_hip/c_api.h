/*
 * bpvo_hip — C ABI of the MI355X-native dense photometric alignment path.
 *
 * This is the drop-in boundary.  bpvo has no FFI
 * layer of its own; the seams this ABI replaces are cited per entry point as
 * `reference: <file>:<line>` (paths relative to the reference checkout).
 *
 * Conventions
 *   - every function returns an int status: 0 = ok, <0 = error (never throws).
 *     bpvo_hip_last_error() gives the message; the C++ facade (vo.hpp) maps a
 *     non-zero status to bpvo::Error like THROW_ERROR does (bpvo/utils.h:211-220).
 *   - matrices are ROW-MAJOR float arrays (K[9], T[16], H[36]).
 *   - host pointers unless a function name ends in `_device`.
 *   - images are contiguous row-major rows x cols, u8 image + f32 disparity, as
 *     VisualOdometry::addFrame takes them (bpvo/vo.h:71).  The caller keeps
 *     ownership; data is copied before the call returns (bpvo/vo_frame.cc:50-51).
 *   - per-point arrays handed back to the host use the REFERENCE layouts:
 *     channel-major `a[c*N + i]` (bpvo/template_data.cc:96-97,108,133),
 *     Jacobians `[C*N][6]`, valid flags uint16_t (bpvo/types.h:69-73).
 *   - one ctx per (host thread, device); calls on one ctx are serialised by the
 *     caller (the reference objects are not re-entrant either,
 *     bpvo/template_data.h:80,86).
 */
#ifndef BPVO_HIP_C_API_H
#define BPVO_HIP_C_API_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- enums: numeric values equal to the reference's (bpvo/types.h:127-169,418-441) */
enum { BPVO_LOSS_HUBER = 0x10, BPVO_LOSS_TUKEY = 0x11, BPVO_LOSS_L2 = 0x12,
       BPVO_LOSS_STUDENT_T = 0x13      /* an extension, no reference member: defined below */ };
/* ---- BPVO_LOSS_STUDENT_T = 0x13 (an extension, no reference member): the t-distribution weights of Kerl, Sturm and Cremers (ICRA 2013) with nu = 5
 * fixed, and a scale that is fitted to the residuals in the place of the MAD.  There is no new parameter, and bpvo_hip_params keeps its layout.
 * Let R be the multiset of residuals r[i][c] of the valid points of a workspace.  Valid flags and residuals are exactly those of bpvo_hip_get_valid /
 * bpvo_hip_get_residuals.  Let n = C * #valid and m = #{r in R : r != 0}.
 * Map.  T(s) = ((nu + 1) / n) * sum_R r^2 * s / (nu * s + r^2) for s > 0.  This form has no division by zero at r = 0.  T is increasing and concave;
 *   its slope at a fixed point is (nu + 1) * mean(a^2) < 1, with a = r^2 / (nu * s + r^2) and mean(a) = 1 / (nu + 1); so a positive fixed point s* is
 *   unique, and plain iteration converges to it monotonically from any s > 0.  It exists if and only if (nu + 1) * m > n, because
 *   T(s) / s -> (nu + 1) m / n as s -> 0.
 * Scale.  If n == 0, or (nu + 1) * m <= n, or the result is below 1e-6, then sigma = 1 (the reference's own answer to a vanishing scale,
 *   mestimator.cc:452-490); the delta stored with it is |1 - sigma_prev|, as the median stage stores it.  Otherwise sigma_k = sqrt(s_k) with
 *   s_{k+1} = T(s_k).  Start: s_0 = sigma_prev^2 when this level already holds an estimated scale; on the first linearisation of a level, or after
 *   reset_scale, s_0 = mean r^2.  Stop: the first k with |sigma_{k+1} - sigma_k| <= 1e-4 * sigma_k, or k + 1 = 64 (a termination guard).  The result
 *   is sigma_{k+1}.
 * Freeze.  If the first pass from sigma_prev already satisfies the stop rule, the scale is frozen for the rest of the level: it keeps sigma_prev bit
 *   for bit.  Otherwise the scale is sigma_{k+1} and the level goes on estimating it.  (The state machine is the one of the other losses: a frozen
 *   scale is what lets the fused frozen-scale reduction serve the late iterations.)
 * Arithmetic.  Terms are f32; the residuals are summed in tiles of a fixed number of points (a function of the point index alone, never of the launch
 *   shape, the batch or the place in the active set), each point's channels in channel order, in f64, and the tiles are combined in a fixed order in
 *   f64; the iteration and the stop rule are f64.  Consequently sigma is the same bits wherever the same workspace history is replayed.
 * Weight.  x = r * sigma_inv; w = 6.0f / (5.0f + x * x), in f32, the operations in that order; w in (0, 1.2].  goodPointThreshold keeps its meaning
 *   (w > thr): at the default 0.75 that is |x| < 1.73, where Tukey's is |x| < 1.71.
 * Covariance.  d(u) = psi'(u) = 6 * (5 - u^2) / (5 + u^2)^2 — negative beyond |u| = sqrt(5), as Tukey's is beyond its own bend; BPVO_COV_INDEFINITE
 *   covers that.
 * Paths.  Estimates with this loss run on the four-kernel chain (the persistent and team kernels are not built for it): single contexts, sequences,
 *   stereo sequences and rigs. */
enum { BPVO_VERB_ITERATION = 0x20, BPVO_VERB_FINAL = 0x21, BPVO_VERB_SILENT = 0x22, BPVO_VERB_DEBUG = 0x23 };
enum { BPVO_DESC_INTENSITY = 0x30, BPVO_DESC_INTENSITY_AND_GRADIENT = 0x31, BPVO_DESC_FIELDS_FIRST_ORDER = 0x32,
       BPVO_DESC_FIELDS_SECOND_ORDER = 0x33, BPVO_DESC_LATCH = 0x34, BPVO_DESC_CENTRAL_DIFFERENCE = 0x35, BPVO_DESC_LAPLACIAN = 0x36, BPVO_DESC_BITPLANES = 0x37 };
enum { BPVO_GRAD_CD3 = 0, BPVO_GRAD_CD5 = 1 };
enum { BPVO_INTERP_LINEAR = 0, BPVO_INTERP_COSINE = 1, BPVO_INTERP_CUBIC = 2, BPVO_INTERP_CUBIC_HERMITE = 3 };
enum { BPVO_STATUS_PARAMETER_TOL = 0x30, BPVO_STATUS_FUNCTION_TOL = 0x31, BPVO_STATUS_GRADIENT_TOL = 0x32,
       BPVO_STATUS_MAX_ITERATIONS = 0x33, BPVO_STATUS_SOLVER_ERROR = 0x34 };
enum { BPVO_KF_LARGE_TRANSLATION = 0x40, BPVO_KF_LARGE_ROTATION = 0x41, BPVO_KF_SMALL_FRAC_GOOD = 0x42,
       BPVO_KF_NO_KEYFRAMING = 0x43, BPVO_KF_FIRST_FRAME = 0x44 };

/* ---- error codes */
enum { BPVO_OK = 0, BPVO_ERR_INVALID_ARG = -1, BPVO_ERR_UNSUPPORTED = -2, BPVO_ERR_NO_DATA = -3,
       BPVO_ERR_NO_TEMPLATE = -4, BPVO_ERR_DEVICE = -5, BPVO_ERR_NO_DEVICE = -6 };

/* POD mirror of bpvo::AlgorithmParameters, same 35 fields in the same order
 * (reference: bpvo/types.h:171-413; defaults bpvo/types.cc:31-66). bool -> int. */
typedef struct bpvo_hip_params {
  int   numPyramidLevels;
  int   minImageDimensionForPyramid;
  float sigmaPriorToCensusTransform;
  float sigmaBitPlanes;
  float dfSigma1;
  float dfSigma2;
  int   latchNumBytes;
  int   latchRotationInvariance;
  int   latchHalfSsdSize;
  int   centralDifferenceRadius;
  float centralDifferenceSigmaBefore;
  float centralDifferenceSigmaAfter;
  int   laplacianKernelSize;
  int   maxIterations;
  float parameterTolerance;
  float functionTolerance;
  float gradientTolerance;
  int   relaxTolerancesForCoarseLevels;
  int   gradientEstimation;
  int   interp;
  int   lossFunction;
  int   descriptor;
  int   verbosity;
  float minTranslationMagToKeyFrame;
  float minRotationMagToKeyFrame;
  float maxFractionOfGoodPointsToKeyFrame;
  float goodPointThreshold;
  int   minNumPixelsForNonMaximaSuppression;
  int   nonMaxSuppRadius;
  int   minNumPixelsToWork;
  float minSaliency;
  float minValidDisparity;
  float maxValidDisparity;
  int   maxTestLevel;
  int   withNormalization;
} bpvo_hip_params;

/* reference: bpvo::OptimizerStatistics (bpvo/types.h:444-482; ctor bpvo/types.cc:306-310) */
typedef struct bpvo_hip_stats {
  int   numIterations;
  float finalError;
  float firstOrderOptimality;
  int   status;
} bpvo_hip_stats;

#define BPVO_HIP_MAX_LEVELS 8

/* reference: bpvo::Result (bpvo/types.h:489-563) minus the point cloud, which is
 * fetched separately with bpvo_hip_get_point_cloud when isKeyFrame && hasPointCloud */
typedef struct bpvo_hip_result {
  float pose[16];
  float covariance[36];                   /* never written by the reference: Identity (Q16) — unless option "pose_covariance" is set: then the
                                           * covariance of the estimate's pose, bpvo_hip_pose_covariance::covariance below */
  bpvo_hip_stats optimizerStatistics[BPVO_HIP_MAX_LEVELS];
  int   numLevels;
  int   isKeyFrame;
  int   keyFramingReason;
  int   hasPointCloud;
} bpvo_hip_result;

/* reference: bpvo::PointWithInfo, 32-byte record (bpvo/point_cloud.h:30-62) */
typedef struct bpvo_hip_point_with_info {
  float   xyzw[4];
  uint8_t rgba[4];
  float   weight;
  char    pad[8];
} bpvo_hip_point_with_info;

typedef struct bpvo_hip_ctx bpvo_hip_ctx;

/* Fill `p` with AlgorithmParameters() defaults (reference: bpvo/types.cc:31-66). */
void bpvo_hip_default_params(bpvo_hip_params* p);

/*
 * Create a context: the device-resident equivalent of
 * VisualOdometry::Impl's three VisualOdometryFrame objects + pose estimator
 * (reference: bpvo/vo.cc:97-115, bpvo/vo_frame.cc:13-29).
 *   n_frames   frame slots (each = image pyramid + disparity + descriptor pyramid + template pyramid)
 *   n_pairs    estimation workspaces (residuals, valid, weights, GN state); 1 for sequential VO,
 *              B for batches of independent frame pairs
 *   device     HIP device ordinal
 * numPyramidLevels <= 0 is resolved like bpvo/vo.cc:103-107.
 */
int bpvo_hip_create(bpvo_hip_ctx** out, const float K[9], float baseline, int rows, int cols,
                    const bpvo_hip_params* p, int device, int n_frames, int n_pairs);
void bpvo_hip_destroy(bpvo_hip_ctx* ctx);
const char* bpvo_hip_last_error(const bpvo_hip_ctx* ctx);   /* ctx may be NULL: last create error */
int bpvo_hip_num_levels(const bpvo_hip_ctx* ctx);
int bpvo_hip_num_channels(const bpvo_hip_ctx* ctx);
int bpvo_hip_level_size(const bpvo_hip_ctx* ctx, int level, int* rows, int* cols);

/* ---- VisualOdometryFrame (reference: bpvo/vo_frame.h:21-90) ------------------------------- */
/* setData: copy image+disparity, build image pyramid + descriptor pyramid
 * (reference: bpvo/vo_frame.cc:48-55 -> dense_descriptor_pyramid.cc:67-78, image_pyramid.cc:43-50). */
int bpvo_hip_frame_set_data(bpvo_hip_ctx* ctx, int slot, const uint8_t* image, const float* disparity);
int bpvo_hip_frame_set_data_device(bpvo_hip_ctx* ctx, int slot, const uint8_t* d_image, const float* d_disparity);
/* setTemplate: pixel selection, 3-D points, normalisation, pixels+gradients+Jacobians for levels
 * L-1..maxTestLevel (reference: bpvo/vo_frame.cc:61-93 -> bpvo/template_data.cc:37-142). */
int bpvo_hip_frame_set_template(bpvo_hip_ctx* ctx, int slot);
int bpvo_hip_frame_clear(bpvo_hip_ctx* ctx, int slot);                /* vo_frame.h:47 */
int bpvo_hip_frame_state(const bpvo_hip_ctx* ctx, int slot, int* has_data, int* has_template);

/* batched forms: `count` slots first_slot, first_slot+stride, ... ; inputs are `count` images /
 * disparities back to back.  One launch per stage covers all of them. */
int bpvo_hip_frames_set_data(bpvo_hip_ctx* ctx, int first_slot, int slot_stride, int count,
                             const uint8_t* images, const float* disparities, int on_device);
int bpvo_hip_frames_set_template(bpvo_hip_ctx* ctx, int first_slot, int slot_stride, int count);

/* accessors (parity surface) */
int bpvo_hip_get_image(bpvo_hip_ctx* ctx, int slot, int level, uint8_t* out);               /* image_pyramid.cc:43-50 */
int bpvo_hip_get_descriptor_channel(bpvo_hip_ctx* ctx, int slot, int level, int channel,
                                    float* out);                                         /* dense_descriptor.h getChannel */
int bpvo_hip_get_saliency(bpvo_hip_ctx* ctx, int slot, int level, float* out);               /* dense_descriptor.cc:92-100 */
int bpvo_hip_num_points(bpvo_hip_ctx* ctx, int slot, int level, int* n);                      /* template_data.h numPoints */
int bpvo_hip_get_points(bpvo_hip_ctx* ctx, int slot, int level, float* xyzw /*[N][4]*/);      /* template_data.h points */
int bpvo_hip_get_point_indices(bpvo_hip_ctx* ctx, int slot, int level, int* inds /*[N], y*W+x*/);
int bpvo_hip_get_pixels(bpvo_hip_ctx* ctx, int slot, int level, float* pixels /*[C*N]*/);     /* template_data.h pixels */
int bpvo_hip_get_jacobians(bpvo_hip_ctx* ctx, int slot, int level, float* J /*[C*N][6]*/);    /* template_data.h jacobians */
int bpvo_hip_get_normalization(bpvo_hip_ctx* ctx, int slot, int level, float T[16], float T_inv[16]); /* rigid_body_warp.h:62-71 */

/* ---- operator-level seam used by PoseEstimatorGN::linearize (reference: bpvo/pose_estimator_gn.h:70-81):
 * computeResiduals + estimateScale + ComputeWeights + LinearSystemBuilder::Run at pose T.
 * reset_scale != 0 resets the AutoScaleEstimator first (pose_estimator_base.h:287-293).
 * Outputs: H (6x6 row-major, symmetric), G, f_norm = sqrt(sum w v r^2), sigma, number of valid points. */
int bpvo_hip_linearize(bpvo_hip_ctx* ctx, int ws, int ref_slot, int cur_slot, int level, const float T[16],
                       int reset_scale, float H[36], float G[6], float* f_norm, float* sigma, int* num_valid);
/* The same seam with the robust scale GIVEN instead of estimated: computeResiduals at T, then MEstimator::ComputeWeights(r, sigma) and
 * LinearSystemBuilder::Run (bpvo/pose_estimator_gn.h:72,76-79 without :74).  The scale estimator of the workspace is left frozen at
 * sigma.  For comparing H, G and f_norm with a reference run at a pose where that run's sigma is known (its freeze history, Q6, is
 * not reproducible from the pose alone). */
int bpvo_hip_linearize_at_scale(bpvo_hip_ctx* ctx, int ws, int ref_slot, int cur_slot, int level, const float T[16],
                                float sigma, float H[36], float G[6], float* f_norm, int* num_valid);
int bpvo_hip_get_residuals(bpvo_hip_ctx* ctx, int ws, float* r /*[C*N]*/, size_t* n);
int bpvo_hip_get_valid(bpvo_hip_ctx* ctx, int ws, uint16_t* v /*[N]*/, size_t* n);
int bpvo_hip_get_weights(bpvo_hip_ctx* ctx, int ws, float* w /*[C*N]*/, size_t* n);          /* vo_pose_estimator.cc:95-99 */
int bpvo_hip_fraction_good(bpvo_hip_ctx* ctx, int ws, float threshold, float* frac);         /* vo_pose_estimator.cc:101-107 */

/* Selects how template points are warped and interpolated (both formulations exist in the reference):
 *   BPVO_WARP_PHOTO_ERROR_F64 (default) — the ACTIVE reference path: PhotoError "standard" branch, projection and bilinear
 *       interpolation in double, Floor(), invalid -> r = 0 (bpvo/photo_error.cc:336-459);
 *   BPVO_WARP_PROJECT_POINTS_F32 — the inactive all-float path (PHOTO_ERROR_OPT): projectPoints + interpolation
 *       coefficients + dot product (bpvo/project_points.cc:180-214, bpvo/photo_error.cc:82-214, bpvo/interp_util.h:49-71):
 *       (int) truncation, C = [(1-xf)(1-yf), xf(1-yf), (1-xf)yf, xf*yf] in its expanded form, invalid -> r = -I0;
 *   BPVO_WARP_DISPARITY_SPACE_F32 — DisparitySpaceWarp in the place of RigidBodyWarp (bpvo/disparity_space_warp.{h,cc}; the
 *       reference declares the class and its warp_traits but typedefs TemplateData::WarpType to RigidBodyWarp,
 *       bpvo/template_data.h:42, so no build of it runs this): template points (x - cx, y - cy, d, 1) (makePoint :31-34),
 *       H = G * T * G_inv (setPose :36), x = (H p)_0 / (H p)_3 + cx (operator() :66-71, all f32) followed by the
 *       interpolation of the projectPoints formulation, Jacobian rows of jacobian() (:40-64), no normalisation (:87-91),
 *       paramsToPose = TwistToMatrix (:79-84).  bpvo_hip_get_points then returns disparity-space points.
 * Switching to or from the disparity-space warp drops the templates (has_template = 0 on every slot; the frame data
 * stay): call it before bpvo_hip_frame_set_template / the first bpvo_hip_add_frame. */
enum { BPVO_WARP_PHOTO_ERROR_F64 = 0, BPVO_WARP_PROJECT_POINTS_F32 = 1, BPVO_WARP_DISPARITY_SPACE_F32 = 2 };
int bpvo_hip_set_warp_formulation(bpvo_hip_ctx* ctx, int mode);

/* ---- VisualOdometryPoseEstimator::estimatePose (reference: bpvo/vo_pose_estimator.cc:63-93):
 * coarse-to-fine PoseEstimatorGN::run (pose_estimator_base.h:324-407). stats[numLevels]. */
int bpvo_hip_estimate_pose(bpvo_hip_ctx* ctx, int ws, int ref_slot, int cur_slot, const float T_init[16],
                           float T_est[16], bpvo_hip_stats* stats);

/* The same estimate with one record per linearisation of the Gauss-Newton runs, in the order they happen (coarse to fine) — what the
 * reference prints per iteration at Verbosity kIteration (PoseEstimatorBase::run, bpvo/pose_estimator_base.h:231-247,373-393: iteration,
 * function value, first-order optimality, step size), with the pose of the linearisation and the system that was solved added:
 *   [0..15] T the linearisation was taken at (row-major)   [16..51] H   [52..57] G   [58] f_norm = sqrt(sum w v r^2)
 *   [59] robust scale sigma the weights used   [60] valid points   [61..66] dp solved from (H, G)   [67] pyramid level
 * Written on the device by the thread that runs the solve / pose update (gn_step, or the persistent single-pair kernel); the
 * estimate itself is the one bpvo_hip_estimate_pose gives, bit for bit.  *n_records = records written (may exceed max_records:
 * only the first max_records are copied). */
#define BPVO_HIP_TRACE_FLOATS 68
int bpvo_hip_estimate_pose_trace(bpvo_hip_ctx* ctx, int ws, int ref_slot, int cur_slot, const float T_init[16], float T_est[16],
                                 bpvo_hip_stats* stats, float* records /*[max_records][68]*/, int max_records, int* n_records);

/* ---- VisualOdometry (reference: bpvo/vo.h:42-100, bpvo/vo.cc:125-224). Uses frame slots 0..2 and
 * workspace 0 of the ctx (needs n_frames >= 3). */
int bpvo_hip_add_frame(bpvo_hip_ctx* ctx, const uint8_t* image, const float* disparity, bpvo_hip_result* result);
int bpvo_hip_vo_num_points_at_level(bpvo_hip_ctx* ctx, int level, int* n);                    /* vo.cc:226-238 */
int bpvo_hip_vo_points_at_level(bpvo_hip_ctx* ctx, int level, float* xyzw);                   /* vo.cc:240-248 */
int bpvo_hip_get_point_cloud(bpvo_hip_ctx* ctx, bpvo_hip_point_with_info* pts, size_t* n, float pose[16]); /* vo.cc:260-281 */
int bpvo_hip_trajectory_size(bpvo_hip_ctx* ctx, int* n);                                      /* trajectory.cc:42-50 */
int bpvo_hip_get_trajectory(bpvo_hip_ctx* ctx, float* poses /*[n][16]*/);

/* ---- many independent VisualOdometry sequences in one context (bpvo/vo.cc:125-224 per sequence).
 * Sequence s owns frame slots 3s, 3s+1, 3s+2 and workspace s: a ctx created with n_frames >= 3 S and n_pairs >= S serves
 * sequences 0 .. S-1.  A context serves either bpvo_hip_add_frame or these entry points, never both (BPVO_ERR_INVALID_ARG).
 * bpvo_hip_add_frames advances sequences seq[0 .. n-1] (distinct ids; NULL = 0 .. n-1) by one frame each: images[i] / disparities[i]
 * are the next frame of sequence seq[i], host memory (on_device = 0) or device memory (1), and results[i] is what bpvo_hip_add_frame
 * would return for that frame on a context of the sequence's own — bit for bit, point clouds and trajectories included.  Any subset of
 * the sequences in any order; every argument error, and every per-sequence error (an empty key-frame template: BPVO_ERR_NO_TEMPLATE,
 * template_data.cc:177), is reported before any sequence changes, with the sequence named in bpvo_hip_last_error. */
int bpvo_hip_add_frames(bpvo_hip_ctx* ctx, int n, const int* seq /*[n] distinct ids, NULL = 0..n-1*/,
                        const uint8_t* images /*[n][rows*cols]*/, const float* disparities /*[n][rows*cols]*/,
                        int on_device, bpvo_hip_result* results /*[n]*/);
int bpvo_hip_seq_capacity(const bpvo_hip_ctx* ctx, int* n_sequences);                                      /* min(n_frames / 3, n_pairs) */
int bpvo_hip_seq_reset(bpvo_hip_ctx* ctx, int seq);                       /* next frame of seq is a first frame again */
int bpvo_hip_seq_num_points_at_level(bpvo_hip_ctx* ctx, int seq, int level, int* n);                       /* vo.cc:226-238 */
int bpvo_hip_seq_get_point_cloud(bpvo_hip_ctx* ctx, int seq, bpvo_hip_point_with_info* pts, size_t* n, float pose[16]);  /* vo.cc:260-281 */
int bpvo_hip_seq_trajectory_size(bpvo_hip_ctx* ctx, int seq, int* n);                                      /* trajectory.cc:42-50 */
int bpvo_hip_seq_get_trajectory(bpvo_hip_ctx* ctx, int seq, float* poses /*[n][16]*/);

/* ---- per-sequence cameras: each sequence of bpvo_hip_add_frames with its own calibration and image size.
 * A sequence whose camera is the context's own runs exactly what it runs without one.  Frame i of a bpvo_hip_add_frames call then takes
 * rows_s x cols_s pixels of images / disparities, s = seq[i], the frames back to back in call order (all cameras of the context's size:
 * the [n][rows*cols] layout above).  Each sequence's results equal bit for bit those of a bpvo_hip_create context of its camera.
 * bpvo_hip_create_sequences: a context for n_sequences sequences (n_frames = 3 S, n_pairs = S); sequence s starts with camera cams[s].
 *   Its image size is the largest rows and the largest cols over the cameras; per pyramid level, its template capacity is the largest of
 *   the cameras' own (a camera whose level falls below minNumPixelsForNonMaximaSuppression keeps a dense capacity there).  The context's
 *   own camera, the one the single-context entry points use, is cams[0] grown to that size.  With numPyramidLevels <= 0 (automatic,
 *   vo.cc:101-105) every camera's own level count must equal the context's (BPVO_ERR_UNSUPPORTED otherwise).
 * bpvo_hip_seq_set_camera: only while the sequence holds no frame (fresh, or after bpvo_hip_seq_reset; BPVO_ERR_INVALID_ARG otherwise), not
 *   on a context that runs bpvo_hip_add_frame.  Both commit the context to bpvo_hip_add_frames (bpvo_hip_add_frame then refuses it).  The camera must fit the context's storage, which never grows: rows, cols and every level's
 *   template capacity within the context's (BPVO_ERR_UNSUPPORTED, with the level and both capacities in bpvo_hip_last_error).
 * Every camera is checked before anything changes: finite K, fx > 0, fy > 0, K[8] = 1, baseline > 0 (BPVO_ERR_INVALID_ARG), no pyramid
 * level under 8 pixels and the context's level count (BPVO_ERR_UNSUPPORTED). */
typedef struct bpvo_hip_camera {
  float K[9];
  float baseline;
  int rows, cols;
} bpvo_hip_camera;
int bpvo_hip_create_sequences(bpvo_hip_ctx** out, int n_sequences, const bpvo_hip_camera* cams /*[n_sequences]*/, const bpvo_hip_params* p,
                              int device);
int bpvo_hip_seq_set_camera(bpvo_hip_ctx* ctx, int seq, const bpvo_hip_camera* cam);
int bpvo_hip_seq_get_camera(const bpvo_hip_ctx* ctx, int seq, bpvo_hip_camera* cam);

/* ---- per-sequence algorithm parameters: each sequence of bpvo_hip_add_frames with its own bpvo_hip_params (a parameter sweep over one
 * dataset in one context).  results[i] of every bpvo_hip_add_frames / bpvo_hip_add_frames_stereo call equals, bit for bit, what
 * bpvo_hip_add_frame(_stereo) returns for that frame on a bpvo_hip_create context of the sequence's camera AND the sequence's parameters.
 * A sequence that was never given parameters has the context's; one whose parameters equal the context's runs exactly what it runs without.
 * A sequence may own: lossFunction, maxIterations, parameterTolerance, functionTolerance, gradientTolerance, minTranslationMagToKeyFrame,
 *   minRotationMagToKeyFrame, maxFractionOfGoodPointsToKeyFrame, goodPointThreshold, minSaliency, minValidDisparity, maxValidDisparity — and
 *   the fields the library stores but never reads (relaxTolerancesForCoarseLevels, minNumPixelsToWork, verbosity), returned as set.
 * Fixed by the context (they size its storage or instantiate its kernels) and therefore equal to its own: numPyramidLevels (after the
 *   automatic count is resolved), minImageDimensionForPyramid, descriptor and every descriptor parameter (the sigmas, the LATCH fields,
 *   centralDifference*, laplacianKernelSize), gradientEstimation, interp, withNormalization, nonMaxSuppRadius,
 *   minNumPixelsForNonMaximaSuppression, maxTestLevel.  A difference: BPVO_ERR_UNSUPPORTED, with the name of the first differing field and
 *   both values in bpvo_hip_last_error.  A value bpvo_hip_create refuses (an unknown lossFunction) is refused with bpvo_hip_create's code.
 * bpvo_hip_seq_set_params: only while the sequence holds no frame (fresh, or after bpvo_hip_seq_reset, which keeps the parameters;
 *   BPVO_ERR_INVALID_ARG otherwise), not on a context that runs bpvo_hip_add_frame; it commits the context to bpvo_hip_add_frames.  Every
 *   check comes before anything changes: after an error bpvo_hip_seq_get_params returns what it returned before. */
int bpvo_hip_seq_set_params(bpvo_hip_ctx* ctx, int seq, const bpvo_hip_params* p);
int bpvo_hip_seq_get_params(const bpvo_hip_ctx* ctx, int seq, bpvo_hip_params* p);

/* ---- Point budget: at most max_points[l] template points at level l, the most salient first.  AN EXTENSION: the reference has no such
 * member (its template size follows from minSaliency, the non-maximum suppression and the scene alone).  Off by default; nothing changes while
 * it is off or while a level's candidates fit its budget.
 * The rule, per frame and level with budget K > 0: cand = the pixels today's selection keeps (border, saliency >= minSaliency, the NMS test where
 * the level has one, the disparity gate), before the cut to a multiple of 16.  |cand| <= K: nothing changes.  Otherwise t = the K-th largest
 * saliency of cand (exact); every candidate with S > t stays, and of those with S == t the first K - #{S > t} in raster order.  The kept set
 * stays in raster order and is cut to a multiple of 16 as ever: N = min(K, capacity) & ~15.  When #{S >= t} == K the template is, bit for bit,
 * the one minSaliency = max(minSaliency, t) gives without a budget.
 * bpvo_hip_set_point_budget (an extension, no reference member): the context's budget — single frames, bpvo_hip_add_frame,
 *   bpvo_hip_frames_set_template, pair batches, and every sequence without a budget of its own.  max_points [n_levels], level 0 first; the levels
 *   beyond n_levels have none; 0 = no budget at that level.  Takes effect at the next template; existing templates are untouched.  A value of
 *   1 .. 15 (always an empty template) or below 0, or n_levels above the context's levels: BPVO_ERR_INVALID_ARG, the setting stays as it was.
 * bpvo_hip_get_point_budget (an extension, no reference member): the setting, max_points [BPVO_HIP_MAX_LEVELS]. */
int bpvo_hip_set_point_budget(bpvo_hip_ctx* ctx, const int* max_points /*[n_levels]*/, int n_levels);
int bpvo_hip_get_point_budget(const bpvo_hip_ctx* ctx, int* max_points /*[BPVO_HIP_MAX_LEVELS]*/);
/* bpvo_hip_seq_set_point_budget (an extension, no reference member): sequence seq's own budget in the place of the context's, for
 *   bpvo_hip_add_frames, bpvo_hip_add_frames_stereo and the members of rigs; n_levels = 0 returns the sequence to the context's budget.  It
 *   outlives bpvo_hip_seq_reset, as the sequence's parameters do.  Refusals as above, and for a sequence the context does not have.
 * bpvo_hip_seq_get_point_budget (an extension, no reference member): the budget the sequence's next template runs with, max_points
 *   [BPVO_HIP_MAX_LEVELS]; own (may be null): 1 if it is the sequence's own. */
int bpvo_hip_seq_set_point_budget(bpvo_hip_ctx* ctx, int seq, const int* max_points /*[n_levels]*/, int n_levels);
int bpvo_hip_seq_get_point_budget(const bpvo_hip_ctx* ctx, int seq, int* max_points /*[BPVO_HIP_MAX_LEVELS]*/, int* own);
/* bpvo_hip_get_selection_info (an extension, no reference member; a diagnostic, valid after set_template, synchronises): what the selection
 *   of the slot's template did at `level` — n_candidates = |cand|; threshold = t, or the frame's minSaliency when no budget was set or it did
 *   not bind; n_ties_kept = K - #{S > t}, the candidates with S == t that stayed (0 when the budget did not bind).  Outputs may be null. */
int bpvo_hip_get_selection_info(bpvo_hip_ctx* ctx, int slot, int level, int* n_candidates, float* threshold, int* n_ties_kept);

/* ---- Normalised intensity: a mode of the Intensity descriptor that survives exposure changes.  AN EXTENSION: the reference has no such member
 * (its Intensity descriptor is float(I) and stands or falls with brightness constancy).  Off by default; while it is off nothing changes, and
 * nothing is launched or allocated for it.  With the mode on, the descriptor plane of every pyramid level is computed on the device from THAT
 * level's u8 image I (n_px pixels) by the rule below (as code: bpvo_amd/csrc/intensity_norm_math.h), and everything downstream — saliency,
 * selection, point budget, templates, Gauss-Newton, scoring, covariance — reads the plane as it reads float(I).
 * radius == 0, whole image: h = the 256-bin histogram of I; med = the smallest v with sum_{u <= v} h[u] >= (n_px + 1) / 2 (integer division: the
 *   lower median); mad = the smallest k with #{|I - med| <= k} >= (n_px + 1) / 2, from the same histogram folded about med; m = max(mad, 1);
 *   c = 32.0 / (1.4826 * m) in f64; D(x) = (float) ((double) (I(x) - med) * c): a 256-entry table applied to the image.
 * radius R in 1 .. 15, local: the window of a pixel is [x - R, x + R] x [y - R, y + R] cut to the image, n pixels; S1 = sum I and S2 = sum I^2 over
 *   it, integers; X = n * I(x, y) - S1 (32 bits); V = n * S2 - S1^2 (64 bits); Vf = max(V, 4 * n * n) — a floor of two grey levels on the window's
 *   standard deviation, so that flat regions do not amplify noise; D = (float) (32.0 * (double) X / sqrt((double) Vf)), f64 product, square root
 *   and quotient each correctly rounded.  The same R at every level.
 * Units: both forms give 32 descriptor units per robust standard deviation (of the image, or of the window).  minSaliency and the tau of
 *   bpvo_hip_score_poses are in those units while the mode is on, not in grey levels.
 * Invariance: an exact affine map I' = a * I + b with a a power of two and no clipping leaves D unchanged bit for bit — in the local form wherever
 *   the floor binds in neither image.
 * bpvo_hip_set_intensity_normalization (an extension, no reference member): radius -1 off (the default), 0 whole image, 1 .. 15 local.  It is
 *   context-wide — it fixes what the stored planes mean — and covers every entry point that runs a data stage: single frames from host or device
 *   memory, bpvo_hip_add_frame, bpvo_hip_add_frames with per-sequence cameras, the stereo and raw-stereo entry points, rigs, bpvo_hip_batch_run
 *   with any number of lanes.  Allowed only while no frame slot of the context holds data or a template (and so no sequence or rig member holds
 *   frames: bpvo_hip_frame_clear, bpvo_hip_seq_reset and their like empty them): BPVO_ERR_INVALID_ARG otherwise.  Any other radius:
 *   BPVO_ERR_INVALID_ARG.  A context whose descriptor is not Intensity: BPVO_ERR_UNSUPPORTED.  After a refusal bpvo_hip_last_error names the
 *   cause and the setting is what it was.
 * bpvo_hip_get_intensity_normalization (an extension, no reference member): the setting. */
int bpvo_hip_set_intensity_normalization(bpvo_hip_ctx* ctx, int radius);
int bpvo_hip_get_intensity_normalization(const bpvo_hip_ctx* ctx, int* radius);

/* ---- batches of independent frame pairs (BASELINE.json config 5).
 * Pair p uses frame slots 2p (reference/template frame A) and 2p+1 (current frame B) and workspace p.
 * For each pair: A.setData, A.setTemplate, B.setData, estimatePose(A, B, Identity) -> poses[p].
 * images = [A0,B0,A1,B1,...] (2*n_pairs images), disparities likewise — B's disparity is never read: estimatePose uses the current
 * frame's descriptor only (bpvo/vo_pose_estimator.cc:63-93), so it is neither uploaded nor stored (40 % of the input bytes); the B slots
 * of a batch therefore cannot be turned into templates afterwards (bpvo_hip_frame_set_template: BPVO_ERR_NO_DATA).
 * stats = [n_pairs][numLevels].
 * A pyramid level of a pair whose template keeps no point does not fail the batch (the reference's computeResiduals throws there,
 * bpvo/template_data.cc:177, and so do the single-pair entry points: BPVO_ERR_NO_TEMPLATE): that level of that pair is skipped, its
 * statistics stay at the OptimizerStatistics() defaults {0, -1, -1, BPVO_STATUS_SOLVER_ERROR} and its pose passes through.
 * With two or more estimation lanes each lane runs its share of the pairs end to end on its own stream (frame stages queued one behind
 * the other): same results, bit for bit, as the three stages called one after the other. */
int bpvo_hip_batch_run(bpvo_hip_ctx* ctx, int n_pairs, const uint8_t* images, const float* disparities,
                       int on_device, float* poses /*[n_pairs][16]*/, bpvo_hip_stats* stats);
/* same, but only the estimatePose stage on already prepared slots */
int bpvo_hip_batch_estimate(bpvo_hip_ctx* ctx, int n_pairs, const float* T_init /*[n_pairs][16] or NULL=Identity*/,
                            float* poses, bpvo_hip_stats* stats);
/* device address of the packed result records of the last batch (32 floats per pair:
 * pose 3x4 row-major (12), twist-free pad, per-level numIterations (4..), status ...) for an RCCL gather. */
int bpvo_hip_batch_result_records_device(bpvo_hip_ctx* ctx, const float** d_records, int* floats_per_pair);
/* device-to-device copy of the first n_pairs records into caller-owned device memory (e.g. the tensor handed to
 * the RCCL gather), complete on return */
int bpvo_hip_batch_copy_records_device(bpvo_hip_ctx* ctx, float* d_dst, int n_pairs);

/* ---- stereo front-end.  reference: StereoAlgorithm (utils/stereo_algorithm.{h,cc}), BlockMatching branch:
 * cvFindStereoCorrespondenceBM with the state of utils/stereo_algorithm.cc:63-82, then disp16.convertTo(CV_32F, 1/16) (:98-111).
 * The matcher is OpenCV 2.4's (third party): restated, parity unpinned.  Invalid pixels carry minDisparity - 1 (getInvalidValue).
 * Two documented deviations where the original depends on memory layout: right-image window columns past the row end are read by
 * linear addressing, clamped at the end of the image; and for minDisparity > 0 the original's column loop runs past the end of the
 * row (its results there depend on the next row's bytes) — here and in the oracle that overrun is CUT at the last column, not
 * reproduced. */
enum { BPVO_STEREO_BLOCK_MATCHING = 0, BPVO_STEREO_SGM = 1, BPVO_STEREO_SGBM = 2 };
typedef struct bpvo_hip_stereo_params {
  int preFilterCap;          /* 31 */
  int SADWindowSize;         /* 15; odd, 5..21 on the device path */
  int minDisparity;          /* 0 */
  int numberOfDisparities;   /* no default in the reference ("must be provided"); multiple of 16, <= 256 */
  int textureThreshold;      /* 10 */
  int uniquenessRatio;       /* 15 */
  /* `StereoAlgorithm` of the reference's config file (utils/stereo_algorithm.cc:25-27,42,62): BPVO_STEREO_BLOCK_MATCHING (the default,
   * the fields above) or BPVO_STEREO_SGM — the in-tree semi-global matcher SgmStereo (utils/sgm.{h,cc}; conf/kitti_eval.cfg:27,
   * conf/kitti_stereo.cfg:5) with SgmStereo::Config below (defaults utils/sgm.cc:47-56 = utils/stereo_algorithm.cc:46-56); it reads
   * numberOfDisparities from the field above.  Invalid pixels carry 0.  Integer arithmetic restated line by line from the source,
   * which includes OpenCV and cannot be built in this image: parity unpinned, HIP = oracle bit for bit. */
  int    algorithm;
  int    sobelCapValue;            /* 15 (clamped to 15..127, made odd: utils/sgm.cc:225-226) */
  int    censusRadius;             /* 2; 1 or 2 */
  int    windowRadius;             /* 2 */
  int    smoothnessPenaltySmall;   /* 100 */
  int    smoothnessPenaltyLarge;   /* 1600 */
  int    consistencyThreshold;     /* 1 */
  int    reserved_;
  double disparityFactor;          /* 256.0 */
  double censusWeightFactor;       /* 1.0 / 6.0 */
  /* BPVO_STEREO_SGBM — `StereoAlgorithm = SGBM | SemiGlobalBlockMatching` (utils/stereo_algorithm.cc:25-40, run :113-121; selected by
   * conf/kitti_seq_0.cfg:6): cv::StereoSGBM of OpenCV 2.4 + its medianBlur(3) + filterSpeckles + convertTo(CV_32F, 1/16).  These are the
   * FIELDS OF cv::StereoSGBM; it also reads minDisparity, numberOfDisparities, SADWindowSize, preFilterCap and uniquenessRatio above.
   * The reference's constructor call passes nine positional arguments to a constructor of eleven, so its config keys land one slot off
   * (uniquenessRatio -> disp12MaxDiff, speckleWindowSize -> preFilterCap, speckleRange -> uniquenessRatio, (bool) fullDP -> speckleWindowSize):
   * bpvo_hip_stereo_params_sgbm_from_config fills the struct from the KEYS exactly like that call.  `<= 0 means` rules of
   * computeDisparitySGBM apply (SADWindowSize <= 0: 5, P1 <= 0: 2, P2 <= 0: 5 then max(P2, P1 + 1), disp12MaxDiff <= 0: 1, uniquenessRatio < 0:
   * 10, preFilterCap: max(cap, 15) | 1).  Invalid pixels carry minDisparity - 1.  OpenCV's source is absent from the reference tree:
   * restated, parity unpinned; the GPU tests hold the kernels to that restatement bit for bit.  Device path: single-pass mode (fullDP = 0: the only mode the
   * reference's call can reach), minDisparity >= 0, numberOfDisparities <= 256, window and penalties that keep the int16 buffers of the
   * original from wrapping (BPVO_ERR_UNSUPPORTED names the limit otherwise). */
  int    P1;                       /* 0 */
  int    P2;                       /* 0 */
  int    disp12MaxDiff;            /* 0 */
  int    speckleWindowSize;        /* 0 */
  int    speckleRange;             /* 0 */
  int    fullDP;                   /* 0 */
} bpvo_hip_stereo_params;
void bpvo_hip_default_stereo_params(bpvo_hip_stereo_params* p);
/* StereoAlgorithm::Impl's SGBM branch (utils/stereo_algorithm.cc:27-40): the struct the reference's constructor call produces from the config
 * KEYS minDisparity, numberOfDisparities, SADWindowSize (3), P1 (0), P2 (0), uniquenessRatio (0), speckleWindowSize (0), speckleRange (0),
 * fullDP (0) — defaults in brackets; algorithm = BPVO_STEREO_SGBM */
void bpvo_hip_stereo_params_sgbm_from_config(bpvo_hip_stereo_params* p, int minDisparity, int numberOfDisparities, int SADWindowSize, int P1, int P2,
                                             int uniquenessRatio, int speckleWindowSize, int speckleRange, int fullDP);
/* StereoAlgorithm::run for `count` rectified pairs of the ctx's image size ([count][rows*cols] u8 each, host or device) ->
 * f32 disparities [count][rows*cols] (host or device); sp->algorithm selects the matcher (the entry point keeps its name) */
int bpvo_hip_stereo_bm(bpvo_hip_ctx* ctx, int count, const uint8_t* left, const uint8_t* right, int on_device,
                       const bpvo_hip_stereo_params* sp, float* disparity, int disparity_on_device);
/* VisualOdometry::addFrame(left, StereoAlgorithm::run(left, right)): the disparity map stays on the device */
int bpvo_hip_add_frame_stereo(bpvo_hip_ctx* ctx, const uint8_t* left, const uint8_t* right, const bpvo_hip_stereo_params* sp,
                              bpvo_hip_result* result);
/* ---- the stereo front-end for many cameras (apps/vo_app.cc per camera: StereoAlgorithm::run on the rectified pair, then addFrame).
 * One sp serves a call; the frames are packed as for bpvo_hip_add_frames with per-sequence cameras: frame i has rows_i x cols_i pixels, the
 * left images back to back in call order, the right images likewise.  Every check — the parameters against every camera's size (SGM:
 * rows > windowRadius; block matching: SADWindowSize below rows and cols; SGBM: its own limits), the arguments, for
 * bpvo_hip_add_frames_stereo also every check of bpvo_hip_add_frames — comes before anything changes, with the sequence (for
 * bpvo_hip_stereo_frames: the frame's index) named in bpvo_hip_last_error where one is at fault; after an error every sequence goes on as
 * if the call had not been made.
 * Block matching runs all the frames of a call in one launch per stage whatever their sizes; SGM runs neighbouring frames of one size
 * together, option "stereo_frames_per_launch" at a time; SGBM runs frame after frame.  The maps do not depend on any of that.
 *
 * StereoAlgorithm::run for n rectified pairs of n cameras' sizes: pair i has cams[i].rows x cams[i].cols pixels, the left images back to
 * back in call order, the right images likewise, the f32 disparities likewise.  Only rows / cols of a camera are read.  Each map equals,
 * bit for bit, what bpvo_hip_stereo_bm returns on a bpvo_hip_create context of that size.  Every size must fit the context's
 * (rows <= ctx rows, cols <= ctx cols; BPVO_ERR_UNSUPPORTED). */
int bpvo_hip_stereo_frames(bpvo_hip_ctx* ctx, int n, const bpvo_hip_camera* cams /*[n]*/, const uint8_t* left, const uint8_t* right,
                           int on_device, const bpvo_hip_stereo_params* sp, float* disparity, int disparity_on_device);
/* bpvo_hip_add_frames fed by the stereo front-end: results[i] is what bpvo_hip_add_frame_stereo(left_i, right_i, sp) returns for that
 * frame on a bpvo_hip_create context of sequence seq[i]'s camera, bit for bit.  The disparities are computed on the device in each
 * camera's own geometry and stay there; left images from host memory are uploaded once.  A context may mix bpvo_hip_add_frames and
 * bpvo_hip_add_frames_stereo calls freely, also within one sequence. */
int bpvo_hip_add_frames_stereo(bpvo_hip_ctx* ctx, int n, const int* seq /*[n] distinct ids, NULL = 0..n-1*/, const uint8_t* left,
                               const uint8_t* right, int on_device, const bpvo_hip_stereo_params* sp, bpvo_hip_result* results /*[n]*/);

/* ---- rectification on the device (an extension: the reference expects rectified input and uses cv::remap only to warp descriptors,
 * bpvo/photo_error.cc:60).  Raw — distorted, unrectified — 8-bit images go in; on the device they become rectified images of a camera of
 * the context, bit for bit what the integer rule below gives (bpvo_amd/csrc/rectify_math.h states it as code), and the raw entry points hand
 * them to the stereo front-end and the VO driver without a visit to the host.
 *
 * THE MAP.  A camera side (0 left, 1 right) has a map with one entry per destination pixel: the source coordinates (x, y) in the raw image,
 * in f64, as xq = (int32) nearbyint(x * 32.0) and yq likewise (1/32 pixel, ties to even).  A coordinate that is not finite, or with
 * |x * 32| >= 2^20, makes the entry "outside": the pixel is stored as 0.  The map is built on the host by a set call and uploaded once.
 *   The lens map (bpvo_hip_lens): Brown-Conrady with the coefficients dist = k1 k2 p1 p2 k3 k4 k5 k6, the raw intrinsics fx fy cx cy, the
 *   rotation R (row-major) from the raw camera to the rectified camera.  The new intrinsics fx' fy' cx' cy' are the camera's K (K[0], K[4],
 *   K[2], K[5]) widened to f64.  For the integer destination (u, v), in f64, one operation per statement in this order, no fused multiply-add:
 *     a = (u - cx') / fx'          b = (v - cy') / fy'
 *     X = (R00 a + R10 b) + R20    Y = (R01 a + R11 b) + R21    W = (R02 a + R12 b) + R22        (R^T (a, b, 1): no matrix inverse)
 *     x = X / W    y = Y / W    x2 = x x    y2 = y y    r2 = x2 + y2    xy = x y
 *     rad = (1 + ((k3 r2 + k2) r2 + k1) r2) / (1 + ((k6 r2 + k5) r2 + k4) r2)
 *     xd = (x rad + (2 p1) xy) + p2 (r2 + 2 x2)        yd = (y rad + p1 (r2 + 2 y2)) + (2 p2) xy
 *     xs = fx xd + cx              ys = fy yd + cy
 *   The caller's maps (the _maps calls): two f32 arrays mapx, mapy of the camera's size, as cv::initUndistortRectifyMap or any fisheye model
 *   gives them; each value is widened to f64 and quantised by the same rule.
 * THE PIXEL.  With ix = xq >> 5 (arithmetic shift), fx = xq & 31, iy and fy likewise, the taps are p(iy + dy, ix + dx), dy, dx in {0, 1}; a tap
 * outside [0, raw_rows) x [0, raw_cols) reads 0 (cv::remap's BORDER_CONSTANT); then
 *     out = ((32 - fy) ((32 - fx) p00 + fx p01) + fy ((32 - fx) p10 + fx p11) + 512) >> 10
 * in plain integer arithmetic.  This is NOT OpenCV's fixed-point table (weights rounded to 1/32768): parity with cv::remap is unpinned —
 * OpenCV is not part of the reference tree.  A destination pixel is OUTSIDE if its entry is "outside" or a tap with a non-zero weight lies
 * outside the raw image; the info calls count them.
 *
 * bpvo_hip_seq_set_rectification(_maps): the map of sequence seq's side, for the sequence's camera as it is now.  bpvo_hip_seq_set_camera
 * clears the sequence's rectification (the destination size and K' may have changed); bpvo_hip_seq_clear_rectification does so on request.
 * bpvo_hip_set_rectification(_maps) / bpvo_hip_clear_rectification / bpvo_hip_rectification_info: the same for the context's own camera, which
 * bpvo_hip_add_frame_stereo_raw reads.  Errors, every check before anything changes:
 *   a raw call or an info call on a sequence or side without a rectification                                            BPVO_ERR_NO_DATA
 *   lens values that are not finite; fx or fy <= 0; max |R^T R - I| > 1e-6; a raw size under 2; a NULL pointer; a bad side   BPVO_ERR_INVALID_ARG
 *   a raw size above 32767; a camera with skew (K[1] != 0)                                                              BPVO_ERR_UNSUPPORTED
 * A set call that replaces a map waits for the context's stream first.  Maps, raw staging and tables are acquired at their first use: a
 * context that never rectifies holds nothing of them. */
typedef struct bpvo_hip_lens {
  double fx, fy, cx, cy;           /* the raw camera's intrinsics */
  double dist[8];                  /* k1 k2 p1 p2 k3 k4 k5 k6 */
  double R[9];                     /* raw camera -> rectified camera, row-major */
  int raw_rows, raw_cols;          /* the raw image: 2 .. 32767 each */
} bpvo_hip_lens;
int bpvo_hip_seq_set_rectification(bpvo_hip_ctx* ctx, int seq, int side /*0 left, 1 right*/, const bpvo_hip_lens* lens);
int bpvo_hip_seq_set_rectification_maps(bpvo_hip_ctx* ctx, int seq, int side, int raw_rows, int raw_cols, const float* mapx /*[rows*cols] of the camera*/,
                                        const float* mapy);
int bpvo_hip_seq_clear_rectification(bpvo_hip_ctx* ctx, int seq);
int bpvo_hip_seq_rectification_info(bpvo_hip_ctx* ctx, int seq, int side, int* raw_rows, int* raw_cols, uint64_t* outside_pixels /*each may be NULL*/);
int bpvo_hip_set_rectification(bpvo_hip_ctx* ctx, int side, const bpvo_hip_lens* lens);
int bpvo_hip_set_rectification_maps(bpvo_hip_ctx* ctx, int side, int raw_rows, int raw_cols, const float* mapx, const float* mapy);
int bpvo_hip_clear_rectification(bpvo_hip_ctx* ctx);
int bpvo_hip_rectification_info(bpvo_hip_ctx* ctx, int side, int* raw_rows, int* raw_cols, uint64_t* outside_pixels);
/* n raw frames of one side -> n rectified frames, ONE launch whatever the frames' sizes.  Frame i is a raw image of raw_rows x raw_cols of
 * seq[i]'s side (seq NULL: n frames of the context's own camera), the raw frames back to back in call order (host or device); the outputs lie
 * back to back in the cameras' sizes (host or device) — the packing of bpvo_hip_add_frames_stereo.  A sequence may appear more than once.
 * Returns with the outputs in place.  Rigs are served by composition: this call with device output for each side, bpvo_hip_stereo_frames with
 * device output, then bpvo_hip_add_frames_rig(s) with device input. */
int bpvo_hip_rectify_frames(bpvo_hip_ctx* ctx, int n, const int* seq /*[n] or NULL*/, int side, const uint8_t* raw, int on_device, uint8_t* out,
                            int out_on_device);
/* bpvo_hip_add_frames_stereo / bpvo_hip_add_frame_stereo from raw pairs: both sides of every frame are rectified by one launch into the stereo
 * front-end's own image buffers, which the front-end and the frame stages then read where they lie — no host synchronisation and no copy in
 * between; raw images from host memory are uploaded once.  The results are, bit for bit, those of the rectified entry point fed the images the
 * rule above gives.  Every check of the rectified entry point, and a rectification of both sides of every sequence of the call
 * (BPVO_ERR_NO_DATA, the sequence named in bpvo_hip_last_error), come before anything changes. */
int bpvo_hip_add_frames_stereo_raw(bpvo_hip_ctx* ctx, int n, const int* seq /*[n] distinct ids, NULL = 0..n-1*/, const uint8_t* left_raw,
                                   const uint8_t* right_raw, int on_device, const bpvo_hip_stereo_params* sp, bpvo_hip_result* results /*[n]*/);
int bpvo_hip_add_frame_stereo_raw(bpvo_hip_ctx* ctx, const uint8_t* left_raw, const uint8_t* right_raw, const bpvo_hip_stereo_params* sp,
                                  bpvo_hip_result* result);
/* the rectification launches of the context so far and the destination pixels they made (the kernel has no class in
 * bpvo_hip_get_kernel_stats: this is its counter) */
int bpvo_hip_rectify_counts(bpvo_hip_ctx* ctx, uint64_t* launches, uint64_t* pixels);

/* ---- rig mode: the cameras of a rigid rig estimated as ONE 6-DoF body pose, from all cameras' residuals at once.
 * Twists are ordered (omega, v).  The body pose T maps key-frame body coordinates to current body coordinates (the role T plays for one
 * camera).  Member p has the extrinsic X_p, camera_from_body (x_cam = X_p x_body; rigid), and runs at the pose T_p = X_p T X_p^-1 (f64,
 * narrowed to f32).  Its linearisation at T_p gives (H_p, G_p) in its Hartley-normalised twist xi — its update would be
 * T_p <- T_p N_p^-1 exp(-xi) N_p with N_p = [sI, -s c; 0 1] —; with the body update T <- T exp(-zeta) that twist is xi = B_p zeta,
 *     B_p = A_p^-1 Ad(X_p),   A_p^-1 = [[I, 0], [-s [c]x, sI]]  (A_p = [[I, 0], [[c]x, I/s]]; without normalisation A_p = I),   Ad(X) = [[R, 0], [[t]x R, R]],
 * and the joint system is H = sum_p B_p^T H_p B_p, G = sum_p B_p^T G_p, f = sqrt(sum_p f_p^2), valid = sum_p valid_p (member order, f64,
 * narrowed to f32 once).  H zeta = G is solved and T <- T twist_to_matrix(-zeta) applied per iteration, with the convergence tests, iteration
 * limits and statistics of a single camera's run; every member keeps its own robust scale.  bpvo_hip_linearize_rig returns exactly this system.
 * The ESTIMATE takes the same Gauss-Newton steps in a normalised parametrisation, because the f32 solve wants one (a camera's plain-twist H has
 * a condition number of 2e4 where its normalised H has 30): it iterates on the pose T_0 of the reference member (member 0) in that member's
 * normalised twist xi_0 = B_0 zeta, so that member p's map is B_p B_0^-1 = A_p^-1 Ad(X_p X_0^-1) A_0 (the identity for p = 0), the convergence
 * tests read (xi_0, f, |G|_inf) of that system, and the body pose is X_0^-1 T_0 X_0 at the end.  A rig of ONE camera therefore takes that
 * camera's own steps: its body pose is X^-1 T_p X of bpvo_hip_estimate_pose's T_p, to the rounding of the conjugation.  Per iteration the members
 * run the four-kernel chain, then one wavefront takes the rig's step; the persistent and team kernels do not serve rig estimates.
 * BPVO_WARP_DISPARITY_SPACE_F32: BPVO_ERR_UNSUPPORTED.  An extrinsic that is not finite, whose last row is not (0, 0, 0, 1) or with
 * max |R^T R - I| > 1e-4, n < 1 or above the capacity, an id twice: BPVO_ERR_INVALID_ARG.  Every check comes before anything changes.
 *
 * Estimator level, stateless like bpvo_hip_estimate_pose: member i = workspace wss[i] (distinct), template refs[i], current frame curs[i],
 * extrinsic X + 16 i.  bpvo_hip_linearize_rig: the joint system at the body pose T_body at one pyramid level (reset_scale as
 * bpvo_hip_linearize's, for every member); T_members, if not NULL, receives the member poses the kernels were run at. */
int bpvo_hip_linearize_rig(bpvo_hip_ctx* ctx, int n, const int* wss, const int* refs, const int* curs, const float* X /*[n][16]*/, int level,
                           const float T_body[16], int reset_scale, float H[36], float G[6], float* f_norm, int* num_valid,
                           float* T_members /*[n][16] or NULL*/);
/* the coarse-to-fine estimate of the body pose from T_init; stats [numLevels] are the joint system's (finalError = f,
 * firstOrderOptimality = |G|_inf).  A member whose template is empty at a level that runs: BPVO_ERR_NO_TEMPLATE. */
int bpvo_hip_estimate_pose_rig(bpvo_hip_ctx* ctx, int n, const int* wss, const int* refs, const int* curs, const float* X /*[n][16]*/,
                               const float T_init[16], float T_est[16], bpvo_hip_stats* stats /*[numLevels]*/);
/* addFrame level.  bpvo_hip_rig_set declares the rig: member p is sequence seq[p] (NULL: 0 .. n-1) of bpvo_hip_add_frames' kind — its own
 * camera (bpvo_hip_create_sequences, bpvo_hip_seq_set_camera) — with extrinsic X + 16 p; only while every named sequence holds no frame.
 * A member with parameters of its own (bpvo_hip_seq_set_params): BPVO_ERR_INVALID_ARG, the rig runs the context's.  A context that
 * declares a rig serves bpvo_hip_add_frames_rig only: bpvo_hip_add_frame, bpvo_hip_add_frames and bpvo_hip_add_frames_stereo return
 * BPVO_ERR_INVALID_ARG. */
int bpvo_hip_rig_set(bpvo_hip_ctx* ctx, int n, const int* seq /*[n] distinct ids, NULL = 0..n-1*/, const float* X /*[n][16]*/);
int bpvo_hip_rig_get(const bpvo_hip_ctx* ctx, int* n, int* seq /*[n] or NULL*/, float* X /*[n][16] or NULL*/);
/* VisualOdometry::addFrame of the rig: the members' frames packed as for bpvo_hip_add_frames, in member order, each in its camera's size.
 * One estimate of the body pose (from the body's pose against the key frame; against a new key frame from the identity), ONE key-frame
 * decision — the context's thresholds on the body pose, the fraction of good points pooled over the members, sum good_p / sum n_p C — and
 * every member the same transition.  `result` is the body's (covariance: Identity, or with option "pose_covariance" the body pose's).  At a key frame every member's point cloud and point
 * counts come from the bpvo_hip_seq_* accessors; a cloud's pose is W_kf X_p^-1 (world_from_camera), W_kf the body trajectory's pose of the
 * result that carries the cloud.  After an error the rig goes on as if the call had not been made. */
int bpvo_hip_add_frames_rig(bpvo_hip_ctx* ctx, const uint8_t* images, const float* disparities, int on_device, bpvo_hip_result* result);
int bpvo_hip_rig_trajectory_size(bpvo_hip_ctx* ctx, int* n);
int bpvo_hip_rig_get_trajectory(bpvo_hip_ctx* ctx, float* poses /*[n][16]: the body's trajectory*/);
/* ---- several rigs in one context, each with its own parameters.  bpvo_hip_rigs_set declares n_rigs rigs over DISJOINT sets of the context's
 * sequences: rig r has count[r] members, the members of all rigs back to back in seq (NULL: 0, 1, 2, ...) and X, rig after rig; every matrix and
 * rule is the rig section's above, per rig.  It replaces every rig declared before (only while all their members are fresh), and every rig
 * starts with the context's parameters.  A sequence in two rigs or twice in one, a sequence with parameters of its own
 * (bpvo_hip_seq_set_params), a membership change on a sequence that holds frames, an extrinsic that is not rigid, n_rigs or a count < 1 or
 * above the sequence capacity: BPVO_ERR_INVALID_ARG, nothing changed.  bpvo_hip_rigs_set with n_rigs = 1 and bpvo_hip_rig_set declare the same
 * rig: the one-rig calls (bpvo_hip_rig_get, bpvo_hip_add_frames_rig, bpvo_hip_rig_trajectory_*, bpvo_hip_rig_pose_covariance) are the plural
 * calls on rig 0; on a context of SEVERAL rigs they return BPVO_ERR_INVALID_ARG and name the plural call. */
int bpvo_hip_rigs_set(bpvo_hip_ctx* ctx, int n_rigs, const int* count /*[n_rigs]*/, const int* seq /*[sum count] distinct ids, NULL = 0..*/,
                      const float* X /*[sum count][16]*/);
int bpvo_hip_rigs_get(const bpvo_hip_ctx* ctx, int* n_rigs, int* count /*[n_rigs] or NULL*/, int* seq /*[sum count] or NULL*/,
                      float* X /*[sum count][16] or NULL*/);
/* One rig, one parameter set: the fields bpvo_hip_seq_set_params accepts — the Gauss-Newton limits and tolerances, the loss, the key-frame
 * thresholds, goodPointThreshold, minSaliency and the disparity gate — for the rig's body and all its members; anything else must equal the
 * context's (BPVO_ERR_UNSUPPORTED, the field named in the error string).  Only while the rig's members hold no frame.  Rigs of different losses
 * in one call run one estimate per loss present. */
int bpvo_hip_rigs_set_params(bpvo_hip_ctx* ctx, int rig, const bpvo_hip_params* p);
int bpvo_hip_rigs_get_params(const bpvo_hip_ctx* ctx, int rig, bpvo_hip_params* p);
/* bpvo_hip_add_frames_rig for n of the declared rigs in one call: rigs[i] (distinct; NULL: 0 .. n-1; any subset, any order) names the rig of
 * results[i]; the frames of all their members back to back, rig after rig in call order, in member order inside a rig, each in its camera's
 * size.  One data stage, ONE estimate of all body poses (the members of every rig share each launch of the four-kernel chain, one launch of the
 * batched rig step per iteration takes every rig's step), one count of good points, per rig its own key-frame decision — its own thresholds on
 * its own body pose, the fraction pooled over its own members —, one estimate for the rigs that estimate again.  Rigs at their first frame take
 * part in the data and template stages only; rigs the call does not name are not touched.  Every rig's results, trajectory, point counts and
 * clouds are bit for bit those of the same rig alone in a context of its own with the rig's parameters as the context's.  A rig named twice,
 * a rig id out of range, BPVO_WARP_DISPARITY_SPACE_F32 (BPVO_ERR_UNSUPPORTED), a member with parameters of its own: refused before anything
 * is queued; after an error the rigs go on as if the call had not been made. */
int bpvo_hip_add_frames_rigs(bpvo_hip_ctx* ctx, int n, const int* rigs /*[n] distinct ids, NULL = 0..n-1*/, const uint8_t* images,
                             const float* disparities, int on_device, bpvo_hip_result* results /*[n]*/);
int bpvo_hip_rigs_trajectory_size(bpvo_hip_ctx* ctx, int rig, int* n);
int bpvo_hip_rigs_get_trajectory(bpvo_hip_ctx* ctx, int rig, float* poses /*[n][16]: the body's trajectory*/);
/* bpvo_hip_estimate_pose_rig for n_rigs rigs in one estimate (stateless): rig r has count[r] members, back to back in wss / refs / curs / X; no
 * workspace in two rigs; T_init / T_est [n_rigs][16] the body poses, stats [n_rigs][numLevels] or NULL.  Every rig's result is bit for bit
 * that of bpvo_hip_estimate_pose_rig on it alone. */
int bpvo_hip_estimate_pose_rigs(bpvo_hip_ctx* ctx, int n_rigs, const int* count /*[n_rigs]*/, const int* wss, const int* refs, const int* curs,
                                const float* X /*[sum count][16]*/, const float* T_init /*[n_rigs][16]*/, float* T_est /*[n_rigs][16]*/,
                                bpvo_hip_stats* stats /*[n_rigs][numLevels] or NULL*/);

/* ---- pose covariance: a robust "sandwich" estimate of the uncertainty of an estimated pose (the reference has none: its Result::covariance is
 * never written, Q16).
 * Definition.  Take the pose T^ of a finished estimate at the finest pyramid level the estimate ran (maxTestLevel) and sigma, the robust scale
 * that level ended with (kL2 ignores it).  With u = r / sigma, w(u) the library's M-estimator weight, v_p the valid flag of template point p — AND the
 * point in front of the camera at T^ (z > 0, f32): the warp's own rule has no such test, a point behind the camera that projects into the image
 * is valid for the estimate as it is in the reference, but it says nothing about the pose's uncertainty; num_valid counts the v_p of this rule — and
 * J_pc the 1x6 Jacobian row of point p, channel c in the level's Hartley-normalised twist (the J of bpvo_hip_get_jacobians):
 *   curvature         M = sum_p v_p sum_c d(u_pc) J_pc^T J_pc,  d = psi':  kL2 d = 1;  Huber d = 1 where |u| <= 1.345 (exactly where w = 1), else 0;
 *                     Tukey, q = (u / 4.685)^2: d = (1 - q)(1 - 5 q) where |u| < 4.685, else 0;
 *                     Student-t (BPVO_LOSS_STUDENT_T): d = 6 (5 - u^2) / (5 + u^2)^2
 *   score covariance  Q = sum_p v_p g_p^T g_p,  g_p = sum_c w(u_pc) r_pc J_pc — the channels of a point are ONE cluster (they see the same pixel
 *                     neighbourhood); sum_p g_p is the G of bpvo_hip_linearize_at_scale at the same pose and scale
 *   Sigma_xi = M^-1 Q M^-1 — no sigma^2 factor, no finite-sample factor —, and in the plain twist Sigma = A Sigma_xi A^T with
 *   A = [[I, 0], [[c]x, I/s]] for the level's normalisation (s, c): the identity without normalisation and for BPVO_WARP_DISPARITY_SPACE_F32.
 * Sigma is the covariance of eps in T_true = T^ twist_to_matrix(eps), twist ordered (omega, v): the parametrisation of the library's own update.
 * Rig: M_b = sum_p B_p^T M_p B_p, Q_b = sum_p B_p^T Q_p B_p with B_p = A_p^-1 Ad(X_p) (bpvo_hip_linearize_rig's map), members in order, and
 * Sigma_b = M_b^-1 Q_b M_b^-1 is the covariance of the body pose in the plain body twist.  One camera is the rig of one member with X = I.
 * The per-tile sums are f32 (the reduction's tiles and wave tree) and combined in tile order in f64 into each camera's M_p and Q_p, which are kept
 * as f32 like H and G of a linearisation (bpvo_hip_debug_pose_covariance_sums returns exactly them); everything behind that is f64 — the maps, the
 * congruences, an LDL^T of the curvature, two solves, the upper triangle mirrored — and the result is narrowed to f32 once.
 * Limits.  The estimate treats the template points as independent clusters.  For the intensity descriptor it is calibrated: over 150 noise draws
 * the empirical standard deviation of the pose is 1.07 - 1.13 times the reported one, under every loss.  For bit-planes it is OPTIMISTIC by a
 * factor of 1.7 - 2.3 in standard deviation (census 3x3 and the 5x5 blur correlate neighbouring points, which no per-point form can see):
 * INTEGRATION.md section 4, profiles/pose_covariance_calibration.json.  It is the uncertainty of the alignment given the template, not of the
 * template's depth.
 * status: BPVO_COV_OK; BPVO_COV_INDEFINITE — the LDL^T of the curvature met a pivot <= 0 (Tukey or Student-t away from a minimum); BPVO_COV_DEGENERATE — fewer
 * than 6 valid points in total, or a sum that is not finite; BPVO_COV_NONE — nothing was estimated (a first frame, a batch pair whose finest level
 * was skipped).  Anything but OK leaves `covariance` at the Identity.  No status is an error return, and no pose raises. */
enum { BPVO_COV_OK = 0, BPVO_COV_INDEFINITE = 1, BPVO_COV_DEGENERATE = 2, BPVO_COV_NONE = 3 };
#define BPVO_HIP_COV_GROUP 64      /* workspaces that go through the pass together (its scratch holds this many finest-level templates) */
typedef struct bpvo_hip_pose_covariance {
  float T[16];              /* the pose the covariance belongs to (a rig: the body pose) */
  float covariance[36];     /* row-major, exactly symmetric */
  float sigma;              /* the robust scale the weights were taken with (a rig: member 0's) */
  int   num_valid;          /* valid template points (a rig: over all members) */
  int   level;
  int   status;             /* BPVO_COV_* */
} bpvo_hip_pose_covariance;
/* Stateless, like bpvo_hip_linearize_at_scale: record i for workspace wss[i] (distinct), template refs[i], current frame curs[i] at pyramid
 * level `level`.  T [n][16] and sigma [n] both given: at those poses and scales.  Both NULL: each workspace's LAST ESTIMATE — its final pose, the
 * scale and the level it ended with, read on the device (`level` is ignored; BPVO_ERR_NO_DATA if a workspace holds no estimate, e.g. after a
 * bpvo_hip_linearize on it) — which is how the covariances of a bpvo_hip_batch_run / bpvo_hip_batch_estimate are asked for.  The pass recomputes
 * the residuals at the pose into scratch of its own (allocated at the first call, for BPVO_HIP_COV_GROUP workspaces; larger calls run in groups):
 * the workspaces' residuals, weights, Gauss-Newton states and every measurement counter stay as they were.
 * A context of more than 48 channels: BPVO_ERR_UNSUPPORTED. */
int bpvo_hip_pose_covariances(bpvo_hip_ctx* ctx, int n, const int* wss, const int* refs, const int* curs, int level, const float* T /*[n][16] or NULL*/,
                              const float* sigma /*[n] or NULL*/, bpvo_hip_pose_covariance* out /*[n]*/);
/* The rig's: ONE record for the body pose from members (wss[i], refs[i], curs[i], X + 16 i) as in bpvo_hip_linearize_rig.  T_body and sigma [n]
 * (every member's own scale) both given, or both NULL = the last bpvo_hip_estimate_pose_rig of exactly these members. */
int bpvo_hip_pose_covariance_rig(bpvo_hip_ctx* ctx, int n, const int* wss, const int* refs, const int* curs, const float* X /*[n][16]*/, int level,
                                 const float* T_body /*[16] or NULL*/, const float* sigma /*[n] or NULL*/, bpvo_hip_pose_covariance* out);
/* The record of the last frame of bpvo_hip_add_frame / of sequence seq of bpvo_hip_add_frames / of bpvo_hip_add_frames_rig with option
 * "pose_covariance" set (status BPVO_COV_NONE otherwise, and for a first frame).  T is the pose of the estimate the result's pose comes from
 * AGAINST ITS KEY FRAME — at a key frame with re-estimation the re-estimate's —, not the frame-to-frame `pose` of the result. */
int bpvo_hip_vo_pose_covariance(bpvo_hip_ctx* ctx, bpvo_hip_pose_covariance* out);
int bpvo_hip_seq_pose_covariance(bpvo_hip_ctx* ctx, int seq, bpvo_hip_pose_covariance* out);
int bpvo_hip_rig_pose_covariance(bpvo_hip_ctx* ctx, bpvo_hip_pose_covariance* out);
int bpvo_hip_rigs_pose_covariance(bpvo_hip_ctx* ctx, int rig, bpvo_hip_pose_covariance* out);      /* rig `rig` of bpvo_hip_add_frames_rigs */
/* diagnostics: the curvature M and the score covariance Q (row-major, symmetric) of the last pass on workspace ws, in its normalised twist */
int bpvo_hip_debug_pose_covariance_sums(bpvo_hip_ctx* ctx, int ws, float M[36], float Q[36]);

/* ---- pose scoring: the robust cost of MANY candidate poses of a pair in one launch (the reference has none).  Gauss-Newton converges only
 * inside the basin of its start; a caller with a handful of plausible starts — a constant-velocity prediction, an IMU guess, Identity, a grid
 * for relocalisation — scores them here and starts at the best (bpvo_hip_estimate_pose_best_start).
 * Definition.  Template (ref_slot, level) of N points and C channels, the current frame's descriptor at that level, a pose T meant as in
 * bpvo_hip_linearize, a truncation tau (finite, > 0).  valid_i and r[i][c] are exactly what bpvo_hip_linearize at T leaves in
 * bpvo_hip_get_valid / bpvo_hip_get_residuals (the context's warp formulation, the same f32 bits).  Then
 *   n_valid  = #{i : valid_i}
 *   n_below  = #{(i, c) : valid_i and |r[i][c]| < tau}
 *   cost_sum = sum over valid i and all c of min(|r[i][c]|, tau), every term converted to f64 and summed in f64
 *   score    = (cost_sum + tau C (N - n_valid)) / (C N): an invalid point is charged tau per channel, so a pose that throws the scene out of
 *              view cannot win by having nothing to explain.  N = 0: cost_sum 0, both counts 0, score = tau.
 * Residuals of invalid points never enter (the f32 formulations' -I0 is ignored).  A pose that is NaN, Inf or beyond the int range makes every
 * point invalid (the warp's rule); no pose raises.  cost_sum is the same bits from call to call and does not depend on how many poses or pairs
 * share the launch nor on a pose's place in the list: no floating-point atomics, one partial per (pose, 256-point chunk), combined in chunk order.
 * tau is in DESCRIPTOR units: about 0.5 for bit-planes (channels in [0, 1]), about 30 grey levels for intensity.
 * Known limit.  The charge for invalid points favours poses that keep the scene in view: when the true motion moves a third of the template out of
 * the image (measured: |t| = 2.5 m on the 240x320 plane scene, 2 626 of 3 856 points still in view), Identity can outscore a start next to the
 * truth.  The score ranks starts; it is no estimate.
 * Served: kLinear interpolation, the three warp formulations, descriptors of at most 48 channels.  Another interpolation, or a descriptor of more
 * than 48 channels (LATCH of 8+ bytes, CentralDifference radius 4+): BPVO_ERR_UNSUPPORTED, the message says which.
 * The calls read the template, the descriptor and the geometry; they touch no workspace: residuals, weights, tap cache, robust scale, Gauss-Newton
 * state and every measurement counter stay as they were.  Device buffers for poses, partials and results belong to the context and grow on demand.
 * ref_slot without a template: BPVO_ERR_NO_TEMPLATE; cur_slot without data: BPVO_ERR_NO_DATA; level outside [maxTestLevel, numLevels), n_poses < 1
 * (or above 1 048 576), n_pairs < 1 (or above 65 535), tau not finite or <= 0, a NULL pointer: BPVO_ERR_INVALID_ARG. */
typedef struct bpvo_hip_pose_score {
  double cost_sum;
  double score;
  int    n_valid;
  int    n_below;
} bpvo_hip_pose_score;      /* 24 bytes */
int bpvo_hip_score_poses(bpvo_hip_ctx* ctx, int ref_slot, int cur_slot, int level, int n_poses, const float* T /*[n_poses][16]*/, float tau,
                         bpvo_hip_pose_score* out /*[n_poses]*/);
/* ... of n_pairs pairs (refs[i], curs[i]) in ONE launch, n_poses poses each; the pairs may have cameras and sizes of their own
 * (bpvo_hip_create_sequences).  Pair i's records are bit for bit those of bpvo_hip_score_poses on it alone. */
int bpvo_hip_score_poses_pairs(bpvo_hip_ctx* ctx, int n_pairs, const int* refs, const int* curs, int level, int n_poses,
                               const float* T /*[n_pairs][n_poses][16]*/, float tau, bpvo_hip_pose_score* out /*[n_pairs][n_poses]*/);
/* Scores the n_cands candidate starts at score_level (< 0: the coarsest level), takes the lowest score (ties: the lowest index; a NaN score never
 * wins) and runs bpvo_hip_estimate_pose on workspace ws with that candidate as T_init: T_est and stats are bit for bit those of
 * bpvo_hip_estimate_pose(T_init = T_cands + 16 * chosen).  chosen and scores [n_cands] may be NULL. */
int bpvo_hip_estimate_pose_best_start(bpvo_hip_ctx* ctx, int ws, int ref_slot, int cur_slot, int n_cands, const float* T_cands /*[n_cands][16]*/,
                                      int score_level, float tau, float T_est[16], bpvo_hip_stats* stats /*[numLevels] or NULL*/, int* chosen,
                                      bpvo_hip_pose_score* scores);

/* ---- start policy: where the addFrame drivers begin Gauss-Newton (an extension, off by default: it replaces no reference member).  The reference
 * starts every estimate at T_kf, the pose accumulated since the key frame, and a key frame's re-estimate at the Identity (bpvo/vo.cc:144-145,184-186): a
 * start that is wrong by one whole inter-frame motion.  A policy lets bpvo_hip_add_frame(_stereo), bpvo_hip_add_frames(_stereo) and
 * bpvo_hip_add_frames_rig(s) start at the body's own last motion, at a caller's hint, or at the best-scoring of them (bpvo_hip_score_poses).
 * The rule (stated once, bpvo_amd/csrc/vo_state.h).  A call makes up to two estimates: which = 0 against the key frame the call began with, base
 * B = T_kf; which = 1 against the new key frame, base B = Identity.  M is the `pose` of the body's last Result (f32; Identity after creation,
 * after bpvo_hip_seq_reset and after a first frame).  A candidate c starts the estimate at c B (the host's f32 4x4 product, index-order sums);
 * for which = 1 it is c itself, and the candidate Identity is B itself, no product.
 *   mode BPVO_START_KEYFRAME_POSE (0, the default, the reference): the one candidate Identity — today's start, bit for bit, no launch added
 *   mode BPVO_START_CONSTANT_VELOCITY (1): the pending hint if there is one, else M; nothing is scored, no launch is added
 *   mode BPVO_START_SCORED (2): Identity (kind 0), M (kind 1), M M (kind 2), then the pending hints (kind 3), scored at score_level (-1: the
 *     coarsest) with truncation tau (descriptor units, finite and > 0: no default is guessed); the lowest score starts the estimate, ties go to
 *     the first — the reference's start —, a NaN never wins.  One more launch pair and one host round trip per estimate; in the batched
 *     drivers one per distinct (score_level, tau) among the entries that estimate.  A rig scores member p at its member pose of the body
 *     candidate and pools like its fraction of good points: (sum_p cost_sum_p + tau sum_p C (N_p - n_valid_p)) / sum_p C N_p, in f64, member order.
 * Hints: at most BPVO_HIP_MAX_START_HINTS rigid 4x4 frame-to-frame guesses in Result::pose's convention (an IMU or odometry prediction), stored
 * by the setter, used by both estimates of the body's next call that estimates, then dropped (bpvo_hip_seq_reset drops them too).
 * A policy outlives bpvo_hip_seq_reset, like parameters and budgets; it may change while the body holds frames and takes effect at the next call.
 * Refusals, each leaving the earlier setting in place: mode outside 0 .. 2, a mode-2 tau that is not finite and positive, score_level other than
 * -1 or within [maxTestLevel, numLevels), a hint that is not rigid and finite, more than 13 hints (mode 1: more than one; mode 0: any), a policy or
 * hints for a sequence that is a member of a rig: BPVO_ERR_INVALID_ARG; mode 2 on a context pose scoring does not serve: BPVO_ERR_UNSUPPORTED. */
#define BPVO_HIP_MAX_START_CANDIDATES 16
#define BPVO_HIP_MAX_START_HINTS 13
enum { BPVO_START_KEYFRAME_POSE = 0, BPVO_START_CONSTANT_VELOCITY = 1, BPVO_START_SCORED = 2 };
typedef struct bpvo_hip_start_policy { int mode; int score_level; float tau; } bpvo_hip_start_policy;
/* What estimate `which` of the body's last call started from: n_candidates = 0 when that estimate did not run; kind[k] as above; chosen: the
 * candidate it started at, T_start its pose (a rig: the body's); scores[k]: the candidates' records — zeroed in modes 0 and 1, which list their
 * one candidate; for a rig score is the pooled score and cost_sum, n_valid, n_below are the members' sums. */
typedef struct bpvo_hip_start_info {
  int   n_candidates;
  int   chosen;
  int   kind[BPVO_HIP_MAX_START_CANDIDATES];
  float T_start[16];
  bpvo_hip_pose_score scores[BPVO_HIP_MAX_START_CANDIDATES];
} bpvo_hip_start_info;      /* 520 bytes */
/* bpvo_hip_set_start_policy / bpvo_hip_get_start_policy (an extension, no reference member): the context's policy — bpvo_hip_add_frame, and every
 * sequence and rig without one of its own. */
int bpvo_hip_set_start_policy(bpvo_hip_ctx* ctx, const bpvo_hip_start_policy* policy);
int bpvo_hip_get_start_policy(const bpvo_hip_ctx* ctx, bpvo_hip_start_policy* policy);
/* bpvo_hip_seq_set_start_policy / bpvo_hip_seq_get_start_policy (an extension, no reference member): sequence seq's own policy in the place of the
 * context's (policy NULL: back to the context's); the getter returns the policy its next call runs with, own (may be NULL): 1 if it is its own. */
int bpvo_hip_seq_set_start_policy(bpvo_hip_ctx* ctx, int seq, const bpvo_hip_start_policy* policy);
int bpvo_hip_seq_get_start_policy(const bpvo_hip_ctx* ctx, int seq, bpvo_hip_start_policy* policy, int* own);
/* bpvo_hip_rigs_set_start_policy / bpvo_hip_rigs_get_start_policy (an extension, no reference member): the same for the body of rig `rig`. */
int bpvo_hip_rigs_set_start_policy(bpvo_hip_ctx* ctx, int rig, const bpvo_hip_start_policy* policy);
int bpvo_hip_rigs_get_start_policy(const bpvo_hip_ctx* ctx, int rig, bpvo_hip_start_policy* policy, int* own);
/* bpvo_hip_vo_set_start_hints / bpvo_hip_seq_set_start_hints / bpvo_hip_rigs_set_start_hints (extensions, no reference member): the pending hints
 * of bpvo_hip_add_frame's state / of sequence seq / of rig `rig` (body poses); n = 0 drops them; a new call replaces the earlier hints. */
int bpvo_hip_vo_set_start_hints(bpvo_hip_ctx* ctx, int n, const float* M /*[n][16]*/);
int bpvo_hip_seq_set_start_hints(bpvo_hip_ctx* ctx, int seq, int n, const float* M /*[n][16]*/);
int bpvo_hip_rigs_set_start_hints(bpvo_hip_ctx* ctx, int rig, int n, const float* M /*[n][16]*/);
/* bpvo_hip_vo_start_info / bpvo_hip_seq_start_info / bpvo_hip_rigs_start_info (extensions, no reference member): the record of estimate which
 * (0 or 1) of the last bpvo_hip_add_frame / of sequence seq's / of rig `rig`'s last call. */
int bpvo_hip_vo_start_info(bpvo_hip_ctx* ctx, int which, bpvo_hip_start_info* out);
int bpvo_hip_seq_start_info(bpvo_hip_ctx* ctx, int seq, int which, bpvo_hip_start_info* out);
int bpvo_hip_rigs_start_info(bpvo_hip_ctx* ctx, int rig, int which, bpvo_hip_start_info* out);

/* Pyramid levels that were run by the persistent single-launch Gauss-Newton kernel (groups of BPVO_HIP_PERSIST_MAX_WS or fewer
 * pairs) since the context was created, and whether such a launch ever gave up at a grid barrier (the
 * context then stays on the four-kernel chain; results are the same either way). */
int bpvo_hip_persistent_counts(bpvo_hip_ctx* ctx, uint64_t* levels, int* gave_up);

/* Upload pipeline of the last bpvo_hip_batch_run that was handed HOST buffers (batches of at least 32 pairs): wall time from the start of
 * the call until the last chunk had landed on the device, and the bytes that crossed the bus (both images, the template frame's
 * disparity).  The uploads run under the compute of the chunks before them. */
int bpvo_hip_upload_stats(bpvo_hip_ctx* ctx, double* seconds, uint64_t* bytes);

/* Batch estimates that ran their whole Gauss-Newton stage in one launch of the team-persistent kernel (batches of 2 ..
 * BPVO_HIP_TEAM_MAX_PAIRS pairs) since the context was created. */
int bpvo_hip_team_counts(bpvo_hip_ctx* ctx, uint64_t* launches);

/* ---- measurement hooks (bench.py): per-kernel HIP-event timing on the ctx's own stream */
typedef struct bpvo_hip_kernel_stat {
  char     name[48];
  uint64_t launches;
  double   total_ms;          /* sum of HIP-event durations */
  double   units;             /* units processed (points or pixels), summed over launches */
  double   bytes_per_unit;    /* algorithmic bytes per unit */
} bpvo_hip_kernel_stat;
/* 0 off; 1: HIP events around the frame stages and around every 5th warp_residual launch of a batch estimate (the
 * reported units are scaled to the sampled launches); 2: around every launch of every kernel; 3: as 1, but around EVERY
 * warp_residual and EVERY irls_reduce launch (the averages are then over the same launches as a rocprofv3 kernel trace's).
 * Resets the counters. */
int bpvo_hip_profiling(bpvo_hip_ctx* ctx, int enable);
int bpvo_hip_get_kernel_stats(bpvo_hip_ctx* ctx, bpvo_hip_kernel_stat* out, int max_out, int* n_out);
int bpvo_hip_total_linearizations(bpvo_hip_ctx* ctx, uint64_t* n);  /* GN iterations done since create/reset */
/* exact median selections served by the bracketed path / by the full 3-pass path since the last counter reset */
int bpvo_hip_median_path_counts(bpvo_hip_ctx* ctx, uint64_t* bracketed, uint64_t* full);
/* BPVO_LOSS_STUDENT_T since the last counter reset: runs of the scale stage (linearisations whose scale was not frozen) and the passes of the
 * iteration over them.  The median-path counts above do not move for such workspaces, and the tap-cache counts (which the median stage folds in
 * from its bracket counters) are not kept for them. */
int bpvo_hip_tscale_counts(bpvo_hip_ctx* ctx, uint64_t* stages, uint64_t* passes);
/* points linearised since the last counter reset: `fused` of `total` went through the fused residual + reduction path that
 * irls_reduce takes once a workspace's robust scale is frozen for the level (warp_residual skips those workspaces) */
int bpvo_hip_fused_point_counts(bpvo_hip_ctx* ctx, uint64_t* fused, uint64_t* total);
/* tap cache of warp_residual since the last counter reset: out[0] hits, out[1] lookups (= valid points), out[2] / out[3] the same over
 * the first 8 linearisations of every level (the moving-pose regime) */
int bpvo_hip_tap_cache_counts(bpvo_hip_ctx* ctx, uint64_t out[4]);
/* ---- per-context options: how the library schedules its work.  None of them changes a result (every setting is covered by a
 * bit-identity test) — with ONE exception, the validation mode "reference_reduction" at the end of the table, which changes the summation
 * order of the normal equations to the reference's own, and a second one, "pose_covariance", which changes the covariance field of the
 * results and nothing else; they exist so that a caller — not the process environment — decides, per context.  Call between API calls, from the
 * thread that drives the context.  Unknown key or value out of range: BPVO_ERR_INVALID_ARG (bpvo_hip_last_error names the key).
 *
 *   key                      default   meaning
 *   "lanes"                  3 / 2     (8-channel / single-channel descriptors) estimation lanes (HIP streams driven by host threads) a pair batch fans out over, 1 .. 8 (at least 8
 *                                      pairs per lane).  The narrow per-pair kernels of one lane overlap the chip-filling kernels of another;
 *                                      per-launch timings are only clean with 1.  A context is created with up to two; more are allocated by this option
 *                                      or by the first batch that fans out over them (host-buffer batches stay on their two-lane upload plan).
 *   "persistent"             1         single pairs (estimatePose, addFrame) run every pyramid level in ONE persistent launch; 0: the
 *                                      four-kernel chain.  Also the master switch of "team".
 *   "persist_max_ws"         1         groups of up to this many pairs take the persistent kernel (1 .. 8; more than 1 measured slower)
 *   "persist_grid"           64        workgroups of the persistent kernel (one per CU)
 *   "persist_max_points"     32768 / 65536  (8 channels / 1) a pyramid level with more template points than this, and the finer levels behind it, take the
 *                                      four-kernel chain even for a single pair: dense templates (no non-maximum suppression: conf/tsukuba.cfg) are
 *                                      bandwidth work for the whole chip, not latency work for 64 workgroups (same bits either way)
 *   "dense_candidates_from"  32768     chain launches over a pyramid level with at least this many template points keep the candidates of
 *                                      the exact median in one contiguous run per workspace instead of one segment per 256-point chunk: the
 *                                      selection reads four totals and one array (a 300 k-point level: 10 us instead of 120); same median
 *   "persist_timeout_ticks"  5e7       100 MHz ticks a device-side barrier waits before the launch gives up and the call falls back to
 *                                      the chain (0.5 s; the tests of that path set 1)
 *   "team"                   1         batches of 2 .. team_max_pairs pairs run their whole Gauss-Newton stage in one team-persistent launch
 *   "team_max_pairs"         128       ... up to this many pairs; above "team_full_pairs" (80) only when CUs / pairs workgroups per pair fill at least
 *                                      95 % of the CUs (128 pairs on 256 CUs do, 96 do not: the chain is faster there)
 *   "team_full_pairs"        80        batches of up to this many pairs take the team kernel whatever the fill of the chip (see "team_max_pairs", "team_spares")
 *   "team_size"              0         workgroups per team; 0 = CUs / pairs, at most an eighth of the CUs (32 of 256: larger teams were slower at 2 - 7 pairs)
 *   "team_cus"               (device)  CUs the team kernel may claim (tests: fewer teams than pairs)
 *   "team_local_barriers"    1         teams whose workgroups all run on one XCD (checked on the device) skip the L2 write-back of their barriers
 *   "team_join"              2         workgroups of a team that has run out of pairs join the teams still at work (a batch ends with its slowest
 *                                      pair: + 7 % at 128 pairs): 0 never, 1 teams on the workgroup's own XCD only, 2 any team; same bits either way
 *   "team_join_from_pairs"   48        smaller batches (few, large teams: little to balance) run the team kernel with teams of fixed size
 *   "team_spares"            1         the growing form's grid fills the chip: workgroups beyond pairs x (CUs / pairs) start without a team and join one
 *                                      (96 pairs: 2 x 96 + 64 spares, + 4 %; 112: + 6 %) — with it every batch of up to team_max_pairs pairs takes the team kernel
 *   "team_joins_seen"        (counter) workgroups that joined another team so far (set: resets it)
 *   "normalization_side_stream" 1      a frame stage that runs alone on the context's stream (single frames, batches on one lane) queues the
 *                                      Hartley normalisation sums on a stream of its own, next to template_build, and joins them before it returns
 *   "vo_disparity_late"      1         bpvo_hip_add_frame uploads the disparity of a host frame — which only a later template stage reads — once the
 *                                      estimate is queued: the copy from pageable memory holds the host for 90 us (640x480), which then lie under the
 *                                      Gauss-Newton kernels — where the estimate is the persistent kernel's launch per level, queued in one go (0, and on
 *                                      the chain, whose rounds the host paces: in the data stage)
 *   "stereo_frames_per_launch" 0       SGM frames of one size that go through every kernel of the matcher in one launch (each on its own slice of the
 *                                      scratch): 0 = as many as fit a third of the device memory that was free when the scratch was first needed, 1 = one
 *                                      frame after the other, k = at most k.  Same maps.
 *   "stereo_frames_per_launch_seen" (read-only) the frames per launch the last SGM call used
 *   "stereo_free_mib_seen"   (read-only) the free device memory, MiB, the rule above saw when this context first needed the SGM scratch
 *   "rectify_last_kernel_ms" (read-only) the duration, ms, of the last rectification launch between two events on the context's stream; -1 unless
 *                                      bpvo_hip_profiling was on when it was queued (measurement: scripts/rectify_bench.py)
 *   "fusion_last_splat_ms"   (read-only) the duration, ms, of the last disparity-fusion stage's splat launch between two events on the context's stream
 *   "fusion_last_update_ms"  (read-only) ... and of its update launch; -1 unless bpvo_hip_profiling was on when the stage was queued (measurement:
 *                                      scripts/disparity_fusion_bench.py); a stage that runs motion stereo has its launch between the two, inside the
 *                                      splat's figure
 *   "variance_last_kernel_ms" (read-only) the duration, ms, of the last measurement-variance launch between two events on the context's stream; -1 unless
 *                                      bpvo_hip_profiling was on when it was queued (measurement: scripts/disparity_variance_bench.py)
 *   "motion_stereo_last_kernel_ms" (read-only) the duration, ms, of the last motion-stereo launch between two events on the context's stream; -1 unless
 *                                      bpvo_hip_profiling was on when it was queued (measurement: scripts/motion_stereo_bench.py)
 *   "normalization_form"     4         the sequential (reference-order) Hartley sums: 1 = hand-scheduled DPP add chains (170 us for a 1241x376 template,
 *                                      2.28 ms for a dense 640x480 one); 0 = the compiler's DPP form (281 us / 3.6 ms); 2 = every lane of a row reads the same
 *                                      four consecutive elements from LDS and adds them with plain adds — no cross-lane traffic, no asm (311 us / 4.0 ms);
 *                                      3 = those reads with the adds as asm blocks of back-to-back plain adds on a wave that does nothing else (170 us /
 *                                      2.04 ms, 118 registers); 4 = 3 for launches of at most 1024 workgroups, 1 for larger ones.  Same sums bit for bit:
 *                                      tests/test_gpu_parity.py runs the four against each other
 *   "normalization_deferred" 1         ... and inside bpvo_hip_batch_run on one lane (not the team kernel), and where addFrame re-estimates against a new key
 *                                      frame, only the coarsest level's sums are joined: the others run on under the Gauss-Newton iterations of the levels
 *                                      above them (the finest level's on a stream of its own), the estimation waits for them level by level
 *   "team_split_max_pairs"   4         ... and team batches of up to this many pairs run the coarsest level of every pair in a launch of its own, the
 *                                      deferred sums under it, the other levels in a second launch behind them (2 / 4 pairs + 1.2 / + 1.5 %; from 8 pairs on the
 *                                      launch boundary — every pair waits for the slowest — costs 4 - 7 %: DESIGN.md 7; 0: one launch, sums joined first)
 *   "levels_in_one_launch_max_frames" 8  frame stages of at most this many frames run ALL levels of the pyramid (three pyrDown steps per launch), of
 *                                      the bit-planes, of the tiled selection and of the template build in one launch each (a single pair: 33 -> 14 launches)
 *   "small_batch_fused"      1         contexts of a few pairs: job table + initial poses in one launch, states copied out by the record-packing launch
 *   "fuse_frozen"            1         residuals recomputed inside the reduction once a workspace's robust scale is frozen (C = 8)
 *   "step_in_reduce_max_pairs" 128     groups (the pairs of one lane) of up to this many pairs: the Gauss-Newton step is taken by the last tile of a pair
 *                                      inside the reduction launch — three kernels per iteration instead of four, same bits (0: never)
 *   "stagger"                1         lanes run their pairs end to end (frame stage of one lane under the estimation of another) ...
 *   "stagger_min_pairs"      192       ... for batches of at least this many pairs (smaller ones: the frame stage of all pairs first, then the lanes)
 *   "tapcache_max_density"   0.5       pyramid levels with more template points per pixel than this gather straight from the descriptor
 *   "upload_workers"         6         host threads that stage a HOST-buffer batch in pinned chunks (0: plain copies)
 *   "upload_plan_first"      0.19      fractions of a host batch in the first (lane 0) and second (lane 1) group of the upload plan;
 *   "upload_plan_second"     0.50      first = 0: two equal groups
 *   "lazy_template_descriptor" 1       bpvo_hip_batch_run keeps, for the TEMPLATE frame (A) of every pair, census bytes + channel 0 instead of the
 *                                      32-byte descriptor records at the pyramid levels with non-maximum suppression (bit-planes, CD3 gradients):
 *                                      one pixel in ~18 is a template point there, template_build forms the records of its stencils from the census
 *                                      bytes (same operations, same bits).  The accessors and a later estimate with such a slot as the CURRENT frame
 *                                      rebuild the records on demand.
 *   "lazy_template_saliency" 1         needs lazy_template_descriptor = 1 (without it the option does nothing).  1: at those levels (NMS radius 1) the
 *                                      template frames of bpvo_hip_batch_run keep the census bytes ONLY: a census launch writes them, the bit-planes
 *                                      kernel runs over the few tile columns that stay dense, the tiled selection forms channel 0 of its windows from
 *                                      the census bytes (same operations, same bits) and does not store the saliency map.  bpvo_hip_get_saliency
 *                                      forms the map on demand from the slot's data — the same bytes — and fails with BPVO_ERR_NO_DATA once that data
 *                                      has been replaced (frame_set_data on the slot, the next batch) before a new template was made of it.
 *   "points_from_compact_stream" 0     debug: bpvo_hip_get_points returns the points as the Gauss-Newton kernels rebuild them from the 8-byte records
 *                                      they stream ({Z or d, x | y << 16}: DESIGN.md 3) instead of the stored (X, Y, Z, 1) — the same bits
 *   "reference_reduction"    0         VALIDATION MODE (the one option that changes numbers).  1: H, G and the squared residual norm of every
 *                                      linearisation are accumulated exactly as the reference's default (serial, WITH_TBB OFF) build does —
 *                                      f32, in index order over the channel-major arrays, w' = w * float(valid), (w' J_a) J_b, (w' r) J, (w' r) r,
 *                                      one multiply and one add per slot (bpvo/linear_system_builder.cc:140-205,239-266) — by one wavefront per
 *                                      pair (kernels_gn_ref.hip): an estimate takes 30 - 50 x as long (scripts/reference_mode_cost.py).  Every iterate, the final pose,
 *                                      numIterations and status of every level then equal the reference path's BIT FOR BIT
 *                                      (tests/test_gpu_reference_order.py, the conf/ sequences, the goldens, a 330-case randomised run).  The
 *                                      default (0) regroups the same sums (rank-2 form, FMA, wave tree, f64 block combine): H, G, f within
 *                                      4e-6 of an f64 evaluation, poses within 1e-4 rad / 1e-3 m, iteration counts inside the reference's own
 *                                      spread between its serial and its TBB build.  In this mode every estimate takes the four-kernel chain
 *                                      (no persistent / team kernel, no fused path, no step inside the reduction).
 *   "pose_covariance"        0         1: bpvo_hip_add_frame(_stereo), bpvo_hip_add_frames(_stereo) and bpvo_hip_add_frames_rig run the pose-covariance pass
 *                                      (bpvo_hip_pose_covariances above) behind the estimate the result's pose comes from — all estimating sequences of
 *                                      a call in one launch set per group of BPVO_HIP_COV_GROUP —, write it into result.covariance and keep the record
 *                                      for bpvo_hip_vo / seq / rig_pose_covariance: about one more finest-level linearisation per estimate.  0: those
 *                                      calls issue exactly the launches they issue without the feature and return the Identity.  Poses, statistics,
 *                                      key-frame decisions, point clouds, residuals, weights and counters are the same either way.  More than 48
 *                                      channels: BPVO_ERR_UNSUPPORTED.
 *   "keep_current_disparity" 0         bpvo_hip_batch_run stores the disparity of the CURRENT frame (B) of every pair too.  By default it is
 *                                      neither uploaded nor stored — nothing on the path reads it — and bpvo_hip_frame(s)_set_template on
 *                                      such a slot returns BPVO_ERR_NO_DATA; set 1 before batches whose B frames become templates later.
 *
 * The environment variable BPVO_HIP_OPTIONS="key=value,key=value" applies the same settings to every context a process creates
 * (measurement scripts and tests; the library reads no other variable). */
int bpvo_hip_set_option(bpvo_hip_ctx* ctx, const char* key, double value);
int bpvo_hip_get_option(bpvo_hip_ctx* ctx, const char* key, double* value);
/* = bpvo_hip_set_option(ctx, "lanes", n); n <= 0 restores the default */
int bpvo_hip_set_max_lanes(bpvo_hip_ctx* ctx, int n);
/* diagnostics: Gauss-Newton state of a workspace after its last call: T (16), H (36), G (6), dp (6), f_norm, scale, delta_scale,
 * g_norm, pose of the last linearisation (16) */
int bpvo_hip_debug_gn_state(bpvo_hip_ctx* ctx, int ws, float out[84]);
/* diagnostics: what the library's contexts hold right now, process-wide: device buffers, pinned host buffers, streams, events (a
 * context that has been destroyed, or whose creation failed, has given back all it took) */
int bpvo_hip_debug_live_resources(int counts[4]);

/* ---- disparity fusion (an extension: no reference member; off by default) ---------------------------------------------------------
 * A sequence in mode 1 carries, in the geometry of its latest frame, a disparity map Dc and a variance map Vc (f32, level-0 size; Vc < 0:
 * the pixel carries nothing), outside its three frame slots.  Every frame, the maps are predicted into the new frame with the frame-to-frame
 * motion the call estimated (Result::pose) and fused with the measured map M; the result replaces the carried maps AND the disparity of the
 * frame's slot, in front of the template stage, so whichever frame becomes a key frame builds its template from the fused map.  It touches
 * no Gauss-Newton kernel.  The rule (bpvo_amd/csrc/disparity_fusion_math.h states it as code, once, for host and device):
 *   valid(d) := d >= lo && d <= hi with lo = minValidDisparity, hi = maxValidDisparity of the sequence's parameters (the template stage's gate).
 *   1. Prediction, a forward splat with a z-buffer.  For every pixel (x, y) with Vc >= 0, in f64, each operation rounded on its own:
 *      Z = fx b / d, X = (x - cx) Z / fx, Y = (y - cy) Z / fy, (X', Y', Z') = R (X, Y, Z) + t of the motion P (row-major 4x4, X_new = P X_old,
 *      summed left to right); dropped unless Z' > 0; u = fx X' / Z' + cx, v = fy Y' / Z' + cy, dropped unless both are of magnitude below
 *      2^30 (NaN fails); the target is (rint(u), rint(v)), ties to even, dropped outside the image; d' = (float)(fx b / Z'), dropped unless
 *      d' > 0 and valid(d'); s = d' / d; v' = (float)(Vc s^2 s^2 + process_sigma^2), dropped unless finite.  A target keeps the candidate of
 *      the LARGEST key bits(d') 2^32 + bits(v'): the nearest surface, then the larger variance — a pure function of the inputs, whatever
 *      order the lanes arrive in.  A motion with a non-finite entry gives no prediction at all.
 *   2. Update, per pixel in f32, every + - * / sqrt correctly rounded and none contracted; m = M[p], r2 = measurement_sigma^2, (pd, pv) the
 *      candidate that arrived, if one did:
 *        valid(m), candidate, |m - pd| <= gate sqrt(pv + r2)   D = pd + k (m - pd), k = pv / (pv + r2) (m if that leaves the gate), V = pv - k pv   "fused"
 *        valid(m), candidate, not consistent                   D = m, V = r2                                                                    "replaced"
 *        valid(m), no candidate                                D = m, V = r2                                                                    "measured"
 *        not valid(m), candidate with pv <= max_fill_sigma^2   D = pd, V = pv                                                                   "filled"
 *        otherwise                                             D = m (the caller's bits), V = -1                                                "none"
 *      A measured-valid pixel stays valid.  On a sequence's first frame, after bpvo_hip_seq_reset, or with nothing carried, every pixel is
 *      "measured" or "none" and the slot's disparity is the caller's, bit for bit.
 * Units: disparity pixels; gate in standard deviations.  Mode 1 needs finite values, measurement_sigma > 0, process_sigma >= 0, gate > 0,
 * max_fill_sigma >= 0 (0: never fill); anything else is BPVO_ERR_INVALID_ARG and changes nothing.  A context that declares a rig refuses
 * mode 1 with BPVO_ERR_UNSUPPORTED (and a context with mode 1 somewhere refuses a rig).  Nothing is allocated and nothing is launched until
 * a sequence has mode 1; with mode 0 everywhere every call is what it was. */
typedef struct bpvo_hip_disparity_fusion {
  int mode;                 /* 0 off, 1 on */
  float measurement_sigma, process_sigma, gate, max_fill_sigma;
} bpvo_hip_disparity_fusion;
/* the last fusion of a sequence: the pixels of each class, whether the carried maps were predicted (0: first frame, nothing carried, or a
 * motion that is not finite), the frame slot whose disparity it replaced, and the motion it was given */
typedef struct bpvo_hip_disparity_fusion_info {
  uint32_t fused, replaced, measured, filled, none;
  int predicted;
  int slot;
  int reserved_;
  float motion[16];
} bpvo_hip_disparity_fusion_info;
/* the context's setting (bpvo_hip_add_frame's sequence, and every sequence without its own) */
int bpvo_hip_set_disparity_fusion(bpvo_hip_ctx* ctx, const bpvo_hip_disparity_fusion* fusion);
int bpvo_hip_get_disparity_fusion(const bpvo_hip_ctx* ctx, bpvo_hip_disparity_fusion* fusion);
/* a sequence's own (null: back to the context's); it outlives bpvo_hip_seq_reset like the parameters, the carried maps do not */
int bpvo_hip_seq_set_disparity_fusion(bpvo_hip_ctx* ctx, int seq, const bpvo_hip_disparity_fusion* fusion);
int bpvo_hip_seq_get_disparity_fusion(const bpvo_hip_ctx* ctx, int seq, bpvo_hip_disparity_fusion* fusion, int* own);
/* the carried maps, to host memory, each of the camera's rows x cols floats; either may be null.  BPVO_ERR_NO_DATA while nothing is carried */
int bpvo_hip_vo_get_fused_disparity(bpvo_hip_ctx* ctx, float* disparity, float* variance);
int bpvo_hip_seq_get_fused_disparity(bpvo_hip_ctx* ctx, int seq, float* disparity, float* variance);
int bpvo_hip_vo_disparity_fusion_info(bpvo_hip_ctx* ctx, bpvo_hip_disparity_fusion_info* info);
int bpvo_hip_seq_disparity_fusion_info(bpvo_hip_ctx* ctx, int seq, bpvo_hip_disparity_fusion_info* info);
/* The filter without the VO, for callers with a tracker of their own: the carried maps of the n sequences seq[i] (null: 0 .. n-1) advance
 * by the caller's motions poses [n][16] with the measured maps `disparities`, packed back to back as for bpvo_hip_add_frames (each of its
 * sequence's camera size; on_device: in device memory).  The fused map also replaces the disparity of the sequence's current frame slot.
 * On a bpvo_hip_create context n = 1 serves the context's own state.  Every check runs before anything changes; every named sequence must
 * be in mode 1. */
int bpvo_hip_fuse_disparities(bpvo_hip_ctx* ctx, int n, const int* seq, const float* disparities, int on_device, const float* poses);
/* a frame slot's disparity map (level-0 size of the slot's camera), to host memory */
int bpvo_hip_get_disparity(bpvo_hip_ctx* ctx, int slot, float* out);
/* measurement: kernel launches of the feature and pixels updated since the context was created */
int bpvo_hip_disparity_fusion_counts(bpvo_hip_ctx* ctx, uint64_t* launches, uint64_t* pixels);

/* ---- measurement variance (an extension: no reference member; off by default) ---------------------------------------------------------
 * The other half of the filter above: instead of the constant measurement_sigma^2 the update's r2 is, per pixel, the variance of the measured
 * disparity, taken from the matching cost of the rectified pair around it (Matthies, Kanade and Szeliski).  The rule
 * (bpvo_amd/csrc/disparity_variance_math.h states it as code, once, for host and device) for the rectified u8 pair L, R (level-0 size), the
 * measured map M (x_right = x_left - d), the gate lo, hi of the sequence's parameters, the radius rho, n = (2 rho + 1)^2, and noise2, min2,
 * max2 the f32 squares of noise_sigma, min_sigma, max_sigma; per pixel (x, y), in this order:
 *   1. not valid(M) (the gate, as above)                                                     R2 = max2   "invalid"
 *   2. d0 = (int) rint((double) M), ties to even
 *   3. the left window, rows y - rho .. y + rho and columns x - rho .. x + rho, or the right windows' columns x - rho - d0 - 1 ..
 *      x + rho - d0 + 1 not inside the image, or |M| >= 2^30                                   R2 = max2   "border"
 *   4. S_k = sum over |i|, |j| <= rho of (L[y + j, x + i] - R[y + j, x + i - d0 - k])^2 for k = -1, 0, +1: exact integers below 2^24
 *   5. a = S_-1 + S_+1 - 2 S_0; a <= 0                                                       R2 = max2   "flat"
 *   6. v = (float) (2 max(2 n noise2, S_0) / (n a)), in f64: the products are exact, the division is the only rounding before the cast
 *   7. v < min2: R2 = min2 "floor"; v > max2: R2 = max2 "ceiling"; otherwise R2 = v "model".
 * (a / 2 is the curvature of the parabola through the three sums; with a pixel noise of variance s per image the variance of its minimum is
 * 4 s / a, and s is the larger of noise_sigma^2 and the match's own residual S_0 / (2 n): the variance rises on weak texture and on bad
 * matches.)  Every value the rule writes lies within (0, FLT_MAX].
 * Units: noise_sigma in grey levels, min_sigma and max_sigma in disparity pixels.  Mode 1 needs radius 1 .. 7, finite values, noise_sigma > 0
 * and 0 < min_sigma <= max_sigma whose f32 squares are positive and finite; no default is guessed; anything else is BPVO_ERR_INVALID_ARG and
 * changes nothing.
 * Where it runs: in the stereo drivers (bpvo_hip_add_frame_stereo, bpvo_hip_add_frames_stereo and their _raw forms), for every frame whose
 * sequence has disparity fusion in mode 1 AND measurement variance in mode 1: one launch per call behind the matcher, and the frame's fusion
 * — whichever of the call's stages runs it — takes r2 from the map.  A sequence with the variance on and fusion off does nothing.  Calls
 * that bring their own disparities (bpvo_hip_add_frame, bpvo_hip_add_frames) have no pair: they use the constant measurement_sigma^2, as
 * before; their composition with a variance map is bpvo_hip_fuse_disparities_var and a context in mode 0.  With mode 0 everywhere nothing is
 * allocated or launched and every call is what it was. */
typedef struct bpvo_hip_measurement_variance {
  int mode;                 /* 0 off, 1 on */
  int radius;               /* the window's, 1 .. 7 */
  float noise_sigma, min_sigma, max_sigma;
} bpvo_hip_measurement_variance;
/* the pixels of each class in a sequence's last map */
typedef struct bpvo_hip_measurement_variance_info {
  uint32_t invalid, border, flat, floor, ceiling, model;
} bpvo_hip_measurement_variance_info;
/* the context's setting (bpvo_hip_add_frame_stereo's sequence, and every sequence without its own) */
int bpvo_hip_set_measurement_variance(bpvo_hip_ctx* ctx, const bpvo_hip_measurement_variance* setting);
int bpvo_hip_get_measurement_variance(const bpvo_hip_ctx* ctx, bpvo_hip_measurement_variance* setting);
/* a sequence's own (null: back to the context's); it outlives bpvo_hip_seq_reset like the fusion setting */
int bpvo_hip_seq_set_measurement_variance(bpvo_hip_ctx* ctx, int seq, const bpvo_hip_measurement_variance* setting);
int bpvo_hip_seq_get_measurement_variance(const bpvo_hip_ctx* ctx, int seq, bpvo_hip_measurement_variance* setting, int* own);
/* The map (to host memory, the camera's rows x cols floats) and the class counts the sequence's frame got in the last stereo call.
 * BPVO_ERR_NO_DATA before the sequence's first such call, after bpvo_hip_seq_reset, and — the map only, which lives in the front-end's
 * scratch — once a later call of the front-end's has reused the scratch without the sequence. */
int bpvo_hip_vo_get_measurement_variance(bpvo_hip_ctx* ctx, float* variance);
int bpvo_hip_seq_get_measurement_variance_map(bpvo_hip_ctx* ctx, int seq, float* variance);
int bpvo_hip_vo_measurement_variance_info(bpvo_hip_ctx* ctx, bpvo_hip_measurement_variance_info* info);
int bpvo_hip_seq_measurement_variance_info(bpvo_hip_ctx* ctx, int seq, bpvo_hip_measurement_variance_info* info);
/* The rule alone: the variance maps of n rectified pairs of the n cameras' sizes with the measured maps `disparity`, images and maps packed
 * back to back as for bpvo_hip_stereo_frames (on_device: all three in device memory), under the gate lo .. hi and the setting (mode 1), in
 * ONE launch; variance_out packed alike (variance_on_device: in device memory); counts_out: null, or [n][6] class counts in the order of
 * bpvo_hip_measurement_variance_info.  Touches no sequence (but the front-end's scratch, like bpvo_hip_stereo_frames). */
int bpvo_hip_disparity_variance_frames(bpvo_hip_ctx* ctx, int n, const bpvo_hip_camera* cams, const uint8_t* left, const uint8_t* right,
                                       const float* disparity, int on_device, float lo, float hi, const bpvo_hip_measurement_variance* setting,
                                       float* variance_out, int variance_on_device, uint32_t* counts_out);
/* bpvo_hip_fuse_disparities with the measurements' variances, packed like the maps (on_device: both in device memory): an entry within
 * (0, FLT_MAX] is the update's r2 for its pixel, any other entry (0, negative, NaN, Inf) takes measurement_sigma^2 */
int bpvo_hip_fuse_disparities_var(bpvo_hip_ctx* ctx, int n, const int* seq, const float* disparities, const float* variances, int on_device,
                                  const float* poses);
/* measurement: launches of the variance kernel and pixels it has served since the context was created, and (tiles: null, or [3]) the tiles
 * whose right strip was staged in LDS, that read the right image directly (disparities spread too far), and that needed no sums at all */
int bpvo_hip_measurement_variance_counts(bpvo_hip_ctx* ctx, uint64_t* launches, uint64_t* pixels, uint64_t* tiles);

/* ---- motion stereo (an extension: no reference member; off by default) ---------------------------------------------------------------
 * Every addFrame estimates the motion between two images of ONE camera, the key frame and the current frame: a second baseline beside the
 * stereo one, which grows with the motion and exists where the matcher returned nothing.  Motion stereo refines the PREDICTION of disparity
 * fusion — the z-buffer word (pd, pv) of a pixel, between the filter's splat and its update — by a short search along the pixel's epipolar
 * line in the key frame.  The rule (bpvo_amd/csrc/motion_stereo_math.h states it as code, once, for host and device) for a pixel (x, y) of
 * the first image C (u8, level 0), the second image K of the same camera and size, the motion Q (row-major, X_K = Q X_C; R its rotation,
 * t its translation), the camera fx, fy, cx, cy, b, the gate lo, hi of the sequence's parameters, and noise2, min2, max2 the f32 squares of
 * noise_sigma, min_sigma, max_sigma; in this order:
 *   1. no prior (a word 0, pv < 0 or NaN), or not lo <= pd <= hi                                                        "no_prior"
 *   2. in f64, every operation rounded on its own: a = (x - cx) / fx, bq = (y - cy) / fy, h = (R_i0 a + R_i1 bq) + R_i2, e = t / (fx b);
 *      N0(d) = h0 + d e0, N1(d) = h1 + d e1, D(d) = h2 + d e2; u(d) = (fx N0) / D + cx, v(d) = (fy N1) / D + cy: the epipolar curve.  At
 *      d = pd: u' = (fx (e0 D - N0 e2)) / (D D), v' = (fy (e1 D - N1 e2)) / (D D), the gain g = sqrt(u' u' + v' v'), in pixels of K per pixel
 *      of disparity.  g not finite or g < min_gain (pure rotation, a pixel next to the epipole)                         "low_parallax"
 *      delta = 1 / g: one pixel along the line.
 *   3. the hypotheses d_j = pd + j delta, j = -steps .. steps.  Each needs d_j > 0, D(d_j) > 0 and |u|, |v| < 2^20; its centre is quantised
 *      to 1/32 pixel, xq = nearbyint(32 u), ties to even, likewise yq (the rectification's entry).  The window of (2 radius + 1)^2 pixels
 *      around (x, y) must lie inside C, and every sample of the window around the centre inside K with all four taps: columns
 *      (xq >> 5) - radius .. (xq >> 5) + radius + 1, rows likewise.  Any hypothesis fails any of these                  "border"
 *   4. S_j = sum over |ii|, |jj| <= radius of (C[y + jj][x + ii] - k)^2 with k the rectification's pixel of K at (xq + 32 ii, yq + 32 jj):
 *      four taps with integer weights of 1/32, + 512 >> 10.  Exact integers.
 *   5. j* the first minimum (the lowest j on ties); |j*| = steps                                                        "edge"
 *      a2 = S_{j*-1} + S_{j*+1} - 2 S_{j*}; a2 <= 0                                                                     "flat"
 *      (as j* is the FIRST minimum and lies inside, S_{j*-1} > S_{j*}: a2 >= 1, the class is a guard that no input reaches)
 *   6. in f64: o = (S_{j*-1} - S_{j*+1}) / (2 a2), dt = (float) (pd + (j* + o) delta); vt = (float) ((2 max(2 n noise2, S_{j*}) / (n a2))
 *      (delta delta)), n = (2 radius + 1)^2, clamped to [min2, max2] — the measurement variance's model with one step in place of one pixel
 *   7. in f32, the "fused" arithmetic of disparity fusion: s = pv + vt; |dt - pd| > gate sqrt(s), or the fused value not positive or outside
 *      the gate: the prior stays                                                                                        "rejected"
 *      k = pv / s, pd' = pd + k (dt - pd), pv' = pv - k pv                                                              "fused"
 * Every class but "fused" keeps the prior's own bits.
 * Units: min_gain in pixels per disparity pixel, noise_sigma in grey levels, min_sigma and max_sigma in disparity pixels, gate in standard
 * deviations.  Mode 1 needs radius 1 .. 3, steps 1 .. 8, finite values, min_gain > 0, noise_sigma > 0, 0 < min_sigma <= max_sigma and
 * gate > 0; no default is guessed; anything else is BPVO_ERR_INVALID_ARG, names the field in bpvo_hip_last_error and changes nothing.  A
 * context that declares a rig refuses mode 1 with BPVO_ERR_UNSUPPORTED (and a context with mode 1 somewhere refuses a rig).
 * Where it runs: in every addFrame driver (bpvo_hip_add_frame, bpvo_hip_add_frames, their stereo and raw stereo forms), for every frame
 * whose sequence has disparity fusion in mode 1 AND motion stereo in mode 1, whose fusion predicts (not a first frame) and whose estimate is
 * finite: ONE launch per fusion stage between the splat and the update.  C is the frame, K the key frame of the call's last estimate T
 * (X_C = T X_K) — the key frame the call began with, or, at a key frame with re-estimation, the new key frame —, Q = T^-1 (the library's f32
 * cofactor inverse).  A sequence with motion stereo on and fusion off does nothing.  With mode 0 everywhere nothing is allocated or launched
 * and every call is what it was. */
typedef struct bpvo_hip_motion_stereo {
  int mode;                 /* 0 off, 1 on */
  int radius;               /* the window's, 1 .. 3 */
  int steps;                /* hypotheses on either side of the prior, 1 .. 8 */
  float min_gain, noise_sigma, min_sigma, max_sigma, gate;
} bpvo_hip_motion_stereo;
/* the last frame of a sequence: the pixels of each class (all 0 when no launch was made for it), whether a launch was made, the frame slot of
 * the second view, and the motion Q the rule was given */
typedef struct bpvo_hip_motion_stereo_info {
  uint32_t no_prior, low_parallax, border, edge, flat, rejected, fused;
  int launched;
  int view_slot;
  int reserved_[3];
  float motion[16];
} bpvo_hip_motion_stereo_info;
/* the context's setting (bpvo_hip_add_frame's sequence, and every sequence without its own) */
int bpvo_hip_set_motion_stereo(bpvo_hip_ctx* ctx, const bpvo_hip_motion_stereo* setting);
int bpvo_hip_get_motion_stereo(const bpvo_hip_ctx* ctx, bpvo_hip_motion_stereo* setting);
/* a sequence's own (null: back to the context's); it outlives bpvo_hip_seq_reset like the fusion setting */
int bpvo_hip_seq_set_motion_stereo(bpvo_hip_ctx* ctx, int seq, const bpvo_hip_motion_stereo* setting);
int bpvo_hip_seq_get_motion_stereo(const bpvo_hip_ctx* ctx, int seq, bpvo_hip_motion_stereo* setting, int* own);
int bpvo_hip_vo_motion_stereo_info(bpvo_hip_ctx* ctx, bpvo_hip_motion_stereo_info* info);
int bpvo_hip_seq_motion_stereo_info(bpvo_hip_ctx* ctx, int seq, bpvo_hip_motion_stereo_info* info);
/* The rule alone, under the context's setting (mode 1) and the gate of the context's parameters: n pairs of views of the n cameras (K,
 * baseline and size are read), the first and the second images packed back to back as for bpvo_hip_stereo_frames, motions [n][16] (Q, X_second
 * = Q X_first), and the priors packed alike — a pixel has no prior where prior_variance < 0 (on_device: all four in device memory, and so are
 * the outputs).  out_disparity, out_variance (f32) and out_class (u8), packed alike; each may be null.  ONE launch; touches no sequence. */
int bpvo_hip_motion_stereo_frames(bpvo_hip_ctx* ctx, int n, const bpvo_hip_camera* cams, const uint8_t* first, const uint8_t* second,
                                  const float* motions, const float* prior_disparity, const float* prior_variance, int on_device,
                                  float* out_disparity, float* out_variance, uint8_t* out_class);
/* measurement: launches of the kernel and pixels it has served since the context was created; tiles: null, or [3], the tiles whose K box was
 * staged in LDS, that read K directly (the samples spread too far), and that needed no sums at all; classes: null, or [7], the pixels of each
 * class over all launches, in the order of bpvo_hip_motion_stereo_info */
int bpvo_hip_motion_stereo_counts(bpvo_hip_ctx* ctx, uint64_t* launches, uint64_t* pixels, uint64_t* tiles, uint64_t* classes);

#ifdef __cplusplus
}
#endif
#endif /* BPVO_HIP_C_API_H */
