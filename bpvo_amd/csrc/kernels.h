// Launchers of the HIP kernels (kernels_frame.hip, kernels_gn.hip).
#pragma once

#include <hip/hip_runtime.h>

#include "types.h"

#include <type_traits>

// The channel counts the kernels are instantiated for: Intensity / Laplacian 1, IntensityAndGradient 3, DescriptorFields 5,
// BitPlanes 8, DescriptorFields2ndOrder 10, CentralDifference 8 / 24 / 48, Latch 8 / 16 / 32.  f receives std::integral_constant<int, C>.
template <class F>
static inline void dispatch_channels(int C, F&& f)
{
  switch(C) {
    case 1: f(std::integral_constant<int, 1>()); break;
    case 3: f(std::integral_constant<int, 3>()); break;
    case 5: f(std::integral_constant<int, 5>()); break;
    case 10: f(std::integral_constant<int, 10>()); break;
    case 16: f(std::integral_constant<int, 16>()); break;
    case 32: f(std::integral_constant<int, 32>()); break;
    case 24: f(std::integral_constant<int, 24>()); break;
    case 48: f(std::integral_constant<int, 48>()); break;
    default: f(std::integral_constant<int, 8>()); break;
  }
}

// ... and the WIDE descriptors (more than 48 channels): LATCH with 8 / 16 / 32 / 64 bytes, CentralDifference radii 4 .. 9.  Only kernels whose
// per-thread state does not grow with C are instantiated for these (the saliency forms: C is a stride and a loop bound there); the per-point
// kernels run the channels in groups (types.h PairJob::pitch) or loop over them at run time.
template <class F>
static inline bool dispatch_wide_channels(int C, F&& f)
{
  switch(C) {
    case 64: f(std::integral_constant<int, 64>()); return true;
    case 80: f(std::integral_constant<int, 80>()); return true;
    case 120: f(std::integral_constant<int, 120>()); return true;
    case 128: f(std::integral_constant<int, 128>()); return true;
    case 168: f(std::integral_constant<int, 168>()); return true;
    case 224: f(std::integral_constant<int, 224>()); return true;
    case 256: f(std::integral_constant<int, 256>()); return true;
    case 288: f(std::integral_constant<int, 288>()); return true;
    case 360: f(std::integral_constant<int, 360>()); return true;
    case 512: f(std::integral_constant<int, 512>()); return true;
    default: return false;
  }
}

namespace bpvo_hip {

// Views carved from one allocation, each rounded up to 256 bytes: a layout is written once as a sequence of take<T>(count) steps — on a null
// base the views are null and `off` ends as the layout's size (the slabs of host_ctx.h, the scratch of the semi-global matchers).
inline size_t align_up(size_t v, size_t a = 256) { return (v + a - 1) / a * a; }
struct Carver {
  unsigned char* base;
  size_t off = 0;
  template <typename T>
  T* take(size_t count)
  {
    T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += align_up(count * sizeof(T));
    return p;
  }
};

// A Gaussian smoothing kernel of cv::GaussianBlur as the descriptors use it: n taps (odd; 0 = no smoothing), k the f32 taps
// of cv::getGaussianKernel, ki their 8-bit fixed-point form cvRound(k * 256) for u8 images.  n = 5 runs the small-kernel
// forms of OpenCV's filter engine, n >= 7 the generic ones (kernels_frame.hip, df_plane_kernel).
constexpr int kMaxGaussTaps = 31;
struct GaussTaps { int n = 0; float k[kMaxGaussTaps] = {}; int ki[kMaxGaussTaps] = {}; };

// per-frame stage (batched over frames)
void launch_ingest(hipStream_t s, const FrameJob* jobs_level0, const uint8_t* d_images, const float* d_disps, size_t npix, int nframes, int skip_odd_disp = 0);
// ... frame z at pixel offset d_offsets[z] (device) of both packed buffers
void launch_ingest_at(hipStream_t s, const FrameJob* jobs_level0, const uint8_t* d_images, const float* d_disps, const size_t* d_offsets, size_t npix, int nframes);
void launch_pyrdown(hipStream_t s, const FrameJob* src, const FrameJob* dst, int dW, int dR, int nframes);
// few frames: `steps` (1..3) pyrDown steps in one launch — src_row is the source level's row of the table [level][job_pitch], dW x dR the COARSEST level of the group
void launch_pyramid_levels(hipStream_t s, const FrameJob* src_row, int job_pitch, int steps, int dW, int dR, int nframes);
// A frame-stage launch over `nlevels` consecutive levels of `nframes` frames each (kernels_frame.hip level_job): `jobs` is the FINEST of these
// levels' row of the table [level][job_pitch] and W x R that level's size — the grid is sized for it.  Built in one place: host_ctx.h frame_launch
struct FrameLaunch { const FrameJob* jobs; int W, R, nframes, nlevels, job_pitch; };
void launch_intensity(hipStream_t s, const FrameLaunch& f);
// normalised intensity (kernels_intensity_norm.hip): radius 0 — histogram + table, then the table applied (two launches; FrameJob::inorm);
// radius 1 .. 15 — the local form, one launch
void launch_intensity_norm(hipStream_t s, const FrameLaunch& f, int radius);
void launch_gradient_descriptor(hipStream_t s, const FrameJob* jobs, int W, int R, int nframes, const GaussTaps& pre);   // (I, Ix, Iy), C = 3
void launch_descriptor_fields(hipStream_t s, const FrameJob* jobs, int W, int R, int nframes, int second_order, const GaussTaps& g1,
                              const GaussTaps& g2);   // C = 5 / 10
void launch_central_difference(hipStream_t s, const FrameJob* jobs, int W, int R, int nframes, int radius, const GaussTaps& before,
                               const GaussTaps& after);   // C = 8 / 24 / 48
void launch_latch(hipStream_t s, const FrameJob* jobs, int W, int R, int nframes, int bytes, int half_ssd, const signed char* d_offsets, int kc, int ks,
                  const GaussTaps& after);   // C = 8 * bytes, bytes = 1 / 2 / 4
void launch_laplacian(hipStream_t s, const FrameJob* jobs, int W, int R, int nframes, int ksize /*1 or 3*/);
void launch_census(hipStream_t s, const FrameLaunch& f, const int* blur_taps /*null: no smoothing, one level*/);
// one level of a pair batch (jobs A, B, A, B, ...) with census-only template frames: B over every tile, A over the dense tile columns only
void launch_bitplanes_pairs(hipStream_t s, const FrameLaunch& f, const float k[3]);
// the census bytes of the census-only levels (FrameJob::lazy == 2) among jobs 0, 2, 4, ... — the template frames of a pair batch; other jobs are left alone
void launch_census_templates(hipStream_t s, const FrameLaunch& f);
// from_image: the census transform is computed inside the bit-planes kernel (no launch_census, sigma_bp > 0 and sigma_ct <= 0); sigma <= 0: one level
void launch_bitplanes(hipStream_t s, const FrameLaunch& f, float sigma, const float k[3], int from_image);
// (minSaliency and the disparity gate: each frame's own, FrameJob::min_saliency / min_disp / max_disp)
// gauss_k: the bit-planes blur taps (census-only levels, FrameJob::lazy == 2: the tiles form channel 0 themselves)
// part: everything, or — a stage with a point budget, which launch_point_budget serves in between — the candidates alone, then the scan and the compaction
enum { SELECT_ALL = 0, SELECT_CANDIDATES = 1, SELECT_COMPACT = 2 };
// nms_radius > 1 (flag bytes): one level
void launch_saliency_select(hipStream_t s, const FrameLaunch& f, int C, int nms_radius, int border, const float gauss_k[3], int part);
// of the candidates of every job with FrameJob::max_points > 0 the max_points most salient stay (kernels_frame.hip point_budget_kernel)
void launch_point_budget(hipStream_t s, const FrameLaunch& f, int nms_radius);
void launch_saliency(hipStream_t s, const FrameLaunch& f, int C);      // the saliency map alone, from dense records (one level)
void launch_copy_rows(hipStream_t s, void* dst, const void* src_host_pinned, size_t pitch_bytes, size_t width_bytes, int rows);   // multiples of 8 bytes
void launch_gather_counts(hipStream_t s, const FrameJob* jobs /*[L][job_pitch]*/, int job_pitch, int nframes, int first_level, int num_levels,
                          int* out /*[nframes][kMaxLevels]*/);
void launch_normalization(hipStream_t s, const FrameJob* jobs /*[L][job_pitch]*/, int job_pitch, int nframes, int first_level,
                          int num_levels, int with_normalization, int form = 1);   // form of the sequential sums (same sums): 1 hand-scheduled DPP add chains, 0 the compiler's DPP form, 2 broadcast LDS reads + plain adds
void launch_export_jacobians(hipStream_t s, const FrameJob* job /*device, one job*/, int C, int n, float* out /*[C*n][6]*/);
// max_points: the most points of a job of the launch; gauss_k: the bit-planes blur taps (lazy levels)
void launch_template_build(hipStream_t s, const FrameLaunch& f, int C, int max_points, int grad_cd5, const float gauss_k[3]);

// stereo front-end (kernels_stereo.hip): OpenCV 2.4 block matching with the reference's parameters, batched over frames
// A frame of a call whose frames differ in size: its size and where its pixels start in the packed images and maps (device table, a row per frame)
struct StereoFrame { int rows, cols; size_t offset; };
struct StereoLaunch {
  const uint8_t* left_pre;    // [nframes][rows*cols] pre-filtered images
  const uint8_t* right_pre;
  float* disp;                // [nframes][rows*cols]
  int rows, cols, nframes;
  const StereoFrame* frames = nullptr;   // non-null: the table form — frame f is frames[f], rows x cols the largest of them, total_pixels their sum
  size_t total_pixels = 0;
  int wsz, ndisp, mindisp, cap, texture_threshold, uniqueness_ratio;
};
void launch_stereo_prefilter(hipStream_t s, const uint8_t* src, uint8_t* dst, int rows, int cols, int cap, int nframes);
void launch_stereo_prefilter_frames(hipStream_t s, const uint8_t* src, uint8_t* dst, const StereoFrame* frames /*device*/, int max_rows, int max_cols,
                                    int cap, int nframes);
bool launch_stereo_bm(hipStream_t s, const StereoLaunch& g);   // false: window size / disparity range outside what the kernel serves
// Rectification (kernels_rectify.hip; the rule: rectify_math.h): one frame of a call — a raw image of raw_rows x raw_cols bytes at src, the map
// of the rows x cols destination pixels (RectEntry per pixel), the rectified image at dst (any byte address).  One launch serves the table.
struct RectifyFrame { int rows, cols, raw_rows, raw_cols; const int2* map; const uint8_t* src; uint8_t* dst; };
void launch_rectify_frames(hipStream_t s, const RectifyFrame* frames /*device*/, int nframes, int max_rows, int max_cols);
// Disparity fusion (kernels_disparity_fusion.hip; the rule: disparity_fusion_math.h): one sequence of a call — its camera and gate, the rule's
// parameters, the motion's first three rows, the slot's disparity (the measured map in, the fused map out), the carried maps, the job's z-buffer
// (u64 per pixel, all zero between calls) and its five class counters.  predict 0: the splat skips the job (nothing carried, or a motion that
// is not finite).  R: null, or the measurement's variance per pixel — an entry within (0, FLT_MAX] is the update's r2 for its pixel, any other
// entry takes the job's r2.  One launch per stage serves the table.
struct FusionJob {
  int rows, cols, predict, pad_;
  float fx, fy, cx, cy, b, lo, hi;
  float r2, q2, gate, fill2;
  float P[12];
  float* slot;
  float* Dc;
  float* Vc;
  unsigned long long* zbuf;
  unsigned* counts;
  const float* R;
};
void launch_fusion_splat(hipStream_t s, const FusionJob* jobs /*device*/, int njobs, size_t max_pixels);
void launch_fusion_update(hipStream_t s, const FusionJob* jobs /*device*/, int njobs, size_t max_pixels);
// Measurement variance (kernels_disparity_variance.hip; the rule: disparity_variance_math.h): one rectified pair of a call — the u8 images, the
// measured map, the variance map it writes (all rows x cols, any byte / 4-byte alignment), the gate, the radius and the three squares of the
// setting, and its counters: the six classes, then the tiles that took the staged / the direct / no path.  One launch serves the table;
// max_tiles: the largest disparity_variance_tiles(rows, cols) among the jobs.
struct VarianceJob {
  const uint8_t* L;
  const uint8_t* R;
  const float* M;
  float* out;
  unsigned* counts;      // [kVarianceCounters]
  int rows, cols, radius, pad_;
  float lo, hi, noise2, min2, max2;
};
constexpr int kVarianceCounters = 6 + 3;
void launch_disparity_variance(hipStream_t s, const VarianceJob* jobs /*device*/, int njobs, int max_tiles);
int disparity_variance_tiles(int rows, int cols);
// Motion stereo (kernels_motion_stereo.hip; the rule: motion_stereo_math.h): one pair of views of a call — the first image C and the second
// image K (u8, rows x cols, any alignment), the geometry of the pair in f64 as ms_geometry forms it, the gate and the setting's numbers, and its
// counters: the seven classes, then the tiles that took the staged / the direct / no path.  The prior and the result are EITHER the words of a
// fusion z-buffer, rewritten in place where a pixel is fused (zbuf; a word 0 has no prior and stays 0), OR the caller's maps: pd, pv in and
// out_d, out_v out (each may be null).  out_c: null, or the class of every pixel.  One launch serves the table; max_tiles: the largest
// motion_stereo_tiles(rows, cols) among the jobs.
struct MotionStereoJob {
  const uint8_t* C;
  const uint8_t* K;
  unsigned long long* zbuf;
  const float* pd;
  const float* pv;
  float* out_d;
  float* out_v;
  uint8_t* out_c;
  unsigned* counts;      // [kMotionStereoCounters]
  double fx, fy, cx, cy, R[9], e[3];
  int rows, cols, radius, steps;
  float lo, hi, min_gain, noise2, min2, max2, gate, pad_;
};
constexpr int kMotionStereoCounters = 7 + 3;
void launch_motion_stereo(hipStream_t s, const MotionStereoJob* jobs /*device*/, int njobs, int max_tiles);
int motion_stereo_tiles(int rows, int cols);

// semi-global matching (kernels_sgm.hip): the reference's in-tree SgmStereo (utils/sgm.cc)
struct SgmLaunch {
  const uint8_t* left;      // [nframes][rows*cols]
  const uint8_t* right;
  float* disp;              // [nframes][rows*cols]
  void* scratch;            // frames_per_launch x sgm_scratch_bytes(rows, cols, ndisp) bytes: a slice per frame of a launch, reused by the next launch
  int rows, cols, nframes;
  int frames_per_launch = 1; // frames that go through every kernel together (the grid's last dimension); 1: one frame after the other
  int ndisp, sobel_cap, census_radius, window_radius, P1, P2, consistency_threshold;
  double disparity_factor, census_weight;
};
size_t sgm_scratch_bytes(int rows, int cols, int ndisp);
bool launch_stereo_sgm(hipStream_t s, const SgmLaunch& g);   // false: disparity range outside what the kernels serve (multiple of 16, <= 256)
// filterSpeckles on a u16 map whose invalid value is 0 (kernels_sgm.hip's union-find kernels): 4-connected regions (neighbours both non-zero,
// |difference| <= max_diff) of at most max_size pixels are zeroed; lab / size: rows * cols ints each
// nframes > 1: frame f on the pointers advanced by f * frame_bytes bytes, in the same launches
void launch_speckle_filter_u16(hipStream_t s, uint16_t* img, int* lab, int* size, int rows, int cols, int max_diff, int max_size, int nframes = 1,
                               size_t frame_bytes = 0);

// semi-global block matching (kernels_sgbm.hip): cv::StereoSGBM of OpenCV 2.4, single-pass mode, + medianBlur(3) + filterSpeckles + / 16
struct SgbmLaunch {
  const uint8_t* left; const uint8_t* right;   // [nframes][rows*cols] u8 (device)
  float* disp;                                 // [nframes][rows*cols] f32 (device)
  void* scratch;                               // sgbm_scratch_bytes(rows, cols, min_disp, ndisp) bytes, shared by the frames
  int rows, cols, nframes;
  // the cv::StereoSGBM fields (their "<= 0 means" defaults are applied by the launcher like computeDisparitySGBM does)
  int min_disp, ndisp, sad_window, P1, P2, disp12_max_diff, pre_filter_cap, uniqueness_ratio, speckle_window, speckle_range, full_dp;
};
size_t sgbm_scratch_bytes(int rows, int cols, int min_disp, int ndisp);
bool sgbm_serves(const SgbmLaunch& g, const char** why);      // false + the reason: what the device path does not take
bool launch_stereo_sgbm(hipStream_t s, const SgbmLaunch& g);

// Gauss-Newton stage (batched over workspaces / pairs)
// Compacted list of the workspaces of a launch that are still iterating (estimate loops).  The host rebuilds it (on the
// device) once per round of kItersPerSync iterations, together with the read-back of the count, and sizes the workspace
// dimension of the next round's grids with that count; entry k of the list names the k-th active workspace.  Without it
// every launch dispatches the workgroups of the finished workspaces as well: ~0.9 ns each, ~150 µs per launch in the tail
// of a level at 1024 pairs.  list == nullptr: every workspace of the launch, in order.
constexpr int kDenseRuns = 64;         // runs of candidates per workspace in the dense form of the exact median's bracket step (gn_common.h, bracket_chunk)
constexpr int kChunkPoints = 256;      // points per chunk of the warp + residual kernels = per bracket segment of the exact median (gn_common.h K6_BLOCK)
struct ActiveSet {
  const int* list = nullptr;   // device [npairs]
};

struct GNLaunch {
  const PairJob* jobs;   // device, [npairs] for the level
  int npairs;            // grid size in workspaces (= number of list entries when an ActiveSet is given)
  ActiveSet active;
  int max_points;        // max n over the pairs (grid sizing)
  int C;
  int loss;
  int interp = 0;        // BPVO_INTERP_* (kLinear uses the tap-cached kernel, the others warp_residual_interp_kernel)
  int fuse_frozen = 0;   // estimate loops, C = 8, kLinear, f64 formulation: once a workspace's scale is frozen, irls_reduce
                         // recomputes the residuals itself and warp_residual skips the workspace
  // 1: the bracket step of warp_residual and median_finish keep a workspace's candidates in one contiguous run with four totals
  // (bracket_chunk<C, true>, gn_common.h) instead of per-chunk segments and counters; both launches of an iteration must agree
  int dense_candidates = 0;
  int fast_warp = 0;     // 1: projectPoints / BilinearInterp all-f32 formulation (bpvo_hip_set_warp_formulation)
  // 1: the tile of a workspace that stores its partial LAST in an irls_reduce launch also takes the Gauss-Newton step (what
  // gn_step_kernel does) — the chain is then three kernels per iteration and launch_gn_step is not called
  int step_in_reduce = 0;
  // gn_persistent_kernel only: begin_level >= 0 — the kernel takes the level's start itself (level_begin_kernel's state reset; the tap-cache
  // keys were invalidated by the kernel of the level before, which was handed this level's jobs as next_jobs)
  int begin_level = -1, begin_moot = 0;
  const PairJob* next_jobs = nullptr;
  // 1: validation mode "reference_reduction" (kernels_gn_ref.hip) — launch_irls_reduce sums H, G and the squared norm in the reference's
  // index order (one partial per workspace), launch_gn_step reads that one partial; the fused path and step_in_reduce are ignored
  int reference_reduction = 0;
};
int  gn_num_blocks(int max_points);
void launch_set_pose(hipStream_t s, const PairJob* jobs, const float* T_init, int n, unsigned* clear = nullptr, int clear_words = 0);   // clear: words zeroed by the same launch
// PoseEstimatorBase::reset of every workspace + invalidation of its tap-cache keys (max_points: the largest template of the launch)
void launch_level_begin(hipStream_t s, const PairJob* jobs, int npairs, int max_points, int level, int scale_is_moot = 0);
void launch_reset_tapkeys(hipStream_t s, const GNLaunch& g);
// out_list / out_count <- the still-active workspaces among the n_in entries of `in` (or of 0..n_in-1), in order
void launch_compact_active(hipStream_t s, const PairJob* jobs, ActiveSet in, int n_in, int* out_list, int* out_count);
void launch_warp_residual(hipStream_t s, const GNLaunch& g);
void launch_refresh_residuals(hipStream_t s, const GNLaunch& g);   // fused path: rebuild r / valid of stale workspaces from T_lin
void launch_median(hipStream_t s, const GNLaunch& g);
void launch_irls_reduce(hipStream_t s, const GNLaunch& g);
void launch_reference_reduce(hipStream_t s, const GNLaunch& g);   // what launch_irls_reduce does with g.reference_reduction (kernels_gn_ref.hip)
// mode 0: full PoseEstimatorBase::run step (solve, update, convergence); mode 1: linearize only (H, G, f_norm)
// The limits and tolerances of the state machine are each workspace's own, PairJob::prm — here and in the persistent and team kernels below
void launch_gn_step(hipStream_t s, const GNLaunch& g, int mode);
// Persistent kernel for small groups: one launch runs a whole level of up to kPersistMaxWs workspaces (kernels_gn_team.hip).  ctl: two
// zeroed words {arrivals, abort}; after the launch ctl[1] != 0 says the kernel gave up (states untouched: rerun the chain).
constexpr int kPersistMaxWs = 8;
bool gn_persistent_serves(const GNLaunch& g);
int  gn_persistent_grid(const GNLaunch& g, int max_grid);
hipError_t launch_gn_persistent(hipStream_t s, const GNLaunch& g, unsigned* ctl, int grid, long long timeout_ticks);
// Team-persistent kernels for small batches (kernels_gn_team.hip: gn_team_kernel, whose teams grow, with join_mode != 0; gn_team_fixed_kernel
// with join_mode 0): ONE launch runs every pair of the group through all its pyramid levels; grid = team_size x n_teams (+ spare_workgroups)
// workgroups, one per CU, all co-resident.  ctl: gn_team_ctl_words(n_teams) zeroed words;
// after the launch ctl[1] != 0 says a team barrier gave up (rerun the group on the chain).
struct GNTeamLaunch {
  const PairJob* jobs_all;   // device [levels][job_pitch]
  int job_pitch, n_pairs, level_hi, level_lo;
  int C, loss, fuse_frozen, scale_is_moot;
  int team_size, n_teams;
  unsigned* ctl;
  long long timeout_ticks;
  int local_barriers = 1;    // teams whose workgroups share one XCD (checked on the device) keep their barriers inside that XCD's L2
  int spare_workgroups = 0;  // workgroups beyond n_teams * team_size that start without a team and join one (join_mode != 0 only): the grid fills the chip
  int join_mode = 2;         // workgroups whose team has run out of pairs join the teams still at work: 0 never, 1 teams on their own XCD, 2 any team
};
int  gn_team_ctl_words(int n_teams);
void launch_team_ctl_reset_keep_abort(hipStream_t s, unsigned* ctl, int n_teams);   // between the launches of a split run: every control word to 0 but the abort word
int  gn_team_max_size();       // teams stop admitting newcomers at this size
hipError_t launch_gn_team(hipStream_t s, const GNTeamLaunch& t);
// Rig mode (kernels_gn_rig.hip): the step of n members' jobs (one level's row of the job table, members 0 .. n-1) estimated as one body pose.
// X: device [n][16] camera_from_body; body: the body's GNState (the entry behind the workspaces' states).  mode 0: the full step from the
// members' linearisations (launch_gn_step mode 1 before it) and every member's next pose; 1: the joint linearisation only; 2: the start of
// pyramid level `level` (the body's reset, the members' poses from the body's) — and, T_init (device [16]) non-null, of the estimate.
struct RigStepArgs {
  const PairJob* jobs;
  int n;
  const float* X;
  GNState* body;
  int mode, level;
  const float* T_init;
  // 1 (the estimate loops): the step is taken in the REFERENCE member's normalised twist — jobs[0]'s —, body's T is that member's pose, X the
  // extrinsics relative to it (X[0] the identity) and T_init that member's initial pose; 0: the plain body twist of the body pose
  int reference;
};
void launch_rig_step(hipStream_t s, const RigStepArgs& a);
// Several rigs in one launch (estimate_rigs): workgroup r takes the step of rig r of a device table — RigStepArgs' arithmetic per rig, a rig whose
// body is no longer active left untouched.  The members of all rigs lie back to back in the level's job row, rig r at [first, first + n).
struct RigEntry {
  int first, n;            // the rig's members in the level's job row
  const float* X;          // device [n][16]: the rig's extrinsics (RigStepArgs::X)
  GNState* body;           // the rig's body state
  const float* T_init;     // device [16]: the pose its estimate starts from (mode 2 with with_init)
};
struct RigStepsArgs {
  const PairJob* jobs;     // the level's job row
  const RigEntry* rigs;    // device [n_rigs]
  int n_rigs;
  int mode, level;         // RigStepArgs'
  int with_init;           // mode 2: the start of the estimate as well (every rig's own T_init)
  int reference;           // RigStepArgs'
  int* active_out;         // device [n_rigs]: every body's `active` after the step (0 for a rig that was left alone)
};
void launch_rig_steps(hipStream_t s, const RigStepsArgs& b);
// Pose covariance (kernels_gn_cov.hip; c_api.h bpvo_hip_pose_covariances).  A pass serves n_records records of `members` members each (a camera:
// one member; a rig: one record of all its members); entry r * members + p of `jobs` / `members_tab` is member p of record r.  The jobs are COPIES
// of the workspaces' jobs whose r, valid, partials, cnt and st point into the pass's own scratch (no tap cache, no median buffers: the scratch
// state's scale is frozen), so the warp_residual launches of the pass write nothing a later call reads.
struct CovMember {
  const GNState* src;      // the workspace's own state: pose (T_out), scale and level of its last estimate, read when none is given
  float* sums;             // [72] the member's M and Q (normalised twist, symmetric, narrowed to f32): bpvo_hip_debug_pose_covariance_sums
};
struct CovLaunch {
  const PairJob* jobs;           // device
  const CovMember* members_tab;  // device
  int n_records, members;
  const float* T;                // device [n_records][16] poses (a rig: body poses), or null: every member's src->T_out
  const float* sigma;            // device [n_records * members], or null: src->scale
  const float* X;                // device [members][16] camera_from_body, or null: one camera per record, X = I
  int level;                     // the level of the jobs (echoed; T == null: the states' own level must equal it, else the record is BPVO_COV_NONE)
  int max_points, C, loss;
  bpvo_hip_pose_covariance* out; // device [n_records]
};
int  pose_cov_partials_floats(int cap, int C);          // floats of one member's tile partials
void launch_pose_cov_prepare(hipStream_t s, const CovLaunch& g);   // the scratch states from (T, sigma) or from the workspaces' last estimates
void launch_pose_cov_reduce(hipStream_t s, const CovLaunch& g);    // loss g.loss; members whose job carries another loss are left alone
void launch_pose_cov_finish(hipStream_t s, const CovLaunch& g);
// Pose scoring (kernels_score.hip; c_api.h bpvo_hip_score_poses): the truncated-L1 cost of n_poses poses of each of n_pairs jobs in one launch,
// one partial per (pair, chunk, pose), then the finish — the partials in chunk order, the score.  The jobs are read for their template, descriptor
// and geometry only (the host clears their workspace pointers).  `tile`: poses a workgroup walks (1 .. kScoreTile; the host sizes it so that the
// launch fills the chip) — no result depends on it.
constexpr int kScoreTile = 16;
struct ScorePartial { double cost; int n_valid, n_below; };
struct ScoreLaunch {
  const PairJob* jobs;           // device [n_pairs]
  int n_pairs, n_poses;
  int max_points;                // the most points of a job (0: every template is empty — the finish alone runs)
  int C, fast_warp, tile;
  float tau;
  const float* T;                // device [n_pairs][n_poses][16]
  ScorePartial* partials;        // device [n_pairs][score_chunks(max_points)][n_poses]
  bpvo_hip_pose_score* out;      // device [n_pairs][n_poses]
};
int  score_chunks(int max_points);      // 256-point chunks of the largest template, at least 1
void launch_score_poses(hipStream_t s, const ScoreLaunch& g);
void launch_prepare_linearize(hipStream_t s, const PairJob* job, const float* T /*device [16]*/, int reset_scale, int level, float given_scale = 0.0f);
int  gn_pts_per_block(int C);
int  gn_partials_entries(int cap, int C);   // kPartialStride-float entries of a workspace's (double-buffered) tile partials
// (C > 48: run-time channel loops over the point-major records)
void launch_weights(hipStream_t s, const PairJob* job, int n, int C, int loss, float* w_out /*[n][C]*/);
void launch_count_good(hipStream_t s, const PairJob* job, int n, int C, int loss, float thr, unsigned int* count);
// the key frame's point cloud (bpvo/vo.cc:250-281) as 32-byte records on the device; K: the level's intrinsics, img: the key frame's level-0 image
void launch_rebuild_points(hipStream_t s, const PairJob& job, float4* out);      // out[i] = load_point(job, i), i < job.n (a debug accessor)
void launch_point_cloud(hipStream_t s, const PairJob* job, int n, int C, int loss, const uint8_t* img, int rows, int cols, const float K[9], int dspace,
                        bpvo_hip_point_with_info* out);
// the same two for a table of jobs in one launch each (bpvo_hip_add_frames): counts[k] (zeroed by the caller) of entry k; max_n: the most points of an entry
void launch_count_good_batch(hipStream_t s, const PairJob* jobs, int n_jobs, int max_n, int C, int loss, float thr, unsigned int* counts);
// ... with each entry's own loss and threshold (PairJob::loss / good_thr: sequences with parameters of their own)
void launch_count_good_jobs(hipStream_t s, const PairJob* jobs, int n_jobs, int max_n, int C, unsigned int* counts);
struct CloudJob {
  const PairJob* job;       // device: the job of the key frame's last linearisation
  const uint8_t* img;       // the key frame's level-0 image
  size_t out_offset;        // first record of this entry in the output
  float K[9];               // the intrinsics of the level the estimate ended on (each sequence its own camera)
  int rows, cols;           // the size of img
  int loss;                 // the loss the weights are taken with (each sequence its own parameters)
};
void launch_point_cloud_batch(hipStream_t s, const CloudJob* jobs, int n_jobs, int max_n, int C, int dspace, bpvo_hip_point_with_info* out);
void launch_pack_records(hipStream_t s, const PairJob* jobs, int n, int L, float* records, const GNState* d_states = nullptr, GNState* h_states = nullptr,
                         const unsigned* d_ctl = nullptr, unsigned* h_ctl = nullptr, int ctl_words = 0, unsigned* zero = nullptr);   // h_states / h_ctl (pinned host): copied out by the same launch; zero: a word cleared by it
// a few pairs: job table upload (from the pinned host rows) + initial poses + cleared control words in one launch
void launch_set_pose_upload(hipStream_t s, PairJob* d_table, const PairJob* h_table, size_t table_jobs, const PairJob* h_jobs_coarsest, const float* T_init,
                            int n, unsigned* clear, int clear_words);

}  // namespace bpvo_hip
