// libbpvo_hip, host side: the context and what its translation units share (internal header; the interface is include/bpvo_hip/c_api.h).
//   context.hip   create / destroy, storage, job tables, per-context options            frames.hip    setData / setTemplate stages + accessors
//   estimate.hip  estimatePose: the Gauss-Newton drivers (chain, persistent, team)       batch.hip     pair batches, the upload pipeline
//   vo.hip        the addFrame drivers (one frame, many sequences), point cloud           measure.hip   profiling, counters, diagnostics
//                                                                                        vo_state.h    addFrame's state machine (host only, no HIP)
//                                                                                        gn_rounds.h   the chain's pipelined rounds (host only, no HIP)
//   pose_cov.hip  the pose-covariance pass behind an estimate (kernels_gn_cov.hip, pose_cov_math.h)      frame_plan.h  the frame stage's decisions (host only, no HIP)
//   rectify.hip   rectification on the device: the maps of the camera sides, the launch in front of the stereo front-end (kernels_rectify.hip, rectify_math.h)
//   disparity_fusion.hip  disparity fusion: the maps a sequence carries between its frames, the stage in front of the template stage (kernels_disparity_fusion.hip, disparity_fusion_math.h)
//   motion_stereo.hip  motion stereo: the prediction of the fusion refined against the key frame, between the fusion stage's two launches (kernels_motion_stereo.hip, motion_stereo_math.h)
//   disparity_variance.hip  measurement variance: the per-pixel variance of a stereo frame's disparities, behind the matcher (kernels_disparity_variance.hip, disparity_variance_math.h)
//   stereo.hip    the stereo front-end: parameter checks, buffers, the matchers' launches over the frames of a call, stereo_front for the addFrame drivers
//                 (kernels_stereo.hip, kernels_sgm.hip, kernels_sgbm.hip; sg_scanline.h: the semi-global matchers' scanline walk)
//   device_owned.h  the owners of every device buffer, pinned buffer, stream and event below (the only place that acquires or releases one)
// The host keeps bpvo's object model (frames with a descriptor pyramid and a template pyramid, a pose estimator with per-level
// Gauss-Newton runs, the VisualOdometry keyframe state machine) but every O(pixels) / O(points) array lives in HBM; per GN iteration the
// host sees one 4-byte "pairs still active" counter.  See DESIGN.md.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "device_owned.h"
#include "frame_plan.h"
#include "gn_rounds.h"
#include "kernels.h"
#include "latch_table.h"
#include "rig_math.h"
#include "vo_state.h"

using namespace bpvo_hip;
#include "latch_table.h"

namespace bpvo_hip_host {

using namespace bpvo_hip;


// live contexts per device: the estimation lanes of one context are streams = hardware queues, of which a process has a handful;
// a second context's lanes end up multiplexed on the same queues and LOSE (measured: 505 k instead of 666 k GN it/s for a
// 128-pair batch next to a second context), so batches only fan out over lanes while theirs is the only context on the device
extern std::atomic<int> g_live_ctx[64];
extern thread_local std::string g_create_error;   // bpvo_hip_last_error(nullptr): the failed create of THIS thread (contexts are created
                                           // concurrently by the per-GPU host threads of multi_gpu.hip)

struct LevelGeom {
  int rows, cols;
  size_t npix;
  int nblk;        // 256-pixel chunks of the row-major scan
  int cap;         // capacity of the template arrays
  int nms_radius;  // <= 0: off
  float K[9];
  float b;
};

struct FrameSlot {
  bool has_data = false, has_template = false;
  bool has_disp = false;     // the slot holds the disparity of its image (false for the current frames B of a pair batch: never uploaded)
  DeviceBuf<unsigned char> data_slab, tmpl_slab;   // the slot's storage: the pointers below are views carved from them (carve_frame_data / carve_frame_tmpl)
  uint8_t* img[kMaxLevels] = {};
  uint8_t* cen[kMaxLevels] = {};
  float* ch0[kMaxLevels] = {};
  uint8_t lazy[kMaxLevels] = {};  // levels whose descriptor records were not stored (FrameJob::lazy): 1 = census bytes + channel 0, 2 = census bytes only
  // the saliency map of a level: kept by the selection (SAL_STORED), formed on demand from the slot's data (SAL_ON_DEMAND: template frames of a pair
  // batch, option lazy_template_saliency; ensure_saliency), or gone because the data such a template was made of has been replaced (SAL_GONE)
  enum : uint8_t { SAL_STORED = 0, SAL_ON_DEMAND = 1, SAL_GONE = 2 };
  uint8_t sal_state[kMaxLevels] = {};
  bool ch0_valid = true;          // false: the descriptor of the slot's current data was computed without the compact channel-0 plane
  float* desc[kMaxLevels] = {};
  float* disp = nullptr;
  float* scratch = nullptr;   // descriptor fields: kDfPlanes work planes
  float* sal[kMaxLevels] = {};
  uint8_t* flag[kMaxLevels] = {};
  int* blk_count[kMaxLevels] = {};
  float4* pts[kMaxLevels] = {};
  float2* ptc[kMaxLevels] = {};   // compact point records (PairJob::ptc)
  int* inds[kMaxLevels] = {};
  float* pix[kMaxLevels] = {};
  float* grad[kMaxLevels] = {};
  float* nrm = nullptr;    // [L][4]
  int* n_dev = nullptr;    // [L]
  int n_host[kMaxLevels] = {};
  // the slot's camera when it is not the context's own (a sequence of bpvo_hip_add_frames with bpvo_hip_seq_set_camera / create_sequences):
  // its level geometry, sizes within the context's storage geometry; slot_geom below picks it
  bool own_geom = false;
  LevelGeom geom[kMaxLevels];
  // the algorithm parameters of the slot's sequence when they are not the context's own (bpvo_hip_seq_set_params: SeqState::params), else null;
  // the frame stages take the selection thresholds from them (make_frame_job)
  const bpvo_hip_params* seq_params = nullptr;
  // the point budget (bpvo_hip_set_point_budget): the slot's sequence's own (bpvo_hip_seq_set_point_budget) in the place of the context's; what the last
  // template stage applied per level, with the minSaliency it ran with (bpvo_hip_get_selection_info); the device record point_budget_kernel leaves
  bool own_budget = false;
  int budget[kMaxLevels] = {};
  int budget_used[kMaxLevels] = {};
  float min_saliency_used = 0.0f;
  int* sel_info = nullptr;  // [L][4]
};

struct Workspace {
  DeviceBuf<float> r;
  DeviceBuf<uint8_t> valid;
  DeviceBuf<uint32_t> cand, med_blk, tapkey;
  DeviceBuf<float> tapcache, partials;
  int last_ref = -1, last_cur = -1, last_level = -1;
  bool has_estimate = false;   // the workspace's state is that of a finished estimate (pose, scale and level of its finest level): what
                               // bpvo_hip_pose_covariances reads when no pose is given; a later linearize call on the workspace clears it
};

// Scratch of the pose-covariance pass (pose_cov.hip), allocated at its first use: `group` slots, each the residuals, valid flags, tile partials,
// counters and Gauss-Newton state of one member, so that the pass writes nothing of a workspace; the tables of a group (jobs, members, poses,
// scales, extrinsics) are staged in pinned memory and uploaded in one copy.
struct CovScratch {
  int group = 0;               // slots: min(BPVO_HIP_COV_GROUP, workspaces of the context)
  DeviceBuf<unsigned char> d_slab;                    // the d_ pointers below are views carved from it
  float* d_r = nullptr; size_t r_floats = 0;          // [group][r_floats]
  uint8_t* d_valid = nullptr; size_t valid_bytes = 0; // [group][valid_bytes]
  float* d_partials = nullptr; size_t partial_floats = 0;
  unsigned long long* d_cnt = nullptr;                // [group][kWsCounters]
  GNState* d_states = nullptr;                        // [group]
  unsigned char* d_tables = nullptr;                  // the uploaded tables, laid out as h_tables
  PinnedBuf<unsigned char> h_tables;
  size_t tables_bytes = 0, off_members = 0, off_T = 0, off_sigma = 0, off_X = 0;
  bpvo_hip_pose_covariance* d_out = nullptr;          // [group]
  PinnedBuf<bpvo_hip_pose_covariance> h_out;          // [group]
  float* d_sums = nullptr;                            // [n_pairs][72]: M and Q of the last pass on each workspace
};

// Device buffers of the pose-scoring calls (score.hip), the context's own, grown on demand: the jobs of a call's pairs, its poses, the
// per-(pair, chunk, pose) partials and the records.
struct ScoreScratch {
  DeviceBuf<PairJob> d_jobs;
  DeviceBuf<float> d_T;
  DeviceBuf<ScorePartial> d_partials;
  DeviceBuf<bpvo_hip_pose_score> d_out;
};

// Rectification (c_api.h "rectification on the device", rectify.hip): the map of one camera side — the entries of its destination pixels
// (rectify_math.h RectEntry), built on the host by a set call and uploaded once — and what the context holds for the calls: everything is
// acquired at its first use, so a context that never rectifies holds nothing.
struct RectMap {
  DeviceBuf<int2> d_map;             // [rows][cols]; empty: the side has no rectification
  int rows = 0, cols = 0;            // the destination: the camera's size when the map was set
  int raw_rows = 0, raw_cols = 0;
  uint64_t outside = 0;              // destination pixels without a full source (rectify_outside)
};
struct RectState {
  RectMap own[2];                    // the context's own camera (bpvo_hip_set_rectification): left, right
  std::vector<RectMap> seq;          // [2 * sequence capacity], made by the first bpvo_hip_seq_set_rectification: sequence s side k at 2 s + k
  DeviceBuf<uint8_t> raw[2];         // raw images of a call that came from host memory, per side of the call
  DeviceBuf<uint8_t> out;            // rectified images on their way to host memory (bpvo_hip_rectify_frames)
  // the frame table of a call (kernels.h RectifyFrame), filled in pinned memory and copied on the stream; tab_ev: behind the last copy
  PinnedBuf<RectifyFrame> h_tab; DeviceBuf<RectifyFrame> d_tab;
  Event tab_ev;
  uint64_t launches = 0, pixels = 0; // bpvo_hip_rectify_counts
  Event t0, t1; bool timed = false;   // while bpvo_hip_profiling is on: events around the last launch (option "rectify_last_kernel_ms")
};

// Disparity fusion (c_api.h "disparity fusion", disparity_fusion.hip): what a sequence carries between its frames — one slab, acquired when the
// sequence first fuses: Dc and Vc (each padded to a multiple of four pixels, so that both are 16-byte aligned) and the u64 z-buffer, zeroed
// once —, its own setting, and the record of its last fusion.  FusionState: the context's setting, the sequences (index 0 is also
// bpvo_hip_add_frame's), the job table of a stage and the class counters it leaves; everything is acquired at its first use, so a context with
// mode 0 everywhere holds nothing.
struct FusionSeq {
  bpvo_hip_disparity_fusion prm = {0, 0.0f, 0.0f, 0.0f, 0.0f};
  bool own = false;
  DeviceBuf<unsigned char> slab;
  size_t npix = 0;                 // the camera size the slab was made for
  float* Dc = nullptr; float* Vc = nullptr; unsigned long long* zbuf = nullptr;
  bool carried = false;            // the maps hold a frame (false: fresh, after bpvo_hip_seq_reset)
  bpvo_hip_disparity_fusion_info info = {};
};
struct FusionState {
  bpvo_hip_disparity_fusion prm = {0, 0.0f, 0.0f, 0.0f, 0.0f};
  std::vector<FusionSeq> seq;      // [max(1, sequence capacity)], made by the first setter that turns mode 1 on
  int n_on = 0;                    // sequences that run in mode 1 right now (0: no driver asks any further)
  PinnedBuf<FusionJob> h_jobs; DeviceBuf<FusionJob> d_jobs;
  PinnedBuf<unsigned> h_counts; DeviceBuf<unsigned> d_counts;      // [jobs][DF_CLASSES] of the last stage
  Event done_ev;                   // behind the last stage's copy of the counters
  std::vector<int> pending;        // the sequences of the last stage, whose counters are still on their way
  uint64_t launches = 0, pixels = 0;
  Event t0, t1, t2; bool timed = false;   // while bpvo_hip_profiling is on: events around the last stage's two launches
};

// Measurement variance (c_api.h "measurement variance", disparity_variance.hip): the context's setting and the sequences' own (index 0 is also
// bpvo_hip_add_frame_stereo's), where a sequence's last map lies in c->st_var, the job table of a launch and the counters it leaves.  Everything
// is acquired at its first use: a context with mode 0 everywhere, or without fusion, holds nothing.
struct VarianceSeq {
  bpvo_hip_measurement_variance prm = {0, 0, 0.0f, 0.0f, 0.0f};
  bool own = false;
  bool has = false;                // a stereo call has made a map for the sequence since its last reset
  size_t offset = 0, npix = 0;     // where in c->st_var, while serial is the state's
  uint64_t serial = 0;
  bpvo_hip_measurement_variance_info info = {};
};
struct VarianceState {
  bpvo_hip_measurement_variance prm = {0, 0, 0.0f, 0.0f, 0.0f};
  std::vector<VarianceSeq> seq;    // [max(1, sequence capacity)], made by the first setter that turns mode 1 on
  int n_on = 0;                    // sequences whose setting is mode 1 right now
  bool live = false;               // the stereo call under way has maps in c->st_var (variance_map_of)
  uint64_t serial = 0;             // moves whenever c->st_var is rewritten
  PinnedBuf<VarianceJob> h_jobs; DeviceBuf<VarianceJob> d_jobs;
  PinnedBuf<unsigned> h_counts; DeviceBuf<unsigned> d_counts;      // [jobs][kVarianceCounters] of the last launch
  Event done_ev;                   // behind the last launch's copy of the counters
  std::vector<int> pending;        // the sequences of the last launch (-1: a stand-alone pair), whose counters are still on their way
  DeviceBuf<float> fuse_var;       // bpvo_hip_fuse_disparities_var: a host caller's maps
  uint64_t launches = 0, pixels = 0, tiles[3] = {0, 0, 0};
  Event t0, t1; bool timed = false;   // while bpvo_hip_profiling is on: events around the last launch (option "variance_last_kernel_ms")
};

// Motion stereo (c_api.h "motion stereo", motion_stereo.hip): the context's setting and the sequences' own (index 0 is also bpvo_hip_add_frame's),
// the record of a sequence's last frame, the job table of a launch and the counters it leaves.  Everything is acquired at its first use: a
// context with mode 0 everywhere, or without fusion, holds nothing.
struct MotionStereoSeq {
  bpvo_hip_motion_stereo prm = {0, 0, 0, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  bool own = false;
  bpvo_hip_motion_stereo_info info = {};
};
struct MotionStereoState {
  bpvo_hip_motion_stereo prm = {0, 0, 0, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  std::vector<MotionStereoSeq> seq;   // [max(1, sequence capacity)], made by the first setter that turns mode 1 on
  int n_on = 0;                       // sequences whose setting is mode 1 right now
  PinnedBuf<MotionStereoJob> h_jobs; DeviceBuf<MotionStereoJob> d_jobs;
  PinnedBuf<unsigned> h_counts; DeviceBuf<unsigned> d_counts;      // [jobs][kMotionStereoCounters] of the last launch
  Event done_ev;                      // behind the last launch's copy of the counters
  std::vector<int> pending;           // the sequences of the last launch (-1: a stand-alone pair), whose counters are still on their way
  DeviceBuf<unsigned char> frames_in, frames_out;      // bpvo_hip_motion_stereo_frames: a host caller's inputs and outputs
  uint64_t launches = 0, pixels = 0, tiles[3] = {0, 0, 0}, classes[7] = {0, 0, 0, 0, 0, 0, 0};
  Event t0, t1; bool timed = false;   // while bpvo_hip_profiling is on: events around the last launch (option "motion_stereo_last_kernel_ms")
};

enum KernelClass { KC_PYRAMID = 0, KC_DESCRIPTOR, KC_SALIENCY_SELECT, KC_NORMALIZATION, KC_TEMPLATE, KC_WARP_RESIDUAL, KC_MEDIAN,
                   KC_IRLS_REDUCE, KC_GN_STEP, KC_POINT_BUDGET, KC_COUNT };
static const char* const kKernelNames[KC_COUNT] = {"pyramid", "descriptor", "saliency_select", "normalization", "template_build", "warp_residual",
                                      "median", "irls_reduce", "gn_step", "point_budget"};

struct EventPair { Event a, b; int kc; double units; };

// An estimation lane: one HIP stream plus the host staging it needs.  Batches of independent pairs are split over
// several lanes driven by their own host threads, so that the narrow per-pair kernels of one group (median select,
// gn_step: one workgroup per pair) overlap with the chip-filling kernels (warp_residual, irls_reduce) of another.
struct Lane {
  hipStream_t stream = nullptr;    // the context's stream (lane 0) or own_stream
  Stream own_stream;
  PinnedBuf<PairJob> h_pjobs;      // [L][n_pairs]
  DeviceBuf<PairJob> d_pjobs;      // [L][n_pairs]
  PinnedBuf<float> h_T;            // [n_pairs][16]
  DeviceBuf<float> d_Tinit;
  DeviceBuf<int> d_active;         // [3][2] per round in flight: entries of the active list, and how many of them still estimate their scale
  DeviceBuf<int> d_list;           // [3][n_pairs] active-workspace lists of the host rounds in flight (ActiveSet)
  PinnedBuf<int> h_active;         // [3][2]
  Event round_ev[3];               // "compaction of round r and its count have landed"
  Event staging_ev[2];             // "the upload of this lane's rows of FrameJob table 0 / 1 has left the pinned staging"
  Event selected_ev;               // staggered batches: "the selection of this lane's templates has been queued" (FrameRun)
  DeviceBuf<unsigned> d_pk_ctl;    // [kMaxLevels][kPkCtlWords] {arrivals, abort} of the persistent kernel, one slot per level
  PinnedBuf<unsigned> h_pk_ctl;    // its host copy
  DeviceBuf<unsigned> d_team_ctl;  // gn_team_ctl_words(kMaxTeams) words of the team-persistent kernel (lane 0 only)
  PinnedBuf<unsigned> h_team_ctl;  // host copy of its first line (abort word)
  PinnedBuf<GNState> h_states;     // [n_pairs + n_pairs]: the workspaces' states, then the body states of rig mode (estimate_rigs)
  std::vector<EventPair> ev_pending;
  std::vector<Event> ev_pool;
  unsigned k6_seq = 0;             // warp_residual launches of this lane since bpvo_hip_profiling (event sampling)
  std::string err;
};
// Estimation lanes (streams driven by host threads) of a batch: the narrow per-pair kernels (median_finish, gn_step: one
// workgroup / wave per pair) of one lane overlap the chip-filling kernels of the other.  Two lanes: +2 % at 1024 pairs of
// 1241x376 bit-planes, +3.7 % at 128, +7 % for 640x480 intensity; four lanes lose at every size.  Per-launch durations of
// overlapping lanes include the time shared with the other lane: measurements that need clean per-kernel times run with
// bpvo_hip_set_max_lanes(ctx, 1) / BPVO_HIP_LANES=1.  Results do not depend on the number of lanes (test_gpu_parity.py).
constexpr int kDefaultLanes = 3;          // C = 8: +1 ... +2.6 % over two at 128 - 512 pairs and at 640x480, +0.5 % at 1024 (profiles/r04_small_batch_model.txt); C = 1: -2 %
constexpr int kDefaultLanesNarrow = 2;
constexpr int kMinPairsPerLane = 8;
constexpr int kPkCtlWords = 32;    // one 128-byte line per level
constexpr int kMaxTeams = 1024;

}  // namespace bpvo_hip_host

using namespace bpvo_hip;
using namespace bpvo_hip_host;

struct bpvo_hip_ctx {

  bpvo_hip_params params;
  int point_budget[kMaxLevels] = {};   // bpvo_hip_set_point_budget: template points a level keeps at most, the most salient first (0: no budget)
  // bpvo_hip_set_intensity_normalization: -1 off, 0 whole image, 1 .. 15 local (intensity_norm_math.h); d_inorm [n_frames][L]: the whole-image
  // form's scratch per (slot, level), held only while the radius is 0
  int inorm_radius = -1;
  DeviceBuf<InormScratch> d_inorm;
  bpvo_hip_start_policy start_policy = {BPVO_START_KEYFRAME_POSE, -1, 0.0f};   // bpvo_hip_set_start_policy: where the addFrame drivers start (vo_state.h); bodies without their own run it
  float K[9];
  float baseline;
  int rows, cols, L, C, device;
  bool auto_levels = false;     // numPyramidLevels <= 0 at creation: L is the automatic count of the image size (bpvo/vo.cc:101-105)
  int n_frames, n_pairs;
  LevelGeom geom[kMaxLevels];
  float gauss_k[3];
  GaussTaps df_g1, df_g2;       // imsmooth kernels of dfSigma1 / dfSigma2 (descriptor fields); n = 0: sigma <= 0
  GaussTaps cd_before, cd_after; // imsmooth kernels of centralDifferenceSigmaBefore (u8 fixed point) / After (f32)
  GaussTaps grad_pre;           // cv::GaussianBlur(Size(), sigma) of GradientDescriptor (sigmaPriorToCensusTransform > 0)
  GaussTaps latch_after;        // imsmooth(1.75) of every LATCH channel (bpvo/latch_descriptor.cc:1082)
  int latch_taps[2] = {0, 0};   // fixed-point {centre, side} taps of LATCH's cv::GaussianBlur(Size(3,3), 2, 2) (:147)
  DeviceBuf<signed char> d_latch_off;   // [48 * latchNumBytes] triplet coordinates as CalcuateSums uses them (:170-236)
  int scratch_planes = kDfPlanes;   // work planes of FrameSlot::scratch
  bool plane_scratch = false; // descriptor built from plane operations (descriptor fields, central difference, smoothed gradient)
  Stream stream;
  std::vector<FrameSlot> frames;
  std::vector<Workspace> ws;
  DeviceBuf<GNState> d_states;
  DeviceBuf<FrameJob> d_fjobs;     // [2][L][n_frames]: the table of the setData stage, then the one of the setTemplate stage
  std::vector<Lane> lanes;         // lanes[0] shares the ctx stream
  DeviceBuf<PairJob> d_job1;       // scratch single job (linearize / weights)
  DeviceBuf<float> d_records;      // [n_pairs][kRecordFloats]
  DeviceBuf<float> d_wtmp;         // [cap_max * C] weights scratch
  DeviceBuf<unsigned int> d_count;
  DeviceBuf<unsigned> d_tickets;             // [n_pairs] PairJob::ticket
  DeviceBuf<unsigned long long> d_counters;   // [4] points, linearisations, bracketed / full median selections
  // pinned staging
  PinnedBuf<FrameJob> h_fjobs;
  PinnedBuf<int> h_ints;           // [max(n_frames*kMaxLevels, 16)]
  DeviceBuf<int> d_ints;           // same size, device
  int cap_max = 0;
  SeqState vo;                     // bpvo_hip_add_frame's VisualOdometry state (vo_state.h) on frame slots 0 .. 2 and workspace 0
  DeviceBuf<bpvo_hip_point_with_info> d_cloud;   // the last key frame's point cloud: built on the device (vo.hip build_point_cloud), copied out when asked for
  // many independent VisualOdometry sequences (bpvo_hip_add_frames, vo.hip): vo_mode 0 = not yet decided, 1 = bpvo_hip_add_frame, 2 = bpvo_hip_add_frames
  int vo_mode = 0;
  std::vector<SeqState> seqs;                      // [seq_capacity], created by the first bpvo_hip_add_frames
  DeviceBuf<bpvo_hip_point_with_info> d_seq_cloud; // [seq_capacity][geom[maxTestLevel].cap] point clouds
  PinnedBuf<PairJob> h_seq_jobs;                   // [seq_capacity]: the jobs of the fraction-of-good-points count and the point clouds
  DeviceBuf<PairJob> d_seq_jobs;
  PinnedBuf<CloudJob> h_cloud_jobs;                // [seq_capacity]
  DeviceBuf<CloudJob> d_cloud_jobs;
  PinnedBuf<unsigned> h_seq_cnt;                   // [seq_capacity]: good-point counters
  DeviceBuf<unsigned> d_seq_cnt;
  PinnedBuf<size_t> h_seq_off;                     // [seq_capacity]: pixel offsets of the frames of a mixed-size call in the packed device inputs
  DeviceBuf<size_t> d_seq_off;
  // Rig mode (bpvo_hip_rig_set / bpvo_hip_rigs_set ... bpvo_hip_add_frames_rig(s), vo.hip): rigs[r] (RigState below) = the cameras of one rigid rig,
  // estimated as one body pose.  A context with a rig (rigs not empty) serves bpvo_hip_add_frames_rig(s) only.
  std::vector<RigState> rigs;
  DeviceBuf<float> d_rig_X;        // [n_pairs][16], allocated at its first use (bpvo_hip_linearize_rig)
  // estimate_rigs' staging (rig_stage_bytes: the rigs' table, extrinsics, initial poses — one upload per estimate) and the bodies' `active` words
  // of a round (device [n_pairs]; pinned [3][n_pairs], a row per round in flight); allocated at their first use
  DeviceBuf<char> d_rig_stage; PinnedBuf<char> h_rig_stage;
  DeviceBuf<int> d_rig_active; PinnedBuf<int> h_rig_active;
  // Pose covariance (c_api.h bpvo_hip_pose_covariances, pose_cov.hip).  Option "pose_covariance": the addFrame entry points run the pass behind
  // the estimate their result's pose comes from and keep the record — vo_cov for bpvo_hip_add_frame, seq_cov[s] per sequence, RigState::cov per rig.
  int pose_covariance = 0;
  CovScratch cov;
  bpvo_hip_pose_covariance vo_cov;
  std::vector<bpvo_hip_pose_covariance> seq_cov;
  ScoreScratch score;              // pose scoring (c_api.h bpvo_hip_score_poses, score.hip)
  // measurement
  double points_fused = 0;     // points linearised through the fused path since the last counter reset
  int fast_warp = 0;           // bpvo_hip_set_warp_formulation
  int dspace = 0;              // BPVO_WARP_DISPARITY_SPACE_F32: DisparitySpaceWarp as the warp (implies fast_warp)
  int fuse_frozen = 1;         // estimate loops: fused residual + reduction once a workspace's scale is frozen (bit-identical,
                               // +3 % GN iterations/s).  Option "fuse_frozen".  (C = 8: ONE irls_reduce launch serves the plain and
                               // the fused workspaces with a per-workspace branch; the two-launch form measured slower at every batch size, round 2)
  int G = 1, Cg = 0;           // channel groups of a wide descriptor (C > 48: C = G x Cg, Cg one of the channel counts the per-point kernels are built for;
                               // types.h PairJob::pitch); G = 1: none
  int reference_reduction = 0; // option "reference_reduction" (validation mode): H, G and the squared norm summed in the reference's index order in f32
                               // (kernels_gn_ref.hip) — the four-kernel chain only, no fused path, no step inside the reduction, no persistent / team kernel
  int step_in_reduce_max = 128; // groups of up to this many pairs run the four-kernel chain as three: the last tile of a workspace in irls_reduce takes
                               // the Gauss-Newton step (gn_step.h gn_last_tile; same sums in the same order).  Worth +2 % at 64 pairs per lane (the
                               // 128-pair shard), nothing at 128, -3 % at 512: the first wave of every tile waits for its write-through store and its
                               // ticket.  Option "step_in_reduce_max_pairs" (0: never)
  // Groups of at most persist_max_ws workspaces (a single pair: sequential addFrame) run every pyramid level in ONE persistent
  // launch (kernels_gn.hip, gn_persistent_kernel) instead of rounds of four kernels per iteration; bit-identical results.
  // Options "persistent" (0 turns it off), "persist_max_ws", "persist_grid" size it.  persistent_failed: a launch gave up at a barrier
  // (workgroups not co-resident) — the context stays on the four-kernel chain from then on.
  int persistent = 1, persist_max_ws = 1, persist_grid = 64;
  int persist_max_points = 32768;     // option "persist_max_points": a level with more template points than this — and the finer levels behind it — takes the
                               // four-kernel chain even for a single pair: the persistent kernel's grid (64 workgroups) wins on the 6 - 26 k points of a
                               // template with non-maximum suppression and loses on dense ones (8 channels: 30.7 against 32.1 us per linearisation at 16 k
                               // points, 59.8 against 49.0 at 38 k, 220 against 134 at 280 k; one channel: equal at 40 k; scripts/persist_crossover.py).
                               // Default 32768 for eight channels, 65536 for one (set at creation).
  // option "dense_candidates_from": chain launches over a level of at least this many template points keep the exact median's candidates
  // in ONE run per workspace (kernels.h, GNLaunch::dense_candidates) — the finish of a 300 k-point level walked 1172 segments, 120 us where the
  // run takes 10.  Not for channel groups (their jobs hold their own counters).
  int dense_candidates_from = 32768;
  long long persist_timeout = 50000000ll;   // ticks of the 100 MHz wall clock a grid barrier waits before it gives up (0.5 s)
  // Batches of 2 .. team_max_pairs pairs run their whole Gauss-Newton stage in ONE launch of the team-persistent kernel
  // (kernels_gn.hip, gn_team_kernel): teams of team_size workgroups, one workgroup per CU, a pair per team at a time.
  // Options "team" (0 turns it off), "team_max_pairs", "team_size" (0 = CUs / pairs), "team_cus" (CUs the grid may claim: tests).
  int team_mode = 1, team_max_pairs = 128, team_full_pairs = 80, team_size_env = 0, num_cus = 0, device_cus = 0;   // (team_full_pairs: up to here whatever the fill)
  int team_join = 2;             // option "team_join": workgroups of a team that has run out of pairs join the teams still at work (kernels_gn_team.hip
                                 // pk_join_team): 0 never, 1 teams on the workgroup's own XCD, 2 any team
  int merge_levels_max_frames = 8;   // option "levels_in_one_launch_max_frames": frame stages of at most this many frames run the levels of the
                                 // bit-planes, selection and template-build kernels in one launch each (frames.hip)
  int small_batch_fused = 1;     // option "small_batch_fused": contexts of a few pairs — job table + poses in one launch, states copied out by pack_records (estimate.hip)
  int nrm_dpp_asm = 4;           // option "normalization_form": the sequential Hartley sums (kernels_frame.hip) as 1: hand-scheduled DPP add chains (170 us for a
                                 // 1241x376 template, 2.28 ms for a dense 640x480 one), 0: the compiler's DPP form (281 us / 3.6 ms), 2: broadcast LDS reads +
                                 // plain adds, no cross-lane traffic and no asm (311 us / 4.0 ms: the compiler's loop does not keep the adds back to back), 3: the
                                 // same reads with the adds as asm blocks of plain v_add_f32 on a wave that does nothing else (170 us / 2.04 ms), 4 (the default):
                                 // 3 for launches of at most 1024 workgroups, 1 for larger ones
  int nrm_side_stream = 1;       // option "normalization_side_stream": frames.hip frames_set_template
  int nrm_defer = 1;             // option "normalization_deferred": ... and the sums of the levels below the coarsest run on under the coarsest level's iterations
  int team_split_max_pairs = 4;  // option "team_split_max_pairs": team batches of up to this many pairs run the coarsest level in a launch of its own, the deferred
                                 // normalisation under it (estimate.hip)
  // the normalisation's streams (created at their first use) and their events: [0] fork, [1] coarsest level done (or all), [2] the levels between the
  // coarsest and the finest done, [3] the finest level done.  Deferred form: the finest level — the long one: 2.3 ms of dependent adds for a dense
  // 640x480 template — has a stream of its own, so that the levels above it are ready, and their Gauss-Newton iterations run, while it is still adding.
  Stream side_stream, side_stream2;
  Stream copy_stream;      // addFrame's disparity upload (frames.hip upload_disparity); created at its first use, with its event
  Event copy_ev;
  // run once by the estimation of a group on the context's stream right before its final synchronisation, i.e. with every kernel of the estimate
  // queued (estimate.hip): addFrame's disparity upload
  std::function<int()> before_final_sync;
  int vo_disparity_late = 1;      // option "vo_disparity_late": addFrame uploads a host frame's disparity under the queued estimate (1) or in its data stage (0)
  Event side_ev[4];
  hipEvent_t nrm_pending = nullptr;   // non-null: recorded behind the normalisation of the levels between the coarsest and the finest of the template stage just
                                 // queued; whoever reads those levels' (scale, centroid) next makes its stream wait for it (estimate.hip) and clears it
  hipEvent_t nrm_pending_finest = nullptr;   // ... and behind the finest level's
  int team_spares = 1;           // option "team_spares": the team kernel's grid fills the chip, the workgroups beyond the teams join them (growing form only)
  int team_join_from_pairs = 48; // option "team_join_from_pairs": smaller batches run the fixed-size team kernel (A/B: profiles/r05_team_join.txt)
  int team_local_barriers = 1;   // option "team_local_barriers": kernels_gn_team.hip pk_team_barrier mode 2 for teams on one XCD (0: agent-scope fences always)
  std::atomic<uint64_t> team_launches{0};
  std::atomic<uint64_t> team_joins{0};            // workgroups that left a team without pairs and joined one at work (measurement)
  std::atomic<bool> persistent_failed{false};      // (atomics: estimate_group runs on the lane threads)
  std::atomic<uint64_t> persistent_levels{0};      // levels run by the persistent kernel (measurement)
  // bpvo_hip_estimate_pose_trace: while trace_ws >= 0 the jobs of that workspace carry the device trace buffer
  DeviceBuf<float> d_trace;    // [records][kTraceFloats]
  int trace_ws = -1;
  int max_lanes_now = 1 << 30; // bpvo_hip_set_max_lanes: measurement runs that need per-launch timings without overlap
  // stereo front-end scratch (st_pixels each: the most pixels a call has held, the sum over its frames): raw and pre-filtered u8 pairs, f32 disparities
  DeviceBuf<uint8_t> st_left, st_right, st_left_pre, st_right_pre;
  DeviceBuf<float> st_disp;
  DeviceBuf<float> st_var;       // the measurement-variance maps of a call, packed like st_disp; acquired when the feature first runs (disparity_variance.hip)
  size_t st_pixels = 0;
  DeviceBuf<unsigned char> st_sgm;      // scratch of the semi-global matchers (cost volumes: the largest frame x disparity range x frames per launch seen)
  // calls whose frames differ in size: the block matcher's frame table (kernels.h StereoFrame), filled in pinned memory and copied on the
  // stream; st_tab_ev: behind the last copy (the pinned rows are rewritten only once it has passed)
  PinnedBuf<StereoFrame> h_st_frames; DeviceBuf<StereoFrame> d_st_frames;
  Event st_tab_ev;
  // option "stereo_frames_per_launch": SGM frames of one size that go through each kernel together; 0: as many as fit a third of the device
  // memory that was free when the SGM scratch was first needed (st_sgm_budget, read once per context), 1: one after the other, k: at most k
  int stereo_frames_per_launch = 0;
  size_t st_sgm_budget = 0, st_free_seen = 0;
  int st_frames_per_launch_seen = 0;      // what the last SGM launch used (measurement: option "stereo_frames_per_launch_seen")
  RectState rect;                         // rectification on the device (rectify.hip)
  FusionState fusion;                     // disparity fusion (disparity_fusion.hip)
  VarianceState variance;                 // measurement variance (disparity_variance.hip)
  MotionStereoState motion_stereo;        // motion stereo (motion_stereo.hip)
  // Upload pipeline of pair batches handed over in HOST buffers (bpvo_hip_batch_run, on_device = 0): worker threads stage chunks of
  // kUploadChunkPairs pairs in pinned memory and copy them on a stream of their own into a device staging area, chunk after chunk in lane
  // order, while the lanes already work on the chunks that have landed (upload_pipeline below).  Option "upload_workers" (0 = off).
  // Fixed by measurement (profiles/r03_host_buffers_tuning.txt, r03_host_timeline.txt): a lane's frame stage takes kUploadGroup chunks at
  // once (16-pair launches are too small to fill the chip), one group per lane, and ONE copy stream shared by the workers — a process has a
  // handful of hardware queues and HIP streams are multiplexed onto them: with a stream per worker the lanes' kernels queued behind other
  // workers' copies and nothing ran until the last chunk had landed.  While a pipeline runs the lanes' small control tables are copied by
  // a kernel from their pinned rows (a hipMemcpyAsync waits its turn behind 45 MB chunk copies in the DMA engines).
  int up_workers = 6;
  std::atomic<bool> ctl_by_kernel{false};
  Stream up_stream;                      // the workers' one copy stream
  std::vector<PinnedBuf<uint8_t>> up_pinned;   // [worker]: 2 slots of up_slot_bytes
  std::vector<Event> up_slot_free;       // [worker * 2 + slot]
  std::vector<Event> up_chunk_done;      // pool, one per chunk of a call
  size_t up_slot_bytes = 0;
  DeviceBuf<uint8_t> up_d_img;           // device staging: images [2 n][npix]
  DeviceBuf<float> up_d_disp;            //                 disparities of the A frames [n][npix]
  // host batches on two lanes: the pairs are cut into a SMALL first group (lane 0 starts its Gauss-Newton stage while most of the batch
  // is still crossing the bus), a large second one for lane 1, and the rest for lane 0 again (host_groups_plan); fractions of the batch
  double up_plan[2] = {0.19, 0.50};      // options "upload_plan_first" / "upload_plan_second"; first = 0: two equal groups.  Measured: profiles/r03_host_buffers_plan.txt
  int points_from_compact = 0;           // option "points_from_compact_stream" (debug): bpvo_hip_get_points returns load_point's rebuilt points
  int lazy_template = 1;                 // option "lazy_template_descriptor": the template frames (A) of a pair batch keep census bytes + channel 0 at the NMS
                                         // levels instead of 32-byte records nobody reads (bit-planes, CD3); template_build forms its stencils from the census
  int lazy_saliency = 1;                 // option "lazy_template_saliency" (needs lazy_template_descriptor): such levels keep the census bytes ONLY — census_kernel
                                         // writes them, the blur runs over the dense tile columns alone, the tiled selection forms channel 0 of its windows from
                                         // the census bytes and does not store the saliency map (bpvo_hip_get_saliency forms it on demand)
  int keep_current_disparity = 0;        // option: pair batches store the disparity of the CURRENT frames (B) too, so that a B slot can be made
                                         // a template later (frames_set_template); off by default: 1.9 GB per 1024-pair step never read
  double up_last_seconds = 0.0;          // wall time the workers of the last call needed for all chunks (measurement)
  size_t up_last_bytes = 0;
  bool counted_live = false;   // this context is in g_live_ctx
  // addFrame: the fraction of good points (should_keyframe's last criterion) is queued right behind the estimation, before the host
  // waits for the pose, instead of in a second round trip; frac_* hold it for fraction_good (same kernels, same count)
  float prefetch_frac_thr = -1.0f;    // >= 0 while bpvo_hip_add_frame runs its estimate
  bool frac_valid = false; int frac_ws = -1; float frac_thr = 0.0f; unsigned frac_cnt = 0; int frac_n = 0;
  double tapcache_max_density = 0.5;   // option: levels with more template points per pixel than this run without the tap cache (batches)
  bool stagger = true;         // option (0: batches run stage by stage over all pairs instead of lane by lane, batch_run_staggered)
  int stagger_min_pairs = 192; // ... for batches of at least this many pairs: below, the lanes' short frame stages are not worth their serialisation
                               // (128 pairs on three lanes: +4.5 % without, +1.4 % with).  Option "stagger_min_pairs"
  int census_taps[2] = {0, 0}; // fixed-point {centre, side} taps of the 3x3 u8 blur before the census (sigma_ct > 0)
  bool profiling = false;      // HIP events around warp_residual (the roofline kernel) and the frame stages
  bool profile_all = false;    // ... and around every GN kernel (diagnostics; costs ~10 % throughput)
  bool profile_k6_all = false; // level 3: events around EVERY warp_residual launch (and nothing else in the loop): bench.py's roofline pass
  double kc_ms[KC_COUNT] = {};
  double kc_units[KC_COUNT] = {};
  uint64_t kc_launches[KC_COUNT] = {};
  uint64_t total_lin = 0, median_bracketed = 0, median_full = 0;
  uint64_t tscale_stages = 0, tscale_passes = 0;      // runs of the Student-t scale stage and the passes of its iteration (PairJob::cnt[11], [9])
  uint64_t tap_counts[4] = {};
  std::mutex units_mu;         // kc_units updates of concurrent frame stages
  std::string err;
};

namespace bpvo_hip_host {

#define HIP_CK(ctx_, expr)                                                                  \
  do {                                                                                      \
    hipError_t e_ = (expr);                                                                 \
    if(e_ != hipSuccess) {                                                                  \
      (ctx_)->err = std::string(#expr) + ": " + hipGetErrorString(e_);                      \
      return BPVO_ERR_DEVICE;                                                               \
    }                                                                                       \
  } while(0)

// (an early return must not leave work in flight that still reads the lane's pinned staging: drain the stream first)
#define LANE_CK(ln_, expr)                                                                  \
  do {                                                                                      \
    hipError_t e_ = (expr);                                                                 \
    if(e_ != hipSuccess) {                                                                  \
      (ln_)->err = std::string(#expr) + ": " + hipGetErrorString(e_);                       \
      (void) hipStreamSynchronize((ln_)->stream);                                           \
      return BPVO_ERR_DEVICE;                                                               \
    }                                                                                       \
  } while(0)

// the automatic pyramid level count of an image size (numPyramidLevels <= 0; bpvo/vo.cc:101-105)
inline int auto_pyramid_levels(int rows, int cols, int minImageDimensionForPyramid)
{
  return 1 + (int) std::round(std::log2(std::min(rows, cols) / (double) minImageDimensionForPyramid));
}

// HIP events around a kernel class on a lane's stream (measurement; resolved by resolve_events)
Event take_event(Lane* ln);
struct ScopedTimer {
  Lane* ln;
  EventPair ep;
  bool on;
  hipStream_t st;      // the stream the timed launches go to: the lane's own, or another one that is joined into it before the lane is synchronised (the side stream)
  ScopedTimer(bpvo_hip_ctx* c_, int kc, double units, Lane* lane = nullptr, bool sampled = true, hipStream_t stream = nullptr)
      : ln(lane ? lane : &c_->lanes[0]), on(c_->profiling && sampled), st(stream ? stream : (lane ? lane : &c_->lanes[0])->stream)
  {
    if(!on) return;
    ep.kc = kc; ep.units = units;
    ep.a = take_event(ln); ep.b = take_event(ln);
    (void) hipEventRecord(ep.a, st);
  }
  ~ScopedTimer()
  {
    if(!on) return;
    (void) hipEventRecord(ep.b, st);
    ln->ev_pending.push_back(std::move(ep));
  }
};

// ---- frame stages ---------------------------------------------------------------------------------------------------
// A frame stage runs either on the ctx stream (single frames, batches on one lane) or, for staggered batches, on a lane's own stream
// with its own rows [tab, tab + count) of the job tables and count staging (FrameRun); errors of a lane go to the lane's string.
struct FrameRun {
  hipStream_t stream;
  Lane* ln;          // timing events are taken from / queued on this lane
  int tab;           // first row of the FrameJob table [L][n_frames] and of h_ints / d_ints [n_frames][kMaxLevels] used by this run
  bool own_thread;   // run by a lane thread next to others: no resolve_events, errors into ln->err
  hipEvent_t selected_ev;   // recorded once the selection of all levels has been queued (the next lane's frame stage starts behind it), or null
  std::function<void()> on_selected;   // ... and called right after that record (releases the next lane's host thread)
  // a template stage whose estimation follows on the same stream inside the same call (bpvo_hip_batch_run on one lane):
  bool defer_finest_nrm = false;       // the normalisation of every level but the coarsest stays on the side streams: ctx->nrm_pending / nrm_pending_finest, joined by the estimation
  bool no_final_sync = false;          // no host synchronisation at the end of the stage
  // frames_set_data from host buffers (addFrame): the disparity — which nothing of the data stage or of the estimate reads — is not copied by the stage;
  // the caller uploads it (upload_disparity, frames.hip) once the estimate is queued, so that the copy's hold on the host lies under the GPU's work
  bool skip_disparity_upload = false;
};
#define FR_CK(c_, fr_, expr)                                                                \
  do {                                                                                      \
    hipError_t e_ = (expr);                                                                 \
    if(e_ != hipSuccess) {                                                                  \
      ((fr_).own_thread ? (fr_).ln->err : (c_)->err) = std::string(#expr) + ": " + hipGetErrorString(e_); \
      return BPVO_ERR_DEVICE;                                                               \
    }                                                                                       \
  } while(0)

// the level geometry of a camera (bpvo/vo_frame.cc:21-28: K *= 0.5, K(2,2) = 1, b *= 2; pyrDown sizes; the NMS rule of template_data.cc:43-49;
// the template capacity) — the one derivation for bpvo_hip_create, bpvo_hip_create_sequences and bpvo_hip_seq_set_camera.  Returns nullptr, or
// why it is unsupported (a level under 8 pixels).
const char* level_geometry(const float K[9], float baseline, int rows, int cols, int L, const bpvo_hip_params& p, LevelGeom* g);
// bpvo_hip_create; min_caps (bpvo_hip_create_sequences): per level, a template capacity the context must hold at least
int create_impl(bpvo_hip_ctx** out, const float K[9], float baseline, int rows, int cols, const bpvo_hip_params* p, int device, int n_frames, int n_pairs,
                const int* min_caps);
// a frame slot's geometry at level l: its camera's, or the context's
inline const LevelGeom& slot_geom(const bpvo_hip_ctx* c, const FrameSlot& f, int l) { return f.own_geom ? f.geom[l] : c->geom[l]; }
// a frame slot's point budget at level l: its sequence's, or the context's
inline int slot_budget(const bpvo_hip_ctx* c, const FrameSlot& f, int l) { return f.own_budget ? f.budget[l] : c->point_budget[l]; }
// BPVO_OK, or why max_points [n_levels] is no budget of this context (0 or at least 16 per level: fewer would always give an empty template)
int check_point_budget(bpvo_hip_ctx* c, const int* max_points, int n_levels);

// ---- shared between the translation units (definitions: see the table at the top)
int fail(bpvo_hip_ctx* c, int code, const char* msg);
void gaussian_kernel5(double sigma, float k[3]);
void gaussian_taps(int n, double sigma, GaussTaps* g);
int imsmooth_taps(float sigma);
int auto_gauss_taps_f32(float sigma);
void carve_frame_data(bpvo_hip_ctx* c, FrameSlot& f, unsigned char* base, size_t* total);
void carve_frame_tmpl(bpvo_hip_ctx* c, FrameSlot& f, unsigned char* base, size_t* total);
hipError_t ensure_template_storage(bpvo_hip_ctx* c, FrameSlot& f, hipStream_t stream);      // a slot without template storage gets it, zeroed on `stream`
FrameJob make_frame_job(bpvo_hip_ctx* c, FrameSlot& f, int l);
PairJob make_pair_job(bpvo_hip_ctx* c, int ws, int ref, int cur, int l);      // (with the context's parameters)
void pair_job_set_params(PairJob& j, const bpvo_hip_params& p);              // ... and a sequence's own in their place
void resolve_events(bpvo_hip_ctx* c);
FrameRun ctx_run(bpvo_hip_ctx* c);
// the frame stages over any list of slots (strided_slots: slots[i] = first + i * stride)
std::vector<int> strided_slots(int first, int stride, int count);
int upload_frame_jobs(bpvo_hip_ctx* c, const int* slots, int count, const FrameRun& fr, int which, const FrameJob** tab);
// the launch of a stage's kernels over the levels of `span` (frame_plan.h) of `count` frames, from the stage's table and level sizes: the jobs and
// the size of the span's FINEST level, which the grid of a launch over several levels is made for
inline bpvo_hip::FrameLaunch frame_launch(const bpvo_hip_ctx* c, const FrameJob* tab, const LevelGeom* geom, LevelSpan span, int count)
{
  return bpvo_hip::FrameLaunch{tab + (size_t) span.first * c->n_frames, geom[span.first].cols, geom[span.first].rows, count, span.count, c->n_frames};
}
// offsets: null, or the pixel offset of each entry's image / disparity in `images` / `disps` (otherwise entry i is at i x its level-0 pixels).  Every
// slot of one stage has the same sizes (slot_geom); mixed sizes run a stage per size
int frames_set_data_slots(bpvo_hip_ctx* c, const int* slots, int count, const uint8_t* images, const float* disps, bool on_device, const FrameRun& fr,
                          int skip_odd_disp = 0, const size_t* offsets = nullptr);
int frames_set_template_slots(bpvo_hip_ctx* c, const int* slots, int count, const FrameRun& fr);
// ... and over first, first + stride, ... on the context's stream, with the checks of the C entry points (slot range, null buffers, data and disparity in a frame made a template)
int frames_set_data(bpvo_hip_ctx* c, int first, int stride, int count, const uint8_t* images, const float* disps, bool on_device, int skip_odd_disp = 0);
int frames_set_template(bpvo_hip_ctx* c, int first, int stride, int count);
int upload_disparity(bpvo_hip_ctx* c, int slot, const float* disparity);
bool team_serves(const bpvo_hip_ctx* c, int n);
PairJob group_pair_job(const bpvo_hip_ctx* c, const PairJob& whole, int k);
inline int job_tables(const bpvo_hip_ctx* c) { return c->G > 1 ? 1 + c->G : 1; }      // job tables of a lane: the whole jobs, then one table per channel group
// The per-point kernels of a linearisation (warp + residual, the reduction): once — or, for a wide descriptor, once per channel group, on the
// group's job table (`stride` jobs behind the table before it) with the group's channel count.
template <class F>
inline void for_each_group(const bpvo_hip_ctx* c, const bpvo_hip::GNLaunch& g, size_t stride, F&& f)
{
  if(c->G <= 1) { f(g); return; }
  for(int k = 0; k < c->G; ++k) {
    bpvo_hip::GNLaunch gg = g;
    gg.jobs = g.jobs + (size_t) (1 + k) * stride;
    gg.C = c->Cg;
    f(gg);
  }
}
// the exact median of a wide descriptor: the WHOLE job (it walks the bracket segments of every group), instantiated for the group's channel count
// (the size of a segment)
// entry of Workspace::med_blk (uint4 units, a multiple of 8 = one 128-byte line) where the dense form's totals begin
inline size_t med_totals_at(const bpvo_hip_ctx* c) { return (((size_t) ((c->cap_max + bpvo_hip::kChunkPoints - 1) / bpvo_hip::kChunkPoints) * (size_t) c->G) + 7) / 8 * 8; }
// The normalisation of the levels below the coarsest, of the template stage queued just before (frames.hip, ctx->nrm_pending), may still be
// running on the context's side streams: whoever reads those levels' (scale, centroid) next makes its stream `s` wait for it.  level: the
// pyramid level about to start — the finest level's own event is joined only there; < 0: everything.
inline hipError_t join_pending_normalization(bpvo_hip_ctx* c, hipStream_t s, int level = -1)
{
  hipError_t e = hipSuccess;
  if(c->nrm_pending) { e = hipStreamWaitEvent(s, c->nrm_pending, 0); c->nrm_pending = nullptr; }
  if(c->nrm_pending_finest && (level < 0 || level <= c->params.maxTestLevel)) {
    const hipError_t e2 = hipStreamWaitEvent(s, c->nrm_pending_finest, 0);
    c->nrm_pending_finest = nullptr;
    if(e == hipSuccess) e = e2;
  }
  return e;
}
// can a template of this context have a level of more points than the persistent kernels are given (persist_max_points)?  Only a level without
// non-maximum suppression selects (nearly) every pixel; known from the parameters alone, before any template exists
inline bool templates_may_be_dense(const bpvo_hip_ctx* c)
{
  for(int l = c->params.maxTestLevel; l < c->L; ++l)
    if(c->geom[l].nms_radius <= 0 && c->geom[l].npix > (size_t) std::max(0, c->persist_max_points)) return true;
  return false;
}
// The Student-t loss (c_api.h) runs on the four-kernel chain only: its scale stage (tscale_kernel) stands in the chain's median launch, and neither the
// persistent nor the team kernels are built for it — what reference_reduction is to the context, this is to a group's loss.
inline bool loss_is_chain_only(int loss) { return loss == BPVO_LOSS_STUDENT_T; }
// will the estimate of ONE pair be a handful of launches — the persistent kernel, a launch per pyramid level — queued in one go?  (Then the host is free
// while the GPU works, and addFrame uploads its frame's disparity in that time: vo.hip.  On the chain the host paces the rounds, and the upload's hold on
// it costs more behind the last round than in front of the first: conf/tsukuba.cfg's parameters 2.9 -> 3.2 ms per frame.)
inline bool single_pair_is_queued_at_once(const bpvo_hip_ctx* c)
{
  return c->persistent && !c->persistent_failed.load() && !c->profile_all && !c->reference_reduction && !loss_is_chain_only(c->params.lossFunction) &&
         (c->C == 8 || c->C == 1) && c->params.interp == BPVO_INTERP_LINEAR && !c->fast_warp && !templates_may_be_dense(c);
}
inline int dense_candidates(const bpvo_hip_ctx* c, int max_points) { return (c->G == 1 && max_points >= c->dense_candidates_from) ? 1 : 0; }
inline bpvo_hip::GNLaunch median_launch(const bpvo_hip_ctx* c, bpvo_hip::GNLaunch g) { if(c->G > 1) g.C = c->Cg; return g; }
// The launch of the chain's kernels over `npairs` jobs of one level: everything the context decides — channels, warp formulation, interpolation,
// reference order, the form of the median's candidates — in ONE place, so that the launches of an iteration agree.  A call site sets only what
// is its own: fuse_frozen and step_in_reduce (the estimate loops of cameras), the persistent kernel's hand-over fields.
inline bpvo_hip::GNLaunch level_launch(const bpvo_hip_ctx* c, const bpvo_hip::PairJob* jobs, int npairs, int max_points, int loss)
{
  bpvo_hip::GNLaunch g;
  g.jobs = jobs; g.npairs = npairs; g.max_points = max_points; g.C = c->C; g.loss = loss;
  g.fast_warp = c->fast_warp; g.interp = c->params.interp;
  g.reference_reduction = c->reference_reduction ? 1 : 0;
  g.dense_candidates = dense_candidates(c, max_points);
  return g;
}
// One linearisation's launches (estimate.hip linearize_launches): which of them run, the step's mode (launch_gn_step), and which timers are armed
//   TIMERS_ESTIMATE  the estimate loops of cameras: a 1-in-kProfileEvery sample of the warp_residual launches of the lane at profiling level 1, every
//                    kernel at level 2, every warp_residual and reduction at level 3 (bench.py's roofline pass)
//   TIMERS_LEVEL2    every kernel at profiling level 2, none below (rigs)
//   TIMERS_ALWAYS    every kernel whenever profiling is on (the operator-level seam)
enum LinearizeTimers { TIMERS_OFF, TIMERS_ESTIMATE, TIMERS_LEVEL2, TIMERS_ALWAYS };
struct LinearizeFlags {
  bool warp = true, median = true, reduce = true, step = true;      // (the step runs in its own launch unless GNLaunch::step_in_reduce folds it into the reduction)
  int step_mode = 0;
  LinearizeTimers timers = TIMERS_OFF;
};
// g: the level's launch; stride: jobs between the channel-group tables of a wide descriptor (for_each_group).  Launches go to the lane's stream.
void linearize_launches(bpvo_hip_ctx* c, Lane* ln, const bpvo_hip::GNLaunch& g, size_t stride, const LinearizeFlags& f);
// The checks every estimate path makes of its pairs, before anything is queued: workspaces and frame slots in range; then templates and data
// in place and, for level_lo <= level_hi, no empty template level among level_lo .. level_hi; then the current frames' full descriptor records
// (ensure_dense_descriptor: a batch's template frame as the current frame of an estimate).
int check_pairs(bpvo_hip_ctx* c, int n, const int* wss, const int* refs, const int* curs, int level_lo, int level_hi);
// prms: null (every entry runs with the context's parameters: the batch entry points, the single-sequence path), or each entry's own parameters
// (bpvo_hip_add_frames).  estimate_batch runs one estimate per loss among them — the loss instantiates the kernels —, so every entry of an
// estimate_group call has the same loss; limits and tolerances travel in the entries' jobs.
int estimate_group(bpvo_hip_ctx* c, Lane* ln, int n, const int* wss, const int* refs, const int* curs, const float* T_init, float* poses,
                   bpvo_hip_stats* stats, float* d_records_out, bool allow_persistent, const bpvo_hip_params* const* prms = nullptr);
int estimate_batch(bpvo_hip_ctx* c, int n, const int* wss, const int* refs, const int* curs, const float* T_init, float* poses, bpvo_hip_stats* stats,
                   const bpvo_hip_params* const* prms = nullptr);
// Rig mode: members i = (workspace wss[i], template refs[i], current curs[i]) with extrinsics X [n][16] estimated as ONE body pose from T_init (the
// coarse-to-fine loop of estimate_group on the four-kernel chain, kernels_gn_rig.hip's step in the place of gn_step); T_est and stats [L] are the body's
int estimate_rig(bpvo_hip_ctx* c, int n, const int* wss, const int* refs, const int* curs, const float* X, const float* T_init, float* T_est, bpvo_hip_stats* stats);
// Several rigs in one estimate (estimate_rig is its R = 1 case): rig r with members, extrinsics and poses as estimate_rig takes them and its own
// parameters (prm: the Gauss-Newton limits, tolerances and loss of its jobs and its body; null: the context's).  No workspace in two rigs, at most
// n_pairs members in all.  Every rig's result is what estimate_rig gives it alone, bit for bit.
struct RigProblem {
  int n;
  const int* wss; const int* refs; const int* curs;
  const float* X;            // [n][16]
  const float* T_init;       // [16]
  float* T_est;              // [16]
  bpvo_hip_stats* stats;     // [L] or null
  const bpvo_hip_params* prm;
};
int estimate_rigs(bpvo_hip_ctx* c, int R, const RigProblem* rigs);
// the pinned / device staging block of estimate_rigs: [n_pairs] RigEntry, then [n_pairs][16] extrinsics, then [n_pairs][16] initial poses
inline size_t rig_stage_X_at(const bpvo_hip_ctx* c) { return (sizeof(bpvo_hip::RigEntry) * (size_t) c->n_pairs + 63) / 64 * 64; }
inline size_t rig_stage_bytes(const bpvo_hip_ctx* c) { return rig_stage_X_at(c) + 2 * sizeof(float) * 16 * (size_t) c->n_pairs; }
void detile_to_channel_major(const float* src, int n, int C, int E, int V, float* out);
size_t tiled_floats(int n, int floats_per_point);
int refresh_counters(bpvo_hip_ctx* c);
int upload_single_job(bpvo_hip_ctx* c, int ws, int ref, int cur, int level);
int ensure_residuals(bpvo_hip_ctx* c, int ws);
int fraction_good(bpvo_hip_ctx* c, int ws, float thr, float* frac);
int get_weights_host(bpvo_hip_ctx* c, int ws, std::vector<float>& w_cm, int* n_out);
int check_template_not_empty(bpvo_hip_ctx* c, int ref_slot);
int ensure_lanes(bpvo_hip_ctx* c, int n);
int lanes_for(bpvo_hip_ctx* c, int n, int cap);
int ensure_saliency(bpvo_hip_ctx* c, int slot, int level);      // a level whose saliency map the selection did not store gets it (every reader of FrameSlot::sal)
int ensure_dense_descriptor(bpvo_hip_ctx* c, int slot);      // a slot with lazy levels gets its full records (accessors, a template frame used as current)
// Pose covariance (pose_cov.hip): n_records records of `members` members each — member p of record r is entry r * members + p of wss / refs / curs
// (and of sigma; prms: each entry's own parameters or null) —, X null (cameras) or [members][16] (a rig: one record), T [n_records][16] and sigma
// given, or both null: the workspaces' last estimates.  Runs on the context's stream and returns with the records in `out`.
int pose_cov_pass(bpvo_hip_ctx* c, int n_records, int members, const int* wss, const int* refs, const int* curs, const float* X, int level,
                  const float* T, const float* sigma, const bpvo_hip_params* const* prms, bpvo_hip_pose_covariance* out);
int pose_cov_ensure_scratch(bpvo_hip_ctx* c);
void pose_cov_none(bpvo_hip_pose_covariance* r);      // the record of "nothing was estimated": Identity pose and covariance, BPVO_COV_NONE
// ... does the context serve pose scoring (kLinear, at most 48 channels)?  BPVO_OK, or BPVO_ERR_UNSUPPORTED with the message
int pose_score_served(bpvo_hip_ctx* c);
// ... and the call behind bpvo_hip_score_poses(_pairs): the records of n_poses poses T [n_pairs][n_poses][16] for each of the pairs, one launch,
// no workspace touched; the addFrame drivers score their start candidates with it (vo.hip)
int score_pairs(bpvo_hip_ctx* c, int n_pairs, const int* refs, const int* curs, int level, int n_poses, const float* T, float tau,
                bpvo_hip_pose_score* out);
// the sequences a context serves (bpvo_hip_add_frames: three frame slots and one workspace each)
inline int seq_capacity(const bpvo_hip_ctx* c) { return std::max(0, std::min(c->n_frames / 3, c->n_pairs)); }
// Rectification (rectify.hip).  rect_map_of: the map of sequence seq's side (seq < 0: the context's own camera), or null where none is set.
// rectify_queue: ONE launch for the n frames of each of n_sides sides — frame i of side k is a raw image of its map's raw size, the frames of a
// side back to back at sides[k].raw (host memory: uploaded once into the context's staging), the rectified frames back to back at sides[k].dst
// (device), each of its map's destination size; the caller has seen to it that every map exists.  Nothing is synchronised.
// rect_clear: the maps of a sequence (seq < 0: the context's own) go, after the stream has finished with them.
const RectMap* rect_map_of(const bpvo_hip_ctx* c, int seq, int side);
struct RectSide { int side; const uint8_t* raw; uint8_t* dst; };
int rectify_queue(bpvo_hip_ctx* c, int n, const int* seq /*null: the context's own camera*/, int n_sides, const RectSide* sides, bool on_device);
int rect_clear(bpvo_hip_ctx* c, int seq);
// Disparity fusion (disparity_fusion.hip).  fusion_stage: ONE splat and ONE update launch on the context's stream for the items of sequences in
// mode 1 (the others are skipped; none: nothing is queued) — item: the sequence, the frame slot whose disparity is the measured map and becomes
// the fused one, and the motion from the sequence's previous frame to this one ([16]; null: a first frame, nothing is predicted).  Nothing is
// synchronised; the class counters are fetched when asked for.  fusion_seq_reset: the sequence carries nothing any more.  R: null, or the
// measurement's variance map on the device (kernels.h FusionJob::R).
// view_slot, T_view: -1 / null, or the second view of motion stereo (motion_stereo.hip) — the frame slot of the key frame of the call's last
// estimate and that estimate ([16], X_frame = T X_view); read only where the stage predicts and the sequence has motion stereo in mode 1.
struct FusionItem { int seq; int slot; const float* P; const float* R = nullptr; int view_slot = -1; const float* T_view = nullptr; };
bool fusion_on(const bpvo_hip_ctx* c, int seq);
int fusion_stage(bpvo_hip_ctx* c, int n, const FusionItem* items);
void fusion_seq_reset(bpvo_hip_ctx* c, int seq);
double fusion_last_ms(bpvo_hip_ctx* c, int which);      // option "fusion_last_splat_ms" (0) / "fusion_last_update_ms" (1)
// Measurement variance (disparity_variance.hip).  variance_front: behind the matcher of a stereo call — pair i of sz[i] pixels for sequence
// ids[i] (null: the context's own) at d_left / d_right (device), its disparities in c->st_disp —, ONE launch for the pairs whose sequence has
// fusion AND the variance in mode 1, into c->st_var (none: nothing is queued or acquired); nothing is synchronised.  variance_map_of: where that
// launch put the sequence's map, null unless the stereo call under way made one; variance_call_done: the call is over.
struct StereoSize;
int variance_front(bpvo_hip_ctx* c, int n, const StereoSize* sz, const int* ids, const uint8_t* d_left, const uint8_t* d_right);
const float* variance_map_of(const bpvo_hip_ctx* c, int seq);
inline void variance_call_done(bpvo_hip_ctx* c) { c->variance.live = false; }
void variance_seq_reset(bpvo_hip_ctx* c, int seq);
int variance_scratch_moved(bpvo_hip_ctx* c, size_t npix);      // stereo_reserve: c->st_var follows the front-end's scratch, if it exists
int stereo_reserve(bpvo_hip_ctx* c, size_t npix);      // stereo.hip: the front-end's scratch holds a call of npix pixels
double variance_last_ms(bpvo_hip_ctx* c);      // option "variance_last_kernel_ms"
// Motion stereo (motion_stereo.hip).  motion_stereo_stage: called by fusion_stage between its splat and its update with one view per job of the
// stage — the sequence, the frame's slot, the second view (slot -1 or T null: none, or the job does not predict) and the job's z-buffer —: ONE
// launch on the context's stream for the views that have a second view, a finite motion and a sequence with the feature in mode 1 (none:
// nothing is queued or acquired, and *launched stays false); the sequences of the other views get the record of "no launch".  The stream is
// not synchronised, but the host waits for the PREVIOUS launch's counters (an event) before it rewrites the pinned job rows and the records
// they belong to — in a call with two fusion stages that is the first stage's launch, as fusion_stage itself waits for its own.
// motion_stereo_on: the sequence's setting is mode 1.
struct MotionStereoView { int seq; int slot; int view_slot; const float* T; unsigned long long* zbuf; };
bool motion_stereo_on(const bpvo_hip_ctx* c, int seq);
int motion_stereo_stage(bpvo_hip_ctx* c, int n, const MotionStereoView* views, bool* launched);
void motion_stereo_seq_reset(bpvo_hip_ctx* c, int seq);
double motion_stereo_last_ms(bpvo_hip_ctx* c);      // option "motion_stereo_last_kernel_ms"
// bpvo_hip_fuse_disparities and bpvo_hip_fuse_disparities_var (disparity_fusion.hip); variances null: the constant
int fuse_disparities_impl(bpvo_hip_ctx* c, int n, const int* seq, const float* disparities, const float* variances, int on_device, const float* poses);
// The stereo front-end of an addFrame call (stereo.hip): n pairs, pair i of sz[i] pixels for sequence ids[i] (ids null: the context's own camera), the
// images of a side back to back at left / right, in host or device memory; raw: unrectified pairs, which go through rectify_queue first.  In order: the
// raw path's map check, the parameter checks per size, (raw) buffers and rectification, the matcher.  The disparities end up in c->st_disp and the
// rectified left images at *d_left, both on the device, nothing synchronised; after a failure behind the checks the stream has been drained.
struct StereoSize { int rows, cols; };
int stereo_front(bpvo_hip_ctx* c, int n, const StereoSize* sz, const int* ids, const uint8_t* left, const uint8_t* right, bool raw, bool on_device,
                 const bpvo_hip_stereo_params* sp, const uint8_t** d_left);
// the failures of sequence `seq` that vo.hip and stereo.hip share (vo.hip)
int seq_fail(bpvo_hip_ctx* c, int code, int seq, const char* what);
int camera_too_large(bpvo_hip_ctx* c, int seq, int rows, int cols);
int set_option(bpvo_hip_ctx* c, const std::string& key, double v);
int apply_options_string(bpvo_hip_ctx* c, const char* str);
struct OptionDef { const char* key; double lo, hi; std::function<double(bpvo_hip_ctx*)> get; std::function<int(bpvo_hip_ctx*, double)> set; };
const std::vector<OptionDef>& option_table();

}  // namespace bpvo_hip_host

#define CHECK_CTX(c) if(!(c)) return BPVO_ERR_INVALID_ARG
#define CHECK_SLOT(c, s) if((s) < 0 || (s) >= (c)->n_frames) return fail(c, BPVO_ERR_INVALID_ARG, "bad frame slot")
#define CHECK_WS(c, w) if((w) < 0 || (w) >= (c)->n_pairs) return fail(c, BPVO_ERR_INVALID_ARG, "bad workspace")
#define CHECK_LEVEL(c, l) if((l) < (c)->params.maxTestLevel || (l) >= (c)->L) return fail(c, BPVO_ERR_INVALID_ARG, "bad level")
