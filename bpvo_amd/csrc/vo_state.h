// libbpvo_hip, host side: the state machine of VisualOdometry::addFrame (reference: bpvo/vo.cc:125-224) for bpvo_hip_add_frame, for every
// sequence of bpvo_hip_add_frames and for every rig of bpvo_hip_add_frames_rig(s).  No HIP header: the two drivers (vo.hip: add_frame_impl, the
// single-sequence latency path, and add_frames_run, the one batched driver of sequences and rigs) queue the GPU work and keep the frame slots'
// flags; every decision and every change of a SeqState — where an estimate starts among them — is made here, once, for all
// (tests/test_vo_state_cpu.py, tests/test_rig_cpu.py and tests/test_start_policy_cpu.py compile this header with a plain C++ compiler).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstring>
#include <utility>
#include <vector>

#include "../../include/bpvo_hip/c_api.h"
#include "device_math.h"
#include "pose_score_math.h"
#include "rig_math.h"

namespace bpvo_hip_host {
using namespace bpvo_hip;

// The VisualOdometry state of bpvo/vo.cc:45-52: bpvo_hip_ctx::vo for bpvo_hip_add_frame (frame slots 0 .. 2, workspace 0), bpvo_hip_ctx::seqs[s]
// for sequence s of bpvo_hip_add_frames (frame slots 3s .. 3s+2, workspace s)
struct SeqState {
  int ref = 0, cur = 1, prev = 2;   // slot roles
  M44 T_kf;
  std::vector<M44> trajectory;
  size_t cloud_n = 0;               // the point cloud of the last Result: bpvo_hip_ctx::d_cloud, or records [s * cap, s * cap + cloud_n) of d_seq_cloud
  M44 cloud_pose;
  // the sequence's algorithm parameters (bpvo_hip_seq_set_params; the context's until then) — they outlive bpvo_hip_seq_reset, like its camera.
  // own_params: they differ from the context's in a field the library reads (only then do the sequence's jobs and decisions take them from here)
  bpvo_hip_params params;
  bool own_params = false;
  // the start policy (below: "where an estimate starts").  M: the pose the body's last Result carried, as vo_finish wrote it — Identity after
  // vo_reset and after a first frame; policy / own_policy: the body's own policy (bpvo_hip_seq / rigs_set_start_policy; the context's until
  // then) — it outlives vo_reset, like the parameters; hints: the pending hints, used by the next call that estimates and dropped by
  // vo_finish and by vo_reset; start[which]: what estimate `which` of the last call started from
  M44 M = m44_identity();
  bpvo_hip_start_policy policy = {BPVO_START_KEYFRAME_POSE, -1, 0.0f};
  bool own_policy = false;
  std::vector<M44> hints;
  bpvo_hip_start_info start[2] = {};
};
// a fresh VisualOdometry on slots first_slot .. first_slot + 2 (the slots' flags are the caller's)
inline void vo_reset(SeqState& q, int first_slot)
{
  q.ref = first_slot; q.cur = first_slot + 1; q.prev = first_slot + 2;
  q.T_kf = m44_identity();
  q.trajectory.clear();
  q.cloud_n = 0;
  q.cloud_pose = m44_identity();
  q.M = m44_identity();
  q.hints.clear();
  std::memset(q.start, 0, sizeof(q.start));
}

// what addFrame hands back before it knows anything
inline void vo_init_result(int numLevels, bpvo_hip_result* ret)
{
  const M44 I = m44_identity();
  std::memset(ret, 0, sizeof(*ret));
  std::memcpy(ret->pose, I.m, 64);
  for(int i = 0; i < 36; ++i) ret->covariance[i] = (i % 7 == 0) ? 1.0f : 0.0f;   // Q16
  ret->numLevels = numLevels;
  for(int l = 0; l < BPVO_HIP_MAX_LEVELS; ++l) ret->optimizerStatistics[l] = bpvo_hip_stats{0, -1.0f, -1.0f, BPVO_STATUS_SOLVER_ERROR};
  ret->isKeyFrame = 0;
  ret->keyFramingReason = BPVO_KF_NO_KEYFRAMING;
  ret->hasPointCloud = 0;
}
inline void vo_begin_frame(SeqState& q, int numLevels, bpvo_hip_result* ret)      // (the point cloud belongs to one Result: bpvo/types.h:549-563)
{
  vo_init_result(numLevels, ret);
  q.cloud_n = 0;
  q.cloud_pose = m44_identity();
  std::memset(q.start, 0, sizeof(q.start));      // (no estimate of this call has run yet)
}
inline void trajectory_push(std::vector<M44>& trajectory, const M44& T)   // Trajectory::push_back + InvertPose (bpvo/trajectory.cc:30-50)
{
  M44 Ti = m44_identity();
  for(int i = 0; i < 3; ++i)
    for(int j = 0; j < 3; ++j) Ti.m[i * 4 + j] = T.m[j * 4 + i];
  for(int i = 0; i < 3; ++i) {
    float s = Ti.m[0 * 4 + i] * T.m[3];
    s += Ti.m[1 * 4 + i] * T.m[7];
    s += Ti.m[2 * 4 + i] * T.m[11];
    Ti.m[i * 4 + 3] = -s;
  }
  if(!trajectory.empty()) trajectory.push_back(m44_mul(trajectory.back(), Ti));
  else trajectory.push_back(Ti);
}

// ---- the key-frame decision (bpvo/vo.cc:199-224).  Its translation and rotation criteria: BPVO_KF_LARGE_TRANSLATION, BPVO_KF_LARGE_ROTATION, or
// BPVO_KF_NO_KEYFRAMING when the fraction of good points decides.  Host floats (asin, sqrt) on purpose.
inline int keyframe_by_motion(const bpvo_hip_params& p, const M44& pose)
{
  const float t_norm = pose.m[3] * pose.m[3] + pose.m[7] * pose.m[7] + pose.m[11] * pose.m[11];
  if(t_norm > p.minTranslationMagToKeyFrame * p.minTranslationMagToKeyFrame) return BPVO_KF_LARGE_TRANSLATION;
  // math::RotationMatrixToEulerAngles (bpvo/math_utils.h:203-216); compared in radians (Q17)
  const float R00 = pose.m[0], R10 = pose.m[4], R20 = pose.m[8], R21 = pose.m[9];
  const float eta = (float) (1.0 / (std::sqrt(R00 * R00 + R10 * R10)));
  const float rz = std::asin(eta * R10), ry = std::asin(-R20), rx = std::asin(eta * R21);
  const float r_norm = rx * rx + ry * ry + rz * rz;
  if(r_norm > p.minRotationMagToKeyFrame * p.minRotationMagToKeyFrame) return BPVO_KF_LARGE_ROTATION;
  return BPVO_KF_NO_KEYFRAMING;
}
// the fraction of good points from their count over the n_points x C residuals of the last linearisation (vo_pose_estimator.cc:105-106)
inline float vo_fraction_good(unsigned good_count, int n_points, int C) { return good_count / static_cast<float>((size_t) n_points * C); }
// The decision: the motion, then the fraction of good points — read only where the motion leaves the decision to it (bpvo_hip_add_frame
// fetches its count only then; bpvo_hip_add_frames has every sequence's from one launch)
inline int vo_keyframe_reason(const bpvo_hip_params& p, const M44& T_est, float fraction_good)
{
  const int reason = keyframe_by_motion(p, T_est);
  if(reason != BPVO_KF_NO_KEYFRAMING) return reason;
  return (fraction_good < p.maxFractionOfGoodPointsToKeyFrame) ? BPVO_KF_SMALL_FRAC_GOOD : BPVO_KF_NO_KEYFRAMING;
}
inline bool vo_decide(const bpvo_hip_params& p, const M44& T_est, float fraction_good, bpvo_hip_result* ret)
{
  ret->keyFramingReason = vo_keyframe_reason(p, T_est, fraction_good);
  ret->isKeyFrame = ret->keyFramingReason != BPVO_KF_NO_KEYFRAMING;
  return ret->isKeyFrame != 0;
}

// ---- the transitions, one per branch of bpvo/vo.cc:133-188.  First frame (vo.cc:133-139): the frame just read becomes the key frame.  Returns
// the slot whose template the caller builds; once that is queued, vo_first_frame_done.
inline int vo_first_frame(SeqState& q) { std::swap(q.ref, q.cur); return q.ref; }
inline void vo_first_frame_done(SeqState& q, bpvo_hip_result* ret)
{
  trajectory_push(q.trajectory, q.T_kf);
  ret->isKeyFrame = 1;
  ret->keyFramingReason = BPVO_KF_FIRST_FRAME;
}
// Key frame (vo.cc:157-188), after its point cloud of cloud_points records has been queued: the slot rotation.
//   template_slot: the new key frame, whose template the caller builds
//   clear_slot:    -1, or the slot whose has_data / has_template flags the caller clears (the old key frame; vo.cc:176 _prev_frame->clear())
//   reestimate:    the previous frame had data: it is the new key frame, and the caller estimates (template_slot, q.cur) again from the identity
struct KeyFrameSlots { int template_slot, clear_slot; bool reestimate; };
inline KeyFrameSlots vo_keyframe(SeqState& q, bool prev_has_data, size_t cloud_points, bpvo_hip_result* ret)
{
  q.cloud_n = cloud_points;
  ret->hasPointCloud = 1;
  if(!prev_has_data) {               // vo.cc:161-173
    std::swap(q.cur, q.ref);
    return KeyFrameSlots{q.ref, -1, false};
  }
  std::swap(q.prev, q.ref);          // vo.cc:174-188
  return KeyFrameSlots{q.ref, q.prev, true};
}
// The end of every addFrame but the first: the slot advance of a frame that is no key frame (vo.cc:149-155), the pose, T_kf, the trajectory and
// the cloud's pose.  T_est: the estimate against the key frame the call began with; T_again: null, or the estimate against the new key frame
// (KeyFrameSlots::reestimate).
// The motion from the previous frame to this one, Result::pose, in every branch: the estimate against the key frame the call began with taken
// off T_kf, or — a key frame with re-estimation — the estimate against the new key frame, which IS the previous frame.  Read before vo_finish
// moves T_kf; vo_finish and the disparity fusion (vo.hip) both take it from here, so the result and the fusion see the same bits.
inline M44 vo_frame_motion(const SeqState& q, const M44& T_est, const M44* T_again)
{
  return T_again ? *T_again : m44_mul(T_est, m44_inverse(q.T_kf));
}
inline void vo_finish(SeqState& q, const M44& T_est, const M44* T_again, bpvo_hip_result* ret)
{
  const M44 pose = vo_frame_motion(q, T_est, ret->isKeyFrame ? T_again : nullptr);
  if(!ret->isKeyFrame) {
    std::swap(q.prev, q.cur);
    q.T_kf = T_est;
  } else if(!T_again) {
    q.T_kf = m44_identity();
  } else {
    q.T_kf = *T_again;
  }
  std::memcpy(ret->pose, pose.m, 64);
  trajectory_push(q.trajectory, pose);
  if(ret->hasPointCloud) q.cloud_pose = q.trajectory.back();
  q.M = pose;
  q.hints.clear();      // (both estimates of the call have used them)
}

// ---- where an estimate starts (an extension: the reference knows mode 0 only, bpvo/vo.cc:144-145,184-186).  A call makes up to two estimates: which = 0
// against the key frame it began with, base B = T_kf; which = 1 against the new key frame, base B = Identity.  A candidate c — a frame-to-frame
// motion in Result::pose's convention — starts the estimate at m44_mul(c, B); for which = 1 that is c itself, and the candidate Identity is B
// itself: neither takes a product.
//   mode 0  Identity                                                      today's start, bit for bit; no hints
//   mode 1  hints[0] if one is pending, else M                            that one; nothing is scored
//   mode 2  Identity (kind 0), M (kind 1), m44_mul(M, M) (kind 2),        the lowest score by pose_score_argmin: ties go to the first — the
//           then the pending hints (kind 3)                               reference's start —, a NaN never wins
// (A sequence's second frame has M = Identity: mode 2 then starts where mode 0 does.)
enum { START_KIND_IDENTITY = 0, START_KIND_LAST_MOTION = 1, START_KIND_LAST_MOTION_TWICE = 2, START_KIND_HINT = 3 };
struct StartCandidates {
  int n = 0;
  int kind[BPVO_HIP_MAX_START_CANDIDATES] = {};
  M44 T[BPVO_HIP_MAX_START_CANDIDATES];
};
// null, or why the policy is refused before the context is asked whether it serves the scoring (numLevels, maxTestLevel: the context's)
inline const char* vo_start_policy_refusal(const bpvo_hip_start_policy& pol, int numLevels, int maxTestLevel)
{
  if(pol.mode < BPVO_START_KEYFRAME_POSE || pol.mode > BPVO_START_SCORED) return "start policy: mode must be 0 (key-frame pose), 1 (constant velocity) or 2 (scored)";
  if(pol.mode != BPVO_START_SCORED) return nullptr;
  if(!(pol.tau > 0.0f) || !(pol.tau - pol.tau == 0.0f)) return "start policy: the scored mode needs a tau that is finite and positive (descriptor units; no default is guessed)";
  if(pol.score_level != -1 && (pol.score_level < maxTestLevel || pol.score_level >= numLevels))
    return "start policy: score_level must be -1 (the coarsest) or within [maxTestLevel, numLevels)";
  return nullptr;
}
// the hints a body may hold under a policy: null, or why n of them are refused (a hint: rigid and finite, rig_extrinsic_ok's rule)
inline const char* vo_start_hints_refusal(const bpvo_hip_start_policy& pol, int n, const float* M)
{
  if(n < 0 || (n > 0 && !M)) return "start hints: n >= 0 poses";
  if(n > 0 && pol.mode == BPVO_START_KEYFRAME_POSE) return "start hints: the body's start policy is mode 0 (key-frame pose), which takes none";
  if(n > 1 && pol.mode == BPVO_START_CONSTANT_VELOCITY) return "start hints: mode 1 (constant velocity) takes at most one";
  if(n > BPVO_HIP_MAX_START_HINTS) return "start hints: at most 13";
  for(int i = 0; i < n; ++i)
    if(!rig_extrinsic_ok(M + 16 * (size_t) i)) return "start hints: a hint is not a rigid transform (finite, last row 0 0 0 1, R^T R = I within 1e-4)";
  return nullptr;
}
inline void vo_set_start_hints(SeqState& q, int n, const float* M)
{
  q.hints.resize((size_t) n);
  for(int i = 0; i < n; ++i) std::memcpy(q.hints[(size_t) i].m, M + 16 * (size_t) i, 64);
}
// the candidates of estimate `which` of body q under the policy it runs with (hints beyond what the mode takes — the policy changed after they
// were set — are not listed)
inline StartCandidates vo_start_candidates(const SeqState& q, const bpvo_hip_start_policy& pol, int which)
{
  StartCandidates sc;
  const M44 B = which == 0 ? q.T_kf : m44_identity();
  auto add = [&](int kind, const M44& c) {
    sc.kind[sc.n] = kind;
    sc.T[sc.n] = kind == START_KIND_IDENTITY ? B : which == 0 ? m44_mul(c, B) : c;
    ++sc.n;
  };
  if(pol.mode == BPVO_START_CONSTANT_VELOCITY) {
    if(!q.hints.empty()) add(START_KIND_HINT, q.hints[0]);
    else add(START_KIND_LAST_MOTION, q.M);
  } else if(pol.mode == BPVO_START_SCORED) {
    add(START_KIND_IDENTITY, B);
    add(START_KIND_LAST_MOTION, q.M);
    add(START_KIND_LAST_MOTION_TWICE, m44_mul(q.M, q.M));
    for(size_t i = 0; i < q.hints.size() && sc.n < BPVO_HIP_MAX_START_CANDIDATES; ++i) add(START_KIND_HINT, q.hints[i]);
  } else {
    add(START_KIND_IDENTITY, B);
  }
  return sc;
}
// The choice: records null (modes 0 and 1: the one candidate, zeroed records) or the candidates' records [sc.n] (mode 2).  Writes q.start[which]
// and returns the pose the estimate starts at.
inline M44 vo_start_choose(SeqState& q, int which, const StartCandidates& sc, const bpvo_hip_pose_score* records)
{
  bpvo_hip_start_info& info = q.start[which];
  std::memset(&info, 0, sizeof(info));
  info.n_candidates = sc.n;
  double score[BPVO_HIP_MAX_START_CANDIDATES];
  for(int k = 0; k < sc.n; ++k) {
    info.kind[k] = sc.kind[k];
    if(records) info.scores[k] = records[k];
    score[k] = info.scores[k].score;
  }
  info.chosen = records ? pose_score_argmin(score, sc.n) : 0;
  std::memcpy(info.T_start, sc.T[info.chosen].m, 64);
  return sc.T[info.chosen];
}
// A rig's record of one body candidate from its members' records of it (rec[p], template of n_points[p] points): the sums are the members' sums,
// the score is pooled like the fraction of good points — (sum cost_sum_p + tau sum C (N_p - n_valid_p)) / sum C N_p, f64, member order; nothing
// to score (sum N_p = 0): tau.  One member: its own record.
inline bpvo_hip_pose_score vo_rig_start_score(const bpvo_hip_pose_score* rec, const int* n_points, int n, int C, float tau)
{
  if(n == 1) return rec[0];
  bpvo_hip_pose_score out = {};
  double charged = 0.0, terms = 0.0;
  for(int p = 0; p < n; ++p) {
    out.cost_sum += rec[p].cost_sum;
    out.n_valid += rec[p].n_valid;
    out.n_below += rec[p].n_below;
    charged += (double) ((long long) C * (long long) (n_points[p] - rec[p].n_valid));
    terms += (double) ((long long) C * (long long) n_points[p]);
  }
  out.score = terms > 0.0 ? (out.cost_sum + (double) tau * charged) / terms : (double) tau;
  return out;
}

// ---- a body that moves as one: what the batched driver (vo.hip: add_frames_run) advances.  A rig (bpvo_hip_add_frames_rig(s)) is a body of n
// cameras that advance in lock step: the body's SeqState keeps T_kf, the trajectory and the RIG's parameters (its slot roles are unused), every
// member takes the same transition on its own slots; X: the extrinsics [n][16], camera_from_body.  A sequence of bpvo_hip_add_frames is a body of
// ONE member that IS the body (members[0] == &body) and has no extrinsics: X null.  A member that is the body is advanced by the body's own
// call and by nothing else, so in that form every vo_rig_* below performs exactly the plain vo_* call above it on that one state — no second
// state, no copy of the result, no float the plain call does not compute, X never read.
// One declared rig (bpvo_hip_ctx::rigs): its members' sequence ids and extrinsics, the body, and the pose-covariance record of its last frame
struct RigState {
  std::vector<int> seq;
  std::vector<float> X;
  SeqState body;
  bpvo_hip_pose_covariance cov;
};
inline void vo_rig_begin_frame(SeqState& body, SeqState* const* members, int n, int numLevels, bpvo_hip_result* ret)
{
  vo_begin_frame(body, numLevels, ret);
  for(int p = 0; p < n; ++p)
    if(members[p] != &body) { bpvo_hip_result own; vo_begin_frame(*members[p], numLevels, &own); }
}
// The fraction of good points of the body's one decision: pooled over the members, sum good_p / sum n_p C (one member: vo_fraction_good itself)
inline float vo_rig_fraction_good(const unsigned* good_counts, const int* n_points, int n, int C)
{
  if(n == 1) return vo_fraction_good(good_counts[0], n_points[0], C);
  size_t good = 0, total = 0;
  for(int p = 0; p < n; ++p) { good += good_counts[p]; total += (size_t) n_points[p] * C; }
  return good / static_cast<float>(total);
}
// the first frame of every member, then of the body (each member's template is queued between vo_first_frame and this)
inline void vo_rig_first_frame_done(SeqState& body, SeqState* const* members, int n, bpvo_hip_result* ret)
{
  for(int p = 0; p < n; ++p)
    if(members[p] != &body) { bpvo_hip_result own = *ret; vo_first_frame_done(*members[p], &own); }
  vo_first_frame_done(body, ret);
}
// the body's decision (vo_decide on the body pose with the pooled fraction) was "key frame": vo_keyframe of every member, slots[p] what its caller
// does (one member: vo_keyframe itself, on the body's result — all it writes there is hasPointCloud)
inline void vo_rig_keyframe(SeqState* const* members, int n, bool prev_has_data, const size_t* cloud_points, KeyFrameSlots* slots, bpvo_hip_result* ret)
{
  if(n == 1) { slots[0] = vo_keyframe(*members[0], prev_has_data, cloud_points[0], ret); return; }
  for(int p = 0; p < n; ++p) { bpvo_hip_result own = *ret; slots[p] = vo_keyframe(*members[p], prev_has_data, cloud_points[p], &own); }
  ret->hasPointCloud = 1;
}
// vo_finish of the body with the body's estimates and of every member with its own, X_p T X_p^-1; a member's point cloud gets the pose
// W_kf X_p^-1 (world_from_camera), W_kf the pose the body's trajectory gives the cloud (SeqState::cloud_pose of the body)
inline void vo_rig_finish(SeqState& body, SeqState* const* members, const float* X, int n, const M44& T_est, const M44* T_again, bpvo_hip_result* ret)
{
  vo_finish(body, T_est, T_again, ret);
  for(int p = 0; p < n; ++p) {
    if(members[p] == &body) continue;
    if(ret->hasPointCloud) body.cloud_n = 0;      // (the clouds are the members')
    const float* Xp = X + 16 * (size_t) p;
    M44 Tp, Tpa;
    rig_member_pose(Xp, T_est.m, Tp.m);
    if(T_again) rig_member_pose(Xp, T_again->m, Tpa.m);
    bpvo_hip_result own = *ret;
    vo_finish(*members[p], Tp, T_again ? &Tpa : nullptr, &own);
    if(ret->hasPointCloud) rig_cloud_pose(body.cloud_pose.m, Xp, members[p]->cloud_pose.m);
  }
}

}  // namespace bpvo_hip_host
