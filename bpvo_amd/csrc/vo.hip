// libbpvo_hip, host side: VisualOdometry::addFrame (reference: bpvo/vo.cc:125-224) on device-resident frame slots, point cloud, trajectory; the stereo
// front-end that feeds the stereo entry points is stereo.hip.
#include "host_ctx.h"

using namespace bpvo_hip;
using namespace bpvo_hip_host;

extern "C" {

// ---- VisualOdometry: one frame (the state machine both drivers run — add_frame_impl here, add_frames_run for sequences and rigs: vo_state.h) --------------------------------------------------
// getPointCloudFromRefFrame + GetColor (reference: bpvo/vo.cc:250-281)
static int build_point_cloud(bpvo_hip_ctx* c, size_t* cloud_points)
{
  // One kernel over the template points of the level the estimate ended on; nothing crosses the bus here: the 32-byte records wait in HBM for
  // bpvo_hip_get_point_cloud (the reference's Result owns its cloud; here the caller fetches it — vo.hpp does, into the Result's vector).
  // (Before: every channel's weights + the points + the image copied out and a host loop over the points — 5 - 9 ms per key frame of a dense
  // 640 x 480 template, more than the estimate itself.)
  const int lvl = c->params.maxTestLevel;
  FrameSlot& ref = c->frames[c->vo.ref];
  const int n = ref.n_host[lvl];
  Workspace& w = c->ws[0];
  if(w.last_ref < 0) return fail(c, BPVO_ERR_NO_DATA, "no linearisation has run on this workspace");
  if(n > c->frames[w.last_ref].n_host[w.last_level]) return fail(c, BPVO_ERR_INVALID_ARG, "size mismatch");
  int rc = ensure_residuals(c, 0);      // (fused path: the residual buffer may lag behind the last linearisation)
  if(rc) return rc;
  rc = upload_single_job(c, 0, w.last_ref, w.last_cur, w.last_level);
  if(rc) return rc;
  if((size_t) n > c->d_cloud.size()) {
    HIP_CK(c, hipStreamSynchronize(c->stream));
    HIP_CK(c, c->d_cloud.reserve(std::max<size_t>((size_t) c->geom[lvl].cap, (size_t) n)));
  }
  launch_point_cloud(c->stream, c->d_job1, n, c->C, c->params.lossFunction, ref.img[0], c->rows, c->cols, c->geom[lvl].K, c->dspace, c->d_cloud);
  HIP_CK(c, hipGetLastError());
  *cloud_points = (size_t) n;
  return BPVO_OK;
}

static int add_frame_impl(bpvo_hip_ctx* c, const uint8_t* image, const float* disparity, bool on_device, bpvo_hip_result* ret);
int bpvo_hip_add_frame(bpvo_hip_ctx* c, const uint8_t* image, const float* disparity, bpvo_hip_result* ret)
{
  CHECK_CTX(c);
  if(!image || !disparity) return fail(c, BPVO_ERR_INVALID_ARG, "nullptr image/disparity");   // bpvo/vo.cc:68-69
  return add_frame_impl(c, image, disparity, false, ret);
}
// addFrame fed by the stereo front-end: the reference's apps run StereoAlgorithm::run on the rectified pair and hand the f32
// disparity to VisualOdometry::addFrame (apps/vo_app.cc, utils/dataset.h); here the disparity never leaves the device.  raw: the pair goes
// through the rectification in front of the front-end first (c_api.h "rectification on the device"; stereo.hip stereo_front).
static int add_frame_stereo(bpvo_hip_ctx* c, const uint8_t* left, const uint8_t* right, bool raw, const bpvo_hip_stereo_params* sp, bpvo_hip_result* ret)
{
  CHECK_CTX(c);
  if(!left || !right) return fail(c, BPVO_ERR_INVALID_ARG, "nullptr image");
  const StereoSize size{c->rows, c->cols};
  const uint8_t* d_left = nullptr;
  if(int rc = stereo_front(c, 1, &size, nullptr, left, right, raw, false, sp, &d_left)) return rc;
  const int rc = add_frame_impl(c, d_left, c->st_disp, true, ret);
  variance_call_done(c);      // (the front-end's measurement-variance map served this call's fusion only)
  return rc;
}
int bpvo_hip_add_frame_stereo(bpvo_hip_ctx* c, const uint8_t* left, const uint8_t* right, const bpvo_hip_stereo_params* sp, bpvo_hip_result* ret)
{
  return add_frame_stereo(c, left, right, false, sp, ret);
}
int bpvo_hip_add_frame_stereo_raw(bpvo_hip_ctx* c, const uint8_t* left_raw, const uint8_t* right_raw, const bpvo_hip_stereo_params* sp, bpvo_hip_result* ret)
{
  return add_frame_stereo(c, left_raw, right_raw, true, sp, ret);
}
static void slot_clear(bpvo_hip_ctx* c, int slot) { c->frames[slot].has_data = false; c->frames[slot].has_template = false; }
// option disparity fusion (c_api.h; disparity_fusion.hip) for bpvo_hip_add_frame's sequence: the frame in `slot` is fused with the carried maps moved
// by P, the motion from the previous frame (vo_state.h vo_frame_motion; null: the first frame).  Mode 0: nothing is computed or queued.  In a stereo
// call whose front-end made a measurement-variance map for the frame (disparity_variance.hip), the item carries it.  key_slot: the key frame the
// call began with — with T_est the second view of motion stereo (motion_stereo.hip), or, behind a re-estimate, the new key frame q.ref with T_again.
static int fuse_frame(bpvo_hip_ctx* c, const SeqState& q, int slot, const M44& T_est, const M44* T_again, bool first, int key_slot = -1)
{
  if(!fusion_on(c, 0)) return BPVO_OK;
  const M44 P = first ? m44_identity() : vo_frame_motion(q, T_est, T_again);
  FusionItem it{0, slot, first ? nullptr : P.m, variance_map_of(c, 0)};
  if(!first) { it.view_slot = T_again ? q.ref : key_slot; it.T_view = T_again ? T_again->m : T_est.m; }
  return fusion_stage(c, 1, &it);
}

// ---- the start policy in the drivers (vo_state.h states the rule: "where an estimate starts") ----------------------------------------------
// the policy a body runs: its own, or the context's
static const bpvo_hip_start_policy& body_policy(const bpvo_hip_ctx* c, const SeqState& q) { return q.own_policy ? q.policy : c->start_policy; }
// A body about to estimate: its n member pairs (refs[p], curs[p]) and their extrinsics X [n][16] (null: one member that is the body)
struct StartBody { SeqState* body; int n; const int* refs; const int* curs; const float* X; };
// Where estimate `which` of each of the m bodies starts: T_start[k], and the body's SeqState::start[which].  Modes 0 and 1 are host work only.  The
// bodies in mode 2 are scored by score_pairs — which touches no workspace and gives a pair the same records whatever shares its launch —, all
// their member pairs in ONE call per distinct (score level, tau) among them, in order of first appearance; a shorter candidate list is padded
// with its candidate 0, whose repeats are not read back.  The choice is vo_start_choose's, on the host, from the returned records.
static int choose_starts(bpvo_hip_ctx* c, int which, int m, const StartBody* b, M44* T_start)
{
  std::vector<StartCandidates> sc((size_t) m);
  std::vector<int> scored;      // the bodies in mode 2
  for(int k = 0; k < m; ++k) {
    const bpvo_hip_start_policy& pol = body_policy(c, *b[k].body);
    sc[k] = vo_start_candidates(*b[k].body, pol, which);
    if(pol.mode == BPVO_START_SCORED) scored.push_back(k);
    else T_start[k] = vo_start_choose(*b[k].body, which, sc[k], nullptr);
  }
  std::vector<char> done((size_t) m, 0);
  for(int k0 : scored) {
    if(done[k0]) continue;
    const bpvo_hip_start_policy& pol0 = body_policy(c, *b[k0].body);
    const int level = pol0.score_level < 0 ? c->L - 1 : pol0.score_level;
    std::vector<int> group, refs, curs;
    int n_poses = 0;
    for(int k : scored) {
      const bpvo_hip_start_policy& pol = body_policy(c, *b[k].body);
      if(done[k] || (pol.score_level < 0 ? c->L - 1 : pol.score_level) != level || pol.tau != pol0.tau) continue;
      done[k] = 1;
      group.push_back(k);
      n_poses = std::max(n_poses, sc[k].n);
      refs.insert(refs.end(), b[k].refs, b[k].refs + b[k].n);
      curs.insert(curs.end(), b[k].curs, b[k].curs + b[k].n);
    }
    const size_t n_pairs = refs.size();
    std::vector<float> T(n_pairs * (size_t) n_poses * 16);
    size_t pair = 0;
    for(int k : group)
      for(int p = 0; p < b[k].n; ++p, ++pair)
        for(int j = 0; j < n_poses; ++j) {
          const M44& cand = sc[k].T[j < sc[k].n ? j : 0];
          float* dst = &T[(pair * (size_t) n_poses + (size_t) j) * 16];
          if(b[k].X) rig_member_pose(b[k].X + 16 * (size_t) p, cand.m, dst);      // (what estimate_rigs starts its members with)
          else std::memcpy(dst, cand.m, 64);
        }
    std::vector<bpvo_hip_pose_score> rec(n_pairs * (size_t) n_poses);
    if(int rc = score_pairs(c, (int) n_pairs, refs.data(), curs.data(), level, n_poses, T.data(), pol0.tau, rec.data())) return rc;
    pair = 0;
    for(int k : group) {
      bpvo_hip_pose_score body_rec[BPVO_HIP_MAX_START_CANDIDATES];
      std::vector<bpvo_hip_pose_score> mine((size_t) b[k].n);
      std::vector<int> n_points((size_t) b[k].n);
      for(int p = 0; p < b[k].n; ++p) n_points[(size_t) p] = c->frames[b[k].refs[p]].n_host[level];
      for(int j = 0; j < sc[k].n; ++j) {
        for(int p = 0; p < b[k].n; ++p) mine[(size_t) p] = rec[(pair + (size_t) p) * (size_t) n_poses + (size_t) j];
        body_rec[j] = vo_rig_start_score(mine.data(), n_points.data(), b[k].n, c->C, pol0.tau);
      }
      T_start[k] = vo_start_choose(*b[k].body, which, sc[k], body_rec);
      pair += (size_t) b[k].n;
    }
  }
  return BPVO_OK;
}

static int add_frame_impl(bpvo_hip_ctx* c, const uint8_t* image, const float* disparity, bool on_device, bpvo_hip_result* ret)
{
  if(!ret) return fail(c, BPVO_ERR_INVALID_ARG, "nullptr result");
  if(c->n_frames < 3) return fail(c, BPVO_ERR_INVALID_ARG, "add_frame needs a ctx with n_frames >= 3");
  if(!c->rigs.empty()) return fail(c, BPVO_ERR_INVALID_ARG, "this context declares a rig (bpvo_hip_rig_set): it serves bpvo_hip_add_frames_rig only");
  if(c->vo_mode == 2) return fail(c, BPVO_ERR_INVALID_ARG, "this context runs bpvo_hip_add_frames: a context serves either add_frame or add_frames");
  c->vo_mode = 1;
  (void) hipSetDevice(c->device);
  SeqState& q = c->vo;
  vo_begin_frame(q, c->L, ret);
  pose_cov_none(&c->vo_cov);

  // _cur_frame->setData (vo.cc:131).  No host synchronisation behind it: the estimate queues behind the data stage on the same stream and ends
  // with one (every copy from the caller's buffers is complete when this function returns — its early returns synchronise themselves).  The
  // disparity of a host frame, which only a later template stage reads, is uploaded once the estimate is queued (upload_disparity): the copy
  // from pageable memory holds the host for 90 us, which then lie under the Gauss-Newton kernels instead of in front of them.
  if(q.cur < 0 || q.cur >= c->n_frames) return fail(c, BPVO_ERR_INVALID_ARG, "bad frame slot range");
  FrameRun data_run = ctx_run(c);
  data_run.skip_disparity_upload = !on_device && c->vo_disparity_late && single_pair_is_queued_at_once(c);
  int rc = frames_set_data_slots(c, &q.cur, 1, image, disparity, on_device, data_run);
  if(rc) { (void) hipStreamSynchronize(c->stream); return rc; }
  const int data_slot = q.cur;
  bool disparity_pending = data_run.skip_disparity_upload;
  auto upload_now = [&]() -> int {
    c->before_final_sync = nullptr;
    if(!disparity_pending) return BPVO_OK;
    disparity_pending = false;
    return upload_disparity(c, data_slot, disparity);
  };

  if(!c->frames[q.ref].has_template) {                // first frame (vo.cc:133-139)
    const int slot = vo_first_frame(q);
    rc = upload_now();                                 // (its template stage reads the disparity)
    if(rc == BPVO_OK) rc = fuse_frame(c, q, slot, q.T_kf, nullptr, true);      // (carried = measurement; the slot keeps the caller's bits)
    if(rc == BPVO_OK) rc = frames_set_template(c, slot, 1, 1);
    if(rc) { (void) hipStreamSynchronize(c->stream); return rc; }
    vo_first_frame_done(q, ret);
    return BPVO_OK;
  }

  M44 T_est, T_again;
  const int ws0 = 0;
  const int key_slot = q.ref;      // (the key frame of the first estimate: its image stays in its slot whatever the slot rotation below does)
  rc = check_template_not_empty(c, q.ref);
  if(rc) { (void) upload_now(); (void) hipStreamSynchronize(c->stream); return rc; }
  // the start (vo_state.h; the default policy: T_kf itself and no launch).  The scored mode's round trip lies here, in front of the estimate
  M44 T_start;
  {
    const StartBody sb{&q, 1, &q.ref, &q.cur, nullptr};
    rc = choose_starts(c, 0, 1, &sb, &T_start);
    if(rc) { (void) upload_now(); (void) hipStreamSynchronize(c->stream); return rc; }
  }
  c->prefetch_frac_thr = c->params.goodPointThreshold;      // the decision's fraction of good points rides behind the estimate
  if(disparity_pending) c->before_final_sync = [&]() { return upload_now(); };
  rc = estimate_batch(c, 1, &ws0, &q.ref, &q.cur, T_start.m, T_est.m, ret->optimizerStatistics);
  c->prefetch_frac_thr = -1.0f;
  {      // (an estimate that did not come by its final synchronisation — an error on the way, another path — : now)
    const int rcu = upload_now();
    if(rc == BPVO_OK) rc = rcu;
  }
  if(rc) { (void) hipStreamSynchronize(c->stream); return rc; }
  // option "pose_covariance": the pass behind the estimate, from the workspace's state on the device and before the key frame's stages rewrite any
  // slot; at a key frame with re-estimation it runs again behind the re-estimate, whose pose the result carries
  if(c->pose_covariance) {
    rc = pose_cov_pass(c, 1, 1, &ws0, &q.ref, &q.cur, nullptr, c->params.maxTestLevel, nullptr, nullptr, nullptr, &c->vo_cov);
    if(rc) return rc;
  }
  // the key-frame decision (vo.cc:199-224).  The fraction of good points is fetched only where the motion leaves the decision to it: an estimate
  // that could not take the count along pays a launch and a round trip for it.
  float frac = 0.0f;
  if(keyframe_by_motion(c->params, T_est) == BPVO_KF_NO_KEYFRAMING) {
    rc = fraction_good(c, 0, c->params.goodPointThreshold, &frac);
    if(rc) return rc;
  }
  bool again = false;
  if(vo_decide(c->params, T_est, frac, ret)) {
    size_t cloud_points = 0;
    rc = build_point_cloud(c, &cloud_points);
    if(rc) return rc;
    const KeyFrameSlots kf = vo_keyframe(q, c->frames[q.prev].has_data, cloud_points, ret);
    if(kf.clear_slot >= 0) slot_clear(c, kf.clear_slot);
    if(!kf.reestimate) {                                // vo.cc:161-173
      // (disparity fusion: the current frame becomes the key frame — fused before its template is built; T_kf moves in vo_finish only)
      rc = fuse_frame(c, q, data_slot, T_est, nullptr, false, key_slot);
      if(rc) return rc;
      rc = frames_set_template(c, kf.template_slot, 1, 1);
      if(rc) return rc;
    } else {                                            // vo.cc:174-188
      // the estimate against the new key frame follows on the same stream: the template stage ends without a host round trip of its own and
      // leaves the normalisation sums of the levels below the coarsest on the side streams, under the Gauss-Newton iterations of the levels
      // above them (a dense 640x480 template, conf/tsukuba.cfg: 2.3 ms of dependent adds for the finest level)
      FrameRun fr = ctx_run(c);
      fr.no_final_sync = !c->profiling;
      fr.defer_finest_nrm = true;
      rc = frames_set_template_slots(c, &kf.template_slot, 1, fr);
      M44 T_start2 = m44_identity();      // (the default policy: the Identity)
      if(rc == BPVO_OK) {
        const StartBody sb{&q, 1, &q.ref, &q.cur, nullptr};
        rc = choose_starts(c, 1, 1, &sb, &T_start2);
      }
      if(rc == BPVO_OK) rc = estimate_batch(c, 1, &ws0, &q.ref, &q.cur, T_start2.m, T_again.m, ret->optimizerStatistics);
      // (an error on the way: nothing of this call stays in flight)
      if(c->nrm_pending) { (void) hipEventSynchronize(c->nrm_pending); c->nrm_pending = nullptr; }
      if(c->nrm_pending_finest) { (void) hipEventSynchronize(c->nrm_pending_finest); c->nrm_pending_finest = nullptr; }
      if(rc) return rc;
      again = true;
      if(c->pose_covariance) {
        rc = pose_cov_pass(c, 1, 1, &ws0, &q.ref, &q.cur, nullptr, c->params.maxTestLevel, nullptr, nullptr, nullptr, &c->vo_cov);
        if(rc) return rc;
      }
      // (disparity fusion: the new key frame is the previous frame, fused in its own call; the current frame with the re-estimate's motion)
      rc = fuse_frame(c, q, data_slot, T_est, &T_again, false, key_slot);
      if(rc) return rc;
    }
  } else {
    rc = fuse_frame(c, q, data_slot, T_est, nullptr, false, key_slot);      // (no key frame: at the end of the call)
    if(rc) return rc;
  }
  vo_finish(q, T_est, again ? &T_again : nullptr, ret);
  if(c->pose_covariance) std::memcpy(ret->covariance, c->vo_cov.covariance, sizeof(ret->covariance));
  return BPVO_OK;
}

// The accessors of a VisualOdometry state, for bpvo_hip_add_frame's and for a sequence's (q: null while the sequences have no state yet)
static int vo_num_points_at_level(bpvo_hip_ctx* c, const SeqState* q, int level, int* n)
{
  if(level < 0) level = c->params.maxTestLevel;
  if(level >= c->L) return fail(c, BPVO_ERR_INVALID_ARG, "bad level");
  *n = q && c->frames[q->ref].has_template ? c->frames[q->ref].n_host[level] : 0;
  return BPVO_OK;
}
static int vo_get_point_cloud(bpvo_hip_ctx* c, const SeqState* q, const bpvo_hip_point_with_info* d_cloud, bpvo_hip_point_with_info* pts, size_t* n,
                              float pose[16])
{
  const size_t cnt = q ? q->cloud_n : 0;
  if(n) *n = cnt;
  if(pts && cnt) {
    (void) hipSetDevice(c->device);
    HIP_CK(c, hipMemcpyAsync(pts, d_cloud, cnt * sizeof(bpvo_hip_point_with_info), hipMemcpyDeviceToHost, c->stream));
    HIP_CK(c, hipStreamSynchronize(c->stream));
  }
  if(pose) {
    const M44 P = q ? q->cloud_pose : m44_identity();
    std::memcpy(pose, P.m, 64);
  }
  return BPVO_OK;
}
static int vo_trajectory_size(const SeqState* q) { return q ? (int) q->trajectory.size() : 0; }
static void vo_get_trajectory(const SeqState* q, float* poses)
{
  for(size_t i = 0; q && i < q->trajectory.size(); ++i) std::memcpy(poses + 16 * i, q->trajectory[i].m, 64);
}

int bpvo_hip_vo_num_points_at_level(bpvo_hip_ctx* c, int level, int* n) { CHECK_CTX(c); return vo_num_points_at_level(c, &c->vo, level, n); }
int bpvo_hip_vo_points_at_level(bpvo_hip_ctx* c, int level, float* xyzw)
{
  CHECK_CTX(c);
  if(level < 0) level = c->params.maxTestLevel;
  return bpvo_hip_get_points(c, c->vo.ref, level, xyzw);
}
int bpvo_hip_get_point_cloud(bpvo_hip_ctx* c, bpvo_hip_point_with_info* pts, size_t* n, float pose[16])
{
  CHECK_CTX(c);
  return vo_get_point_cloud(c, &c->vo, c->d_cloud, pts, n, pose);
}
int bpvo_hip_trajectory_size(bpvo_hip_ctx* c, int* n) { CHECK_CTX(c); *n = vo_trajectory_size(&c->vo); return BPVO_OK; }
int bpvo_hip_get_trajectory(bpvo_hip_ctx* c, float* poses) { CHECK_CTX(c); vo_get_trajectory(&c->vo, poses); return BPVO_OK; }

// ---- many independent VisualOdometry sequences in one context (bpvo/vo.cc:125-224 per sequence) ---------------------------------------------
// Sequence s owns frame slots 3s .. 3s+2 and workspace s.  One call runs every phase of addFrame once for all the sequences it advances
// (add_frames_run below, the driver rigs share): one data stage over their current slots, one template stage for the first frames, one estimate,
// one count of good points, one point-cloud launch and one template stage for the key frames, one estimate against the new key frames.  Each
// sequence sees the same kernels on the same inputs as the single path's addFrame (the frame stages, the estimate and the counts do not depend
// on the batch a frame or pair is in), and the host decides with the same float code — every decision and every change of a sequence's state
// is a call into vo_state.h that performs the calls add_frame_impl makes —: the results are the single path's, bit for bit.
static void seq_reset_state(bpvo_hip_ctx* c, int s)
{
  vo_reset(c->seqs[s], 3 * s);
  for(int k = 0; k < 3; ++k) slot_clear(c, 3 * s + k);
  Workspace& w = c->ws[s];
  w.last_ref = w.last_cur = w.last_level = -1;
  w.has_estimate = false;
  if((size_t) s < c->seq_cov.size()) pose_cov_none(&c->seq_cov[(size_t) s]);
}
// the sequences' host state (no device storage: bpvo_hip_seq_set_params may come before the first frame); every sequence starts with the context's parameters
static void seq_states(bpvo_hip_ctx* c)
{
  if(!c->seqs.empty()) return;
  const int S = seq_capacity(c);
  c->seqs.resize((size_t) S);
  for(int s = 0; s < S; ++s) {
    c->seqs[s].params = c->params;
    seq_reset_state(c, s);
  }
}
static int seq_storage(bpvo_hip_ctx* c)
{
  const size_t S = (size_t) seq_capacity(c), cap = (size_t) c->geom[c->params.maxTestLevel].cap;
  if(!c->d_seq_cloud) HIP_CK(c, c->d_seq_cloud.alloc(S * cap));
  if(!c->d_seq_jobs) HIP_CK(c, c->d_seq_jobs.alloc(S));
  if(!c->h_seq_jobs) HIP_CK(c, c->h_seq_jobs.alloc(S));
  if(!c->d_cloud_jobs) HIP_CK(c, c->d_cloud_jobs.alloc(S));
  if(!c->h_cloud_jobs) HIP_CK(c, c->h_cloud_jobs.alloc(S));
  if(!c->d_seq_cnt) HIP_CK(c, c->d_seq_cnt.alloc(S));
  if(!c->h_seq_cnt) HIP_CK(c, c->h_seq_cnt.alloc(S));
  if(!c->d_seq_off) HIP_CK(c, c->d_seq_off.alloc(S));
  if(!c->h_seq_off) HIP_CK(c, c->h_seq_off.alloc(S));
  return BPVO_OK;
}
// BPVO_OK while none of the sequence's slots holds a frame, else the failure; what: "camera changes" / "parameters change"
static int seq_is_fresh(bpvo_hip_ctx* c, int seq, const char* what)
{
  for(int k = 0; k < 3; ++k)
    if(c->frames[3 * seq + k].has_data || c->frames[3 * seq + k].has_template)
      return seq_fail(c, BPVO_ERR_INVALID_ARG, seq, ("holds frames: its " + std::string(what) + " only while it is fresh or after bpvo_hip_seq_reset").c_str());
  return BPVO_OK;
}
}  // extern "C"

int bpvo_hip_host::seq_fail(bpvo_hip_ctx* c, int code, int seq, const char* what)
{
  c->err = "sequence " + std::to_string(seq) + ": " + what;
  return code;
}
// the failures the camera and parameter setters share
int bpvo_hip_host::camera_too_large(bpvo_hip_ctx* c, int seq, int rows, int cols)
{
  return seq_fail(c, BPVO_ERR_UNSUPPORTED, seq, ("camera " + std::to_string(cols) + "x" + std::to_string(rows) + " larger than the context's " +
                                                 std::to_string(c->cols) + "x" + std::to_string(c->rows)).c_str());
}

// The frame stages of a call run once per camera size among its slots (their kernels take launch-wide sizes; the intrinsics they read from the
// jobs), each group on its own rows [tab, tab + count) of the job tables.  One size — every context without per-sequence cameras of several
// sizes — is one stage over all the slots, as before.  offsets (the data stage): each entry's pixel offset in the packed inputs, or null.
template <class F>
static int for_each_size(bpvo_hip_ctx* c, const std::vector<int>& slots, const std::vector<size_t>* offsets, F&& stage)
{
  const int n = (int) slots.size();
  auto size_of = [&](int i) { const LevelGeom& g = slot_geom(c, c->frames[slots[i]], 0); return std::make_pair(g.rows, g.cols); };
  bool uniform = true;
  for(int i = 1; i < n && uniform; ++i) uniform = size_of(i) == size_of(0);
  if(uniform) return stage(slots.data(), n, (const size_t*) nullptr, ctx_run(c));
  std::vector<char> done((size_t) n, 0);
  int tab = 0;
  for(int i = 0; i < n; ++i) {
    if(done[i]) continue;
    std::vector<int> gs;
    std::vector<size_t> go;
    for(int k = i; k < n; ++k)
      if(!done[k] && size_of(k) == size_of(i)) {
        done[k] = 1;
        gs.push_back(slots[k]);
        if(offsets) go.push_back((*offsets)[k]);
      }
    FrameRun fr = ctx_run(c);
    fr.tab = tab;
    const int rc = stage(gs.data(), (int) gs.size(), offsets ? (const size_t*) go.data() : (const size_t*) nullptr, fr);
    if(rc) return rc;
    tab += (int) gs.size();
  }
  return BPVO_OK;
}

extern "C" {

// ---- the one batched driver: a call advances ENTRIES, bodies that move as one ------------------------------------------------------------------
// An entry is a body (vo_state.h: vo_rig_*), its member sequences, its extrinsics, where its result goes and where its covariance record goes.
// A sequence of bpvo_hip_add_frames is an entry of one member whose body IS the member (&c->seqs[s]), with null extrinsics; a rig of
// bpvo_hip_add_frames_rig(s) is its RigState.  A call is homogeneous — a context serves one kind or the other — and the members of its entries
// lie flattened, entry after entry in member order, wherever a phase runs over members (frame slots, count jobs, cloud jobs).  What the kinds do
// differently is chosen by the kind in three places and nowhere else: the estimate (entries_estimate), the covariance pass (entries_covariance)
// and launch_refresh_residuals before the count (sequences only).  Every phase both kinds share is thereby pinned, bit for bit, by the
// sequences' comparison with add_frame_impl and the oracle (tests/test_gpu_multi_sequence.py).
struct Entry {
  SeqState* body;
  const int* seq; int n;             // the members' sequence ids = their workspaces
  std::vector<SeqState*> mem;        // &c->seqs[seq[p]]
  const float* X;                    // [n][16] camera_from_body, or null: one member, the body is the member
  bpvo_hip_result* ret;
  bpvo_hip_pose_covariance* cov;     // seq_cov[s] / RigState::cov
};
static void rig_param_target(bpvo_hip_ctx* c, const RigState& g)      // the members' frame jobs read the rig's selection thresholds
{
  for(int s : g.seq)
    for(int k = 0; k < 3; ++k) c->frames[3 * s + k].seq_params = g.body.own_params ? &g.body.params : nullptr;
}
static int id_fail(bpvo_hip_ctx* c, bool rig, int id, const char* what)
{
  c->err = std::string(rig ? "rig " : "sequence ") + std::to_string(id) + ": " + what;
  return BPVO_ERR_INVALID_ARG;
}
// 1. every check of a call before any state changes; ids: the sequences (given null: 0 .. n-1) or the rigs it advances
static int add_frames_check(bpvo_hip_ctx* c, bool rig, int n, const int* given, const void* images, const void* second, const char* what_null,
                            bpvo_hip_result* results, std::vector<int>& ids)
{
  const int limit = rig ? (int) c->rigs.size() : seq_capacity(c);
  if(!rig) {
    if(!c->rigs.empty()) return fail(c, BPVO_ERR_INVALID_ARG, "this context declares a rig (bpvo_hip_rig_set): it serves bpvo_hip_add_frames_rig only");
    if(c->vo_mode == 1) return fail(c, BPVO_ERR_INVALID_ARG, "this context runs bpvo_hip_add_frame: a context serves either add_frame or add_frames");
    if(limit < 1) return fail(c, BPVO_ERR_INVALID_ARG, "add_frames needs a ctx with n_frames >= 3 and n_pairs >= 1");
  }
  if(n < 1 || n > limit)
    return fail(c, BPVO_ERR_INVALID_ARG, rig ? "add_frames_rigs: n must be within 1 .. the declared rigs" : "add_frames: n must be within 1 .. the sequence capacity");
  if(!images || !second) return fail(c, BPVO_ERR_INVALID_ARG, what_null);   // bpvo/vo.cc:68-69
  if(!results) return fail(c, BPVO_ERR_INVALID_ARG, "nullptr result");
  ids.assign((size_t) n, 0);
  std::vector<char> seen((size_t) limit, 0);
  for(int i = 0; i < n; ++i) {
    ids[i] = given ? given[i] : i;
    if(ids[i] < 0 || ids[i] >= limit)
      return id_fail(c, rig, ids[i], rig ? "no such rig (bpvo_hip_rigs_set declares rigs 0 .. n_rigs-1)" : "no such sequence (n_frames >= 3 S and n_pairs >= S serve sequences 0 .. S-1)");
    if(seen[ids[i]]) return id_fail(c, rig, ids[i], "appears twice in one call");
    seen[ids[i]] = 1;
  }
  if(c->seqs.empty()) return BPVO_OK;      // (no sequence holds a frame yet; rigs_set_impl makes the states)
  auto members = [&](int i) { return rig ? c->rigs[ids[i]].seq : std::vector<int>(1, ids[i]); };
  // a member's own parameters are its body's: a sequence's its own, a rig's never
  for(int i = 0; i < n && rig; ++i)
    for(int s : members(i))
      if(c->seqs[s].own_params) return seq_fail(c, BPVO_ERR_INVALID_ARG, s, "has parameters of its own: a rig runs its own (bpvo_hip_rigs_set_params) or the context's parameters");
  if(rig && c->dspace) return fail(c, BPVO_ERR_UNSUPPORTED, "rig mode does not serve BPVO_WARP_DISPARITY_SPACE_F32");
  for(int i = 0; i < n; ++i) {
    const std::vector<int> mem = members(i);
    if(!c->frames[c->seqs[mem[0]].ref].has_template) continue;      // (its first frame)
    for(int s : mem) {
      const FrameSlot& ref = c->frames[c->seqs[s].ref];
      for(int l = c->params.maxTestLevel; l < c->L; ++l)      // template_data.cc:177 (check_template_not_empty)
        if(!ref.has_template || ref.n_host[l] <= 0)
          return seq_fail(c, BPVO_ERR_NO_TEMPLATE, s, "the key frame's template is empty (you should call setData before calling computeResiduals)");
    }
  }
  return BPVO_OK;
}
// the entries of a checked call (sequences: their states and covariance records are made at the first call)
static std::vector<Entry> call_entries(bpvo_hip_ctx* c, bool rig, const std::vector<int>& ids, bpvo_hip_result* results)
{
  if(!rig) {
    seq_states(c);
    c->vo_mode = 2;
    if(c->seq_cov.size() != c->seqs.size()) {
      c->seq_cov.resize(c->seqs.size());
      for(auto& r : c->seq_cov) pose_cov_none(&r);
    }
  }
  std::vector<Entry> E(ids.size());
  for(size_t i = 0; i < ids.size(); ++i) {
    Entry& e = E[i];
    if(rig) {
      RigState& g = c->rigs[ids[i]];
      rig_param_target(c, g);
      e.body = &g.body; e.seq = g.seq.data(); e.n = (int) g.seq.size(); e.X = g.X.data(); e.cov = &g.cov;
    } else {
      e.body = &c->seqs[ids[i]]; e.seq = &ids[i]; e.n = 1; e.X = nullptr; e.cov = &c->seq_cov[(size_t) ids[i]];
    }
    for(int p = 0; p < e.n; ++p) e.mem.push_back(&c->seqs[e.seq[p]]);
    e.ret = results + i;
  }
  return E;
}
// the members of some entries, flattened: member j is workspace wss[j] on the pair (refs[j], curs[j]); entry k's are [first[k], first[k + 1])
struct Members { std::vector<int> wss, refs, curs, first; };
static Members members_of(const std::vector<const Entry*>& which)
{
  Members M;
  M.first.push_back(0);
  for(const Entry* e : which) {
    for(int p = 0; p < e->n; ++p) { M.wss.push_back(e->seq[p]); M.refs.push_back(e->mem[p]->ref); M.curs.push_back(e->mem[p]->cur); }
    M.first.push_back((int) M.wss.size());
  }
  return M;
}
// each entry's parameters (its body's).  Whether the jobs take them is the kind's rule: sequences hand them on only when one of the call's estimating
// sequences has its own — a call of uniform parameters runs exactly what it ran before there were any (null: the context's, from the launches'
// one source); a rig hands on its own, or null, rig by rig
static std::vector<const bpvo_hip_params*> entry_params(const std::vector<const Entry*>& which)
{
  std::vector<const bpvo_hip_params*> prms;
  for(const Entry* e : which) prms.push_back(&e->body->params);
  return prms;
}
// 4. ONE estimate of the entries `which`, entry k from T_init[k] to T_out[k], the statistics into the results.  Sequences: estimate_batch over the
// pairs; rigs: estimate_rigs, each body pose from all its members' residuals.  own: one of the call's estimating entries has parameters of its own
static int entries_estimate(bpvo_hip_ctx* c, const std::vector<const Entry*>& which, const Members& M, bool own, const std::vector<M44>& T_init,
                            std::vector<M44>& T_out)
{
  const int m = (int) which.size(), L = c->L;
  const std::vector<const bpvo_hip_params*> prms = entry_params(which);
  T_out.assign((size_t) m, m44_identity());
  if(which[0]->X) {
    std::vector<RigProblem> pr((size_t) m);
    for(int k = 0; k < m; ++k) {
      const int at = M.first[k];
      pr[k] = RigProblem{which[k]->n, &M.wss[at], &M.refs[at], &M.curs[at], which[k]->X, T_init[k].m, T_out[k].m, which[k]->ret->optimizerStatistics,
                         which[k]->body->own_params ? prms[k] : nullptr};
    }
    return estimate_rigs(c, m, pr.data());
  }
  std::vector<bpvo_hip_stats> stats((size_t) m * L);
  const int rc = estimate_batch(c, m, M.wss.data(), M.refs.data(), M.curs.data(), T_init[0].m, T_out[0].m, stats.data(), own ? prms.data() : nullptr);
  if(rc) return rc;
  for(int k = 0; k < m; ++k) std::memcpy(which[k]->ret->optimizerStatistics, &stats[(size_t) k * L], sizeof(bpvo_hip_stats) * L);
  return BPVO_OK;
}
// option "pose_covariance": the records of the entries' last estimates, from the workspaces' states on the device, into cov[k].  Sequences: all in
// ONE pass of one-member records; rigs: the one-record pass rig by rig (its launch takes ONE set of extrinsics for all its records: DESIGN.md §5)
static int entries_covariance(bpvo_hip_ctx* c, const std::vector<const Entry*>& which, const Members& M, bool own, bpvo_hip_pose_covariance* cov)
{
  const int m = (int) which.size(), lvl = c->params.maxTestLevel;
  const std::vector<const bpvo_hip_params*> prms = entry_params(which);
  if(!which[0]->X)
    return pose_cov_pass(c, m, 1, M.wss.data(), M.refs.data(), M.curs.data(), nullptr, lvl, nullptr, nullptr, own ? prms.data() : nullptr, cov);
  for(int k = 0; k < m; ++k) {
    const int at = M.first[k];
    const std::vector<const bpvo_hip_params*> mine((size_t) which[k]->n, prms[k]);
    const int rc = pose_cov_pass(c, 1, which[k]->n, &M.wss[at], &M.refs[at], &M.curs[at], which[k]->X, lvl, nullptr, nullptr,
                                 which[k]->body->own_params ? mine.data() : nullptr, cov + k);
    if(rc) return rc;
  }
  return BPVO_OK;
}
// The seven phases of addFrame, each ONCE for all the entries of the call (phase 1: add_frames_check)
static int add_frames_run(bpvo_hip_ctx* c, bool rig, const std::vector<int>& ids, const uint8_t* images, const float* disparities, bool on_device,
                          bpvo_hip_result* results)
{
  const bpvo_hip_params& p = c->params;
  const int L = c->L, lvl = p.maxTestLevel;
  (void) hipSetDevice(c->device);
  std::vector<Entry> E = call_entries(c, rig, ids, results);
  int rc = seq_storage(c);
  if(rc) return rc;
  for(Entry& e : E) {
    vo_rig_begin_frame(*e.body, e.mem.data(), e.n, L, e.ret);
    pose_cov_none(e.cov);
  }
  auto drain = [&](int code) { (void) hipStreamSynchronize(c->stream); return code; };
  auto template_stage = [&](const int* sl, int count, const size_t*, const FrameRun& fr) { return frames_set_template_slots(c, sl, count, fr); };

  // 2. _cur_frame->setData (vo.cc:131) of every member: one data stage over their current slots
  // (member j: slot_geom(cur, 0).npix pixels — its camera's — at the sum of the members' before it)
  std::vector<int> slots;
  std::vector<size_t> offsets;
  size_t at = 0;
  for(const Entry& e : E)
    for(const SeqState* q : e.mem) {
      slots.push_back(q->cur);
      offsets.push_back(at);
      at += slot_geom(c, c->frames[q->cur], 0).npix;
    }
  rc = for_each_size(c, slots, &offsets, [&](const int* sl, int count, const size_t* off, const FrameRun& fr) {
    return frames_set_data_slots(c, sl, count, images, disparities, on_device, fr, 0, off);
  });
  if(rc) return drain(rc);
  // option disparity fusion (c_api.h; disparity_fusion.hip; sequences only — a context with a rig refuses mode 1): the frame of every sequence in
  // mode 1 is fused with the sequence's carried maps, moved by the motion from its previous frame (vo_state.h vo_frame_motion), in ONE stage for
  //   * the sequences whose current frame becomes the key frame, in front of the key frames' template stage (phase 6);
  //   * all the others at the end of the call: first frames (nothing is predicted, the slot keeps the caller's bits), frames that are no key
  //     frame, and key frames with re-estimation — their new key frame is the previous frame, fused in its own call.
  // data_slot: where phase 2 put entry i's frame (the slot roles move below).  Mode 0 everywhere: nothing is computed or queued.
  // key_slot: the key frame entry i's first estimate runs against.  Motion stereo (motion_stereo.hip) takes the second view of a frame from the
  // call's last estimate: (key_slot, T_est), or, behind a re-estimate, the new key frame — the body's ref by then — with T_again.  The old key
  // frame's image stays in its slot until a later call's data stage; every stage of this call is queued before.
  std::vector<int> data_slot, key_slot;
  std::vector<FusionItem> fuse_now, fuse_last;
  std::vector<M44> fuse_P;
  bool fusing = false;
  if(!rig) {
    for(const Entry& e : E) { data_slot.push_back(e.mem[0]->cur); key_slot.push_back(e.mem[0]->ref); fusing = fusing || fusion_on(c, e.seq[0]); }
    fuse_P.reserve(2 * E.size());      // (the items point into it)
  }
  auto fuse_item = [&](const Entry& e, const M44* P, const M44* T_view = nullptr, bool view_is_new_key = false) {
    if(P) fuse_P.push_back(*P);
    // (a stereo call whose front-end made a measurement-variance map for the frame: the item carries it — disparity_variance.hip)
    FusionItem it{e.seq[0], data_slot[(size_t) (&e - E.data())], P ? fuse_P.back().m : nullptr, variance_map_of(c, e.seq[0])};
    if(T_view) {
      fuse_P.push_back(*T_view);
      it.view_slot = view_is_new_key ? e.mem[0]->ref : key_slot[(size_t) (&e - E.data())];
      it.T_view = fuse_P.back().m;
    }
    return it;
  };

  // 3. first frames (vo.cc:133-139): every member's template in one stage
  std::vector<const Entry*> est, firsts;      // the entries that estimate / that are at their first frame
  slots.clear();
  for(Entry& e : E) {
    if(c->frames[e.mem[0]->ref].has_template) { est.push_back(&e); continue; }
    firsts.push_back(&e);
    for(SeqState* q : e.mem) slots.push_back(vo_first_frame(*q));
  }
  if(!firsts.empty()) {
    rc = for_each_size(c, slots, nullptr, template_stage);
    if(rc) return drain(rc);
    for(const Entry* e : firsts) vo_rig_first_frame_done(*e->body, e->mem.data(), e->n, e->ret);
    for(const Entry* e : firsts)
      if(fusing) fuse_last.push_back(fuse_item(*e, nullptr));
  }
  const int m = (int) est.size();
  if(m == 0) return fusing ? fusion_stage(c, (int) fuse_last.size(), fuse_last.data()) : BPVO_OK;

  // 4. estimatePose(ref, cur, T_kf) of the others, each from its body's T_kf: one estimate
  bool own = false;
  std::vector<M44> T_init((size_t) m), T_est, T_again;
  for(int k = 0; k < m; ++k) own = own || est[k]->body->own_params;
  const Members M = members_of(est);
  // (their starts: vo_state.h's rule — the default policy gives T_kf itself and adds no launch; the scored mode one score_pairs call per
  // distinct (level, tau) among them)
  auto starts = [&](int which, const std::vector<const Entry*>& ents, const Members& Mm, std::vector<M44>& T) {
    std::vector<StartBody> sb(ents.size());
    for(size_t k = 0; k < ents.size(); ++k) sb[k] = StartBody{ents[k]->body, ents[k]->n, &Mm.refs[Mm.first[k]], &Mm.curs[Mm.first[k]], ents[k]->X};
    T.assign(ents.size(), m44_identity());
    return choose_starts(c, which, (int) ents.size(), sb.data(), T.data());
  };
  rc = starts(0, est, M, T_init);
  if(rc) return drain(rc);
  rc = entries_estimate(c, est, M, own, T_init, T_est);
  if(rc) return drain(rc);
  // option "pose_covariance": behind the estimate and before the key frames' stages rewrite any slot (the entries that estimate again: once more
  // behind that estimate)
  std::vector<bpvo_hip_pose_covariance> cov((size_t) (c->pose_covariance ? m : 0));
  if(c->pose_covariance) {
    rc = entries_covariance(c, est, M, own, cov.data());
    if(rc) return rc;
  }

  // 5. the key-frame decision (vo.cc:199-224) per entry: the body's motion on the host, then the fraction of good points pooled over its members —
  // every member's count from ONE launch over the workspaces' last linearisations (estimate: level maxTestLevel)
  const int N = M.first[m];
  std::vector<int> n_points((size_t) N);
  int max_n = 0;
  for(int k = 0; k < m; ++k)
    for(int j = M.first[k]; j < M.first[k + 1]; ++j) {
      PairJob& pj = c->h_seq_jobs[j];
      pj = make_pair_job(c, M.wss[j], M.refs[j], M.curs[j], lvl);
      if(own) pair_job_set_params(pj, est[k]->body->params);
      n_points[j] = pj.n;
      max_n = std::max(max_n, pj.n);
    }
  HIP_CK(c, hipMemcpyAsync(c->d_seq_jobs, c->h_seq_jobs, sizeof(PairJob) * (size_t) N, hipMemcpyHostToDevice, c->stream));
  if(!rig) {
    // (estimate_batch's fused path: the residual buffers may lag behind the last linearisation — ensure_residuals; estimate_rigs' chain writes them always)
    launch_refresh_residuals(c->stream, level_launch(c, c->d_seq_jobs, N, max_n, p.lossFunction));
  }
  HIP_CK(c, hipMemsetAsync(c->d_seq_cnt, 0, sizeof(unsigned) * (size_t) N, c->stream));
  if(own) launch_count_good_jobs(c->stream, c->d_seq_jobs, N, max_n, c->C, c->d_seq_cnt);      // (each entry's loss and threshold, from its members' jobs)
  else launch_count_good_batch(c->stream, c->d_seq_jobs, N, max_n, c->C, p.lossFunction, p.goodPointThreshold, c->d_seq_cnt);
  HIP_CK(c, hipMemcpyAsync(c->h_seq_cnt, c->d_seq_cnt, sizeof(unsigned) * (size_t) N, hipMemcpyDeviceToHost, c->stream));
  HIP_CK(c, hipStreamSynchronize(c->stream));
  HIP_CK(c, hipGetLastError());
  std::vector<int> kf;            // entries of est that key-frame
  for(int k = 0; k < m; ++k) {
    const float frac = vo_rig_fraction_good(c->h_seq_cnt + M.first[k], n_points.data() + M.first[k], est[k]->n, c->C);
    // with the entry's thresholds (the context's unless it was given its own)
    if(vo_decide(est[k]->body->params, T_est[k], frac, est[k]->ret)) kf.push_back(k);
  }

  // 6. key frames: every member's point cloud from its old key frame and its last linearisation (build_point_cloud; one launch), the slot
  // rotation, the new templates (one stage), then ONE estimate against them of the entries that had a previous frame (vo.cc:161-188)
  std::vector<int> re;            // entries of est that estimate again
  if(!kf.empty()) {
    const size_t cap = (size_t) c->geom[lvl].cap;
    int max_c = 0, nj = 0;
    for(int k : kf)
      for(int j = M.first[k]; j < M.first[k + 1]; ++j)
        if((size_t) n_points[j] > cap) return seq_fail(c, BPVO_ERR_INVALID_ARG, M.wss[j], "size mismatch");
    for(int k : kf)
      for(int j = M.first[k]; j < M.first[k + 1]; ++j, ++nj) {
        const FrameSlot& kfr = c->frames[M.refs[j]];
        CloudJob& cj = c->h_cloud_jobs[nj];
        cj.job = c->d_seq_jobs + j; cj.img = kfr.img[0]; cj.out_offset = (size_t) M.wss[j] * cap;
        std::memcpy(cj.K, slot_geom(c, kfr, lvl).K, sizeof(cj.K));      // (build_point_cloud: the context's size and level intrinsics; here the member's)
        cj.rows = slot_geom(c, kfr, 0).rows; cj.cols = slot_geom(c, kfr, 0).cols;
        cj.loss = est[k]->body->params.lossFunction;
        max_c = std::max(max_c, n_points[j]);
      }
    HIP_CK(c, hipMemcpyAsync(c->d_cloud_jobs, c->h_cloud_jobs, sizeof(CloudJob) * (size_t) nj, hipMemcpyHostToDevice, c->stream));
    launch_point_cloud_batch(c->stream, c->d_cloud_jobs, nj, max_c, c->C, c->dspace, c->d_seq_cloud);
    HIP_CK(c, hipGetLastError());
    slots.clear();
    std::vector<const Entry*> again;
    for(int k : kf) {
      const Entry& e = *est[k];
      std::vector<size_t> cloud_points(n_points.begin() + M.first[k], n_points.begin() + M.first[k + 1]);
      std::vector<KeyFrameSlots> ks((size_t) e.n);
      vo_rig_keyframe(e.mem.data(), e.n, c->frames[e.mem[0]->prev].has_data, cloud_points.data(), ks.data(), e.ret);
      for(const KeyFrameSlots& s : ks) {
        if(s.clear_slot >= 0) slot_clear(c, s.clear_slot);
        slots.push_back(s.template_slot);
      }
      if(ks[0].reestimate) { re.push_back(k); again.push_back(&e); }
      else if(fusing) {      // (its current frame is the new key frame: fused before the template stage; T_kf moves in vo_finish only)
        const M44 P = vo_frame_motion(*e.body, T_est[k], nullptr);
        fuse_now.push_back(fuse_item(e, &P, &T_est[k]));
      }
    }
    if(!fuse_now.empty()) {
      rc = fusion_stage(c, (int) fuse_now.size(), fuse_now.data());
      if(rc) return drain(rc);
    }
    rc = for_each_size(c, slots, nullptr, template_stage);
    if(rc) return drain(rc);
    if(!re.empty()) {
      const Members M2 = members_of(again);
      std::vector<M44> T_init2;
      rc = starts(1, again, M2, T_init2);
      if(rc) return drain(rc);
      rc = entries_estimate(c, again, M2, own, T_init2, T_again);
      if(rc) return drain(rc);
      if(c->pose_covariance) {
        std::vector<bpvo_hip_pose_covariance> cov2(re.size());
        rc = entries_covariance(c, again, M2, own, cov2.data());
        if(rc) return rc;
        for(size_t t = 0; t < re.size(); ++t) cov[(size_t) re[t]] = cov2[t];
      }
    }
  }

  // 7. per entry: the pose, T_kf and the trajectory of the body (a rig: every member's slots, and its cloud's pose), the covariance record
  std::vector<int> again_of((size_t) m, -1);
  for(size_t t = 0; t < re.size(); ++t) again_of[re[t]] = (int) t;
  if(fusing) {
    for(int k = 0; k < m; ++k) {
      const Entry& e = *est[k];
      if(e.ret->isKeyFrame && again_of[k] < 0) continue;      // (fused in front of its template stage)
      const M44 P = vo_frame_motion(*e.body, T_est[k], again_of[k] >= 0 ? &T_again[again_of[k]] : nullptr);
      if(again_of[k] >= 0) fuse_last.push_back(fuse_item(e, &P, &T_again[again_of[k]], true));
      else fuse_last.push_back(fuse_item(e, &P, &T_est[k]));
    }
    rc = fusion_stage(c, (int) fuse_last.size(), fuse_last.data());
    if(rc) return drain(rc);
  }
  for(int k = 0; k < m; ++k) {
    const Entry& e = *est[k];
    vo_rig_finish(*e.body, e.mem.data(), e.X, e.n, T_est[k], again_of[k] >= 0 ? &T_again[again_of[k]] : nullptr, e.ret);
    if(c->pose_covariance) {
      *e.cov = cov[(size_t) k];
      std::memcpy(e.ret->covariance, e.cov->covariance, sizeof(e.ret->covariance));
    }
  }
  return BPVO_OK;
}

int bpvo_hip_add_frames(bpvo_hip_ctx* c, int n, const int* seq, const uint8_t* images, const float* disparities, int on_device, bpvo_hip_result* results)
{
  CHECK_CTX(c);
  std::vector<int> ids;
  const int rc = add_frames_check(c, false, n, seq, images, disparities, "nullptr image/disparity", results, ids);
  if(rc) return rc;
  return add_frames_run(c, false, ids, images, disparities, on_device != 0, results);
}
// ---- rig mode: the cameras of a rigid rig as ONE body (c_api.h; rig_math.h states the maps) ------------------------------------------------
// A context declares one rig (bpvo_hip_rig_set) or several over disjoint sets of its sequences (bpvo_hip_rigs_set): bpvo_hip_ctx::rigs.  Member p
// of a rig is sequence seq[p] — its frame slots, its workspace, its camera — with extrinsic X[p] (camera_from_body).  A call IS add_frames_run
// over the rigs it names as entries: one data stage over every member's frame, ONE estimate of the body poses from all members' residuals
// (entries_estimate -> estimate_rigs), one count of good points, per rig one key-frame decision on its body pose with the fraction pooled over
// its members and its own thresholds, every member of a rig the same transition (vo_state.h: vo_rig_*), one estimate against the new key
// frames.  A body keeps T_kf, the trajectory and the rig's parameters.  The one-rig entry points are the calls of the plural ones on rig 0.
static int rigs_set_impl(bpvo_hip_ctx* c, int n_rigs, const int* count, const int* seq, const float* X, const char* who)
{
  const std::string w(who);
  if(c->vo_mode == 1) return fail(c, BPVO_ERR_INVALID_ARG, "this context runs bpvo_hip_add_frame: a rig's members are sequences of bpvo_hip_add_frames' kind");
  if(c->fusion.n_on > 0) return fail(c, BPVO_ERR_UNSUPPORTED, (w + ": a context with disparity fusion in mode 1 does not serve rigs").c_str());
  if(c->motion_stereo.n_on > 0) return fail(c, BPVO_ERR_UNSUPPORTED, (w + ": a context with motion stereo in mode 1 does not serve rigs").c_str());
  const int S = seq_capacity(c);
  if(n_rigs < 1 || n_rigs > S) return fail(c, BPVO_ERR_INVALID_ARG, (w + ": n_rigs must be within 1 .. the sequence capacity").c_str());
  if(!count) return fail(c, BPVO_ERR_INVALID_ARG, (w + ": nullptr member counts").c_str());
  int n = 0;
  for(int r = 0; r < n_rigs; ++r) {
    if(count[r] < 1 || count[r] > S - n) return fail(c, BPVO_ERR_INVALID_ARG, (w + ": n must be within 1 .. the sequence capacity").c_str());
    n += count[r];
  }
  if(!X) return fail(c, BPVO_ERR_INVALID_ARG, (w + ": nullptr extrinsics").c_str());
  std::vector<int> ids((size_t) n);
  std::vector<char> seen((size_t) S, 0);
  for(int i = 0; i < n; ++i) {
    ids[i] = seq ? seq[i] : i;
    if(ids[i] < 0 || ids[i] >= S) return seq_fail(c, BPVO_ERR_INVALID_ARG, ids[i], "no such sequence");
    if(seen[ids[i]]) return seq_fail(c, BPVO_ERR_INVALID_ARG, ids[i], n_rigs > 1 ? "appears twice in the rigs (a sequence belongs to one rig, once)" : "appears twice in the rig");
    seen[ids[i]] = 1;
  }
  for(int i = 0; i < n; ++i)
    if(!rig_extrinsic_ok(X + 16 * (size_t) i))
      return seq_fail(c, BPVO_ERR_INVALID_ARG, ids[i], "extrinsic is not a rigid transform (finite, last row 0 0 0 1, R^T R = I within 1e-4)");
  for(int i = 0; i < n; ++i)
    if(int rc = seq_is_fresh(c, ids[i], "rig membership changes")) return rc;
  for(const RigState& g : c->rigs)      // (rigs declared before: their members leave them only fresh, too)
    for(int s : g.seq)
      if(int rc = seq_is_fresh(c, s, "rig membership changes")) return rc;
  for(int i = 0; i < n && !c->seqs.empty(); ++i)
    if(c->seqs[ids[i]].own_params) return seq_fail(c, BPVO_ERR_INVALID_ARG, ids[i], "has parameters of its own: a rig runs its own (bpvo_hip_rigs_set_params) or the context's parameters");
  for(int i = 0; i < n && !c->seqs.empty(); ++i)
    if(c->seqs[ids[i]].own_policy || !c->seqs[ids[i]].hints.empty())
      return seq_fail(c, BPVO_ERR_INVALID_ARG, ids[i], "has a start policy or hints of its own: a rig runs its body's (bpvo_hip_rigs_set_start_policy) or the context's");
  seq_states(c);
  for(RigState& g : c->rigs) { g.body.own_params = false; rig_param_target(c, g); }
  c->rigs.assign((size_t) n_rigs, RigState());
  for(int r = 0, at = 0; r < n_rigs; at += count[r], ++r) {
    RigState& g = c->rigs[r];
    g.seq.assign(ids.begin() + at, ids.begin() + at + count[r]);
    g.X.assign(X + 16 * (size_t) at, X + 16 * (size_t) (at + count[r]));
    vo_reset(g.body, 0);
    g.body.params = c->params;
    g.body.own_params = false;
    pose_cov_none(&g.cov);
  }
  c->vo_mode = 2;
  return BPVO_OK;
}
// the one-rig entry points on a context of several rigs
static int rig_is_singular(bpvo_hip_ctx* c, const char* plural)
{
  if(c->rigs.size() > 1) return fail(c, BPVO_ERR_INVALID_ARG, (std::string("this context declares several rigs (bpvo_hip_rigs_set): call ") + plural).c_str());
  return BPVO_OK;
}
int bpvo_hip_rig_set(bpvo_hip_ctx* c, int n, const int* seq, const float* X)
{
  CHECK_CTX(c);
  return rigs_set_impl(c, 1, &n, seq, X, "rig_set");
}
int bpvo_hip_rigs_set(bpvo_hip_ctx* c, int n_rigs, const int* count, const int* seq, const float* X)
{
  CHECK_CTX(c);
  return rigs_set_impl(c, n_rigs, count, seq, X, "rigs_set");
}
int bpvo_hip_rig_get(const bpvo_hip_ctx* c, int* n, int* seq, float* X)
{
  if(!c || !n || c->rigs.size() > 1) return BPVO_ERR_INVALID_ARG;
  *n = c->rigs.empty() ? 0 : (int) c->rigs[0].seq.size();
  if(seq && !c->rigs.empty()) std::copy(c->rigs[0].seq.begin(), c->rigs[0].seq.end(), seq);
  if(X && !c->rigs.empty()) std::copy(c->rigs[0].X.begin(), c->rigs[0].X.end(), X);
  return BPVO_OK;
}
int bpvo_hip_rigs_get(const bpvo_hip_ctx* c, int* n_rigs, int* count, int* seq, float* X)
{
  if(!c || !n_rigs) return BPVO_ERR_INVALID_ARG;
  *n_rigs = (int) c->rigs.size();
  size_t at = 0;
  for(size_t r = 0; r < c->rigs.size(); ++r) {
    const RigState& g = c->rigs[r];
    if(count) count[r] = (int) g.seq.size();
    if(seq) std::copy(g.seq.begin(), g.seq.end(), seq + at);
    if(X) std::copy(g.X.begin(), g.X.end(), X + 16 * at);
    at += g.seq.size();
  }
  return BPVO_OK;
}
#define CHECK_RIG(c, rig) do { if((rig) < 0 || (size_t) (rig) >= (c)->rigs.size()) return fail((c), BPVO_ERR_INVALID_ARG, ("rig " + std::to_string(rig) + ": no such rig (bpvo_hip_rigs_set declares rigs 0 .. n_rigs-1)").c_str()); } while(0)
int bpvo_hip_rig_trajectory_size(bpvo_hip_ctx* c, int* n)
{
  CHECK_CTX(c);
  if(!n) return fail(c, BPVO_ERR_INVALID_ARG, "nullptr count");
  if(int rc = rig_is_singular(c, "bpvo_hip_rigs_trajectory_size")) return rc;
  if(c->rigs.empty()) { *n = 0; return BPVO_OK; }
  return bpvo_hip_rigs_trajectory_size(c, 0, n);
}
int bpvo_hip_rig_get_trajectory(bpvo_hip_ctx* c, float* poses)
{
  CHECK_CTX(c);
  if(int rc = rig_is_singular(c, "bpvo_hip_rigs_get_trajectory")) return rc;
  if(c->rigs.empty()) return BPVO_OK;
  return bpvo_hip_rigs_get_trajectory(c, 0, poses);
}
int bpvo_hip_rigs_trajectory_size(bpvo_hip_ctx* c, int rig, int* n)
{
  CHECK_CTX(c); CHECK_RIG(c, rig);
  if(!n) return fail(c, BPVO_ERR_INVALID_ARG, "nullptr count");
  *n = vo_trajectory_size(&c->rigs[rig].body);
  return BPVO_OK;
}
int bpvo_hip_rigs_get_trajectory(bpvo_hip_ctx* c, int rig, float* poses)
{
  CHECK_CTX(c); CHECK_RIG(c, rig);
  if(!poses && vo_trajectory_size(&c->rigs[rig].body) > 0) return fail(c, BPVO_ERR_INVALID_ARG, "nullptr poses");
  vo_get_trajectory(&c->rigs[rig].body, poses);
  return BPVO_OK;
}

int bpvo_hip_add_frames_rigs(bpvo_hip_ctx* c, int n, const int* rigs, const uint8_t* images, const float* disparities, int on_device, bpvo_hip_result* results)
{
  CHECK_CTX(c);
  if(c->rigs.empty()) return fail(c, BPVO_ERR_INVALID_ARG, "add_frames_rigs: the context declares no rig (bpvo_hip_rigs_set)");
  std::vector<int> ids;
  const int rc = add_frames_check(c, true, n, rigs, images, disparities, "nullptr image/disparity", results, ids);
  if(rc) return rc;
  return add_frames_run(c, true, ids, images, disparities, on_device != 0, results);
}
int bpvo_hip_add_frames_rig(bpvo_hip_ctx* c, const uint8_t* images, const float* disparities, int on_device, bpvo_hip_result* result)
{
  CHECK_CTX(c);
  if(c->rigs.empty()) return fail(c, BPVO_ERR_INVALID_ARG, "add_frames_rig: the context declares no rig (bpvo_hip_rig_set)");
  if(int rc = rig_is_singular(c, "bpvo_hip_add_frames_rigs")) return rc;
  return bpvo_hip_add_frames_rigs(c, 1, nullptr, images, disparities, on_device, result);
}
// StereoAlgorithm::run + addFrame of every sequence of the call (apps/vo_app.cc per camera): the front-end once over all the pairs, each in
// its sequence's camera geometry, into the context's own maps, which the frame stages then read where they lie — no host synchronisation
// and no copy between the two; images from host memory are uploaded once, for both.  raw: every sequence's pair is rectified into the
// front-end's image buffers by ONE launch first (stereo.hip stereo_front).
static int add_frames_stereo(bpvo_hip_ctx* c, int n, const int* seq, const uint8_t* left, const uint8_t* right, bool raw, int on_device,
                             const bpvo_hip_stereo_params* sp, bpvo_hip_result* results)
{
  CHECK_CTX(c);
  std::vector<int> ids;
  int rc = add_frames_check(c, false, n, seq, left, right, "nullptr image", results, ids);
  if(rc) return rc;
  std::vector<StereoSize> sz((size_t) n);
  for(int i = 0; i < n; ++i) {
    const LevelGeom& g = slot_geom(c, c->frames[3 * ids[i]], 0);
    sz[i] = StereoSize{g.rows, g.cols};
  }
  const uint8_t* d_left = nullptr;
  rc = stereo_front(c, n, sz.data(), ids.data(), left, right, raw, on_device != 0, sp, &d_left);
  if(rc) return rc;
  rc = add_frames_run(c, false, ids, d_left, c->st_disp, true, results);
  variance_call_done(c);      // (the front-end's measurement-variance maps served this call's fusion only)
  return rc;
}
int bpvo_hip_add_frames_stereo(bpvo_hip_ctx* c, int n, const int* seq, const uint8_t* left, const uint8_t* right, int on_device,
                               const bpvo_hip_stereo_params* sp, bpvo_hip_result* results)
{
  return add_frames_stereo(c, n, seq, left, right, false, on_device, sp, results);
}
int bpvo_hip_add_frames_stereo_raw(bpvo_hip_ctx* c, int n, const int* seq, const uint8_t* left_raw, const uint8_t* right_raw, int on_device,
                                   const bpvo_hip_stereo_params* sp, bpvo_hip_result* results)
{
  return add_frames_stereo(c, n, seq, left_raw, right_raw, true, on_device, sp, results);
}
int bpvo_hip_seq_capacity(const bpvo_hip_ctx* c, int* n_sequences)
{
  if(!c || !n_sequences) return BPVO_ERR_INVALID_ARG;
  *n_sequences = seq_capacity(c);
  return BPVO_OK;
}
#define CHECK_SEQ(c, s) if((s) < 0 || (s) >= seq_capacity(c)) return seq_fail(c, BPVO_ERR_INVALID_ARG, s, "no such sequence")
int bpvo_hip_seq_reset(bpvo_hip_ctx* c, int seq)
{
  CHECK_CTX(c); CHECK_SEQ(c, seq);
  if(!c->seqs.empty()) seq_reset_state(c, seq);
  fusion_seq_reset(c, seq);      // (the carried maps go; the setting stays, like the parameters)
  variance_seq_reset(c, seq);
  motion_stereo_seq_reset(c, seq);
  return BPVO_OK;
}
// A sequence's own point budget (an extension: no reference member), kept on its three frame slots: it outlives bpvo_hip_seq_reset like the
// sequence's parameters; n_levels = 0 returns the sequence to the context's budget
int bpvo_hip_seq_set_point_budget(bpvo_hip_ctx* c, int seq, const int* max_points, int n_levels)
{
  CHECK_CTX(c); CHECK_SEQ(c, seq);
  if(int rc = check_point_budget(c, max_points, n_levels)) return rc;
  for(int k = 0; k < 3; ++k) {
    FrameSlot& f = c->frames[3 * seq + k];
    f.own_budget = n_levels > 0;
    for(int l = 0; l < kMaxLevels; ++l) f.budget[l] = l < n_levels ? max_points[l] : 0;
  }
  return BPVO_OK;
}
int bpvo_hip_seq_get_point_budget(const bpvo_hip_ctx* c, int seq, int* max_points, int* own)
{
  if(!c || !max_points || seq < 0 || seq >= seq_capacity(c)) return BPVO_ERR_INVALID_ARG;
  const FrameSlot& f = c->frames[3 * seq];
  for(int l = 0; l < kMaxLevels; ++l) max_points[l] = slot_budget(c, f, l);
  if(own) *own = f.own_budget ? 1 : 0;
  return BPVO_OK;
}
static const SeqState* seq_state(const bpvo_hip_ctx* c, int seq) { return c->seqs.empty() ? nullptr : &c->seqs[seq]; }
int bpvo_hip_seq_num_points_at_level(bpvo_hip_ctx* c, int seq, int level, int* n)
{
  CHECK_CTX(c); CHECK_SEQ(c, seq);
  if(!n) return fail(c, BPVO_ERR_INVALID_ARG, "nullptr count");
  return vo_num_points_at_level(c, seq_state(c, seq), level, n);
}
int bpvo_hip_seq_get_point_cloud(bpvo_hip_ctx* c, int seq, bpvo_hip_point_with_info* pts, size_t* n, float pose[16])
{
  CHECK_CTX(c); CHECK_SEQ(c, seq);
  return vo_get_point_cloud(c, seq_state(c, seq), c->d_seq_cloud + (size_t) seq * (size_t) c->geom[c->params.maxTestLevel].cap, pts, n, pose);
}
int bpvo_hip_seq_trajectory_size(bpvo_hip_ctx* c, int seq, int* n)
{
  CHECK_CTX(c); CHECK_SEQ(c, seq);
  if(!n) return fail(c, BPVO_ERR_INVALID_ARG, "nullptr count");
  *n = vo_trajectory_size(seq_state(c, seq));
  return BPVO_OK;
}
int bpvo_hip_seq_get_trajectory(bpvo_hip_ctx* c, int seq, float* poses)
{
  CHECK_CTX(c); CHECK_SEQ(c, seq);
  if(!poses && vo_trajectory_size(seq_state(c, seq)) > 0) return fail(c, BPVO_ERR_INVALID_ARG, "nullptr poses");
  vo_get_trajectory(seq_state(c, seq), poses);
  return BPVO_OK;
}

// ---- per-sequence cameras ----------------------------------------------------------------------------------------------------------------
// A camera's level geometry (level_geometry: the one derivation bpvo_hip_create uses) for L levels, after the checks every camera passes.
// Returns the status, with what failed in *why.
static int camera_geometry(const bpvo_hip_camera& cam, const bpvo_hip_params& p, bool auto_levels, int L, LevelGeom* g, std::string* why)
{
  for(int k = 0; k < 9; ++k)
    if(!std::isfinite(cam.K[k])) { *why = "camera: K must be finite"; return BPVO_ERR_INVALID_ARG; }
  if(!(cam.K[0] > 0.0f) || !(cam.K[4] > 0.0f)) { *why = "camera: fx and fy must be positive"; return BPVO_ERR_INVALID_ARG; }
  if(cam.K[8] != 1.0f) { *why = "camera: K[8] must be 1"; return BPVO_ERR_INVALID_ARG; }
  if(!std::isfinite(cam.baseline) || !(cam.baseline > 0.0f)) { *why = "camera: the baseline must be positive"; return BPVO_ERR_INVALID_ARG; }
  if(cam.rows < 8 || cam.cols < 8 || cam.rows > 65535 || cam.cols > 65535 || (long long) cam.rows * cam.cols * 8 > 0x7fffffffLL) {
    *why = "camera: image size out of range (8 .. 65535 rows and cols, at most 2^28 pixels)";
    return BPVO_ERR_INVALID_ARG;
  }
  if(auto_levels) {      // bpvo/vo.cc:101-105, as bpvo_hip_create counts them
    const int own = auto_pyramid_levels(cam.rows, cam.cols, p.minImageDimensionForPyramid);
    if(own != L) {
      *why = "camera " + std::to_string(cam.cols) + "x" + std::to_string(cam.rows) + ": its automatic pyramid has " + std::to_string(own) +
             " levels, the context's " + std::to_string(L);
      return BPVO_ERR_UNSUPPORTED;
    }
  }
  if(const char* w = level_geometry(cam.K, cam.baseline, cam.rows, cam.cols, L, p, g)) { *why = std::string("camera: ") + w; return BPVO_ERR_UNSUPPORTED; }
  return BPVO_OK;
}
static bool same_geometry(const LevelGeom* a, const LevelGeom* b, int L)
{
  for(int l = 0; l < L; ++l)
    if(a[l].rows != b[l].rows || a[l].cols != b[l].cols || a[l].npix != b[l].npix || a[l].nblk != b[l].nblk || a[l].cap != b[l].cap ||
       a[l].nms_radius != b[l].nms_radius || a[l].b != b[l].b || std::memcmp(a[l].K, b[l].K, sizeof(a[l].K)) != 0)
      return false;
  return true;
}
// the camera of sequence s = the geometry of its three slots (a camera whose geometry is the context's own: none, the plain path)
static void assign_camera(bpvo_hip_ctx* c, int s, const LevelGeom* g)
{
  const bool own = !same_geometry(g, c->geom, c->L);
  for(int k = 0; k < 3; ++k) {
    FrameSlot& f = c->frames[3 * s + k];
    f.own_geom = own;
    for(int l = 0; l < kMaxLevels; ++l) f.geom[l] = own && l < c->L ? g[l] : LevelGeom{};
  }
}

int bpvo_hip_create_sequences(bpvo_hip_ctx** out, int n_sequences, const bpvo_hip_camera* cams, const bpvo_hip_params* p, int device)
{
  if(!out || n_sequences < 1 || !cams || !p) {
    g_create_error = "invalid argument";
    return BPVO_ERR_INVALID_ARG;
  }
  int rows = 0, cols = 0;
  for(int s = 0; s < n_sequences; ++s) { rows = std::max(rows, cams[s].rows); cols = std::max(cols, cams[s].cols); }
  const bool auto_levels = p->numPyramidLevels <= 0;
  int L = p->numPyramidLevels;
  if(auto_levels && rows >= 8 && cols >= 8) L = auto_pyramid_levels(rows, cols, p->minImageDimensionForPyramid);
  if(L < 1 || L > kMaxLevels) {
    g_create_error = "numPyramidLevels out of range (1..8)";
    return BPVO_ERR_UNSUPPORTED;
  }
  // every camera's geometry, and per level the largest template capacity among them
  std::vector<LevelGeom> geoms((size_t) n_sequences * kMaxLevels);
  int min_caps[kMaxLevels] = {};
  for(int s = 0; s < n_sequences; ++s) {
    std::string why;
    const int rc = camera_geometry(cams[s], *p, auto_levels, L, &geoms[(size_t) s * kMaxLevels], &why);
    if(rc) { g_create_error = "sequence " + std::to_string(s) + ": " + why; return rc; }
    for(int l = 0; l < L; ++l) min_caps[l] = std::max(min_caps[l], geoms[(size_t) s * kMaxLevels + l].cap);
  }
  bpvo_hip_ctx* c = nullptr;
  const int rc = create_impl(&c, cams[0].K, cams[0].baseline, rows, cols, p, device, 3 * n_sequences, n_sequences, min_caps);
  if(rc) return rc;
  for(int s = 0; s < n_sequences; ++s) assign_camera(c, s, &geoms[(size_t) s * kMaxLevels]);
  c->vo_mode = 2;      // (its slots carry the sequences' cameras: bpvo_hip_add_frame would read frames of the context's size into them)
  *out = c;
  return BPVO_OK;
}
int bpvo_hip_seq_set_camera(bpvo_hip_ctx* c, int seq, const bpvo_hip_camera* cam)
{
  CHECK_CTX(c); CHECK_SEQ(c, seq);
  if(!cam) return fail(c, BPVO_ERR_INVALID_ARG, "nullptr camera");
  if(c->vo_mode == 1) return fail(c, BPVO_ERR_INVALID_ARG, "this context runs bpvo_hip_add_frame: per-sequence cameras serve bpvo_hip_add_frames");
  int rc = seq_is_fresh(c, seq, "camera changes");
  if(rc) return rc;
  LevelGeom g[kMaxLevels];
  std::string why;
  rc = camera_geometry(*cam, c->params, c->auto_levels, c->L, g, &why);
  if(rc) return seq_fail(c, rc, seq, why.c_str());
  if(cam->rows > c->rows || cam->cols > c->cols) return camera_too_large(c, seq, cam->rows, cam->cols);
  for(int l = 0; l < c->L; ++l)
    if(g[l].cap > c->geom[l].cap)
      return seq_fail(c, BPVO_ERR_UNSUPPORTED, seq, ("camera needs a template capacity of " + std::to_string(g[l].cap) + " points at level " + std::to_string(l) +
                                                     ", the context holds " + std::to_string(c->geom[l].cap)).c_str());
  rc = rect_clear(c, seq);      // (its rectification was made for the camera that goes: the destination size and K' may have changed)
  if(rc) return rc;
  assign_camera(c, seq, g);
  c->vo_mode = 2;      // a context with per-sequence cameras serves bpvo_hip_add_frames
  return BPVO_OK;
}
int bpvo_hip_seq_get_camera(const bpvo_hip_ctx* c, int seq, bpvo_hip_camera* cam)
{
  if(!c || !cam || seq < 0 || seq >= seq_capacity(c)) return BPVO_ERR_INVALID_ARG;
  const LevelGeom& g = slot_geom(c, c->frames[3 * seq], 0);
  std::memcpy(cam->K, g.K, sizeof(cam->K));
  cam->baseline = g.b;
  cam->rows = g.rows; cam->cols = g.cols;
  return BPVO_OK;
}

// ---- per-sequence algorithm parameters ---------------------------------------------------------------------------------------------------
// What a sequence may own is what travels in its jobs (the Gauss-Newton limits and tolerances, the loss, the good-point threshold: PairJob; the
// selection thresholds: FrameJob) or is decided on the host per sequence (the key-frame thresholds).  What sizes the context's storage or
// instantiates its kernels — the pyramid, the descriptor, the gradient and interpolation forms, the non-maximum suppression, maxTestLevel — is
// fixed at creation: a difference there is BPVO_ERR_UNSUPPORTED, named in the error string.
static bool structural_difference(const bpvo_hip_ctx* c, int seq, const bpvo_hip_params& p, std::string* why)
{
  const bpvo_hip_params& q = c->params;
  auto differs = [&](const char* name, const std::string& a, const std::string& b) {
    *why = std::string(name) + " = " + a + " differs from the context's " + b + " (it fixes the context's storage or kernels: set at creation only)";
    return true;
  };
  auto fstr = [](float v) { char buf[48]; std::snprintf(buf, sizeof(buf), "%.9g", (double) v); return std::string(buf); };
#define SP_INT(field) if(p.field != q.field) return differs(#field, std::to_string(p.field), std::to_string(q.field))
#define SP_FLT(field) if(std::memcmp(&p.field, &q.field, sizeof(float)) != 0) return differs(#field, fstr(p.field), fstr(q.field))
  SP_INT(minImageDimensionForPyramid);
  {
    // numPyramidLevels after resolution (bpvo/vo.cc:101-105, for the sequence's own image size, as bpvo_hip_create counts them)
    const LevelGeom& g = slot_geom(c, c->frames[3 * seq], 0);
    const int own = p.numPyramidLevels > 0 ? p.numPyramidLevels : auto_pyramid_levels(g.rows, g.cols, p.minImageDimensionForPyramid);
    if(own != c->L) return differs("numPyramidLevels", std::to_string(own), std::to_string(c->L));
  }
  SP_INT(descriptor);
  SP_FLT(sigmaPriorToCensusTransform); SP_FLT(sigmaBitPlanes); SP_FLT(dfSigma1); SP_FLT(dfSigma2);
  SP_INT(latchNumBytes); SP_INT(latchRotationInvariance); SP_INT(latchHalfSsdSize);
  SP_INT(centralDifferenceRadius); SP_FLT(centralDifferenceSigmaBefore); SP_FLT(centralDifferenceSigmaAfter);
  SP_INT(laplacianKernelSize);
  SP_INT(gradientEstimation); SP_INT(interp); SP_INT(withNormalization);
  SP_INT(nonMaxSuppRadius); SP_INT(minNumPixelsForNonMaximaSuppression);
  SP_INT(maxTestLevel);
#undef SP_INT
#undef SP_FLT
  return false;
}
// does anything the library reads per sequence (or per rig) differ between two parameter sets?
static bool params_differ_where_read(const bpvo_hip_params& p, const bpvo_hip_params& o)
{
  return p.lossFunction != o.lossFunction || p.maxIterations != o.maxIterations || p.parameterTolerance != o.parameterTolerance ||
         p.functionTolerance != o.functionTolerance || p.gradientTolerance != o.gradientTolerance ||
         p.minTranslationMagToKeyFrame != o.minTranslationMagToKeyFrame || p.minRotationMagToKeyFrame != o.minRotationMagToKeyFrame ||
         p.maxFractionOfGoodPointsToKeyFrame != o.maxFractionOfGoodPointsToKeyFrame || p.goodPointThreshold != o.goodPointThreshold ||
         p.minSaliency != o.minSaliency || p.minValidDisparity != o.minValidDisparity || p.maxValidDisparity != o.maxValidDisparity;
}
int bpvo_hip_seq_set_params(bpvo_hip_ctx* c, int seq, const bpvo_hip_params* p)
{
  CHECK_CTX(c); CHECK_SEQ(c, seq);
  if(!p) return fail(c, BPVO_ERR_INVALID_ARG, "nullptr parameters");
  if(c->vo_mode == 1) return fail(c, BPVO_ERR_INVALID_ARG, "this context runs bpvo_hip_add_frame: per-sequence parameters serve bpvo_hip_add_frames");
  const int rc = seq_is_fresh(c, seq, "parameters change");
  if(rc) return rc;
  std::string why;
  if(structural_difference(c, seq, *p, &why)) return seq_fail(c, BPVO_ERR_UNSUPPORTED, seq, why.c_str());
  if(p->lossFunction != BPVO_LOSS_HUBER && p->lossFunction != BPVO_LOSS_TUKEY && p->lossFunction != BPVO_LOSS_L2 && p->lossFunction != BPVO_LOSS_STUDENT_T)
    return seq_fail(c, BPVO_ERR_UNSUPPORTED, seq, "unknown lossFunction");      // (bpvo_hip_create's answer)
  seq_states(c);
  SeqState& q = c->seqs[seq];
  const bpvo_hip_params& o = c->params;
  q.params = *p;
  // does anything the library reads differ from the context's?  (No: the sequence stays on the plain path, whatever the unread fields say)
  q.own_params = params_differ_where_read(*p, o);
  for(int k = 0; k < 3; ++k) c->frames[3 * seq + k].seq_params = q.own_params ? &q.params : nullptr;
  c->vo_mode = 2;      // a context with per-sequence parameters serves bpvo_hip_add_frames
  return BPVO_OK;
}
int bpvo_hip_seq_get_params(const bpvo_hip_ctx* c, int seq, bpvo_hip_params* p)
{
  if(!c || !p || seq < 0 || seq >= seq_capacity(c)) return BPVO_ERR_INVALID_ARG;
  *p = c->seqs.empty() ? c->params : c->seqs[seq].params;
  return BPVO_OK;
}
// A rig's parameters: the fields a sequence may own (bpvo_hip_seq_set_params), for all its members and its body — one rig, one parameter set
int bpvo_hip_rigs_set_params(bpvo_hip_ctx* c, int rig, const bpvo_hip_params* p)
{
  CHECK_CTX(c); CHECK_RIG(c, rig);
  if(!p) return fail(c, BPVO_ERR_INVALID_ARG, "nullptr parameters");
  RigState& g = c->rigs[rig];
  for(int s : g.seq)
    if(int rc = seq_is_fresh(c, s, "rig's parameters change")) return rc;
  std::string why;
  for(int s : g.seq)
    if(structural_difference(c, s, *p, &why)) return fail(c, BPVO_ERR_UNSUPPORTED, ("rig " + std::to_string(rig) + ": " + why).c_str());
  if(p->lossFunction != BPVO_LOSS_HUBER && p->lossFunction != BPVO_LOSS_TUKEY && p->lossFunction != BPVO_LOSS_L2 && p->lossFunction != BPVO_LOSS_STUDENT_T)
    return fail(c, BPVO_ERR_UNSUPPORTED, ("rig " + std::to_string(rig) + ": unknown lossFunction").c_str());
  g.body.params = *p;
  g.body.own_params = params_differ_where_read(*p, c->params);
  rig_param_target(c, g);
  return BPVO_OK;
}
int bpvo_hip_rigs_get_params(const bpvo_hip_ctx* c, int rig, bpvo_hip_params* p)
{
  if(!c || !p || rig < 0 || (size_t) rig >= c->rigs.size()) return BPVO_ERR_INVALID_ARG;
  *p = c->rigs[rig].body.params;
  return BPVO_OK;
}

// ---- the start policy's setters and records (extensions; the rule and its refusals: vo_state.h) ---------------------------------------------
// BPVO_OK, or why the context refuses the policy (nothing is changed)
static int start_policy_check(bpvo_hip_ctx* c, const bpvo_hip_start_policy* pol)
{
  if(!pol) return fail(c, BPVO_ERR_INVALID_ARG, "nullptr start policy");
  if(const char* why = vo_start_policy_refusal(*pol, c->L, c->params.maxTestLevel)) return fail(c, BPVO_ERR_INVALID_ARG, why);
  if(pol->mode == BPVO_START_SCORED) return pose_score_served(c);
  return BPVO_OK;
}
static int start_hints_set(bpvo_hip_ctx* c, SeqState& q, int n, const float* M)
{
  if(const char* why = vo_start_hints_refusal(body_policy(c, q), n, M)) return fail(c, BPVO_ERR_INVALID_ARG, why);
  vo_set_start_hints(q, n, M);
  return BPVO_OK;
}
static int start_info_get(bpvo_hip_ctx* c, const SeqState* q, int which, bpvo_hip_start_info* out)
{
  if(!out) return fail(c, BPVO_ERR_INVALID_ARG, "nullptr start info");
  if(which < 0 || which > 1) return fail(c, BPVO_ERR_INVALID_ARG, "start info: which must be 0 (against the key frame the call began with) or 1 (the re-estimate)");
  if(q) *out = q->start[which];
  else std::memset(out, 0, sizeof(*out));
  return BPVO_OK;
}
static int seq_not_in_a_rig(bpvo_hip_ctx* c, int seq, const char* what)
{
  for(const RigState& g : c->rigs)
    for(int s : g.seq)
      if(s == seq) return seq_fail(c, BPVO_ERR_INVALID_ARG, seq, (std::string("is a member of a rig: ") + what + " belong to the rig's body (bpvo_hip_rigs_set_start_policy / _hints)").c_str());
  return BPVO_OK;
}
int bpvo_hip_set_start_policy(bpvo_hip_ctx* c, const bpvo_hip_start_policy* policy)
{
  CHECK_CTX(c);
  if(int rc = start_policy_check(c, policy)) return rc;
  c->start_policy = *policy;
  return BPVO_OK;
}
int bpvo_hip_get_start_policy(const bpvo_hip_ctx* c, bpvo_hip_start_policy* policy)
{
  if(!c || !policy) return BPVO_ERR_INVALID_ARG;
  *policy = c->start_policy;
  return BPVO_OK;
}
int bpvo_hip_seq_set_start_policy(bpvo_hip_ctx* c, int seq, const bpvo_hip_start_policy* policy)
{
  CHECK_CTX(c); CHECK_SEQ(c, seq);
  if(int rc = seq_not_in_a_rig(c, seq, "a start policy and hints")) return rc;
  if(policy)
    if(int rc = start_policy_check(c, policy)) return rc;
  seq_states(c);
  SeqState& q = c->seqs[seq];
  q.own_policy = policy != nullptr;
  if(policy) q.policy = *policy;
  return BPVO_OK;
}
int bpvo_hip_seq_get_start_policy(const bpvo_hip_ctx* c, int seq, bpvo_hip_start_policy* policy, int* own)
{
  if(!c || !policy || seq < 0 || seq >= seq_capacity(c)) return BPVO_ERR_INVALID_ARG;
  const SeqState* q = seq_state(c, seq);
  *policy = q ? body_policy(c, *q) : c->start_policy;
  if(own) *own = q && q->own_policy ? 1 : 0;
  return BPVO_OK;
}
int bpvo_hip_rigs_set_start_policy(bpvo_hip_ctx* c, int rig, const bpvo_hip_start_policy* policy)
{
  CHECK_CTX(c); CHECK_RIG(c, rig);
  if(policy)
    if(int rc = start_policy_check(c, policy)) return rc;
  SeqState& q = c->rigs[rig].body;
  q.own_policy = policy != nullptr;
  if(policy) q.policy = *policy;
  return BPVO_OK;
}
int bpvo_hip_rigs_get_start_policy(const bpvo_hip_ctx* c, int rig, bpvo_hip_start_policy* policy, int* own)
{
  if(!c || !policy || rig < 0 || (size_t) rig >= c->rigs.size()) return BPVO_ERR_INVALID_ARG;
  *policy = body_policy(c, c->rigs[rig].body);
  if(own) *own = c->rigs[rig].body.own_policy ? 1 : 0;
  return BPVO_OK;
}
int bpvo_hip_vo_set_start_hints(bpvo_hip_ctx* c, int n, const float* M) { CHECK_CTX(c); return start_hints_set(c, c->vo, n, M); }
int bpvo_hip_seq_set_start_hints(bpvo_hip_ctx* c, int seq, int n, const float* M)
{
  CHECK_CTX(c); CHECK_SEQ(c, seq);
  if(int rc = seq_not_in_a_rig(c, seq, "a start policy and hints")) return rc;
  seq_states(c);
  return start_hints_set(c, c->seqs[seq], n, M);
}
int bpvo_hip_rigs_set_start_hints(bpvo_hip_ctx* c, int rig, int n, const float* M)
{
  CHECK_CTX(c); CHECK_RIG(c, rig);
  return start_hints_set(c, c->rigs[rig].body, n, M);
}
int bpvo_hip_vo_start_info(bpvo_hip_ctx* c, int which, bpvo_hip_start_info* out) { CHECK_CTX(c); return start_info_get(c, &c->vo, which, out); }
int bpvo_hip_seq_start_info(bpvo_hip_ctx* c, int seq, int which, bpvo_hip_start_info* out)
{
  CHECK_CTX(c); CHECK_SEQ(c, seq);
  return start_info_get(c, seq_state(c, seq), which, out);
}
int bpvo_hip_rigs_start_info(bpvo_hip_ctx* c, int rig, int which, bpvo_hip_start_info* out)
{
  CHECK_CTX(c); CHECK_RIG(c, rig);
  return start_info_get(c, &c->rigs[rig].body, which, out);
}
#undef CHECK_RIG
#undef CHECK_SEQ

}  // extern "C"
