// libbpvo_hip, host side: the pose-covariance pass (c_api.h bpvo_hip_pose_covariances; kernels_gn_cov.hip the kernels, pose_cov_math.h the f64
// finish).  Per group of up to CovScratch::group members: copies of the workspaces' jobs whose residuals, valid flags, partials, counters and
// state point into the pass's scratch, one upload of the tables, then prepare -> warp_residual (the chain's own) -> reduce -> finish and one copy of
// the records back.  Nothing a later call reads is written: the workspaces stay as their estimates left them.
#include "host_ctx.h"

using namespace bpvo_hip;
using namespace bpvo_hip_host;

namespace bpvo_hip_host {

void pose_cov_none(bpvo_hip_pose_covariance* r)
{
  std::memset(r, 0, sizeof(*r));
  for(int i = 0; i < 16; ++i) r->T[i] = (i % 5 == 0) ? 1.0f : 0.0f;
  for(int i = 0; i < 36; ++i) r->covariance[i] = (i % 7 == 0) ? 1.0f : 0.0f;
  r->level = -1;
  r->status = BPVO_COV_NONE;
}

static int pose_cov_supported(bpvo_hip_ctx* c)
{
  if(c->G > 1 || c->C > 48) return fail(c, BPVO_ERR_UNSUPPORTED, "pose covariance: descriptors of more than 48 channels are not served (the channels of a point are one cluster)");
  return BPVO_OK;
}

int pose_cov_ensure_scratch(bpvo_hip_ctx* c)
{
  if(int rc = pose_cov_supported(c)) return rc;
  CovScratch& k = c->cov;
  if(k.d_slab) return BPVO_OK;
  (void) hipSetDevice(c->device);
  const int group = std::max(1, std::min(BPVO_HIP_COV_GROUP, c->n_pairs));
  // a slot holds the largest template of the context (the finest level's, wherever the levels differ)
  const size_t r_floats = tiled_floats(c->cap_max, c->C);
  const size_t valid_bytes = align_up((size_t) c->cap_max);
  const size_t partial_floats = (size_t) pose_cov_partials_floats(c->cap_max, c->C);
  // the tables of a group, one contiguous upload: jobs, members, poses, scales, extrinsics
  Carver t{nullptr};
  t.take<PairJob>((size_t) group);
  const size_t off_members = t.off; t.take<CovMember>((size_t) group);
  const size_t off_T = t.off; t.take<float>((size_t) group * 16);
  const size_t off_sigma = t.off; t.take<float>((size_t) group);
  const size_t off_X = t.off; t.take<float>((size_t) group * 16);
  const size_t tables_bytes = t.off;
  auto carve = [&](unsigned char* base, CovScratch* out) {
    Carver cv{base};
    float* r = cv.take<float>((size_t) group * r_floats);
    uint8_t* valid = cv.take<uint8_t>((size_t) group * valid_bytes);
    float* partials = cv.take<float>((size_t) group * partial_floats);
    unsigned long long* cnt = cv.take<unsigned long long>((size_t) group * kWsCounters);
    GNState* states = cv.take<GNState>((size_t) group);
    unsigned char* tables = cv.take<unsigned char>(tables_bytes);
    bpvo_hip_pose_covariance* d_out = cv.take<bpvo_hip_pose_covariance>((size_t) group);
    float* sums = cv.take<float>((size_t) c->n_pairs * 72);
    if(out) { out->d_r = r; out->d_valid = valid; out->d_partials = partials; out->d_cnt = cnt; out->d_states = states; out->d_tables = tables; out->d_out = d_out; out->d_sums = sums; }
    return cv.off;
  };
  const size_t total = carve(nullptr, nullptr);
  // (local owners: the scratch is the context's only once all of it exists)
  DeviceBuf<unsigned char> slab;
  PinnedBuf<unsigned char> h_tables;
  PinnedBuf<bpvo_hip_pose_covariance> h_out;
  HIP_CK(c, slab.alloc(total));
  HIP_CK(c, hipMemset(slab, 0, total));
  HIP_CK(c, h_tables.alloc(tables_bytes));
  HIP_CK(c, h_out.alloc((size_t) group));
  k.group = group;
  k.r_floats = r_floats; k.valid_bytes = valid_bytes; k.partial_floats = partial_floats;
  carve(slab, &k);
  k.d_slab = std::move(slab); k.h_tables = std::move(h_tables); k.h_out = std::move(h_out);
  k.tables_bytes = tables_bytes; k.off_members = off_members; k.off_T = off_T; k.off_sigma = off_sigma; k.off_X = off_X;
  return BPVO_OK;
}

int pose_cov_pass(bpvo_hip_ctx* c, int n_records, int members, const int* wss, const int* refs, const int* curs, const float* X, int level,
                  const float* T, const float* sigma, const bpvo_hip_params* const* prms, bpvo_hip_pose_covariance* out)
{
  if(n_records <= 0) return BPVO_OK;
  if(int rc = pose_cov_ensure_scratch(c)) return rc;
  CovScratch& k = c->cov;
  if(members < 1 || members > k.group) return fail(c, BPVO_ERR_UNSUPPORTED, "pose covariance: a rig of more than BPVO_HIP_COV_GROUP members");
  (void) hipSetDevice(c->device);
  hipStream_t s = c->stream;
  HIP_CK(c, join_pending_normalization(c, s));
  const int per_group = k.group / members;      // records of one launch set
  PairJob* h_jobs = reinterpret_cast<PairJob*>(k.h_tables.get());
  CovMember* h_members = reinterpret_cast<CovMember*>(k.h_tables + k.off_members);
  float* h_T = reinterpret_cast<float*>(k.h_tables + k.off_T);
  float* h_sigma = reinterpret_cast<float*>(k.h_tables + k.off_sigma);
  float* h_X = reinterpret_cast<float*>(k.h_tables + k.off_X);
  for(int first = 0; first < n_records; first += per_group) {
    const int nr = std::min(per_group, n_records - first), nm = nr * members;
    int max_points = 0;
    unsigned losses = 0;      // bit 0 Huber, 1 Tukey, 2 L2, 3 Student-t: the losses present in the group (one launch of the reduction each)
    for(int m = 0; m < nm; ++m) {
      const int e = first * members + m;
      PairJob& pj = h_jobs[m];
      pj = make_pair_job(c, wss[e], refs[e], curs[e], level);
      if(prms) pair_job_set_params(pj, *prms[e]);
      h_members[m].src = c->d_states + wss[e];
      h_members[m].sums = k.d_sums + 72 * (size_t) wss[e];
      pj.r = k.d_r + (size_t) m * k.r_floats;
      pj.valid = k.d_valid + (size_t) m * k.valid_bytes;
      pj.partials = k.d_partials + (size_t) m * k.partial_floats;
      pj.cnt = k.d_cnt + (size_t) m * kWsCounters;
      pj.st = k.d_states + m;
      pj.tapcache_on = 0;
      pj.tapkey = nullptr; pj.tapcache = nullptr; pj.cand = nullptr; pj.med_blk = nullptr; pj.ticket = nullptr;
      pj.trace = nullptr; pj.trace_cap = 0;
      max_points = std::max(max_points, pj.n);
      losses |= pj.loss == BPVO_LOSS_HUBER ? 1u : pj.loss == BPVO_LOSS_TUKEY ? 2u : pj.loss == BPVO_LOSS_STUDENT_T ? 8u : 4u;
      if(sigma) h_sigma[m] = sigma[e];
    }
    if(T) std::memcpy(h_T, T + 16 * (size_t) first, sizeof(float) * 16 * (size_t) nr);
    if(X) std::memcpy(h_X, X, sizeof(float) * 16 * (size_t) members);
    HIP_CK(c, hipMemcpyAsync(k.d_tables, k.h_tables, k.tables_bytes, hipMemcpyHostToDevice, s));
    CovLaunch g;
    g.jobs = reinterpret_cast<const PairJob*>(k.d_tables);
    g.members_tab = reinterpret_cast<const CovMember*>(k.d_tables + k.off_members);
    g.n_records = nr; g.members = members;
    g.T = T ? reinterpret_cast<const float*>(k.d_tables + k.off_T) : nullptr;
    g.sigma = sigma ? reinterpret_cast<const float*>(k.d_tables + k.off_sigma) : nullptr;
    g.X = X ? reinterpret_cast<const float*>(k.d_tables + k.off_X) : nullptr;
    g.level = level;
    g.max_points = max_points; g.C = c->C; g.loss = c->params.lossFunction;
    g.out = k.d_out;
    launch_pose_cov_prepare(s, g);
    // the residuals at the pose: the chain's warp_residual on the copies (every descriptor, interpolation and warp formulation)
    GNLaunch w = level_launch(c, g.jobs, nm, max_points, g.loss);
    w.dense_candidates = 0;      // (the copies hold no candidate buffers: warp_residual reads this field, and no median follows)
    LinearizeFlags warp_only;
    warp_only.median = warp_only.reduce = warp_only.step = false;
    linearize_launches(c, &c->lanes[0], w, 0, warp_only);      // (lane 0 is the context's stream)
    for(int b = 0; b < 4; ++b)
      if(losses & (1u << b)) {
        g.loss = b == 0 ? BPVO_LOSS_HUBER : b == 1 ? BPVO_LOSS_TUKEY : b == 2 ? BPVO_LOSS_L2 : BPVO_LOSS_STUDENT_T;
        launch_pose_cov_reduce(s, g);
      }
    launch_pose_cov_finish(s, g);
    HIP_CK(c, hipMemcpyAsync(k.h_out, k.d_out, sizeof(bpvo_hip_pose_covariance) * (size_t) nr, hipMemcpyDeviceToHost, s));
    HIP_CK(c, hipStreamSynchronize(s));      // (the pinned tables are rewritten by the next group)
    HIP_CK(c, hipGetLastError());
    std::memcpy(out + first, k.h_out, sizeof(bpvo_hip_pose_covariance) * (size_t) nr);
  }
  return BPVO_OK;
}

// the checks of the stateless calls; level_io: the level asked for, or (no pose given) the level the workspaces' estimates ended on
static int pose_cov_check(bpvo_hip_ctx* c, int n, const int* wss, const int* refs, const int* curs, bool given, int* level_io)
{
  if(int rc = pose_cov_supported(c)) return rc;
  if(n < 1 || !wss || !refs || !curs) return fail(c, BPVO_ERR_INVALID_ARG, "pose covariance: n < 1 or nullptr workspaces / frame slots");
  if(!given) *level_io = c->params.maxTestLevel;
  const int level = *level_io;
  CHECK_LEVEL(c, level);
  if(int rc = check_pairs(c, n, wss, refs, curs, 0, -1)) return rc;      // (an empty template level is answered by its record: no level check)
  for(int i = 0; i < n; ++i) {
    const Workspace& w = c->ws[wss[i]];
    if(!given && !(w.has_estimate && w.last_ref == refs[i] && w.last_cur == curs[i] && w.last_level == level))
      return fail(c, BPVO_ERR_NO_DATA, "pose covariance: the workspace holds no estimate of this pair (give T and sigma)");
  }
  return BPVO_OK;
}

}  // namespace bpvo_hip_host

extern "C" {

int bpvo_hip_pose_covariances(bpvo_hip_ctx* c, int n, const int* wss, const int* refs, const int* curs, int level, const float* T, const float* sigma,
                              bpvo_hip_pose_covariance* out)
{
  CHECK_CTX(c);
  if(!out) return fail(c, BPVO_ERR_INVALID_ARG, "nullptr records");
  if((T == nullptr) != (sigma == nullptr)) return fail(c, BPVO_ERR_INVALID_ARG, "pose covariance: T and sigma both given, or both NULL");
  if(int rc = pose_cov_check(c, n, wss, refs, curs, T != nullptr, &level)) return rc;
  return pose_cov_pass(c, n, 1, wss, refs, curs, nullptr, level, T, sigma, nullptr, out);
}

int bpvo_hip_pose_covariance_rig(bpvo_hip_ctx* c, int n, const int* wss, const int* refs, const int* curs, const float* X, int level, const float* T_body,
                                 const float* sigma, bpvo_hip_pose_covariance* out)
{
  CHECK_CTX(c);
  if(!out || !X) return fail(c, BPVO_ERR_INVALID_ARG, "nullptr record / extrinsics");
  if((T_body == nullptr) != (sigma == nullptr)) return fail(c, BPVO_ERR_INVALID_ARG, "pose covariance: T_body and sigma both given, or both NULL");
  if(c->dspace) return fail(c, BPVO_ERR_UNSUPPORTED, "rig mode does not serve BPVO_WARP_DISPARITY_SPACE_F32");
  if(int rc = pose_cov_check(c, n, wss, refs, curs, T_body != nullptr, &level)) return rc;
  for(int i = 0; i < n; ++i) {
    for(int k = 0; k < i; ++k)
      if(wss[k] == wss[i]) return fail(c, BPVO_ERR_INVALID_ARG, "rig: a workspace appears twice");
    if(!rig_extrinsic_ok(X + 16 * (size_t) i)) return fail(c, BPVO_ERR_INVALID_ARG, "rig: an extrinsic is not a rigid transform (finite, last row 0 0 0 1, R^T R = I within 1e-4)");
  }
  return pose_cov_pass(c, 1, n, wss, refs, curs, X, level, T_body, sigma, nullptr, out);
}

int bpvo_hip_vo_pose_covariance(bpvo_hip_ctx* c, bpvo_hip_pose_covariance* out)
{
  CHECK_CTX(c);
  if(!out) return fail(c, BPVO_ERR_INVALID_ARG, "nullptr record");
  *out = c->vo_cov;
  return BPVO_OK;
}
int bpvo_hip_seq_pose_covariance(bpvo_hip_ctx* c, int seq, bpvo_hip_pose_covariance* out)
{
  CHECK_CTX(c);
  if(!out) return fail(c, BPVO_ERR_INVALID_ARG, "nullptr record");
  if(seq < 0 || seq >= std::min(c->n_frames / 3, c->n_pairs)) return fail(c, BPVO_ERR_INVALID_ARG, "no such sequence");
  if((size_t) seq < c->seq_cov.size()) *out = c->seq_cov[(size_t) seq];
  else pose_cov_none(out);
  return BPVO_OK;
}
int bpvo_hip_rig_pose_covariance(bpvo_hip_ctx* c, bpvo_hip_pose_covariance* out)
{
  CHECK_CTX(c);
  if(!out) return fail(c, BPVO_ERR_INVALID_ARG, "nullptr record");
  if(c->rigs.size() > 1) return fail(c, BPVO_ERR_INVALID_ARG, "this context declares several rigs (bpvo_hip_rigs_set): call bpvo_hip_rigs_pose_covariance");
  if(c->rigs.empty()) { pose_cov_none(out); return BPVO_OK; }
  return bpvo_hip_rigs_pose_covariance(c, 0, out);
}
int bpvo_hip_rigs_pose_covariance(bpvo_hip_ctx* c, int rig, bpvo_hip_pose_covariance* out)
{
  CHECK_CTX(c);
  if(!out) return fail(c, BPVO_ERR_INVALID_ARG, "nullptr record");
  if(rig < 0 || (size_t) rig >= c->rigs.size()) return fail(c, BPVO_ERR_INVALID_ARG, "no such rig (bpvo_hip_rigs_set declares rigs 0 .. n_rigs-1)");
  *out = c->rigs[(size_t) rig].cov;
  return BPVO_OK;
}

int bpvo_hip_debug_pose_covariance_sums(bpvo_hip_ctx* c, int ws, float M[36], float Q[36])
{
  CHECK_CTX(c); CHECK_WS(c, ws);
  if(!M || !Q) return fail(c, BPVO_ERR_INVALID_ARG, "nullptr sums");
  if(!c->cov.d_sums) return fail(c, BPVO_ERR_NO_DATA, "no pose-covariance pass has run on this context");
  (void) hipSetDevice(c->device);
  float h[72];
  HIP_CK(c, hipMemcpyAsync(h, c->cov.d_sums + 72 * (size_t) ws, sizeof(h), hipMemcpyDeviceToHost, c->stream));
  HIP_CK(c, hipStreamSynchronize(c->stream));
  std::memcpy(M, h, sizeof(float) * 36);
  std::memcpy(Q, h + 36, sizeof(float) * 36);
  return BPVO_OK;
}

}  // extern "C"
