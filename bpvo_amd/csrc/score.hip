// libbpvo_hip, host side: pose scoring (c_api.h bpvo_hip_score_poses; kernels_score.hip the kernels, pose_score_math.h the finish).  A call builds
// COPIES of its pairs' jobs with every workspace pointer cleared — the kernels read the template, the descriptor and the geometry only —, uploads
// them and the poses, queues the two launches on the context's stream and copies the records back.  Nothing a later call reads is written.
#include "host_ctx.h"
#include "pose_score_math.h"

using namespace bpvo_hip;
using namespace bpvo_hip_host;

namespace bpvo_hip_host {

int pose_score_served(bpvo_hip_ctx* c)
{
  if(c->params.interp != BPVO_INTERP_LINEAR) {
    const char* kind = c->params.interp == BPVO_INTERP_COSINE ? "kCosine" : c->params.interp == BPVO_INTERP_CUBIC ? "kCubic" : "kCubicHermite";
    return fail(c, BPVO_ERR_UNSUPPORTED, (std::string("pose score: kLinear interpolation only, this context runs ") + kind).c_str());
  }
  if(c->G > 1 || c->C > 48)
    return fail(c, BPVO_ERR_UNSUPPORTED, ("pose score: descriptors of at most 48 channels only, this context's has " + std::to_string(c->C)).c_str());
  return BPVO_OK;
}

int score_pairs(bpvo_hip_ctx* c, int n_pairs, const int* refs, const int* curs, int level, int n_poses, const float* T, float tau,
                bpvo_hip_pose_score* out)
{
  if(!refs || !curs || !T || !out) return fail(c, BPVO_ERR_INVALID_ARG, "pose score: nullptr slots / poses / records");
  if(n_pairs < 1 || n_pairs > 65535) return fail(c, BPVO_ERR_INVALID_ARG, "pose score: n_pairs must be within 1 .. 65535");
  if(n_poses < 1 || n_poses > (1 << 20)) return fail(c, BPVO_ERR_INVALID_ARG, "pose score: n_poses must be within 1 .. 1048576");
  if(!(tau > 0.0f) || !std::isfinite(tau)) return fail(c, BPVO_ERR_INVALID_ARG, "pose score: tau must be finite and positive");
  CHECK_LEVEL(c, level);
  for(int i = 0; i < n_pairs; ++i) { CHECK_SLOT(c, refs[i]); CHECK_SLOT(c, curs[i]); }
  if(int rc = pose_score_served(c)) return rc;
  for(int i = 0; i < n_pairs; ++i) {
    if(!c->frames[refs[i]].has_template) return fail(c, BPVO_ERR_NO_TEMPLATE, "pose score: reference frame has no template");
    if(!c->frames[curs[i]].has_data) return fail(c, BPVO_ERR_NO_DATA, "pose score: no data in frame");
  }
  for(int i = 0; i < n_pairs; ++i)
    if(int rc = ensure_dense_descriptor(c, curs[i])) return rc;
  (void) hipSetDevice(c->device);
  hipStream_t s = c->stream;

  std::vector<PairJob> h_jobs((size_t) n_pairs);
  int max_points = 0;
  for(int i = 0; i < n_pairs; ++i) {
    PairJob& pj = h_jobs[(size_t) i];
    pj = make_pair_job(c, 0, refs[i], curs[i], level);
    pj.r = nullptr; pj.valid = nullptr; pj.tapkey = nullptr; pj.tapcache = nullptr; pj.tapcache_on = 0; pj.cand = nullptr; pj.med_blk = nullptr;
    pj.partials = nullptr; pj.cnt = nullptr; pj.st = nullptr; pj.ticket = nullptr; pj.trace = nullptr; pj.trace_cap = 0;
    pj.grad = nullptr; pj.nrm = nullptr;
    max_points = std::max(max_points, pj.n);
  }
  const size_t records = (size_t) n_pairs * (size_t) n_poses;
  const int chunks = score_chunks(max_points);
  ScoreScratch& k = c->score;
  // (nothing of an earlier call is in flight when the scratch grows: every call ends with a synchronisation)
  HIP_CK(c, k.d_jobs.reserve((size_t) n_pairs));
  HIP_CK(c, k.d_T.reserve(records * 16));
  HIP_CK(c, k.d_partials.reserve(records * (size_t) chunks));
  HIP_CK(c, k.d_out.reserve(records));

  HIP_CK(c, hipMemcpyAsync(k.d_jobs, h_jobs.data(), sizeof(PairJob) * (size_t) n_pairs, hipMemcpyHostToDevice, s));
  HIP_CK(c, hipMemcpyAsync(k.d_T, T, sizeof(float) * 16 * records, hipMemcpyHostToDevice, s));
  ScoreLaunch g;
  g.jobs = k.d_jobs; g.n_pairs = n_pairs; g.n_poses = n_poses; g.max_points = max_points;
  g.C = c->C; g.fast_warp = c->fast_warp; g.tau = tau;
  g.T = k.d_T; g.partials = k.d_partials; g.out = k.d_out;
  // poses per workgroup: as many as leave the launch about four workgroups per CU (a pose more in a tile saves one load of the point and its
  // template values, a workgroup fewer leaves a CU idle); n_poses above 65535 tiles: the full tile
  const size_t work = (size_t) chunks * records;
  const size_t wanted = 4 * (size_t) std::max(64, c->device_cus);
  g.tile = (int) std::max<size_t>(1, std::min<size_t>((size_t) kScoreTile, work / wanted));
  if((n_poses + g.tile - 1) / g.tile > 65535) g.tile = kScoreTile;
  launch_score_poses(s, g);
  HIP_CK(c, hipGetLastError());
  HIP_CK(c, hipMemcpyAsync(out, k.d_out, sizeof(bpvo_hip_pose_score) * records, hipMemcpyDeviceToHost, s));
  HIP_CK(c, hipStreamSynchronize(s));
  HIP_CK(c, hipGetLastError());
  return BPVO_OK;
}

}  // namespace bpvo_hip_host

extern "C" {

int bpvo_hip_score_poses(bpvo_hip_ctx* c, int ref_slot, int cur_slot, int level, int n_poses, const float* T, float tau, bpvo_hip_pose_score* out)
{
  CHECK_CTX(c);
  return score_pairs(c, 1, &ref_slot, &cur_slot, level, n_poses, T, tau, out);
}

int bpvo_hip_score_poses_pairs(bpvo_hip_ctx* c, int n_pairs, const int* refs, const int* curs, int level, int n_poses, const float* T, float tau,
                               bpvo_hip_pose_score* out)
{
  CHECK_CTX(c);
  return score_pairs(c, n_pairs, refs, curs, level, n_poses, T, tau, out);
}

int bpvo_hip_estimate_pose_best_start(bpvo_hip_ctx* c, int ws, int ref_slot, int cur_slot, int n_cands, const float* T_cands, int score_level, float tau,
                                      float T_est[16], bpvo_hip_stats* stats, int* chosen, bpvo_hip_pose_score* scores)
{
  CHECK_CTX(c); CHECK_WS(c, ws);
  if(!T_cands || !T_est) return fail(c, BPVO_ERR_INVALID_ARG, "nullptr pose");
  if(n_cands < 1) return fail(c, BPVO_ERR_INVALID_ARG, "pose score: n_poses must be within 1 .. 1048576");
  const int level = score_level < 0 ? c->L - 1 : score_level;
  std::vector<bpvo_hip_pose_score> sc((size_t) n_cands);
  if(int rc = score_pairs(c, 1, &ref_slot, &cur_slot, level, n_cands, T_cands, tau, sc.data())) return rc;
  std::vector<double> v((size_t) n_cands);
  for(int i = 0; i < n_cands; ++i) v[(size_t) i] = sc[(size_t) i].score;
  const int best = pose_score_argmin(v.data(), n_cands);
  if(scores) std::memcpy(scores, sc.data(), sizeof(bpvo_hip_pose_score) * (size_t) n_cands);
  if(chosen) *chosen = best;
  return bpvo_hip_estimate_pose(c, ws, ref_slot, cur_slot, T_cands + 16 * (size_t) best, T_est, stats);
}

}  // extern "C"
