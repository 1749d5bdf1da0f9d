// Pose covariance (gfx950): the robust sandwich estimate Sigma = M^-1 Q M^-1 of an estimated pose (c_api.h bpvo_hip_pose_covariances).
//   pose_cov_prepare  the pass's scratch states: pose, frozen scale and level of every member, given or from the workspace's last estimate
//   (warp_residual)   the chain's own kernel on the pass's copies of the jobs: residuals and valid flags at that pose, into the pass's scratch
//   pose_cov_reduce   per tile of points: M = sum d(u) J^T J (rank-2 form, d in the place of w) and Q = sum_p g_p^T g_p (one rank-1 update per
//                     point), wave tree + 4-wave LDS combine into per-tile partials                      (moved: irls_reduce's 18 + 12*C B/point)
//   pose_cov_finish   one wavefront per record: tile partials combined in tile order in f64 into the member's M_p, Q_p (kept as f32, like H and G of a
//                     linearisation: the debug accessor's values), then all in f64: brought to the body twist (B_p = A_p^-1 Ad(X_p)), added in member
//                     order, LDL^T of the curvature, two solves; the result narrowed to f32 once
#include <float.h>

#include "kernels.h"

#include "gn_common.h"
#include "gn_warp.h"
#include "gn_median.h"
#include "gn_irls.h"
#include "gn_step.h"
#include "gn_cov.h"
#include "pose_cov_math.h"

namespace bpvo_hip {

__global__ __launch_bounds__(64) void pose_cov_prepare_kernel(CovLaunch g)
{
  const int m = blockIdx.x * 64 + threadIdx.x;
  if(m >= g.n_records * g.members) return;
  const int rec = m / g.members, p = m - rec * g.members;
  GNState* st = g.jobs[m].st;
  const GNState* src = g.members_tab[m].src;
  if(g.T) {
    const float* T = g.T + 16 * (size_t) rec;
    if(g.X) rig_member_pose(g.X + 16 * (size_t) p, T, st->T);
    else
      for(int i = 0; i < 16; ++i) st->T[i] = T[i];
    st->scale = g.sigma[m];
    st->level = g.level;
  } else {
    for(int i = 0; i < 16; ++i) st->T[i] = src->T_out[i];
    st->scale = src->scale;
    st->level = src->level;
  }
  // frozen scale: warp_residual's bracket step and the median leave the state alone; active: the kernels of the chain run
  st->delta_scale = 0.0f;
  st->median_valid = 0;
  st->r_stale = 0;
  st->active = 1;
}

// three waves per SIMD are enough for a kernel that runs once per estimate (the 43 accumulators next to the loads of a point: 98 - 104 registers
// for C = 8, 156 for C = 24); the widest descriptors hold 3 x C loaded floats per point and get the registers of two waves / one wave instead of spilling
constexpr int cov_min_waves(int C) { return C <= 24 ? 3 : C <= 32 ? 2 : 1; }
template <int C, int LOSS>
__global__ __launch_bounds__(GN_BLOCK, cov_min_waves(C)) void pose_cov_reduce_kernel(const PairJob* __restrict__ jobs, int pts_per_block)
{
  const PairJob& j = jobs[blockIdx.y];
  if(j.loss != LOSS) return;      // (sequences with parameters of their own: a launch per loss of the call)
  if((int) blockIdx.x * pts_per_block >= j.n) return;
  __shared__ CovPartLds s_part;
  pose_cov_tile<C, LOSS>(j, j.st, pts_per_block, blockIdx.x, threadIdx.x, s_part, j.partials);
}

struct CovFinishLds {
  double packed[kCovNumM + kCovNumQ];   // the member's sums over its tiles: M (21), valid points, Q (21)
  double Mp[36], Qp[36];                // ... as symmetric matrices
  double Ai[36], Ad[36], B[36];         // A_p^-1, Ad(X_p), B_p = A_p^-1 Ad(X_p)
  double Mb[36], Qb[36];                // the joint sums in the body twist
  PoseCovScratch scratch;
  float X[16], nrm[4], cov[36];
  int status;
};

__global__ __launch_bounds__(64) void pose_cov_finish_kernel(CovLaunch g, int pts_per_block)
{
  __shared__ CovFinishLds s;
  const int lane = threadIdx.x, rec = blockIdx.x;
  const int ea = lane / 6, eb = lane % 6;
  const int ua = ea <= eb ? ea : eb, ub = ea <= eb ? eb : ea;      // a lane below the diagonal computes its mirror entry: the same sums, the same bits
  double accM = 0.0, accQ = 0.0, valid = 0.0;
  bool estimated = true;
  for(int p = 0; p < g.members; ++p) {
    const int m = rec * g.members + p;
    const PairJob& j = g.jobs[m];
    const int n = j.n;
    estimated = estimated && n > 0 && (g.T != nullptr || g.members_tab[m].src->level == g.level);
    if(lane < kCovNumM + kCovNumQ) {      // tile order, f64
      const int slot = lane < kCovNumM ? lane : kCovQAt + (lane - kCovNumM);
      const int tiles = n > 0 ? (n + pts_per_block - 1) / pts_per_block : 0;
      double v = 0.0;
      for(int t = 0; t < tiles; ++t) v += (double) j.partials[(size_t) t * kCovPartialStride + slot];
      s.packed[lane] = v;
    } else if(lane < kCovNumM + kCovNumQ + 4) {
      const int k = lane - (kCovNumM + kCovNumQ);
      s.nrm[k] = j.dspace ? (k == 0 ? 1.0f : 0.0f) : j.nrm[k];
    }
    if(lane < 16) s.X[lane] = g.X ? g.X[16 * (size_t) p + lane] : ((lane % 5 == 0) ? 1.0f : 0.0f);
    wave_lds_sync();
    if(lane == 0) pose_cov_unpack(s.packed, s.Mp);
    if(lane == 1) pose_cov_unpack(s.packed + kCovNumM, s.Qp);
    if(lane == 2) rig_normalization_map_inverse(s.nrm, s.Ai);
    if(lane == 3) rig_adjoint(s.X, s.Ad);
    wave_lds_sync();
    if(lane < 36) {
      s.B[lane] = rig_body_map_at(s.Ai, s.Ad, ea, eb);
      // the member's sums are narrowed to f32 here, like H and G of a linearisation: what bpvo_hip_debug_pose_covariance_sums returns IS what
      // the f64 algebra below starts from (each lane its own entry)
      float* sums = g.members_tab[m].sums;
      const float mp = (float) s.Mp[lane], qp = (float) s.Qp[lane];
      sums[lane] = mp;
      sums[36 + lane] = qp;
      s.Mp[lane] = (double) mp;
      s.Qp[lane] = (double) qp;
    }
    wave_lds_sync();
    if(lane < 36) {
      accM += pose_cov_congruence_at(s.B, s.Mp, ua, ub);
      accQ += pose_cov_congruence_at(s.B, s.Qp, ua, ub);
    }
    valid += s.packed[kCovNumM - 1];
    wave_lds_sync();
  }
  if(lane < 36) { s.Mb[lane] = accM; s.Qb[lane] = accQ; }
  wave_lds_sync();
  if(lane == 0) s.status = pose_cov_finish(estimated, valid, s.Mb, s.Qb, s.cov, &s.scratch);
  wave_lds_sync();
  // the record: one dword per lane, plain vector stores
  bpvo_hip_pose_covariance* out = g.out + rec;
  const GNState* st0 = g.jobs[rec * g.members].st;      // member 0's scratch state: the pose and scale the pass ran at
  if(lane < 36) out->covariance[lane] = s.cov[lane];
  else if(lane < 52) {
    const int e = lane - 36;
    float t;
    if(g.T) t = g.T[16 * (size_t) rec + e];
    else if(g.X) t = e >= 12 ? (e == 15 ? 1.0f : 0.0f) : (float) rig_body_pose_at(g.X, st0->T, e >> 2, e & 3);      // X_0^-1 T_0 X_0
    else t = st0->T[e];
    out->T[e] = t;
  } else if(lane == 52) out->sigma = st0->scale;
  else if(lane == 53) out->num_valid = (int) valid;
  else if(lane == 54) out->level = g.T ? g.level : st0->level;
  else if(lane == 55) out->status = s.status;
}

int pose_cov_partials_floats(int cap, int C)
{
  const int ppb = gn_pts_per_block(C);
  return std::max(1, (cap + ppb - 1) / ppb) * kCovPartialStride;
}

void launch_pose_cov_prepare(hipStream_t s, const CovLaunch& g)
{
  const int n = g.n_records * g.members;
  if(n <= 0) return;
  hipLaunchKernelGGL(pose_cov_prepare_kernel, dim3((n + 63) / 64), dim3(64), 0, s, g);
}

template <int C>
static void launch_pose_cov_reduce_c(hipStream_t s, const CovLaunch& g, int ppb)
{
  const dim3 grid((g.max_points + ppb - 1) / ppb, g.n_records * g.members);
  switch(g.loss) {
    case BPVO_LOSS_HUBER: hipLaunchKernelGGL((pose_cov_reduce_kernel<C, BPVO_LOSS_HUBER>), grid, dim3(GN_BLOCK), 0, s, g.jobs, ppb); break;
    case BPVO_LOSS_TUKEY: hipLaunchKernelGGL((pose_cov_reduce_kernel<C, BPVO_LOSS_TUKEY>), grid, dim3(GN_BLOCK), 0, s, g.jobs, ppb); break;
    case BPVO_LOSS_STUDENT_T: hipLaunchKernelGGL((pose_cov_reduce_kernel<C, BPVO_LOSS_STUDENT_T>), grid, dim3(GN_BLOCK), 0, s, g.jobs, ppb); break;
    default: hipLaunchKernelGGL((pose_cov_reduce_kernel<C, BPVO_LOSS_L2>), grid, dim3(GN_BLOCK), 0, s, g.jobs, ppb); break;
  }
}
void launch_pose_cov_reduce(hipStream_t s, const CovLaunch& g)
{
  if(g.max_points <= 0 || g.n_records * g.members <= 0) return;
  const int ppb = gn_pts_per_block(g.C);
  dispatch_channels(g.C, [&](auto c) { launch_pose_cov_reduce_c<decltype(c)::value>(s, g, ppb); });
}
void launch_pose_cov_finish(hipStream_t s, const CovLaunch& g)
{
  if(g.n_records <= 0) return;
  hipLaunchKernelGGL(pose_cov_finish_kernel, dim3(g.n_records), dim3(64), 0, s, g, gn_pts_per_block(g.C));
}

}  // namespace bpvo_hip
