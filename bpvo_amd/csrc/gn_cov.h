// Pose covariance, device side (kernels_gn_cov.hip): the reduction of one tile of points into the curvature M = sum d(u) J^T J and the score
// covariance Q = sum_p g_p^T g_p of the robust sandwich estimate (c_api.h bpvo_hip_pose_covariances; pose_cov_math.h the f64 finish).
#pragma once
#include "gn_irls.h"

namespace bpvo_hip {

// per-tile partials of the pass: [0 .. 20] M (upper triangle, row by row), [21] valid points, [32 .. 52] Q
constexpr int kCovPartialStride = 64;
constexpr int kCovNumM = 22, kCovNumQ = 21, kCovQAt = 32;

// d(u) = psi'(u), the second derivative of the loss, next to mest_weight's w(u) = psi(u) / u — from the same f32 product r * sigma_inv
template <int LOSS>
__device__ __forceinline__ float mest_curvature(float r, float sigma_inv)
{
  if(LOSS == BPVO_LOSS_HUBER) {
    return (fabsf(r * sigma_inv) <= 1.345f) ? 1.0f : 0.0f;      // exactly where mest_weight is 1
  } else if(LOSS == BPVO_LOSS_TUKEY) {
    const float t = 4.685f;
    const float t_i = (float) (1.0 / 4.685f);
    const float x = r * sigma_inv;
    float q = x * t_i;
    q = q * q;
    return (fabsf(x) < t) ? (1.0f - q) * (1.0f - 5.0f * q) : 0.0f;
  } else if(LOSS == BPVO_LOSS_STUDENT_T) {      // psi(u) = 6 u / (5 + u^2): psi'(u) = 6 (5 - u^2) / (5 + u^2)^2, negative beyond |u| = sqrt(5)
    const float x = r * sigma_inv;
    const float x2 = x * x;
    const float den = 5.0f + x2;
    return (6.0f * (5.0f - x2)) / (den * den);
  }
  return 1.0f;
}

// One tile of points of workspace j by 256 threads: irls_tile's non-fused loads and rank-2 structure with d in the place of w for M, the
// point's score g_p = Gx A + Gy B and ONE 21-entry rank-1 update per point for Q (the channels of a point are one cluster).  Residuals and valid
// flags are those warp_residual left at the pose of j.st (a point behind the camera there counts as invalid, see below); the same wave tree and 4-wave LDS combine as the normal equations.
typedef float CovPartLds[4][kCovPartialStride];
template <int C, int LOSS>
__device__ __forceinline__ void pose_cov_tile(const PairJob& j, const GNState* __restrict__ st, int pts_per_block, int tile, int vtid, CovPartLds& s_part,
                                              float* __restrict__ partials)
{
  const int n = j.n;
  const int p_begin = tile * pts_per_block;
  const int p_end = min(n, p_begin + pts_per_block);
  const float sigma_inv = 1.0f / st->scale;
  const IrlsRowGeom geom = irls_row_geom(j);
  const float Tz[4] = {st->T[8], st->T[9], st->T[10], st->T[11]};      // uniform over the workgroup

  float accM[kCovNumM], accQ[kCovNumQ];
#pragma unroll
  for(int k = 0; k < kCovNumM; ++k) accM[k] = 0.0f;
#pragma unroll
  for(int k = 0; k < kCovNumQ; ++k) accQ[k] = 0.0f;

  for(int i = p_begin + vtid; i < p_end; i += GN_BLOCK) {
    float rr[C], Ix[C], Iy[C];
    const float4 Pt = load_point<true>(j, i);
    // cheirality: the warp's validity rule has no z > 0 test (a point behind the camera that projects into the image is valid for the estimate,
    // as in the reference); such a point tells nothing about the pose's uncertainty and counts as invalid HERE.  Its depth at the pose, f32:
    // row 2 of T on the point (DisparitySpaceWarp: on the point rebuilt from (x - cx, y - cy, d)).  In front of the camera nothing changes.
    float X3 = Pt.x, Y3 = Pt.y, Z3 = Pt.z;
    if(geom.dspace) { Z3 = (j.b * geom.ds_fx) / Pt.z; X3 = Pt.x * Z3 * geom.ds_fx_i; Y3 = Pt.y * Z3 * geom.ds_fy_i; }
    const float zc = ((Tz[0] * X3 + Tz[1] * Y3) + Tz[2] * Z3) + Tz[3];
    const float v = (zc > 0.0f) ? (float) j.valid[i] : 0.0f;
    accM[21] += v;
    irls_load_residuals<C>(j, i, rr);
    irls_load_gradients<C>(j, i, Ix, Iy);
    float Sxx = 0.0f, Sxy = 0.0f, Syy = 0.0f, Gx = 0.0f, Gy = 0.0f;
#pragma unroll
    for(int c = 0; c < C; ++c) {
      const float r = rr[c];
      const float d = mest_curvature<LOSS>(r, sigma_inv) * v;
      const float w = mest_weight<LOSS>(r, sigma_inv) * v;
      const float dx = d * Ix[c], dy = d * Iy[c];
      Sxx = irls_mad(dx, Ix[c], Sxx);
      Sxy = irls_mad(dx, Iy[c], Sxy);
      Syy = irls_mad(dy, Iy[c], Syy);
      const float wr = w * r;
      Gx = irls_mad(wr, Ix[c], Gx);
      Gy = irls_mad(wr, Iy[c], Gy);
    }
    float A[6], B[6];
    irls_point_rows(geom, Pt, A, B);
    irls_rank2_update(Sxx, Sxy, Syy, A, B, accM);
    float g[6];
#pragma unroll
    for(int a = 0; a < 6; ++a) g[a] = irls_mad(Gy, B[a], Gx * A[a]);
    int idx = 0;
#pragma unroll
    for(int a = 0; a < 6; ++a)
#pragma unroll
      for(int b = a; b < 6; ++b) { accQ[idx] = irls_mad(g[a], g[b], accQ[idx]); ++idx; }
  }

  const int lane = vtid & 63, wave = vtid >> 6;
  wave_tree_sums_to<kCovNumM>(accM, lane, s_part[wave]);
  wave_tree_sums_to<kCovNumQ>(accQ, lane, s_part[wave] + kCovQAt);
  __syncthreads();
  const bool is_m = vtid < kCovNumM, is_q = vtid >= kCovQAt && vtid < kCovQAt + kCovNumQ;
  if(is_m || is_q) partials[(size_t) tile * kCovPartialStride + vtid] = (s_part[0][vtid] + s_part[1][vtid]) + (s_part[2][vtid] + s_part[3][vtid]);
}

}  // namespace bpvo_hip
