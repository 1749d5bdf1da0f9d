// The small f64 algebra of the pose covariance (bpvo_hip_pose_covariances; include/bpvo_hip/c_api.h states the definition): the robust
// "sandwich" estimate  Sigma = M^-1 Q M^-1  from the curvature M = sum d(u) J^T J and the score covariance Q = sum_p g_p^T g_p, brought from
// each camera's Hartley-normalised twist to the plain body twist with the maps of rig_math.h.  Shared by the device-side finish
// (kernels_gn_cov.hip, one wavefront per record) and the CPU tests (tests/test_pose_covariance_cpu.py compiles this header with a plain C++
// compiler).  6x6 matrices are row-major double[36]; twists are ordered (omega, v).
//
//   member p           curvature M_p and score covariance Q_p in ITS normalised twist xi (what bpvo_hip_get_jacobians' J is taken in)
//   body twist         xi = B_p zeta,  B_p = A_p^-1 Ad(X_p)  (rig_body_map; one camera: X = I, B = A^-1)
//   joint sums         M_b = sum_p B_p^T M_p B_p,  Q_b = sum_p B_p^T Q_p B_p   (member order)
//   covariance         Sigma_b = M_b^-1 Q_b M_b^-1: of eps in T_true = T_hat twist_to_matrix(eps)
//   one camera         Sigma_b = A Sigma_xi A^T with Sigma_xi = M^-1 Q M^-1, the same thing
#pragma once
#include "../../include/bpvo_hip/c_api.h"
#include "rig_math.h"

namespace bpvo_hip {

// entry (a, b) of B^T S B for a symmetric f64 S, sums in index order (i outer, j inner) — rig_congruence_at for sums that are already f64
BPVO_HD double pose_cov_congruence_at(const double B[36], const double S[36], int a, int b)
{
  double v = 0.0;
  for(int i = 0; i < 6; ++i) {
    double row = 0.0;
    for(int j = 0; j < 6; ++j) row += S[i * 6 + j] * B[j * 6 + b];
    v += B[i * 6 + a] * row;
  }
  return v;
}
// S_out += B^T S B: the upper triangle is computed, the lower one mirrored (exactly symmetric)
BPVO_HD void pose_cov_add_congruence(const double B[36], const double S[36], double S_out[36])
{
  for(int a = 0; a < 6; ++a)
    for(int b = a; b < 6; ++b) {
      const double v = S_out[a * 6 + b] + pose_cov_congruence_at(B, S, a, b);
      S_out[a * 6 + b] = v;
      S_out[b * 6 + a] = v;
    }
}

// The 21 packed upper-triangle sums (row by row: (0,0) (0,1) .. (0,5) (1,1) ..) as a full symmetric matrix
BPVO_HD void pose_cov_unpack(const double packed[21], double S[36])
{
  int idx = 0;
  for(int a = 0; a < 6; ++a)
    for(int b = a; b < 6; ++b) {
      S[a * 6 + b] = packed[idx];
      S[b * 6 + a] = packed[idx];
      ++idx;
    }
}

// M = L D L^T without pivoting (unit lower L, row-major).  false at the first pivot that is not > 0 — M is then not positive definite (by
// Sylvester's law of inertia a symmetric M is positive definite exactly when every pivot is) — or not finite.
BPVO_HD bool pose_cov_ldlt(const double M[36], double L[36], double D[6])
{
  for(int i = 0; i < 36; ++i) L[i] = 0.0;
  for(int j = 0; j < 6; ++j) {
    double d = M[j * 6 + j];
    for(int k = 0; k < j; ++k) d -= L[j * 6 + k] * L[j * 6 + k] * D[k];
    if(!(d > 0.0) || !(d - d == 0.0)) return false;
    D[j] = d;
    L[j * 6 + j] = 1.0;
    for(int i = j + 1; i < 6; ++i) {
      double v = M[i * 6 + j];
      for(int k = 0; k < j; ++k) v -= L[i * 6 + k] * L[j * 6 + k] * D[k];
      L[i * 6 + j] = v / d;
    }
  }
  return true;
}
// x = (L D L^T)^-1 b
BPVO_HD void pose_cov_ldlt_solve(const double L[36], const double D[6], const double b[6], double x[6])
{
  for(int i = 0; i < 6; ++i) {
    double v = b[i];
    for(int k = 0; k < i; ++k) v -= L[i * 6 + k] * x[k];
    x[i] = v;
  }
  for(int i = 0; i < 6; ++i) x[i] /= D[i];
  for(int i = 5; i >= 0; --i) {
    double v = x[i];
    for(int k = i + 1; k < 6; ++k) v -= L[k * 6 + i] * x[k];
    x[i] = v;
  }
}

// Sigma = M^-1 Q M^-1 for symmetric M, Q: the LDL^T of M, Y = M^-1 Q (a solve per column of Q), Sigma^T = M^-1 Y^T (a solve per row of Y) —
// the two solves —, the upper triangle of the result mirrored.  BPVO_COV_INDEFINITE (Sigma untouched) when the factorisation meets a pivot <= 0.
// The work arrays come from the caller (the device keeps them in LDS: arrays a thread indexes at run time would otherwise live in scratch memory).
struct PoseCovScratch { double L[36], D[6], Y[36], S[36], b[6], x[6]; };
BPVO_HD int pose_cov_sandwich(const double M[36], const double Q[36], double Sigma[36], PoseCovScratch* ws)
{
  double* const L = ws->L; double* const D = ws->D; double* const Y = ws->Y; double* const b = ws->b; double* const x = ws->x;
  if(!pose_cov_ldlt(M, L, D)) return BPVO_COV_INDEFINITE;
  for(int c = 0; c < 6; ++c) {
    for(int i = 0; i < 6; ++i) b[i] = Q[i * 6 + c];
    pose_cov_ldlt_solve(L, D, b, x);
    for(int i = 0; i < 6; ++i) Y[i * 6 + c] = x[i];
  }
  for(int r = 0; r < 6; ++r) {      // row r of Y = M^-1 Q; M^-1 (row)^T = column r of M^-1 Q M^-1 ... = row r of Sigma (symmetric)
    for(int i = 0; i < 6; ++i) b[i] = Y[r * 6 + i];
    pose_cov_ldlt_solve(L, D, b, x);
    for(int c = r; c < 6; ++c) {
      Sigma[r * 6 + c] = x[c];
      Sigma[c * 6 + r] = x[c];
    }
  }
  return BPVO_COV_OK;
}

// The whole finish for the joint sums: the status rules of c_api.h and the result narrowed to f32 once.  Anything but BPVO_COV_OK leaves
// `covariance` at the Identity.  `estimated` = false: nothing was estimated (BPVO_COV_NONE).
BPVO_HD int pose_cov_finish(bool estimated, double total_valid, const double M_b[36], const double Q_b[36], float covariance[36], PoseCovScratch* ws)
{
  for(int i = 0; i < 36; ++i) covariance[i] = (i % 7 == 0) ? 1.0f : 0.0f;
  if(!estimated) return BPVO_COV_NONE;
  bool finite = total_valid - total_valid == 0.0;
  for(int i = 0; i < 36; ++i) finite = finite && (M_b[i] - M_b[i] == 0.0) && (Q_b[i] - Q_b[i] == 0.0);
  if(!finite || total_valid < 6.0) return BPVO_COV_DEGENERATE;
  double* const S = ws->S;
  const int status = pose_cov_sandwich(M_b, Q_b, S, ws);
  if(status != BPVO_COV_OK) return status;
  for(int i = 0; i < 36; ++i) {
    const float v = (float) S[i];
    if(!(v - v == 0.0f)) return BPVO_COV_DEGENERATE;      // (overflows f32: no covariance to hand out)
  }
  for(int i = 0; i < 36; ++i) covariance[i] = (float) S[i];
  return BPVO_COV_OK;
}

}  // namespace bpvo_hip
