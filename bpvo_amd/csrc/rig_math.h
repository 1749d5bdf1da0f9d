// The small maps of rig mode (bpvo_hip_*_rig): the cameras of a rigid rig estimated as ONE body pose.  Shared by the device-side rig step
// (kernels_gn_rig.hip), the host drivers (estimate.hip, vo.hip) and the CPU tests (tests/test_rig_cpu.py compiles this header with a plain
// C++ compiler).  Everything is evaluated in f64 from the f32 inputs; twists are ordered (omega, v) as twist_to_matrix takes them.
//
//   body pose T        key-frame body coordinates -> current body coordinates
//   extrinsic X_p      camera_from_body of member p: x_cam = X_p x_body (rigid)
//   member pose        T_p = X_p T X_p^-1 (f64, narrowed to f32: the kernels read an f32 pose)
//   member update      T_p <- T_p N_p^-1 exp(-xi) N_p,  N_p = [sI, -s c; 0 1]  (Hartley normalisation (s, c) of the member's template level)
//                      N^-1 exp(xi) N = exp(A xi),  A = [[I, 0], [[c]x, I/s]],  A^-1 = [[I, 0], [-s [c]x, sI]]
//   body update        T <- T exp(-zeta)  =>  T_p <- T_p exp(-Ad(X_p) zeta),  Ad(X) = [[R, 0], [[t]x R, R]]
//   so                 xi = B_p zeta,  B_p = A_p^-1 Ad(X_p)
//   joint system       H = sum_p B_p^T H_p B_p,  G = sum_p B_p^T G_p   (member order, f64, narrowed once)
//   the estimate's own parametrisation: the f32 solve wants a normalised system (the plain-twist H of a camera has a condition number of 2e4
//   where its normalised one has 30), so the coarse-to-fine loop iterates on the pose of the REFERENCE member (member 0) in ITS normalised
//   twist xi_0: zeta = B_0^-1 xi_0, member p's map becomes B_p B_0^-1 = A_p^-1 Ad(X_p X_0^-1) A_0 (the identity for p = 0), and the body pose is
//   X_0^-1 T_0 X_0 at the end.  The same Gauss-Newton steps; a rig of one camera then takes exactly that camera's own steps.
#pragma once
#include "device_math.h"

namespace bpvo_hip {

// [v]x as a row-major 3x3
BPVO_HD void rig_skew(const double v[3], double S[9])
{
  S[0] = 0.0; S[1] = -v[2]; S[2] = v[1];
  S[3] = v[2]; S[4] = 0.0; S[5] = -v[0];
  S[6] = -v[1]; S[7] = v[0]; S[8] = 0.0;
}

// Ad(X) = [[R, 0], [[t]x R, R]], row-major 6x6
BPVO_HD void rig_adjoint(const float X[16], double Ad[36])
{
  double R[9], S[9];
  const double t[3] = {(double) X[3], (double) X[7], (double) X[11]};
  for(int i = 0; i < 3; ++i)
    for(int j = 0; j < 3; ++j) R[i * 3 + j] = (double) X[i * 4 + j];
  rig_skew(t, S);
  for(int i = 0; i < 3; ++i)
    for(int j = 0; j < 3; ++j) {
      double v = S[i * 3 + 0] * R[0 * 3 + j];
      v += S[i * 3 + 1] * R[1 * 3 + j];
      v += S[i * 3 + 2] * R[2 * 3 + j];
      Ad[i * 6 + j] = R[i * 3 + j];
      Ad[i * 6 + 3 + j] = 0.0;
      Ad[(3 + i) * 6 + j] = v;
      Ad[(3 + i) * 6 + 3 + j] = R[i * 3 + j];
    }
}

// A = [[I, 0], [[c]x, I/s]] and its inverse [[I, 0], [-s [c]x, sI]] for the normalisation nrm = (s, c1, c2, c3); (1, 0, 0, 0): the identity
BPVO_HD void rig_normalization_map(const float nrm[4], double A[36])
{
  double S[9];
  const double s = (double) nrm[0], c[3] = {(double) nrm[1], (double) nrm[2], (double) nrm[3]};
  rig_skew(c, S);
  for(int i = 0; i < 36; ++i) A[i] = 0.0;
  for(int i = 0; i < 3; ++i) {
    A[i * 6 + i] = 1.0;
    A[(3 + i) * 6 + 3 + i] = 1.0 / s;
    for(int j = 0; j < 3; ++j) A[(3 + i) * 6 + j] = S[i * 3 + j];
  }
}
BPVO_HD void rig_normalization_map_inverse(const float nrm[4], double Ai[36])
{
  double S[9];
  const double s = (double) nrm[0], c[3] = {(double) nrm[1], (double) nrm[2], (double) nrm[3]};
  rig_skew(c, S);
  for(int i = 0; i < 36; ++i) Ai[i] = 0.0;
  for(int i = 0; i < 3; ++i) {
    Ai[i * 6 + i] = 1.0;
    Ai[(3 + i) * 6 + 3 + i] = s;
    for(int j = 0; j < 3; ++j) Ai[(3 + i) * 6 + j] = -s * S[i * 3 + j];
  }
}

// entry (a, b) of B = A^-1 Ad(X): what one lane of the rig step computes
BPVO_HD double rig_body_map_at(const double Ai[36], const double Ad[36], int a, int b)
{
  double v = 0.0;
  for(int k = 0; k < 6; ++k) v += Ai[a * 6 + k] * Ad[k * 6 + b];
  return v;
}
BPVO_HD void rig_body_map(const float X[16], const float nrm[4], double B[36])
{
  double Ai[36], Ad[36];
  rig_normalization_map_inverse(nrm, Ai);
  rig_adjoint(X, Ad);
  for(int a = 0; a < 6; ++a)
    for(int b = 0; b < 6; ++b) B[a * 6 + b] = rig_body_map_at(Ai, Ad, a, b);
}

// entry (a, b) of B^T H B and entry a of B^T G, sums in index order (i outer, j inner)
BPVO_HD double rig_congruence_at(const double B[36], const float H[36], int a, int b)
{
  double v = 0.0;
  for(int i = 0; i < 6; ++i) {
    double row = 0.0;
    for(int j = 0; j < 6; ++j) row += (double) H[i * 6 + j] * B[j * 6 + b];
    v += B[i * 6 + a] * row;
  }
  return v;
}
BPVO_HD double rig_gradient_at(const double B[36], const float G[6], int a)
{
  double v = 0.0;
  for(int i = 0; i < 6; ++i) v += B[i * 6 + a] * (double) G[i];
  return v;
}
BPVO_HD void rig_congruence(const double B[36], const float H[36], const float G[6], double Hb[36], double Gb[6])
{
  for(int a = 0; a < 6; ++a) {
    for(int b = 0; b < 6; ++b) Hb[a * 6 + b] = rig_congruence_at(B, H, a, b);
    Gb[a] = rig_gradient_at(B, G, a);
  }
}

// entry (r, c) of X^-1 for a rigid X: [R^T, -R^T t; 0 1]
BPVO_HD double rig_inverse_at(const float X[16], int r, int c)
{
  if(r == 3) return c == 3 ? 1.0 : 0.0;
  if(c < 3) return (double) X[c * 4 + r];
  double v = (double) X[0 * 4 + r] * (double) X[3];
  v += (double) X[1 * 4 + r] * (double) X[7];
  v += (double) X[2 * 4 + r] * (double) X[11];
  return -v;
}
// entry (r, c) of the member pose X T X^-1 in f64, evaluated as I + X (T - I) X^-1: the identity maps to the identity and a member at the body's
// origin (X = I) gets T itself, exactly; poses near the identity — what visual odometry estimates — lose nothing to the rounding of R R^T
BPVO_HD double rig_member_pose_at(const float X[16], const float T[16], int r, int c)
{
  double v = 0.0;
  for(int k = 0; k < 4; ++k) {
    double xt = 0.0;
    for(int l = 0; l < 4; ++l) xt += (double) X[r * 4 + l] * ((double) T[l * 4 + k] - (l == k ? 1.0 : 0.0));
    v += xt * rig_inverse_at(X, k, c);
  }
  return v + (r == c ? 1.0 : 0.0);
}
// ... and of its inverse map, the body pose X^-1 T_p X of a member pose, as I + X^-1 (T_p - I) X
BPVO_HD double rig_body_pose_at(const float X[16], const float Tp[16], int r, int c)
{
  double v = 0.0;
  for(int k = 0; k < 4; ++k) {
    double xt = 0.0;
    for(int l = 0; l < 4; ++l) xt += rig_inverse_at(X, r, l) * ((double) Tp[l * 4 + k] - (l == k ? 1.0 : 0.0));
    v += xt * (double) X[k * 4 + c];
  }
  return v + (r == c ? 1.0 : 0.0);
}
BPVO_HD void rig_body_pose(const float X[16], const float Tp[16], float T[16])
{
  for(int r = 0; r < 4; ++r)
    for(int c = 0; c < 4; ++c) T[r * 4 + c] = (float) rig_body_pose_at(X, Tp, r, c);
  T[12] = 0.0f; T[13] = 0.0f; T[14] = 0.0f; T[15] = 1.0f;
}
// X_p X_0^-1 in f64, narrowed: member p's extrinsic relative to the reference member (camera p from camera 0); p = 0 gives the identity exactly
BPVO_HD void rig_relative_extrinsic(const float Xp[16], const float X0[16], float M[16])
{
  for(int r = 0; r < 4; ++r)
    for(int c = 0; c < 4; ++c) {
      double v = 0.0;
      for(int k = 0; k < 4; ++k) v += (double) Xp[r * 4 + k] * rig_inverse_at(X0, k, c);
      M[r * 4 + c] = (float) v;
    }
  M[12] = 0.0f; M[13] = 0.0f; M[14] = 0.0f; M[15] = 1.0f;
}
BPVO_HD void rig_member_pose(const float X[16], const float T[16], float Tp[16])
{
  for(int r = 0; r < 4; ++r)
    for(int c = 0; c < 4; ++c) Tp[r * 4 + c] = (float) rig_member_pose_at(X, T, r, c);
  Tp[12] = 0.0f; Tp[13] = 0.0f; Tp[14] = 0.0f; Tp[15] = 1.0f;
}
// W X^-1 in f64, narrowed: the pose of a member's point cloud (world_from_camera) from the body's (world_from_body)
BPVO_HD void rig_cloud_pose(const float W[16], const float X[16], float out[16])
{
  for(int r = 0; r < 4; ++r)
    for(int c = 0; c < 4; ++c) {
      double v = 0.0;
      for(int k = 0; k < 4; ++k) v += (double) W[r * 4 + k] * rig_inverse_at(X, k, c);
      out[r * 4 + c] = (float) v;
    }
}

// is X a rigid transform?  finite, last row (0, 0, 0, 1), max_ij |R^T R - I| <= 1e-4
BPVO_HD bool rig_extrinsic_ok(const float X[16])
{
  for(int i = 0; i < 16; ++i)
    if(!(X[i] - X[i] == 0.0f)) return false;      // (NaN and infinities)
  if(X[12] != 0.0f || X[13] != 0.0f || X[14] != 0.0f || X[15] != 1.0f) return false;
  for(int i = 0; i < 3; ++i)
    for(int j = 0; j < 3; ++j) {
      double v = 0.0;
      for(int k = 0; k < 3; ++k) v += (double) X[k * 4 + i] * (double) X[k * 4 + j];
      const double e = v - (i == j ? 1.0 : 0.0);
      if(!((e < 0.0 ? -e : e) <= 1e-4)) return false;
    }
  return true;
}

}  // namespace bpvo_hip
