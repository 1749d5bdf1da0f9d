// Where a template point lands in the current image and whether it is valid there: the reference's projection-and-validity step, stated
// ONCE for every Gauss-Newton kernel path (gn_warp.h, gn_irls.h, kernels_gn_team.hip, kernels_gn.hip) and for the CPU test
// (tests/test_warp_rule_cpu.py compiles this header with a plain C++ compiler).  The rule decides bit parity with the reference: same
// operations in the same order as there, and the library is built with -ffp-contract=off, so nothing here may be regrouped.
#pragma once
#include "device_math.h"

#ifdef __HIPCC__
#define BPVO_WARP_RULE __host__ __device__ __forceinline__      // (BPVO_HD is only `inline`: the kernels count on these being inlined)
#else
#define BPVO_WARP_RULE inline
#endif

namespace bpvo_hip {

// The standard (f64) rule.  reference: PhotoError::Impl::init (bpvo/photo_error.cc:344-363): x = normHomog(P.cast<double>() *
// X.cast<double>()) with the f32 P = K * T[0:3,:] (index-order sums), Floor (:255-265), valid = LO <= xi < W - HI && LO <= yi < R - 1 with
// (LO, HI) = (0, 1) for kLinear and the cosine form and (1, 3) for the 4 x 4 footprints of kCubic / kCubicHermite (:347-348; `yi < R - 1` for
// every kind, as there).  No z > 0 test.  (xf, yf): the fractional parts; of an invalid point only `valid` means anything.
struct WarpFoot { int xi, yi; bool valid; double xf, yf; };
template <int LO = 0, int HI = 1>
BPVO_WARP_RULE WarpFoot warp_foot(const float (&P)[12], float Xx, float Xy, float Xz, float Xw, int W, int R)
{
  const double X0 = (double) Xx, X1 = (double) Xy, X2 = (double) Xz, X3 = (double) Xw;
  double u[3];
#pragma unroll
  for(int r = 0; r < 3; ++r) {
    double s = (double) P[r * 4 + 0] * X0;
    s += (double) P[r * 4 + 1] * X1;
    s += (double) P[r * 4 + 2] * X2;
    s += (double) P[r * 4 + 3] * X3;
    u[r] = s;
  }
  const double zi = 1.0 / u[2];
  const double x = zi * u[0], y = zi * u[1];
  // Floor(): static_cast<int> then -(i > v).  x86 yields INT_MIN for NaN / out-of-range doubles (cvttsd2si), which can never be a
  // valid pixel; the explicit range test gives the same verdict without relying on v_cvt_i32_f64 saturation.
  const bool in_range = (x > -2147483648.0) && (x < 2147483648.0) && (y > -2147483648.0) && (y < 2147483648.0);
  WarpFoot f;
  f.xi = 0; f.yi = 0;
  if(in_range) {
    f.xi = (int) x; f.xi -= (f.xi > x);
    f.yi = (int) y; f.yi -= (f.yi > y);
  }
  f.valid = in_range && f.xi >= LO && f.xi < W - HI && f.yi >= LO && f.yi < R - 1;
  f.xf = x - (double) f.xi; f.yf = y - (double) f.yi;
  return f;
}

// The reference's alternative all-f32 rule (inactive there, PHOTO_ERROR_OPT = 0).  reference: projectPoints (bpvo/project_points.cc:180-214):
// x = P * X in f32, w = 1.0f / x2, xi = (int) xf — truncation, not floor: x in (-1, 0) is pixel 0 with a negative fraction — valid =
// 0 <= xi < W - 1 && 0 <= yi < R - 1, coefficients cf = [xf*yf - yf - xf + 1, xf - xf*yf, yf - xf*yf, xf*yf].  `dspace`: the point is in
// disparity space and P holds rows 0, 1, 3 of H = G * T * G_inv: DisparitySpaceWarp::operator() (bpvo/disparity_space_warp.h:66-71) adds the
// principal point (cx, cy) to the quotient.
struct WarpFootF32 { int xi, yi; bool valid; float cf[4]; };
BPVO_WARP_RULE WarpFootF32 warp_foot_f32(const float (&P)[12], float Xx, float Xy, float Xz, float Xw, bool dspace, float cx, float cy, int W, int R)
{
  float u[3];
#pragma unroll
  for(int r = 0; r < 3; ++r) {
    float s = P[r * 4 + 0] * Xx;
    s += P[r * 4 + 1] * Xy;
    s += P[r * 4 + 2] * Xz;
    s += P[r * 4 + 3] * Xw;
    u[r] = s;
  }
  const float w_i = 1.0f / u[2];
  float fx = w_i * u[0], fy = w_i * u[1];
  if(dspace) { fx = fx + cx; fy = fy + cy; }
  // (int) xf: cvttss2si gives INT_MIN for NaN / out-of-range, never a valid pixel
  const bool in_range = (fx > -2147483648.0f) && (fx < 2147483648.0f) && (fy > -2147483648.0f) && (fy < 2147483648.0f);
  WarpFootF32 f;
  f.xi = 0; f.yi = 0;
  if(in_range) { f.xi = (int) fx; f.yi = (int) fy; }
  f.valid = in_range && f.xi >= 0 && f.xi < W - 1 && f.yi >= 0 && f.yi < R - 1;
  fx -= (float) f.xi; fy -= (float) f.yi;
  const float xfyf = fx * fy;
  f.cf[0] = xfyf - fy - fx + 1.0f; f.cf[1] = fx - xfyf; f.cf[2] = fy - xfyf; f.cf[3] = xfyf;
  return f;
}

}  // namespace bpvo_hip
