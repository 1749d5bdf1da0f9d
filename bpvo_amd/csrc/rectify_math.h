// Rectification on the device: the rule, stated once (no HIP; compiled by a plain host compiler with -ffp-contract=off for the CPU tests, by
// hipcc for the library — the map is built on the host, the pixel is formed by kernels_rectify.hip).  include/bpvo_hip/c_api.h states the same
// rule in words.
//   * a map entry: the source coordinates (x, y) of a destination pixel in 1/32 pixel, xq = (int32) nearbyint(x * 32.0), ties to even; a
//     non-finite coordinate or |x * 32| >= 2^20 gives the entry "outside" (kRectOutside in both words), which stores a 0 pixel
//   * the lens map: Brown-Conrady with eight coefficients, every operation a statement of its own in the order c_api.h gives, all f64
//   * the pixel: four taps, a tap outside the raw image reads 0, integer weights of 1/32, + 512 >> 10
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define BPVO_RECT_HD __host__ __device__
#else
#define BPVO_RECT_HD
#endif

namespace bpvo_hip {

constexpr int32_t kRectOutside = INT32_MIN;      // both words of the entry of a destination pixel without a source
constexpr int kRectMaxRaw = 32767;               // rows and cols of a raw image at most (every tap index of an entry in range fits 16 bits + sign)

struct RectEntry { int32_t xq, yq; };

// (x, y) -> the entry.  |x * 32| < 2^20 keeps nearbyint inside int32 and the tap indices inside +-32768
BPVO_RECT_HD inline RectEntry rect_quantise(double x, double y)
{
  const double sx = x * 32.0;
  const double sy = y * 32.0;
  if(!(std::fabs(sx) < 1048576.0) || !(std::fabs(sy) < 1048576.0)) return RectEntry{kRectOutside, kRectOutside};      // (NaN and Inf fail the comparison)
  return RectEntry{(int32_t) std::nearbyint(sx), (int32_t) std::nearbyint(sy)};
}

// The lens: raw intrinsics, distortion k1 k2 p1 p2 k3 k4 k5 k6, the rotation from the raw camera to the rectified camera (row-major)
struct RectLens { double fx, fy, cx, cy; double dist[8]; double R[9]; };

// the source coordinates of the integer destination pixel (u, v) of a rectified camera with intrinsics fxn fyn cxn cyn
inline void rect_lens_source(const RectLens& q, double fxn, double fyn, double cxn, double cyn, int u, int v, double* xs_out, double* ys_out)
{
  const double k1 = q.dist[0], k2 = q.dist[1], p1 = q.dist[2], p2 = q.dist[3], k3 = q.dist[4], k4 = q.dist[5], k5 = q.dist[6], k6 = q.dist[7];
  const double a = ((double) u - cxn) / fxn;
  const double b = ((double) v - cyn) / fyn;
  const double X = (q.R[0] * a + q.R[3] * b) + q.R[6];
  const double Y = (q.R[1] * a + q.R[4] * b) + q.R[7];
  const double W = (q.R[2] * a + q.R[5] * b) + q.R[8];      // R^T (a, b, 1): no matrix inverse
  const double x = X / W;
  const double y = Y / W;
  const double x2 = x * x;
  const double y2 = y * y;
  const double r2 = x2 + y2;
  const double xy = x * y;
  const double num = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2;
  const double den = 1.0 + ((k6 * r2 + k5) * r2 + k4) * r2;
  const double rad = num / den;
  const double tp1 = 2.0 * p1;
  const double tp2 = 2.0 * p2;
  const double xd = (x * rad + tp1 * xy) + p2 * (r2 + 2.0 * x2);
  const double yd = (y * rad + p1 * (r2 + 2.0 * y2)) + tp2 * xy;
  *xs_out = q.fx * xd + q.cx;
  *ys_out = q.fy * yd + q.cy;
}
inline RectEntry rect_lens_entry(const RectLens& q, double fxn, double fyn, double cxn, double cyn, int u, int v)
{
  double xs, ys;
  rect_lens_source(q, fxn, fyn, cxn, cyn, u, v, &xs, &ys);
  return rect_quantise(xs, ys);
}
// max |R^T R - I|: how far R is from orthonormal
inline double rect_orthonormal_error(const double R[9])
{
  double worst = 0.0;
  for(int i = 0; i < 3; ++i)
    for(int j = 0; j < 3; ++j) {
      double s = 0.0;
      for(int k = 0; k < 3; ++k) s += R[3 * k + i] * R[3 * k + j];
      worst = std::fmax(worst, std::fabs(s - (i == j ? 1.0 : 0.0)));
    }
  return worst;
}

// The destination pixel of entry (xq, yq) from a raw image of raw_rows x raw_cols bytes
BPVO_RECT_HD inline uint8_t rectify_pixel(const uint8_t* raw, int raw_rows, int raw_cols, int32_t xq, int32_t yq)
{
  if(xq == kRectOutside) return 0;
  const int ix = xq >> 5, fx = xq & 31;      // (arithmetic shift: the floor, also left of 0)
  const int iy = yq >> 5, fy = yq & 31;
  const bool x0 = ix >= 0 && ix < raw_cols, x1 = ix + 1 >= 0 && ix + 1 < raw_cols;
  const bool y0 = iy >= 0 && iy < raw_rows, y1 = iy + 1 >= 0 && iy + 1 < raw_rows;
  const long long o = (long long) iy * raw_cols + ix;      // (an index, formed into an address only where the flags allow)
  const int p00 = y0 && x0 ? (int) raw[o] : 0;
  const int p01 = y0 && x1 ? (int) raw[o + 1] : 0;
  const int p10 = y1 && x0 ? (int) raw[o + raw_cols] : 0;
  const int p11 = y1 && x1 ? (int) raw[o + raw_cols + 1] : 0;
  return (uint8_t) (((32 - fy) * ((32 - fx) * p00 + fx * p01) + fy * ((32 - fx) * p10 + fx * p11) + 512) >> 10);
}
// Is the destination pixel of the entry "outside": the sentinel, or a tap with a non-zero weight outside the raw image
BPVO_RECT_HD inline bool rectify_outside(int raw_rows, int raw_cols, int32_t xq, int32_t yq)
{
  if(xq == kRectOutside) return true;
  const int ix = xq >> 5, fx = xq & 31;
  const int iy = yq >> 5, fy = yq & 31;
  const bool x0 = ix >= 0 && ix < raw_cols, x1 = ix + 1 >= 0 && ix + 1 < raw_cols;
  const bool y0 = iy >= 0 && iy < raw_rows, y1 = iy + 1 >= 0 && iy + 1 < raw_rows;
  return !(x0 && y0) || (fx != 0 && !x1) || (fy != 0 && !y1);      // (the fourth tap's weight fx fy is non-zero only where both of these are)
}

}  // namespace bpvo_hip
