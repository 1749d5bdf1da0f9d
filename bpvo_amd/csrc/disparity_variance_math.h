// Measurement variance: the rule, stated once (no HIP header; compiled by a plain host compiler for the CPU tests, by hipcc for the library —
// kernels_disparity_variance.hip calls dv_locate and dv_finish per pixel and forms the three sums between them).  include/bpvo_hip/c_api.h states
// the same rule in words; tests/disparity_variance_ref.py follows this file.
//   The variance of a measured disparity m at pixel (x, y), from the rectified pair (Matthies, Kanade and Szeliski's companion to the filter of
//   disparity_fusion_math.h): d0 = rint(m), and S_k the sum of squared differences of the (2 rho + 1)^2 window around (x, y) in the left image
//   and around (x - d0 - k, y) in the right one, k = -1, 0, +1.  The parabola through (k, S_k) has the quadratic coefficient a / 2 with
//   a = S_-1 + S_+1 - 2 S_0; with a pixel noise of variance sn2 per image the variance of its minimum is 2 sn2 / (a / 2) = 4 sn2 / a per pixel
//   of the window, where sn2 is the larger of the caller's noise_sigma^2 and the match's own residual S_0 / (2 n), n = (2 rho + 1)^2.  So
//       v = 2 max(2 n noise2, S_0) / (n a):
//   it rises on weak texture (small a) and on bad matches — fattening, occlusion — (large S_0), and is clamped to [min2, max2].
//   The sums are exact integers (at most 225 * 65025 < 2^24 each, |a| < 2^25); the products of the quotient's operands are exact in f64, the
//   division is the only rounding before the cast to f32 — the same number on the host and on the device, whatever adds the sums in which order.
#pragma once
#include <cmath>
#include <cstdint>

#include "disparity_fusion_math.h"

#if defined(__HIPCC__)
#define BPVO_DV_HD __host__ __device__
#else
#define BPVO_DV_HD
#endif

namespace bpvo_hip {

enum { DV_INVALID = 0, DV_BORDER = 1, DV_FLAT = 2, DV_FLOOR = 3, DV_CEILING = 4, DV_MODEL = 5, DV_CLASSES = 6 };
constexpr int kDvMaxRadius = 7;

// the setting as the rule reads it: the squares are f32 products, formed once on the host (dv_rule)
struct DvRule { int radius; float noise2, min2, max2; };
inline DvRule dv_rule(int radius, float noise_sigma, float min_sigma, float max_sigma)
{
  return DvRule{radius, noise_sigma * noise_sigma, min_sigma * min_sigma, max_sigma * max_sigma};
}
// null, or why mode 1 refuses the setting
inline const char* dv_refusal(int radius, float noise_sigma, float min_sigma, float max_sigma)
{
  if(radius < 1 || radius > kDvMaxRadius) return "measurement variance: radius must be within 1 .. 7";
  if(!std::isfinite(noise_sigma) || !std::isfinite(min_sigma) || !std::isfinite(max_sigma)) return "measurement variance: the parameters must be finite";
  if(!(noise_sigma > 0.0f)) return "measurement variance: noise_sigma must be positive (grey levels; no default is guessed)";
  if(!(min_sigma > 0.0f) || !(min_sigma <= max_sigma)) return "measurement variance: 0 < min_sigma <= max_sigma (disparity pixels; no default is guessed)";
  const DvRule r = dv_rule(radius, noise_sigma, min_sigma, max_sigma);
  if(!(r.noise2 > 0.0f) || !(r.min2 > 0.0f) || !std::isfinite(r.noise2) || !std::isfinite(r.max2))
    return "measurement variance: the squares of the parameters must be positive and finite in f32";
  return nullptr;
}

// Steps 1 - 3 for the pixel (x, y) of a rows x cols pair with the measured disparity m: DV_INVALID or DV_BORDER (the variance is max2), or -1 and
// *d0: the windows of the three sums lie inside both images.
BPVO_DV_HD inline int dv_locate(float m, float lo, float hi, int x, int y, int rows, int cols, int radius, int* d0)
{
  if(!df_valid(m, lo, hi)) return DV_INVALID;
  if(!(fabsf(m) < 1073741824.0f)) return DV_BORDER;      // (below 2^30 in magnitude the cast is exact; beyond, the right windows are outside anyway)
  const int d = (int) rint((double) m);      // ties to even
  *d0 = d;
  if(y - radius < 0 || y + radius >= rows || x - radius < 0 || x + radius >= cols) return DV_BORDER;
  // (|d| <= 2^30 and x, radius far below it: no overflow)
  if(x - radius - d - 1 < 0 || x + radius - d + 1 >= cols) return DV_BORDER;
  return -1;
}

// Steps 5 - 7: the class and the variance from the three sums (s_m1: k = -1, the right window one pixel to the right; s_p1: k = +1)
BPVO_DV_HD inline int dv_finish(const DvRule& r, int s_m1, int s_0, int s_p1, float* r2)
{
  const int n = (2 * r.radius + 1) * (2 * r.radius + 1);
  const int a = s_m1 + s_p1 - 2 * s_0;
  if(a <= 0) { *r2 = r.max2; return DV_FLAT; }
  const double floor_ = (double) (2 * n) * (double) r.noise2;
  const double s0 = (double) s_0;
  const double num = 2.0 * (floor_ > s0 ? floor_ : s0);
  const double den = (double) n * (double) a;
  const float v = (float) (num / den);
  if(v < r.min2) { *r2 = r.min2; return DV_FLOOR; }
  if(v > r.max2) { *r2 = r.max2; return DV_CEILING; }
  *r2 = v;
  return DV_MODEL;
}

// The whole rule for one pixel as a serial loop over the windows (the CPU harness; the kernel forms the same integers from its tiles).
// L, R: u8 [rows][cols]
inline int dv_pixel(const DvRule& r, float lo, float hi, const uint8_t* L, const uint8_t* R, int rows, int cols, int x, int y, float m, float* r2)
{
  int d0 = 0;
  const int cls = dv_locate(m, lo, hi, x, y, rows, cols, r.radius, &d0);
  if(cls >= 0) { *r2 = r.max2; return cls; }
  int s[3] = {0, 0, 0};
  for(int k = -1; k <= 1; ++k)
    for(int j = -r.radius; j <= r.radius; ++j)
      for(int i = -r.radius; i <= r.radius; ++i) {
        const int l = (int) L[(size_t) (y + j) * cols + (x + i)];
        const int q = (int) R[(size_t) (y + j) * cols + (x + i - d0 - k)];
        s[k + 1] += (l - q) * (l - q);
      }
  return dv_finish(r, s[0], s[1], s[2], r2);
}

}  // namespace bpvo_hip
