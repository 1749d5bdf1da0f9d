// Motion stereo: the rule, stated once (no HIP header; compiled by a plain host compiler with -ffp-contract=off for the CPU tests, by hipcc for
// the library — kernels_motion_stereo.hip calls ms_locate, ms_hypothesis, ms_min_push and ms_finish per pixel and forms the sums between them).
// include/bpvo_hip/c_api.h states the same rule in words; tests/motion_stereo_ref.py follows this file.
//   A pixel (x, y) of the first image C carries a prior disparity pd with variance pv.  The second image K of the same camera saw the scene from
//   X_K = Q X_C.  With X_C = (fx b / d) (a, bq, 1), a = (x - cx) / fx, bq = (y - cy) / fy, the pixel's image in K as a function of its disparity is
//       u(d) = fx N0(d) / D(d) + cx,  v(d) = fy N1(d) / D(d) + cy,   N0 = h0 + d e0, N1 = h1 + d e1, D = h2 + d e2,   h = R (a, bq, 1), e = t / (fx b):
//   the epipolar curve.  Its speed at pd, g = |(u', v')| in pixels per disparity pixel, is the gain of the second baseline over the stereo one;
//   one pixel along the line is delta = 1 / g of disparity.  2 J + 1 hypotheses d_j = pd + j delta are scored by the sum of squared differences of
//   the (2 rho + 1)^2 window around (x, y) in C and the window around (u(d_j), v(d_j)) in K, interpolated with rectify_pixel's integer taps at
//   1/32 pixel; the parabola through the minimum and its neighbours gives the measurement dt and, by disparity_variance_math.h's model with one
//   step in place of one pixel, its variance vt; the prior is updated with df_update's FUSED arithmetic, or kept.
//   Everything up to the sums is f64, one operation per statement in the order written here; the sums are exact integers; the measurement is f64
//   rounded once to f32 each; the update is f32 with df_div / df_sqrt.  So the host, the device and numpy give the same bits.
#pragma once
#include <cmath>
#include <cstdint>

#include "disparity_fusion_math.h"
#include "rectify_math.h"

#if defined(__HIPCC__)
#define BPVO_MS_HD __host__ __device__
#else
#define BPVO_MS_HD
#endif

namespace bpvo_hip {

enum { MS_NO_PRIOR = 0, MS_LOW_PARALLAX = 1, MS_BORDER = 2, MS_EDGE = 3, MS_FLAT = 4, MS_REJECTED = 5, MS_FUSED = 6, MS_CLASSES = 7 };
constexpr int kMsMaxRadius = 3;
constexpr int kMsMaxSteps = 8;

// the setting as the rule reads it: the squares are f32 products, formed once on the host (ms_rule)
struct MsRule { int radius, steps; float min_gain, noise2, min2, max2, gate; };
inline MsRule ms_rule(int radius, int steps, float min_gain, float noise_sigma, float min_sigma, float max_sigma, float gate)
{
  return MsRule{radius, steps, min_gain, noise_sigma * noise_sigma, min_sigma * min_sigma, max_sigma * max_sigma, gate};
}
// null, or why the setting is refused; the cause names the field
inline const char* ms_refusal(int radius, int steps, float min_gain, float noise_sigma, float min_sigma, float max_sigma, float gate)
{
  if(radius < 1 || radius > kMsMaxRadius) return "motion stereo: radius must be within 1 .. 3";
  if(steps < 1 || steps > kMsMaxSteps) return "motion stereo: steps must be within 1 .. 8";
  if(!std::isfinite(min_gain) || !(min_gain > 0.0f)) return "motion stereo: min_gain must be positive and finite (pixels per disparity pixel)";
  if(!std::isfinite(noise_sigma) || !(noise_sigma > 0.0f)) return "motion stereo: noise_sigma must be positive and finite (grey levels; no default is guessed)";
  if(!std::isfinite(min_sigma) || !(min_sigma > 0.0f)) return "motion stereo: min_sigma must be positive and finite (disparity pixels; no default is guessed)";
  if(!std::isfinite(max_sigma) || !(min_sigma <= max_sigma)) return "motion stereo: max_sigma must be finite and at least min_sigma (disparity pixels; no default is guessed)";
  if(!std::isfinite(gate) || !(gate > 0.0f)) return "motion stereo: gate must be positive and finite (standard deviations)";
  const MsRule r = ms_rule(radius, steps, min_gain, noise_sigma, min_sigma, max_sigma, gate);
  if(!(r.noise2 > 0.0f) || !std::isfinite(r.noise2)) return "motion stereo: the square of noise_sigma must be positive and finite in f32";
  if(!(r.min2 > 0.0f)) return "motion stereo: the square of min_sigma must be positive in f32";
  if(!std::isfinite(r.max2)) return "motion stereo: the square of max_sigma must be finite in f32";
  return nullptr;
}

// What a pair of views shares: the camera in f64 and the motion Q (X_K = Q X_C; row-major [3][4] in f32), with e = t / (fx b).  Formed once per
// pair on the host (ms_geometry), the same numbers for every pixel.
struct MsGeometry { double fx, fy, cx, cy; double R[9]; double e[3]; };
inline MsGeometry ms_geometry(const DfCamera& c, const float* Q)
{
  MsGeometry g;
  g.fx = (double) c.fx; g.fy = (double) c.fy; g.cx = (double) c.cx; g.cy = (double) c.cy;
  const double fb = g.fx * (double) c.b;
  for(int r = 0; r < 3; ++r) {
    for(int k = 0; k < 3; ++k) g.R[3 * r + k] = (double) Q[4 * r + k];
    g.e[r] = (double) Q[4 * r + 3] / fb;
  }
  return g;
}

// the epipolar curve of one pixel: N0 = h[0] + d e[0], N1 = h[1] + d e[1], D = h[2] + d e[2]; delta: one pixel along it, in disparity
struct MsLine { double h[3]; double delta; };

// Steps 1 and 2 for the pixel (x, y) with the prior (has, pd, pv): MS_NO_PRIOR or MS_LOW_PARALLAX, or -1 and the pixel's curve.
BPVO_MS_HD inline int ms_locate(const MsRule& r, const MsGeometry& g, float lo, float hi, int x, int y, bool has, float pd, float pv, MsLine* line)
{
  if(!has || !(pv >= 0.0f) || !df_valid(pd, lo, hi)) return MS_NO_PRIOR;      // (NaN fails both comparisons)
  const double xa = (double) x - g.cx;
  const double a = xa / g.fx;
  const double yb = (double) y - g.cy;
  const double bq = yb / g.fy;
  const double h0 = (g.R[0] * a + g.R[1] * bq) + g.R[2];
  const double h1 = (g.R[3] * a + g.R[4] * bq) + g.R[5];
  const double h2 = (g.R[6] * a + g.R[7] * bq) + g.R[8];
  const double d = (double) pd;
  const double N0 = h0 + d * g.e[0];
  const double N1 = h1 + d * g.e[1];
  const double D = h2 + d * g.e[2];
  const double DD = D * D;
  const double nu = g.e[0] * D - N0 * g.e[2];
  const double nv = g.e[1] * D - N1 * g.e[2];
  const double up = (g.fx * nu) / DD;
  const double vp = (g.fy * nv) / DD;
  const double gain = sqrt(up * up + vp * vp);
  if(!(gain <= 1.7976931348623157e308) || gain < (double) r.min_gain) return MS_LOW_PARALLAX;      // (NaN and Inf fail the first comparison)
  line->h[0] = h0; line->h[1] = h1; line->h[2] = h2;
  line->delta = 1.0 / gain;
  return -1;
}

// Step 3 for hypothesis j: true and the quantised centre in K (1/32 pixel), or false (MS_BORDER).  True says that the window around (x, y) lies
// inside C and that every sample of the window around the centre has all its four taps inside K: columns (xq >> 5) - rho .. (xq >> 5) + rho + 1,
// rows likewise.
BPVO_MS_HD inline bool ms_hypothesis(const MsRule& r, const MsGeometry& g, const MsLine& line, float pd, int j, int x, int y, int rows, int cols, int32_t* xq, int32_t* yq)
{
  const int rho = r.radius;
  if(x - rho < 0 || x + rho >= cols || y - rho < 0 || y + rho >= rows) return false;
  const double dj = (double) pd + (double) j * line.delta;
  if(!(dj > 0.0)) return false;
  const double N0 = line.h[0] + dj * g.e[0];
  const double N1 = line.h[1] + dj * g.e[1];
  const double D = line.h[2] + dj * g.e[2];
  if(!(D > 0.0)) return false;
  const double u = (g.fx * N0) / D + g.cx;
  const double v = (g.fy * N1) / D + g.cy;
  if(!(fabs(u) < 1048576.0) || !(fabs(v) < 1048576.0)) return false;      // (NaN and Inf fail the comparison)
  const RectEntry q = rect_quantise(u, v);
  if(q.xq == kRectOutside) return false;
  const int ix = q.xq >> 5, iy = q.yq >> 5;
  if(ix - rho < 0 || ix + rho + 1 >= cols || iy - rho < 0 || iy + rho + 1 >= rows) return false;
  *xq = q.xq; *yq = q.yq;
  return true;
}

// rectify_pixel's interpolation of four taps that are known to lie inside the image
BPVO_MS_HD inline int ms_tap(int p00, int p01, int p10, int p11, int fx, int fy)
{
  return ((32 - fy) * ((32 - fx) * p00 + fx * p01) + fy * ((32 - fx) * p10 + fx * p11) + 512) >> 10;
}

// Step 5, first half: the first minimum of the sums as they arrive in the order j = -J .. J, with its two neighbours
struct MsMin { int j, s, s_before, s_after; int last; };
BPVO_MS_HD inline void ms_min_start(MsMin* m) { m->j = 0; m->s = 0x7FFFFFFF; m->s_before = 0; m->s_after = 0; m->last = 0; }
BPVO_MS_HD inline void ms_min_push(MsMin* m, int j, int s)
{
  if(j == m->j + 1) m->s_after = s;      // (the sum behind the minimum so far; a later minimum overwrites it)
  if(s < m->s) { m->s_before = m->last; m->s = s; m->j = j; }
  m->last = s;
}

// Steps 5 - 7 from the minimum: the class and the updated pair (the prior's own bits in every class but MS_FUSED)
BPVO_MS_HD inline int ms_finish(const MsRule& r, float lo, float hi, const MsLine& line, float pd, float pv, const MsMin& m, float* D, float* V)
{
  *D = pd; *V = pv;
  if(m.j == -r.steps || m.j == r.steps) return MS_EDGE;
  const int a2 = m.s_before + m.s_after - 2 * m.s;
  if(a2 <= 0) return MS_FLAT;
  const int n = (2 * r.radius + 1) * (2 * r.radius + 1);
  const double o = (double) (m.s_before - m.s_after) / (double) (2 * a2);
  const double t = (double) m.j + o;
  const float dt = (float) ((double) pd + t * line.delta);
  const double floor_ = (double) (2 * n) * (double) r.noise2;
  const double s0 = (double) m.s;
  const double num = 2.0 * (floor_ > s0 ? floor_ : s0);
  const double den = (double) n * (double) a2;
  const double q = num / den;
  const double d2 = line.delta * line.delta;
  float vt = (float) (q * d2);
  if(vt < r.min2) vt = r.min2;
  if(vt > r.max2) vt = r.max2;
  // df_update's FUSED branch with the measurement (dt, vt)
  const float s = pv + vt;
  const float bound = r.gate * df_sqrt(s);
  const float diff = dt - pd;
  if(!(fabsf(diff) <= bound)) return MS_REJECTED;
  const float k = df_div(pv, s);
  const float kd = k * diff;
  const float f = pd + kd;
  const float kv = k * pv;
  if(!(f > 0.0f) || !df_valid(f, lo, hi)) return MS_REJECTED;      // (a z-buffer word of a candidate is never 0)
  *D = f;
  *V = pv - kv;
  return MS_FUSED;
}

// The whole rule for one pixel as a serial loop over the windows (the CPU harness; the kernel forms the same integers from its tiles).
// C, K: u8 [rows][cols]
inline int ms_pixel(const MsRule& r, const MsGeometry& g, float lo, float hi, const uint8_t* C, const uint8_t* K, int rows, int cols, int x, int y,
                    bool has, float pd, float pv, float* D, float* V)
{
  *D = pd; *V = pv;
  MsLine line;
  const int cls = ms_locate(r, g, lo, hi, x, y, has, pd, pv, &line);
  if(cls >= 0) return cls;
  int32_t xq = 0, yq = 0;
  for(int j = -r.steps; j <= r.steps; ++j)
    if(!ms_hypothesis(r, g, line, pd, j, x, y, rows, cols, &xq, &yq)) return MS_BORDER;
  MsMin m;
  ms_min_start(&m);
  for(int j = -r.steps; j <= r.steps; ++j) {
    (void) ms_hypothesis(r, g, line, pd, j, x, y, rows, cols, &xq, &yq);
    int s = 0;
    for(int jj = -r.radius; jj <= r.radius; ++jj)
      for(int ii = -r.radius; ii <= r.radius; ++ii) {
        const int c = (int) C[(size_t) (y + jj) * cols + (x + ii)];
        const int k = (int) rectify_pixel(K, rows, cols, xq + 32 * ii, yq + 32 * jj);
        s += (c - k) * (c - k);
      }
    ms_min_push(&m, j, s);
  }
  return ms_finish(r, lo, hi, line, pd, pv, m, D, V);
}

}  // namespace bpvo_hip
