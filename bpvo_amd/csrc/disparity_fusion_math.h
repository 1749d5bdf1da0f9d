// Disparity fusion: the rule, stated once (no HIP header; compiled by a plain host compiler with -ffp-contract=off for the CPU tests, by hipcc
// for the library — kernels_disparity_fusion.hip calls the two functions below per pixel).  include/bpvo_hip/c_api.h states the same rule in
// words; tests/disparity_fusion_ref.py follows this file.
//   * prediction (df_splat): a pixel (x, y) of the carried maps (disparity d, variance vc >= 0) is moved by the motion P (X_new = P X_old) in
//     f64, every operation a statement of its own in the order written here, and becomes a candidate (target pixel, key) or is dropped.  A
//     target keeps the LARGEST key = bits(d') * 2^32 + bits(v'): d' > 0 and v' >= 0, so the key orders as the pair (d', v') does — the nearest
//     surface wins, then the larger variance — and the maximum over a set does not depend on the order its members arrive in.
//   * update (df_update): per pixel, f32.  Division and square root are taken in f64 on the f32 operands and rounded once to f32: for p = 24
//     and 53 >= 2 p + 2 bits that IS the correctly rounded f32 operation (double rounding is innocuous for / and sqrt), on the host and on the
//     device, whatever the compiler's f32 division and square-root forms are.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define BPVO_DF_HD __host__ __device__
#else
#define BPVO_DF_HD
#endif

namespace bpvo_hip {

enum { DF_FUSED = 0, DF_REPLACED = 1, DF_MEASURED = 2, DF_FILLED = 3, DF_NONE = 4, DF_CLASSES = 5 };

// the camera of the maps (level 0) and the gate of its sequence's parameters
struct DfCamera { float fx, fy, cx, cy, b; float lo, hi; int rows, cols; };
// the fusion parameters as the rule reads them: the squares are f32 products, formed once on the host (df_rule)
struct DfRule { float r2, q2, gate, fill2; };
inline DfRule df_rule(float measurement_sigma, float process_sigma, float gate, float max_fill_sigma)
{
  return DfRule{measurement_sigma * measurement_sigma, process_sigma * process_sigma, gate, max_fill_sigma * max_fill_sigma};
}
// null, or why mode 1 refuses the parameters
inline const char* df_refusal(float measurement_sigma, float process_sigma, float gate, float max_fill_sigma)
{
  const bool finite = std::isfinite(measurement_sigma) && std::isfinite(process_sigma) && std::isfinite(gate) && std::isfinite(max_fill_sigma);
  if(!finite) return "disparity fusion: the parameters must be finite";
  if(!(measurement_sigma > 0.0f)) return "disparity fusion: measurement_sigma must be positive (disparity pixels; no default is guessed)";
  if(!(process_sigma >= 0.0f)) return "disparity fusion: process_sigma must not be negative";
  if(!(gate > 0.0f)) return "disparity fusion: gate must be positive (standard deviations)";
  if(!(max_fill_sigma >= 0.0f)) return "disparity fusion: max_fill_sigma must not be negative (0: never fill)";
  return nullptr;
}
// a motion with a non-finite entry among its twelve gives no prediction at all (the last row is not read)
inline bool df_motion_ok(const float* P)
{
  for(int k = 0; k < 12; ++k)
    if(!std::isfinite(P[k])) return false;
  return true;
}

// the template stage's own gate: inclusive, false for NaN
BPVO_DF_HD inline bool df_valid(float d, float lo, float hi) { return d >= lo && d <= hi; }

BPVO_DF_HD inline uint32_t df_bits(float f)
{
#if defined(__HIP_DEVICE_COMPILE__)
  return __float_as_uint(f);
#else
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
#endif
}
BPVO_DF_HD inline float df_float(uint32_t u)
{
#if defined(__HIP_DEVICE_COMPILE__)
  return __uint_as_float(u);
#else
  float f;
  std::memcpy(&f, &u, 4);
  return f;
#endif
}
BPVO_DF_HD inline uint64_t df_key(float d, float v) { return ((uint64_t) df_bits(d) << 32) | (uint64_t) df_bits(v); }

// Prediction of one carried pixel.  P: the motion's first three rows, row-major [3][4].  True: *target = ty * cols + tx and *key are the candidate.
BPVO_DF_HD inline bool df_splat(const DfCamera& c, const float* P, float q2, int x, int y, float d, float vc, int* target, uint64_t* key)
{
  if(!(vc >= 0.0f)) return false;      // (the pixel carries nothing; NaN too)
  const double fx = (double) c.fx, fy = (double) c.fy, cx = (double) c.cx, cy = (double) c.cy;
  const double fb = fx * (double) c.b;
  const double Z = fb / (double) d;
  const double X = (((double) x - cx) * Z) / fx;
  const double Y = (((double) y - cy) * Z) / fy;
  const double Xn = (((double) P[0] * X + (double) P[1] * Y) + (double) P[2] * Z) + (double) P[3];
  const double Yn = (((double) P[4] * X + (double) P[5] * Y) + (double) P[6] * Z) + (double) P[7];
  const double Zn = (((double) P[8] * X + (double) P[9] * Y) + (double) P[10] * Z) + (double) P[11];
  if(!(Zn > 0.0)) return false;
  const double u = (fx * Xn) / Zn + cx;
  const double v = (fy * Yn) / Zn + cy;
  if(!(fabs(u) < 1073741824.0) || !(fabs(v) < 1073741824.0)) return false;      // (NaN and Inf fail the comparison; below 2^30 the cast is exact)
  const int tx = (int) rint(u);      // ties to even
  const int ty = (int) rint(v);
  if(tx < 0 || tx >= c.cols || ty < 0 || ty >= c.rows) return false;
  const float dn = (float) (fb / Zn);
  if(!(dn > 0.0f) || !df_valid(dn, c.lo, c.hi)) return false;      // (d' > 0: the key of a candidate is never 0, the word of "no candidate")
  const double s = (double) dn / (double) d;
  const double s2 = s * s;
  const float vn = (float) (((double) vc * s2) * s2 + (double) q2);
  if(!(vn >= 0.0f) || !(vn <= 3.4028234663852886e38f)) return false;      // (finite; a carried variance is never negative)
  *target = ty * c.cols + tx;
  *key = df_key(dn, vn);
  return true;
}

BPVO_DF_HD inline float df_div(float a, float b) { return (float) ((double) a / (double) b); }
BPVO_DF_HD inline float df_sqrt(float a) { return (float) sqrt((double) a); }

// Update of one pixel: the measurement m and the target's word (0: no candidate arrived).  Writes the carried pair and returns the class;
// *D is m's own bits wherever the row says m.
BPVO_DF_HD inline int df_update(const DfRule& r, float lo, float hi, float m, uint64_t word, float* D, float* V)
{
  const bool mv = df_valid(m, lo, hi);
  const bool has = word != 0;
  const float pd = df_float((uint32_t) (word >> 32)), pv = df_float((uint32_t) word);
  if(mv && has) {
    const float s = pv + r.r2;
    const float bound = r.gate * df_sqrt(s);
    const float diff = m - pd;
    if(fabsf(diff) <= bound) {
      const float k = df_div(pv, s);
      const float kd = k * diff;
      const float f = pd + kd;
      const float kv = k * pv;
      *D = df_valid(f, lo, hi) ? f : m;
      *V = pv - kv;
      return DF_FUSED;
    }
    *D = m; *V = r.r2;
    return DF_REPLACED;
  }
  if(mv) { *D = m; *V = r.r2; return DF_MEASURED; }
  if(has && pv <= r.fill2) { *D = pd; *V = pv; return DF_FILLED; }
  *D = m; *V = -1.0f;
  return DF_NONE;
}

}  // namespace bpvo_hip
