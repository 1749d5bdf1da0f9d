// Normalised intensity (bpvo_hip_set_intensity_normalization; include/bpvo_hip/c_api.h states the rule): the rule as code, once.  Shared by the
// kernels (kernels_intensity_norm.hip) and the CPU test (tests/test_intensity_norm_cpu.py builds tests/cpp/intensity_norm_harness.cc around this
// header with a plain C++ compiler and compares it with tests/intensity_norm_ref.py bit for bit).  Integers up to the last step; the last step is
// f64 — one product (whole image), or one product, one square root and one quotient (local), each correctly rounded on host and device alike
// (the library is built with -ffp-contract=off) — and one conversion to f32.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define BPVO_INORM_HD __host__ __device__ inline
#else
#define BPVO_INORM_HD inline
#endif

namespace bpvo_hip {

constexpr int kInormOff = -1;          // the radius that turns the mode off
constexpr int kInormMaxRadius = 15;    // radius 0: whole image; 1 .. kInormMaxRadius: local, a (2 R + 1)^2 window
constexpr double kInormUnit = 32.0;    // descriptor units per robust standard deviation
constexpr double kInormMadToSigma = 1.4826;

// ---- radius 0, whole image: median and MAD from the 256-bin histogram h of the n_px pixels, through its running sums cum[v] = #{I <= v}.
// med: the smallest v with cum[v] >= (n_px + 1) / 2 (the lower median of an even count); mad: the smallest k with #{|I - med| <= k} >= (n_px + 1) / 2,
// the same histogram folded about med — inorm_folded_count reads that count off the running sums.
BPVO_INORM_HD uint32_t inorm_half(uint32_t n_px) { return (n_px + 1u) / 2u; }
template <class Cum>
BPVO_INORM_HD uint32_t inorm_folded_count(const Cum& cum, int med, int k)      // #{|I - med| <= k}
{
  const int hi = med + k < 255 ? med + k : 255, lo = med - k - 1;
  return cum[hi] - (lo >= 0 ? cum[lo] : 0u);
}
// (serial: the host's statement; the kernel forms cum with a parallel scan and counts, per bin, the two predicates below that are still false)
template <class Hist>
BPVO_INORM_HD void inorm_median_mad(const Hist& h, uint32_t n_px, int* med, int* mad)
{
  const uint32_t half = inorm_half(n_px);
  uint32_t cum[256];
  uint32_t acc = 0;
  for(int v = 0; v < 256; ++v) { acc += h[v]; cum[v] = acc; }
  int m = 0, k = 0;
  while(m < 255 && cum[m] < half) ++m;
  while(k < 255 && inorm_folded_count(cum, m, k) < half) ++k;
  *med = m;
  *mad = k;
}
// entry v of the table the plane is: D = (float) ((double) (v - med) * c), c = 32 / (1.4826 * max(mad, 1)) in f64
BPVO_INORM_HD float inorm_table_entry(int v, int med, int mad)
{
  const double c = kInormUnit / (kInormMadToSigma * (double) (mad > 1 ? mad : 1));
  return (float) ((double) (v - med) * c);
}

// ---- radius 1 .. 15, local: the window [x - R, x + R] x [y - R, y + R] cut to the W x H image
BPVO_INORM_HD int inorm_window_count(int x, int y, int W, int H, int R)
{
  const int x0 = x - R > 0 ? x - R : 0, x1 = x + R < W - 1 ? x + R : W - 1;
  const int y0 = y - R > 0 ? y - R : 0, y1 = y + R < H - 1 ? y + R : H - 1;
  return (x1 - x0 + 1) * (y1 - y0 + 1);
}
// I: the pixel; n, S1 = sum I, S2 = sum I^2 over its window.  X = n I - S1 (32 bits), V = n S2 - S1^2 (64 bits), Vf = max(V, 4 n^2): a floor of
// two grey levels on the window's standard deviation.  D = (float) (32 X / sqrt(Vf)) in f64.
BPVO_INORM_HD float inorm_local_value(int I, int n, uint32_t S1, uint32_t S2)
{
  const int32_t X = (int32_t) n * (int32_t) I - (int32_t) S1;
  const int64_t V = (int64_t) n * (int64_t) S2 - (int64_t) S1 * (int64_t) S1;
  const int64_t floor_ = 4 * (int64_t) n * (int64_t) n;
  const int64_t Vf = V > floor_ ? V : floor_;
  return (float) (kInormUnit * (double) X / sqrt((double) Vf));
}

}  // namespace bpvo_hip
