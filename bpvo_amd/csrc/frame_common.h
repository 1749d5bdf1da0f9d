// Per-frame kernels, shared device helpers: OpenCV's border rule, the launch grid of the one-thread-per-pixel kernels.
#pragma once
#include "kernels.h"

namespace bpvo_hip {

__device__ __forceinline__ int reflect101(int p, int len)
{
  // cv::borderInterpolate(BORDER_REFLECT_101); one reflection suffices for the <= 3 pixel halos used here
  if(p < 0) p = -p;
  if(p >= len) p = 2 * len - 2 - p;
  if(p < 0) p = 0;   // degenerate len == 1
  return p;
}

// the same for halos that may exceed the image (wide smoothing kernels on the coarsest levels): reflect until inside
__device__ __forceinline__ int reflect101_wide(int p, int len)
{
  if(len == 1) return 0;
  while(p < 0 || p >= len) p = p < 0 ? -p : 2 * len - 2 - p;
  return p;
}

// ---- the arithmetic of the bit-planes blur (cv::GaussianBlur 5x5 on 0 / 1 samples, f32, no fusing), stated once for the three kernels
// that evaluate it: bitplanes_blur_kernel, template_build_kernel (lazy levels) and saliency_select_tile_kernel (census-only levels).
// A census byte spread to one BYTE per plane (two words: planes 0-3, 4-7)
__device__ __forceinline__ uint2 spread_planes(unsigned c)
{
  unsigned lo = c & 0xFu, hi = (c >> 4) & 0xFu;
  lo = (lo | (lo << 14)) & 0x00030003u; lo = (lo | (lo << 7)) & 0x01010101u;
  hi = (hi | (hi << 14)) & 0x00030003u; hi = (hi | (hi << 7)) & 0x01010101u;
  return make_uint2(lo, hi);
}
// Row pass: t = S0*k0 + (S-1 + S+1)*k1 + (S-2 + S+2)*k2 of samples that are 0 or 1 takes one of 2 x 3 x 3 values.  The index
// a + 3 b + 9 S0 of the five positions of a row window (bytewise for four planes at once: <= 17, no carries) ...
__device__ __forceinline__ unsigned bp_row_index(unsigned cm2, unsigned cm1, unsigned c0, unsigned cp1, unsigned cp2)
{
  return (cm1 + cp1) + 3u * (cm2 + cp2) + 9u * c0;
}
// ... and entry e of the eighteen-entry table, evaluated with the very expression of the row pass
__device__ __forceinline__ float bp_row_entry(int e, float k0, float k1, float k2)
{
  const float S0 = (float) (e / 9), A = (float) (e % 3), B = (float) ((e / 3) % 3);
  return S0 * k0 + A * k1 + B * k2;
}
// Column pass over the row-pass values of rows y-2 .. y+2: exactly OpenCV's symmetric 5-tap filter
__device__ __forceinline__ float bp_col(float Tm2, float Tm1, float T0, float Tp1, float Tp2, float k0, float k1, float k2)
{
  float o = k0 * T0;
  o += k1 * (Tp1 + Tm1);
  o += k2 * (Tp2 + Tm2);
  return o;
}
// REFLECT_101 on a CENSUS coordinate of a staged window whose far end may run past the halo (p <= len + 1 after the clamp)
__device__ __forceinline__ int bp_census_coord(int p, int len) { return reflect101(min(p, len + 1), len); }

// Template frames of a pair batch at the NMS levels keep no records (FrameJob::lazy) — except in the 64-pixel tile columns whose records
// the saliency of the columns the reference's SIMD body treats apart reads (saliency_generic): x < 4 is formed from columns n - 4 + x and
// x >= n = W & ~3 is the scalar tail (Q7), together columns n - 5 .. W - 1: the tile columns at the right edge stay dense.  And when W is
// a multiple of 4, column x = 3 is formed at xs = W - 1, whose right neighbour is the reference's read past the end of the row, the
// record of column 0 of the NEXT row: the first tile column stays dense too.  x0: first column of the tile (a multiple of 64).
__host__ __device__ __forceinline__ bool bp_tile_column_is_lazy(int x0, int W)
{
  return x0 + 64 + 8 <= (W & ~3) && !(x0 == 0 && (W & 3) == 0);
}

// 64 x 4-pixel workgroups over a W x R level, one grid plane per frame
static inline dim3 grid2d(int W, int R, int nz) { return dim3((W + 63) / 64, (R + 3) / 4, nz); }

}  // namespace bpvo_hip
