// K6 warp + residual, device side: projection, validity, (cached) bilinear taps, residuals of one template point / one 256-point chunk.
#pragma once
#include "gn_common.h"
#include "warp_rule.h"

namespace bpvo_hip {

// ------------------------------------------------------------------------------------------------------------------
// K6 warp_residual.  reference: TemplateData::computeResiduals (bpvo/template_data.cc:174-189) =
//   RigidBodyWarp::setPose (bpvo/rigid_body_warp.h:111-114): P = K * T[0:3,:] in f32, index-order sums
//   PhotoError::Impl::init: projection, Floor and validity — warp_foot (warp_rule.h)
//   PhotoError::Impl::run kLinear (bpvo/photo_error.cc:365-389,446-449): Iw in f64, r = float(Iw - I0); invalid -> 0
// One thread per template point; all C channels of the point are handled by the same thread because the descriptor is
// pixel-interleaved: the 4 taps are 2 x (2*C floats) contiguous, fetched as 16-byte loads.
// FAST selects the reference's alternative all-f32 formulation (inactive there, PHOTO_ERROR_OPT = 0): projectPoints (warp_foot_f32,
// warp_rule.h: truncation, coefficients C) followed by PhotoError::Impl::operator() / run of that branch (bpvo/photo_error.cc:118-214; same arithmetic as BilinearInterp,
// bpvo/interp_util.h:49-71,93-96,184-203): Iw = dp_ps(C, [I00, I01, I10, I11]) = (C0*I00 + C1*I01) + (C2*I10 + C3*I11),
// r = Iw - I0, and for an invalid point Iw = 0, i.e. r = -I0.
// P = K * T[0:3,:] in f32, index-order sums (RigidBodyWarp::setPose, bpvo/rigid_body_warp.h:111-114)
__device__ __forceinline__ void projection_matrix(const PairJob& j, const float* __restrict__ T, float (&P)[12])
{
#pragma unroll
  for(int r = 0; r < 3; ++r)
#pragma unroll
    for(int c = 0; c < 4; ++c) {
      float s = j.K[r * 3 + 0] * T[0 * 4 + c];
      s += j.K[r * 3 + 1] * T[1 * 4 + c];
      s += j.K[r * 3 + 2] * T[2 * 4 + c];
      P[r * 4 + c] = s;
    }
}

// DisparitySpaceWarp::setPose (bpvo/disparity_space_warp.h:36): H = G * T * G_inv in f32, the two fixed 4x4 products left
// to right, G / G_inv as the constructor fills them (bpvo/disparity_space_warp.cc:26-47).  P <- rows 0, 1, 3 of H: with
// them operator() (:66-71) is projectPoints' form plus the principal point (x = pw0 * (1 / pw3) + cx): warp_foot_f32 with `dspace`.
__device__ __forceinline__ void dspace_matrix(const PairJob& j, const float* __restrict__ T, float (&P)[12])
{
  const float fx = j.K[0], fy = j.K[4];
  M44 G, Gi, Tm;
  for(int i = 0; i < 16; ++i) { G.m[i] = 0.0f; Gi.m[i] = 0.0f; Tm.m[i] = T[i]; }
  G.m[0] = fx; G.m[5] = fy; G.m[11] = fx * j.b; G.m[14] = 1.0f;
  Gi.m[0] = (float) (1.0 / (double) fx); Gi.m[5] = (float) (1.0 / (double) fy); Gi.m[11] = 1.0f;
  Gi.m[14] = (float) (1.0 / (double) (fx * j.b));
  const M44 H = m44_mul(m44_mul(G, Tm), Gi);
#pragma unroll
  for(int c = 0; c < 4; ++c) { P[c] = H.m[c]; P[4 + c] = H.m[4 + c]; P[8 + c] = H.m[12 + c]; }
}

// PhotoError::Impl::run kLinear on one channel: Iw in f64 from the four taps, r = float(Iw - I0)
__device__ __forceinline__ float bilinear_res(float i00, float i01, float i10, float i11, float i0, double xf, double yf, double wx, double wy)
{
  const double Iw = wy * ((double) i00 * wx + (double) i01 * xf) + yf * ((double) i10 * wx + (double) i11 * xf);
  return (float) (Iw - (double) i0);
}
// ... and of the all-f32 formulation (FAST): Iw = dp_ps(cf, [I00, I01, I10, I11]), r = Iw - I0
__device__ __forceinline__ float bilinear_res_f32(float i00, float i01, float i10, float i11, float i0, const float (&cf)[4])
{
  const float Iw = (cf[0] * i00 + cf[1] * i01) + (cf[2] * i10 + cf[3] * i11);
  return Iw - i0;
}

// The C = 8 bilinear footprint as eight 16-byte pieces, which is how it is gathered and how the tap cache keeps it.
// pieces 0, 1: I00 of channels 0-3 / 4-7; 2, 3: I01; 4, 5: I10; 6, 7: I11
__device__ __forceinline__ unsigned tap_key(int xi, int yi) { return ((unsigned) yi << 16) | (unsigned) xi; }
__device__ __forceinline__ void taps8_gather(const PairJob& j, int xi, int yi, int W, float4 (&t)[8])
{
  const float4* q0 = reinterpret_cast<const float4*>(j.desc + ((size_t) yi * W + xi) * 8);
  const float4* q1 = q0 + (size_t) W * 2;
  t[0] = q0[0]; t[1] = q0[1]; t[2] = q0[2]; t[3] = q0[3];
  t[4] = q1[0]; t[5] = q1[1]; t[6] = q1[2]; t[7] = q1[3];
}
template <bool NT>
__device__ __forceinline__ void taps8_cache_store(const PairJob& j, int i, unsigned key, const float4 (&t)[8])
{
  float4* tc = reinterpret_cast<float4*>(j.tapcache.get());
#pragma unroll
  for(int k = 0; k < 8; ++k) store_v4<NT>(tc + tile_index<8>(i, k), t[k]);
  j.tapkey[i] = key;
}
__device__ __forceinline__ void taps8_unpack(const float4 (&t)[8], const float4 px0, const float4 px1, float (&i00)[8], float (&i01)[8],
                                             float (&i10)[8], float (&i11)[8], float (&i0)[8])
{
#pragma unroll
  for(int h = 0; h < 2; ++h) {
    i00[4 * h] = t[h].x; i00[4 * h + 1] = t[h].y; i00[4 * h + 2] = t[h].z; i00[4 * h + 3] = t[h].w;
    i01[4 * h] = t[2 + h].x; i01[4 * h + 1] = t[2 + h].y; i01[4 * h + 2] = t[2 + h].z; i01[4 * h + 3] = t[2 + h].w;
    i10[4 * h] = t[4 + h].x; i10[4 * h + 1] = t[4 + h].y; i10[4 * h + 2] = t[4 + h].z; i10[4 * h + 3] = t[4 + h].w;
    i11[4 * h] = t[6 + h].x; i11[4 * h + 1] = t[6 + h].y; i11[4 * h + 2] = t[6 + h].z; i11[4 * h + 3] = t[6 + h].w;
  }
  i0[0] = px0.x; i0[1] = px0.y; i0[2] = px0.z; i0[3] = px0.w; i0[4] = px1.x; i0[5] = px1.y; i0[6] = px1.z; i0[7] = px1.w;
}
// residuals of the eight channels from the pieces and the template pixel's two halves
__device__ __forceinline__ void taps8_residuals(const float4 (&t)[8], const float4 px0, const float4 px1, double xf, double yf, float (&res)[8])
{
  const double wx = 1.0 - xf, wy = 1.0 - yf;
  float i00[8], i01[8], i10[8], i11[8], i0[8];
  taps8_unpack(t, px0, px1, i00, i01, i10, i11, i0);
#pragma unroll
  for(int c = 0; c < 8; ++c) res[c] = bilinear_res(i00[c], i01[c], i10[c], i11[c], i0[c], xf, yf, wx, wy);
}

// One template point of warp_residual: projection, validity, (cached) bilinear taps, residuals of all C channels.
// `in_block` gates the tap-cache update (lanes past the end of a block redo the last point, loads only).  Returns valid.
// HALF (C = 8, f64 formulation): the taps are fetched and consumed in two groups of four channels, which halves the
// registers they occupy — for the fused path of irls_reduce, where the 29 accumulators are live as well.
// `X_out` (optional): receives the point as rebuilt here, for a caller that needs it as well — the fused path's Jacobian — so that it is
// requested from memory once per point, not twice (streaming loads: the second request went out to HBM again, 3.8 % of irls_reduce_both's bytes).
template <int C, bool FAST, bool HALF = false, bool NT = true>
__device__ __forceinline__ bool warp_point(const PairJob& j, const float (&P)[12], int i, bool in_block, float (&res)[C], bool& cache_hit,
                                           float4* X_out = nullptr)
{
  cache_hit = false;
  const int W = j.cols, R = j.rows;
  const float4 X = load_point<NT>(j, i);
  if(X_out) *X_out = X;
  // C = 1: the launches are short and latency-bound, so the key, the cached taps and the template pixel are requested
  // together with the point instead of after the projection (16 speculative bytes per point; for C = 8 the same
  // speculation costs 128 bytes and was measured slower)
  unsigned spec_key = 0; float4 spec_taps = make_float4(0.0f, 0.0f, 0.0f, 0.0f); float spec_pix = 0.0f;
  if constexpr(C == 1) {
    if(j.tapcache_on) {      // (uniform over the workspace: dense levels run without the cache)
      spec_key = j.tapkey[i];
      spec_taps = load_v4<NT>(reinterpret_cast<const float4*>(j.tapcache.get()) + i);
    }
    spec_pix = j.pix[i];
  }
  int xi = 0, yi = 0;
  bool valid;
  double xf = 0.0, yf = 0.0;       // fractional parts (standard formulation)
  float cf[4] = {0, 0, 0, 0};      // interpolation coefficients (FAST formulation)
  if constexpr(!FAST) {
    const WarpFoot f = warp_foot(P, X.x, X.y, X.z, X.w, W, R);
    xi = f.xi; yi = f.yi; valid = f.valid; xf = f.xf; yf = f.yf;
  } else {
    const WarpFootF32 f = warp_foot_f32(P, X.x, X.y, X.z, X.w, j.dspace != 0, j.K[2], j.K[5], W, R);
    xi = f.xi; yi = f.yi; valid = f.valid;
#pragma unroll
    for(int k = 0; k < 4; ++k) cf[k] = f.cf[k];
  }

  if constexpr(HALF && C == 8 && !FAST) {
    if(valid) {
      const double wx = 1.0 - xf, wy = 1.0 - yf;
      const float4* q0 = reinterpret_cast<const float4*>(j.desc + ((size_t) yi * W + xi) * 8);
      const float4* q1 = q0 + (size_t) W * 2;
      const unsigned key = tap_key(xi, yi);
      const bool cached = j.tapcache_on != 0;       // (uniform over the workspace) dense levels gather straight from the descriptor
      const bool hit = cached && j.tapkey[i] == key;
      cache_hit = hit;
      float4* tc = reinterpret_cast<float4*>(j.tapcache.get());
      const float4* p0 = reinterpret_cast<const float4*>(j.pix.get());
#pragma unroll
      for(int h = 0; h < 2; ++h) {
        float4 a, b, c, d;      // I00, I01, I10, I11 of channels 4h .. 4h+3
        if(hit) {
          a = load_v4<NT>(tc + tile_index<8>(i, h)); b = load_v4<NT>(tc + tile_index<8>(i, 2 + h));
          c = load_v4<NT>(tc + tile_index<8>(i, 4 + h)); d = load_v4<NT>(tc + tile_index<8>(i, 6 + h));
        } else {
          a = q0[h]; b = q0[2 + h]; c = q1[h]; d = q1[2 + h];
          if(in_block && cached) {
            store_v4<NT>(tc + tile_index<8>(i, h), a); store_v4<NT>(tc + tile_index<8>(i, 2 + h), b);
            store_v4<NT>(tc + tile_index<8>(i, 4 + h), c); store_v4<NT>(tc + tile_index<8>(i, 6 + h), d);
          }
        }
        const float4 t = load_v4<NT>(p0 + tile_index<2>(i, h));
        const float i00[4] = {a.x, a.y, a.z, a.w}, i01[4] = {b.x, b.y, b.z, b.w}, i10[4] = {c.x, c.y, c.z, c.w},
                    i11[4] = {d.x, d.y, d.z, d.w}, i0[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
        for(int k = 0; k < 4; ++k) res[4 * h + k] = bilinear_res(i00[k], i01[k], i10[k], i11[k], i0[k], xf, yf, wx, wy);
        if(h == 0) __builtin_amdgcn_sched_barrier(0);   // keep the second group's loads behind the first group's arithmetic
      }
      if(!hit && in_block && cached) j.tapkey[i] = key;
    } else {
#pragma unroll
      for(int c = 0; c < 8; ++c) res[c] = 0.0f;
    }
    return valid;
  }

  // generic layout: records of `pitch` floats (= C, or the whole channel count when this job is one channel group of a wide descriptor)
  const int PT = (C == 8 || C == 1) ? C : j.pitch;
  if(valid) {
    const double wx = 1.0 - xf, wy = 1.0 - yf;
    const float* __restrict__ d0 = j.desc + ((size_t) yi * W + xi) * PT;
    const float* __restrict__ d1 = d0 + (size_t) W * PT;
    float I00[C], I01[C], I10[C], I11[C], I0[C];
    if constexpr(C == 8) {
      // Tap cache: the integer footprint (xi, yi) of a point rarely changes between consecutive GN iterations of a level
      // (sub-pixel pose updates), and then the four taps are the same 128 bytes.  They are kept per point in a tiled,
      // fully coalesced buffer keyed by (yi << 16 | xi): a hit replaces the gather — two 64-byte segments that cost
      // 2.3 128-byte HBM lines on average (profiles/r01_pmc_summary.txt) — by one coalesced 128-byte read.
      const unsigned key = tap_key(xi, yi);
      const bool cached = j.tapcache_on != 0;       // (uniform over the workspace) dense levels gather straight from the descriptor
      const bool hit = cached && j.tapkey[i] == key;
      cache_hit = hit;
      float4 t[8];
      if(hit) {
        const float4* tc = reinterpret_cast<const float4*>(j.tapcache.get());
#pragma unroll
        for(int k = 0; k < 8; ++k) t[k] = load_v4<NT>(tc + tile_index<8>(i, k));
      } else {
        taps8_gather(j, xi, yi, W, t);
        if(in_block && cached) taps8_cache_store<NT>(j, i, key, t);
      }
      const float4* p0 = reinterpret_cast<const float4*>(j.pix.get());
      const float4 t0 = load_v4<NT>(p0 + tile_index<2>(i, 0)), t1 = load_v4<NT>(p0 + tile_index<2>(i, 1));
      taps8_unpack(t, t0, t1, I00, I01, I10, I11, I0);
    } else if constexpr(C == 1) {
      // the same tap cache for single-channel descriptors: the four taps of a point are one 16-byte record.  The gather
      // costs two (mostly distinct) HBM lines per point at the sparse levels for 16 useful bytes; a hit is one coalesced load.
      const unsigned key = tap_key(xi, yi);
      float4* tc = reinterpret_cast<float4*>(j.tapcache.get());
      float4 t = spec_taps;
      const bool cached = j.tapcache_on != 0;
      cache_hit = cached && spec_key == key;
      if(!cache_hit) {
        t = make_float4(d0[0], d0[1], d1[0], d1[1]);
        if(in_block && cached) { store_v4<NT>(tc + i, t); j.tapkey[i] = key; }
      }
      I00[0] = t.x; I01[0] = t.y; I10[0] = t.z; I11[0] = t.w;
      I0[0] = spec_pix;
    } else {
#pragma unroll
      for(int c = 0; c < C; ++c) {
        I00[c] = d0[c]; I01[c] = d0[PT + c]; I10[c] = d1[c]; I11[c] = d1[PT + c];
        I0[c] = j.pix[(size_t) i * PT + c];
      }
    }
#pragma unroll
    for(int c = 0; c < C; ++c) {
      if constexpr(!FAST) {
        res[c] = bilinear_res(I00[c], I01[c], I10[c], I11[c], I0[c], xf, yf, wx, wy);
      } else {
        res[c] = bilinear_res_f32(I00[c], I01[c], I10[c], I11[c], I0[c], cf);
      }
    }
  } else {
    if constexpr(!FAST) {
#pragma unroll
      for(int c = 0; c < C; ++c) res[c] = 0.0f;
    } else {   // operator() returns 0 for an invalid point and run() still subtracts I0 (photo_error.cc:203-210)
      if constexpr(C == 8) {
        const float4* p0 = reinterpret_cast<const float4*>(j.pix.get());
        const float4 t0 = p0[tile_index<2>(i, 0)], t1 = p0[tile_index<2>(i, 1)];
        res[0] = 0.0f - t0.x; res[1] = 0.0f - t0.y; res[2] = 0.0f - t0.z; res[3] = 0.0f - t0.w;
        res[4] = 0.0f - t1.x; res[5] = 0.0f - t1.y; res[6] = 0.0f - t1.z; res[7] = 0.0f - t1.w;
      } else {
#pragma unroll
        for(int c = 0; c < C; ++c) res[c] = 0.0f - j.pix[(size_t) i * PT + c];
      }
    }
  }
  return valid;
}

// The work of one 256-thread chunk of warp_residual on workspace j: points [chunk * 256, chunk * 256 + 256), `s` the chunk's LDS
// scratch of the bracket step.  All 256 threads must call it.
// mode 0: every active workspace.  mode 1 (estimate loops with the fused path): skip workspaces whose scale is frozen
// for the rest of the level — no median is needed and irls_reduce recomputes their residuals itself.  mode 2: refresh
// the residual / valid buffers of workspaces marked r_stale from the pose of their last linearisation (T_lin).
// dense: the bracket step's dense form (bracket_chunk; chain launches only).
template <int C, bool FAST>
__device__ __forceinline__ void warp_chunk(const PairJob& j, int mode, unsigned chunk, BracketLds& s, bool dense = false)
{
  const GNState* __restrict__ st = j.st;
  if(mode == 2) { if(!st->r_stale) return; }
  else {
    if(!st->active) return;
    if(mode == 1 && !(st->delta_scale > 1e-6f)) return;
  }
  const int n = j.n;
  if((int) (chunk * K6_BLOCK) >= n) return;

  if(mode != 2 && chunk == 0 && threadIdx.x == 0) j.cnt[4] += (unsigned long long) n;   // points this kernel processes

  float P[12];
  if(FAST && j.dspace) dspace_matrix(j, mode == 2 ? st->T_lin : st->T, P);
  else projection_matrix(j, mode == 2 ? st->T_lin : st->T, P);

  // lanes past the end of the last block redo the last point (loads only) so that the whole block reaches the
  // block-level bracket step below; their stores are masked
  const int i_raw = chunk * K6_BLOCK + threadIdx.x;
  const bool in_block = i_raw < n;
  const int i = in_block ? i_raw : n - 1;
  float res[C];
  bool hit;
  const bool valid = warp_point<C, FAST>(j, P, i, in_block, res, hit);
  if(in_block) j.valid[i] = valid ? 1 : 0;
  if(in_block) {
    if constexpr(C == 8) {     // tiled residual record: two fully coalesced 16-byte stores per lane
      float4* o = reinterpret_cast<float4*>(j.r.get());
      store_stream(o + tile_index<2>(i, 0), make_float4(res[0], res[1], res[2], res[3]));
      store_stream(o + tile_index<2>(i, 1), make_float4(res[4], res[5], res[6], res[7]));
    } else {      // generic C: point-major records [N][pitch]
#pragma unroll
      for(int c = 0; c < C; ++c) j.r[(size_t) i * j.pitch + c] = res[c];
    }
  }
  // bracket pass of the exact median (see bracket_chunk) while the residuals are in registers
  if(mode != 2 && (st->delta_scale > 1e-6f) && st->median_valid) {
    if(dense) bracket_chunk<C, true>(j, st->lo_key, st->hi_key, valid && in_block, hit && valid && in_block, res, chunk, (int) (threadIdx.x >> 6), s, true);
    else bracket_chunk<C, false>(j, st->lo_key, st->hi_key, valid && in_block, hit && valid && in_block, res, chunk, (int) (threadIdx.x >> 6), s, true);
  }
}

}  // namespace bpvo_hip
