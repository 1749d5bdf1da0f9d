// The scale of the Student-t loss, device side: the fixed point of T (tscale_math.h, c_api.h) over the residuals of one workspace by one workgroup.
// It stands where the exact median stands for the other losses (launch_median), behind the same gate.
#pragma once
#include "gn_common.h"
#include "tscale_math.h"

namespace bpvo_hip {

// The residuals are summed in WAVE TILES: 64 consecutive points (C = 1: 256, a lane's float4 of four points), every channel of a point in channel
// order on the point's lane in f64, the 64 lanes by a fixed butterfly, the tiles of a round of TS_ROUND tiles from an LDS table in tile order
// (lane l: tiles l, l + 64, ...; then the butterfly), the rounds one after the other.  Which wave sums a tile, how many waves there are, the
// batch and the place in the active list do not enter: the sum of a pass — and with it sigma — is a function of the residuals alone.
constexpr int TS_ROUND = 2048;      // wave tiles per combine round (16 KB of f64 tile sums)
constexpr int TS_U = 4;             // wave tiles in flight per wave: all loads of a step are issued before the first use

__device__ __forceinline__ double wave_sum_f64(double v)      // xor butterfly: both partners of a step add the same two values, so every lane ends with the same bits
{
#pragma unroll
  for(int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

struct TScaleLds {
  double tile[TS_ROUND];
  TScaleFit fit;
  double sum;                // the last pass's sum (wave 0 writes, everybody reads behind a barrier)
  unsigned cnt[2];           // valid points, non-zero entries (the first pass)
};

// One pass over the valid residuals of j: the f64 sum of val(r) over every entry, in wave 0 (uniform over it).  COUNT: the thread's valid points
// and non-zero entries are added to nv / nz.  Block-wide (it holds barriers).  The three layouts are for_each_valid_key's (gn_median.h).
template <int C, int NT, bool COUNT, typename Val>
__device__ __forceinline__ double tscale_pass(const PairJob& j, TScaleLds& s, Val val, unsigned& nv, unsigned& nz)
{
  constexpr int NW = NT / 64;
  constexpr int PTS = (C == 1) ? 256 : 64;      // points of a wave tile
  const int n = j.n;
  const int ntiles = (n + PTS - 1) / PTS;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double total = 0.0;
  auto entry = [&](float r, double& acc) {
    acc += (double) val(r);
    if(COUNT) nz += (r != 0.0f) ? 1u : 0u;
  };
  for(int r0 = 0; r0 < ntiles; r0 += TS_ROUND) {
    const int r1 = min(ntiles, r0 + TS_ROUND);
    for(int t0 = r0 + wave; t0 < r1; t0 += NW * TS_U) {
      if constexpr(C == 8) {
        const float4* q = reinterpret_cast<const float4*>(j.r.get());
        unsigned char v[TS_U];
        float4 a[TS_U], b[TS_U];
#pragma unroll
        for(int u = 0; u < TS_U; ++u) {
          const int t = t0 + u * NW, pt = t * 64 + lane;
          const bool in = t < r1 && pt < n;
          v[u] = in ? j.valid[pt] : (unsigned char) 0;
          a[u] = in ? q[tile_index<2>(pt, 0)] : make_float4(0, 0, 0, 0);
          b[u] = in ? q[tile_index<2>(pt, 1)] : make_float4(0, 0, 0, 0);
        }
#pragma unroll
        for(int u = 0; u < TS_U; ++u) {
          const int t = t0 + u * NW;
          if(t >= r1) continue;      // (uniform over the wave)
          double acc = 0.0;
          if(v[u]) {
            if(COUNT) nv += 1u;
            entry(a[u].x, acc); entry(a[u].y, acc); entry(a[u].z, acc); entry(a[u].w, acc);
            entry(b[u].x, acc); entry(b[u].y, acc); entry(b[u].z, acc); entry(b[u].w, acc);
          }
          acc = wave_sum_f64(acc);
          if(lane == 0) s.tile[t - r0] = acc;
        }
      } else if constexpr(C == 1) {
        uchar4 v[TS_U];
        float4 a[TS_U];
#pragma unroll
        for(int u = 0; u < TS_U; ++u) {
          const int t = t0 + u * NW, p4 = t * 256 + lane * 4;      // n is a multiple of 16
          const bool in = t < r1 && p4 < n;
          v[u] = in ? *reinterpret_cast<const uchar4*>(j.valid + p4) : make_uchar4(0, 0, 0, 0);
          a[u] = in ? *reinterpret_cast<const float4*>(j.r + p4) : make_float4(0, 0, 0, 0);
        }
#pragma unroll
        for(int u = 0; u < TS_U; ++u) {
          const int t = t0 + u * NW;
          if(t >= r1) continue;
          double acc = 0.0;
          if(v[u].x) { if(COUNT) nv += 1u; entry(a[u].x, acc); }
          if(v[u].y) { if(COUNT) nv += 1u; entry(a[u].y, acc); }
          if(v[u].z) { if(COUNT) nv += 1u; entry(a[u].z, acc); }
          if(v[u].w) { if(COUNT) nv += 1u; entry(a[u].w, acc); }
          acc = wave_sum_f64(acc);
          if(lane == 0) s.tile[t - r0] = acc;
        }
      } else {      // generic C: point-major records; every channel of the record (C x the groups of a wide descriptor)
        const int CT = C * j.n_groups;
        const size_t PT = (size_t) j.pitch;
#pragma unroll
        for(int u = 0; u < TS_U; ++u) {
          const int t = t0 + u * NW;
          if(t >= r1) continue;
          const int pt = t * 64 + lane;
          double acc = 0.0;
          if(pt < n && j.valid[pt]) {
            if(COUNT) nv += 1u;
            for(int c0 = 0; c0 < CT; c0 += C) {
              float rr[C];
#pragma unroll
              for(int c = 0; c < C; ++c) rr[c] = j.r[(size_t) pt * PT + c0 + c];
#pragma unroll
              for(int c = 0; c < C; ++c) entry(rr[c], acc);
            }
          }
          acc = wave_sum_f64(acc);
          if(lane == 0) s.tile[t - r0] = acc;
        }
      }
    }
    __syncthreads();
    if(wave == 0) {
      double a = 0.0;
#pragma unroll 4
      for(int q = 0; q < TS_ROUND / 64; ++q) {
        const int k = q * 64 + lane;
        a += (r0 + k < r1) ? s.tile[k] : 0.0;
      }
      total += wave_sum_f64(a);
    }
    __syncthreads();
  }
  return total;
}

// The work of one NT-thread workgroup on workspace j: the fit, then (thread 0) the state.  `last_median` > 0 marks a level that holds an estimated
// scale (it is 0 after gn_level_reset and after a reset of the seam); median_valid stays 0, so the bracket step never runs for such a workspace.
template <int C, int NT>
__device__ __forceinline__ void tscale_block(const PairJob& j, GNState* st, TScaleLds& s)
{
  const int tid = threadIdx.x;
  const float sigma_prev = st->scale;
  const bool have_prev = st->last_median > 0.0f;
  if(tid == 0) { s.cnt[0] = 0u; s.cnt[1] = 0u; s.sum = 0.0; }
  __syncthreads();
  unsigned nv = 0, nz = 0;
  // the entries of the first pass are counted: cold, the pass that sums r^2 for the start; warm, the first pass of the iteration
  auto counts_in = [&]() {
    nv = wave_sum_u32(nv); nz = wave_sum_u32(nz);
    if((tid & 63) == 0) { atomicAdd(&s.cnt[0], nv); atomicAdd(&s.cnt[1], nz); }      // (integers: any order)
  };
  const unsigned CT = (unsigned) (C == 8 || C == 1 ? C : C * j.n_groups);
  double s0 = (double) sigma_prev * (double) sigma_prev;
  if(!have_prev) {
    const double sq = tscale_pass<C, NT, true>(j, s, [](float r) { return tscale_square(r); }, nv, nz);
    counts_in();
    if(tid == 0) s.sum = sq;
    __syncthreads();
    const unsigned long long n_ent = (unsigned long long) CT * s.cnt[0];
    s0 = n_ent ? s.sum / (double) n_ent : 0.0;
  }
  bool exists = have_prev || (tscale_exists((unsigned long long) CT * s.cnt[0], s.cnt[1]) && s0 >= kTScaleFloor * kTScaleFloor);
  if(exists) {
    if(tid == 0) tscale_start(s.fit, s0);
    __syncthreads();
    bool first = have_prev;
    for(;;) {
      const float sf = (float) s.fit.s;
      double sum;
      if(first) { sum = tscale_pass<C, NT, true>(j, s, [sf](float r) { return tscale_term(r, sf); }, nv, nz); counts_in(); }
      else sum = tscale_pass<C, NT, false>(j, s, [sf](float r) { return tscale_term(r, sf); }, nv, nz);
      __syncthreads();      // (the counts have landed; everybody has read s.fit.s)
      if(first) {
        first = false;
        exists = tscale_exists((unsigned long long) CT * s.cnt[0], s.cnt[1]);
        if(!exists) break;      // (uniform over the workgroup)
      }
      if(tid == 0) tscale_step(s.fit, sum, (unsigned long long) CT * s.cnt[0]);      // wave 0 finishes the pass; the others learn through LDS
      __syncthreads();
      if(s.fit.done) break;
    }
  }
  if(tid == 0) {
    const TScaleOut o = exists ? tscale_commit(s.fit, have_prev, sigma_prev) : tscale_commit_none(sigma_prev);
    st->scale = o.scale;
    st->delta_scale = o.delta_scale;
    st->last_median = o.scale;
    st->median_valid = 0;
    j.cnt[9] += exists ? (unsigned long long) s.fit.passes : 0ull;      // measurement: passes of the iteration, and runs of the stage
    j.cnt[11] += 1ull;
  }
}

}  // namespace bpvo_hip
