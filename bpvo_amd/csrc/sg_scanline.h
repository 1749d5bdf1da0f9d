// The scanline walk of the semi-global matchers, once: sgm_path_packed_kernel (kernels_sgm.hip) and sgbm_path_kernel (kernels_sgbm.hip) find
// their line — start, signed stride, length, output volume — and call sg_walk_line; what is sequential in the algorithm lives here.
//   L(p, d) = min(L'(d), L'(d +- 1) + P1, min L' + P2) - (min L' + P2) + C(p, d),   L' = 0 and min L' = 0 ahead of a line's first step,
// in int16 saturating arithmetic.  A lane holds 2 NP consecutive disparities as PAIRS of 16-bit values in 32-bit registers: v_pk_add_i16 /
// v_pk_sub_i16 with clamp and v_pk_min_i16 do two disparities per instruction and the saturation for free (the costs are below 2^15: the
// callers' parameter checks reject windows whose sums are not).  What is sequential is a step's dependent chain — neighbours across lanes,
// the recurrence, the wave minimum that the next step needs — so the chain is kept on the VALU: neighbours by DPP wave shifts, the minimum
// by the DPP row ladder + v_readlane (__shfl compiles to ds_bpermute, an LDS round trip each, eight in a row per step).
// The host part: the dispatch of the two template widths the matchers' launchers choose.
#pragma once
#include <cstddef>
#include <cstdint>
#include <type_traits>

namespace bpvo_hip {

// ---- host: the template widths the launchers choose.
// pairs of disparities per lane of the path kernels (64 lanes x 2 NP disparities >= D), and disparities per lane of the winner-takes-all
// kernels (64 V >= D).  f receives std::integral_constant<int, N>.
template <class F>
static inline void dispatch_path_width(int D, F&& f)
{
  if(D <= 128) f(std::integral_constant<int, 1>());
  else f(std::integral_constant<int, 2>());
}
template <class F>
static inline void dispatch_wta_width(int D, F&& f)
{
  if(D <= 64) f(std::integral_constant<int, 1>());
  else if(D <= 128) f(std::integral_constant<int, 2>());
  else f(std::integral_constant<int, 4>());
}

// ---- device
// steps per batch of the walk (see the loop), and whether the kernels raise the issue priority of their longest lines (s_setprio 3 on the
// rows: the launch lasts as long as its longest chains while every SIMD time-slices four or five lines — the short lines fill the gaps)
#ifndef SG_PF_VALUE
#define SG_PF_VALUE 16
#endif
#ifndef SG_PRIO_VALUE
#define SG_PRIO_VALUE 1
#endif
constexpr int SG_PF = SG_PF_VALUE;

typedef short sg_s16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ sg_s16x2 sg_pk(unsigned u) { return __builtin_bit_cast(sg_s16x2, u); }
__device__ __forceinline__ unsigned sg_bits(sg_s16x2 v) { return __builtin_bit_cast(unsigned, v); }

// One line per wavefront (64 lanes): `n` steps from element `base` of `cost` / `L`, `step_stride` elements apart (signed: a backward path
// starts at the line's last element), D disparities per step, lane l at disparities 2 NP l ...  CostT: a 16-bit type.
template <int NP, class CostT>
__device__ __forceinline__ void sg_walk_line(const CostT* __restrict__ cost, int16_t* __restrict__ L, long long base, long long step_stride, int n, int D,
                                             int P1, int P2)
{
  static_assert(sizeof(CostT) == 2, "16-bit costs");
  constexpr int PF = SG_PF, V = 2 * NP;
  const int lane = threadIdx.x;
  const int d0 = lane * V;
  const bool live = d0 < D;                                    // (D is a multiple of 16 and V divides it: a lane is all in or all out)
  // The cost loads are UNCONDITIONAL — the step clamped to the line's last one, the lanes beyond D reading disparity 0: a load inside a
  // branch makes the compiler wait for it at the end of the branch (s_waitcnt vmcnt(0) right behind every load: the first version of the
  // SGM kernel spent a full memory round trip per step, 1241 of them per row — that, not arithmetic or shuffles, was its 1.1 ms).
  const int d0_load = live ? d0 : 0;
  unsigned prev[NP];
#pragma unroll
  for(int j = 0; j < NP; ++j) prev[j] = 0u;
  int prev_min = 0;
  const sg_s16x2 P1v = {(short) P1, (short) P1};
  using word_t = typename std::conditional<NP == 1, uint32_t, uint64_t>::type;
  // A scanline is walked in BATCHES of PF steps: the PF cost words of a batch are requested back to back, the PF steps run on registers,
  // the PF words of path costs are stored back to back.  Loads and stores share one counter on this hardware and may complete out of
  // order with respect to each other, so the compiler can only wait for "everything" (vmcnt(0)) once both kinds are in flight: a load per
  // step next to a store per step — the software pipeline of the first versions — degenerates into one full memory round trip per STEP
  // (1241 of them per row).  In batches the round trip is paid once per PF steps.  (Requesting the NEXT batch's words before this one's
  // steps run was measured on SGBM: 0.719 against 0.715 ms per 1241 x 376 x 128 frame — no gain, the batch's own loads are consumed with
  // partial waits as they arrive and the chain of dependent steps is what a line costs; that variant is gone.)
  for(int s0 = 0; s0 < n; s0 += PF) {
    word_t cw[PF], ow[PF];
#pragma unroll
    for(int i = 0; i < PF; ++i) cw[i] = *reinterpret_cast<const word_t*>(cost + base + (long long) min(s0 + i, n - 1) * step_stride + d0_load);
#pragma unroll
    for(int i = 0; i < PF; ++i) {
      const word_t cword = cw[i];
      const short pm = (short) (prev_min + P2);
      const sg_s16x2 pmv = {pm, pm};
      // neighbours by DPP wave shifts (a VALU move: ~10 cycles; ds_bpermute, what __shfl compiles to, is an LDS round trip of ~120): lane
      // 0 / lane 63 keep the `old` operand — the sentinel 32767 below disparity 0 / (for D = 64 V) behind the last one
      const unsigned left = (unsigned) __builtin_amdgcn_update_dpp((int) 0x7fff0000u, (int) prev[NP - 1], 0x138 /*wave_shr:1*/, 0xf, 0xf, false);
      const unsigned right = (unsigned) __builtin_amdgcn_update_dpp((int) 0x00007fffu, (int) prev[0], 0x130 /*wave_shl:1*/, 0xf, 0xf, false);
      unsigned cur[NP];
      int mn = 32767;
#pragma unroll
      for(int j = 0; j < NP; ++j) {
        const unsigned below = j > 0 ? prev[j - 1] : left;
        unsigned above = j < NP - 1 ? prev[j + 1] : right;
        if(d0 + 2 * j + 2 >= D) above = 0x7fffu;              // the sentinel behind the last disparity
        const sg_s16x2 lm = sg_pk((below >> 16) | (prev[j] << 16));      // (d - 1) of both halves
        const sg_s16x2 lp = sg_pk((prev[j] >> 16) | (above << 16));      // (d + 1) of both halves
        const sg_s16x2 c = sg_pk((unsigned) (cword >> (32 * j)));
        sg_s16x2 a = __builtin_elementwise_min(sg_pk(prev[j]), __builtin_elementwise_add_sat(lm, P1v));
        a = __builtin_elementwise_min(a, __builtin_elementwise_add_sat(lp, P1v));
        a = __builtin_elementwise_min(a, pmv);
        a = __builtin_elementwise_add_sat(__builtin_elementwise_sub_sat(a, pmv), c);
        cur[j] = sg_bits(a);
        if(live) mn = min(mn, min((int) a.x, (int) a.y));
      }
      // wave minimum by the DPP ladder (row shifts inside the rows of 16 lanes, then the two row broadcasts): lane 63 ends up with it
      mn = min(mn, __builtin_amdgcn_update_dpp(mn, mn, 0x111 /*row_shr:1*/, 0xf, 0xf, false));
      mn = min(mn, __builtin_amdgcn_update_dpp(mn, mn, 0x112 /*row_shr:2*/, 0xf, 0xf, false));
      mn = min(mn, __builtin_amdgcn_update_dpp(mn, mn, 0x114 /*row_shr:4*/, 0xf, 0xf, false));
      mn = min(mn, __builtin_amdgcn_update_dpp(mn, mn, 0x118 /*row_shr:8*/, 0xf, 0xf, false));
      mn = min(mn, __builtin_amdgcn_update_dpp(mn, mn, 0x142 /*row_bcast:15*/, 0xa, 0xf, false));
      mn = min(mn, __builtin_amdgcn_update_dpp(mn, mn, 0x143 /*row_bcast:31*/, 0xc, 0xf, false));
      word_t out = 0;
#pragma unroll
      for(int j = 0; j < NP; ++j) out |= (word_t) cur[j] << (32 * j);
      ow[i] = out;
      // (steps past the end of the line — the last batch of a ragged line — leave the state alone: nothing follows them)
      if(s0 + i < n) {
        prev_min = __builtin_amdgcn_readlane(mn, 63);
#pragma unroll
        for(int j = 0; j < NP; ++j) prev[j] = cur[j];
      }
    }
    if(live) {
#pragma unroll
      for(int i = 0; i < PF; ++i)
        if(s0 + i < n) *reinterpret_cast<word_t*>(L + base + (long long) (s0 + i) * step_stride + d0) = ow[i];
    }
  }
}

}  // namespace bpvo_hip
