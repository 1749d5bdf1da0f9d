// Pose scoring (gfx950; c_api.h bpvo_hip_score_poses states the definition): the truncated-L1 cost of MANY poses of a pair in one launch.
//   score_poses   one workgroup = one 256-point chunk of one pair x a tile of poses.  The tile's 3x4 projection matrices sit in LDS; a thread loads
//                 its template point and its C template values ONCE and walks the tile's poses: projection and validity (warp_rule.h), the
//                 bilinear gather of the current frame's descriptor, the residuals — the statements of warp_residual (gn_warp.h), so valid
//                 flags and residuals are that kernel's, bit for bit — then min(|r|, tau) summed in f64 per thread (channel order), over the
//                 wavefront (shuffle tree) and over the four waves (wave order).  One partial {cost, valid points, terms below tau} per
//                 (pose, chunk); no atomics, so a partial depends on nothing but its pose and its chunk.
//   score_finish  one thread per (pair, pose): the partials summed in chunk order, the score (pose_score_math.h), the record.
// Reads the template (ptc, pix), the descriptor and the job's geometry only: no workspace, no tap cache, no counter, no GNState.
// kLinear interpolation; the three warp formulations; every channel count of dispatch_channels (one channel group: C <= 48).
#include "kernels.h"

#include "gn_common.h"
#include "gn_warp.h"
#include "pose_score_math.h"

namespace bpvo_hip {

static_assert(sizeof(ScorePartial) == 16, "one 16-byte store per (pose, chunk)");
static_assert(sizeof(bpvo_hip_pose_score) == 24, "bpvo_hip_pose_score is 24 bytes (c_api.h)");

template <int C, bool FAST>
__global__ __launch_bounds__(K6_BLOCK) void score_poses_kernel(const PairJob* __restrict__ jobs, const float* __restrict__ T, int n_poses, int tile,
                                                               float tau, int max_chunks, ScorePartial* __restrict__ partials)
{
  const PairJob& j = jobs[blockIdx.z];
  const int n = j.n;
  const unsigned chunk = blockIdx.x;
  if((int) (chunk * K6_BLOCK) >= n) return;      // (the grid is sized by the largest template of the launch)
  const int pose0 = (int) blockIdx.y * tile;
  const int np = min(tile, n_poses - pose0);

  __shared__ float s_P[kScoreTile][12];
  __shared__ double s_cost[kScoreTile][K6_WAVES];
  __shared__ unsigned s_cnt[kScoreTile][K6_WAVES];
  if((int) threadIdx.x < np) {
    const float* Tp = T + ((size_t) blockIdx.z * n_poses + pose0 + threadIdx.x) * 16;
    float P[12];
    if(FAST && j.dspace) dspace_matrix(j, Tp, P);
    else projection_matrix(j, Tp, P);
#pragma unroll
    for(int k = 0; k < 12; ++k) s_P[threadIdx.x][k] = P[k];
  }
  __syncthreads();

  // lanes past the end of the last chunk redo the last point (loads only) and count for nothing
  const int i_raw = chunk * K6_BLOCK + threadIdx.x;
  const bool in_block = i_raw < n;
  const int i = in_block ? i_raw : n - 1;
  const int W = j.cols, R = j.rows;
  const int PT = (C == 8 || C == 1) ? C : j.pitch;
  // the point and its template values: once for the whole tile (plain loads: the next pose tile's workgroup reads the same lines)
  const float4 X = load_point<false>(j, i);
  float4 px0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), px1 = px0;
  float I0[C];
  if constexpr(C == 8) {
    const float4* p0 = reinterpret_cast<const float4*>(j.pix.get());
    px0 = p0[tile_index<2>(i, 0)]; px1 = p0[tile_index<2>(i, 1)];
  } else {
#pragma unroll
    for(int c = 0; c < C; ++c) I0[c] = j.pix[(size_t) i * PT + c];
  }

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for(int p = 0; p < np; ++p) {
    float P[12];
#pragma unroll
    for(int k = 0; k < 12; ++k) P[k] = s_P[p][k];
    int xi = 0, yi = 0;
    bool valid;
    double xf = 0.0, yf = 0.0;
    float cf[4] = {0, 0, 0, 0};
    if constexpr(!FAST) {
      const WarpFoot f = warp_foot(P, X.x, X.y, X.z, X.w, W, R);
      xi = f.xi; yi = f.yi; valid = f.valid; xf = f.xf; yf = f.yf;
    } else {
      const WarpFootF32 f = warp_foot_f32(P, X.x, X.y, X.z, X.w, j.dspace != 0, j.K[2], j.K[5], W, R);
      xi = f.xi; yi = f.yi; valid = f.valid;
#pragma unroll
      for(int k = 0; k < 4; ++k) cf[k] = f.cf[k];
    }
    valid = valid && in_block;

    double cost = 0.0;
    unsigned below = 0;
    auto add = [&](float r) {      // one term: min(|r|, tau) as f32, summed in f64
      const float a = fabsf(r);
      below += a < tau ? 1u : 0u;
      cost += (double) (a < tau ? a : tau);
    };
    if(valid) {
      if constexpr(C == 8) {
        float4 t[8];
        taps8_gather(j, xi, yi, W, t);
        float res[8];
        if constexpr(!FAST) {
          taps8_residuals(t, px0, px1, xf, yf, res);
        } else {
          float i00[8], i01[8], i10[8], i11[8], i0[8];
          taps8_unpack(t, px0, px1, i00, i01, i10, i11, i0);
#pragma unroll
          for(int c = 0; c < 8; ++c) res[c] = bilinear_res_f32(i00[c], i01[c], i10[c], i11[c], i0[c], cf);
        }
#pragma unroll
        for(int c = 0; c < 8; ++c) add(res[c]);
      } else {
        const double wx = 1.0 - xf, wy = 1.0 - yf;
        const float* __restrict__ d0 = j.desc + ((size_t) yi * W + xi) * PT;
        const float* __restrict__ d1 = d0 + (size_t) W * PT;
#pragma unroll
        for(int c = 0; c < C; ++c) {      // channel by channel: the four taps of a channel live only as long as its residual
          if constexpr(!FAST) add(bilinear_res(d0[c], d0[PT + c], d1[c], d1[PT + c], I0[c], xf, yf, wx, wy));
          else add(bilinear_res_f32(d0[c], d0[PT + c], d1[c], d1[PT + c], I0[c], cf));
        }
      }
    }
    // over the wavefront: the counts (integers, any order) and the cost with the fixed pairing of a shuffle tree
    const unsigned cnt = wave_sum_u32((valid ? 1u : 0u) | (below << 16));      // (<= 64 points, <= 64 * 48 terms a wave)
#pragma unroll
    for(int o = 32; o >= 1; o >>= 1) cost += __shfl_down(cost, o);
    if(lane == 0) { s_cost[p][wave] = cost; s_cnt[p][wave] = cnt; }
  }
  __syncthreads();
  if((int) threadIdx.x < np) {      // over the waves, in wave order (<= 256 points, <= 256 * 48 terms a chunk: 16 bits each)
    double s = s_cost[threadIdx.x][0];
    unsigned cnt = s_cnt[threadIdx.x][0];
#pragma unroll
    for(int w = 1; w < K6_WAVES; ++w) { s += s_cost[threadIdx.x][w]; cnt += s_cnt[threadIdx.x][w]; }
    ScorePartial q;
    q.cost = s; q.n_valid = (int) (cnt & 0xffffu); q.n_below = (int) (cnt >> 16);
    partials[((size_t) blockIdx.z * max_chunks + chunk) * n_poses + pose0 + threadIdx.x] = q;
  }
}

__global__ __launch_bounds__(GN_BLOCK) void score_finish_kernel(const PairJob* __restrict__ jobs, int n_pairs, int n_poses, int C, float tau, int max_chunks,
                                                                const ScorePartial* __restrict__ partials, bpvo_hip_pose_score* __restrict__ out)
{
  const size_t idx = (size_t) blockIdx.x * GN_BLOCK + threadIdx.x;
  if(idx >= (size_t) n_pairs * n_poses) return;
  const int pair = (int) (idx / (size_t) n_poses), pose = (int) (idx % (size_t) n_poses);
  const int n = jobs[pair].n;
  const int chunks = (n + K6_BLOCK - 1) / K6_BLOCK;
  const ScorePartial* q = partials + (size_t) pair * max_chunks * n_poses + pose;      // (consecutive threads: consecutive poses of a chunk)
  double cost = 0.0;
  int n_valid = 0, n_below = 0;
#pragma unroll 8
  for(int k = 0; k < chunks; ++k) {
    const ScorePartial v = q[(size_t) k * n_poses];
    cost += v.cost; n_valid += v.n_valid; n_below += v.n_below;
  }
  bpvo_hip_pose_score r;
  r.cost_sum = cost;
  r.score = pose_score_value(cost, n_valid, n, C, tau);
  r.n_valid = n_valid; r.n_below = n_below;
  out[idx] = r;
}

int score_chunks(int max_points) { return std::max(1, (max_points + K6_BLOCK - 1) / K6_BLOCK); }

void launch_score_poses(hipStream_t s, const ScoreLaunch& g)
{
  const int tile = std::max(1, std::min(g.tile, kScoreTile));
  const int max_chunks = score_chunks(g.max_points);
  const dim3 grid(max_chunks, (g.n_poses + tile - 1) / tile, g.n_pairs);
  if(g.max_points > 0) {
    dispatch_channels(g.C, [&](auto c) {
      constexpr int CC = decltype(c)::value;
      if(g.fast_warp) hipLaunchKernelGGL((score_poses_kernel<CC, true>), grid, dim3(K6_BLOCK), 0, s, g.jobs, g.T, g.n_poses, tile, g.tau, max_chunks, g.partials);
      else hipLaunchKernelGGL((score_poses_kernel<CC, false>), grid, dim3(K6_BLOCK), 0, s, g.jobs, g.T, g.n_poses, tile, g.tau, max_chunks, g.partials);
    });
  }
  const size_t records = (size_t) g.n_pairs * g.n_poses;
  hipLaunchKernelGGL(score_finish_kernel, dim3((unsigned) ((records + GN_BLOCK - 1) / GN_BLOCK)), dim3(GN_BLOCK), 0, s, g.jobs, g.n_pairs, g.n_poses, g.C, g.tau,
                     max_chunks, g.partials, g.out);
}

}  // namespace bpvo_hip
