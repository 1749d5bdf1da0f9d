// libbpvo_hip, device side: motion stereo — per pixel, the prior disparity refined by a short search along the pixel's epipolar line in a second
// image of the same camera.  motion_stereo_math.h states the rule; motion_stereo.hip fills the job table.
#include "kernels.h"
#include "motion_stereo_math.h"

namespace bpvo_hip {

// One launch for all the pairs of a call: job blockIdx.y is the row of the table (uniform: scalar loads, the f64 geometry of the pair stays in
// scalar registers), the grid covers the tiles of the largest frame, and the workgroups beyond their own frame leave at once (before any
// barrier).  A workgroup of 256 lanes takes a tile of kTileW x kTileH pixels, a lane one pixel; a wavefront is two rows of 32.
//   1. every lane decides steps 1 - 3 of the rule for its pixel (ms_locate, then ms_hypothesis for j = -J .. J); the lanes that go on put the
//      columns and rows their K taps span into a workgroup bounding box (LDS integer atomics).  A tile in which no lane goes on is "idle".
//   2. the C tile plus its halo of rho goes to LDS, and the K box too if it is at most kBoxW x kBoxH ("staged": a tile under a small motion
//      spans the tile plus 2 rho + 2 plus the 2 J + 1 pixels of the search plus the spread of the priors).  A tile whose samples spread further —
//      a large rotation about the optical axis, a prior map with jumps — reads K where it lies ("direct").  Only pixels of the images are read:
//      the taps of a lane that goes on lie inside K (ms_hypothesis), so their bounding box does, and the bytes of LDS that stay unwritten are
//      never read.
//   3. the sums, one hypothesis after the other: ms_hypothesis again (two f64 divisions per hypothesis, about as many instructions as the window
//      walk of radius 1; keeping 2 (2 J + 1) quantised centres per lane instead would need indexed registers, that is scratch), then the window
//      walk, unrolled for the radius: a row of 2 rho + 2 K bytes gives the 2 rho + 1 horizontal interpolations, two consecutive rows the
//      samples — (2 rho + 2)^2 K bytes and (2 rho + 1)^2 C bytes per hypothesis.  The sums are integers: both paths give the same numbers.
//   4. ms_finish, the stores, and the class counts: a ballot per class into wave-uniform counts, the four wavefronts' counts summed in LDS, one
//      integer atomic per workgroup and class that occurred, and one for the tile's path.
// LDS layout (u8): byte reads bank by dword within each 32-lane half, and a half of a wavefront is one row of the tile: its 32 lanes read 32
// consecutive bytes of C (8 or 9 dwords, lanes that share a dword are one broadcast), so any pitch is conflict-free for C; kCPitch = 48 (12
// dwords).  The K reads of a half follow the motion; under a small one they are consecutive too.  kBoxPitch = 100 (25 dwords, odd: the rows a
// rotated half touches fall on different banks).  14 x 48 + 48 x 100 bytes = 5.4 KiB per workgroup.
// The tile is 32 x 8 and not larger: the f64 curve of a lane (h, delta, the prior, the running minimum) is live across the whole search, about
// 24 VGPRs beside the walk's rows, and the f64 divisions are long dependent chains that need other wavefronts to hide behind — 256 lanes with
// a few KiB of LDS leave the occupancy to the registers.
constexpr int kTileW = 32, kTileH = 8;
constexpr int kCRows = kTileH + 2 * kMsMaxRadius;                 // 14 rows
constexpr int kCPitch = 48;                                       // >= kTileW + 2 * 3 = 38
constexpr int kBoxW = 96, kBoxH = 48, kBoxPitch = 100;
enum { MS_TILE_STAGED = 0, MS_TILE_DIRECT = 1, MS_TILE_IDLE = 2 };
static_assert(kTileW * kTileH == 256 && kCPitch >= kTileW + 2 * kMsMaxRadius && kBoxPitch >= kBoxW, "tile layout");

// the sum of one hypothesis: cp at the C window's first byte, kp at the first tap of the window's first sample, rows cpitch / kpitch apart
template <int RHO>
static __device__ __forceinline__ int window_sum(const uint8_t* cp, int cpitch, const uint8_t* kp, int kpitch, int fx, int fy)
{
  constexpr int W = 2 * RHO + 1;
  int top[W], s = 0;
  {
    int p = (int) kp[0];
#pragma unroll
    for(int i = 0; i < W; ++i) {
      const int q = (int) kp[i + 1];
      top[i] = (32 - fx) * p + fx * q;
      p = q;
    }
  }
#pragma unroll
  for(int r = 0; r < W; ++r) {
    kp += kpitch;
    int p = (int) kp[0];
#pragma unroll
    for(int i = 0; i < W; ++i) {
      const int q = (int) kp[i + 1];
      const int bot = (32 - fx) * p + fx * q;
      const int k = ((32 - fy) * top[i] + fy * bot + 512) >> 10;      // (ms_tap, the horizontal halves shared between neighbours)
      const int c = (int) cp[i];
      s += (c - k) * (c - k);
      top[i] = bot;
      p = q;
    }
    cp += cpitch;
  }
  return s;
}
static __device__ __forceinline__ int window_sum_of(int rho, const uint8_t* cp, int cpitch, const uint8_t* kp, int kpitch, int fx, int fy)
{
  if(rho == 1) return window_sum<1>(cp, cpitch, kp, kpitch, fx, fy);
  if(rho == 2) return window_sum<2>(cp, cpitch, kp, kpitch, fx, fy);
  return window_sum<3>(cp, cpitch, kp, kpitch, fx, fy);
}

__global__ __launch_bounds__(256) void motion_stereo_kernel(const MotionStereoJob* __restrict__ jobs)
{
  __shared__ uint8_t ctile[kCRows * kCPitch];
  __shared__ uint8_t kbox[kBoxH * kBoxPitch];
  __shared__ int box[4];
  __shared__ unsigned block_counts[MS_CLASSES];
  const MotionStereoJob& j = jobs[blockIdx.y];
  const int rows = j.rows, cols = j.cols, rho = j.radius, J = j.steps;
  const int tiles_x = (cols + kTileW - 1) / kTileW;
  const int ty = (int) blockIdx.x / tiles_x, tx = (int) blockIdx.x - ty * tiles_x;
  if(ty * kTileH >= rows) return;      // (the whole workgroup: no barrier has been passed)
  const int x0 = tx * kTileW, y0 = ty * kTileH;
  const int lx = threadIdx.x & (kTileW - 1), ly = threadIdx.x / kTileW;
  const int x = x0 + lx, y = y0 + ly;
  const bool in = x < cols && y < rows;
  const size_t pix = (size_t) y * (size_t) cols + (size_t) x;
  if(threadIdx.x < MS_CLASSES) block_counts[threadIdx.x] = 0;
  if(threadIdx.x == 0) { box[0] = 0x7FFFFFFF; box[1] = -1; box[2] = 0x7FFFFFFF; box[3] = -1; }
  __syncthreads();

  const MsRule rule{rho, J, j.min_gain, j.noise2, j.min2, j.max2, j.gate};
  MsGeometry geo;
  geo.fx = j.fx; geo.fy = j.fy; geo.cx = j.cx; geo.cy = j.cy;
#pragma unroll
  for(int k = 0; k < 9; ++k) geo.R[k] = j.R[k];
#pragma unroll
  for(int k = 0; k < 3; ++k) geo.e[k] = j.e[k];

  // the prior: the z-buffer word of the pixel (0: none), or the caller's two maps
  bool has = false;
  float pd = 0.0f, pv = -1.0f;
  if(in) {
    if(j.zbuf) {
      const unsigned long long word = j.zbuf[pix];
      has = word != 0;
      pd = df_float((uint32_t) (word >> 32));
      pv = df_float((uint32_t) word);
    } else {
      has = true;
      pd = j.pd[pix];
      pv = j.pv[pix];
    }
  }
  MsLine line;
  line.h[0] = line.h[1] = line.h[2] = 0.0; line.delta = 0.0;
  int cls = in ? ms_locate(rule, geo, j.lo, j.hi, x, y, has, pd, pv, &line) : MS_CLASSES;      // (MS_CLASSES: no pixel)
  if(cls < 0) {
    int ix_lo = 0x7FFFFFFF, ix_hi = -1, iy_lo = 0x7FFFFFFF, iy_hi = -1;
    for(int h = -J; h <= J; ++h) {
      int32_t xq, yq;
      if(!ms_hypothesis(rule, geo, line, pd, h, x, y, rows, cols, &xq, &yq)) { cls = MS_BORDER; break; }
      ix_lo = min(ix_lo, xq >> 5); ix_hi = max(ix_hi, xq >> 5);
      iy_lo = min(iy_lo, yq >> 5); iy_hi = max(iy_hi, yq >> 5);
    }
    if(cls < 0) {      // the taps of all the samples: columns ix - rho .. ix + rho + 1, inside K
      atomicMin(&box[0], ix_lo - rho);
      atomicMax(&box[1], ix_hi + rho + 1);
      atomicMin(&box[2], iy_lo - rho);
      atomicMax(&box[3], iy_hi + rho + 1);
    }
  }
  const bool go = cls < 0;
  __syncthreads();
  const int bx0 = box[0], bx1 = box[1], by0 = box[2], by1 = box[3];
  const int path = bx1 < 0 ? MS_TILE_IDLE : (bx1 - bx0 + 1 <= kBoxW && by1 - by0 + 1 <= kBoxH ? MS_TILE_STAGED : MS_TILE_DIRECT);      // (uniform over the workgroup)
  float D = pd, V = pv;
  if(path != MS_TILE_IDLE) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    {      // the rectangle of the tile's C windows, clipped to the image
      const int ya = max(y0 - rho, 0), yb = min(y0 + kTileH - 1 + rho, rows - 1);
      const int xa = max(x0 - rho, 0), xb = min(x0 + kTileW - 1 + rho, cols - 1);
      for(int yy = ya + wave; yy <= yb; yy += 4) {
        const uint8_t* src = j.C + (size_t) yy * (size_t) cols;
        uint8_t* dst = ctile + (yy - (y0 - rho)) * kCPitch;
        for(int xx = xa + lane; xx <= xb; xx += 64) dst[xx - (x0 - rho)] = src[xx];
      }
    }
    if(path == MS_TILE_STAGED) {
      for(int yy = by0 + wave; yy <= by1; yy += 4) {
        const uint8_t* src = j.K + (size_t) yy * (size_t) cols;
        uint8_t* dst = kbox + (yy - by0) * kBoxPitch;
        for(int xx = bx0 + lane; xx <= bx1; xx += 64) dst[xx - bx0] = src[xx];
      }
    }
    __syncthreads();
    if(go) {
      const uint8_t* cp = ctile + ly * kCPitch + lx;      // (row y - rho, column x - rho of the image)
      MsMin m;
      ms_min_start(&m);
      for(int h = -J; h <= J; ++h) {
        int32_t xq = 0, yq = 0;
        (void) ms_hypothesis(rule, geo, line, pd, h, x, y, rows, cols, &xq, &yq);      // (true: step 1 has seen it)
        const int ix = (xq >> 5) - rho, iy = (yq >> 5) - rho;
        int s;
        if(path == MS_TILE_STAGED) s = window_sum_of(rho, cp, kCPitch, kbox + (iy - by0) * kBoxPitch + (ix - bx0), kBoxPitch, xq & 31, yq & 31);
        else s = window_sum_of(rho, cp, kCPitch, j.K + (size_t) iy * (size_t) cols + (size_t) ix, cols, xq & 31, yq & 31);
        ms_min_push(&m, h, s);
      }
      cls = ms_finish(rule, j.lo, j.hi, line, pd, pv, m, &D, &V);
    }
  }
  if(in) {
    if(j.zbuf) {
      if(cls == MS_FUSED) j.zbuf[pix] = (unsigned long long) df_key(D, V);      // (every other class keeps the word, 0 included)
    } else {
      if(j.out_d) j.out_d[pix] = D;
      if(j.out_v) j.out_v[pix] = V;
    }
    if(j.out_c) j.out_c[pix] = (uint8_t) cls;
  }
  unsigned counts[MS_CLASSES];
#pragma unroll
  for(int k = 0; k < MS_CLASSES; ++k) counts[k] = (unsigned) __popcll(__ballot(cls == k));
  if((threadIdx.x & 63) == 0) {
#pragma unroll
    for(int k = 0; k < MS_CLASSES; ++k)
      if(counts[k]) atomicAdd(&block_counts[k], counts[k]);
  }
  __syncthreads();
  if(threadIdx.x < MS_CLASSES && block_counts[threadIdx.x]) atomicAdd(j.counts + threadIdx.x, block_counts[threadIdx.x]);
  if(threadIdx.x == 64) atomicAdd(j.counts + MS_CLASSES + path, 1u);
}

void launch_motion_stereo(hipStream_t s, const MotionStereoJob* jobs, int njobs, int max_tiles)
{
  hipLaunchKernelGGL(motion_stereo_kernel, dim3((unsigned) max_tiles, (unsigned) njobs), dim3(256), 0, s, jobs);
}
int motion_stereo_tiles(int rows, int cols)
{
  return ((cols + kTileW - 1) / kTileW) * ((rows + kTileH - 1) / kTileH);
}

}  // namespace bpvo_hip
