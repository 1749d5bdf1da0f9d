// libbpvo_hip, device side: the measurement variance — per pixel, the variance of a measured disparity from the matching cost of the rectified
// pair around it.  disparity_variance_math.h states the rule; disparity_variance.hip fills the job table.
#include "kernels.h"
#include "disparity_variance_math.h"

namespace bpvo_hip {

// One launch for all the pairs of a call: job blockIdx.y is the row of the table (uniform: scalar loads), the grid covers the tiles of the
// largest frame, and the workgroups beyond their own frame leave at once (before any barrier).  A workgroup of 256 lanes takes a tile of
// kTileW x kTileH pixels, a lane one pixel; a wavefront is two rows of 32.
//   1. every lane decides steps 1 - 3 of the rule for its pixel (dv_locate); the lanes that go on put the columns their right windows span
//      into a workgroup minimum / maximum (LDS integer atomics).  A tile in which no lane goes on writes max2 and leaves ("idle").
//   2. the left tile plus its halo of rho goes to LDS, and the right strip — the rows of the tile plus halo, the columns min .. max — too,
//      if it is at most kStripW wide ("staged": a smooth map's tile spans 32 + 2 rho + 2 columns plus the spread of d0 in it).  A tile whose
//      disparities spread further reads the right image where it lies ("direct").  Only pixels of the images are read: the windows of a
//      lane that goes on lie inside both images (dv_locate), so the rectangle of the tile's windows clipped to the image holds them all, and
//      the bytes of LDS that stay unwritten are never read.
//   3. the three sums in one walk over the window: per row the right window slides by one pixel per step, so a step reads ONE new right byte
//      and one left byte for three squared differences.  The sums are integers: both paths give the same numbers whatever the order.
//   4. dv_finish, the store, and the class counts: a ballot per class into wave-uniform counts, the four wavefronts' counts summed in LDS, one
//      integer atomic per workgroup and class that occurred, and one for the tile's path.
// LDS layout (u8): the left tile's rows are kLeftPitch = 48 bytes apart and the strip's kStripPitch = 164 — 12 and 41 dwords, so the two rows
// of a wavefront (32 consecutive bytes each, 8 or 9 dwords; lanes that share a dword are one broadcast) fall into disjoint banks: pitches of
// 32 or 64 dwords would put both rows on the same banks.  4.6 KiB per workgroup.
constexpr int kTileW = 32, kTileH = 8;
constexpr int kHaloH = kTileH + 2 * kDvMaxRadius;                 // 22 rows
constexpr int kLeftPitch = 48;                                    // >= kTileW + 2 * 7 = 46
constexpr int kStripW = 160, kStripPitch = 164;
enum { DV_TILE_STAGED = 0, DV_TILE_DIRECT = 1, DV_TILE_IDLE = 2 };
static_assert(kTileW * kTileH == 256 && kLeftPitch >= kTileW + 2 * kDvMaxRadius && kStripPitch >= kStripW, "tile layout");

// the three sums of one pixel: lp at the left window's first byte, rp at the byte LEFT of the k = +1 window's first (so the walk's first two
// bytes prime it), rows lpitch / rpitch apart.  Inlined at both call sites: the staged walk compiles to LDS reads only.
static __device__ __forceinline__ void variance_sums(const uint8_t* lp, int lpitch, const uint8_t* rp, int rpitch, int rho, int* s_m1, int* s_0, int* s_p1)
{
  int a = 0, b = 0, c = 0;
  const int w = 2 * rho + 1;
  for(int j = 0; j < w; ++j) {
    int rm = (int) rp[0], r0 = (int) rp[1];      // columns x - rho - d0 - 1 and x - rho - d0
    for(int i = 0; i < w; ++i) {
      const int rn = (int) rp[i + 2];
      const int l = (int) lp[i];
      a += (l - rn) * (l - rn);      // k = -1
      b += (l - r0) * (l - r0);      // k =  0
      c += (l - rm) * (l - rm);      // k = +1
      rm = r0; r0 = rn;
    }
    lp += lpitch; rp += rpitch;
  }
  *s_m1 = a; *s_0 = b; *s_p1 = c;
}

__global__ __launch_bounds__(256) void disparity_variance_kernel(const VarianceJob* __restrict__ jobs)
{
  __shared__ uint8_t left[kHaloH * kLeftPitch];
  __shared__ uint8_t strip[kHaloH * kStripPitch];
  __shared__ int span[2];
  __shared__ unsigned block_counts[DV_CLASSES];
  const VarianceJob& j = jobs[blockIdx.y];
  const int rows = j.rows, cols = j.cols, rho = j.radius;
  const int tiles_x = (cols + kTileW - 1) / kTileW;
  const int ty = (int) blockIdx.x / tiles_x, tx = (int) blockIdx.x - ty * tiles_x;
  if(ty * kTileH >= rows) return;      // (the whole workgroup: no barrier has been passed)
  const int x0 = tx * kTileW, y0 = ty * kTileH;
  const int lx = threadIdx.x & (kTileW - 1), ly = threadIdx.x / kTileW;
  const int x = x0 + lx, y = y0 + ly;
  const bool in = x < cols && y < rows;
  const size_t pix = (size_t) y * (size_t) cols + (size_t) x;
  if(threadIdx.x < DV_CLASSES) block_counts[threadIdx.x] = 0;
  if(threadIdx.x == 0) { span[0] = 0x7FFFFFFF; span[1] = -1; }
  __syncthreads();

  const DvRule rule{rho, j.noise2, j.min2, j.max2};
  int d0 = 0;
  int cls = in ? dv_locate(j.M[pix], j.lo, j.hi, x, y, rows, cols, rho, &d0) : DV_CLASSES;      // (DV_CLASSES: no pixel)
  const bool go = cls < 0;
  const int first = x - rho - d0 - 1;      // the columns the right windows span: first .. first + 2 rho + 2, inside the image where go
  if(go) {
    atomicMin(&span[0], first);
    atomicMax(&span[1], first + 2 * rho + 2);
  }
  __syncthreads();
  const int c_lo = span[0], c_hi = span[1];
  const int path = c_hi < 0 ? DV_TILE_IDLE : (c_hi - c_lo + 1 <= kStripW ? DV_TILE_STAGED : DV_TILE_DIRECT);      // (uniform over the workgroup)
  float r2 = j.max2;
  if(path != DV_TILE_IDLE) {
    // the rectangle of the tile's windows, clipped to the image: rows ya .. yb; the left columns xa .. xb; the strip's c_lo .. c_hi
    const int ya = max(y0 - rho, 0), yb = min(y0 + kTileH - 1 + rho, rows - 1);
    const int xa = max(x0 - rho, 0), xb = min(x0 + kTileW - 1 + rho, cols - 1);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for(int yy = ya + wave; yy <= yb; yy += 4) {
      const uint8_t* src = j.L + (size_t) yy * (size_t) cols;
      uint8_t* dst = left + (yy - (y0 - rho)) * kLeftPitch;
      for(int xx = xa + lane; xx <= xb; xx += 64) dst[xx - (x0 - rho)] = src[xx];
      if(path == DV_TILE_STAGED) {
        const uint8_t* rsrc = j.R + (size_t) yy * (size_t) cols;
        uint8_t* rdst = strip + (yy - (y0 - rho)) * kStripPitch;
        for(int xx = c_lo + lane; xx <= c_hi; xx += 64) rdst[xx - c_lo] = rsrc[xx];
      }
    }
    __syncthreads();
    if(go) {
      int s_m1, s_0, s_p1;
      const uint8_t* lp = left + ly * kLeftPitch + lx;      // (row y - rho, column x - rho of the image)
      if(path == DV_TILE_STAGED) variance_sums(lp, kLeftPitch, strip + ly * kStripPitch + (first - c_lo), kStripPitch, rho, &s_m1, &s_0, &s_p1);
      else variance_sums(lp, kLeftPitch, j.R + (size_t) (y - rho) * (size_t) cols + (size_t) first, cols, rho, &s_m1, &s_0, &s_p1);
      cls = dv_finish(rule, s_m1, s_0, s_p1, &r2);
    }
  }
  if(in) j.out[pix] = r2;
  unsigned counts[DV_CLASSES];
#pragma unroll
  for(int k = 0; k < DV_CLASSES; ++k) counts[k] = (unsigned) __popcll(__ballot(cls == k));
  if((threadIdx.x & 63) == 0) {
#pragma unroll
    for(int k = 0; k < DV_CLASSES; ++k)
      if(counts[k]) atomicAdd(&block_counts[k], counts[k]);
  }
  __syncthreads();
  if(threadIdx.x < DV_CLASSES && block_counts[threadIdx.x]) atomicAdd(j.counts + threadIdx.x, block_counts[threadIdx.x]);
  if(threadIdx.x == 64) atomicAdd(j.counts + DV_CLASSES + path, 1u);
}

void launch_disparity_variance(hipStream_t s, const VarianceJob* jobs, int njobs, int max_tiles)
{
  hipLaunchKernelGGL(disparity_variance_kernel, dim3((unsigned) max_tiles, (unsigned) njobs), dim3(256), 0, s, jobs);
}
int disparity_variance_tiles(int rows, int cols)
{
  return ((cols + kTileW - 1) / kTileW) * ((rows + kTileH - 1) / kTileH);
}

}  // namespace bpvo_hip
