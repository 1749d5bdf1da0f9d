// Normalised intensity (gfx950): the descriptor plane of an Intensity context under bpvo_hip_set_intensity_normalization — the rule of
// include/bpvo_hip/c_api.h, stated as code in intensity_norm_math.h — written where intensity_kernel writes float(I).  All kernels are batched
// over frames and levels like intensity_kernel (kernels_frame.hip level_job): z = level x nframes + frame, the grid sized for the finest level
// of the launch, the workgroups outside a coarser level's own grid leave at once.  Rows and columns are the job's own (FrameJob::rows / cols).
// Both forms move 1 B in and 4 B out per pixel.
#include "frame_common.h"
#include "intensity_norm_math.h"

namespace bpvo_hip {

__device__ __forceinline__ const FrameJob& inorm_level_job(const FrameJob* jobs, unsigned z, int nframes, int job_pitch)
{
  const unsigned lvl = z / (unsigned) nframes;
  return jobs[(size_t) lvl * job_pitch + (size_t) (z - lvl * (unsigned) nframes)];
}

// ---- radius 0, whole image, first launch: the 256-bin histogram of every (frame, level), and from it the 256-entry table.
// At most max_tiles workgroups share a (frame, level) — INORM_HIST_TILES for a few frames, fewer as the launch holds more (inorm_hist_max_tiles:
// about a workgroup per CU in all; measured, the launch's time follows the number of workgroups that flush and draw tickets, 12.8 k of them over 64
// frames of 640x480 took 1.09 ms, 2.9 k 0.31 ms) —: each walks its share of the image in 8-byte words (four loads in flight), counts
// into one LDS histogram per wave (a constant image has every lane on one bin: four waves on four counters instead of one) and adds its
// non-empty bins to the (frame, level)'s bins in memory with integer atomics — the bins, and so the table, are the same bits whatever shares
// the launch and in whatever order the workgroups arrive; few workgroups per image, because the adds of all of them meet on the same 1 KB.
// Then it draws a ticket; the workgroup that draws the LAST one of its (frame, level) takes the bins — clearing them and the ticket for the
// next stage on this slot: no memset launch —, scans them, finds median and MAD (the rule of inorm_median_mad, a bin per thread) and writes the
// table.  The apply launch follows in stream order and reads only the table.
constexpr int INORM_HIST_PX = 2048;      // pixels a workgroup takes at least (a smaller image: fewer workgroups)
constexpr int INORM_HIST_TILES = 16;
__host__ __device__ inline int inorm_hist_tiles(int n, int max_tiles) { const int t = (n + INORM_HIST_PX - 1) / INORM_HIST_PX; return t < max_tiles ? t : max_tiles; }
static inline int inorm_hist_max_tiles(int nz) { return std::max(2, std::min(INORM_HIST_TILES, 256 / std::max(nz, 1))); }
__device__ __forceinline__ void inorm_count8(uint32_t* h, uint2 v)
{
#pragma unroll
  for(int k = 0; k < 4; ++k) {
    atomicAdd(&h[(v.x >> (8 * k)) & 255u], 1u);
    atomicAdd(&h[(v.y >> (8 * k)) & 255u], 1u);
  }
}
__global__ __launch_bounds__(256) void inorm_hist_kernel(const FrameJob* jobs, int nframes, int job_pitch, int max_tiles)
{
  const FrameJob& j = inorm_level_job(jobs, blockIdx.z, nframes, job_pitch);
  const int n = j.rows * j.cols;
  const int tiles = inorm_hist_tiles(n, max_tiles);
  if((int) blockIdx.x >= tiles) return;
  __shared__ uint32_t h[4][256];
  __shared__ uint32_t cum[2][256];
  __shared__ int s_last, s_below[2];
  const int t = threadIdx.x;
  for(int w = 0; w < 4; ++w) h[w][t] = 0;
  __syncthreads();
  uint32_t* mine = h[t >> 6];
  const uint8_t* img = j.img;
  const uint2* words = reinterpret_cast<const uint2*>(img);      // (level images start on 256-byte boundaries)
  const int nw = n / 8, stride = tiles * 256;
  for(int w = blockIdx.x * 256 + t; w < nw; w += 4 * stride) {
    uint2 v[4];
#pragma unroll
    for(int u = 0; u < 4; ++u) v[u] = w + u * stride < nw ? words[w + u * stride] : make_uint2(0u, 0u);
#pragma unroll
    for(int u = 0; u < 4; ++u)
      if(w + u * stride < nw) inorm_count8(mine, v[u]);
  }
  if(blockIdx.x == 0 && t < n - 8 * nw) atomicAdd(&mine[img[8 * nw + t]], 1u);      // the last n mod 8 pixels
  __syncthreads();
  InormScratch* sc = j.inorm;
  const uint32_t s = h[0][t] + h[1][t] + h[2][t] + h[3][t];
  if(s) __hip_atomic_fetch_add(&sc->bins[t], s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  // the adds of this workgroup are ordered before its ticket, the last ticket before the reads of the bins
  __threadfence();
  __syncthreads();
  if(t == 0) {
    const unsigned ticket = __hip_atomic_fetch_add(&sc->ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    s_last = ticket == (unsigned) tiles - 1u;
    s_below[0] = s_below[1] = 0;
  }
  __syncthreads();
  if(!s_last) return;
  __threadfence();
  // running sums of the bins: a scan over the 256 threads, double-buffered
  cum[0][t] = __hip_atomic_exchange(&sc->bins[t], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if(t == 0) __hip_atomic_store(&sc->ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  int cur = 0;
#pragma unroll
  for(int d = 1; d < 256; d <<= 1) {
    cum[cur ^ 1][t] = cum[cur][t] + (t >= d ? cum[cur][t - d] : 0u);
    cur ^= 1;
    __syncthreads();
  }
  // med = #{v : cum[v] < half}, mad = #{k : folded count of k < half}: both predicates are monotone, so the counts are the first index that fails them
  const uint32_t half = inorm_half((uint32_t) n);
  if(cum[cur][t] < half) atomicAdd(&s_below[0], 1);
  __syncthreads();
  const int med = s_below[0] < 255 ? s_below[0] : 255;
  if(inorm_folded_count(cum[cur], med, t) < half) atomicAdd(&s_below[1], 1);
  __syncthreads();
  const int mad = s_below[1] < 255 ? s_below[1] : 255;
  sc->table[t] = inorm_table_entry(t, med, mad);
}

// ---- radius 0, second launch: the table applied to the image, 16 pixels per thread in four 4-byte loads / 16-byte stores
constexpr int INORM_APPLY_PX = 4096;
__global__ __launch_bounds__(256) void inorm_apply_kernel(const FrameJob* jobs, int nframes, int job_pitch)
{
  const FrameJob& j = inorm_level_job(jobs, blockIdx.z, nframes, job_pitch);
  const int n = j.rows * j.cols;
  const int base = blockIdx.x * INORM_APPLY_PX;
  if(base >= n) return;
  __shared__ float tab[256];
  tab[threadIdx.x] = j.inorm->table[threadIdx.x];
  __syncthreads();
  const uint8_t* img = j.img;
  float* desc = j.desc;
#pragma unroll
  for(int it = 0; it < INORM_APPLY_PX / 1024; ++it) {
    const int i = base + (it * 256 + (int) threadIdx.x) * 4;
    if(i + 3 < n) {
      const uchar4 v = *reinterpret_cast<const uchar4*>(img + i);
      *reinterpret_cast<float4*>(desc + i) = make_float4(tab[v.x], tab[v.y], tab[v.z], tab[v.w]);
    } else {
      for(int k = i; k < n; ++k) desc[k] = tab[img[k]];
    }
  }
}

// ---- radius 1 .. 15, local: one launch.  A workgroup owns a 64 x 16 tile: it stages the tile and its halo of R pixels in LDS as whole dwords
// (pixels outside the image are zeros: they add nothing to the sums, and the window's pixel count comes in closed form, inorm_window_count),
// forms the sums S1 / S2 of every staged row's (2 R + 1)-wide windows as running sums along the row — one thread per (row, 16 columns) —, then
// those of the (2 R + 1) rows of a window as running sums down the column — one thread per (column, 4 rows) —, and writes inorm_local_value.
// LDS: 4600 B of pixels + 2 x 46 x 65 dwords of row sums = 28.5 KB.  Pitches: 100 bytes = 25 dwords per staged row and 65 dwords per row of
// sums, both odd in dwords, so the row-per-lane accesses of the row pass spread over the banks; the column pass reads consecutive dwords.
constexpr int INORM_TW = 64, INORM_TH = 16;
constexpr int INORM_SH = INORM_TH + 2 * kInormMaxRadius;                 // staged rows at most (46)
constexpr int INORM_PITCH = 100;                                         // bytes per staged row: 64 + 30 columns + up to 3 in front, in dwords
constexpr int INORM_RPITCH = INORM_TW + 1;
static_assert(INORM_TW + 2 * kInormMaxRadius + 3 <= INORM_PITCH && INORM_PITCH % 4 == 0, "a staged row holds the tile, both halos and the alignment bytes");
__global__ __launch_bounds__(256) void inorm_local_kernel(const FrameJob* jobs, int nframes, int job_pitch, int R)
{
  const FrameJob& j = inorm_level_job(jobs, blockIdx.z, nframes, job_pitch);
  const int W = j.cols, H = j.rows;
  const int x0 = blockIdx.x * INORM_TW, y0 = blockIdx.y * INORM_TH;
  if(x0 >= W || y0 >= H) return;
  __shared__ uint32_t px[INORM_SH * INORM_PITCH / 4];
  __shared__ uint32_t r1[INORM_SH * INORM_RPITCH], r2[INORM_SH * INORM_RPITCH];
  const int t = threadIdx.x;
  const int sh = INORM_TH + 2 * R;
  const int xa = (x0 - R) & ~3;                    // image column of staged byte 0 (a multiple of 4, may be negative)
  const int off = (x0 - R) - xa;                   // staged byte of the first window column
  const int ndw = (off + INORM_TW + 2 * R + 3) / 4;
  const uint8_t* img = j.img;
  const int npix = W * H;
  for(int k = t; k < sh * ndw; k += 256) {
    const int sy = k / ndw, d = k - sy * ndw;
    const int y = y0 - R + sy, x = xa + 4 * d;     // (x is a multiple of 4: the dword lies wholly left of the image or begins inside its row or right of it)
    uint32_t v = 0;
    if(y >= 0 && y < H && x >= 0 && x < W) {
      // the four bytes from pixel (x, y) on, from the one or two aligned dwords that hold them; the second only where it begins inside the image
      const int a = y * W + x, a4 = a & ~3;
      const uint32_t lo = *reinterpret_cast<const uint32_t*>(img + a4);
      const uint32_t hi = ((a & 3) && a4 + 4 < npix) ? *reinterpret_cast<const uint32_t*>(img + a4 + 4) : 0u;
      v = (uint32_t) (((uint64_t) hi << 32 | lo) >> (8 * (a & 3)));
      const int keep = W - x;                      // bytes of the dword that are pixels of this row
      if(keep < 4) v &= (1u << (8 * keep)) - 1u;
    }
    px[sy * (INORM_PITCH / 4) + d] = v;
  }
  __syncthreads();
  const uint8_t* pb = reinterpret_cast<const uint8_t*>(px);
  if(t < sh * 4) {
    const int sy = t % sh, seg = t / sh;
    const uint8_t* p = pb + sy * INORM_PITCH + off + seg * 16;
    uint32_t* o1 = r1 + sy * INORM_RPITCH + seg * 16;
    uint32_t* o2 = r2 + sy * INORM_RPITCH + seg * 16;
    uint32_t s1 = 0, s2 = 0;
    for(int d = 0; d <= 2 * R; ++d) { const uint32_t v = p[d]; s1 += v; s2 += v * v; }
    o1[0] = s1; o2[0] = s2;
    for(int c = 1; c < 16; ++c) {
      const uint32_t a = p[c + 2 * R], b = p[c - 1];
      s1 += a - b; s2 += a * a - b * b;
      o1[c] = s1; o2[c] = s2;
    }
  }
  __syncthreads();
  const int x = t & 63, q = t >> 6;
  const int gx = x0 + x;
  uint32_t s1 = 0, s2 = 0;
  for(int d = 0; d <= 2 * R; ++d) { s1 += r1[(q * 4 + d) * INORM_RPITCH + x]; s2 += r2[(q * 4 + d) * INORM_RPITCH + x]; }
  float* desc = j.desc;
#pragma unroll
  for(int r = 0; r < 4; ++r) {
    const int ty = q * 4 + r, gy = y0 + ty;
    if(r > 0) {
      s1 += r1[(ty + 2 * R) * INORM_RPITCH + x] - r1[(ty - 1) * INORM_RPITCH + x];
      s2 += r2[(ty + 2 * R) * INORM_RPITCH + x] - r2[(ty - 1) * INORM_RPITCH + x];
    }
    if(gx < W && gy < H) {
      const int I = pb[(ty + R) * INORM_PITCH + off + R + x];
      desc[(size_t) gy * W + gx] = inorm_local_value(I, inorm_window_count(gx, gy, W, H, R), s1, s2);
    }
  }
}

void launch_intensity_norm(hipStream_t s, const FrameLaunch& f, int radius)
{
  const int nz = f.nframes * f.nlevels;
  if(radius == 0) {
    const int max_tiles = inorm_hist_max_tiles(nz);
    hipLaunchKernelGGL(inorm_hist_kernel, dim3(inorm_hist_tiles(f.W * f.R, max_tiles), 1, nz), dim3(256), 0, s, f.jobs, f.nframes, f.job_pitch, max_tiles);
    hipLaunchKernelGGL(inorm_apply_kernel, dim3((f.W * f.R + INORM_APPLY_PX - 1) / INORM_APPLY_PX, 1, nz), dim3(256), 0, s, f.jobs, f.nframes, f.job_pitch);
  } else {
    hipLaunchKernelGGL(inorm_local_kernel, dim3((f.W + INORM_TW - 1) / INORM_TW, (f.R + INORM_TH - 1) / INORM_TH, nz), dim3(256), 0, s, f.jobs, f.nframes,
                       f.job_pitch, radius);
  }
}

}  // namespace bpvo_hip
