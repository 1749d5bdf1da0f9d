// Stereo front-end, second matcher: the reference's in-tree semi-global matcher SgmStereo (utils/sgm.{h,cc} — the
// SPS-stereo SGM; selected by `StereoAlgorithm = SGM`, utils/stereo_algorithm.cc:42-59,127-133; conf/kitti_eval.cfg:27 and
// conf/kitti_stereo.cfg:5 run the KITTI evaluation with it).  Integer arithmetic throughout (int16 saturating path costs; two double
// expressions: the census weight and the sub-pixel step), so the bar is bit-equality with the oracle's restatement, which cites the
// source line by line (parity unpinned: utils/sgm.cc includes OpenCV and cannot be built here).
//
// The CPU code is one sequential sweep per pass that carries two paths at once; on the device the same sums are computed from
// their definitions, the sequential part reduced to what is sequential in the algorithm:
//   sgm_census_sobel   capped x-Sobel (right image mirrored, as the original stores it) and the 5x5 / 3x3 census code       per pixel
//   sgm_pixel_cost     Birchfield-Tomasi style sampling-insensitive |dSobel| + weighted census Hamming distance            per (y, x, d)
//   sgm_box_rows/cols  (2r+1)^2 box sum with clamped coordinates = the sliding row / column sums of the original, incl. the rows and
//                      the column the original never writes (S1 in the oracle); separable, four disparities per thread      per (y, x, d)
//   sgm_right_cost     the right image's cost volume: right(x, d) = left(x + d, d), clamped                                  per (y, x, d)
//   sgm_path_packed    one scanline (a row for the horizontal paths, a column for the vertical ones) per wavefront, lanes = pairs of
//                      disparities, sequential along the line: L(p, d) = min(L'(d), L'(d +- 1) + P1, min L' + P2) - (min L' + P2) +
//                      C(p, d) in packed int16 saturating arithmetic, neighbours and the wave minimum by DPP (sg_scanline.h)   per line
//   sgm_wta            winner takes all + the original's sub-pixel expression in double                                      per pixel
//   speckle filter     connected components (|difference| <= 2 * factor between 4-neighbours) by lock-free union-find over run labels, sizes by
//                      atomics, regions of <= 100 pixels zeroed — the flood fill of the original finds the same components
//   sgm_lr_check       left-right consistency of the left map, conversion to float
// Bounds (profiles/r04_stereo_pmc.txt): the scanline kernel is a chain of `width` (or `height`) dependent steps per wavefront with
// 2 (2 H + 2 W) wavefronts in flight; everything else streams the 1- and 2-byte volumes once or twice.
#include <algorithm>
#include <type_traits>

#include "kernels.h"
#include "sg_scanline.h"

namespace bpvo_hip {

namespace {

__device__ __forceinline__ int sat16(int v) { return min(32767, max(-32768, v)); }

// Frame f of a launch (the grid's last dimension): the images and the f32 map advance by the frame's pixels, every scratch pointer by ONE
// stride in bytes — frame f works on the f-th copy of the whole scratch layout (sgm_scratch_bytes, a multiple of 256).  What a kernel
// indexes stays relative to its own frame: the labels of the union-find are pixel indices of the frame, its atomics never leave it.
template <class T>
__device__ __forceinline__ T* sgm_frame(T* p, size_t stride_bytes, unsigned f)
{
  return reinterpret_cast<T*>(reinterpret_cast<uintptr_t>(p) + stride_bytes * f);
}

__global__ __launch_bounds__(256) void sgm_census_sobel_kernel(const uint8_t* __restrict__ img, uint8_t* __restrict__ sobel, int* __restrict__ census,
                                                              int rows, int cols, int pitch, int cap, int crad, int flip, size_t fs)
{
  const int x = blockIdx.x * 64 + (threadIdx.x & 63);
  const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if(y >= rows) return;
  img += (size_t) rows * cols * blockIdx.z;
  sobel = sgm_frame(sobel, fs, blockIdx.z);
  census = sgm_frame(census, fs, blockIdx.z);
  // the row pitch is wider than the image: the padding (and the image border) holds `cap` (memset in the original)
  if(x >= cols) {
    if(x < pitch) sobel[(size_t) pitch * y + x] = (uint8_t) cap;
    return;
  }
  const int c = img[(size_t) cols * y + x];
  int code = 0;
  for(int oy = -crad; oy <= crad; ++oy)
    for(int ox = -crad; ox <= crad; ++ox) {
      code <<= 1;
      const int yy = y + oy, xx = x + ox;
      if(yy >= 0 && yy < rows && xx >= 0 && xx < cols && (int) img[(size_t) cols * yy + xx] >= c) code += 1;
    }
  census[(size_t) cols * y + x] = code;
  int v = cap;
  const bool interior = y >= 1 && y < rows - 1 && x >= 1 && x < cols - 1;
  if(interior) {
    const uint8_t* r0 = img + (size_t) cols * (y - 1);
    const uint8_t* r1 = r0 + cols;
    const uint8_t* r2 = r1 + cols;
    v = ((int) r0[x + 1] + 2 * (int) r1[x + 1] + (int) r2[x + 1]) - ((int) r0[x - 1] + 2 * (int) r1[x - 1] + (int) r2[x - 1]);
    v = v > cap ? 2 * cap : (v < -cap ? 0 : v + cap);
  }
  // interior pixels land mirrored for the right image; the border columns keep `cap` at their own (unmirrored) place — which the
  // mirrored interior never touches (columns 0 and W - 1 map onto each other)
  const int xo = (flip && interior) ? cols - x - 1 : x;
  sobel[(size_t) pitch * y + xo] = (uint8_t) v;
}

__device__ __forceinline__ void half_minmax(const uint8_t* __restrict__ row, int x, int W, int& mn, int& mx)
{
  const int c = row[x];
  const int l = x > 0 ? (c + (int) row[x - 1]) / 2 : c;
  const int r = x < W - 1 ? (c + (int) row[x + 1]) / 2 : c;
  mn = min(min(l, r), c);
  mx = max(max(l, r), c);
}

// pixel-wise cost u8 [rows][cols][D] per ROW TILE: a workgroup handles SPC_TX pixels of one row; what a cost needs of the left pixel (centre,
// half-pixel minimum and maximum, census word) and of the SPC_TX + D - 1 right positions the tile's disparities reach is formed ONCE in LDS (one
// workgroup per pixel recomputing it per disparity from six loads: 200 us per 1241 x 376 x 128 frame, now 47), the weighted Hamming term
// (uint8) ((double) ham * cweight) comes from a 33-entry table of that very expression, and a thread writes four consecutive disparities as
// one dword.  D a multiple of 4, D <= 256.
constexpr int SPC_TX = 32, SPC_MAXD = 256;
__global__ __launch_bounds__(256) void sgm_pixel_cost_tile_kernel(const uint8_t* __restrict__ sl, const uint8_t* __restrict__ sr, const int* __restrict__ cl,
                                                                   const int* __restrict__ cr, uint8_t* __restrict__ pc, int rows, int cols, int pitch, int D,
                                                                   double cweight, size_t fs)
{
  sl = sgm_frame(sl, fs, blockIdx.z); sr = sgm_frame(sr, fs, blockIdx.z); cl = sgm_frame(cl, fs, blockIdx.z); cr = sgm_frame(cr, fs, blockIdx.z);
  pc = sgm_frame(pc, fs, blockIdx.z);
  __shared__ uint8_t s_lc[SPC_TX], s_lmin[SPC_TX], s_lmax[SPC_TX];
  __shared__ int s_cl[SPC_TX];
  __shared__ uint8_t s_rc[SPC_TX + SPC_MAXD], s_rmin[SPC_TX + SPC_MAXD], s_rmax[SPC_TX + SPC_MAXD];
  __shared__ int s_cr[SPC_TX + SPC_MAXD];
  __shared__ uint8_t s_ham[33];
  const int y = blockIdx.y, x0 = blockIdx.x * SPC_TX, tid = threadIdx.x;
  const uint8_t* lrow = sl + (size_t) pitch * y;
  const uint8_t* rrow = sr + (size_t) pitch * y;               // mirrored: original column x - d sits at cols - 1 - x + d
  const int nr = SPC_TX + D - 1;
  // right positions ri0 + k, k = 0 .. nr - 1, with ri0 = cols - 1 - (x0 + SPC_TX - 1) (those outside the row are never indexed: d <= x)
  const int ri0 = cols - SPC_TX - x0;
  // census words of the right image at columns cx0 + k, cx0 = x0 - (D - 1)
  const int cx0 = x0 - D + 1;
  for(int k = tid; k < nr; k += 256) {
    const int ri = ri0 + k;
    if(ri >= 0 && ri < cols) {
      int mn, mx;
      half_minmax(rrow, ri, cols, mn, mx);
      s_rc[k] = rrow[ri]; s_rmin[k] = (uint8_t) mn; s_rmax[k] = (uint8_t) mx;
    }
    const int cx = cx0 + k;
    if(cx >= 0 && cx < cols) s_cr[k] = cr[(size_t) cols * y + cx];
  }
  if(tid < SPC_TX && x0 + tid < cols) {
    const int x = x0 + tid;
    int mn, mx;
    half_minmax(lrow, x, cols, mn, mx);
    s_lc[tid] = lrow[x]; s_lmin[tid] = (uint8_t) mn; s_lmax[tid] = (uint8_t) mx;
    s_cl[tid] = cl[(size_t) cols * y + x];
  }
  if(tid >= 64 && tid < 64 + 33) s_ham[tid - 64] = (uint8_t) ((double) (tid - 64) * cweight);
  __syncthreads();
  const int dq = D >> 2;
  for(int it = tid; it < SPC_TX * dq; it += 256) {
    const int xi = it / dq, q = it - xi * dq;
    const int x = x0 + xi;
    if(x >= cols) break;                                       // (items are ordered by pixel)
    const int lc = s_lc[xi], lmin = s_lmin[xi], lmax = s_lmax[xi];
    const unsigned lcen = (unsigned) s_cl[xi];
    unsigned out = 0;
#pragma unroll
    for(int e = 0; e < 4; ++e) {
      const int d = min(4 * q + e, x);                          // costs beyond d = x repeat the one at d = x (S2)
      const int kr = (SPC_TX - 1 - xi) + d;                     // = cols - 1 - x + d - ri0
      const int kc = (xi + D - 1) - d;                          // = x - d - cx0
      const int rc = s_rc[kr], rmin = s_rmin[kr], rmax = s_rmax[kr];
      int l2r = max(0, lc - rmax);
      l2r = max(l2r, rmin - lc);
      int r2l = max(0, rc - lmax);
      r2l = max(r2l, lmin - rc);
      const int sad = min(l2r, r2l);
      const int ham = __popc(lcen ^ (unsigned) s_cr[kc]);
      out |= (unsigned) (uint8_t) (sad + (int) s_ham[ham]) << (8 * e);
    }
    *reinterpret_cast<unsigned*>(pc + ((size_t) cols * y + x) * D + 4 * q) = out;
  }
}

// (2r+1)^2 box sums with clamped coordinates; rows y + r >= rows and (for y >= 1) column 0 stay 0 (S1).  Separable: the sum over the
// window's columns first (u16, at most (2r+1) * 255), then over its rows — 2 (2r+1) reads per output instead of (2r+1)^2; integer sums,
// any order (round 3 evaluated the 25 clamped taps per output directly: 0.6 ms per 1241 x 376 x 128 frame, profiles/r03_stereo.txt).
// A thread owns four consecutive disparities of one pixel: 4-byte / 8-byte accesses, coalesced along d.
__global__ __launch_bounds__(256) void sgm_box_rows_kernel(const uint8_t* __restrict__ pc, uint16_t* __restrict__ rowsum, int rows, int cols, int D, int wrad, size_t fs)
{
  pc = sgm_frame(pc, fs, blockIdx.y);
  rowsum = sgm_frame(rowsum, fs, blockIdx.y);
  const size_t t = (size_t) blockIdx.x * 256 + threadIdx.x;          // (pixel, group of 4 disparities)
  const int dq = D >> 2;
  const size_t p = t / dq;
  if(p >= (size_t) rows * cols) return;
  const int d = (int) (t - p * dq) * 4;
  const int x = (int) (p % cols);
  const size_t row0 = p - x;
  int s0 = 0, s1 = 0, s2 = 0, s3 = 0;
  for(int ox = -wrad; ox <= wrad; ++ox) {
    const int xx = min(max(x + ox, 0), cols - 1);
    const uchar4 v = *reinterpret_cast<const uchar4*>(pc + (row0 + xx) * D + d);
    s0 += v.x; s1 += v.y; s2 += v.z; s3 += v.w;
  }
  *reinterpret_cast<ushort4*>(rowsum + p * D + d) = make_ushort4((uint16_t) s0, (uint16_t) s1, (uint16_t) s2, (uint16_t) s3);
}
__global__ __launch_bounds__(256) void sgm_box_cols_kernel(const uint16_t* __restrict__ rowsum, uint16_t* __restrict__ cost, int rows, int cols, int D, int wrad, size_t fs)
{
  rowsum = sgm_frame(rowsum, fs, blockIdx.y);
  cost = sgm_frame(cost, fs, blockIdx.y);
  const size_t t = (size_t) blockIdx.x * 256 + threadIdx.x;
  const int dq = D >> 2;
  const size_t p = t / dq;
  if(p >= (size_t) rows * cols) return;
  const int d = (int) (t - p * dq) * 4;
  const int x = (int) (p % cols), y = (int) (p / cols);
  int s0 = 0, s1 = 0, s2 = 0, s3 = 0;
  if(y + wrad < rows && (y == 0 || x >= 1)) {
    for(int oy = -wrad; oy <= wrad; ++oy) {
      const int yy = min(max(y + oy, 0), rows - 1);
      const ushort4 v = *reinterpret_cast<const ushort4*>(rowsum + ((size_t) cols * yy + x) * D + d);
      s0 += v.x; s1 += v.y; s2 += v.z; s3 += v.w;
    }
  }
  *reinterpret_cast<ushort4*>(cost + p * D + d) = make_ushort4((uint16_t) s0, (uint16_t) s1, (uint16_t) s2, (uint16_t) s3);
}

__global__ void sgm_right_cost_kernel(const uint16_t* __restrict__ lcost, uint16_t* __restrict__ rcost, int rows, int cols, int D, size_t fs)
{
  lcost = sgm_frame(lcost, fs, blockIdx.z);
  rcost = sgm_frame(rcost, fs, blockIdx.z);
  const int x = blockIdx.x, y = blockIdx.y, d = threadIdx.x;
  if(d >= D) return;
  const int dd = min(d, cols - 1 - x);                         // past the image the last valid disparity's cost repeats
  rcost[((size_t) cols * y + x) * D + d] = lcost[((size_t) cols * y + x + dd) * D + dd];
}

// The same through LDS (D <= 128): the gather above reads one 2-byte value per lane, every lane from another 256-byte row (eight times
// the volume in requests: profiles/r04_stereo_pmc.txt).  Here a workgroup fetches the SRC_TX + D - 1 rows its SRC_TX pixels reach as
// whole rows (16-byte loads; neighbouring tiles share most of them in the L2) and reads the diagonal from LDS.
constexpr int SRC_TX = 64, SRC_MAXD = 128, SRC_PITCH = SRC_MAXD + 8;      // halfwords per staged row: 272 bytes, 16-byte aligned, banks spread along the diagonal
__global__ __launch_bounds__(256) void sgm_right_cost_tile_kernel(const uint16_t* __restrict__ lcost, uint16_t* __restrict__ rcost, int rows, int cols, int D, size_t fs)
{
  lcost = sgm_frame(lcost, fs, blockIdx.y);
  rcost = sgm_frame(rcost, fs, blockIdx.y);
  __shared__ __attribute__((aligned(16))) uint16_t s_rows[(SRC_TX + SRC_MAXD - 1) * SRC_PITCH];
  // Workgroups are handed to the XCDs round robin, and every XCD has its own L2: consecutive tiles of a row, which share all but SRC_TX of
  // their rows, go to ONE XCD (each takes a contiguous eighth of the tiles): 563 -> 119.5 MB read per 1241 x 376 x 128 frame, the volume itself.
  // (a 1-D grid of 8 * per workgroups, per = ceil(tiles / 8))
  const int gx = (cols + SRC_TX - 1) / SRC_TX, ntile = gx * rows, per = (int) gridDim.x >> 3;
  const int tile = ((int) blockIdx.x & 7) * per + ((int) blockIdx.x >> 3);
  if(tile >= ntile) return;
  const int y = tile / gx, x0 = (tile - y * gx) * SRC_TX, tid = threadIdx.x;
  const int nrow = min(SRC_TX + D - 1, cols - x0);             // rows of pixels x0 .. x0 + nrow - 1 (past the image nothing is read: dd <= cols - 1 - x)
  const int v8 = D >> 3;                                       // 16-byte vectors per row
  const uint4* __restrict__ src = reinterpret_cast<const uint4*>(lcost + ((size_t) cols * y + x0) * D);
  for(int i = tid; i < nrow * v8; i += 256) {
    const int r = i / v8, c = i - r * v8;
    *reinterpret_cast<uint4*>(&s_rows[r * SRC_PITCH + 8 * c]) = src[(size_t) r * v8 + c];
  }
  __syncthreads();
  const int dq = D >> 2;
  for(int it = tid; it < SRC_TX * dq; it += 256) {
    const int xl = it / dq, q = it - xl * dq;
    const int x = x0 + xl;
    if(x >= cols) break;
    const int last = cols - 1 - x;                             // past the image the last valid disparity's cost repeats
    uint16_t v[4];
#pragma unroll
    for(int e = 0; e < 4; ++e) {
      const int dd = min(4 * q + e, last);
      v[e] = s_rows[(xl + dd) * SRC_PITCH + dd];
    }
    *reinterpret_cast<ushort4*>(rcost + ((size_t) cols * y + x) * D + 4 * q) = make_ushort4(v[0], v[1], v[2], v[3]);
  }
}

// One scanline per wavefront.  The four directions of a cost volume — along the rows left to right and back, along the columns down and
// up — depend on the cost volume alone, and so do the two volumes (left, right image): ALL EIGHT sets of scanlines run in ONE launch,
// 2 * (2 rows + 2 cols) wavefronts, every direction writing its path costs L into a volume of its own (the original adds them into one
// sum volume as it goes; the winner-takes-all kernel adds the four in the original's order).  The walk itself: sg_scanline.h.
template <int NP>
__global__ __launch_bounds__(64) void sgm_path_packed_kernel(const uint16_t* __restrict__ cost_l, const uint16_t* __restrict__ cost_r, int16_t* __restrict__ Lvol,
                                                             int rows, int cols, int D, int P1, int P2, size_t fs)
{
  cost_l = sgm_frame(cost_l, fs, blockIdx.y); cost_r = sgm_frame(cost_r, fs, blockIdx.y); Lvol = sgm_frame(Lvol, fs, blockIdx.y);
  // dispatch order: the rows of both cost volumes first (with cols > rows the longest chains of the launch), then the columns
  int side, path, line;
  {
    int q = blockIdx.x;
    if(q < 4 * rows) { side = q / (2 * rows); q -= side * 2 * rows; path = q < rows ? 0 : 2; line = q < rows ? q : q - rows; }
    else { q -= 4 * rows; side = q / (2 * cols); q -= side * 2 * cols; path = q < cols ? 1 : 3; line = q < cols ? q : q - cols; }
  }
  const int vertical = path & 1, dir = path < 2 ? 1 : -1;
#if SG_PRIO_VALUE
  if(!vertical && cols > rows) __builtin_amdgcn_s_setprio(3);      // the longest chains of the launch first (sg_scanline.h)
#endif
  const uint16_t* __restrict__ cost = side ? cost_r : cost_l;
  const size_t vol = (size_t) rows * cols * D;
  int16_t* __restrict__ L = Lvol + (size_t) (side * 4 + path) * vol;
  const int nsteps = vertical ? rows : cols;
  const long long stride = vertical ? (long long) cols * D : (long long) D;
  const long long first = vertical ? (long long) line * D : (long long) line * cols * D;
  // (a backward path walks from the line's last element with the stride negated)
  sg_walk_line<NP>(cost, L, dir > 0 ? first : first + (nsteps - 1) * stride, dir > 0 ? stride : -stride, nsteps, D, P1, P2);
}

// winner takes all (first minimum) + the sub-pixel expression of the original in double.  A wavefront per pixel: the D sums are read
// coalesced (V per lane), the first minimum is the wave minimum of (sum, d) packed into one integer.
// The sum of the four path costs in the original's order and saturating arithmetic: ((((0 + rows forward) + columns forward) + rows
// backward) + columns backward) (utils/sgm.cc:831-836, pass after pass).
__device__ __forceinline__ int sgm_sum4(const int16_t* __restrict__ L, size_t vol, size_t i)
{
  int s = sat16(0 + (int) L[i]);
  s = sat16(s + (int) L[vol + i]);
  s = sat16(s + (int) L[2 * vol + i]);
  return sat16(s + (int) L[3 * vol + i]);
}
template <int V>
__global__ __launch_bounds__(256) void sgm_wta_kernel(const int16_t* __restrict__ L4, uint16_t* __restrict__ disp, size_t npix, int D, double factor, size_t fs)
{
  L4 = sgm_frame(L4, fs, blockIdx.y);
  disp = sgm_frame(disp, fs, blockIdx.y);
  const size_t p = (size_t) blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if(p >= npix) return;
  const size_t vol = npix * D;
  int v[V];
  int key = 0x7fffffff;
#pragma unroll
  for(int k = 0; k < V; ++k) {
    const int d = lane * V + k;
    v[k] = d < D ? sgm_sum4(L4, vol, p * D + d) : 32767;
    if(d < D) key = min(key, ((v[k] + 32768) << 9) | d);      // (d < 512)
  }
  // minimum over the wave on the VALU (DPP row ladder + v_readlane: six ds_bpermute round trips as __shfl_xor), and the three sums the
  // sub-pixel step needs out of the lanes' registers instead of twelve more dependent loads by lane 0
  key = min(key, __builtin_amdgcn_update_dpp(key, key, 0x111 /*row_shr:1*/, 0xf, 0xf, false));
  key = min(key, __builtin_amdgcn_update_dpp(key, key, 0x112 /*row_shr:2*/, 0xf, 0xf, false));
  key = min(key, __builtin_amdgcn_update_dpp(key, key, 0x114 /*row_shr:4*/, 0xf, 0xf, false));
  key = min(key, __builtin_amdgcn_update_dpp(key, key, 0x118 /*row_shr:8*/, 0xf, 0xf, false));
  key = min(key, __builtin_amdgcn_update_dpp(key, key, 0x142 /*row_bcast:15*/, 0xa, 0xf, false));
  key = min(key, __builtin_amdgcn_update_dpp(key, key, 0x143 /*row_bcast:31*/, 0xc, 0xf, false));
  const int bd = __builtin_amdgcn_readlane(key, 63) & 511;
  auto sum_at = [&](int dsel) {      // dsel uniform over the wave
    const int li = __builtin_amdgcn_readfirstlane(dsel / V), rem = dsel % V;
    int r = 0;
#pragma unroll
    for(int k = 0; k < V; ++k) {
      const int t = __builtin_amdgcn_readlane(v[k], li);
      r = (k == rem) ? t : r;
    }
    return r;
  };
  int out;
  if(bd > 0 && bd < D - 1) {
    const int c = sum_at(bd), l = sum_at(bd - 1), r = sum_at(bd + 1);
    double w;
    if(r < l) w = (double) bd * factor + (double) (r - l) / (double) (c - l) / 2.0 * factor + 0.5;
    else w = (double) bd * factor + (double) (r - l) / (double) (c - r) / 2.0 * factor + 0.5;
    // static_cast<int> on x86: truncation, INT_MIN for NaN / infinities / out of range (a zero denominator: S5)
    const bool ok = (w == w) && w > -2147483649.0 && w < 2147483648.0;
    out = ok ? (int) w : (int) 0x80000000;
  } else {
    out = (int) ((double) bd * factor);
  }
  if(lane == 0) disp[p] = (uint16_t) out;
}

// ---- speckle filter: connected components by lock-free union-find (roots = smallest pixel index of the component)
__device__ __forceinline__ int uf_find(int* __restrict__ lab, int a)
{
  int p = lab[a];
  while(p != a) { a = p; p = lab[a]; }
  return a;
}
__device__ __forceinline__ void uf_union(int* __restrict__ lab, int a, int b)
{
  for(;;) {
    a = uf_find(lab, a);
    b = uf_find(lab, b);
    if(a == b) return;
    if(a < b) { const int t = a; a = b; b = t; }       // link the larger root under the smaller
    const int old = atomicMin(&lab[a], b);
    if(old == a) return;
    a = old;
  }
}
// Two pixels are connected when both are non-zero and differ by at most max_diff.  Labels START as the first pixel of the horizontal run
// a pixel belongs to, found inside the wavefront by a ballot of the run starts (no atomics; a run that enters the wavefront from the left
// starts, for now, at the wavefront's first pixel): one union per wavefront ties such a run to its left part, and a vertical pair
// (p, p + cols) needs a union only where its left neighbour pair does not already imply it — (p - 1, p), (p - 1 + cols, p + cols) and
// (p - 1, p - 1 + cols) all connected — i.e. about once per pair of overlapping runs instead of once per pixel.  Same components as
// linking every neighbour pair (round 3: 0.27 ms per launch on a 1241 x 376 plane, every pixel of which is one component).
__device__ __forceinline__ bool sgm_connected(int a, int b, int max_diff) { return a != 0 && b != 0 && abs(a - b) <= max_diff; }
__global__ __launch_bounds__(256) void sgm_cc_init_kernel(const uint16_t* __restrict__ img, int* __restrict__ lab, int* __restrict__ size, int rows, int cols,
                                                         int max_diff, size_t fs)
{
  img = sgm_frame(img, fs, blockIdx.y); lab = sgm_frame(lab, fs, blockIdx.y); size = sgm_frame(size, fs, blockIdx.y);
  const int p = blockIdx.x * 256 + threadIdx.x;
  const int npix = rows * cols;
  const int lane = threadIdx.x & 63;
  const int v = p < npix ? (int) img[p] : 0;
  const int x = p < npix ? p % cols : 0;
  const bool start = p >= npix || v == 0 || x == 0 || !sgm_connected(v, (int) img[p - 1], max_diff);     // (a zero pixel "starts" nothing: it breaks runs)
  const unsigned long long starts = __ballot(start) | 1ull;          // lane 0 stands in for a run that comes in from the left
  if(p >= npix) return;
  const unsigned long long upto = starts & (~0ull >> (63 - lane));   // run starts at lanes <= this one
  const int first = 63 - __clzll((long long) upto);
  lab[p] = v != 0 ? p - (lane - first) : -1;
  size[p] = 0;
}
__global__ __launch_bounds__(256) void sgm_cc_merge_kernel(const uint16_t* __restrict__ img, int* __restrict__ lab, int rows, int cols, int max_diff, size_t fs)
{
  img = sgm_frame(img, fs, blockIdx.y);
  lab = sgm_frame(lab, fs, blockIdx.y);
  const int p = blockIdx.x * 256 + threadIdx.x;
  if(p >= rows * cols) return;
  const int v = img[p];
  if(v == 0) return;
  const int x = p % cols, y = p / cols;
  // a run cut by the wavefront boundary: its first pixel of this wavefront and the pixel before it
  if((threadIdx.x & 63) == 0 && x > 0 && sgm_connected(v, (int) img[p - 1], max_diff)) uf_union(lab, p, p - 1);
  if(y < rows - 1) {
    const int q = img[p + cols];
    if(sgm_connected(v, q, max_diff)) {
      bool implied = false;
      if(x > 0) {
        const int vl = img[p - 1], ql = img[p + cols - 1];
        implied = sgm_connected(vl, v, max_diff) && sgm_connected(ql, q, max_diff) && sgm_connected(vl, ql, max_diff);
      }
      if(!implied) uf_union(lab, p, p + cols);
    }
  }
}
__global__ __launch_bounds__(256) void sgm_cc_count_kernel(int* __restrict__ lab, int* __restrict__ size, int npix, size_t fs)
{
  lab = sgm_frame(lab, fs, blockIdx.y);
  size = sgm_frame(size, fs, blockIdx.y);
  const int p = blockIdx.x * 256 + threadIdx.x;
  int r = -1;
  if(p < npix && lab[p] >= 0) {
    r = uf_find(lab, p);
    lab[p] = r;                                            // (path compression; roots never change after the merge kernel)
  }
  // the pixels of a wavefront mostly share one root (a plane is ONE component of 400 k pixels: one atomic per pixel on one address took
  // 4.3 ms): the lanes with the leader's root are counted with one atomic, then the next root, ... — and the root the workgroup's first
  // lanes have is counted in LDS first, one global atomic per workgroup (7 300 waves on one address were 90 us of queueing)
  __shared__ int s_root, s_cnt;
  if(threadIdx.x == 0) { s_root = r; s_cnt = 0; }
  __syncthreads();
  const int wg_root = s_root;
  unsigned long long todo = __ballot(r >= 0);
  while(todo) {
    const int leader = __ffsll((long long) todo) - 1;
    const int lr = __builtin_amdgcn_readlane(r, leader);
    const unsigned long long same = __ballot(r == lr) & todo;
    if((threadIdx.x & 63) == leader) {
      if(lr == wg_root) atomicAdd(&s_cnt, (int) __popcll(same));
      else atomicAdd(&size[lr], (int) __popcll(same));
    }
    todo &= ~same;
  }
  __syncthreads();
  if(threadIdx.x == 0 && s_cnt > 0) atomicAdd(&size[wg_root], s_cnt);
}
__global__ __launch_bounds__(256) void sgm_cc_apply_kernel(uint16_t* __restrict__ img, const int* __restrict__ lab, const int* __restrict__ size, int npix,
                                                          int max_size, size_t fs)
{
  img = sgm_frame(img, fs, blockIdx.y); lab = sgm_frame(lab, fs, blockIdx.y); size = sgm_frame(size, fs, blockIdx.y);
  const int p = blockIdx.x * 256 + threadIdx.x;
  if(p >= npix || lab[p] < 0) return;
  if(size[lab[p]] <= max_size) img[p] = 0;
}

// enforceLeftRightConsistency (left half) + disparity / factor -> float
__global__ __launch_bounds__(256) void sgm_lr_check_kernel(const uint16_t* __restrict__ dl, const uint16_t* __restrict__ dr, float* __restrict__ out, int rows,
                                                          int cols, double factor, int thresh, size_t fs)
{
  dl = sgm_frame(dl, fs, blockIdx.y);
  dr = sgm_frame(dr, fs, blockIdx.y);
  out += (size_t) rows * cols * blockIdx.y;
  const int p = blockIdx.x * 256 + threadIdx.x;
  if(p >= rows * cols) return;
  const int x = p % cols;
  int v = dl[p];
  if(v != 0) {
    const int ld = (int) ((double) v / factor + 0.5);
    if(x - ld < 0) v = 0;
    else {
      const int rd = (int) ((double) dr[p - ld] / factor + 0.5);
      if(rd == 0 || abs(ld - rd) > thresh) v = 0;
    }
  }
  out[p] = (float) ((double) v / factor);
}

}  // namespace

void launch_speckle_filter_u16(hipStream_t s, uint16_t* img, int* lab, int* size, int rows, int cols, int max_diff, int max_size, int nframes,
                               size_t frame_bytes)
{
  const size_t npix = (size_t) rows * cols;
  const dim3 nb((unsigned) ((npix + 255) / 256), (unsigned) nframes);
  hipLaunchKernelGGL(sgm_cc_init_kernel, nb, dim3(256), 0, s, img, lab, size, rows, cols, max_diff, frame_bytes);
  hipLaunchKernelGGL(sgm_cc_merge_kernel, nb, dim3(256), 0, s, img, lab, rows, cols, max_diff, frame_bytes);
  hipLaunchKernelGGL(sgm_cc_count_kernel, nb, dim3(256), 0, s, lab, size, (int) npix, frame_bytes);
  hipLaunchKernelGGL(sgm_cc_apply_kernel, nb, dim3(256), 0, s, img, lab, size, (int) npix, max_size, frame_bytes);
}

// The scratch of ONE frame, carved in one place: the launcher uses the pointers, sgm_scratch_bytes is the same walk on a null base — the
// stride from a frame's slice to the next (sgm_frame), so the two cannot disagree.
struct SgmScratch {
  int pitch;                     // row pitch of the Sobel planes: cols rounded up to 16
  uint8_t *sob_l, *sob_r;        // [rows][pitch]
  int *cen_l, *cen_r;            // census codes [rows][cols]
  uint8_t* pc;                   // pixel-wise cost [rows][cols][D]
  uint16_t *cost_l, *cost_r;     // box-summed cost volumes
  int16_t* Lvol;                 // path costs: [side][direction][rows][cols][D]
  uint16_t* rowsum;              // = Lvol: the row sums borrow the first path-cost volume (the scanline kernel overwrites it later on the same stream)
  uint16_t *disp_l, *disp_r;
  int *lab, *size;               // the speckle filter's labels and region sizes
  size_t bytes;                  // the whole layout, a multiple of 256
};
static SgmScratch sgm_layout(int rows, int cols, int D, unsigned char* base)
{
  const size_t npix = (size_t) rows * cols;
  Carver w{base};
  SgmScratch m;
  m.pitch = cols + 15 - (cols - 1) % 16;
  m.sob_l = w.take<uint8_t>((size_t) m.pitch * rows);
  m.sob_r = w.take<uint8_t>((size_t) m.pitch * rows);
  m.cen_l = w.take<int>(npix);
  m.cen_r = w.take<int>(npix);
  m.pc = w.take<uint8_t>(npix * D);
  m.cost_l = w.take<uint16_t>(npix * D);
  m.cost_r = w.take<uint16_t>(npix * D);
  m.Lvol = w.take<int16_t>(8 * npix * D);
  m.rowsum = reinterpret_cast<uint16_t*>(m.Lvol);
  m.disp_l = w.take<uint16_t>(npix);
  m.disp_r = w.take<uint16_t>(npix);
  m.lab = w.take<int>(npix);
  m.size = w.take<int>(npix);
  m.bytes = w.off;
  return m;
}
size_t sgm_scratch_bytes(int rows, int cols, int D) { return sgm_layout(rows, cols, D, nullptr).bytes; }

// SGMStereo::compute (utils/sgm.cc:250-285) for `nframes` rectified pairs of one size, in chunks of `frames_per_launch` frames: every kernel
// takes a chunk in one launch, frame f of it on the f-th slice of the scratch (sgm_frame).  One frame per launch is one frame after the other
// on one slice (the cost volumes of a 1241 x 376 x 128 frame are 120 MB each, and they fill the chip); small frames — a rig of 320 x 240
// cameras: 2 (2 rows + 2 cols) single-wave scanlines per frame — share the launches.  Integer arithmetic per frame: same maps either way.
bool launch_stereo_sgm(hipStream_t s, const SgmLaunch& g)
{
  const int rows = g.rows, cols = g.cols, D = g.ndisp;
  if(D <= 0 || D % 16 || D > 256) return false;
  const size_t npix = (size_t) rows * cols;
  const SgmScratch m = sgm_layout(rows, cols, D, (unsigned char*) g.scratch);
  const int pitch = m.pitch;
  const size_t fs = m.bytes;                                    // the stride from a frame's slice to the next
  const int cap = (std::min(std::max(g.sobel_cap, 15), 127)) | 1;
  const int dthreads = (D + 63) / 64 * 64;
  const unsigned nb = (unsigned) ((npix + 255) / 256);
  const int per = std::max(1, std::min(g.frames_per_launch, 65535));      // (the frame is a grid's y or z)
  for(int f0 = 0; f0 < g.nframes; f0 += per) {
    const unsigned F = (unsigned) std::min(per, g.nframes - f0);
    const uint8_t* L = g.left + npix * f0;
    const uint8_t* R = g.right + npix * f0;
    const dim3 gpix((pitch + 63) / 64, (rows + 3) / 4, F);
    hipLaunchKernelGGL(sgm_census_sobel_kernel, gpix, dim3(256), 0, s, L, m.sob_l, m.cen_l, rows, cols, pitch, cap, g.census_radius, 0, fs);
    hipLaunchKernelGGL(sgm_census_sobel_kernel, gpix, dim3(256), 0, s, R, m.sob_r, m.cen_r, rows, cols, pitch, cap, g.census_radius, 1, fs);
    hipLaunchKernelGGL(sgm_pixel_cost_tile_kernel, dim3((cols + SPC_TX - 1) / SPC_TX, rows, F), dim3(256), 0, s, m.sob_l, m.sob_r, m.cen_l, m.cen_r, m.pc, rows, cols,
                       pitch, D, g.census_weight, fs);
    {
      const dim3 nbq((unsigned) ((npix * (size_t) (D / 4) + 255) / 256), F);
      hipLaunchKernelGGL(sgm_box_rows_kernel, nbq, dim3(256), 0, s, m.pc, m.rowsum, rows, cols, D, g.window_radius, fs);
      hipLaunchKernelGGL(sgm_box_cols_kernel, nbq, dim3(256), 0, s, m.rowsum, m.cost_l, rows, cols, D, g.window_radius, fs);
    }
    if(D <= SRC_MAXD) hipLaunchKernelGGL(sgm_right_cost_tile_kernel, dim3(8u * (unsigned) (((cols + SRC_TX - 1) / SRC_TX * rows + 7) / 8), F), dim3(256), 0, s, m.cost_l, m.cost_r, rows, cols, D, fs);
    else hipLaunchKernelGGL(sgm_right_cost_kernel, dim3(cols, rows, F), dim3(dthreads), 0, s, m.cost_l, m.cost_r, rows, cols, D, fs);
    dispatch_path_width(D, [&](auto np) {
      hipLaunchKernelGGL(sgm_path_packed_kernel<decltype(np)::value>, dim3((unsigned) (2 * (2 * rows + 2 * cols)), F), dim3(64), 0, s, m.cost_l, m.cost_r, m.Lvol, rows, cols,
                         D, g.P1, g.P2, fs);
    });
    for(int side = 0; side < 2; ++side) {
      uint16_t* disp = side == 0 ? m.disp_l : m.disp_r;
      const int16_t* L4 = m.Lvol + (size_t) side * 4 * npix * D;
      dispatch_wta_width(D, [&](auto v) {
        hipLaunchKernelGGL(sgm_wta_kernel<decltype(v)::value>, dim3((unsigned) ((npix + 3) / 4), F), dim3(256), 0, s, L4, disp, npix, D, g.disparity_factor, fs);
      });
      // speckleFilter(100, 2 * factor) (utils/sgm.cc:898)
      launch_speckle_filter_u16(s, disp, m.lab, m.size, rows, cols, (int) (2 * g.disparity_factor), 100, (int) F, fs);
    }
    hipLaunchKernelGGL(sgm_lr_check_kernel, dim3(nb, F), dim3(256), 0, s, m.disp_l, m.disp_r, g.disp + npix * f0, rows, cols, g.disparity_factor, g.consistency_threshold, fs);
  }
  return true;
}

}  // namespace bpvo_hip
