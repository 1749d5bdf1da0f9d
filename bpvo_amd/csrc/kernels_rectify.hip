// libbpvo_hip, device side: raw (distorted, unrectified) 8-bit images -> rectified images, through a map of 1/32-pixel source coordinates
// built on the host (rectify_math.h states the rule; rectify.hip builds and keeps the maps).
#include "kernels.h"
#include "rectify_math.h"

namespace bpvo_hip {

// All the frames of a call — both sides, whatever their sizes — in one launch: frame blockIdx.z is the row of the table (uniform: scalar
// loads), the grid covers the largest frame, and the workgroups beyond their own frame leave at once (there is no barrier in the kernel).
// A workgroup is 4 rows x 64 lanes, a wavefront one row, a lane four consecutive destination pixels, stored as ONE dword: the frames of a
// call lie back to back, so a row begins at any byte address, and the groups of four are laid on the ADDRESS grid, not on the column grid
// — lane g of a row takes the columns 4 g - off .. 4 g - off + 3, off = the row's address mod 4 —, which leaves byte stores to the first and
// last group of a row alone.  A lane reads its four map entries (32 B, consecutive; the wavefront's 2 KiB are contiguous) before any tap, so
// that eight-byte loads of four pixels are in flight together; the taps come through the caches (neighbouring destinations share source
// lines: with a mild lens a lane's sixteen taps lie in two or three 64-byte lines).  No LDS.
__global__ __launch_bounds__(256) void rectify_frames_kernel(const RectifyFrame* __restrict__ frames)
{
  const RectifyFrame fr = frames[blockIdx.z];
  if((int) blockIdx.x * 256 - 3 >= fr.cols || (int) blockIdx.y * 4 >= fr.rows) return;
  const int row = (int) blockIdx.y * 4 + (int) (threadIdx.x >> 6);
  if(row >= fr.rows) return;
  const size_t row_at = (size_t) row * (size_t) fr.cols;
  uint8_t* __restrict__ drow = fr.dst + row_at;
  const int2* __restrict__ mrow = fr.map + row_at;
  const int off = (int) (reinterpret_cast<uintptr_t>(drow) & 3u);
  const int c0 = ((int) blockIdx.x * 64 + (int) (threadIdx.x & 63)) * 4 - off;      // (> -4)
  if(c0 >= fr.cols) return;
  int2 e[4];
#pragma unroll
  for(int k = 0; k < 4; ++k) {
    const int c = c0 + k;
    e[k] = (c >= 0 && c < fr.cols) ? mrow[c] : make_int2(kRectOutside, kRectOutside);
  }
  uint32_t word = 0;
#pragma unroll
  for(int k = 0; k < 4; ++k) word |= (uint32_t) rectify_pixel(fr.src, fr.raw_rows, fr.raw_cols, e[k].x, e[k].y) << (8 * k);
  if(c0 >= 0 && c0 + 4 <= fr.cols) {
    *reinterpret_cast<uint32_t*>(drow + c0) = word;      // (drow + c0 = the row's address - off + a multiple of 4)
  } else {
#pragma unroll
    for(int k = 0; k < 4; ++k) {
      const int c = c0 + k;
      if(c >= 0 && c < fr.cols) drow[c] = (uint8_t) (word >> (8 * k));
    }
  }
}

void launch_rectify_frames(hipStream_t s, const RectifyFrame* frames, int nframes, int max_rows, int max_cols)
{
  const int groups = (max_cols + 3) / 4 + 1;      // of four columns on the address grid: a row that begins off the grid has one more
  dim3 grid((unsigned) ((groups + 63) / 64), (unsigned) ((max_rows + 3) / 4), (unsigned) nframes);
  hipLaunchKernelGGL(rectify_frames_kernel, grid, dim3(256), 0, s, frames);
}

}  // namespace bpvo_hip
