// libbpvo_hip, device side: disparity fusion — the carried disparity and variance maps of a sequence predicted into the new frame (splat) and
// fused with the measured map (update).  disparity_fusion_math.h states the rule; disparity_fusion.hip keeps the maps and fills the job table.
#include <cfloat>

#include "kernels.h"
#include "disparity_fusion_math.h"

namespace bpvo_hip {

static __device__ __forceinline__ DfCamera fusion_camera(const FusionJob& j)
{
  return DfCamera{j.fx, j.fy, j.cx, j.cy, j.b, j.lo, j.hi, j.rows, j.cols};
}

// Splat: all the sequences of a call in one launch — job blockIdx.y is the row of the table (uniform: scalar loads), the grid covers the
// largest frame, and the workgroups beyond their own frame leave at once (no barrier in the kernel).  A lane takes four consecutive source
// pixels of the row-major scan: one 16-byte load of Dc and one of Vc (the carried maps are allocations of their own, so pixel 4 i is 16-byte
// aligned), the wavefront's loads 1 KiB contiguous each.  Every surviving candidate is ONE 64-bit max atomic, without return, into the job's
// z-buffer; for the small motions of consecutive frames neighbouring lanes hit neighbouring targets, so a wavefront's atomics of one source
// column k fall on 8-byte words 32 bytes apart within a row of the target.  The maximum of the keys is what the buffer holds at the end of the
// launch, whatever order the lanes arrive in (disparity_fusion_math.h).  No LDS.
__global__ __launch_bounds__(256) void fusion_splat_kernel(const FusionJob* __restrict__ jobs)
{
  const FusionJob& j = jobs[blockIdx.y];
  if(!j.predict) return;
  const size_t npix = (size_t) j.rows * (size_t) j.cols;
  const size_t i0 = ((size_t) blockIdx.x * 256 + threadIdx.x) * 4;
  if(i0 >= npix) return;
  const DfCamera cam = fusion_camera(j);
  float P[12];
#pragma unroll
  for(int k = 0; k < 12; ++k) P[k] = j.P[k];
  float d[4], v[4];
  if(i0 + 4 <= npix) {
    const float4 d4 = *reinterpret_cast<const float4*>(j.Dc + i0);
    const float4 v4 = *reinterpret_cast<const float4*>(j.Vc + i0);
    d[0] = d4.x; d[1] = d4.y; d[2] = d4.z; d[3] = d4.w;
    v[0] = v4.x; v[1] = v4.y; v[2] = v4.z; v[3] = v4.w;
  } else {
#pragma unroll
    for(int k = 0; k < 4; ++k) {
      const bool in = i0 + k < npix;
      d[k] = in ? j.Dc[i0 + k] : 0.0f;
      v[k] = in ? j.Vc[i0 + k] : -1.0f;      // (carries nothing: dropped)
    }
  }
  int y = (int) (i0 / (size_t) j.cols);
  int x = (int) (i0 - (size_t) y * (size_t) j.cols);
#pragma unroll
  for(int k = 0; k < 4; ++k) {
    int target;
    uint64_t key;
    if(df_splat(cam, P, j.q2, x, y, d[k], v[k], &target, &key))      // (target within [0, rows * cols): df_splat's inside test)
      (void) atomicMax(j.zbuf + target, (unsigned long long) key);
    if(++x == j.cols) { x = 0; ++y; }
  }
}

// Update: per pixel, the measured disparity (the slot's) and the target's z-buffer word in, the fused disparity out to the slot and to the
// carried map, the variance to the carried map, and ZERO back to a word that held a candidate — the buffer is all zero again when the launch
// ends, so no memset runs per call.  A workgroup takes kUpdatePixels consecutive pixels, a lane every 256th of them (the slot's map is a view
// into the slot's slab, of any 4-byte alignment): a wavefront instruction reads 256 or 512 contiguous bytes and writes 256.
// With a variance map (FusionJob::R) a pixel's r2 is its entry of the map, one more contiguous 256-byte read.  The classes are counted
// exactly, in integers: a ballot per class and pixel round into wave-uniform counts, the four wavefronts' counts summed in LDS, then
// one integer atomic per workgroup and class that occurred (a first form with one atomic per wavefront, class and 64 pixels spent its time
// queueing on the five counters of a job: 69 us for one 640 x 480 map).
constexpr int kUpdateRounds = 8;
constexpr int kUpdatePixels = 256 * kUpdateRounds;
__global__ __launch_bounds__(256) void fusion_update_kernel(const FusionJob* __restrict__ jobs)
{
  __shared__ unsigned block_counts[DF_CLASSES];
  const FusionJob& j = jobs[blockIdx.y];
  const size_t npix = (size_t) j.rows * (size_t) j.cols;
  const size_t base = (size_t) blockIdx.x * kUpdatePixels;
  if(base >= npix) return;      // (the whole workgroup: no barrier has been passed)
  if(threadIdx.x < DF_CLASSES) block_counts[threadIdx.x] = 0;
  __syncthreads();
  DfRule rule{j.r2, j.q2, j.gate, j.fill2};
  const float lo = j.lo, hi = j.hi;
  const float* __restrict__ R = j.R;      // (null: the job's r2 for every pixel)
  unsigned counts[DF_CLASSES] = {};
#pragma unroll
  for(int r = 0; r < kUpdateRounds; ++r) {
    const size_t i = base + (size_t) r * 256 + threadIdx.x;
    int cls = -1;
    if(i < npix) {
      const float m = j.slot[i];
      const unsigned long long word = j.zbuf[i];
      if(R) {      // (the measurement's own variance where the map holds one; NaN fails the first comparison)
        const float r = R[i];
        rule.r2 = r > 0.0f && r <= FLT_MAX ? r : j.r2;
      }
      float D, V;
      cls = df_update(rule, lo, hi, m, (uint64_t) word, &D, &V);
      j.slot[i] = D;
      j.Dc[i] = D;
      j.Vc[i] = V;
      if(word != 0) j.zbuf[i] = 0;
    }
#pragma unroll
    for(int k = 0; k < DF_CLASSES; ++k) counts[k] += (unsigned) __popcll(__ballot(cls == k));
  }
  if((threadIdx.x & 63) == 0) {
#pragma unroll
    for(int k = 0; k < DF_CLASSES; ++k)
      if(counts[k]) atomicAdd(&block_counts[k], counts[k]);
  }
  __syncthreads();
  if(threadIdx.x < DF_CLASSES && block_counts[threadIdx.x]) atomicAdd(j.counts + threadIdx.x, block_counts[threadIdx.x]);
}

static dim3 fusion_grid(size_t max_pixels, int per_lane, int njobs)
{
  const size_t lanes = (max_pixels + (size_t) per_lane - 1) / (size_t) per_lane;
  return dim3((unsigned) ((lanes + 255) / 256), (unsigned) njobs);
}
void launch_fusion_splat(hipStream_t s, const FusionJob* jobs, int njobs, size_t max_pixels)
{
  hipLaunchKernelGGL(fusion_splat_kernel, fusion_grid(max_pixels, 4, njobs), dim3(256), 0, s, jobs);
}
void launch_fusion_update(hipStream_t s, const FusionJob* jobs, int njobs, size_t max_pixels)
{
  hipLaunchKernelGGL(fusion_update_kernel, fusion_grid(max_pixels, kUpdateRounds, njobs), dim3(256), 0, s, jobs);
}

}  // namespace bpvo_hip
