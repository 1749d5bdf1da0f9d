// libbpvo_hip, host side: the decisions of the frame stage (frames.hip) — which descriptor kernels a context's parameters ask for, which levels
// share a launch, where the normalisation runs and what waits for it — host only, no HIP, plain values in: tests/cpp/frame_plan_harness.cc prints
// them without a GPU.  Fixed arrays throughout: a stage plans without touching the heap.
#pragma once
#include "../../include/bpvo_hip/c_api.h"

namespace bpvo_hip_host {

// ---- the descriptor kernels of the data stage (DenseDescriptorPyramid::init, dense_descriptor_pyramid.cc:67-71), in the order they are told apart:
// the descriptor's name first, then the channel count C.  Bit-planes (C = 8): the census FUSED into the blur kernel, unless the census is taken
// of the smoothed image (SMOOTHED_CENSUS: the census-and-blur kernel, then the blur of the planes) or the planes stay UNSMOOTHED (the census
// kernel — of the smoothed image where sigmaPriorToCensusTransform > 0 —, then the plain bit-planes kernel)
enum DescriptorForm { DF_BITPLANES_FUSED, DF_BITPLANES_SMOOTHED_CENSUS, DF_BITPLANES_UNSMOOTHED, DF_INTENSITY, DF_LAPLACIAN, DF_GRADIENT,
                      DF_FIELDS_1ST, DF_FIELDS_2ND, DF_CENTRAL_DIFFERENCE, DF_LATCH, DF_INTENSITY_NORM };
// intensity_norm_radius: bpvo_hip_set_intensity_normalization (-1: off).  It is a mode of the Intensity descriptor: where the parameters ask for
// Intensity and the mode is on the plane is the normalised one (DF_INTENSITY_NORM, kernels_intensity_norm.hip), every other form ignores it
inline DescriptorForm descriptor_form(const bpvo_hip_params& p, int C, int intensity_norm_radius = -1)
{
  if(p.descriptor == BPVO_DESC_CENTRAL_DIFFERENCE) return DF_CENTRAL_DIFFERENCE;
  if(p.descriptor == BPVO_DESC_LATCH) return DF_LATCH;
  if(C == 5) return DF_FIELDS_1ST;
  if(C == 10) return DF_FIELDS_2ND;
  if(C == 3) return DF_GRADIENT;
  if(C == 1) return p.descriptor == BPVO_DESC_LAPLACIAN ? DF_LAPLACIAN : (intensity_norm_radius >= 0 ? DF_INTENSITY_NORM : DF_INTENSITY);
  if(!(p.sigmaBitPlanes > 0.0f)) return DF_BITPLANES_UNSMOOTHED;
  return p.sigmaPriorToCensusTransform > 0.0f ? DF_BITPLANES_SMOOTHED_CENSUS : DF_BITPLANES_FUSED;
}

// ---- levels in one launch (kernels_frame.hip level_job).  Few frames: every per-level launch is a latency floor, so a stage of at most
// merge_levels_max_frames frames (option "levels_in_one_launch_max_frames") with more than one tested level runs them in one — where the
// stage's kernels can: the descriptor kernels that read the level from the job (the two blurred bit-planes forms, intensity, normalised intensity), the selection
// when EVERY level is on the tiled path (NMS radius <= 1), the template build always.
inline bool few_frames(int count, int merge_levels_max_frames, int tested_levels) { return count <= merge_levels_max_frames && tested_levels > 1; }
inline bool merge_descriptor_levels(int count, int merge_levels_max_frames, int tested_levels, DescriptorForm form)
{
  return (form == DF_BITPLANES_FUSED || form == DF_BITPLANES_SMOOTHED_CENSUS || form == DF_INTENSITY || form == DF_INTENSITY_NORM) && few_frames(count, merge_levels_max_frames, tested_levels);
}
inline bool merge_selection_levels(int count, int merge_levels_max_frames, int tested_levels, bool every_level_tiled)
{
  return every_level_tiled && few_frames(count, merge_levels_max_frames, tested_levels);
}
inline bool merge_template_levels(int count, int merge_levels_max_frames, int tested_levels) { return few_frames(count, merge_levels_max_frames, tested_levels); }

// the launches of a stage over the tested levels [maxTestLevel, L): one span over all of them, or one per level, coarsest first
struct LevelSpan { int first, count; };
struct LevelSpans {
  int n = 0;
  LevelSpan span[BPVO_HIP_MAX_LEVELS];
  const LevelSpan* begin() const { return span; }
  const LevelSpan* end() const { return span + n; }
};
inline LevelSpans level_spans(int L, int maxTestLevel, bool merged)
{
  LevelSpans s;
  if(merged) s.span[s.n++] = LevelSpan{maxTestLevel, L - maxTestLevel};
  else for(int l = L - 1; l >= maxTestLevel; --l) s.span[s.n++] = LevelSpan{l, 1};
  return s;
}

// ---- the normalisation of a template stage: sequential sums in the reference's order, one workgroup per (frame, level), read by the
// Gauss-Newton kernels only.  In line (no side stream: lanes of a fanned-out batch) it is ONE launch queued behind the read-back of the point
// counts.  On the side stream it forks behind the selection, and the stage joins it (event 1) before it returns.  Deferred (the estimate
// follows on the same stream, more than one tested level): the stage joins the COARSEST level alone; the rest is left pending for the
// estimate — sparse templates: the other levels in a second launch (event 2); parameters that allow a dense level: the finest level first, on
// the second side stream (event 3: its long chain of adds runs under the iterations of all the levels above), the coarsest, then the levels
// between where there are any (event 2).  Events: indices of the context's side_ev (0 is the fork), -1 = none.
// (Measured: the finest level of a dense template is the longest chain of adds, 2 ms for 300 k points, hence its own stream; for sparse templates
// the third launch, the second stream and their events cost a single pair 1 % of its step, hence two launches on one stream.)
enum NrmStream { NRM_INLINE, NRM_SIDE, NRM_SIDE2 };
struct NrmPart { int first_level, end_level; NrmStream stream; int event; };
struct NrmPlan {
  int n = 0;
  NrmPart part[3];
  int join_event = -1;               // the stage's stream waits for it before the stage returns
  int pending_event = -1;            // becomes the context's nrm_pending
  int pending_finest_event = -1;     // ... nrm_pending_finest
  bool behind_readback = false;      // the (in-line) launch is queued behind the read-back of the point counts
};
inline NrmPlan normalization_plan(int L, int maxTestLevel, bool side, bool defer, bool templates_may_be_dense)
{
  NrmPlan p;
  auto add = [&p](int first_level, int end_level, NrmStream stream, int event) { p.part[p.n++] = NrmPart{first_level, end_level, stream, event}; };
  const int lo = maxTestLevel, top = L - 1;
  if(!side) { add(lo, L, NRM_INLINE, -1); p.behind_readback = true; return p; }
  p.join_event = 1;
  if(!defer || top <= lo) { add(lo, L, NRM_SIDE, 1); return p; }
  const int rest = templates_may_be_dense ? lo + 1 : lo;      // the first of the levels left to the second launch on the side stream
  if(templates_may_be_dense) { add(lo, lo + 1, NRM_SIDE2, 3); p.pending_finest_event = 3; }
  add(top, L, NRM_SIDE, 1);
  if(top > rest) { add(rest, top, NRM_SIDE, 2); p.pending_event = 2; }
  return p;
}

}  // namespace bpvo_hip_host
