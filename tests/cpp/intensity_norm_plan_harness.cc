// The frame stage's decisions for the normalised intensity (bpvo_amd/csrc/frame_plan.h), host only:
//   intensity_norm_plan_harness <descriptor> <C> <radius> <count> <max_frames> <tested_levels>
// prints "<form with the radius> <form without> <levels merged with> <levels merged without>": the enumerators as integers, the predicates as 0 / 1.
#include <cstdio>
#include <cstdlib>

#include "frame_plan.h"

using namespace bpvo_hip_host;

int main(int argc, char** argv)
{
  if(argc != 7) return 2;
  bpvo_hip_params p = {};
  p.sigmaBitPlanes = 0.5f;
  p.descriptor = std::atoi(argv[1]);
  const int C = std::atoi(argv[2]), radius = std::atoi(argv[3]), count = std::atoi(argv[4]), max_frames = std::atoi(argv[5]), tested = std::atoi(argv[6]);
  const DescriptorForm with = descriptor_form(p, C, radius), without = descriptor_form(p, C);
  std::printf("%d %d %d %d\n", (int) (with == DF_INTENSITY_NORM), (int) (without == DF_INTENSITY), (int) merge_descriptor_levels(count, max_frames, tested, with),
              (int) merge_descriptor_levels(count, max_frames, tested, without));
  return 0;
}
