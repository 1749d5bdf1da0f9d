// The frame stage's decisions (bpvo_amd/csrc/frame_plan.h) without a GPU: compiled by the host's C++ compiler from that header and the C API alone,
// prints one line per query of its command line (queries separated by a "," argument) — tests/test_frame_plan_cpu.py:
//   form DESCRIPTOR SIGMA_CENSUS SIGMA_BITPLANES C                -> the descriptor form's name
//   merge COUNT MAX_FRAMES TESTED_LEVELS FORM_NAME EVERY_TILED    -> descriptor selection template (0 / 1 each)
//   spans L MAX_TEST_LEVEL MERGED                                 -> first:count ...
//   nrm L MAX_TEST_LEVEL SIDE DEFER DENSE                         -> first-end:stream:event ... | join J pending P finest F behind B
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "bpvo_hip/c_api.h"
#include "frame_plan.h"

using namespace bpvo_hip_host;

static const char* const kFormNames[] = {"bitplanes_fused", "bitplanes_smoothed_census", "bitplanes_unsmoothed", "intensity", "laplacian", "gradient",
                                         "fields_1st", "fields_2nd", "central_difference", "latch"};
static const char* const kStreamNames[] = {"inline", "side", "side2"};

static DescriptorForm form_of(char** a)
{
  bpvo_hip_params p = {};
  p.descriptor = (int) std::strtol(a[0], nullptr, 0);
  p.sigmaPriorToCensusTransform = (float) std::atof(a[1]);
  p.sigmaBitPlanes = (float) std::atof(a[2]);
  return descriptor_form(p, std::atoi(a[3]));
}

static int query(int n, char** a)
{
  if(n == 5 && !std::strcmp(a[0], "form")) {
    std::printf("%s\n", kFormNames[form_of(a + 1)]);
  } else if(n == 6 && !std::strcmp(a[0], "merge")) {
    int form = -1;
    for(int k = 0; k < 10; ++k)
      if(!std::strcmp(a[4], kFormNames[k])) form = k;
    if(form < 0) return 2;
    const int count = std::atoi(a[1]), max_frames = std::atoi(a[2]), tested = std::atoi(a[3]);
    std::printf("%d %d %d\n", (int) merge_descriptor_levels(count, max_frames, tested, (DescriptorForm) form),
                (int) merge_selection_levels(count, max_frames, tested, std::atoi(a[5]) != 0), (int) merge_template_levels(count, max_frames, tested));
  } else if(n == 4 && !std::strcmp(a[0], "spans")) {
    for(const LevelSpan& sp : level_spans(std::atoi(a[1]), std::atoi(a[2]), std::atoi(a[3]) != 0)) std::printf("%d:%d ", sp.first, sp.count);
    std::printf("\n");
  } else if(n == 6 && !std::strcmp(a[0], "nrm")) {
    const NrmPlan p = normalization_plan(std::atoi(a[1]), std::atoi(a[2]), std::atoi(a[3]) != 0, std::atoi(a[4]) != 0, std::atoi(a[5]) != 0);
    for(int k = 0; k < p.n; ++k) std::printf("%d-%d:%s:%d ", p.part[k].first_level, p.part[k].end_level, kStreamNames[p.part[k].stream], p.part[k].event);
    std::printf("| join %d pending %d finest %d behind %d\n", p.join_event, p.pending_event, p.pending_finest_event, (int) p.behind_readback);
  } else {
    return 2;
  }
  return 0;
}

int main(int argc, char** argv)
{
  for(int i = 1; i < argc;) {
    int j = i;
    while(j < argc && std::strcmp(argv[j], ",")) ++j;
    if(int rc = query(j - i, argv + i)) { std::fprintf(stderr, "bad query at argument %d\n", i); return rc; }
    i = j + 1;
  }
  return 0;
}
