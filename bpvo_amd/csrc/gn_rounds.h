// libbpvo_hip, host side: the pipelined rounds of the four-kernel chain (estimate.hip) — host only, no HIP: tests/cpp/gn_rounds_harness.cc drives
// run_rounds against a fake device without a GPU.
//
// At most maxIterations + 2 linearisations per level (pose_estimator_base.h:373-393); the state machine on the device enforces the limits, the
// host queues rounds of kItersPerSync iterations until the device reports nothing active.  Every round ends with its flags — cameras: a
// compaction of the list of still-active workspaces (ActiveSet, kernels.h) and the copy of its count; rigs: the bodies' `active` words — queued
// into slot round % 3.  The rounds are PIPELINED: round r + 1 is queued with what came out of round r - 1, as soon as that has landed — the
// device never waits for the host (a synchronisation per round was a ~30 us bubble: 7 % of a round at 128 pairs, 11 % for a single pair).
// Workspaces that finished in between are still dispatched for one more round (their workgroups exit on the first load), and the level ends
// with one round of empty launches.
#pragma once
#include <algorithm>

namespace bpvo_hip_host {

constexpr int kMaxFunEvals = 6 * 200;   // PoseEstimatorParameters::maxFuncEvals, which AlgorithmParameters does not reach (Q4)
constexpr int kItersPerSync = 4;

// at most min(maxIterations + 2, maxFuncEvals) linearisations per level (pose_estimator_base.h:373-393)
inline int max_linearizations(int max_iterations) { return std::min(std::max(max_iterations, 0) + 2, kMaxFunEvals); }
// ... in rounds of kItersPerSync, plus the round queued before the last flags were read and the empty one
inline int max_rounds(int max_iterations) { return (max_linearizations(max_iterations) + kItersPerSync - 1) / kItersPerSync + 2; }

// The rounds of one pyramid level.  Each callable but `read` returns 0 or the error that ends the level (returned as it is):
//   queue_iterations(round)  queues the round's kItersPerSync iterations, with what the last `read` left
//   queue_flags(slot)        queues the round's flags into `slot` and marks the slot
//   wait(slot)               returns once the slot's mark has passed
//   read(slot) -> bool       takes the slot's flags in (cameras: the count, the active list, "none estimates its scale any more"); false: nothing
//                            is active any more (the round just queued runs empty)
template <class QueueIterations, class QueueFlags, class Wait, class Read>
int run_rounds(int max_iterations, QueueIterations&& queue_iterations, QueueFlags&& queue_flags, Wait&& wait, Read&& read)
{
  const int rounds = max_rounds(max_iterations);
  for(int round = 0; round < rounds; ++round) {
    if(int rc = queue_iterations(round)) return rc;
    if(int rc = queue_flags(round % 3)) return rc;
    if(round == 0) continue;              // nothing to learn yet: queue the second round behind the first
    const int prev = (round - 1) % 3;
    if(int rc = wait(prev)) return rc;
    if(!read(prev)) break;
  }
  return 0;
}

}  // namespace bpvo_hip_host
