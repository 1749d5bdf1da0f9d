// The finish of the pose score (bpvo_hip_score_poses; include/bpvo_hip/c_api.h states the definition): the score of one pose from its sums, and
// the choice among scored poses.  Shared by the device-side finish (kernels_score.hip), the host (score.hip) and the CPU test
// (tests/test_pose_score_cpu.py compiles this header with a plain C++ compiler).  Everything is f64; the library is built with
// -ffp-contract=off, so the three operations of the score round the same on host and device.
#pragma once

#if defined(__HIPCC__)
#define BPVO_SCORE_HD __host__ __device__ inline
#else
#define BPVO_SCORE_HD inline
#endif

namespace bpvo_hip {

// score = (cost_sum + tau * C * (N - n_valid)) / (C * N): the mean truncated |r| over ALL C * N terms of the template, an invalid point charged
// tau per channel.  C * (N - n_valid) and C * N are exact integers; then one product, one sum, one quotient.  N = 0: tau.
BPVO_SCORE_HD double pose_score_value(double cost_sum, int n_valid, int N, int C, float tau)
{
  if(N <= 0) return (double) tau;
  const double charged = (double) ((long long) C * (long long) (N - n_valid));
  const double terms = (double) ((long long) C * (long long) N);
  return (cost_sum + (double) tau * charged) / terms;
}

// the lowest score, ties to the lowest index; a NaN never wins (every comparison with it is false); all NaN, or n <= 0: 0
BPVO_SCORE_HD int pose_score_argmin(const double* score, int n)
{
  int best = -1;
  for(int i = 0; i < n; ++i) {
    if(score[i] != score[i]) continue;
    if(best < 0 || score[i] < score[best]) best = i;
  }
  return best < 0 ? 0 : best;
}

}  // namespace bpvo_hip
