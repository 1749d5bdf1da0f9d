// The scale of the Student-t loss (BPVO_LOSS_STUDENT_T; include/bpvo_hip/c_api.h states the definition): the term of the map T, the existence rule,
// the stop rule and the freeze decision.  Shared by the device-side fit (gn_tscale.h: tscale_kernel) and the CPU harness
// (tests/cpp/tscale_harness.cc compiles this header with a plain C++ compiler); no HIP types.  The library is built with -ffp-contract=off, so
// the operations below stay apart on host and device.
#pragma once

#include <math.h>

#if defined(__HIPCC__)
#define BPVO_TSCALE_HD __host__ __device__ inline
#else
#define BPVO_TSCALE_HD inline
#endif

namespace bpvo_hip {

constexpr float kTScaleNu = 5.0f;            // degrees of freedom, fixed
constexpr int kTScaleMaxPasses = 64;         // termination guard of the plain iteration
constexpr double kTScaleStopRel = 1e-4;      // |sigma_{k+1} - sigma_k| <= kTScaleStopRel * sigma_k
constexpr double kTScaleFloor = 1e-6;        // a scale below it reads 1 (mestimator.cc:452-490: the reference's answer to a vanishing scale)

// one term of T(s) = ((nu + 1) / n) * sum r^2 s / (nu s + r^2), f32; s > 0: no division by zero at r = 0
BPVO_TSCALE_HD float tscale_term(float r, float s)
{
  const float r2 = r * r;
  return (r2 * s) / (kTScaleNu * s + r2);
}
// one term of the cold start s_0 = mean r^2
BPVO_TSCALE_HD float tscale_square(float r) { return r * r; }

// a positive fixed point exists iff (nu + 1) m > n: n entries, m of them non-zero (T(s) / s -> (nu + 1) m / n as s -> 0)
BPVO_TSCALE_HD bool tscale_exists(unsigned long long n, unsigned long long m) { return n > 0ull && 6ull * m > n; }

// The iteration s_{k+1} = T(s_k), sigma_k = sqrt(s_k), in f64 from the f64 sum of a pass's terms.
struct TScaleFit {
  double s, sigma;      // s_k and sigma_k: what the next pass is evaluated at, and after the last pass the result
  int passes;           // passes taken so far (k + 1)
  int done;             // the stop rule held, the guard was reached, or s fell below the floor (the result then reads 1)
  int stopped_first;    // the FIRST pass already satisfied the stop rule (the freeze decision's input)
};
BPVO_TSCALE_HD void tscale_start(TScaleFit& f, double s0)
{
  f.s = s0; f.sigma = sqrt(s0); f.passes = 0; f.done = 0; f.stopped_first = 0;
}
BPVO_TSCALE_HD void tscale_step(TScaleFit& f, double term_sum, unsigned long long n)
{
  const double s1 = (((double) kTScaleNu + 1.0) / (double) n) * term_sum;
  const double sigma1 = sqrt(s1);
  const bool stop = fabs(sigma1 - f.sigma) <= kTScaleStopRel * f.sigma;
  f.passes += 1;
  if(stop && f.passes == 1) f.stopped_first = 1;
  // (the iteration is monotone: an s below the floor's square never comes back above it)
  f.done = (stop || f.passes >= kTScaleMaxPasses || !(s1 >= kTScaleFloor * kTScaleFloor)) ? 1 : 0;
  f.s = s1; f.sigma = sigma1;
}

// What the stage leaves in the state: the scale, AutoScaleEstimator's delta (<= 1e-6: frozen for the rest of the level), whether it froze.
struct TScaleOut { float scale, delta_scale; int frozen; };
// no fixed point (n == 0, (nu + 1) m <= n, a start or a result below the floor): sigma = 1, and the delta the median stage would store
BPVO_TSCALE_HD TScaleOut tscale_commit_none(float sigma_prev)
{
  TScaleOut o;
  o.scale = 1.0f;
  o.delta_scale = fabsf(1.0f - sigma_prev);
  o.frozen = !(o.delta_scale > 1e-6f) ? 1 : 0;
  return o;
}
// have_prev: the fit started at sigma_prev^2 (the level held an estimated scale); otherwise at mean r^2
BPVO_TSCALE_HD TScaleOut tscale_commit(const TScaleFit& f, bool have_prev, float sigma_prev)
{
  const float sigma = (float) f.sigma;
  if(!((double) sigma >= kTScaleFloor)) return tscale_commit_none(sigma_prev);
  TScaleOut o;
  if(have_prev && f.stopped_first) {      // frozen: sigma_prev stays, bit for bit
    o.scale = sigma_prev; o.delta_scale = 0.0f; o.frozen = 1;
    return o;
  }
  o.scale = sigma;
  o.delta_scale = fabsf(sigma - sigma_prev);
  if(!(o.delta_scale > 1e-6f)) o.delta_scale = 2e-6f;      // "not frozen" stays true
  o.frozen = 0;
  return o;
}

}  // namespace bpvo_hip
