// The scale of the Student-t loss in its serial form, from bpvo_amd/csrc/tscale_math.h alone (no GPU, no HIP): the same term, existence rule, stop
// rule and freeze decision the device-side fit uses, the sums taken one entry after the other in f64.
//   tscale_harness <file of raw f32 residuals> <have_prev 0|1> <sigma_prev>
// prints: exists frozen passes sigma delta_scale
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "tscale_math.h"

using namespace bpvo_hip;

int main(int argc, char** argv)
{
  if(argc != 4) { std::fprintf(stderr, "usage: %s <f32 file> <have_prev> <sigma_prev>\n", argv[0]); return 2; }
  std::vector<float> r;
  {
    std::FILE* f = std::fopen(argv[1], "rb");
    if(!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    float buf[4096];
    size_t got;
    while((got = std::fread(buf, sizeof(float), 4096, f)) > 0) r.insert(r.end(), buf, buf + got);
    std::fclose(f);
  }
  const bool have_prev = std::atoi(argv[2]) != 0;
  const float sigma_prev = (float) std::atof(argv[3]);

  const unsigned long long n = r.size();
  unsigned long long m = 0;
  for(size_t i = 0; i < r.size(); ++i) m += r[i] != 0.0f ? 1ull : 0ull;
  double s0 = (double) sigma_prev * (double) sigma_prev;
  if(!have_prev) {
    double sq = 0.0;
    for(size_t i = 0; i < r.size(); ++i) sq += (double) tscale_square(r[i]);
    s0 = n ? sq / (double) n : 0.0;
  }
  const bool exists = tscale_exists(n, m) && s0 >= kTScaleFloor * kTScaleFloor;
  TScaleFit fit;
  tscale_start(fit, exists ? s0 : 1.0);
  if(exists) {
    do {
      const float sf = (float) fit.s;
      double sum = 0.0;
      for(size_t i = 0; i < r.size(); ++i) sum += (double) tscale_term(r[i], sf);
      tscale_step(fit, sum, n);
    } while(!fit.done);
  }
  const TScaleOut o = exists ? tscale_commit(fit, have_prev, sigma_prev) : tscale_commit_none(sigma_prev);
  std::printf("%d %d %d %.9g %.9g\n", exists ? 1 : 0, o.frozen, exists ? fit.passes : 0, (double) o.scale, (double) o.delta_scale);
  return 0;
}
