// A main around bpvo_amd/csrc/disparity_variance_math.h (no HIP, no library): the measurement variance of one pair as a serial loop over the
// pixels, for the comparison with tests/disparity_variance_ref.py, plain and under AddressSanitizer / UBSan.
//   disparity_variance_harness PARAMS LEFT RIGHT M OUT   writes OUT (f32 [rows][cols]) and prints the six class counts
// PARAMS: 8 f64 = rows cols lo hi radius noise_sigma min_sigma max_sigma (every value but rows, cols and radius an f32 widened).
// LEFT, RIGHT: u8 [rows][cols]; M: f32 [rows][cols].
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "disparity_variance_math.h"

using namespace bpvo_hip;

template <class T>
static std::vector<T> read_all(const char* path, size_t want)
{
  std::vector<T> v(want);
  FILE* f = std::fopen(path, "rb");
  if(!f) { std::fprintf(stderr, "cannot open %s\n", path); std::exit(2); }
  const size_t got = std::fread(v.data(), sizeof(T), want, f);
  const bool more = std::fgetc(f) != EOF;
  std::fclose(f);
  if(got != want || more) { std::fprintf(stderr, "%s: expected %zu elements\n", path, want); std::exit(2); }
  return v;
}

int main(int argc, char** argv)
{
  if(argc != 6) {
    std::fprintf(stderr, "usage: disparity_variance_harness PARAMS LEFT RIGHT M OUT\n");
    return 2;
  }
  const std::vector<double> p = read_all<double>(argv[1], 8);
  const int rows = (int) p[0], cols = (int) p[1];
  if(rows < 1 || cols < 1) { std::fprintf(stderr, "bad sizes\n"); return 2; }
  const float lo = (float) p[2], hi = (float) p[3];
  if(const char* why = dv_refusal((int) p[4], (float) p[5], (float) p[6], (float) p[7])) { std::fprintf(stderr, "%s\n", why); return 2; }
  const DvRule rule = dv_rule((int) p[4], (float) p[5], (float) p[6], (float) p[7]);
  const size_t n = (size_t) rows * cols;
  const std::vector<uint8_t> L = read_all<uint8_t>(argv[2], n), R = read_all<uint8_t>(argv[3], n);
  const std::vector<float> M = read_all<float>(argv[4], n);
  std::vector<float> out(n);
  unsigned long long counts[DV_CLASSES] = {};
  for(int y = 0; y < rows; ++y)
    for(int x = 0; x < cols; ++x) {
      const size_t i = (size_t) y * cols + x;
      counts[dv_pixel(rule, lo, hi, L.data(), R.data(), rows, cols, x, y, M[i], &out[i])] += 1;
    }
  FILE* f = std::fopen(argv[5], "wb");
  if(!f || std::fwrite(out.data(), sizeof(float), n, f) != n) { std::fprintf(stderr, "cannot write %s\n", argv[5]); return 2; }
  std::fclose(f);
  std::printf("%llu %llu %llu %llu %llu %llu\n", counts[0], counts[1], counts[2], counts[3], counts[4], counts[5]);
  return 0;
}
