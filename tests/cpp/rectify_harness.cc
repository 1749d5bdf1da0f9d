// A main around bpvo_amd/csrc/rectify_math.h (no HIP, no library): the map of a lens or of a caller's f32 maps, the integer remap of a raw image
// and the count of outside pixels, as the library's host code and kernel form them — for the comparison with tests/rectify_ref.py, plain and under
// AddressSanitizer / UBSan, and for the single-thread host timing of scripts/rectify_bench.py.
//   rectify_harness lens  PARAMS RAW OUT         PARAMS: 29 f64 = rows cols raw_rows raw_cols fx' fy' cx' cy' fx fy cx cy dist[8] R[9]
//   rectify_harness maps  PARAMS MAPX MAPY RAW OUT   PARAMS: 4 f64 = rows cols raw_rows raw_cols; MAPX / MAPY: f32 [rows][cols]
//   rectify_harness bench PARAMS FRAMES PASSES   the remap loop alone over FRAMES pseudo-random raw frames, PASSES times: seconds per frame of each pass
// RAW: u8 [raw_rows][raw_cols].  Writes OUT.map (int32 xq yq per pixel) and OUT.img (u8 [rows][cols]); prints the outside count.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "rectify_math.h"

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
template <class T>
static void write_all(const std::string& path, const std::vector<T>& v)
{
  FILE* f = std::fopen(path.c_str(), "wb");
  if(!f || std::fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) { std::fprintf(stderr, "cannot write %s\n", path.c_str()); std::exit(2); }
  std::fclose(f);
}
struct Sizes { int rows, cols, raw_rows, raw_cols; };
static Sizes sizes_of(const std::vector<double>& p)
{
  const Sizes s{(int) p[0], (int) p[1], (int) p[2], (int) p[3]};
  if(s.rows < 1 || s.cols < 1 || s.raw_rows < 1 || s.raw_cols < 1 || s.raw_rows > kRectMaxRaw || s.raw_cols > kRectMaxRaw) { std::fprintf(stderr, "bad sizes\n"); std::exit(2); }
  return s;
}
static std::vector<RectEntry> lens_entries(const std::vector<double>& p, const Sizes& s)
{
  RectLens q;
  q.fx = p[8]; q.fy = p[9]; q.cx = p[10]; q.cy = p[11];
  for(int k = 0; k < 8; ++k) q.dist[k] = p[12 + k];
  for(int k = 0; k < 9; ++k) q.R[k] = p[20 + k];
  std::vector<RectEntry> e((size_t) s.rows * s.cols);
  for(int v = 0; v < s.rows; ++v)
    for(int u = 0; u < s.cols; ++u) e[(size_t) v * s.cols + u] = rect_lens_entry(q, p[4], p[5], p[6], p[7], u, v);
  return e;
}
static void remap(const std::vector<RectEntry>& e, const Sizes& s, const uint8_t* raw, uint8_t* out)
{
  for(size_t i = 0; i < e.size(); ++i) out[i] = rectify_pixel(raw, s.raw_rows, s.raw_cols, e[i].xq, e[i].yq);
}
static int finish(const std::vector<RectEntry>& e, const Sizes& s, const char* raw_path, const std::string& out)
{
  const std::vector<uint8_t> raw = read_all<uint8_t>(raw_path, (size_t) s.raw_rows * s.raw_cols);
  std::vector<uint8_t> img(e.size());
  remap(e, s, raw.data(), img.data());
  unsigned long long outside = 0;
  std::vector<int32_t> words(2 * e.size());
  for(size_t i = 0; i < e.size(); ++i) {
    outside += rectify_outside(s.raw_rows, s.raw_cols, e[i].xq, e[i].yq) ? 1u : 0u;
    words[2 * i] = e[i].xq; words[2 * i + 1] = e[i].yq;
  }
  write_all(out + ".map", words);
  write_all(out + ".img", img);
  std::printf("%llu\n", outside);
  return 0;
}

int main(int argc, char** argv)
{
  const std::string mode = argc > 1 ? argv[1] : "";
  if(mode == "lens" && argc == 5) {
    const std::vector<double> p = read_all<double>(argv[2], 29);
    const Sizes s = sizes_of(p);
    return finish(lens_entries(p, s), s, argv[3], argv[4]);
  }
  if(mode == "maps" && argc == 7) {
    const std::vector<double> p = read_all<double>(argv[2], 4);
    const Sizes s = sizes_of(p);
    const size_t n = (size_t) s.rows * s.cols;
    const std::vector<float> mx = read_all<float>(argv[3], n), my = read_all<float>(argv[4], n);
    std::vector<RectEntry> e(n);
    for(size_t i = 0; i < n; ++i) e[i] = rect_quantise((double) mx[i], (double) my[i]);
    return finish(e, s, argv[5], argv[6]);
  }
  if(mode == "bench" && argc == 5) {
    const std::vector<double> p = read_all<double>(argv[2], 29);
    const Sizes s = sizes_of(p);
    const int frames = std::atoi(argv[3]), passes = std::atoi(argv[4]);
    if(frames < 1 || passes < 1) return 2;
    const std::vector<RectEntry> e = lens_entries(p, s);
    const size_t raw_n = (size_t) s.raw_rows * s.raw_cols;
    std::vector<uint8_t> raw(raw_n * frames), img(e.size() * frames);
    uint32_t x = 12345u;
    for(size_t i = 0; i < raw.size(); ++i) { x = x * 1664525u + 1013904223u; raw[i] = (uint8_t) (x >> 24); }
    unsigned sum = 0;
    for(int k = 0; k <= passes; ++k) {      // (pass 0 warms up)
      const auto t0 = std::chrono::steady_clock::now();
      for(int f = 0; f < frames; ++f) remap(e, s, raw.data() + raw_n * f, img.data() + e.size() * f);
      const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      sum += img[(size_t) k % img.size()];
      if(k > 0) std::printf("%.9f\n", dt / frames);
    }
    std::fprintf(stderr, "checksum %u\n", sum);
    return 0;
  }
  std::fprintf(stderr, "usage: rectify_harness lens PARAMS RAW OUT | maps PARAMS MAPX MAPY RAW OUT | bench PARAMS FRAMES PASSES\n");
  return 2;
}
