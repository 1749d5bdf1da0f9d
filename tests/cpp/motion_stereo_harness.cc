// A main around bpvo_amd/csrc/motion_stereo_math.h (no HIP, no library): the motion-stereo rule of one image pair as a serial loop over the
// pixels, for the comparison with tests/motion_stereo_ref.py, plain and under AddressSanitizer / UBSan.
//   motion_stereo_harness PARAMS FIRST SECOND PD PV OUT   writes OUT.d, OUT.v (f32 [rows][cols]) and OUT.c (u8) and prints the seven class counts
// PARAMS: 28 f64 = rows cols lo hi radius steps min_gain noise_sigma min_sigma max_sigma gate fx fy cx cy b Q[12] (every value but the integers an
// f32 widened).  FIRST, SECOND: u8 [rows][cols]; PD, PV: f32 [rows][cols], a pixel has no prior where PV < 0.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "motion_stereo_math.h"

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

int main(int argc, char** argv)
{
  if(argc != 7) {
    std::fprintf(stderr, "usage: motion_stereo_harness PARAMS FIRST SECOND PD PV OUT\n");
    return 2;
  }
  const std::vector<double> p = read_all<double>(argv[1], 28);
  const int rows = (int) p[0], cols = (int) p[1];
  if(rows < 1 || cols < 1) { std::fprintf(stderr, "bad sizes\n"); return 2; }
  const float lo = (float) p[2], hi = (float) p[3];
  if(const char* why = ms_refusal((int) p[4], (int) p[5], (float) p[6], (float) p[7], (float) p[8], (float) p[9], (float) p[10])) {
    std::fprintf(stderr, "%s\n", why);
    return 2;
  }
  const MsRule rule = ms_rule((int) p[4], (int) p[5], (float) p[6], (float) p[7], (float) p[8], (float) p[9], (float) p[10]);
  const DfCamera cam{(float) p[11], (float) p[12], (float) p[13], (float) p[14], (float) p[15], lo, hi, rows, cols};
  float Q[12];
  for(int k = 0; k < 12; ++k) Q[k] = (float) p[16 + k];
  const MsGeometry geo = ms_geometry(cam, Q);
  const size_t n = (size_t) rows * cols;
  const std::vector<uint8_t> C = read_all<uint8_t>(argv[2], n), K = read_all<uint8_t>(argv[3], n);
  const std::vector<float> PD = read_all<float>(argv[4], n), PV = read_all<float>(argv[5], n);
  std::vector<float> D(n), V(n);
  std::vector<uint8_t> cls(n);
  unsigned long long counts[MS_CLASSES] = {};
  for(int y = 0; y < rows; ++y)
    for(int x = 0; x < cols; ++x) {
      const size_t i = (size_t) y * cols + x;
      const int c = ms_pixel(rule, geo, lo, hi, C.data(), K.data(), rows, cols, x, y, true, PD[i], PV[i], &D[i], &V[i]);
      cls[i] = (uint8_t) c;
      counts[c] += 1;
    }
  const std::string out = argv[6];
  write_all(out + ".d", D);
  write_all(out + ".v", V);
  write_all(out + ".c", cls);
  std::printf("%llu %llu %llu %llu %llu %llu %llu\n", counts[0], counts[1], counts[2], counts[3], counts[4], counts[5], counts[6]);
  return 0;
}
