// Test harness: bpvo_amd/csrc/warp_rule.h — where a template point lands and whether it is valid there, the one statement every Gauss-Newton
// kernel path calls — compiled by a plain C++ compiler and run over an array of points (tests/test_warp_rule_cpu.py).
#include "warp_rule.h"

using namespace bpvo_hip;

namespace {
template <int LO, int HI>
void run_f64(const float* P_in, const float* X, int n, int W, int R, int* xi, int* yi, unsigned char* valid, double* xf, double* yf)
{
  float P[12];
  for(int k = 0; k < 12; ++k) P[k] = P_in[k];
  for(int i = 0; i < n; ++i) {
    const WarpFoot f = warp_foot<LO, HI>(P, X[4 * i], X[4 * i + 1], X[4 * i + 2], X[4 * i + 3], W, R);
    xi[i] = f.xi; yi[i] = f.yi; valid[i] = f.valid ? 1 : 0; xf[i] = f.xf; yf[i] = f.yf;
  }
}
}

extern "C" {

// the f64 rule with the borders of kLinear / cosine (0, 1) and of the 4 x 4 footprints (1, 3); P: 3 x 4 row-major, X: [n][4]
void wr_foot_0_1(const float* P, const float* X, int n, int W, int R, int* xi, int* yi, unsigned char* valid, double* xf, double* yf)
{
  run_f64<0, 1>(P, X, n, W, R, xi, yi, valid, xf, yf);
}
void wr_foot_1_3(const float* P, const float* X, int n, int W, int R, int* xi, int* yi, unsigned char* valid, double* xf, double* yf)
{
  run_f64<1, 3>(P, X, n, W, R, xi, yi, valid, xf, yf);
}

// the f32 rule; dspace != 0: disparity-space points, (cx, cy) added; cf: [n][4]
void wr_foot_f32(const float* P_in, const float* X, int n, int dspace, float cx, float cy, int W, int R, int* xi, int* yi, unsigned char* valid,
                 float* cf)
{
  float P[12];
  for(int k = 0; k < 12; ++k) P[k] = P_in[k];
  for(int i = 0; i < n; ++i) {
    const WarpFootF32 f = warp_foot_f32(P, X[4 * i], X[4 * i + 1], X[4 * i + 2], X[4 * i + 3], dspace != 0, cx, cy, W, R);
    xi[i] = f.xi; yi[i] = f.yi; valid[i] = f.valid ? 1 : 0;
    for(int k = 0; k < 4; ++k) cf[4 * i + k] = f.cf[k];
  }
}

}
