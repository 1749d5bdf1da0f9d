// Test harness: bpvo_amd/csrc/rig_math.h — the maps of rig mode, shared by the device-side rig step and the host drivers — and the rig additions to
// bpvo_amd/csrc/vo_state.h, compiled by a plain C++ compiler and driven the way bpvo_hip_add_frames_rig drives them, with the estimates, the counts
// of good points and the frame slots' flags supplied by the test (tests/test_rig_cpu.py).
#include <vector>

#include "rig_math.h"
#include "vo_state.h"

using namespace bpvo_hip;
using namespace bpvo_hip_host;

namespace {
constexpr int kMaxMembers = 8;
SeqState g_body, g_member[kMaxMembers];
bool g_data[3 * kMaxMembers], g_tmpl[3 * kMaxMembers];
}

extern "C" {

void rg_adjoint(const float* X, double* Ad) { rig_adjoint(X, Ad); }
void rg_normalization_map(const float* nrm, double* A) { rig_normalization_map(nrm, A); }
void rg_normalization_map_inverse(const float* nrm, double* Ai) { rig_normalization_map_inverse(nrm, Ai); }
void rg_body_map(const float* X, const float* nrm, double* B) { rig_body_map(X, nrm, B); }
void rg_congruence(const double* B, const float* H, const float* G, double* Hb, double* Gb) { rig_congruence(B, H, G, Hb, Gb); }
void rg_member_pose(const float* X, const float* T, float* Tp) { rig_member_pose(X, T, Tp); }
void rg_cloud_pose(const float* W, const float* X, float* out) { rig_cloud_pose(W, X, out); }
int rg_extrinsic_ok(const float* X) { return rig_extrinsic_ok(X) ? 1 : 0; }
float rg_fraction_good(const unsigned* good, const int* n_points, int n, int C) { return vo_rig_fraction_good(good, n_points, n, C); }
float rg_fraction_good_one(unsigned good, int n_points, int C) { return vo_fraction_good(good, n_points, C); }

void rg_reset(int n)
{
  vo_reset(g_body, 0);
  for(int p = 0; p < n; ++p) vo_reset(g_member[p], 3 * p);
  for(int k = 0; k < 3 * kMaxMembers; ++k) g_data[k] = g_tmpl[k] = false;
}

// One bpvo_hip_add_frames_rig of n members with extrinsics X.  T_est / T_again: the body estimates; good / n_points: the members' counts.
// out[p] = {ref, cur, prev, slot to template or -1, slot to clear or -1, re-estimate asked for} of member p
void rg_add_frame(const bpvo_hip_params* prm, int numLevels, int n, const float* X, const float* T_est, const float* T_again, const unsigned* good,
                  const int* n_points, int C, const size_t* cloud_points, bpvo_hip_result* ret, int* out)
{
  SeqState* members[kMaxMembers];
  for(int p = 0; p < n; ++p) members[p] = &g_member[p];
  vo_begin_frame(g_body, numLevels, ret);
  for(int p = 0; p < n; ++p) {
    bpvo_hip_result own;
    vo_begin_frame(g_member[p], numLevels, &own);
    g_data[g_member[p].cur] = true;
    out[6 * p + 3] = out[6 * p + 4] = -1; out[6 * p + 5] = 0;
  }
  if(!g_tmpl[g_member[0].ref]) {
    for(int p = 0; p < n; ++p) { out[6 * p + 3] = vo_first_frame(g_member[p]); g_tmpl[out[6 * p + 3]] = true; }
    vo_rig_first_frame_done(g_body, members, n, ret);
  } else {
    M44 T, T2;
    std::memcpy(T.m, T_est, 64);
    std::memcpy(T2.m, T_again, 64);
    bool again = false;
    if(vo_decide(*prm, T, vo_rig_fraction_good(good, n_points, n, C), ret)) {
      std::vector<KeyFrameSlots> ks((size_t) n);
      vo_rig_keyframe(members, n, g_data[g_member[0].prev], cloud_points, ks.data(), ret);
      for(int p = 0; p < n; ++p) {
        if(ks[p].clear_slot >= 0) g_data[ks[p].clear_slot] = g_tmpl[ks[p].clear_slot] = false;
        g_tmpl[ks[p].template_slot] = true;
        out[6 * p + 3] = ks[p].template_slot; out[6 * p + 4] = ks[p].clear_slot; out[6 * p + 5] = ks[p].reestimate ? 1 : 0;
      }
      again = ks[0].reestimate;
    }
    vo_rig_finish(g_body, members, X, n, T, again ? &T2 : nullptr, ret);
  }
  for(int p = 0; p < n; ++p) { out[6 * p + 0] = g_member[p].ref; out[6 * p + 1] = g_member[p].cur; out[6 * p + 2] = g_member[p].prev; }
}

// member < 0: the body.  T_kf, cloud_pose, the trajectory's last pose; returns the trajectory's length
int rg_state(int member, float* T_kf, float* cloud_pose, float* trajectory_back, size_t* cloud_n)
{
  const SeqState& q = member < 0 ? g_body : g_member[member];
  std::memcpy(T_kf, q.T_kf.m, 64);
  std::memcpy(cloud_pose, q.cloud_pose.m, 64);
  if(!q.trajectory.empty()) std::memcpy(trajectory_back, q.trajectory.back().m, 64);
  *cloud_n = q.cloud_n;
  return (int) q.trajectory.size();
}

}
