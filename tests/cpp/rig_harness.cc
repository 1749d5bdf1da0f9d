// Test harness: bpvo_amd/csrc/rig_math.h — the maps of rig mode, shared by the device-side rig step and the host drivers — and the transitions of a
// body (vo_rig_*) of bpvo_amd/csrc/vo_state.h, compiled by a plain C++ compiler and driven the way the batched driver (vo.hip: add_frames_run)
// drives them — a rig with its extrinsics, a sequence with none, the body its own member —, with the estimates, the counts of good points and the
// frame slots' flags supplied by the test (tests/test_rig_cpu.py).  rg_plain_add_frame: the same frame through the plain vo_* calls, as
// add_frame_impl makes them.
#include <vector>

#include "rig_math.h"
#include "vo_state.h"

using namespace bpvo_hip;
using namespace bpvo_hip_host;

namespace {
constexpr int kMaxMembers = 8;
SeqState g_body, g_member[kMaxMembers], g_plain;
bool g_data[3 * kMaxMembers], g_tmpl[3 * kMaxMembers], g_pdata[3], g_ptmpl[3];
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
float rg_fraction_good_null(unsigned good, int n_points, int C) { return vo_rig_fraction_good(&good, &n_points, 1, C); }
float rg_fraction_good_one(unsigned good, int n_points, int C) { return vo_fraction_good(good, n_points, C); }

void rg_reset(int n)
{
  vo_reset(g_body, 0);
  vo_reset(g_plain, 0);
  for(int p = 0; p < n; ++p) vo_reset(g_member[p], 3 * p);
  for(int k = 0; k < 3 * kMaxMembers; ++k) g_data[k] = g_tmpl[k] = false;
  for(int k = 0; k < 3; ++k) g_pdata[k] = g_ptmpl[k] = false;
}

// One frame of a body of n members with extrinsics X — or X null and n = 1: a sequence, the body its own member — through vo_rig_*.
// T_est / T_again: the body estimates; good / n_points: the members' counts.
// out[p] = {ref, cur, prev, slot to template or -1, slot to clear or -1, re-estimate asked for} of member p
void rg_add_frame(const bpvo_hip_params* prm, int numLevels, int n, const float* X, const float* T_est, const float* T_again, const unsigned* good,
                  const int* n_points, int C, const size_t* cloud_points, bpvo_hip_result* ret, int* out)
{
  SeqState* members[kMaxMembers];
  for(int p = 0; p < n; ++p) members[p] = X ? &g_member[p] : &g_body;
  vo_rig_begin_frame(g_body, members, n, numLevels, ret);
  for(int p = 0; p < n; ++p) {
    g_data[members[p]->cur] = true;
    out[6 * p + 3] = out[6 * p + 4] = -1; out[6 * p + 5] = 0;
  }
  if(!g_tmpl[members[0]->ref]) {
    for(int p = 0; p < n; ++p) { out[6 * p + 3] = vo_first_frame(*members[p]); g_tmpl[out[6 * p + 3]] = true; }
    vo_rig_first_frame_done(g_body, members, n, ret);
  } else {
    M44 T, T2;
    std::memcpy(T.m, T_est, 64);
    std::memcpy(T2.m, T_again, 64);
    bool again = false;
    if(vo_decide(*prm, T, vo_rig_fraction_good(good, n_points, n, C), ret)) {
      std::vector<KeyFrameSlots> ks((size_t) n);
      vo_rig_keyframe(members, n, g_data[members[0]->prev], cloud_points, ks.data(), ret);
      for(int p = 0; p < n; ++p) {
        if(ks[p].clear_slot >= 0) g_data[ks[p].clear_slot] = g_tmpl[ks[p].clear_slot] = false;
        g_tmpl[ks[p].template_slot] = true;
        out[6 * p + 3] = ks[p].template_slot; out[6 * p + 4] = ks[p].clear_slot; out[6 * p + 5] = ks[p].reestimate ? 1 : 0;
      }
      again = ks[0].reestimate;
    }
    vo_rig_finish(g_body, members, X, n, T, again ? &T2 : nullptr, ret);
  }
  for(int p = 0; p < n; ++p) { out[6 * p + 0] = members[p]->ref; out[6 * p + 1] = members[p]->cur; out[6 * p + 2] = members[p]->prev; }
}
// The same frame of ONE sequence through the plain calls, in add_frame_impl's order, on a state of its own; out as above
void rg_plain_add_frame(const bpvo_hip_params* prm, int numLevels, const float* T_est, const float* T_again, unsigned good, int n_points, int C,
                        size_t cloud_points, bpvo_hip_result* ret, int* out)
{
  SeqState& q = g_plain;
  vo_begin_frame(q, numLevels, ret);
  g_pdata[q.cur] = true;
  out[3] = out[4] = -1; out[5] = 0;
  if(!g_ptmpl[q.ref]) {
    out[3] = vo_first_frame(q);
    g_ptmpl[out[3]] = true;
    vo_first_frame_done(q, ret);
  } else {
    M44 T, T2;
    std::memcpy(T.m, T_est, 64);
    std::memcpy(T2.m, T_again, 64);
    bool again = false;
    if(vo_decide(*prm, T, vo_fraction_good(good, n_points, C), ret)) {
      const KeyFrameSlots ks = vo_keyframe(q, g_pdata[q.prev], cloud_points, ret);
      if(ks.clear_slot >= 0) g_pdata[ks.clear_slot] = g_ptmpl[ks.clear_slot] = false;
      g_ptmpl[ks.template_slot] = true;
      out[3] = ks.template_slot; out[4] = ks.clear_slot; out[5] = ks.reestimate ? 1 : 0;
      again = ks.reestimate;
    }
    vo_finish(q, T, again ? &T2 : nullptr, ret);
  }
  out[0] = q.ref; out[1] = q.cur; out[2] = q.prev;
}
// the whole SeqState of the body (which = 0) or of rg_plain_add_frame's state (1) as bytes: roles, T_kf, cloud_n, cloud_pose, the trajectory;
// returns the bytes written (cap: the buffer's size)
int rg_state_bytes(int which, unsigned char* out, int cap)
{
  const SeqState& q = which ? g_plain : g_body;
  const int roles[3] = {q.ref, q.cur, q.prev};
  const size_t need = sizeof(roles) + 64 + sizeof(size_t) + 64 + 64 * q.trajectory.size();
  if(need > (size_t) cap) return -1;
  unsigned char* at = out;
  std::memcpy(at, roles, sizeof(roles)); at += sizeof(roles);
  std::memcpy(at, q.T_kf.m, 64); at += 64;
  std::memcpy(at, &q.cloud_n, sizeof(size_t)); at += sizeof(size_t);
  std::memcpy(at, q.cloud_pose.m, 64); at += 64;
  for(const M44& T : q.trajectory) { std::memcpy(at, T.m, 64); at += 64; }
  return (int) need;
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
