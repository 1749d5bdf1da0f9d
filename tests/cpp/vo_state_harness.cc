// Test harness: bpvo_amd/csrc/vo_state.h — the addFrame state machine of both drivers in vo.hip — compiled by a plain C++ compiler (no HIP
// anywhere: that it compiles is the proof that the header is host-only), driven the way the drivers drive it, with the estimates, the fraction
// of good points and the frame slots' flags supplied by the test (tests/test_vo_state_cpu.py).
#include "vo_state.h"

using namespace bpvo_hip_host;

namespace {
SeqState g_q;
bool g_data[3], g_tmpl[3];      // the FrameSlot flags the drivers keep
}

extern "C" {

void vs_reset()
{
  vo_reset(g_q, 0);
  for(int k = 0; k < 3; ++k) g_data[k] = g_tmpl[k] = false;
}

// One addFrame.  T_est: the estimate against the key frame; T_again: the one against a new key frame, read where the state machine asks for it;
// fraction_good, cloud_points: what the count and the point-cloud launch would give.
// out = {ref, cur, prev, slot to template or -1, slot to clear or -1, re-estimate asked for}
void vs_add_frame(const bpvo_hip_params* p, int numLevels, const float* T_est, const float* T_again, float fraction_good, size_t cloud_points,
                  bpvo_hip_result* ret, int* out)
{
  SeqState& q = g_q;
  vo_begin_frame(q, numLevels, ret);
  out[3] = out[4] = -1; out[5] = 0;
  g_data[q.cur] = true;      // setData
  if(!g_tmpl[q.ref]) {
    out[3] = vo_first_frame(q);
    g_tmpl[out[3]] = true;   // setTemplate
    vo_first_frame_done(q, ret);
  } else {
    M44 T, T2;
    std::memcpy(T.m, T_est, 64);
    std::memcpy(T2.m, T_again, 64);
    bool again = false;
    if(vo_decide(*p, T, fraction_good, ret)) {
      const KeyFrameSlots ks = vo_keyframe(q, g_data[q.prev], cloud_points, ret);
      if(ks.clear_slot >= 0) g_data[ks.clear_slot] = g_tmpl[ks.clear_slot] = false;
      g_tmpl[ks.template_slot] = true;
      again = ks.reestimate;
      out[3] = ks.template_slot; out[4] = ks.clear_slot; out[5] = ks.reestimate ? 1 : 0;
    }
    vo_finish(q, T, again ? &T2 : nullptr, ret);
  }
  out[0] = q.ref; out[1] = q.cur; out[2] = q.prev;
}

// T_kf, cloud_pose, the trajectory's last pose (untouched while it is empty); returns the trajectory's length
int vs_state(float* T_kf, float* cloud_pose, float* trajectory_back, size_t* cloud_n)
{
  std::memcpy(T_kf, g_q.T_kf.m, 64);
  std::memcpy(cloud_pose, g_q.cloud_pose.m, 64);
  if(!g_q.trajectory.empty()) std::memcpy(trajectory_back, g_q.trajectory.back().m, 64);
  *cloud_n = g_q.cloud_n;
  return (int) g_q.trajectory.size();
}

int vs_keyframe_reason(const bpvo_hip_params* p, const float* T_est, unsigned good_count, int n_points, int C)
{
  M44 T;
  std::memcpy(T.m, T_est, 64);
  return vo_keyframe_reason(*p, T, vo_fraction_good(good_count, n_points, C));
}

void vs_init_result(int numLevels, bpvo_hip_result* ret) { vo_init_result(numLevels, ret); }

}
