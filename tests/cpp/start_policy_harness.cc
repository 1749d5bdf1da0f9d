// Test harness: the start policy of bpvo_amd/csrc/vo_state.h ("where an estimate starts") compiled by a plain C++ compiler — no HIP anywhere — and
// driven the way the drivers in vo.hip drive it (tests/test_start_policy_cpu.py): one body whose T_kf, last motion, policy and hints the test
// sets, the candidate lists, the choice from given records, the refusals, and the pooled score of a rig.
#include "vo_state.h"

using namespace bpvo_hip_host;

namespace {
SeqState g_q;
}

extern "C" {

void sp_reset() { vo_reset(g_q, 0); }
// a frame that estimated: vo_finish with the estimate T_est against the key frame (no key frame: T_kf becomes T_est, M the frame-to-frame pose)
void sp_finish(const float* T_est)
{
  bpvo_hip_result ret;
  vo_init_result(3, &ret);
  M44 T;
  std::memcpy(T.m, T_est, 64);
  vo_finish(g_q, T, nullptr, &ret);
}
void sp_begin_frame()
{
  bpvo_hip_result ret;
  vo_begin_frame(g_q, 3, &ret);
}
void sp_set_state(const float* T_kf, const float* M)
{
  std::memcpy(g_q.T_kf.m, T_kf, 64);
  std::memcpy(g_q.M.m, M, 64);
}
void sp_get_state(float* T_kf, float* M, int* n_hints, bpvo_hip_start_policy* policy, int* own)
{
  std::memcpy(T_kf, g_q.T_kf.m, 64);
  std::memcpy(M, g_q.M.m, 64);
  *n_hints = (int) g_q.hints.size();
  *policy = g_q.policy;
  *own = g_q.own_policy ? 1 : 0;
}
// 0, or 1 with the policy refused and the earlier one kept (numLevels 3, maxTestLevel 0)
int sp_set_policy(const bpvo_hip_start_policy* pol)
{
  if(vo_start_policy_refusal(*pol, 3, 0)) return 1;
  g_q.policy = *pol;
  g_q.own_policy = true;
  return 0;
}
int sp_set_hints(int n, const float* M)
{
  if(vo_start_hints_refusal(g_q.policy, n, M)) return 1;
  vo_set_start_hints(g_q, n, M);
  return 0;
}
// the candidates of estimate `which`: their number; poses [16][16] and kinds [16] filled up to it
int sp_candidates(int which, float* poses, int* kinds)
{
  const StartCandidates sc = vo_start_candidates(g_q, g_q.policy, which);
  for(int k = 0; k < sc.n; ++k) {
    std::memcpy(poses + 16 * k, sc.T[k].m, 64);
    kinds[k] = sc.kind[k];
  }
  return sc.n;
}
// the choice among them from records (null: modes 0 and 1); the record it leaves in the state, and the start
void sp_choose(int which, const bpvo_hip_pose_score* records, bpvo_hip_start_info* info, float* T_start)
{
  const StartCandidates sc = vo_start_candidates(g_q, g_q.policy, which);
  const M44 T = vo_start_choose(g_q, which, sc, records);
  *info = g_q.start[which];
  std::memcpy(T_start, T.m, 64);
}
void sp_info(int which, bpvo_hip_start_info* info) { *info = g_q.start[which]; }
void sp_rig_score(const bpvo_hip_pose_score* rec, const int* n_points, int n, int C, float tau, bpvo_hip_pose_score* out)
{
  *out = vo_rig_start_score(rec, n_points, n, C, tau);
}
int sp_sizes(int what) { return what == 0 ? (int) sizeof(bpvo_hip_start_policy) : (int) sizeof(bpvo_hip_start_info); }

}
