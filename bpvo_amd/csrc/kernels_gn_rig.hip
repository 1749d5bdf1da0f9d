// Rig mode (bpvo_hip_*_rig): the Gauss-Newton step of a rigid rig of cameras, ONE body pose for all of them (rig_math.h states the maps).
//   rig_step  per iteration the members run the chain unchanged — warp_residual, median, irls_reduce, gn_step in its linearise-only mode, which
//             leaves (H_p, G_p, f_p, valid count) of member p in its GNState — then ONE wavefront takes the rig's step: the members' systems
//             brought to the body's twist and summed in member order in f64, gn_logic itself on an LDS copy of the BODY's GNState (the extra
//             entry behind the workspaces' states), and every member's next pose X_p T X_p^-1 written back.  The twist of the step: the plain
//             body twist (bpvo_hip_linearize_rig), or the reference member's normalised twist (the estimate loops; RigStepArgs::reference).
#include <float.h>

#include "kernels.h"

#include "gn_common.h"
#include "gn_warp.h"
#include "gn_median.h"
#include "gn_irls.h"
#include "gn_step.h"
#include "rig_math.h"

namespace bpvo_hip {

struct RigStepLds {
  GNStepLds step;          // the body's state, the packed sums, nrm, the solver's scratch: what gn_step_wave keeps for one workspace
  double Ai[36], Ad[36];   // A_p^-1 and Ad(X_p) of the member being added
  double A0[36], AdA0[36]; // the reference member's A_0 (the identity for the plain body twist), Ad(X_p) A_0
  double B[36];            // B_p = A_p^-1 Ad(X_p) A_0
  float H[36], G[6];       // the member's system
  float X[16], nrm[4], nrm0[4];
};

// the members' poses from the body's T in LDS: lanes over the 16 n entries; with_out: T_out too (a level's start and end)
__device__ __forceinline__ void rig_write_member_poses(const RigStepArgs& a, const float* body_T, const float* body_T_out, bool with_out, int lane)
{
  for(int idx = lane; idx < 16 * a.n; idx += 64) {
    const int p = idx >> 4, e = idx & 15;
    const float* X = a.X + 16 * (size_t) p;
    GNState* st = a.jobs[p].st;
    const bool last_row = e >= 12;
    st->T[e] = last_row ? (e == 15 ? 1.0f : 0.0f) : (float) rig_member_pose_at(X, body_T, e >> 2, e & 3);
    if(with_out) st->T_out[e] = last_row ? (e == 15 ? 1.0f : 0.0f) : (float) rig_member_pose_at(X, body_T_out, e >> 2, e & 3);
  }
}

// mode 0: the full step (solve, update, convergence: gn_logic); 1: linearise only (the joint H, G, f, valid count into the body's state);
// 2: the start of a level (PoseEstimatorBase::reset of the body, the members' poses from the body's) — with T_init != null the start of the
// estimate as well (set_pose of the body).  One wavefront, one rig: a.jobs is the rig's first member.  The ONE step of both kernels below.
__device__ __forceinline__ int rig_step_wave(RigStepLds& s, const RigStepArgs& a)      // returns the body's `active` after the step
{
  constexpr int kWords = (int) (sizeof(GNState) / sizeof(uint32_t));
  const int lane = threadIdx.x;
  GNState* gst = a.body;
  if(a.mode == 0 && !gst->active) return 0;    // (the level is over: the host's pipelined rounds run out empty)
  for(int i = lane; i < kWords; i += 64) s.step.state[i] = reinterpret_cast<const uint32_t*>(gst)[i];
  // the twist the step is taken in: the plain body twist (the path nrm[4] != 0 selects in gn_update_pose), or — a.reference, the estimate
  // loops — the reference member's normalised twist, the state's T then being THAT member's pose and a.X the extrinsics relative to it
  if(lane < 4) s.step.nrm[lane] = a.reference ? a.jobs[0].nrm[lane] : (lane == 0 ? 1.0f : 0.0f);
  if(lane == 4) s.step.nrm[4] = a.reference ? 0.0f : 1.0f;
  if(lane < 4) s.nrm0[lane] = a.reference ? a.jobs[0].nrm[lane] : (lane == 0 ? 1.0f : 0.0f);
  wave_lds_sync();
  GNState* st = reinterpret_cast<GNState*>(s.step.state);

  if(a.mode == 2) {
    if(lane == 0) {
      if(a.T_init) {      // set_pose_kernel's part
        for(int i = 0; i < 16; ++i) st->T_out[i] = a.T_init[i];
        st->trace_n = 0;
        st->prm = a.jobs[0].prm;
        for(int l = 0; l < kMaxLevels; ++l) {
          st->stats[l].numIterations = 0;
          st->stats[l].finalError = -1.0f;
          st->stats[l].firstOrderOptimality = -1.0f;
          st->stats[l].status = BPVO_STATUS_SOLVER_ERROR;
        }
      }
      gn_level_reset(st, a.level, 0, 1);
    }
    wave_lds_sync();
    rig_write_member_poses(a, st->T, st->T_out, true, lane);
    for(int i = lane; i < kWords; i += 64) reinterpret_cast<uint32_t*>(gst)[i] = s.step.state[i];
    return st->active;
  }

  // the joint system: lane a * 6 + b < 36 holds entry (a, b) of H, lanes 36 .. 41 the entries of G, lane 42 the squared norm, lane 43 the valid count
  if(lane == 0) rig_normalization_map(s.nrm0, s.A0);
  double acc = 0.0;
  for(int p = 0; p < a.n; ++p) {
    const PairJob& j = a.jobs[p];
    const GNState* ms = j.st;
    if(lane < 36) s.H[lane] = ms->H[lane];
    else if(lane < 42) s.G[lane - 36] = ms->G[lane - 36];
    else if(lane < 46) s.nrm[lane - 42] = j.dspace ? (lane == 42 ? 1.0f : 0.0f) : j.nrm[lane - 42];
    else if(lane < 62) s.X[lane - 46] = a.X[16 * (size_t) p + (lane - 46)];
    wave_lds_sync();
    if(lane == 0) rig_normalization_map_inverse(s.nrm, s.Ai);
    if(lane == 1) rig_adjoint(s.X, s.Ad);
    wave_lds_sync();
    if(lane < 36) s.AdA0[lane] = rig_body_map_at(s.Ad, s.A0, lane / 6, lane % 6);
    wave_lds_sync();
    // (the reference member in its own twist: the identity, exactly — its system passes through bit for bit)
    if(lane < 36) s.B[lane] = (a.reference && p == 0) ? (lane / 6 == lane % 6 ? 1.0 : 0.0) : rig_body_map_at(s.Ai, s.AdA0, lane / 6, lane % 6);
    wave_lds_sync();
    if(lane < 36) acc += rig_congruence_at(s.B, s.H, lane / 6, lane % 6);
    else if(lane < 42) acc += rig_gradient_at(s.B, s.G, lane - 36);
    else if(lane == 42) acc += (double) ms->f_norm * (double) ms->f_norm;
    else if(lane == 43) acc += (double) ms->n_valid;
    wave_lds_sync();
  }
  // packed as gn_logic consumes it (s_sum: 21 upper-triangle entries, 6 of G, the squared norm, the valid count): narrowed to f32 once
  if(lane < 36) {
    const int r = lane / 6, c = lane % 6;
    if(c >= r) s.step.sum[r * 6 - r * (r - 1) / 2 + (c - r)] = (float) acc;
  } else if(lane < 42) s.step.sum[21 + (lane - 36)] = (float) acc;
  else if(lane == 42) s.step.sum[27] = (float) acc;
  else if(lane == 43) s.step.sum[28] = (float) acc;
  wave_lds_sync();
  if(lane == 0) {
    const GNParams prm = st->prm;
    (void) gn_logic(st, s.step.nrm, s.step.sum, &s.step.scratch, a.mode, prm.max_iterations, prm.max_fun_evals, prm.p_tol, prm.f_tol, prm.g_tol);
  }
  wave_lds_sync();
  if(a.mode == 0) {
    const bool done = st->active == 0;
    rig_write_member_poses(a, st->T, st->T_out, done, lane);
    if(done && lane < a.n) a.jobs[lane].st->active = 0;
    for(int p = 64 + lane; done && p < a.n; p += 64) a.jobs[p].st->active = 0;
  }
  for(int i = lane; i < kWords; i += 64) reinterpret_cast<uint32_t*>(gst)[i] = s.step.state[i];
  return st->active;
}

__global__ __launch_bounds__(64) void rig_step_kernel(RigStepArgs a)
{
  __shared__ RigStepLds s;
  (void) rig_step_wave(s, a);
}

// Several rigs in one launch: workgroup r (one wavefront) takes the step of rig r of the table — its members jobs[first .. first + n) of the
// level's row, its extrinsics, its body state, its initial pose — with exactly rig_step_kernel's arithmetic.  A rig whose body is no longer
// active leaves at once (rig_step_wave's first test): nothing of it is touched while the other rigs of the launch iterate.  active_out[r]: the
// body's `active` after the step, the words the host reads once per round.
__global__ __launch_bounds__(64) void rig_steps_kernel(RigStepsArgs b)
{
  __shared__ RigStepLds s;
  const RigEntry e = b.rigs[blockIdx.x];
  const RigStepArgs a{b.jobs + e.first, e.n, e.X, e.body, b.mode, b.level, (b.mode == 2 && b.with_init) ? e.T_init : nullptr, b.reference};
  const int active = rig_step_wave(s, a);
  if(threadIdx.x == 0) b.active_out[blockIdx.x] = active;
}

void launch_rig_step(hipStream_t s, const RigStepArgs& a)
{
  if(a.n <= 0) return;
  hipLaunchKernelGGL(rig_step_kernel, dim3(1), dim3(64), 0, s, a);
}
void launch_rig_steps(hipStream_t s, const RigStepsArgs& b)
{
  if(b.n_rigs <= 0) return;
  hipLaunchKernelGGL(rig_steps_kernel, dim3(b.n_rigs), dim3(64), 0, s, b);
}

}  // namespace bpvo_hip
