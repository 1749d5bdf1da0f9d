// libbpvo_hip, host side: VisualOdometryPoseEstimator::estimatePose.  estimate_group, the driver of every estimate of cameras, is
//   1. group_upload         the group's job tables and initial poses
//   2. run_team             small batches: every level of every pair in ONE launch of the team kernel (or two: the split form)
//   3. run_levels           otherwise level by level, coarse to fine: run_level_persistent (the level in one launch) or run_level_chain (the four-kernel
//                           chain in pipelined rounds: gn_rounds.h run_rounds queues linearize_launches)
//   4. queue_fraction_good  the result records, and addFrame's count of good points behind the estimate
//   5. group_collect        states and control words back, the one synchronisation; a persistent form gave up: 1 .. 5 once more without
//   6. group_outputs        poses and statistics
// The rig estimates (estimate_rigs) run on the same rounds and the same launches.  Also here: the operator-level seam (linearize, residuals, weights)
// and bpvo_hip_batch_estimate.
#include "host_ctx.h"

using namespace bpvo_hip;
using namespace bpvo_hip_host;

namespace bpvo_hip_host {

// ---- estimatePose ---------------------------------------------------------------------------------------------------

// The shape of the team launch for a group of n pairs — ONE place decides it, for run_team below and for team_serves: one workgroup per CU,
// teams of CUs / pairs workgroups (at most an eighth of the device's CUs, 32 of 256: teams of 64 were 8 - 12 % slower at 2 - 5 pairs, 4 % at 6 - 7; a
// team's workgroups stay dealt over ALL XCDs — pinned to one XCD each, 2 - 4 teams were 3 - 8 % slower), as many teams as fit; whether idle
// workgroups may join other teams (the growing form), and how many spare workgroups the division leaves for that.
struct TeamPlan { int team_size, n_teams, join_mode, spare_workgroups; };
static TeamPlan team_plan(const bpvo_hip_ctx* c, int n)
{
  TeamPlan t;
  const int slots = std::max(1, c->num_cus);
  int ts = c->team_size_env > 0 ? c->team_size_env : std::max(1, std::min(std::max(1, c->device_cus > 0 ? c->device_cus / 8 : 32), slots / std::max(1, n)));
  ts = std::max(1, std::min(ts, slots));
  t.team_size = ts;
  t.n_teams = std::max(1, std::min(std::min(n, slots / ts), kMaxTeams));
  // (nobody can join where the teams start at the admission cap or there is one team only: the leaders' looks at the tickets are then
  // skipped altogether — a 16-pair batch, teams of 16, lost 1.5 % to them)
  t.join_mode = (t.team_size < gn_team_max_size() && t.n_teams > 1 && n >= c->team_join_from_pairs) ? c->team_join : 0;
  // what the division CUs / pairs leaves over starts as spare workgroups that join the teams at their first admission
  t.spare_workgroups = (t.join_mode && c->team_spares) ? std::max(0, slots - t.team_size * t.n_teams) : 0;
  return t;
}

// Does a group of n pairs take the team-persistent kernel?  (kLinear, the f64 formulation, C = 8 or 1 like gn_persistent_kernel; not
// while per-kernel timings are being collected: there are no kernels to time)
bool team_serves(const bpvo_hip_ctx* c, int n)
{
  bool size_ok = n >= 2 && n > c->persist_max_ws && n <= c->team_max_pairs;
  // above team_full_pairs only when the launch fills the chip: the kernel runs CUs / n workgroups per pair, and what that division leaves over
  // idles for the whole launch (96 pairs: 2 x 96 of 256 CUs, 770 k GN it/s against the chain's 840 k; 128 pairs: 2 x 128, 935 k against 890 k) —
  // unless the PLAN of this very launch turns the remainder into spare workgroups that join the teams (the growing form)
  if(size_ok && n > c->team_full_pairs && c->team_size_env <= 0 && c->num_cus > 0) {
    const TeamPlan t = team_plan(c, n);
    const int busy = t.team_size * t.n_teams + t.spare_workgroups;
    size_ok = 20 * busy >= 19 * c->num_cus;
  }
  return c->team_mode && c->persistent && !c->persistent_failed.load() && size_ok && !c->reference_reduction && !loss_is_chain_only(c->params.lossFunction) &&
         (c->C == 8 || c->C == 1) && c->params.interp == BPVO_INTERP_LINEAR && !c->fast_warp && !c->profile_all && !c->profile_k6_all &&
         c->num_cus >= 2 && g_live_ctx[c->device & 63].load() <= 1;
}

// ... and only templates the team kernel is good at: a pyramid level of more points than the persistent kernels are given (persist_max_points: dense
// templates, NMS off) is bandwidth work for the chain's chip-wide launches — the teams' per-pair median alone walks a thousand candidate segments
// per iteration there (640x480 bit-planes, NMS off, 4 / 16 / 64 pairs: 11.4 / 15.2 / 30.1 ms per step on the team kernel, 6.0 / 10.1 / 20.8 on the
// chain: scripts/dense_batch_ab.py)
static bool templates_suit_teams(const bpvo_hip_ctx* c, int n, const int* refs)
{
  for(int i = 0; i < n; ++i)
    for(int l = c->params.maxTestLevel; l < c->L; ++l)
      if(c->frames[refs[i]].n_host[l] > c->persist_max_points) return false;
  return true;
}

// The job tables of a lane: rows [first, first + n) at every level — job i of workspace wss[i] on the pair (refs[i], curs[i]), with prm_of(i)'s
// parameters where that is not null, the G channel-group rows of a wide descriptor behind table 0 — and into max_pts[l] the most points of a row
// at level l (max_pts is the caller's: rigs fill their ranges one after the other).  Every estimate path lays its jobs out here.
template <class PrmOf>
static void fill_job_tables(bpvo_hip_ctx* c, Lane* ln, int first, int n, const int* wss, const int* refs, const int* curs, PrmOf&& prm_of, int* max_pts)
{
  const int NP = c->n_pairs;
  const size_t table = (size_t) c->L * NP;      // jobs of one table [L][NP]; wide descriptors: table 0 the whole jobs, tables 1 .. G their channel groups
  for(int l = 0; l < c->L; ++l)
    for(int i = 0; i < n; ++i) {
      PairJob& pj = ln->h_pjobs[(size_t) l * NP + first + i];
      pj = make_pair_job(c, wss[i], refs[i], curs[i], l);
      if(const bpvo_hip_params* prm = prm_of(i)) pair_job_set_params(pj, *prm);
      for(int k = 0; k < c->G && c->G > 1; ++k) ln->h_pjobs[(size_t) (1 + k) * table + (size_t) l * NP + first + i] = group_pair_job(c, pj, k);
      max_pts[l] = std::max(max_pts[l], pj.n);
    }
}
// One estimate per loss present among n entries (the loss instantiates the kernels): run(at) for the entries `at` of one loss, the losses in the
// order of their first occurrence, the entries of a loss in call order.  One loss: one run over all the entries.
template <class LossOf, class Run>
static int for_each_loss(int n, LossOf&& loss_of, Run&& run)
{
  std::vector<char> done((size_t) n, 0);
  for(int i = 0; i < n; ++i) {
    if(done[i]) continue;
    std::vector<int> at;
    for(int k = i; k < n; ++k)
      if(!done[k] && loss_of(k) == loss_of(i)) { done[k] = 1; at.push_back(k); }
    if(int rc = run(at)) return rc;
  }
  return BPVO_OK;
}

// One linearisation of the jobs of g at their states' poses: warp_residual (K6) per channel group, the median (K7), the reduction (K8) per channel
// group — or once, in reference order —, and the step unless the reduction takes it.  The ONE place that queues these four kernels: the estimate
// loops of cameras and rigs, the operator-level seam and the pose-covariance pass (its residuals: the warp alone) all come here.
void linearize_launches(bpvo_hip_ctx* c, Lane* ln, const GNLaunch& g, size_t stride, const LinearizeFlags& f)
{
  constexpr unsigned kProfileEvery = 5;   // co-prime with kItersPerSync: no phase lock with the host round trips
  const bool all = f.timers == TIMERS_ALWAYS || (f.timers != TIMERS_OFF && c->profile_all);
  if(f.warp) {
    // TIMERS_ESTIMATE, level 1, brackets every kProfileEvery-th warp_residual launch of the lane with events (a running counter, so the
    // sampled launches rotate through all iterations and levels): an event pair costs a few µs of dispatch gap
    const bool sampled = all || (f.timers == TIMERS_ESTIMATE && (c->profile_k6_all || (ln->k6_seq++ % kProfileEvery) == 0));
    ScopedTimer t(c, KC_WARP_RESIDUAL, 0.0, ln, sampled);
    for_each_group(c, g, stride, [&](const GNLaunch& gg) { launch_warp_residual(ln->stream, gg); });
  }
  // level 2 times every kernel; level 3 (bench.py's single-lane roofline pass) every warp_residual AND every irls_reduce launch
  { ScopedTimer t(c, KC_MEDIAN, 0.0, ln, all && f.median); if(f.median) launch_median(ln->stream, median_launch(c, g)); }
  if(f.reduce) {
    ScopedTimer t(c, KC_IRLS_REDUCE, 0.0, ln, all || (f.timers == TIMERS_ESTIMATE && c->profile_k6_all));
    if(g.reference_reduction) launch_irls_reduce(ln->stream, g);      // (reference order: one wave per pair walks every channel of the whole job)
    else for_each_group(c, g, stride, [&](const GNLaunch& gg) { launch_irls_reduce(ln->stream, gg); });
  }
  if(f.step && !g.step_in_reduce) {
    ScopedTimer t(c, KC_GN_STEP, 0.0, ln, all);
    launch_gn_step(ln->stream, g, f.step_mode);
  }
}

// run_rounds (gn_rounds.h) on a lane: a round's flags are marked by the lane's event of the slot ("the flags of round r have landed"), which the
// host waits for a round later.  queue_flags(slot): the copy of the flags into the slot's pinned words.
template <class QueueIterations, class QueueFlags, class Read>
static int lane_rounds(Lane* ln, int max_iterations, QueueIterations&& queue_iterations, QueueFlags&& queue_flags, Read&& read)
{
  return run_rounds(max_iterations, queue_iterations,
                    [&](int slot) -> int {
                      if(int rc = queue_flags(slot)) return rc;
                      LANE_CK(ln, hipEventRecord(ln->round_ev[slot], ln->stream));
                      return BPVO_OK;
                    },
                    [&](int slot) -> int {
                      LANE_CK(ln, hipEventSynchronize(ln->round_ev[slot]));
                      return BPVO_OK;
                    },
                    read);
}

// One estimate_group call: what its steps share.  The modes are set per attempt (group_modes).
struct GroupRun {
  bpvo_hip_ctx* c;
  Lane* ln;
  int n;
  const int* wss; const int* refs; const int* curs;      // [n] workspace, template slot, current slot
  const float* T_init;                                   // host [n][16] or null (Identity)
  const bpvo_hip_params* const* prms;                    // [n] or null
  float* d_records_out;
  // the group's loss (one per group: estimate_batch) and the largest iteration limit among its entries: the host sizes its rounds by it, the
  // device enforces each workspace's own (PairJob::prm)
  int loss, max_iterations;
  std::vector<int> max_pts;      // [L] the most points of a job at the level
  // validation mode "reference_reduction": the four-kernel chain with the index-order reduction in irls_reduce's place — residuals always written
  // (no fused path), the step in its own launch, no persistent / team kernel
  bool ref_mode;
  int fuse_frozen;
  bool allow_persistent;         // this attempt may take the persistent forms
  bool pk_group;                 // ... and is a group for the persistent single-pair kernel
  bool small_ctx;                // a context of a few pairs (one pair per call): table, poses and control words in one launch, the states copied out by the last one
  bool l2_moot;                  // kL2: the weights are 1 whatever the robust scale — with the fused path every linearisation is irls_reduce + gn_step only
  bool team_ran, team_split, frac_queued;
};
static void group_modes(GroupRun& r, bool allow_persistent)
{
  const bpvo_hip_ctx* c = r.c;
  r.ref_mode = c->reference_reduction != 0;
  r.fuse_frozen = r.ref_mode ? 0 : c->fuse_frozen;
  r.allow_persistent = allow_persistent;
  r.pk_group = allow_persistent && c->persistent && !c->persistent_failed.load() && r.n <= c->persist_max_ws && !c->profile_all && !r.ref_mode &&
               !loss_is_chain_only(r.loss);
  r.small_ctx = (size_t) c->L * c->n_pairs <= 64 && r.n <= 8 && c->small_batch_fused && c->G == 1;
  r.l2_moot = r.loss == BPVO_LOSS_L2 && c->C == 8 && r.fuse_frozen && !c->fast_warp && c->params.interp == BPVO_INTERP_LINEAR;
  r.team_ran = r.team_split = r.frac_queued = false;
}

// 1. the job tables of the group (dense levels without the tap cache), and the initial poses into the states of the coarsest level's jobs
static int group_upload(GroupRun& r)
{
  bpvo_hip_ctx* c = r.c;
  Lane* ln = r.ln;
  const int n = r.n, NP = c->n_pairs;
  const int* refs = r.refs;
  const float* T_init = r.T_init;
  const bool persistent = r.pk_group;
  // (the pinned staging of a lane is free here: every call that uses it ends with a synchronisation of the lane's stream)
  std::fill(r.max_pts.begin(), r.max_pts.end(), 0);
  const size_t table = (size_t) c->L * NP;
  fill_job_tables(c, ln, 0, n, r.wss, refs, r.curs, [&](int i) { return r.prms ? r.prms[i] : nullptr; }, r.max_pts.data());
  // Dense levels (no non-maximum suppression: most pixels are template points) gather their taps straight from the descriptor:
  // neighbouring points share three quarters of their footprints, so the 32-byte records are fetched about once per pixel
  // from HBM, where the per-point tap cache reads 128 bytes per point whatever the neighbours do.  The cache pays at the
  // sparse levels (one point in ~25 pixels: every footprint its own two or three lines).  Batches only: the persistent
  // single-pair kernel keeps its (L2-resident) cache.  (8 channels or 1: one table, no channel-group rows to copy the flag to.)
  if((c->C == 8 || c->C == 1) && n > c->persist_max_ws)
    for(int l = 0; l < c->L; ++l)
      for(int i = 0; i < n; ++i) {
        PairJob& pj = ln->h_pjobs[(size_t) l * NP + i];
        if((double) pj.n > c->tapcache_max_density * (double) slot_geom(c, c->frames[refs[i]], l).npix) pj.tapcache_on = 0;
      }
  if(r.small_ctx) {
    if(T_init) std::memcpy(ln->h_T, T_init, sizeof(float) * 16 * n);
    launch_set_pose_upload(ln->stream, ln->d_pjobs, ln->h_pjobs, (size_t) c->L * NP, ln->h_pjobs + (size_t) (c->L - 1) * NP, T_init ? ln->h_T : nullptr, n,
                           persistent ? ln->d_pk_ctl : nullptr, persistent ? kPkCtlWords * kMaxLevels : 0);
  } else {
    const size_t table_bytes = sizeof(PairJob) * table * (size_t) job_tables(c);
    if(c->ctl_by_kernel.load()) launch_copy_rows(ln->stream, ln->d_pjobs, ln->h_pjobs, table_bytes, table_bytes, 1);
    else LANE_CK(ln, hipMemcpyAsync(ln->d_pjobs, ln->h_pjobs, table_bytes, hipMemcpyHostToDevice, ln->stream));
    const float* dT = nullptr;
    if(T_init) {
      std::memcpy(ln->h_T, T_init, sizeof(float) * 16 * n);
      if(c->ctl_by_kernel.load()) launch_copy_rows(ln->stream, ln->d_Tinit, ln->h_T, sizeof(float) * 16 * n, sizeof(float) * 16 * n, 1);
      else LANE_CK(ln, hipMemcpyAsync(ln->d_Tinit, ln->h_T, sizeof(float) * 16 * n, hipMemcpyHostToDevice, ln->stream));
      dT = ln->d_Tinit;
    }
    launch_set_pose(ln->stream, ln->d_pjobs + (size_t) (c->L - 1) * NP, dT, n, persistent ? ln->d_pk_ctl : nullptr, persistent ? kPkCtlWords * kMaxLevels : 0);
  }
  return BPVO_OK;
}

// 2. Small batches: the whole level loop in ONE launch, a team of workgroups per pair (gn_team_kernel).  r.team_ran: the launch went out — a
// launch the device refuses degrades the context to the chain, now and for later calls.
static int run_team(GroupRun& r)
{
  bpvo_hip_ctx* c = r.c;
  Lane* ln = r.ln;
  const bpvo_hip_params& p = c->params;
  const int n = r.n;
  // Small batches whose template stage left the normalisation of the levels below the coarsest on the side stream (frames.hip): the
  // team kernel in TWO launches — the coarsest level of every pair, then (behind that normalisation) the others.  The sums (0.17 - 0.19 ms
  // for a 1241x376 frame, whatever the batch) then run under the coarsest level's iterations instead of in front of the first one;
  // larger batches join them here, at once: a launch boundary makes every pair wait for the slowest (measured: 2 / 4 pairs + 1.2 / + 1.5 %,
  // 8 / 16 / 32 / 64 pairs - 5 / - 7 / - 4 / - 6 %: option "team_split_max_pairs", 4).
  r.team_split = (c->nrm_pending != nullptr || c->nrm_pending_finest != nullptr) && n <= c->team_split_max_pairs && c->L - 1 > p.maxTestLevel;
  if(!r.team_split) LANE_CK(ln, join_pending_normalization(c, ln->stream));
  GNTeamLaunch t;
  t.jobs_all = ln->d_pjobs; t.job_pitch = c->n_pairs; t.n_pairs = n; t.level_hi = c->L - 1; t.level_lo = p.maxTestLevel;
  t.C = c->C; t.loss = r.loss; t.fuse_frozen = c->fuse_frozen;
  t.scale_is_moot = (r.loss == BPVO_LOSS_L2 && c->C == 8 && c->fuse_frozen) ? 1 : 0;
  const TeamPlan plan = team_plan(c, n);      // (the same plan team_serves judged)
  t.team_size = plan.team_size;
  t.n_teams = plan.n_teams;
  t.ctl = ln->d_team_ctl;
  t.timeout_ticks = c->persist_timeout;
  t.local_barriers = c->team_local_barriers;
  t.join_mode = plan.join_mode;
  t.spare_workgroups = plan.spare_workgroups;
  LANE_CK(ln, hipMemsetAsync(ln->d_team_ctl, 0, sizeof(unsigned) * (size_t) gn_team_ctl_words(t.n_teams), ln->stream));
  hipError_t te;
  if(r.team_split) {
    t.level_lo = c->L - 1;
    te = launch_gn_team(ln->stream, t);
    if(te == hipSuccess) {
      // (the first launch's control words: its abort word and join count are looked at with the second's)
      LANE_CK(ln, hipMemcpyAsync(ln->h_team_ctl + 32, ln->d_team_ctl, sizeof(unsigned) * 32, hipMemcpyDeviceToHost, ln->stream));
      launch_team_ctl_reset_keep_abort(ln->stream, ln->d_team_ctl, t.n_teams);      // (a first launch that gave up: the second leaves at once)
    }
    LANE_CK(ln, join_pending_normalization(c, ln->stream));
    t.level_hi = c->L - 2; t.level_lo = p.maxTestLevel;
    if(te == hipSuccess) te = launch_gn_team(ln->stream, t);
  } else {
    te = launch_gn_team(ln->stream, t);
  }
  if(te == hipSuccess) {
    r.team_ran = true;
    c->team_launches.fetch_add(1);
    LANE_CK(ln, hipMemcpyAsync(ln->h_team_ctl, ln->d_team_ctl, sizeof(unsigned) * 32, hipMemcpyDeviceToHost, ln->stream));
  } else {
    (void) hipGetLastError();
    c->persistent_failed.store(true);      // degrade to the chain, now and for later calls
  }
  return BPVO_OK;
}

// the launch of level l's kernels over the whole group
static GNLaunch group_level_launch(const GroupRun& r, int l)
{
  const bpvo_hip_ctx* c = r.c;
  GNLaunch g = level_launch(c, r.ln->d_pjobs + (size_t) l * c->n_pairs, r.n, r.max_pts[l], r.loss);
  g.fuse_frozen = r.fuse_frozen;
  g.step_in_reduce = (r.n <= c->step_in_reduce_max && !r.ref_mode && c->G == 1) ? 1 : 0;
  return g;
}
static bool persistent_serves_level(const GroupRun& r, int l)
{
  return r.max_pts[l] > 0 && gn_persistent_serves(group_level_launch(r, l)) && r.max_pts[l] <= r.c->persist_max_points;
}

// 3a. The whole level l in one launch of the persistent kernel — and the start of the next level with it, when that one takes the kernel too.
// was_begun: this level's start was left to this launch by the one before.
struct PersistentLevel { bool served, began_next; };
static PersistentLevel run_level_persistent(GroupRun& r, GNLaunch g, int l, bool was_begun)
{
  bpvo_hip_ctx* c = r.c;
  Lane* ln = r.ln;
  const bool next_too = l - 1 >= c->params.maxTestLevel && persistent_serves_level(r, l - 1);
  g.begin_level = was_begun ? l : -1;
  g.begin_moot = r.l2_moot ? 1 : 0;
  g.next_jobs = next_too ? ln->d_pjobs + (size_t) (l - 1) * c->n_pairs : nullptr;
  const hipError_t pe = launch_gn_persistent(ln->stream, g, ln->d_pk_ctl + (size_t) l * kPkCtlWords, gn_persistent_grid(g, c->persist_grid), c->persist_timeout);
  if(pe == hipSuccess) {
    c->persistent_levels.fetch_add(1);
    return {true, next_too};
  }
  // the device cannot grant the kernel its LDS / residency (or the launch failed): degrade to the four-kernel chain — this level,
  // the rest of the pyramid and every later call of the context — instead of failing the estimate
  (void) hipGetLastError();
  c->persistent_failed.store(true);
  if(was_begun) launch_level_begin(ln->stream, g.jobs, r.n, g.max_points, l, r.l2_moot ? 1 : 0);
  return {false, false};
}

// 3b. The level on the four-kernel chain, in pipelined rounds (gn_rounds.h): a round's flags are the compacted list of the still-active
// workspaces, its count and how many of them still estimate their scale; round r + 1 runs over the list that came out of round r - 1.
static int run_level_chain(GroupRun& r, GNLaunch g)
{
  bpvo_hip_ctx* c = r.c;
  Lane* ln = r.ln;
  const int NP = c->n_pairs;
  const size_t table = (size_t) c->L * NP;
  int* const lists[3] = {ln->d_list, ln->d_list + NP, ln->d_list + 2 * (size_t) NP};
  int n_cur = r.n;
  g.active.list = nullptr;                // first rounds: every workspace of the group, in order
  // Once NO active workspace of the list estimates its robust scale any more (a frozen scale stays frozen for the level, and the
  // list only shrinks), the median has nothing to do and — with the fused path, where irls_reduce recomputes the residuals of
  // frozen workspaces itself — neither has warp_residual: their launches are dropped for the rest of the level.  (Each would
  // still cost its floor of ~5 us per iteration in the tail of a level.)  l2_moot: true from the first linearisation.
  const bool fused_path = c->C == 8 && r.fuse_frozen && !c->fast_warp && c->params.interp == BPVO_INTERP_LINEAR;
  bool none_moving = r.l2_moot;
  LinearizeFlags f;
  f.timers = TIMERS_ESTIMATE;
  return lane_rounds(ln, r.max_iterations,
                     [&](int) -> int {
                       g.npairs = n_cur;
                       f.median = !none_moving;
                       f.warp = !(none_moving && fused_path);
                       for(int k = 0; k < kItersPerSync; ++k) linearize_launches(c, ln, g, table, f);
                       return BPVO_OK;
                     },
                     [&](int slot) -> int {
                       launch_compact_active(ln->stream, g.jobs, g.active, n_cur, lists[slot], ln->d_active + 2 * slot);
                       LANE_CK(ln, hipMemcpyAsync(ln->h_active + 2 * slot, ln->d_active + 2 * slot, 2 * sizeof(int), hipMemcpyDeviceToHost, ln->stream));
                       return BPVO_OK;
                     },
                     [&](int slot) {
                       const int n_left = ln->h_active[2 * slot];
                       if(n_left <= 0) return false;
                       n_cur = n_left;
                       none_moving = none_moving || ln->h_active[2 * slot + 1] == 0;
                       g.active.list = lists[slot];
                       return true;
                     });
}

// 3. Level by level, coarse to fine.  A level the persistent kernel does not serve takes the chain, and the rest of the pyramid with it.
static int run_levels(GroupRun& r)
{
  bpvo_hip_ctx* c = r.c;
  Lane* ln = r.ln;
  bool persistent = r.pk_group;
  bool begun = false;      // this level's start was left to its persistent kernel (its tap-cache keys invalidated by the kernel of the level before)
  for(int l = c->L - 1; l >= c->params.maxTestLevel; --l) {
    const GNLaunch g = group_level_launch(r, l);
    // (the deferred normalisation: this lane waits for it where the second level starts)
    if(l < c->L - 1) LANE_CK(ln, join_pending_normalization(c, ln->stream, l));
    const bool was_begun = begun;
    begun = false;
    if(!was_begun) launch_level_begin(ln->stream, g.jobs, r.n, g.max_points, l, r.l2_moot ? 1 : 0);    // (and the tap-cache keys of the level)
    if(g.max_points <= 0) continue;
    if(persistent && persistent_serves_level(r, l)) {
      const PersistentLevel pk = run_level_persistent(r, g, l, was_begun);
      begun = pk.began_next;
      if(pk.served) continue;
    }
    persistent = false;
    if(int rc = run_level_chain(r, g)) return rc;
  }
  return BPVO_OK;
}

// 4. The result records; and for addFrame (one pair, lane 0) the fraction of good points of the workspace at the level the estimate ended on,
// from the job already on the device, queued behind the estimate
static int queue_fraction_good(GroupRun& r)
{
  bpvo_hip_ctx* c = r.c;
  Lane* ln = r.ln;
  const bpvo_hip_params& p = c->params;
  const int NP = c->n_pairs;
  const PairJob* coarsest = ln->d_pjobs + (size_t) (c->L - 1) * NP;
  const bool want_frac = r.n == 1 && c->prefetch_frac_thr >= 0.0f && ln == &c->lanes[0];
  if(r.small_ctx) launch_pack_records(ln->stream, coarsest, r.n, c->L, r.d_records_out, c->d_states, ln->h_states, r.pk_group ? ln->d_pk_ctl : nullptr,
                                      r.pk_group ? ln->h_pk_ctl : nullptr, kPkCtlWords * kMaxLevels, want_frac ? c->d_count : nullptr);
  else launch_pack_records(ln->stream, coarsest, r.n, c->L, r.d_records_out);
  const int npts = ln->h_pjobs[(size_t) p.maxTestLevel * NP].n;
  if(!want_frac || npts <= 0) return BPVO_OK;
  const PairJob* job = ln->d_pjobs + (size_t) p.maxTestLevel * NP;
  launch_refresh_residuals(ln->stream, level_launch(c, job, 1, npts, p.lossFunction));
  if(!r.small_ctx) LANE_CK(ln, hipMemsetAsync(c->d_count, 0, sizeof(unsigned int), ln->stream));      // (small contexts: cleared by pack_records)
  launch_count_good(ln->stream, job, npts, c->C, p.lossFunction, c->prefetch_frac_thr, c->d_count);
  LANE_CK(ln, hipMemcpyAsync(c->h_ints, c->d_count, sizeof(unsigned int), hipMemcpyDeviceToHost, ln->stream));
  r.frac_queued = true;
  c->frac_n = npts;
  return BPVO_OK;
}

#ifdef BPVO_PK_TIMING
// library built with -DBPVO_PK_TIMING: per-phase ticks (10 ns) of workgroup 0 of the persistent kernel / of team 0's first workgroup
static void print_pk_timing(const GroupRun& r)
{
  const bpvo_hip_ctx* c = r.c;
  const Lane* ln = r.ln;
  static const char* names[6] = {"warp", "barrier1", "median", "irls", "barrier2", "step"};
  if(r.pk_group) {
    for(int l = c->L - 1; l >= 0; --l) {
      const unsigned* t = ln->h_pk_ctl + (size_t) l * kPkCtlWords;
      if(!t[15]) continue;
      std::fprintf(stderr, "pk level %d: %u iterations;", l, t[15]);
      for(int k = 0; k < 6; ++k) std::fprintf(stderr, " %s %.2f", names[k], 0.01 * t[8 + k] / t[15]);
      std::fprintf(stderr, " | step: sum_partials %.2f unpack %.2f solve %.2f pose %.2f tests %.2f", 0.01 * t[20] / t[15], 0.01 * t[16] / t[15], 0.01 * t[17] / t[15],
                   0.01 * t[18] / t[15], 0.01 * t[19] / t[15]);
      std::fprintf(stderr, " us per iteration\n");
    }
  }
  if(r.team_ran) {
    for(int l = c->L - 1; l >= 0 && l < 4; --l) {
      const unsigned* t = ln->h_team_ctl + 4 + 7 * l;
      if(!t[6]) continue;
      std::fprintf(stderr, "team level %d: %u iterations;", l, t[6]);
      for(int k = 0; k < 6; ++k) std::fprintf(stderr, " %s %.2f", names[k], 0.01 * t[k] / t[6]);
      std::fprintf(stderr, " us per iteration\n");
    }
  }
}
#endif

// 5. The group's states and the control words of the persistent forms back, addFrame's work under the queued estimate, the synchronisation.
// gave_up: a barrier of the persistent or of the team kernel timed out (workgroups not co-resident) — the states of that level were not written back.
static int group_collect(GroupRun& r, bool* gave_up)
{
  bpvo_hip_ctx* c = r.c;
  Lane* ln = r.ln;
  // only this group's states: other lanes may still be writing theirs
  int ws_lo = r.wss[0], ws_hi = r.wss[0];
  for(int i = 1; i < r.n; ++i) { ws_lo = std::min(ws_lo, r.wss[i]); ws_hi = std::max(ws_hi, r.wss[i]); }
  if(!r.small_ctx) {
    LANE_CK(ln, hipMemcpyAsync(ln->h_states + ws_lo, c->d_states + ws_lo, sizeof(GNState) * (size_t) (ws_hi - ws_lo + 1), hipMemcpyDeviceToHost, ln->stream));
    if(r.pk_group)
      LANE_CK(ln, hipMemcpyAsync(ln->h_pk_ctl, ln->d_pk_ctl, sizeof(unsigned) * kPkCtlWords * kMaxLevels, hipMemcpyDeviceToHost, ln->stream));
  }
  if(c->before_final_sync && ln == &c->lanes[0]) {      // (every kernel of the estimate is queued: the host is free for a moment)
    const std::function<int()> f = std::move(c->before_final_sync);
    c->before_final_sync = nullptr;
    if(const int rcf = f()) return rcf;
  }
  LANE_CK(ln, hipStreamSynchronize(ln->stream));
  LANE_CK(ln, hipGetLastError());
  if(r.frac_queued) { c->frac_valid = true; c->frac_ws = r.wss[0]; c->frac_thr = c->prefetch_frac_thr; c->frac_cnt = (unsigned) c->h_ints[0]; }
#ifdef BPVO_PK_TIMING
  print_pk_timing(r);
#endif
  if(r.team_ran) {
    c->team_joins.fetch_add(ln->h_team_ctl[3] + (r.team_split ? ln->h_team_ctl[32 + 3] : 0u));      // workgroups that joined another team (measurement)
    *gave_up = ln->h_team_ctl[1] != 0 || (r.team_split && ln->h_team_ctl[32 + 1] != 0);
  }
  if(r.pk_group)
    for(int l = 0; l < c->L; ++l) *gave_up = *gave_up || ln->h_pk_ctl[(size_t) l * kPkCtlWords + 1] != 0;
  return BPVO_OK;
}

// 6. poses [n][16] and statistics [n][L] from the states, where asked for
static void group_outputs(const GroupRun& r, float* poses, bpvo_hip_stats* stats)
{
  const int L = r.c->L;
  for(int i = 0; i < r.n; ++i) {
    const GNState& st = r.ln->h_states[r.wss[i]];
    if(poses) std::memcpy(poses + 16 * (size_t) i, st.T_out, 16 * sizeof(float));
    if(stats)
      for(int l = 0; l < L; ++l) stats[(size_t) i * L + l] = st.stats[l];
  }
}

// VisualOdometryPoseEstimator::estimatePose (reference: bpvo/vo_pose_estimator.cc:63-93) for a group of `n` workspaces on one lane.
// wss[i]: workspace, refs[i] / curs[i]: frame slots.  T_init host [n][16] or null (Identity).
// allow_persistent: only a group that has the device to itself (a batch on ONE lane) may take the persistent kernel — two
// hand-barrier grids of concurrent lanes must not be co-scheduled.
int estimate_group(bpvo_hip_ctx* c, Lane* ln, int n, const int* wss, const int* refs, const int* curs, const float* T_init,
                   float* poses, bpvo_hip_stats* stats, float* d_records_out, bool allow_persistent, const bpvo_hip_params* const* prms)
{
  if(n <= 0) return BPVO_OK;
  (void) hipSetDevice(c->device);
  GroupRun r{c, ln, n, wss, refs, curs, T_init, prms, d_records_out};
  r.loss = prms ? prms[0]->lossFunction : c->params.lossFunction;
  r.max_iterations = c->params.maxIterations;
  if(prms) {
    r.max_iterations = prms[0]->maxIterations;
    for(int i = 1; i < n; ++i) r.max_iterations = std::max(r.max_iterations, prms[i]->maxIterations);
  }
  r.max_pts.assign((size_t) c->L, 0);
  // with the persistent forms where the group may take them; one of them gave up at a barrier: the group once more through the four-kernel
  // chain (same results), and the context stays on it
  for(const bool persistent_forms : {allow_persistent, false}) {
    group_modes(r, persistent_forms);
    if(int rc = group_upload(r)) return rc;
    if(persistent_forms && ln == &c->lanes[0] && !loss_is_chain_only(r.loss) && team_serves(c, n) && templates_suit_teams(c, n, refs))
      if(int rc = run_team(r)) return rc;
    if(!r.team_ran)
      if(int rc = run_levels(r)) return rc;
    if(int rc = queue_fraction_good(r)) return rc;
    bool gave_up = false;
    if(int rc = group_collect(r, &gave_up)) return rc;
    if(!gave_up) break;
    c->persistent_failed.store(true);
  }
  group_outputs(r, poses, stats);
  return BPVO_OK;
}

int check_pairs(bpvo_hip_ctx* c, int n, const int* wss, const int* refs, const int* curs, int level_lo, int level_hi)
{
  for(int i = 0; i < n; ++i) {
    CHECK_WS(c, wss[i]); CHECK_SLOT(c, refs[i]); CHECK_SLOT(c, curs[i]);
  }
  for(int i = 0; i < n; ++i) {
    if(!c->frames[refs[i]].has_template) return fail(c, BPVO_ERR_NO_TEMPLATE, "reference frame has no template");
    if(!c->frames[curs[i]].has_data) return fail(c, BPVO_ERR_NO_DATA, "no data in frame");
    for(int l = level_lo; l <= level_hi; ++l)
      if(c->frames[refs[i]].n_host[l] <= 0) return fail(c, BPVO_ERR_NO_TEMPLATE, "you should call setData before calling computeResiduals");
  }
  for(int i = 0; i < n; ++i)
    if(int rc = ensure_dense_descriptor(c, curs[i])) return rc;
  return BPVO_OK;
}

// Entries with parameters of their own (bpvo_hip_add_frames): the loss is a template parameter of the reduction, persistent and team kernels, so
// the entries of a call are PARTITIONED by loss — at most four estimates, one per loss present and never one per sequence, each over the
// entries of that loss in call order; everything else a sequence may own travels in its jobs.  One loss (every call without per-sequence
// parameters): the one estimate there has always been.  (The alternative, a loss read per workspace inside the kernels: DESIGN.md §5.)
static int estimate_one_loss(bpvo_hip_ctx* c, int n, const int* wss, const int* refs, const int* curs, const float* T_init, float* poses, bpvo_hip_stats* stats,
                             const bpvo_hip_params* const* prms);
int estimate_batch(bpvo_hip_ctx* c, int n, const int* wss, const int* refs, const int* curs, const float* T_init, float* poses, bpvo_hip_stats* stats,
                   const bpvo_hip_params* const* prms)
{
  if(!prms) return estimate_one_loss(c, n, wss, refs, curs, T_init, poses, stats, prms);
  return for_each_loss(n, [&](int i) { return prms[i]->lossFunction; }, [&](const std::vector<int>& at) {
    const int m = (int) at.size();
    if(m == n) return estimate_one_loss(c, n, wss, refs, curs, T_init, poses, stats, prms);      // (one loss: the call's own arrays)
    std::vector<int> w(m), r(m), cu(m);
    std::vector<const bpvo_hip_params*> pp(m);
    std::vector<float> Ti, To((size_t) m * 16);
    std::vector<bpvo_hip_stats> st((size_t) m * c->L);
    if(T_init) Ti.resize((size_t) m * 16);
    for(int k = 0; k < m; ++k) {
      w[k] = wss[at[k]]; r[k] = refs[at[k]]; cu[k] = curs[at[k]]; pp[k] = prms[at[k]];
      if(T_init) std::memcpy(&Ti[(size_t) k * 16], T_init + 16 * (size_t) at[k], 64);
    }
    const int rc = estimate_one_loss(c, m, w.data(), r.data(), cu.data(), T_init ? Ti.data() : nullptr, To.data(), st.data(), pp.data());
    if(rc) return rc;
    for(int k = 0; k < m; ++k) {
      if(poses) std::memcpy(poses + 16 * (size_t) at[k], &To[(size_t) k * 16], 64);
      if(stats) std::memcpy(stats + (size_t) at[k] * c->L, &st[(size_t) k * c->L], sizeof(bpvo_hip_stats) * (size_t) c->L);
    }
    return (int) BPVO_OK;
  });
}
static int estimate_one_loss(bpvo_hip_ctx* c, int n, const int* wss, const int* refs, const int* curs, const float* T_init, float* poses, bpvo_hip_stats* stats,
                             const bpvo_hip_params* const* prms)
{
  if(n <= 0) return BPVO_OK;
  if(n > c->n_pairs) return fail(c, BPVO_ERR_INVALID_ARG, "more pairs than workspaces");
  const bpvo_hip_params& p = c->params;
  // (no level check: the batch entry points skip the empty levels of a pair, the single-pair ones have refused them — check_template_not_empty)
  if(int rc = check_pairs(c, n, wss, refs, curs, 0, -1)) return rc;
  int nl = lanes_for(c, n, 8);
  if(nl < 0) return nl;
  const int loss = prms ? prms[0]->lossFunction : p.lossFunction;      // (one loss per call of this function: estimate_batch)
  if(!loss_is_chain_only(loss) && team_serves(c, n) && templates_suit_teams(c, n, refs)) nl = 1;      // the team-persistent kernel takes the whole chip
  // frame stages run on the ctx stream: the other lanes' streams start from a quiet device.  A single lane IS the ctx stream — its
  // launches simply queue behind the frame stage (sequential addFrame: ~30 us of idle device per frame otherwise).
  if(nl > 1) {
    HIP_CK(c, join_pending_normalization(c, c->stream));
    HIP_CK(c, hipStreamSynchronize(c->stream));
  }
  std::vector<int> rcs(nl, BPVO_OK);
  c->frac_valid = false;      // (on the API thread: the lane threads only read the context's settings)
  auto run = [&](int k) {
    const int lo = (int) ((long long) n * k / nl), hi = (int) ((long long) n * (k + 1) / nl);
    rcs[k] = estimate_group(c, &c->lanes[k], hi - lo, wss + lo, refs + lo, curs + lo, T_init ? T_init + 16 * (size_t) lo : nullptr,
                            poses ? poses + 16 * (size_t) lo : nullptr, stats ? stats + (size_t) lo * c->L : nullptr,
                            c->d_records + (size_t) kRecordFloats * lo, nl == 1, prms ? prms + lo : nullptr);
  };
  if(nl == 1) {
    run(0);
  } else {
    std::vector<std::thread> th;
    for(int k = 1; k < nl; ++k) th.emplace_back(run, k);
    run(0);
    for(auto& t : th) t.join();
  }
  for(int k = 0; k < nl; ++k)
    if(rcs[k]) { c->err = c->lanes[k].err; return rcs[k]; }
  resolve_events(c);
  for(int i = 0; i < n; ++i) {
    Workspace& w = c->ws[wss[i]];
    w.last_ref = refs[i];
    w.last_cur = curs[i];
    w.last_level = p.maxTestLevel;
    w.has_estimate = true;
  }
  return BPVO_OK;
}

// tiled device layout (types.h tile_index) -> reference channel-major layout: out[(ch*n + i)*E + e] for records of
// C*E floats per point cut in V-float pieces
void detile_to_channel_major(const float* src, int n, int C, int E, int V, float* out)
{
  const int W = C * E, pieces = W / V;
  for(int i = 0; i < n; ++i)
    for(int w = 0; w < W; ++w) {
      const int piece = w / V, within = w - piece * V;
      const float v = src[(((size_t) (i / kTile) * pieces + piece) * kTile + (size_t) (i % kTile)) * V + within];
      const int ch = w / E, e = w - ch * E;
      out[((size_t) ch * n + i) * E + e] = v;
    }
}
size_t tiled_floats(int n, int floats_per_point) { return (size_t) ((n + kTile - 1) / kTile) * kTile * floats_per_point; }

int refresh_counters(bpvo_hip_ctx* c)
{
  // per-workspace counters (PairJob::cnt), summed here
  std::vector<unsigned long long> all(kWsCounters * (size_t) c->n_pairs);
  HIP_CK(c, hipMemcpy(all.data(), c->d_counters, all.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  unsigned long long h[kWsCounters] = {};
  for(int w = 0; w < c->n_pairs; ++w)
    for(int k = 0; k < kWsCounters; ++k) h[k] += all[kWsCounters * (size_t) w + k];
  c->median_bracketed = h[2];
  c->median_full = h[3];
  c->tscale_passes = h[9]; c->tscale_stages = h[11];
  for(int k = 0; k < 4; ++k) c->tap_counts[k] = h[5 + k];
  c->total_lin = h[1];
  // units of the GN kernels = points linearised (device-side count: only the pairs still active in a launch count)
  // warp_residual at profiling level 1 is timed on a 1-in-kProfileEvery sample of its launches: its units are scaled to
  // the sampled launches so that units / launches stays the points of an average launch
  double all_k6 = 0;
  for(const auto& ln : c->lanes) all_k6 += ln.k6_seq;
  const bool sampled = c->profiling && !c->profile_all && !c->profile_k6_all && all_k6 > 0;
  // (h[4]: the points warp_residual itself processed; workspaces with a frozen scale go through irls_reduce's fused path)
  c->kc_units[KC_WARP_RESIDUAL] = sampled ? (double) h[4] * (double) c->kc_launches[KC_WARP_RESIDUAL] / all_k6 : (double) h[4];
  c->points_fused = (double) h[10];
  c->kc_units[KC_IRLS_REDUCE] = (double) h[0];
  c->kc_units[KC_MEDIAN] = (double) h[0];
  c->kc_units[KC_GN_STEP] = (double) h[1];
  return BPVO_OK;
}

int upload_single_job(bpvo_hip_ctx* c, int ws, int ref, int cur, int level)
{
  PairJob* h = c->lanes[0].h_pjobs;
  h[0] = make_pair_job(c, ws, ref, cur, level);
  for(int k = 0; k < c->G && c->G > 1; ++k) h[1 + k] = group_pair_job(c, h[0], k);      // (wide descriptors: d_job1[1 + k] = channel group k)
  HIP_CK(c, hipMemcpyAsync(c->d_job1, h, sizeof(PairJob) * (size_t) job_tables(c), hipMemcpyHostToDevice, c->stream));
  HIP_CK(c, hipStreamSynchronize(c->stream));   // h_pjobs is reused by the next call
  return BPVO_OK;
}

// Fused path of the estimate loops: the residual / valid buffers of a workspace may lag behind its last linearisation
// (GNState::r_stale).  Everything that reads them goes through here first; the check itself happens on the device.
int ensure_residuals(bpvo_hip_ctx* c, int ws)
{
  Workspace& w = c->ws[ws];
  if(w.last_ref < 0 || c->C != 8) return BPVO_OK;
  int rc = upload_single_job(c, ws, w.last_ref, w.last_cur, w.last_level);
  if(rc) return rc;
  launch_refresh_residuals(c->stream, level_launch(c, c->d_job1, 1, c->frames[w.last_ref].n_host[w.last_level], c->params.lossFunction));
  return BPVO_OK;
}

int fraction_good(bpvo_hip_ctx* c, int ws, float thr, float* frac)
{
  Workspace& w = c->ws[ws];
  if(w.last_ref < 0) return fail(c, BPVO_ERR_NO_DATA, "no linearisation has run on this workspace");
  const int n = c->frames[w.last_ref].n_host[w.last_level];
  if(c->frac_valid && c->frac_ws == ws && c->frac_thr == thr && c->frac_n == n) {      // queued behind the estimate by addFrame
    *frac = vo_fraction_good(c->frac_cnt, n, c->C);
    return BPVO_OK;
  }
  int rc = ensure_residuals(c, ws);
  if(rc) return rc;
  rc = upload_single_job(c, ws, w.last_ref, w.last_cur, w.last_level);
  if(rc) return rc;
  HIP_CK(c, hipMemsetAsync(c->d_count, 0, sizeof(unsigned int), c->stream));
  launch_count_good(c->stream, c->d_job1, n, c->C, c->params.lossFunction, thr, c->d_count);
  unsigned int cnt = 0;
  HIP_CK(c, hipMemcpyAsync(c->h_ints, c->d_count, sizeof(unsigned int), hipMemcpyDeviceToHost, c->stream));
  HIP_CK(c, hipStreamSynchronize(c->stream));
  cnt = (unsigned int) c->h_ints[0];
  *frac = vo_fraction_good(cnt, n, c->C);
  return BPVO_OK;
}

int get_weights_host(bpvo_hip_ctx* c, int ws, std::vector<float>& w_cm, int* n_out)
{
  Workspace& w = c->ws[ws];
  if(w.last_ref < 0) return fail(c, BPVO_ERR_NO_DATA, "no linearisation has run on this workspace");
  const int n = c->frames[w.last_ref].n_host[w.last_level];
  const int C = c->C;
  int rc = ensure_residuals(c, ws);
  if(rc) return rc;
  rc = upload_single_job(c, ws, w.last_ref, w.last_cur, w.last_level);
  if(rc) return rc;
  launch_weights(c->stream, c->d_job1, n, C, c->params.lossFunction, c->d_wtmp);
  std::vector<float> pm((size_t) n * C);
  HIP_CK(c, hipMemcpyAsync(pm.data(), c->d_wtmp, pm.size() * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIP_CK(c, hipStreamSynchronize(c->stream));
  w_cm.resize(pm.size());
  for(int i = 0; i < n; ++i)
    for(int ch = 0; ch < C; ++ch) w_cm[(size_t) ch * n + i] = pm[(size_t) i * C + ch];
  *n_out = n;
  return BPVO_OK;
}

// ---- rig mode: the cameras of a rigid rig estimated as one body pose (rig_math.h, kernels_gn_rig.hip) -------------------------------------
// (Lane 0 on the API thread.  The functions that queue work check with LANE_CK — nothing stays in flight that reads the lane's pinned staging —
// and their callers hand the lane's error to the context: lane_error.)
static int lane_error(bpvo_hip_ctx* c, const Lane* ln, int rc)
{
  if(rc) c->err = ln->err;
  return rc;
}
// Every check of a rig estimate over pyramid levels level_lo .. level_hi, before anything is queued
static int rig_check(bpvo_hip_ctx* c, int n, const int* wss, const int* refs, const int* curs, const float* X, int level_lo, int level_hi)
{
  if(n < 1 || n > c->n_pairs) return fail(c, BPVO_ERR_INVALID_ARG, "rig: n must be within 1 .. the context's workspaces");
  if(!wss || !refs || !curs || !X) return fail(c, BPVO_ERR_INVALID_ARG, "rig: nullptr members / extrinsics");
  // (DisparitySpaceWarp's parameters are no rigid-body twist of the camera frame: Ad(X) does not carry them to the body)
  if(c->dspace) return fail(c, BPVO_ERR_UNSUPPORTED, "rig mode does not serve BPVO_WARP_DISPARITY_SPACE_F32");
  for(int i = 0; i < n; ++i) {
    for(int k = 0; k < i; ++k)
      if(wss[k] == wss[i]) return fail(c, BPVO_ERR_INVALID_ARG, "rig: a workspace appears twice");
    if(!rig_extrinsic_ok(X + 16 * (size_t) i)) return fail(c, BPVO_ERR_INVALID_ARG, "rig: an extrinsic is not a rigid transform (finite, last row 0 0 0 1, R^T R = I within 1e-4)");
  }
  return check_pairs(c, n, wss, refs, curs, level_lo, level_hi);
}
// the members' job tables (every level, as estimate_group lays them out) and extrinsics to the device, on lane 0; max_pts[l]: the most points of a member at level l
static int rig_upload(bpvo_hip_ctx* c, Lane* ln, int n, const int* wss, const int* refs, const int* curs, const float* X, std::vector<int>& max_pts)
{
  const int NP = c->n_pairs;
  const size_t table = (size_t) c->L * NP;
  max_pts.assign((size_t) c->L, 0);
  fill_job_tables(c, ln, 0, n, wss, refs, curs, [](int) { return (const bpvo_hip_params*) nullptr; }, max_pts.data());
  LANE_CK(ln, hipMemcpyAsync(ln->d_pjobs, ln->h_pjobs, sizeof(PairJob) * table * (size_t) job_tables(c), hipMemcpyHostToDevice, ln->stream));
  if(!c->d_rig_X) LANE_CK(ln, c->d_rig_X.alloc(16 * (size_t) NP));
  // (from the caller's pageable memory: the copy has left it when the call returns)
  LANE_CK(ln, hipMemcpyAsync(c->d_rig_X, X, sizeof(float) * 16 * (size_t) n, hipMemcpyHostToDevice, ln->stream));
  return BPVO_OK;
}
// The launch of the members' kernels at a level (fuse_frozen and step_in_reduce stay 0: both assume a step per workspace), and one linearisation
// of every member at its state's pose: the chain's own kernels, the step in its linearise-only mode (what bpvo_hip_linearize queues)
static GNLaunch rig_level_launch(const bpvo_hip_ctx* c, const Lane* ln, int level, int n, int max_points, int loss)
{
  return level_launch(c, ln->d_pjobs + (size_t) level * c->n_pairs, n, max_points, loss);
}
static LinearizeFlags rig_linearize_flags()
{
  LinearizeFlags f;
  f.step_mode = 1;
  f.timers = TIMERS_LEVEL2;
  return f;
}

// the staging of estimate_rigs, allocated at its first use: the table of the call's rigs, their extrinsics and initial poses in ONE pinned block
// (one upload per estimate), the bodies' `active` words of a round
static int rig_storage(bpvo_hip_ctx* c, Lane* ln)
{
  const size_t NP = (size_t) c->n_pairs;
  if(!c->d_rig_stage) LANE_CK(ln, c->d_rig_stage.alloc(rig_stage_bytes(c)));
  if(!c->h_rig_stage) LANE_CK(ln, c->h_rig_stage.alloc(rig_stage_bytes(c)));
  if(!c->d_rig_active) LANE_CK(ln, c->d_rig_active.alloc(NP));
  if(!c->h_rig_active) LANE_CK(ln, c->h_rig_active.alloc(3 * NP));
  return BPVO_OK;
}

// R rigs of ONE loss (the loss instantiates the chain's kernels: estimate_rigs).  The members of all rigs back to back in the job tables, rig
// after rig; body r is state n_pairs + r; one level loop, every launch of the chain shared by all rigs, one launch of the batched rig step
// per iteration.  A rig that has finished a level idles — its body and its members inactive, skipped by every kernel — until every rig has.
static int estimate_rigs_on_lane(bpvo_hip_ctx* c, Lane* ln, int R, const RigProblem* rigs, int loss)
{
  const bpvo_hip_params& p = c->params;
  c->frac_valid = false;
  LANE_CK(ln, join_pending_normalization(c, ln->stream));
  int rc = rig_storage(c, ln);
  if(rc) return rc;
  const int NP = c->n_pairs, L = c->L;
  int N = 0, max_iterations = 0;
  for(int r = 0; r < R; ++r) { N += rigs[r].n; max_iterations = std::max(max_iterations, (rigs[r].prm ? rigs[r].prm : &p)->maxIterations); }
  // The loop iterates on the pose of each rig's REFERENCE member (its member 0) in that member's normalised twist (rig_math.h: the f32 solve wants
  // a normalised system; a rig of one camera takes that camera's own steps): the extrinsics relative to it, its initial pose, and the body pose at the end
  RigEntry* tab = reinterpret_cast<RigEntry*>(c->h_rig_stage.get());
  float* hX = reinterpret_cast<float*>(c->h_rig_stage + rig_stage_X_at(c));
  float* hT = hX + 16 * (size_t) NP;
  char* const d_stage = c->d_rig_stage;
  const float* dX = reinterpret_cast<const float*>(d_stage + rig_stage_X_at(c));
  const float* dT = dX + 16 * (size_t) NP;
  GNState* bodies = c->d_states + NP;
  const size_t table = (size_t) L * NP;
  std::vector<int> max_pts((size_t) L, 0);
  for(int r = 0, first = 0; r < R; first += rigs[r].n, ++r) {
    const RigProblem& q = rigs[r];
    for(int i = 0; i < q.n; ++i) rig_relative_extrinsic(q.X + 16 * (size_t) i, q.X, hX + 16 * (size_t) (first + i));
    rig_member_pose(q.X, q.T_init, hT + 16 * (size_t) r);
    tab[r] = RigEntry{first, q.n, dX + 16 * (size_t) first, bodies + r, dT + 16 * (size_t) r};
    fill_job_tables(c, ln, first, q.n, q.wss, q.refs, q.curs, [&](int) { return q.prm; }, max_pts.data());
  }
  LANE_CK(ln, hipMemcpyAsync(ln->d_pjobs, ln->h_pjobs, sizeof(PairJob) * table * (size_t) job_tables(c), hipMemcpyHostToDevice, ln->stream));
  LANE_CK(ln, hipMemcpyAsync(d_stage, c->h_rig_stage, rig_stage_bytes(c), hipMemcpyHostToDevice, ln->stream));
  launch_set_pose(ln->stream, ln->d_pjobs + (size_t) (L - 1) * NP, nullptr, N);
  const LinearizeFlags members = rig_linearize_flags();
  for(int l = L - 1; l >= p.maxTestLevel; --l) {
    const GNLaunch g = rig_level_launch(c, ln, l, N, max_pts[l], loss);
    launch_level_begin(ln->stream, g.jobs, N, g.max_points, l, 0);
    RigStepsArgs a{g.jobs, reinterpret_cast<const RigEntry*>(d_stage), R, 2, l, l == L - 1 ? 1 : 0, 1, c->d_rig_active};
    launch_rig_steps(ln->stream, a);
    a.mode = 0; a.with_init = 0;
    // the pipelined rounds of the chain (gn_rounds.h): the flags are the BODIES' `active` words (the rig step clears the members' with them), R
    // words in one copy; every rig goes on — a finished one idling — while any body is active
    rc = lane_rounds(ln, max_iterations,
                     [&](int) -> int {
                       for(int k = 0; k < kItersPerSync; ++k) {
                         linearize_launches(c, ln, g, table, members);
                         launch_rig_steps(ln->stream, a);
                       }
                       return BPVO_OK;
                     },
                     [&](int slot) -> int {
                       LANE_CK(ln, hipMemcpyAsync(c->h_rig_active + (size_t) slot * NP, c->d_rig_active, sizeof(int) * (size_t) R, hipMemcpyDeviceToHost, ln->stream));
                       return BPVO_OK;
                     },
                     [&](int slot) {
                       bool any = false;
                       for(int r = 0; r < R; ++r) any = any || c->h_rig_active[(size_t) slot * NP + r] != 0;
                       return any;
                     });
    if(rc) return rc;
  }
  LANE_CK(ln, hipMemcpyAsync(ln->h_states + NP, bodies, sizeof(GNState) * (size_t) R, hipMemcpyDeviceToHost, ln->stream));
  LANE_CK(ln, hipStreamSynchronize(ln->stream));
  LANE_CK(ln, hipGetLastError());
  resolve_events(c);
  for(int r = 0; r < R; ++r) {
    const RigProblem& q = rigs[r];
    const GNState& st = ln->h_states[NP + r];
    rig_body_pose(q.X, st.T_out, q.T_est);      // X_0^-1 T_0 X_0
    if(q.stats)
      for(int l = 0; l < L; ++l) q.stats[l] = st.stats[l];
    for(int i = 0; i < q.n; ++i) {
      Workspace& w = c->ws[q.wss[i]];
      w.last_ref = q.refs[i]; w.last_cur = q.curs[i]; w.last_level = p.maxTestLevel;
      w.has_estimate = true;
    }
  }
  return BPVO_OK;
}
static int estimate_rigs_one_loss(bpvo_hip_ctx* c, int R, const RigProblem* rigs, int loss)
{
  (void) hipSetDevice(c->device);
  Lane* ln = &c->lanes[0];      // (the context's stream: the estimate queues behind the frame stages)
  return lane_error(c, ln, estimate_rigs_on_lane(c, ln, R, rigs, loss));
}

// Rigs with different losses in one call: one estimate per loss present, the rigs of a loss in call order (what estimate_batch does for sequences
// with parameters of their own; everything else a rig may own travels in its members' jobs and its body's state)
int estimate_rigs(bpvo_hip_ctx* c, int R, const RigProblem* rigs)
{
  const bpvo_hip_params& p = c->params;
  if(R < 1 || !rigs) return fail(c, BPVO_ERR_INVALID_ARG, "rigs: n_rigs must be at least 1");
  int N = 0;
  for(int r = 0; r < R; ++r) {
    if(!rigs[r].T_init || !rigs[r].T_est) return fail(c, BPVO_ERR_INVALID_ARG, "nullptr pose");
    if(int rc = rig_check(c, rigs[r].n, rigs[r].wss, rigs[r].refs, rigs[r].curs, rigs[r].X, p.maxTestLevel, c->L - 1)) return rc;
    N += rigs[r].n;
    for(int q = 0; q < r; ++q)
      for(int i = 0; i < rigs[r].n; ++i)
        for(int k = 0; k < rigs[q].n; ++k)
          if(rigs[r].wss[i] == rigs[q].wss[k]) return fail(c, BPVO_ERR_INVALID_ARG, "rigs: a workspace appears in two rigs");
  }
  if(N > c->n_pairs) return fail(c, BPVO_ERR_INVALID_ARG, "rigs: more members than the context's workspaces");
  auto loss_of = [&](int r) { return (rigs[r].prm ? rigs[r].prm : &p)->lossFunction; };
  return for_each_loss(R, loss_of, [&](const std::vector<int>& at) {
    if((int) at.size() == R) return estimate_rigs_one_loss(c, R, rigs, loss_of(0));
    std::vector<RigProblem> part;
    for(int r : at) part.push_back(rigs[r]);
    return estimate_rigs_one_loss(c, (int) part.size(), part.data(), loss_of(at[0]));
  });
}

// one rig: the R = 1 case
int estimate_rig(bpvo_hip_ctx* c, int n, const int* wss, const int* refs, const int* curs, const float* X, const float* T_init, float* T_est, bpvo_hip_stats* stats)
{
  if(!T_init || !T_est) return fail(c, BPVO_ERR_INVALID_ARG, "nullptr pose");
  const RigProblem q{n, wss, refs, curs, X, T_init, T_est, stats, nullptr};
  return estimate_rigs(c, 1, &q);
}

}  // namespace bpvo_hip_host

extern "C" {

// the members' linearisations at the body pose and the joint one, queued on lane 0 and waited for: the body's state in ln->h_states[n_pairs]
static int linearize_rig_on_lane(bpvo_hip_ctx* c, Lane* ln, int n, const int* wss, const int* refs, const int* curs, const float* X, int level,
                                 const float T_body[16], int reset_scale, float* T_members)
{
  LANE_CK(ln, join_pending_normalization(c, ln->stream));
  std::vector<int> max_pts;
  if(int rc = rig_upload(c, ln, n, wss, refs, curs, X, max_pts)) return rc;
  const int NP = c->n_pairs;
  GNState* body = c->d_states + NP;
  for(int i = 0; i < n; ++i) rig_member_pose(X + 16 * (size_t) i, T_body, ln->h_T + 16 * (size_t) i);      // the poses the members' kernels run at
  if(T_members) std::memcpy(T_members, ln->h_T, sizeof(float) * 16 * (size_t) n);
  LANE_CK(ln, hipMemcpyAsync(ln->d_Tinit, ln->h_T, sizeof(float) * 16 * (size_t) n, hipMemcpyHostToDevice, ln->stream));
  const GNLaunch g = rig_level_launch(c, ln, level, n, max_pts[level], c->params.lossFunction);
  for(int i = 0; i < n; ++i) launch_prepare_linearize(ln->stream, g.jobs + i, ln->d_Tinit + 16 * (size_t) i, reset_scale ? 1 : 0, level);
  launch_reset_tapkeys(ln->stream, g);
  linearize_launches(c, ln, g, (size_t) c->L * NP, rig_linearize_flags());
  launch_rig_step(ln->stream, RigStepArgs{g.jobs, n, c->d_rig_X, body, 1, level, nullptr, 0});
  LANE_CK(ln, hipMemcpyAsync(ln->h_states + NP, body, sizeof(GNState), hipMemcpyDeviceToHost, ln->stream));
  LANE_CK(ln, hipStreamSynchronize(ln->stream));
  LANE_CK(ln, hipGetLastError());
  return BPVO_OK;
}
int bpvo_hip_linearize_rig(bpvo_hip_ctx* c, int n, const int* wss, const int* refs, const int* curs, const float* X, int level, const float T_body[16],
                           int reset_scale, float H[36], float G[6], float* f_norm, int* num_valid, float* T_members)
{
  CHECK_CTX(c); CHECK_LEVEL(c, level);
  if(!T_body || !H || !G || !f_norm || !num_valid) return fail(c, BPVO_ERR_INVALID_ARG, "nullptr pose / outputs");
  int rc = rig_check(c, n, wss, refs, curs, X, level, level);
  if(rc) return rc;
  (void) hipSetDevice(c->device);
  Lane* ln = &c->lanes[0];
  c->frac_valid = false;
  rc = lane_error(c, ln, linearize_rig_on_lane(c, ln, n, wss, refs, curs, X, level, T_body, reset_scale, T_members));
  if(rc) return rc;
  resolve_events(c);
  const GNState& st = ln->h_states[c->n_pairs];
  std::memcpy(H, st.H, sizeof(st.H));
  std::memcpy(G, st.G, sizeof(st.G));
  *f_norm = st.f_norm;
  *num_valid = (int) st.n_valid;
  for(int i = 0; i < n; ++i) {
    Workspace& w = c->ws[wss[i]];
    w.last_ref = refs[i]; w.last_cur = curs[i]; w.last_level = level;
    w.has_estimate = false;
  }
  return BPVO_OK;
}
int bpvo_hip_estimate_pose_rig(bpvo_hip_ctx* c, int n, const int* wss, const int* refs, const int* curs, const float* X, const float T_init[16],
                               float T_est[16], bpvo_hip_stats* stats)
{
  CHECK_CTX(c);
  return estimate_rig(c, n, wss, refs, curs, X, T_init, T_est, stats);
}
int bpvo_hip_estimate_pose_rigs(bpvo_hip_ctx* c, int n_rigs, const int* count, const int* wss, const int* refs, const int* curs, const float* X,
                                const float* T_init, float* T_est, bpvo_hip_stats* stats)
{
  CHECK_CTX(c);
  if(n_rigs < 1 || n_rigs > c->n_pairs) return fail(c, BPVO_ERR_INVALID_ARG, "rigs: n_rigs must be within 1 .. the context's workspaces");
  if(!count || !wss || !refs || !curs || !X) return fail(c, BPVO_ERR_INVALID_ARG, "rigs: nullptr counts / members / extrinsics");
  if(!T_init || !T_est) return fail(c, BPVO_ERR_INVALID_ARG, "nullptr pose");
  std::vector<RigProblem> rigs((size_t) n_rigs);
  size_t at = 0;
  for(int r = 0; r < n_rigs; ++r) {
    if(count[r] < 1 || count[r] > c->n_pairs) return fail(c, BPVO_ERR_INVALID_ARG, "rigs: every rig has 1 .. the context's workspaces members");
    rigs[r] = RigProblem{count[r], wss + at, refs + at, curs + at, X + 16 * at, T_init + 16 * (size_t) r, T_est + 16 * (size_t) r,
                         stats ? stats + (size_t) r * c->L : nullptr, nullptr};
    at += (size_t) count[r];
  }
  return estimate_rigs(c, n_rigs, rigs.data());
}

}  // extern "C"

namespace bpvo_hip_host {

int check_template_not_empty(bpvo_hip_ctx* c, int ref_slot)
{
  if(ref_slot < 0 || ref_slot >= c->n_frames || !c->frames[ref_slot].has_template) return BPVO_OK;   // reported elsewhere
  for(int l = c->params.maxTestLevel; l < c->L; ++l)
    if(c->frames[ref_slot].n_host[l] <= 0) return fail(c, BPVO_ERR_NO_TEMPLATE, "you should call setData before calling computeResiduals");
  return BPVO_OK;
}

}  // namespace bpvo_hip_host

extern "C" {

// ---- operator-level seam --------------------------------------------------------------------------------------------
static int linearize_impl(bpvo_hip_ctx* c, int ws, int ref_slot, int cur_slot, int level, const float T[16], int reset_scale, float given_scale,
                          float H[36], float G[6], float* f_norm, float* sigma, int* num_valid)
{
  CHECK_CTX(c); CHECK_LEVEL(c, level);
  if(int rc0 = check_pairs(c, 1, &ws, &ref_slot, &cur_slot, level, level)) return rc0;
  c->frac_valid = false;
  (void) hipSetDevice(c->device);
  int rc = upload_single_job(c, ws, ref_slot, cur_slot, level);
  if(rc) return rc;
  Lane& l0 = c->lanes[0];
  std::memcpy(l0.h_T, T, 16 * sizeof(float));
  HIP_CK(c, hipMemcpyAsync(l0.d_Tinit, l0.h_T, 16 * sizeof(float), hipMemcpyHostToDevice, c->stream));
  launch_prepare_linearize(c->stream, c->d_job1, l0.d_Tinit, reset_scale, level, given_scale);
  const GNLaunch g = level_launch(c, c->d_job1, 1, c->frames[ref_slot].n_host[level], c->params.lossFunction);
  launch_reset_tapkeys(c->stream, g);
  LinearizeFlags f;      // (lane 0 is the context's stream; every launch timed, the step in its linearise-only mode; d_job1[1 + k]: channel group k)
  f.step_mode = 1;
  f.timers = TIMERS_ALWAYS;
  linearize_launches(c, &l0, g, 1, f);
  HIP_CK(c, hipMemcpyAsync(l0.h_states, c->d_states + ws, sizeof(GNState), hipMemcpyDeviceToHost, c->stream));
  HIP_CK(c, hipStreamSynchronize(c->stream));
  HIP_CK(c, hipGetLastError());
  resolve_events(c);
  const GNState& st = l0.h_states[0];
  std::memcpy(H, st.H, sizeof(st.H));
  std::memcpy(G, st.G, sizeof(st.G));
  *f_norm = st.f_norm;
  if(sigma) *sigma = st.scale;
  *num_valid = (int) st.n_valid;
  c->ws[ws].last_ref = ref_slot; c->ws[ws].last_cur = cur_slot; c->ws[ws].last_level = level;
  c->ws[ws].has_estimate = false;
  return BPVO_OK;
}
int bpvo_hip_linearize(bpvo_hip_ctx* c, int ws, int ref_slot, int cur_slot, int level, const float T[16], int reset_scale,
                       float H[36], float G[6], float* f_norm, float* sigma, int* num_valid)
{
  return linearize_impl(c, ws, ref_slot, cur_slot, level, T, reset_scale ? 1 : 0, 0.0f, H, G, f_norm, sigma, num_valid);
}
int bpvo_hip_linearize_at_scale(bpvo_hip_ctx* c, int ws, int ref_slot, int cur_slot, int level, const float T[16], float sigma,
                                float H[36], float G[6], float* f_norm, int* num_valid)
{
  if(c && !(sigma > 0.0f)) return fail(c, BPVO_ERR_INVALID_ARG, "sigma must be positive");
  return linearize_impl(c, ws, ref_slot, cur_slot, level, T, 2, sigma, H, G, f_norm, nullptr, num_valid);
}

int bpvo_hip_get_residuals(bpvo_hip_ctx* c, int ws, float* r, size_t* n_out)
{
  CHECK_CTX(c); CHECK_WS(c, ws);
  Workspace& w = c->ws[ws];
  if(w.last_ref < 0) return fail(c, BPVO_ERR_NO_DATA, "no linearisation has run on this workspace");
  const int n = c->frames[w.last_ref].n_host[w.last_level], C = c->C;
  if(n_out) *n_out = (size_t) n * C;
  if(!r) return BPVO_OK;
  (void) hipSetDevice(c->device);
  { int rc = ensure_residuals(c, ws); if(rc) return rc; }
  std::vector<float> t(tiled_floats(n, C));
  if(n) HIP_CK(c, hipMemcpyAsync(t.data(), w.r, t.size() * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIP_CK(c, hipStreamSynchronize(c->stream));
  detile_to_channel_major(t.data(), n, C, 1, C == 8 ? 4 : C, r);
  return BPVO_OK;
}
int bpvo_hip_get_valid(bpvo_hip_ctx* c, int ws, uint16_t* v, size_t* n_out)
{
  CHECK_CTX(c); CHECK_WS(c, ws);
  Workspace& w = c->ws[ws];
  if(w.last_ref < 0) return fail(c, BPVO_ERR_NO_DATA, "no linearisation has run on this workspace");
  const int n = c->frames[w.last_ref].n_host[w.last_level];
  if(n_out) *n_out = (size_t) n;
  if(!v) return BPVO_OK;
  (void) hipSetDevice(c->device);
  { int rc = ensure_residuals(c, ws); if(rc) return rc; }
  std::vector<uint8_t> b((size_t) n);
  HIP_CK(c, hipMemcpyAsync(b.data(), w.valid, b.size(), hipMemcpyDeviceToHost, c->stream));
  HIP_CK(c, hipStreamSynchronize(c->stream));
  for(int i = 0; i < n; ++i) v[i] = b[i];
  return BPVO_OK;
}
int bpvo_hip_get_weights(bpvo_hip_ctx* c, int ws, float* w, size_t* n_out)
{
  CHECK_CTX(c); CHECK_WS(c, ws);
  Workspace& wk = c->ws[ws];
  if(wk.last_ref < 0) return fail(c, BPVO_ERR_NO_DATA, "no linearisation has run on this workspace");
  const int n0 = c->frames[wk.last_ref].n_host[wk.last_level];
  if(n_out) *n_out = (size_t) n0 * c->C;
  if(!w) return BPVO_OK;
  (void) hipSetDevice(c->device);
  std::vector<float> cm;
  int n = 0;
  int rc = get_weights_host(c, ws, cm, &n);
  if(rc) return rc;
  std::memcpy(w, cm.data(), cm.size() * sizeof(float));
  return BPVO_OK;
}
int bpvo_hip_fraction_good(bpvo_hip_ctx* c, int ws, float threshold, float* frac)
{
  CHECK_CTX(c); CHECK_WS(c, ws);
  (void) hipSetDevice(c->device);
  return fraction_good(c, ws, threshold, frac);
}

// TemplateData::computeResiduals throws on an empty template (reference: bpvo/template_data.cc:177).  The single-pair entry
// points mirror that; the batch entry points skip such levels of the affected pair (its statistics keep kSolverError).

int bpvo_hip_set_warp_formulation(bpvo_hip_ctx* c, int mode)
{
  CHECK_CTX(c);
  if(mode != BPVO_WARP_PHOTO_ERROR_F64 && mode != BPVO_WARP_PROJECT_POINTS_F32 && mode != BPVO_WARP_DISPARITY_SPACE_F32)
    return fail(c, BPVO_ERR_INVALID_ARG, "unknown warp formulation");
  if(mode != BPVO_WARP_PHOTO_ERROR_F64 && c->params.interp != BPVO_INTERP_LINEAR)
    return fail(c, BPVO_ERR_UNSUPPORTED, "the f32 formulations are kLinear only (bpvo/photo_error.cc:118-214)");
  const int dspace = (mode == BPVO_WARP_DISPARITY_SPACE_F32) ? 1 : 0;
  if(dspace != c->dspace) {
    // templates hold the points / gradients of the other warp: they have to be rebuilt (frame data stays)
    for(auto& f : c->frames) f.has_template = false;
  }
  c->dspace = dspace;
  c->fast_warp = (mode != BPVO_WARP_PHOTO_ERROR_F64) ? 1 : 0;
  return BPVO_OK;
}

int bpvo_hip_estimate_pose(bpvo_hip_ctx* c, int ws, int ref_slot, int cur_slot, const float T_init[16], float T_est[16],
                           bpvo_hip_stats* stats)
{
  CHECK_CTX(c); CHECK_WS(c, ws);
  if(!T_init || !T_est) return fail(c, BPVO_ERR_INVALID_ARG, "nullptr pose");
  if(int rc = check_template_not_empty(c, ref_slot)) return rc;
  (void) hipSetDevice(c->device);
  return estimate_batch(c, 1, &ws, &ref_slot, &cur_slot, T_init, T_est, stats);
}

int bpvo_hip_estimate_pose_trace(bpvo_hip_ctx* c, int ws, int ref_slot, int cur_slot, const float T_init[16], float T_est[16],
                                 bpvo_hip_stats* stats, float* records, int max_records, int* n_records)
{
  CHECK_CTX(c); CHECK_WS(c, ws);
  if(!T_init || !T_est || !n_records || max_records < 0 || (max_records > 0 && !records)) return fail(c, BPVO_ERR_INVALID_ARG, "nullptr pose / records");
  if(int rc = check_template_not_empty(c, ref_slot)) return rc;
  (void) hipSetDevice(c->device);
  const size_t cap = (size_t) kTraceFloats * c->L * (max_linearizations(c->params.maxIterations) + 1);
  if(cap > c->d_trace.size()) {
    HIP_CK(c, hipStreamSynchronize(c->stream));
    HIP_CK(c, c->d_trace.reserve(cap));
  }
  c->trace_ws = ws;
  const int rc = estimate_batch(c, 1, &ws, &ref_slot, &cur_slot, T_init, T_est, stats);
  c->trace_ws = -1;
  if(rc) return rc;
  const int n = c->lanes[0].h_states[ws].trace_n;
  *n_records = n;
  const int ncopy = std::min(std::min(n, max_records), (int) (c->d_trace.size() / kTraceFloats));
  if(ncopy > 0) HIP_CK(c, hipMemcpy(records, c->d_trace, sizeof(float) * kTraceFloats * (size_t) ncopy, hipMemcpyDeviceToHost));
  return BPVO_OK;
}

// ---- batches --------------------------------------------------------------------------------------------------------
int bpvo_hip_batch_estimate(bpvo_hip_ctx* c, int n_pairs, const float* T_init, float* poses, bpvo_hip_stats* stats)
{
  CHECK_CTX(c);
  if(n_pairs < 0 || 2 * n_pairs > c->n_frames || n_pairs > c->n_pairs) return fail(c, BPVO_ERR_INVALID_ARG, "batch exceeds ctx capacity");
  (void) hipSetDevice(c->device);
  std::vector<int> wss(n_pairs), refs(n_pairs), curs(n_pairs);
  for(int p = 0; p < n_pairs; ++p) { wss[p] = p; refs[p] = 2 * p; curs[p] = 2 * p + 1; }
  return estimate_batch(c, n_pairs, wss.data(), refs.data(), curs.data(), T_init, poses, stats);
}

}  // extern "C"
