// Test harness: bpvo_amd/csrc/gn_rounds.h — the pipelined rounds of the four-kernel chain — compiled by a plain C++ compiler (no HIP anywhere:
// that it compiles is the proof that the header is host-only).  The host side is the real run_rounds, driven the way estimate.hip drives it for
// cameras (run_level_chain) and for rigs (estimate_rigs); the device is a fake that executes what is queued in order: workspace i leaves the
// active set after finish[i] iterations and estimates its scale for the first freeze[i] of them.  Every call of a callable goes into a log
// that tests/test_gn_rounds_cpu.py reads.
#include <vector>

#include "gn_rounds.h"

using namespace bpvo_hip_host;

namespace {

enum { QUEUE_ITERATIONS = 0, QUEUE_FLAGS = 1, WAIT = 2, READ = 3 };      // log records {kind, a, b, c, d}

struct Log {
  int* out; int cap; int n = 0;
  void add(int kind, int a, int b = 0, int c = 0, int d = 0)
  {
    if(5 * (n + 1) <= cap) { int* p = out + 5 * n; p[0] = kind; p[1] = a; p[2] = b; p[3] = c; p[4] = d; }
    ++n;
  }
};

struct Slot { std::vector<int> list; int count = 0, moving = 0; bool marked = false; };

}  // namespace

extern "C" {

int gr_iters_per_sync() { return kItersPerSync; }
int gr_max_fun_evals() { return kMaxFunEvals; }
int gr_max_linearizations(int max_iterations) { return max_linearizations(max_iterations); }
int gr_max_rounds(int max_iterations) { return max_rounds(max_iterations); }

// One level of n cameras.  done[i] <- the iterations workspace i was given while active.  log records:
//   {QUEUE_ITERATIONS, round, workspaces dispatched, warp launched, median launched}   {QUEUE_FLAGS, slot, 1 if the slot was still marked}
//   {WAIT, slot, 1 if the slot was marked}   {READ, slot, count, how many of them estimate their scale}
// Returns run_rounds' value; fail_at >= 0: queue_flags fails with 7 at that round.
int gr_run_cameras(int max_iterations, int n, const int* finish, const int* freeze, int l2_moot, int fused_path, int fail_at, int* done, int* log_out, int log_cap,
                   int* n_log)
{
  Log log{log_out, log_cap};
  // the device: the state machine enforces the limit of linearisations whatever the host queues
  const int limit = max_linearizations(max_iterations);
  std::vector<char> active((size_t) n, 1);
  for(int i = 0; i < n; ++i) done[i] = 0;
  Slot slots[3];
  // the host, as run_level_chain keeps it
  int n_cur = n, flags_queued = 0;
  const std::vector<int>* list = nullptr;      // null: every workspace, in order
  bool none_moving = l2_moot != 0;
  auto entry = [&](int k) { return list ? (*list)[(size_t) k] : k; };
  const int rc = run_rounds(max_iterations,
    [&](int round) {
      const bool median = !none_moving, warp = !(none_moving && fused_path);
      log.add(QUEUE_ITERATIONS, round, n_cur, warp, median);
      for(int it = 0; it < kItersPerSync; ++it)
        for(int k = 0; k < n_cur; ++k) {
          const int i = entry(k);
          if(!active[i]) continue;
          ++done[i];
          if(done[i] >= finish[i] || done[i] >= limit) active[i] = 0;
        }
      return 0;
    },
    [&](int slot) {
      Slot& s = slots[slot];
      log.add(QUEUE_FLAGS, slot, s.marked);
      if(flags_queued++ == fail_at) return 7;
      std::vector<int> out;
      int moving = 0;
      for(int k = 0; k < n_cur; ++k) {
        const int i = entry(k);
        if(!active[i]) continue;
        out.push_back(i);
        moving += done[i] < freeze[i];
      }
      s.list = out; s.count = (int) out.size(); s.moving = moving; s.marked = true;
      return 0;
    },
    [&](int slot) { log.add(WAIT, slot, slots[slot].marked); return 0; },
    [&](int slot) {
      Slot& s = slots[slot];
      log.add(READ, slot, s.count, s.moving);
      s.marked = false;
      if(s.count <= 0) return false;
      n_cur = s.count;
      none_moving = none_moving || s.moving == 0;
      list = &s.list;
      return true;
    });
  *n_log = log.n;
  return rc;
}

// One level of R rigs: body r is active for finish[r] iterations; the flags of a round are the bodies' `active` words, and every rig is dispatched
// while any of them is set.  log records as above, {QUEUE_ITERATIONS, round, R, 1, 1} and {READ, slot, bodies still active, 0}.
int gr_run_rigs(int max_iterations, int R, const int* finish, int* done, int* log_out, int log_cap, int* n_log)
{
  Log log{log_out, log_cap};
  const int limit = max_linearizations(max_iterations);
  std::vector<int> active((size_t) R, 1);
  for(int r = 0; r < R; ++r) done[r] = 0;
  std::vector<int> words[3];
  bool marked[3] = {false, false, false};
  const int rc = run_rounds(max_iterations,
    [&](int round) {
      log.add(QUEUE_ITERATIONS, round, R, 1, 1);
      for(int it = 0; it < kItersPerSync; ++it)
        for(int r = 0; r < R; ++r) {
          if(!active[r]) continue;
          ++done[r];
          if(done[r] >= finish[r] || done[r] >= limit) active[r] = 0;
        }
      return 0;
    },
    [&](int slot) { log.add(QUEUE_FLAGS, slot, marked[slot]); words[slot] = active; marked[slot] = true; return 0; },
    [&](int slot) { log.add(WAIT, slot, marked[slot]); return 0; },
    [&](int slot) {
      int left = 0;
      for(int r = 0; r < R; ++r) left += words[slot][(size_t) r] != 0;
      log.add(READ, slot, left, 0);
      marked[slot] = false;
      return left != 0;
    });
  *n_log = log.n;
  return rc;
}

}  // extern "C"
