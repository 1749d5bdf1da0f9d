// The owner types of bpvo_amd/csrc/device_owned.h over a fake runtime, for tests/test_device_owned_cpu.py: this file includes only that header —
// compiled by the host's C++ compiler, which proves it free of HIP.  The fake hands out real malloc blocks (a double release or a leak is the
// sanitizers' to see), counts what is live per kind, logs every call and can be told to fail the k-th acquisition.
//   device_owned_harness CASE      prints "ok CASE"; a failed check prints its line to stderr and exits 1
#include "device_owned.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

using namespace bpvo_hip_host;

namespace {

struct Fake {
  using status = int;
  struct StreamRec;
  struct EventRec;
  using stream_t = StreamRec*;
  using event_t = EventRec*;
  static constexpr status ok = 0;
  static constexpr status failed = 2;
  static int live[RES_KINDS];
  static int acquisitions, fail_at;      // fail_at = k: the k-th acquisition from now fails (1-based; 0: none)
  static unsigned last_event_flags;
  static std::vector<std::string> log;

  static void arm(int k) { acquisitions = 0; fail_at = k; }
  static status acquire(int kind, void** p, size_t bytes)
  {
    if(++acquisitions == fail_at) { log.push_back("fail"); return failed; }
    *p = std::malloc(bytes ? bytes : 1);
    ++live[kind];
    log.push_back("acquire");
    return ok;
  }
  static void release(int kind, void* p)
  {
    std::free(p);
    --live[kind];
    log.push_back("release");
  }
  static status alloc(ResourceKind kind, void** p, size_t bytes) { return acquire(kind, p, bytes); }
  static void free(ResourceKind kind, void* p) { release(kind, p); }
  static status create(stream_t* s, unsigned) { return acquire(RES_STREAM, reinterpret_cast<void**>(s), 1); }
  static status create(event_t* e, unsigned flags) { last_event_flags = flags; return acquire(RES_EVENT, reinterpret_cast<void**>(e), 1); }
  static void destroy(stream_t s) { release(RES_STREAM, s); }
  static void destroy(event_t e) { release(RES_EVENT, e); }
};
int Fake::live[RES_KINDS] = {};
int Fake::acquisitions = 0, Fake::fail_at = 0;
unsigned Fake::last_event_flags = 0;
std::vector<std::string> Fake::log;

template <class T> using DeviceBuf = BasicBuf<T, Fake, RES_DEVICE>;
template <class T> using PinnedBuf = BasicBuf<T, Fake, RES_PINNED>;
using Stream = BasicHandle<Fake::stream_t, Fake, RES_STREAM>;
using Event = BasicHandle<Fake::event_t, Fake, RES_EVENT>;

#define CHECK(cond) do { if(!(cond)) { std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } } while(0)

// the fake's counts and the header's own agree, kind by kind
bool live_is(int device, int pinned, int streams, int events)
{
  const int want[RES_KINDS] = {device, pinned, streams, events};
  for(int k = 0; k < RES_KINDS; ++k)
    if(Fake::live[k] != want[k] || g_live_resources[k].load() != want[k]) return false;
  return true;
}

void case_scope()
{
  {
    DeviceBuf<float> d;
    PinnedBuf<int> h;
    Stream s;
    Event e;
    CHECK(!d && !h && !s && !e && d.size() == 0 && d.get() == nullptr);
    CHECK(d.alloc(100) == Fake::ok && h.alloc(7) == Fake::ok && s.create() == Fake::ok && e.create(2u) == Fake::ok);
    CHECK(Fake::last_event_flags == 2u);
    CHECK(d && h && s && e && d.size() == 100 && h.size() == 7);
    float* p = d;      // converts like the raw pointer: writes go to the whole block
    for(int i = 0; i < 100; ++i) p[i] = (float) i;
    h[6] = 42;
    CHECK(d[99] == 99.0f && h[6] == 42 && d + 1 == p + 1);
    CHECK(live_is(1, 1, 1, 1));
  }
  CHECK(live_is(0, 0, 0, 0));
  // reset by hand, twice: the second finds nothing to release
  DeviceBuf<char> d;
  CHECK(d.alloc(5) == Fake::ok);
  d.reset();
  d.reset();
  CHECK(!d && d.size() == 0 && live_is(0, 0, 0, 0));
}

void case_reserve_keeps()
{
  DeviceBuf<int> d;
  CHECK(d.reserve(64) == Fake::ok && d.size() == 64);
  int* const p = d;
  const size_t calls = Fake::log.size();
  CHECK(d.reserve(64) == Fake::ok && d.reserve(63) == Fake::ok && d.reserve(1) == Fake::ok && d.reserve(0) == Fake::ok);
  CHECK(d.get() == p && d.size() == 64 && Fake::log.size() == calls && live_is(1, 0, 0, 0));
}

void case_reserve_grows()
{
  PinnedBuf<int> h;
  CHECK(h.reserve(8) == Fake::ok);
  Fake::log.clear();
  CHECK(h.reserve(9) == Fake::ok && h.size() == 9 && h);
  // the old block goes before the new one comes: never two at a time
  CHECK(Fake::log.size() == 2 && Fake::log[0] == "release" && Fake::log[1] == "acquire");
  h[8] = 1;
  CHECK(live_is(0, 1, 0, 0));
}

void case_reserve_fails()
{
  DeviceBuf<double> d;
  CHECK(d.alloc(4) == Fake::ok);
  Fake::log.clear();
  Fake::arm(1);
  CHECK(d.reserve(5) == Fake::failed);
  CHECK(!d && d.get() == nullptr && d.size() == 0 && live_is(0, 0, 0, 0));
  CHECK(Fake::log.size() == 2 && Fake::log[0] == "release" && Fake::log[1] == "fail");
  CHECK(d.reserve(5) == Fake::ok && d && d.size() == 5 && live_is(1, 0, 0, 0));
  d[4] = 1.0;
  // a failed alloc of an empty buffer, a failed stream and a failed event leave them empty too
  DeviceBuf<int> e;
  Stream s;
  Event ev;
  Fake::arm(1); CHECK(e.alloc(3) == Fake::failed && !e && e.size() == 0);
  Fake::arm(1); CHECK(s.create() == Fake::failed && !s);
  Fake::arm(1); CHECK(ev.create(0u) == Fake::failed && !ev);
  CHECK(live_is(1, 0, 0, 0));
}

void case_zero()
{
  DeviceBuf<int> d;
  PinnedBuf<int> h;
  Fake::log.clear();
  CHECK(d.alloc(0) == Fake::ok && h.reserve(0) == Fake::ok);
  CHECK(!d && !h && d.size() == 0 && h.size() == 0 && Fake::log.empty() && live_is(0, 0, 0, 0));
  CHECK(d.alloc(0) == Fake::ok && d.alloc(3) == Fake::ok && d.size() == 3);      // (still empty after alloc(0): alloc is allowed)
}

void case_moves()
{
  DeviceBuf<int> a;
  CHECK(a.alloc(10) == Fake::ok);
  int* const pa = a;
  DeviceBuf<int> b(std::move(a));      // construction: the source is left empty
  CHECK(!a && a.size() == 0 && b.get() == pa && b.size() == 10 && live_is(1, 0, 0, 0));
  DeviceBuf<int> c;
  CHECK(c.alloc(20) == Fake::ok && live_is(2, 0, 0, 0));
  int* const pc = c;
  b = std::move(c);      // assignment onto a full owner: what it held is released
  CHECK(!c && c.size() == 0 && b.get() == pc && b.size() == 20 && live_is(1, 0, 0, 0));
  DeviceBuf<int>& self = b;
  b = std::move(self);      // onto itself: nothing happens
  CHECK(b.get() == pc && b.size() == 20 && live_is(1, 0, 0, 0));
  b[19] = 7;

  Stream s, t;
  Event e, f;
  CHECK(s.create() == Fake::ok && t.create() == Fake::ok && e.create(0u) == Fake::ok && f.create(2u) == Fake::ok && live_is(1, 0, 2, 2));
  Fake::stream_t const ps = s;
  Fake::event_t const pe = e;
  t = std::move(s);
  f = std::move(e);
  CHECK(!s && !e && t.get() == ps && f.get() == pe && live_is(1, 0, 1, 1));
  Stream& ts = t;
  Event& fs = f;
  t = std::move(ts);
  f = std::move(fs);
  CHECK(t.get() == ps && f.get() == pe && live_is(1, 0, 1, 1));
  Stream u(std::move(t));
  Event g(std::move(f));
  CHECK(!t && !f && u.get() == ps && g.get() == pe && live_is(1, 0, 1, 1));
}

struct Bundle {
  DeviceBuf<int> d;
  PinnedBuf<int> h;
  Stream s;
  Event e;
  int tag = 0;
};

void case_vector()
{
  {
    std::vector<Bundle> v;
    for(int i = 0; i < 100; ++i) {      // grown an element at a time: every reallocation moves what is there
      v.emplace_back();
      Bundle& b = v.back();
      b.tag = i;
      CHECK(b.d.alloc((size_t) i + 1) == Fake::ok && b.h.alloc(2) == Fake::ok && b.s.create() == Fake::ok && b.e.create(2u) == Fake::ok);
      b.d[i] = i;
      b.h[1] = -i;
      CHECK(live_is(i + 1, i + 1, i + 1, i + 1));
    }
    for(int i = 0; i < 100; ++i) CHECK(v[i].tag == i && v[i].d.size() == (size_t) i + 1 && v[i].d[i] == i && v[i].h[1] == -i && v[i].s && v[i].e);
    v.erase(v.begin(), v.begin() + 50);      // (move assignment onto full owners, 50 times over)
    CHECK(live_is(50, 50, 50, 50) && v[0].tag == 50 && v[0].d[50] == 50);
  }
  CHECK(live_is(0, 0, 0, 0));
}

// one owner of each kind, acquired in turn; the first failure is returned with whatever came before it still in `b`
int build(Bundle& b)
{
  if(int e = b.d.alloc(16)) return e;
  if(int e = b.h.alloc(16)) return e;
  if(int e = b.s.create()) return e;
  if(int e = b.e.create(2u)) return e;
  return Fake::ok;
}

void case_build_fails()
{
  for(int k = 1; k <= 5; ++k) {      // (k = 5: nothing fails)
    {
      Bundle b;
      Fake::arm(k);
      const int rc = build(b);
      CHECK(rc == (k <= 4 ? Fake::failed : Fake::ok));
      CHECK(live_is(k > 1, k > 2, k > 3, k > 4));
      CHECK((bool) b.d == (k > 1) && (bool) b.h == (k > 2) && (bool) b.s == (k > 3) && (bool) b.e == (k > 4));
    }
    CHECK(live_is(0, 0, 0, 0));
  }
}

const struct { const char* name; void (*run)(); } kCases[] = {
  {"scope", case_scope}, {"reserve_keeps", case_reserve_keeps}, {"reserve_grows", case_reserve_grows}, {"reserve_fails", case_reserve_fails},
  {"zero", case_zero}, {"moves", case_moves}, {"vector", case_vector}, {"build_fails", case_build_fails},
};

}  // namespace

int main(int argc, char** argv)
{
  if(argc == 2 && !std::strcmp(argv[1], "list")) {
    for(const auto& c : kCases) std::printf("%s\n", c.name);
    return 0;
  }
  for(const auto& c : kCases) {
    if(argc != 2 || std::strcmp(argv[1], c.name)) continue;
    Fake::arm(0);
    c.run();
    Fake::arm(0);
    // whatever the case still held went with its scope
    if(!live_is(0, 0, 0, 0)) { std::fprintf(stderr, "%s: resources live after the case\n", c.name); return 1; }
    std::printf("ok %s\n", c.name);
    return 0;
  }
  std::fprintf(stderr, "usage: device_owned_harness CASE | list\n");
  return 2;
}
