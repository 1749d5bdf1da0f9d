// libbpvo_hip, host side: the owners of what the host holds of the device — device buffers, pinned buffers, streams, events.  Each is move-only,
// empty when default-constructed, releases in its destructor and converts to the raw pointer / handle, so that job tables, launches and copies
// read as they would with raw fields.  No owner ever synchronises: whoever releases something the device may still use waits for it first, at the
// call site.  The runtime is reached through a traits parameter only (HipTraits below, under hipcc), so the templates compile with a plain host
// compiler and no ROCm header, and a test substitutes a counting, failing fake (tests/cpp/device_owned_harness.cc).
#pragma once
#include <atomic>
#include <cassert>
#include <cstddef>
#include <utility>

namespace bpvo_hip_host {

// live resources of the process by kind: up on a successful acquisition, down on release (bpvo_hip_debug_live_resources)
enum ResourceKind { RES_DEVICE = 0, RES_PINNED, RES_STREAM, RES_EVENT, RES_KINDS };
inline std::atomic<int> g_live_resources[RES_KINDS];

// A block of n elements of device (RES_DEVICE) or pinned host (RES_PINNED) memory.
template <class T, class Tr, ResourceKind Kind>
class BasicBuf {
 public:
  using status = typename Tr::status;
  BasicBuf() = default;
  BasicBuf(BasicBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), n_(std::exchange(o.n_, 0)) {}
  BasicBuf& operator=(BasicBuf&& o) noexcept
  {
    if(this != &o) { reset(); p_ = std::exchange(o.p_, nullptr); n_ = std::exchange(o.n_, 0); }
    return *this;
  }
  ~BasicBuf() { reset(); }
  status alloc(size_t n)      // the buffer must be empty; n = 0 leaves it so and succeeds
  {
    assert(!p_);
    if(n == 0) return Tr::ok;
    void* p = nullptr;
    const status e = Tr::alloc(Kind, &p, n * sizeof(T));
    if(e != Tr::ok) return e;
    p_ = static_cast<T*>(p); n_ = n;
    g_live_resources[Kind].fetch_add(1);
    return e;
  }
  // at least n elements: the old block is released BEFORE the new one is acquired (the peak is one block, not two), nothing of it is kept, and a
  // failure leaves the buffer empty
  status reserve(size_t n) { if(n <= n_) return Tr::ok; reset(); return alloc(n); }
  void reset()
  {
    if(!p_) return;
    Tr::free(Kind, p_);
    p_ = nullptr; n_ = 0;
    g_live_resources[Kind].fetch_sub(1);
  }
  size_t size() const { return n_; }      // elements
  T* get() const { return p_; }
  operator T*() const { return p_; }

 private:
  T* p_ = nullptr;
  size_t n_ = 0;
};

// A stream (H = Tr::stream_t, RES_STREAM) or an event (H = Tr::event_t, RES_EVENT).
template <class H, class Tr, ResourceKind Kind>
class BasicHandle {
 public:
  using status = typename Tr::status;
  BasicHandle() = default;
  BasicHandle(BasicHandle&& o) noexcept : h_(std::exchange(o.h_, H())) {}
  BasicHandle& operator=(BasicHandle&& o) noexcept
  {
    if(this != &o) { reset(); h_ = std::exchange(o.h_, H()); }
    return *this;
  }
  ~BasicHandle() { reset(); }
  // the owner must be empty.  flags: an event's, as the runtime's create-with-flags call takes them (0: a plain event, with timing); streams take none
  status create(unsigned flags = 0)
  {
    assert(!h_);
    const status e = Tr::create(&h_, flags);
    if(e != Tr::ok) { h_ = H(); return e; }
    g_live_resources[Kind].fetch_add(1);
    return e;
  }
  void reset()
  {
    if(!h_) return;
    Tr::destroy(h_);
    h_ = H();
    g_live_resources[Kind].fetch_sub(1);
  }
  H get() const { return h_; }
  operator H() const { return h_; }

 private:
  H h_ = H();
};

}  // namespace bpvo_hip_host

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

namespace bpvo_hip_host {

// the only place of the library (multi_gpu.hip's node aside) that acquires or releases a device resource
struct HipTraits {
  using status = hipError_t;
  using stream_t = hipStream_t;
  using event_t = hipEvent_t;
  static constexpr status ok = hipSuccess;
  static status alloc(ResourceKind kind, void** p, size_t bytes) { return kind == RES_DEVICE ? hipMalloc(p, bytes) : hipHostMalloc(p, bytes); }
  static void free(ResourceKind kind, void* p) { (void) (kind == RES_DEVICE ? hipFree(p) : hipHostFree(p)); }
  static status create(stream_t* s, unsigned) { return hipStreamCreateWithFlags(s, hipStreamNonBlocking); }
  static status create(event_t* e, unsigned flags) { return flags ? hipEventCreateWithFlags(e, flags) : hipEventCreate(e); }
  static void destroy(stream_t s) { (void) hipStreamDestroy(s); }
  static void destroy(event_t e) { (void) hipEventDestroy(e); }
};
template <class T> using DeviceBuf = BasicBuf<T, HipTraits, RES_DEVICE>;
template <class T> using PinnedBuf = BasicBuf<T, HipTraits, RES_PINNED>;
using Stream = BasicHandle<hipStream_t, HipTraits, RES_STREAM>;
using Event = BasicHandle<hipEvent_t, HipTraits, RES_EVENT>;

}  // namespace bpvo_hip_host
#endif
