// ksim_mem.h — the owners of everything the host runtime allocates: device
// memory, pinned host memory, the stream and the events.  Each is move-only
// and frees in its destructor, on the device that is current then
// (ksim_destroy and every other delete of a handle set the handle's first).
// Private to csrc/ (ksim_host.h includes it); alloc and the two reserves are
// defined in ksim_engine.cpp.
#pragma once

#include <hip/hip_runtime.h>

#include <utility>
#include <vector>

struct ksim_handle;

#define KSIM_HIDDEN __attribute__((visibility("hidden")))

struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
};

// Device allocations that live and go together, in allocation order, each with
// its byte size.  `x = DevPool{}` and clear() free them all.
class KSIM_HIDDEN DevPool {
 public:
  DevPool() = default;
  DevPool(const DevPool&) = delete;
  DevPool& operator=(const DevPool&) = delete;
  DevPool(DevPool&& o) noexcept : v_(std::move(o.v_)) { o.v_.clear(); }
  DevPool& operator=(DevPool&& o) noexcept {
    if (this != &o) {
      clear();
      v_.swap(o.v_);
    }
    return *this;
  }
  ~DevPool() { clear(); }
  void clear() {
    for (auto& b : v_) (void)hipFree(b.p);
    v_.clear();
  }
  bool empty() const { return v_.empty(); }
  size_t size() const { return v_.size(); }
  const DevBuf& operator[](size_t i) const { return v_[i]; }
  // A new array of `bytes` (0: 16) into a typed field, filled from src on the
  // handle's stream (null: zero-filled): the one way the host runtime
  // allocates a device array.  T may be const-qualified, as the fields the
  // kernels only read are.  The pool owns the array from before the copy is
  // enqueued, so a failed copy leaks nothing.
  template <class T>
  int alloc(ksim_handle* h, T*& dst, size_t bytes, const void* src = nullptr) {
    void* p = nullptr;
    if (const int rc = upload(h, src, bytes, &p)) return rc;
    dst = (T*)p;
    return 0;
  }

 private:
  int upload(ksim_handle* h, const void* src, size_t bytes, void** out);
  std::vector<DevBuf> v_;
};

// The two grow-only buffers below share one reserve rule.
//
// reserve(h, bytes, idle) leaves the buffer at least `bytes` large.  It never
// shrinks and never keeps contents: when it has to grow it frees the old
// allocation first and makes a new one, of max(2 * bytes, floor) bytes, or of
// exactly `bytes` (16 at least) when the buffer's floor is 0.  The old
// contents, and the old address, are gone from that moment, so nothing
// enqueued on the handle's stream may still read or write them:
//   Idle::kSync    reserve synchronizes the stream itself, and only when it
//                  reallocates (the caller may have work in flight);
//   Idle::kCaller  the caller vouches that the stream is idle, or that every
//                  reader of this buffer has run (the upload ring's events),
//                  whenever bytes > cap; each such call site says why.
// A buffer that fits is returned untouched, with no synchronization at all.
enum class Idle { kCaller, kSync };

// A device buffer reused across calls: the per-call uploads of the
// framework-driven calls (one pod, its terms and uses) without a hipMalloc /
// hipFree pair per call, the sweep's vectors and rows.
class KSIM_HIDDEN DevGrow {
 public:
  void* p = nullptr;                    // read-only outside reserve
  size_t cap = 0;
  explicit DevGrow(size_t floor = 1 << 16, const char* what = "hipMalloc (arena)") : floor_(floor), what_(what) {}
  DevGrow(const DevGrow&) = delete;
  DevGrow& operator=(const DevGrow&) = delete;
  DevGrow(DevGrow&& o) noexcept : floor_(o.floor_), what_(o.what_) { swap(o); }
  DevGrow& operator=(DevGrow&& o) noexcept { return swap(o), *this; }   // o frees what this held
  ~DevGrow() {
    if (p) (void)hipFree(p);
  }
  int reserve(ksim_handle* h, size_t bytes, Idle idle);

 private:
  void swap(DevGrow& o) {
    std::swap(p, o.p), std::swap(cap, o.cap), std::swap(floor_, o.floor_), std::swap(what_, o.what_);
  }
  size_t floor_;
  const char* what_;                    // the failing call, as the error text names it
};

// Pinned host memory reused across calls.  The flags it is allocated with are
// part of it; with hipHostMallocMapped, d is the device's address of p (copy
// kernels read / write it directly).
class KSIM_HIDDEN PinGrow {
 public:
  void* p = nullptr;                    // read-only outside reserve
  void* d = nullptr;
  size_t cap = 0;
  PinGrow(unsigned flags, size_t floor, const char* what) : flags_(flags), floor_(floor), what_(what) {}
  PinGrow(const PinGrow&) = delete;
  PinGrow& operator=(const PinGrow&) = delete;
  PinGrow(PinGrow&& o) noexcept : flags_(o.flags_), floor_(o.floor_), what_(o.what_) { swap(o); }
  PinGrow& operator=(PinGrow&& o) noexcept { return swap(o), *this; }   // o frees what this held
  ~PinGrow() {
    if (p) (void)hipHostFree(p);
  }
  int reserve(ksim_handle* h, size_t bytes, Idle idle);

 private:
  void swap(PinGrow& o) {
    std::swap(p, o.p), std::swap(d, o.d), std::swap(cap, o.cap);
    std::swap(flags_, o.flags_), std::swap(floor_, o.floor_), std::swap(what_, o.what_);
  }
  unsigned flags_;
  size_t floor_;
  const char* what_;
};
constexpr unsigned kPinMapped = hipHostMallocCoherent | hipHostMallocMapped;

// The stream and an event: created by their user through out(), destroyed here.
template <class T, hipError_t (*Destroy)(T)>
class KSIM_HIDDEN HipOwned {
 public:
  HipOwned() = default;
  HipOwned(const HipOwned&) = delete;
  HipOwned& operator=(const HipOwned&) = delete;
  HipOwned(HipOwned&& o) noexcept { std::swap(v_, o.v_); }
  HipOwned& operator=(HipOwned&& o) noexcept { return std::swap(v_, o.v_), *this; }
  ~HipOwned() {
    if (v_) (void)Destroy(v_);
  }
  operator T() const { return v_; }
  T* out() { return &v_; }

 private:
  T v_ = nullptr;
};
using HipStream = HipOwned<hipStream_t, hipStreamDestroy>;
using HipEvent = HipOwned<hipEvent_t, hipEventDestroy>;
