// hip_owned.h -- move-only owners of what the host side allocates from the HIP runtime: device and pinned buffers, events, streams, and
// the ring of pinned staging entries the device reads later.  Default-constructed empty; freed by the destructor and by reset().  A
// group of them is built into locals and moved into place when every member succeeded, so a failure half-way leaves nothing behind.
// Kernels and argument structs take the raw pointer / handle (get(), or the implicit conversion).
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>
#include <utility>
#include <vector>

namespace bhip {

bool hip_ok(hipError_t e, const char* what);  // logs once per site when BEATRICE_HIP_DEBUG is set (common.hip)

template <class T>
class DevBuf {  // hipMalloc / hipFree
 public:
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept { swap(o); }
  DevBuf& operator=(DevBuf&& o) noexcept { if (this != &o) { reset(); swap(o); } return *this; }
  ~DevBuf() { reset(); }
  bool alloc(size_t n, const char* what, bool zero = true) {
    reset();
    if (!hip_ok(hipMalloc(reinterpret_cast<void**>(&p_), sizeof(T) * n), what)) { p_ = nullptr; return false; }
    n_ = n;
    if (zero && !hip_ok(hipMemset(p_, 0, sizeof(T) * n), what)) { reset(); return false; }
    return true;
  }
  void reset() { if (p_) (void)hipFree(p_); p_ = nullptr; n_ = 0; }
  T* get() const { return p_; }
  operator T*() const { return p_; }
  size_t size() const { return n_; }
 private:
  void swap(DevBuf& o) { std::swap(p_, o.p_); std::swap(n_, o.n_); }
  T* p_ = nullptr;
  size_t n_ = 0;
};

template <class T>
class PinnedBuf {  // hipHostMalloc / hipHostFree
 public:
  PinnedBuf() = default;
  PinnedBuf(PinnedBuf&& o) noexcept { swap(o); }
  PinnedBuf& operator=(PinnedBuf&& o) noexcept { if (this != &o) { reset(); swap(o); } return *this; }
  ~PinnedBuf() { reset(); }
  bool alloc(size_t n, const char* what, bool zero = true) {
    reset();
    if (!hip_ok(hipHostMalloc(reinterpret_cast<void**>(&p_), sizeof(T) * n, hipHostMallocDefault), what)) { p_ = nullptr; return false; }
    n_ = n;
    if (zero) std::memset(static_cast<void*>(p_), 0, sizeof(T) * n);
    return true;
  }
  void reset() { if (p_) (void)hipHostFree(p_); p_ = nullptr; n_ = 0; }
  T* get() const { return p_; }
  operator T*() const { return p_; }
  size_t size() const { return n_; }
 private:
  void swap(PinnedBuf& o) { std::swap(p_, o.p_); std::swap(n_, o.n_); }
  T* p_ = nullptr;
  size_t n_ = 0;
};

class Event {
 public:
  Event() = default;
  Event(Event&& o) noexcept { std::swap(e_, o.e_); }
  Event& operator=(Event&& o) noexcept { if (this != &o) { reset(); std::swap(e_, o.e_); } return *this; }
  ~Event() { reset(); }
  bool create(const char* what, bool timing = false) {
    reset();
    if (hip_ok(timing ? hipEventCreate(&e_) : hipEventCreateWithFlags(&e_, hipEventDisableTiming), what)) return true;
    e_ = nullptr;
    return false;
  }
  void reset() { if (e_) (void)hipEventDestroy(e_); e_ = nullptr; }
  hipEvent_t get() const { return e_; }
  operator hipEvent_t() const { return e_; }
 private:
  hipEvent_t e_ = nullptr;
};

class Stream {  // an owned stream: non-blocking, or one made elsewhere and handed over with adopt()
 public:
  Stream() = default;
  Stream(Stream&& o) noexcept { std::swap(s_, o.s_); }
  Stream& operator=(Stream&& o) noexcept { if (this != &o) { reset(); std::swap(s_, o.s_); } return *this; }
  ~Stream() { reset(); }
  bool create(const char* what) {
    reset();
    if (hip_ok(hipStreamCreateWithFlags(&s_, hipStreamNonBlocking), what)) return true;
    s_ = nullptr;
    return false;
  }
  void adopt(hipStream_t s) { reset(); s_ = s; }
  void reset() { if (s_) (void)hipStreamDestroy(s_); s_ = nullptr; }
  hipStream_t get() const { return s_; }
  operator hipStream_t() const { return s_; }
 private:
  hipStream_t s_ = nullptr;
};

// n entries of len elements of pinned memory that the host writes and the device reads later (in place, or through the copy into the
// device ring of the same shape), one event per entry: entry i may be rewritten only after the event recorded behind its last reader
// has passed.  claim(i) before writing entry i, mark(i, stream) behind its last reader.
template <class T>
class StagedRing {
 public:
  bool alloc(int n, size_t len, const char* what, bool device_copy = false) {
    StagedRing r;
    r.len_ = len;
    if (!r.h_.alloc(n * len, what) || (device_copy && !r.d_.alloc(n * len, what, false))) return false;
    r.ev_.resize(n);
    r.marked_.assign(n, 0);
    for (Event& e : r.ev_) if (!e.create(what)) return false;
    *this = std::move(r);
    return true;
  }
  void reset() { *this = StagedRing(); }
  int entries() const { return (int)ev_.size(); }
  T* host(int i) const { return h_.get() + (size_t)i * len_; }
  T* dev(int i) const { return d_.get() + (size_t)i * len_; }
  T* claim(int i) {  // the host entry, free to be written: waits if its last reader is still marked (nullptr: the wait failed)
    if (marked_[i] && !hip_ok(hipEventSynchronize(ev_[i]), "staged ring entry")) return nullptr;
    marked_[i] = 0;
    return host(i);
  }
  bool mark(int i, hipStream_t s) {  // what is on `s` so far reads entry i
    if (!hip_ok(hipEventRecord(ev_[i], s), "staged ring event")) return false;
    marked_[i] = 1;
    return true;
  }
  void forget() { marked_.assign(marked_.size(), 0); }  // after a drain: no reader is left
 private:
  PinnedBuf<T> h_;
  DevBuf<T> d_;
  std::vector<Event> ev_;
  std::vector<char> marked_;
  size_t len_ = 0;
};

}  // namespace bhip
