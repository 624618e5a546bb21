// wpt_devmem.h — who frees what: the owner of one device or pinned allocation,
// the scratch of a test hook, and the layout rule of a scratch block.
//
// Plain hipMalloc / hipFree (and the pinned pair) behind RAII: no pool, no
// reference counts, nothing stream-ordered. A free happens, and synchronises,
// exactly where reset(), alloc(), a growing grow() or the destructor runs.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <utility>
#include <vector>

namespace wpt {

struct DeviceMem {
  static hipError_t take(void** p, size_t bytes) { return hipMalloc(p, bytes); }
  static void give(void* p) { (void)hipFree(p); }
};
struct PinnedMem {
  static hipError_t take(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
  static void give(void* p) { (void)hipHostFree(p); }
};

// Move-only owner of one allocation of `cap()` elements. It converts to T*, so
// launches, copies and pointer arithmetic read as they do on a raw pointer.
template <class T, class Mem>
class Buf {
 public:
  Buf() = default;
  Buf(Buf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
  Buf& operator=(Buf&& o) noexcept {
    if (this != &o) {
      reset();
      std::swap(p_, o.p_);
      std::swap(cap_, o.cap_);
    }
    return *this;
  }
  Buf(const Buf&) = delete;
  Buf& operator=(const Buf&) = delete;
  ~Buf() { reset(); }
  void reset() {
    if (p_) Mem::give(p_);
    p_ = nullptr;
    cap_ = 0;
  }
  // exactly n elements, whatever it held; empty after a failure
  hipError_t alloc(size_t n) {
    reset();
    void* p = nullptr;
    const hipError_t e = Mem::take(&p, sizeof(T) * n);
    if (e != hipSuccess) return e;
    p_ = static_cast<T*>(p);
    cap_ = n;
    return hipSuccess;
  }
  // at least n elements: nothing happens while they fit
  hipError_t grow(size_t n) { return n <= cap_ ? hipSuccess : alloc(n); }
  T* get() const { return p_; }
  size_t cap() const { return cap_; }
  operator T*() const { return p_; }
  explicit operator bool() const { return p_ != nullptr; }

 private:
  T* p_ = nullptr;
  size_t cap_ = 0;
};
template <class T>
using DevBuf = Buf<T, DeviceMem>;
template <class T>
using PinBuf = Buf<T, PinnedMem>;

// The parts of one scratch block, each starting on a 256 B boundary: take()
// gives the part's offset, `at` ends as the block's size.
struct Slices {
  size_t at = 0;
  constexpr size_t take(size_t bytes) {
    const size_t o = at;
    at += (bytes + 255) / 256 * 256;
    return o;
  }
};

// A test hook's buffers, freed together when the hook returns. After the
// first failure `ok` is false and the later requests allocate nothing.
struct HookScratch {
  std::vector<DevBuf<char>> dev;
  std::vector<PinBuf<char>> pinned;
  bool ok = true;
  template <class T>
  T* d(size_t n) { return static_cast<T*>(add(dev, sizeof(T) * (n ? n : 1))); }
  template <class T>
  T* h(size_t n) { return static_cast<T*>(add(pinned, sizeof(T) * (n ? n : 1))); }

 private:
  template <class B>
  void* add(std::vector<B>& v, size_t bytes) {
    if (!ok) return nullptr;
    B b;
    ok = b.alloc(bytes) == hipSuccess;
    void* p = b.get();
    if (ok) v.push_back(std::move(b));
    return p;
  }
};

}  // namespace wpt
