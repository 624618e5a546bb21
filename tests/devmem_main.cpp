// Host test of csrc/wpt_devmem.h without the HIP runtime: the four allocation
// calls are defined here over malloc, count their calls and live blocks, catch
// a free of a block that is not live, and can fail the k-th allocation.
// tests/test_devmem_cpu.py builds it with -fsanitize=address,undefined.
#include <stdio.h>
#include <stdlib.h>

#include <set>
#include <utility>

#include "wpt_devmem.h"

namespace {
std::set<void*> g_live[2];  // device, pinned
int g_allocs = 0, g_frees = 0, g_bad_frees = 0;
int g_fail_at = 0;  // fail the allocation call with this number (1-based, counted from arm()), 0: none
int g_since_arm = 0;

void arm(int k) { g_fail_at = k; g_since_arm = 0; }

hipError_t take(int kind, void** p, size_t bytes) {
  g_allocs++;
  if (g_fail_at && ++g_since_arm == g_fail_at) {
    *p = nullptr;
    return hipErrorOutOfMemory;
  }
  *p = malloc(bytes ? bytes : 1);
  g_live[kind].insert(*p);
  return hipSuccess;
}

hipError_t give(int kind, void* p) {
  g_frees++;
  if (!p) return hipSuccess;
  if (!g_live[kind].erase(p)) {
    g_bad_frees++;  // a double free, or a block of the other kind
    return hipErrorInvalidValue;
  }
  free(p);
  return hipSuccess;
}

size_t live() { return g_live[0].size() + g_live[1].size(); }

int g_failed = 0;
#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
      g_failed++;                                             \
    }                                                         \
  } while (0)
}  // namespace

extern "C" {
hipError_t hipMalloc(void** p, size_t bytes) { return take(0, p, bytes); }
hipError_t hipFree(void* p) { return give(0, p); }
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned int) { return take(1, p, bytes); }
hipError_t hipHostFree(void* p) { return give(1, p); }
}

using wpt::DevBuf;
using wpt::PinBuf;

template <class B>
static void owner_cases() {
  const size_t live0 = live();
  {
    B a;
    CHECK(!a && a.get() == nullptr && a.cap() == 0);
    int calls = g_allocs + g_frees;
    a.reset();  // an empty owner frees nothing
    CHECK(g_allocs + g_frees == calls);
    CHECK(a.alloc(10) == hipSuccess);
    CHECK(a && a.cap() == 10 && live() == live0 + 1);
    auto* p10 = a.get();
    CHECK(static_cast<decltype(p10)>(a) == p10 && a + 3 == p10 + 3);
    // grow within the capacity: no call at all, the block stays
    calls = g_allocs + g_frees;
    CHECK(a.grow(10) == hipSuccess && a.grow(1) == hipSuccess && a.grow(0) == hipSuccess);
    CHECK(g_allocs + g_frees == calls && a.get() == p10 && a.cap() == 10);
    // grow past it: one free, one allocation
    CHECK(a.grow(11) == hipSuccess);
    CHECK(g_allocs + g_frees == calls + 2 && a.cap() == 11 && live() == live0 + 1);
    // alloc reallocates whatever it holds, also a smaller size
    calls = g_allocs + g_frees;
    CHECK(a.alloc(4) == hipSuccess);
    CHECK(g_allocs + g_frees == calls + 2 && a.cap() == 4 && live() == live0 + 1);
    a[3] = {};  // the last element is inside the block (the sanitizer looks)

    // move construction: the source ends empty, one block in all
    B b(std::move(a));
    CHECK(!a && a.cap() == 0 && b && b.cap() == 4 && live() == live0 + 1);
    // move assignment onto a full owner frees its block
    B c;
    CHECK(c.alloc(7) == hipSuccess && live() == live0 + 2);
    c = std::move(b);
    CHECK(!b && b.cap() == 0 && c.cap() == 4 && live() == live0 + 1);
    // ... and onto itself changes nothing
    B& cr = c;
    c = std::move(cr);
    CHECK(c && c.cap() == 4 && live() == live0 + 1);
    // a moved-from owner can be used again
    CHECK(a.alloc(2) == hipSuccess && live() == live0 + 2);

    // a failed allocation leaves the owner empty; a later alloc works
    arm(1);
    CHECK(c.alloc(100) == hipErrorOutOfMemory);
    arm(0);
    CHECK(!c && c.get() == nullptr && c.cap() == 0 && live() == live0 + 1);
    arm(1);
    CHECK(a.grow(100) == hipErrorOutOfMemory);  // the same through grow
    arm(0);
    CHECK(!a && a.cap() == 0 && live() == live0);
    CHECK(c.alloc(5) == hipSuccess && c.cap() == 5 && live() == live0 + 1);
    c.reset();
    CHECK(!c && c.cap() == 0 && live() == live0);
    c.reset();
    CHECK(c.grow(3) == hipSuccess && live() == live0 + 1);
  }  // the destructors free what is left
  CHECK(live() == live0);
}

static void scratch_cases() {
  {
    wpt::HookScratch S;
    float* a = S.d<float>(8);
    unsigned* b = S.h<unsigned>(0);  // (0 elements are one)
    char* c = S.d<char>(1000);
    CHECK(S.ok && a && b && c && g_live[0].size() == 2 && g_live[1].size() == 1);
    a[7] = 1.0f;
    b[0] = 1u;
    c[999] = 1;
  }
  CHECK(live() == 0);
  {
    // the third of five fails: the first two are freed at the end of the
    // scope, the last two allocate nothing
    wpt::HookScratch S;
    const int calls = g_allocs;
    arm(3);
    void* p[5] = {S.d<float>(4), S.h<float>(4), S.d<double>(4), S.d<char>(4), S.h<char>(4)};
    arm(0);
    CHECK(!S.ok && p[0] && p[1] && !p[2] && !p[3] && !p[4]);
    CHECK(g_allocs == calls + 3 && live() == 2);
  }
  CHECK(live() == 0);
}

static void slices_cases() {
  const size_t bytes[] = {0, 1, 255, 256, 257, 12 * 777};
  wpt::Slices z;
  size_t at = 0;
  for (size_t b : bytes) {
    CHECK(z.take(b) == at);
    at += (b + 255) / 256 * 256;
    CHECK(z.at == at && z.at % 256 == 0);
  }
  CHECK(z.at == 0 + 256 + 256 + 256 + 512 + 9472);
  constexpr size_t total = [] {
    wpt::Slices c;
    c.take(1);
    c.take(257);
    return c.at;
  }();
  static_assert(total == 768, "Slices is usable in constant expressions");
}

int main() {
  owner_cases<DevBuf<float>>();
  owner_cases<PinBuf<unsigned>>();
  owner_cases<DevBuf<char>>();
  scratch_cases();
  slices_cases();
  CHECK(live() == 0);
  CHECK(g_bad_frees == 0);
  printf("devmem: %d allocations, %d frees, %d bad frees, %zu live, %d failed checks\n", g_allocs, g_frees, g_bad_frees,
         live(), g_failed);
  return g_failed || g_bad_frees || live() ? 1 : 0;
}
