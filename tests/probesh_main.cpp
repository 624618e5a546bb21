// Host test of csrc/wpt_sh.h's plain part as a program of its own: sh_basis and
// the host entry's body (sh_basis_rows) over axis, diagonal, signed-zero,
// denormal and non-finite directions, every input and output in a heap block of
// exactly its size, so that a read or write past either is an AddressSanitizer
// report. tests/test_probesh_cpu.py builds it with -fsanitize=address,undefined
// and runs it; no Python, no GPU.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <limits>
#include <memory>
#include <vector>

#include "wpt_math.h"

namespace wpt {
#include "wpt_rays.h"
#include "wpt_points.h"
#include "wpt_sh.h"
}  // namespace wpt

namespace {
int g_failed = 0;
#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
      g_failed++;                                                  \
    }                                                              \
  } while (0)

uint32_t bits(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
}

std::vector<float> directions() {
  const float r = 0.57735026f, t = ldexpf(1.0f, -149), m = ldexpf(1.0f, -127);
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  const float z0 = sqrtf(1.0f / 3.0f);
  std::vector<float> d = {1, 0, 0, -1, 0, 0, 0, 1, 0, 0, -1, 0, 0, 0, 1, 0, 0, -1};
  for (float sx : {r, -r})
    for (float sy : {r, -r})
      for (float sz : {r, -r}) d.insert(d.end(), {sx, sy, sz});
  d.insert(d.end(), {-0.0f, 1, 0, 1, -0.0f, 0, -0.0f, -0.0f, -0.0f, t, 1, 0, m, m, 1, t, t, t});
  for (float z : {nextafterf(z0, 0.0f), z0, nextafterf(z0, 1.0f)}) d.insert(d.end(), {0.6f, 0.8f, z});
  d.insert(d.end(), {0.5f, -0.5f, 0.70710678f, 3e38f, 3e38f, 3e38f, nan, 0, 1, 0, inf, 0, -inf, inf, nan});
  return d;
}
}  // namespace

int main() {
  const std::vector<float> dirs = directions();
  const size_t n = dirs.size() / 3;
  std::unique_ptr<float[]> in(new float[3 * n]);  // exactly the directions
  memcpy(in.get(), dirs.data(), sizeof(float) * 3 * n);
  std::unique_ptr<float[]> full(new float[9 * n]);
  wpt::sh_basis_rows(n, in.get(), 2, full.get());
  size_t finite = 0, signs = 0;
  for (uint32_t order = 0; order <= wpt::kShMaxOrder; order++) {
    const uint32_t nc = wpt::sh_coeffs(order);
    CHECK(nc == (order + 1) * (order + 1));
    std::unique_ptr<float[]> out(new float[nc * n]);  // exactly the rows
    wpt::sh_basis_rows(n, in.get(), order, out.get());
    for (size_t i = 0; i < n; i++) {
      const wpt::V3 d = wpt::mk(in[3 * i], in[3 * i + 1], in[3 * i + 2]);
      std::unique_ptr<float[]> one(new float[nc]);
      wpt::sh_basis(d, order, one.get());
      for (uint32_t k = 0; k < nc; k++) {
        // the rows, the single call, the per-coefficient form and the prefix of order 2: the same bits
        CHECK(bits(out[nc * i + k]) == bits(one[k]) || (isnan(out[nc * i + k]) && isnan(one[k])));
        CHECK(bits(one[k]) == bits(wpt::sh_basis_at(d, k)) || isnan(one[k]));
        CHECK(bits(one[k]) == bits(full[9 * i + k]) || isnan(one[k]));
      }
      if (order < 2 || !(isfinite(d.x) && isfinite(d.y) && isfinite(d.z)) || fabsf(d.x) > 2.0f) continue;
      finite++;
      const float* Y = out.get() + 9 * i;
      CHECK(Y[0] == wpt::kShC0);
      CHECK(Y[1] == wpt::kShC1 * d.y && Y[2] == wpt::kShC1 * d.z && Y[3] == wpt::kShC1 * d.x);
      CHECK(fabsf(d.x) != fabsf(d.y) || Y[8] == 0.0f);
      // a signed zero keeps its sign through the products of band 1
      if (bits(d.y) == 0x80000000u) { CHECK(bits(Y[1]) == 0x80000000u); signs++; }
      for (uint32_t k = 0; k < 9; k++) CHECK(isfinite(Y[k]) && fabsf(Y[k]) < 1.1f);
    }
  }
  // Y6 changes sign between the neighbours of sqrt(1 / 3)
  {
    const float z0 = sqrtf(1.0f / 3.0f);
    const float lo = wpt::sh_basis_at(wpt::mk(0.6f, 0.8f, nextafterf(nextafterf(z0, 0.0f), 0.0f)), 6);
    const float hi = wpt::sh_basis_at(wpt::mk(0.6f, 0.8f, nextafterf(nextafterf(z0, 1.0f), 1.0f)), 6);
    CHECK(lo < 0.0f && hi > 0.0f);
  }
  // an empty call touches nothing
  wpt::sh_basis_rows(0, nullptr, 2, nullptr);
  CHECK(finite > 0 && signs > 0);
  printf("%zu directions, %zu finite ones checked at order 2, %zu signed zeros\n", n, finite, signs);
  printf("probesh_main: %d failed checks\n", g_failed);
  return g_failed ? 1 : 0;
}
