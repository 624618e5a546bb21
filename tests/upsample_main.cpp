// Host test of csrc/wpt_upsample.h (and the filter's host half it builds on)
// as a program of its own: upsample_host on frames of 1 x 1, 1 x 5 and 9 x 7
// coarse pixels at every scale, with every input and output in a heap block of
// exactly its size, so that a tap or a store one element out of bounds is an
// AddressSanitizer report. tests/test_upsample_cpu.py builds it with
// -fsanitize=address,undefined and runs it; no Python, no GPU.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <limits>
#include <vector>

#include "wpt_math.h"

namespace wpt {
#include "wpt_denoise.h"
#include "wpt_upsample.h"
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

uint32_t g_rng = 0x2545F491u;
float rnd() {  // xorshift32 -> [0, 1)
  g_rng ^= g_rng << 13;
  g_rng ^= g_rng >> 17;
  g_rng ^= g_rng << 5;
  return (float)(g_rng >> 8) * (1.0f / 16777216.0f);
}

struct Frame {
  std::vector<float> acc, t, n, alb;
  std::vector<uint32_t> cnt;
  std::vector<uint8_t> kind;
};

// every kind, pixels without samples, NaN and infinite sums, denormal depths,
// albedo components of 0, normals along the three axes
Frame make(uint32_t w, uint32_t h) {
  const size_t np = (size_t)w * h;
  Frame f;
  f.acc.resize(3 * np); f.t.resize(np); f.n.resize(3 * np); f.alb.resize(3 * np); f.cnt.resize(np); f.kind.resize(np);
  for (size_t i = 0; i < np; i++) {
    const float p = rnd();
    f.kind[i] = p < 0.7f ? 1 : p < 0.85f ? 2 : 0;
    if (np == 1) f.kind[i] = 1;
    const int axis = (int)(rnd() * 3.0f) % 3;
    for (int k = 0; k < 3; k++) {
      f.n[3 * i + k] = f.kind[i] && k == axis ? (rnd() < 0.1f ? -1.0f : 1.0f) : 0.0f;
      f.alb[3 * i + k] = f.kind[i] ? (rnd() < 0.1f ? 0.0f : 0.05f + 0.9f * rnd()) : 0.0f;
      f.acc[3 * i + k] = 4.0f * rnd();
    }
    f.t[i] = f.kind[i] ? (rnd() < 0.1f ? 1e-41f : 2.0f + rnd()) : std::numeric_limits<float>::infinity();
    f.cnt[i] = rnd() < 0.1f ? 0u : 1u + (uint32_t)(rnd() * 15.0f);
    const float q = rnd();
    if (q < 0.05f) f.acc[3 * i] = std::numeric_limits<float>::quiet_NaN();
    else if (q < 0.1f) f.acc[3 * i + 2] = std::numeric_limits<float>::infinity();
  }
  return f;
}

void run(uint32_t w, uint32_t h, uint32_t s, uint32_t iterations, float sigma_z) {
  const Frame c = make(w, h), f = make(s * w, s * h);
  const size_t nf = (size_t)s * w * s * h;
  const float bg[3] = {0.25f, -0.0f, 3.0e-41f};
  std::vector<float> rgb(3 * nf, -7.0f);
  std::vector<uint8_t> valid(nf, 0xA5), rgba(4 * nf, 0xA5);
  wpt::upsample_host(w, h, s, c.acc.data(), c.cnt.data(), c.t.data(), c.n.data(), c.alb.data(), c.kind.data(),
                     f.t.data(), f.n.data(), f.alb.data(), f.kind.data(), bg, iterations, 1.0f, sigma_z, rgb.data(),
                     valid.data(), rgba.data());
  size_t seen[3] = {0, 0, 0};
  for (size_t i = 0; i < nf; i++) {
    CHECK(valid[i] <= 2);
    if (valid[i] > 2) continue;
    seen[valid[i]]++;
    CHECK(rgba[4 * i + 3] == 255);
    if (f.kind[i] == 0) CHECK(valid[i] == 1 && memcmp(&rgb[3 * i], bg, sizeof bg) == 0);
    if (f.kind[i] == 2) CHECK(valid[i] == 1 && memcmp(&rgb[3 * i], &f.alb[3 * i], 3 * sizeof(float)) == 0);
    if (f.kind[i] == 1 && valid[i] == 0) CHECK(rgb[3 * i] == 0.0f && rgb[3 * i + 1] == 0.0f && rgb[3 * i + 2] == 0.0f);
    if (f.kind[i] == 1 && valid[i] != 0)
      CHECK(wpt::dn_finite(rgb[3 * i]) && wpt::dn_finite(rgb[3 * i + 1]) && wpt::dn_finite(rgb[3 * i + 2]));
  }
  // a second call that asks for one output leaves the others alone
  std::vector<uint8_t> valid2(nf, 0xA5);
  wpt::upsample_host(w, h, s, c.acc.data(), c.cnt.data(), c.t.data(), c.n.data(), c.alb.data(), c.kind.data(),
                     f.t.data(), f.n.data(), f.alb.data(), f.kind.data(), bg, iterations, 1.0f, sigma_z, nullptr,
                     valid2.data(), nullptr);
  CHECK(valid2 == valid);
  printf("%ux%u x%u, %u passes, sigma_z %g: valid 0/1/2 = %zu/%zu/%zu\n", w, h, s, iterations, (double)sigma_z, seen[0],
         seen[1], seen[2]);
}
}  // namespace

int main() {
  const uint32_t shapes[3][2] = {{1, 1}, {1, 5}, {9, 7}};
  for (const auto& wh : shapes)
    for (uint32_t s = 2; s <= 4; s++)
      for (uint32_t it : {0u, 1u, 5u}) {
        run(wh[0], wh[1], s, it, 0.1f);
        run(wh[0], wh[1], s, it, 1e-5f);  // sigma_z * T underflows on the denormal depths
      }
  // the tap positions at the ends of the 32-bit range of fine coordinates
  for (uint32_t s = 2; s <= 4; s++) {
    long long i0;
    float f;
    wpt::up_axis(0u, s, i0, f);
    CHECK(i0 == -1 && f == (float)(s + 1) / (float)(2 * s));
    wpt::up_axis(0xFFFFFFFFu, s, i0, f);
    const long long a = 2ll * 0xFFFFFFFFll + 1 - s;
    CHECK(i0 == a / (2ll * s) && f == (float)(a % (2ll * s)) / (float)(2 * s));
  }
  printf("upsample_main: %d failed checks\n", g_failed);
  return g_failed ? 1 : 0;
}
