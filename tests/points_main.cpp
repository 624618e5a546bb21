// Host test of csrc/wpt_points.h's plain part as a program of its own: point_ray
// over the decision table of tests/points_fixtures.py (normals on each side of
// orthogonal's thresholds, the axis normals, invalid records, normals far from
// unit length), each record in a heap block of exactly its 24 bytes, so that a
// read past a record is an AddressSanitizer report. tests/test_points_cpu.py
// builds it with -fsanitize=address,undefined and runs it; no Python, no GPU.
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

struct Rec {
  float v[6];
  bool unit;
};

bool finite3(wpt::V3 a) { return isfinite(a.x) && isfinite(a.y) && isfinite(a.z); }

std::vector<Rec> table() {
  const float t = 0.1f, up = nextafterf(t, 1.0f), down = nextafterf(t, 0.0f);
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  const float tiny = ldexpf(1.0f, -70), huge = 1e30f;
  std::vector<Rec> out;
  const auto unit = [&](float x, float z, float ys) {
    const float y = ys * (float)sqrt(1.0 - (double)x * x - (double)z * z);
    out.push_back({{0.25f, 1.5f, -2.0f, x, y, z}, true});
  };
  for (float z : {up, -up, t, down, -down})
    for (float x : {0.3f, up, -up, t, down}) unit(x, z, z > 0 ? 1.0f : -1.0f);
  for (int a = 0; a < 3; a++)
    for (float s : {1.0f, -1.0f}) {
      Rec r = {{0.25f, 1.5f, -2.0f, 0, 0, 0}, true};
      r.v[3 + a] = s;
      out.push_back(r);
    }
  for (int k = 0; k < 6; k++)
    for (float bad : {nan, inf, -inf}) {
      Rec r = {{0, 1, 0, 0, 1, 0}, false};
      r.v[k] = bad;
      out.push_back(r);
    }
  out.push_back({{1, 2, 3, 0.0f, 0.0f, 0.0f}, false});
  out.push_back({{1, 2, 3, -0.0f, -0.0f, -0.0f}, false});
  out.push_back({{1, 2, 3, 0.0f, -0.0f, 0.0f}, false});
  for (float l : {tiny, huge, 2.0e19f})
    for (int a = 0; a < 3; a++) {
      Rec r = {{1, 2, 3, 0, 0, 0}, false};
      r.v[3 + a] = l;
      out.push_back(r);
    }
  return out;
}
}  // namespace

int main() {
  const uint32_t seed = 0xBABABEBEu;
  const std::vector<Rec> recs = table();
  size_t traced = 0, rejected = 0, not_finite = 0;
  for (const Rec& r : recs) {
    std::unique_ptr<float[]> rec(new float[6]);  // exactly the record
    memcpy(rec.get(), r.v, sizeof r.v);
    const bool valid = wpt::ray_valid(rec.get());
    for (uint32_t dist : {wpt::kPointsCosine, wpt::kPointsSphere})
      for (uint32_t sample : {0u, 7u, 0xFFFFFFFFu})
        for (uint32_t k = 0; k < 200; k++) {
          const uint32_t key = k < 100 ? k : k * 0x9E3779B1u;
          wpt::V3 o = wpt::mk(-7.0f, -7.0f, -7.0f), wi = o;
          uint32_t st = 0xA5A5A5A5u;
          const bool ok = wpt::point_ray(rec.get(), key, seed, sample, dist, o, wi, st);
          CHECK(ok == valid);
          if (!ok) {
            // nothing is written for a rejected record
            CHECK(o.x == -7.0f && wi.z == -7.0f && st == 0xA5A5A5A5u);
            rejected++;
            continue;
          }
          uint32_t want = wpt::path_seed(seed, key, sample);
          wpt::xs_next_u32(want);
          wpt::xs_next_u32(want);
          CHECK(st == want);
          if (!r.unit) {
            not_finite += !wpt::point_ray_valid(o, wi);
            continue;
          }
          traced++;
          CHECK(finite3(o) && finite3(wi) && wpt::point_ray_valid(o, wi));
          const double l2 = (double)wi.x * wi.x + (double)wi.y * wi.y + (double)wi.z * wi.z;
          CHECK(fabs(l2 - 1.0) <= 4.0 * ldexp(1.0, -23));
          const double cosn = (double)wi.x * rec[3] + (double)wi.y * rec[4] + (double)wi.z * rec[5];
          if (dist == wpt::kPointsCosine) CHECK(cosn >= 0.0);
        }
  }
  CHECK(traced > 0 && rejected > 0 && not_finite > 0);
  printf("%zu records: %zu unit-normal rays, %zu rejected calls, %zu generated rays the status rule rejects\n",
         recs.size(), traced, rejected, not_finite);
  printf("points_main: %d failed checks\n", g_failed);
  return g_failed ? 1 : 0;
}
