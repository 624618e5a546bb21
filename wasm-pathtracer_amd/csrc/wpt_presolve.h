// wpt_presolve.h — the exact "presolve" of an extension ray, compiled for both
// the host (tests, guard build) and gfx950 (k_generate, k_shade).
//
// Most extension rays end on a plane or in the background and never test a
// finite shape. presolve_ray decides that for a ray without touching the BVH:
// it computes the plane seed exactly as planes_closest does, tests the
// reference BVH2's root box against that seed exactly as enter_root does
// (box_entry's operations), and, if the root is entered, tests up to
// kMaxGuards guard boxes. A ray is resolved when the root test fails, or when
// every guard is missed or lies strictly behind the seed (best < entry); its
// result is then the seed itself: (t, id) of the closest plane, or (+inf, -1).
//
// Why the result is what the exact machine (begin_extend + step) returns.
// Each guard is the exact min/max union of the stored bounds of a group of
// BVH2 leaf nodes, and the groups partition all leaves (wpt_scene.cpp
// build_guards). The slab test is monotone in the bounds: with 1/d finite and
// non-zero on every axis, (bound - o) * inv is monotone in the bound, and
// fminf / fmaxf are monotone, so a box inside a guard has tmin' >= tmin and
// tmax' <= tmax, hence an entry hh' = max(tmin', 0) >= hh. (wpt_trav4.h's
// quirk proof relies on the same monotonicity.)
//   * Guard missed (!(hh <= tmax)): hh' >= hh > tmax >= tmax', so every leaf
//     box in it is missed as well.
//   * Guard strictly behind the seed (best < hh): best < hh' for every leaf box
//     in it. The machine's closest hit never exceeds the seed, so the strict
//     push cull (hh' < best) rejects the leaf's box wherever it is tested, and a
//     deferred entry, which was pushed only after passing that cull, cannot
//     exist for it; the pop rule !(best < h) has nothing to resume.
// A primitive is tested only inside a leaf whose box was entered, so the
// machine tests no primitive at all and returns its seed. The root test is the
// machine's own first step with the same operands.
// A ray whose direction has a zero component, or whose 1/d is not finite, is
// never resolved (0 * inf = NaN breaks the monotonicity): it goes to the
// machine. Scenes without a BVH or without finite shapes resolve nothing
// (num_guards = 0).
#pragma once
#include "wpt_math.h"

namespace wpt {

constexpr int kMaxGuards = 4;

struct PresolveBoxes {
  uint32_t num_guards;          // 0: nothing is resolved
  float root[6];                // the BVH2 root's stored bounds: x_min, y_min, z_min, x_max, y_max, z_max
  float guard[kMaxGuards][6];   // the same layout
};

// AABB::hit's entry and exit (box_entry of wpt_render.hip, the same f32
// operations in the same order): hh = max(tmin, 0).
WPT_HD void presolve_slab(const float* b, V3 o, V3 inv, float& hh, float& tmax) {
  const float tx1 = (b[0] - o.x) * inv.x;
  const float tx2 = (b[3] - o.x) * inv.x;
  const float ty1 = (b[1] - o.y) * inv.y;
  const float ty2 = (b[4] - o.y) * inv.y;
  const float tz1 = (b[2] - o.z) * inv.z;
  const float tz2 = (b[5] - o.z) * inv.z;
  const float tmin = fmaxf(fmaxf(fminf(tx1, tx2), fminf(ty1, ty2)), fminf(tz1, tz2));
  tmax = fminf(fminf(fmaxf(tx1, tx2), fmaxf(ty1, ty2)), fmaxf(tz1, tz2));
  hh = fmaxf(tmin, 0.0f);
}

// +inf. On the device it is made by an instruction the compiler cannot move:
// as a plain constant it is hoisted out of k_shade's path loop and held in a
// VGPR across shade_path, the kernel's register peak.
WPT_HD float presolve_inf() {
#if defined(__HIP_DEVICE_COMPILE__)
  float v;
  asm volatile("v_mov_b32 %0, 0x7f800000" : "=v"(v));
  return v;
#else
  return u2f(0x7f800000u);
#endif
}

// SC: the scene's infinite shapes as planes[i].x/.y/.z/.w = (normal,
// normal . location) and num_inf (DevScene on the device, HostPlanes below on
// the host). Returns true when the ray is resolved; (t, id) is then the exact
// machine's result. Unresolved: (t, id) are not meaningful.
template <class SC>
WPT_HD bool presolve_ray(const SC& S, const PresolveBoxes& B, V3 o, V3 d, float& t, int32_t& id) {
  t = 0.0f;
  id = -1;
  if (B.num_guards == 0u) return false;
  if (d.x == 0.0f || d.y == 0.0f || d.z == 0.0f) return false;
  const V3 inv = mk(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);  // inv_dir (ray.rs:31-33)
  const float inf = presolve_inf();
  if (!(fabsf(inv.x) < inf) || !(fabsf(inv.y) < inf) || !(fabsf(inv.z) < inf)) return false;
  // the plane seed: planes_closest over plane_hit (plane.rs:80-99)
  float best = inf;
  int32_t best_id = -1;
  bool found = false;
  for (uint32_t i = 0; i < S.num_inf; i++) {
    const V3 n = mk(S.planes[i].x, S.planes[i].y, S.planes[i].z);
    const float n_dot_dir = dot(n, d);
    if (n_dot_dir == 0.0f) continue;
    const float tt = (S.planes[i].w - dot(n, o)) / n_dot_dir;
    if (tt <= 0.0f) continue;
    if (!found || (0.0f < tt && tt < best)) {
      found = true;
      best = tt;
      best_id = (int32_t)i;
    }
  }
  float hh, tmax;
  presolve_slab(B.root, o, inv, hh, tmax);
  if ((hh <= tmax) & (hh < best)) {  // enter_root's verdict: the root is entered
    bool clear = true;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int g = 0; g < kMaxGuards; g++) {
      if ((uint32_t)g < B.num_guards) {
        presolve_slab(B.guard[g], o, inv, hh, tmax);
        clear = clear && (!(hh <= tmax) || best < hh);
      }
    }
    if (!clear) return false;
  }
  t = best_id >= 0 ? best : inf;
  id = best_id;
  return true;
}

// The host's view of a scene's planes for presolve_ray.
struct HostPlanes {
  struct P4 { float x, y, z, w; };
  P4 planes[16];
  uint32_t num_inf;
};

}  // namespace wpt
