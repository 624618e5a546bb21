// wpt_presolve.h — the exact "presolve" of an extension ray, and further down
// of an NEE shadow ray (presolve_shadow), compiled for both the host (tests,
// guard build) and gfx950 (k_generate, k_shade).
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
constexpr int kMaxGuardLights = 4;  // primitives of all light guards together (presolve_shadow)

struct PresolveBoxes {
  uint32_t num_guards;          // 0: nothing is resolved
  float root[6];                // the BVH2 root's stored bounds: x_min, y_min, z_min, x_max, y_max, z_max
  float guard[kMaxGuards][6];   // the same layout
  // presolve_shadow: bit g set = guard g is a light guard (every primitive of
  // every leaf in it is an emissive triangle); the primitives of all light
  // guards: shape ids and triangle records (tri_record)
  uint32_t light_guards;
  uint32_t num_guard_lights;
  int32_t guard_light_id[kMaxGuardLights];
  float guard_light[kMaxGuardLights][16];
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

// ---------------------------------------------------------------------------
// The exact presolve of an NEE shadow ray (k_shade's presolving variants).
//
// presolve_shadow returns true only when the shadow machine (begin_shadow +
// step<true> + shadow_verdict of wpt_render.hip) ends "unoccluded" for the
// ray; its producer then adds the contribution itself and the ray is written
// to no stream. Operands: the eps-offset origin o, the unit direction d,
// dir_len = |q - p| and the light's shape id, as shade_path emits them.
// It refuses (the ray goes to the stream) unless all of these hold:
//   * Direction: no component of d is 0 and every 1/d is finite (as above).
//   * Planes: no plane has a plane_hit with 0 < t and !(t >= dir_len).
//     begin_shadow's plane result pt is then +inf, a NaN or some t >= dir_len
//     >= early, so it neither ends at a plane (pt < early) nor seeds the
//     search with one (pt < dir_len): best = dir_len, best_id = -1.
//   * Ordinary guards: each is missed or lies strictly behind dir_len
//     (!(hh <= tmax) || dir_len < hh, presolve_slab). best starts at dir_len
//     and only shrinks (leaf_test accepts t <= max_dis = best), so the
//     monotonicity argument above holds with dir_len in place of the plane
//     seed: box_entry fails for every leaf box in such a guard wherever it is
//     tested (the root included, when it is a leaf), no entry is pushed for
//     one, and no leaf of it is entered: none of its primitives is tested.
//   * Light guards (build_guards: every primitive of every leaf in the group
//     is an emissive triangle, and all light guards together hold at most
//     kMaxGuardLights primitives): not box-tested, since the box holds the
//     ray's target and its entry is about dir_len. For each of their
//     primitives other than `light`, tri_hit's operations on the same 64-B
//     record (tri_hit_rec) must not report a hit with !(t >= dir_len).
// Why that is exact. The machine sets "occluded" in two ways only:
//   (a) leaf_test: a shape sid != light with a hit and t < early, where
//       early = dir_len or min(tl, dir_len) <= dir_len;
//   (b) shadow_verdict: best_id >= 0 && best < dir_len && best_id != light,
//       where best_id >= 0 was accepted by leaf_test with t = best <= max_dis
//       <= dir_len (the plane seed is excluded above).
// Either way a primitive other than `light` has a pure hit with t < dir_len,
// and it sits in a leaf the machine entered. Under the conditions the only
// enterable leaves are the light guards', and tri_hit depends on neither best
// nor the visit order, so the test over their primitives excludes (a) and (b)
// whatever the order or the tie rule. begin_shadow's own test of `light` only
// sets `early`. The BVH4 fast path with its exact re-trace returns the BVH2
// machine's verdict by its own contract (wpt_trav4.h), so both traversals are
// covered. A NaN direction (p == q) fails the 1/d test; scenes without a BVH
// or without finite shapes have num_guards = 0 and resolve nothing.
// ---------------------------------------------------------------------------

// The triangle record of the kernels (4 float4: (v0, n.x) (v1, n.y) (v2, n.z)
// (normalize(n), n . v0), n = (v1 - v0) x (v2 - v0)) from a triangle's nine
// vertex floats (triangle.rs:164, :172, :183).
WPT_HD void tri_record(const float* g, float* out) {
  const V3 v0 = mk(g[0], g[1], g[2]), v1 = mk(g[3], g[4], g[5]), v2 = mk(g[6], g[7], g[8]);
  const V3 n = cross(sub(v1, v0), sub(v2, v0));
  const V3 nn = normalize(n);
  const float od = dot(n, v0);
  out[0] = v0.x; out[1] = v0.y; out[2] = v0.z; out[3] = n.x;
  out[4] = v1.x; out[5] = v1.y; out[6] = v1.z; out[7] = n.y;
  out[8] = v2.x; out[9] = v2.y; out[10] = v2.z; out[11] = n.z;
  out[12] = nn.x; out[13] = nn.y; out[14] = nn.z; out[15] = od;
}

// tri_hit of wpt_render.hip on such a record: the same f32 operations in the
// same order (triangle.rs:159-191), hence the same verdict and t.
WPT_HD bool tri_hit_rec(const float* r, V3 o, V3 d, float& t) {
  const V3 n = mk(r[3], r[7], r[11]);
  const float n_dot_d = dot(n, d);
  if (n_dot_d == 0.0f) return false;
  const float tt = (r[15] - dot(n, o)) / n_dot_d;
  if (tt <= 0.0f) return false;
  const V3 nn = mk(r[12], r[13], r[14]);
  const V3 pp = add(o, scale(d, tt));
  const V3 v0 = mk(r[0], r[1], r[2]), v1 = mk(r[4], r[5], r[6]), v2 = mk(r[8], r[9], r[10]);
  if (!(dot(nn, cross(sub(v1, v0), sub(pp, v0))) + kTriSlack >= 0.0f)) return false;
  if (!(dot(nn, cross(sub(v2, v1), sub(pp, v1))) + kTriSlack >= 0.0f)) return false;
  if (!(dot(nn, cross(sub(v0, v2), sub(pp, v2))) + kTriSlack >= 0.0f)) return false;
  t = tt;
  return true;
}

// A shadow ray's operands from its end points, shade_path's operations
// (Scene::shadow_ray, scene.rs:105-108): d = (q - p) / |q - p|, o = p + d * EPSILON.
WPT_HD void shadow_operands(V3 p, V3 q, V3& o, V3& d, float& dir_len) {
  V3 tl = sub(q, p);
  dir_len = sqrtf(dot(tl, tl));
  tl = divs(tl, dir_len);
  o = add(p, scale(tl, kEpsilon));
  d = tl;
}

template <class SC>
WPT_HD bool presolve_shadow(const SC& S, const PresolveBoxes& B, V3 o, V3 d, float dir_len, int32_t light) {
  if (B.num_guards == 0u) return false;
  if (d.x == 0.0f || d.y == 0.0f || d.z == 0.0f) return false;
  const V3 inv = mk(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
  const float inf = presolve_inf();
  if (!(fabsf(inv.x) < inf) || !(fabsf(inv.y) < inf) || !(fabsf(inv.z) < inf)) return false;
  // no plane in front of the target (plane_hit, plane.rs:80-99)
  for (uint32_t i = 0; i < S.num_inf; i++) {
    const V3 n = mk(S.planes[i].x, S.planes[i].y, S.planes[i].z);
    const float n_dot_dir = dot(n, d);
    if (n_dot_dir == 0.0f) continue;
    const float tt = (S.planes[i].w - dot(n, o)) / n_dot_dir;
    if (tt <= 0.0f) continue;
    if (0.0f < tt && !(tt >= dir_len)) return false;
  }
  // every ordinary guard missed or strictly behind the target
  bool clear = true;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int g = 0; g < kMaxGuards; g++) {
    if ((uint32_t)g < B.num_guards && ((B.light_guards >> g) & 1u) == 0u) {
      float hh, tmax;
      presolve_slab(B.guard[g], o, inv, hh, tmax);
      clear = clear && (!(hh <= tmax) || dir_len < hh);
    }
  }
  if (!clear) return false;
  // no other primitive of a light guard hit before the target
  for (uint32_t k = 0; k < B.num_guard_lights; k++) {
    if (B.guard_light_id[k] == light) continue;
    float t;
    if (tri_hit_rec(B.guard_light[k], o, d, t) && !(t >= dir_len)) return false;
  }
  return true;
}

// The host's view of a scene's planes for presolve_ray.
struct HostPlanes {
  struct P4 { float x, y, z, w; };
  P4 planes[16];
  uint32_t num_inf;
};

}  // namespace wpt
