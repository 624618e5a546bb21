// wpt_first_hit.h — first-hit feature planes (wpt_first_hit, include/wpt.h):
// the integrator's debug variants trace_original_depth / trace_original_bvh
// (tracer.rs:205-219) for one primary ray per frame pixel, plus the surface
// planes a host needs beside them (normal, albedo, kind).
//
// Included by wpt_render.hip inside its anonymous namespace, after the
// traversal machine, gen_path and hit_normal, which it calls and does not
// restate: the ray of a pixel is gen_path's (the bits wpt_compute traces for
// that pixel and sample), the closest hit is begin_extend + step on the exact
// BVH2 (also on scenes whose production batches run the BVH4 fast path), the
// material is the shade kernels' S.mats lookup.
//
// Visit count = the reference's num_bvh_hits of the ray (scene.rs:191-288):
// one per traverse_bvh call and one per traverse_bvh_guarded call. The
// machine's COUNT visits give 1 for the guarded root, 1 per internal node
// expanded and 1 per leaf tested; step's REF_VISITS adds the one call they
// lack, the guarded right child of a node whose left box test fails. 0 where
// no BVH is traversed (no finite shape, or the BVH disabled).
//
// Lane mapping: one lane per pixel, a wave per 8 x 8 pixel tile, tiles in
// raster order; a block's waves take consecutive tiles and, on a grid clamped
// by the spill area, further ones a grid stride on. Lanes of a tile that
// overhang the viewport never start a ray but stay in the wave's loop, so the
// machine's wave-wide tests (push / pop's __any) see the whole wave.
//
// Occupancy: the block is the traversal kernels' (kTBlock lanes: the LDS stack
// and the treelet are laid out for it), 9 stack slots + treelet + lights =
// 19.9 KB of LDS, and the launch bounds are theirs, so 8 blocks per CU fit
// (WPT_TRACE_WAVES). One-shot, no feed: a wave's 64 rays start together and
// the wave leaves when its slowest ray ends.
#pragma once

constexpr uint32_t kFhDir = 1u, kFhT = 2u, kFhId = 4u, kFhVisits = 8u, kFhNormal = 16u, kFhAlbedo = 32u,
                   kFhKind = 64u;
constexpr size_t kFhElem[7] = {12, 4, 4, 4, 12, 12, 1};  // bytes per pixel of the planes, in kFh* bit order
constexpr uint32_t kFhTile = 8;  // pixels per tile side: kFhTile^2 = one wave
static_assert(kFhTile * kFhTile == 64 && kTBlock % 64 == 0, "a wave per tile");

struct FirstHitParams {
  GenParams G;  // npix = W * H: path k = sample * npix + pixel
  uint32_t sample;
  uint32_t mask;  // kFh*: the planes wanted; the others are neither computed nor stored
  uint32_t tiles_x, ntiles;
  float* dir;       // 3 per pixel
  float* t;
  int32_t* id;
  uint32_t* visits;
  float* normal;    // 3 per pixel
  float* albedo;    // 3 per pixel
  uint8_t* kind;
};

template <bool TRI_ONLY>
__global__ void WPT_TRACE_BOUNDS k_first_hit(DevScene S, FirstHitParams P, uint2* __restrict__ spill) {
  __shared__ uint32_t s_code[kLdsSlots * kTBlock];
  __shared__ float s_h[kLdsSlots * kTBlock];
  __shared__ float s_lrec[16 * kLdsLights];
  __shared__ int32_t s_lid[kLdsLights];
  __shared__ f4v s_tree[4 * kTreePairs + 1];
  const Hot H = load_hot(S, (lds_f32h*)s_lrec, (lds_i32*)s_lid, (lds_f4v*)s_tree, (const float4*)s_tree);
  const uint32_t G = gridDim.x * kTBlock;
  const Stack stk{(lds_u32*)(s_code + threadIdx.x), (lds_f32*)(s_h + threadIdx.x),
                  spill + blockIdx.x * kTBlock + threadIdx.x, G, S.stack_cap, S.overflow};
  constexpr uint32_t kWaves = kTBlock / 64;
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const float inf = __int_as_float(0x7f800000);
  const V3 o = mk(P.G.cam[0], P.G.cam[1], P.G.cam[2]);
  // wave-uniform: every lane of a wave makes the same trips
  for (uint32_t tile = blockIdx.x * kWaves + wave; tile < P.ntiles; tile += gridDim.x * kWaves) {
    const uint32_t x = (tile % P.tiles_x) * kFhTile + (lane % kFhTile);
    const uint32_t y = (tile / P.tiles_x) * kFhTile + (lane / kFhTile);
    const bool inside = x < P.G.W && y < P.G.H;
    const uint32_t pixel = inside ? y * P.G.W + x : 0u;
    const GenPath g = gen_path(P.G, nullptr, (uint64_t)P.sample * P.G.npix + pixel, nullptr, nullptr, nullptr);
    uint32_t visits = 0, tests = 0, nbytes = 0;
    bool dummy = false;
    Lane L;
    L.best = inf;
    L.best_id = -1;
    bool live = false;
    if (inside) live = begin_extend<TRI_ONLY, true, false>(S, H, L, o, g.v, visits, tests, nbytes);
    while (__any(live)) {
      if (live) live = step<false, TRI_ONLY, true, false, true>(S, H, L, stk, -1, 0.0f, dummy, visits, tests, nbytes);
    }
    if (!inside) continue;
    const V3 d = L.d;  // g.v (begin_extend): not held twice across the walk
    const int32_t id = L.best_id;
    const bool hit = id >= 0;
    const float t = hit ? L.best : inf;
    if (P.mask & kFhDir) st3(P.dir + 3 * (size_t)pixel, d);
    if (P.mask & kFhT) P.t[pixel] = t;
    if (P.mask & kFhId) P.id[pixel] = id;
    if (P.mask & kFhVisits) P.visits[pixel] = visits;
    if (P.mask & kFhNormal) {
      V3 n = mk(0.0f, 0.0f, 0.0f);
      if (hit) n = hit_normal<TRI_ONLY>(S, id, o, d, t);
      st3(P.normal + 3 * (size_t)pixel, n);
    }
    if (P.mask & (kFhAlbedo | kFhKind)) {
      float4 m = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (hit) m = S.mats[id];
      if (P.mask & kFhAlbedo) st3(P.albedo + 3 * (size_t)pixel, ld3(m));
      if (P.mask & kFhKind) P.kind[pixel] = hit ? (m.w != 0.0f ? 2 : 1) : 0;
    }
  }
}
