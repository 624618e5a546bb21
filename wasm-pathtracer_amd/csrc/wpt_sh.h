// wpt_sh.h — spherical-harmonic projection of a point's gathers (wpt_probe_sh,
// include/wpt.h; the definition to the operation: DESIGN.md §2).
//
// An SH query is a point query (wpt_points.h) whose samples are not summed as
// colours but weighted, each by the real SH basis of its own direction: a
// record's coefficient k is the sequential f32 sum of Y_k(w_j) * c_j over its
// traced samples, in sample order.
//
// Two parts. The first is plain C++ for host and device: the basis, written
// once for wpt_sh_basis (wpt_api.cpp) and the kernel. The second
// (WPT_SH_KERNELS, wpt_render.hip, after wpt_points.h) holds the two kernels
// that stand where k_accumulate_round stands for a query batch. Included inside
// namespace wpt, after wpt_points.h.
#pragma once

constexpr uint32_t kShMaxOrder = 2u;  // WPT_SH_MAX_ORDER
constexpr uint32_t sh_coeffs(uint32_t order) { return (order + 1u) * (order + 1u); }

// The f32 nearest to sqrt(1 / 4pi), sqrt(3 / 4pi), sqrt(15 / 4pi), sqrt(5 / 16pi),
// sqrt(15 / 16pi)
constexpr float kShC0 = 0.282094806f;  // 0x3e906ebb
constexpr float kShC1 = 0.488602519f;  // 0x3efa2a1c
constexpr float kShC2 = 1.09254849f;   // 0x3f8bd8a1
constexpr float kShC3 = 0.31539157f;   // 0x3ea17b01
constexpr float kShC4 = 0.546274245f;  // 0x3f0bd8a1

// Y_k of direction d (used as given), k < 9: real SH in world axes, z the polar
// axis, no Condon-Shortley sign. Every operation is one f32 rounding.
WPT_HD float sh_basis_at(V3 d, uint32_t k) {
  switch (k) {
    case 0u: return kShC0;
    case 1u: return kShC1 * d.y;
    case 2u: return kShC1 * d.z;
    case 3u: return kShC1 * d.x;
    case 4u: return kShC2 * (d.x * d.y);
    case 5u: return kShC2 * (d.y * d.z);
    case 6u: return kShC3 * ((3.0f * (d.z * d.z)) - 1.0f);
    case 7u: return kShC2 * (d.x * d.z);
    default: return kShC4 * ((d.x * d.x) - (d.y * d.y));
  }
}
// the (order + 1)^2 values of orders 0 .. order, order <= kShMaxOrder
WPT_HD void sh_basis(V3 d, uint32_t order, float* Y) {
  const uint32_t nc = sh_coeffs(order);
  for (uint32_t k = 0; k < nc; k++) Y[k] = sh_basis_at(d, k);
}

// wpt_sh_basis: row i of out holds the values of direction dirs3[3i .. 3i + 2]
inline void sh_basis_rows(size_t n, const float* dirs3, uint32_t order, float* out) {
  const size_t nc = sh_coeffs(order);
  for (size_t i = 0; i < n; i++) sh_basis(mk(dirs3[3 * i], dirs3[3 * i + 1], dirs3[3 * i + 2]), order, out + nc * i);
}

#if defined(WPT_SH_KERNELS)

// The direction of every position of a lane's slice, made again from the key
// and the sample index by the generators' own code (point_path: the records and
// their frames staged in LDS, point_sample): dirs[i] = {w.xyz, traced} for
// position k0 + i, traced = 1.0f where the generator appended a path (a valid
// record and a valid generated ray), else +0.
__global__ void __launch_bounds__(kBlock) k_sh_dirs(RayQuery Q, uint32_t seed, uint64_t k0, uint32_t n,
                                                    float4* __restrict__ dirs) {
  __shared__ float s_ray[6 * kBlock];
  __shared__ float s_frame[6 * kBlock];
  const uint32_t base = blockIdx.x * kBlock;  // < n: the grid is ceil(n / kBlock)
  const uint32_t i = base + threadIdx.x;
  const uint32_t npos = n - base < kBlock ? n - base : kBlock;
  const RayBlock R = stage_rays(Q, k0 + base, npos, s_ray);
  stage_frames(block_records(Q, k0 + base, npos), s_ray, s_frame);
  if (i >= n) return;
  const QueryPath q = point_path(Q, seed, R, s_ray, s_frame, threadIdx.x);
  dirs[i] = make_float4(q.d.x, q.d.y, q.d.z, q.ok ? 1.0f : 0.0f);
}

// k_accumulate_round for an SH query: one lane per (path i of the slice,
// coefficient k); the lanes of a record's first path in the slice walk its run
// in sample order (past block ends, as that kernel does) and continue the
// three running sums the target holds, so a record whose samples straddle
// lanes, batches and blocks still sums in sample order. A run's nc lanes are
// neighbours: their loads of col[j] and dirs[j] are one broadcast. An untraced
// sample is skipped, not multiplied by its +0 colour (its direction may be
// non-finite).
__global__ void __launch_bounds__(kBlock) k_accumulate_sh(uint32_t n, uint32_t nc, const uint32_t* __restrict__ pidx,
                                                          const float4* __restrict__ col,
                                                          const float4* __restrict__ dirs, float* __restrict__ sh) {
  const uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  const uint64_t i64 = t / nc;
  if (i64 >= n) return;
  const uint32_t i = (uint32_t)i64, k = (uint32_t)(t - i64 * nc);
  const uint32_t p = pidx[i];
  if (i > 0 && pidx[i - 1] == p) return;
  float* a = sh + ((size_t)p * nc + k) * 3u;
  float x = a[0], y = a[1], z = a[2];
  for (uint32_t j = i; j < n && pidx[j] == p; j++) {
    const float4 w = dirs[j];
    if (w.w == 0.0f) continue;
    const float4 v = col[j];
    const float Y = sh_basis_at(mk(w.x, w.y, w.z), k);
    x += Y * v.x;
    y += Y * v.y;
    z += Y * v.z;
  }
  a[0] = x;
  a[1] = y;
  a[2] = z;
}

#endif  // WPT_SH_KERNELS
