// wpt_guided.h — guided sampling: a per-pixel sample map planned from the
// session's counts and the history length wpt_reproject recovered
// (wpt_sample_map, wpt_sample_map_planes, wpt_sample_map_host), and the plan
// of a batch that traces such a map (wpt_compute_map); include/wpt.h, the
// definition to the operation: DESIGN.md §2.
//
// After a camera move the accumulation starts at zero, but wpt_reproject gives
// most pixels a history of len samples. A pixel's effective count is
// e = min(cnt + len, 2^32 - 1); it needs min(max(target - e, 0), max_per_pixel)
// new samples, and a budget below the sum T of the needs is dealt in
// proportion: with P the exclusive prefix of the needs in raster order,
// count[p] = floor(P[p+1] * budget / T) - floor(P[p] * budget / T). The floors
// telescope, so the counts sum to the budget exactly, no count exceeds its need
// (budget < T) and a pixel that needs nothing gets nothing (P[p+1] == P[p]).
// All of it is u32 / u64 integer arithmetic: T and budget are below 2^32, so no
// product wraps, and host and device agree on every bit without further care.
//
// Two parts. The first is plain C++ for host and device: the two rules and the
// host restatement that calls them on planes. The second holds the kernels,
// which call the same two functions, under two guards so that each is compiled
// in one unit: the planning kernels (WPT_GUIDED_KERNELS, wpt_post.hip) are
// k_map_need, a three-pass exclusive scan of u64 (the shape of k_scan_local /
// k_scan_sums / k_scan_add, wpt_adaptive.h) and k_map_deal; k_map_plan
// (WPT_GUIDED_PLAN_KERNEL, wpt_render.hip) belongs to the tracing call.
// Included inside namespace wpt, after wpt_reproject.h.
#pragma once

constexpr uint32_t kMapMissOnce = 1u;  // WPT_MAP_MISS_ONCE

// The samples pixel p needs. kind: the first-hit kind of the guide sample
// (read under kMapMissOnce only).
WPT_HD uint32_t map_need(uint32_t cnt, uint32_t len, uint32_t kind, bool member, uint32_t target, uint32_t max_pp,
                         uint32_t flags) {
  if (!member) return 0u;
  if ((flags & kMapMissOnce) && kind == 0u) return cnt == 0u ? 1u : 0u;
  const uint64_t s = (uint64_t)cnt + (uint64_t)len;
  const uint32_t e = s > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)s;
  const uint32_t d = target > e ? target - e : 0u;
  return d < max_pp ? d : max_pp;
}

// The samples a pixel gets: p0, p1 the exclusive prefix of the needs at the
// pixel and after it, T their sum (below 2^32, as budget is).
WPT_HD uint32_t map_deal(uint64_t p0, uint64_t p1, uint64_t budget, uint64_t T) {
  if (budget == 0ull || T <= budget) return (uint32_t)(p1 - p0);
  return (uint32_t)(p1 * budget / T - p0 * budget / T);
}

// The sum of the counts map_deal gives over a frame whose needs sum to T.
inline uint64_t map_dealt(uint64_t budget, uint64_t T) { return budget == 0ull || T <= budget ? T : budget; }

// The restatement on the host. False (nothing written but total_out[0]) if the
// needs sum to 2^32 or more.
inline bool sample_map_host(uint32_t W, uint32_t H, const uint32_t* cnt, const uint32_t* len, const uint8_t* kind,
                            const uint8_t* member, uint32_t target, uint32_t max_pp, uint32_t budget, uint32_t flags,
                            uint32_t* count_out, uint64_t* total_out) {
  const size_t np = (size_t)W * H;
  uint64_t T = 0;
  for (size_t i = 0; i < np; i++) T += map_need(cnt[i], len[i], kind[i], member[i] != 0, target, max_pp, flags);
  if (total_out) { total_out[0] = T; total_out[1] = 0; }
  if (T >= (1ull << 32)) return false;
  if (total_out) total_out[1] = map_dealt(budget, T);
  if (!count_out) return true;
  uint64_t p0 = 0;
  for (size_t i = 0; i < np; i++) {
    const uint64_t p1 = p0 + map_need(cnt[i], len[i], kind[i], member[i] != 0, target, max_pp, flags);
    count_out[i] = map_deal(p0, p1, budget, T);
    p0 = p1;
  }
  return true;
}

#if defined(WPT_GUIDED_KERNELS)

// One lane per pixel: its need as the u64 the scan runs over; entry np = 0 is
// the scan's sentinel (after the scan it holds T). A null len plane is 0
// everywhere (no reprojection in this accumulation), a null member plane 1
// everywhere (one rank), a null kind plane is never read (no kMapMissOnce).
__global__ void __launch_bounds__(kBlock) k_map_need(uint32_t np, const uint32_t* __restrict__ cnt,
                                                     const uint32_t* __restrict__ len,
                                                     const uint8_t* __restrict__ kind,
                                                     const uint8_t* __restrict__ member, uint32_t target,
                                                     uint32_t max_pp, uint32_t flags, u64* __restrict__ need) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i > np) return;
  if (i == np) { need[i] = 0ull; return; }
  need[i] = map_need(cnt[i], len ? len[i] : 0u, kind ? kind[i] : 1u, member ? member[i] != 0 : true, target, max_pp,
                     flags);
}

// Exclusive scan of n u64 (in place), three passes as the u32 one's
// (wpt_adaptive.h): per-chunk scans and sums, one block scanning the chunk
// sums kBlock at a time with a carry, then each chunk adds its offset.
__device__ __forceinline__ u64 shfl_up64(u64 v, int d) {
  const uint32_t lo = __shfl_up((uint32_t)v, d, 64), hi = __shfl_up((uint32_t)(v >> 32), d, 64);
  return (u64)lo | ((u64)hi << 32);
}
__device__ __forceinline__ u64 block_excl_scan64(u64 v, u64& total) {
  __shared__ u64 ws[kBlock / 64];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  u64 inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const u64 y = shfl_up64(inc, d);
    if (lane >= d) inc += y;
  }
  if (lane == 63) ws[wid] = inc;
  __syncthreads();
  u64 pre = 0;
  total = 0;
  for (int w = 0; w < (int)(kBlock / 64); w++) {
    if (w < wid) pre += ws[w];
    total += ws[w];
  }
  __syncthreads();
  return pre + inc - v;
}

__global__ void __launch_bounds__(kBlock) k_scan64_local(u64* __restrict__ a, uint32_t n, u64* __restrict__ sums) {
  const uint64_t base = (uint64_t)blockIdx.x * kScanChunk + threadIdx.x * kScanPer;
  u64 v[kScanPer], t = 0;
#pragma unroll
  for (uint32_t k = 0; k < kScanPer; k++) {
    v[k] = base + k < n ? a[base + k] : 0ull;
    t += v[k];
  }
  u64 total;
  u64 off = block_excl_scan64(t, total);
#pragma unroll
  for (uint32_t k = 0; k < kScanPer; k++) {
    if (base + k < n) a[base + k] = off;
    off += v[k];
  }
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

__global__ void __launch_bounds__(kBlock) k_scan64_sums(u64* __restrict__ sums, uint32_t nb) {
  u64 carry = 0;
  for (uint32_t c0 = 0; c0 < nb; c0 += kBlock) {
    const uint32_t i = c0 + threadIdx.x;
    const u64 v = i < nb ? sums[i] : 0ull;
    u64 total;
    const u64 e = block_excl_scan64(v, total);
    if (i < nb) sums[i] = carry + e;
    carry += total;
  }
}

__global__ void __launch_bounds__(kBlock) k_scan64_add(u64* __restrict__ a, uint32_t n, const u64* __restrict__ sums) {
  const uint64_t base = (uint64_t)blockIdx.x * kScanChunk + threadIdx.x * kScanPer;
  const u64 off = sums[blockIdx.x];
#pragma unroll
  for (uint32_t k = 0; k < kScanPer; k++)
    if (base + k < n) a[base + k] += off;
}

// One lane per pixel: its share of the budget from the scanned needs
// (pre[np] = T).
__global__ void __launch_bounds__(kBlock) k_map_deal(uint32_t np, const u64* __restrict__ pre, uint32_t budget,
                                                     uint32_t* __restrict__ count) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= np) return;
  count[i] = map_deal(pre[i], pre[i + 1], budget, pre[np]);
}

#endif  // WPT_GUIDED_KERNELS

#if defined(WPT_GUIDED_PLAN_KERNEL)

// The plan of a batch that traces a sample map: per partition entry p its
// pixel's count (then, scanned, its first position) and base = the pixel's
// sample count, the next unused sample index; off[npart] = 0 is the scan's
// sentinel. words: [0] the sum of the counts (u64, one atomic per wave),
// [1] set if a pixel's cnt + count would pass 2^32 - 1.
__global__ void __launch_bounds__(kBlock) k_map_plan(const uint32_t* __restrict__ part_pix, uint32_t npart,
                                                     const uint32_t* __restrict__ map,
                                                     const uint32_t* __restrict__ cnt, uint32_t* __restrict__ off,
                                                     uint32_t* __restrict__ base, u64* __restrict__ words) {
  const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
  uint32_t c = 0u;
  if (p < npart) {
    const uint32_t pixel = part_pix ? part_pix[p] : p;
    const uint32_t b = cnt[pixel];
    c = map[pixel];
    off[p] = c;
    base[p] = b;
    if (c > 0xFFFFFFFFu - b) words[1] = 1ull;  // (every writer stores the same value)
  } else if (p == npart) {
    off[p] = 0u;
  }
  u64 s = c;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const uint32_t lo = __shfl_down((uint32_t)s, d, 64), hi = __shfl_down((uint32_t)(s >> 32), d, 64);
    s += (u64)lo | ((u64)hi << 32);
  }
  if ((threadIdx.x & 63) == 0 && s != 0ull) atomicAdd(words, s);
}

#endif  // WPT_GUIDED_PLAN_KERNEL
