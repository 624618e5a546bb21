// wpt_rays.h — radiance along a caller's rays (wpt_radiance_rays,
// include/wpt.h; the definition to the operation: DESIGN.md §2).
//
// A ray query is a camera path whose primary ray the caller supplies: position
// k of a call is ray k / spp, sample `sample` + k % spp, on the stream
// path_seed(frame_seed, key, sample) advanced by primary_dir's two jitter draws.
// From bounce 0 on the path is any batch's: the generators below only stand
// where k_generate / k_generate_ps stand for camera paths.
//
// Two parts. The first is plain C++ for host and device: the validity rule. The
// second (WPT_RAYS_KERNELS, wpt_render.hip) holds the kernels. Included inside
// namespace wpt.
#pragma once

// A ray {ox,oy,oz,dx,dy,dz} is traced if its six components are finite and its
// direction is not three zeros (of either sign). On the bits: no comparison
// whose result a denormal mode could change.
WPT_HD bool ray_valid(const float* r) {
  bool finite = true;
  for (int k = 0; k < 6; k++) finite = finite && (f2u(r[k]) & 0x7f800000u) != 0x7f800000u;
  const uint32_t mag = (f2u(r[3]) | f2u(r[4]) | f2u(r[5])) & 0x7fffffffu;
  return finite && mag != 0u;
}

#if defined(WPT_RAYS_KERNELS)

// The rays of a block's kBlock consecutive positions, staged in LDS: at most
// kBlock rays (spp = 1), 24 bytes each in the caller's AoS layout. The block
// reads the 6 * rays floats as consecutive dwords, thread t the floats t,
// t + kBlock, ...: every load instruction of a wave covers 256 contiguous bytes
// (six 4-byte loads at a 24-byte stride per lane would touch six times the
// lines per instruction), and a dword needs no alignment the caller's pointer
// might not have, which 96 float4 loads per wave would. A lane then reads its
// ray from LDS (stride 6 dwords: two lanes per bank at spp = 1, a broadcast
// within a ray's samples).
struct RayBlock {
  uint32_t r0;    // the block's first ray
  uint32_t rem0;  // the sample offset of its first position within that ray
};
__device__ __forceinline__ RayBlock stage_rays(const RayQuery& Q, uint64_t kb, uint32_t npos, float* s_ray) {
  RayBlock R;
  R.r0 = (uint32_t)(kb / Q.spp);
  R.rem0 = (uint32_t)(kb % Q.spp);
  const uint32_t r1 = (uint32_t)((kb + npos - 1u) / Q.spp);
  const uint32_t nf = 6u * (r1 - R.r0 + 1u);  // <= 6 * kBlock: r1 - r0 <= npos - 1
  const float* __restrict__ src = Q.rays + 6 * (size_t)R.r0;
  for (uint32_t f = threadIdx.x; f < nf; f += kBlock) s_ray[f] = src[f];
  __syncthreads();
  return R;
}

// Position t of the block: its ray (of the call's chunk), origin, direction,
// validity and the path's stream after the two discarded jitter draws.
struct QueryPath {
  uint32_t ray, s;
  V3 o, d;
  bool ok;
};
__device__ __forceinline__ QueryPath query_path(const RayQuery& Q, uint32_t seed, const RayBlock& R,
                                                const float* s_ray, uint32_t t) {
  // 32-bit arithmetic: t < kBlock, and the 64-bit division is the block's
  const uint32_t head = Q.spp - R.rem0;  // positions left in the block's first ray
  uint32_t lr, so;
  if (t < head) {
    lr = 0u;
    so = R.rem0 + t;
  } else {
    const uint32_t u = t - head;
    lr = 1u + u / Q.spp;
    so = u % Q.spp;
  }
  QueryPath q;
  q.ray = R.r0 + lr;
  const float* r = s_ray + 6u * lr;
  float c[6];
  for (int k = 0; k < 6; k++) c[k] = r[k];
  q.ok = ray_valid(c);
  q.o = mk(c[0], c[1], c[2]);
  q.d = mk(c[3], c[4], c[5]);
  const uint32_t key = Q.keys ? Q.keys[q.ray] : Q.key0 + q.ray;
  uint32_t s = path_seed(seed, key, Q.sample + so);
  xs_next_u32(s);  // primary_dir's two jitter draws, taken and discarded
  xs_next_u32(s);
  q.s = s;
  return q;
}

// The producer of a query batch that presolves nothing (what k_generate is for
// camera paths): positions k0 .. k0 + n - 1 of the chunk. The radiance and the
// ray's index stay at the path's batch index i; an invalid ray's paths are
// compacted out of the stream (the valid ones are appended to its front, one
// reservation per block), so they cost no ray and their colour stays +0.
__global__ void __launch_bounds__(kBlock) k_generate_rays(RayQuery Q, uint32_t seed, uint64_t k0, uint32_t n,
                                                          uint32_t* __restrict__ pix_out, float4* __restrict__ thr,
                                                          float4* __restrict__ col, float4* __restrict__ ro,
                                                          float4* __restrict__ rd, uint32_t* __restrict__ count0) {
  constexpr uint32_t kWaves = kBlock / 64;
  __shared__ float s_ray[6 * kBlock];
  __shared__ uint32_t s_off[1][kWaves];
  const BlockAppend<1, kWaves> A{s_off};
  const uint32_t base = blockIdx.x * kBlock;  // < n: the grid is ceil(n / kBlock)
  const uint32_t i = base + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
  const RayBlock R = stage_rays(Q, k0 + base, (n - base < kBlock ? n - base : kBlock), s_ray);
  const bool in = i < n;
  const QueryPath q = query_path(Q, seed, R, s_ray, in ? threadIdx.x : 0u);
  const bool live = in && q.ok;
  if (in) {
    pix_out[i] = q.ray;
    col[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  }
  const uint64_t lm = __ballot(live);
  if (lane == 0) A.publish(wid, {(uint32_t)__popcll(lm)});
  __syncthreads();
  if (wid == 0) {
    // lane kWaves - 1: the block's rays to count0 (64-bit: the word after it is unused)
    A.reserve(lane, {{0, false, ~0u}},
              [&](const uint32_t(&incl)[1]) { return A.take(count0, incl[0], 0u, lane == kWaves - 1); });
  }
  __syncthreads();
  if (!live) return;
  const uint32_t p = A.at(0, wid, (uint32_t)__popcll(lm & ((1ull << lane) - 1ull)));
  thr[p] = make_float4(1.0f, 1.0f, 1.0f, __uint_as_float(Q.type << kTypeShift));
  ro[p] = make_float4(q.o.x, q.o.y, q.o.z, __uint_as_float(q.s));  // w: the path's rng state
  rd[p] = make_float4(q.d.x, q.d.y, q.d.z, __uint_as_float(i));    // w: the path's index in the batch
}

// The same for a presolving batch (what k_generate_ps is for camera paths; a
// body of its own, so that kernel's code stays as it is): presolve_ray on the
// query ray, unresolved rays to the front of the two-ended stream (count0),
// resolved ones with their (t, id) to the back (res0's low word), a ray
// resolved to a miss that adds nothing dropped under drop_miss (res0's high
// word), both ranges reserved by one atomic instruction per block. An invalid
// ray's paths enter neither end and no count.
__global__ void __launch_bounds__(kBlock) k_generate_rays_ps(RayQuery Q, uint32_t seed, uint64_t k0, uint32_t n,
                                                             uint32_t* __restrict__ pix_out, float4* __restrict__ thr,
                                                             float4* __restrict__ col, float4* __restrict__ ro,
                                                             float4* __restrict__ rd, uint32_t* __restrict__ count0,
                                                             DevScene S, float* __restrict__ t_out,
                                                             int32_t* __restrict__ id_out, uint32_t* __restrict__ res0,
                                                             uint32_t drop_miss) {
  constexpr uint32_t kWaves = kBlock / 64;
  using F = Fields<16, kBlock>;  // column 1: resolved and stored, dropped
  __shared__ float s_ray[6 * kBlock];
  __shared__ uint32_t s_off[2][kWaves];
  const BlockAppend<2, kWaves> A{s_off};
  const uint32_t base = blockIdx.x * kBlock;
  const uint32_t i = base + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
  const uint64_t below = (1ull << lane) - 1ull;
  const RayBlock R = stage_rays(Q, k0 + base, (n - base < kBlock ? n - base : kBlock), s_ray);
  const bool in = i < n;
  const QueryPath q = query_path(Q, seed, R, s_ray, in ? threadIdx.x : 0u);
  const bool live = in && q.ok;
  const bool drop_misses = drop_miss != 0u && adds_nothing(mk(1.0f, 1.0f, 1.0f), S);
  float t = 0.0f;
  int32_t id = -1;
  const bool res = live && presolve_ray(S, *S.pre, q.o, q.d, t, id);
  const bool drop = res && id < 0 && drop_misses;
  if (in) {
    pix_out[i] = q.ray;
    col[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  }
  const uint64_t hm = __ballot(live && !res), rm = __ballot(res && !drop), dm = __ballot(drop);
  if (lane == 0) A.publish(wid, {(uint32_t)__popcll(hm), F::pack((uint32_t)__popcll(rm), (uint32_t)__popcll(dm))});
  __syncthreads();
  if (wid == 0) {
    // lane kWaves - 1: the unresolved rays to count0; lane kWaves: resolved and stored | dropped to res0
    A.reserve(lane, {{0, false, ~0u}, {1, false, F::kMask}}, [&](const uint32_t(&incl)[2]) {
      const uint32_t tb = A.total(incl[1]);
      const bool first = lane == kWaves - 1;
      return A.take(first ? count0 : res0, first ? incl[0] : F::get(tb, 0), first ? 0u : F::top(tb, 1),
                    first || lane == kWaves);
    });
  }
  __syncthreads();
  const bool front = (hm >> lane) & 1ull, back = (rm >> lane) & 1ull;
  if (!front && !back) return;  // past the batch's end, invalid, or dropped
  uint32_t p;  // the ray's entry in the stream
  if (back) {
    p = n - 1u - A.at(1, wid, (uint32_t)__popcll(rm & below));
    t_out[p] = t;
    id_out[p] = id;
  } else {
    p = A.at(0, wid, (uint32_t)__popcll(hm & below));
  }
  thr[p] = make_float4(1.0f, 1.0f, 1.0f, __uint_as_float(Q.type << kTypeShift));
  ro[p] = make_float4(q.o.x, q.o.y, q.o.z, __uint_as_float(q.s));  // w: the path's rng state
  rd[p] = make_float4(q.d.x, q.d.y, q.d.z, __uint_as_float(i));    // w: the path's index in the batch
}

// One lane per ray of a chunk: its status byte (launched only when the caller
// asks for them; the call's paths come from the batches' bounce-0 counts).
__global__ void __launch_bounds__(kBlock) k_rays_status(uint32_t n, const float* __restrict__ rays,
                                                        uint8_t* __restrict__ status) {
  __shared__ float s_ray[6 * kBlock];
  const uint32_t base = blockIdx.x * kBlock;
  const uint32_t nf = 6u * (n - base < kBlock ? n - base : kBlock);
  const float* __restrict__ src = rays + 6 * (size_t)base;
  for (uint32_t f = threadIdx.x; f < nf; f += kBlock) s_ray[f] = src[f];
  __syncthreads();
  const uint32_t i = base + threadIdx.x;
  if (i >= n) return;
  float c[6];
  for (int k = 0; k < 6; k++) c[k] = s_ray[6u * threadIdx.x + k];
  status[i] = ray_valid(c) ? 1 : 0;
}

// The query's float4 sums to the caller's packed rgb.
__global__ void __launch_bounds__(kBlock) k_rays_unpack(uint32_t n, const float4* __restrict__ acc,
                                                        float* __restrict__ rgb3) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const float4 a = acc[i];
  rgb3[3 * (size_t)i] = a.x;
  rgb3[3 * (size_t)i + 1] = a.y;
  rgb3[3 * (size_t)i + 2] = a.z;
}

#endif  // WPT_RAYS_KERNELS
