// wpt_points.h — hemisphere gathers at a caller's points (wpt_radiance_points,
// include/wpt.h; the definition to the operation: DESIGN.md §2).
//
// A point query is a ray query (wpt_rays.h) whose ray the generator makes: record
// i = {px,py,pz, nx,ny,nz}, and sample s of it leaves the point along a
// direction drawn about the normal from the two jitter draws a camera path
// takes first (the draws a ray query throws away). From there on the path is
// wpt_radiance_rays' path of that ray, so a point's sum is the sequential f32
// sum of ray queries the oracle answers.
//
// Two parts. The first is plain C++ for host and device: point_ray, written
// once for wpt_point_rays (wpt_api.cpp) and the kernels. The second
// (WPT_POINTS_KERNELS, wpt_render.hip, after wpt_rays.h) holds the two
// generators. Included inside namespace wpt, after wpt_rays.h.
#pragma once

constexpr uint32_t kPointsCosine = 0u, kPointsSphere = 1u;  // WPT_POINTS_COSINE / _SPHERE

// The frame about a record's normal: shade_path's xn and zn. Per record, not per
// sample (orthogonal and cross cost two normalises with a divide each).
struct PointFrame {
  V3 n, xn, zn;
};
WPT_HD PointFrame point_frame(V3 n) {
  PointFrame F;
  F.n = n;
  F.xn = orthogonal(n);
  F.zn = cross(n, F.xn);
  return F;
}

// Sample s of a record with frame F at p: the generated ray (o, wi) and the
// stream after the two draws. sample_hemisphere's operations (material.rs:97-118)
// as shade_path states them for COSINE; SPHERE: uniform over the sphere, the
// normal the pole of the parameterisation.
WPT_HD void point_sample(V3 p, const PointFrame& F, uint32_t key, uint32_t seed, uint32_t s, uint32_t dist, V3& o,
                         V3& wi, uint32_t& state) {
  uint32_t st = path_seed(seed, key, s);
  const float r1 = xs_next(st);
  const float r2 = xs_next(st);
  const float ang = (2.0f * kPi) * r1;
  float x, y, z;
  if (dist == kPointsSphere) {
    y = 1.0f - 2.0f * r2;
    const float q = sqrtf(1.0f - y * y);
    x = mcos(ang) * q;
    z = msin(ang) * q;
  } else {
    x = mcos(ang) * sqrtf(1.0f - r2);
    y = sqrtf(r2);
    z = msin(ang) * sqrtf(1.0f - r2);
  }
  wi = normalize(add(add(scale(F.xn, x), scale(F.n, y)), scale(F.zn, z)));
  o = add(p, scale(wi, kEpsilon));  // as a bounce leaves a hit point
  state = st;
}

// The ray of (record, key, sample): false for a record ray_valid rejects (o, wi
// and state are then not written). A generated ray may itself fail ray_valid (a
// normal far from unit length): the caller asks.
WPT_HD bool point_ray(const float* rec, uint32_t key, uint32_t seed, uint32_t s, uint32_t dist, V3& o, V3& wi,
                      uint32_t& state) {
  if (!ray_valid(rec)) return false;
  point_sample(mk(rec[0], rec[1], rec[2]), point_frame(mk(rec[3], rec[4], rec[5])), key, seed, s, dist, o, wi, state);
  return true;
}
WPT_HD bool point_ray_valid(V3 o, V3 wi) {
  const float c[6] = {o.x, o.y, o.z, wi.x, wi.y, wi.z};
  return ray_valid(c);
}

#if defined(WPT_POINTS_KERNELS)

// Position t of the block: its record, the generated ray, whether it is traced
// (a valid record and a valid generated ray) and the path's stream. The block's
// records are staged as rays are (stage_rays: the same 24-byte layout); their
// frames are made once per record by the block's first threads and read from
// LDS by the record's samples (s_frame: xn, zn; a broadcast within a record).
__device__ __forceinline__ void stage_frames(uint32_t nrec, const float* s_ray, float* s_frame) {
  for (uint32_t r = threadIdx.x; r < nrec; r += kBlock) {
    const PointFrame F = point_frame(mk(s_ray[6u * r + 3u], s_ray[6u * r + 4u], s_ray[6u * r + 5u]));
    s_frame[6u * r] = F.xn.x;
    s_frame[6u * r + 1u] = F.xn.y;
    s_frame[6u * r + 2u] = F.xn.z;
    s_frame[6u * r + 3u] = F.zn.x;
    s_frame[6u * r + 4u] = F.zn.y;
    s_frame[6u * r + 5u] = F.zn.z;
  }
  __syncthreads();
}
__device__ __forceinline__ QueryPath point_path(const RayQuery& Q, uint32_t seed, const RayBlock& R, const float* s_ray,
                                                const float* s_frame, uint32_t t) {
  const uint32_t head = Q.spp - R.rem0;  // query_path's mapping
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
  const float* f = s_frame + 6u * lr;
  float c[6];
  for (int k = 0; k < 6; k++) c[k] = r[k];
  PointFrame F;
  F.n = mk(c[3], c[4], c[5]);
  F.xn = mk(f[0], f[1], f[2]);
  F.zn = mk(f[3], f[4], f[5]);
  const uint32_t key = Q.keys ? Q.keys[q.ray] : Q.key0 + q.ray;
  point_sample(mk(c[0], c[1], c[2]), F, key, seed, Q.sample + so, Q.source - 1u, q.o, q.d, q.s);
  q.ok = ray_valid(c) && point_ray_valid(q.o, q.d);
  return q;
}
// the records a block of npos positions from kb on touches (<= kBlock)
__device__ __forceinline__ uint32_t block_records(const RayQuery& Q, uint64_t kb, uint32_t npos) {
  return (uint32_t)((kb + npos - 1u) / Q.spp) - (uint32_t)(kb / Q.spp) + 1u;
}

// k_generate_rays for a point query: the same stream of paths, the ray made
// here. Not bandwidth-bound as that kernel is: the f64 polynomials of msin /
// mcos and three normalises per path.
__global__ void __launch_bounds__(kBlock) k_generate_points(RayQuery Q, uint32_t seed, uint64_t k0, uint32_t n,
                                                            uint32_t* __restrict__ pix_out, float4* __restrict__ thr,
                                                            float4* __restrict__ col, float4* __restrict__ ro,
                                                            float4* __restrict__ rd, uint32_t* __restrict__ count0) {
  constexpr uint32_t kWaves = kBlock / 64;
  __shared__ float s_ray[6 * kBlock];
  __shared__ float s_frame[6 * kBlock];
  __shared__ uint32_t s_off[1][kWaves];
  const BlockAppend<1, kWaves> A{s_off};
  const uint32_t base = blockIdx.x * kBlock;  // < n: the grid is ceil(n / kBlock)
  const uint32_t i = base + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
  const uint32_t npos = n - base < kBlock ? n - base : kBlock;
  const RayBlock R = stage_rays(Q, k0 + base, npos, s_ray);
  stage_frames(block_records(Q, k0 + base, npos), s_ray, s_frame);
  const bool in = i < n;
  const QueryPath q = point_path(Q, seed, R, s_ray, s_frame, in ? threadIdx.x : 0u);
  const bool live = in && q.ok;
  if (in) {
    pix_out[i] = q.ray;
    col[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  }
  const uint64_t lm = __ballot(live);
  if (lane == 0) A.publish(wid, {(uint32_t)__popcll(lm)});
  __syncthreads();
  if (wid == 0) {
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

// k_generate_rays_ps for a point query: presolve_ray on the generated ray, the
// two-ended stream and drop-miss as there.
__global__ void __launch_bounds__(kBlock) k_generate_points_ps(RayQuery Q, uint32_t seed, uint64_t k0, uint32_t n,
                                                               uint32_t* __restrict__ pix_out, float4* __restrict__ thr,
                                                               float4* __restrict__ col, float4* __restrict__ ro,
                                                               float4* __restrict__ rd, uint32_t* __restrict__ count0,
                                                               DevScene S, float* __restrict__ t_out,
                                                               int32_t* __restrict__ id_out, uint32_t* __restrict__ res0,
                                                               uint32_t drop_miss) {
  constexpr uint32_t kWaves = kBlock / 64;
  using F = Fields<16, kBlock>;  // column 1: resolved and stored, dropped
  __shared__ float s_ray[6 * kBlock];
  __shared__ float s_frame[6 * kBlock];
  __shared__ uint32_t s_off[2][kWaves];
  const BlockAppend<2, kWaves> A{s_off};
  const uint32_t base = blockIdx.x * kBlock;
  const uint32_t i = base + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
  const uint64_t below = (1ull << lane) - 1ull;
  const uint32_t npos = n - base < kBlock ? n - base : kBlock;
  const RayBlock R = stage_rays(Q, k0 + base, npos, s_ray);
  stage_frames(block_records(Q, k0 + base, npos), s_ray, s_frame);
  const bool in = i < n;
  const QueryPath q = point_path(Q, seed, R, s_ray, s_frame, in ? threadIdx.x : 0u);
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

#endif  // WPT_POINTS_KERNELS
