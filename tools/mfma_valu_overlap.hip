// Micro-benchmark: how much of the K4x matcher's per-block vector work (the 16-way maximum of the previous block's accumulators, the
// compare + branch, the fp4 expansion of the next rows) hides behind its v_mfma_f32_32x32x64_f8f6f4 chain, two waves per SIMD as in
// the product kernel. A "block" is NM dependent MFMAs into one of two alternating accumulators; the test of a block runs after the
// next block's first MFMA was issued (the product's software pipeline). Prints ns per block per SIMD for every variant; the sum
// model (MFMA-only time + VALU-only time) and the overlap model (the larger of the two) bracket what the hardware does.
//   hipcc -O3 --offload-arch=gfx950 -o tools/mfma_valu_overlap tools/mfma_valu_overlap.hip
//   tools/mfma_valu_overlap              every line
//   tools/mfma_valu_overlap pairs [turns]  two split blocks per accumulator against today's block, then the packing's exactness (below)
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include "../tod_amd/csrc/match_pair_pack.h"

typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef __attribute__((ext_vector_type(16))) float f32x16;
constexpr int kIters = 8192;   // trips of two blocks

__host__ __device__ __forceinline__ unsigned mix(unsigned x) { x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16; return x; }

template <int NM>
__device__ __forceinline__ f32x16 block(const i32x8 (&a)[4], const i32x8 (&b)[4]) {
  f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < NM; ++s) acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a[s], b[s], acc, 4, 4, 0, 0, 0, 0);
  return acc;
}

// TEST 1: the product's chain (max, 7 max3); 2: a tree (5 independent max3, then 2 max3 + max); 3: chain on 8 of the 16 registers
template <int TEST>
__device__ __forceinline__ bool test(const f32x16& acc, float thr) {
  if (TEST == 1) {
    int m = max(max(__float_as_int(acc[0]), __float_as_int(acc[1])), __float_as_int(acc[2]));
#pragma unroll
    for (int i = 3; i < 15; i += 2) m = max(max(m, __float_as_int(acc[i])), __float_as_int(acc[i + 1]));
    m = max(m, __float_as_int(acc[15]));
    return m > __float_as_int(thr);
  } else if (TEST == 2) {
    int g[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) g[j] = max(max(__float_as_int(acc[3 * j]), __float_as_int(acc[3 * j + 1])), __float_as_int(acc[3 * j + 2]));
    const int u = max(max(g[0], g[1]), g[2]), v = max(max(g[3], g[4]), __float_as_int(acc[15]));
    return max(u, v) > __float_as_int(thr);
  } else {
    int m = max(max(__float_as_int(acc[0]), __float_as_int(acc[1])), __float_as_int(acc[2]));
#pragma unroll
    for (int i = 3; i < 7; i += 2) m = max(max(m, __float_as_int(acc[i])), __float_as_int(acc[i + 1]));
    m = max(m, __float_as_int(acc[7]));
    return m > __float_as_int(thr);
  }
}

template <int NM, int TEST, int XV>
__global__ __launch_bounds__(256, 2) void k(float* out, int seed, float thr, unsigned* sink) {
  i32x8 a[4], b[4];
#pragma unroll
  for (int s = 0; s < 4; ++s)
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      a[s][i] = i < 4 ? (int)((mix(threadIdx.x * 131u + s * 17u + i + seed) & 0x88888888u) | 0x22222222u) : 0;
      b[s][i] = i < 4 ? (int)((mix(threadIdx.x * 977u + s * 29u + i * 7u + blockIdx.x) & 0x88888888u) | 0x22222222u) : 0;
    }
  f32x16 acc_e, acc_o;
#pragma unroll
  for (int i = 0; i < 16; ++i) { acc_e[i] = -4096.f; acc_o[i] = -4096.f; }
  unsigned x = mix(threadIdx.x + seed), hits = 0;
  const unsigned sign = 0x88888888u, one = 0x22222222u;
  for (int it = 0; it < kIters; ++it) {
    if (NM) acc_e = block<NM ? NM : 1>(a, b);
    if (XV) {                                             // 4 independent shift + and_or pairs: one word's fp4 expansion
      a[0][0] = (int)(((x << 3) & sign) | one); a[0][1] = (int)(((x << 2) & sign) | one);
      a[0][2] = (int)(((x << 1) & sign) | one); a[0][3] = (int)((x & sign) | one);
      x += 0x9e3779b9u;
    }
    if (TEST) { if (__builtin_amdgcn_ballot_w64(test<TEST ? TEST : 1>(acc_o, thr)) != 0ull) { ++hits; thr += 1.f; asm volatile("global_store_dword %0, %1, off" :: "v"(sink + (threadIdx.x & 63u)), "v"(hits) : "memory"); } }
    if (NM) acc_o = block<NM ? NM : 1>(a, b);
    if (XV) {
      b[0][0] = (int)(((x << 3) & sign) | one); b[0][1] = (int)(((x << 2) & sign) | one);
      b[0][2] = (int)(((x << 1) & sign) | one); b[0][3] = (int)((x & sign) | one);
      x += 0x9e3779b9u;
    }
    if (TEST) { if (__builtin_amdgcn_ballot_w64(test<TEST ? TEST : 1>(acc_e, thr)) != 0ull) { ++hits; thr += 1.f; asm volatile("global_store_dword %0, %1, off" :: "v"(sink + (threadIdx.x & 63u)), "v"(hits) : "memory"); } }
    if (!NM) {                                            // keep the tested registers moving without the matrix pipe
#pragma unroll
      for (int i = 0; i < 16; i += 8) { acc_e[i] = __int_as_float(__float_as_int(acc_e[i]) ^ (int)(x & 1u)); acc_o[i] = __int_as_float(__float_as_int(acc_o[i]) ^ (int)(x & 1u)); }
    }
  }
  float r = 0.f;
  for (int i = 0; i < 16; ++i) r += acc_e[i] + acc_o[i];
  out[blockIdx.x * 256 + threadIdx.x] = r + (float)a[0][0] + (float)b[1][2];
  if (hits) atomicAdd(sink, hits);
}

// the same 1024 pairs x 128 bit positions as four 16 x 16 x 128 tiles: one MFMA each, no accumulator input, 4 result registers
typedef __attribute__((ext_vector_type(4))) float f32x4;
template <int XV>
__global__ __launch_bounds__(256, 2) void k16(float* out, int seed, float thr, unsigned* sink) {
  i32x8 a[4], b[4];
#pragma unroll
  for (int s = 0; s < 4; ++s)
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      a[s][i] = i < 4 ? (int)((mix(threadIdx.x * 131u + s * 17u + i + seed) & 0x88888888u) | 0x22222222u) : 0;
      b[s][i] = i < 4 ? (int)((mix(threadIdx.x * 977u + s * 29u + i * 7u + blockIdx.x) & 0x88888888u) | 0x22222222u) : 0;
    }
  f32x4 e[4], o[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) for (int i = 0; i < 4; ++i) { e[j][i] = -4096.f; o[j][i] = -4096.f; }
  unsigned x = mix(threadIdx.x + seed), hits = 0;
  const unsigned sign = 0x88888888u, one = 0x22222222u;
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  auto test16 = [&](const f32x4 (&v)[4]) {
    int m = max(max(__float_as_int(v[0][0]), __float_as_int(v[0][1])), __float_as_int(v[0][2]));
    m = max(max(m, __float_as_int(v[0][3])), __float_as_int(v[1][0]));
    m = max(max(m, __float_as_int(v[1][1])), __float_as_int(v[1][2]));
    m = max(max(m, __float_as_int(v[1][3])), __float_as_int(v[2][0]));
    m = max(max(m, __float_as_int(v[2][1])), __float_as_int(v[2][2]));
    m = max(max(m, __float_as_int(v[2][3])), __float_as_int(v[3][0]));
    m = max(max(m, __float_as_int(v[3][1])), __float_as_int(v[3][2]));
    m = max(m, __float_as_int(v[3][3]));
    return m > __float_as_int(thr);
  };
  for (int it = 0; it < kIters; ++it) {
#pragma unroll
    for (int j = 0; j < 4; ++j) e[j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a[j], b[j], z, 4, 4, 0, 0, 0, 0);
    if (XV) {
      a[0][0] = (int)(((x << 3) & sign) | one); a[0][1] = (int)(((x << 2) & sign) | one);
      a[0][2] = (int)(((x << 1) & sign) | one); a[0][3] = (int)((x & sign) | one);
      x += 0x9e3779b9u;
    }
    if (__builtin_amdgcn_ballot_w64(test16(o)) != 0ull) { ++hits; thr += 1.f; asm volatile("global_store_dword %0, %1, off" :: "v"(sink + (threadIdx.x & 63u)), "v"(hits) : "memory"); }
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a[j], b[j], z, 4, 4, 0, 0, 0, 0);
    if (XV) {
      b[0][0] = (int)(((x << 3) & sign) | one); b[0][1] = (int)(((x << 2) & sign) | one);
      b[0][2] = (int)(((x << 1) & sign) | one); b[0][3] = (int)((x & sign) | one);
      x += 0x9e3779b9u;
    }
    if (__builtin_amdgcn_ballot_w64(test16(e)) != 0ull) { ++hits; thr += 1.f; asm volatile("global_store_dword %0, %1, off" :: "v"(sink + (threadIdx.x & 63u)), "v"(hits) : "memory"); }
  }
  float r = 0.f;
  for (int j = 0; j < 4; ++j) for (int i = 0; i < 4; ++i) r += e[j][i] + o[j][i];
  out[blockIdx.x * 256 + threadIdx.x] = r + (float)a[0][0] + (float)b[1][2];
  if (hits) atomicAdd(sink, hits);
}

template <int XV>
void run16(const char* what, int n_cu, float* d_out, unsigned* d_sink) {
  const int grid = n_cu * 2;
  hipEvent_t e0, e1; (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
  hipLaunchKernelGGL((k16<XV>), dim3(grid), dim3(256), 0, 0, d_out, 1, 1e30f, d_sink);
  hipDeviceSynchronize();
  float best = 1e30f;
  for (int r = 0; r < 6; ++r) {
    hipEventRecord(e0, 0);
    hipLaunchKernelGGL((k16<XV>), dim3(grid), dim3(256), 0, 0, d_out, r + 2, 1e30f, d_sink);
    hipEventRecord(e1, 0); hipEventSynchronize(e1);
    float ms; hipEventElapsedTime(&ms, e0, e1); if (ms < best) best = ms;
  }
  const double ns = best * 1e6 / (2.0 * kIters * 2.0);
  printf("%-58s %.3f ms  %6.1f ns per block per SIMD (%5.1f cycles @2.1 GHz)\n", what, best, ns, ns * 2.1);
}

template <int NM, int TEST, int XV>
double run(const char* what, int n_cu, float* d_out, unsigned* d_sink) {
  const int grid = n_cu * 2;
  hipEvent_t e0, e1; (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
  hipLaunchKernelGGL((k<NM, TEST, XV>), dim3(grid), dim3(256), 0, 0, d_out, 1, 1e30f, d_sink);
  hipDeviceSynchronize();
  float best = 1e30f;
  for (int r = 0; r < 6; ++r) {
    hipEventRecord(e0, 0);
    hipLaunchKernelGGL((k<NM, TEST, XV>), dim3(grid), dim3(256), 0, 0, d_out, r + 2, 1e30f, d_sink);
    hipEventRecord(e1, 0); hipEventSynchronize(e1);
    float ms; hipEventElapsedTime(&ms, e0, e1); if (ms < best) best = ms;
  }
  const double blocks_per_simd = 2.0 * kIters * 2.0;       // two waves per SIMD, two blocks per trip
  const double ns = best * 1e6 / blocks_per_simd;
  printf("%-58s %.3f ms  %6.1f ns per block per SIMD (%5.1f cycles @2.1 GHz)\n", what, best, ns, ns * 2.1);
  return ns;
}

// ---- The fast path of hamming_topk_fp4rows<2, 6, 2> (tod_amd/csrc/match_fp4rows.h), one ingredient at a time on the "2 MFMAs + tree
// test" loop above. kp<0,0,0,0> is that loop in the product's shape: six query blocks per 32-row step, two steps per trip, the step's
// last test carried into the next step's block 0, a tiny slow path that counts itself. The ingredients:
//   LOADS  the rows come from a 128 MB fp4 copy, four 1 KB buffer loads per step addressed as Fp4StepLoader does (lane offset in the
//          vector operand, step offset scalar, clamped to the tile's last step), two in front of block 0's test and two behind it; the
//          first two feed the next step's MFMAs, the other two only the slow path, as in the product
//   FLAG   every block's 0/1 "went on" flag, summed per trip (the product's n_pass); without it the slow path bumps a counter itself
//   BIG    the slow path inline behind each test at the product's size: two more MFMAs, a second tree test, the 16-row walk into a
//          2-entry list, the threshold update -- never executed (thr = 1e30), so the fast path is the taken side of a far branch
//   TAIL   the per-trip remainder: the lane's row base and the share-period test with its (never taken) exchange of bounds
//   COLD   the slow path marked unlikely: hipcc lays it out behind the loop and the fast path falls through (what the product does now)
// The clock climbs over the first launches of a process and differs between these loops (1.9 - 2.3 GHz seen): a warm-up runs first, and
// tools/match_fastpath.sh clock gives every line in cycles as well. Compare variants in cycles.
// 16 tiles of 2048 steps; the 128 waves of 32 workgroups with equal blockIdx.x % 8 read one tile together (the product: 167 query waves).
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
constexpr int kQT = 6, kTileSteps = 2048, kTiles = 16;
struct Row { i32x8 s[4]; };

__device__ __forceinline__ i32x8 frag(__amdgpu_buffer_rsrc_t rs, unsigned lane_off, unsigned step_off, int m) {
  const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)(lane_off + m * 1024u), (int)step_off, 0);
  return i32x8{(int)v.x, (int)v.y, (int)v.z, (int)v.w, 0, 0, 0, 0};
}

template <bool FLAG, bool BIG, bool COLD>
__device__ __forceinline__ bool part_test(f32x16& acc, const Row& rows, const Row& q, float& thr, float& thrp, unsigned r_lane,
                                          unsigned (&best)[2], unsigned& hits, unsigned* sink) {
  const bool none = __builtin_amdgcn_ballot_w64(test<2>(acc, thrp)) == 0ull;
  if (COLD ? __builtin_expect(none, 1) : none) return false;
  if (!FLAG) ++hits;
  if (!BIG) {
    thrp += 1.f;
    asm volatile("global_store_dword %0, %1, off" :: "v"(sink + (threadIdx.x & 63u)), "v"(thrp) : "memory");
    return true;
  }
#pragma unroll
  for (int s = 2; s < 4; ++s) acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(rows.s[s], q.s[s], acc, 4, 4, 0, 0, 0, 0);
  if (__builtin_amdgcn_ballot_w64(test<2>(acc, thr)) != 0ull) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const bool hit = acc[i] > thr;
      if (__builtin_amdgcn_ballot_w64(hit) != 0ull) {
        const unsigned key = hit ? ((unsigned)((256.f - acc[i]) * 2097152.f) | r_lane | (unsigned)((i & 3) + 8 * (i >> 2))) : 0xFFFFFFFFu;
        const unsigned lo = min(best[0], key), hi = max(best[0], key);
        best[0] = lo; best[1] = min(best[1], hi);
      }
    }
    thr = fmaxf(thr, 256.f - 2.f * (float)(best[1] >> 22));
  }
  thrp = thr - 128.f;
  return true;
}

template <bool LOADS, bool FLAG, bool BIG, bool COLD>
__device__ __forceinline__ unsigned pstep(const Row& a, Row& a_next, __amdgpu_buffer_rsrc_t rs, unsigned lane_off, unsigned step_off,
                                          const Row (&qb)[kQT], float (&thr)[kQT], float (&thrp)[kQT], unsigned (&best)[kQT][2],
                                          f32x16& acc_e, f32x16& acc_o, unsigned r_lane, unsigned& hits, unsigned* sink) {
  unsigned n_pass = 0;
#pragma unroll
  for (int t = 0; t < kQT; ++t) {
    if (t & 1) acc_o = block<2>(a.s, qb[t].s); else acc_e = block<2>(a.s, qb[t].s);
    if (LOADS && t == 0) { a_next.s[0] = frag(rs, lane_off, step_off, 0); a_next.s[1] = frag(rs, lane_off, step_off, 1); }
    if (LOADS && t == 1) { a_next.s[2] = frag(rs, lane_off, step_off, 2); a_next.s[3] = frag(rs, lane_off, step_off, 3); }
    bool went_on;
    if (t == 0) went_on = part_test<FLAG, BIG, COLD>(acc_o, a_next, qb[kQT - 1], thr[kQT - 1], thrp[kQT - 1], r_lane - 32u, best[kQT - 1], hits, sink);
    else went_on = part_test<FLAG, BIG, COLD>((t & 1) ? acc_e : acc_o, a, qb[t - 1], thr[t - 1], thrp[t - 1], r_lane, best[t - 1], hits, sink);
    if (FLAG) n_pass += went_on ? 1u : 0u;
  }
  return n_pass;
}

__global__ void fill_fp4(unsigned* p, size_t n_words) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n_words; i += (size_t)gridDim.x * blockDim.x)
    p[i] = (mix((unsigned)i * 2654435761u + (unsigned)(i >> 32)) & 0x88888888u) | 0x22222222u;
}

template <bool LOADS, bool FLAG, bool BIG, bool TAIL, bool COLD = false>
__global__ __launch_bounds__(256, 2) void kp(const u32x4* rows_fp4, unsigned copy_bytes, unsigned n_steps, unsigned share_period,
                                             float* out, int seed, float thr0, unsigned* sink) {
  const unsigned lane = threadIdx.x & 63u, h = lane >> 5;
  const unsigned tile = __builtin_amdgcn_readfirstlane(((blockIdx.x & 7u) * 2u + ((blockIdx.x >> 3) & 1u)) % kTiles);
  const unsigned step0 = tile * kTileSteps;
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<u32x4*>(rows_fp4), 0, (int)copy_bytes, 0x00020000);
  const unsigned lane_off = lane * 16u;
  Row qb[kQT];
  unsigned best[kQT][2];
  float thr[kQT], thrp[kQT];
#pragma unroll
  for (int t = 0; t < kQT; ++t) {
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int i = 0; i < 8; ++i) qb[t].s[s][i] = i < 4 ? (int)((mix(threadIdx.x * 977u + t * 61u + s * 29u + i * 7u + blockIdx.x) & 0x88888888u) | 0x22222222u) : 0;
    best[t][0] = best[t][1] = 0xFFFFFFFFu;
    thr[t] = thr0; thrp[t] = thr0 - 128.f;
  }
  Row a0, a1;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    if (LOADS) a0.s[s] = frag(rs, lane_off, step0 * 4096u, s);
    else
#pragma unroll
      for (int i = 0; i < 8; ++i) a0.s[s][i] = i < 4 ? (int)((mix(threadIdx.x * 131u + s * 17u + i + seed) & 0x88888888u) | 0x22222222u) : 0;
  }
  a1 = a0;
  f32x16 acc_e, acc_o;
#pragma unroll
  for (int i = 0; i < 16; ++i) { acc_e[i] = -4096.f; acc_o[i] = -4096.f; }
  unsigned hits = 0, n_pass = 0, next_share = 2u, seen = 0xFFFFFFFFu;
  auto off = [&](unsigned step) { return (step0 + min(step, n_steps - 1u)) * 4096u; };   // wave-uniform
  for (unsigned step = 0; step + 2u <= n_steps; step += 2u) {
    n_pass += pstep<LOADS, FLAG, BIG, COLD>(a0, a1, rs, lane_off, off(step + 1u), qb, thr, thrp, best, acc_e, acc_o, 32u * step + 4u * h, hits, sink);
    n_pass += pstep<LOADS, FLAG, BIG, COLD>(a1, a0, rs, lane_off, off(step + 2u), qb, thr, thrp, best, acc_e, acc_o, 32u * step + 4u * h + 32u, hits, sink);
    if (TAIL && step + 2u >= next_share) {
      next_share += share_period;
#pragma unroll
      for (int t = 0; t < kQT; ++t)
        if (seen != 0xFFFFFFFFu) { thr[t] = fmaxf(thr[t], 256.f - 2.f * (float)(seen + 1u)); thrp[t] = thr[t] - 128.f; }
      seen = __hip_atomic_load(sink + 2 + (lane & 31u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  float r = 0.f;
  for (int i = 0; i < 16; ++i) r += acc_e[i] + acc_o[i];
  for (int t = 0; t < kQT; ++t) r += thr[t] + thrp[t] + (float)(best[t][0] ^ best[t][1]);
  out[blockIdx.x * 256 + threadIdx.x] = r + (float)a0.s[0][0] + (float)a1.s[2][1] + (float)seen;
  if (lane == 0 && n_pass) atomicAdd(sink, n_pass);
  if (lane == 0 && hits) atomicAdd(sink + 1, hits);
}

template <bool LOADS, bool FLAG, bool BIG, bool TAIL, bool COLD = false>
double runp(const char* what, int n_cu, const u32x4* d_rows, float* d_out, unsigned* d_sink) {
  const int grid = n_cu * 2;
  const unsigned bytes = (unsigned)kTiles * kTileSteps * 4096u;
  hipEvent_t e0, e1; (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
  hipLaunchKernelGGL((kp<LOADS, FLAG, BIG, TAIL, COLD>), dim3(grid), dim3(256), 0, 0, d_rows, bytes, (unsigned)kTileSteps, 16u, d_out, 1, 1e30f, d_sink);
  hipDeviceSynchronize();
  float best = 1e30f;
  for (int r = 0; r < 6; ++r) {
    hipEventRecord(e0, 0);
    hipLaunchKernelGGL((kp<LOADS, FLAG, BIG, TAIL, COLD>), dim3(grid), dim3(256), 0, 0, d_rows, bytes, (unsigned)kTileSteps, 16u, d_out, r + 2, 1e30f, d_sink);
    hipEventRecord(e1, 0); hipEventSynchronize(e1);
    float ms; hipEventElapsedTime(&ms, e0, e1); if (ms < best) best = ms;
  }
  const double blocks_per_simd = 2.0 * kTileSteps * kQT;   // two waves per SIMD
  const double ns = best * 1e6 / blocks_per_simd;
  printf("%-58s %.3f ms  %6.1f ns per block per SIMD (%5.1f cycles @2.1 GHz)\n", what, best, ns, ns * 2.1);
  return ns;
}

// ---- Two split blocks per accumulator (profiles/match_pairs.json). The first two MFMAs of a block give even integers in [-128, 128];
// an f32 accumulator holds two of them as fixed-point fields when the second block's MFMAs run with an E8M0 scale of 2^11 on the rows
// and the first MFMA's srcC is M = 1.5 * 2^23 + (512 - t) * 2049, t = thrp + 1: acc = M + dA + 2048 dB is an integer in [2^23, 2^24),
// so its mantissa bits ARE that integer, field A = dA - t + 512 in [257, 639] at bit 0 and field B the same at bit 11; bit 9 is set
// exactly when dA > thrp and bit 20 exactly when dB > thrp. "Does any pair of either block reach the threshold" is then an OR over
// the 16 registers and one mask for two blocks. kq<PV> is the loop of hamming_topk_fp4rows<2, 6, 2> as it stands now -- fragments 0-1
// of the rows from the 128 MB copy, the tails on demand in a cold slow path, the step's last test carried -- with
//   PV 0  (p0) today's block: 2 MFMAs into a zero accumulator, the tree of 8 v_max3 against the block's own threshold
//   PV 1  (p1) a pair: 4 MFMAs in the scaled form (scales 2^0 and 2^11), two accumulators, the test behind the next pair's MFMAs
//   PV 2  (p2) the same with the first block's two MFMAs in the unscaled form (scale arguments constant 0)
//   PV 3, 4  (p3) p1 and p2 with three accumulators: the test trails by a pair and a half (behind the first block of the next but one)
// The slow path of a pair is the crude one: each block that goes on is recomputed whole from the copy. It never runs here (cut = 1 on
// random bits), so only what it does to the fast path's registers and layout is priced. pair_exact checks the packing on the device.
constexpr int kFieldBits = PairPack::kFieldBits;                               // (the one definition: tod_amd/csrc/match_pair_pack.h)
constexpr unsigned kFlagA = PairPack::kFlagA, kFlagB = PairPack::kFlagB, kFlagMask = PairPack::kFlagMask;
constexpr int kScaleOne = PairPack::kScaleOne, kScaleField = PairPack::kScaleField;   // E8M0: 2^0 and 2^11
inline __host__ __device__ float pair_magic(unsigned cut) { return PairPack::magic(cut); }
struct Frag2 { i32x8 s[2]; };

template <bool SCALED_A>
__device__ __forceinline__ void pair_first(f32x16& acc, const f32x16& magic, const Frag2& a, const Frag2& q, int s_one) {
  if (SCALED_A) {
    acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a.s[0], q.s[0], magic, 4, 4, 0, s_one, 0, s_one);
    acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a.s[1], q.s[1], acc, 4, 4, 0, s_one, 0, s_one);
  } else {
    acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a.s[0], q.s[0], magic, 4, 4, 0, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a.s[1], q.s[1], acc, 4, 4, 0, 0, 0, 0);
  }
}
__device__ __forceinline__ void pair_second(f32x16& acc, const Frag2& a, const Frag2& q, int s_one, int s_field) {
  acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a.s[0], q.s[0], acc, 4, 4, 0, s_field, 0, s_one);
  acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a.s[1], q.s[1], acc, 4, 4, 0, s_field, 0, s_one);
}
__device__ __forceinline__ unsigned pair_or(const f32x16& acc) {
  unsigned g[5];
#pragma unroll
  for (int j = 0; j < 5; ++j) g[j] = (unsigned)__float_as_int(acc[3 * j]) | (unsigned)__float_as_int(acc[3 * j + 1]) | (unsigned)__float_as_int(acc[3 * j + 2]);
#pragma unroll
  for (int j = 0; j < 5; ++j) asm("" : "+v"(g[j]));      // a tree, as the maximum is: hipcc reassociates the ORs into one chain of seven
  return (g[0] | g[1] | g[2]) | (g[3] | g[4] | (unsigned)__float_as_int(acc[15]));
}

// one whole block from the copy, against its own threshold: the completion of a block that went on (cold)
__device__ __forceinline__ void whole_block(__amdgpu_buffer_rsrc_t rs, unsigned lane_off, unsigned step_off, const u32x4* qsrc, unsigned qi,
                                         float& thr, unsigned r_lane, unsigned (&best)[2]) {
  const unsigned sign = 0x88888888u, one = 0x22222222u;
  const u32x4 p = qsrc[qi];
  f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const unsigned x = p[s];
    const i32x8 qe = {(int)(((x << 3) & sign) | one), (int)(((x << 2) & sign) | one), (int)(((x << 1) & sign) | one), (int)((x & sign) | one), 0, 0, 0, 0};
    acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(frag(rs, lane_off, step_off, s), qe, acc, 4, 4, 0, 0, 0, 0);
  }
  if (__builtin_amdgcn_ballot_w64(test<2>(acc, thr)) != 0ull) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const bool hit = acc[i] > thr;
      if (__builtin_amdgcn_ballot_w64(hit) != 0ull) {
        const unsigned key = hit ? ((unsigned)((256.f - acc[i]) * 2097152.f) | r_lane | (unsigned)((i & 3) + 8 * (i >> 2))) : 0xFFFFFFFFu;
        const unsigned lo = min(best[0], key), hi = max(best[0], key);
        best[0] = lo; best[1] = min(best[1], hi);
      }
    }
    thr = fmaxf(thr, 256.f - 2.f * (float)(best[1] >> 22));
  }
}

// today's block test, tails on demand
__device__ __forceinline__ void q_block_test(f32x16& acc, __amdgpu_buffer_rsrc_t rs, unsigned lane_off, unsigned step_off, const u32x4* qsrc,
                                             unsigned qi, float& thr, float& thrp, unsigned r_lane, unsigned (&best)[2], unsigned& hits) {
  if (__builtin_expect(__builtin_amdgcn_ballot_w64(test<2>(acc, thrp)) == 0ull, 1)) return;
  ++hits;
  asm volatile("" : "+v"(qi));
  whole_block(rs, lane_off, step_off, qsrc, qi, thr, r_lane, best);
  asm("" : "+v"(thr));
  thrp = thr - 128.f;
}
// the pair's test: blocks ta and ta + 1 of one step
__device__ __forceinline__ void q_pair_test(const f32x16& acc, __amdgpu_buffer_rsrc_t rs, unsigned lane_off, unsigned step_off, const u32x4* qsrc,
                                            unsigned qi, float& thr_a, float& thr_b, unsigned r_lane, unsigned (&best_a)[2], unsigned (&best_b)[2],
                                            unsigned& hits) {
  const unsigned o = pair_or(acc);
  if (__builtin_expect(__builtin_amdgcn_ballot_w64((o & kFlagMask) != 0u) == 0ull, 1)) return;
  asm volatile("" : "+v"(qi));
  if (__builtin_amdgcn_ballot_w64((o & kFlagA) != 0u) != 0ull) { ++hits; whole_block(rs, lane_off, step_off, qsrc, qi, thr_a, r_lane, best_a); asm("" : "+v"(thr_a)); }
  if (__builtin_amdgcn_ballot_w64((o & kFlagB) != 0u) != 0ull) { ++hits; whole_block(rs, lane_off, step_off, qsrc, qi + 32u, thr_b, r_lane, best_b); asm("" : "+v"(thr_b)); }
}

// PH: the step's place in the trip (two accumulators and three pairs per step: the pending pair's accumulator alternates per step)
template <int PV, int PH>
__device__ __forceinline__ void qstep(const Frag2& a, Frag2& a_next, __amdgpu_buffer_rsrc_t rs, unsigned lane_off, unsigned prev_off, unsigned own_off,
                                      unsigned next_off, const Frag2 (&qh)[kQT], const u32x4* qsrc, unsigned q0c, float (&thr)[kQT], float (&thrp)[kQT],
                                      unsigned (&best)[kQT][2], f32x16 (&acc)[3], const f32x16& magic, int s_one, int s_field, unsigned r_lane, unsigned& hits) {
  if (PV == 0) {
#pragma unroll
    for (int t = 0; t < kQT; ++t) {
      acc[t & 1] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a.s[0], qh[t].s[0], f32x16{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, 4, 4, 0, 0, 0, 0);
      acc[t & 1] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a.s[1], qh[t].s[1], acc[t & 1], 4, 4, 0, 0, 0, 0);
      if (t == 0) { a_next.s[0] = frag(rs, lane_off, next_off, 0); a_next.s[1] = frag(rs, lane_off, next_off, 1); }
      if (t == 0) q_block_test(acc[1], rs, lane_off, prev_off, qsrc, q0c + 32u * (kQT - 1), thr[kQT - 1], thrp[kQT - 1], r_lane - 32u, best[kQT - 1], hits);
      else q_block_test(acc[(t & 1) ^ 1], rs, lane_off, own_off, qsrc, q0c + 32u * (t - 1), thr[t - 1], thrp[t - 1], r_lane, best[t - 1], hits);
    }
    return;
  }
  constexpr bool SCALED_A = PV == 1 || PV == 3, THREE = PV >= 3;
  constexpr int NP = kQT / 2;
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    f32x16& cur = THREE ? acc[j] : acc[(NP * PH + j) & 1];
    pair_first<SCALED_A>(cur, magic, a, qh[2 * j], s_one);
    if (THREE) {                                       // the pair two back: j + 1 of the step before, or pair 0 of this one
      asm volatile("" : "+v"(cur));
      const int u = (j + 1) % NP;
      q_pair_test(acc[u], rs, lane_off, j < 2 ? prev_off : own_off, qsrc, q0c + 64u * u, thr[2 * u], thr[2 * u + 1], j < 2 ? r_lane - 32u : r_lane,
                  best[2 * u], best[2 * u + 1], hits);
    }
    pair_second(cur, a, qh[2 * j + 1], s_one, s_field);
    if (j == 0) { a_next.s[0] = frag(rs, lane_off, next_off, 0); a_next.s[1] = frag(rs, lane_off, next_off, 1); }
    asm volatile("" : "+v"(cur));                      // the MFMAs stay HERE: hipcc otherwise sinks them behind the test in front of their own
    if (!THREE) {                                      // the pair before: the last of the step before, or j - 1 of this one
      const int u = (j + NP - 1) % NP;
      q_pair_test(acc[(NP * PH + j + 1) & 1], rs, lane_off, j == 0 ? prev_off : own_off, qsrc, q0c + 64u * u, thr[2 * u], thr[2 * u + 1],
                  j == 0 ? r_lane - 32u : r_lane, best[2 * u], best[2 * u + 1], hits);
    }
  }
}

template <int PV>
__global__ __launch_bounds__(256, 2) void kq(const u32x4* rows_fp4, unsigned copy_bytes, unsigned n_steps, unsigned share_period,
                                             float* out, int seed, unsigned cut, int s_one, int s_field, unsigned* sink) {
  const unsigned lane = threadIdx.x & 63u, h = lane >> 5;
  const unsigned tile = __builtin_amdgcn_readfirstlane(((blockIdx.x & 7u) * 2u + ((blockIdx.x >> 3) & 1u)) % kTiles);
  const unsigned step0 = tile * kTileSteps;
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<u32x4*>(rows_fp4), 0, (int)copy_bytes, 0x00020000);
  const unsigned lane_off = lane * 16u, q0c = (blockIdx.x * 4u + (threadIdx.x >> 6)) * (32u * kQT) % 4096u + (lane & 31u) + 64u * h;
  Frag2 qh[kQT];
  unsigned best[kQT][2];
  float thr[kQT], thrp[kQT];
#pragma unroll
  for (int t = 0; t < kQT; ++t) {
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int i = 0; i < 8; ++i) qh[t].s[s][i] = i < 4 ? (int)((mix(threadIdx.x * 977u + t * 61u + s * 29u + i * 7u + blockIdx.x + seed) & 0x88888888u) | 0x22222222u) : 0;
    best[t][0] = best[t][1] = 0xFFFFFFFFu;
    thr[t] = 256.f - 2.f * (float)cut; thrp[t] = thr[t] - 128.f;
  }
  Frag2 a0, a1;
#pragma unroll
  for (int s = 0; s < 2; ++s) a0.s[s] = frag(rs, lane_off, step0 * 4096u, s);
  a1 = a0;
  // the scales live in vector registers for the whole loop: from scalar registers hipcc copies both in front of every pair
  asm volatile("v_mov_b32 %0, %1" : "=v"(s_one) : "s"(s_one));
  asm volatile("v_mov_b32 %0, %1" : "=v"(s_field) : "s"(s_field));
  f32x16 acc[3], magic;
  const float m = PV ? pair_magic(cut) : -4096.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) { magic[i] = m; acc[0][i] = m; acc[1][i] = m; acc[2][i] = m; }
  unsigned hits = 0, next_share = 2u, seen = 0xFFFFFFFFu;
  auto off = [&](unsigned step) { return (step0 + min(step, n_steps - 1u)) * 4096u; };   // wave-uniform
  for (unsigned step = 0; step + 2u <= n_steps; step += 2u) {
    qstep<PV, 0>(a0, a1, rs, lane_off, off(step - 1u), off(step), off(step + 1u), qh, rows_fp4, q0c, thr, thrp, best, acc, magic, s_one, s_field, 32u * step + 4u * h, hits);
    qstep<PV, 1>(a1, a0, rs, lane_off, off(step), off(step + 1u), off(step + 2u), qh, rows_fp4, q0c, thr, thrp, best, acc, magic, s_one, s_field, 32u * step + 4u * h + 32u, hits);
    if (step + 2u >= next_share) {
      next_share += share_period;
#pragma unroll
      for (int t = 0; t < kQT; ++t)
        if (seen != 0xFFFFFFFFu) { thr[t] = fmaxf(thr[t], 256.f - 2.f * (float)(seen + 1u)); thrp[t] = thr[t] - 128.f; }
      seen = __hip_atomic_load(sink + 2 + (lane & 31u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  float r = 0.f;
  for (int i = 0; i < 16; ++i) r += acc[0][i] + acc[1][i] + acc[2][i];
  for (int t = 0; t < kQT; ++t) r += thr[t] + thrp[t] + (float)(best[t][0] ^ best[t][1]);
  out[blockIdx.x * 256 + threadIdx.x] = r + (float)a0.s[0][0] + (float)a1.s[1][1] + (float)seen;
  if (lane == 0 && hits) atomicAdd(sink + 1, hits);
}

template <int PV>
double runq(const char* what, int n_cu, const u32x4* d_rows, float* d_out, unsigned* d_sink) {
  const int grid = n_cu * 2;
  const unsigned bytes = (unsigned)kTiles * kTileSteps * 4096u;
  hipEvent_t e0, e1; (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
  hipLaunchKernelGGL((kq<PV>), dim3(grid), dim3(256), 0, 0, d_rows, bytes, (unsigned)kTileSteps, 16u, d_out, 1, 1u, kScaleOne, kScaleField, d_sink);
  hipDeviceSynchronize();
  float best = 1e30f;
  for (int r = 0; r < 6; ++r) {
    hipEventRecord(e0, 0);
    hipLaunchKernelGGL((kq<PV>), dim3(grid), dim3(256), 0, 0, d_rows, bytes, (unsigned)kTileSteps, 16u, d_out, r + 2, 1u, kScaleOne, kScaleField, d_sink);
    hipEventRecord(e1, 0); hipEventSynchronize(e1);
    float ms; hipEventElapsedTime(&ms, e0, e1); if (ms < best) best = ms;
  }
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  const double ns = best * 1e6 / (2.0 * kTileSteps * kQT);   // two waves per SIMD
  printf("%-58s %.3f ms  %6.1f ns per block per SIMD (%5.1f cycles @2.1 GHz)\n", what, best, ns, ns * 2.1);
  return ns;
}

// The packing on the device, one wave: 32 rows (fa, fragments 0-1 as the lanes hold them) against the 32 queries of block t (fqa) and of
// block t + 1 (fqb); every lane's 16 packed accumulators go out as they are.
template <bool SCALED_A>
__global__ void pair_exact(const u32x4* fa, const u32x4* fqa, const u32x4* fqb, unsigned cut, int s_one, int s_field, unsigned* out) {
  const unsigned lane = threadIdx.x;
  Frag2 a, qa, qb;
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const u32x4 x = fa[s * 64 + lane], y = fqa[s * 64 + lane], z = fqb[s * 64 + lane];
    a.s[s] = i32x8{(int)x.x, (int)x.y, (int)x.z, (int)x.w, 0, 0, 0, 0};
    qa.s[s] = i32x8{(int)y.x, (int)y.y, (int)y.z, (int)y.w, 0, 0, 0, 0};
    qb.s[s] = i32x8{(int)z.x, (int)z.y, (int)z.z, (int)z.w, 0, 0, 0, 0};
  }
  f32x16 magic, acc;
  const float m = pair_magic(cut);
#pragma unroll
  for (int i = 0; i < 16; ++i) magic[i] = m;
  pair_first<SCALED_A>(acc, magic, a, qa, s_one);
  pair_second(acc, a, qb, s_one, s_field);
#pragma unroll
  for (int i = 0; i < 16; ++i) out[lane * 16 + i] = (unsigned)__float_as_int(acc[i]);
}

// bits[r][p]: 128 bit positions of 32 rows / queries; position p = 64 h + 32 s + b sits in lane r + 32 h, fragment s, dword b & 3, nibble b >> 2
static void pack_frags(const unsigned char (*bits)[128], unsigned* frags /* [2][64][4] */) {
  for (int s = 0; s < 2; ++s) for (int l = 0; l < 64; ++l) for (int j = 0; j < 4; ++j) {
    unsigned w = 0x22222222u;
    for (int n = 0; n < 8; ++n) if (bits[l & 31][64 * (l >> 5) + 32 * s + 4 * n + j]) w |= 8u << (4 * n);
    frags[(s * 64 + l) * 4 + j] = w;
  }
}
// Returns the number of wrong accumulators over all cases, cuts and both forms
static long check_pairs_exact() {
  static unsigned char R[32][128], QA[32][128], QB[32][128];
  static unsigned h_f[3][2 * 64 * 4], h_out[64 * 16];
  unsigned *d_f[3], *d_out;
  for (int i = 0; i < 3; ++i) (void)hipMalloc(&d_f[i], sizeof(h_f[0]));
  (void)hipMalloc(&d_out, sizeof(h_out));
  const char* names[] = {"all equal", "all different", "A equal, B different", "A different, B equal", "random", "at the threshold"};
  long wrong = 0;
  const unsigned cuts[] = {1u, 36u, 64u};
  for (unsigned cut : cuts) {
    const int thrp = 128 - 2 * (int)cut;
    for (int c = 0; c < 6; ++c) {
      long at_a[2] = {0, 0}, at_b[2] = {0, 0};             // fields exactly at thrp and at thrp + 2
      for (int r = 0; r < 32; ++r) for (int p = 0; p < 128; ++p) {
        const unsigned char x = (unsigned char)(mix(1000u * cut + 128u * r + p) & 1u);
        if (c < 4) { R[r][p] = x; QA[r][p] = 0; QB[r][p] = 0; }
        else if (c == 4) { R[r][p] = x; QA[r][p] = (unsigned char)(mix(77777u + 128u * r + p) & 1u); QB[r][p] = (unsigned char)(mix(99999u + 128u * r + p) & 1u); }
        else {                                             // row r differs from X in its first cut - 2 + r % 5 positions (never below 0), query
          const unsigned char X = (unsigned char)(mix(5u + p) & 1u);   // c of block t in its last c & 1, of block t + 1 in its last c % 4
          const int fr = (int)cut - 2 + r % 5 < 0 ? 0 : (int)cut - 2 + r % 5;
          R[r][p] = (unsigned char)(X ^ (p < fr)); QA[r][p] = (unsigned char)(X ^ (p >= 128 - (r & 1))); QB[r][p] = (unsigned char)(X ^ (p >= 128 - r % 4));
        }
      }
      if (c < 4) for (int q = 0; q < 32; ++q) for (int p = 0; p < 128; ++p) {   // queries: row q's bits or their complement -- only the diagonal is
        const unsigned char x = (unsigned char)(mix(1000u * cut + 128u * q + p) & 1u);   // "all equal"; the other pairs are random
        QA[q][p] = (unsigned char)(x ^ (c == 1 || c == 3)); QB[q][p] = (unsigned char)(x ^ (c == 1 || c == 2));
      }
      pack_frags(R, h_f[0]); pack_frags(QA, h_f[1]); pack_frags(QB, h_f[2]);
      for (int i = 0; i < 3; ++i) (void)hipMemcpy(d_f[i], h_f[i], sizeof(h_f[0]), hipMemcpyHostToDevice);
      for (int form = 0; form < 2; ++form) {
        (void)hipMemset(d_out, 0, sizeof(h_out));
        if (form == 0) hipLaunchKernelGGL((pair_exact<true>), dim3(1), dim3(64), 0, 0, (const u32x4*)d_f[0], (const u32x4*)d_f[1], (const u32x4*)d_f[2], cut, kScaleOne, kScaleField, d_out);
        else hipLaunchKernelGGL((pair_exact<false>), dim3(1), dim3(64), 0, 0, (const u32x4*)d_f[0], (const u32x4*)d_f[1], (const u32x4*)d_f[2], cut, kScaleOne, kScaleField, d_out);
        if (hipMemcpy(h_out, d_out, sizeof(h_out), hipMemcpyDeviceToHost) != hipSuccess) { printf("pair_exact failed\n"); return -1; }
        long bad = 0;
        for (int l = 0; l < 64; ++l) for (int i = 0; i < 16; ++i) {
          const int row = (i & 3) + 8 * (i >> 2) + 4 * (l >> 5), col = l & 31;
          int dA = 0, dB = 0;
          for (int p = 0; p < 128; ++p) { dA += R[row][p] == QA[col][p] ? 1 : -1; dB += R[row][p] == QB[col][p] ? 1 : -1; }
          const long want = 12582912L + (512 - (thrp + 1)) * 2049L + dA + 2048L * dB;          // the integer, below 2^24
          const unsigned want_bits = 0x4B000000u + (unsigned)(want - 8388608L);                // f32 in [2^23, 2^24): mantissa = value - 2^23
          const unsigned got = h_out[l * 16 + i];
          const bool flags_ok = ((got & kFlagA) != 0u) == (dA > thrp) && ((got & kFlagB) != 0u) == (dB > thrp);
          if (got != want_bits || !flags_ok) { if (++bad <= 3) printf("  lane %d reg %d: dA %d dB %d want %08x got %08x\n", l, i, dA, dB, want_bits, got); }
          if (form == 0) { at_a[0] += dA == thrp; at_a[1] += dA == thrp + 2; at_b[0] += dB == thrp; at_b[1] += dB == thrp + 2; }
        }
        wrong += bad;
        printf("exact: cut %2u %-22s %s: %ld of 1024 wrong", cut, names[c], form == 0 ? "all scaled   " : "first unscaled", bad);
        if (form == 0) printf("   (dA = thrp %ld, thrp + 2 %ld; dB = thrp %ld, thrp + 2 %ld)", at_a[0], at_a[1], at_b[0], at_b[1]);
        printf("\n");
      }
    }
  }
  for (int i = 0; i < 3; ++i) (void)hipFree(d_f[i]);
  (void)hipFree(d_out);
  return wrong;
}

// `pairs`: the lines p0 .. p3 in alternating turns, then the exactness check -- nothing else
static int main_pairs(int n_cu, float* d_out, unsigned* d_sink, int turns) {
  const size_t bytes = (size_t)kTiles * kTileSteps * 4096u;
  u32x4* d_rows; if (hipMalloc(&d_rows, bytes) != hipSuccess) { printf("no memory for the fp4 copy\n"); return 1; }
  hipLaunchKernelGGL(fill_fp4, dim3(n_cu * 8), dim3(256), 0, 0, reinterpret_cast<unsigned*>(d_rows), bytes / 4);
  if (hipDeviceSynchronize() != hipSuccess) { printf("fill failed\n"); return 1; }
  for (int r = 0; r < 300; ++r)
    hipLaunchKernelGGL((kq<0>), dim3(n_cu * 2), dim3(256), 0, 0, d_rows, (unsigned)bytes, (unsigned)kTileSteps, 16u, d_out, 1, 1u, kScaleOne, kScaleField, d_sink);
  if (hipDeviceSynchronize() != hipSuccess) { printf("warm-up failed\n"); return 1; }
  for (int turn = 0; turn < turns; ++turn) {
    printf("turn %d\n", turn + 1);
    runq<0>("(p0) split-2 block, 8 max3 + compare per block", n_cu, d_rows, d_out, d_sink);
    runq<1>("(p1) pair, four scaled MFMAs, two accumulators", n_cu, d_rows, d_out, d_sink);
    runq<2>("(p2) pair, first block unscaled, two accumulators", n_cu, d_rows, d_out, d_sink);
    runq<3>("(p3) = (p1), three accumulators", n_cu, d_rows, d_out, d_sink);
    runq<4>("(p3) = (p2), three accumulators", n_cu, d_rows, d_out, d_sink);
  }
  unsigned h_sink[2] = {0, 0};
  (void)hipMemcpy(h_sink, d_sink, sizeof(h_sink), hipMemcpyDeviceToHost);
  printf("blocks that went on in all launches: %u (expected 0)\n", h_sink[1]);
  (void)hipFree(d_rows);
  const long wrong = check_pairs_exact();
  printf("exactness: %s (%ld wrong)\n", wrong == 0 ? "PASS" : "FAIL", wrong);
  return wrong == 0 ? 0 : 2;
}

int main(int argc, char** argv) {
  hipDeviceProp_t p; hipGetDeviceProperties(&p, 0);
  const int n_cu = p.multiProcessorCount;
  float* d_out; hipMalloc(&d_out, (size_t)n_cu * 2 * 256 * sizeof(float));
  unsigned* d_sink; (void)hipMalloc(&d_sink, 1024); (void)hipMemset(d_sink, 0, 1024);
  if (argc > 1 && argv[1][0] == 'p') return main_pairs(n_cu, d_out, d_sink, argc > 2 ? atoi(argv[2]) : 3);
  {
    const size_t bytes = (size_t)kTiles * kTileSteps * 4096u;
    u32x4* d_rows; if (hipMalloc(&d_rows, bytes) != hipSuccess) { printf("no memory for the fp4 copy\n"); return 1; }
    hipLaunchKernelGGL(fill_fp4, dim3(n_cu * 8), dim3(256), 0, 0, reinterpret_cast<unsigned*>(d_rows), bytes / 4);
    if (hipDeviceSynchronize() != hipSuccess) { printf("fill failed\n"); return 1; }
    for (int r = 0; r < 300; ++r)                              // warm-up: about 0.3 s of the full loop
      hipLaunchKernelGGL((kp<true, true, true, true>), dim3(n_cu * 2), dim3(256), 0, 0, d_rows, (unsigned)bytes, (unsigned)kTileSteps, 16u, d_out, 1, 1e30f, d_sink);
    if (hipDeviceSynchronize() != hipSuccess) { printf("warm-up failed\n"); return 1; }
    printf("the product's fast path (hamming_topk_fp4rows<2,6,2>), one ingredient at a time:\n");
    const double base = runp<false, false, false, false>("six blocks x two steps per trip, 2 MFMAs + tree test", n_cu, d_rows, d_out, d_sink);
    const double va = runp<true, false, false, false>("(a) + four fragment loads per step", n_cu, d_rows, d_out, d_sink);
    const double vb = runp<false, true, false, false>("(b) + per-block pass flag, summed per trip", n_cu, d_rows, d_out, d_sink);
    const double vc = runp<false, false, true, false>("(c) + large inline slow path (never executed)", n_cu, d_rows, d_out, d_sink);
    const double vt = runp<false, false, false, true>("    + row base and share-period test per trip", n_cu, d_rows, d_out, d_sink);
    const double vac = runp<true, false, true, true>("(d) without the pass flag: loads + slow path + tail", n_cu, d_rows, d_out, d_sink);
    const double vab = runp<true, true, false, true>("(d) with a small slow path: loads + flag + tail", n_cu, d_rows, d_out, d_sink);
    const double vd = runp<true, true, true, true>("(d) everything: loads + flag + slow path + tail", n_cu, d_rows, d_out, d_sink);
    const double ve = runp<true, false, true, true, true>("(e) = (d), flag counted in the slow path, slow path unlikely", n_cu, d_rows, d_out, d_sink);
    printf("prices in ns per block and SIMD: (a) %+.2f  (b) %+.2f  (c) %+.2f  tail %+.2f  (d) %+.2f; flag inside (d) %+.2f, slow path inside (d) %+.2f; (e) against (d) %+.2f\n",
           va - base, vb - base, vc - base, vt - base, vd - base, vd - vac, vd - vab, ve - vd);
    (void)hipFree(d_rows);
    printf("the earlier variants:\n");
  }
  run<2, 0, 0>("2 MFMAs per block, nothing else", n_cu, d_out, d_sink);
  run<0, 1, 0>("chain test only", n_cu, d_out, d_sink);
  run<0, 1, 4>("chain test + expansion only", n_cu, d_out, d_sink);
  run<2, 1, 0>("2 MFMAs + chain test", n_cu, d_out, d_sink);
  run<2, 2, 0>("2 MFMAs + tree test", n_cu, d_out, d_sink);
  run<2, 3, 0>("2 MFMAs + chain over 8 registers", n_cu, d_out, d_sink);
  run<2, 1, 4>("2 MFMAs + chain test + expansion (the product's half)", n_cu, d_out, d_sink);
  run<2, 2, 4>("2 MFMAs + tree test + expansion", n_cu, d_out, d_sink);
  run16<0>("4 x (16x16x128, C = 0) + chain test", n_cu, d_out, d_sink);
  run16<4>("4 x (16x16x128, C = 0) + chain test + expansion", n_cu, d_out, d_sink);
  run<3, 0, 0>("3 MFMAs per block, nothing else", n_cu, d_out, d_sink);
  run<3, 1, 4>("3 MFMAs + chain test + expansion", n_cu, d_out, d_sink);
  run<4, 0, 0>("4 MFMAs per block, nothing else", n_cu, d_out, d_sink);
  run<4, 1, 4>("4 MFMAs + chain test + expansion (the product's whole)", n_cu, d_out, d_sink);
  run<4, 2, 4>("4 MFMAs + tree test + expansion", n_cu, d_out, d_sink);
  return 0;
}
