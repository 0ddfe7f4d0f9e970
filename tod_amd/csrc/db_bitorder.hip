// The optional bit order of the resident Hamming DB (todhip_set_db_bit_order): statistics of the shard's rows, the order (host:
// db_bitorder.h) and the kernel that rewrites DB rows and query rows alike. Hamming distance does not depend on the order of the bit
// positions, so every result is the unordered DB's; what changes is which positions the matrix-core engine's split blocks see first
// (mfma_block_test_part, match_mfma.h). Load-time work, except the query permutation in front of a search (tod_match_lists).
// No reference lines: the reference has no such step.
//
//   BO1 bit_planes_kernel        wave = 64 sample rows: per bit position a ballot, so planes[w][b] = bit b of sample rows 64 w .. 64 w + 63
//   BO2 bit_pair_counts_kernel   block = bit a, thread = bit b: both[a][b] = sum over w of popcount(planes[w][a] & planes[w][b])
//   BO3 permute_bits_kernel      thread = row: stored position p takes original bit src_of[p]; in place or into another buffer
#include <vector>

#include "ctx.h"
#include "db_bitorder.h"

namespace {

constexpr uint32_t kMaxSample = 65536;

// sample row i = row floor(i * n_rows / S); lanes beyond S contribute zeros
__global__ __launch_bounds__(256) void bit_planes_kernel(const uint32_t* __restrict__ db, uint32_t n_rows, uint32_t S, uint64_t* __restrict__ planes) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u, w = i >> 6;
  uint32_t d[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
  if (i < S) {
    const uint64_t row = (uint64_t)i * n_rows / S;
    const uint4 a = reinterpret_cast<const uint4*>(db + row * 8u)[0], b = reinterpret_cast<const uint4*>(db + row * 8u)[1];
    d[0] = a.x; d[1] = a.y; d[2] = a.z; d[3] = a.w; d[4] = b.x; d[5] = b.y; d[6] = b.z; d[7] = b.w;
  }
  if (w * 64u >= S) return;                                           // whole waves leave together
#pragma unroll
  for (uint32_t g = 0; g < 4; ++g) {                                  // 64 bit positions at a time: lane l keeps the ballot of position 64 g + l
    uint64_t mine = 0;
#pragma unroll
    for (uint32_t t = 0; t < 64; ++t) {
      const uint64_t m = __builtin_amdgcn_ballot_w64((d[2 * g + (t >> 5)] >> (t & 31u)) & 1u);
      if (lane == t) mine = m;
    }
    planes[(size_t)w * 256u + 64u * g + lane] = mine;
  }
}

// out[0..255] = ones, out[256 + a * 256 + b] = both[a][b]
__global__ __launch_bounds__(256) void bit_pair_counts_kernel(const uint64_t* __restrict__ planes, uint32_t n_words, uint32_t* __restrict__ out) {
  const uint32_t a = blockIdx.x, b = threadIdx.x;
  uint32_t n = 0;
  for (uint32_t w = 0; w < n_words; ++w) n += (uint32_t)__popcll(planes[(size_t)w * 256u + a] & planes[(size_t)w * 256u + b]);
  out[256u + a * 256u + b] = n;
  if (a == b) out[a] = n;
}

// tab: src_of as 64 dwords (wave-uniform reads). A thread keeps its row in its own column of the shared array -- an indexable
// register file, read by nobody else, so there is no barrier -- and writes only its own row: src == dst is allowed.
__global__ __launch_bounds__(256) void permute_bits_kernel(const uint32_t* src, uint32_t* dst, uint32_t n_rows, const uint32_t* __restrict__ tab) {
  __shared__ uint32_t s_in[8][256];
  const uint32_t tid = threadIdx.x;
  const size_t row = (size_t)blockIdx.x * 256u + tid;
  if (row >= n_rows) return;
  {
    const uint4 a = reinterpret_cast<const uint4*>(src + row * 8u)[0], b = reinterpret_cast<const uint4*>(src + row * 8u)[1];
    s_in[0][tid] = a.x; s_in[1][tid] = a.y; s_in[2][tid] = a.z; s_in[3][tid] = a.w;
    s_in[4][tid] = b.x; s_in[5][tid] = b.y; s_in[6][tid] = b.z; s_in[7][tid] = b.w;
  }
  uint32_t o[8];
  for (uint32_t j = 0; j < 8; ++j) {
    uint32_t acc = 0;
#pragma unroll
    for (uint32_t t = 0; t < 32; ++t) {
      const uint32_t p = (tab[8u * j + (t >> 2)] >> (8u * (t & 3u))) & 0xFFu;
      acc |= ((s_in[p >> 5][tid] >> (p & 31u)) & 1u) << t;
    }
    o[j] = acc;
  }
  reinterpret_cast<uint4*>(dst + row * 8u)[0] = uint4{o[0], o[1], o[2], o[3]};
  reinterpret_cast<uint4*>(dst + row * 8u)[1] = uint4{o[4], o[5], o[6], o[7]};
}

int launch_permute(todhip_ctx* ctx, const void* src, void* dst, uint32_t n_rows) {
  if (n_rows == 0) return TODHIP_OK;
  hipLaunchKernelGGL(permute_bits_kernel, dim3((n_rows + 255u) / 256u), dim3(256), 0, ctx->stream, reinterpret_cast<const uint32_t*>(src),
                     reinterpret_cast<uint32_t*>(dst), n_rows, ctx->bit_tab.as<uint32_t>());
  TOD_HIP(hipGetLastError());
  return TODHIP_OK;
}

}  // namespace

// Called by todhip_db_load with the shard's rows in ctx->db_desc, before any index is built over them: with the order switched on,
// measure, decide and rewrite the rows in place (never a byte behind row shard_rows - 1); otherwise back to the identity.
int tod_bit_order_load(todhip_ctx* ctx) {
  ctx->bit_order_on = false;
  tod_db_rows_written(ctx);                                            // (the load has said so already; the rewrite below is a write of its own)
  for (int p = 0; p < 256; ++p) ctx->bit_src_of[p] = (uint8_t)p;
  if (ctx->bit_order_mode != TODHIP_BIT_ORDER_INFORMATIVE_FIRST || ctx->desc_bytes != 32 || ctx->shard_rows == 0) return TODHIP_OK;
  if (ctx->shard_rows > 0xFFFFFFFFull) return TODHIP_EINVAL;
  const uint32_t n = (uint32_t)ctx->shard_rows, S = std::min(n, kMaxSample), n_words = (S + 63u) / 64u;
  DevBuf planes, stats;                                                // load-time scratch: freed on return
  TOD_HIP(planes.reserve((size_t)n_words * 256u * sizeof(uint64_t)));
  TOD_HIP(stats.reserve((256u + 65536u) * sizeof(uint32_t)));
  hipLaunchKernelGGL(bit_planes_kernel, dim3((S + 255u) / 256u), dim3(256), 0, ctx->stream, ctx->db_desc.as<uint32_t>(), n, S, planes.as<uint64_t>());
  hipLaunchKernelGGL(bit_pair_counts_kernel, dim3(256), dim3(256), 0, ctx->stream, planes.as<uint64_t>(), n_words, stats.as<uint32_t>());
  TOD_HIP(hipGetLastError());
  std::vector<uint32_t> h(256u + 65536u);
  TOD_HIP(hipMemcpyAsync(h.data(), stats.p, h.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  TOD_HIP(hipStreamSynchronize(ctx->stream));
  tod_bit_order_from_stats(S, h.data(), h.data() + 256, ctx->bit_src_of);
  bool identity = true;
  for (int p = 0; p < 256; ++p) identity = identity && ctx->bit_src_of[p] == p;
  if (identity) return TODHIP_OK;
  TOD_HIP(ctx->bit_tab.reserve(256));
  TOD_HIP(hipMemcpyAsync(ctx->bit_tab.p, ctx->bit_src_of, 256, hipMemcpyHostToDevice, ctx->stream));
  TOD_HIP(hipStreamSynchronize(ctx->stream));                          // (pageable source: complete before anybody changes it)
  ctx->bit_order_on = true;
  return launch_permute(ctx, ctx->db_desc.p, ctx->db_desc.p, n);
}

// The nq query rows in the resident order, in a workspace of the context (the caller's buffer is only read); *d_out is what the
// search kernels take. Only called while an order is in force.
int tod_bit_order_queries(todhip_ctx* ctx, const void* d_q, uint32_t nq, const void** d_out) {
  TOD_HIP(ctx->m_qord.reserve((size_t)nq * 32u));
  *d_out = ctx->m_qord.p;
  return launch_permute(ctx, d_q, ctx->m_qord.p, nq);
}

extern "C" int todhip_set_db_bit_order(todhip_ctx* ctx, int mode) {
  if (!ctx || (mode != TODHIP_BIT_ORDER_NONE && mode != TODHIP_BIT_ORDER_INFORMATIVE_FIRST)) return TODHIP_EINVAL;
  ctx->bit_order_mode = mode;
  tod_db_rows_written(ctx);                                            // the next load stores the rows in another order
  return TODHIP_OK;
}

extern "C" int todhip_db_bit_order(const todhip_ctx* ctx, uint8_t src_of[256]) {
  if (!ctx || !src_of) return TODHIP_EINVAL;
  for (int p = 0; p < 256; ++p) src_of[p] = ctx->bit_src_of[p];
  return TODHIP_OK;
}
