// todhip_db_select_objects: search a chosen subset of the resident Hamming DB's objects without another load. The reference's detector
// is told which objects to find (json_object_ids, python/object_recognition_tod/detector.py:53-60) and its
// DescriptorMatcher::parameter_callback builds the matcher from those objects alone; here the DB stays resident and a selection
// builds a compacted VIEW of the shard's selected rows beside it. The DB-pass kernels then run over the view as they would over a
// shard (same row format, same bit order, same slack behind the last row) and the keys they produce are mapped back to rows of the
// full DB, so everything downstream -- shard merge, ratio test, radius cut, object lookup, 3D gather, the verifier's spans -- reads
// the numbering of the whole DB. Host-side tables: db_select.h.
//
//   DS1 gather_view_kernel   wave = 128 view rows of 32 bytes or 64 of 64 bytes (4 KB): one wave-uniform binary search of the segment table for the wave's first
//                            row, a per-lane walk forward from there (objects are mostly longer than a wave's rows: no step at
//                            all), then lane = 16 bytes of a row, four loads in flight, four stores. Bound by HBM: every selected
//                            row is read once and written once.
//   DS2 remap_keys_kernel    thread = key of a merge list: (distance << 32 | view row) -> (distance << 32 | global row), by the same
//                            search; padding keys (~0) stay. The map is increasing, so ascending lists stay ascending and the order
//                            (distance, global row) of decision D1 is the one the view's search already used.
#include "ctx.h"

namespace {

constexpr uint32_t kGatherSteps = 4;                        // 1 KB steps per wave

// src: the shard's rows as stored (row i of the shard = global row shard_first + i); dst: view_rows rows. L lanes of 16 bytes per
// row: two for 32-byte rows, four for 64-byte ones.
template <uint32_t L>
__global__ __launch_bounds__(256) void gather_view_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst,
                                                          const uint32_t* __restrict__ seg_view, const uint32_t* __restrict__ seg_global,
                                                          uint32_t n_segs, uint32_t view_rows, uint32_t shard_first) {
  const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6)), lane = threadIdx.x & 63u;
  constexpr uint32_t kStepRows = 64u / L, kGatherRows = kStepRows * kGatherSteps;
  const uint32_t r0 = wave * kGatherRows;
  if (r0 >= view_rows) return;                               // whole waves leave together
  uint32_t lo = 0, hi = n_segs;                              // wave-uniform: the last segment whose first view row is <= r0
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (seg_view[mid] <= r0) lo = mid; else hi = mid;
  }
  uint32_t s = lo;
  uint4 v[kGatherSteps];
#pragma unroll
  for (uint32_t g = 0; g < kGatherSteps; ++g) {
    const uint32_t r = r0 + kStepRows * g + lane / L;
    v[g] = uint4{0u, 0u, 0u, 0u};
    if (r < view_rows) {
      while (r >= seg_view[s + 1]) ++s;                      // ends: r < view_rows = seg_view[n_segs]
      const size_t row = (size_t)(seg_global[s] - shard_first) + (r - seg_view[s]);
      v[g] = src[row * L + lane % L];
    }
  }
#pragma unroll
  for (uint32_t g = 0; g < kGatherSteps; ++g) {
    const uint32_t r = r0 + kStepRows * g + lane / L;
    if (r < view_rows) dst[(size_t)r * L + lane % L] = v[g];
  }
}

__global__ __launch_bounds__(256) void remap_keys_kernel(uint64_t* __restrict__ keys, size_t n, const uint32_t* __restrict__ seg_view,
                                                         const uint32_t* __restrict__ seg_global, uint32_t n_segs) {
  TOD_LATENCY_PRIO();   // latency-bound, as the merges it follows
  const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint64_t key = keys[i];
  if (key == ~0ull) return;
  const uint32_t r = (uint32_t)key;
  uint32_t lo = 0, hi = n_segs;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (seg_view[mid] <= r) lo = mid; else hi = mid;
  }
  keys[i] = (key & 0xFFFFFFFF00000000ull) | (uint64_t)(seg_global[lo] + (r - seg_view[lo]));
}

// the view of `t` on the device: tables, rows, zeroed slack
int build_view(todhip_ctx* ctx, const TodViewTables& t) {
  const uint32_t n_segs = t.n_segs(), rows = t.view_rows();
  if (rows == 0) return TODHIP_OK;                           // nothing to search: no launch ever reads the buffers
  TOD_HIP(ctx->view_tab.reserve((size_t)(2u * n_segs + 1u) * sizeof(uint32_t)));
  const uint32_t desc_bytes = ctx->desc_bytes;              // 32 or 64 (todhip_db_select_objects)
  TOD_HIP(ctx->view_desc.reserve((size_t)rows * desc_bytes + kDbSlackBytes));
  uint32_t* const d_view = ctx->view_tab.as<uint32_t>();
  uint32_t* const d_global = d_view + n_segs + 1u;
  TOD_HIP(hipMemcpyAsync(d_view, t.seg_view.data(), (size_t)(n_segs + 1u) * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
  TOD_HIP(hipMemcpyAsync(d_global, t.seg_global.data(), (size_t)n_segs * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
  // hamming_topk_mfma and hamming_topk_wide load whole 32-row steps without a per-lane clamp: up to 31 rows behind the view's last one
  TOD_HIP(hipMemsetAsync(ctx->view_desc.as<uint8_t>() + (size_t)rows * desc_bytes, 0, kDbSlackBytes, ctx->stream));
  const uint32_t wave_rows = 1024u / desc_bytes * kGatherSteps, waves = (rows + wave_rows - 1u) / wave_rows;
  hipLaunchKernelGGL(desc_bytes == 64 ? gather_view_kernel<4> : gather_view_kernel<2>, dim3((waves + 3u) / 4u), dim3(256), 0, ctx->stream, ctx->db_desc.as<uint4>(), ctx->view_desc.as<uint4>(),
                     d_view, d_global, n_segs, rows, (uint32_t)ctx->shard_first);
  TOD_HIP(hipGetLastError());
  TOD_HIP(hipStreamSynchronize(ctx->stream));                // (pageable sources: complete before t may go)
  return TODHIP_OK;
}

}  // namespace

// all objects again, the view's memory returned
void tod_view_reset(todhip_ctx* ctx) {
  ctx->sel_on = false;
  ctx->sel = TodViewTables();
  ctx->view_desc.release();
  ctx->view_tab.release();
}

int tod_view_remap(todhip_ctx* ctx, uint64_t* d_keys, size_t n) {
  if (n == 0) return TODHIP_OK;
  const uint32_t n_segs = ctx->sel.n_segs();
  hipLaunchKernelGGL(remap_keys_kernel, dim3((uint32_t)((n + 255u) / 256u)), dim3(256), 0, ctx->stream, d_keys, n, ctx->view_tab.as<uint32_t>(),
                     ctx->view_tab.as<uint32_t>() + n_segs + 1u, n_segs);
  TOD_HIP(hipGetLastError());
  return TODHIP_OK;
}

extern "C" int todhip_db_select_objects(todhip_ctx* ctx, const uint32_t* ids, uint32_t n_ids) {
  if (!ctx) return TODHIP_EINVAL;
  if (ctx->total_rows == 0) return TODHIP_ENODB;
  if (ctx->desc_bytes != 32 && ctx->desc_bytes != 64) return TODHIP_EINVAL;   // the float DB has no view
  TodViewTables t;
  if (ids && !tod_view_build(ids, n_ids, ctx->h_obj_off.data(), ctx->n_objs, ctx->shard_first, ctx->shard_rows, &t)) return TODHIP_EINVAL;
  TOD_HIP(hipSetDevice(ctx->device));
  TOD_HIP(hipStreamSynchronize(ctx->stream));
  tod_db_rows_written(ctx);                                  // on or off: the searches read other rows from here on
  // every object listed is the state after a load: today's pointers, no second copy of the rows
  const bool all = !ids || t.objs.size() == ctx->n_objs;
  if (all) {
    tod_view_reset(ctx);
  } else {
    ctx->sel_on = false;                                     // (the buffers stay for the next view)
    ctx->sel = TodViewTables();
    int rc = build_view(ctx, t);
    if (rc != TODHIP_OK) { tod_view_reset(ctx); return rc; }   // a HIP error leaves all objects selected
    ctx->sel = std::move(t);
    ctx->sel_on = true;
  }
  ctx->k4x.restart();                                        // the split controller's state described the rows searched so far
  if (tod_lsh_enabled(ctx)) {                                // todhip_set_lsh indexes the active rows
    int rc = tod_lsh_build(ctx);
    if (rc != TODHIP_OK) return rc;
  }
  TOD_HIP(hipStreamSynchronize(ctx->stream));
  return TODHIP_OK;
}

extern "C" int todhip_db_selection(const todhip_ctx* ctx, uint32_t* n_selected_objs, uint64_t* selected_rows, uint64_t* selected_shard_rows) {
  if (!ctx) return TODHIP_EINVAL;
  if (n_selected_objs) *n_selected_objs = ctx->sel_on ? (uint32_t)ctx->sel.objs.size() : ctx->n_objs;
  if (selected_rows) *selected_rows = ctx->sel_on ? ctx->sel.selected_rows : ctx->total_rows;
  if (selected_shard_rows) *selected_shard_rows = tod_db_n_rows(ctx);
  return TODHIP_OK;
}
