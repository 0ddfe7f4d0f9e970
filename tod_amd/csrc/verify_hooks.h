// The todhip_test_* entry points: single kernels of the verifier driven from tests (FillAdjacency, selectWithinDistance for given
// triples, the clique search on an explicit graph as in the reference's test/test_maximum_clique.cpp).
// Included last by verify.hip, after its anonymous namespace and C entry points.

// the kernel of todhip_test_depth_lookup
namespace {
struct LookupArgs { const float* kp_xy; const void* depth; float* z; uint32_t* err; uint32_t n, H, W; int is_u16, rescale; RescaleGeom geom; };
__global__ __launch_bounds__(256) void depth_lookup_kernel(LookupArgs a) {
  const uint32_t q = blockIdx.x * 256u + threadIdx.x;
  if (q >= a.n) return;
  const int row = (int)a.kp_xy[2 * q + 1], col = (int)a.kp_xy[2 * q];      // float -> int truncation, as cluster_frame
  if (row < 0 || col < 0 || (uint32_t)row >= a.H || (uint32_t)col >= a.W) { atomicExch(a.err, 1u); return; }
  a.z[q] = a.rescale ? rescaled_depth_at(a.depth, a.is_u16, a.geom, (uint32_t)col, (uint32_t)row)
                     : depth_metres(a.depth, a.is_u16, (size_t)row * a.W + col);
}
// the kernel of todhip_test_kabsch: one lane per case
__global__ __launch_bounds__(64) void kabsch_test_kernel(uint32_t n, const double* Hd, const float* C, float* R, float* T) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= n) return;
  double h[9]; float c[6], r[9], t[3];
  for (int k = 0; k < 9; ++k) h[k] = Hd[(size_t)i * 9 + k];
  for (int k = 0; k < 6; ++k) c[k] = C[(size_t)i * 6 + k];
  kabsch_solve(h, c, r, t);
  for (int k = 0; k < 9; ++k) R[(size_t)i * 9 + k] = r[k];
  for (int k = 0; k < 3; ++k) T[(size_t)i * 3 + k] = t[k];
}
}  // namespace

extern "C" {

// Test hook: kabsch_solve (verify_growth.h) alone, as growth_kernel and sprint_kernel call it -- n_cases correlation matrices Hd
// (n x 9 doubles, row-major) and centroid pairs C (n x 6: train, query) give R (n x 9) and T (n x 3), query -> train, before the
// inversion. Host arrays. Whole frames cannot produce the matrices that try an SVD (rank deficient, equal singular values, the ends
// of the float range); this can.
int todhip_test_kabsch(todhip_ctx* ctx, uint32_t n_cases, const double* Hd, const float* C, float* R, float* T) {
  if (!ctx || !Hd || !C || !R || !T || n_cases == 0 || n_cases > (1u << 20)) return TODHIP_EINVAL;
  TOD_HIP(hipSetDevice(ctx->device));
  VerifyWs* ws = ws_of(ctx);
  hipStream_t st = ctx->stream;
  const size_t n = n_cases;
  TOD_HIP(ws->phys.reserve(n * 9 * sizeof(double))); TOD_HIP(ws->train.reserve(n * 6 * sizeof(float)));
  TOD_HIP(ws->query.reserve(n * 9 * sizeof(float))); TOD_HIP(ws->kpxy.reserve(n * 3 * sizeof(float)));
  TOD_HIP(hipMemcpyAsync(ws->phys.p, Hd, n * 9 * sizeof(double), hipMemcpyHostToDevice, st));
  TOD_HIP(hipMemcpyAsync(ws->train.p, C, n * 6 * sizeof(float), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(kabsch_test_kernel, dim3((n_cases + 63u) / 64u), dim3(64), 0, st, n_cases, ws->phys.as<double>(),
                     ws->train.as<float>(), ws->query.as<float>(), ws->kpxy.as<float>());
  TOD_HIP(hipGetLastError());
  TOD_HIP(hipMemcpyAsync(R, ws->query.p, n * 9 * sizeof(float), hipMemcpyDeviceToHost, st));
  TOD_HIP(hipMemcpyAsync(T, ws->kpxy.p, n * 3 * sizeof(float), hipMemcpyDeviceToHost, st));
  TOD_HIP(hipStreamSynchronize(st));
  return TODHIP_OK;
}

int todhip_test_adjacency(todhip_ctx* ctx, const float* train, const float* query, const float* kpxy, uint32_t n,
                          float span, float err, uint64_t* phys, uint64_t* samp) {
  if (!ctx || !train || !query || !kpxy || !phys || !samp || n == 0 || n > (uint32_t)kMaxWords * 64u) return TODHIP_EINVAL;
  TOD_HIP(hipSetDevice(ctx->device));
  VerifyWs* ws = ws_of(ctx);
  const uint32_t W = (n + 63u) / 64u;
  hipStream_t st = ctx->stream;
  TOD_HIP(ws->train.reserve((size_t)n * 12)); TOD_HIP(ws->query.reserve((size_t)n * 12));
  TOD_HIP(ws->kpxy.reserve((size_t)n * 8));
  TOD_HIP(ws->phys.reserve((size_t)n * W * 8)); TOD_HIP(ws->samp.reserve((size_t)n * W * 8));
  TOD_HIP(ws->bits.reserve((size_t)8 * W * 8));
  TOD_HIP(hipMemcpyAsync(ws->train.p, train, (size_t)n * 12, hipMemcpyHostToDevice, st));
  TOD_HIP(hipMemcpyAsync(ws->query.p, query, (size_t)n * 12, hipMemcpyHostToDevice, st));
  TOD_HIP(hipMemcpyAsync(ws->kpxy.p, kpxy, (size_t)n * 8, hipMemcpyHostToDevice, st));
  ObjJob job;
  std::memset(&job, 0, sizeof(job));
  job.n = n; job.W = W;
  job.train = ws->train.as<float>(); job.query = ws->query.as<float>(); job.kpxy = ws->kpxy.as<float>();
  job.phys = ws->phys.as<u64>(); job.samp = ws->samp.as<u64>();
  launch_list<kManySlots>(st, adjacency_kernel<Slots<AdjArgs, kManySlots>>, std::vector<AdjArgs>{{job, span, err}}, 256, 0, 2,
              [](const AdjArgs& a) { return dim3(a.job.n, (a.job.W + 3u) / 4u); });
  TOD_HIP(hipGetLastError());
  TOD_HIP(hipMemcpyAsync(phys, ws->phys.p, (size_t)n * W * 8, hipMemcpyDeviceToHost, st));
  TOD_HIP(hipMemcpyAsync(samp, ws->samp.p, (size_t)n * W * 8, hipMemcpyDeviceToHost, st));
  TOD_HIP(hipStreamSynchronize(st));
  return TODHIP_OK;
}

// Test hook: FillAdjacency + selectWithinDistance (sac_model_registration_graph.h:171-269) for given sample
// triples (samples_ order). counts[t] = consensus size (0 = rejected by the gate). With stop_level 1 the clique
// search is skipped and counts[t] = -|F| for hypotheses that reach it. dbg (optional): dbg_stride words per triple.
int todhip_test_consensus(todhip_ctx* ctx, const float* train, const float* query, const float* kpxy, uint32_t n,
                          float span, float err, const uint32_t* triples, uint32_t n_triples, uint32_t stop_level,
                          int32_t* counts, uint32_t* dbg, uint32_t dbg_stride) {
  if (!ctx || !train || !query || !kpxy || !triples || !counts || n < 3 || n > (uint32_t)kMaxWords * 64u || n_triples == 0)
    return TODHIP_EINVAL;
  TOD_HIP(hipSetDevice(ctx->device));
  int rc = set_big_lds_once(ctx);
  if (rc != TODHIP_OK) return rc;
  VerifyWs* ws = ws_of(ctx);
  const uint32_t W = (n + 63u) / 64u;
  hipStream_t st = ctx->stream;
  TOD_HIP(ws->train.reserve((size_t)n * 12)); TOD_HIP(ws->query.reserve((size_t)n * 12));
  TOD_HIP(ws->qidx.reserve((size_t)n * 4)); TOD_HIP(ws->kpxy.reserve((size_t)n * 8));
  TOD_HIP(ws->phys.reserve((size_t)n * W * 8)); TOD_HIP(ws->samp.reserve((size_t)n * W * 8));
  TOD_HIP(ws->bits.reserve((size_t)8 * W * 8)); TOD_HIP(ws->sampdeg.reserve((size_t)n * 4));
  TOD_HIP(ws->small.reserve(256 * sizeof(uint32_t))); TOD_HIP(ws->h_small.reserve(256 * sizeof(uint32_t)));
  TOD_HIP(ws->iter_samples.reserve((size_t)n_triples * 12)); TOD_HIP(ws->counts.reserve((size_t)n_triples * 4));
  TOD_HIP(ws->gate_m.reserve((size_t)n_triples * 4)); TOD_HIP(ws->deferred.reserve((size_t)n_triples * 4));
  TOD_HIP(ws->stacks.reserve((size_t)kMaxEvalWaves * kStackCap * sizeof(uint16_t)));
  if (dbg) TOD_HIP(ws->table.reserve((size_t)n_triples * dbg_stride * 4));
  TOD_HIP(hipMemcpyAsync(ws->train.p, train, (size_t)n * 12, hipMemcpyHostToDevice, st));
  TOD_HIP(hipMemcpyAsync(ws->query.p, query, (size_t)n * 12, hipMemcpyHostToDevice, st));
  TOD_HIP(hipMemcpyAsync(ws->kpxy.p, kpxy, (size_t)n * 8, hipMemcpyHostToDevice, st));
  TOD_HIP(hipMemcpyAsync(ws->iter_samples.p, triples, (size_t)n_triples * 12, hipMemcpyHostToDevice, st));
  TOD_HIP(hipMemsetAsync(ws->qidx.p, 0, (size_t)n * 4, st));
  if (dbg) TOD_HIP(hipMemsetAsync(ws->table.p, 0, (size_t)n_triples * dbg_stride * 4, st));
  ObjJob job;
  job.n = n; job.W = W;
  job.train = ws->train.as<float>(); job.query = ws->query.as<float>(); job.qidx = ws->qidx.as<uint32_t>();
  job.kpxy = ws->kpxy.as<float>(); job.phys = ws->phys.as<u64>(); job.samp = ws->samp.as<u64>();
  u64* bits = ws->bits.as<u64>();
  job.finite = bits; job.valid = bits + W; job.deg7 = bits + 2 * W; job.sampdeg = ws->sampdeg.as<uint32_t>();
  SlotCtl* d_ctl = ws->small.as<SlotCtl>();
  EvalStatus* h_eval = &ws->h_small.as<SlotCtl>()->eval;
  TOD_HIP(hipMemsetAsync(d_ctl, 0, sizeof(SlotCtl), st));
  launch_list<kManySlots>(st, finite_kernel<Slots<JobArgs, kManySlots>>, std::vector<JobArgs>{{job}}, 256, 0, 1, [](const JobArgs& a) { return dim3((a.job.n + 255u) / 256u); });
  launch_list<kManySlots>(st, adjacency_kernel<Slots<AdjArgs, kManySlots>>, std::vector<AdjArgs>{{job, span, err}}, 256, 0, 2,
              [](const AdjArgs& a) { return dim3(a.job.n, (a.job.W + 3u) / 4u); });
  launch_list<kManySlots>(st, round_prep_kernel<Slots<PrepArgs, kManySlots>>, std::vector<PrepArgs>{{job, d_ctl->prep, nullptr, 0u}}, 256, 0, 1,
              [](const PrepArgs& a) { return dim3((a.job.n + 255u) / 256u); });
  EvalArgs A = eval_args(job, ws, ws->counts.as<int32_t>(), 0u, n_triples, kEvalLdsSmall);
  A.dbg = dbg ? ws->table.as<uint32_t>() : nullptr; A.dbg_stride = dbg_stride; A.stop_level = stop_level;
  if (n_triples > kMaxEvalWaves) return TODHIP_EINVAL;
  auto launch = [&](auto, auto kern, auto ext) { launch_list(st, kern, std::vector<EvalArgs>{A}, 64, A.lds_bytes, 1, ext); };
  pick_eval(W > 8u, false, launch);
  TOD_HIP(hipGetLastError());
  TOD_HIP(hipMemcpyAsync(h_eval, &d_ctl->eval, sizeof(EvalStatus), hipMemcpyDeviceToHost, st));
  TOD_HIP(hipStreamSynchronize(st));
  const uint32_t status = h_eval->error, n_def = h_eval->n_deferred;
  if (status == 0 && n_def > 0) {
    A.lds_bytes = kEvalLdsBig; A.from_deferred = 1; A.n_deferred = n_def;
    TOD_HIP(ws->adjc_scratch.reserve((size_t)n_def * kAdjcScratchWords * sizeof(u64)));
    A.adjc_scratch = ws->adjc_scratch.as<u64>();
    TOD_HIP(hipMemsetAsync(&d_ctl->eval_work, 0, sizeof(uint32_t), st));
    pick_eval(W > 8u, true, launch);
    TOD_HIP(hipGetLastError());
    TOD_HIP(hipMemcpyAsync(h_eval, &d_ctl->eval, sizeof(EvalStatus), hipMemcpyDeviceToHost, st));
    TOD_HIP(hipStreamSynchronize(st));
  }
  TOD_HIP(hipMemcpyAsync(counts, ws->counts.p, (size_t)n_triples * 4, hipMemcpyDeviceToHost, st));
  if (dbg) TOD_HIP(hipMemcpyAsync(dbg, ws->table.p, (size_t)n_triples * dbg_stride * 4, hipMemcpyDeviceToHost, st));
  TOD_HIP(hipStreamSynchronize(st));
  if (h_eval->error != 0) {
    TOD_DBG("consensus status %u: g=%u value=%u m=%u it=%u", h_eval->error, h_eval->detail_g, h_eval->detail_value, h_eval->detail_m, h_eval->detail_it);
    return TODHIP_ESCRATCH;
  }
  return TODHIP_OK;
}

// Test hook: the speculative draw table of one object alone -- the S entries that the attempts starting at positions 0 .. S - 1 of
// the window_len stream words rnd leave, for the n x W sample bit matrix samp and the W valid words (host arrays; W = ceil(n / 64);
// bits of valid at or beyond n end an attempt as the kernels' in-bounds guard says). form picks the kernel: 0 = the engine's
// routing (draw_form_of), 1 = one lane per position, 2 = one wave per position with one slice, 3 = with eight slices, 4 = one lane
// per position with eight words a lane whatever W (form 1 gives an object of one or two words the two-word kernel, as the engine
// does; 4 runs the eight-word one on it); a form that cannot hold the object's W words is TODHIP_EINVAL. entries_out: S x 6
// words (DrawEntry).
int todhip_test_draw_table(todhip_ctx* ctx, const uint64_t* samp, const uint64_t* valid, uint32_t n, const uint32_t* rnd,
                           uint32_t window_len, uint32_t S, uint32_t form, uint32_t* entries_out) {
  if (!ctx || !samp || !valid || !rnd || !entries_out || n == 0 || n > (uint32_t)kMaxWords * 64u || S == 0 || S > (1u << 20) ||
      window_len == 0 || window_len > (1u << 24) || form > 4u)
    return TODHIP_EINVAL;
  const uint32_t W = (n + 63u) / 64u;
  DrawForm f = draw_form_of(W);
  if (form == 1u) f = W <= 2u ? DRAW_LANE2 : DRAW_LANE8;
  if (form == 2u) f = DRAW_WAVE1;
  if (form == 3u) f = DRAW_WAVE8;
  if (form == 4u) f = DRAW_LANE8;
  if (W > draw_form_max_words(f)) return TODHIP_EINVAL;
  TOD_HIP(hipSetDevice(ctx->device));
  VerifyWs* ws = ws_of(ctx);
  hipStream_t st = ctx->stream;
  TOD_HIP(ws->samp.reserve((size_t)n * W * 8)); TOD_HIP(ws->bits.reserve((size_t)8 * W * 8));
  TOD_HIP(ws->iter_samples.reserve((size_t)window_len * 4));            // (the stream words)
  TOD_HIP(ws->table.reserve((size_t)S * sizeof(DrawEntry)));
  TOD_HIP(hipMemcpyAsync(ws->samp.p, samp, (size_t)n * W * 8, hipMemcpyHostToDevice, st));
  TOD_HIP(hipMemcpyAsync(ws->bits.as<u64>() + W, valid, (size_t)W * 8, hipMemcpyHostToDevice, st));
  TOD_HIP(hipMemcpyAsync(ws->iter_samples.p, rnd, (size_t)window_len * 4, hipMemcpyHostToDevice, st));
  TOD_HIP(hipMemsetAsync(ws->table.p, 0xFF, (size_t)S * sizeof(DrawEntry), st));   // an entry nobody wrote does not pass for one
  ObjJob job;
  std::memset(&job, 0, sizeof(job));
  job.n = n; job.W = W; job.samp = ws->samp.as<u64>(); job.valid = ws->bits.as<u64>() + W;
  launch_draws(st, f, std::vector<DrawArgs>{{job, ws->iter_samples.as<uint32_t>(), window_len, S, ws->table.as<DrawEntry>()}});
  TOD_HIP(hipGetLastError());
  TOD_HIP(hipMemcpyAsync(entries_out, ws->table.p, (size_t)S * sizeof(DrawEntry), hipMemcpyDeviceToHost, st));
  TOD_HIP(hipStreamSynchronize(st));
  return TODHIP_OK;
}

// Test hook: the depth lookup of cluster_frame_kernel alone -- z of the keypoint's 3D point for n pixel positions, out of a dH x dW
// depth image seen as rescale_depth's H x W result (equal sizes: the plain load). A position outside the H x W image is what the
// cluster kernel refuses (ClusterCtl::error 1, TODHIP_ERANGE from the verify calls): its z_out is left as it was and the call returns
// TODHIP_ERANGE after filling the others.

int todhip_test_depth_lookup(todhip_ctx* ctx, const void* d_depth, int depth_is_u16, uint32_t dH, uint32_t dW, int nearest, uint32_t H,
                             uint32_t W, const float* kp_xy, uint32_t n, float* z_out) {
  if (!ctx || !d_depth || !kp_xy || !z_out || !dH || !dW || !H || !W || n == 0 || n > (1u << 24)) return TODHIP_EINVAL;
  LookupArgs a = {};
  if (!rescale_geometry(dH, dW, H, W, nearest, &a.geom)) return TODHIP_EINVAL;
  TOD_HIP(hipSetDevice(ctx->device));
  VerifyWs* ws = ws_of(ctx);
  hipStream_t st = ctx->stream;
  TOD_HIP(ws->kpxy.reserve((size_t)n * 8)); TOD_HIP(ws->c_qpt.reserve((size_t)n * 4)); TOD_HIP(ws->small.reserve(256 * sizeof(uint32_t)));
  TOD_HIP(hipMemcpyAsync(ws->kpxy.p, kp_xy, (size_t)n * 8, hipMemcpyHostToDevice, st));
  TOD_HIP(hipMemcpyAsync(ws->c_qpt.p, z_out, (size_t)n * 4, hipMemcpyHostToDevice, st));     // refused positions keep the caller's value
  TOD_HIP(hipMemsetAsync(ws->small.p, 0, sizeof(uint32_t), st));
  a.kp_xy = ws->kpxy.as<float>(); a.depth = d_depth; a.z = ws->c_qpt.as<float>(); a.err = ws->small.as<uint32_t>();
  a.n = n; a.H = H; a.W = W; a.is_u16 = depth_is_u16 ? 1 : 0; a.rescale = a.geom.mode != RescaleGeom::kEqual;
  hipLaunchKernelGGL(depth_lookup_kernel, dim3((n + 255u) / 256u), dim3(256), 0, st, a);
  TOD_HIP(hipGetLastError());
  uint32_t err = 0;
  TOD_HIP(hipMemcpyAsync(z_out, ws->c_qpt.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  TOD_HIP(hipMemcpyAsync(&err, ws->small.p, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  TOD_HIP(hipStreamSynchronize(st));
  return err ? TODHIP_ERANGE : TODHIP_OK;
}

// Test hook: the clique search on an explicit graph (edges as pairs), FindClique(minimal_size).
// out3 = {clique size, error flag, steps}. Mirrors the reference's gtest shape (test/test_maximum_clique.cpp).
static int test_clique_impl(todhip_ctx* ctx, uint32_t m, const uint32_t* edges, uint32_t n_edges, uint32_t minimal_size,
                            uint32_t* out3, bool gate) {
  if (!ctx || !out3 || m == 0 || m > 1024 || (n_edges && !edges)) return TODHIP_EINVAL;
  TOD_HIP(hipSetDevice(ctx->device));
  int rc = set_big_lds_once(ctx);
  if (rc != TODHIP_OK) return rc;
  VerifyWs* ws = ws_of(ctx);
  const uint32_t MW = (m + 63u) / 64u;
  std::vector<u64> adj((size_t)m * MW, 0ull);
  for (uint32_t e = 0; e < n_edges; ++e) {
    const uint32_t a = edges[2 * e], b = edges[2 * e + 1];
    if (a >= m || b >= m || a == b) return TODHIP_EINVAL;
    adj[(size_t)a * MW + (b >> 6)] |= 1ull << (b & 63u);
    adj[(size_t)b * MW + (a >> 6)] |= 1ull << (a & 63u);
  }
  TOD_HIP(ws->clique_adj.reserve(adj.size() * 8 + 64));
  TOD_HIP(ws->stacks.reserve((size_t)kStackCap * sizeof(uint16_t)));
  TOD_HIP(ws->small.reserve(256 * sizeof(uint32_t)));
  TOD_HIP(hipMemcpyAsync(ws->clique_adj.p, adj.data(), adj.size() * 8, hipMemcpyHostToDevice, ctx->stream));
  if (gate_lds_bytes(m) > kEvalLdsBig) return TODHIP_ESCRATCH;
  const uint32_t lds = gate_lds_bytes(m) <= kEvalLdsSmall ? kEvalLdsSmall : kEvalLdsBig;   // the two LDS tiers of eval_kernel
  auto launch = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3(1), dim3(64), lds, ctx->stream, ws->clique_adj.as<u64>(), m, minimal_size,
                       ws->stacks.as<uint16_t>(), kStackCap, lds, ws->small.as<uint32_t>());
  };
  if (m <= 512u) { if (gate) launch(clique_test_kernel<true, false>); else launch(clique_test_kernel<false, false>); }   // the product's narrow search
  else { if (gate) launch(clique_test_kernel<true, true>); else launch(clique_test_kernel<false, true>); }
  TOD_HIP(hipGetLastError());
  TOD_HIP(hipMemcpyAsync(out3, ws->small.p, 3 * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  TOD_HIP(hipStreamSynchronize(ctx->stream));
  return TODHIP_OK;
}

int todhip_test_clique(todhip_ctx* ctx, uint32_t m, const uint32_t* edges, uint32_t n_edges, uint32_t minimal_size,
                       uint32_t* out3) {
  return test_clique_impl(ctx, m, edges, n_edges, minimal_size, out3, false);
}

// The same graph through the form of the search the verifier's gate runs (clique_search<., kGate = true>): it stops as soon as
// "is the clique FindClique(minimal_size) returns larger than minimal_size" is decided, so out3[0] is that clique's size only
// when it is <= minimal_size, and a lower bound > minimal_size otherwise; out3[2] counts the steps actually walked.
int todhip_test_clique_gate(todhip_ctx* ctx, uint32_t m, const uint32_t* edges, uint32_t n_edges, uint32_t minimal_size,
                            uint32_t* out3) {
  return test_clique_impl(ctx, m, edges, n_edges, minimal_size, out3, true);
}

}  // extern "C"
