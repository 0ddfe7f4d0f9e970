// Stage A on gfx950: ORB keypoints (FAST-9/16 + Harris ranking + intensity-centroid orientation) and 256-bit
// rBRIEF descriptors. In the reference this stage is third-party code outside its tree
// (ecto_opencv.features2d.FeatureDescriptor -> cv::ORB; python/object_recognition_tod/detector.py:10,27,
// src/training/Trainer.cpp:144-150), so there is nothing to be bit-exact with except the published algorithm;
// the free choices (fixed-point resize and blur, score definition, tie-breaks, rotation without angle
// quantisation, output order) are the ones stated at the top of this repo's CPU restatement and are followed
// here operation for operation (integer moments and gradients; float expressions without contraction).
//
// All images of a 640x480 pyramid are a few hundred KB: every kernel is latency/launch bound, not bandwidth
// bound; the per-level work is a fixed sequence of small launches with no host round trip until the final count.
// A batch of frames AND the pyramid levels ride in the last grid dimension of every launch: (level l, frame f) is "virtual
// frame" l F + f and owns slice l F + f of every workspace buffer and its own row of control words, the per-level geometry
// comes from a small table in the kernel arguments (LevelTab). A batch of any size and any number of levels therefore costs
// 12 + (levels - 1) launches (round 1 and most of round 2: 2 + 11 per level), blocks beyond a smaller level's extent leave at once.
// This file is the host side: workspace, graph cache, launch sequence, entry points. Sizes and grids: orb_plan.h; kernels: orb_*.h.
//
// ORB's kernels run at the default wave priority (none raises it as ctx.h's other latency-bound kernels do). They are wide (a thread
// per pixel, a wave per keypoint) and their stage has slack in the pipeline: at the raised wave priority of the verifier's single-wave
// kernels they took issue slots from the matcher's DB pass -- with the default priority the pass is 6 % faster in the pipeline (1.91
// instead of 2.03 ms per 32 000 x 1M launch) and the headline 4 % (tools/ab_prio.sh), ORB's own stage time unchanged within the spread.
#include <algorithm>
#include <cstring>
#include <vector>

#include "ctx.h"
#include "orb_arc.h"
#include "orb_compass.h"
#include "orb_stages.h"

using namespace tod_orb;

namespace {

#include "orb_pyramid.h"
#include "orb_fast.h"
#include "orb_select.h"
#include "orb_describe.h"

// The launch sequence is static for a given geometry: captured once per context, replayed. It reads and writes workspace buffers
// only (image and mask are copied in, keypoints copied out), so the caller's pointers may change from call to call without a
// re-capture. The key says what the captured sequence depends on.
struct OrbGraph {
  struct Key { uint32_t H, W, n_features, n_levels, cap, F; float sf; const void *kp, *aux, *desc, *img0, *mask, *taps; } key = {};
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  void drop() {                                            // the only teardown
    if (exec) (void)hipGraphExecDestroy(exec);
    if (graph) (void)hipGraphDestroy(graph);
    exec = nullptr; graph = nullptr; key = {};
  }
  bool matches(const Key& k) const { return exec && std::memcmp(&k, &key, sizeof(k)) == 0; }
  // thread-local capture: other host threads keep using the runtime while this one records
  hipError_t begin_capture(hipStream_t st) { drop(); return hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal); }
  hipError_t end_capture(hipStream_t st, const Key& k) {
    hipError_t e = hipStreamEndCapture(st, &graph);
    if (e == hipSuccess) e = graph ? hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) : hipErrorUnknown;
    if (e == hipSuccess) key = k;
    return e;
  }
  hipError_t launch(hipStream_t st) { return hipGraphLaunch(exec, st); }
};

struct OrbWs : TodWs {
  static constexpr int kSlot = kWsOrb;
  DevBuf pyr, blur, cand, eq, sel1, sel2, small, pattern, in_img, kp_xy, kp_aux, desc, o_xy, o_aux, o_desc, maskbuf, taps;
  HostBuf h_out, h_kp;                                     // h_kp: the host form's keypoints, written by copy_out_kernel itself
  bool pattern_is_default = false;
  struct TapsFor { uint32_t H, W, n_levels; float sf; const void* p; } taps_for = {};   // the pyramid whose resize taps are in `taps`
  OrbGraph graph;
  OrbPlan plan = {};                                       // of the last call, tab.img filled in: for tod_orb_stages
  ~OrbWs() override { graph.drop(); }                      // the captured graph goes before the buffers it refers to
};

// F frames of H x W u8 on the device (row stride `stride`, frame stride gray_fs bytes; the mask, if any, packed); what to compute;
// where the results go: frame f's keypoints at row f * cap of the three device arrays, n_out[f] (host) is read back
struct OrbIn { const uint8_t* d_gray; size_t gray_fs; const uint8_t* d_mask; uint32_t F, H, W, stride; };
struct OrbParams { uint32_t n_features, n_levels; float scale_factor; const int8_t* pattern; };
struct OrbOut { float* kp_xy; float* kp_aux; uint8_t* desc; uint32_t cap; uint32_t* n_out; };

inline dim3 grid(const OrbGrid& g) { return dim3(g.x, g.y, g.z); }

int reserve_buffers(todhip_ctx* ctx, OrbWs* ws, const OrbPlan& P, bool masked) {
  TOD_HIP(ws->pyr.reserve(P.V * P.px)); TOD_HIP(ws->blur.reserve(P.V * P.px));
  TOD_HIP(ws->cand.reserve(P.V * P.cand_cap * sizeof(Cand))); TOD_HIP(ws->eq.reserve(P.V * P.cand_cap * sizeof(Cand)));
  TOD_HIP(ws->sel1.reserve(P.V * P.sel1_cap * sizeof(Cand))); TOD_HIP(ws->sel2.reserve(P.V * P.sel2_cap * sizeof(Cand)));
  TOD_HIP(ws->small.reserve(P.ctl_words * sizeof(uint32_t))); TOD_HIP(ws->pattern.reserve(1024));
  TOD_HIP(ws->h_out.reserve((size_t)P.F * sizeof(uint32_t) + 64));
  TOD_HIP(ws->o_xy.reserve((size_t)P.F * P.cap * 8)); TOD_HIP(ws->o_aux.reserve((size_t)P.F * P.cap * 16));
  TOD_HIP(ws->o_desc.reserve((size_t)P.F * P.cap * 32));
  if (masked) TOD_HIP(ws->maskbuf.reserve(P.F * P.px));
  TOD_HIP(ws->taps.reserve((size_t)P.n_taps * sizeof(ResizeTap) + 32));
  return TODHIP_OK;
}

// the caller's pattern, or the built-in one unless it is already there
int upload_pattern(todhip_ctx* ctx, OrbWs* ws, const int8_t* pattern) {
  if (!pattern && ws->pattern_is_default) return TODHIP_OK;
  int8_t hpat[1024];
  if (pattern) std::memcpy(hpat, pattern, 1024); else default_pattern(hpat);
  ws->pattern_is_default = !pattern;
  TOD_HIP(hipMemcpyAsync(ws->pattern.p, hpat, 1024, hipMemcpyHostToDevice, ctx->stream));
  TOD_HIP(hipStreamSynchronize(ctx->stream));            // hpat lives on this stack frame
  return TODHIP_OK;
}

// the resize's tap tables (orb_plan.h), unless those of this pyramid are already there: they depend on the level sizes alone, so a
// context that sees one geometry fills them once, and a replay of the cached graph uploads nothing
int upload_taps(todhip_ctx* ctx, OrbWs* ws, const OrbPlan& P, float scale_factor) {
  const OrbWs::TapsFor now = {P.H, P.W, P.n_levels, scale_factor, ws->taps.p};
  if (std::memcmp(&now, &ws->taps_for, sizeof(now)) == 0 || P.n_taps == 0u) return TODHIP_OK;
  std::vector<ResizeTap> taps(P.n_taps);
  fill_resize_taps(P, taps.data());
  TOD_HIP(hipMemcpyAsync(ws->taps.p, taps.data(), taps.size() * sizeof(ResizeTap), hipMemcpyHostToDevice, ctx->stream));
  TOD_HIP(hipStreamSynchronize(ctx->stream));            // the vector lives on this stack frame
  ws->taps_for = now;
  return TODHIP_OK;
}

// The launch sequence and nothing else: the pyramid first (level l from level l - 1), then every kernel once for all levels and
// frames. P is the workspace's plan (tab.img filled in); the image is in ws->pyr, the keypoints go to ws->o_*.
void record_stages(const OrbPlan& P, const OrbWs* ws, const uint8_t* d_mask, hipStream_t st) {
  const LevelTab& T = P.tab;
  const size_t px = P.px;
  for (uint32_t lvl = 1; lvl < P.n_levels; ++lvl) {
    // a level of zero pixels has nothing to resize (an empty grid is no launch); the sizes only shrink, so no later level
    // reads it, and with want == 0 no kernel looks at its image
    if (P.resize_x[lvl] == 0u) continue;
    uint8_t* img = ws->pyr.as<uint8_t>() + (size_t)lvl * P.F * px;
    const ResizeTap* taps = ws->taps.as<ResizeTap>();
    hipLaunchKernelGGL(resize_kernel, grid(P.resize[lvl]), dim3(256), 0, st, img - (size_t)P.F * px, T.w[lvl - 1], img, T.h[lvl], T.w[lvl],
                       taps + P.tap_x[lvl], taps + P.tap_y[lvl], px);
  }
  uint32_t* ctl = ws->small.as<uint32_t>();
  uint32_t* level_counts = ctl + P.level_counts_off;
  Cand* cand = ws->cand.as<Cand>(); Cand* eq = ws->eq.as<Cand>(); Cand* sel1 = ws->sel1.as<Cand>(); Cand* sel2 = ws->sel2.as<Cand>();
  hipLaunchKernelGGL(fast_nms_kernel, grid(P.fast_nms), dim3(256), 0, st, T, cand, P.cand_cap, ctl, ctl + W_HIST, d_mask, P.H, P.W, px);
  hipLaunchKernelGGL(fast_threshold_kernel, grid(P.fast_threshold), dim3(64), 0, st, T, ctl, P.cand_cap);
  hipLaunchKernelGGL(split_kernel, grid(P.split), dim3(256), 0, st, T, cand, ctl, sel1, eq, P.cand_cap, P.sel1_cap);
  hipLaunchKernelGGL(rank_tiled_kernel, grid(P.rank_ties), dim3(256), 0, st, RankArgs::rank_ties(eq, P.cand_cap, sel1, P.sel1_cap, ctl));
  hipLaunchKernelGGL(harris_kernel, grid(P.harris), dim3(256), 0, st, T, sel1, ctl + W_NSEL1, px, P.sel1_cap);
  hipLaunchKernelGGL(rank_tiled_kernel, grid(P.rank_harris), dim3(256), 0, st,
                     RankArgs::rank_harris(sel1, P.sel1_cap, sel2, P.sel2_cap, ctl, level_counts, P.F));
  hipLaunchKernelGGL(blur_kernel, grid(P.blur), dim3(256), 0, st, T, ws->blur.as<uint8_t>(), px);
  DescribeArgs D;
  std::memset(&D, 0, sizeof(D));
  disc_umax(D.umax);
  D.blur = ws->blur.as<uint8_t>(); D.sel = sel2; D.level_counts = level_counts; D.cap = P.cap; D.pattern = ws->pattern.as<int8_t>();
  D.kp_xy = ws->o_xy.as<float>(); D.kp_aux = ws->o_aux.as<float>(); D.desc = ws->o_desc.as<uint8_t>(); D.fs = px; D.sel_fs = P.sel2_cap;
  hipLaunchKernelGGL(describe_kernel, grid(P.describe), dim3(256), 0, st, T, D);
}

int orb_device(todhip_ctx* ctx, const OrbIn& in, const OrbParams& par, const OrbOut& out) {
  OrbPlan P;
  if (const int bad = orb_plan(in.F, in.H, in.W, par.n_features, par.n_levels, par.scale_factor, out.cap, &P)) return bad;
  // where every form's pattern enters: a point outside the domain would steer a test out of the keypoint's level (steered_test reads
  // blur[(y + y0) * W + x + x0] unchecked). Refused before the workspace, the cached pattern or the graph are touched.
  if (const int bad = check_pattern(par.pattern)) return bad;
  OrbWs* ws = tod_ws<OrbWs>(ctx);
  hipStream_t st = ctx->stream;
  if (P.want_max == 0) {
    // no level is large enough for a keypoint: nothing to launch (and no empty graph to capture), no keypoints, outputs untouched.
    // The captured sequence of another geometry goes, so that ws->plan always describes what the next replay would run.
    ws->graph.drop();
    ws->plan = P;
    for (uint32_t f = 0; f < in.F; ++f) out.n_out[f] = 0;
    TOD_HIP(hipStreamSynchronize(st));                     // as every return: a host form's copies of the caller's image are done
    return TODHIP_OK;
  }
  if (const int rc = reserve_buffers(ctx, ws, P, in.d_mask != nullptr)) return rc;
  if (const int rc = upload_pattern(ctx, ws, par.pattern)) return rc;
  if (const int rc = upload_taps(ctx, ws, P, par.scale_factor)) return rc;
  for (uint32_t lvl = 0; lvl < P.n_levels; ++lvl) P.tab.img[lvl] = ws->pyr.as<uint8_t>() + (size_t)lvl * P.F * P.px;
  ws->plan = P;
  uint32_t* ctl = ws->small.as<uint32_t>();
  TOD_HIP(hipMemsetAsync(ctl, 0, P.ctl_words * sizeof(uint32_t), st));
  if (in.stride == P.W && (P.F == 1 || in.gray_fs == P.px))   // densely packed input: one device-to-device copy
    TOD_HIP(hipMemcpyAsync(ws->pyr.p, in.d_gray, (size_t)P.F * P.px, hipMemcpyDeviceToDevice, st));
  else
    hipLaunchKernelGGL(copy_rows_kernel, grid(P.copy_rows), dim3(256), 0, st, in.d_gray, in.stride, ws->pyr.as<uint8_t>(), P.H, P.W,
                       in.gray_fs, P.px);
  const uint8_t* ws_mask = nullptr;                        // the mask's own copy: the captured sequence reads workspace buffers only
  if (in.d_mask) {
    ws_mask = ws->maskbuf.as<uint8_t>();
    hipLaunchKernelGGL(copy_rows_kernel, grid(P.copy_rows), dim3(256), 0, st, in.d_mask, P.W, ws->maskbuf.as<uint8_t>(), P.H, P.W, P.px, P.px);
  }
  float* const ws_xy = ws->o_xy.as<float>(); float* const ws_aux = ws->o_aux.as<float>(); uint8_t* const ws_desc = ws->o_desc.as<uint8_t>();
  static const bool use_graph = getenv("TODHIP_ORB_NO_GRAPH") == nullptr;
  if (!use_graph) {
    record_stages(ws->plan, ws, ws_mask, st);
  } else {
    const OrbGraph::Key key = {P.H, P.W, par.n_features, P.n_levels, P.cap, P.F, par.scale_factor, ws_xy, ws_aux, ws_desc, ws->pyr.p, ws_mask, ws->taps.p};
    if (!ws->graph.matches(key)) {
      TOD_HIP(ws->graph.begin_capture(st));
      record_stages(ws->plan, ws, ws_mask, st);
      TOD_HIP(ws->graph.end_capture(st, key));
    }
    TOD_HIP(ws->graph.launch(st));
  }
  uint32_t* d_totals = ctl + P.totals_off;
  hipLaunchKernelGGL(copy_out_kernel, grid(P.copy_out), dim3(256), 0, st, ctl + P.level_counts_off, P.n_levels, P.cap, ws_xy, ws_aux,
                     reinterpret_cast<const uint32_t*>(ws_desc), out.kp_xy, out.kp_aux, reinterpret_cast<uint32_t*>(out.desc), d_totals);
  TOD_HIP(hipGetLastError());
  uint32_t* h_totals = ws->h_out.as<uint32_t>();
  TOD_HIP(hipMemcpyAsync(h_totals, d_totals, (size_t)P.F * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  TOD_HIP(hipStreamSynchronize(st));
  for (uint32_t f = 0; f < P.F; ++f) out.n_out[f] = std::min(h_totals[f], P.cap);
  return TODHIP_OK;
}

}  // namespace

// used by train.hip: ORB with a level-0 mask on device-resident inputs
int tod_orb_device(todhip_ctx* ctx, const uint8_t* d_gray, const uint8_t* d_mask, uint32_t H, uint32_t W, uint32_t stride,
                   uint32_t n_features, uint32_t n_levels, float scale_factor, const int8_t* pattern, float* d_kp_xy,
                   float* d_kp_aux, uint8_t* d_desc, uint32_t cap, uint32_t* n_out) {
  return orb_device(ctx, {d_gray, 0, d_mask, 1, H, W, stride}, {n_features, n_levels, scale_factor, pattern},
                    {d_kp_xy, d_kp_aux, d_desc, cap, n_out});
}

// used by train.hip: F masked views in one call (frame f at d_gray + f * gray_fs, its mask at d_mask + f * H * W, its keypoints at
// row f * cap of the three arrays, their number in n_out[f])
int tod_orb_batch_device(todhip_ctx* ctx, const uint8_t* d_gray, size_t gray_fs, const uint8_t* d_mask, uint32_t F, uint32_t H,
                         uint32_t W, uint32_t stride, uint32_t n_features, uint32_t n_levels, float scale_factor, const int8_t* pattern,
                         float* d_kp_xy, float* d_kp_aux, uint8_t* d_desc, uint32_t cap, uint32_t* n_out) {
  return orb_device(ctx, {d_gray, gray_fs, d_mask, F, H, W, stride}, {n_features, n_levels, scale_factor, pattern},
                    {d_kp_xy, d_kp_aux, d_desc, cap, n_out});
}

// orb_stages.h
int tod_orb_stage_host_view(todhip_ctx* ctx, const uint8_t* gray, const uint8_t* mask, uint32_t H, uint32_t W, uint32_t stride,
                            const uint8_t** d_gray, const uint8_t** d_mask) {
  OrbWs* ws = tod_ws<OrbWs>(ctx);
  const size_t img_bytes = (size_t)H * W;
  TOD_HIP(ws->in_img.reserve(mask ? 2 * img_bytes : img_bytes));       // the mask rides behind the image
  uint8_t* const d = ws->in_img.as<uint8_t>();
  if (stride == W)
    TOD_HIP(hipMemcpyAsync(d, gray, img_bytes, hipMemcpyHostToDevice, ctx->stream));
  else
    TOD_HIP(hipMemcpy2DAsync(d, W, gray, stride, W, H, hipMemcpyHostToDevice, ctx->stream));
  if (mask) TOD_HIP(hipMemcpy2DAsync(d + img_bytes, W, mask, stride, W, H, hipMemcpyHostToDevice, ctx->stream));
  *d_gray = d; *d_mask = mask ? d + img_bytes : nullptr;
  return TODHIP_OK;
}

// orb_stages.h: one frame through the detection stages, and where they left their results
int tod_orb_stages(todhip_ctx* ctx, const uint8_t* d_gray, const uint8_t* d_mask, uint32_t H, uint32_t W, uint32_t stride,
                   uint32_t n_features, uint32_t n_levels, float scale_factor, Stages* out) {
  OrbWs* ws = tod_ws<OrbWs>(ctx);
  TOD_HIP(ws->kp_xy.reserve((size_t)n_features * 8)); TOD_HIP(ws->kp_aux.reserve((size_t)n_features * 16));
  TOD_HIP(ws->desc.reserve((size_t)n_features * 32));
  uint32_t n = 0;
  const int rc = orb_device(ctx, {d_gray, 0, d_mask, 1, H, W, stride}, {n_features, n_levels, scale_factor, nullptr},
                            {ws->kp_xy.as<float>(), ws->kp_aux.as<float>(), ws->desc.as<uint8_t>(), n_features, &n});
  if (rc != TODHIP_OK) return rc;
  const OrbPlan& P = ws->plan;
  out->T = P.tab;
  out->blur = ws->blur.as<uint8_t>(); out->sel = ws->sel2.as<Cand>();
  out->level_counts = ws->small.as<uint32_t>() + P.level_counts_off;
  out->fs = P.px; out->sel_fs = P.sel2_cap; out->want_max = P.want_max; out->n = n;
  disc_umax(out->umax);
  return TODHIP_OK;
}

extern "C" {

// d_mask: frame f's mask at d_mask + f * H * W (packed, whatever the frames' strides are), or NULL. orb_device copies the masks
// into the workspace (one launch for all frames) and fast_nms_kernel offsets that copy per frame; the graph cache's key holds the
// copy's address or NULL, so a masked and an unmasked call of one shape never replay each other's sequence.
int todhip_orb_batch_device_masked(todhip_ctx* ctx, const void* d_gray, const void* d_mask, uint32_t n_frames, uint64_t frame_stride,
                                   uint32_t H, uint32_t W, uint32_t stride, uint32_t n_features, uint32_t n_levels, float scale_factor,
                                   const int8_t* pattern, void* d_kp_xy, void* d_kp_aux, void* d_desc, uint32_t cap, uint32_t* n_out) {
  if (!ctx || !d_gray || !d_kp_xy || !d_kp_aux || !d_desc || !n_out || stride < W || n_frames == 0) return TODHIP_EINVAL;
  if (n_frames > 1 && frame_stride < (uint64_t)H * stride) return TODHIP_EINVAL;
  TOD_HIP(hipSetDevice(ctx->device));
  for (uint32_t f = 0; f < n_frames; ++f) n_out[f] = 0;
  return orb_device(ctx, {reinterpret_cast<const uint8_t*>(d_gray), (size_t)frame_stride, reinterpret_cast<const uint8_t*>(d_mask), n_frames, H, W, stride},
                    {n_features, n_levels, scale_factor, pattern},
                    {reinterpret_cast<float*>(d_kp_xy), reinterpret_cast<float*>(d_kp_aux), reinterpret_cast<uint8_t*>(d_desc), cap, n_out});
}

int todhip_orb_batch_device(todhip_ctx* ctx, const void* d_gray, uint32_t n_frames, uint64_t frame_stride, uint32_t H, uint32_t W,
                            uint32_t stride, uint32_t n_features, uint32_t n_levels, float scale_factor, const int8_t* pattern,
                            void* d_kp_xy, void* d_kp_aux, void* d_desc, uint32_t cap, uint32_t* n_out) {
  return todhip_orb_batch_device_masked(ctx, d_gray, nullptr, n_frames, frame_stride, H, W, stride, n_features, n_levels, scale_factor,
                                        pattern, d_kp_xy, d_kp_aux, d_desc, cap, n_out);
}

// one frame: the batch of one, the capacity arrives in *n_out
int todhip_orb_device(todhip_ctx* ctx, const void* d_gray, uint32_t H, uint32_t W, uint32_t stride, uint32_t n_features,
                      uint32_t n_levels, float scale_factor, const int8_t* pattern, void* d_kp_xy, void* d_kp_aux,
                      void* d_desc, uint32_t* n_out) {
  if (!n_out) return TODHIP_EINVAL;
  return todhip_orb_batch_device(ctx, d_gray, 1, 0, H, W, stride, n_features, n_levels, scale_factor, pattern, d_kp_xy, d_kp_aux, d_desc,
                                 *n_out, n_out);
}

int todhip_orb_masked(todhip_ctx* ctx, const uint8_t* gray, const uint8_t* mask, uint32_t H, uint32_t W, uint32_t stride,
                      uint32_t n_features, uint32_t n_levels, float scale_factor, const int8_t* pattern, float* kp_xy, float* kp_aux,
                      uint8_t* desc, uint32_t* n_out) {
  if (!ctx || !gray || !kp_xy || !kp_aux || !desc || !n_out || stride < W) return TODHIP_EINVAL;
  TOD_HIP(hipSetDevice(ctx->device));
  OrbWs* ws = tod_ws<OrbWs>(ctx);
  const uint32_t cap = *n_out;
  *n_out = 0;
  if (const int bad = check_args(1, H, W, n_features, n_levels, scale_factor, cap)) return bad;   // before anything is read
  if (const int bad = check_pattern(pattern)) return bad;
  // the outputs land in pinned host memory, written by the last kernel itself (56 B per keypoint over PCIe): no device-to-host
  // copies and no second synchronization behind orb_device's own
  TOD_HIP(ws->h_kp.reserve((size_t)cap * 56 + 64));
  float* const p_xy = ws->h_kp.as<float>(); float* const p_aux = p_xy + (size_t)cap * 2;
  uint8_t* const p_desc = reinterpret_cast<uint8_t*>(p_aux + (size_t)cap * 4);
  const uint8_t *d_gray = nullptr, *d_mask = nullptr;
  if (const int rc = tod_orb_stage_host_view(ctx, gray, mask, H, W, stride, &d_gray, &d_mask)) return rc;
  uint32_t n = 0;
  const int rc = orb_device(ctx, {d_gray, 0, d_mask, 1, H, W, W}, {n_features, n_levels, scale_factor, pattern},
                            {p_xy, p_aux, p_desc, cap, &n});         // (synchronizes the stream before it returns)
  if (rc != TODHIP_OK) return rc;
  if (n) {
    std::memcpy(kp_xy, p_xy, (size_t)n * 8); std::memcpy(kp_aux, p_aux, (size_t)n * 16); std::memcpy(desc, p_desc, (size_t)n * 32);
  }
  *n_out = n;
  return TODHIP_OK;
}

int todhip_orb(todhip_ctx* ctx, const uint8_t* gray, uint32_t H, uint32_t W, uint32_t stride, uint32_t n_features,
               uint32_t n_levels, float scale_factor, const int8_t* pattern, float* kp_xy, float* kp_aux, uint8_t* desc,
               uint32_t* n_out) {
  return todhip_orb_masked(ctx, gray, nullptr, H, W, stride, n_features, n_levels, scale_factor, pattern, kp_xy, kp_aux, desc, n_out);
}

}  // extern "C"
