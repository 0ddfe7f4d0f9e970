// todhip_pipeline (include/todhip.h): ORB -> matcher -> verifier on batches of frames behind submit / wait, with the stage overlap
// of tod_amd/pipeline.py's StagePipeline as bench.py drives it -- in C++, on plain HIP streams and events and std::thread. It calls
// the stages only through their public entry points (todhip_orb_batch_device[_masked], todhip_match_device,
// todhip_verify_batch_device_depth[_rescaled]) and adds two kernels of its own: the colour conversion in front of ORB and the
// padding rule behind the matcher.
//
// A ticket owns one ring slot from submit to wait; the slot holds every buffer of its step. Step i (ticket i + 1) goes through ORB
// worker i % orb_workers, the one matcher thread (in ticket order) and verifier worker i % verify_workers; each worker thread is the
// only caller of its context, so one call in flight per context holds by construction. One mutex and one condition variable carry all
// hand-overs: there are three per step of several milliseconds.
#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <thread>
#include <vector>

#include "ctx.h"
#include "depth_rescale.h"
#include "orb_plan.h"

namespace {

constexpr uint32_t kMaxFrames = 64, kMaxWorkers = 8, kMaxRing = 16;

// ---- device code -----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t gray_of(uint32_t b, uint32_t g, uint32_t r) {
  return (1868u * b + 9617u * g + 4899u * r + 8192u) >> 14;        // adapter/ecto_cells.hpp bgr_to_gray
}

// BGR8 / BGRA8 -> the gray frames ORB reads; frame = blockIdx.y. A bandwidth kernel: a thread owns a group of P pixels whose source
// bytes are whole 16-byte words (BGRA: 4 pixels = one word, BGR: 16 pixels = three) and loads them as such where the address allows;
// rows whose stride breaks the alignment, and the W % P pixels at the end of a row, go byte by byte.
template <int CH>
__global__ __launch_bounds__(256) void bgr_to_gray_kernel(const uint8_t* __restrict__ src, size_t src_fs, uint32_t src_stride,
                                                          uint8_t* __restrict__ gray, size_t gray_fs, uint32_t gray_stride, uint32_t H,
                                                          uint32_t W) {
  constexpr uint32_t P = CH == 4 ? 4u : 16u, NW = CH * P / 4u;
  const uint32_t full = W / P, groups = full + (W % P ? 1u : 0u);
  const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
  if (idx >= H * groups) return;
  const uint32_t y = idx / groups, g = idx - y * groups, x0 = g * P;
  const uint8_t* s = src + blockIdx.y * src_fs + (size_t)y * src_stride + (size_t)x0 * CH;
  uint8_t* o = gray + blockIdx.y * gray_fs + (size_t)y * gray_stride + x0;
  if (g < full && (reinterpret_cast<uintptr_t>(s) & 15u) == 0u) {
    uint32_t w[NW];
#pragma unroll
    for (uint32_t i = 0; i < NW / 4u; ++i) {
      const uint4 v = reinterpret_cast<const uint4*>(s)[i];
      w[4 * i] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w;
    }
    uint32_t out[P / 4u] = {};
#pragma unroll
    for (uint32_t p = 0; p < P; ++p) {
      const uint32_t b0 = p * CH, b1 = b0 + 1u, b2 = b0 + 2u;
      const uint32_t yv = gray_of((w[b0 >> 2] >> (8u * (b0 & 3u))) & 255u, (w[b1 >> 2] >> (8u * (b1 & 3u))) & 255u,
                                  (w[b2 >> 2] >> (8u * (b2 & 3u))) & 255u);
      out[p >> 2] |= yv << (8u * (p & 3u));
    }
    if ((reinterpret_cast<uintptr_t>(o) & (P - 1u)) == 0u) {
      if constexpr (P == 4u) *reinterpret_cast<uint32_t*>(o) = out[0];
      else *reinterpret_cast<uint4*>(o) = make_uint4(out[0], out[1], out[2], out[3]);
    } else {
#pragma unroll
      for (uint32_t p = 0; p < P; ++p) o[p] = (uint8_t)(out[p >> 2] >> (8u * (p & 3u)));
    }
    return;
  }
  const uint32_t n = g < full ? P : W - x0;
  for (uint32_t p = 0; p < n; ++p) o[p] = (uint8_t)gray_of(s[p * CH], s[p * CH + 1u], s[p * CH + 2u]);
}

int launch_bgr_to_gray(hipStream_t st, const void* d_src, uint32_t channels, size_t src_fs, uint32_t src_stride, void* d_gray,
                       size_t gray_fs, uint32_t gray_stride, uint32_t F, uint32_t H, uint32_t W) {
  const uint32_t P = channels == 4 ? 4u : 16u, groups = W / P + (W % P ? 1u : 0u);
  const uint64_t threads = (uint64_t)H * groups;
  if (threads > 0x7FFFFFFFull) return TODHIP_EINVAL;
  const dim3 grid((uint32_t)((threads + 255u) / 256u), F);
  if (channels == 4)
    hipLaunchKernelGGL(bgr_to_gray_kernel<4>, grid, dim3(256), 0, st, reinterpret_cast<const uint8_t*>(d_src), src_fs, src_stride,
                       reinterpret_cast<uint8_t*>(d_gray), gray_fs, gray_stride, H, W);
  else
    hipLaunchKernelGGL(bgr_to_gray_kernel<3>, grid, dim3(256), 0, st, reinterpret_cast<const uint8_t*>(d_src), src_fs, src_stride,
                       reinterpret_cast<uint8_t*>(d_gray), gray_fs, gray_stride, H, W);
  return hipGetLastError() == hipSuccess ? TODHIP_OK : TODHIP_EHIP;
}

// todhip.h's padding rule for the batched verifier: a frame with fewer than nq keypoints pads with counts 0. The matcher ran over all
// nq rows of every frame of the ring slot, and the rows behind n_kp[f] hold descriptors of an earlier step. frame = blockIdx.y.
struct FrameCounts { uint32_t n[kMaxFrames]; };
__global__ __launch_bounds__(256) void mask_short_frames_kernel(uint32_t* __restrict__ counts, uint32_t nq, FrameCounts n_kp) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j < nq && j >= n_kp.n[blockIdx.y]) counts[(size_t)blockIdx.y * nq + j] = 0u;
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
using Clock = std::chrono::steady_clock;
double seconds_since(Clock::time_point t) { return std::chrono::duration<double>(Clock::now() - t).count(); }

enum SlotState { kFree, kFilling, kSubmitted, kOrbDone, kMatched, kDone };

struct Slot {
  uint64_t ticket = 0;
  SlotState state = kFree;
  uint32_t n_frames = 0;
  int status = TODHIP_OK;
  bool host_form = false;
  const void* d_frames = nullptr;        // what the stages read: the caller's buffers (device form) or this slot's uploads
  const void* d_depth = nullptr;
  const void* d_masks = nullptr;         // this step's masks, or nullptr: set by every submit, so a slot's earlier masks never reach a later step
  bool host_masks = false;               // the masks are in st_masks and go up with the frames
  DevBuf up_masks; HostBuf st_masks;     // the host form's masks (allocated by the slot's first masked submit)
  DevBuf up_frames, up_depth, gray, kp, aux, desc, counts, matches, xyz;
  HostBuf st_frames, st_depth, h_kp;     // pinned: staging of the host form, the keypoints on their way out
  hipEvent_t matched = nullptr;          // recorded behind the matcher's work of the step
  uint32_t n_kp[kMaxFrames] = {};
  std::vector<todhip_pose> poses;
  std::vector<uint32_t> pose_ptr;
  std::unique_ptr<uint32_t[]> inl;       // (not a vector: its pages are touched only as far as poses fill them)
  uint32_t n_poses = 0, n_inl = 0;
};

}  // namespace

struct todhip_pipeline {
  todhip_pipeline_params prm = {};
  int device = 0;
  uint32_t B = 0, NO = 0, NV = 0, D = 0, nq = 0;
  size_t frame_bytes = 0, depth_bytes = 0, px = 0;
  // todhip_pipeline_set_depth_size: written only while every slot is free. depth_rescaled: a depth image is dH x dW and the verifier
  // looks rescale_depth's result up at the keypoints; otherwise it has the image's size
  uint32_t dH = 0, dW = 0; int depth_nearest = 0; bool depth_rescaled = false;
  uint32_t inl_cap = 0, pose_cap = 0;

  todhip_ctx* mctx = nullptr;
  std::vector<todhip_ctx*> octx, vctx;
  std::vector<hipStream_t> streams;      // matcher, ORB workers, verifier workers: all from tod_stream_create
  std::vector<Slot> slots;
  std::vector<float> spans;
  uint32_t n_objs = 0;
  todhip_rng rng0;
  int8_t pattern[1024] = {};             // todhip_pipeline_set_pattern: written only while every slot is free
  bool has_pattern = false;
  bool cross_check = false;              // todhip_pipeline_set_cross_check: written only while every slot is free

  std::mutex mu;                         // slot states, tickets, stats, dead, stop
  std::condition_variable cv;
  std::mutex mctx_mu;                    // the matcher context: its thread's calls against todhip_pipeline_get_stats
  uint64_t next_ticket = 1;
  bool dead = false, stop = false;
  todhip_pipeline_stats stats = {};
  std::vector<std::thread> threads;

  Slot* find(uint64_t ticket) {
    for (Slot& s : slots)
      if (s.state != kFree && s.ticket == ticket) return &s;
    return nullptr;
  }
  // the slot of step `step` once it has reached `want`; nullptr when the pipeline is stopping
  Slot* take(std::unique_lock<std::mutex>& lk, uint64_t step, SlotState want) {
    Slot* s = nullptr;
    cv.wait(lk, [&] { return stop || ((s = find(step + 1)) && s->state == want); });
    return stop ? nullptr : s;
  }
  void pass(Slot* s, int rc, SlotState next, double todhip_pipeline_stats::*stage_s, Clock::time_point t0) {
    std::lock_guard<std::mutex> lk(mu);
    if (rc != TODHIP_OK && s->status == TODHIP_OK) s->status = rc;
    if (rc == TODHIP_EHIP) dead = true;
    stats.*stage_s += seconds_since(t0);
    s->state = next;
    cv.notify_all();
  }

  int orb_step(Slot* s, uint32_t w);
  int match_step(Slot* s);
  int verify_step(Slot* s, uint32_t w);
  void orb_worker(uint32_t w);
  void match_worker();
  void verify_worker(uint32_t w);
  int reserve_host_form(Slot* s, bool masks);
  int submit(const void* frames, const void* masks, const void* depth, uint32_t n_frames, uint64_t* ticket, bool host_form);
  int set_depth_size(uint32_t dH_in, uint32_t dW_in, int nearest);
  int db_load(const todhip_object* objs, uint32_t n_objs_in, uint32_t desc_bytes, bool device_src);
};

#define PIPE_HIP(call) do { if ((call) != hipSuccess) return TODHIP_EHIP; } while (0)

int todhip_pipeline::orb_step(Slot* s, uint32_t w) {
  hipStream_t st = streams[1 + w];
  const uint32_t n = s->n_frames;
  if (s->host_form) {
    PIPE_HIP(hipMemcpyAsync(s->up_frames.p, s->st_frames.p, n * frame_bytes, hipMemcpyHostToDevice, st));
    PIPE_HIP(hipMemcpyAsync(s->up_depth.p, s->st_depth.p, n * depth_bytes, hipMemcpyHostToDevice, st));   // complete when ORB returns
    s->d_frames = s->up_frames.p; s->d_depth = s->up_depth.p;
    if (s->host_masks) {
      PIPE_HIP(hipMemcpyAsync(s->up_masks.p, s->st_masks.p, n * px, hipMemcpyHostToDevice, st));
      s->d_masks = s->up_masks.p;
    }
  }
  const void* gray = s->d_frames;
  if (prm.frame_format != TODHIP_FRAME_GRAY8) {
    const uint32_t ch = prm.frame_format == TODHIP_FRAME_BGRA8 ? 4u : 3u;
    const int rc = launch_bgr_to_gray(st, s->d_frames, ch, frame_bytes, prm.W * ch, s->gray.p, px, prm.W, n, prm.H, prm.W);
    if (rc != TODHIP_OK) return rc;
    gray = s->gray.p;
  }
  return todhip_orb_batch_device_masked(octx[w], gray, s->d_masks, n, px, prm.H, prm.W, prm.W, prm.n_features, prm.n_levels,
                                        prm.scale_factor, has_pattern ? pattern : nullptr, s->kp.p, s->aux.p, s->desc.p, nq, s->n_kp);
}

int todhip_pipeline::match_step(Slot* s) {
  std::lock_guard<std::mutex> lk(mctx_mu);
  const uint32_t n = s->n_frames;
  const int rc = todhip_match_device(mctx, s->desc.p, n * nq, prm.k, prm.radius, s->counts.p, s->matches.p, s->xyz.p);
  if (rc != TODHIP_OK) return rc;
  FrameCounts fc = {};
  bool any_short = false;
  for (uint32_t f = 0; f < n; ++f) { fc.n[f] = s->n_kp[f]; any_short = any_short || s->n_kp[f] < nq; }
  if (any_short) {
    hipLaunchKernelGGL(mask_short_frames_kernel, dim3((nq + 255u) / 256u, n), dim3(256), 0, streams[0], s->counts.as<uint32_t>(), nq, fc);
    PIPE_HIP(hipGetLastError());
  }
  if (cross_check) {
    // per frame, among its n_kp keypoints: the rows behind n_kp[f] hold an earlier step's descriptors and do not compete (the
    // matcher's stream is the context's, and up to kMaxFrames frame counts travel as a kernel argument: no copy, no wait)
    const int rc2 = todhip_cross_check_device(mctx, s->desc.p, n * nq, nq, s->n_kp, prm.k, s->counts.p, s->matches.p, s->xyz.p);
    if (rc2 != TODHIP_OK) return rc2;
  }
  PIPE_HIP(hipEventRecord(s->matched, streams[0]));
  return TODHIP_OK;
}

int todhip_pipeline::verify_step(Slot* s, uint32_t w) {
  hipStream_t st = streams[1 + NO + w];
  const uint32_t n = s->n_frames;
  PIPE_HIP(hipStreamWaitEvent(st, s->matched, 0));                 // the device-side edge from the matcher
  PIPE_HIP(hipMemcpyAsync(s->h_kp.p, s->kp.p, (size_t)n * nq * 2 * sizeof(float), hipMemcpyDeviceToHost, st));
  todhip_rng rngs[kMaxFrames];
  for (uint32_t f = 0; f < n; ++f) rngs[f] = rng0;
  s->n_poses = pose_cap; s->n_inl = inl_cap;
  const int rc = depth_rescaled
      ? todhip_verify_batch_device_depth_rescaled(vctx[w], n, s->kp.p, nq, s->d_depth, prm.depth_is_u16, dH, dW, depth_nearest, prm.H,
                                                  prm.W, prm.K9, s->counts.p, s->matches.p, s->xyz.p, prm.k, spans.data(), n_objs,
                                                  &prm.verify, rngs, s->poses.data(), &s->n_poses, s->pose_ptr.data(), s->inl.get(),
                                                  &s->n_inl)
      : todhip_verify_batch_device_depth(vctx[w], n, s->kp.p, nq, s->d_depth, prm.depth_is_u16, prm.H, prm.W, prm.K9,
                                         s->counts.p, s->matches.p, s->xyz.p, prm.k, spans.data(), n_objs, &prm.verify, rngs,
                                         s->poses.data(), &s->n_poses, s->pose_ptr.data(), s->inl.get(), &s->n_inl);
  if (rc != TODHIP_OK) return rc;
  PIPE_HIP(hipStreamSynchronize(st));                              // the keypoint copy (the verifier returns early on an empty step)
  return TODHIP_OK;
}

void todhip_pipeline::orb_worker(uint32_t w) {
  (void)hipSetDevice(device);
  for (uint64_t step = w;; step += NO) {
    std::unique_lock<std::mutex> lk(mu);
    Slot* s = take(lk, step, kSubmitted);
    if (!s) return;
    const bool run = !dead && s->status == TODHIP_OK;
    lk.unlock();
    const Clock::time_point t0 = Clock::now();
    pass(s, run ? orb_step(s, w) : TODHIP_OK, kOrbDone, &todhip_pipeline_stats::orb_s, t0);
  }
}

void todhip_pipeline::match_worker() {
  (void)hipSetDevice(device);
  for (uint64_t step = 0;; ++step) {
    std::unique_lock<std::mutex> lk(mu);
    Slot* s = take(lk, step, kOrbDone);
    if (!s) return;
    const bool run = !dead && s->status == TODHIP_OK;
    lk.unlock();
    const Clock::time_point t0 = Clock::now();
    pass(s, run ? match_step(s) : TODHIP_OK, kMatched, &todhip_pipeline_stats::match_issue_s, t0);
  }
}

void todhip_pipeline::verify_worker(uint32_t w) {
  (void)hipSetDevice(device);
  for (uint64_t step = w;; step += NV) {
    std::unique_lock<std::mutex> lk(mu);
    Slot* s = take(lk, step, kMatched);
    if (!s) return;
    bool run = !dead && s->status == TODHIP_OK;
    lk.unlock();
    int rc = TODHIP_OK;
    // host side too, so that the stage time is the verifier's own (as StagePipeline does)
    if (run && hipEventSynchronize(s->matched) != hipSuccess) { rc = TODHIP_EHIP; run = false; }
    const Clock::time_point t0 = Clock::now();
    if (run) rc = verify_step(s, w);
    if (run && rc == TODHIP_OK) {
      std::lock_guard<std::mutex> g(mu);
      stats.steps += 1; stats.frames += s->n_frames; stats.poses += s->n_poses;
      for (uint32_t f = 0; f < s->n_frames; ++f) stats.keypoints += s->n_kp[f];
    }
    pass(s, rc, kDone, &todhip_pipeline_stats::verify_s, t0);
  }
}

// (every reserve returns at once when the buffer is large enough; the depth pair follows todhip_pipeline_set_depth_size, the mask
// pair exists from the slot's first masked step on)
int todhip_pipeline::reserve_host_form(Slot* s, bool masks) {
  PIPE_HIP(s->st_frames.reserve(B * frame_bytes)); PIPE_HIP(s->st_depth.reserve(B * depth_bytes));
  PIPE_HIP(s->up_frames.reserve(B * frame_bytes)); PIPE_HIP(s->up_depth.reserve(B * depth_bytes));
  if (masks) { PIPE_HIP(s->st_masks.reserve(B * px)); PIPE_HIP(s->up_masks.reserve(B * px)); }
  return TODHIP_OK;
}

int todhip_pipeline::submit(const void* frames, const void* masks, const void* depth, uint32_t n_frames, uint64_t* ticket, bool host_form) {
  if (!frames || !depth || !ticket || n_frames == 0 || n_frames > B) return TODHIP_EINVAL;
  Slot* s = nullptr;
  {
    std::lock_guard<std::mutex> lk(mu);
    if (dead) return TODHIP_EHIP;
    for (Slot& c : slots)
      if (c.state == kFree) { s = &c; break; }
    if (!s) return TODHIP_EBUSY;
    s->state = kFilling; s->ticket = next_ticket++;
    s->n_frames = n_frames; s->status = TODHIP_OK; s->host_form = host_form;
    s->d_frames = frames; s->d_depth = depth;
    s->d_masks = host_form ? nullptr : masks; s->host_masks = host_form && masks;
    s->n_poses = s->n_inl = 0;
  }
  int rc = TODHIP_OK;
  if (host_form) {                                                 // outside the lock: tens of megabytes per step
    rc = hipSetDevice(device) == hipSuccess ? reserve_host_form(s, masks != nullptr) : TODHIP_EHIP;
    if (rc == TODHIP_OK) {
      std::memcpy(s->st_frames.p, frames, n_frames * frame_bytes);
      std::memcpy(s->st_depth.p, depth, n_frames * depth_bytes);
      if (masks) std::memcpy(s->st_masks.p, masks, n_frames * px);
    }
  }
  std::lock_guard<std::mutex> lk(mu);
  if (rc != TODHIP_OK) { s->status = rc; dead = dead || rc == TODHIP_EHIP; }   // travels through the stages untouched; wait returns it
  *ticket = s->ticket;
  s->state = kSubmitted;
  cv.notify_all();
  return TODHIP_OK;
}

int todhip_pipeline::set_depth_size(uint32_t dH_in, uint32_t dW_in, int nearest) {
  tod::RescaleGeom g = {};
  const bool own = dH_in == 0 && dW_in == 0;               // the image's size again
  if (!own && (dH_in == 0 || dW_in == 0 || dH_in > 16384 || dW_in > 16384 || !tod::rescale_geometry(dH_in, dW_in, prm.H, prm.W, nearest, &g)))
    return TODHIP_EINVAL;
  std::lock_guard<std::mutex> lk(mu);
  if (dead) return TODHIP_EHIP;
  for (const Slot& s : slots)
    if (s.state != kFree) return TODHIP_EBUSY;
  dH = own ? prm.H : dH_in; dW = own ? prm.W : dW_in;
  depth_nearest = nearest ? 1 : 0;
  depth_rescaled = !own && g.mode != tod::RescaleGeom::kEqual;
  depth_bytes = (size_t)dH * dW * (prm.depth_is_u16 ? 2u : 4u);
  return TODHIP_OK;
}

int todhip_pipeline::db_load(const todhip_object* objs, uint32_t n_objs_in, uint32_t desc_bytes, bool device_src) {
  if (desc_bytes != 32 || (!objs && n_objs_in)) return TODHIP_EINVAL;
  std::lock_guard<std::mutex> lk(mu);
  if (dead) return TODHIP_EHIP;
  for (const Slot& s : slots)
    if (s.state != kFree) return TODHIP_EBUSY;
  std::lock_guard<std::mutex> g(mctx_mu);
  std::vector<float> sp(std::max(n_objs_in, 1u), 0.f);
  const int rc = device_src ? todhip_db_load_device(mctx, objs, n_objs_in, 32, 0, 1, sp.data())
                            : todhip_db_load(mctx, objs, n_objs_in, 32, 0, 1, sp.data());
  if (rc == TODHIP_EHIP) dead = true;
  if (rc != TODHIP_OK) return rc;
  spans.swap(sp); n_objs = n_objs_in;
  return TODHIP_OK;
}

static void pipeline_teardown(todhip_pipeline* p) {
  (void)hipSetDevice(p->device);
  for (todhip_ctx* c : p->vctx) todhip_destroy(c);
  for (todhip_ctx* c : p->octx) todhip_destroy(c);
  todhip_destroy(p->mctx);
  for (Slot& s : p->slots)
    if (s.matched) (void)hipEventDestroy(s.matched);
  p->slots.clear();                                                // the buffers, while the runtime is certainly up
  for (hipStream_t st : p->streams) (void)hipStreamDestroy(st);
  delete p;
}

extern "C" {

int todhip_pipeline_default_params(todhip_pipeline_params* out) {
  if (!out) return TODHIP_EINVAL;
  std::memset(out, 0, sizeof(*out));
  out->struct_size = (uint32_t)sizeof(*out);
  out->frames_per_step = 32; out->H = 480; out->W = 640;
  out->frame_format = TODHIP_FRAME_GRAY8;
  out->n_features = 1000; out->n_levels = 3; out->scale_factor = 1.2f;
  out->k = 5; out->radius = 55;
  out->verify.min_inliers = 15; out->verify.n_ransac_iterations = 1000; out->verify.sensor_error = 0.01f;
  out->rng_seed = 1;
  out->orb_workers = 1; out->verify_workers = 2; out->ring_depth = 4; out->max_poses_per_frame = 64;
  return TODHIP_OK;
}

int todhip_pipeline_create(int device, const todhip_pipeline_params* in, todhip_pipeline** out) {
  if (!out) return TODHIP_EINVAL;
  *out = nullptr;
  if (!in || in->struct_size != sizeof(todhip_pipeline_params)) return TODHIP_EINVAL;
  todhip_pipeline_params q = *in;
  if (q.orb_workers == 0) q.orb_workers = 1;
  if (q.verify_workers == 0) q.verify_workers = 2;
  if (q.ring_depth == 0) q.ring_depth = q.verify_workers + 2;
  if (q.max_poses_per_frame == 0) q.max_poses_per_frame = 64;
  if (q.rng_seed == 0) q.rng_seed = 1;
  if (q.frames_per_step == 0 || q.frames_per_step > kMaxFrames || q.H < 8 || q.W < 8 || q.H > 16384 || q.W > 16384) return TODHIP_EINVAL;
  if (q.frame_format < TODHIP_FRAME_GRAY8 || q.frame_format > TODHIP_FRAME_BGRA8) return TODHIP_EINVAL;
  if (q.n_features == 0 || q.n_features > 65536u || q.n_levels == 0 || !(q.scale_factor > 1.f)) return TODHIP_EINVAL;
  if (q.k == 0 || q.k > 8 || q.radius == 0) return TODHIP_EINVAL;
  if (q.orb_workers > kMaxWorkers || q.verify_workers > kMaxWorkers || q.ring_depth > kMaxRing || q.ring_depth <= q.verify_workers)
    return TODHIP_EINVAL;
  if (q.max_poses_per_frame > 4096u) return TODHIP_EINVAL;
  q.depth_is_u16 = q.depth_is_u16 ? 1 : 0;
  if (hipSetDevice(device) != hipSuccess) return TODHIP_EHIP;

  todhip_pipeline* p = new (std::nothrow) todhip_pipeline();
  if (!p) return TODHIP_ENOMEM;
  p->prm = q; p->device = device;
  p->B = q.frames_per_step; p->NO = q.orb_workers; p->NV = q.verify_workers; p->D = q.ring_depth; p->nq = q.n_features;
  p->px = (size_t)q.H * q.W;
  p->frame_bytes = p->px * (q.frame_format == TODHIP_FRAME_GRAY8 ? 1u : q.frame_format == TODHIP_FRAME_BGR8 ? 3u : 4u);
  p->depth_bytes = p->px * (q.depth_is_u16 ? 2u : 4u);
  p->dH = q.H; p->dW = q.W;
  p->pose_cap = p->B * q.max_poses_per_frame;
  const uint64_t inl = (uint64_t)p->pose_cap * p->nq;
  p->inl_cap = (uint32_t)std::min<uint64_t>(inl, 0x40000000ull);
  todhip_rng_seed(&p->rng0, q.rng_seed);

  int rc = TODHIP_OK;
  auto add_ctx = [&](int kind, todhip_ctx** c) {
    hipStream_t st = nullptr;
    if (tod_stream_create(&st, device, kind) != hipSuccess) { rc = TODHIP_EHIP; return; }
    p->streams.push_back(st);
    rc = todhip_create(device, st, c);
  };
  add_ctx(TODHIP_STREAM_THROUGHPUT, &p->mctx);
  p->octx.assign(p->NO, nullptr); p->vctx.assign(p->NV, nullptr);
  for (uint32_t w = 0; w < p->NO && rc == TODHIP_OK; ++w) add_ctx(TODHIP_STREAM_LATENCY, &p->octx[w]);
  for (uint32_t w = 0; w < p->NV && rc == TODHIP_OK; ++w) add_ctx(TODHIP_STREAM_LATENCY, &p->vctx[w]);

  std::vector<Slot> ring(p->D);
  p->slots.swap(ring);
  const size_t rows = (size_t)p->B * p->nq;
  auto dev = [&](DevBuf& b, size_t bytes) {                        // zeroed: the first step's spare rows are defined too
    if (rc != TODHIP_OK) return;
    if (b.reserve(bytes) != hipSuccess || hipMemset(b.p, 0, bytes) != hipSuccess) rc = TODHIP_EHIP;
  };
  for (Slot& s : p->slots) {
    if (rc != TODHIP_OK) break;
    if (q.frame_format != TODHIP_FRAME_GRAY8) dev(s.gray, p->B * p->px);
    dev(s.kp, rows * 8); dev(s.aux, rows * 16); dev(s.desc, rows * 32);
    dev(s.counts, rows * 4); dev(s.matches, rows * q.k * sizeof(todhip_dmatch)); dev(s.xyz, rows * q.k * 12);
    if (rc == TODHIP_OK && s.h_kp.reserve(rows * 8) != hipSuccess) rc = TODHIP_EHIP;
    if (rc == TODHIP_OK && hipEventCreateWithFlags(&s.matched, hipEventDisableTiming) != hipSuccess) rc = TODHIP_EHIP;
    s.poses.resize(p->pose_cap); s.pose_ptr.assign(p->B + 1, 0u);
    s.inl.reset(new (std::nothrow) uint32_t[std::max(p->inl_cap, 1u)]);
    if (!s.inl) rc = TODHIP_ENOMEM;
  }
  if (rc == TODHIP_OK && hipDeviceSynchronize() != hipSuccess) rc = TODHIP_EHIP;
  if (rc != TODHIP_OK) { pipeline_teardown(p); return rc; }
  for (uint32_t w = 0; w < p->NO; ++w) p->threads.emplace_back(&todhip_pipeline::orb_worker, p, w);
  p->threads.emplace_back(&todhip_pipeline::match_worker, p);
  for (uint32_t w = 0; w < p->NV; ++w) p->threads.emplace_back(&todhip_pipeline::verify_worker, p, w);
  *out = p;
  return TODHIP_OK;
}

void todhip_pipeline_destroy(todhip_pipeline* p) {
  if (!p) return;
  {
    std::unique_lock<std::mutex> lk(p->mu);
    p->cv.wait(lk, [&] {                                           // every submitted step runs to its end (a dead pipeline's pass through)
      for (const Slot& s : p->slots)
        if (s.state != kFree && s.state != kDone) return false;
      return true;
    });
    p->stop = true;
    p->cv.notify_all();
  }
  for (std::thread& t : p->threads) t.join();
  pipeline_teardown(p);
}

todhip_ctx* todhip_pipeline_matcher(todhip_pipeline* p) { return p ? p->mctx : nullptr; }

int todhip_pipeline_db_load(todhip_pipeline* p, const todhip_object* objs, uint32_t n_objs, uint32_t desc_bytes) {
  return p ? p->db_load(objs, n_objs, desc_bytes, false) : TODHIP_EINVAL;
}
int todhip_pipeline_db_load_device(todhip_pipeline* p, const todhip_object* objs, uint32_t n_objs, uint32_t desc_bytes) {
  return p ? p->db_load(objs, n_objs, desc_bytes, true) : TODHIP_EINVAL;
}

int todhip_pipeline_set_pattern(todhip_pipeline* p, const int8_t* pattern) {
  if (!p) return TODHIP_EINVAL;
  if (const int bad = tod_orb::check_pattern(pattern)) return bad;     // here, not at the next submit: the pattern in use stays
  std::lock_guard<std::mutex> lk(p->mu);
  if (p->dead) return TODHIP_EHIP;
  for (const Slot& s : p->slots)
    if (s.state != kFree) return TODHIP_EBUSY;
  p->has_pattern = pattern != nullptr;
  if (pattern) std::memcpy(p->pattern, pattern, sizeof(p->pattern));
  return TODHIP_OK;
}

int todhip_pipeline_set_cross_check(todhip_pipeline* p, int enable) {
  if (!p) return TODHIP_EINVAL;
  std::lock_guard<std::mutex> lk(p->mu);
  if (p->dead) return TODHIP_EHIP;
  for (const Slot& s : p->slots)
    if (s.state != kFree) return TODHIP_EBUSY;
  p->cross_check = enable != 0;
  return TODHIP_OK;
}

int todhip_pipeline_select_objects(todhip_pipeline* p, const uint32_t* ids, uint32_t n_ids) {
  if (!p) return TODHIP_EINVAL;
  std::lock_guard<std::mutex> lk(p->mu);
  if (p->dead) return TODHIP_EHIP;
  for (const Slot& s : p->slots)
    if (s.state != kFree) return TODHIP_EBUSY;
  std::lock_guard<std::mutex> g(p->mctx_mu);
  const int rc = todhip_db_select_objects(p->mctx, ids, n_ids);
  if (rc == TODHIP_EHIP) p->dead = true;
  return rc;
}

int todhip_pipeline_submit(todhip_pipeline* p, const uint8_t* frames, const void* depth, uint32_t n_frames, uint64_t* ticket) {
  return p ? p->submit(frames, nullptr, depth, n_frames, ticket, true) : TODHIP_EINVAL;
}
int todhip_pipeline_submit_device(todhip_pipeline* p, const void* d_frames, const void* d_depth, uint32_t n_frames, uint64_t* ticket) {
  return p ? p->submit(d_frames, nullptr, d_depth, n_frames, ticket, false) : TODHIP_EINVAL;
}
int todhip_pipeline_submit_masked(todhip_pipeline* p, const uint8_t* frames, const uint8_t* masks, const void* depth, uint32_t n_frames,
                                  uint64_t* ticket) {
  return p ? p->submit(frames, masks, depth, n_frames, ticket, true) : TODHIP_EINVAL;
}
int todhip_pipeline_submit_masked_device(todhip_pipeline* p, const void* d_frames, const void* d_masks, const void* d_depth,
                                         uint32_t n_frames, uint64_t* ticket) {
  return p ? p->submit(d_frames, d_masks, d_depth, n_frames, ticket, false) : TODHIP_EINVAL;
}
int todhip_pipeline_set_depth_size(todhip_pipeline* p, uint32_t dH, uint32_t dW, int nearest) {
  return p ? p->set_depth_size(dH, dW, nearest) : TODHIP_EINVAL;
}

int todhip_pipeline_wait(todhip_pipeline* p, uint64_t ticket, uint32_t timeout_ms, uint32_t* n_kp, float* kp_xy, todhip_pose* poses,
                         uint32_t* n_poses, uint32_t* pose_ptr, uint32_t* inlier_kp, uint32_t* n_inlier_kp) {
  if (!p || !n_kp || !n_poses || !pose_ptr || !n_inlier_kp || (*n_poses && !poses) || (*n_inlier_kp && !inlier_kp)) return TODHIP_EINVAL;
  std::unique_lock<std::mutex> lk(p->mu);
  if (!p->find(ticket)) return p->dead ? TODHIP_EHIP : TODHIP_EINVAL;
  Slot* s = nullptr;
  auto ready = [&] { s = p->find(ticket); return !s || s->state == kDone; };
  if (timeout_ms == 0) p->cv.wait(lk, ready);
  else if (!p->cv.wait_for(lk, std::chrono::milliseconds(timeout_ms), ready)) return TODHIP_ETIMEOUT;
  if (!s) return TODHIP_EINVAL;                                    // another thread waited for it meanwhile
  auto release = [&] { s->state = kFree; s->ticket = 0; };
  if (p->dead) { release(); return TODHIP_EHIP; }
  if (s->status != TODHIP_OK) { const int rc = s->status; release(); return rc; }
  if (s->n_poses > *n_poses || s->n_inl > *n_inlier_kp) {
    *n_poses = s->n_poses; *n_inlier_kp = s->n_inl;
    return TODHIP_ECAPACITY;
  }
  const uint32_t n = s->n_frames, nq = p->nq;
  for (uint32_t f = 0; f < n; ++f) n_kp[f] = s->n_kp[f];
  if (kp_xy)
    for (uint32_t f = 0; f < n; ++f) {                             // rows behind n_kp[f] come back as zeros, not as an earlier step's
      float* dst = kp_xy + (size_t)f * nq * 2;
      std::memcpy(dst, s->h_kp.as<float>() + (size_t)f * nq * 2, (size_t)s->n_kp[f] * 2 * sizeof(float));
      std::memset(dst + (size_t)s->n_kp[f] * 2, 0, (size_t)(nq - s->n_kp[f]) * 2 * sizeof(float));
    }
  std::copy(s->poses.begin(), s->poses.begin() + s->n_poses, poses);
  std::copy(s->pose_ptr.begin(), s->pose_ptr.begin() + n + 1, pose_ptr);
  std::copy(s->inl.get(), s->inl.get() + s->n_inl, inlier_kp);
  *n_poses = s->n_poses; *n_inlier_kp = s->n_inl;
  release();
  return TODHIP_OK;
}

int todhip_pipeline_get_stats(todhip_pipeline* p, todhip_pipeline_stats* out) {
  if (!p || !out) return TODHIP_EINVAL;
  todhip_counters c;
  {
    std::lock_guard<std::mutex> g(p->mctx_mu);
    if (hipSetDevice(p->device) != hipSuccess) return TODHIP_EHIP;
    const int rc = todhip_get_counters(p->mctx, &c);
    if (rc != TODHIP_OK) return rc;
  }
  std::lock_guard<std::mutex> lk(p->mu);
  *out = p->stats;
  out->sum_match_kernel_ms = c.sum_match_kernel_ms;
  out->n_match_kernel_launches = c.n_match_kernel_launches;
  return TODHIP_OK;
}

int todhip_bgr_to_gray_device(todhip_ctx* ctx, const void* d_src, uint32_t channels, uint32_t H, uint32_t W, uint32_t src_stride,
                              void* d_gray, uint32_t gray_stride) {
  if (!ctx || !d_src || !d_gray || (channels != 3 && channels != 4) || H == 0 || W == 0 || W > 0x10000000u) return TODHIP_EINVAL;
  if (src_stride < W * channels || gray_stride < W) return TODHIP_EINVAL;
  TOD_HIP(hipSetDevice(ctx->device));
  const int rc = launch_bgr_to_gray(ctx->stream, d_src, channels, 0, src_stride, d_gray, 0, gray_stride, 1, H, W);
  if (rc == TODHIP_EHIP) ctx->last_hip_error = (int)hipErrorLaunchFailure;
  return rc;
}

}  // extern "C"
