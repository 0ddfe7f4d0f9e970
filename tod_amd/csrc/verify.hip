// Stage C on gfx950: GuessGenerator::process (reference src/detection/GuessGenerator.cpp:127-250) and the
// verifier library under src/common (adjacency_ransac.cpp, sac_model_registration_graph.h, ransac.h,
// maximum_clique.cpp). Decisions D2-D4 of SURVEY.md App. A apply.
//
// This file is the one translation unit of the verifier: it includes the device code, one header per concern, into its anonymous
// namespace, and holds the host side -- workspaces, SideStreams, StreamCache, the C entry points -- around the batch engine
// (verify_engine.h). The todhip_test_* hooks are in verify_hooks.h.
//
// Kernels
//   K6  adjacency_kernel     (verify_prep.h) FillAdjacency (adjacency_ransac.cpp:127-172): one wave = 64 pair tests -> one
//                            64-bit word of the physical and of the sample bit matrix via __ballot
//   K7a draw_table_lane_kernel, draw_table_kernel (verify_draw.h, verify_draw_bits.h) drawIndexSampleHelper
//                            (sac_model_registration_graph.h:102-132) evaluated speculatively from EVERY position of the rand()
//                            stream window: one lane each for objects of up to 512 matches (bitsets of 2 or 8 words in the
//                            lane's registers), one wave each beyond (bitsets of one or eight slices of 64 words)
//   K7b chain_kernel         (verify_draw.h) getSamples (:141-168) x iterations: pointer chase through the table
//   K8  eval_kernel          (verify_eval.h, verify_clique.h) selectWithinDistance (:171-269): 3-row AND + popcount, degree filter and the
//                            maximum-clique gate (maximum_clique.cpp:286-369) on an LDS-resident induced graph
//   K9  growth_kernel        (verify_growth.h) Ransac's refinement loop (adjacency_ransac.cpp:255-308) incl. Kabsch/SVD (:304-347)
//   K11 invalidate_kernel    (verify_prep.h) InvalidateQueryIndices / InvalidateIndices (:63-123)
//   K_c cluster_frame_kernel (verify_prep.h) ClusterPerObject (:176-205); cluster_frame_rescaled_kernel: the same body with the depth
//                            image at a size of its own, the rescaled pixel computed at each keypoint (depth_rescale.h)
//       sprint_kernel        (verify_sprint.h) all of the above for a frame's small objects, by one workgroup
// What kernels and host exchange through the slot's control block and mailbox is laid out in verify_kernels.h (SlotCtl, SlotMail).
// The RANSAC bookkeeping (ransac.h:95-135: strictly-better test, adaptive k with pow/log) is replayed on the
// host from the per-iteration consensus counts, so that libm results are those of the CPU reference.
#include <algorithm>
#include <chrono>
#include <atomic>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "ctx.h"
#include "depth_rescale.h"
#include "verify_kernels.h"
#include "verify_draw_bits.h"

using namespace tod;

namespace {

#include "verify_launch.h"
#include "verify_prep.h"
#include "verify_draw.h"
#include "verify_clique.h"
#include "verify_eval.h"
#include "verify_growth.h"
#include "verify_sprint.h"


// ------------------------------------------------------------------------------------------------ host side
struct VerifyWs {
  DevBuf train, query, qidx, kpxy, phys, samp, bits, sampdeg, nvalid, table, iter_samples, counts, gate_m,
      small, deferred, stacks, kp_bits, clique_adj, adjc_scratch, c_kept, c_offs, c_qpt, c_obj, c_hist, c_goff,
      sprint_status, sprint_stack, c_src, c_cnt;
  // the slot's mailbox: pinned host memory that kernels read and write directly (see copy_words_kernel)
  HostBuf m_small, m_hist, m_pos, m_counts, m_kp, m_nvalid;
  HostBuf m_sprint, m_sprint_out, m_sprint_kp;              // sprint_kernel: the object list in, records and keypoint lists out
  HostBuf h_small;                                          // staging of the test hooks
};

// one workspace per frame slot of a batch; slot 0 also serves the single-frame entry points and the test hooks
struct StreamCache;
struct VerifyPool : TodWs {
  static constexpr int kSlot = kWsVerify;
  std::vector<VerifyWs*> slots; std::vector<StreamCache*> streams;
  std::vector<hipEvent_t> side_ev;                          // one per lane of a batch (Engine::run_ticks), created on first use
  // argument sets of a launch group's long lists (launch_many): one pair per lane, so that groups in flight on different streams
  // never share staging memory, and a pair only grows while its lane is idle
  static constexpr size_t kMaxLanes = 17;
  HostBuf args_stage[kMaxLanes]; DevBuf args_dev[kMaxLanes];
  DevBuf kceil; bool kceil_ready = false;                   // sprint_kernel: ceil(k) of ransac.h:130 per (|valid|, n_best), 65 x 65
  ~VerifyPool() override;                                   // (below StreamCache)
};
// The flights' streams belong to the process, not to a context: a process has eight hardware queues for all of its streams
// (DESIGN 7), the runtime deals streams onto them round robin, and every further stream -- busy or not -- makes it likelier that two
// busy ones share a queue. Contexts driven from several host threads share these few: a flight takes a stream for itself
// (`taken`) and gives it back when it has landed; a context that finds none free keeps its heavy phase in the lock-step -- with
// several batches in flight on contexts of their own the batches overlap each other anyway.
struct SideStreams {
  struct PerDevice {
    std::vector<hipStream_t> st;
    std::atomic<bool> taken[16];
    uint32_t partition = 0;                                 // todhip_set_cu_partition's value the streams were created under
    PerDevice() { for (auto& t : taken) t.store(false); }
  };
  std::mutex mu;
  std::map<int, PerDevice> by_device;
  hipError_t get(int device, uint32_t n, std::vector<hipStream_t>& out, PerDevice** pd) {
    std::lock_guard<std::mutex> g(mu);
    PerDevice& d = by_device[device];
    const uint32_t part = tod_cu_partition();
    if (d.partition != part) {                              // the CU partition changed: new streams, once nobody is on the old ones
      bool in_use = false;
      for (size_t i = 0; i < d.st.size(); ++i) in_use = in_use || d.taken[i].load();
      if (!in_use) {
        for (hipStream_t s0 : d.st) { (void)hipStreamSynchronize(s0); (void)hipStreamDestroy(s0); }
        d.st.clear();
        d.partition = part;
      }
    }
    while (d.st.size() < n) {
      hipStream_t s2;                                       // latency-bound work: the highest priority there is, or the CU partition's
      const hipError_t e = tod_stream_create(&s2, device, TODHIP_STREAM_LATENCY);
      if (e != hipSuccess) return e;
      d.st.push_back(s2);
    }
    out.assign(d.st.begin(), d.st.begin() + n);
    *pd = &d;
    return hipSuccess;
  }
};
SideStreams g_side_streams;
// batches being verified right now, over all contexts of the process: with three or more in the air the hardware queues are
// already kept busy by each other's ticks and a flight only adds a stream to wait behind (bench `chained`, 4 workers: 4060
// frames/s in lock-step, 3740 with flights; 1 worker: 1490 / 2230, 2 workers: 2400 / 2900)
std::atomic<int> g_batches_in_air{0};

constexpr uint32_t kEvalLdsSmall = 48u * 1024u;
constexpr uint32_t kEvalLdsBig = 160u * 1024u - 512u;
constexpr uint32_t kStackCap = 128u * 1024u;       // u16 entries per wave beyond the LDS part of the stack (256 KB)
constexpr uint32_t kMaxEvalWaves = 4096u;          // hypotheses per evaluation batch

VerifyWs* ws_of(todhip_ctx* ctx, size_t slot = 0) {
  VerifyPool* p = tod_ws<VerifyPool>(ctx);
  while (p->slots.size() <= slot) p->slots.push_back(new VerifyWs());
  return p->slots[slot];
}

// The rand() stream of a frame, generated once and shared: every round of every object reads a window of it, and
// frames that start from the same generator state (a harness restarting rand() per frame, decision D4) share one
// copy. Snapshots of the generator every kSnap draws give the state at any position without replaying the stream.
struct StreamCache {
  static constexpr uint64_t kSnap = 4096;
  todhip_rng init, gen;
  std::vector<uint32_t> vals;                              // vals[i] = i-th draw after `init`
  std::vector<todhip_rng> snaps;                           // snaps[j] = generator state before draw j * kSnap
  explicit StreamCache(const todhip_rng& r) : init(r), gen(r) {}
  bool same_start(const todhip_rng& r) const {
    return r.f == init.f && r.b == init.b && std::memcmp(r.s, init.s, sizeof(init.s)) == 0;
  }
  void extend_to(uint64_t n) {
    while (vals.size() < n) {
      if (vals.size() % kSnap == 0) snaps.push_back(gen);
      vals.push_back(rng_next(gen));
    }
  }
  // device copy of the stream (append-only): a round's window is an offset into it, nothing is copied per tick
  DevBuf dev;
  uint64_t dev_valid = 0;
  hipError_t ensure_device(uint64_t n, hipStream_t st) {
    extend_to(n);
    if (n <= dev_valid) return hipSuccess;
    const uint64_t want = std::max<uint64_t>(n, 2 * dev_valid);
    extend_to(want);
    if (dev.cap < want * sizeof(uint32_t)) {                // grow: DevBuf::reserve drops the old contents, upload all again
      hipError_t e = hipDeviceSynchronize();                // kernels of earlier ticks and of flights on other streams may still read it
      if (e != hipSuccess) return e;
      e = dev.reserve((size_t)want * 2 * sizeof(uint32_t));
      if (e != hipSuccess) return e;
      dev_valid = 0;
    }
    hipError_t e = hipMemcpyAsync(dev.as<uint32_t>() + dev_valid, vals.data() + dev_valid, (size_t)(want - dev_valid) * sizeof(uint32_t),
                                  hipMemcpyHostToDevice, st);
    // complete before anyone is told the stream reaches this far: slots that share the cache may read it from another stream
    // (the copy doubles the valid length, so a context in steady state never gets here)
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) dev_valid = want;
    return e;
  }
  todhip_rng state_at(uint64_t pos) {                      // generator after `pos` draws (draw counter relative to init)
    extend_to(pos + 1);
    todhip_rng g = snaps[pos / kSnap];
    for (uint64_t i = (pos / kSnap) * kSnap; i < pos; ++i) (void)rng_next(g);
    return g;
  }
};

// ransac.h:121-130 with libm: k = log(1 - 0.99) / log(1 - w^3), w = n_best / |valid|. The host's replay and the device's table
// (VerifyPool::kceil) must be this one sequence of double operations: round traces are compared bit for bit on iteration counts.
inline double ransac_k(double w) {
  double p_no_outliers = 1.0 - std::pow(w, 3.0);
  p_no_outliers = std::max(std::numeric_limits<double>::epsilon(), p_no_outliers);
  p_no_outliers = std::min(1.0 - std::numeric_limits<double>::epsilon(), p_no_outliers);
  return std::log(1.0 - 0.99) / std::log(p_no_outliers);
}

// launch(staged kernel, by-value kernel, extent) with eval_kernel's instantiations for the objects' width (wide: more than 512 matches)
// in the two forms of passing argument sets (SlotsPtr<EvalArgs>: launch_many, Slots<EvalArgs>: launch_list), the pass (deferred: the
// instantiations that carry the third tier; every argument set of such a launch has from_deferred set), and the blocks one
// argument set needs: its iterations, or its deferred ones.
template <class Launch>
void pick_eval(bool wide, bool deferred, Launch launch) {
  auto extent = [deferred](const EvalArgs& a) { return dim3(deferred ? a.n_deferred : a.it_end - a.it_begin); };
  typedef SlotsPtr<EvalArgs> P;
  typedef Slots<EvalArgs> V;
  if (wide && deferred) launch(eval_kernel<true, P, true>, eval_kernel<true, V, true>, extent);
  else if (wide) launch(eval_kernel<true, P>, eval_kernel<true, V>, extent);
  else if (deferred) launch(eval_kernel<false, P, true>, eval_kernel<false, V, true>, extent);
  else launch(eval_kernel<false, P>, eval_kernel<false, V>, extent);
}

int set_big_lds_once(todhip_ctx* ctx) {
  static std::atomic<bool> done{false};                   // contexts may be driven from several host threads
  if (!done.load(std::memory_order_acquire)) {
    const void* const big[] = {reinterpret_cast<const void*>(eval_kernel<false>), reinterpret_cast<const void*>(eval_kernel<true>),
                               reinterpret_cast<const void*>(eval_kernel<false, SlotsPtr<EvalArgs>>),
                               reinterpret_cast<const void*>(eval_kernel<true, SlotsPtr<EvalArgs>>),
                               reinterpret_cast<const void*>(eval_kernel<false, Slots<EvalArgs>, true>),
                               reinterpret_cast<const void*>(eval_kernel<true, Slots<EvalArgs>, true>),
                               reinterpret_cast<const void*>(eval_kernel<false, SlotsPtr<EvalArgs>, true>),
                               reinterpret_cast<const void*>(eval_kernel<true, SlotsPtr<EvalArgs>, true>),
                               reinterpret_cast<const void*>(clique_test_kernel<false>), reinterpret_cast<const void*>(clique_test_kernel<true>),
                               reinterpret_cast<const void*>(clique_test_kernel<false, false>), reinterpret_cast<const void*>(clique_test_kernel<true, false>),
                               reinterpret_cast<const void*>(chain_kernel)};
    for (const void* f : big) TOD_HIP(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kEvalLdsBig));
    TOD_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(sprint_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)kSprintLds));
    done.store(true, std::memory_order_release);
  }
  return TODHIP_OK;
}

// the first-pass evaluation of iterations [it_lo, it_hi) of `job` out of the slot's buffers (ws->stacks is reserved by the caller)
EvalArgs eval_args(const ObjJob& job, VerifyWs* ws, int32_t* counts, uint32_t it_lo, uint32_t it_hi, uint32_t lds_bytes) {
  SlotCtl* c = ws->small.as<SlotCtl>();
  EvalArgs A;
  A.job = job; A.iter_samples = ws->iter_samples.as<uint32_t>(); A.it_begin = it_lo; A.it_end = it_hi;
  A.counts = counts; A.gate_m = ws->gate_m.as<uint32_t>(); A.work = &c->eval_work;
  A.status = &c->eval; A.deferred = ws->deferred.as<uint32_t>(); A.stacks = ws->stacks.as<uint16_t>();
  A.stack_cap = kStackCap; A.lds_bytes = lds_bytes; A.from_deferred = 0u; A.n_deferred = 0u;
  A.adjc_scratch = nullptr; A.dbg = nullptr; A.dbg_stride = 0; A.stop_level = 0; A.n_items_dev = nullptr;
  return A;
}
// the part of cluster_frame_kernel's arguments that is the slot's own scratch, whoever receives the grouped outputs
void cluster_scratch(ClusterArgs& ca, VerifyWs* ws) {
  ca.kept = ws->c_kept.as<uint32_t>(); ca.offs = ws->c_offs.as<uint32_t>(); ca.obj_of = ws->c_obj.as<uint32_t>();
  ca.src = ws->c_src.as<uint32_t>(); ca.cnt = ws->c_cnt.as<uint32_t>(); ca.qpt = ws->c_qpt.as<float>();
  ca.query = ws->query.as<float>(); ca.kpxy = ws->kpxy.as<float>(); ca.m_hist = ws->m_hist.as<uint32_t>();
}

struct ObjSpan {
  uint32_t obj, offset, n;
  // this object's slices of the slot's adjacency / bitset / degree buffers (all objects of a frame are prepared in
  // one tick, so each needs its own), and its first round's |valid|
  uint64_t adj_off = 0; uint32_t bits_off = 0, deg_off = 0, nvalid = 0, degsum = 0, triangle = 1;
  bool resume = false, counted = false;                    // sprint_kernel left it unfinished (its first-round statistics are stale) / in the counters
};
// geom (rescale == true): the depth image is geom.dH x geom.dW and the verifier sees rescale_depth's H x W result of it, computed at
// the keypoint pixels only (todhip_verify*_depth_rescaled); otherwise the depth image has the image's size
struct DepthInput { const void* d_depth; int is_u16; float fx, fy, cx, cy; bool rescale; RescaleGeom geom; };

#include "verify_engine.h"

}  // namespace

// ClusterPerObject of F frames without a cloud, for the 2D-only branch (pnp.hip): per frame f the matches grouped by object -- model
// points into d_X and keypoint indices f nq + q into d_qidx, both at [f nq k, ...) -- and per object its count and offset
// (d_hist, d_goff: F x n_objs). One launch, nothing comes to the host; d_err: one ClusterCtl (8 words) per frame, error != 0: the frame's inputs
// were refused.
int tod_cluster_frames_nocloud(todhip_ctx* ctx, uint32_t F, const float* d_kp_xy, uint32_t nq, const uint32_t* d_counts,
                               const todhip_dmatch* d_matches, const float* d_mxyz, uint32_t k, uint32_t n_objs, float* d_X,
                               uint32_t* d_qidx, uint32_t* d_hist, uint32_t* d_goff, uint32_t* d_err) {
  Engine E = {ctx, ctx->stream, nq, 0xFFFFFFFFu, 0xFFFFFFFFu, k, n_objs, nullptr, nullptr, {}};
  std::vector<ClusterArgs> v;
  const size_t per = (size_t)nq * k;
  for (uint32_t f = 0; f < F; ++f) {
    Slot s;
    s.ws = ws_of(ctx, f);
    int rc = E.reserve_common(s);
    if (rc == TODHIP_OK) rc = E.reserve_cluster(s);
    if (rc != TODHIP_OK) return rc;
    ClusterArgs ca;
    ca.kp_xy = d_kp_xy + 2 * (size_t)f * nq; ca.cloud = nullptr; ca.depth = nullptr; ca.counts = d_counts + (size_t)f * nq;
    ca.matches = d_matches + f * per; ca.mxyz = d_mxyz + 3 * f * per; ca.nq = nq; ca.k = k; ca.H = ca.Wimg = 0xFFFFFFFFu; ca.n_objs = n_objs;
    ca.qidx_add = f * nq; ca.depth_is_u16 = 0; ca.fx = ca.fy = 1.f; ca.cx = ca.cy = 0.f;
    cluster_scratch(ca, s.ws);
    ca.hist = d_hist + (size_t)f * n_objs; ca.goff = d_goff + (size_t)f * n_objs;
    ca.train = d_X + 3 * f * per; ca.qidx = d_qidx + f * per;
    ca.m_ctl = reinterpret_cast<ClusterCtl*>(d_err) + f;      // (device words here)
    v.push_back(ca);
  }
  launch_list(ctx->stream, cluster_frame_kernel, v, 256, 0, 0, [](const ClusterArgs&) { return dim3(1); });
  TOD_HIP(hipGetLastError());
  return TODHIP_OK;
}

VerifyPool::~VerifyPool() {
  for (VerifyWs* ws : slots) delete ws;
  for (StreamCache* c : streams) delete c;
  for (hipEvent_t e : side_ev) (void)hipEventDestroy(e);
}

extern "C" {

void todhip_rng_seed(todhip_rng* r, uint32_t seed) {
  if (!r) return;
  if (seed == 0) seed = 1;
  int32_t word = (int32_t)seed;
  r->s[0] = seed;
  for (int i = 1; i < 31; ++i) {                          // srandom_r: Lehmer LCG, Schrage's method
    const long hi = word / 127773, lo = word % 127773;
    word = (int32_t)(16807 * lo - 2836 * hi);
    if (word < 0) word += 2147483647;
    r->s[i] = (uint32_t)word;
  }
  r->f = 3; r->b = 0;
  for (int i = 0; i < 310; ++i) {
    r->s[r->f] += r->s[r->b];
    r->f = (r->f + 1) % 31; r->b = (r->b + 1) % 31;
  }
  r->draws = 0;
}

static int verify_prologue(todhip_ctx* ctx, const todhip_verify_params* prm) {
  if (!ctx || !prm) return TODHIP_EINVAL;
  ctx->counters.last_objects_verified = ctx->counters.last_rounds = ctx->counters.last_hypotheses = 0;
  ctx->counters.last_gate_calls = ctx->counters.last_poses = 0;
  ctx->counters.last_sprint_launches = ctx->counters.last_sprint_rounds = ctx->counters.last_verify_ticks = 0;
  ctx->traces.clear();
  TOD_HIP(hipSetDevice(ctx->device));
  return set_big_lds_once(ctx);
}

// poses and inlier lists of the slots, concatenated in slot order; pose_ptr (optional) = CSR offsets per slot
static int collect(todhip_ctx* ctx, std::vector<Slot>& slots, todhip_pose* poses, uint32_t pose_cap, uint32_t* n_poses,
                   uint32_t* pose_ptr, uint32_t* inlier_kp, uint32_t kp_cap, uint32_t* n_inlier_kp) {
  uint32_t np = 0, nk = 0;
  for (size_t f = 0; f < slots.size(); ++f) {
    Slot& s = slots[f];
    if (pose_ptr) pose_ptr[f] = np;
    for (const todhip_round_trace& t : s.traces) ctx->traces.push_back(t);
    if (np + s.poses.size() > pose_cap || nk + s.inliers.size() > kp_cap) return TODHIP_ECAPACITY;
    for (todhip_pose p : s.poses) {
      p.inlier_begin += nk; p.inlier_end += nk;
      poses[np++] = p;
    }
    for (uint32_t v : s.inliers) inlier_kp[nk++] = v;
  }
  if (pose_ptr) pose_ptr[slots.size()] = np;
  *n_poses = np; *n_inlier_kp = nk;
  return TODHIP_OK;
}

int todhip_verify(todhip_ctx* ctx, const float* kp_xy, uint32_t nq, const float* cloud, uint32_t H, uint32_t Wimg,
                  const uint32_t* row_ptr, const todhip_dmatch* matches, const float* mxyz, const float* spans,
                  uint32_t n_objs, const todhip_verify_params* prm, todhip_rng* rng, todhip_pose* poses,
                  uint32_t* n_poses, uint32_t* inlier_kp, uint32_t* n_inlier_kp) {
  if (!ctx || !prm || !rng || !n_poses || !n_inlier_kp || (*n_poses && !poses) || (*n_inlier_kp && !inlier_kp))
    return TODHIP_EINVAL;
  int rc = verify_prologue(ctx, prm);
  if (rc != TODHIP_OK) return rc;
  const uint32_t pose_cap = *n_poses, kp_cap = *n_inlier_kp;
  *n_poses = 0; *n_inlier_kp = 0;
  if (!cloud || H == 0 || Wimg == 0) return TODHIP_OK;   // 2D-only input is an empty TODO (GuessGenerator.cpp:147-152)
  if (nq && (!kp_xy || !row_ptr || !spans)) return TODHIP_EINVAL;
  VerifyWs* ws = ws_of(ctx);

  // ---- ClusterPerObject (adjacency_ransac.cpp:176-205) on the host buffers the caller handed over: a gather of
  // one cloud point per keypoint and a bucket by imgIdx; per object, matches stay in (query asc, rank asc) order
  struct HostCluster { std::vector<float> train, query, kpxy; std::vector<uint32_t> qidx; };
  std::map<uint32_t, HostCluster> objects;
  for (uint32_t qi = 0; qi < nq; ++qi) {
    const int row = (int)kp_xy[2 * qi + 1], col = (int)kp_xy[2 * qi];   // float -> int truncation (:185)
    if (row < 0 || col < 0 || (uint32_t)row >= H || (uint32_t)col >= Wimg) return TODHIP_ERANGE;
    const float* qp = cloud + 3 * ((size_t)row * Wimg + col);
    if (std::isnan(qp[0])) continue;                                     // only .x is tested (:189)
    for (uint32_t m = row_ptr[qi]; m < row_ptr[qi + 1]; ++m) {
      if (matches[m].imgIdx < 0 || (uint32_t)matches[m].imgIdx >= n_objs) return TODHIP_ERANGE;
      HostCluster& c = objects[(uint32_t)matches[m].imgIdx];
      for (int k = 0; k < 3; ++k) { c.train.push_back(mxyz[3 * (size_t)m + k]); c.query.push_back(qp[k]); }
      c.kpxy.push_back(kp_xy[2 * qi]); c.kpxy.push_back(kp_xy[2 * qi + 1]);
      c.qidx.push_back(qi);
    }
  }
  hipStream_t st = ctx->stream;
  std::vector<Slot> slots(1);
  Slot& s = slots[0];
  s.ws = ws; s.rng = rng;
  uint32_t total = 0, max_n = 0;
  for (auto& kv : objects) {
    s.objs.push_back({kv.first, total, (uint32_t)kv.second.qidx.size()});
    total += (uint32_t)kv.second.qidx.size();
    max_n = std::max(max_n, (uint32_t)kv.second.qidx.size());
  }
  if (total == 0) return TODHIP_OK;
  TOD_HIP(ws->train.reserve((size_t)total * 12)); TOD_HIP(ws->query.reserve((size_t)total * 12));
  TOD_HIP(ws->qidx.reserve((size_t)total * 4)); TOD_HIP(ws->kpxy.reserve((size_t)total * 8));
  // the objects' slices are contiguous on the device (object order): four uploads for the frame, not four per object (a frame of
  // self-similar texture spreads its matches over a couple of hundred objects)
  std::vector<float> h_train((size_t)total * 3), h_query((size_t)total * 3), h_kpxy((size_t)total * 2);
  std::vector<uint32_t> h_qidx(total);
  size_t i = 0;
  for (auto& kv : objects) {
    HostCluster& c = kv.second;
    const ObjSpan& o = s.objs[i++];
    if (o.n == 0) continue;
    std::memcpy(h_train.data() + 3 * (size_t)o.offset, c.train.data(), (size_t)o.n * 12);
    std::memcpy(h_query.data() + 3 * (size_t)o.offset, c.query.data(), (size_t)o.n * 12);
    std::memcpy(h_qidx.data() + o.offset, c.qidx.data(), (size_t)o.n * 4);
    std::memcpy(h_kpxy.data() + 2 * (size_t)o.offset, c.kpxy.data(), (size_t)o.n * 8);
  }
  TOD_HIP(hipMemcpyAsync(ws->train.p, h_train.data(), (size_t)total * 12, hipMemcpyHostToDevice, st));
  TOD_HIP(hipMemcpyAsync(ws->query.p, h_query.data(), (size_t)total * 12, hipMemcpyHostToDevice, st));
  TOD_HIP(hipMemcpyAsync(ws->qidx.p, h_qidx.data(), (size_t)total * 4, hipMemcpyHostToDevice, st));
  TOD_HIP(hipMemcpyAsync(ws->kpxy.p, h_kpxy.data(), (size_t)total * 8, hipMemcpyHostToDevice, st));
  TOD_HIP(hipStreamSynchronize(st));   // the host vectors die with this scope
  Engine E = {ctx, st, nq, H, Wimg, 0u, n_objs, spans, prm, {}};
  rc = E.reserve_common(s);
  if (rc != TODHIP_OK) return rc;
  if (!E.reserve_objects(s, max_n)) return s.rc;
  s.ph = PH_PREPALL;
  std::vector<Slot*> live = {&s};
  rc = E.run(live);
  const int rc2 = collect(ctx, slots, poses, pose_cap, n_poses, nullptr, inlier_kp, kp_cap, n_inlier_kp);
  return rc != TODHIP_OK ? rc : rc2;
}

// Device-resident form for a batch of F frames (F = 1 for the single-frame entry points): keypoints, cloud or
// depth, and the matcher's fixed-stride outputs (counts[nq], matches[nq*k], matches_xyz[nq*k*3], see
// todhip_match_device) of frame f start at f times their per-frame size; only poses come back to the host.
static int verify_batch_impl(todhip_ctx* ctx, uint32_t F, const void* d_kp_xy, uint32_t nq, const void* d_cloud,
                             const DepthInput* dep, uint32_t H, uint32_t Wimg, const void* d_counts, const void* d_matches,
                             const void* d_mxyz, uint32_t k, const float* spans, uint32_t n_objs,
                             const todhip_verify_params* prm, todhip_rng* rng, todhip_pose* poses, uint32_t* n_poses,
                             uint32_t* pose_ptr, uint32_t* inlier_kp, uint32_t* n_inlier_kp) {
  if (!ctx || !prm || !rng || !n_poses || !n_inlier_kp || (*n_poses && !poses) || (*n_inlier_kp && !inlier_kp) || F == 0)
    return TODHIP_EINVAL;
  int rc = verify_prologue(ctx, prm);
  if (rc != TODHIP_OK) return rc;
  const uint32_t pose_cap = *n_poses, kp_cap = *n_inlier_kp;
  *n_poses = 0; *n_inlier_kp = 0;
  if (pose_ptr) for (uint32_t f = 0; f <= F; ++f) pose_ptr[f] = 0;
  if ((!d_cloud && !dep) || H == 0 || Wimg == 0) return TODHIP_OK;
  if (nq == 0 || n_objs == 0) return TODHIP_OK;
  if (!d_kp_xy || !d_counts || !d_matches || !d_mxyz || !spans || k == 0) return TODHIP_EINVAL;
  Engine E = {ctx, ctx->stream, nq, H, Wimg, k, n_objs, spans, prm, {}};
  std::vector<Slot> slots(F);
  std::vector<Slot*> live;
  const size_t px = (size_t)H * Wimg;
  const size_t depth_px = dep && dep->rescale ? (size_t)dep->geom.dH * dep->geom.dW : px;   // of one frame's depth image
  for (uint32_t f = 0; f < F; ++f) {
    Slot& s = slots[f];
    s.ws = ws_of(ctx, f);
    s.rng = rng + f;
    s.d_kp_xy = reinterpret_cast<const float*>(d_kp_xy) + (size_t)f * nq * 2;
    s.d_counts = reinterpret_cast<const uint32_t*>(d_counts) + (size_t)f * nq;
    s.d_matches = reinterpret_cast<const todhip_dmatch*>(d_matches) + (size_t)f * nq * k;
    s.d_mxyz = reinterpret_cast<const float*>(d_mxyz) + (size_t)f * nq * k * 3;
    if (dep) {
      s.use_depth = true;
      s.dep = *dep;
      s.dep.d_depth = reinterpret_cast<const unsigned char*>(dep->d_depth) + (size_t)f * depth_px * (dep->is_u16 ? 2 : 4);
    } else {
      s.d_cloud = reinterpret_cast<const float*>(d_cloud) + (size_t)f * px * 3;
    }
    rc = E.reserve_common(s);
    if (rc != TODHIP_OK) return rc;
    rc = E.reserve_cluster(s);
    if (rc != TODHIP_OK) return rc;
    s.ph = PH_CLUSTER;
    live.push_back(&s);
  }
  rc = E.run(live);
  const int rc2 = collect(ctx, slots, poses, pose_cap, n_poses, pose_ptr, inlier_kp, kp_cap, n_inlier_kp);
  return rc != TODHIP_OK ? rc : rc2;
}

int todhip_verify_device(todhip_ctx* ctx, const void* d_kp_xy, uint32_t nq, const void* d_cloud, uint32_t H,
                         uint32_t Wimg, const void* d_counts, const void* d_matches, const void* d_mxyz, uint32_t k,
                         const float* spans, uint32_t n_objs, const todhip_verify_params* prm, todhip_rng* rng,
                         todhip_pose* poses, uint32_t* n_poses, uint32_t* inlier_kp, uint32_t* n_inlier_kp) {
  return verify_batch_impl(ctx, 1, d_kp_xy, nq, d_cloud, nullptr, H, Wimg, d_counts, d_matches, d_mxyz, k, spans, n_objs, prm, rng,
                           poses, n_poses, nullptr, inlier_kp, n_inlier_kp);
}

int todhip_verify_device_depth(todhip_ctx* ctx, const void* d_kp_xy, uint32_t nq, const void* d_depth, int depth_is_u16,
                               uint32_t H, uint32_t Wimg, const float* K9, const void* d_counts, const void* d_matches,
                               const void* d_mxyz, uint32_t k, const float* spans, uint32_t n_objs,
                               const todhip_verify_params* prm, todhip_rng* rng, todhip_pose* poses, uint32_t* n_poses,
                               uint32_t* inlier_kp, uint32_t* n_inlier_kp) {
  if (!d_depth || !K9) return TODHIP_EINVAL;
  DepthInput dep = {d_depth, depth_is_u16, K9[0], K9[4], K9[2], K9[5], false, {}};
  return verify_batch_impl(ctx, 1, d_kp_xy, nq, nullptr, &dep, H, Wimg, d_counts, d_matches, d_mxyz, k, spans, n_objs, prm, rng,
                           poses, n_poses, nullptr, inlier_kp, n_inlier_kp);
}

int todhip_verify_batch_device(todhip_ctx* ctx, uint32_t n_frames, const void* d_kp_xy, uint32_t nq, const void* d_cloud,
                               uint32_t H, uint32_t Wimg, const void* d_counts, const void* d_matches, const void* d_mxyz,
                               uint32_t k, const float* spans, uint32_t n_objs, const todhip_verify_params* prm,
                               todhip_rng* rng, todhip_pose* poses, uint32_t* n_poses, uint32_t* pose_ptr,
                               uint32_t* inlier_kp, uint32_t* n_inlier_kp) {
  if (!pose_ptr) return TODHIP_EINVAL;
  return verify_batch_impl(ctx, n_frames, d_kp_xy, nq, d_cloud, nullptr, H, Wimg, d_counts, d_matches, d_mxyz, k, spans, n_objs,
                           prm, rng, poses, n_poses, pose_ptr, inlier_kp, n_inlier_kp);
}

int todhip_verify_batch_device_depth(todhip_ctx* ctx, uint32_t n_frames, const void* d_kp_xy, uint32_t nq, const void* d_depth,
                                     int depth_is_u16, uint32_t H, uint32_t Wimg, const float* K9, const void* d_counts,
                                     const void* d_matches, const void* d_mxyz, uint32_t k, const float* spans, uint32_t n_objs,
                                     const todhip_verify_params* prm, todhip_rng* rng, todhip_pose* poses, uint32_t* n_poses,
                                     uint32_t* pose_ptr, uint32_t* inlier_kp, uint32_t* n_inlier_kp) {
  if (!d_depth || !K9 || !pose_ptr) return TODHIP_EINVAL;
  DepthInput dep = {d_depth, depth_is_u16, K9[0], K9[4], K9[2], K9[5], false, {}};
  return verify_batch_impl(ctx, n_frames, d_kp_xy, nq, nullptr, &dep, H, Wimg, d_counts, d_matches, d_mxyz, k, spans, n_objs, prm,
                           rng, poses, n_poses, pose_ptr, inlier_kp, n_inlier_kp);
}

// The depth image at the sensor's own size: what todhip_rescale_depth_device would write into an H x W image is computed at the
// keypoint pixels inside the cluster kernel (cluster_frame_rescaled_kernel); everything behind the lookup is the code of the calls above.
static bool depth_rescaled_input(const void* d_depth, int depth_is_u16, uint32_t dH, uint32_t dW, int nearest, uint32_t H, uint32_t Wimg,
                                 const float* K9, DepthInput* dep) {
  if (!d_depth || !K9 || !dH || !dW || !H || !Wimg) return false;
  *dep = {d_depth, depth_is_u16 ? 1 : 0, K9[0], K9[4], K9[2], K9[5], false, {}};
  if (!rescale_geometry(dH, dW, H, Wimg, nearest, &dep->geom)) return false;
  dep->rescale = dep->geom.mode != RescaleGeom::kEqual;    // equal sizes: the existing call
  return true;
}

int todhip_verify_device_depth_rescaled(todhip_ctx* ctx, const void* d_kp_xy, uint32_t nq, const void* d_depth, int depth_is_u16,
                                        uint32_t dH, uint32_t dW, int nearest, uint32_t H, uint32_t Wimg, const float* K9,
                                        const void* d_counts, const void* d_matches, const void* d_mxyz, uint32_t k, const float* spans,
                                        uint32_t n_objs, const todhip_verify_params* prm, todhip_rng* rng, todhip_pose* poses,
                                        uint32_t* n_poses, uint32_t* inlier_kp, uint32_t* n_inlier_kp) {
  DepthInput dep;
  if (!depth_rescaled_input(d_depth, depth_is_u16, dH, dW, nearest, H, Wimg, K9, &dep)) return TODHIP_EINVAL;
  return verify_batch_impl(ctx, 1, d_kp_xy, nq, nullptr, &dep, H, Wimg, d_counts, d_matches, d_mxyz, k, spans, n_objs, prm, rng,
                           poses, n_poses, nullptr, inlier_kp, n_inlier_kp);
}

int todhip_verify_batch_device_depth_rescaled(todhip_ctx* ctx, uint32_t n_frames, const void* d_kp_xy, uint32_t nq, const void* d_depth,
                                              int depth_is_u16, uint32_t dH, uint32_t dW, int nearest, uint32_t H, uint32_t Wimg,
                                              const float* K9, const void* d_counts, const void* d_matches, const void* d_mxyz,
                                              uint32_t k, const float* spans, uint32_t n_objs, const todhip_verify_params* prm,
                                              todhip_rng* rng, todhip_pose* poses, uint32_t* n_poses, uint32_t* pose_ptr,
                                              uint32_t* inlier_kp, uint32_t* n_inlier_kp) {
  DepthInput dep;
  if (!pose_ptr || !depth_rescaled_input(d_depth, depth_is_u16, dH, dW, nearest, H, Wimg, K9, &dep)) return TODHIP_EINVAL;
  return verify_batch_impl(ctx, n_frames, d_kp_xy, nq, nullptr, &dep, H, Wimg, d_counts, d_matches, d_mxyz, k, spans, n_objs, prm,
                           rng, poses, n_poses, pose_ptr, inlier_kp, n_inlier_kp);
}

int todhip_verify_trace(const todhip_ctx* ctx, todhip_round_trace* out, uint32_t* n) {
  if (!ctx || !n || (*n && !out)) return TODHIP_EINVAL;
  const uint32_t cap = *n;
  *n = (uint32_t)ctx->traces.size();
  for (uint32_t i = 0; i < cap && i < ctx->traces.size(); ++i) out[i] = ctx->traces[i];
  return ctx->traces.size() > cap ? TODHIP_ECAPACITY : TODHIP_OK;
}
}  // extern "C"

#include "verify_hooks.h"
