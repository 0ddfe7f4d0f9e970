// Internal context of libtodhip (not part of the C ABI).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <type_traits>
#include <vector>

#include "../../include/todhip.h"
#include "db_select.h"
#include "fp4_rows.h"
#include "match_split.h"
#include "match_tiles.h"

#define TOD_HIP(call)                                  \
  do {                                                 \
    hipError_t e_ = (call);                            \
    if (e_ != hipSuccess) {                            \
      ctx->last_hip_error = (int)e_;                   \
      return TODHIP_EHIP;                              \
    }                                                  \
  } while (0)

// The short, latency-bound kernels (verifier, merges) raise their wave priority: beside the matcher's VALU-saturating waves a wave
// at default priority gets ~1/5 of a SIMD's issue slots. ORB's kernels do not (orb.hip says why).
#ifndef TOD_LATENCY_PRIO_LEVEL
#define TOD_LATENCY_PRIO_LEVEL 3
#endif
#define TOD_LATENCY_PRIO() __builtin_amdgcn_s_setprio(TOD_LATENCY_PRIO_LEVEL)

// bytes todhip_db_load allocates behind the last descriptor row: hamming_topk_mfma loads whole 32-row steps without a per-lane clamp
constexpr size_t kDbSlackBytes = 2048;
// (and hamming_topk_wide, match_wide.hip: the last 32-row step of 64-byte rows reaches 31 rows behind the end -- it fits, only just)
static_assert(31 * 64 <= kDbSlackBytes, "a 32-row step of the widest binary row must end inside the slack");

// Growable device buffer: the hot path never calls hipMalloc once sizes have been seen.
// A buffer frees itself with its owner and is never copied (release() is for freeing early on purpose). Nothing that holds one may
// have static storage duration: its destructor would call hipFree after the runtime has shut down.
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  hipError_t reserve(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    size_t want = bytes + bytes / 4 + 256;
    hipError_t e = hipMalloc(&p, want);
    if (e == hipSuccess) cap = want;
    // diagnostics (tests/test_verify_gpu.py's poisoned run): fresh allocations start as 0xCD bytes instead of whatever the
    // allocator hands back, so that a read of memory nobody wrote shows up on every run, not on one in five
    static const bool poison = getenv("TODHIP_POISON_ALLOC") != nullptr;
    if (e == hipSuccess && poison) { e = hipMemset(p, 0xCD, want); if (e == hipSuccess) e = hipDeviceSynchronize(); }
    return e;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
  template <typename T> T* as() const { return reinterpret_cast<T*>(p); }
};

// Pinned host staging buffer.
struct HostBuf {
  void* p = nullptr;
  size_t cap = 0;
  HostBuf() = default;
  HostBuf(const HostBuf&) = delete;
  HostBuf& operator=(const HostBuf&) = delete;
  ~HostBuf() { release(); }
  hipError_t reserve(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
    size_t want = bytes + bytes / 4 + 256;
    hipError_t e = hipHostMalloc(&p, want, hipHostMallocDefault);
    if (e == hipSuccess) cap = want;
    static const bool poison = getenv("TODHIP_POISON_ALLOC") != nullptr;   // as DevBuf
    if (e == hipSuccess && poison) std::memset(p, 0xCD, want);
    return e;
  }
  void release() {
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
  }
  template <typename T> T* as() const { return reinterpret_cast<T*>(p); }
};

// A stage's workspace: defined in the stage's translation unit (struct XWs : TodWs with kSlot = its slot), created on first use by
// tod_ws<XWs>(ctx), owned by the context. Its destructor is the stage's whole teardown. The slots are released in this order.
struct TodWs { virtual ~TodWs() {} };
enum TodWsSlot { kWsVerify, kWsOrb, kWsL2, kWsPnp, kWsLsh, kWsLearn, kWsCompact, kWsRadius, kWsCrossCheck, kWsOther, kWsSlots };

struct todhip_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  int last_hip_error = 0;
  int n_cu = 256;

  // ---- object database (stage B1). Rows of this shard only; points + object table complete.
  uint32_t desc_bytes = 0;
  uint64_t total_rows = 0, shard_first = 0, shard_rows = 0;
  uint32_t n_objs = 0;
  DevBuf db_desc;          // shard_rows (+pad) x desc_bytes
  DevBuf db_pts;           // total_rows x 3 f32
  DevBuf db_obj_off;       // n_objs + 1 u32
  std::vector<uint32_t> h_obj_off;
  std::vector<float> h_spans;

  // ---- matcher workspaces
  DevBuf m_q, m_part, m_keys, m_counts, m_matches, m_xyz, m_bound;
  HostBuf h_stage;
  // optional HIP-event bracketing of the dominant matcher kernel: a ring of event pairs that is
  // drained lazily, so timing never adds a host sync inside the timed region
  bool time_kernels = false;
  static constexpr int kEvPairs = 64;
  hipEvent_t evp[2 * kEvPairs] = {};
  uint64_t ev_head = 0, ev_tail = 0;   // pairs [ev_tail, ev_head) are recorded and not yet read
  todhip_counters counters = {};
  int matcher_engine = TODHIP_ENGINE_AUTO;   // todhip_set_matcher_engine
  // K4x's split blocks (match_launch.h, launch_topk_mfma_qt): cumulative {blocks that went on, blocks} of the launches in that mode,
  // as the DB pass counts them and as the merge kernel leaves them in pinned memory; the controller that reads them (match_split.h)
  HostBuf k4x_stats_host; DevBuf k4x_stats_dev;
  K4xSplit k4x;                              // k4x.force: todhip_set_matcher_block_split
  float ratio = 0.f;                         // todhip_set_ratio_test (0 = off)
  uint32_t cross_check_q = 0;                // todhip_set_cross_check: the frame size todhip_match[_device] filter with (0 = off)
  float ratio_other = 0.f;                   // todhip_set_ratio_test_other (0 = off): the filter todhip_match[_device] run behind finalize
  float l2_ratio = 0.f;                      // todhip_set_l2_ratio_test (0 = off): the float forms' own ratio test
  uint32_t l2_cross_check_q = 0;             // todhip_set_l2_cross_check: the frame size todhip_match_l2[_device] filter with (0 = off)
  // todhip_set_db_bit_order (db_bitorder.hip): the mode the next load uses; the order of the resident shard (stored position p holds
  // original bit bit_src_of[p]) and whether it differs from the identity; its device copy and the queries' workspace -- both stay
  // empty until a load computes an order
  int bit_order_mode = TODHIP_BIT_ORDER_NONE;
  bool bit_order_on = false;
  uint8_t bit_src_of[256];
  DevBuf bit_tab, m_qord;
  // todhip_db_select_objects (db_select.hip): while sel_on, every Hamming search runs over view_desc -- the shard's rows of the selected
  // objects, compacted in ascending object order, kDbSlackBytes of zeros behind them as behind db_desc -- and its keys go through
  // view_tab (sel.seg_view, then sel.seg_global) back to rows of the full DB. Off (all objects): sel is empty, both buffers are unused.
  bool sel_on = false;
  TodViewTables sel;
  DevBuf view_desc, view_tab;
  // The resident fp4 copy of the active 32-byte rows (tod_db_rows; layout: fp4_rows.h), read by hamming_topk_fp4rows instead of
  // expanding every row in every launch. Built by the first launch that reads it (match_launch.h) and again whenever the rows it
  // was built from have changed: rows_gen counts the writes of db_desc / view_desc and the switches between them
  // (tod_db_rows_written), fp4_gen is the count the copy was built at (0: no copy).
  DevBuf db_fp4;
  uint64_t rows_gen = 1, fp4_gen = 0;

  std::vector<todhip_round_trace> traces;

  std::unique_ptr<TodWs> ws[kWsSlots];       // todhip_destroy releases them before the events and the stream go

  todhip_ctx() { for (int p = 0; p < 256; ++p) bit_src_of[p] = (uint8_t)p; }
};

// What the Hamming searches read: the active view, or the whole shard exactly as before while all objects are selected. Keys of a view
// are built on first row 0 and mapped by tod_view_remap.
inline const void* tod_db_rows(const todhip_ctx* ctx) { return ctx->sel_on ? ctx->view_desc.p : ctx->db_desc.p; }
inline uint64_t tod_db_n_rows(const todhip_ctx* ctx) { return ctx->sel_on ? ctx->sel.view_rows() : ctx->shard_rows; }
inline uint64_t tod_db_first_row(const todhip_ctx* ctx) { return ctx->sel_on ? 0ull : ctx->shard_first; }
// Every writer of what tod_db_rows returns says so (todhip_db_load, todhip_db_select_objects on and off, todhip_set_db_bit_order):
// what was derived from the rows (the fp4 copy) is stale from here on
inline void tod_db_rows_written(todhip_ctx* ctx) { ++ctx->rows_gen; }

template <typename T> T* tod_ws(todhip_ctx* ctx) {
  std::unique_ptr<TodWs>& s = ctx->ws[T::kSlot];
  if (!s) s.reset(new T());
  return static_cast<T*>(s.get());
}
template <typename T> const T* tod_ws(const todhip_ctx* ctx) { return static_cast<const T*>(ctx->ws[T::kSlot].get()); }   // nullptr: never used

// glibc random_r TYPE_3 (see include/todhip.h, decision D4)
inline uint32_t rng_next(todhip_rng& r) {
  r.s[r.f] += r.s[r.b];
  const uint32_t out = r.s[r.f] >> 1;
  r.f = r.f == 30u ? 0u : r.f + 1u; r.b = r.b == 30u ? 0u : r.b + 1u;
  ++r.draws;
  return out;
}

// capi.hip: fixed stride k -> CSR (the cell's vector<vector<DMatch>> / vector<Mat> shapes): query qi's first counts[qi] slots, packed;
// returns the total (== row_ptr[nq])
uint32_t tod_pack_csr(const uint32_t* counts, const todhip_dmatch* m, const float* xyz, uint32_t nq, uint32_t k, uint32_t* row_ptr,
                      todhip_dmatch* matches, float* matches_xyz);
// capi.hip: a stream of the given kind (todhip_stream_create), honouring the process's CU partition
extern "C" hipError_t tod_stream_create(hipStream_t* out, int device, int kind);
extern "C" uint32_t tod_cu_partition();                     // todhip_set_cu_partition's current value
// match.hip (the launchers: match_launch.h, match_plan.h)
int tod_timing_begin(todhip_ctx* ctx, int* slot);
int tod_timing_end(todhip_ctx* ctx, int slot);
int tod_timing_drain(todhip_ctx* ctx, uint64_t keep);
// The optional HIP-event bracket around a DB pass (todhip_set_kernel_timing)
struct KernelTimer {
  todhip_ctx* ctx;
  int slot = -1;
  int begin() { return ctx->time_kernels ? tod_timing_begin(ctx, &slot) : TODHIP_OK; }
  int end() { return slot >= 0 ? tod_timing_end(ctx, slot) : TODHIP_OK; }
};
int tod_match_lists(todhip_ctx* ctx, const void* d_q, uint32_t nq, uint32_t k, uint32_t radius, uint64_t* d_lists,
                    uint32_t* n_lists);
size_t tod_match_lists_bytes(uint32_t nq, uint32_t k);
// match_wide.hip: the search over the active rows of a 64-byte DB, tod_match_lists' step for that width (k in 1..8, at least one row)
int tod_wide_lists_active(todhip_ctx* ctx, const void* d_q, uint32_t nq, uint32_t k, uint32_t radius, uint64_t* d_lists,
                          uint32_t* n_lists);
// The list length k of a search as a template argument: fn(std::integral_constant<int, K>) for k = K in 1..8, TODHIP_EINVAL otherwise
template <typename Fn>
int dispatch_k(uint32_t k, Fn fn) {
  switch (k) {
    case 1: return fn(std::integral_constant<int, 1>{});
    case 2: return fn(std::integral_constant<int, 2>{});
    case 3: return fn(std::integral_constant<int, 3>{});
    case 4: return fn(std::integral_constant<int, 4>{});
    case 5: return fn(std::integral_constant<int, 5>{});
    case 6: return fn(std::integral_constant<int, 6>{});
    case 7: return fn(std::integral_constant<int, 7>{});
    case 8: return fn(std::integral_constant<int, 8>{});
    default: return TODHIP_EINVAL;
  }
}
int tod_match_shard_keys(todhip_ctx* ctx, const void* d_q, uint32_t nq, uint32_t k, uint32_t radius, uint64_t* d_keys);
// k_in: entries per list; k_out: matches per query in the outputs (k_in > k_out only for the ratio test with k == 1)
int tod_match_finalize(todhip_ctx* ctx, const uint64_t* d_keys_all, uint32_t n_shards, uint32_t nq, uint32_t k_in, uint32_t k_out,
                       uint32_t radius, uint32_t* d_counts, todhip_dmatch* d_matches, float* d_xyz,
                       hipStream_t stream = nullptr);   // nullptr: the context's stream
// cross_check.hip: todhip_cross_check_device behind its argument checks (what todhip_match[_device] run while todhip_set_cross_check is on)
int tod_cross_check(todhip_ctx* ctx, const void* d_q, uint32_t nq, uint32_t frame_queries, const uint32_t* frame_nq, uint32_t stride,
                    uint32_t* d_counts, todhip_dmatch* d_matches, float* d_xyz);
// match_other.hip: todhip_ratio_other_device behind its argument checks (what todhip_match[_device] run while
// todhip_set_ratio_test_other is on); max_d1: no kept match is further than this (the call's radius; the row width when unknown)
int tod_ratio_other(todhip_ctx* ctx, const void* d_q, uint32_t nq, float ratio, uint32_t max_d1, uint32_t stride, uint32_t* d_counts,
                    todhip_dmatch* d_matches);
// cross_check.hip: todhip_cross_check_l2_device behind its argument checks (what todhip_match_l2[_device] run while
// todhip_set_l2_cross_check is on); d_q: nq rows of 128 f32
int tod_cross_check_l2(todhip_ctx* ctx, const void* d_q, uint32_t nq, uint32_t frame_queries, const uint32_t* frame_nq, uint32_t stride,
                       uint32_t* d_counts, todhip_dmatch* d_matches, float* d_xyz);
// verify.hip: ClusterPerObject of F frames on the device without a cloud (pnp.hip's 2D-only branch); d_err: 8 words per frame
// (ClusterCtl of verify_kernels.h: word 0 = error, word 4 = matches kept)
int tod_cluster_frames_nocloud(todhip_ctx* ctx, uint32_t F, const float* d_kp_xy, uint32_t nq, const uint32_t* d_counts,
                               const todhip_dmatch* d_matches, const float* d_mxyz, uint32_t k, uint32_t n_objs, float* d_X,
                               uint32_t* d_qidx, uint32_t* d_hist, uint32_t* d_goff, uint32_t* d_err);
// db_bitorder.hip: the optional bit order of the resident Hamming DB (todhip_set_db_bit_order). _load: todhip_db_load's step between
// the rows' arrival and the LSH index; _queries: nq query rows in the resident order (only while ctx->bit_order_on)
int tod_bit_order_load(todhip_ctx* ctx);
int tod_bit_order_queries(todhip_ctx* ctx, const void* d_q, uint32_t nq, const void** d_out);
// db_select.hip: back to all objects (todhip_db_load); n keys (distance << 32 | view row, or ~0) -> (distance << 32 | global row)
void tod_view_reset(todhip_ctx* ctx);
int tod_view_remap(todhip_ctx* ctx, uint64_t* d_keys, size_t n);
// lsh.hip: the optional LSH-approximate mode (todhip_set_lsh)
bool tod_lsh_enabled(const todhip_ctx* ctx);
int tod_lsh_build(todhip_ctx* ctx);
int tod_lsh_lists(todhip_ctx* ctx, const void* d_q, uint32_t nq, uint32_t k, uint64_t* d_lists, uint32_t* n_lists);
int tod_l2_db_prepare(todhip_ctx* ctx);      // l2.hip: bf16 image + norms of a 128 x f32 DB resident in db_desc
int tod_orb_device(todhip_ctx* ctx, const uint8_t* d_gray, const uint8_t* d_mask, uint32_t H, uint32_t W, uint32_t stride,
                   uint32_t n_features, uint32_t n_levels, float scale_factor, const int8_t* pattern, float* d_kp_xy,
                   float* d_kp_aux, uint8_t* d_desc, uint32_t cap, uint32_t* n_out);
int tod_orb_batch_device(todhip_ctx* ctx, const uint8_t* d_gray, size_t gray_fs, const uint8_t* d_mask, uint32_t F, uint32_t H,
                         uint32_t W, uint32_t stride, uint32_t n_features, uint32_t n_levels, float scale_factor, const int8_t* pattern,
                         float* d_kp_xy, float* d_kp_aux, uint8_t* d_desc, uint32_t cap, uint32_t* n_out);
