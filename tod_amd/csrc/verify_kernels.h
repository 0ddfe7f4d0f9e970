// Stage C device code (gfx950): the graph-constrained RANSAC verifier of wg-perception/tod.
// Reference: src/common/adjacency_ransac.cpp, sac_model_registration_graph.h, ransac.h, maximum_clique.cpp.
// All adjacency is kept as bit matrices (n rows of W 64-bit words); one wave owns one hypothesis.
// Holds what more than one of the verify_*.h headers needs: ObjJob, the draw table entry, the result structs kernels hand to the
// host and the layout of the slot's control block and mailbox they sit in, wave helpers, float helpers. Precedes every other
// verifier header.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace tod {

typedef unsigned long long u64;

constexpr int kMaxWords = 512;     // n <= 32768 matches per object (conf/detection.ork:26,  n_features 5000 x the cell's k = 5 -> 25000)
constexpr int kWPL = 8;            // bitset words per lane (kMaxWords / 64)
constexpr uint32_t kMaxSampleChecks = 1000;   // sac_model_registration_graph.h:366
constexpr uint32_t kGateMinimal = 7;          // min(best_inlier_number_, 7) is always 7 (:85,:203,:268)
constexpr int kStepCap = 100000;              // maximum_clique.cpp:318

// One object's matches == one tod::AdjacencyRansac (adjacency_ransac.h:48-133), device resident.
struct ObjJob {
  uint32_t n, W;
  const float* train;     // n x 3  training_points_
  const float* query;     // n x 3  query_points_
  const uint32_t* qidx;   // n      query_indices_ (non-decreasing)
  const float* kpxy;      // n x 2  pixel of the keypoint of each match
  u64* phys;              // n x W  physical_adjacency_
  u64* samp;              // n x W  sample_adjacency_
  u64* finite;            // W      matches whose six coordinates are finite
  u64* valid;             // W      valid_indices_
  u64* deg7;              // W      valid vertices with sample degree >= 7
  uint32_t* sampdeg;      // n      sample degree inside the valid set
};

// one entry of the speculative draw table: the outcome of ONE drawIndexSampleHelper attempt that starts
// at a given position of the rand() stream
struct DrawEntry { uint32_t status, consumed, s0, s1, s2, pad; };   // status: 0 fail, 1 ok, 2 window overflow
enum { DRAW_FAIL = 0, DRAW_OK = 1, DRAW_OVERFLOW = 2 };

struct ChainOut {       // result of walking the draw table (getSamples x iterations)
  uint32_t n_done;      // iterations drawn in this walk
  uint32_t pos_end;     // table position after the last completed attempt
  uint32_t attempts;    // failed attempts of the unfinished getSamples call (carried to the next window)
  uint32_t flag;        // 0 = all requested iterations drawn, 1 = window exhausted, 2 = selection empty (1000 failures)
};

// status words of hypothesis evaluations (gate_eval): counters accumulate over the launches of one batch
struct EvalStatus {
  uint32_t error;        // 0 = none, 1 = clique search failed, 2 = graph too large for any tier, 3 = corrupt draw table, 4 = bad index
  uint32_t gate_calls;   // hypotheses that reached the clique search
  uint32_t n_deferred;   // hypotheses left to the big-LDS pass (length of EvalArgs::deferred)
  uint32_t pad_;
  uint32_t detail_g, detail_value, detail_m, detail_it;   // diagnostics of an error: graph index, its value, |F|, iteration
};

struct GrowthOut {      // result of growth_kernel
  float R[9], T[3];             // inverted pose (training -> camera), adjacency_ransac.cpp:304-305
  uint32_t n_match_inliers;     // match indices in the grown set
  uint32_t n_kp_inliers;        // unique keypoint indices (:306-308)
  uint32_t passes;
  uint32_t n_model_inliers;
};

// what cluster_frame_kernel reports per frame (ClusterArgs::m_ctl); an array of these is the d_err of tod_cluster_frames_nocloud
struct ClusterCtl {
  uint32_t error, pad1_[3];     // != 0: the frame's inputs were refused
  uint32_t n_kept, pad5_[3];    // matches kept (n_all)
};

// The control block of one frame slot, 64 words of device memory (VerifyWs::small) that a tick's last kernel copies to the slot's
// mailbox (pinned host memory, VerifyWs::m_small). The mailbox form has the same head and a tail that only the host side has:
// cluster_frame_kernel writes it straight into the mailbox.
template <class Tail>
struct SlotWords {
  uint32_t pad0_;
  ChainOut chain;               // chain_kernel; chain.n_done also bounds the evaluation launched in the same tick
  uint32_t prep[3];             // round_prep_kernel's statistics: |valid|, sum of sample degrees inside valid, triangle found
  uint32_t eval_work;           // EvalArgs::work
  uint32_t pad9_[3];
  EvalStatus eval;
  uint32_t pad20_[12];
  GrowthOut growth;
  uint32_t pad48_[12];
  Tail tail;
};
struct SlotCtlTail { uint32_t pad60_[4]; };
struct SlotMailTail { ClusterCtl cluster; uint32_t pad68_[60]; };
typedef SlotWords<SlotCtlTail> SlotCtl;
typedef SlotWords<SlotMailTail> SlotMail;
constexpr uint32_t kMailSmallWords = 128u;         // [0, 64) = the slot's device control words, then the rest of ClusterCtl

#define TOD_WORD_AT(T, member, word) static_assert(offsetof(T, member) == (word) * 4u, #T "::" #member " moved")
TOD_WORD_AT(EvalStatus, error, 0); TOD_WORD_AT(EvalStatus, gate_calls, 1); TOD_WORD_AT(EvalStatus, n_deferred, 2);
TOD_WORD_AT(EvalStatus, detail_g, 4); TOD_WORD_AT(EvalStatus, detail_value, 5); TOD_WORD_AT(EvalStatus, detail_m, 6);
TOD_WORD_AT(EvalStatus, detail_it, 7);
TOD_WORD_AT(ClusterCtl, error, 0); TOD_WORD_AT(ClusterCtl, n_kept, 4);
TOD_WORD_AT(SlotCtl, chain, 1); TOD_WORD_AT(SlotCtl, prep, 5); TOD_WORD_AT(SlotCtl, eval_work, 8); TOD_WORD_AT(SlotCtl, eval, 12);
TOD_WORD_AT(SlotCtl, growth, 32); TOD_WORD_AT(SlotCtl, tail, 60);
TOD_WORD_AT(SlotMail, chain, 1); TOD_WORD_AT(SlotMail, prep, 5); TOD_WORD_AT(SlotMail, eval_work, 8); TOD_WORD_AT(SlotMail, eval, 12);
TOD_WORD_AT(SlotMail, growth, 32); TOD_WORD_AT(SlotMail, tail.cluster.error, 60); TOD_WORD_AT(SlotMail, tail.cluster.n_kept, 64);
static_assert(sizeof(EvalStatus) == 8 * 4 && sizeof(ChainOut) == 4 * 4 && sizeof(GrowthOut) == 16 * 4 && sizeof(ClusterCtl) == 8 * 4, "mailbox layout");
static_assert(sizeof(SlotCtl) == 64 * 4 && sizeof(SlotMail) == kMailSmallWords * 4, "mailbox layout");

#undef TOD_WORD_AT

// ---------------------------------------------------------------------------------------------- wave helpers
__device__ __forceinline__ uint32_t lane_id() { return threadIdx.x & 63u; }

// wave-uniform value -> SGPR: branches on it are scalar, so the compiler cannot split the wave's lanes
__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

__device__ __forceinline__ uint32_t rdlane(uint32_t v, uint32_t lane) {    // lane is wave-uniform: v_readlane_b32
  return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)lane);
}
__device__ __forceinline__ u64 rdlane64(u64 v, uint32_t lane) {
  return ((u64)rdlane((uint32_t)(v >> 32), lane) << 32) | rdlane((uint32_t)v, lane);
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return uni(v);
}
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v) {
  const uint32_t l = lane_id();
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    uint32_t t = __shfl_up(v, d);
    if (l >= (uint32_t)d) v += t;
  }
  return v;
}
__device__ __forceinline__ u64 shfl64(u64 v, uint32_t src) {
  uint32_t lo = __shfl((uint32_t)v, src), hi = __shfl((uint32_t)(v >> 32), src);
  return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ uint32_t nth_set_bit(u64 w, uint32_t n) {
  for (uint32_t i = 0; i < n; ++i) w &= w - 1;
  return (uint32_t)__ffsll((long long)w) - 1u;
}

// A bitset over the n matches, distributed over the wave: lane l holds words l, l + 64, ... of kSlices x 64 words. kWPL slices
// hold any object; a kernel that knows its objects to be smaller carries fewer (one slice: W <= 64 words, n <= 4096 matches) and
// every helper below then loops over those alone.
template <int kSlices = kWPL>
struct WaveBitsT {
  u64 w[kSlices];
};
typedef WaveBitsT<> WaveBits;
template <int kSlices>
__device__ __forceinline__ void wb_load(WaveBitsT<kSlices>& b, const u64* p, uint32_t W) {
  const uint32_t l = lane_id();
#pragma unroll
  for (int j = 0; j < kSlices; ++j) b.w[j] = (j * 64u + l) < W ? p[j * 64u + l] : 0ull;
}
template <int kSlices>
__device__ __forceinline__ void wb_and(WaveBitsT<kSlices>& b, const u64* p, uint32_t W) {
  const uint32_t l = lane_id();
#pragma unroll
  for (int j = 0; j < kSlices; ++j) b.w[j] &= (j * 64u + l) < W ? p[j * 64u + l] : 0ull;
}
template <int kSlices>
__device__ __forceinline__ uint32_t wb_count(const WaveBitsT<kSlices>& b) {
  uint32_t c = 0;
#pragma unroll
  for (int j = 0; j < kSlices; ++j) c += (uint32_t)__popcll(b.w[j]);
  return wave_sum(c);
}
template <int kSlices>
__device__ __forceinline__ void wb_clear(WaveBitsT<kSlices>& b, uint32_t v) {
  const uint32_t word = v >> 6, l = lane_id();
#pragma unroll
  for (int j = 0; j < kSlices; ++j)
    if (word == j * 64u + l) b.w[j] &= ~(1ull << (v & 63u));
}
template <int kSlices>
__device__ __forceinline__ void wb_set(WaveBitsT<kSlices>& b, uint32_t v) {
  const uint32_t word = v >> 6, l = lane_id();
#pragma unroll
  for (int j = 0; j < kSlices; ++j)
    if (word == j * 64u + l) b.w[j] |= (1ull << (v & 63u));
}
// index of the idx-th set bit (ascending); idx < count and idx wave-uniform
template <int kSlices>
__device__ __forceinline__ uint32_t wb_select(const WaveBitsT<kSlices>& b, uint32_t idx) {
  idx = uni(idx);
  uint32_t result = 0xFFFFFFFFu;
#pragma unroll
  for (int j = 0; j < kSlices; ++j) {
    const uint32_t c = (uint32_t)__popcll(b.w[j]);
    const uint32_t incl = wave_incl_scan(c);
    const uint32_t total = uni(__shfl(incl, 63));
    if (result == 0xFFFFFFFFu) {
      if (idx < total) {
        const bool mine = (incl - c) <= idx && idx < incl;
        const u64 bal = __ballot(mine);
        const uint32_t owner = (uint32_t)__ffsll((long long)bal) - 1u;
        const uint32_t bit = mine ? nth_set_bit(b.w[j], idx - (incl - c)) : 0u;
        result = (j * 64u + owner) * 64u + uni(__shfl(bit, owner));
      } else {
        idx -= total;
      }
    }
  }
  return result;
}

// ---------------------------------------------------------------------------------------------- float helpers
// Arithmetic order and precision follow the reference; the library is compiled with
// -ffp-contract=off so no product is fused into a following sum.
__device__ __forceinline__ float dist_sq3(const float* a, const float* b) {   // sac_model_registration_graph.h:52-58
  float t0 = a[0] - b[0], t1 = a[1] - b[1], t2 = a[2] - b[2];
  return t0 * t0 + t1 * t1 + t2 * t2;
}
__device__ __forceinline__ double norm3d(float x, float y, float z) {         // cv::norm(Vec3f): double accumulation
  return sqrt((double)x * (double)x + (double)y * (double)y + (double)z * (double)z);
}

}  // namespace tod
