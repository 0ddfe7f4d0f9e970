// What the two cross-check translation units share (cross_check.hip: the Hamming test X1 and the compaction X2; cross_check_l2.hip:
// the float test X1L): how a call's frame_nq reaches a kernel, the valid range of a frame as a kernel sees it, and the launcher of
// X2, which both filters end in. Included behind ctx.h and cross_check.h.
#pragma once

constexpr uint32_t kArgFrames = 64;          // frame_nq of up to this many frames travels as a kernel argument (the pipeline's steps)

// frame_nq: none (every row of a frame is valid), by value, or in device memory (more than kArgFrames frames)
enum LimitMode { kLimitNone = 0, kLimitArg = 1, kLimitDev = 2 };
struct FrameLimits { uint32_t n[kArgFrames]; };

__device__ __forceinline__ tod::CrossCheckRange valid_range(uint32_t f, uint32_t nq, uint32_t Q, int mode, const FrameLimits& lim,
                                                            const uint32_t* __restrict__ d_frame_nq) {
  const uint32_t n = mode == kLimitArg ? lim.n[f] : mode == kLimitDev ? d_frame_nq[f] : 0u;
  return tod::cross_check_valid(f, nq, Q, mode != kLimitNone, n);
}

// the three kernel arguments a call's frame_nq becomes (both tests and X2 take them)
struct FrameLimitArgs {
  int mode = kLimitNone;
  FrameLimits lim = {};
  const uint32_t* d_frame_nq = nullptr;
};

// cross_check.hip. frame_nq (host, n_frames entries, or null) -> *out; more than kArgFrames frames are copied into the context's
// workspace on its stream before the call returns
int tod_cross_check_frame_limits(todhip_ctx* ctx, const uint32_t* frame_nq, uint32_t n_frames, FrameLimitArgs* out);
// cross_check.hip. X2 on the context's stream behind a test kernel
void tod_cross_check_compact(todhip_ctx* ctx, uint32_t nq, uint32_t Q, const FrameLimitArgs& a, uint32_t stride, uint32_t* d_counts,
                             todhip_dmatch* d_matches, float* d_xyz);
