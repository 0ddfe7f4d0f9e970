// The speculative draw table (K7a, drawIndexSampleHelper, sac_model_registration_graph.h:102-132) in its wave-per-position and
// lane-per-position forms, and the chain walk through it (K7b, getSamples, :141-168).
// Included by verify.hip inside its anonymous namespace, after verify_kernels.h and verify_launch.h.

struct DrawArgs { ObjJob job; const uint32_t* rnd; uint32_t window_len, S; DrawEntry* table; };
struct ChainArgs {
  const DrawEntry* table; uint32_t S, n_req, attempts0, out_base;
  uint32_t* iter_samples; uint32_t* iter_pos_after; ChainOut* out;
};

// ------------------------------------------------------------------------------------------------ K7a
__global__ __launch_bounds__(256) void draw_table_kernel(Slots<DrawArgs, kWideSlots> SL) {
  TOD_LATENCY_PRIO();   // latency-bound: win issue arbitration against the VALU-saturating matcher
  const ObjJob& job = SL.a[blockIdx.y].job;
  const uint32_t* __restrict__ rnd = SL.a[blockIdx.y].rnd;
  const uint32_t window_len = SL.a[blockIdx.y].window_len, S = SL.a[blockIdx.y].S;
  DrawEntry* const table = SL.a[blockIdx.y].table;
  const uint32_t s = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (s >= S) return;
  const uint32_t W = job.W;
  WaveBits VA;
  wb_load(VA, job.valid, W);
  uint32_t nA = wb_count(VA);
  uint32_t pos = s, status = DRAW_FAIL, s0 = 0, s1 = 0, s2 = 0;
  while (nA > 0) {                                        // level "3 samples left"
    if (pos >= window_len) { status = DRAW_OVERFLOW; break; }
    const uint32_t a = wb_select(VA, rnd[pos++] % nA);    // valid_samples[rand() % size], :111
    if (a >= job.n) break;                                // cannot happen; keeps every address in bounds
    WaveBits VB = VA;
    wb_and(VB, job.samp + (size_t)a * W, W);              // set_intersection with the sample neighbours, :113-117
    uint32_t nB = wb_count(VB);
    bool ok = false;
    uint32_t b = 0, c = 0;
    while (nB > 0) {                                      // level "2 samples left"
      if (pos >= window_len) { status = DRAW_OVERFLOW; break; }
      b = wb_select(VB, rnd[pos++] % nB);
      if (b >= job.n) { nB = 0; break; }
      WaveBits VC = VB;
      wb_and(VC, job.samp + (size_t)b * W, W);
      const uint32_t nC = wb_count(VC);
      if (nC > 0) {                                       // level "1 sample left": any pick succeeds
        if (pos >= window_len) { status = DRAW_OVERFLOW; break; }
        c = wb_select(VC, rnd[pos++] % nC);
        ok = true;
        break;
      }
      wb_clear(VB, b);                                    // std::remove of the failed pick, :125-128
      --nB;
    }
    if (status == DRAW_OVERFLOW) break;
    if (ok) { status = DRAW_OK; s0 = c; s1 = b; s2 = a; break; }   // samples_ is deepest-first, :118-121
    wb_clear(VA, a);
    --nA;
  }
  if (lane_id() == 0) {
    DrawEntry e;
    e.status = status; e.consumed = pos - s; e.s0 = s0; e.s1 = s1; e.s2 = s2; e.pad = 0;
    table[s] = e;
  }
}

// K7a for objects of at most 128 matches (W <= 2): ONE LANE per stream position instead of one wave -- the bitsets fit
// two 64-bit registers, so a lane runs the helper's three levels on its own. Distractor objects (a few dozen random
// matches, hopeless, burning their whole iteration budget and hundreds of failed attempts) are what makes the table
// large, and they are small: 64 x fewer waves for the same table.
__device__ __forceinline__ uint32_t nth_set_bit128(u64 w0, u64 w1, uint32_t n) {   // n-th set bit (ascending), n < popc
  const uint32_t c0 = (uint32_t)__popcll(w0);
  u64 w = w0; uint32_t base = 0;
  if (n >= c0) { n -= c0; w = w1; base = 64u; }
  uint32_t pos = 0;
#pragma unroll
  for (uint32_t shift = 32; shift > 0; shift >>= 1) {
    const uint32_t cnt = (uint32_t)__popcll((w >> pos) & ((1ull << shift) - 1ull));
    if (n >= cnt) { n -= cnt; pos += shift; }
  }
  return base + pos;
}
__global__ __launch_bounds__(256) void draw_table_small_kernel(Slots<DrawArgs, kWideSlots> SL) {
  TOD_LATENCY_PRIO();   // latency-bound: win issue arbitration against the VALU-saturating matcher
  const ObjJob& job = SL.a[blockIdx.y].job;
  const uint32_t* __restrict__ rnd = SL.a[blockIdx.y].rnd;
  const uint32_t window_len = SL.a[blockIdx.y].window_len, S = SL.a[blockIdx.y].S;
  DrawEntry* const table = SL.a[blockIdx.y].table;
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  if (s >= S) return;
  const uint32_t W = job.W;                                // 1 or 2
  u64 a0 = job.valid[0], a1 = W > 1u ? job.valid[1] : 0ull;
  uint32_t nA = (uint32_t)(__popcll(a0) + __popcll(a1));
  uint32_t pos = s, status = DRAW_FAIL, s0 = 0, s1 = 0, s2 = 0;
  while (nA > 0) {                                          // level "3 samples left"
    if (pos >= window_len) { status = DRAW_OVERFLOW; break; }
    const uint32_t a = nth_set_bit128(a0, a1, rnd[pos++] % nA);   // valid_samples[rand() % size], :111
    if (a >= job.n) break;                                  // cannot happen; keeps every address in bounds
    u64 b0 = a0 & job.samp[(size_t)a * W], b1 = W > 1u ? (a1 & job.samp[(size_t)a * W + 1]) : 0ull;   // :113-117
    uint32_t nB = (uint32_t)(__popcll(b0) + __popcll(b1));
    bool ok = false;
    uint32_t b = 0, c = 0;
    while (nB > 0) {                                        // level "2 samples left"
      if (pos >= window_len) { status = DRAW_OVERFLOW; break; }
      b = nth_set_bit128(b0, b1, rnd[pos++] % nB);
      if (b >= job.n) { nB = 0; break; }
      const u64 c0 = b0 & job.samp[(size_t)b * W], c1 = W > 1u ? (b1 & job.samp[(size_t)b * W + 1]) : 0ull;
      const uint32_t nC = (uint32_t)(__popcll(c0) + __popcll(c1));
      if (nC > 0) {                                         // level "1 sample left": any pick succeeds
        if (pos >= window_len) { status = DRAW_OVERFLOW; break; }
        c = nth_set_bit128(c0, c1, rnd[pos++] % nC);
        ok = true;
        break;
      }
      if (b < 64u) b0 &= ~(1ull << b); else b1 &= ~(1ull << (b - 64u));   // std::remove of the failed pick, :125-128
      --nB;
    }
    if (status == DRAW_OVERFLOW) break;
    if (ok) { status = DRAW_OK; s0 = c; s1 = b; s2 = a; break; }   // samples_ is deepest-first, :118-121
    if (a < 64u) a0 &= ~(1ull << a); else a1 &= ~(1ull << (a - 64u));
    --nA;
  }
  DrawEntry e;
  e.status = status; e.consumed = pos - s; e.s0 = s0; e.s1 = s1; e.s2 = s2; e.pad = 0;
  table[s] = e;
}

// ------------------------------------------------------------------------------------------------ K7b
// The walk is a pointer chase (position -> position + consumed): through global memory every hop costs a DRAM/L2
// round trip (~1.5 us; 2500 iterations of a hopeless object = 4 ms), so the hop data (status, consumed) of the whole
// window is first packed into LDS by all threads, one lane walks it there, recording where each successful attempt
// started, and all threads then fetch those attempts' triples.
constexpr uint32_t kChainLdsEntries = 36u * 1024u;       // 144 KB of packed (consumed << 2 | status) words
constexpr uint32_t kChainMaxReq = 4096u;                  // == kMaxEvalWaves
__global__ __launch_bounds__(256) void chain_kernel(Slots<ChainArgs, kWideSlots> SL) {
  TOD_LATENCY_PRIO();   // latency-bound: win issue arbitration against the VALU-saturating matcher
  extern __shared__ __align__(16) unsigned char lds_raw[];
  uint32_t* s_hop = reinterpret_cast<uint32_t*>(lds_raw);                       // min(S, kChainLdsEntries)
  const ChainArgs& a = SL.a[blockIdx.x];
  const DrawEntry* __restrict__ table = a.table;
  const uint32_t S = a.S, n_req = a.n_req, attempts0 = a.attempts0, out_base = a.out_base;
  uint32_t* const iter_samples = a.iter_samples; uint32_t* const iter_pos_after = a.iter_pos_after; ChainOut* const out = a.out;
  const uint32_t n_lds = min(S, kChainLdsEntries);
  uint32_t* s_start = s_hop + n_lds;                                            // n_req: table position of each drawn iteration
  __shared__ uint32_t s_done;
  for (uint32_t i = threadIdx.x; i < n_lds; i += 256u) s_hop[i] = (table[i].consumed << 2) | table[i].status;
  __syncthreads();
  if (threadIdx.x < 64u) {
    // Wave 0 walks, with wave-uniform control flow: the hop words of 64 consecutive positions sit in one register (lane i = position
    // base + i) and a hop inside the window is a v_readlane -- an attempt consumes a handful of draws, so a window serves ~10 hops
    // and the dependent LDS round trip (~100 cycles, what a hop cost before) is paid once per window.
    const uint32_t lane = threadIdx.x;
    uint32_t p = 0, done = 0, attempts = attempts0, flag = 0, base = 0xFFFFFF00u, win = 0;
    while (done < n_req) {
      bool got = false;
      while (true) {
        if (p >= S) { flag = 1; break; }
        if (p - base >= 64u) {                              // wave-uniform (also true on the first pass: base is far above)
          base = p;
          const uint32_t idx = base + lane;
          win = idx < n_lds ? s_hop[idx] : (idx < S ? ((table[idx].consumed << 2) | table[idx].status) : 0u);
        }
        const uint32_t hop = (uint32_t)__builtin_amdgcn_readlane((int)win, (int)(p - base));
        const uint32_t status = hop & 3u;
        if (status == DRAW_OVERFLOW) { flag = 1; break; }
        const uint32_t at = p;
        p = uni(p + (hop >> 2));
        if (status == DRAW_OK) {
          if (lane == 0) { s_start[done] = at; iter_pos_after[out_base + done] = p; }
          got = true;
          break;
        }
        if (++attempts >= kMaxSampleChecks) { flag = 2; break; }   // getSamples gives up: samples.clear(), :167
      }
      if (!got) break;
      attempts = 0;
      ++done;
    }
    if (lane == 0) {
      out->n_done = done; out->pos_end = p; out->attempts = attempts; out->flag = flag;
      s_done = done;
    }
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < s_done; i += 256u) {
    const DrawEntry e = table[s_start[i]];
    iter_samples[3 * (out_base + i) + 0] = e.s0;
    iter_samples[3 * (out_base + i) + 1] = e.s1;
    iter_samples[3 * (out_base + i) + 2] = e.s2;
  }
}
