// The speculative draw table (K7a, drawIndexSampleHelper, sac_model_registration_graph.h:102-132) in its wave-per-position and
// lane-per-position forms with the routing between them, and the chain walk through it (K7b, getSamples, :141-168).
// Included by verify.hip inside its anonymous namespace, after verify_kernels.h, verify_draw_bits.h and verify_launch.h.

struct DrawArgs { ObjJob job; const uint32_t* rnd; uint32_t window_len, S; DrawEntry* table; };
struct ChainArgs {
  const DrawEntry* table; uint32_t S, n_req, attempts0, out_base;
  uint32_t* iter_samples; uint32_t* iter_pos_after; ChainOut* out;
};

// ------------------------------------------------------------------------------------------------ K7a
// Wave form: one wave per stream position, the bitsets distributed over its lanes. kSlices = 1 serves objects of up to 4096
// matches (W <= 64: lane l holds word l), kSlices = kWPL any object; the scans, popcounts and predicated loads of the helpers are
// per slice, so the one-slice form executes an eighth of them.
template <int kSlices>
__global__ __launch_bounds__(256) void draw_table_kernel(Slots<DrawArgs, kWideSlots> SL) {
  TOD_LATENCY_PRIO();   // latency-bound: win issue arbitration against the VALU-saturating matcher
  const ObjJob& job = SL.a[blockIdx.y].job;
  const uint32_t* __restrict__ rnd = SL.a[blockIdx.y].rnd;
  const uint32_t window_len = SL.a[blockIdx.y].window_len, S = SL.a[blockIdx.y].S;
  DrawEntry* const table = SL.a[blockIdx.y].table;
  const uint32_t s = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (s >= S) return;
  const uint32_t W = job.W;                               // <= 64 kSlices
  typedef WaveBitsT<kSlices> Bits;
  Bits VA;
  wb_load(VA, job.valid, W);
  uint32_t nA = wb_count(VA);
  uint32_t pos = s, status = DRAW_FAIL, s0 = 0, s1 = 0, s2 = 0;
  while (nA > 0) {                                        // level "3 samples left"
    if (pos >= window_len) { status = DRAW_OVERFLOW; break; }
    const uint32_t a = wb_select(VA, rnd[pos++] % nA);    // valid_samples[rand() % size], :111
    if (a >= job.n) break;                                // cannot happen; keeps every address in bounds
    Bits VB = VA;
    wb_and(VB, job.samp + (size_t)a * W, W);              // set_intersection with the sample neighbours, :113-117
    uint32_t nB = wb_count(VB);
    bool ok = false;
    uint32_t b = 0, c = 0;
    while (nB > 0) {                                      // level "2 samples left"
      if (pos >= window_len) { status = DRAW_OVERFLOW; break; }
      b = wb_select(VB, rnd[pos++] % nB);
      if (b >= job.n) { nB = 0; break; }
      Bits VC = VB;
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

// Lane form, for objects of at most 64 WL matches (W <= WL): ONE LANE per stream position instead of one wave -- the three
// levels' bitsets fit 3 x WL 64-bit registers, so a lane runs the helper's three levels on its own (verify_draw_bits.h: the n-th
// set bit by running popcounts and a search inside the word, the removal of a failed pick by unrolled compares; no array is
// indexed by a run-time value, so nothing goes to scratch). 64 x fewer waves for the same table, and each of them a few hundred
// vector instructions where a wave of the other form executes ~1400 per attempt on a bitset that has a handful of words.
// WL = 2: distractor objects (a few dozen random matches, hopeless, burning their whole iteration budget and hundreds of failed
// attempts), which are what makes a table large. WL = 8: objects of up to 512 matches, the visible object of a frame among them.
// A wave of this form lasts as long as its slowest lane's attempt; the entries are those of the wave form bit for bit.
template <int WL>
__device__ __forceinline__ void lane_and_row(u64 (&dst)[WL], const u64 (&src)[WL], const u64* __restrict__ row, uint32_t W) {
#pragma unroll
  for (int j = 0; j < WL; ++j) dst[j] = (uint32_t)j < W ? (src[j] & row[j]) : 0ull;   // W is uniform over the launch's slot
}
template <int WL>
__global__ __launch_bounds__(256) void draw_table_lane_kernel(Slots<DrawArgs, kWideSlots> SL) {
  TOD_LATENCY_PRIO();   // latency-bound: win issue arbitration against the VALU-saturating matcher
  const ObjJob& job = SL.a[blockIdx.y].job;
  const uint32_t* __restrict__ rnd = SL.a[blockIdx.y].rnd;
  const uint32_t window_len = SL.a[blockIdx.y].window_len, S = SL.a[blockIdx.y].S;
  DrawEntry* const table = SL.a[blockIdx.y].table;
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  if (s >= S) return;
  const uint32_t W = job.W;                                 // 1 .. WL
  u64 va[WL], vb[WL], vc[WL];
#pragma unroll
  for (int j = 0; j < WL; ++j) va[j] = (uint32_t)j < W ? job.valid[j] : 0ull;
  uint32_t nA = tod_bits::count_bits(va);
  uint32_t pos = s, status = DRAW_FAIL, s0 = 0, s1 = 0, s2 = 0;
  while (nA > 0) {                                          // level "3 samples left"
    if (pos >= window_len) { status = DRAW_OVERFLOW; break; }
    const uint32_t a = tod_bits::nth_set_bit(va, rnd[pos++] % nA);   // valid_samples[rand() % size], :111
    if (a >= job.n) break;                                  // cannot happen; keeps every address in bounds
    lane_and_row(vb, va, job.samp + (size_t)a * W, W);      // set_intersection with the sample neighbours, :113-117
    uint32_t nB = tod_bits::count_bits(vb);
    bool ok = false;
    uint32_t b = 0, c = 0;
    while (nB > 0) {                                        // level "2 samples left"
      if (pos >= window_len) { status = DRAW_OVERFLOW; break; }
      b = tod_bits::nth_set_bit(vb, rnd[pos++] % nB);
      if (b >= job.n) { nB = 0; break; }
      lane_and_row(vc, vb, job.samp + (size_t)b * W, W);
      const uint32_t nC = tod_bits::count_bits(vc);
      if (nC > 0) {                                         // level "1 sample left": any pick succeeds
        if (pos >= window_len) { status = DRAW_OVERFLOW; break; }
        c = tod_bits::nth_set_bit(vc, rnd[pos++] % nC);
        ok = true;
        break;
      }
      tod_bits::clear_bit(vb, b);                           // std::remove of the failed pick, :125-128
      --nB;
    }
    if (status == DRAW_OVERFLOW) break;
    if (ok) { status = DRAW_OK; s0 = c; s1 = b; s2 = a; break; }   // samples_ is deepest-first, :118-121
    tod_bits::clear_bit(va, a);
    --nA;
  }
  DrawEntry e;
  e.status = status; e.consumed = pos - s; e.s0 = s0; e.s1 = s1; e.s2 = s2; e.pad = 0;
  table[s] = e;
}

// Which form builds an object's table: a plain function of its word count. The engine (PH_DRAW) and the test hook both ask here.
// A hopeless object of 65-512 matches (hundreds of draws per attempt, a lane's wave as long as its slowest lane) stays with the
// lane form, with no rule on the window's draws per iteration: the scene of six such objects of ~450 matches in
// tools/time_verify_many_objects.py went from 8.73-8.75 ms per frame with one wave per position to 6.13-6.71 (median 6.14) with
// one lane (five alternating turns, profiles/verify_draw.json), so the divergence costs less than the waves it replaces.
enum DrawForm { DRAW_LANE2 = 0, DRAW_LANE8 = 1, DRAW_WAVE1 = 2, DRAW_WAVE8 = 3, DRAW_FORMS = 4 };
inline DrawForm draw_form_of(uint32_t W) { return W <= 2u ? DRAW_LANE2 : W <= 8u ? DRAW_LANE8 : W <= 64u ? DRAW_WAVE1 : DRAW_WAVE8; }
inline uint32_t draw_form_max_words(DrawForm f) { return f == DRAW_LANE2 ? 2u : f == DRAW_LANE8 ? 8u : f == DRAW_WAVE1 ? 64u : (uint32_t)kMaxWords; }
inline void launch_draws(hipStream_t st, DrawForm f, const std::vector<DrawArgs>& v) {
  auto per_wave = [](const DrawArgs& a) { return dim3((a.S + 3u) / 4u); };
  auto per_lane = [](const DrawArgs& a) { return dim3((a.S + 255u) / 256u); };
  switch (f) {
    case DRAW_LANE2: launch_list<kWideSlots>(st, draw_table_lane_kernel<2>, v, 256, 0, 1, per_lane); break;
    case DRAW_LANE8: launch_list<kWideSlots>(st, draw_table_lane_kernel<8>, v, 256, 0, 1, per_lane); break;
    case DRAW_WAVE1: launch_list<kWideSlots>(st, draw_table_kernel<1>, v, 256, 0, 1, per_wave); break;
    default: launch_list<kWideSlots>(st, draw_table_kernel<kWPL>, v, 256, 0, 1, per_wave); break;
  }
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
