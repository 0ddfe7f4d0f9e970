// Hypothesis evaluation (K8, selectWithinDistance, sac_model_registration_graph.h:171-269): EvalArgs, the gate of one hypothesis
// (gate_eval: induced sample sub-graph, degree test, clique search) and eval_kernel.
// Included by verify.hip inside its anonymous namespace, after verify_kernels.h, verify_launch.h and verify_clique.h.

constexpr uint32_t kAdjcScratchWords = 256u * 1024u;   // 2 MB per deferred hypothesis: m * ceil(m/64) <= 262144 -> m <= 4064

struct EvalArgs {
  ObjJob job;
  const uint32_t* iter_samples;   // 3 per iteration
  uint32_t it_begin, it_end;      // iterations of this batch
  int32_t* counts;                // consensus size per iteration (0 = rejected by the gate)
  uint32_t* gate_m;               // per iteration: |F| when the gate ran (diagnostics), else 0
  uint32_t* work;                 // atomic work counter (zeroed by the host)
  EvalStatus* status;
  uint32_t* deferred;             // iteration indices that need the big-LDS pass
  uint16_t* stacks;               // per resident wave: stack_cap entries
  uint32_t stack_cap;
  uint32_t lds_bytes;
  uint32_t from_deferred;         // 1: the work list is `deferred`
  uint32_t n_deferred;
  u64* adjc_scratch;              // deferred pass only: kAdjcScratchWords u64 per block for graphs beyond the LDS
  uint32_t* dbg;                  // optional: per iteration dbg_stride words {cnt, m, F members...}
  uint32_t dbg_stride;
  uint32_t stop_level;            // 0 = full evaluation, 1 = stop before the clique search (diagnostics)
  const uint32_t* n_items_dev;    // optional: only the first *n_items_dev items exist (an evaluation launched in the tick of the walk
                                  // that draws its iterations: ChainOut::n_done)
};

// The gate of one hypothesis (sac_model_registration_graph.h:219-265): induced sample sub-graph of F, degree test,
// maximum clique. Returns the consensus count to report (cnt, 0 = rejected, INT_MIN = error).
// F carries the slices its caller's objects need (eval_kernel: one for W <= 64 words, kWPL for any object).
template <bool kExt, bool kWide, int kSlices>
__device__ __forceinline__ int32_t gate_eval(const EvalArgs& A, const WaveBitsT<kSlices>& F, uint32_t m, uint32_t it, uint32_t cnt,
                                             unsigned char* lds_raw, uint16_t* stack) {
  const uint32_t l = lane_id();
  const ObjJob& job = A.job;
  const uint32_t W = job.W;
  int32_t result = (int32_t)cnt;
  const uint32_t MW = (m + 63u) / 64u;
  // An object of up to 1024 matches whose consensus list needs as many 64-bit words as the object itself (MW == W: the usual
  // case when the object is really there) keeps the object's vertex numbers: the induced graph is then the object's sample rows
  // masked with F, a copy, instead of a column compaction that costs ~200 k cycles for 264 vertices; vertex numbers only ever
  // serve as row / bit indices and in comparisons, and F is ascending, so the search cannot tell the difference.
  const bool ident = !kExt && W <= (kWide ? 16u : 8u) && MW == W && gate_lds_bytes(m) + 8u * (job.n - m) * MW <= A.lds_bytes;
  GateLds L = gate_carve<kExt>(lds_raw, m, A.lds_bytes, kExt ? A.adjc_scratch + (size_t)blockIdx.x * kAdjcScratchWords : nullptr,
                               ident ? job.n : m);
  const long long t_start = A.dbg ? clock64() : 0;   // phase stamps (diagnostics builds of the call only)
  // F in ascending order (:219) -> graph index = rank (:241-243)
  uint32_t base = 0;
#pragma unroll
  for (int j = 0; j < kSlices; ++j) {
    const uint32_t c = (uint32_t)__popcll(F.w[j]);
    const uint32_t incl = wave_incl_scan(c);
    u64 w = F.w[j];
    uint32_t o = base + incl - c;
    while (w) {
      const uint32_t bit = (uint32_t)__ffsll((long long)w) - 1u;
      L.flist[o++] = (uint16_t)((j * 64u + l) * 64u + bit);
      w &= w - 1ull;
    }
    base += uni(__shfl(incl, 63));
  }
  __syncthreads();
  // induced sample sub-graph (:245-256) as an m x MW bit matrix in LDS, plus vertex degrees
  const long long t_flist = A.dbg ? clock64() : 0;
  bool bad_index = false;
  for (uint32_t g = l; g < m; g += 64u) bad_index = bad_index || L.flist[g] >= job.n;
  bad_index = __ballot(bad_index) != 0ull;           // never dereference an unchecked index
  if (bad_index && l == 0) { atomicExch(&A.status->error, 4u); A.status->detail_m = m; A.status->detail_it = it; }
  if (!bad_index && A.stop_level != 3u) {
    if (ident) {
      if (l < W) L.mask[l] = F.w[0];                       // lane l holds word l of F (W <= 16 < 64)
      __syncthreads();
      for (uint32_t i = l; i < job.n * W; i += 64u) {
        const uint32_t v = i / W, w = i - v * W;
        const bool member = (L.mask[v >> 6] >> (v & 63u)) & 1ull;
        L.adjc[i] = member ? (job.samp[i] & L.mask[w]) : 0ull;
      }
      __syncthreads();
      for (uint32_t g = l; g < m; g += 64u) {
        const u64* row = L.adjc + (size_t)L.flist[g] * MW;
        uint32_t d = 0;
        for (uint32_t w = 0; w < MW; ++w) d += (uint32_t)__popcll(row[w]);
        L.deg[g] = d;
      }
    } else if (W <= 8u) {
      // n <= 512: lane = one row of the induced graph, its whole sample row (<= 16 dwords) in registers;
      // the members of F are walked once per 64 rows, one v_readlane + bit-field extract + shift-or each.
      // F is ascending, so the source dword only ever moves forward.
      uint32_t fl[kRegChunks];
#pragma unroll
      for (uint32_t c = 0; c < kRegChunks; ++c) fl[c] = (c * 64u + l) < m ? L.flist[c * 64u + l] : 0u;
      for (uint32_t rc = 0; rc < MW; ++rc) {
        const uint32_t grow = rc * 64u + l;
        const bool have = grow < m;
        const uint32_t myv = have ? (uint32_t)L.flist[grow] : 0u;
        uint32_t rw[16];
        {
          const uint32_t* src = reinterpret_cast<const uint32_t*>(job.samp + (size_t)myv * W);
#pragma unroll
          for (uint32_t w = 0; w < 16u; ++w) rw[w] = (have && w < 2u * W) ? src[w] : 0u;
        }
        uint32_t out[2u * kRegChunks];
#pragma unroll
        for (uint32_t c = 0; c < 2u * kRegChunks; ++c) out[c] = 0u;
        uint32_t wcur = 0xFFFFFFFFu, word = 0u;
#pragma unroll
        for (uint32_t cj = 0; cj < 2u * kRegChunks; ++cj) {      // 32 positions per step: the target dword is static
          if (cj * 32u < m) {                                     // wave-uniform
            const uint32_t cnt = min(32u, m - cj * 32u);
            for (uint32_t lj = 0; lj < cnt; ++lj) {
              const uint32_t h = rdlane(fl[cj >> 1], (cj & 1u) * 32u + lj);
              if ((h >> 5) != wcur) {                             // wave-uniform, at most 2 W times per 64 rows
                wcur = h >> 5;
#pragma unroll
                for (uint32_t w = 0; w < 16u; ++w) if (wcur == w) word = rw[w];
              }
              out[cj] |= ((word >> (h & 31u)) & 1u) << lj;
            }
          }
        }
        if (have) {
          uint32_t d = 0;
#pragma unroll
          for (uint32_t c = 0; c < kRegChunks; ++c) {
            if (c < MW) {
              const u64 wv = ((u64)out[2u * c + 1u] << 32) | out[2u * c];
              L.adjc[(size_t)grow * MW + c] = wv;
              d += (uint32_t)__popcll(wv);
            }
          }
          L.deg[grow] = d;
        }
      }
    } else if (W <= 64u) {
      // lane l holds word l of a row; kRows rows are in flight so the global latency is paid once per group
      constexpr uint32_t kRows = 8;
      for (uint32_t g0 = 0; g0 < m; g0 += kRows) {
        u64 rw[kRows];
#pragma unroll
        for (uint32_t j = 0; j < kRows; ++j) {
          const uint32_t g = g0 + j;
          rw[j] = (g < m && l < W) ? job.samp[(size_t)uni(L.flist[g < m ? g : 0u]) * W + l] : 0ull;
        }
#pragma unroll
        for (uint32_t j = 0; j < kRows; ++j) {
          const uint32_t g = g0 + j;
          if (g < m) {                               // wave-uniform
            uint32_t d = 0;
            for (uint32_t c = 0; c < MW; ++c) {
              const uint32_t pos = c * 64u + l;
              const uint32_t h = pos < m ? L.flist[pos] : 0u;
              const bool adj = row_test(rw[j], h) && pos < m;
              const u64 bal = __ballot(adj);
              if (l == 0) L.adjc[(size_t)g * MW + c] = bal;
              d += (uint32_t)__popcll(bal);
            }
            if (l == 0) L.deg[g] = d;
          }
        }
      }
    } else {
      for (uint32_t g = 0; g < m; ++g) {
        const u64* row = job.samp + (size_t)uni(L.flist[g]) * W;
        uint32_t d = 0;
        for (uint32_t c = 0; c < MW; ++c) {
          const uint32_t pos = c * 64u + l;
          bool adj = false;
          if (pos < m) { const uint32_t h = L.flist[pos]; adj = (row[h >> 6] >> (h & 63u)) & 1ull; }
          const u64 bal = __ballot(adj);
          if (l == 0) L.adjc[(size_t)g * MW + c] = bal;
          d += (uint32_t)__popcll(bal);
        }
        if (l == 0) L.deg[g] = d;
      }
    }
  }
  __syncthreads();
  const long long t_adjc = A.dbg ? clock64() : 0;
  if (A.dbg) {
    uint32_t* d = A.dbg + (size_t)it * A.dbg_stride;
    if (l == 0) { d[0] = cnt; d[1] = m; }
    for (uint32_t g = l; g < m && 2u + 2u * g + 1u < A.dbg_stride; g += 64u) { d[2 + 2 * g] = L.flist[g]; d[3 + 2 * g] = L.deg[g]; }
  }
  // "make sure that those inliers have enough neighbors within the inliers themselves" (:221-238)
  bool any = false;
  for (uint32_t g = l; g < m; g += 64u) any = any || L.deg[g] > kGateMinimal;
  if (bad_index) {
    result = INT_MIN;
  } else if (A.stop_level != 0u) {
    result = -(int32_t)m;
  } else if (__ballot(any) == 0ull) {
    result = 0;
  } else {
    int err = 0;
    uint32_t steps = 0;
    uint32_t* prof = (A.dbg && A.dbg_stride >= 16u) ? A.dbg + (size_t)it * A.dbg_stride + (A.dbg_stride - 12u) : nullptr;
    const uint32_t q = clique_search<kWide, true>(L, m, kGateMinimal, stack, A.stack_cap, &err, &steps, prof, ident ? L.flist : nullptr);
    if (A.dbg && l == 0 && A.dbg_stride >= 8u) {
      uint32_t* d = A.dbg + (size_t)it * A.dbg_stride + (A.dbg_stride - 6u);
      d[0] = (uint32_t)(t_flist - t_start); d[1] = (uint32_t)(t_adjc - t_flist);
      d[2] = (uint32_t)(clock64() - t_adjc); d[3] = steps; d[4] = q;
    }
    if (err) {
      if (l == 0) atomicExch(&A.status->error, 1u);
      result = INT_MIN;
    } else if (q <= kGateMinimal) {
      result = 0;                                    // :260-265
    }
    if (l == 0) atomicAdd(&A.status->gate_calls, 1u);
  }
  __syncthreads();
  return result;
}

// The argument set of a block. By value in kernarg it is scalar already. Staged in device memory (written by the host before the
// launch, constant for the kernel's lifetime) it is read once through the constant address space into scalar registers: read
// through the plain pointer its fields and their addresses sat in 23 vector registers across the clique search.
template <class A, uint32_t N>
__device__ __forceinline__ const A& arg_set(const Slots<A, N>& S, uint32_t i) { return S.a[i]; }
template <class A>
__device__ __forceinline__ A arg_set(const SlotsPtr<A>& S, uint32_t i) {
  A r;
  __builtin_memcpy(&r, (const __attribute__((address_space(4))) A*)(S.a + i), sizeof(A));
  return r;
}

// launched with 64 threads; the bound is deliberately larger so that hipcc keeps __syncthreads() as a real,
// convergent s_barrier (with a 64-thread bound it drops the barrier and may split the lanes of the wave)
// kWide = false: objects of up to 512 matches (job.W <= 8), the launch's every slot, so P and F are one slice of 64 words;
// true: any size, eight slices
// kDeferred: the second pass over the hypotheses the first one deferred (A.from_deferred, big LDS). Only it can take the third tier
// (adjacency in global scratch), so only its instantiations carry gate_eval<true>: with both tiers inlined side by side the
// first pass held 10 registers more across the search, and it is the first pass that has to start beside the DB pass's waves.
template <bool kWide, class H = Slots<EvalArgs>, bool kDeferred = false>
__global__ __launch_bounds__(128) void eval_kernel(H SL) {
  TOD_LATENCY_PRIO();   // latency-bound: win issue arbitration against the VALU-saturating matcher
  const EvalArgs& A = arg_set(SL, blockIdx.y);
  extern __shared__ __align__(16) unsigned char lds_raw[];
  const uint32_t l = lane_id();
  const ObjJob& job = A.job;
  const uint32_t W = job.W;
  uint16_t* stack = A.stacks + (size_t)blockIdx.x * A.stack_cap;
  uint32_t n_items = kDeferred ? A.n_deferred : (A.it_end - A.it_begin);
  if (A.n_items_dev) n_items = min(n_items, uni(*A.n_items_dev));
  {                                                        // one block = one hypothesis
    const uint32_t item = blockIdx.x;
    if (item >= n_items) return;
    const uint32_t it = uni(kDeferred ? A.deferred[item] : (A.it_begin + item));
    const uint32_t s0 = uni(A.iter_samples[3 * it]), s1 = uni(A.iter_samples[3 * it + 1]),
                   s2 = uni(A.iter_samples[3 * it + 2]);
    if (s0 >= job.n || s1 >= job.n || s2 >= job.n) {       // corrupt draw table: report, never dereference
      if (l == 0) { atomicExch(&A.status->error, 3u); A.counts[it] = INT_MIN; }
      return;
    }
    // common physical neighbours of the three samples (:178-184); the geometric test of :197 is
    // `finite < +inf` because threshold_ is DBL_MAX (D2), i.e. a finiteness test
    typedef WaveBitsT<kWide ? kWPL : 1> Bits;
    Bits P;
    wb_load(P, job.phys + (size_t)s0 * W, W);
    wb_and(P, job.phys + (size_t)s1 * W, W);
    wb_and(P, job.phys + (size_t)s2 * W, W);
    wb_and(P, job.valid, W);
    wb_and(P, job.finite, W);
    const uint32_t cnt = wb_count(P) + 3u;                 // + the samples themselves (:185-186)
    int32_t result = (int32_t)cnt;
    uint32_t m_diag = 0;
    if (cnt > kGateMinimal && A.stop_level != 2u) {        // :203-205
      Bits F = P;
      wb_set(F, s0); wb_set(F, s1); wb_set(F, s2);
      wb_and(F, job.deg7, W);                              // :211-213
      const uint32_t m = wb_count(F);
      m_diag = m;
      if (m <= kGateMinimal) {
        result = 0;                                        // :214-218
      } else if (gate_lds_bytes(m) > A.lds_bytes &&
                 !(kDeferred && A.adjc_scratch && gate_small_bytes(m) <= A.lds_bytes &&
                   m * ((m + 63u) / 64u) <= kAdjcScratchWords)) {
        if (kDeferred) {
          if (l == 0) atomicExch(&A.status->error, 2u);        // graph too large even with the adjacency in global memory
          result = INT_MIN;
        } else {
          if (l == 0) A.deferred[atomicAdd(&A.status->n_deferred, 1u)] = it;
          result = INT_MIN + 1;                            // filled in by the second pass
        }
      } else if constexpr (kDeferred) {
        // third tier: adjacency matrix in global scratch
        result = gate_lds_bytes(m) > A.lds_bytes ? gate_eval<true, kWide>(A, F, m, it, cnt, lds_raw, stack)
                                                 : gate_eval<false, kWide>(A, F, m, it, cnt, lds_raw, stack);
      } else {
        result = gate_eval<false, kWide>(A, F, m, it, cnt, lds_raw, stack);
      }
    }
    if (l == 0) {
      if (result != INT_MIN + 1) A.counts[it] = result;
      if (A.gate_m) A.gate_m[it] = m_diag;
    }
  }
}
