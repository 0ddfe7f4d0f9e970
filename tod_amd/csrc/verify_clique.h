// The maximum-clique search of the gate (maximum_clique.cpp:263-369: DegreeSort, ColorSort, Intersection, FindClique) on a bit matrix
// in LDS or global scratch, with its LDS carve, rank sorts and colourings, and the stand-alone test kernel on an explicit graph.
// Included by verify.hip inside its anonymous namespace, after verify_kernels.h.

// ------------------------------------------------------------------------------------------------ K8
struct GateLds {
  u64* adjc;                                   // m x MW induced sample adjacency, graph index = rank in F
  u64* mask;                                   // MW
  uint16_t *flist, *cur, *nxt, *tmp;           // m each
  uint32_t *C, *deg, *keys;                    // m each
  uint32_t *S, *SOld, *lbase, *lsize, *lcap;   // m + 2 each
  uint32_t* trash;                             // 64 words: where the lanes that have nothing to record write (colour_first_fit64)
  uint16_t* lstack;                            // LDS part of the per-level vertex lists (the rest is in global memory)
  uint32_t lstack_cap;
};
__host__ __device__ inline uint32_t gate_lds_bytes(uint32_t m) {
  const uint32_t MW = (m + 63u) / 64u, ma = (m + 7u) & ~3u;      // ma >= m + 2
  return 8u * m * MW + 8u * MW + 8u * 4u * ma + 4u * 2u * ma + 256u + 64u;
}
__host__ __device__ inline uint32_t gate_small_bytes(uint32_t m) {           // everything except the adjacency matrix
  const uint32_t MW = (m + 63u) / 64u, ma = (m + 7u) & ~3u;
  return 8u * MW + 8u * 4u * ma + 4u * 2u * ma + 256u + 64u;
}
// ext_adjc != nullptr: the m x MW matrix lives in global scratch (graphs beyond one CU's LDS); same code path,
// the pointers are generic
// kExt is a template parameter so that, in the LDS instantiation, every pointer provably comes from the LDS allocation:
// the compiler then emits ds_read/ds_write for the adjacency rows instead of flat loads (the rows are on the critical
// path of Intersection and ColorSort)
// rows: how many adjacency rows to make room for (m, or the object's n when the graph keeps the object's vertex numbers)
template <bool kExt>
__device__ __forceinline__ GateLds gate_carve(unsigned char* base, uint32_t m, uint32_t lds_bytes, u64* ext_adjc = nullptr, uint32_t rows = 0) {
  const uint32_t MW = (m + 63u) / 64u, ma = (m + 7u) & ~3u;
  if (rows == 0u) rows = m;
  unsigned char* const base0 = base;
  GateLds L;
  if constexpr (kExt) { L.adjc = ext_adjc; } else { L.adjc = reinterpret_cast<u64*>(base); base += 8u * rows * MW; }
  L.mask = reinterpret_cast<u64*>(base); base += 8u * MW;
  L.C = reinterpret_cast<uint32_t*>(base); base += 4u * ma;
  L.deg = reinterpret_cast<uint32_t*>(base); base += 4u * ma;
  L.keys = reinterpret_cast<uint32_t*>(base); base += 4u * ma;
  L.S = reinterpret_cast<uint32_t*>(base); base += 4u * ma;
  L.SOld = reinterpret_cast<uint32_t*>(base); base += 4u * ma;
  L.lbase = reinterpret_cast<uint32_t*>(base); base += 4u * ma;
  L.lsize = reinterpret_cast<uint32_t*>(base); base += 4u * ma;
  L.lcap = reinterpret_cast<uint32_t*>(base); base += 4u * ma;
  L.trash = reinterpret_cast<uint32_t*>(base); base += 256u;
  L.flist = reinterpret_cast<uint16_t*>(base); base += 2u * ma;
  L.cur = reinterpret_cast<uint16_t*>(base); base += 2u * ma;
  L.nxt = reinterpret_cast<uint16_t*>(base); base += 2u * ma;
  L.tmp = reinterpret_cast<uint16_t*>(base); base += 2u * ma;
  // whatever the launch's LDS allocation has left is the first part of the level stack
  uint32_t used = ((uint32_t)(base - base0) + 15u) & ~15u;
  L.lstack = reinterpret_cast<uint16_t*>(base0 + used);
  L.lstack_cap = lds_bytes > used ? (lds_bytes - used) / 2u : 0u;
  return L;
}

// per-level vertex lists: entry i lives in LDS while it fits, in the wave's global stack beyond
struct LevelStack { uint16_t* lds; uint32_t lds_cap; uint16_t* glob; };
__device__ __forceinline__ uint16_t stk_get(const LevelStack& s, uint32_t i) {
  return i < s.lds_cap ? s.lds[i] : s.glob[i - s.lds_cap];
}
__device__ __forceinline__ void stk_put(const LevelStack& s, uint32_t i, uint16_t v) {
  if (i < s.lds_cap) s.lds[i] = v; else s.glob[i - s.lds_cap] = v;
}

__device__ __forceinline__ bool row_test(u64 roww, uint32_t h) {   // roww: lane l holds word l of the row
  const u64 wv = shfl64(roww, h >> 6);
  return (wv >> (h & 63u)) & 1ull;
}

constexpr uint32_t kRegChunks = 8;                         // the column compaction's register path covers graphs of up to 512 vertices
constexpr uint32_t kSortChunks = 16;                       // DegreeSort's register path: lists of up to 1024 vertices

// DegreeSort (maximum_clique.cpp:263-284): (degree inside the list, vertex) ascending, then reversed.
// deg[] must hold the degree of list[i] at position i. Rank by counting; keys are unique.
// keys stay in registers (lane l: positions l, l + 64, ...); every key is broadcast once with v_readlane. NCH = chunks of 64
// positions, a template parameter so that the per-key work is straight-line code over exactly NCH registers.
template <uint32_t NCH>
__device__ __forceinline__ void rank_sort_regs(uint16_t* list, const uint32_t* deg, uint32_t r) {
  const uint32_t l = lane_id();
  uint32_t kreg[NCH], rank[NCH];
#pragma unroll
  for (uint32_t c = 0; c < NCH; ++c) {
    const uint32_t i = c * 64u + l;
    kreg[c] = i < r ? ((deg[i] << 16) | list[i]) : 0u;
    rank[c] = 0u;
  }
#pragma unroll
  for (uint32_t cj = 0; cj < NCH; ++cj) {
    const uint32_t cnt = cj * 64u < r ? min(64u, r - cj * 64u) : 0u;   // (the last chunk of a merged case may be empty)
    for (uint32_t lj = 0; lj < cnt; ++lj) {
      const uint32_t kj = rdlane(kreg[cj], lj);
#pragma unroll
      for (uint32_t c = 0; c < NCH; ++c) rank[c] += (kj > kreg[c]) ? 1u : 0u;
    }
  }
  __syncthreads();                                         // every lane holds its keys: the list can be overwritten
#pragma unroll
  for (uint32_t c = 0; c < NCH; ++c)
    if (c * 64u + l < r) list[rank[c]] = (uint16_t)(kreg[c] & 0xFFFFu);
  __syncthreads();
}

// kWide: the instantiation for objects of 513..1024 matches (eval_kernel<true>); the narrow one carries none of its code, so that
// the registers of the common case are allocated as if the wide case did not exist (it costs 6 % otherwise)
template <bool kWide>
__device__ __forceinline__ void rank_sort_desc(uint16_t* list, uint16_t* tmp, const uint32_t* deg, uint32_t r, uint32_t* keys) {
  const uint32_t l = lane_id();
  if (r <= kRegChunks * 64u) {
    switch ((r + 63u) / 64u) {                             // wave-uniform
      case 0: case 1: rank_sort_regs<1>(list, deg, r); break;
      case 2: rank_sort_regs<2>(list, deg, r); break;
      case 3: rank_sort_regs<3>(list, deg, r); break;
      case 4: rank_sort_regs<4>(list, deg, r); break;
      case 5: rank_sort_regs<5>(list, deg, r); break;
      case 6: rank_sort_regs<6>(list, deg, r); break;
      case 7: rank_sort_regs<7>(list, deg, r); break;
      default: rank_sort_regs<8>(list, deg, r); break;
    }
    return;
  }
  if constexpr (kWide) {
    if (r <= kSortChunks * 64u) {
      switch ((r + 63u) / 64u) {                           // wave-uniform
        case 9: rank_sort_regs<9>(list, deg, r); break;
        case 10: rank_sort_regs<10>(list, deg, r); break;
        case 11: rank_sort_regs<11>(list, deg, r); break;
        case 12: rank_sort_regs<12>(list, deg, r); break;
        case 13: case 14: rank_sort_regs<14>(list, deg, r); break;
        default: rank_sort_regs<16>(list, deg, r); break;
      }
      return;
    }
  }
  for (uint32_t i = l; i < r; i += 64u) keys[i] = (deg[i] << 16) | list[i];
  __syncthreads();
  for (uint32_t i0 = 0; i0 < r; i0 += 64u) {
    const uint32_t i = i0 + l;
    const uint32_t mine = i < r ? keys[i] : 0u;
    uint32_t rank = 0;
    for (uint32_t j = 0; j < r; ++j) rank += keys[j] > mine;
    if (i < r) tmp[rank] = (uint16_t)(mine & 0xFFFFu);
  }
  __syncthreads();
  for (uint32_t i = l; i < r; i += 64u) list[i] = tmp[i];
  __syncthreads();
}

// degrees of the members of list[0..r) inside the list, into L.deg[0..r)
__device__ __forceinline__ void degrees_in_list(const GateLds& L, const uint16_t* list, uint32_t r, uint32_t MW) {
  const uint32_t l = lane_id();
  if (l < MW) L.mask[l] = 0ull;
  __syncthreads();
  for (uint32_t i = l; i < r; i += 64u) atomicOr(&L.mask[list[i] >> 6], 1ull << (list[i] & 63u));
  __syncthreads();
  for (uint32_t i = l; i < r; i += 64u) {
    const u64* row = L.adjc + (size_t)list[i] * MW;
    uint32_t d = 0;
    for (uint32_t w = 0; w < MW; ++w) d += (uint32_t)__popcll(row[w] & L.mask[w]);
    L.deg[i] = d;
  }
  __syncthreads();
}

// The same first-fit colouring for at most 64 classes, with nothing but vector instructions between one vertex and the next. A lone
// wave pays for every hand-over between the vector and the scalar unit (ballot -> find-first-set -> lane compare -> exec mask, the
// shape of colour_first_fit below, costs ~530 cycles per vertex for ~45 instructions). Here the first free class is found
// lane-locally: the free-class mask stays in VCC, v_mbcnt counts the free classes below each lane, the one lane that is free
// with none below it joins -- a select and an or on its own registers. What ColorSort needs for its output order, (class, rank
// inside the class) per list position, is written by that lane itself: every lane stores one word, the others into a trash slot.
// Returns false (nothing written to the list or to C) when some vertex found all 64 classes taken: the caller then runs the
// two-set form below.
template <uint32_t MWT>
__device__ __forceinline__ bool colour_first_fit64(const GateLds& L, uint16_t* list, uint32_t r) {
  typedef uint32_t u32x16 __attribute__((ext_vector_type(MWT <= 8u ? 16 : 32)));   // (2 MWT halves; the tuple sizes the hardware indexes)
  const uint32_t l = lane_id();
  // class l's members as a bitset over graph vertices, 32-bit halves in ONE register tuple: the half that receives a vertex is
  // picked with the hardware's register indexing (s_set_gpr_idx, the index v >> 5 is wave-uniform) -- three instructions to read,
  // three to write, no branch tree and no per-word selects
  u32x16 cls = {};
  uint32_t rec = l << 16;                                  // (class l, members of class l so far): what a joining vertex records
  uint32_t* const my_trash = L.trash + l;
  for (uint32_t c0 = 0; c0 < r; c0 += 64u) {
    const uint32_t cnt = min(64u, r - c0);
    // lanes past the list hold its last vertex, so that the row prefetch one vertex ahead needs no clamp (lane 64 wraps to lane 0:
    // any vertex will do, the row is never used); and every lane keeps the BYTE offset of its vertex's row next to the vertex
    const uint32_t vmine = (uint32_t)list[min(c0 + l, r - 1u)];
    const uint32_t voff = vmine * (MWT * 8u);
    auto place = [&](const u64 (&row)[MWT], u64 (&next)[MWT], uint32_t li) {
      const uint32_t v = rdlane(vmine, li);
      {
        const u64* g = reinterpret_cast<const u64*>(reinterpret_cast<const unsigned char*>(L.adjc) + rdlane(voff, (li + 1u) & 63u));
#pragma unroll
        for (uint32_t w = 0; w < MWT; ++w) next[w] = g[w];
      }
      // (row & class) over all halves: one v_and_or per half. Left to itself the compiler builds and + and + or3 trees, three
      // instructions per two halves, which is shallower but longer -- and a lone wave is bound by what it must issue, not by depth
      uint32_t hit32 = (uint32_t)row[0] & cls[0];
      {
        const uint32_t rh = (uint32_t)(row[0] >> 32), ch = cls[1];
        asm("v_and_or_b32 %0, %1, %2, %0" : "+v"(hit32) : "v"(rh), "v"(ch));
      }
#pragma unroll
      for (uint32_t w = 1; w < MWT; ++w) {
        const uint32_t rl = (uint32_t)row[w], rh = (uint32_t)(row[w] >> 32), cl = cls[2u * w], ch = cls[2u * w + 1u];
        asm("v_and_or_b32 %0, %1, %2, %0" : "+v"(hit32) : "v"(rl), "v"(cl));
        asm("v_and_or_b32 %0, %1, %2, %0" : "+v"(hit32) : "v"(rh), "v"(ch));
      }
      const u64 fm = __ballot(hit32 == 0u);                // classes without a neighbour of v
      const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(fm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)fm, 0u));
      const uint32_t lw = hit32 == 0u ? below : 1u;
      const bool join = lw == 0u;                          // the first free class: exactly one lane, or none (overflow)
      uint32_t* const dst = join ? (L.keys + (c0 + li)) : my_trash;
      *dst = rec;                                          // (class, rank inside the class) of position c0 + li
      rec += join ? 1u : 0u;
      cls[v >> 5] |= join ? (1u << (v & 31u)) : 0u;
    };
    u64 rowA[MWT], rowB[MWT];
    {
      const u64* g = L.adjc + (size_t)rdlane(vmine, 0u) * MWT;
#pragma unroll
      for (uint32_t w = 0; w < MWT; ++w) rowA[w] = g[w];
    }
    uint32_t li = 0;
    for (; li + 2u <= cnt; li += 2u) {                     // two vertices per trip: the row buffers swap roles, nothing is copied
      place(rowA, rowB, li);
      place(rowB, rowA, li + 1u);
    }
    if (li < cnt) place(rowA, rowB, li);
  }
  const uint32_t cnt0 = rec & 0xFFFFu;                     // members of class l
  const uint32_t incl0 = wave_incl_scan(cnt0), total0 = uni(__shfl(incl0, 63));
  if (total0 != r) return false;                           // a vertex found no free class among 64
  const uint32_t base0 = incl0 - cnt0;
  __syncthreads();
  for (uint32_t i = l; i < r + 63u - ((r + 63u) & 63u); i += 64u) {   // whole waves: the shuffles need every lane
    const uint32_t rec = i < r ? L.keys[i] : 0u;
    const uint32_t k = rec >> 16;
    const uint32_t b = __shfl(base0, k & 63u);
    if (i < r) {
      const uint32_t pos = b + (rec & 0xFFFFu);
      L.tmp[pos] = list[i];
      L.C[pos] = k + 1u;
    }
  }
  __syncthreads();
  for (uint32_t i = l; i < r; i += 64u) list[i] = L.tmp[i];
  __syncthreads();
  return true;
}

// ColorSort (maximum_clique.cpp:219-261) on list[0..r), writing colours into the shared array C by absolute
// position (decision D3). With min_k == 1 every vertex joins a class and first-fit colouring in list order
// equals colouring class by class (each class = greedy independent set in list order), which is what the
// bit-parallel loop below does. With min_k >= 2 class 1 is never filled (:242-245), so every vertex gets
// k = 1 < min_k, the order is unchanged and only C[r-1] = 0 is written (:247-248).
// First-fit colouring in list order with one LANE per colour class (graphs of up to 512 vertices).
// ColorSort (maximum_clique.cpp:219-261) gives vertex i the smallest class none of whose members it is adjacent to; lane c
// keeps class c's members as a bitset over GRAPH vertices in MWT registers, so "is v adjacent to a member of class c" is
// (row_v & class_c) != 0 for all classes at once: MWT broadcast LDS reads of row_v (prefetched: the list order is known),
// MWT and-or pairs, one ballot, one find-first-set. Nothing on the critical path waits for LDS, and no position-space
// adjacency has to be built (the class-by-class forms that this replaces paid ~600 cycles per coloured vertex for both).
// A second register set serves classes 64..127 once the first 64 are in use; with more than 128 classes the caller falls
// back to the generic class-by-class loop. Output as ColorSort's: the list regrouped by class (each class in list order),
// C[position] = class.
// WIDE = false: classes 0..63 only (one register set); returns false as soon as a vertex finds all 64 taken, and the caller
// starts over with WIDE = true (two sets, 128 classes). Lists that need more than 64 classes are rare (dense graphs of
// several hundred vertices), so the common loop carries no second set and no range checks.
template <uint32_t MWT, bool WIDE>
__device__ __forceinline__ bool colour_first_fit(const GateLds& L, uint16_t* list, uint32_t r) {
  const uint32_t l = lane_id();
  u64 cls0[MWT], cls1[WIDE ? MWT : 1];
#pragma unroll
  for (uint32_t w = 0; w < MWT; ++w) cls0[w] = 0ull;
#pragma unroll
  for (uint32_t w = 0; w < (WIDE ? MWT : 1); ++w) cls1[w] = 0ull;
  uint32_t cnt0 = 0u, cnt1 = 0u;                           // members of class l / class 64 + l so far
  bool wide = false, overflow = false;                     // wave-uniform
  for (uint32_t c0 = 0; c0 < r; c0 += 64u) {
    const uint32_t cnt = min(64u, r - c0);
    const uint32_t vmine = (c0 + l) < r ? (uint32_t)list[c0 + l] : 0u;
    uint32_t rec = 0u;                                     // lane li: (class << 16 | index inside the class) of position c0 + li
    // one vertex. Its adjacency row is loaded here, not one vertex ahead as colour_first_fit64 does: with two class sets a second
    // row buffer made this rare form the register peak of the whole hypothesis kernel (16 registers at MWT = 8)
    auto place = [&](uint32_t li) {
      const uint32_t v = rdlane(vmine, li);
      u64 row[MWT];
      {
        const u64* g = L.adjc + (size_t)v * MWT;
#pragma unroll
        for (uint32_t w = 0; w < MWT; ++w) row[w] = g[w];
      }
      u64 hit = 0ull;
#pragma unroll
      for (uint32_t w = 0; w < MWT; ++w) hit |= row[w] & cls0[w];
      const u64 free0 = __ballot(hit == 0ull);
      uint32_t k = 0u;
      bool second = false;
      if (free0 != 0ull) {
        k = (uint32_t)__ffsll((long long)free0) - 1u;
      } else if (WIDE) {
        wide = true; second = true;
        u64 hit1 = 0ull;
#pragma unroll
        for (uint32_t w = 0; w < (WIDE ? MWT : 1); ++w) hit1 |= row[w] & cls1[w];
        const u64 free1 = __ballot(hit1 == 0ull);
        if (free1 == 0ull) overflow = true; else k = (uint32_t)__ffsll((long long)free1) - 1u;
      } else {
        overflow = true;
      }
      // vertex v joins class k (of the first or second set): only lane k executes the update; which register pair receives
      // the bit is a scalar branch on the (wave-uniform) word index, so the arrays are only ever indexed statically and stay
      // in registers, and one word is touched instead of all of them
      const uint32_t vw = v >> 6;
      const u64 bit = 1ull << (v & 63u);
      const uint32_t idx = second ? rdlane(cnt1, k) : rdlane(cnt0, k);
      if (l == k) {
        if (!second) {
          cnt0 += 1u;
#pragma unroll
          for (uint32_t w = 0; w < MWT; ++w)
            if (vw == w) { cls0[w] |= bit; asm volatile("" ::: "memory"); }   // (the empty asm keeps this a branch, not MWT selects)
        } else if (WIDE) {
          cnt1 += 1u;
#pragma unroll
          for (uint32_t w = 0; w < (WIDE ? MWT : 1); ++w)
            if (vw == w) { cls1[w] |= bit; asm volatile("" ::: "memory"); }
        }
      }
      if (l == li) rec = ((second ? k + 64u : k) << 16) | idx;
    };
    for (uint32_t li = 0; li < cnt && !overflow; ++li) place(li);
    if (overflow) return false;                            // nothing has been written to the list or to C
    if (c0 + l < r) L.keys[c0 + l] = rec;
  }
  // class c's block starts after all smaller classes: exclusive prefix of the class sizes over the lanes
  const uint32_t incl0 = wave_incl_scan(cnt0), total0 = uni(__shfl(incl0, 63));
  const uint32_t base0 = incl0 - cnt0;
  uint32_t base1 = 0u;
  if (wide) { const uint32_t incl1 = wave_incl_scan(cnt1); base1 = total0 + incl1 - cnt1; }
  __syncthreads();
  for (uint32_t i = l; i < r + 63u - ((r + 63u) & 63u); i += 64u) {   // whole waves: the shuffles need every lane
    const uint32_t rec = i < r ? L.keys[i] : 0u;
    const uint32_t k = rec >> 16;
    uint32_t b = __shfl(base0, k & 63u);
    if (wide) { const uint32_t b1 = __shfl(base1, k & 63u); b = k >= 64u ? b1 : b; }
    if (i < r) {
      const uint32_t pos = b + (rec & 0xFFFFu);
      L.tmp[pos] = list[i];
      L.C[pos] = k + 1u;
    }
  }
  __syncthreads();
  for (uint32_t i = l; i < r; i += 64u) list[i] = L.tmp[i];
  __syncthreads();
  return true;
}

template <bool kWide>
__device__ __forceinline__ void colour_sort(const GateLds& L, uint16_t* list, uint32_t r, uint32_t MW, uint32_t qmax, uint32_t qsz) {
  const uint32_t l = lane_id();
  const int min_k = max(1, (int)qmax - (int)qsz + 1);
  if (min_k >= 2) {
    if (l == 0) L.C[r - 1] = 0u;
    __syncthreads();
    return;
  }
  if (r <= 2u) {
    // one or two vertices (about half of all calls deep in the tree): the order cannot change; the second vertex opens
    // class 2 iff it is adjacent to the first
    if (l == 0) {
      L.C[0] = 1u;
      if (r == 2u) {
        const uint32_t a = list[0], b = list[1];
        L.C[1] = ((L.adjc[(size_t)a * MW + (b >> 6)] >> (b & 63u)) & 1ull) ? 2u : 1u;
      }
    }
    __syncthreads();
    return;
  }
  if (MW <= 8u) {                                          // graphs of up to 512 vertices: one lane per colour class
    bool done = false;
    switch (MW) {                                          // wave-uniform
      case 1: done = colour_first_fit64<1>(L, list, r) || colour_first_fit<1, true>(L, list, r); break;
      case 2: done = colour_first_fit64<2>(L, list, r) || colour_first_fit<2, true>(L, list, r); break;
      case 3: done = colour_first_fit64<3>(L, list, r) || colour_first_fit<3, true>(L, list, r); break;
      case 4: done = colour_first_fit64<4>(L, list, r) || colour_first_fit<4, true>(L, list, r); break;
      case 5: done = colour_first_fit64<5>(L, list, r) || colour_first_fit<5, true>(L, list, r); break;
      case 6: done = colour_first_fit64<6>(L, list, r) || colour_first_fit<6, true>(L, list, r); break;
      case 7: done = colour_first_fit64<7>(L, list, r) || colour_first_fit<7, true>(L, list, r); break;
      default: done = colour_first_fit64<8>(L, list, r) || colour_first_fit<8, true>(L, list, r); break;
    }
    if (done) return;                                      // else: more than 128 classes -> the generic loop below
  }
  if constexpr (kWide) {
    if (MW > 8u && MW <= 16u) {                            // up to 1024 vertices: the same, with a 32-register class tuple
      bool done = false;
      switch (MW) {                                        // wave-uniform
        case 9: done = colour_first_fit64<9>(L, list, r) || colour_first_fit<9, true>(L, list, r); break;
        case 10: done = colour_first_fit64<10>(L, list, r) || colour_first_fit<10, true>(L, list, r); break;
        case 11: done = colour_first_fit64<11>(L, list, r) || colour_first_fit<11, true>(L, list, r); break;
        case 12: done = colour_first_fit64<12>(L, list, r) || colour_first_fit<12, true>(L, list, r); break;
        case 13: done = colour_first_fit64<13>(L, list, r) || colour_first_fit<13, true>(L, list, r); break;
        case 14: done = colour_first_fit64<14>(L, list, r) || colour_first_fit<14, true>(L, list, r); break;
        case 15: done = colour_first_fit64<15>(L, list, r) || colour_first_fit<15, true>(L, list, r); break;
        default: done = colour_first_fit64<16>(L, list, r) || colour_first_fit<16, true>(L, list, r); break;
      }
      if (done) return;
    }
  }
  // generic class-by-class colouring (graphs beyond 1024 vertices, or more than 128 classes)
  const uint32_t nchunks = (r + 63u) / 64u;
  u64 uncol = 0ull;                                        // lane c holds positions [64c, 64c + 64)
  if (l < nchunks) uncol = (l * 64u + 64u <= r) ? ~0ull : ((1ull << (r - l * 64u)) - 1ull);
  uint32_t k = 1, outpos = 0;
  while (__ballot(uncol != 0ull) != 0ull) {
    u64 Q = uncol;
    while (true) {
      const u64 balQ = __ballot(Q != 0ull);
      if (balQ == 0ull) break;
      const uint32_t ll = (uint32_t)__ffsll((long long)balQ) - 1u;
      const u64 wq = shfl64(Q, ll);
      const uint32_t bit = uni((uint32_t)__ffsll((long long)wq) - 1u);
      const uint32_t g = uni(list[ll * 64u + bit]);
      if (l == 0) { L.tmp[outpos] = (uint16_t)g; L.C[outpos] = k; }
      ++outpos;
      if (l == ll) { uncol &= ~(1ull << bit); Q &= ~(1ull << bit); }
      const u64* grow = L.adjc + (size_t)g * MW;
      for (uint32_t c = 0; c < nchunks; ++c) {
        if (!((balQ >> c) & 1ull)) continue;               // wave-uniform
        const uint32_t pos = c * 64u + l;
        bool adj = false;
        if (pos < r) { const uint32_t h = list[pos]; adj = (grow[h >> 6] >> (h & 63u)) & 1ull; }
        const u64 bal = __ballot(adj);
        if (l == c) Q &= ~bal;                             // neighbours cannot join this class
      }
    }
    ++k;
  }
  __syncthreads();
  for (uint32_t i = l; i < r; i += 64u) list[i] = L.tmp[i];
  __syncthreads();
}

// FindClique + MaxCliqueDyn (maximum_clique.cpp:286-369) as an explicit state machine over one wave.
// Returns QMax.size(); *err != 0 when the per-wave stack is too small.
// vertices: the graph's vertex numbers in ascending order (nullptr: 0 .. m - 1). The search only ever compares vertex numbers and
// uses them as row / bit indices, so a graph whose m vertices keep larger, ascending numbers (all below 64 MW) behaves exactly
// like its renumbered copy. L.deg[i] = degree of the i-th vertex on entry.
// kGate: the caller only asks whether the clique FindClique(minimal_size) returns is LARGER than minimal_size
// (sac_model_registration_graph.h:260-262). FindClique stops at the first leaf with |Q| >= minimal_size, and that leaf's size is
// decided long before it is reached: once Q holds minimal_size vertices and their common neighbourhood Rp is not empty, the
// recursion can only go down -- the child's first candidate always passes |Q| + c > |QMax| (|QMax| < minimal_size <= |Q|, or the
// search had returned), so an (minimal_size + 1)-th vertex is pushed, and from there every path ends in a leaf of at least that
// size before anything is popped. (While |QMax| < minimal_size, that is: after the first such leaf the reference unwinds through
// the ancestors' remaining candidates, which can no longer change QMax -- the gate stops there too.) The only other exit is the step cap (:318), at most |Rp| + 1 steps away: if the cap cannot be
// reached within them the answer is known and the rest of the descent (typically 20-45 more levels, each colouring a list of
// several hundred vertices) is not walked; the returned size is then a lower bound, |Q| + 1. Otherwise: the search as it is.
template <bool kWide, bool kGate>
__device__ __forceinline__ uint32_t clique_search(GateLds L, uint32_t m, uint32_t minimal_size, uint16_t* gstack, uint32_t stack_cap,
                                  int* err, uint32_t* steps_out, uint32_t* prof = nullptr, const uint16_t* vertices = nullptr) {
  const uint32_t l = lane_id();
  const LevelStack stack = {L.lstack, L.lstack_cap, gstack};
  stack_cap += L.lstack_cap;
  const uint32_t MW = (m + 63u) / 64u;
  // R = all vertices, DegreeSort(R); L.deg holds the degree of the i-th vertex at index i
  uint32_t dmax = 0;
  for (uint32_t i = l; i < m; i += 64u) { L.cur[i] = vertices ? vertices[i] : (uint16_t)i; dmax = max(dmax, L.deg[i]); }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) dmax = max(dmax, (uint32_t)__shfl_xor((int)dmax, o));
  const uint32_t max_degree = uni(dmax);                 // = the degree of the sorted list's head (:352-355)
  __syncthreads();
  rank_sort_desc<kWide>(L.cur, L.tmp, L.deg, m, L.keys);
  __syncthreads();
  for (uint32_t i = l; i < m; i += 64u) L.C[i] = i < max_degree ? i + 1u : max_degree + 1u;     // :356-361
  for (uint32_t i = l; i < m + 2u; i += 64u) { L.S[i] = 0u; L.SOld[i] = 0u; }
  for (uint32_t i = l; i < m; i += 64u) stk_put(stack, i, L.cur[i]);
  if (l == 0) { L.lbase[1] = 0u; L.lsize[1] = m; L.lcap[1] = m; }
  __syncthreads();

  uint32_t level = 1, qsz = 0, qmax = 0, top = m;
  int all_steps = 1;
  // optional phase profile (diagnostics): cycles in intersection / degree re-sort / colouring, and their counts
  uint32_t pf_isect = 0, pf_sort = 0, pf_col = 0, pf_vfull = 0, pf_big = 0, pf_vbig = 0;
  // A level's list lives where it will be kept: on the LDS part of the level stack when it fits there whole (the usual case:
  // the lists of one root-to-leaf path add up to a few thousand entries) -- the child is built in place right behind its
  // parent's list, nothing is copied down when the search descends and nothing is restored when it returns. A list that does not
  // fit (the stack continues in global memory) is worked on in one of two LDS buffers and copied to / from the stack as before.
  auto in_lds = [&](uint32_t b, uint32_t n) { return b + n <= stack.lds_cap; };
  uint16_t* cur = in_lds(0u, m) ? stack.lds : L.cur;
  // The current level's frame -- list size, S[level], and where its list sits on the stack -- lives in scalar registers;
  // the LDS arrays are only touched when the level changes, and then all of a frame's words come back in ONE LDS round trip
  // (S, SOld, lbase, lsize, lcap are consecutive arrays of `ma` words: lane j reads array j at [level]). A lone wave pays
  // ~130 cycles per dependent LDS read, and the per-word form of this bookkeeping cost a dozen of them per step.
  const uint32_t ma = (m + 7u) & ~3u;
  auto frame_word = [&](uint32_t lvl) -> uint32_t { return l < 5u ? (L.S + (size_t)l * ma)[lvl] : 0u; };
  uint32_t sz = m, S_cur = 0u, base_cur = 0u, cap_cur = m;     // level 1: S[1] = S[1] + S[0] - SOld[1] = 0, SOld[1] = S[0] = 0 (:300-301)
  while (true) {
    bool ret = false;
    if (sz == 0u) {
      ret = true;                                          // while (!R.empty()) falls through, function returns
    } else {
      const uint32_t pv = cur[sz - 1u];
      const uint32_t cv = top > 0u ? L.C[top - 1u] : 0u;   // C.back(), decision D3
      const uint32_t p = uni(pv), c = uni(cv);
      if (qsz + c > qmax) {                                // :307
        ++qsz;                                             // Q.push_back(p)
        // Intersection(p, R, Rp), :209-217 -- order preserving compaction
        const u64* prow = L.adjc + (size_t)p * MW;
        const long long pt0 = prof ? clock64() : 0;
        const uint32_t nb = base_cur + cap_cur;            // where the child's list goes on the stack
        const bool in_place = in_lds(nb, sz);              // rp <= sz
        uint16_t* const nxt = in_place ? stack.lds + nb : (cur == L.cur ? L.nxt : L.cur);
        uint32_t rp = 0;
        for (uint32_t i0 = 0; i0 < sz; i0 += 64u) {
          const uint32_t i = i0 + l;
          uint32_t h = 0;
          bool adj = false;
          if (i < sz) { h = cur[i]; adj = (prow[h >> 6] >> (h & 63u)) & 1ull; }
          const u64 bal = __ballot(adj);
          if (adj) nxt[rp + (uint32_t)__popcll(bal & ((1ull << l) - 1ull))] = (uint16_t)h;
          rp += (uint32_t)__popcll(bal);
        }
        rp = uni(rp);
        __syncthreads();
        const long long pt1 = prof ? clock64() : 0;
        pf_isect += (uint32_t)(pt1 - pt0);
        if constexpr (kGate) {
          if (rp > 0u && qmax < minimal_size && qsz >= minimal_size && (uint32_t)all_steps + rp + 1u <= (uint32_t)kStepCap) { qmax = qsz + 1u; break; }
        }
        if (rp > 0u) {
          // :313 is (double)S[level] / all_steps_ < 0.025. With all_steps <= 100001 a quotient other than 1/40
          // differs from 1/40 by more than 1e-7, and 1/40 itself rounds to the literal: the test is 40 S < all_steps
          if ((uint64_t)S_cur * 40ull < (uint64_t)all_steps) {
            degrees_in_list(L, nxt, rp, MW);
            rank_sort_desc<kWide>(nxt, L.tmp, L.deg, rp, L.keys);
          }
          const long long pt2 = prof ? clock64() : 0;
          pf_sort += (uint32_t)(pt2 - pt1);
          colour_sort<kWide>(L, nxt, rp, MW, qmax, qsz);
          if (prof) {
            const uint32_t dt = (uint32_t)(clock64() - pt2);
            pf_col += dt;
            if ((int)qmax - (int)qsz + 1 < 2) { pf_vfull += rp; if (rp > 64u) { pf_big += dt; pf_vbig += rp; } }
          }
          S_cur += 1u;
          ++all_steps;
          if (all_steps > kStepCap) {
            ret = true;                                    // :318-319: returns without popping Q
          } else {
            if (nb + rp > stack_cap) { *err = 1; break; }
            if (!in_place)
              for (uint32_t i = l; i < rp; i += 64u) stk_put(stack, nb + i, nxt[i]);
            // leave this level: its frame goes to LDS; read the child's S / SOld in the same round trip
            const uint32_t child = frame_word(level + 1u);
            if (l == 0) { L.S[level] = S_cur; L.lsize[level] = sz; L.lbase[level] = base_cur; L.lcap[level] = cap_cur; }
            const uint32_t s_child = rdlane(child, 0u), sold_child = rdlane(child, 1u);
            ++level;
            cur = nxt;
            if (qmax >= minimal_size) {                    // :290-291 at the entry of the child: it returns at once; its S and
              // SOld stay as they were. Its frame must still be readable when the common return path below stores S
              if (l == 0) L.S[level] = s_child;
              S_cur = s_child; sz = rp; base_cur = nb; cap_cur = rp;
              ret = true;
            } else {
              if (l == 0) L.SOld[level] = S_cur;           // :300-301: S[level] += S[level - 1] - SOld[level]; SOld[level] = S[level - 1]
              S_cur = s_child + S_cur - sold_child;
              sz = rp; base_cur = nb; cap_cur = rp;
              __syncthreads();
              continue;
            }
          }
        } else {
          if (qsz > qmax) {                                // :322-326
            qmax = qsz;
            if (qmax >= minimal_size) {
              // (what follows in the reference is the unwinding: every ancestor still expands its remaining candidates, whose
              // children return at once (:290); a leaf there has |Q| < |QMax|, so QMax is final -- the gate needs no more)
              if constexpr (kGate) break;
              ret = true;
            }
          }
          if (!ret) --qsz;                                 // Q.pop_back(), :329
        }
      } else {
        ret = true;                                        // :331-332
      }
      if (!ret) {                                          // R.pop_back(); C.pop_back(), :333-334
        --sz;
        if (top > 0u) --top;
        continue;
      }
    }
    // the current level's function returns; its caller continues after the recursive call (:320)
    if (level == 1u) break;
    if (l == 0) L.S[level] = S_cur;                        // a later sibling re-enters this level and reads it (:300)
    --level;
    --qsz;                                                 // Q.pop_back()
    if (top > 0u) --top;                                   // C.pop_back()
    __syncthreads();
    const uint32_t fw = frame_word(level);                 // S, -, lbase, lsize, lcap of the caller: one round trip
    S_cur = rdlane(fw, 0u); base_cur = rdlane(fw, 2u); sz = rdlane(fw, 3u) - 1u; cap_cur = rdlane(fw, 4u);   // R.pop_back()
    if (in_lds(base_cur, cap_cur)) {
      cur = stack.lds + base_cur;                          // the caller's list is where it was built
    } else {
      cur = L.cur;
      for (uint32_t i = l; i < sz; i += 64u) cur[i] = stk_get(stack, base_cur + i);
    }
    __syncthreads();
  }
  if (steps_out) *steps_out = (uint32_t)all_steps;
  if (prof && l == 0) { prof[0] = pf_isect; prof[1] = pf_sort; prof[2] = pf_col; prof[3] = pf_big; prof[4] = pf_vbig; prof[5] = pf_vfull; }
  return qmax;
}

// stand-alone clique search on an explicit graph (the reference's test/test_maximum_clique.cpp shape):
// adj = m x MW bit matrix in global memory. One block of 64 threads. kWide as eval_kernel's: false is the search of the
// instantiation that evaluates objects of up to 512 matches, and a graph of up to 512 vertices is run through that one.
template <bool kGate, bool kWide = true>
__global__ __launch_bounds__(128) void clique_test_kernel(const u64* adj, uint32_t m, uint32_t minimal_size,
                                                         uint16_t* stack, uint32_t stack_cap, uint32_t lds_bytes,
                                                         uint32_t* out) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  const uint32_t l = lane_id();
  GateLds L = gate_carve<false>(lds_raw, m, lds_bytes);
  const uint32_t MW = (m + 63u) / 64u;
  for (uint32_t i = l; i < m * MW; i += 64u) L.adjc[i] = adj[i];
  __syncthreads();
  for (uint32_t g = l; g < m; g += 64u) {
    uint32_t d = 0;
    for (uint32_t w = 0; w < MW; ++w) d += (uint32_t)__popcll(L.adjc[(size_t)g * MW + w]);
    L.deg[g] = d;
  }
  __syncthreads();
  int err = 0;
  uint32_t steps = 0;
  const uint32_t q = clique_search<kWide, kGate>(L, m, minimal_size, stack, stack_cap, &err, &steps);
  if (l == 0) { out[0] = q; out[1] = (uint32_t)err; out[2] = steps; }
}
