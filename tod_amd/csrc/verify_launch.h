// Launch plumbing of the verifier: the argument-set holders every kernel is launched with (Slots by value in kernarg, SlotsPtr
// staged in device memory), the slot-count constants with their kernarg arithmetic, the word copy / zero-fill kernel that carries
// the mailbox traffic, launch_list, and the TODHIP_DEBUG helpers. No reference lines: this is how the batch engine shares launches.
// Included by verify.hip inside its anonymous namespace, after verify_kernels.h and the standard headers.

// Every kernel takes up to kMaxSlots argument sets and picks its own with the last grid dimension: the frames of a
// batch (each at its own point of its own RANSAC state machine) share launches, so a batch costs the launches and
// host round trips of one frame.
constexpr uint32_t kMaxSlots = 16;                         // 16 x 200 B of EvalArgs stays under the 4 KB kernarg limit
constexpr uint32_t kManySlots = 36;                        // kernels with ~110 B of arguments per slot (4 KB of kernarg in all)
template <class A, uint32_t N = kMaxSlots> struct Slots { A a[N]; };
// the same argument sets in device memory (lists of thousands of objects: launch_many)
template <class A> struct SlotsPtr { const A* a; };

struct CopyArgs { const uint32_t* src; uint32_t* dst; uint32_t n; };   // src == nullptr: zero fill

// words from one address space to another (device <-> device-visible pinned host memory) or zero fill: the
// host's mailbox traffic rides in kernels, so a tick of the batch engine is launches + ONE stream synchronize
constexpr uint32_t kWideSlots = 32;                        // argument sets of <= 124 B: a 32-frame batch's tick in one launch
constexpr uint32_t kCopySlots = 160;                       // 24 B per copy: a tick's copies of 16 frames in one launch
__global__ __launch_bounds__(256) void copy_words_kernel(Slots<CopyArgs, kCopySlots> S) {
  const CopyArgs& a = S.a[blockIdx.y];
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < a.n; i += gridDim.x * 256u) a.dst[i] = a.src ? a.src[i] : 0u;
}

// TODHIP_DEBUG=1: ticks, flights and sprints (a timeline that costs a few lines per tick); 2: also every round, draw window, evaluation
inline int tod_debug_level() { static const int lv = [] { const char* e = getenv("TODHIP_DEBUG"); return e ? std::max(1, atoi(e)) : 0; }(); return lv; }   // read once
inline bool tod_debug() { return tod_debug_level() > 0; }
inline double dbg_us() {
  static const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
}
inline int dbg_thread() { static std::atomic<int> next{0}; thread_local int id = next.fetch_add(1); return id; }   // which host thread (= which context's batch)
#define TOD_DBG2(...) do { if (tod_debug_level() > 1) { fprintf(stderr, "[todhip %.0f] ", dbg_us()); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); fflush(stderr); } } while (0)
#define TOD_DBG(...) do { if (tod_debug()) { char b_[512]; int n_ = snprintf(b_, sizeof(b_), "[todhip %.0f] ", dbg_us()); n_ += snprintf(b_ + n_, sizeof(b_) - n_, __VA_ARGS__); \
    snprintf(b_ + std::min<int>(n_, (int)sizeof(b_) - 16), 16, " {t%d}\n", dbg_thread()); fputs(b_, stderr); } } while (0)   /* one write per line: threads do not interleave */

// launch `kern` over the argument sets of v, kMaxSlots at a time; extent(a) = blocks one set needs in x (and y)
template <uint32_t N = kMaxSlots, class A, class Kern, class Extent>
void launch_list(hipStream_t st, Kern kern, const std::vector<A>& v, uint32_t block, uint32_t lds, int slot_dim, Extent extent) {
  static_assert(sizeof(Slots<A, N>) <= 4096, "kernel arguments are limited to 4 KB");
  for (size_t i0 = 0; i0 < v.size(); i0 += N) {
    const uint32_t n = (uint32_t)std::min<size_t>(N, v.size() - i0);
    Slots<A, N> S;
    std::memset(&S, 0, sizeof(S));
    uint32_t gx = 1, gy = 1;
    for (uint32_t i = 0; i < n; ++i) {
      S.a[i] = v[i0 + i];
      const dim3 e = extent(v[i0 + i]);
      gx = std::max(gx, e.x); gy = std::max(gy, e.y);
    }
    dim3 grid;
    if (slot_dim == 0) grid = dim3(n);
    else if (slot_dim == 1) grid = dim3(gx, n);
    else grid = dim3(gx, gy, n);
    hipLaunchKernelGGL(kern, grid, dim3(block), lds, st, S);
  }
}
