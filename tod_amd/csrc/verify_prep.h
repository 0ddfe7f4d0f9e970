// Preparation kernels of the verifier: FillAdjacency (adjacency_ransac.cpp:127-172) as K6 adjacency / finite / round-prep and their
// one-wave form for small objects, K11 InvalidateQueryIndices / InvalidateIndices (:63-123), and K_c ClusterPerObject (:176-205),
// each with its argument struct.
// Included by verify.hip inside its anonymous namespace, after verify_kernels.h and verify_launch.h.

struct AdjArgs { ObjJob job; float span, err; };
struct JobArgs { ObjJob job; };
// gate (optional): the kernel does nothing unless *gate >= gate_min -- the next round's preparation rides in the tick of the growth
// that decides whether there is a next round (GrowthOut::n_kp_inliers against min_inliers, GuessGenerator.cpp:205-206)
struct PrepArgs { ObjJob job; uint32_t* stats; const uint32_t* gate; uint32_t gate_min; };   // stats[0] = |valid|, [1] = sum of sample degrees inside valid, [2] = triangle found

// ------------------------------------------------------------------------------------------------ K6
// one pair of FillAdjacency (adjacency_ransac.cpp:136-166): q / t = query / training point, k = keypoint pixel of the two matches
__device__ __forceinline__ void pair_test(const float* q1, const float* q2, const float* t1, const float* t2, const float* k1, const float* k2,
                                          float span, float err, bool& phys, bool& samp) {
  phys = false; samp = false;
  float dq = dist_sq3(q1, q2);
  const float lim = (span + 2 * err) * (span + 2 * err);
  if (!(dq > lim)) {                                      // adjacency_ransac.cpp:144
    dq = sqrtf(dq);
    const float dt = (float)norm3d(t1[0] - t2[0], t1[1] - t2[1], t1[2] - t2[2]);
    const float a = fabsf(dt - dq);
    if (!(a > 4 * err)) {                                 // :151
      phys = true;
      const float px = (k1[0] - k2[0]) * (k1[0] - k2[0]) + (k1[1] - k2[1]) * (k1[1] - k2[1]);
      samp = (px > 20 * 20) && (a < 2 * err);             // :158-161
    }
  }
}

template <class H>
__global__ __launch_bounds__(256) void adjacency_kernel(H S) {
  TOD_LATENCY_PRIO();   // latency-bound: win issue arbitration against the VALU-saturating matcher
  const ObjJob& job = S.a[blockIdx.z].job;
  const float span = S.a[blockIdx.z].span, err = S.a[blockIdx.z].err;
  const uint32_t i = blockIdx.x;
  if (i >= job.n) return;
  const uint32_t word = blockIdx.y * 4u + (threadIdx.x >> 6);
  if (word >= job.W) return;
  const uint32_t j = word * 64u + lane_id();
  bool phys = false, samp = false;
  if (j < job.n && j != i) {
    const uint32_t lo = min(i, j), hi = max(i, j);       // the reference visits each pair once with i < j
    pair_test(job.query + 3 * lo, job.query + 3 * hi, job.train + 3 * lo, job.train + 3 * hi, job.kpxy + 2 * lo, job.kpxy + 2 * hi, span, err,
              phys, samp);
  }
  const u64 pb = __ballot(phys), sb = __ballot(samp);
  if (lane_id() == 0) {
    job.phys[(size_t)i * job.W + word] = pb;
    job.samp[(size_t)i * job.W + word] = sb;
  }
}

template <class H>
__global__ __launch_bounds__(256) void finite_kernel(H S) {
  TOD_LATENCY_PRIO();   // latency-bound: win issue arbitration against the VALU-saturating matcher
  const ObjJob& job = S.a[blockIdx.y].job;
  const uint32_t v = blockIdx.x * 256u + threadIdx.x;
  bool f = false;
  if (v < job.n) {
    f = true;
    for (int c = 0; c < 3; ++c) f = f && isfinite(job.train[3 * v + c]) && isfinite(job.query[3 * v + c]);
  }
  const u64 b = __ballot(f);
  const uint32_t word = v >> 6;
  if (lane_id() == 0 && word < job.W) {
    job.finite[word] = b;
    const uint32_t base = word * 64u;
    job.valid[word] = base + 64u <= job.n ? ~0ull : (base < job.n ? ((1ull << (job.n - base)) - 1ull) : 0ull);
  }
}

// per round: sample degree inside the valid set, the ">= 7" filter mask (:211-213), |valid| -- and whether the sample
// graph on the valid matches holds a triangle at all. Without one, no drawIndexSampleHelper attempt can succeed
// (sac_model_registration_graph.h:102-132 needs three mutually sample-adjacent indices), and a failing attempt consumes a
// number of rand() calls that does not depend on the values drawn: the top level draws and erases every valid index once
// (|valid| draws); under pick v the second level draws and erases every not-yet-erased neighbour of v (one draw each --
// its own third level is empty, so it returns before drawing), i.e. every edge is paid for exactly once, at whichever
// endpoint is picked first. A triangle-free object therefore advances the stream by exactly 1000 (|valid| + |E|) draws
// (getSamples' 1000 attempts, :141-168) and yields nothing: the host skips its draw table and chain walk altogether.
template <class H>
__global__ __launch_bounds__(256) void round_prep_kernel(H S) {
  TOD_LATENCY_PRIO();   // latency-bound: win issue arbitration against the VALU-saturating matcher
  const ObjJob& job = S.a[blockIdx.y].job;
  uint32_t* const stats = S.a[blockIdx.y].stats;
  if (S.a[blockIdx.y].gate && *S.a[blockIdx.y].gate < S.a[blockIdx.y].gate_min) return;   // block-uniform
  const uint32_t v = blockIdx.x * 256u + threadIdx.x;
  bool isv = false;
  uint32_t d = 0;
  if (v < job.n) {
    isv = (job.valid[v >> 6] >> (v & 63u)) & 1ull;
    if (isv)
      for (uint32_t w = 0; w < job.W; ++w) d += (uint32_t)__popcll(job.samp[(size_t)v * job.W + w] & job.valid[w]);
    job.sampdeg[v] = d;
  }
  const u64 b7 = __ballot(isv && d >= kGateMinimal), bv = __ballot(isv);
  const uint32_t dsum = wave_sum(d);
  if (lane_id() == 0 && (v >> 6) < job.W) {
    job.deg7[v >> 6] = b7;
    if (bv) atomicAdd(stats, (uint32_t)__popcll(bv));
    if (dsum) atomicAdd(stats + 1, dsum);
  }
  // triangle through v: a neighbour j > v that shares a neighbour with v (all inside valid). One finder is enough.
  if (isv && d >= 2u) {
    const u64* rv = job.samp + (size_t)v * job.W;
    for (uint32_t wj = v >> 6; wj < job.W; ++wj) {
      u64 nb = rv[wj] & job.valid[wj];
      if (wj == (v >> 6)) nb &= (v & 63u) == 63u ? 0ull : ~0ull << ((v & 63u) + 1u);
      while (nb) {
        if (__hip_atomic_load(stats + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) return;
        const uint32_t j = wj * 64u + (uint32_t)__ffsll((long long)nb) - 1u;
        nb &= nb - 1ull;
        const u64* rj = job.samp + (size_t)j * job.W;
        u64 common = 0;
        for (uint32_t w = 0; w < job.W; ++w) common |= rv[w] & rj[w] & job.valid[w];
        if (common) { __hip_atomic_store(stats + 2, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); return; }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ K11
// InvalidateQueryIndices (adjacency_ransac.cpp:93-123): drop every valid match whose keypoint is an inlier
// keypoint, then InvalidateIndices (:63-89): repeatedly drop valid matches whose sample degree is < 3.
struct InvArgs { ObjJob job; const u64* kp_bits; u64* scratch; const uint32_t* gate; uint32_t gate_min; };   // gate: as PrepArgs
// 256 threads (one wave per SIMD): a block this size still finds wave slots on a CU whose other slots are held by the
// matcher's resident grid; a 1024-thread block had to wait for a whole matcher launch to end (1.4 ms on average)
__global__ __launch_bounds__(256) void invalidate_kernel(Slots<InvArgs, kWideSlots> SL) {
  TOD_LATENCY_PRIO();   // latency-bound: win issue arbitration against the VALU-saturating matcher
  const ObjJob& job = SL.a[blockIdx.x].job;
  const u64* const kp_bits = SL.a[blockIdx.x].kp_bits; u64* const scratch = SL.a[blockIdx.x].scratch;
  if (SL.a[blockIdx.x].gate && *SL.a[blockIdx.x].gate < SL.a[blockIdx.x].gate_min) return;   // block-uniform
  __shared__ uint32_t sAny;
  const uint32_t tid = threadIdx.x, W = job.W, n = job.n;
  if (tid == 0) sAny = 0u;
  __syncthreads();
  for (uint32_t w = tid; w < W; w += 256u) {
    u64 gone = 0ull, val = job.valid[w];
    u64 bits = val;
    while (bits) {
      const uint32_t b = (uint32_t)__ffsll((long long)bits) - 1u;
      const uint32_t qi = job.qidx[w * 64u + b];
      if ((kp_bits[qi >> 6] >> (qi & 63u)) & 1ull) gone |= 1ull << b;
      bits &= bits - 1ull;
    }
    if (gone) { job.valid[w] = val & ~gone; atomicOr(&sAny, 1u); }
  }
  __syncthreads();
  if (sAny == 0u) return;                                  // InvalidateIndices(empty) does nothing (:68)
  while (true) {
    __syncthreads();
    if (tid == 0) sAny = 0u;
    __syncthreads();
    for (uint32_t w = tid; w < W; w += 256u) scratch[w] = 0ull;
    __syncthreads();
    for (uint32_t v = tid; v < n; v += 256u) {
      if ((job.valid[v >> 6] >> (v & 63u)) & 1ull) {
        uint32_t d = 0;
        for (uint32_t w = 0; w < W; ++w) d += (uint32_t)__popcll(job.samp[(size_t)v * W + w] & job.valid[w]);
        if (d < 3u) { atomicOr(&scratch[v >> 6], 1ull << (v & 63u)); atomicOr(&sAny, 1u); }   // min_sample_size_
      }
    }
    __syncthreads();
    if (sAny == 0u) break;
    for (uint32_t w = tid; w < W; w += 256u) job.valid[w] &= ~scratch[w];
  }
}

// finite_kernel + adjacency_kernel + round_prep_kernel for an object of at most 64 matches, by ONE wave: lane j = match j, row i of
// both bit matrices is one ballot, and the first round's statistics come from the rows in registers. A frame of self-similar texture
// has ~190 such objects and one big one: three dependent launches of ~2000 mostly empty blocks per frame become one launch of one
// wave per object (inside the pipeline, beside the matcher's resident grid, every dependent launch and every block costs a multiple
// of what it costs alone).
struct PrepSmallArgs { ObjJob job; uint32_t* stats; float span, err; };
template <class H>
__global__ __launch_bounds__(64) void small_prep_kernel(H S) {
  TOD_LATENCY_PRIO();
  const PrepSmallArgs& A = S.a[blockIdx.y];
  const ObjJob& job = A.job;
  const uint32_t n = job.n, l = lane_id();
  const float span = A.span, err = A.err;
  float q[3] = {0.f, 0.f, 0.f}, t[3] = {0.f, 0.f, 0.f}, kp[2] = {0.f, 0.f};
  if (l < n) {
    for (int c = 0; c < 3; ++c) { q[c] = job.query[3 * l + c]; t[c] = job.train[3 * l + c]; }
    kp[0] = job.kpxy[2 * l]; kp[1] = job.kpxy[2 * l + 1];
  }
  bool fin = l < n;
  for (int c = 0; c < 3; ++c) fin = fin && isfinite(t[c]) && isfinite(q[c]);
  const u64 finite = __ballot(fin);
  const u64 valid = n >= 64u ? ~0ull : ((1ull << n) - 1ull);
  u64 my_phys = 0ull, my_samp = 0ull;
  for (uint32_t i = 0; i < n; ++i) {                       // row i: the pair (i, lane)
    float qi[3], ti[3], ki[2];
    for (int c = 0; c < 3; ++c) { qi[c] = __shfl(q[c], (int)i); ti[c] = __shfl(t[c], (int)i); }
    ki[0] = __shfl(kp[0], (int)i); ki[1] = __shfl(kp[1], (int)i);
    bool ph = false, sa = false;
    if (l < n && l != i) {
      if (i < l) pair_test(qi, q, ti, t, ki, kp, span, err, ph, sa);   // the reference visits each pair once with i < j
      else pair_test(q, qi, t, ti, kp, ki, span, err, ph, sa);
    }
    const u64 pb = __ballot(ph), sb = __ballot(sa);
    if (l == i) { my_phys = pb; my_samp = sb; }
  }
  const bool isv = l < n;
  const uint32_t d = isv ? (uint32_t)__popcll(my_samp & valid) : 0u;
  const u64 deg7 = __ballot(isv && d >= kGateMinimal);
  const uint32_t degsum = wave_sum(d);
  bool on_tri = false;                                     // (wave-uniform loop: cross-lane reads need every lane active)
  for (uint32_t o = 0; o < n; ++o) {
    const u64 ro = rdlane64(my_samp, o);
    on_tri = on_tri || (((my_samp >> o) & 1ull) && (my_samp & ro & valid) != 0ull);
  }
  const bool triangle = __ballot(on_tri) != 0ull;
  if (l < n) { job.phys[l] = my_phys; job.samp[l] = my_samp; job.sampdeg[l] = d; }
  if (l == 0u) {
    job.finite[0] = finite; job.valid[0] = valid; job.deg7[0] = deg7;
    A.stats[0] = n; A.stats[1] = degsum; A.stats[2] = triangle ? 1u : 0u;
  }
}

// ------------------------------------------------------------------------------------------------ K_c
// ClusterPerObject (adjacency_ransac.cpp:176-205) of one frame, for device-resident inputs, in ONE launch of one block: lookup ->
// scan -> scatter + histogram -> object offsets -> stable grouping, with the histogram and the frame's totals written straight into
// the slot's mailbox. Matches arrive in the matcher's fixed-stride layout (k slots per query, counts[q] used); the flat order
// (query asc, rank asc) is what the reference's push_back order produces, and grouping by object is stable, so query_indices_
// stays non-decreasing per object (App. A Q4).
// The keypoint's 3D point: with cloud != nullptr it is read from the H x W x 3 cloud (adjacency_ransac.cpp:184-185). Otherwise N3
// (SURVEY 8(f)): the reference back-projects the WHOLE registered depth image to an H x W x 3 cloud (ecto_opencv DepthTo3d,
// python/object_recognition_tod/detector.py:26,62,66-69) and then reads Q points of it. Here the Q points are computed directly:
// same pixel truncation, same pinhole back-projection as cv::depthTo3d (x = (u - cx) z / fx, y = (v - cy) z / fy), uint16 depth
// in millimetres with 0 = no measurement -> NaN as cv::rescaleDepth does (third-party conventions, recalled; parity unpinned).
// Inside the pipeline every dependent launch waits for wave slots beside the matcher's resident grid: five dependent launches and
// a host round trip between the scatter and the grouping were 0.4-0.5 ms per batch there (45 us alone).
struct ClusterArgs {
  const float* kp_xy; const float* cloud; const void* depth; const uint32_t* counts; const todhip_dmatch* matches; const float* mxyz;
  uint32_t nq, k, H, Wimg, n_objs, qidx_add; int depth_is_u16; float fx, fy, cx, cy;   // qidx_add: added to the keypoint index stored per match
  uint32_t *kept, *offs, *obj_of, *src, *hist, *goff, *cnt; float* qpt;          // device scratch
  float *train, *query, *kpxy; uint32_t* qidx;                                    // grouped outputs
  uint32_t* m_hist; ClusterCtl* m_ctl;                                            // mailbox (pinned): histogram; error and n_all
};
// The kernel's body. kRescale: the depth image is geom->dH x geom->dW, not of the image size; the pixel rescale_depth would have
// written at (col, row) is computed from its taps (depth_rescale.h) instead of being read from an H x W intermediate, NaN band
// included. It is a kernel of its own (cluster_frame_rescaled_kernel), so that cluster_frame_kernel stays the code and the arguments
// it was before there was a geometry.
struct ClusterRescaledArgs { ClusterArgs c; RescaleGeom geom; };
template <bool kRescale>
__device__ __forceinline__ void cluster_frame(const ClusterArgs& a, const RescaleGeom* geom) {
  __shared__ uint32_t part[256], s_o[256], s_err, s_total;
  const uint32_t tid = threadIdx.x, nq = a.nq, k = a.k, n_objs = a.n_objs;
  if (tid == 0) s_err = 0u;
  for (uint32_t o = tid; o < n_objs; o += 256u) { a.hist[o] = 0u; a.cnt[o] = 0u; }
  __syncthreads();
  // ---- the keypoint's 3D point (adjacency_ransac.cpp:184-189): cloud lookup, or the depth pixel back-projected (see above)
  for (uint32_t q = tid; q < nq; q += 256u) {
    const int row = (int)a.kp_xy[2 * q + 1], col = (int)a.kp_xy[2 * q];    // float -> int truncation (:185)
    const bool lookup = a.cloud || a.depth;                                // neither: the 2D-only branch (GuessGenerator.cpp:147-152), no 3D point
    if (lookup && (row < 0 || col < 0 || (uint32_t)row >= a.H || (uint32_t)col >= a.Wimg)) { atomicExch(&s_err, 1u); a.kept[q] = 0; continue; }
    float x, y, z;
    if (!lookup) {
      x = y = z = 0.f;
    } else if (a.cloud) {
      const float* p = a.cloud + 3 * ((size_t)row * a.Wimg + col);
      x = p[0]; y = p[1]; z = p[2];
    } else {
      if (kRescale) {                                                      // the pixel of the rescaled image, computed here (depth_rescale.h)
        z = rescaled_depth_at(a.depth, a.depth_is_u16, *geom, (uint32_t)col, (uint32_t)row);
      } else if (a.depth_is_u16) {
        const uint16_t d = reinterpret_cast<const uint16_t*>(a.depth)[(size_t)row * a.Wimg + col];
        z = d == 0 ? __builtin_nanf("") : (float)d * 0.001f;
      } else {
        z = reinterpret_cast<const float*>(a.depth)[(size_t)row * a.Wimg + col];
      }
      x = ((float)col - a.cx) * z / a.fx; y = ((float)row - a.cy) * z / a.fy;
    }
    a.qpt[3 * q] = x; a.qpt[3 * q + 1] = y; a.qpt[3 * q + 2] = z;
    uint32_t c_q = a.counts[q];
    if (c_q > k) { atomicExch(&s_err, 3u); c_q = k; }                      // (a count beyond the fixed stride: refused)
    a.kept[q] = isnan(x) ? 0u : c_q;                                       // only .x is tested (:189)
  }
  __syncthreads();
  // ---- exclusive scan of kept -> offs: the flat order (query asc, rank asc) of the reference's push_back
  {
    const uint32_t chunk = (nq + 255u) / 256u;
    const uint32_t lo = min(nq, tid * chunk), hi = min(nq, lo + chunk);
    uint32_t sum = 0;
    for (uint32_t i = lo; i < hi; ++i) sum += a.kept[i];
    part[tid] = sum;
    __syncthreads();
    if (tid == 0) {
      uint32_t acc = 0;
      for (uint32_t i = 0; i < 256u; ++i) { const uint32_t c = part[i]; part[i] = acc; acc += c; }
      s_total = acc;
    }
    __syncthreads();
    uint32_t acc = part[tid];
    for (uint32_t i = lo; i < hi; ++i) { a.offs[i] = acc; acc += a.kept[i]; }
  }
  const uint32_t n_all = s_total;
  __syncthreads();
  // ---- every match's flat slot, object and source; histogram per object
  for (uint32_t t = tid; t < nq * k; t += 256u) {
    const uint32_t q = t / k, j = t % k;
    if (j >= a.kept[q]) continue;
    const uint32_t f = a.offs[q] + j;
    const todhip_dmatch m = a.matches[t];
    uint32_t o = (uint32_t)m.imgIdx;
    if (m.imgIdx < 0 || o >= n_objs) { atomicExch(&s_err, 2u); o = 0; }
    a.obj_of[f] = o; a.src[f] = t;
    atomicAdd(&a.hist[o], 1u);
  }
  __threadfence();
  __syncthreads();
  // ---- object offsets = exclusive scan of the histogram; the histogram goes to the host
  {
    const uint32_t chunk = (n_objs + 255u) / 256u;
    const uint32_t lo = min(n_objs, tid * chunk), hi = min(n_objs, lo + chunk);
    uint32_t sum = 0;
    for (uint32_t i = lo; i < hi; ++i) sum += __hip_atomic_load(a.hist + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    part[tid] = sum;
    __syncthreads();
    if (tid == 0) {
      uint32_t acc = 0;
      for (uint32_t i = 0; i < 256u; ++i) { const uint32_t c = part[i]; part[i] = acc; acc += c; }
    }
    __syncthreads();
    uint32_t acc = part[tid];
    for (uint32_t i = lo; i < hi; ++i) {
      const uint32_t h = __hip_atomic_load(a.hist + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      a.goff[i] = acc; a.m_hist[i] = h;
      acc += h;
    }
  }
  __syncthreads();
  // ---- stable grouping by object, 256 flat slots at a time: destination = object offset + matches of the object in earlier
  // chunks (cnt) + earlier matches of the object in this chunk
  for (uint32_t base = 0; base < n_all; base += 256u) {
    const uint32_t f = base + tid;
    const bool have = f < n_all;
    const uint32_t o = have ? a.obj_of[f] : 0xFFFFFFFFu;
    s_o[tid] = o;
    // the object's matches in earlier chunks: read by EVERY thread before any thread of this chunk updates it (the barrier below) --
    // the last match of an object in the chunk may sit in a wave that runs ahead of the waves holding its earlier ones, and a count
    // read after that update sends the earlier matches to the wrong places (found as one batch result in five differing from the
    // frame-by-frame call: tools/verify_repeat_frame.py)
    const uint32_t seen = have ? a.cnt[o] : 0u;
    __syncthreads();
    if (have) {
      uint32_t before = 0, after = 0;
      for (uint32_t u = 0; u < tid; ++u) before += s_o[u] == o;
      for (uint32_t u = tid + 1u; u < 256u; ++u) after += s_o[u] == o;
      const uint32_t d = a.goff[o] + seen + before;
      const uint32_t t = a.src[f], q = t / k;
      for (int c = 0; c < 3; ++c) { a.train[3 * d + c] = a.mxyz[(size_t)t * 3 + c]; a.query[3 * d + c] = a.qpt[3 * q + c]; }
      a.qidx[d] = q + a.qidx_add;
      a.kpxy[2 * d] = a.kp_xy[2 * q]; a.kpxy[2 * d + 1] = a.kp_xy[2 * q + 1];
      if (after == 0u) a.cnt[o] = seen + before + 1u;       // the object's last match of the chunk
    }
    __syncthreads();
  }
  if (tid == 0) { a.m_ctl->error = s_err; a.m_ctl->n_kept = n_all; }
}
__global__ __launch_bounds__(256) void cluster_frame_kernel(Slots<ClusterArgs> SL) {
  TOD_LATENCY_PRIO();
  cluster_frame<false>(SL.a[blockIdx.x], nullptr);
}
__global__ __launch_bounds__(256) void cluster_frame_rescaled_kernel(Slots<ClusterRescaledArgs> SL) {
  TOD_LATENCY_PRIO();
  cluster_frame<true>(SL.a[blockIdx.x].c, &SL.a[blockIdx.x].geom);
}
