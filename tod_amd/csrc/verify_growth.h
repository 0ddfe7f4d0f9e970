// The refinement of a winning hypothesis (K9, adjacency_ransac.cpp:255-308): 3x3 SVD, Kabsch (sac_model_registration_graph.h:304-347),
// the admission test, pose inversion and growth_kernel. The result struct GrowthOut is part of the control block (verify_kernels.h).
// Included by verify.hip inside its anonymous namespace, after verify_kernels.h and verify_launch.h.

// ------------------------------------------------------------------------------------------------ K9
// 3x3 one-sided Jacobi SVD in float, A = U diag(w) Vt, w descending. cv::SVD on a CV_32F 3x3
// (sac_model_registration_graph.h:333) is third-party arithmetic that the reference tree does not contain.
__device__ void svd3(const float Ain[3][3], float U[3][3], float w[3], float Vt[3][3]) {
  float A[3][3], V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) A[i][j] = Ain[i][j];
  // Far from 1 the squares below leave the float range (entries beyond 1.8e19) or go denormal (the rounding residue of a rank-deficient
  // A, about 1e-7 of its largest entry, below 1e-12): such an A is first brought to a largest entry in [0.5, 1) by a power of two, in
  // two exact steps that stay inside the range. U and Vt do not depend on the scale; w is then the scaled matrix's (kabsch_solve uses
  // no w). Between 2^-32 and 2^40, where all data in metres lies, nothing is scaled and no bit moves.
  float amax = 0.f;
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) amax = fabsf(A[i][j]) > amax ? fabsf(A[i][j]) : amax;
  if (amax > 0.f && amax <= 3.4028235e+38f && (amax < 2.3283064e-10f || amax > 1.0995116e12f)) {
    int e;
    frexpf(amax, &e);
    const float s1 = ldexpf(1.f, -(e / 2)), s2 = ldexpf(1.f, -(e - e / 2));
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) A[i][j] = A[i][j] * s1 * s2;
  }
  for (int sweep = 0; sweep < 30; ++sweep) {
    bool rotated = false;
    for (int p = 0; p < 2; ++p)
      for (int q = p + 1; q < 3; ++q) {
        float alpha = 0, beta = 0, gamma = 0;
        for (int i = 0; i < 3; ++i) { alpha += A[i][p] * A[i][p]; beta += A[i][q] * A[i][q]; gamma += A[i][p] * A[i][q]; }
        // alpha * beta leaves the float range long before alpha and beta do (sigma1 * sigma2 beyond 1.8e19, or below 1e-19): there the
        // product's root is taken factor by factor; a finite non-zero product keeps the one root it always had, bit for bit
        const float ab = alpha * beta;
        const float lim = (ab != 0.f && ab <= 3.4028235e+38f) ? 1.1920929e-07f * sqrtf(ab) : 1.1920929e-07f * sqrtf(alpha) * sqrtf(beta);
        if (fabsf(gamma) <= lim || gamma == 0.f) continue;
        rotated = true;
        const float zeta = (beta - alpha) / (2.f * gamma);
        const float t = (zeta >= 0.f ? 1.f : -1.f) / (fabsf(zeta) + sqrtf(1.f + zeta * zeta));
        const float c = 1.f / sqrtf(1.f + t * t), s = c * t;
        for (int i = 0; i < 3; ++i) {
          const float ap = A[i][p], aq = A[i][q];
          A[i][p] = c * ap - s * aq; A[i][q] = s * ap + c * aq;
          const float vp = V[i][p], vq = V[i][q];
          V[i][p] = c * vp - s * vq; V[i][q] = s * vp + c * vq;
        }
      }
    if (!rotated) break;
  }
  float nrm[3];
  int order[3] = {0, 1, 2};
  for (int j = 0; j < 3; ++j) nrm[j] = sqrtf(A[0][j] * A[0][j] + A[1][j] * A[1][j] + A[2][j] * A[2][j]);
  for (int a = 0; a < 2; ++a)
    for (int b = 0; b < 2 - a; ++b)
      if (nrm[order[b]] < nrm[order[b + 1]]) { int t = order[b]; order[b] = order[b + 1]; order[b + 1] = t; }
  for (int jj = 0; jj < 3; ++jj) {
    const int j = order[jj];
    w[jj] = nrm[j];
    for (int i = 0; i < 3; ++i) { Vt[jj][i] = V[i][j]; U[i][jj] = nrm[j] > 0.f ? A[i][j] / nrm[j] : 0.f; }
  }
  const float tiny = 1.1920929e-07f * (w[0] > 0.f ? w[0] : 1.f);
  if (w[0] <= 0.f) { for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) U[i][j] = (i == j) ? 1.f : 0.f; return; }
  if (w[1] <= tiny) {
    int ax = 0;
    for (int i = 1; i < 3; ++i) if (fabsf(U[i][0]) < fabsf(U[ax][0])) ax = i;
    float e[3] = {0, 0, 0};
    e[ax] = 1.f;
    float c1[3] = {U[1][0] * e[2] - U[2][0] * e[1], U[2][0] * e[0] - U[0][0] * e[2], U[0][0] * e[1] - U[1][0] * e[0]};
    const float n1 = sqrtf(c1[0] * c1[0] + c1[1] * c1[1] + c1[2] * c1[2]);
    for (int i = 0; i < 3; ++i) U[i][1] = c1[i] / n1;
  }
  if (w[2] <= tiny) {
    U[0][2] = U[1][0] * U[2][1] - U[2][0] * U[1][1];
    U[1][2] = U[2][0] * U[0][1] - U[0][0] * U[2][1];
    U[2][2] = U[0][0] * U[1][1] - U[1][0] * U[0][1];
  }
}
__device__ inline float det3f(const float m[3][3]) {
  return m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0]) +
         m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]);
}

// The serial tail of estimateRigidTransformationSVD (sac_model_registration_graph.h:330-346): H (double sums, rounded to float), SVD,
// reflection fix, R = U Vt (double accumulation), T = c_train - R c_query. C = {c_train, c_query}. One lane's work; shared by the
// block form (growth_kernel) and the single-wave form (sprint_kernel) so that both execute the same arithmetic.
__device__ inline void kabsch_solve(const double Hd[9], const float C[6], float R[9], float T[3]) {
  float H[3][3], U[3][3], wv[3], Vt[3][3], Rm[3][3];
  for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) H[r][c] = (float)Hd[3 * r + c];
  svd3(H, U, wv, Vt);
  if (det3f(U) * det3f(Vt) < 0)
    for (int x = 0; x < 3; ++x) Vt[2][x] *= -1;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      double s = 0;
      for (int k = 0; k < 3; ++k) s += (double)U[r][k] * (double)Vt[k][c];
      Rm[r][c] = (float)s;
    }
  for (int r = 0; r < 3; ++r) {
    float s = 0;
    for (int k = 0; k < 3; ++k) s += Rm[r][k] * C[3 + k];
    T[r] = C[r] - s;
    for (int c = 0; c < 3; ++c) R[3 * r + c] = Rm[r][c];
  }
}
// adjacency_ransac.cpp:275-283: norm(R q + T - t)^2 < thresh, the norm in double
__device__ __forceinline__ bool growth_admits(const float R[9], const float T[3], const float* q, const float* t, double thresh) {
  float p[3];
  for (int r = 0; r < 3; ++r) {
    float s = 0;
    for (int k = 0; k < 3; ++k) s += R[3 * r + k] * q[k];
    p[r] = s + T[r];
  }
  const double nn = norm3d(p[0] - t[0], p[1] - t[1], p[2] - t[2]);
  return nn * nn < thresh;
}
// adjacency_ransac.cpp:304-305: R = R^T, T = -R T
__device__ inline void pose_invert(const float R[9], const float T[3], float Rout[9], float Tout[3]) {
  float Rt[3][3];
  for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) Rt[r][c] = R[3 * c + r];
  for (int r = 0; r < 3; ++r) {
    float s = 0;
    for (int k = 0; k < 3; ++k) s += (-Rt[r][k]) * T[k];
    Tout[r] = s;
    for (int c = 0; c < 3; ++c) Rout[3 * r + c] = Rt[r][c];
  }
}

constexpr uint32_t kGrowthLdsPoints = 2048;   // inlier points staged in LDS per Kabsch pass (48 KB)

// One block. inl/rest/extra are W-word bitsets in global scratch. Sums that the reference accumulates
// sequentially (centroids in float, the correlation matrix in double) are accumulated sequentially here too,
// each by one lane, so that the admitted sets are reproducible bit for bit against a sequential CPU evaluation.
struct GrowthArgs {
  ObjJob job; const uint32_t* triple; float err;          // triple: the winning iteration's samples (device)
  u64 *inl, *rest, *extra; uint32_t* kp_list; u64* kp_bits; uint32_t kp_words; GrowthOut* out;
};
__global__ __launch_bounds__(256) void growth_kernel(Slots<GrowthArgs> SL) {
  TOD_LATENCY_PRIO();   // latency-bound: win issue arbitration against the VALU-saturating matcher
  const GrowthArgs& ga = SL.a[blockIdx.x];
  const ObjJob& job = ga.job;
  const uint32_t s0 = ga.triple[0], s1 = ga.triple[1], s2 = ga.triple[2];
  const float err = ga.err;
  u64* const inl = ga.inl; u64* const rest = ga.rest; u64* const extra = ga.extra;
  uint32_t* const kp_list = ga.kp_list; u64* const kp_bits = ga.kp_bits; const uint32_t kp_words = ga.kp_words;
  GrowthOut* const out = ga.out;
  __shared__ float sR[9], sT[3];
  __shared__ double sAcc[16];
  __shared__ float sC[6];
  __shared__ uint32_t sFlag, sCount;
  __shared__ uint32_t sPre[kMaxWords];
  __shared__ float sPts[kGrowthLdsPoints * 6];
  const uint32_t tid = threadIdx.x, W = job.W, n = job.n;
  // consensus set of the winning iteration: common physical neighbours + the samples
  for (uint32_t w = tid; w < W; w += 256u) {
    u64 v = job.phys[(size_t)s0 * W + w] & job.phys[(size_t)s1 * W + w] & job.phys[(size_t)s2 * W + w] &
            job.valid[w] & job.finite[w];
    if ((s0 >> 6) == w) v |= 1ull << (s0 & 63u);
    if ((s1 >> 6) == w) v |= 1ull << (s1 & 63u);
    if ((s2 >> 6) == w) v |= 1ull << (s2 & 63u);
    inl[w] = v;
    rest[w] = job.valid[w] & ~v;                           // :260-264
  }
  for (uint32_t w = tid; w < kp_words; w += 256u) kp_bits[w] = 0ull;
  __syncthreads();
  if (tid == 0) {
    uint32_t c = 0;
    for (uint32_t w = 0; w < W; ++w) c += (uint32_t)__popcll(inl[w]);
    out->n_model_inliers = c;
  }
  bool do_final = false;
  double thresh = (double)(err * err);                     // float product widened, :267
  uint32_t passes = 0;
  while (true) {
    // ---- estimateRigidTransformationSVD (sac_model_registration_graph.h:304-347) on the current inliers
    // ordered compaction of the inlier points into LDS (ascending match index = the reference's list order)
    for (uint32_t w = tid; w < W; w += 256u) sPre[w] = (uint32_t)__popcll(inl[w]);
    __syncthreads();
    if (tid == 0) {
      uint32_t acc = 0;
      for (uint32_t w = 0; w < W; ++w) { const uint32_t c = sPre[w]; sPre[w] = acc; acc += c; }
      sCount = acc;
    }
    __syncthreads();
    const uint32_t cnt = sCount;
    const bool staged = cnt <= kGrowthLdsPoints;
    if (staged) {                                          // one thread per match: its slot = inliers below it
      for (uint32_t v = tid; v < W * 64u; v += 256u) {
        const u64 bits = inl[v >> 6];
        if ((bits >> (v & 63u)) & 1ull) {
          const uint32_t o = sPre[v >> 6] + (uint32_t)__popcll(bits & ((1ull << (v & 63u)) - 1ull));
          for (int c = 0; c < 3; ++c) { sPts[o * 6u + c] = job.train[3 * v + c]; sPts[o * 6u + 3 + c] = job.query[3 * v + c]; }
        }
      }
    }
    __syncthreads();
    if (tid < 6) {                                         // 6 sequential float sums: centroids
      float s = 0.f;
      if (staged) {
        // 8 LDS reads in flight at once; the additions stay in list order
        uint32_t i = 0;
        for (; i + 8u <= cnt; i += 8u) {
          float v[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) v[j] = sPts[(i + j) * 6u + tid];
#pragma unroll
          for (int j = 0; j < 8; ++j) s += v[j];
        }
        for (; i < cnt; ++i) s += sPts[i * 6u + tid];
      } else {
        const float* src = tid < 3 ? job.train : job.query;
        const uint32_t c = tid % 3u;
        for (uint32_t w = 0; w < W; ++w) {
          u64 bits = inl[w];
          while (bits) {
            const uint32_t v = w * 64u + (uint32_t)__ffsll((long long)bits) - 1u;
            s += src[3 * v + c];
            bits &= bits - 1ull;
          }
        }
      }
      const double inv = 1. / (float)cnt;                  // Vec /= float: times the double reciprocal
      sC[tid] = (float)(s * inv);
    }
    __syncthreads();
    if (tid < 9) {                                         // H = sub_training^T * sub_query, double accumulation
      const uint32_t r = tid / 3u, c = tid % 3u;
      const float ct = sC[r], cq = sC[3 + c];
      double h = 0.0;
      if (staged) {
        uint32_t i = 0;
        for (; i + 8u <= cnt; i += 8u) {
          float va[8], vb[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) { va[j] = sPts[(i + j) * 6u + r]; vb[j] = sPts[(i + j) * 6u + 3 + c]; }
#pragma unroll
          for (int j = 0; j < 8; ++j) h += (double)(va[j] - ct) * (double)(vb[j] - cq);
        }
        for (; i < cnt; ++i) {
          const float a = sPts[i * 6u + r] - ct, b = sPts[i * 6u + 3 + c] - cq;
          h += (double)a * (double)b;
        }
      } else {
        for (uint32_t w = 0; w < W; ++w) {
          u64 bits = inl[w];
          while (bits) {
            const uint32_t v = w * 64u + (uint32_t)__ffsll((long long)bits) - 1u;
            const float a = job.train[3 * v + r] - ct, b = job.query[3 * v + c] - cq;
            h += (double)a * (double)b;
            bits &= bits - 1ull;
          }
        }
      }
      sAcc[tid] = h;
    }
    __syncthreads();
    if (tid == 0) {
      kabsch_solve(sAcc, sC, sR, sT);
      sFlag = 0u;
    }
    __syncthreads();
    ++passes;
    // ---- admit every valid non-inlier within thresh (adjacency_ransac.cpp:275-283)
    for (uint32_t w0 = 0; w0 < W; w0 += 4u) {
      const uint32_t w = w0 + (tid >> 6);
      bool pass = false;
      if (w < W) {
        const uint32_t v = w * 64u + (tid & 63u);
        if (v < n && ((rest[w] >> (v & 63u)) & 1ull)) {
          pass = growth_admits(sR, sT, job.query + 3 * v, job.train + 3 * v, thresh);
        }
      }
      const u64 bal = __ballot(pass);
      if ((tid & 63u) == 0 && w < W) {
        extra[w] = bal;
        if (bal) atomicOr(&sFlag, 1u);
      }
    }
    __syncthreads();
    for (uint32_t w = tid; w < W; w += 256u) { inl[w] |= extra[w]; rest[w] &= ~extra[w]; }
    const bool any_extra = sFlag != 0u;
    __syncthreads();
    if (do_final) break;
    if (!any_extra) { do_final = true; thresh *= 4; }      // :295-301
  }
  // ---- pose inversion (:304-305) and unique keypoint indices (:306-308)
  if (tid == 0) pose_invert(sR, sT, out->R, out->T);
  // unique keypoint indices in ascending match order (:306-308). qidx is non-decreasing in the match index (App. A Q4),
  // so an inlier starts a new keypoint iff the inlier before it has another qidx: one wave per 64-match word, the word
  // boundaries are stitched by one lane.
  uint32_t* const sFirstQ = sPre;                          // sPre is free after the last pass
  __shared__ uint32_t sLastQ[kMaxWords], sNewIn[kMaxWords], sOff[kMaxWords];
  const uint32_t lane = tid & 63u;
  for (uint32_t w = tid >> 6; w < W; w += 4u) {
    const u64 bits = inl[w];
    const bool in = (bits >> lane) & 1ull;
    const uint32_t q = in ? job.qidx[w * 64u + lane] : 0u;
    const u64 lower = bits & ((1ull << lane) - 1ull);
    const uint32_t pq = __shfl(q, lower ? 63u - (uint32_t)__clzll((long long)lower) : 0u);
    const u64 fresh = __ballot(in && lower != 0ull && q != pq);      // new keypoint, previous inlier in the same word
    if (lane == 0) sNewIn[w] = (uint32_t)__popcll(fresh);
    if (bits) {
      const uint32_t lo = (uint32_t)__ffsll((long long)bits) - 1u, hi = 63u - (uint32_t)__clzll((long long)bits);
      if (lane == lo) sFirstQ[w] = q;
      if (lane == hi) sLastQ[w] = q;
    }
  }
  __syncthreads();
  if (tid == 0) {
    uint32_t nm = 0, nk = 0, last = 0xFFFFFFFFu;
    for (uint32_t w = 0; w < W; ++w) {
      const u64 bits = inl[w];
      uint32_t first_new = 0;
      if (bits) { first_new = sFirstQ[w] != last ? 1u : 0u; last = sLastQ[w]; }
      sOff[w] = nk | (first_new << 31);
      nk += first_new + sNewIn[w];
      nm += (uint32_t)__popcll(bits);
    }
    out->n_match_inliers = nm;
    out->n_kp_inliers = nk;
    out->passes = passes;
  }
  __syncthreads();
  for (uint32_t w = tid >> 6; w < W; w += 4u) {
    const u64 bits = inl[w];
    if (!bits) continue;                                   // wave-uniform
    const bool in = (bits >> lane) & 1ull;
    const uint32_t q = in ? job.qidx[w * 64u + lane] : 0u;
    const u64 lower = bits & ((1ull << lane) - 1ull);
    const uint32_t pq = __shfl(q, lower ? 63u - (uint32_t)__clzll((long long)lower) : 0u);
    const bool first_new = (sOff[w] >> 31) != 0u;
    const bool is_new = in && (lower != 0ull ? q != pq : first_new);
    const u64 bal = __ballot(is_new);
    if (is_new) {
      kp_list[(sOff[w] & 0x7FFFFFFFu) + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull))] = q;
      atomicOr(&kp_bits[q >> 6], 1ull << (q & 63u));
    }
  }
}
