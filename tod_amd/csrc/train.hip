// the per-observation arithmetic of the reference's training cell on the GPU
// (src/training/Trainer.cpp:121-187, src/training/training.cpp:57-195): ORB on the masked view, depth rescale
// (equal-size case), validateKeyPoints, depthTo3dSparse, cameraToWorld, mergePoints. A model is accumulated in HBM
// observation by observation and read back once; its rows (32-byte descriptors + object-frame points) are exactly
// what todhip_db_load ingests, so DBs built here match this repo's ORB.
#include <algorithm>
#include <cfloat>
#include <cstring>
#include <new>

#include "depth_rescale.h"
#include "model.h"
#include "orb_plan.h"
#include "train_validate.h"

namespace {

// erosion by the 3x3 element, 4 iterations == minimum over the 9x9 window restricted to the image
// (cv::erode's border value is +inf), done separably: rows, then columns (training.cpp:69-71)
__global__ __launch_bounds__(256) void erode_rows_kernel(const uint8_t* __restrict__ src, uint32_t H, uint32_t W, uint8_t* dst) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= H * W) return;
  const int x = (int)(i % W), y = (int)(i / W);
  int all = 1;
  for (int dx = -4; dx <= 4; ++dx) { const int xx = x + dx; if (xx >= 0 && xx < (int)W && !src[(size_t)y * W + xx]) all = 0; }
  dst[i] = all ? 255 : 0;
}
__global__ __launch_bounds__(256) void erode_cols_kernel(const uint8_t* __restrict__ src, uint32_t H, uint32_t W, uint8_t* dst) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= H * W) return;
  const int x = (int)(i % W), y = (int)(i / W);
  int all = 1;
  for (int dy = -4; dy <= 4; ++dy) { const int yy = y + dy; if (yy >= 0 && yy < (int)H && !src[(size_t)yy * W + x]) all = 0; }
  dst[i] = all ? 255 : 0;
}

using Cam = tod::TrainCam;

// rescale_depth (Trainer.cpp:62-81): the arithmetic is depth_rescale.h's, here once per pixel of the H x W result
__global__ __launch_bounds__(256) void rescale_depth_kernel(const void* __restrict__ src, int is_u16, tod::RescaleGeom geom,
                                                            float* __restrict__ dst, uint32_t H, uint32_t W) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= H * W) return;
  dst[i] = tod::rescaled_depth_at(src, is_u16, geom, i % W, i / W);
}

// validateKeyPoints (training.cpp:57-145) + depthTo3dSparse + cameraToWorld (:175-195) for one keypoint per thread: the arithmetic
// is train_validate.h's, the eroded pixels come from the image the two erosion kernels wrote.
__global__ __launch_bounds__(256) void validate_kernel(const float* __restrict__ kp_xy, const uint32_t* __restrict__ n_ptr,
                                                       const uint8_t* __restrict__ er, const void* __restrict__ depth,
                                                       int depth_is_u16, uint32_t H, uint32_t W, Cam cam, uint32_t* flags,
                                                       float* pts_tmp) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= *n_ptr) return;
  const float px = kp_xy[2 * i], py = kp_xy[2 * i + 1];
  int x, y;
  tod::rounded_pixel(px, py, (int)H, (int)W, &x, &y);
  bool good = er[(size_t)y * W + x] != 0;
  if (!good) good = tod::rescue_pixel([&](int ii, int jj) { return er[(size_t)jj * W + ii] != 0; }, px, py, (int)H, (int)W, &x, &y);
  float z = 0.f;
  if (good) {
    z = tod::depth_metres(depth, depth_is_u16, (size_t)y * W + x);   // cv::rescaleDepth: millimetres -> metres, 0 -> NaN
    if (!tod::valid_depth(z)) good = false;
  }
  flags[i] = good ? 1u : 0u;
  if (good) tod::back_project(cam, x, y, z, pts_tmp + 3 * (size_t)i);
}

// stable compaction of the accepted keypoints behind the rows the model already has (mergePoints, :147-173)
__global__ __launch_bounds__(1024) void append_kernel(const uint32_t* __restrict__ flags, const uint32_t* __restrict__ n_ptr,
                                                      const uint8_t* __restrict__ kp_desc, const float* __restrict__ pts_tmp,
                                                      uint32_t* counters /* [0] model rows, [1] added by this call */,
                                                      uint32_t cap, uint8_t* desc, float* pts) {
  __shared__ uint32_t part[1024];
  const uint32_t n = *n_ptr, tid = threadIdx.x;
  const uint32_t chunk = (n + 1023u) / 1024u;
  const uint32_t lo = min(n, tid * chunk), hi = min(n, lo + chunk);
  uint32_t s = 0;
  for (uint32_t i = lo; i < hi; ++i) s += flags[i];
  part[tid] = s;
  __syncthreads();
  __shared__ uint32_t base, total;
  if (tid == 0) {
    uint32_t acc = 0;
    for (uint32_t i = 0; i < 1024u; ++i) { const uint32_t c = part[i]; part[i] = acc; acc += c; }
    base = counters[0];
    total = acc;
  }
  __syncthreads();
  uint32_t o = base + part[tid];
  for (uint32_t i = lo; i < hi; ++i) {
    if (!flags[i]) continue;
    if (o < cap) {
      for (int b = 0; b < 8; ++b) reinterpret_cast<uint32_t*>(desc)[(size_t)o * 8 + b] = reinterpret_cast<const uint32_t*>(kp_desc)[(size_t)i * 8 + b];
      pts[3 * (size_t)o] = pts_tmp[3 * i]; pts[3 * (size_t)o + 1] = pts_tmp[3 * i + 1]; pts[3 * (size_t)o + 2] = pts_tmp[3 * i + 2];
    }
    ++o;
  }
  __syncthreads();
  if (tid == 0) { counters[1] = min(total, cap > base ? cap - base : 0u); counters[0] = min(base + total, cap); }
}

// ---- a batch of device-resident views (todhip_model_add_observations_device): no eroded image, no rescaled depth image ----------
// View v's keypoints, flags and points are rows v * n_features .. of their arrays. The keypoints per view are on the host once the
// ORB call has returned, so they travel as a kernel argument; what the kernels hand to each other is a BatchWords.
struct BatchCounts { uint32_t n[kTrainBatchMaxViews]; };
struct BatchWords { uint32_t total[kTrainBatchMaxViews], base[kTrainBatchMaxViews], added[kTrainBatchMaxViews]; };

// validate_kernel over (view, keypoint), a keypoint per thread. The eroded pixels a keypoint asks about come from the 13 x 13
// neighbourhood of the view's mask (169 byte loads; 13 rows of 13 bytes, so at most 26 lines), the depth at the chosen pixel from
// the sensor-sized image through the rescale's own arithmetic. A thread per keypoint, not a wave per keypoint with a cooperative
// read: the loads of one keypoint do not depend on each other or on the other lanes', and nothing has to be reduced across lanes
// at the end (48 us for 32 views x 1300 keypoints; the cooperative form was not built).
__global__ __launch_bounds__(256) void validate_batch_kernel(const float* __restrict__ kp_xy, BatchCounts cnt, uint32_t n_features,
                                                             const uint8_t* __restrict__ mask, const uint8_t* __restrict__ depth,
                                                             int depth_is_u16, tod::RescaleGeom geom, uint32_t H, uint32_t W,
                                                             const Cam* __restrict__ cams, uint32_t* flags, float* pts_tmp) {
  const uint32_t v = blockIdx.y, i = blockIdx.x * 256u + threadIdx.x;
  if (i >= cnt.n[v]) return;
  const size_t row = (size_t)v * n_features + i;
  const uint8_t* view_mask = mask + (size_t)v * H * W;
  const void* view_depth = depth + (size_t)v * geom.dH * geom.dW * (depth_is_u16 ? 2u : 4u);
  const float px = kp_xy[2 * row], py = kp_xy[2 * row + 1];
  int x, y;
  tod::rounded_pixel(px, py, (int)H, (int)W, &x, &y);
  const int x0 = x, y0 = y;
  const uint32_t win = tod::eroded_window(view_mask, (int)H, (int)W, x0, y0);
  bool good = tod::eroded_window_at(win, x0, y0, x0, y0);
  if (!good) good = tod::rescue_pixel([&](int ii, int jj) { return tod::eroded_window_at(win, x0, y0, ii, jj); }, px, py, (int)H, (int)W, &x, &y);
  float z = 0.f;
  if (good) {
    z = tod::train_depth_at(view_depth, depth_is_u16, geom, x, y);
    if (!tod::valid_depth(z)) good = false;
  }
  flags[row] = good ? 1u : 0u;
  if (good) tod::back_project(cams[v], x, y, z, pts_tmp + 3 * row);
}

// mergePoints (training.cpp:147-173) across the views, a stable compaction in (view, keypoint) order in three ordinary launches:
// a block per view counts its accepted keypoints, one wave scans the view totals behind the model's rows and applies the capacity
// cut, a block per view writes its rows.
__global__ __launch_bounds__(256) void count_batch_kernel(const uint32_t* __restrict__ flags, BatchCounts cnt, uint32_t n_features,
                                                          BatchWords* bw) {
  __shared__ uint32_t part[4];
  const uint32_t v = blockIdx.x, n = cnt.n[v], tid = threadIdx.x;
  uint32_t s = 0;
  for (uint32_t i0 = 0; i0 < n; i0 += 256u) {               // (n is the block's: every lane is there for every ballot)
    const uint32_t i = i0 + tid;
    s += (uint32_t)__popcll(__ballot(i < n && flags[(size_t)v * n_features + i] != 0u));
  }
  if ((tid & 63u) == 0u) part[tid >> 6] = s;
  __syncthreads();
  if (tid == 0u) bw->total[v] = part[0] + part[1] + part[2] + part[3];
}

// one wave, lane v = view v: the rows the model holds before view v exactly as the sequence of single calls would find them
// (counters[0] never passes the capacity), what the view adds, and the counters as append_kernel leaves them
__global__ __launch_bounds__(64) void scan_batch_kernel(BatchWords* bw, uint32_t n_views, uint32_t cap, uint32_t* counters) {
  const uint32_t v = threadIdx.x;
  const unsigned long long rows = counters[0], t = v < n_views ? bw->total[v] : 0u;
  unsigned long long incl = t;
  for (uint32_t d = 1; d < 64u; d <<= 1) {
    const unsigned long long up = __shfl_up(incl, d);
    if (v >= d) incl += up;
  }
  const unsigned long long before = min(rows + incl - t, (unsigned long long)cap), after = min(rows + incl, (unsigned long long)cap);
  if (v < n_views) { bw->base[v] = (uint32_t)before; bw->added[v] = (uint32_t)(after - before); }
  if (v == 63u) { counters[1] = (uint32_t)(after - min(rows, (unsigned long long)cap)); counters[0] = (uint32_t)after; }
}

__global__ __launch_bounds__(256) void append_batch_kernel(const uint32_t* __restrict__ flags, BatchCounts cnt, uint32_t n_features,
                                                           const uint8_t* __restrict__ kp_desc, const float* __restrict__ pts_tmp,
                                                           const BatchWords* __restrict__ bw, uint8_t* desc, float* pts) {
  __shared__ uint32_t wave_n[4];
  const uint32_t v = blockIdx.x, n = cnt.n[v], tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
  const uint32_t base = bw->base[v], added = bw->added[v];  // rows base .. base + added - 1 are this view's: all below the capacity
  uint32_t done = 0;                                        // accepted keypoints of the view before this round's 256
  for (uint32_t i0 = 0; i0 < n && done < added; i0 += 256u) {
    const uint32_t i = i0 + tid;
    const size_t src = (size_t)v * n_features + i;
    const bool f = i < n && flags[src] != 0u;
    const unsigned long long b = __ballot(f);
    if (lane == 0u) wave_n[w] = (uint32_t)__popcll(b);
    __syncthreads();
    uint32_t r = done, all = 0;
    for (uint32_t k = 0; k < 4u; ++k) { const uint32_t c = wave_n[k]; r += k < w ? c : 0u; all += c; }
    r += (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
    if (f && r < added) {
      const size_t o = (size_t)base + r;
      const uint4* s16 = reinterpret_cast<const uint4*>(kp_desc) + 2 * src;   // a descriptor: two 16-byte copies
      uint4* d16 = reinterpret_cast<uint4*>(desc) + 2 * o;
      d16[0] = s16[0]; d16[1] = s16[1];
      pts[3 * o] = pts_tmp[3 * src]; pts[3 * o + 1] = pts_tmp[3 * src + 1]; pts[3 * o + 2] = pts_tmp[3 * src + 2];
    }
    done += all;
    __syncthreads();                                        // wave_n is written again in the next round
  }
}

}  // namespace

extern "C" {

int todhip_model_begin(todhip_ctx* ctx, uint32_t capacity_rows, todhip_model** out) {
  if (!ctx || !out || capacity_rows == 0) return TODHIP_EINVAL;
  TOD_HIP(hipSetDevice(ctx->device));
  todhip_model* m = new (std::nothrow) todhip_model();
  if (!m) return TODHIP_ENOMEM;
  m->cap = capacity_rows;
  hipError_t e = m->desc.reserve((size_t)capacity_rows * 32);
  if (e == hipSuccess) e = m->pts.reserve((size_t)capacity_rows * 12);
  if (e == hipSuccess) e = m->small.reserve(64 * sizeof(uint32_t));
  if (e == hipSuccess) e = hipMemsetAsync(m->small.p, 0, 64 * sizeof(uint32_t), ctx->stream);
  if (e != hipSuccess) { ctx->last_hip_error = (int)e; delete m; return TODHIP_EHIP; }
  *out = m;
  return TODHIP_OK;
}

void todhip_model_free(todhip_ctx* ctx, todhip_model* m) {
  if (!m) return;
  if (ctx) { (void)hipSetDevice(ctx->device); (void)hipStreamSynchronize(ctx->stream); }
  delete m;
}

// Trainer::process for one observation (Trainer.cpp:136-171). depth has the image size (rescale_depth's equal-size
// branch, :63-72): float metres or uint16 millimetres. K9/R9 row-major, T3. *n_added = rows appended to the model.
int todhip_model_add_observation(todhip_ctx* ctx, todhip_model* m, const uint8_t* gray, const uint8_t* mask, const void* depth,
                                 int depth_is_u16, uint32_t H, uint32_t W, const float* K9, const float* R9, const float* T3,
                                 uint32_t n_features, uint32_t n_levels, float scale_factor, const int8_t* pattern,
                                 uint32_t* n_added) {
  if (!ctx || !m || !gray || !mask || !depth || !K9 || !R9 || !T3 || H < 8 || W < 8 || n_features == 0) return TODHIP_EINVAL;
  if (const int bad = tod_orb::check_pattern(pattern)) return bad;     // before the view is copied in
  TOD_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const size_t px = (size_t)H * W, dbytes = px * (depth_is_u16 ? 2 : 4);
  TOD_HIP(m->img.reserve(px)); TOD_HIP(m->mask.reserve(px)); TOD_HIP(m->er_tmp.reserve(px)); TOD_HIP(m->er.reserve(px));
  TOD_HIP(m->depth.reserve(dbytes));
  TOD_HIP(m->kp_xy.reserve((size_t)n_features * 8)); TOD_HIP(m->kp_aux.reserve((size_t)n_features * 16));
  TOD_HIP(m->kp_desc.reserve((size_t)n_features * 32)); TOD_HIP(m->flags.reserve((size_t)n_features * 4));
  TOD_HIP(m->offs.reserve((size_t)n_features * 12));
  TOD_HIP(hipMemcpyAsync(m->img.p, gray, px, hipMemcpyHostToDevice, st));
  TOD_HIP(hipMemcpyAsync(m->mask.p, mask, px, hipMemcpyHostToDevice, st));
  TOD_HIP(hipMemcpyAsync(m->depth.p, depth, dbytes, hipMemcpyHostToDevice, st));
  uint32_t n_kp = 0;
  int rc = tod_orb_device(ctx, m->img.as<uint8_t>(), m->mask.as<uint8_t>(), H, W, W, n_features, n_levels, scale_factor, pattern,
                          m->kp_xy.as<float>(), m->kp_aux.as<float>(), m->kp_desc.as<uint8_t>(), n_features, &n_kp);
  if (rc != TODHIP_OK) return rc;
  if (n_added) *n_added = 0;
  if (n_kp == 0) return TODHIP_OK;
  uint32_t* d_small = m->small.as<uint32_t>();
  TOD_HIP(hipMemcpyAsync(d_small + 2, &n_kp, sizeof(uint32_t), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(erode_rows_kernel, dim3((uint32_t)((px + 255) / 256)), dim3(256), 0, st, m->mask.as<uint8_t>(), H, W, m->er_tmp.as<uint8_t>());
  hipLaunchKernelGGL(erode_cols_kernel, dim3((uint32_t)((px + 255) / 256)), dim3(256), 0, st, m->er_tmp.as<uint8_t>(), H, W, m->er.as<uint8_t>());
  Cam cam;
  cam.fx = K9[0]; cam.fy = K9[4]; cam.cx = K9[2]; cam.cy = K9[5];
  std::memcpy(cam.R, R9, sizeof(cam.R)); std::memcpy(cam.T, T3, sizeof(cam.T));
  hipLaunchKernelGGL(validate_kernel, dim3((n_kp + 255u) / 256u), dim3(256), 0, st, m->kp_xy.as<float>(), d_small + 2,
                     m->er.as<uint8_t>(), m->depth.p, depth_is_u16, H, W, cam, m->flags.as<uint32_t>(), m->offs.as<float>());
  hipLaunchKernelGGL(append_kernel, dim3(1), dim3(1024), 0, st, m->flags.as<uint32_t>(), d_small + 2, m->kp_desc.as<uint8_t>(),
                     m->offs.as<float>(), d_small, m->cap, m->desc.as<uint8_t>(), m->pts.as<float>());
  TOD_HIP(hipGetLastError());
  uint32_t h[2] = {0, 0};
  TOD_HIP(hipMemcpyAsync(h, d_small, sizeof(h), hipMemcpyDeviceToHost, st));
  TOD_HIP(hipStreamSynchronize(st));                     // also keeps gray/mask/depth/n_kp alive until the copies are done
  if (n_added) *n_added = h[1];
  return TODHIP_OK;
}

// Trainer::process (Trainer.cpp:121-187) for n_views device-resident views in one call; the definition is include/todhip.h's: the
// model after the sequence of todhip_rescale_depth + todhip_model_add_observation per view, byte for byte. One batched masked ORB
// call, one copy of the cameras, four launches, one copy back, one synchronization.
int todhip_model_add_observations_device(todhip_ctx* ctx, todhip_model* m, const void* d_gray, uint64_t frame_stride, uint32_t stride,
                                         const void* d_mask, const void* d_depth, int depth_is_u16, uint32_t dH, uint32_t dW,
                                         int nearest, uint32_t n_views, uint32_t H, uint32_t W, const float* K9, const float* R9,
                                         const float* T3, uint32_t n_features, uint32_t n_levels, float scale_factor,
                                         const int8_t* pattern, uint32_t* n_added) {
  if (!ctx || !m || !d_gray || !d_mask || !d_depth || !K9 || !R9 || !T3 || H < 8 || W < 8 || n_features == 0) return TODHIP_EINVAL;
  if (n_views == 0 || n_views > kTrainBatchMaxViews || stride < W) return TODHIP_EINVAL;
  if (n_views > 1 && frame_stride < (uint64_t)H * stride) return TODHIP_EINVAL;
  if ((dH == 0) != (dW == 0) || (uint64_t)H * W > 0xFFFFFFFFull) return TODHIP_EINVAL;
  if (dH == 0) { dH = H; dW = W; }
  tod::RescaleGeom geom;
  if (!tod::rescale_geometry(dH, dW, H, W, nearest, &geom)) return TODHIP_EINVAL;
  if (const int bad = tod_orb::check_args(n_views, H, W, n_features, n_levels, scale_factor, n_features)) return bad;
  if (const int bad = tod_orb::check_pattern(pattern)) return bad;
  TOD_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const size_t rows = (size_t)n_views * n_features;
  TOD_HIP(m->kp_xy.reserve(rows * 8)); TOD_HIP(m->kp_aux.reserve(rows * 16)); TOD_HIP(m->kp_desc.reserve(rows * 32));
  TOD_HIP(m->flags.reserve(rows * 4)); TOD_HIP(m->offs.reserve(rows * 12));
  TOD_HIP(m->cams.reserve(kTrainBatchMaxViews * sizeof(Cam))); TOD_HIP(m->batch.reserve(sizeof(BatchWords)));
  BatchCounts cnt = {};
  const int rc = tod_orb_batch_device(ctx, static_cast<const uint8_t*>(d_gray), (size_t)frame_stride, static_cast<const uint8_t*>(d_mask),
                                      n_views, H, W, stride, n_features, n_levels, scale_factor, pattern, m->kp_xy.as<float>(),
                                      m->kp_aux.as<float>(), m->kp_desc.as<uint8_t>(), n_features, cnt.n);
  if (rc != TODHIP_OK) return rc;
  if (n_added) std::memset(n_added, 0, n_views * sizeof(uint32_t));
  uint32_t most = 0;
  for (uint32_t v = 0; v < n_views; ++v) most = std::max(most, cnt.n[v]);
  if (most == 0) return TODHIP_OK;
  Cam cams[kTrainBatchMaxViews];
  for (uint32_t v = 0; v < n_views; ++v) {
    const float* K = K9 + 9 * (size_t)v;
    cams[v].fx = K[0]; cams[v].fy = K[4]; cams[v].cx = K[2]; cams[v].cy = K[5];
    std::memcpy(cams[v].R, R9 + 9 * (size_t)v, sizeof(cams[v].R)); std::memcpy(cams[v].T, T3 + 3 * (size_t)v, sizeof(cams[v].T));
  }
  TOD_HIP(hipMemcpyAsync(m->cams.p, cams, n_views * sizeof(Cam), hipMemcpyHostToDevice, st));
  BatchWords* bw = m->batch.as<BatchWords>();
  uint32_t* d_small = m->small.as<uint32_t>();
  hipLaunchKernelGGL(validate_batch_kernel, dim3((most + 255u) / 256u, n_views), dim3(256), 0, st, m->kp_xy.as<float>(), cnt, n_features,
                     static_cast<const uint8_t*>(d_mask), static_cast<const uint8_t*>(d_depth), depth_is_u16, geom, H, W,
                     m->cams.as<Cam>(), m->flags.as<uint32_t>(), m->offs.as<float>());
  hipLaunchKernelGGL(count_batch_kernel, dim3(n_views), dim3(256), 0, st, m->flags.as<uint32_t>(), cnt, n_features, bw);
  hipLaunchKernelGGL(scan_batch_kernel, dim3(1), dim3(64), 0, st, bw, n_views, m->cap, d_small);
  hipLaunchKernelGGL(append_batch_kernel, dim3(n_views), dim3(256), 0, st, m->flags.as<uint32_t>(), cnt, n_features,
                     m->kp_desc.as<uint8_t>(), m->offs.as<float>(), bw, m->desc.as<uint8_t>(), m->pts.as<float>());
  TOD_HIP(hipGetLastError());
  uint32_t h_added[kTrainBatchMaxViews];
  TOD_HIP(hipMemcpyAsync(h_added, bw->added, n_views * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  TOD_HIP(hipStreamSynchronize(st));                     // also keeps cams and h_added alive until the copies are done
  if (n_added) std::memcpy(n_added, h_added, n_views * sizeof(uint32_t));
  return TODHIP_OK;
}

// rescale_depth (Trainer.cpp:62-81) on device-resident images: d_depth_in dH x dW (float metres or uint16 mm),
// d_depth_out H x W float metres. Asynchronous on the context's stream.
int todhip_rescale_depth_device(todhip_ctx* ctx, const void* d_depth_in, int depth_is_u16, uint32_t dH, uint32_t dW,
                                void* d_depth_out, uint32_t H, uint32_t W, int nearest) {
  if (!ctx || !d_depth_in || !d_depth_out || !dH || !dW || !H || !W || (uint64_t)H * W > 0xFFFFFFFFull) return TODHIP_EINVAL;
  tod::RescaleGeom geom;
  if (!tod::rescale_geometry(dH, dW, H, W, nearest, &geom)) return TODHIP_EINVAL;
  TOD_HIP(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(rescale_depth_kernel, dim3((uint32_t)(((size_t)H * W + 255) / 256)), dim3(256), 0, ctx->stream, d_depth_in,
                     depth_is_u16, geom, static_cast<float*>(d_depth_out), H, W);
  TOD_HIP(hipGetLastError());
  return TODHIP_OK;
}

// Host-buffer form (what Trainer::process does per observation before validateKeyPoints, :142-143).
int todhip_rescale_depth(todhip_ctx* ctx, const void* depth_in, int depth_is_u16, uint32_t dH, uint32_t dW, float* depth_out,
                         uint32_t H, uint32_t W, int nearest) {
  if (!ctx || !depth_in || !depth_out || !dH || !dW || !H || !W) return TODHIP_EINVAL;
  TOD_HIP(hipSetDevice(ctx->device));
  const size_t in_bytes = (size_t)dH * dW * (depth_is_u16 ? 2 : 4), out_bytes = (size_t)H * W * 4;
  DevBuf in, out;
  int rc = TODHIP_OK;
  if (in.reserve(in_bytes) != hipSuccess || out.reserve(out_bytes) != hipSuccess) rc = TODHIP_EHIP;
  if (rc == TODHIP_OK && hipMemcpyAsync(in.p, depth_in, in_bytes, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) rc = TODHIP_EHIP;
  if (rc == TODHIP_OK) rc = todhip_rescale_depth_device(ctx, in.p, depth_is_u16, dH, dW, out.p, H, W, nearest);
  if (rc == TODHIP_OK && hipMemcpyAsync(depth_out, out.p, out_bytes, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) rc = TODHIP_EHIP;
  (void)hipStreamSynchronize(ctx->stream);                    // (in and out are freed on return, after the copies)
  return rc;
}

// Rows trained earlier (a stored model, ModelFiller.cpp:23-24) behind the model's rows, cut at its capacity.
int todhip_model_add_rows(todhip_ctx* ctx, todhip_model* m, const uint8_t* desc, const float* pts_xyz, uint32_t n, uint32_t* n_added) {
  if (n_added) *n_added = 0;
  if (!ctx || !m || (n && (!desc || !pts_xyz))) return TODHIP_EINVAL;
  if (n == 0) return TODHIP_OK;
  TOD_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  uint32_t rows = 0;
  TOD_HIP(hipMemcpyAsync(&rows, m->small.p, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  TOD_HIP(hipStreamSynchronize(st));
  if (rows > m->cap) return TODHIP_EINVAL;
  const uint32_t add = std::min(n, m->cap - rows);
  const uint32_t h[2] = {rows + add, add};                  // as append_kernel leaves the counters
  if (add) {
    TOD_HIP(hipMemcpyAsync(m->desc.as<uint8_t>() + (size_t)rows * 32, desc, (size_t)add * 32, hipMemcpyHostToDevice, st));
    TOD_HIP(hipMemcpyAsync(m->pts.as<float>() + (size_t)rows * 3, pts_xyz, (size_t)add * 12, hipMemcpyHostToDevice, st));
  }
  TOD_HIP(hipMemcpyAsync(m->small.p, h, sizeof(h), hipMemcpyHostToDevice, st));
  TOD_HIP(hipStreamSynchronize(st));                        // desc, pts_xyz and h may go once this returns
  if (n_added) *n_added = add;
  return TODHIP_OK;
}

// mergePoints (training.cpp:147-173) + ModelFiller (ModelFiller.cpp:20-26): the stacked descriptors and points.
// the model where it is: device pointers of its descriptors (n x 32) and points (n x 3 f32), valid until todhip_model_free --
// todhip_db_load_device takes them as a todhip_object, so a freshly trained model reaches the matcher without visiting the host
int todhip_model_device(todhip_ctx* ctx, todhip_model* m, const void** d_desc, const void** d_pts_xyz, uint32_t* n) {
  if (!ctx || !m || !n) return TODHIP_EINVAL;
  TOD_HIP(hipSetDevice(ctx->device));
  uint32_t rows = 0;
  TOD_HIP(hipMemcpyAsync(&rows, m->small.p, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  TOD_HIP(hipStreamSynchronize(ctx->stream));                 // (every observation's kernels have run: the buffers are complete)
  *n = rows;
  if (d_desc) *d_desc = m->desc.p;
  if (d_pts_xyz) *d_pts_xyz = m->pts.p;
  return TODHIP_OK;
}

int todhip_model_finish(todhip_ctx* ctx, todhip_model* m, uint8_t* desc, float* pts, uint32_t* n) {
  if (!ctx || !m || !n) return TODHIP_EINVAL;
  TOD_HIP(hipSetDevice(ctx->device));
  uint32_t rows = 0;
  TOD_HIP(hipMemcpyAsync(&rows, m->small.p, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  TOD_HIP(hipStreamSynchronize(ctx->stream));
  const uint32_t cap = *n;
  *n = rows;
  if (rows > cap) return TODHIP_ECAPACITY;
  if (rows && (!desc || !pts)) return TODHIP_EINVAL;
  if (rows) {
    TOD_HIP(hipMemcpyAsync(desc, m->desc.p, (size_t)rows * 32, hipMemcpyDeviceToHost, ctx->stream));
    TOD_HIP(hipMemcpyAsync(pts, m->pts.p, (size_t)rows * 12, hipMemcpyDeviceToHost, ctx->stream));
    TOD_HIP(hipStreamSynchronize(ctx->stream));
  }
  return TODHIP_OK;
}

}  // extern "C"
