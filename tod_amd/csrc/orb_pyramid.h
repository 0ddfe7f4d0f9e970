// The images of stage A: the strided copy of the input into level 0, the fixed-point bilinear resize that makes level l from level
// l - 1, and the 7-tap Gaussian blur of every level that the descriptor tests read; load_px4 / store_px4, the unaligned four-pixel
// accesses that the blur and fast_nms_kernel share. Included by orb.hip inside its anonymous namespace, after orb_stages.h.

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ __launch_bounds__(256) void copy_rows_kernel(const uint8_t* __restrict__ src, uint32_t stride, uint8_t* dst,
                                                        uint32_t h, uint32_t w, size_t src_fs, size_t dst_fs) {
  src += blockIdx.y * src_fs; dst += blockIdx.y * dst_fs;   // frame
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= h * w) return;
  dst[i] = src[(size_t)(i / w) * stride + (i % w)];
}

// four pixels of a row at any byte offset: level rows have pitch w, so a pixel group is not dword-aligned
__device__ __forceinline__ uint32_t load_px4(const uint8_t* p) { uint32_t v; __builtin_memcpy(&v, p, 4); return v; }
__device__ __forceinline__ void store_px4(uint8_t* p, uint32_t v) { __builtin_memcpy(p, &v, 4); }

// 11-bit fixed-point bilinear resize, sample positions (x + 0.5) * sx - 0.5, replicate border: the source indices and weights of
// every column and row come from the plan's tap tables (resize_taps), the blend is the integer one. A block writes a tile of
// 4 kResizeGroups x kResizeRows pixels, a lane four neighbouring pixels of a row; a group past the row's end has copies of the last
// column's taps, so every lane of a row computes four pixels and stores those inside it.
__global__ __launch_bounds__(256) void resize_kernel(const uint8_t* __restrict__ src, uint32_t sw, uint8_t* dst, uint32_t dh, uint32_t dw,
                                                     const ResizeTap* __restrict__ xtaps, const ResizeTap* __restrict__ ytaps, size_t fs) {
  src += blockIdx.z * fs; dst += blockIdx.z * fs;
  const uint32_t x = 4u * (blockIdx.x * kResizeGroups + threadIdx.x % kResizeGroups), y = blockIdx.y * kResizeRows + threadIdx.x / kResizeGroups;
  if (x >= dw || y >= dh) return;
  const ResizeTap ty = ytaps[y];
  const uint32_t ra = ty.a * sw, rb = ty.b * sw;             // 32-bit offsets into the frame's slice, as every pixel index of a level is
  uint32_t px = 0u;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const ResizeTap tx = xtaps[x + i];
    // every factor is below 2^24 and every sum below 2^31 (255 * 2048 * 2048 + 2^21): the 24-bit multiplies are exact
    const uint32_t top = __umul24(src[ra + tx.a], tx.wa) + __umul24(src[ra + tx.b], tx.wb);
    const uint32_t bot = __umul24(src[rb + tx.a], tx.wa) + __umul24(src[rb + tx.b], tx.wb);
    px |= (uint32_t)(uint8_t)((__umul24(top, ty.wa) + __umul24(bot, ty.wb) + (1u << 21)) >> 22) << (8 * i);
  }
  uint8_t* o = dst + (y * dw + x);
  if (x + 3u < dw) {
    store_px4(o, px);
  } else {                                                   // the row ends inside these four
    o[0] = (uint8_t)px;
    if (x + 1u < dw) o[1] = (uint8_t)(px >> 8);
    if (x + 2u < dw) o[2] = (uint8_t)(px >> 16);
  }
}

__constant__ int c_gauss7[7] = {18, 33, 49, 56, 49, 33, 18};

// The 7-tap sums of two pixels in one register: pixels in bits 0-7 and 16-23, weights summing to 256, so a half-word's sum with
// the rounding term is at most 255 * 256 + 128 < 2^16 and never carries into its neighbour. Every half-word is the integer
// s + 128 of sum k c_gauss7[k] * pixel[k], and its bits 8-15 are (s + 128) >> 8.
constexpr uint32_t kPairMask = 0x00FF00FFu, kPairRound = 0x00800080u;
__device__ __forceinline__ uint32_t gauss7_pairs(const uint32_t (&g)[7], const uint32_t* q) {
  uint32_t s = kPairRound;
#pragma unroll
  for (int k = 0; k < 7; ++k) s += g[k] * q[k];
  return s;
}
// four result pixels from the sums of pixels (0, 2) and of pixels (1, 3)
__device__ __forceinline__ uint32_t gauss7_px4(uint32_t even, uint32_t odd) { return ((even >> 8) & kPairMask) | (odd & ~kPairMask); }

// Separable 7-tap Gaussian, replicate border, in one launch: a block writes the horizontally blurred rows of a 128 x 64 pixel tile
// and of 3 rows above and below it into LDS, then runs the vertical pass from LDS; a lane works on four neighbouring pixels at a
// time. x is clamped in the horizontal pass; the vertical pass clamps the row index into the horizontally blurred image, so a halo
// row outside the image is the horizontal blur of row 0 or row h - 1.
constexpr int kBlurDw = kBlurTileW / 4, kBlurRows = kBlurTileH + 6, kBlurRun = 8;
__global__ __launch_bounds__(256) void blur_kernel(LevelTab T, uint8_t* dst, size_t fs) {
  const uint32_t v = blockIdx.z, lvl = v / T.F, f = v - lvl * T.F;
  const int h = (int)T.h[lvl], w = (int)T.w[lvl];
  const int x0 = (int)blockIdx.x * kBlurTileW, y0 = (int)blockIdx.y * kBlurTileH;
  if (T.want[lvl] == 0u || x0 >= w || y0 >= h) return;      // block-uniform; want != 0: w > 2 kEdge
  const uint8_t* __restrict__ src = T.img[lvl] + f * fs;
  dst += v * fs;
  __shared__ uint32_t s_h[kBlurRows * kBlurDw];             // row r: the horizontal blur of image row clamp(y0 - 3 + r), four pixels a word
  uint32_t g[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) g[k] = (uint32_t)c_gauss7[k];
  for (int t = (int)threadIdx.x; t < kBlurRows * kBlurDw; t += 256) {
    const int x = x0 + 4 * (t % kBlurDw);
    if (x >= w) continue;
    const uint8_t* row = src + (size_t)clampi(y0 - 3 + t / kBlurDw, 0, h - 1) * w;
    // a = pixels x - 4 .. x + 7 of the row, x clamped
    uint32_t a[3];
    if (x + 7 < w) {
      a[1] = load_px4(row + x); a[2] = load_px4(row + x + 4);
    } else {                                                 // the row ends inside these eight
      a[1] = 0u; a[2] = 0u;
#pragma unroll
      for (int i = 0; i < 8; ++i) a[1 + i / 4] |= (uint32_t)row[min(x + i, w - 1)] << (8 * (i % 4));
    }
    a[0] = x >= 4 ? load_px4(row + x - 4) : (a[1] & 0xFFu) * 0x01010101u;   // x is a multiple of 4: all four inside or all four pixel 0
    // q[j]: pixels x - 3 + j and x - 1 + j as a pair; result pixels (x, x + 2) use q[0..6], (x + 1, x + 3) use q[1..7]
    uint32_t q[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int i0 = j + 1, i1 = j + 3;
      q[j] = ((a[i0 / 4] >> (8 * (i0 % 4))) & 0xFFu) | (((a[i1 / 4] >> (8 * (i1 % 4))) & 0xFFu) << 16);
    }
    s_h[t] = gauss7_px4(gauss7_pairs(g, q), gauss7_pairs(g, q + 1));
  }
  __syncthreads();
  // a lane takes four columns and kBlurRun rows: one LDS word per row and a window of seven rows
  const int c = (int)(threadIdx.x % kBlurDw), r0 = (int)(threadIdx.x / kBlurDw) * kBlurRun, x = x0 + 4 * c;
  if (x >= w || y0 + r0 >= h) return;
  uint32_t even[kBlurRun + 6], odd[kBlurRun + 6];
#pragma unroll
  for (int i = 0; i < kBlurRun + 6; ++i) {
    const uint32_t px = s_h[(r0 + i) * kBlurDw + c];
    even[i] = px & kPairMask; odd[i] = (px >> 8) & kPairMask;
  }
#pragma unroll
  for (int j = 0; j < kBlurRun; ++j) {
    const int y = y0 + r0 + j;
    if (y >= h) break;
    const uint32_t px = gauss7_px4(gauss7_pairs(g, even + j), gauss7_pairs(g, odd + j));
    uint8_t* o = dst + (size_t)y * w + x;
    if (x + 3 < w) {
      store_px4(o, px);
    } else {
      for (int i = 0; x + i < w; ++i) o[i] = (uint8_t)(px >> (8 * i));
    }
  }
}
