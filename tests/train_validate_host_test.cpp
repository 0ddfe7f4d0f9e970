// tod_amd/csrc/train_validate.h on the host (tests/test_train_batch_cpu.py builds this with -fsanitize=address,undefined). For every
// case of a list -- one line "H W n mask_file keypoint_file depth_file camera_file result_prefix" each: an H x W u8 mask, n keypoints
// (x, y) f32, an H x W f32 depth image in metres, a camera of 16 f32 (fx fy cx cy R[9] T[3]) --
//   * the eroded pixel at every pixel, borders included, from eroded_at and from eroded_window (all 25 bits of every window), against
//     four erosions by the 3 x 3 element written here (a pixel outside the image closes nothing);
//   * every keypoint through the header as validate_batch_kernel uses it (the window's bits) and as validate_kernel uses it (a lookup
//     in an eroded image), against a brute-force statement of the rescue's tie rule: the open pixels of the clipped +-2 window, the
//     least float32 squared distance, among those the lowest column, among those the lowest row.
// Any disagreement is a line on stderr and exit status 1. The buffers are exactly H x W, so a read outside the mask or the depth image
// is the sanitizer's to report. Written for Python to compare with tests/train_ref.py: <prefix>.er (H x W u8), <prefix>.res
// (n x 3 i32: class 0 direct / 1 rescued / 2 outside the mask / 3 invalid depth, then the chosen column and row) and <prefix>.pts
// (n x 3 f32, zeros where the keypoint is not accepted). Prints "ok <H> <W> <n>" per case.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "train_validate.h"

static bool read_all(const char* path, void* dst, size_t bytes) {
  FILE* f = std::fopen(path, "rb");
  if (!f) return false;
  const size_t got = bytes ? std::fread(dst, 1, bytes, f) : 0;
  const bool at_end = std::fgetc(f) == EOF;
  std::fclose(f);
  return got == bytes && at_end;
}

static bool write_all(const std::string& path, const void* src, size_t bytes) {
  FILE* f = std::fopen(path.c_str(), "wb");
  if (!f) return false;
  const bool ok = std::fwrite(src, 1, bytes, f) == bytes;
  return std::fclose(f) == 0 && ok;
}

// cv::erode by the 3 x 3 element, border value +inf, four times
static std::vector<uint8_t> erode4(const std::vector<uint8_t>& mask, int H, int W) {
  std::vector<uint8_t> a(mask.size()), b(mask.size());
  for (size_t i = 0; i < mask.size(); ++i) a[i] = mask[i] ? 255 : 0;
  for (int it = 0; it < 4; ++it) {
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        uint8_t v = 255;
        for (int dy = -1; dy <= 1; ++dy)
          for (int dx = -1; dx <= 1; ++dx) {
            const int yy = y + dy, xx = x + dx;
            if (yy >= 0 && yy < H && xx >= 0 && xx < W && a[(size_t)yy * W + xx] < v) v = a[(size_t)yy * W + xx];
          }
        b[(size_t)y * W + x] = v;
      }
    a.swap(b);
  }
  return a;
}

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: %s case_list\n", argv[0]); return 2; }
  FILE* list = std::fopen(argv[1], "r");
  if (!list) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  int H, W, n, bad = 0;
  char mask_path[1024], kp_path[1024], depth_path[1024], cam_path[1024], prefix[1024];
  while (std::fscanf(list, "%d %d %d %1023s %1023s %1023s %1023s %1023s", &H, &W, &n, mask_path, kp_path, depth_path, cam_path, prefix) == 8) {
    const size_t px = (size_t)H * W;
    std::vector<uint8_t> mask(px);
    std::vector<float> kp((size_t)n * 2), depth(px);
    tod::TrainCam cam;
    static_assert(sizeof(cam) == 16 * sizeof(float), "a camera is 16 floats");
    if (!read_all(mask_path, mask.data(), px) || !read_all(kp_path, kp.data(), kp.size() * 4) || !read_all(depth_path, depth.data(), px * 4) ||
        !read_all(cam_path, &cam, sizeof(cam))) {
      std::fprintf(stderr, "bad input files of %s\n", prefix);
      return 2;
    }
    const std::vector<uint8_t> er = erode4(mask, H, W);
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        const bool want = er[(size_t)y * W + x] != 0;
        if (tod::eroded_at(mask.data(), H, W, x, y) != want) { std::fprintf(stderr, "%s: eroded_at(%d, %d)\n", prefix, x, y); ++bad; }
        const uint32_t win = tod::eroded_window(mask.data(), H, W, x, y);
        if (win >> 25) { std::fprintf(stderr, "%s: eroded_window(%d, %d) sets bits above 24\n", prefix, x, y); ++bad; }
        for (int dy = -2; dy <= 2; ++dy)
          for (int dx = -2; dx <= 2; ++dx) {
            const int xx = x + dx, yy = y + dy;
            const bool in = xx >= 0 && xx < W && yy >= 0 && yy < H;
            const bool w = in && er[(size_t)yy * W + xx] != 0;
            if (tod::eroded_window_at(win, x, y, xx, yy) != w) { std::fprintf(stderr, "%s: eroded_window(%d, %d) at (%d, %d)\n", prefix, x, y, dx, dy); ++bad; }
          }
      }
    tod::RescaleGeom geom;
    if (!tod::rescale_geometry((uint32_t)H, (uint32_t)W, (uint32_t)H, (uint32_t)W, 0, &geom) || geom.mode != tod::RescaleGeom::kEqual) return 2;
    std::vector<int32_t> res((size_t)n * 3);
    std::vector<float> pts((size_t)n * 3, 0.f);
    for (int i = 0; i < n; ++i) {
      const float fx = kp[2 * (size_t)i], fy = kp[2 * (size_t)i + 1];
      int x0, y0;
      tod::rounded_pixel(fx, fy, H, W, &x0, &y0);
      // as validate_batch_kernel
      const uint32_t win = tod::eroded_window(mask.data(), H, W, x0, y0);
      int xb = x0, yb = y0;
      bool good_b = tod::eroded_window_at(win, x0, y0, x0, y0), rescued = false;
      if (!good_b) rescued = good_b = tod::rescue_pixel([&](int ii, int jj) { return tod::eroded_window_at(win, x0, y0, ii, jj); }, fx, fy, H, W, &xb, &yb);
      // as validate_kernel
      int xs = x0, ys = y0;
      bool good_s = er[(size_t)y0 * W + x0] != 0;
      if (!good_s) good_s = tod::rescue_pixel([&](int ii, int jj) { return er[(size_t)jj * W + ii] != 0; }, fx, fy, H, W, &xs, &ys);
      if (good_b != good_s || xb != xs || yb != ys) { std::fprintf(stderr, "%s: keypoint %d differs between the two lookups\n", prefix, i); ++bad; }
      // the tie rule, brute force
      int xw = x0, yw = y0;
      bool good_w = er[(size_t)y0 * W + x0] != 0;
      if (!good_w) {
        struct C { int x, y; float d; };
        std::vector<C> c;
        for (int dy = -2; dy <= 2; ++dy)
          for (int dx = -2; dx <= 2; ++dx) {
            const int xx = x0 + dx, yy = y0 + dy;
            if (xx < 0 || xx >= W || yy < 0 || yy >= H || !er[(size_t)yy * W + xx]) continue;
            const float ddx = (float)xx - fx, ddy = (float)yy - fy;
            const float sx = ddx * ddx, sy = ddy * ddy;
            c.push_back({xx, yy, sx + sy});
          }
        if (!c.empty()) {
          float dmin = c[0].d;
          for (const C& k : c) if (k.d < dmin) dmin = k.d;
          int xmin = W;
          for (const C& k : c) if (k.d == dmin && k.x < xmin) xmin = k.x;
          int ymin = H;
          for (const C& k : c) if (k.d == dmin && k.x == xmin && k.y < ymin) ymin = k.y;
          xw = xmin; yw = ymin; good_w = true;
        }
      }
      if (good_b != good_w || xb != xw || yb != yw) {
        std::fprintf(stderr, "%s: keypoint %d (%g, %g): (%d, %d, %d), brute force (%d, %d, %d)\n", prefix, i, (double)fx, (double)fy, (int)good_b, xb, yb,
                     (int)good_w, xw, yw);
        ++bad;
      }
      int cls = good_b ? (rescued ? 1 : 0) : 2;
      if (good_b) {
        const float z = tod::train_depth_at(depth.data(), 0, geom, xb, yb);
        if (!tod::valid_depth(z)) cls = 3;
        else tod::back_project(cam, xb, yb, z, &pts[3 * (size_t)i]);
      }
      res[3 * (size_t)i] = cls; res[3 * (size_t)i + 1] = xb; res[3 * (size_t)i + 2] = yb;
    }
    const std::string p(prefix);
    if (!write_all(p + ".er", er.data(), px) || !write_all(p + ".res", res.data(), res.size() * 4) || !write_all(p + ".pts", pts.data(), pts.size() * 4)) {
      std::fprintf(stderr, "cannot write %s.*\n", prefix);
      return 2;
    }
    std::printf("ok %d %d %d\n", H, W, n);
  }
  std::fclose(list);
  return bad ? 1 : 0;
}
