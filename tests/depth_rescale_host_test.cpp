// tod_amd/csrc/depth_rescale.h on the host (tests/test_depth_rescale_cpu.py builds this with -fsanitize=address,undefined): for every
// case of a list -- one line "is_u16 dH dW H W nearest source_file result_file" each -- rescale_geometry, then rescaled_depth_at for
// every pixel of the H x W result, written as raw float32. Prints one line per case: "ok <sub_rows> <mode>" or "refused".
// The source buffer is exactly dH x dW values, so a tap outside it is the sanitizer's to report.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "depth_rescale.h"

static bool read_all(const char* path, std::vector<unsigned char>& buf, size_t bytes) {
  FILE* f = std::fopen(path, "rb");
  if (!f) return false;
  buf.resize(bytes);
  const size_t got = std::fread(buf.data(), 1, bytes, f);
  const bool at_end = std::fgetc(f) == EOF;
  std::fclose(f);
  return got == bytes && at_end;
}

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: %s case_list\n", argv[0]); return 2; }
  FILE* list = std::fopen(argv[1], "r");
  if (!list) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  int is_u16, nearest;
  unsigned dH, dW, H, W;
  char src_path[1024], dst_path[1024];
  while (std::fscanf(list, "%d %u %u %u %u %d %1023s %1023s", &is_u16, &dH, &dW, &H, &W, &nearest, src_path, dst_path) == 8) {
    tod::RescaleGeom g;
    if (!tod::rescale_geometry(dH, dW, H, W, nearest, &g)) { std::printf("refused\n"); continue; }
    std::vector<unsigned char> src;
    if (!read_all(src_path, src, (size_t)dH * dW * (is_u16 ? 2 : 4))) { std::fprintf(stderr, "bad source %s\n", src_path); return 2; }
    std::vector<float> out((size_t)H * W);
    for (unsigned y = 0; y < H; ++y)
      for (unsigned x = 0; x < W; ++x) out[(size_t)y * W + x] = tod::rescaled_depth_at(src.data(), is_u16, g, x, y);
    FILE* o = std::fopen(dst_path, "wb");
    if (!o || std::fwrite(out.data(), sizeof(float), out.size(), o) != out.size()) { std::fprintf(stderr, "cannot write %s\n", dst_path); return 2; }
    std::fclose(o);
    std::printf("ok %u %d\n", g.sub_rows, g.mode);
  }
  std::fclose(list);
  return 0;
}
