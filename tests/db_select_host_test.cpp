// Stand-alone driver of tod_amd/csrc/db_select.h for tests/test_db_select_cpu.py: built with the host compiler and
// -fsanitize=address,undefined, run as its own process. Arguments: shard_first shard_rows, then after "--" the objects' row counts,
// then after "--" the ids of the selection. Output: "EINVAL", or five lines -- the distinct selected objects; selected_rows and the
// view's rows; per segment "object:first view row:first global row"; the global row of every view row; the segment of every view
// row found by walking forward from the segment of the row's 128-row group (what the gather kernel does).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "db_select.h"

int main(int argc, char** argv) {
  if (argc < 5) { fprintf(stderr, "usage: %s shard_first shard_rows -- rows... -- ids...\n", argv[0]); return 2; }
  const uint64_t shard_first = strtoull(argv[1], nullptr, 10), shard_rows = strtoull(argv[2], nullptr, 10);
  std::vector<uint32_t> off(1, 0u), ids;
  int a = 4;
  for (; a < argc && strcmp(argv[a], "--") != 0; ++a) off.push_back(off.back() + (uint32_t)strtoul(argv[a], nullptr, 10));
  for (++a; a < argc; ++a) ids.push_back((uint32_t)strtoul(argv[a], nullptr, 10));
  TodViewTables t;
  t.selected_rows = 12345;                                   // a refused list leaves *out alone
  if (!tod_view_build(ids.data(), (uint32_t)ids.size(), off.data(), (uint32_t)off.size() - 1u, shard_first, shard_rows, &t)) {
    if (t.selected_rows != 12345 || !t.objs.empty()) return 3;
    printf("EINVAL\n");
    return 0;
  }
  for (size_t i = 0; i < t.objs.size(); ++i) printf("%u%c", t.objs[i], i + 1 == t.objs.size() ? '\n' : ' ');
  if (t.objs.empty()) printf("\n");
  printf("%llu %u\n", (unsigned long long)t.selected_rows, t.view_rows());
  for (uint32_t j = 0; j < t.n_segs(); ++j) printf("%u:%u:%u%c", t.seg_obj[j], t.seg_view[j], t.seg_global[j], j + 1 == t.n_segs() ? '\n' : ' ');
  if (t.n_segs() == 0) printf("\n");
  for (uint32_t r = 0; r < t.view_rows(); ++r) printf("%u%c", tod_view_to_global(t, r), r + 1 == t.view_rows() ? '\n' : ' ');
  if (t.view_rows() == 0) printf("\n");
  for (uint32_t r = 0; r < t.view_rows(); ++r) {
    uint32_t s = tod_view_segment(t.seg_view.data(), t.n_segs(), r / 128u * 128u);
    while (r >= t.seg_view[s + 1]) ++s;
    printf("%u%c", s, r + 1 == t.view_rows() ? '\n' : ' ');
  }
  if (t.view_rows() == 0) printf("\n");
  return 0;
}
