// Stand-alone driver of tod_amd/csrc/db_bitorder.h for tests/test_bit_order_cpu.py: built with the host compiler and
// -fsanitize=address,undefined, run as its own process. Input file (text): S, 256 x ones, 256 x 256 x both (row a, column b).
// Output: the 256 ranks on one line, the 256 entries of src_of on the next.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "db_bitorder.h"

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s statistics.txt\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "r");
  if (!f) { perror(argv[1]); return 2; }
  unsigned long long S = 0;
  std::vector<uint32_t> ones(256), both(256 * 256);
  bool ok = fscanf(f, "%llu", &S) == 1;
  for (size_t i = 0; i < ones.size() && ok; ++i) ok = fscanf(f, "%u", &ones[i]) == 1;
  for (size_t i = 0; i < both.size() && ok; ++i) ok = fscanf(f, "%u", &both[i]) == 1;
  fclose(f);
  if (!ok || S == 0 || S > 65536) { fprintf(stderr, "bad statistics file\n"); return 2; }
  uint8_t rank[256], src_of[256];
  tod_bit_order_rank(S, ones.data(), both.data(), rank);
  tod_bit_order_layout(rank, src_of);
  for (int i = 0; i < 256; ++i) printf("%d%c", rank[i], i == 255 ? '\n' : ' ');
  for (int i = 0; i < 256; ++i) printf("%d%c", src_of[i], i == 255 ? '\n' : ' ');
  return 0;
}
