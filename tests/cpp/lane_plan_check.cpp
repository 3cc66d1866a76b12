// lane_plan_check.cpp — dumps the chunk and lane plan of the multi-pass blind rotations (csrc/pbs_passes.hpp:
// chunk_items, lanes_wanted, lane_part) for tests/test_lane_plan_host.py, which checks every line against its own
// restatement of the rules.  Host only, no GPU:
//   hipcc -O2 -x hip lane_plan_check.cpp -o lane_plan_check && ./lane_plan_check OUT
// OUT is text, one record per line:
//   W nb dflt wanted              lanes_wanted(nb, dflt), nb = 1 ... 300, dflt = 0 ... 6
//   P nb lanes j off n            lane_part(nb, lanes, j) for every granted lane count 1 ... wanted and every lane j
//   C item_bytes batch chunk      chunk_items(item_bytes, batch)
#include <cstdio>

#include "../../tfhe-rs-main_modified_amd/csrc/pbs_passes.hpp"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* out = std::fopen(argv[1], "w");
  if (!out) return 4;
  for (uint32_t nb = 1; nb <= 300; ++nb) {
    int most = 1;  // the largest lane count any default asks for
    for (int dflt = 0; dflt <= 6; ++dflt) {
      const int wanted = mi::lanes_wanted(nb, dflt);
      std::fprintf(out, "W %u %d %d\n", nb, dflt, wanted);
      if (wanted > most) most = wanted;
    }
    for (int lanes = 1; lanes <= most; ++lanes)
      for (int j = 0; j < lanes; ++j) {
        const mi::LanePart p = mi::lane_part(nb, lanes, j);
        std::fprintf(out, "P %u %d %d %u %u\n", nb, lanes, j, p.off, p.n);
      }
  }
  const size_t gib4 = (size_t)4 << 30;
  const size_t items[] = {1, 4096, (size_t)5 << 20, (size_t)3 << 30, gib4 - 1, gib4, gib4 + 1, (size_t)1 << 40};
  const size_t batches[] = {1, 2, 70, 819, 820, 1000, (size_t)1 << 20, gib4 - 1, gib4, gib4 + 1, (size_t)1 << 40};
  for (size_t item : items)
    for (size_t batch : batches)
      std::fprintf(out, "C %zu %zu %zu\n", item, batch, mi::chunk_items(item, batch));
  return std::fclose(out) == 0 ? 0 : 4;
}
