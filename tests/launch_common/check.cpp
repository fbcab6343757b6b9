// Prints what csrc/launch_common.hpp answers for the cases of
// tests/test_launch_common_cpu.py, one line per case.  Plain host C++17.
#include <cinttypes>
#include <cstdio>
#include <initializer_list>

#include "launch_common.hpp"

using namespace np;

template <int... Ks>
void k_cases(const char* name, std::initializer_list<uint32_t> ks) {
  for (uint32_t k : ks)
    std::printf("with_k %s %u %d\n", name, k, with_k<Ks...>(k, -1, [](auto kc) { return static_cast<int>(kc.value); }));
}

void show(const char* name, uint64_t count, unsigned width, uint64_t batch, const TileGrid& g) {
  static const char* const state[] = {"empty", "invalid", "ok"};
  std::printf("%s %" PRIu64 " %u %" PRIu64 " %s", name, count, width, batch, state[g.state]);
  if (g.state == kGridOk) std::printf(" count=%u tiles=%u per=%u blocks=%u", g.count, g.tiles, g.per, g.blocks);
  std::printf("\n");
}

int main() {
  k_cases<64, 128, 256>("fast", {64, 128, 256, 0, 3, 96, 512});
  k_cases<1, 2, 4, 8, 16, 32>("small", {1, 2, 4, 8, 16, 32, 0, 3, 96, 512});
  k_cases<2, 4, 8, 16>("huge_m", {2, 4, 8, 16, 0, 3, 96, 512});
  k_cases<1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024>("records",
                                                      {1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 0, 3, 96, 2048});
  std::printf("k_in %d %d %d\n", k_in(Ints<64, 128, 256>{}, 128), k_in(Ints<64, 128, 256>{}, 96),
              k_in(Ints<64, 128, 256>{}, 0));

  for (uint32_t k : {1u, 64u, 1024u}) {
    for (uint32_t n : {k, 2 * k, 3 * k, 4 * k, 8 * k, 16 * k, 2 * k + 1})
      std::printf("with_nq %u %u %d %d\n", n, k, with_nq(n, k, -1, [](auto qc) { return static_cast<int>(qc.value); }),
                  nq_supported(n, k) ? 1 : 0);
  }
  std::printf("with_nq 8 0 %d\n", with_nq(8, 0, -1, [](auto qc) { return static_cast<int>(qc.value); }));

  const uint64_t two31 = uint64_t{1} << 31, two32 = uint64_t{1} << 32;
  for (unsigned w : {256u, 64u}) {
    for (uint64_t count : std::initializer_list<uint64_t>{0, 1, 64, 65, 256, 257, two32 - 1, two32})
      show("grid", count, w, 1, tile_grid(count, w, 1));
    show("grid", 1, w, 0, tile_grid(1, w, 0));
    show("grid", 1, w, two31 - 1, tile_grid(1, w, two31 - 1));
    show("grid", 1, w, two31, tile_grid(1, w, two31));
    // around the limit with three tiles per entry
    show("grid", 3 * w, w, 715827882, tile_grid(3 * w, w, 715827882));  // 3 tiles * 715827882 = 2^31 - 2
    show("grid", 3 * w, w, 715827883, tile_grid(3 * w, w, 715827883));  // 2^31 + 1
    // workgroups of two consecutive tiles of one entry
    show("grid2", 5 * w, w, 3, tile_grid(5 * w, w, 3, [](uint32_t) { return 2u; }));
    show("grid2", 5 * w, w, two31 / 3 + 1, tile_grid(5 * w, w, two31 / 3 + 1, [](uint32_t) { return 2u; }));
    // four tiles per workgroup numbered across the entries
    for (uint64_t batch : std::initializer_list<uint64_t>{0, 1, 4, 5, two32 - 1, two32})
      show("packed", 1, w, batch, tile_grid_packed(1, w, batch, 4));
    show("packed", 0, w, 1, tile_grid_packed(0, w, 1, 4));
    show("packed", 5 * w, w, 1, tile_grid_packed(5 * w, w, 1, 4));
    show("packed", two32 - 1, w, 1, tile_grid_packed(two32 - 1, w, 1, 4));
    show("packed", two32, w, 1, tile_grid_packed(two32, w, 1, 4));
    show("packed", 2 * w, w, two31, tile_grid_packed(2 * w, w, two31, 4));  // batch * tiles = 2^32
  }
  return 0;
}
