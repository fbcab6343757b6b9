// Launch dispatch and grid arithmetic shared by the kernel files: a runtime k
// or n / k to its compile-time instance, the conditions the *_supported
// predicates share, and the column count -> tiles -> workgroups arithmetic
// with its range checks.  Host-only plain C++17 (no HIP includes), so that a
// CPU program can include it (tests/test_launch_common_cpu.py).
#pragma once
#include <cstddef>
#include <cstdint>
#include <type_traits>

namespace np {

template <int F>
using Int = std::integral_constant<int, F>;

// A list of compile-time sizes, e.g. the K of a kernel family.
template <int... Ks>
struct Ints {};
// The segment counts n / k every specialised decode serves.
using NqList = Ints<2, 4, 8>;

// f(Int<K>{}) for the K of the list equal to k; `fallback` when there is none.
template <int... Ks, typename R, typename F>
R with_k(uint32_t k, R fallback, F&& f) {
  R r = fallback;
  (void)((k == static_cast<uint32_t>(Ks) && (r = f(Int<Ks>{}), true)) || ...);
  return r;
}
template <int... Ks, typename R, typename F>
R with_k(Ints<Ks...>, uint32_t k, R fallback, F&& f) {
  return with_k<Ks...>(k, fallback, f);
}

// f(Int<K>{}) for every K of the list, in order.
template <int... Ks, typename F>
void each_k(Ints<Ks...>, F&& f) {
  (f(Int<Ks>{}), ...);
}

// Whether k is in the list.
template <int... Ks>
constexpr bool k_in(Ints<Ks...>, uint32_t k) {
  return ((k == static_cast<uint32_t>(Ks)) || ...);
}

// n / k in {2, 4, 8}.
constexpr bool nq_supported(uint32_t n, uint32_t k) { return n == 2 * k || n == 4 * k || n == 8 * k; }

// f(Int<NQ>{}) for NQ = n / k in {2, 4, 8}; `fallback` for every other n, one
// that is no multiple of k included.
template <typename R, typename F>
R with_nq(uint32_t n, uint32_t k, R fallback, F&& f) {
  if (k == 0 || n % k != 0) return fallback;
  return with_k(NqList{}, n / k, fallback, f);
}

// The grid of a launch over `batch` entries of `count` columns (payload chunks
// or shard symbols) in tiles of `width` columns.
enum GridState { kGridEmpty, kGridInvalid, kGridOk };  // nothing to do; out of range; launch
struct TileGrid {
  GridState state;
  uint32_t count;   // columns of an entry (<= 2^32 - 1)
  uint32_t tiles;   // tiles of an entry
  uint32_t per;     // tiles per workgroup
  uint32_t blocks;  // workgroups of the launch (<= 2^31 - 1)
};

// Sizes the entries: false when there is nothing to launch (g.state says why).
inline bool grid_tiles(TileGrid& g, size_t count, uint32_t width, size_t batch) {
  g = TileGrid{kGridEmpty, 0, 0, 0, 0};
  if (count == 0 || batch == 0) return false;
  g.state = kGridInvalid;
  if (count > 0xffffffffu) return false;
  g.count = static_cast<uint32_t>(count);
  g.tiles = static_cast<uint32_t>((count + width - 1) / width);
  return true;
}
inline TileGrid grid_blocks(TileGrid g, size_t blocks) {
  if (blocks > 0x7fffffffu) return g;
  g.blocks = static_cast<uint32_t>(blocks);
  g.state = kGridOk;
  return g;
}

// Workgroups of tpw(tiles) consecutive tiles of one entry.
template <typename TPW>
TileGrid tile_grid(size_t count, uint32_t width, size_t batch, TPW tpw) {
  TileGrid g;
  if (!grid_tiles(g, count, width, batch)) return g;
  g.per = tpw(g.tiles);
  return grid_blocks(g, batch * ((g.tiles + g.per - 1) / g.per));
}
// One tile per workgroup.
inline TileGrid tile_grid(size_t count, uint32_t width, size_t batch) {
  return tile_grid(count, width, batch, [](uint32_t) { return 1u; });
}
// Workgroups of `per` tiles numbered across the entries (tile t of entry b is
// number b * tiles + t, a 32-bit value: batch * tiles <= 2^32 - 1).
inline TileGrid tile_grid_packed(size_t count, uint32_t width, size_t batch, uint32_t per) {
  TileGrid g;
  if (!grid_tiles(g, count, width, batch)) return g;
  g.per = per;
  if (batch * g.tiles > 0xffffffffu) return g;
  return grid_blocks(g, (batch * g.tiles + per - 1) / per);
}

}  // namespace np
