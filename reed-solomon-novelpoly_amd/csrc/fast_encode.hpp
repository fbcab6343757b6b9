// Device code the encode units of the fast family share
// (kernels_fast_encode.hip, kernels_fast_planned.hip): the shift primitives,
// the tile of a single-tile encode workgroup with its loader, and the grid of
// an encode launch.  See kernels_fast_encode.hip for the design.
#pragma once
#include "fast_family.hpp"

namespace np {
namespace {

// ----------------------------------------------------------------- encode ----
// Encode shifts run in tower coordinates while gen_of(index) <= kEncMaxGen
// (index < 2048: n <= 8K at k = 256, every n the crate derives), their levels
// below gen_of(index) with the full map; farther shifts of larger explicit
// codes run in Cantor coordinates.
constexpr int kEncMaxGen = 3;
__device__ __forceinline__ bool enc_tower(uint32_t index) {
  return __builtin_amdgcn_readfirstlane(gen_of(index)) <= static_cast<uint32_t>(kEncMaxGen);
}

// Shifts 1..3 are compile-time (SH): tower coordinates, the top-level products
// shared between them (fwd_top), their cq levels below gen_of(SH * K) with the
// full map.  SH = 23: shift 2 or 3 (runtime sh; both have gen_of = 2 at
// K = 256).  SH = 0: a shift >= 4 (n > 4K) in Cantor coordinates.  A runtime
// choice between instances inside a pass makes the register allocator spill,
// so each call site is one instance.
template <int K, int SH>
constexpr int kShiftGen = static_cast<int>(gen_of((SH == 23 ? 2 : SH) * K));

// X = M, then the forward high levels of shift sh (top level included).
template <int K, int SH, typename HOOK = NoHiHook>
__device__ __forceinline__ void shift_hi(const DevTables& T, const uint32_t* vp, uint32_t index,
                                         const uint32_t (&ML)[16], const uint32_t (&MH)[16], uint32_t (&XL)[16],
                                         uint32_t (&XH)[16], uint32_t (&PL)[8], uint32_t (&PH)[8], HOOK hook = HOOK{}) {
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    XL[q] = ML[q];
    XH[q] = MH[q];
  }
  if constexpr (SH == 0) {
    tower_convert(T, XL, XH);  // M is in tower coordinates
    fwd_top<K, 0, -1>(T, vp, index, XL, XH, PL, PH);
    hi_levels<K, false, false, 1, -1, kEncPrio>(T, vp, index, XL, XH);
  } else {
    if constexpr (SH == 23) {
      if (index == 2 * K)
        fwd_top<K, 2, 0>(T, vp, index, XL, XH, PL, PH);
      else
        fwd_top<K, 3, 0>(T, vp, index, XL, XH, PL, PH);
    } else {
      fwd_top<K, SH, 0>(T, vp, index, XL, XH, PL, PH);
    }
    hi_levels<K, false, false, 1, 0, kEncPrio>(T, vp, index, XL, XH, hook);  // hi levels: gen_of(index) <= 4
  }
}

// Shifts whose level 0 multiplies by full elements (gen_of(sK) >= 1: every
// shift at k = 256) leave the tower inside that level (cq_levels CONV,
// qbfly_fwd_conv) instead of converting the 16 rows after it.  Measured:
// config-3 encode 1.656 / 1.663 -> 1.629 / 1.631 ms (-1.8 %, profiles/r04_ab.txt).
// Whether shift sh of a size-K encode fuses its conversion; the staging of its
// tables must agree (stage_vpools l0_out).  SH = 23 stands for shifts 2 and 3.
__host__ __device__ constexpr bool enc_conv(int K, uint32_t sh) {
  return sh >= 1 && sh <= 3 && gen_of(sh * static_cast<uint32_t>(K)) >= 1;
}
template <int K, int SH>
constexpr bool kEncConv = SH != 0 && enc_conv(K, SH == 23 ? 2u : static_cast<uint32_t>(SH));

// The forward cq levels of shift sh, ending in Cantor coordinates.
template <int K, int SH, typename POST = NoPost>
__device__ __forceinline__ void shift_cq(const DevTables& T, const uint32_t* vp, uint32_t index, uint32_t g,
                                         uint32_t (&XL)[16], uint32_t (&XH)[16], POST post = POST{}) {
  if constexpr (SH == 0) {
    cq_levels<K, false, false, -1, false, kEncPrioCq>(T, vp, index, g, XL, XH, ~0u, post);
  } else {
    static_assert(SH != 23 || kShiftGen<K, 2> == kShiftGen<K, 3>, "shifts 2 and 3 share one instance");
    static_assert(SH != 23 || enc_conv(K, 2) == enc_conv(K, 3), "shifts 2 and 3 share one instance");
    cq_levels<K, false, false, kShiftGen<K, SH>, kEncConv<K, SH>, kEncPrioCq>(T, vp, index, g, XL, XH, ~0u, post);
    if constexpr (!kEncConv<K, SH>) tower_convert(T, XL, XH);  // back to Cantor coordinates for the shard rows
  }
}

// The fast encodes exchange layouts through quad items (cq_write_q ..
// hi_read_q, fast_common.hpp): no byte transposes.  The multi-tile encode
// writes each shift's high-layout quads to LDS right after their last
// (level-4) butterfly group instead of after the whole high pass: encode
// -1.9 % at config 3 (1.686 -> 1.655 ms, profiles/r04_ab.txt).

// The tile of a single-tile encode workgroup (workgroup-uniform).  The uniform
// kernels fill it from the launch record and tile_of, the ragged ones from the
// item's record (ragged_head); the flows below see nothing else of the caller.
struct EncTile {
  const uint8_t* pay;  // the payload and its length
  size_t payload_len;
  uint8_t* out;  // row 0 of the item at the tile's first column
  size_t shard_len;
  uint32_t ch0, ncols;  // first chunk, chunks of the tile
  bool full, nt;        // whole tile of 8-byte row pieces; streaming row stores
};

__device__ __forceinline__ EncTile enc_tile(const EncodeArgs& a, uint32_t nchunks, TileRef tr) {
  EncTile t;
  t.pay = a.payloads + static_cast<size_t>(tr.pb) * a.payload_stride;
  t.payload_len = a.payload_len;
  t.ch0 = tr.tl * kTile;
  t.ncols = min(static_cast<uint32_t>(kTile), nchunks - t.ch0);
  t.out = a.shards + static_cast<size_t>(tr.pb) * a.batch_stride + 2 * static_cast<size_t>(t.ch0);
  t.shard_len = a.shard_len;
  t.full = t.ncols == kTile && rows_vec_ok(a.shards, a.batch_stride, a.shard_len);
  t.nt = rows_nt(a.shards, a.batch_stride, a.shard_len);
  return t;
}

// Tile load: thread tid moves blocks (c0 + 16 i, m0), i = 0..15; a tile that
// reaches past the payload's end loads by bytes and pads with zeros.
template <int K>
__device__ __forceinline__ void load_tile(uint8_t* tile, const EncTile& t, uint32_t tid) {
  using G = Geo<K>;
  const uint32_t c0 = tid / G::Q, m0 = tid % G::Q;
  const uint32_t base = col_base<K>(c0) ^ (8u * m0);
  const size_t gbase = static_cast<size_t>(t.ch0 + c0) * 2 * K + 8u * m0;
  const bool fast = out_vec_ok(t.pay, 0) && static_cast<size_t>(t.ch0 + kTile) * 2 * K <= t.payload_len;
  if (fast) {
    uint2 v[16];
#pragma unroll
    for (int i = 0; i < 16; ++i)
      v[i] = (kExp & 4) ? make_uint2(i, tid) : load_once(t.pay + gbase + static_cast<size_t>(i) * 32 * K);
#pragma unroll
    for (int i = 0; i < 16; ++i) *reinterpret_cast<uint2*>(tile + (base ^ col_base_c<K>(16u * i))) = v[i];
  } else {
#pragma unroll 1
    for (uint32_t i = 0; i < 16; ++i) {
      const size_t g0 = gbase + static_cast<size_t>(i) * 32 * K;
      uint32_t w[2] = {0, 0};
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (g0 + e < t.payload_len) w[e >> 2] |= static_cast<uint32_t>(*NP_BCHK(t.pay + (g0 + e), 1, kBkPayloads)) << (8 * (e & 3));
      *reinterpret_cast<uint2*>(tile + (base ^ col_base_c<K>(16u * i))) = make_uint2(w[0], w[1]);
    }
  }
}

// The item's tile: what enc_tile derives per launch, per item.
__device__ __forceinline__ EncTile enc_tile(const RaggedHead& h) {
  EncTile t;
  t.pay = reinterpret_cast<const uint8_t*>(h.data);
  t.payload_len = h.data_len;
  t.shard_len = h.shard_len;
  uint8_t* const shards = reinterpret_cast<uint8_t*>(h.shards);
  const uint32_t nchunks = static_cast<uint32_t>(t.shard_len / 2);  // = ceil(payload_len / 2K), validated by the host
  t.ch0 = h.tile * kTile;
  t.ncols = min(static_cast<uint32_t>(kTile), nchunks - t.ch0);
  t.out = shards + 2 * static_cast<size_t>(t.ch0);
  t.full = t.ncols == kTile && rows_vec_ok(shards, 0, t.shard_len);
  t.nt = rows_nt(shards, 0, t.shard_len);
  return t;
}

template <int K>
size_t encode_lds_bytes() {
  return static_cast<size_t>(Geo<K>::kTileBytes) + 4u * 4u * Geo<K>::kVPWords;  // up to 4 resident tables
}

// The grid of an encode launch: the chunks of a payload, their 256-chunk tiles
// and the workgroups of tpw_of(tiles) tiles each, range-checked (tile_grid);
// launch(grid) starts the kernel.
template <typename TPW, typename F>
hipError_t with_encode_grid(const EncodeArgs& a, TPW tpw_of, F launch) {
  const TileGrid g = tile_grid(encode_chunks(a), kTile, a.batch, tpw_of);
  if (g.state != kGridOk) return grid_status(g);
  launch(g);
  return hipGetLastError();
}
// One tile per workgroup at every K (the masked and verify encodes: the
// multi-tile encode counts its outstanding row stores, which they do not issue).
uint32_t one_tile(uint32_t) { return 1u; }

}  // namespace
}  // namespace np
