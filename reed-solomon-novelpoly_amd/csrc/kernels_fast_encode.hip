// Specialised gfx950 kernels for the hot shapes: k = K in {64, 128, 256},
// encode for n >= 2K, reconstruct for n in {2K, 4K} (every BASELINE shape
// with k <= 256).
//
// Work mapping.  A workgroup owns a tile of 256 codeword columns (encode: 256
// payload chunks; reconstruct: 256 symbol columns of the shards).  A
// size-K transform (K = 2^logK positions) is split in two register layouts
// that meet in a 256 x K LDS tile:
//
//  * "column-quad" (cq) layout -- levels 0..3.  Wave g owns positions
//    16g..16g+15, lane l owns columns 4l..4l+3; register CL[p] / CH[p] hold
//    the low / high bytes of position 16g+p of those four columns.  Shard rows
//    are position-major, so this layout is also the one that reads and writes
//    shard rows with coalesced 8-byte accesses.
//  * "high" layout -- levels 4..logK-1.  R = K/64 adjacent lanes share a
//    column; lane (c, r) holds the 16 position-quads m = R*j + r (j = 0..15)
//    as byte-planar pairs (L[j], H[j]).  Butterflies of these levels pair
//    quads j and j + 2^(b-2-logR) of one lane.
//
// In both layouts every butterfly group is the same for all lanes of a wave,
// so each GF(2^16) multiplier is wave-uniform: c*y is the XOR of 12 v_perm
// byte-table lookups whose 20 table dwords are fetched with s_load
// (field_tables.cpp builds them).  Each lane keeps 32 state dwords, so a
// 4K-thread workgroup fits 4 waves per SIMD.
//
// Reference: additive FFT inc_afft.rs:139-214 (inverse) / :267-332 (forward);
// encode inc_encode.rs:15-48 + mod.rs:117-157; reconstruct inc_reconstruct.rs:1-85
// + mod.rs:162-239.  The skew of group t at level b and transform index I is
// the field element with Cantor coordinates 2t + (I >> b)
// (tests/test_oracle.py::test_skews_are_cantor_points).
//
// This file: the encodes (k_encode_fast, k_encode_multi, k_encode_ragged).
// The planned encodes (restore, verify, recover): kernels_fast_planned.hip;
// the decodes: kernels_fast_decode.hip; their per-payload records:
// kernels_fast_records.hip.
#include "fast_encode.hpp"
// (The next tile's payload is read once: its LDS-DMA loads stream (nt),
// keeping L2 for the tables and the row stores; config 3 encode -4 %.)

namespace np {
namespace {

// One workgroup: 256 chunks of one payload, every row below wanted_n.
// mod.rs:144-154 / inc_encode.rs:15-48.
template <int K>
__device__ __forceinline__ void encode_all(const DevTables& T, uint8_t* smem, uint32_t n, uint32_t wanted_n,
                                           const EncTile& t) {
  using G = Geo<K>;
  uint8_t* tile = smem;
  uint32_t* VP = reinterpret_cast<uint32_t*>(smem + G::kTileBytes);  // 2 staged transforms
  const uint32_t tid = threadIdx.x, lane = tid & 63u, g = uniform(tid >> 6);
  load_tile<K>(tile, t, tid);
  const uint32_t nshift = n / K;
  const uint32_t wanted_store = ((kExp & 2) && n != 12345u) ? 0u : wanted_n;  // experiment: no stores
  // n <= 4K: the tables of every transform stay staged (one buffer each, as
  // k_encode_multi: no table load inside the shift loop, where it would wait
  // for the row stores issued before it); otherwise two buffers alternate
  const bool resident = nshift <= 4;
  if (resident) {
    for (uint32_t sh = 0; sh < nshift && sh * K < wanted_n; ++sh)
      stage_vpools<K, G::kThreads>(T, sh * K, VP + sh * G::kVPWords, true, enc_conv(K, sh));
  } else {
    stage_vpools<K, G::kThreads>(T, 0, VP, true);                                   // inverse transform, index 0
    if (nshift > 1) stage_vpools<K, G::kThreads>(T, K, VP + G::kVPWords, true, enc_conv(K, 1));  // first shift
  }
  __syncthreads();

  const uint32_t cqb = col_base<K>(4 * lane) ^ (32u * g);  // blocks 4g..4g+3 of columns 4l..4l+3
  // ---- cq pass: systematic rows, inverse levels 0..3
  {
    uint32_t CL[16], CH[16];
    cq_read<K>(tile, cqb, CL, CH);
    store_rows(t.out, t.shard_len, 16 * g, wanted_store, CL, CH, lane, t.ncols, t.full, t.nt);
    tower_convert(T, CL, CH);  // transforms run in tower coordinates
    cq_levels<K, true, true, 0, false, kEncPrioCq>(T, VP, 0, g, CL, CH);
    // the quad items overlay payload blocks that other waves read: wait for
    // every wave's cq_read
    __syncthreads();
    cq_write_q(tile, g, lane, CL, CH);
  }
  __syncthreads();
  // ---- high layout: inverse levels 4.. -> coefficients M
  uint32_t ML[16], MH[16];
  hi_read_q<K>(tile, g, lane, ML, MH);
  hi_levels<K, true, true, 0, 0, kEncPrio>(T, VP, 0, ML, MH);
#pragma unroll
  for (int q = 0; q < 16; ++q) asm volatile("" : "+v"(ML[q]), "+v"(MH[q]));  // materialise M once

  uint32_t PL[8], PH[8];  // top-level products of shift 1, then of shifts 1 ^ 2 (fwd_top)
  auto shift = [&](auto shc, uint32_t sh) __attribute__((always_inline)) {
    constexpr int SH = decltype(shc)::value;
    const uint32_t index = sh * K;
    uint32_t XL[16], XH[16];
    const uint32_t* vp = VP + (resident ? sh : (sh & 1u)) * G::kVPWords;
    shift_hi<K, SH>(T, vp, index, ML, MH, XL, XH, PL, PH);
    __syncthreads();  // the previous cq pass is done with the tile and with the other table buffer
    if (!resident && sh + 1 < nshift && (sh + 1) * K < wanted_n)
      stage_vpools<K, G::kThreads>(T, (sh + 1) * K, VP + ((sh + 1) & 1u) * G::kVPWords, sh + 1 < 4,
                                   enc_conv(K, sh + 1));
    hi_write_q<K>(tile, g, lane, XL, XH);
    __syncthreads();
    cq_read_q(tile, g, lane, XL, XH);
    shift_cq<K, SH>(T, vp, index, g, XL, XH);
    store_rows(t.out, t.shard_len, index + 16 * g, wanted_store, XL, XH, lane, t.ncols, t.full, t.nt);
  };
  if (nshift > 1 && K < wanted_n) shift(Int<1>{}, 1);
  if (nshift > 2 && 2 * K < wanted_n) shift(Int<2>{}, 2);
  if (nshift > 3 && 3 * K < wanted_n) shift(Int<3>{}, 3);
#pragma unroll 1
  for (uint32_t sh = 4; sh < nshift && sh * K < wanted_n; ++sh) shift(Int<0>{}, sh);
}

template <int K>
__global__ __launch_bounds__(4 * K) __attribute__((amdgpu_waves_per_eu(4))) void k_encode_fast(DevTables T, EncodeArgs a, uint32_t nchunks, uint32_t tiles) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
#if NP_BOUNDS_CHECK
  bounds_arm(bounds_of_enc(a));
#endif
  encode_all<K>(T, smem, a.n, a.wanted_n, enc_tile(a, nchunks, tile_of(blockIdx.x, tiles, (a.batch & 7u) == 0)));
}

// ----------------------------------------------------- multi-tile encode ----
// k = 256: a workgroup encodes `tpw` consecutive tiles of one payload, and the
// payload blocks of the next tile flow into the LDS tile by LDS-DMA while the
// last shift's cq levels and row stores of this tile run (the tile is free
// once every wave has read it back for that last cq pass).  The launch record
// is re-read from the kernarg segment at every tile, so that none of it stays
// live in registers across the tile loop.

// Table buffers of the multi-tile encode: the inverse transform's and one per
// shift, staged once per workgroup (n <= 4K); with the 128 KiB tile they fill
// the 160 KiB of LDS.  Table loads inside the tile loop would wait (vmcnt
// counts in order) for the row stores issued before them.
constexpr int kEncBuffers = 4;

struct EncLaunch {
  DevTables T;
  EncodeArgs a;
  uint32_t nchunks, tiles, tpw;
};
typedef const __attribute__((address_space(4))) EncLaunch* enc_launch_ptr;

// The next tile's payload by 16-byte LDS-DMA pieces (8 per wave instead of 32
// of 4 bytes), which needs the payload tile's swizzle at 16-byte granularity
// (col_base EVEN; the tile's cq reads then conflict 2-way).  From the stamps
// (profiles/r04_encode_stamps_hiw.txt): 32 pieces per wave overfill the wave's
// memory queue and the DMA's issue stalls.  Measured: encode 1.625 / 1.630 /
// 1.625 -> 1.598 / 1.603 / 1.596 ms (-1.7 %, profiles/r04_ab.txt probe 15).
// The pieces' addresses are a scalar base plus a 32-bit lane offset (1 VALU per
// piece instead of 7 for 64-bit per-lane addresses; -0.5 %, probe 17).  Issuing
// all pieces from 4 waves after a barrier measured -0.8 % on top, neutral with
// the issue priority (probe 18).
template <int K>
constexpr bool kEncDmaX4 = K == 256;

// kEncDmaX4: wave w's columns 16w..16w+15 in 8 pieces of two columns (lanes
// 0-31 the first, 32-63 the second, 16 bytes each): lane l of a piece writes
// LDS blocks 2(l & 31), 2(l & 31) + 1 of its column, which hold the payload's
// contiguous blocks 2(l & 31) ^ sw, (2(l & 31) ^ sw) + 1 (sw even).
template <int K>
__device__ __forceinline__ void dma_tile_x4(const uint8_t* pay, uint32_t ch0, uint8_t* tile, uint32_t w, uint32_t lane) {
  static_assert(K == 256, "two 512-byte columns per 1 KiB piece");
  constexpr uint32_t kColBytes = 2 * K;
  const uint32_t lds0 = static_cast<uint32_t>(
      reinterpret_cast<uintptr_t>((__attribute__((address_space(3))) uint8_t*)(tile)));
  const uint32_t half = lane >> 5, li = lane & 31u;
  const uint32_t swh = half ? (swz<K>(1) & ~1u) : 0u;  // the odd column's part of the (linear) swizzle
  // scalar base per piece (column 16w + 2j), 32-bit lane offset: the swizzle
  // is linear, so piece j's offset is the lane's piece-0 offset XOR a constant
  const uint32_t off0 = 512u * half + 8u * ((2u * li) ^ (swz<K>(16u * w) & ~1u) ^ swh);
  const uint8_t* base = pay + static_cast<size_t>(ch0 + 16u * w) * kColBytes;
#pragma unroll
  for (uint32_t j = 0; j < 8; ++j) {
    const uint32_t off = off0 ^ (8u * (swz<K>(2u * j) & ~1u));
    const uint8_t* sb = base + 2u * j * kColBytes;
    NP_BNOTE(sb + off, 16, kBkPayloads);
    const uint32_t dst = uniform(lds0 + (16u * w + 2u * j) * kColBytes);
    uint32_t keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2 nt\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(off), "s"(sb), "s"(dst)
                 : "memory");
  }
}

// One shift of the encode (rows sK .. sK+K-1), SH = 1..3.  With `dma_pay`,
// the last cq pass starts the next tile's payload DMA once every wave has read
// the tile.
template <int K, int SH>
__device__ __forceinline__ void encode_shift(const DevTables& T, const EncodeArgs& a, uint8_t* tile, uint32_t* VP,
                                             uint8_t* out, uint32_t sh, uint32_t g, uint32_t lane, uint32_t ncols,
                                             bool full, const uint32_t (&ML)[16],
                                             const uint32_t (&MH)[16], uint32_t (&PL)[8], uint32_t (&PH)[8],
                                             const uint8_t* dma_pay, uint32_t dma_ch0, uint64_t* dbg) {
  using G = Geo<K>;
  const uint32_t index = sh * K;
  uint32_t XL[16], XH[16];
  const uint32_t* vp = VP + sh * G::kVPWords;  // the tables of every shift stay staged (kEncBuffers)
  constexpr int st0 = 7 + 4 * (SH - 1);  // stamp slots of this shift
  {
    // the quads of each level-4 group go to LDS as soon as they are final,
    // among the level's VALU work; the barrier that frees the tile (every
    // wave's previous cq read) moves before level 4
    uint8_t* hb0 = tile + 512u * (256u / K) * g + fresh_v(8u * lane);
    struct Hook {
      uint8_t* b;
      uint32_t (&L)[16];
      uint32_t (&H)[16];
      __device__ __forceinline__ void pre() const { __syncthreads(); }
      __device__ __forceinline__ void post(int t) const {
        *reinterpret_cast<uint2*>(b + hi_q_off<K>(2 * t)) = make_uint2(L[2 * t], H[2 * t]);
        *reinterpret_cast<uint2*>(b + hi_q_off<K>(2 * t + 1)) = make_uint2(L[2 * t + 1], H[2 * t + 1]);
      }
    };
    shift_hi<K, SH>(T, vp, index, ML, MH, XL, XH, PL, PH, Hook{hb0, XL, XH});
    stamp(dbg, st0);
    __syncthreads();
    cq_read_q(tile, g, lane, XL, XH);
  }
  if (dma_pay) {
    // No workgroup barrier: wave g's quad items and its share of the next
    // payload tile are the same 8 KiB (cq_read_q, dma_tile_x4), so once its
    // own reads are back no other wave touches that region.  Measured: encode
    // 1.646 / 1.648 -> 1.638 / 1.638 ms (-0.6 %, profiles/r04_ab.txt probe 13).
    // Spreading the DMA pieces over the last cq pass measured +0.3 to +0.7 %.
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if constexpr (!(kExp & 4)) dma_tile_x4<K>(dma_pay, dma_ch0, tile, g, lane);
  }
  stamp(dbg, st0 + 1);
  const uint32_t row0 = index + 16 * g;
  const uint32_t wanted = (kExp & 2) ? 0u : a.wanted_n;
  const bool nt = rows_nt(a.shards, a.batch_stride, a.shard_len);
  shift_cq<K, SH>(T, vp, index, g, XL, XH);
  stamp(dbg, st0 + 2);
  store_rows(out, a.shard_len, row0, wanted, XL, XH, lane, ncols, full, nt);
  stamp(dbg, st0 + 3);
}

// One tile; returns whether the next tile's payload is on its way by DMA.
template <int K>
__device__ __forceinline__ bool encode_tile_multi(const DevTables& T, const EncodeArgs& a, uint8_t* smem, uint32_t pb,
                                                  uint32_t tl, uint32_t nchunks, bool first, bool have_dma,
                                                  bool stored16, uint32_t next_tl) {
  using G = Geo<K>;
  uint8_t* tile = smem;
  uint32_t* VP = reinterpret_cast<uint32_t*>(smem + G::kTileBytes);  // 2 staged transforms
  const uint32_t ch0 = tl * kTile;
  const uint32_t ncols = min(static_cast<uint32_t>(kTile), nchunks - ch0);
  const uint8_t* pay = a.payloads + static_cast<size_t>(pb) * a.payload_stride;
  uint8_t* out = a.shards + static_cast<size_t>(pb) * a.batch_stride + 2 * static_cast<size_t>(ch0);
  // opaque per tile: otherwise the lane-derived addresses of the loads, DMA and
  // row guards are hoisted out of the tile loop and spilled, and each reload
  // (a VMEM op) waits with vmcnt(0) for the DMA and every row store before it
  const uint32_t tid = fresh_v(threadIdx.x), lane = tid & 63u, g = uniform(tid >> 6);
  const bool full =
      ncols == kTile && rows_vec_ok(a.shards, a.batch_stride, a.shard_len);
  // experiment builds (NP_EXP bit 6): s_memtime stamps past the payload's shard
  // rows (tools/enc_stamps.py allocates batch_stride = n shard_len + 4 KiB per tile)
  uint64_t* dbg = (kExp & 64) ? reinterpret_cast<uint64_t*>(a.shards + static_cast<size_t>(pb) * a.batch_stride +
                                                             static_cast<size_t>(a.n) * a.shard_len + 4096u * tl)
                              : nullptr;
  stamp(dbg, 0);
  // whole tiles load by 8-byte vector loads at any address; the LDS-DMA of the
  // next tile's payload (4-byte pieces) only from 8-byte aligned payloads
  const bool aligned_pay = (reinterpret_cast<uintptr_t>(pay) & (kEncDmaX4<K> ? 15u : 7u)) == 0;
  auto tile_whole = [&](uint32_t t) __attribute__((always_inline)) {
    return static_cast<size_t>(t * kTile + kTile) * 2 * K <= a.payload_len;
  };
  auto tile_fast = [&](uint32_t t) __attribute__((always_inline)) { return aligned_pay && tile_whole(t); };
  if (have_dma) {
    // this wave's DMA pieces have landed; the previous tile's last 16 row
    // stores, issued after them, may still be in flight
    if (stored16)
      asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
    else
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  } else {
    const uint32_t c0 = tid / G::Q, m0 = tid % G::Q;
    const uint32_t base = col_base<K, kEncDmaX4<K>>(c0) ^ (8u * m0);
    const size_t gbase = static_cast<size_t>(ch0 + c0) * 2 * K + 8u * m0;
    if (out_vec_ok(pay, 0) && tile_whole(tl)) {
      uint2 v[16];
#pragma unroll
      for (int i = 0; i < 16; ++i)
        v[i] = (kExp & 4) ? make_uint2(i, tid) : load_once(pay + gbase + static_cast<size_t>(i) * 32 * K);
#pragma unroll
      for (int i = 0; i < 16; ++i) *reinterpret_cast<uint2*>(tile + (base ^ col_base_c<K, kEncDmaX4<K>>(16u * i))) = v[i];
    } else {
#pragma unroll 1
      for (uint32_t i = 0; i < 16; ++i) {
        const size_t g0 = gbase + static_cast<size_t>(i) * 32 * K;
        uint32_t w[2] = {0, 0};
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (g0 + e < a.payload_len) w[e >> 2] |= static_cast<uint32_t>(*NP_BCHK(pay + (g0 + e), 1, kBkPayloads)) << (8 * (e & 3));
        *reinterpret_cast<uint2*>(tile + (base ^ col_base_c<K, kEncDmaX4<K>>(16u * i))) = make_uint2(w[0], w[1]);
      }
    }
  }
  const uint32_t nshift = a.n / K;
  const uint32_t last = min(nshift, (a.wanted_n + K - 1) / K) - 1;  // last shift with wanted rows
  if (first) {  // tables of the inverse transform (index 0) and of every shift, kept for all tiles
    for (uint32_t sh = 0; sh <= last; ++sh)
      stage_vpools<K, G::kThreads>(T, sh * K, VP + sh * G::kVPWords, true, enc_conv(K, sh));
  }
  __syncthreads();
  stamp(dbg, 1);

  const uint32_t cqb = col_base<K, kEncDmaX4<K>>(4 * lane) ^ (32u * g);  // the payload tile's swizzle
  {
    uint32_t CL[16], CH[16];
    cq_read<K, kEncDmaX4<K>>(tile, cqb, CL, CH);
    store_rows(out, a.shard_len, 16 * g, (kExp & 2) ? 0u : a.wanted_n, CL, CH, lane, ncols, full,
               rows_nt(a.shards, a.batch_stride, a.shard_len));
    stamp(dbg, 2);
    tower_convert(T, CL, CH);  // transforms run in tower coordinates
    cq_levels<K, true, true, 0, false, kEncPrioCq>(T, VP, 0, g, CL, CH);
    stamp(dbg, 3);
    // the quad items overlay payload blocks that other waves read: wait for
    // every wave's cq_read
    __syncthreads();
    cq_write_q(tile, g, lane, CL, CH);
  }
  stamp(dbg, 4);
  __syncthreads();
  uint32_t ML[16], MH[16];
  hi_read_q<K>(tile, g, lane, ML, MH);
  stamp(dbg, 5);
  hi_levels<K, true, true, 0, 0, kEncPrio>(T, VP, 0, ML, MH);
#pragma unroll
  for (int q = 0; q < 16; ++q) asm volatile("" : "+v"(ML[q]), "+v"(MH[q]));  // materialise M once
  stamp(dbg, 6);
  uint32_t PL[8], PH[8];
  const bool dma = last >= 1 && next_tl != ~0u && tile_fast(next_tl);
  const uint8_t* dpay = dma ? pay : nullptr;
  const uint32_t dch0 = next_tl * kTile;
  if (last >= 1)
    encode_shift<K, 1>(T, a, tile, VP, out, 1, g, lane, ncols, full, ML, MH, PL, PH,
                       last == 1 ? dpay : nullptr, dch0, dbg);
  if (last >= 2)
    encode_shift<K, 2>(T, a, tile, VP, out, 2, g, lane, ncols, full, ML, MH, PL, PH,
                       last == 2 ? dpay : nullptr, dch0, dbg);
  if (last >= 3)
    encode_shift<K, 3>(T, a, tile, VP, out, 3, g, lane, ncols, full, ML, MH, PL, PH, dpay, dch0, dbg);
  return dma;
}

template <int K>
__global__ __launch_bounds__(4 * K) __attribute__((amdgpu_waves_per_eu(4))) void k_encode_multi(EncLaunch L) {
#if defined(__HIP_DEVICE_COMPILE__)  // (the host pass cannot bind the kernarg-segment record to references)
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
#if NP_BOUNDS_CHECK
  bounds_arm(bounds_of_enc(L.a));
#endif
  const uint32_t groups = (L.tiles + L.tpw - 1) / L.tpw;  // workgroups per batch entry
  const TileRef tr = tile_of(blockIdx.x, groups, (L.a.batch & 7u) == 0);
  const uint32_t pb = tr.pb, tl0 = tr.tl * L.tpw;
  const uint32_t ntl = min(L.tpw, L.tiles - tl0);
  const uint64_t kp = reinterpret_cast<uint64_t>(__builtin_amdgcn_kernarg_segment_ptr());
  bool dma = false;
#pragma unroll 1
  for (uint32_t t = 0; t < ntl; ++t) {
    if (t > 0) __syncthreads();  // the previous tile's last cq pass is done with the tables
    const enc_launch_ptr lp = reinterpret_cast<enc_launch_ptr>(fresh(kp));
    const DevTables T = lp->T;
    const EncodeArgs a = lp->a;
    // the previous tile's last shift stored 16 rows per wave (store_rows' full path)
    const uint32_t pch0 = (tl0 + t - 1) * kTile;
    const bool stored16 = t > 0 && pch0 + kTile <= lp->nchunks &&
                          rows_vec_ok(a.shards, a.batch_stride, a.shard_len) &&
                          (min(a.n / K, (a.wanted_n + K - 1) / K) - 1) * K + 16 * 16 <= a.wanted_n &&
                          16 * a.shard_len < 0x7fffffffu;
    dma = encode_tile_multi<K>(T, a, smem, fresh(pb), fresh(tl0) + t, lp->nchunks, t == 0, dma, stored16,
                               t + 1 < ntl ? tl0 + t + 1 : ~0u);
  }
#endif
}

// One workgroup: 256 chunks of one item (k_encode_fast's flow).
template <int K>
__global__ __launch_bounds__(4 * K) __attribute__((amdgpu_waves_per_eu(4))) void k_encode_ragged(DevTables T, RaggedArgs r) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
#if NP_BOUNDS_CHECK
  bounds_arm(bounds_of_ragged(r, T, false));
#endif
  const RaggedHead h = ragged_head(r);
  if (h.item == kRaggedNoItem) return;  // padding of the plan
  encode_all<K>(T, smem, r.n, r.wanted_n, enc_tile(h));
}

// ------------------------------------------------------------- launchers ----
template <int K>
size_t encode_multi_lds_bytes() {
  return static_cast<size_t>(Geo<K>::kTileBytes) + kEncBuffers * 4u * Geo<K>::kVPWords;
}

template <int K>
hipError_t launch_encode_k(const DevTables& T, const EncodeArgs& a, hipStream_t s) {
  const bool multi = kMultiTile<K> && a.n <= kEncBuffers * K;
  return with_encode_grid(
      a, [&](uint32_t tiles) { return multi ? tiles_per_workgroup<K>(a.batch, tiles, "NP_ENC_TPW") : 1u; },
      [&](const TileGrid& g) {
        if constexpr (kMultiTile<K>) {
          if (multi) {
            k_encode_multi<K><<<g.blocks, Geo<K>::kThreads, encode_multi_lds_bytes<K>(), s>>>(
                EncLaunch{T, a, g.count, g.tiles, g.per});
            return;
          }
        }
        k_encode_fast<K><<<g.blocks, Geo<K>::kThreads, encode_lds_bytes<K>(), s>>>(T, a, g.count, g.tiles);
      });
}

}  // namespace

bool fast_encode_supported(uint32_t n, uint32_t k) {
  return (fast_k(k) && n >= 2 * k && n <= 65536) || small_encode_supported(n, k);
}

hipError_t launch_encode_fast(const DevTables& T, const EncodeArgs& a, hipStream_t s) {
  if (!fast_k(a.k)) return launch_encode_small(T, a, s);  // k <= 32; hipErrorNotSupported for any other k
  return with_k(FastKs{}, a.k, hipErrorNotSupported, [&](auto kc) { return launch_encode_k<kc.value>(T, a, s); });
}

bool ragged_encode_supported(uint32_t n, uint32_t k) { return fast_k(k) && n >= 2 * k && n <= 65536; }

hipError_t launch_encode_ragged(const DevTables& T, const RaggedArgs& r, hipStream_t s) {
  return with_ragged_k(r, [&](auto kc) {
    constexpr int K = kc.value;
    k_encode_ragged<K><<<r.nblocks, Geo<K>::kThreads, encode_lds_bytes<K>(), s>>>(T, r);
    return hipGetLastError();
  });
}

hipError_t configure_fast_encode_kernels() {
  LdsSetup lds;
  each_k(FastKs{}, [&](auto kc) {
    constexpr int K = kc.value;
    lds(&k_encode_fast<K>, encode_lds_bytes<K>());
    if constexpr (kMultiTile<K>) lds(&k_encode_multi<K>, encode_multi_lds_bytes<K>());
    lds(&k_encode_ragged<K>, encode_lds_bytes<K>());
  });
  return lds.err;
}

hipError_t bounds_take_fast_encode(uint32_t out[8]) { return bounds_take_tu(out); }

}  // namespace np
