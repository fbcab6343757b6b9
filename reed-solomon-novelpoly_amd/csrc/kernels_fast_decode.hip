// The decodes of the fast family: k_reconstruct_fast and its ragged form, from
// the per-payload records of kernels_fast_records.hip.  See
// kernels_fast_encode.hip for the work mapping and the register layouts.
#include "fast_family.hpp"

namespace np {
namespace {

// ------------------------------------------------------------ reconstruct ----
struct RecCtx {
  const DevTables& T;
  size_t shard_len;
  uint8_t* tile;
  const uint32_t* R;  // row table records of the payload (prefix record)
  const uint8_t* sh;
  uint32_t* VP;  // 2 staged transforms
  uint32_t g, lane, tid, ncols;
  bool full;
  uint32_t cqb, hb;
  uint64_t* dbg;  // experiment builds only (stamp)
  uint32_t occ;   // bit q: segment q holds a present row (k_prefix_locator, record byte 1)
};

// Segment q of the sweep at step `step` (segments 2, 3, 1, 0 for NQ = 4; 1, 0
// for NQ = 2; 7, 6, ..., 0 for NQ = 8).
template <int NQ>
__host__ __device__ constexpr int seg_of(int step) {
  return NQ == 8 ? 7 - step : NQ == 4 ? (step == 0 ? 2 : step == 1 ? 3 : 3 - step) : 1 - step;
}

// NQ = 8: the first K outputs of the size-8K decode need
//   d = D_K(x0) ^ sum_q kappa_q x_q,  x_q = IFFT(K, qK)(premultiplied segment q),
// the three top inverse levels of index 0 (skews 0, Cantor(2), Cantor(4),
// Cantor(6)) and the derivative's single-bit terms K, 2K, 4K folded into one
// coefficient per segment: kappa = (1, 1, 1+b1, b1, (1+b1)(1+b2), (1+b1) b2,
// b1 (1+b3), b1 b3) with b_i = Cantor(2i), in Cantor coordinates below (all in
// GF(16); tests/test_oracle.py::test_rec8_kappa re-derives them with the
// oracle).  One accumulator, one subfield multiply per segment and position.
__host__ __device__ constexpr uint32_t rec8_kappa(int q) {
  constexpr uint32_t k[8] = {1, 1, 3, 2, 12, 15, 10, 8};
  return k[q];
}

// Presence of rows row0..row0+15 as bits (wave-uniform): one byte load per
// lane and a ballot, so row sources can be chosen before the flags reach LDS.
__device__ __forceinline__ uint32_t row_mask16(const uint8_t* pres, uint32_t row0, uint32_t lane) {
  const bool p = lane < 16u && *NP_BCHK(pres + (row0 + lane), 1, kBkPresent) != 0;
  return static_cast<uint32_t>(__ballot(p));
}

// Row loads: streaming (nt) for rows read once -- the parity segments' rows
// and the merge's final read of the systematic rows -- and the default policy
// for segment 0's systematic rows, which the merge reads again, so that the
// parity rows do not push them (and the payload's row-table records, re-read
// by every tile) out of L2.  (Every load with the default policy measured
// +1.5 % on the decode, all-nt +0.5 % in round 1.)
// Issues the loads of the lane's pieces of rows row0..row0+15; the data is
// consumed later.  Full tiles: one buffer descriptor per row whose size is 0
// for an absent row, so that load returns zeros with no HBM traffic and no
// branch.  Partial tiles: absent rows read the zero page.
template <int CPOL>
__device__ __forceinline__ void issue_rows_c(uint2 (&raw)[16], const uint8_t* sh, size_t shard_len, uint32_t mask,
                                             uint32_t row0, const uint8_t* zeros, uint32_t lane, uint32_t ncols,
                                             bool full) {
  if (full) {
#pragma unroll
    for (int p = 0; p < 16; ++p) {
      if ((mask >> p) & 1u) NP_BNOTE(sh + static_cast<size_t>(row0 + p) * shard_len + 8u * lane, 8, kBkShards);
      const __amdgpu_buffer_rsrc_t r = buf_rsrc(sh + static_cast<size_t>(row0 + p) * shard_len, ((mask >> p) & 1u) ? 512u : 0u);
      const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(r, 8u * lane, 0, CPOL);
      raw[p] = make_uint2(v.x, v.y);
    }
  } else {
#pragma unroll
    for (int p = 0; p < 16; ++p) {
      const uint8_t* src = ((mask >> p) & 1u) ? sh + static_cast<size_t>(row0 + p) * shard_len : zeros;
      raw[p] = load4(src, lane, ncols, false);
    }
  }
}

// reread: the rows are read again later (segment 0 before the merge).
__device__ __forceinline__ void issue_rows(uint2 (&raw)[16], const uint8_t* sh, size_t shard_len, uint32_t mask,
                                           uint32_t row0, const uint8_t* zeros, uint32_t lane, uint32_t ncols,
                                           bool full, bool reread = false) {
  if (!reread)
    issue_rows_c<2>(raw, sh, shard_len, mask, row0, zeros, lane, ncols, full);
  else
    issue_rows_c<0>(raw, sh, shard_len, mask, row0, zeros, lane, ncols, full);
}

// Copy-out straight from the cq registers: lane l holds columns 4l..4l+3 at
// positions 16g..16g+15, i.e. bytes [32g, 32g + 32) of each of those four
// 2K-byte output columns (two 16-byte stores per column).  Full tiles with
// 16-byte aligned output only; saves the LDS round trip and its two barriers.
// (Streaming stores here cost +26 %: each wave writes a quarter of a line.)
// PAIR: lanes l and l + 32 first trade one 16-byte half per column
// (v_permlane32_swap: the upper lanes of its first operand against the lower
// lanes of its second), so that a store instruction has the pair writing the
// two halves of one column's 32 bytes: 32 lines touched per instruction
// instead of 64, for 16 swaps per wave and tile.  Config-3 decode -2 to -3 %
// (profiles/r07/decode_phases_ab.txt).  Not where the next tile's rows are
// live across the copy-out (kRowPrefetch): there it costs a spilled VGPR at
// K = 256.
template <int K, bool PAIR>
__device__ __forceinline__ void copy_out_cq(uint8_t* out_tile, uint32_t lane, uint32_t g, const uint32_t (&L)[16],
                                            const uint32_t (&H)[16]) {
  uint2 d[4][4];
#pragma unroll
  for (int u = 0; u < 4; ++u) cq_to_blks(&L[4 * u], &H[4 * u], d[u]);
  if constexpr (PAIR) {
    // afterwards d[0..1][i] hold bytes [0, 16) (in lane l) and [16, 32) (in
    // lane l + 32) of lane l's column i, d[2..3][i] those of lane l + 32's
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const auto x = __builtin_amdgcn_permlane32_swap(d[u][i].x, d[u + 2][i].x, false, false);
        const auto y = __builtin_amdgcn_permlane32_swap(d[u][i].y, d[u + 2][i].y, false, false);
        d[u][i] = make_uint2(x[0], y[0]);
        d[u + 2][i] = make_uint2(x[1], y[1]);
      }
    }
    // 32-bit lane offsets from the wave-uniform tile address (256 columns of
    // 2K bytes): one address register per half of the columns
    const uint32_t off = (lane & 31u) * (4u * 2 * K) + (lane >> 5) * 16u + 32u * g;
    uint8_t* lo = out_tile + off;
    uint8_t* up = out_tile + (off + 128u * 2 * K);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      *reinterpret_cast<uint4*>(NP_BCHK(lo + i * 2 * K, 16, kBkOut)) = make_uint4(d[0][i].x, d[0][i].y, d[1][i].x, d[1][i].y);
      *reinterpret_cast<uint4*>(NP_BCHK(up + i * 2 * K, 16, kBkOut)) = make_uint4(d[2][i].x, d[2][i].y, d[3][i].x, d[3][i].y);
    }
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      uint8_t* o = NP_BCHK(out_tile + static_cast<size_t>(4u * lane + i) * 2 * K + 32u * g, 32, kBkOut);
      *reinterpret_cast<uint4*>(o) = make_uint4(d[0][i].x, d[0][i].y, d[1][i].x, d[1][i].y);
      *reinterpret_cast<uint4*>(o + 16) = make_uint4(d[2][i].x, d[2][i].y, d[3][i].x, d[3][i].y);
    }
  }
}

// The merge's systematic rows (4- and 8-segment decodes) load before the
// forward transform's cq pass.  Measured: decode 0 to -2 % at config 3 (box to
// box), -4 % at n/k = 8, k = 64, against loading them at the merge; before the
// forward high pass instead: -0.9 %.

// Row loads run one step ahead of their use where the registers allow it
// (prefixes of up to 2 segments); the 4-segment decode, which keeps more
// state live, loads each step's rows where it uses them.
template <int NQ>
constexpr bool kRowPrefetch = NQ <= 2;

// The tables of all NQ segment transforms fit in LDS next to the tile (K = 256:
// 128 KiB + 4 x 8 KiB of the 160 KiB): staged once per workgroup and kept for
// all its tiles, instead of two buffers restaged per step.  Measured -1 % to
// +0.6 % at config 3 (noise), -1.2 % at config 2.  (An L2 prefetch of the next
// step's rows by LDS-DMA into a dummy LDS area measured +8 %: vector loads
// complete in order, so the wait for a step's last row also waited for the
// prefetch behind it.)
// Only where it keeps the workgroups per CU (4K threads each, four waves per
// SIMD): K = 64 / 128 with NQ = 8 would lose one of four / two (measured +24 %
// / +65 % decode time).
template <int K, int NQ>
constexpr bool kRecResident =
    NQ > 1 &&
    Geo<K>::kTileBytes + NQ * 4u * Geo<K>::kVPWords <= 160u * 1024u * Geo<K>::kThreads / 1024u;
// LDS buffer of segment q's tables at decode step `step`.
template <int K, int NQ>
__device__ __forceinline__ uint32_t vp_slot(int q, int step) {
  return kRecResident<K, NQ> ? static_cast<uint32_t>(q) : static_cast<uint32_t>(step & 1);
}

// Largest gen_of over the decode's segment transforms (index qK, q < NQ).
template <int K, int NQ>
constexpr int kRecMaxGen = static_cast<int>(gen_of(static_cast<uint32_t>((NQ - 1) * K)));

// Tables staged before the first step: every segment's (kRecResident, slot q)
// or those of steps 0 and 1 (slots 0 and 1).  Caller synchronises.
template <int K, int NQ>
__device__ __forceinline__ void stage_rec_tables(const DevTables& T, uint32_t* VP) {
  if constexpr (kRecResident<K, NQ>) {
#pragma unroll 1
    for (int q = 0; q < NQ; ++q)
      stage_vpools<K, Geo<K>::kThreads>(T, static_cast<uint32_t>(q) * K, VP + q * Geo<K>::kVPWords, true);
  } else {
    stage_vpools<K, Geo<K>::kThreads>(T, static_cast<uint32_t>(seg_of<NQ>(0)) * K, VP, true);
    stage_vpools<K, Geo<K>::kThreads>(T, static_cast<uint32_t>(seg_of<NQ>(1)) * K, VP + Geo<K>::kVPWords, true);
  }
}

// msk[step] (16-bit row masks, wave-uniform) through shifts of packed scalars:
// a select chain over msk[] becomes a dynamically indexed private array, i.e.
// a scratch load whose vmcnt(0) wait also waits for every row load and store
// issued before it.
template <int NQ>
__device__ __forceinline__ uint32_t seg_mask(const uint32_t (&msk)[NQ], int step) {
  if constexpr (NQ <= 2) return step == 0 ? msk[0] : msk[NQ - 1];  // one select (the packed form spills here)
  uint64_t lo = 0, hi = 0;
#pragma unroll
  for (int i = 0; i < NQ; ++i) {
    const uint64_t v = static_cast<uint64_t>(msk[i] & 0xffffu);
    if (i < 4)
      lo |= v << (16 * i);
    else
      hi |= v << (16 * (i - 4));
  }
  const uint32_t sh = 16u * static_cast<uint32_t>(step & 3);
  return static_cast<uint32_t>(((step < 4 ? lo : hi) >> sh) & 0xffffu);
}

// The segment sweep: x_q = IFFT(K, qK)(premultiplied segment q), folded into
// A.  With kRowPrefetch `raw` holds segment seg_of(0)'s rows on entry and the
// systematic rows (for the merge) on exit.  A runtime loop keeps
// the kernel small; at index 0 the t = 0 multipliers are the zero element,
// whose table yields 0 (the reference's skipped multiply).
// Tile prefetch: the multi-tile decodes that load each step's rows
// where they use them (NQ >= 4) load the next tile's first-step rows during
// this tile's copy-out (and the first tile's before the tables are staged), as
// the 2-segment decode does: at the tile boundary only the rows and the output
// registers are live.  Measured (profiles/r04_ab.txt): config-3 decode
// 2.78 -> 2.73 ms (-1.6 %); the 8-segment decode (1200 validators) +0.5 %, so
// 4 segments only.
template <int K, int NQ>
constexpr bool kTilePrefetch = NQ == 4 && kMultiTile<K>;

// PRE0: step 0's rows are in `raw` on entry (kTilePrefetch).
template <int NQ>
constexpr bool kSkipEmpty = NQ == 8;

template <int K, int NQ, bool PRE0 = false>
__device__ __forceinline__ void rec_segments(const RecCtx& c, const uint32_t (&msk)[NQ], uint2 (&raw)[16],
                                             uint32_t (&AL)[16], uint32_t (&AH)[16], bool after_tile) {
  const DevTables& T = c.T;
  uint32_t XL[16], XH[16];
  // A (+)= the fold of x_q (XL / XH in the high layout) for segment q at `step`
  auto fold = [&](int step, int q) __attribute__((always_inline)) {
    if (NQ == 8 && q != 0) {  // A ^= kappa_q x_q (kRec8Kappa, all in GF(2^8))
      const uint32_t kq = uniform(rec8_kappa(q));
      if (kq == 1u) {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          AL[j] ^= XL[j];
          AH[j] ^= XH[j];
        }
      } else {
        uint32_t kp[20];
        pool_of<true>(T, kq, kp);
        const Mult pool = make_mult(kp);
        if (step == 0) {
#pragma unroll
          for (int j = 0; j < 16; ++j) qmul_sub_set(AL[j], AH[j], XL[j], XH[j], pool);
        } else {
#pragma unroll
          for (int j = 0; j < 16; ++j) qmul_sub(AL[j], AH[j], XL[j], XH[j], pool);
        }
      }
    } else if (step == 0) {
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        AL[j] = XL[j];
        AH[j] = XH[j];
      }
    } else if (q == 0) {
      if (NQ == 2 || NQ == 8) {  // kappa_0 = 1
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          AL[j] ^= XL[j];
          AH[j] ^= XH[j];
        }
      }
      add_derivative<K>(AL, XL, c.tid % Geo<K>::R);
      add_derivative<K>(AH, XH, c.tid % Geo<K>::R);
    } else if (NQ == 4 && q == 3) {
      uint32_t beta[20];
      pool_of<true>(T, 2u, beta);  // beta = Cantor(2) in GF(2^8), the t = 1 skew of level logK at index 0
      const Mult pool = make_mult(beta);
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        XL[j] ^= AL[j];
        XH[j] ^= AH[j];
        qmul_sub(AL[j], AH[j], XL[j], XH[j], pool);
      }
    } else {
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        AL[j] ^= XL[j];
        AH[j] ^= XH[j];
      }
    }
  };
#pragma unroll 1
  for (int step = 0; step < NQ; ++step) {
    const int q = seg_of<NQ>(step);
    // A segment without a present row contributes x_q = 0 (absent rows are
    // zeros): no loads, premultiply, transform or exchange, only the fold.
    // The 8-segment decodes only (n = 8k, e.g. 300, 700 and 1,200
    // validators: the segments above wanted_n are empty); the others are
    // compiled without the branch.  The next step's tables are still staged
    // here when they are not resident (in the other buffer, which the
    // previous step's high pass read).
    if (kSkipEmpty<NQ> && !((c.occ >> q) & 1u)) {
#pragma unroll
      for (int j = 0; j < 16; ++j) XL[j] = XH[j] = 0;
      if constexpr (!kRecResident<K, NQ>) {
        if (step > 0 && step + 1 < NQ) {
          __syncthreads();
          stage_vpools<K, Geo<K>::kThreads>(T, static_cast<uint32_t>(seg_of<NQ>(step + 1)) * K,
                                            c.VP + ((step + 1) & 1) * Geo<K>::kVPWords, true);
          __syncthreads();
        }
      }
    } else {
      const uint32_t index = uniform(static_cast<uint32_t>(q) * K);
      __builtin_amdgcn_sched_barrier(0);
      const uint32_t g = fresh(c.g);
      const uint8_t* sh = fresh(c.sh);
      const uint32_t* R = fresh(c.R);
      const size_t shard_len = fresh(c.shard_len);
      const uint32_t cqb = fresh_v(c.cqb), hb = fresh_v(c.hb);
      uint32_t m = uniform(seg_mask<NQ>(msk, step));
      if (!kRowPrefetch<NQ> && !(PRE0 && step == 0))
        issue_rows(raw, (kExp & 32) ? T.zeros : sh, (kExp & 32) ? 0 : shard_len, m, index + 16 * g, T.zeros, c.lane,
                   c.ncols, c.full, q == 0);
      stamp(c.dbg, 2 + 6 * step);
      __builtin_amdgcn_s_setprio(kRecPrioPremul);
      pipelined_rec<16>(
          [&](auto pc) __attribute__((always_inline)) {
            NP_BNOTE(reinterpret_cast<const uint8_t*>(R) + (index + 16 * g + decltype(pc)::value) * 4 * kPoolWords,
                     4 * kPoolWords, kBkRecords);
            return (cpool_t)(R) + (index + 16 * g + decltype(pc)::value) * kPoolWords;
          },
          [&](auto pc) __attribute__((always_inline)) { return ((m >> decltype(pc)::value) & 1u) != 0; },  // present
          [&](auto pc, const Mult& pool) __attribute__((always_inline)) {
            constexpr int x = decltype(pc)::value;
            XL[x] = 0;  // absent rows contribute zero
            XH[x] = 0;
            if ((m >> x) & 1u) {
              uint32_t l, h;
              blk_to_quad(raw[x], l, h);
              if constexpr (kExp & 16) {  // experiment: no premultiply
                XL[x] = l;
                XH[x] = h;
              } else {
                qmul_set(XL[x], XH[x], l, h, pool);
              }
            }
          });
      const uint32_t* vp = c.VP + vp_slot<K, NQ>(q, step) * Geo<K>::kVPWords;
      stamp(c.dbg, 3 + 6 * step);
      // absent rows are zero; segment q's transform has gen_of(qK) <= kRecMaxGen
      with_gen<0, kRecMaxGen<K, NQ>, false>(index, [&](auto gc) __attribute__((always_inline)) {
        cq_levels<K, true, false, decltype(gc)::value, false, kRecPrioCq>(T, vp, index, g, XL, XH, m);
      });
      stamp(c.dbg, 4 + 6 * step);
      if (step > 0 || after_tile) {
        __syncthreads();  // the previous high pass (or tile's copy-out) is done with the tile and the other table buffer
        if (!kRecResident<K, NQ> && step + 1 < NQ) {
          const int qn = seg_of<NQ>(step + 1);
          stage_vpools<K, Geo<K>::kThreads>(T, static_cast<uint32_t>(qn) * K, c.VP + ((step + 1) & 1) * Geo<K>::kVPWords, true);
        }
      }
      cq_write_p<K>(c.tile, cqb, XL, XH);
      // next step's rows (the systematic rows after the last step) load during
      // this step's high pass
      if constexpr (kRowPrefetch<NQ>) {
        uint32_t mn = msk[0];
        uint32_t qn = 0;
  #pragma unroll
        for (int i = 1; i < NQ; ++i) {
          if (step + 1 == i) {
            mn = msk[i];
            qn = static_cast<uint32_t>(seg_of<NQ>(i));
          }
        }
        if (step + 1 == NQ) mn = msk[NQ - 1], qn = 0;  // segment 0 is the last step's
        issue_rows(raw, (kExp & 32) ? T.zeros : sh, (kExp & 32) ? 0 : shard_len, uniform(mn), uniform(qn) * K + 16 * g,
                   T.zeros, c.lane, c.ncols, c.full, qn == 0 && step + 1 < NQ);
      }
      __syncthreads();
      stamp(c.dbg, 5 + 6 * step);
      hi_read_p<K>(c.tile, hb, XL, XH);
      // hi levels: gen_of(index) <= 4; segment 0 (index 0) skips the t = 0
      // groups, whose skew is the zero element (15 of the 32 quad multiplies)
      // (the 2-segment decode keeps its rows prefetch live here: no room for two instances)
      if (NQ == 4 && q == 0)  // -1.1 % (config 3)
        hi_levels<K, true, true, 0, 0, kRecPrioHi>(T, vp, 0, XL, XH);
      else
        hi_levels<K, true, false, 0, 0, kRecPrioHi>(T, vp, index, XL, XH);
      stamp(c.dbg, 6 + 6 * step);
    }
    __builtin_amdgcn_sched_barrier(0);
    fold(step, q);
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (PRE0) {
      // raw is reloaded at every later step: an instruction-free definition
      // here ends its live range (the loop header's phi would otherwise keep
      // step 0's rows live through every step)
#pragma unroll
      for (int x = 0; x < 16; ++x) asm volatile("" : "=v"(raw[x].x), "=v"(raw[x].y));
    }
  }
}

// Decode of one tile (K < 256: see kMultiTile), as rec_tiles with ntl = 1.
template <int K, int NQ>
__device__ __forceinline__ void rec_tile(const DevTables& T, const ReconstructArgs& a, const uint8_t* sh,
                                         const uint8_t* pres, const uint32_t* rows, uint8_t* smem,
                                         uint32_t pb, uint32_t col0, uint32_t ncols, bool full, uint64_t* dbg,
                                         uint32_t occ) {
  using G = Geo<K>;
  uint8_t* tile = smem;
  uint32_t* VP = reinterpret_cast<uint32_t*>(smem + G::kTileBytes);  // 2 staged transforms
  const uint32_t tid = threadIdx.x, lane = tid & 63u, g = uniform(tid >> 6);
  const uint32_t cqb = col_base<K>(4 * lane) ^ (32u * g);

  // presence bits of this wave's rows in every segment of the prefix; the
  // first step's rows start loading before the tables are staged
  stamp(dbg, 0);
  uint32_t msk[NQ];
#pragma unroll
  for (int i = 0; i < NQ; ++i) msk[i] = row_mask16(pres, static_cast<uint32_t>(NQ == 1 ? 0 : seg_of<NQ>(i)) * K + 16 * g, lane);
  uint2 raw[16];
  if constexpr (kRowPrefetch<NQ>)
    issue_rows(raw, (NQ > 1 && (kExp & 32)) ? T.zeros : sh, (NQ > 1 && (kExp & 32)) ? 0 : a.shard_len, msk[0],
               static_cast<uint32_t>(NQ == 1 ? 0 : seg_of<NQ>(0)) * K + 16 * g, T.zeros, lane, ncols, full);

  uint32_t XL[16], XH[16];
  if constexpr (NQ > 1) {
    // multiplier tables of the first two segment transforms (indices 2K, 3K or
    // K, 0), or of all of them (kRecResident)
    stage_rec_tables<K, NQ>(T, VP);
    __syncthreads();
    stamp(dbg, 1);

    const uint32_t hb = col_base<K>(tid / G::R) ^ (8u * (tid % G::R));
    uint32_t AL[16], AH[16];
    RecCtx c{T, a.shard_len, tile, rows, sh, VP, g, lane, tid, ncols, full, cqb, hb, dbg, occ};
    rec_segments<K, NQ>(c, msk, raw, AL, AH, false);
    // ---- forward transform of size K at index 0
    const uint32_t* vp0 = VP + vp_slot<K, NQ>(0, NQ - 1) * G::kVPWords;  // segment 0's tables = FFT(K, 0)'s
    stamp(dbg, 26);
    hi_levels<K, false, true, 0, 0, kRecPrioFwdHi>(T, vp0, 0, AL, AH);
    stamp(dbg, 27);
    __syncthreads();
    hi_write<K>(tile, fresh_v(hb), AL, AH);
    __syncthreads();
    stamp(dbg, 28);
    if constexpr (!kRowPrefetch<NQ>)  // the merge's rows load during the FFT's cq pass
      issue_rows(raw, sh, a.shard_len, uniform(msk[NQ - 1]), 16 * g, T.zeros, lane, ncols, full);
    cq_read<K>(tile, fresh_v(cqb), XL, XH);
    cq_levels<K, false, true, 0, false, kRecPrioFwdCq>(T, vp0, 0, g, XL, XH, ~uniform(msk[NQ - 1]));  // erased rows only
    stamp(dbg, 29);
  }
  // ---- merge: received systematic rows, postmultiplied recovered ones
  const uint32_t cqbf = fresh_v(cqb);
  const uint32_t m0 = uniform(msk[NQ == 1 ? 0 : NQ - 1]);  // segment 0 = the last step's
  if constexpr (NQ == 1) {
#pragma unroll
    for (int p = 0; p < 16; ++p) blk_to_quad(raw[p], XL[p], XH[p]);
  } else {
    pipelined_rec<16>(
        [&](auto pc) __attribute__((always_inline)) {
          NP_BNOTE(reinterpret_cast<const uint8_t*>(rows) + (16 * g + decltype(pc)::value) * 4 * kPoolWords,
                   4 * kPoolWords, kBkRecords);
          return (cpool_t)(fresh(rows)) + (16 * g + decltype(pc)::value) * kPoolWords;
        },
        [&](auto pc) __attribute__((always_inline)) { return ((m0 >> decltype(pc)::value) & 1u) == 0; },  // erased
        [&](auto pc, const Mult& pool) __attribute__((always_inline)) {
          constexpr int x = decltype(pc)::value;
          // present: the received symbol (mod.rs:225-235); erased: the
          // postmultiplied recovered symbol (inc_reconstruct.rs:76-84)
          if ((m0 >> x) & 1u) {
            blk_to_quad(raw[x], XL[x], XH[x]);
          } else {
            const uint32_t l = XL[x], h = XH[x];
            qmul_set(XL[x], XH[x], l, h, pool);
          }
        });
  }
  stamp(dbg, 30);
  if (full && out_vec_ok(a.out, a.out_stride)) {
    copy_out_cq<K, !kRowPrefetch<NQ>>(
        a.out + static_cast<size_t>(pb) * a.out_stride + static_cast<size_t>(col0) * 2 * K, lane, g, XL, XH);
    stamp(dbg, 31);
    return;
  }
  __syncthreads();
  cq_write<K>(tile, cqbf, XL, XH);
  __syncthreads();
  // ---- copy-out: column c of the tile is 2K contiguous bytes of the output
  {
    uint8_t* out = a.out + static_cast<size_t>(pb) * a.out_stride + static_cast<size_t>(col0) * 2 * K;
    const bool al_o = true;  // 8-byte stores at any address (rows_vec_ok)
    const uint32_t c0 = tid / G::Q, m0 = tid % G::Q;
    const uint32_t base = col_base<K>(c0) ^ (8u * m0);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const uint32_t c = c0 + 16u * i;
      if (c >= ncols) break;
      const uint2 v = *reinterpret_cast<const uint2*>(tile + (base ^ col_base_c<K>(16u * i)));
      uint8_t* o = NP_BCHK(out + static_cast<size_t>(c) * 2 * K + 8u * m0, 8, kBkOut);
      if (al_o) {
        *reinterpret_cast<uint2*>(o) = v;
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = static_cast<uint8_t>((e < 4 ? v.x : v.y) >> (8 * (e & 3)));
      }
    }
  }
  stamp(dbg, 31);
}

// Decode of ntl consecutive tiles of one payload from the first NQ segments (NQ * K rows).  The inverse
// transform of size NQ * K is NQ inverse transforms of size K (index qK)
// followed by log2(NQ) top levels whose skews at index 0 are 0 (t = 0) or
// beta = Cantor(2) (t = 1).  Only the first k = K outputs are needed; for them
//   NQ = 2:  d = D_K(x0) ^ x0 ^ x1
//   NQ = 4:  d = D_K(x0) ^ x1 ^ x2 ^ beta * (x2 ^ x3)
// where x_q = IFFT(K, qK)(premultiplied segment q) and D_K is the formal
// derivative of size K; then out = FFT(K, 0)(d) (the size-n forward transform
// restricted to its first K outputs is FFT(K, 0): its t = 0 skews are 0).
// NQ = 1: every systematic row is present, the output is those rows.
//
// Decoding from a prefix (trusted codewords only, ReconstructArgs::trusted).
// The first NQ * K codeword symbols are the codeword of the same message
// under the (NQ * K, K) code: the size-n forward transform of the zero-padded
// coefficients copies its lower half into the upper half at every top level
// (inc_afft.rs:267-332 with x[i + d] = 0), so its first NQ * K outputs are
// FFT(NQ * K, 0) of the same coefficients.  A message of K symbols is
// determined by any K of its codeword symbols, so when the received shards
// ARE a codeword, decoding the prefix with the rows beyond it treated as
// erased yields the reference's output.  For any other input the reference's
// decode (a linear map of every present row) differs, so the crate-equivalent
// entry points always decode from all n rows (or copy, NQ = 1).
template <int K, int NQ>
__device__ __forceinline__ void rec_tiles(const DevTables& T, const ReconstructArgs& a, const uint8_t* pres,
                                          const uint32_t* rows, uint8_t* smem, uint32_t pb,
                                          uint32_t tl0, uint32_t ntl, uint32_t nsyms, uint32_t occ) {
  using G = Geo<K>;
  uint8_t* tile = smem;
  uint32_t* VP = reinterpret_cast<uint32_t*>(smem + G::kTileBytes);  // 2 staged transforms
  const uint32_t tid0 = threadIdx.x, g0 = uniform(tid0 >> 6);
  const bool aligned = rows_vec_ok(a.shards, a.batch_stride, a.shard_len);
  const uint8_t* shp = a.shards + static_cast<size_t>(pb) * a.batch_stride;

  // presence bits of this wave's rows in every segment of the prefix (the
  // same for every tile of the payload); the first tile's first-step rows
  // start loading before the tables are staged
  uint32_t msk0[NQ];
#pragma unroll
  for (int i = 0; i < NQ; ++i) msk0[i] = row_mask16(pres, static_cast<uint32_t>(NQ == 1 ? 0 : seg_of<NQ>(i)) * K + 16 * g0, tid0 & 63u);
  auto tile_cols = [&](uint32_t tl) __attribute__((always_inline)) {
    return min(static_cast<uint32_t>(kTile), nsyms - tl * kTile);
  };
  // Tile order rotated by the batch entry: the workgroups running at the same
  // time then read different 512-byte pieces of their rows, instead of every
  // one the same offset of 4 KiB-strided rows (L2 conflict misses).
  const uint32_t rot = pb % ntl;
  auto tile_at = [&](uint32_t t) __attribute__((always_inline)) {
    const uint32_t i = t + rot;
    return tl0 + (i >= ntl ? i - ntl : i);
  };
  uint2 raw[16];
  if constexpr (kRowPrefetch<NQ> || kTilePrefetch<K, NQ>) {
    const uint32_t nc = tile_cols(tile_at(0));
    issue_rows(raw, (NQ > 1 && (kExp & 32)) ? T.zeros : shp + 2u * static_cast<size_t>(tile_at(0)) * kTile,
               (NQ > 1 && (kExp & 32)) ? 0 : a.shard_len, msk0[0],
               static_cast<uint32_t>(NQ == 1 ? 0 : seg_of<NQ>(0)) * K + 16 * g0, T.zeros, tid0 & 63u, nc,
               nc == kTile && aligned);
  }
  if constexpr (NQ > 1) {
    // multiplier tables of the first two segment transforms (indices 2K, 3K or
    // K, 0), or of all of them (kRecResident): kept for every tile
    stage_rec_tables<K, NQ>(T, VP);
    __syncthreads();
  }

#pragma unroll 1
  for (uint32_t t = 0; t < ntl; ++t) {
    // per-tile copies the compiler must treat as new: otherwise it hoists the
    // row offsets, sizes and descriptors derived from them out of the tile loop
    // and keeps them live in (spilled) registers across it
    const uint32_t g = fresh(g0);
    // (a copy of threadIdx.x kept across the tile loop was the kernel's one
    // spilled VGPR, and its reload waited with vmcnt(0) for every load in flight)
    const uint32_t lane = lane_fresh(), tid = 64u * g + lane;
    const uint32_t cqb = col_base<K>(4 * lane) ^ (32u * g);
    const size_t shard_len = fresh(a.shard_len);
    uint32_t msk[NQ];
#pragma unroll
    for (int i = 0; i < NQ; ++i) msk[i] = fresh(msk0[i]);
    const uint32_t tl = tile_at(t), col0 = tl * kTile, ncols = tile_cols(tl);
    const bool full = ncols == kTile && aligned;
    const uint8_t* sh = shp + 2u * static_cast<size_t>(col0);
    uint64_t* dbg = (kExp & 64) ? reinterpret_cast<uint64_t*>(a.out + static_cast<size_t>(pb) * a.out_stride +
                                                               static_cast<size_t>(nsyms) * 2 * K + ((kExp & 128) ? 4096u : 256u) * tl)
                                 : nullptr;
    stamp(dbg, 0);
    if constexpr (NQ >= 4 && !kRecResident<K, NQ>) {
      if (t > 0) {  // the first two segments' tables were replaced during the previous tile
        __syncthreads();
        stage_vpools<K, G::kThreads>(T, static_cast<uint32_t>(seg_of<NQ>(0)) * K, VP, true);
        stage_vpools<K, G::kThreads>(T, static_cast<uint32_t>(seg_of<NQ>(1)) * K, VP + G::kVPWords, true);
        __syncthreads();
      }
    }
    stamp(dbg, 1);
    uint32_t XL[16], XH[16];
    if constexpr (NQ > 1) {
      const uint32_t hb = col_base<K>(tid / G::R) ^ (8u * (tid % G::R));
      uint32_t AL[16], AH[16];
      RecCtx c{T, shard_len, tile, rows, sh, VP, g, lane, tid, ncols, full, cqb, hb, dbg, occ};
      // t > 0: step 0 waits for the previous tile's last LDS reads (its FFT's
      // cq_read, the copy-out) before writing the tile
      rec_segments<K, NQ, kTilePrefetch<K, NQ>>(c, msk, raw, AL, AH, t > 0 && (NQ == 2 || kRecResident<K, NQ>));
      // ---- forward transform of size K at index 0
      const uint32_t* vp0 = VP + vp_slot<K, NQ>(0, NQ - 1) * G::kVPWords;  // segment 0's tables = FFT(K, 0)'s
      stamp(dbg, 26);
      hi_levels<K, false, true, 0, 0, kRecPrioFwdHi>(T, vp0, 0, AL, AH);
      stamp(dbg, 27);
      __syncthreads();
      hi_write<K>(tile, fresh_v(hb), AL, AH);
      __syncthreads();
      stamp(dbg, 28);
      if constexpr (!kRowPrefetch<NQ>)  // the merge's rows load during the FFT's cq pass
        issue_rows(raw, sh, shard_len, uniform(msk[NQ - 1]), 16 * g, T.zeros, lane, ncols, full);
      cq_read<K>(tile, fresh_v(cqb), XL, XH);
      cq_levels<K, false, true, 0, false, kRecPrioFwdCq>(T, vp0, 0, g, XL, XH, ~uniform(msk[NQ - 1]));  // erased rows only
      stamp(dbg, 29);
    }
    // ---- merge: received systematic rows, postmultiplied recovered ones
    const uint32_t cqbf = fresh_v(cqb);
    const uint32_t m0 = uniform(msk[NQ == 1 ? 0 : NQ - 1]);  // segment 0 = the last step's
    if constexpr (NQ == 1) {
#pragma unroll
      for (int p = 0; p < 16; ++p) blk_to_quad(raw[p], XL[p], XH[p]);
    } else {
      pipelined_rec<16>(
          [&](auto pc) __attribute__((always_inline)) {
            NP_BNOTE(reinterpret_cast<const uint8_t*>(rows) + (16 * g + decltype(pc)::value) * 4 * kPoolWords,
                     4 * kPoolWords, kBkRecords);
            return (cpool_t)(fresh(rows)) + (16 * g + decltype(pc)::value) * kPoolWords;
          },
          [&](auto pc) __attribute__((always_inline)) { return ((m0 >> decltype(pc)::value) & 1u) == 0; },  // erased
          [&](auto pc, const Mult& pool) __attribute__((always_inline)) {
            constexpr int x = decltype(pc)::value;
            // present: the received symbol (mod.rs:225-235); erased: the
            // postmultiplied recovered symbol (inc_reconstruct.rs:76-84)
            if ((m0 >> x) & 1u) {
              blk_to_quad(raw[x], XL[x], XH[x]);
            } else {
              const uint32_t l = XL[x], h = XH[x];
              qmul_set(XL[x], XH[x], l, h, pool);
            }
          });
    }
    stamp(dbg, 30);
    // the next tile's first-step rows load during this tile's copy-out
    if constexpr (kRowPrefetch<NQ> || kTilePrefetch<K, NQ>) {
      if (t + 1 < ntl) {
        const uint32_t tn = tile_at(t + 1), nc = tile_cols(tn);
        issue_rows(raw, (NQ > 1 && (kExp & 32)) ? T.zeros : shp + 2u * static_cast<size_t>(tn) * kTile,
                   (NQ > 1 && (kExp & 32)) ? 0 : shard_len,
                   msk[0], static_cast<uint32_t>(NQ == 1 ? 0 : seg_of<NQ>(0)) * K + 16 * g, T.zeros, lane, nc,
                   nc == kTile && aligned);
      }
    }
    if (full && out_vec_ok(a.out, a.out_stride)) {
      copy_out_cq<K, !kRowPrefetch<NQ>>(
          a.out + static_cast<size_t>(pb) * a.out_stride + static_cast<size_t>(col0) * 2 * K, lane, g, XL, XH);
      stamp(dbg, 31);
      continue;
    }
    __syncthreads();
    cq_write<K>(tile, cqbf, XL, XH);
    __syncthreads();
    // ---- copy-out: column c of the tile is 2K contiguous bytes of the output
    {
      uint8_t* out = a.out + static_cast<size_t>(pb) * a.out_stride + static_cast<size_t>(col0) * 2 * K;
      const bool al_o = true;  // 8-byte stores at any address (rows_vec_ok)
      const uint32_t c0 = tid / G::Q, q0 = tid % G::Q;
      const uint32_t base = col_base<K>(c0) ^ (8u * q0);
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const uint32_t c = c0 + 16u * i;
        if (c >= ncols) break;
        const uint2 v = *reinterpret_cast<const uint2*>(tile + (base ^ col_base_c<K>(16u * i)));
        uint8_t* o = NP_BCHK(out + static_cast<size_t>(c) * 2 * K + 8u * q0, 8, kBkOut);
        if (al_o) {
          *reinterpret_cast<uint2*>(o) = v;
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e) o[e] = static_cast<uint8_t>((e < 4 ? v.x : v.y) >> (8 * (e & 3)));
        }
      }
    }
    stamp(dbg, 31);
  }
}

// One workgroup: `tpw` consecutive 256-column tiles of one batch entry (the
// row multipliers and the staged tables of a payload serve all of them, and
// the next tile's rows load during a tile's copy-out), n = NQ * K.  Without
// caller locators (a.locators == nullptr) the workgroup decodes from the rows
// that k_prefix_locator chose (NQ' = 1: the K systematic rows, all present;
// NQ' = NQ: all n rows; NQ' = 2 for trusted codewords only; NQ' = 0: fewer
// than K present rows, no decode) with its row multipliers.  Caller locators
// are over all n rows, so they pin the full decode.  An instance serves the
// payloads whose prefix has
// at most SERVE segments (SERVE = 2: prefixes of 1 and 2 segments; SERVE = 4:
// the 4-segment ones only), so each code path gets its own register allocation;
// for n = 4K the host launches both over the same grid.
template <int K, int NQ, int SERVE>
__global__ __launch_bounds__(4 * K) __attribute__((amdgpu_waves_per_eu(4))) void k_reconstruct_fast(
    DevTables T, ReconstructArgs a, uint32_t nsyms, uint32_t tiles, uint32_t tpw) {
  constexpr int N = NQ * K;
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
#if NP_BOUNDS_CHECK
  bounds_arm(bounds_of(a, T, prefix_stride_c(N, K)));
#endif
  const uint32_t groups = (tiles + tpw - 1) / tpw;  // workgroups per batch entry
  const TileRef tr = tile_of(blockIdx.x, groups, (a.batch & 7u) == 0);
  const uint32_t pb = tr.pb, tl0 = tr.tl * tpw;
  const uint32_t ntl = min(tpw, tiles - tl0);
  const uint8_t* pres = a.present + static_cast<size_t>(pb) * N;
  // the payload's decode prefix and row tables (k_prefix_locator, or
  // k_locator_records for caller locators)
  const uint8_t* rec = NP_BCHK(a.prefix + static_cast<size_t>(pb) * prefix_stride_c(N, K), 2, kBkRecords);
  const int nq = uniform(rec[0]);
  const uint32_t occ = uniform(rec[1]);  // segments with a present row
  const uint32_t* rows = reinterpret_cast<const uint32_t*>(rec + prefix_pools_offset(N));
  if constexpr (kMultiTile<K>) {
    if constexpr (SERVE >= 4) {
      if (nq == SERVE) rec_tiles<K, SERVE>(T, a, pres, rows, smem, pb, tl0, ntl, nsyms, occ);
    } else if (nq == 1) {
      rec_tiles<K, 1>(T, a, pres, rows, smem, pb, tl0, ntl, nsyms, occ);
    } else if (NQ <= 4 && nq == 2) {
      rec_tiles<K, 2>(T, a, pres, rows, smem, pb, tl0, ntl, nsyms, occ);
    }
  } else {  // tpw == 1
    const uint32_t col0 = tl0 * kTile;
    const uint32_t ncols = min(static_cast<uint32_t>(kTile), nsyms - col0);
    const uint8_t* sh = a.shards + static_cast<size_t>(pb) * a.batch_stride + 2 * static_cast<size_t>(col0);
    const bool full =
        ncols == kTile && rows_vec_ok(a.shards, a.batch_stride, a.shard_len);
    uint64_t* dbg = (kExp & 64) ? reinterpret_cast<uint64_t*>(a.out + static_cast<size_t>(pb) * a.out_stride +
                                                               static_cast<size_t>(nsyms) * 2 * K + ((kExp & 128) ? 4096u : 256u) * tl0)
                                 : nullptr;
    if constexpr (SERVE >= 4) {
      if (nq == SERVE) rec_tile<K, SERVE>(T, a, sh, pres, rows, smem, pb, col0, ncols, full, dbg, occ);
    } else if (nq == 1) {
      rec_tile<K, 1>(T, a, sh, pres, rows, smem, pb, col0, ncols, full, dbg, occ);
    } else if (NQ <= 4 && nq == 2) {
      rec_tile<K, 2>(T, a, sh, pres, rows, smem, pb, col0, ncols, full, dbg, occ);
    }
  }
}

// One workgroup: one 256-column tile of one item, decoded as k_reconstruct_fast
// decodes it (rec_tile; rec_tiles with one tile at K = 256), from the rows the
// item's prefix record names.  Instances by SERVE as k_reconstruct_fast's.
template <int K, int NQ, int SERVE>
__global__ __launch_bounds__(4 * K) __attribute__((amdgpu_waves_per_eu(4))) void k_reconstruct_ragged(DevTables T, RaggedArgs r) {
  constexpr int N = NQ * K;
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
#if NP_BOUNDS_CHECK
  bounds_arm(bounds_of_ragged(r, T, true));
#endif
  const RaggedHead h = ragged_head(r);
  if (h.item == kRaggedNoItem) return;  // padding of the plan
  // the item as a batch of one at stride 0
  ReconstructArgs a{};
  a.shards = reinterpret_cast<const uint8_t*>(h.shards);
  a.shard_len = h.shard_len;
  a.batch = 1;
  a.n = N;
  a.k = K;
  a.out = reinterpret_cast<uint8_t*>(h.data);
  const uint32_t nsyms = static_cast<uint32_t>(h.shard_len / 2);
  const uint8_t* pres = r.present + static_cast<size_t>(h.item) * N;
  const uint8_t* rec = NP_BCHK(r.prefix + static_cast<size_t>(h.item) * prefix_stride_c(N, K), 2, kBkRecords);
  const int nq = uniform(rec[0]);
  const uint32_t occ = uniform(rec[1]);  // segments with a present row
  const uint32_t* rows = reinterpret_cast<const uint32_t*>(rec + prefix_pools_offset(N));
  if constexpr (kMultiTile<K>) {
    if constexpr (SERVE >= 4) {
      if (nq == SERVE) rec_tiles<K, SERVE>(T, a, pres, rows, smem, 0, h.tile, 1, nsyms, occ);
    } else if (nq == 1) {
      rec_tiles<K, 1>(T, a, pres, rows, smem, 0, h.tile, 1, nsyms, occ);
    } else if (NQ <= 4 && nq == 2) {
      rec_tiles<K, 2>(T, a, pres, rows, smem, 0, h.tile, 1, nsyms, occ);
    }
  } else {
    const uint32_t col0 = h.tile * kTile;
    const uint32_t ncols = min(static_cast<uint32_t>(kTile), nsyms - col0);
    const uint8_t* sh = a.shards + 2 * static_cast<size_t>(col0);
    const bool full = ncols == kTile && rows_vec_ok(a.shards, 0, a.shard_len);
    if constexpr (SERVE >= 4) {
      if (nq == SERVE) rec_tile<K, SERVE>(T, a, sh, pres, rows, smem, 0, col0, ncols, full, nullptr, occ);
    } else if (nq == 1) {
      rec_tile<K, 1>(T, a, sh, pres, rows, smem, 0, col0, ncols, full, nullptr, occ);
    } else if (NQ <= 4 && nq == 2) {
      rec_tile<K, 2>(T, a, sh, pres, rows, smem, 0, col0, ncols, full, nullptr, occ);
    }
  }
}

// ------------------------------------------------------------- launchers ----
template <int K, int NQ>
size_t reconstruct_lds_bytes() {
  return static_cast<size_t>(Geo<K>::kTileBytes) + (kRecResident<K, NQ> ? NQ : 2) * 4u * Geo<K>::kVPWords;
}

template <int K, int NQ>
hipError_t launch_reconstruct_k(const DevTables& T, const ReconstructArgs& a, hipStream_t s) {
  const TileGrid g = tile_grid(a.shard_len / 2, kTile, a.batch, [&](uint32_t tiles) {
    return tiles_per_workgroup<K>(a.batch, tiles, "NP_REC_TPW");
  });
  if (g.state != kGridOk) return grid_status(g);
  k_reconstruct_fast<K, NQ, 2><<<g.blocks, Geo<K>::kThreads, reconstruct_lds_bytes<K, NQ>(), s>>>(T, a, g.count, g.tiles, g.per);
  if constexpr (NQ >= 4)
    k_reconstruct_fast<K, NQ, NQ><<<g.blocks, Geo<K>::kThreads, reconstruct_lds_bytes<K, NQ>(), s>>>(T, a, g.count, g.tiles, g.per);
  return hipGetLastError();
}

template <int K, int NQ>
hipError_t launch_reconstruct_ragged_k(const DevTables& T, const RaggedArgs& r, hipStream_t s) {
  k_reconstruct_ragged<K, NQ, 2><<<r.nblocks, Geo<K>::kThreads, reconstruct_lds_bytes<K, NQ>(), s>>>(T, r);
  if constexpr (NQ >= 4)
    k_reconstruct_ragged<K, NQ, NQ><<<r.nblocks, Geo<K>::kThreads, reconstruct_lds_bytes<K, NQ>(), s>>>(T, r);
  return hipGetLastError();
}

}  // namespace

bool fast_reconstruct_supported(uint32_t n, uint32_t k) {
  return (fast_k(k) && nq_supported(n, k)) || small_reconstruct_supported(n, k);
}

hipError_t launch_reconstruct_fast(const DevTables& T, const ReconstructArgs& a, hipStream_t s) {
  if (!fast_k(a.k)) return launch_reconstruct_small(T, a, s);  // k <= 32; hipErrorNotSupported for any other k
  return with_k(FastKs{}, a.k, hipErrorNotSupported, [&](auto kc) {
    constexpr int K = kc.value;
    return with_nq(a.n, a.k, hipErrorNotSupported,
                   [&](auto qc) { return launch_reconstruct_k<K, qc.value>(T, a, s); });
  });
}

bool ragged_reconstruct_supported(uint32_t n, uint32_t k) { return fast_k(k) && nq_supported(n, k); }

hipError_t launch_reconstruct_ragged(const DevTables& T, const RaggedArgs& r, hipStream_t s) {
  return with_ragged_k(r, [&](auto kc) {
    constexpr int K = kc.value;
    return with_nq(r.n, r.k, hipErrorNotSupported,
                   [&](auto qc) { return launch_reconstruct_ragged_k<K, qc.value>(T, r, s); });
  });
}

hipError_t configure_fast_decode_kernels() {
  LdsSetup lds;
  each_k(FastKs{}, [&](auto kc) {
    constexpr int K = kc.value;
    each_k(NqList{}, [&](auto qc) {
      constexpr int NQ = qc.value;
      lds(&k_reconstruct_fast<K, NQ, 2>, reconstruct_lds_bytes<K, NQ>());
      lds(&k_reconstruct_ragged<K, NQ, 2>, reconstruct_lds_bytes<K, NQ>());
      if constexpr (NQ >= 4) {
        lds(&k_reconstruct_fast<K, NQ, NQ>, reconstruct_lds_bytes<K, NQ>());
        lds(&k_reconstruct_ragged<K, NQ, NQ>, reconstruct_lds_bytes<K, NQ>());
      }
    });
  });
  return lds.err;
}

hipError_t bounds_take_fast_decode(uint32_t out[8]) { return bounds_take_tu(out); }

}  // namespace np
