// The planned encodes of the fast family: the single-tile encode of
// kernels_fast_encode.hip (fast_encode.hpp) on a reconstructed payload, with a
// per-payload plan that says which rows are stored (restore), compared with
// the received ones (verify), or either (recover), for uniform and ragged
// batches.
#include "fast_encode.hpp"

namespace np {
namespace {

// --------------------------------------------------------- masked encode ----
// np_restore_shards_batch_dev: k_encode_fast's flow on a reconstructed payload,
// storing only the rows of the payload's plan (launchers.hpp restore_plan_words:
// absent rows below wanted_n of a decoded payload, from k_restore_plan) into
// the buffer that holds the received rows.  The plan is read with scalar
// loads: one word of segment bits decides what the workgroup runs, 16 row bits
// per wave and pass what it stores.
//  - no row to restore: the workgroup exits before the tile load;
//  - none in [K, wanted_n): it stores its absent systematic rows and exits
//    before the inverse transform;
//  - shift s runs only when segment s holds a row to restore; the tables of
//    the other shifts are not staged;
//  - inside a shift's cq levels a wave runs only the butterfly groups that
//    feed one of its rows to restore (cq_levels `rows`).
// Every exit is workgroup-uniform and sits before the barrier it would miss.

// First segment >= from with its plan bit set, or nseg (wave-uniform).
__device__ __forceinline__ uint32_t next_segment(cpool_t seg, uint32_t from, uint32_t nseg) {
  uint32_t r = nseg;
  for (uint32_t w = from >> 5; 32u * w < nseg; ++w) {
    uint32_t x = seg[w];
    if (w == (from >> 5)) x &= ~0u << (from & 31u);
    if (x) {
      r = 32u * w + static_cast<uint32_t>(__builtin_ctz(x));
      break;
    }
  }
  return uniform(r);
}

// The table choices of stage_vpools are scalar selects: their conditions must
// be in SGPRs whatever the compiler proves about a shift number.
__device__ __forceinline__ bool uniform_b(bool v) { return uniform(v ? 1u : 0u) != 0; }
// enc_conv(K, sh) of a runtime shift (gen_of(sh K) >= 1 is sh K >= 256), inlined.
template <int K>
__device__ __forceinline__ bool enc_conv_u(uint32_t sh) {
  static_assert(!enc_conv(K, 0) && enc_conv(K, 1) == (K >= 256) && enc_conv(K, 2) == (2 * K >= 256) &&
                    enc_conv(K, 3) == (3 * K >= 256) && !enc_conv(K, 4),
                "enc_conv");
  return uniform_b(sh >= 1u && sh <= 3u && sh * K >= 256u);
}

// Bit p: row row0 + p is restored (row0 a multiple of 16, wave-uniform).
__device__ __forceinline__ uint32_t restore_mask16(cpool_t rows, uint32_t row0) {
  return uniform((rows[row0 >> 5] >> (row0 & 16u)) & 0xffffu);
}

// store_rows for the rows of `mask` only (wave-uniform: a scalar branch per row).
__device__ __forceinline__ void store_rows_masked(uint8_t* out, size_t shard_len, uint32_t row0, uint32_t mask,
                                                  const uint32_t (&L)[16], const uint32_t (&H)[16], uint32_t lane,
                                                  uint32_t ncols, bool full, bool nt) {
  if (mask == 0) return;
  if (full && 16 * shard_len < 0x7fffffffu) {
    // (the descriptor spans 16 rows; only rows of the mask, all below wanted_n, are accessed)
    const __amdgpu_buffer_rsrc_t r = buf_rsrc(out + static_cast<size_t>(row0) * shard_len, 16 * static_cast<uint32_t>(shard_len));
    if (nt) {
#pragma unroll
      for (int p = 0; p < 16; ++p)
        if ((mask >> p) & 1u) {
          const uint2 v = cq_row(L[p], H[p]);
          __builtin_amdgcn_raw_buffer_store_b64(u32x2{v.x, v.y}, r, 8u * lane,
                                                static_cast<uint32_t>(p * shard_len), kRowStoreCpol);
        }
    } else {
#pragma unroll
      for (int p = 0; p < 16; ++p)
        if ((mask >> p) & 1u) {
          const uint2 v = cq_row(L[p], H[p]);
          __builtin_amdgcn_raw_buffer_store_b64(u32x2{v.x, v.y}, r, 8u * lane, static_cast<uint32_t>(p * shard_len), 0);
        }
    }
  } else if (4 * lane + 4 <= ncols) {  // partial tile, lanes with all four columns
#pragma unroll
    for (int p = 0; p < 16; ++p)
      if ((mask >> p) & 1u) *reinterpret_cast<uint2*>(out + static_cast<size_t>(row0 + p) * shard_len + 8u * lane) = cq_row(L[p], H[p]);
  } else {
#pragma unroll
    for (int p = 0; p < 16; ++p)
      if ((mask >> p) & 1u) store4(out + static_cast<size_t>(row0 + p) * shard_len, cq_row(L[p], H[p]), lane, ncols, false);
  }
}

// shift_cq for the output rows of `rows` only.
template <int K, int SH>
__device__ __forceinline__ void shift_cq_rows(const DevTables& T, const uint32_t* vp, uint32_t index, uint32_t g,
                                              uint32_t (&XL)[16], uint32_t (&XH)[16], uint32_t rows) {
  if constexpr (SH == 0) {
    cq_levels<K, false, false, -1, false, kEncPrioCq>(T, vp, index, g, XL, XH, rows);
  } else {
    cq_levels<K, false, false, kShiftGen<K, SH>, kEncConv<K, SH>, kEncPrioCq>(T, vp, index, g, XL, XH, rows);
    if constexpr (!kEncConv<K, SH>) tower_convert(T, XL, XH);  // back to Cantor coordinates for the shard rows
  }
}

// SH of shift 3 when shift 1 or 2 was skipped: fwd_top's MODE 3 takes shift
// 3's top-level products from PL / PH, where shifts 1 and 2 leave them; this
// instance multiplies for itself (MODE 0).
constexpr int kShift3Own = 30;

// What encode_planned does with the 16 rows of a wave and pass that its plan
// marks: the restore stores them (here), the verify compares them with the
// received rows (CompareRows, with compare_rows_masked).  kSeg0: whether the
// plan can mark systematic rows.
struct StoreRows {
  static constexpr bool kSeg0 = true;
  __device__ __forceinline__ void operator()(const EncTile& t, uint32_t row0, uint32_t mask, const uint32_t (&L)[16],
                                             const uint32_t (&H)[16], uint32_t lane) const {
    store_rows_masked(t.out, t.shard_len, row0, mask, L, H, lane, t.ncols, t.full, t.nt);
  }
};

// The plan words of payload or item `i` (scalar loads).
__device__ __forceinline__ cpool_t plan_of(const uint32_t* plan, size_t i, uint32_t n, uint32_t k) {
  const uint32_t planw = static_cast<uint32_t>(restore_plan_words(n, k));
  NP_BNOTE(plan + i * planw, 4u * planw, kBkRecords);
  return (cpool_t)(plan) + i * planw;
}

// One workgroup: 256 chunks of one payload, the rows of its plan `seg` (segment
// words, then row words) handed to `sink`.
template <int K, typename SINK>
__device__ __forceinline__ void encode_planned(const DevTables& T, uint8_t* smem, uint32_t n, const EncTile& t,
                                               cpool_t seg, SINK sink) {
  using G = Geo<K>;
  uint8_t* tile = smem;
  uint32_t* VP = reinterpret_cast<uint32_t*>(smem + G::kTileBytes);  // up to 4 staged transforms
  const uint32_t nshift = n / K;
  const cpool_t rowbits = seg + static_cast<uint32_t>(restore_seg_words(n, K));
  const bool seg0 = SINK::kSeg0 && (seg[0] & 1u) != 0;
  const uint32_t first = next_segment(seg, 1, nshift);  // the first shift to run
  if (!seg0 && first == nshift) return;                 // no row of the plan (or NeedMoreShards)
  const uint32_t tid = threadIdx.x, lane = tid & 63u, g = uniform(tid >> 6);
  load_tile<K>(tile, t, tid);
  // n <= 4K: one table buffer per transform that runs; otherwise two buffers
  // alternate, each shift staging the next one that runs
  const bool resident = nshift <= 4;
  if (!SINK::kSeg0 || first < nshift) {
    stage_vpools<K, G::kThreads>(T, 0, VP, true);  // inverse transform, index 0
    if (resident) {
      for (uint32_t sh = first; sh < nshift; sh = next_segment(seg, sh + 1, nshift))
        stage_vpools<K, G::kThreads>(T, sh * K, VP + sh * G::kVPWords, true, enc_conv_u<K>(sh));
    } else {
      stage_vpools<K, G::kThreads>(T, first * K, VP + G::kVPWords, uniform_b(first < 4), enc_conv_u<K>(first));
    }
  }
  __syncthreads();

  const uint32_t cqb = col_base<K>(4 * lane) ^ (32u * g);  // blocks 4g..4g+3 of columns 4l..4l+3
  // ---- cq pass: marked systematic rows, inverse levels 0..3
  {
    uint32_t CL[16], CH[16];
    cq_read<K>(tile, cqb, CL, CH);
    if constexpr (SINK::kSeg0) {
      if (seg0) sink(t, 16 * g, restore_mask16(rowbits, 16 * g), CL, CH, lane);
      if (first == nshift) return;  // no parity row of the plan
    }
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

  // top-level products of shift 1, then of shifts 1 ^ 2 (fwd_top); zero, so that
  // a shift 2 without shift 1 accumulates into defined values (which nobody reads)
  uint32_t PL[8] = {}, PH[8] = {};
  uint32_t slot = 1;  // !resident: the table buffer of the shift that runs
  // shift sh; nxt: the next shift that runs (nshift: none)
  auto shift = [&](auto shc, uint32_t sh, uint32_t nxt) __attribute__((always_inline)) {
    constexpr int SH = decltype(shc)::value;
    constexpr int SHC = SH == kShift3Own ? 3 : SH;
    const uint32_t index = sh * K;
    uint32_t XL[16], XH[16];
    const uint32_t* vp = VP + (resident ? sh : slot) * G::kVPWords;
    if constexpr (SH == kShift3Own) {
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        XL[q] = ML[q];
        XH[q] = MH[q];
      }
      fwd_top<K, 0, 0>(T, vp, index, XL, XH, PL, PH);
      hi_levels<K, false, false, 1, 0, kEncPrio>(T, vp, index, XL, XH);
    } else {
      shift_hi<K, SH>(T, vp, index, ML, MH, XL, XH, PL, PH);
    }
    __syncthreads();  // the previous cq pass is done with the tile and with the other table buffer
    if (!resident && nxt < nshift)
      stage_vpools<K, G::kThreads>(T, nxt * K, VP + (slot ^ 1u) * G::kVPWords, uniform_b(nxt < 4),
                                   enc_conv_u<K>(nxt));
    hi_write_q<K>(tile, g, lane, XL, XH);
    __syncthreads();
    cq_read_q(tile, g, lane, XL, XH);
    const uint32_t mask = restore_mask16(rowbits, index + 16 * g);
    shift_cq_rows<K, SHC>(T, vp, index, g, XL, XH, mask);
    sink(t, index + 16 * g, mask, XL, XH, lane);
    slot ^= 1u;
  };
  const bool own3 = ((seg[0] >> 1) & 3u) != 3u;  // shift 1 or 2 skipped
  // cur: the next shift to run; nshift (2 at n = 2K: not "shift 2") when none is left
  uint32_t cur = first;
  if (cur == 1) {
    const uint32_t nxt = next_segment(seg, 2, nshift);
    shift(Int<1>{}, 1, nxt);
    cur = nxt;
  }
  if (cur == 2 && cur < nshift) {
    const uint32_t nxt = next_segment(seg, 3, nshift);
    shift(Int<2>{}, 2, nxt);
    cur = nxt;
  }
  if (cur == 3 && cur < nshift) {
    const uint32_t nxt = next_segment(seg, 4, nshift);
    if (own3)
      shift(Int<kShift3Own>{}, 3, nxt);
    else
      shift(Int<3>{}, 3, nxt);
    cur = nxt;
  }
#pragma unroll 1
  while (cur < nshift) {
    const uint32_t nxt = next_segment(seg, cur + 1, nshift);
    shift(Int<0>{}, cur, nxt);
    cur = nxt;
  }
}

#if NP_BOUNDS_CHECK
// bounds_of_enc plus the plan and (verify) the flag map.
__device__ __forceinline__ BoundsSet bounds_of_enc_planned(const EncodeArgs& a, const uint32_t* plan,
                                                           const uint8_t* flags) {
  BoundsSet b = bounds_of_enc(a);  // (verify: shards are the received rows, read only)
  b.lo[kBkRecords] = reinterpret_cast<uint64_t>(plan);
  b.hi[kBkRecords] = b.lo[kBkRecords] + a.batch * restore_plan_words(a.n, a.k) * 4u;
  if (flags) {
    b.lo[kBkOut] = reinterpret_cast<uint64_t>(flags);
    b.hi[kBkOut] = b.lo[kBkOut] + a.batch * static_cast<uint64_t>(a.n);
  }
  return b;
}
#endif

// --------------------------------------------------------- verify encode ----
// np_verify_shards_batch_dev: k_encode_masked's flow on the reconstructed
// payload with a compare in place of the store.  The plan (k_verify_plan) marks
// the present rows in [K, wanted_n) of a decoded payload; a wave re-encodes its
// 16 rows of a shift, reads the received bytes of the marked ones and sets the
// row's flag when any of the tile's columns differs.  Nothing else is written:
// a.shards is only read.  Segment 0 is never marked (a present systematic row
// equals its re-encoding), so a payload with no marked row exits before the
// tile load; the skipped shifts, the unstaged tables, the `rows` mask of the cq
// levels and kShift3Own are the masked encode's.

// Received rows a wave loads before it compares them.  A workgroup's waves
// reach the compare together, so nothing else hides the loads' latency: 8 in
// flight measured 1 % below 4 on the whole call at config 3;
// 16 spill (28-40 bytes of scratch per lane).
constexpr int kVerifyGroup = 8;

// XOR of the received 4 columns of this lane with the re-encoded ones, for
// lanes and columns below ncols (others: 0).
__device__ __forceinline__ uint32_t diff4(const uint8_t* rowp, uint2 v, uint32_t lane, uint32_t ncols) {
  uint32_t d = 0;
  if (4 * lane + 4 <= ncols) {  // lanes with all four columns
    const uint2 r = *reinterpret_cast<const uint2*>(rowp + 8u * lane);
    d = (r.x ^ v.x) | (r.y ^ v.y);
  } else {
    const uint32_t w[2] = {v.x, v.y};
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (4 * lane + i < ncols) {
        const uint32_t r = *reinterpret_cast<const uint16_t*>(rowp + 8u * lane + 2 * i);
        d |= r ^ ((w[i >> 1] >> (16 * (i & 1))) & 0xffffu);
      }
  }
  return d;
}

// The rows of `mask` (wave-uniform) among row0..row0+15: flag[row0 + p] = 1
// when the received row differs from cq_row(L[p], H[p]) in a column of this
// tile.  Full tiles load kVerifyGroup rows at a time through per-row
// descriptors of size 0 for unmarked rows (no branch, no traffic; as
// issue_rows_c): loading all 16 ahead of the cq levels, or after them, spills.
__device__ __forceinline__ void compare_rows_masked(const uint8_t* in, size_t shard_len, uint32_t row0, uint32_t mask,
                                                    const uint32_t (&L)[16], const uint32_t (&H)[16], uint32_t lane,
                                                    uint32_t ncols, bool full, uint8_t* flag) {
  if (mask == 0) return;
  if (full) {
#pragma unroll
    for (int p0 = 0; p0 < 16; p0 += kVerifyGroup) {
      if (((mask >> p0) & ((1u << kVerifyGroup) - 1u)) == 0) continue;
      u32x2 r[kVerifyGroup];
#pragma unroll
      for (int q = 0; q < kVerifyGroup; ++q) {
        const int p = p0 + q;
        const uint8_t* rowp = in + static_cast<size_t>(row0 + p) * shard_len;
        if ((mask >> p) & 1u) NP_BNOTE(rowp + 8u * lane, 8, kBkShards);
        const __amdgpu_buffer_rsrc_t rs = buf_rsrc(rowp, ((mask >> p) & 1u) ? 512u : 0u);
        r[q] = __builtin_amdgcn_raw_buffer_load_b64(rs, 8u * lane, 0, 2);  // read once: streaming
      }
#pragma unroll
      for (int q = 0; q < kVerifyGroup; ++q) {
        const int p = p0 + q;
        if ((mask >> p) & 1u) {
          const uint2 v = cq_row(L[p], H[p]);
          const bool any = __builtin_amdgcn_ballot_w64(((r[q].x ^ v.x) | (r[q].y ^ v.y)) != 0) != 0;
          NP_BNOTE(flag + (row0 + p), 1, kBkOut);
          if (any && lane == 0) flag[row0 + p] = 1;
        }
      }
    }
  } else {
#pragma unroll
    for (int p = 0; p < 16; ++p)
      if ((mask >> p) & 1u) {
        const uint8_t* rowp = in + static_cast<size_t>(row0 + p) * shard_len;
        NP_BNOTE(rowp, 2u * ncols, kBkShards);
        const uint32_t d = diff4(rowp, cq_row(L[p], H[p]), lane, ncols);
        const bool any = __builtin_amdgcn_ballot_w64(d != 0) != 0;
        NP_BNOTE(flag + (row0 + p), 1, kBkOut);
        if (any && lane == 0) flag[row0 + p] = 1;
      }
  }
}

// encode_planned's sink of the verify: the tile's shard rows are the received
// ones, `flag` the flag row of the payload.  The verify plan never marks segment 0.
struct CompareRows {
  static constexpr bool kSeg0 = false;
  uint8_t* flag;
  __device__ __forceinline__ void operator()(const EncTile& t, uint32_t row0, uint32_t mask, const uint32_t (&L)[16],
                                             const uint32_t (&H)[16], uint32_t lane) const {
    compare_rows_masked(t.out, t.shard_len, row0, mask, L, H, lane, t.ncols, t.full, flag);
  }
};

// -------------------------------------------------------- recover encode ----
// np_recover_batch_dev with the restore and the verify requested: one pass over
// the re-encoding of the reconstructed payload that stores the absent rows
// below wanted_n into a.shards (k_encode_masked's part) and compares the present
// rows in [K, wanted_n) with a.shards (k_encode_verify's part).  The plan
// (k_recover_plan, launchers.hpp recover_plan_words) marks the union of the two
// in the words encode_planned reads, so that a segment or a butterfly group is
// skipped only when neither purpose needs it; a further array of row words says
// which rows of the union are stored.  A row is stored or compared, never both:
// the stores touch absent rows only, the loads present rows only, so no
// workgroup reads what another writes.

// encode_planned's sink of the recover.  The compare goes first: its loads are
// what the wave waits for, while the stores need no answer and drain under the
// next shift's transforms.
struct RecoverRows {
  static constexpr bool kSeg0 = true;  // absent systematic rows are stored (present ones are never marked)
  cpool_t stores;                      // the payload's row words of the rows to store
  uint8_t* flag;
  __device__ __forceinline__ void operator()(const EncTile& t, uint32_t row0, uint32_t mask, const uint32_t (&L)[16],
                                             const uint32_t (&H)[16], uint32_t lane) const {
    const uint32_t st = restore_mask16(stores, row0) & mask;
    compare_rows_masked(t.out, t.shard_len, row0, mask & ~st, L, H, lane, t.ncols, t.full, flag);
    store_rows_masked(t.out, t.shard_len, row0, st, L, H, lane, t.ncols, t.full, t.nt);
  }
};

// --------------------------------------------------------------- kernels ----
template <int K>
__global__ __launch_bounds__(4 * K) __attribute__((amdgpu_waves_per_eu(4))) void k_encode_masked(
    DevTables T, EncodeArgs a, uint32_t nchunks, uint32_t tiles, const uint32_t* plan) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
#if NP_BOUNDS_CHECK
  bounds_arm(bounds_of_enc_planned(a, plan, nullptr));
#endif
  const TileRef tr = tile_of(blockIdx.x, tiles, (a.batch & 7u) == 0);
  encode_planned<K>(T, smem, a.n, enc_tile(a, nchunks, tr), plan_of(plan, tr.pb, a.n, K), StoreRows{});
}

template <int K>
__global__ __launch_bounds__(4 * K) __attribute__((amdgpu_waves_per_eu(4))) void k_encode_verify(
    DevTables T, EncodeArgs a, uint32_t nchunks, uint32_t tiles, const uint32_t* plan, uint8_t* flags) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
#if NP_BOUNDS_CHECK
  bounds_arm(bounds_of_enc_planned(a, plan, flags));
#endif
  const TileRef tr = tile_of(blockIdx.x, tiles, (a.batch & 7u) == 0);
  encode_planned<K>(T, smem, a.n, enc_tile(a, nchunks, tr), plan_of(plan, tr.pb, a.n, K),
                    CompareRows{flags + static_cast<size_t>(tr.pb) * a.n});
}

template <int K>
__global__ __launch_bounds__(4 * K) __attribute__((amdgpu_waves_per_eu(4))) void k_encode_recover(
    DevTables T, EncodeArgs a, uint32_t nchunks, uint32_t tiles, const uint32_t* plan, uint8_t* flags) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const uint32_t planw = static_cast<uint32_t>(recover_plan_words(a.n, K));
#if NP_BOUNDS_CHECK
  {
    BoundsSet b = bounds_of_enc(a);  // shards: the received rows, read and written
    b.lo[kBkRecords] = reinterpret_cast<uint64_t>(plan);
    b.hi[kBkRecords] = b.lo[kBkRecords] + a.batch * static_cast<uint64_t>(planw) * 4u;
    b.lo[kBkOut] = reinterpret_cast<uint64_t>(flags);
    b.hi[kBkOut] = b.lo[kBkOut] + a.batch * static_cast<uint64_t>(a.n);
    bounds_arm(b);
  }
#endif
  const TileRef tr = tile_of(blockIdx.x, tiles, (a.batch & 7u) == 0);
  NP_BNOTE(plan + static_cast<size_t>(tr.pb) * planw, 4u * planw, kBkRecords);
  const cpool_t seg = (cpool_t)(plan) + static_cast<size_t>(tr.pb) * planw;  // scalar loads
  encode_planned<K>(T, smem, a.n, enc_tile(a, nchunks, tr), seg,
                    RecoverRows{seg + static_cast<uint32_t>(restore_plan_words(a.n, K)),
                                flags + static_cast<size_t>(tr.pb) * a.n});
}

// ------------------------------------------- ragged restore and verify ----
// np_restore_shards_ragged_dev / np_verify_shards_ragged_dev: the flows of
// k_encode_masked and k_encode_verify with the ragged head.  The item's record
// names its decoded payload in the context scratch ({address, (shard_len / 2) *
// 2K}) and its shard rows; the plan words (k_restore_plan / k_verify_plan) and
// the verify's flag row stay per item at their fixed strides.  `plan` and
// `flags` are kernel parameters of their own: RaggedArgs is what the kernels
// above take.  Every skip of the uniform kernels is kept, each exit
// workgroup-uniform and before the barrier it would miss.

#if NP_BOUNDS_CHECK
// bounds_of_ragged's extents (the payload scratch, the caller's shard buffer,
// the records, the block table) plus what the engine's flow around the launch
// holds per item: plan, present flags, status and (verify) the flag map.
__device__ __forceinline__ BoundsSet bounds_of_ragged_masked(const RaggedArgs& r, const DevTables& T,
                                                             const uint32_t* plan, const uint8_t* flags) {
  BoundsSet b = bounds_of_ragged(r, T, false);
  auto set = [&](uint32_t k, const void* p, uint64_t bytes) {
    if (!p || bytes == 0) return;
    b.lo[k] = reinterpret_cast<uint64_t>(p);
    b.hi[k] = b.lo[k] + bytes;
  };
  set(kBkRecords, plan, static_cast<uint64_t>(r.nitems) * restore_plan_words(r.n, r.k) * 4u);
  set(kBkPresent, r.present, static_cast<uint64_t>(r.nitems) * r.n);
  set(kBkStatus, r.status, static_cast<uint64_t>(r.nitems) * 8u);
  set(kBkOut, flags, static_cast<uint64_t>(r.nitems) * r.n);
  return b;
}
#endif

// One workgroup: one 256-column tile of one item, the rows of the item's plan
// stored into its shard rows (k_encode_masked's flow).
template <int K>
__global__ __launch_bounds__(4 * K) __attribute__((amdgpu_waves_per_eu(4))) void k_encode_masked_ragged(
    DevTables T, RaggedArgs r, const uint32_t* plan) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
#if NP_BOUNDS_CHECK
  bounds_arm(bounds_of_ragged_masked(r, T, plan, nullptr));
#endif
  const RaggedHead h = ragged_head(r);
  if (h.item == kRaggedNoItem) return;  // padding of the plan
  encode_planned<K>(T, smem, r.n, enc_tile(h), plan_of(plan, h.item, r.n, K), StoreRows{});
}

// One workgroup: one 256-column tile of one item, the present rows of the
// item's plan compared with its re-encoding (k_encode_verify's flow); the flag
// row of item i is flags + i * n.  The shard rows are only read.
template <int K>
__global__ __launch_bounds__(4 * K) __attribute__((amdgpu_waves_per_eu(4))) void k_encode_verify_ragged(
    DevTables T, RaggedArgs r, const uint32_t* plan, uint8_t* flags) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
#if NP_BOUNDS_CHECK
  bounds_arm(bounds_of_ragged_masked(r, T, plan, flags));
#endif
  const RaggedHead h = ragged_head(r);
  if (h.item == kRaggedNoItem) return;  // padding of the plan
  encode_planned<K>(T, smem, r.n, enc_tile(h), plan_of(plan, h.item, r.n, K),
                    CompareRows{flags + static_cast<size_t>(h.item) * r.n});
}

// ------------------------------------------------ ragged recover encode ----
// np_recover_ragged_dev with the restore and the verify requested:
// k_encode_recover's flow with the ragged head.  The item's record names its
// decoded payload (in the context scratch, or in the caller's output buffer at
// any byte address) and its shard rows; the plan words (k_recover_plan) and the
// flag row stay per item at their fixed strides.

// One workgroup: one 256-column tile of one item, the absent rows of the item's
// plan stored into its shard rows and the present ones compared with them.
template <int K>
__global__ __launch_bounds__(4 * K) __attribute__((amdgpu_waves_per_eu(4))) void k_encode_recover_ragged(
    DevTables T, RaggedArgs r, const uint32_t* plan, uint8_t* flags) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const uint32_t planw = static_cast<uint32_t>(recover_plan_words(r.n, K));
#if NP_BOUNDS_CHECK
  {
    BoundsSet b = bounds_of_ragged_masked(r, T, plan, flags);  // shards: the received rows, read and written
    b.hi[kBkRecords] = b.lo[kBkRecords] + static_cast<uint64_t>(r.nitems) * planw * 4u;
    bounds_arm(b);
  }
#endif
  const RaggedHead h = ragged_head(r);
  if (h.item == kRaggedNoItem) return;  // padding of the plan
  // (plan_of steps by the restore plan's words; this plan is longer)
  NP_BNOTE(plan + static_cast<size_t>(h.item) * planw, 4u * planw, kBkRecords);
  const cpool_t seg = (cpool_t)(plan) + static_cast<size_t>(h.item) * planw;  // scalar loads
  encode_planned<K>(T, smem, r.n, enc_tile(h), seg,
                    RecoverRows{seg + static_cast<uint32_t>(restore_plan_words(r.n, K)),
                                flags + static_cast<size_t>(h.item) * r.n});
}

// ------------------------------------------------------------- launchers ----
// launch(Int<K>{}, grid) starts the kernel of a.k.  One tile per workgroup at
// every K (one_tile).
template <typename F>
hipError_t with_planned(const EncodeArgs& a, F launch) {
  return with_k(FastKs{}, a.k, hipErrorNotSupported, [&](auto kc) {
    return with_encode_grid(a, one_tile, [&](const TileGrid& g) { launch(kc, g); });
  });
}

}  // namespace

bool masked_encode_supported(uint32_t n, uint32_t k) { return fast_k(k) && n >= 2 * k && n <= 65536; }
bool ragged_masked_supported(uint32_t n, uint32_t k) { return ragged_reconstruct_supported(n, k); }

hipError_t launch_encode_masked(const DevTables& T, const EncodeArgs& a, const uint32_t* plan, hipStream_t s) {
  return with_planned(a, [&](auto kc, const TileGrid& g) {
    constexpr int K = kc.value;
    k_encode_masked<K><<<g.blocks, Geo<K>::kThreads, encode_lds_bytes<K>(), s>>>(T, a, g.count, g.tiles, plan);
  });
}

hipError_t launch_encode_verify(const DevTables& T, const EncodeArgs& a, const uint32_t* plan, uint8_t* flags, hipStream_t s) {
  return with_planned(a, [&](auto kc, const TileGrid& g) {
    constexpr int K = kc.value;
    k_encode_verify<K><<<g.blocks, Geo<K>::kThreads, encode_lds_bytes<K>(), s>>>(T, a, g.count, g.tiles, plan, flags);
  });
}

hipError_t launch_encode_recover(const DevTables& T, const EncodeArgs& a, const uint32_t* plan, uint8_t* flags, hipStream_t s) {
  return with_planned(a, [&](auto kc, const TileGrid& g) {
    constexpr int K = kc.value;
    k_encode_recover<K><<<g.blocks, Geo<K>::kThreads, encode_lds_bytes<K>(), s>>>(T, a, g.count, g.tiles, plan, flags);
  });
}

hipError_t launch_encode_masked_ragged(const DevTables& T, const RaggedArgs& r, const uint32_t* plan,
                                       hipStream_t s) {
  return with_ragged_k(r, [&](auto kc) {
    constexpr int K = kc.value;
    k_encode_masked_ragged<K><<<r.nblocks, Geo<K>::kThreads, encode_lds_bytes<K>(), s>>>(T, r, plan);
    return hipGetLastError();
  });
}

hipError_t launch_encode_verify_ragged(const DevTables& T, const RaggedArgs& r, const uint32_t* plan, uint8_t* flags,
                                       hipStream_t s) {
  return with_ragged_k(r, [&](auto kc) {
    constexpr int K = kc.value;
    k_encode_verify_ragged<K><<<r.nblocks, Geo<K>::kThreads, encode_lds_bytes<K>(), s>>>(T, r, plan, flags);
    return hipGetLastError();
  });
}

hipError_t launch_encode_recover_ragged(const DevTables& T, const RaggedArgs& r, const uint32_t* plan, uint8_t* flags,
                                        hipStream_t s) {
  return with_ragged_k(r, [&](auto kc) {
    constexpr int K = kc.value;
    k_encode_recover_ragged<K><<<r.nblocks, Geo<K>::kThreads, encode_lds_bytes<K>(), s>>>(T, r, plan, flags);
    return hipGetLastError();
  });
}

hipError_t configure_fast_planned_kernels() {
  LdsSetup lds;
  each_k(FastKs{}, [&](auto kc) {
    constexpr int K = kc.value;
    lds(&k_encode_masked<K>, encode_lds_bytes<K>());
    lds(&k_encode_verify<K>, encode_lds_bytes<K>());
    lds(&k_encode_recover<K>, encode_lds_bytes<K>());
    lds(&k_encode_masked_ragged<K>, encode_lds_bytes<K>());
    lds(&k_encode_verify_ragged<K>, encode_lds_bytes<K>());
    lds(&k_encode_recover_ragged<K>, encode_lds_bytes<K>());
  });
  return lds.err;
}

hipError_t bounds_take_fast_planned(uint32_t out[8]) { return bounds_take_tu(out); }

}  // namespace np
