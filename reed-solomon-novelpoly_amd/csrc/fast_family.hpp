// What the translation units of the fast family (kernels_fast_encode.hip,
// kernels_fast_planned.hip, kernels_fast_decode.hip) share besides
// fast_common.hpp: the K list, the issue priorities, the multi-tile rule, the
// dynamic-LDS set-up and the head of the ragged kernels.
#pragma once
#include <algorithm>
#include <cstdlib>

#include "fast_common.hpp"

namespace np {
namespace {

// The k the family serves (every kernel is a template over K).
using FastKs = Ints<64, 128, 256>;
constexpr bool fast_k(uint32_t k) { return k_in(FastKs{}, k); }

// Issue priority (s_setprio, fast_common.hpp progress_prio; DESIGN.md §4.2,
// §4.3).  Encode: every transform pass by progress (priority 3 in its first
// quarter of butterfly groups down to 0 in the last): config-3 encode 1.601 /
// 1.602 -> 1.514 / 1.527 ms (-5 %, profiles/r04_ab.txt probe 18).  Decode: one
// schedule over each barrier-free span of the segment sweep (high levels of
// step s, fold, premultiply and cq levels of step s + 1): priority 2 in the
// high levels (progress schedule 2), 2 in the premultiply, 3 then 0 in the cq
// levels: config-3 reconstruct -3.2 % (probe 21); the forward transform's
// spans likewise (its high levels 3, its cq levels and the merge 2): -1.7 %
// (probe 22).  Per-pass priority in the decode measured +1.5 to +2.8 %, the
// encode's span schedule neutral, premultiply priorities 1 and 3 and high-level
// schedule 4 within noise (probes 24, 26).
constexpr int kEncPrio = 1, kEncPrioCq = 1;
constexpr int kRecPrioPremul = 2, kRecPrioCq = 3, kRecPrioHi = 2, kRecPrioFwdHi = 3, kRecPrioFwdCq = 2;

// Multi-tile workgroups (k = 256 only).  Tried for the k = 64 / 128 decodes
// too: 5-11 % slower at 190, 300 and 700 validators, neutral at config 2
// (profiles/r04_ab.txt probe 11) -- there four workgroups share a CU, and
// fewer, longer ones hid less.
template <int K>
constexpr bool kMultiTile = K == 256;

// Tiles per workgroup (kMultiTile): as many as keep >= kWorkgroups
// workgroups (4 per CU on 256 CUs) in the grid.  `knob` names an environment
// variable that pins the count (tests).
constexpr size_t kWorkgroups = 1024;

template <int K>
uint32_t tiles_per_workgroup(size_t batch, uint32_t tiles, const char* knob) {
  if (!kMultiTile<K>) return 1;
  size_t want = batch * tiles / kWorkgroups;
  if (const char* e = std::getenv(knob)) want = std::strtoul(e, nullptr, 10);
  return static_cast<uint32_t>(std::max<size_t>(1, std::min<size_t>(tiles, want)));
}

// ---------------------------------------------------------- ragged batches ----
// np_encode_ragged_dev / np_reconstruct_ragged_dev: the single-tile flows of
// k_encode_fast and k_reconstruct_fast on a batch whose items differ in length
// and sit anywhere in the caller's buffers.  The workgroup head reads its
// (item, tile) from the block table of the host's plan (np_ragged_plan) and the
// item's addresses and lengths from its RaggedRec with scalar loads; what the
// uniform kernels derive per launch (the column count, `full`, the streaming
// stores, the tile load's fast test) is derived per item.  Padding entries of
// the table (kRaggedNoItem) exit, workgroup-uniformly, before any barrier of
// the flow.  The present flags, the prefix records and the status stay per
// item at their fixed strides.
typedef const __attribute__((address_space(4))) uint64_t* crec_t;

struct RaggedHead {
  uint32_t item, tile;
  uint64_t data, data_len, shards, shard_len;
};

// The workgroup's block-table entry and its item's record (wave-uniform).
__device__ __forceinline__ RaggedHead ragged_head(const RaggedArgs& r) {
  RaggedHead h{};
  NP_BNOTE(r.block_item + blockIdx.x, 4, kBkBlocks);
  NP_BNOTE(r.block_tile + blockIdx.x, 4, kBkBlocks);
  h.item = ((cpool_t)(r.block_item))[blockIdx.x];
  if (h.item == kRaggedNoItem) return h;
  h.tile = ((cpool_t)(r.block_tile))[blockIdx.x];
  NP_BNOTE(r.recs + h.item, sizeof(RaggedRec), kBkItems);
  const crec_t rec = (crec_t)(r.recs + h.item);
  h.data = rec[0], h.data_len = rec[1], h.shards = rec[2], h.shard_len = rec[3];
  return h;
}

#if NP_BOUNDS_CHECK
__device__ __forceinline__ BoundsSet bounds_of_ragged(const RaggedArgs& r, const DevTables& T, bool reconstruct) {
  BoundsSet b{};
  auto set = [&](uint32_t k, const void* p, uint64_t bytes) {
    if (!p || bytes == 0) return;
    b.lo[k] = reinterpret_cast<uint64_t>(p);
    b.hi[k] = b.lo[k] + bytes;
  };
  set(reconstruct ? kBkOut : kBkPayloads, r.data_base, r.data_size);
  set(kBkShards, r.shards_base, r.shards_size);
  set(kBkItems, r.recs, static_cast<uint64_t>(r.nitems) * sizeof(RaggedRec));
  // both arrays of the block table: the tiles follow the items in one allocation
  set(kBkBlocks, r.block_item, static_cast<uint64_t>(r.block_tile + r.nblocks - r.block_item) * 4u);
  if (reconstruct) {
    set(kBkPresent, r.present, static_cast<uint64_t>(r.nitems) * r.n);
    set(kBkRecords, r.prefix, static_cast<uint64_t>(r.nitems) * prefix_stride_c(r.n, r.k));
    set(kBkStatus, r.status, static_cast<uint64_t>(r.nitems) * 8u);
    set(kBkZeros, T.zeros, kZeroPageBytes);
  }
  return b;
}
#endif

// A ragged launch: launch(Int<K>{}) starts the kernels of r.k over the block
// table (one workgroup per entry) and returns the launch error.
template <typename F>
hipError_t with_ragged_k(const RaggedArgs& r, F launch) {
  if (r.nblocks == 0) return hipSuccess;
  if (r.nblocks > 0x7fffffffu) return hipErrorInvalidValue;
  return with_k(FastKs{}, r.k, hipErrorNotSupported, launch);
}

}  // namespace
}  // namespace np
