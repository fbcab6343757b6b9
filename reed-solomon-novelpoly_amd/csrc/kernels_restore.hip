// Restoring absent shard rows (np_restore_shards_batch_dev, engine.cpp): the
// small kernels around the encode that follows the reconstruct.
//
//  * k_restore_plan -- per payload, which rows the row-masked fast encode
//    (kernels_fast_planned.hip k_encode_masked) stores and which size-k segments hold
//    one, as bit words that kernel reads with scalar loads: one pass over the
//    n present flags per payload instead of one per column tile.
//    k_verify_plan and k_recover_plan (below) are the same pass for the verify
//    and for a call that restores and verifies (np_recover_batch_dev).
//  * k_copy_absent_rows -- every shape without a masked encode: the unchanged
//    encode writes all rows below wanted_n to a scratch shard buffer, and this
//    kernel copies the absent rows of the decoded payloads to the caller's
//    buffer (HBM to HBM, any even row address).
#include <algorithm>

#include "device_common.hpp"
#include "launchers.hpp"

namespace np {
namespace {

constexpr uint32_t kPlanThreads = 256;

// What a plan marks (PlanKind, launchers.hpp): the absent rows in [lo, hi)
// (restore), the present ones (verify), or both -- the absent rows below hi and
// the present ones in [lo, hi) -- with a second array of row words that tells
// the two apart (recover).

// One workgroup per payload: the plan that marks the rows of a decoded payload
// that KIND names.  A wave takes 64 consecutive rows at a time (one flag byte
// per lane, a ballot): two row words, and one bit of the segment words (64 rows
// never straddle a segment: k >= 64).  kPlanRecover: the row words hold the
// union, and n / 32 further words behind them the rows of the union to store.
template <PlanKind KIND>
__device__ __forceinline__ void plan_rows(const uint8_t* __restrict__ present, const uint32_t* __restrict__ status,
                                          uint32_t n, uint32_t k, uint32_t lo, uint32_t hi, size_t batch,
                                          uint32_t* __restrict__ plan) {
  __shared__ uint32_t seg[32];  // n / k <= 1024 segments
  const uint32_t pb = blockIdx.x, tid = threadIdx.x, lane = tid & 63u;
  const uint32_t segw = static_cast<uint32_t>(restore_seg_words(n, k));
  const size_t words = KIND == kPlanRecover ? recover_plan_words(n, k) : restore_plan_words(n, k);
#if NP_BOUNDS_CHECK
  {
    BoundsSet b{};
    b.lo[kBkPresent] = reinterpret_cast<uint64_t>(present);
    b.hi[kBkPresent] = b.lo[kBkPresent] + batch * n;
    b.lo[kBkStatus] = reinterpret_cast<uint64_t>(status);
    b.hi[kBkStatus] = b.lo[kBkStatus] + batch * 8;
    b.lo[kBkRecords] = reinterpret_cast<uint64_t>(plan);
    b.hi[kBkRecords] = b.lo[kBkRecords] + batch * words * 4;
    bounds_arm(b);
  }
#endif
  if (tid < 32) seg[tid] = 0;
  __syncthreads();
  const bool ok = *NP_BCHK(status + 2 * static_cast<size_t>(pb), 4, kBkStatus) == 0;
  const uint8_t* pres = present + static_cast<size_t>(pb) * n;
  uint32_t* pl = plan + static_cast<size_t>(pb) * words;
  for (uint32_t v0 = tid - lane; v0 < n; v0 += kPlanThreads) {  // n is a multiple of 64
    const uint32_t v = v0 + lane;
    bool mark, store = false;
    if constexpr (KIND == kPlanRecover) {
      const bool here = *NP_BCHK(pres + v, 1, kBkPresent) != 0;
      store = ok && v < hi && !here;
      mark = store || (ok && v >= lo && v < hi && here);
    } else {
      mark = ok && v >= lo && v < hi && (*NP_BCHK(pres + v, 1, kBkPresent) != 0) == (KIND == kPlanPresent);
    }
    const uint64_t m = __ballot(mark);
    const uint64_t ms = KIND == kPlanRecover ? __ballot(store) : 0;
    if (lane == 0) {
      *NP_BCHK(pl + segw + v0 / 32, 8, kBkRecords) = static_cast<uint32_t>(m);
      pl[segw + v0 / 32 + 1] = static_cast<uint32_t>(m >> 32);
      if constexpr (KIND == kPlanRecover) {
        *NP_BCHK(pl + segw + n / 32 + v0 / 32, 8, kBkRecords) = static_cast<uint32_t>(ms);
        pl[segw + n / 32 + v0 / 32 + 1] = static_cast<uint32_t>(ms >> 32);
      }
      if (m) atomicOr(&seg[(v0 / k) >> 5], 1u << ((v0 / k) & 31u));
    }
  }
  __syncthreads();
  if (tid < segw) *NP_BCHK(pl + tid, 4, kBkRecords) = seg[tid];
}

// The restore's plan: the absent rows below wanted_n.
__global__ __launch_bounds__(kPlanThreads) void k_restore_plan(const uint8_t* __restrict__ present,
                                                               const uint32_t* __restrict__ status, uint32_t n,
                                                               uint32_t k, uint32_t wanted_n, size_t batch,
                                                               uint32_t* __restrict__ plan) {
  plan_rows<kPlanAbsent>(present, status, n, k, 0, wanted_n, batch, plan);
}

constexpr uint32_t kCopyWaves = 4;
constexpr size_t kCopyChunk = 4096;

// One wave per 4 KiB piece of a row (as k_copy_rows, kernels_systematic.hip).
__global__ __launch_bounds__(64 * kCopyWaves) void k_copy_absent_rows(const uint8_t* __restrict__ src, size_t sstride,
                                                                     uint8_t* __restrict__ dst, size_t dstride,
                                                                     size_t row_bytes,
                                                                     const uint8_t* __restrict__ present,
                                                                     const uint32_t* __restrict__ status, uint32_t n,
                                                                     uint32_t rows, size_t count, size_t chunks,
                                                                     size_t total) {
  const uint32_t lane = threadIdx.x & 63;
#if NP_BOUNDS_CHECK
  {
    BoundsSet b{};
    b.lo[kBkPresent] = reinterpret_cast<uint64_t>(present);
    b.hi[kBkPresent] = b.lo[kBkPresent] + count * n;
    b.lo[kBkStatus] = reinterpret_cast<uint64_t>(status);
    b.hi[kBkStatus] = b.lo[kBkStatus] + count * 8;
    b.lo[kBkPayloads] = reinterpret_cast<uint64_t>(src);  // the encode's scratch rows
    b.hi[kBkPayloads] = b.lo[kBkPayloads] + (count - 1) * sstride + rows * row_bytes;
    b.lo[kBkShards] = reinterpret_cast<uint64_t>(dst);
    b.hi[kBkShards] = b.lo[kBkShards] + (count - 1) * dstride + rows * row_bytes;
    bounds_arm(b);
  }
#endif
  const size_t waves = static_cast<size_t>(gridDim.x) * kCopyWaves;
  const uintptr_t al = reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst) | sstride | dstride | row_bytes;
  const bool vec = (al & 15) == 0, vec4 = (al & 3) == 0;
  for (size_t u = static_cast<size_t>(blockIdx.x) * kCopyWaves + (threadIdx.x >> 6); u < total; u += waves) {
    const size_t r = u / chunks, ch = u - r * chunks;
    const size_t b = r / rows, v = r - b * rows;
    if (*NP_BCHK(present + (b * n + v), 1, kBkPresent) != 0 || *NP_BCHK(status + 2 * b, 4, kBkStatus) != 0) continue;
    const size_t off = ch * kCopyChunk, len = row_bytes - off < kCopyChunk ? row_bytes - off : kCopyChunk;
    const uint8_t* s = src + b * sstride + v * row_bytes + off;
    uint8_t* d = dst + b * dstride + v * row_bytes + off;
    NP_BNOTE(s, len, kBkPayloads);
    NP_BNOTE(d, len, kBkShards);
    if (vec) {
      const uint4* s4 = reinterpret_cast<const uint4*>(s);
      uint4* d4 = reinterpret_cast<uint4*>(d);
      for (size_t i = lane; i < len / 16; i += 64) d4[i] = s4[i];
    } else if (vec4) {
      const uint32_t* s1 = reinterpret_cast<const uint32_t*>(s);
      uint32_t* d1 = reinterpret_cast<uint32_t*>(d);
      for (size_t i = lane; i < len / 4; i += 64) d1[i] = s1[i];
    } else {  // rows are whole symbols at even addresses: 2-byte pieces
      const uint16_t* s1 = reinterpret_cast<const uint16_t*>(s);
      uint16_t* d1 = reinterpret_cast<uint16_t*>(d);
      for (size_t i = lane; i < len / 2; i += 64) d1[i] = s1[i];
    }
  }
}

}  // namespace

hipError_t launch_copy_absent_rows(const uint8_t* src, size_t sstride, uint8_t* dst, size_t dstride,
                                   size_t row_bytes, const uint8_t* present, const uint32_t* status, uint32_t n,
                                   uint32_t rows, size_t count, hipStream_t s) {
  const size_t chunks = (row_bytes + kCopyChunk - 1) / kCopyChunk, total = count * rows * chunks;
  if (total == 0) return hipSuccess;
  const uintptr_t al = reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst) | sstride | dstride | row_bytes;
  if (al & 1) return hipErrorInvalidValue;
  const size_t grid = std::min<size_t>((total + kCopyWaves - 1) / kCopyWaves, 8192);
  k_copy_absent_rows<<<static_cast<uint32_t>(grid), 64 * kCopyWaves, 0, s>>>(src, sstride, dst, dstride, row_bytes,
                                                                            present, status, n, rows, count, chunks,
                                                                            total);
  return hipGetLastError();
}

// ------------------------------------------------------------- verify ----
// np_verify_shards_batch_dev (engine.cpp launch_recover): the same flow with
// "present" in place of "absent" and a compare in place of the store.
//
//  * k_verify_plan -- the plan of kernels_fast_planned.hip k_encode_verify: bit v set
//    when row v is present, in [k, wanted_n), and the payload decoded.  Present
//    systematic rows never differ from the re-encoding (the decode passes
//    present data positions through), so the segment-0 bit is always clear.
//  * k_compare_present_rows -- every shape without a verify encode: the
//    unchanged encode writes all rows to scratch, and this kernel sets the flag
//    of every present row in [k, wanted_n) that differs from its scratch row.
//  * k_verify_summary -- per payload, the number of set flags (UINT32_MAX for
//    a payload that did not decode).  Flags are only ever set to 1, by whichever
//    tile or piece sees a difference, and are counted after all of them ran: the
//    count does not depend on any order.
namespace {

// The verify's plan: the present rows in [k, wanted_n).
__global__ __launch_bounds__(kPlanThreads) void k_verify_plan(const uint8_t* __restrict__ present,
                                                              const uint32_t* __restrict__ status, uint32_t n,
                                                              uint32_t k, uint32_t wanted_n, size_t batch,
                                                              uint32_t* __restrict__ plan) {
  plan_rows<kPlanPresent>(present, status, n, k, k, wanted_n, batch, plan);
}

// One wave per 4 KiB piece of a row in [k, rows) (as k_copy_absent_rows): enc
// holds the re-encoding (row_bytes per row, estride per payload), recv the
// received rows; any even address.
__global__ __launch_bounds__(64 * kCopyWaves) void k_compare_present_rows(
    const uint8_t* __restrict__ enc, size_t estride, const uint8_t* __restrict__ recv, size_t rstride,
    size_t row_bytes, const uint8_t* __restrict__ present, const uint32_t* __restrict__ status, uint32_t n, uint32_t k,
    uint32_t rows, size_t count, size_t chunks, size_t total, uint8_t* __restrict__ flags) {
  const uint32_t lane = threadIdx.x & 63;
#if NP_BOUNDS_CHECK
  {
    BoundsSet b{};
    b.lo[kBkPresent] = reinterpret_cast<uint64_t>(present);
    b.hi[kBkPresent] = b.lo[kBkPresent] + count * n;
    b.lo[kBkStatus] = reinterpret_cast<uint64_t>(status);
    b.hi[kBkStatus] = b.lo[kBkStatus] + count * 8;
    b.lo[kBkPayloads] = reinterpret_cast<uint64_t>(enc);  // the encode's scratch rows
    b.hi[kBkPayloads] = b.lo[kBkPayloads] + (count - 1) * estride + rows * row_bytes;
    b.lo[kBkShards] = reinterpret_cast<uint64_t>(recv);  // read only
    b.hi[kBkShards] = b.lo[kBkShards] + (count - 1) * rstride + rows * row_bytes;
    b.lo[kBkOut] = reinterpret_cast<uint64_t>(flags);
    b.hi[kBkOut] = b.lo[kBkOut] + count * n;
    bounds_arm(b);
  }
#endif
  const size_t waves = static_cast<size_t>(gridDim.x) * kCopyWaves;
  const uintptr_t al = reinterpret_cast<uintptr_t>(enc) | reinterpret_cast<uintptr_t>(recv) | estride | rstride | row_bytes;
  const bool vec = (al & 15) == 0, vec4 = (al & 3) == 0;
  const size_t crows = rows - k;  // rows compared per payload
  for (size_t u = static_cast<size_t>(blockIdx.x) * kCopyWaves + (threadIdx.x >> 6); u < total; u += waves) {
    const size_t r = u / chunks, ch = u - r * chunks;
    const size_t b = r / crows, v = k + (r - b * crows);
    if (*NP_BCHK(present + (b * n + v), 1, kBkPresent) == 0 || *NP_BCHK(status + 2 * b, 4, kBkStatus) != 0) continue;
    const size_t off = ch * kCopyChunk, len = row_bytes - off < kCopyChunk ? row_bytes - off : kCopyChunk;
    const uint8_t* e = enc + b * estride + v * row_bytes + off;
    const uint8_t* d = recv + b * rstride + v * row_bytes + off;
    NP_BNOTE(e, len, kBkPayloads);
    NP_BNOTE(d, len, kBkShards);
    uint32_t diff = 0;
    if (vec) {
      const uint4* e4 = reinterpret_cast<const uint4*>(e);
      const uint4* d4 = reinterpret_cast<const uint4*>(d);
      for (size_t i = lane; i < len / 16; i += 64) {
        const uint4 x = e4[i], y = d4[i];
        diff |= (x.x ^ y.x) | (x.y ^ y.y) | (x.z ^ y.z) | (x.w ^ y.w);
      }
    } else if (vec4) {
      const uint32_t* e1 = reinterpret_cast<const uint32_t*>(e);
      const uint32_t* d1 = reinterpret_cast<const uint32_t*>(d);
      for (size_t i = lane; i < len / 4; i += 64) diff |= e1[i] ^ d1[i];
    } else {  // rows are whole symbols at even addresses: 2-byte pieces
      const uint16_t* e1 = reinterpret_cast<const uint16_t*>(e);
      const uint16_t* d1 = reinterpret_cast<const uint16_t*>(d);
      for (size_t i = lane; i < len / 2; i += 64) diff |= static_cast<uint32_t>(e1[i] ^ d1[i]);
    }
    const bool any = __ballot(diff != 0) != 0;
    NP_BNOTE(flags + (b * n + v), 1, kBkOut);
    if (any && lane == 0) flags[b * n + v] = 1;
  }
}

constexpr uint32_t kSummaryThreads = 256;

// One workgroup per payload: counts[pb] = number of set flags of its n, or
// UINT32_MAX when its status is not OK.
__global__ __launch_bounds__(kSummaryThreads) void k_verify_summary(const uint8_t* __restrict__ flags,
                                                                    const uint32_t* __restrict__ status, uint32_t n,
                                                                    size_t batch, uint32_t* __restrict__ counts) {
  __shared__ uint32_t total;
  const uint32_t pb = blockIdx.x, tid = threadIdx.x;
#if NP_BOUNDS_CHECK
  {
    BoundsSet b{};
    b.lo[kBkOut] = reinterpret_cast<uint64_t>(flags);
    b.hi[kBkOut] = b.lo[kBkOut] + batch * n;
    b.lo[kBkStatus] = reinterpret_cast<uint64_t>(status);
    b.hi[kBkStatus] = b.lo[kBkStatus] + batch * 8;
    b.lo[kBkLocators] = reinterpret_cast<uint64_t>(counts);
    b.hi[kBkLocators] = b.lo[kBkLocators] + batch * 4;
    bounds_arm(b);
  }
#endif
  if (tid == 0) total = 0;
  __syncthreads();
  const uint8_t* f = flags + static_cast<size_t>(pb) * n;
  uint32_t mine = 0;
  for (uint32_t v = tid; v < n; v += kSummaryThreads) mine += *NP_BCHK(f + v, 1, kBkOut) != 0 ? 1u : 0u;
  if (mine) atomicAdd(&total, mine);  // integer sum: the same in any order
  __syncthreads();
  if (tid == 0) {
    const bool ok = *NP_BCHK(status + 2 * static_cast<size_t>(pb), 4, kBkStatus) == 0;
    *NP_BCHK(counts + pb, 4, kBkLocators) = ok ? total : 0xffffffffu;
  }
}

}  // namespace

hipError_t launch_compare_present_rows(const uint8_t* enc, size_t estride, const uint8_t* recv, size_t rstride,
                                       size_t row_bytes, const uint8_t* present, const uint32_t* status, uint32_t n,
                                       uint32_t k, uint32_t rows, size_t count, uint8_t* flags, hipStream_t s) {
  if (rows <= k) return hipSuccess;
  const size_t chunks = (row_bytes + kCopyChunk - 1) / kCopyChunk, total = count * (rows - k) * chunks;
  if (total == 0) return hipSuccess;
  const uintptr_t al = reinterpret_cast<uintptr_t>(enc) | reinterpret_cast<uintptr_t>(recv) | estride | rstride | row_bytes;
  if (al & 1) return hipErrorInvalidValue;
  const size_t grid = std::min<size_t>((total + kCopyWaves - 1) / kCopyWaves, 8192);
  k_compare_present_rows<<<static_cast<uint32_t>(grid), 64 * kCopyWaves, 0, s>>>(
      enc, estride, recv, rstride, row_bytes, present, status, n, k, rows, count, chunks, total, flags);
  return hipGetLastError();
}

hipError_t launch_verify_summary(const uint8_t* flags, const uint32_t* status, uint32_t n, size_t batch,
                                 uint32_t* counts, hipStream_t s) {
  if (batch == 0) return hipSuccess;
  if (batch > 0x7fffffffu) return hipErrorInvalidValue;
  k_verify_summary<<<static_cast<uint32_t>(batch), kSummaryThreads, 0, s>>>(flags, status, n, batch, counts);
  return hipGetLastError();
}

// ------------------------------------------------------------ recover ----
// np_recover_batch_dev with both the restore and the verify requested (engine.cpp
// launch_recover): one plan for kernels_fast_planned.hip k_encode_recover, which stores
// the absent rows below wanted_n and compares the present ones in [k, wanted_n)
// in one pass over the re-encoding.
namespace {

__global__ __launch_bounds__(kPlanThreads) void k_recover_plan(const uint8_t* __restrict__ present,
                                                               const uint32_t* __restrict__ status, uint32_t n,
                                                               uint32_t k, uint32_t wanted_n, size_t batch,
                                                               uint32_t* __restrict__ plan) {
  plan_rows<kPlanRecover>(present, status, n, k, k, wanted_n, batch, plan);
}

}  // namespace

// The plan of `kind` for each of `batch` payloads, by its kernel above.
hipError_t launch_masked_plan(PlanKind kind, const uint8_t* present, const uint32_t* status, uint32_t n, uint32_t k,
                              uint32_t wanted_n, size_t batch, uint32_t* plan, hipStream_t s) {
  if (batch == 0) return hipSuccess;
  if (batch > 0x7fffffffu || k < 64 || n % 64 != 0 || n / k > 1024) return hipErrorInvalidValue;
  const auto kernel = kind == kPlanRecover ? k_recover_plan : kind == kPlanAbsent ? k_restore_plan : k_verify_plan;
  kernel<<<static_cast<uint32_t>(batch), kPlanThreads, 0, s>>>(present, status, n, k, wanted_n, batch, plan);
  return hipGetLastError();
}

hipError_t bounds_take_restore(uint32_t out[8]) { return bounds_take_tu(out); }

}  // namespace np
