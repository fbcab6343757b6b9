// The per-payload decode records of the specialised decodes (kernels_fast_decode.hip,
// kernels_small.hip, kernels_res.hip): k_prefix_locator, and k_locator_records
// for caller locators, on the locator code of fast_common.hpp.
#include "fast_common.hpp"

namespace np {
namespace {

// ---------------------------------------------------------- prefix locator ----
// The v_perm tables of row multipliers E[0..rows) into the record (thread
// tid copies the rows it wrote E for: no barrier).
// Present rows get the premultiply's tables (Cantor in, tower out: in_pools),
// erased rows the postmultiply's (tower in, Cantor out: out_pools).
__device__ __forceinline__ void write_row_pools(const DevTables& T, const uint16_t* E, const uint8_t* PR,
                                                uint32_t rows, uint8_t* dst) {
  for (uint32_t v = threadIdx.x; v < rows; v += 256) {
    const uint32_t* pools = PR[v] ? T.in_pools : T.out_pools;
    const uint4* src = reinterpret_cast<const uint4*>(pools + static_cast<size_t>(NP_ICHK(*NP_BCHK(E + v, 2, kBkRecords), 65536u)) * kPoolWords);
    uint4* d = NP_BCHK(reinterpret_cast<uint4*>(dst + static_cast<size_t>(v) * 4 * kPoolWords), 4 * kPoolWords, kBkRecords);
    const uint4 a0 = src[0], a1 = src[1], a2 = src[2], a3 = src[3], a4 = src[4];
    d[0] = a0, d[1] = a1, d[2] = a2, d[3] = a3, d[4] = a4;
  }
}


// One workgroup per payload: the decode prefix (rec_tile) and the erasure
// locator folded to it (fused_locator, SURVEY F8: eval_error_polynomial
// inc_reconstruct.rs:90-113 over [0, NQ' * K)), as row multipliers EXP[loc]
// (present) / EXP[-loc] (erased).  Record: byte 0 = NQ' in {1, 2, NQ}, byte 1
// the segment occupancy, the rows' 80-byte multiplier tables from
// prefix_pools_offset (k_locator_records also leaves the u16 multipliers at
// kPrefixHeader; the decodes read only the tables).  Computed once per payload
// instead of once per column tile.
// Present rows of payload pb in [0, K), [0, 2K) and [0, N) (256 threads).
template <int K, int N>
__device__ __forceinline__ void count_present(const uint8_t* pres, int& have1, int& have2, int& have) {
  have1 = have2 = have = 0;
  for (int r = 0; r < N; r += 256) {
    const int v = static_cast<int>(threadIdx.x) + r;
    const bool p = v < N && *NP_BCHK(pres + v, 1, kBkPresent) != 0;
    if (r < K) have1 += __syncthreads_count(v < K && p);
    if (r < 2 * K) have2 += __syncthreads_count(v < 2 * K && p);
    have += __syncthreads_count(p);
  }
}

// Bit q: segment q (rows [qK, (q+1)K)) holds a present row (record byte 1:
// the decodes skip the transforms of empty segments).
template <int K, int N>
__device__ __forceinline__ uint32_t segment_occupancy(const uint8_t* pres) {
  uint32_t occ = 0;
#pragma unroll 1
  for (int q = 0; q < N / K; ++q) {
    int any = 0;
    for (int v = static_cast<int>(threadIdx.x); v < K; v += 256) any |= *NP_BCHK(pres + (q * K + v), 1, kBkPresent) != 0;
    if (__syncthreads_or(any)) occ |= 1u << q;
  }
  return occ;
}

// Status of payload pb (launchers.hpp ReconstructArgs::status); true if it
// decodes.
__device__ __forceinline__ bool write_status(const ReconstructArgs& a, uint32_t pb, int have) {
  const bool ok = have >= static_cast<int>(a.k);  // mod.rs:178-180
  if (threadIdx.x == 0 && a.status) {
    *NP_BCHK(a.status + 2 * pb, 4, kBkStatus) = ok ? 0u : kStatusNeedMoreShards;
    *NP_BCHK(a.status + 2 * pb + 1, 4, kBkStatus) = static_cast<uint32_t>(have);
  }
  return ok;
}

// Threads of k_prefix_locator for n = N rows: 512 from N = 512 on, so that
// each thread's chain of dependent loads (flag, multiplier, its 80-byte
// table) runs N / 512 times.  Config 3 (N = 1024), with the counters summed
// per wave before the LDS atomics: 256 threads 51.0 / 50.6 us per launch,
// 512 49.8 / 50.0, 1024 54.5 / 54.6 (two workgroups per CU instead of four;
// profiles/r06/prefix_threads.txt); 55.4 before the wave sums.
template <int N>
constexpr int kPrefixThreads = N >= 512 ? 512 : 256;

// NQ' = 0 marks a payload with fewer than K present rows: no decode.
template <int K, int NQ, int NT = kPrefixThreads<NQ * K>>
__global__ __launch_bounds__(NT) void k_prefix_locator(DevTables T, ReconstructArgs a, uint8_t* out) {
  constexpr int N = NQ * K;
  __shared__ uint32_t W[N];
  __shared__ uint8_t PR[N];
  const uint32_t pb = blockIdx.x, tid = threadIdx.x;
#if NP_BOUNDS_CHECK
  {
    ReconstructArgs ab = a;
    ab.prefix = out;
    bounds_arm(bounds_of(ab, T, prefix_stride_c(N, K)));
  }
#endif
  const uint8_t* pres = a.present + static_cast<size_t>(pb) * N;
  uint8_t* rec = out + static_cast<size_t>(pb) * prefix_stride_c(N, K);
  // One pass over the present flags: PR, the erasure indicator W for the
  // locator, the present rows in [0, K), [0, 2K), [0, N) and the segments
  // holding one (was count_present + segment_occupancy + the locator's own
  // load: 17 barriers fewer).
  __shared__ uint32_t acc[4];  // have1, have2, have, occupancy
  if (tid < 4) acc[tid] = 0;
  __syncthreads();
  {
    uint32_t c1 = 0, c2 = 0, c = 0, occ = 0;
    for (uint32_t v = tid; v < static_cast<uint32_t>(N); v += NT) {
      const uint8_t p = *NP_BCHK(pres + v, 1, kBkPresent);
      PR[v] = p;
      W[v] = p ? 0u : 1u;
      const uint32_t on = p ? 1u : 0u;
      c += on;
      c1 += v < static_cast<uint32_t>(K) ? on : 0u;
      c2 += v < 2u * K ? on : 0u;
      occ |= on << (v / K);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {  // wave sums first: one LDS atomic per wave and counter
      c1 += __shfl_xor(c1, o);
      c2 += __shfl_xor(c2, o);
      c += __shfl_xor(c, o);
      occ |= __shfl_xor(occ, o);
    }
    if ((tid & 63u) == 0) {
      atomicAdd(&acc[0], c1);
      atomicAdd(&acc[1], c2);
      atomicAdd(&acc[2], c);
      atomicOr(&acc[3], occ);
    }
  }
  __syncthreads();
  const int have1 = static_cast<int>(acc[0]), have2 = static_cast<int>(acc[1]), have = static_cast<int>(acc[2]);
  // All K systematic rows present: the output is those rows (the reference
  // copies received rows < k, inc_reconstruct.rs:46-50), exact for any input.
  // Otherwise the full decode from every present row, as the reference
  // (inc_reconstruct.rs:61-85); the 2K-row prefix only for trusted codewords.
  const int nq = !write_status(a, pb, have) ? 0 : have1 == K ? 1 : (a.trusted && NQ == 4 && have2 >= K) ? 2 : NQ;
  if (tid == 0) *NP_BCHK(rec, 2, kBkRecords) = static_cast<uint8_t>(nq), *NP_BCHK(rec + 1, 1, kBkRecords) = static_cast<uint8_t>(acc[3]);
  if (nq <= 1) return;
  // the row tables straight from the multipliers (the decodes read only the
  // tables, not the u16 multipliers)
  if (NQ == 4 && nq == 2) {
    fused_locator_pools<2 * K, NT>(T, W, PR, rec + prefix_pools_offset(N));  // the first 2K entries of W and PR
  } else {
    fused_locator_pools<N, NT>(T, W, PR, rec + prefix_pools_offset(N));
  }
}

// The record for caller locators (log form, all n rows: the full decode,
// NQ' = NQ): row multipliers EXP[loc] and their tables.  One workgroup per
// payload.
template <int K, int NQ>
__global__ __launch_bounds__(256) void k_locator_records(DevTables T, ReconstructArgs a, uint8_t* out) {
  constexpr int N = NQ * K;
  const uint32_t pb = blockIdx.x, tid = threadIdx.x;
#if NP_BOUNDS_CHECK
  {
    ReconstructArgs ab = a;
    ab.prefix = out;
    bounds_arm(bounds_of(ab, T, prefix_stride_c(N, K)));
  }
#endif
  const uint16_t* loc = a.locators + static_cast<size_t>(pb) * N;
  uint8_t* rec = out + static_cast<size_t>(pb) * prefix_stride_c(N, K);
  uint16_t* E = reinterpret_cast<uint16_t*>(rec + kPrefixHeader);
  int have1, have2, have;
  count_present<K, N>(a.present + static_cast<size_t>(pb) * N, have1, have2, have);
  const bool ok = write_status(a, pb, have);
  const uint32_t occ = segment_occupancy<K, N>(a.present + static_cast<size_t>(pb) * N);
  if (tid == 0) *NP_BCHK(rec, 2, kBkRecords) = static_cast<uint8_t>(ok ? NQ : 0), *NP_BCHK(rec + 1, 1, kBkRecords) = static_cast<uint8_t>(occ);
  if (!ok) return;
  // mul(x, log m) == x * EXP[m] (inc_log_mul.rs:42-49)
  for (uint32_t v = tid; v < static_cast<uint32_t>(N); v += 256) *NP_BCHK(E + v, 2, kBkRecords) = T.exp[*NP_BCHK(loc + v, 2, kBkLocators)];
  write_row_pools(T, E, a.present + static_cast<size_t>(pb) * N, N, rec + prefix_pools_offset(N));
}

// ------------------------------------------------------------- launchers ----
template <int K, int NQ>
hipError_t launch_prefix_k(const DevTables& T, const ReconstructArgs& a, uint8_t* out, hipStream_t s) {
  if (a.batch == 0) return hipSuccess;
  if (a.batch > 0x7fffffffu) return hipErrorInvalidValue;
  if (a.locators)
    k_locator_records<K, NQ><<<static_cast<uint32_t>(a.batch), 256, 0, s>>>(T, a, out);
  else
    k_prefix_locator<K, NQ><<<static_cast<uint32_t>(a.batch), kPrefixThreads<NQ * K>, 0, s>>>(T, a, out);
  return hipGetLastError();
}

}  // namespace

size_t prefix_stride(uint32_t n, uint32_t k) { return prefix_stride_c(n, k); }

// Every k of the decodes that read these records: kernels_small.hip (k <= 32),
// kernels_fast_decode.hip, kernels_res.hip (k >= 512).
hipError_t launch_prefix_locator(const DevTables& T, const ReconstructArgs& a, uint8_t* out, hipStream_t s) {
  return with_k<1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024>(a.k, hipErrorNotSupported, [&](auto kc) {
    constexpr int K = kc.value;
    return with_nq(a.n, a.k, hipErrorNotSupported,
                   [&](auto qc) { return launch_prefix_k<K, qc.value>(T, a, out, s); });
  });
}

hipError_t bounds_take_fast_records(uint32_t out[8]) { return bounds_take_tu(out); }

}  // namespace np
