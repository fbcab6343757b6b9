/*
 * novelpoly.h -- C ABI of the MI355X-native novel-polynomial-basis
 * Reed-Solomon engine (drop-in for the encode/reconstruct hot path of
 * paritytech/reed-solomon-novelpoly v2.0.0).
 *
 * Paths cited below are relative to the reference crate
 * /root/reference/reed-solomon-novelpoly/.  Every entry point names the
 * reference interface it replaces.  The reference's own FFI slot for an
 * alternative implementation is src/cxx.rs:23-31 (encode/reconstruct are
 * `unimplemented!()` there); INTEGRATION.md shows the Rust-side binding.
 *
 * Conventions
 *  - plain pointers and sizes only; every buffer is caller-owned;
 *  - host entry points take host memory; `_dev` entry points take device
 *    pointers (hipMalloc'd on the context's device) and a hipStream_t passed
 *    as `void*` and are asynchronous on that stream; NULL is HIP's legacy
 *    null stream (the caller's default stream, e.g. torch's), so work queued
 *    there before the call is ordered before it;
 *  - a context is bound to one GPU; host-API calls on one context are
 *    serialised on its own stream; distinct contexts may be used from
 *    distinct threads;
 *  - status 0 is success, 1..8 mirror `Error` in src/errors.rs:4-28 in
 *    declaration order, >= 100 are engine failures.
 */
#ifndef NOVELPOLY_H
#define NOVELPOLY_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes: src/errors.rs:4-28 ------------------------------------ */
typedef enum np_status {
  NP_OK = 0,
  NP_ERR_WANTED_SHARD_COUNT_TOO_HIGH = 1,        /* Error::WantedShardCountTooHigh(n)          */
  NP_ERR_WANTED_SHARD_COUNT_TOO_LOW = 2,         /* Error::WantedShardCountTooLow(n)           */
  NP_ERR_WANTED_PAYLOAD_SHARD_COUNT_TOO_LOW = 3, /* Error::WantedPayloadShardCountTooLow(k)    */
  NP_ERR_PAYLOAD_SIZE_IS_ZERO = 4,               /* Error::PayloadSizeIsZero                   */
  NP_ERR_NEED_MORE_SHARDS = 5,                   /* Error::NeedMoreShards{have,min,all}        */
  NP_ERR_PARAMETER_MUST_BE_POWER_OF_2 = 6,       /* Error::ParamterMustBePowerOf2{n,k}         */
  NP_ERR_INCONSISTENT_SHARD_LENGTHS = 7,         /* Error::InconsistentShardLengths{first,other}*/
  NP_ERR_EMPTY_SHARD = 8,                        /* Error::EmptyShard                          */
  NP_ERR_INVALID_ARGUMENT = 100, /* NULL pointer, too-small buffer, or a case the reference asserts on */
  NP_ERR_DEVICE = 101,           /* HIP runtime / kernel launch failure                           */
  NP_ERR_ALLOC = 102,            /* device or pinned allocation failed                            */
  NP_ERR_NO_DEVICE = 103         /* no usable gfx950 device                                       */
} np_status;

/* Error payload of the last failing call on this thread (fields as in
 * errors.rs: NeedMoreShards -> {have,min,all}; InconsistentShardLengths ->
 * {first,other,0}; WantedShardCountTooHigh/Low -> {n,0,0};
 * WantedPayloadShardCountTooLow -> {k,0,0}; ParamterMustBePowerOf2 -> {n,k,0};
 * NP_ERR_DEVICE / NP_ERR_ALLOC -> {hipError_t, call-site id, 0}: the id is the
 * engine line of the HIP call that returned the error, 0 if not recorded). */
void np_last_error_detail(size_t out[3]);
/* The HIP call behind the last NP_ERR_DEVICE / NP_ERR_ALLOC on this thread, as
 * text ("engine.cpp:<line> <call>: <hipError name>"; "" before any).  An
 * asynchronous kernel or copy fault is reported by the synchronisation that saw
 * it; with NP_SYNC_EACH set in the environment the host batch calls synchronise
 * after every step, so that the step itself is named. */
const char* np_last_error_site(void);
/* Human readable message mirroring the thiserror strings of errors.rs. */
const char* np_status_message(int status);

/* ---- parameters: src/novel_poly_basis/mod.rs:24-115, src/util.rs:1-42 ---- */
typedef struct np_code_params {
  size_t n;        /* power of two, total symbols per codeword   (CodeParams::n, mod.rs:80) */
  size_t k;        /* power of two, data symbols per codeword    (CodeParams::k, mod.rs:85) */
  size_t wanted_n; /* shards actually produced                   (CodeParams.wanted_n)      */
} np_code_params;

/* util.rs:40 recoverablity_subset_size */
size_t np_recoverability_subset_size(size_t n_wanted_shards);
/* mod.rs:43-61 CodeParams::derive_parameters */
int np_derive_parameters(size_t n_wanted, size_t k_wanted, np_code_params* out);
/* mod.rs:109-115 ReedSolomon::new validation (fails only if neither n nor k is a power of 2) */
int np_params_new(size_t n, size_t k, size_t wanted_n, np_code_params* out);
/* mod.rs:102-107 ReedSolomon::shard_len */
size_t np_shard_len(const np_code_params* params, size_t payload_size);
/* mod.rs:64-71 CodeParams::is_faster8 analogue: 1 if specialised GPU kernels serve both
   directions of (n,k) for 1 MiB payloads (fast, small, resident, huge or big kernels) */
int np_is_fast_path(const np_code_params* params);
/* The kernel families of the engine's dispatch: the generic LOG/EXP-gather
 * kernels, the small (k <= 32), fast (k = 64 .. 256), resident (k = 512 / 1024), big
 * (k = 512 .. 2048) and sub-transform ("huge", k = 2048 .. 16384) kernels.  (An enum tag only:
 * in C a typedef of this name would collide with the function below.) */
enum np_kernel_family { NP_FAMILY_GENERIC = 0, NP_FAMILY_SMALL = 1, NP_FAMILY_FAST = 2,
                        NP_FAMILY_RES = 3, NP_FAMILY_BIG = 4, NP_FAMILY_HUGE = 5 };
/* The kernel family an encode (reconstruct == 0) or a reconstruct of rows of shard_len bytes runs on
 * in this process (the NP_RES / NP_HUGE switches as read; NP_REC_RES256 per call); -1 for invalid params.
 * No device needed.  It is the dispatch's own choice (engine.cpp enc_path / rec_path), so restore,
 * verify, recover and the ragged calls, which run a reconstruct and an ordinary encode at k >= 512,
 * follow it too.  (The sub-transform kernels' pairing of narrow payloads, NP_HUGE_PAIR, is a launch
 * geometry inside one family and is not reported.) */
int np_kernel_family(const np_code_params* params, size_t shard_len, int reconstruct);

/* ---- context ------------------------------------------------------------- */
typedef struct np_ctx np_ctx;
/* Creates a context on HIP device `device` (-1 = current), uploads the field
 * tables (inc_gen_field_tables.rs:29-72) and skew factors (inc_afft.rs:386-445). */
int np_ctx_create(int device, np_ctx** out);
void np_ctx_destroy(np_ctx* ctx);
/* Checked builds only (lib/libnovelpoly_hip_chk.so, -DNP_BOUNDS_CHECK=1;
 * DESIGN.md §6): waits for the device, then returns in out[0] the number of
 * global accesses since the last call that fell outside the buffers the
 * kernels' arguments imply (error locator, prefix locator / locator records,
 * the encode and reconstruct kernels' payload, row and output accesses), and
 * in out[1..7] the first one (buffer kind, kernel
 * source line, workgroup, thread, byte offset lo/hi, width); clears them.
 * NP_ERR_INVALID_ARGUMENT in the product build. */
int np_debug_bounds_check(np_ctx* ctx, uint32_t out[8]);

/* The in-place pin registry of the host batch calls (NP_PAGEABLE=pin):
 * out[0] = page ranges registered now (0 between calls), out[1] =
 * hipHostUnregister calls the runtime refused since the process started. */
void np_pin_registry_stats(size_t out[2]);

/* The context's stream (hipStream_t as void*). */
void* np_ctx_stream(np_ctx* ctx);
int np_ctx_device(np_ctx* ctx);
/* Waits for all work queued on the context's stream and on the device's
 * legacy null stream (the `_dev` calls given a NULL stream). */
int np_ctx_synchronize(np_ctx* ctx);

/* ---- host-memory API (the crate's surface) -------------------------------- */
/* encode.rs:6-11 `encode(bytes, n_min)`: derives (n,k) from n_min like the crate.
 * shards_out: wanted_n rows of `shard_len` bytes each, row-major; shard_len must
 * equal np_shard_len(params, payload_len). */
int np_encode(np_ctx* ctx, const uint8_t* payload, size_t payload_len, size_t n_min, uint8_t* shards_out,
              size_t shard_len);
/* mod.rs:117-157 ReedSolomon::encode with explicit parameters. */
int np_rs_encode(np_ctx* ctx, const np_code_params* params, const uint8_t* payload, size_t payload_len,
                 uint8_t* shards_out, size_t shard_len);
/* reconstruct.rs:4-9 `reconstruct(received, validator_count)`.
 * shards[i] == NULL marks a missing shard; shard_lens[i] in bytes (odd lengths
 * are zero padded like WrappedShard::new, wrapped_shard.rs:33-39).
 * out receives shard_symbols*2*k bytes (payload zero padded; the caller
 * truncates, as with the crate).  *out_len is set on success. */
int np_reconstruct(np_ctx* ctx, const uint8_t* const* shards, const size_t* shard_lens, size_t n_received,
                   size_t validator_count, uint8_t* out, size_t out_capacity, size_t* out_len);
/* mod.rs:162-239 ReedSolomon::reconstruct with explicit parameters. */
int np_rs_reconstruct(np_ctx* ctx, const np_code_params* params, const uint8_t* const* shards,
                      const size_t* shard_lens, size_t n_received, uint8_t* out, size_t out_capacity,
                      size_t* out_len);
/* np_restore_shards_batch_dev for one payload in host memory:
 * shards/shard_lens/n_received as np_rs_reconstruct (same validation, same
 * errors, odd lengths zero padded).  restored: wanted_n host pointers;
 * restored[i] != NULL for an absent i receives 2*ceil(len/2) bytes;
 * restored_len is the capacity of each. */
int np_rs_restore_shards(np_ctx* ctx, const np_code_params* params, const uint8_t* const* shards,
                         const size_t* shard_lens, size_t n_received, uint8_t* const* restored,
                         size_t restored_len);
/* np_verify_shards_batch_dev for one payload in host memory, staged as
 * np_rs_restore_shards stages it: shards/shard_lens/n_received as
 * np_rs_reconstruct (same validation, same errors -- NP_ERR_NEED_MORE_SHARDS is
 * a return status here; odd lengths zero padded and compared over the padded
 * row).  *bad_rows: the number of mismatching rows; mismatch: n bytes, 1 for a
 * mismatching row, or NULL. */
int np_rs_verify_shards(np_ctx* ctx, const np_code_params* params, const uint8_t* const* shards,
                        const size_t* shard_lens, size_t n_received, size_t* bad_rows, uint8_t* mismatch);
/* np_recover_batch_dev for one payload in host memory, staged as
 * np_rs_restore_shards stages it: shards/shard_lens/n_received as
 * np_rs_reconstruct (same validation, same errors -- NP_ERR_NEED_MORE_SHARDS is
 * a return status; odd lengths zero padded).  Three output groups, each
 * optional through NULL, at least one required:
 *   out / out_capacity / out_len   the payload, as np_rs_reconstruct;
 *   restored / restored_len        the absent rows, as np_rs_restore_shards;
 *   bad_rows / mismatch            the verdict, as np_rs_verify_shards
 *                                  (mismatch needs bad_rows).
 * One staging of the rows and one decode serve all of them. */
int np_rs_recover(np_ctx* ctx, const np_code_params* params, const uint8_t* const* shards, const size_t* shard_lens,
                  size_t n_received, uint8_t* out, size_t out_capacity, size_t* out_len, uint8_t* const* restored,
                  size_t restored_len, size_t* bad_rows, uint8_t* mismatch);
/* mod.rs:247-285 ReedSolomon::reconstruct_from_systematic (first k shards, all present). */
int np_rs_reconstruct_from_systematic(np_ctx* ctx, const np_code_params* params, const uint8_t* const* chunks,
                                      const size_t* chunk_lens, size_t n_chunks, uint8_t* out,
                                      size_t out_capacity, size_t* out_len);

/* ---- device-resident batch API (what bench.py measures) ------------------- */
/* Encodes `batch` independent payloads of equal length.
 *   d_payloads: payload b at d_payloads + b*payload_stride (bytes)
 *   d_shards  : shard v of payload b at d_shards + b*batch_stride + v*shard_len
 *               (batch_stride >= wanted_n*shard_len)
 * Equivalent to calling ReedSolomon::encode (mod.rs:117-157) per payload. */
int np_encode_batch_dev(np_ctx* ctx, const np_code_params* params, const uint8_t* d_payloads,
                        size_t payload_len, size_t payload_stride, size_t batch, uint8_t* d_shards,
                        size_t batch_stride, void* stream);
/* Reconstructs `batch` payloads; every payload has its own erasure pattern.
 *   d_shards : shard v of payload b at d_shards + b*batch_stride + v*shard_len (n rows;
 *              rows of missing shards are never read)
 *   present  : HOST array, present[b*n + v] != 0 if shard v of payload b was received
 *   d_out    : payload b at d_out + b*out_stride, (shard_len/2)*2k bytes
 * Fails with NP_ERR_NEED_MORE_SHARDS (host-side check) like mod.rs:178-180. */
int np_reconstruct_batch_dev(np_ctx* ctx, const np_code_params* params, const uint8_t* d_shards,
                             size_t shard_len, size_t batch_stride, const uint8_t* present, size_t batch,
                             uint8_t* d_out, size_t out_stride, void* stream);
/* Per-payload outcome of a device batch reconstruct (device memory, one entry
 * per payload): status = NP_OK, or NP_ERR_NEED_MORE_SHARDS when the payload
 * has fewer than k present shards (mod.rs:178-180; the error's fields are
 * {have, min = k, all = n}); have = its present-shard count.  A payload marked
 * NeedMoreShards is not decoded: its output bytes are left untouched. */
typedef struct np_payload_status {
  int32_t status;
  uint32_t have;
} np_payload_status;

/* Same as np_reconstruct_batch_dev with the present mask on the device
 * (d_present: batch rows of n bytes) and optionally the erasure locators already
 * computed (d_locators: batch rows of n uint16, see np_error_locator_dev).
 * d_locators == NULL: the locators are computed on the device by a per-payload
 * kernel.  Every payload is decoded from all its present shards, as the
 * reference (inc_reconstruct.rs:61-85), or copied when its k systematic shards
 * are all present (inc_reconstruct.rs:46-50) -- bit-exact for any received
 * bytes.  d_status (device, batch entries, may be NULL) receives each
 * payload's np_payload_status; the NeedMoreShards check runs on the device. */
int np_reconstruct_batch_dev3(np_ctx* ctx, const np_code_params* params, const uint8_t* d_shards,
                              size_t shard_len, size_t batch_stride, const uint8_t* d_present,
                              const uint16_t* d_locators, size_t batch, uint8_t* d_out, size_t out_stride,
                              np_payload_status* d_status, void* stream);
/* The 0.1.0 entry: np_reconstruct_batch_dev3 with d_status = NULL (kept with
 * its original argument list, so callers built against 0.1.0 stay correct). */
int np_reconstruct_batch_dev2(np_ctx* ctx, const np_code_params* params, const uint8_t* d_shards,
                              size_t shard_len, size_t batch_stride, const uint8_t* d_present,
                              const uint16_t* d_locators, size_t batch, uint8_t* d_out, size_t out_stride,
                              void* stream);
/* OPT-IN, not crate-equivalent: for callers whose received shards are known
 * to be an unmodified codeword (e.g. verified by a Merkle proof upstream).
 * Like np_reconstruct_batch_dev3 with d_locators = NULL, but a payload whose
 * first 2k shards hold k present ones may be decoded from those 2k rows only
 * (n = 4k shapes of the fast path).  That equals the reference's output only
 * when the shards form a codeword; for other bytes the reference's decode
 * (a linear map of every present shard) differs. */
int np_reconstruct_codewords_batch_dev(np_ctx* ctx, const np_code_params* params, const uint8_t* d_shards,
                                       size_t shard_len, size_t batch_stride, const uint8_t* d_present,
                                       size_t batch, uint8_t* d_out, size_t out_stride,
                                       np_payload_status* d_status, void* stream);
/* Restores the missing shards in place (what the `reed-solomon-erasure` crate
 * calls `reconstruct`, next to its payload-only `reconstruct_data`).
 * For every payload with >= k present rows: writes each row v < wanted_n with
 * present[b*n+v] == 0 as row v of ReedSolomon::encode(ReedSolomon::reconstruct(received))
 * (mod.rs:117-157 after mod.rs:162-239), bit-exact for any received bytes.
 * No other byte of d_shards is written: present rows, rows >= wanted_n, bytes
 * between rows' end and batch_stride.  Payloads with < k present rows get
 * NP_ERR_NEED_MORE_SHARDS in d_status and are left untouched.  Layouts and
 * d_status (may be NULL) as np_reconstruct_batch_dev3; asynchronous on stream.
 * k in {64, 128, 256} (every n >= 2k): the reconstruct, then an encode that
 * stores the absent rows straight into d_shards and skips the transforms of
 * the size-k row segments that lack none.  Every other shape (k <= 32,
 * k >= 512): the reconstruct, the ordinary encode into context scratch, and a
 * copy of the absent rows.  The context keeps the decoded payloads of a slice
 * of the batch (up to 1/256 of the device's memory, 1 GiB on an MI355X; larger
 * batches run in slices); NP_ERR_ALLOC if that scratch cannot be allocated. */
int np_restore_shards_batch_dev(np_ctx* ctx, const np_code_params* params, uint8_t* d_shards, size_t shard_len,
                                size_t batch_stride, const uint8_t* d_present, size_t batch,
                                np_payload_status* d_status, void* stream);
/* Checks the received shards against their re-encoding (what the
 * `reed-solomon-erasure` crate calls `verify`, next to its `reconstruct`).
 * For a payload with >= k present rows let E = ReedSolomon::encode(
 * ReedSolomon::reconstruct(received)) (mod.rs:117-157 after mod.rs:162-239, the
 * composition np_restore_shards_batch_dev writes).  Row v MISMATCHES when
 * v < wanted_n, present[b*n+v] != 0 and the received row differs from E[v] in
 * any byte; the payload is CONSISTENT when no row mismatches.  Bit-exact with
 * the reference for any received bytes.
 *   d_bad_rows  (required) batch entries: the number of mismatching rows, or
 *               UINT32_MAX for a payload with < k present rows (== 0 never
 *               holds for an undecodable payload).
 *   d_mismatch  (may be NULL) batch rows of n bytes, laid out like d_present:
 *               1 for a mismatching row, 0 for every other entry (rows >=
 *               wanted_n included); all 0 for an undecodable payload.
 * d_shards is only read.  Layouts, validation, stream rules, d_status (may be
 * NULL), the context scratch with its slices and NP_ERR_ALLOC as
 * np_restore_shards_batch_dev.  The results do not depend on any execution
 * order: kernels set per-row flags, and the count is taken from the flags.
 * What the answer means (checked on the CPU reference over (n_wanted, k_wanted)
 * = (256,86), (600,256), (60,20), (16,8), (1024,512), (10,4);
 * tests/test_verify_cpu.py):
 *  - a present systematic row (v < k) never mismatches: the reference decode
 *    passes present data positions through unchanged, so only present rows in
 *    [k, wanted_n) are compared;
 *  - with exactly k present rows the payload is always consistent, random
 *    bytes included; with >= k+1 present rows of a codeword, changing any one
 *    symbol of a present row makes at least one row mismatch;
 *  - the map says which rows differ from the re-encoding, not which rows were
 *    corrupted: with some systematic rows absent one flipped symbol makes most
 *    present parity rows mismatch (at (16,8) the flipped row itself did not);
 *    with every systematic row present exactly the altered parity rows do.
 * k in {64, 128, 256} (every n >= 2k): the reconstruct, then an encode that
 * compares the present parity rows with d_shards as it produces them and skips
 * the transforms of segments that hold none.  Every other shape: the
 * reconstruct, the ordinary encode into context scratch, and a compare of the
 * present parity rows. */
int np_verify_shards_batch_dev(np_ctx* ctx, const np_code_params* params, const uint8_t* d_shards, size_t shard_len,
                               size_t batch_stride, const uint8_t* d_present, size_t batch, uint32_t* d_bad_rows,
                               uint8_t* d_mismatch, np_payload_status* d_status, void* stream);
/* The payload, the missing shards and the verdict from one decode: what
 * np_reconstruct_batch_dev3 (d_locators = NULL), np_restore_shards_batch_dev
 * and np_verify_shards_batch_dev give on the same received rows, each output
 * bit for bit what the separate call produces, for any received bytes.
 *   d_out / out_stride  (d_out may be NULL) the payloads, (shard_len/2)*2k bytes
 *               each at out_stride;
 *   restore     != 0: the absent rows below wanted_n are written into d_shards
 *               and no other byte of it; == 0: d_shards is only read;
 *   d_bad_rows / d_mismatch  (d_bad_rows may be NULL: no verify; d_mismatch may
 *               be NULL) as np_verify_shards_batch_dev: the present rows in
 *               [k, wanted_n) against E.  Restored rows are absent and compared
 *               rows present: the verdict is that of the received rows;
 *   d_status    (may be NULL) as in the three calls.
 * A payload with < k present rows gets NP_ERR_NEED_MORE_SHARDS in d_status,
 * UINT32_MAX in d_bad_rows and an all-zero map; its d_out bytes and its rows are
 * left untouched.  An output that was not requested is never written.
 * Validation as np_restore_shards_batch_dev, and NP_ERR_INVALID_ARGUMENT when
 * nothing is requested (d_out == NULL, restore == 0, d_bad_rows == NULL), when
 * d_mismatch comes without d_bad_rows, or when d_out comes with out_stride <
 * (shard_len/2)*2k.  batch == 0 returns NP_OK and launches nothing.
 * Asynchronous on stream.  d_out must not overlap d_shards.
 * With d_out the decode goes straight to the caller's buffer: the context then
 * keeps no payloads, and for k in {64, 128, 256} the batch is not sliced.  For
 * those k a call that restores and verifies runs one encode that stores the
 * absent rows and compares the present ones as it produces them; with one of
 * the two it runs that call's encode.  Every other shape: the ordinary encode
 * into context scratch once, then the copy and / or the compare. */
int np_recover_batch_dev(np_ctx* ctx, const np_code_params* params, uint8_t* d_shards, size_t shard_len,
                         size_t batch_stride, const uint8_t* d_present, size_t batch, uint8_t* d_out,
                         size_t out_stride, int restore, uint32_t* d_bad_rows, uint8_t* d_mismatch,
                         np_payload_status* d_status, void* stream);
/* ---- ragged device batches: one call for payloads of different lengths -----
 * One entry per payload (item).  The same array serves an encode and then the
 * reconstruct of its shards.  `items` is HOST memory, read before the call
 * returns and never referenced afterwards. */
typedef struct np_ragged_item {
  uint64_t payload_off; /* encode: payload at d_payloads + payload_off; reconstruct: output at d_out + payload_off;
                           restore / verify: ignored, not validated; recover: as reconstruct with d_out, else ignored */
  uint64_t payload_len; /* encode: bytes, > 0.  reconstruct: ignored.  restore / verify / recover: ignored, not validated */
  uint64_t shards_off;  /* row v of this item at d_shards + shards_off + v * shard_len */
  uint64_t shard_len;   /* bytes per row, even, > 0; encode: must equal np_shard_len(params, payload_len) */
} np_ragged_item;

/* Item b is np_encode_batch_dev with batch = 1 on that payload
 * (ReedSolomon::encode, mod.rs:117-157); no byte outside rows < wanted_n of an
 * item is written.  Validation, all on the host before any launch:
 * payload_len == 0 -> NP_ERR_PAYLOAD_SIZE_IS_ZERO; an odd or zero shard_len ->
 * NP_ERR_EMPTY_SHARD; NP_ERR_INVALID_ARGUMENT for a shard_len that does not
 * match payload_len, an odd shards_off, or an extent (payload_off +
 * payload_len, shards_off + wanted_n * shard_len) past payloads_size /
 * shards_size.  payload_off may be any byte offset; overlap between items is
 * the caller's business.  batch == 0 is NP_OK and launches nothing.
 * Asynchronous on `stream`; the stream is not synchronised.
 * k in {64, 128, 256} (every n >= 2k): one launch, one workgroup per item and
 * 256-column tile (np_ragged_plan).  Every other shape: maximal runs of
 * consecutive items with equal lengths and constant spacing go as one
 * np_encode_batch_dev-style launch, anything else one item per launch --
 * correct, and slow for many distinct lengths. */
int np_encode_ragged_dev(np_ctx* ctx, const np_code_params* params, const uint8_t* d_payloads, size_t payloads_size,
                         uint8_t* d_shards, size_t shards_size, const np_ragged_item* items, size_t batch,
                         void* stream);
/* Item b is np_reconstruct_batch_dev3 with d_locators = NULL and batch = 1:
 * bit-exact with the reference for any received bytes, the copy mode, the
 * NeedMoreShards handling (output left untouched) and d_status (device, batch
 * entries, may be NULL) included.  d_present: device, batch rows of n bytes.
 * Writes (shard_len / 2) * 2k bytes at d_out + payload_off and nothing else;
 * reads no absent row.  payload_len is ignored; the extents checked are
 * shards_off + n * shard_len against shards_size and payload_off +
 * (shard_len / 2) * 2k against out_size, the rest as np_encode_ragged_dev.
 * k in {64, 128, 256} with n / k in {2, 4, 8}: one launch (two for n >= 4k, as
 * the uniform call); every other shape in runs as np_encode_ragged_dev. */
int np_reconstruct_ragged_dev(np_ctx* ctx, const np_code_params* params, const uint8_t* d_shards, size_t shards_size,
                              const uint8_t* d_present, uint8_t* d_out, size_t out_size,
                              const np_ragged_item* items, size_t batch, np_payload_status* d_status, void* stream);
/* Restore and verify on a ragged buffer, with the item array that served the
 * encode.  Item b is np_restore_shards_batch_dev / np_verify_shards_batch_dev
 * with batch = 1, bit for bit, on rows d_shards + shards_off + v * shard_len,
 * presence row b of d_present (batch rows of n bytes) and entry b of d_status,
 * d_bad_rows and d_mismatch (batch rows of n bytes; it and d_status may be
 * NULL, d_bad_rows is required).  Everything those calls document carries
 * over: the restore writes only the absent rows below wanted_n of items that
 * decode, the rows of encode(reconstruct(received)), and no other byte of
 * d_shards; the verify only reads d_shards; NeedMoreShards items are left
 * untouched (UINT32_MAX and an all-zero map); d_bad_rows is counted from the
 * flags.  payload_off and payload_len are ignored and not validated.
 * Overlapping shard ranges between items are undefined for the restore.
 * Validation, all on the host before any launch and in this order: params and
 * items (an odd or zero shard_len -> NP_ERR_EMPTY_SHARD; NP_ERR_INVALID_ARGUMENT
 * for an odd shards_off or shards_off + n * shard_len past shards_size, the
 * rest as np_reconstruct_ragged_dev without the output extent); a NULL ctx ->
 * NP_ERR_INVALID_ARGUMENT; batch == 0 -> NP_OK, nothing launched; NULL
 * d_shards, d_present or (verify) d_bad_rows -> NP_ERR_INVALID_ARGUMENT.
 * Asynchronous on `stream`; the stream is not synchronised and `items` is not
 * referenced after the call returns.
 * k in {64, 128, 256} with n / k in {2, 4, 8}: per slice of the batch (the
 * decoded payloads of a slice fit the restore scratch, item boundaries) the
 * ragged reconstruct into context scratch, then the row-masked / comparing
 * encode, one workgroup per item and 256-column tile.  Every other shape:
 * maximal runs of consecutive items with equal shard_len at a constant spacing
 * go as one uniform call, anything else one item per call -- correct, and slow
 * for many distinct lengths. */
int np_restore_shards_ragged_dev(np_ctx* ctx, const np_code_params* params, uint8_t* d_shards, size_t shards_size,
                                 const uint8_t* d_present, const np_ragged_item* items, size_t batch,
                                 np_payload_status* d_status, void* stream);
int np_verify_shards_ragged_dev(np_ctx* ctx, const np_code_params* params, const uint8_t* d_shards, size_t shards_size,
                                const uint8_t* d_present, const np_ragged_item* items, size_t batch,
                                uint32_t* d_bad_rows, uint8_t* d_mismatch, np_payload_status* d_status, void* stream);
/* The payload, the missing shards and the verdict of a ragged batch from one
 * decode (0.6.0).  Item b is np_recover_batch_dev with batch = 1 on rows
 * d_shards + shards_off + v * shard_len, presence row b of d_present, output
 * d_out + payload_off ((shard_len / 2) * 2k bytes written) and entry b of
 * d_status, d_bad_rows and d_mismatch: each output bit for bit what
 * np_reconstruct_ragged_dev, np_restore_shards_ragged_dev and
 * np_verify_shards_ragged_dev give on the same received rows, for any received
 * bytes.  Everything np_recover_batch_dev documents carries over: any
 * non-empty subset of {d_out, restore, d_bad_rows (+ d_mismatch)} may be
 * requested and an output that was not requested is never written; an item
 * with < k present rows gets NP_ERR_NEED_MORE_SHARDS, UINT32_MAX and an
 * all-zero map, its d_out bytes and its rows left untouched; the verdict is
 * that of the received rows (restored rows are absent, compared rows present);
 * d_bad_rows is counted from the flags.  d_out must not overlap d_shards;
 * overlap between items' shard ranges or output ranges is undefined when the
 * restore or the verify is requested.  payload_len is ignored and never
 * validated.
 * Validation, all on the host before any launch and in this order: params and
 * items -- with d_out exactly np_reconstruct_ragged_dev's checks (payload_off
 * + (shard_len / 2) * 2k against out_size), without it exactly those of the
 * two calls above (payload_off is then ignored too); a NULL ctx ->
 * NP_ERR_INVALID_ARGUMENT; nothing requested, or d_mismatch without d_bad_rows
 * -> NP_ERR_INVALID_ARGUMENT (also at batch == 0); batch == 0 -> NP_OK,
 * nothing launched; NULL d_shards or d_present -> NP_ERR_INVALID_ARGUMENT.
 * Asynchronous on `stream`; `items` is not referenced after the call returns.
 * The payload alone is np_reconstruct_ragged_dev.  k in {64, 128, 256} with
 * n / k in {2, 4, 8}: with d_out the ragged reconstruct goes straight to the
 * caller's buffer, which the encode then reads (the context keeps no payloads;
 * a slice of the batch ends only where the per-item plan words would outgrow
 * the scratch); without it the slices are those of the two calls above.  A
 * call that restores and verifies runs one encode that stores the absent rows
 * and compares the present ones; with one of the two it runs that call's
 * encode.  Every other shape: maximal runs of consecutive items with equal
 * shard_len at constant spacings (of the shards, and with d_out of the
 * outputs) go as one np_recover_batch_dev, anything else one item per call. */
int np_recover_ragged_dev(np_ctx* ctx, const np_code_params* params, uint8_t* d_shards, size_t shards_size,
                          const uint8_t* d_present, uint8_t* d_out, size_t out_size, const np_ragged_item* items,
                          size_t batch, int restore, uint32_t* d_bad_rows, uint8_t* d_mismatch,
                          np_payload_status* d_status, void* stream);
/* Pure host code, no device needed: validates `items` exactly as the encode and
 * the reconstruct above do (reconstruct != 0: as np_reconstruct_ragged_dev, payloads_size being
 * its out_size) and returns the launch plan of the direct path: *nblocks
 * workgroups, workgroup i working on tile block_tile[i] (256 columns) of item
 * block_item[i].  Every (item, tile) occurs exactly once; all workgroups of an
 * item share i % 8 (one XCD's L2 serves the item's records and flags); items
 * are dealt longest first onto the residue with the fewest tiles so far;
 * residues that run out are padded with no-op workgroups, block_item[i] ==
 * UINT32_MAX.  block_item / block_tile may be NULL (count only); cap = their
 * capacity in entries, NP_ERR_INVALID_ARGUMENT (with *nblocks set) when it is
 * too small. */
int np_ragged_plan(const np_code_params* params, const np_ragged_item* items, size_t batch, int reconstruct,
                   size_t payloads_size, size_t shards_size, uint32_t* block_item, uint32_t* block_tile, size_t cap,
                   size_t* nblocks);

/* mod.rs:247-285 ReedSolomon::reconstruct_from_systematic for `batch` payloads
 * whose first k shards are all present: d_shards as for np_encode_batch_dev
 * (batch_stride >= k*shard_len, only rows 0..k-1 are read), d_out as for
 * np_reconstruct_batch_dev.  A transpose-gather, no field arithmetic. */
int np_reconstruct_from_systematic_batch_dev(np_ctx* ctx, const np_code_params* params, const uint8_t* d_shards,
                                             size_t shard_len, size_t batch_stride, size_t batch, uint8_t* d_out,
                                             size_t out_stride, void* stream);
/* inc_reconstruct.rs:90-113 eval_error_polynomial for `batch` erasure patterns
 * (d_present: batch rows of n bytes, nonzero = present).  Writes the first n
 * entries of each 65536-entry locator (log form) to d_locators (batch x n). */
int np_error_locator_dev(np_ctx* ctx, size_t n, const uint8_t* d_present, size_t batch, uint16_t* d_locators,
                         void* stream);

/* ---- host-memory batch API: the caller's buffers in host memory ----------
 * Same layouts as the device batch API, host pointers.  The batch is
 * pipelined over several streams in sub-batches (H2D, kernel, D2H overlap);
 * pinned host memory (hipHostMalloc / hipHostRegister) gives full overlap.
 * Reconstruct copies only the shard rows the kernels read (the k systematic
 * rows when every payload of the batch has them all, else all n rows).  Both
 * calls return when the outputs are in host memory. */
int np_encode_batch_host(np_ctx* ctx, const np_code_params* params, const uint8_t* payloads, size_t payload_len,
                         size_t payload_stride, size_t batch, uint8_t* shards, size_t batch_stride);
int np_reconstruct_batch_host(np_ctx* ctx, const np_code_params* params, const uint8_t* shards, size_t shard_len,
                              size_t batch_stride, const uint8_t* present, size_t batch, uint8_t* out,
                              size_t out_stride);
/* np_recover_batch_dev for a batch in HOST memory, pipelined like the two calls
 * above: per payload the decoded payload (out, may be NULL), the missing shards
 * (restore != 0) and the verdict (bad_rows, may be NULL; mismatch, may be NULL)
 * from one decode.  All pointers are host memory, laid out as in
 * np_recover_batch_dev: row v of payload b at shards + b*batch_stride +
 * v*shard_len, present batch x n bytes, out spaced at out_stride, bad_rows batch
 * entries, mismatch batch x n bytes, status (may be NULL) batch entries.
 * Each requested output is, bit for bit, what np_recover_batch_dev gives on the
 * same bytes, for any received bytes.  An output that was not requested is never
 * written.  In `shards` only the absent rows below wanted_n of payloads that
 * decode are written (restore != 0); no other byte of it changes -- present
 * rows, rows >= wanted_n, the gap up to batch_stride -- and absent rows are
 * never read.  The call returns when every output is in host memory.
 * Only what the answer needs crosses PCIe: in, the present rows the kernels
 * read (the k systematic rows when no verdict is asked for and every payload has
 * them all; every present row otherwise); out, the payloads, the restored rows
 * -- packed on the device, so present rows never come back -- and the counts,
 * map and statuses that were requested.
 * A payload with < k present rows: with status != NULL it gets
 * {NP_ERR_NEED_MORE_SHARDS, have}, UINT32_MAX in bad_rows and an all-zero map
 * row, its out bytes and rows stay untouched, none of its rows crosses PCIe, and
 * the call goes on and returns NP_OK.  With status == NULL the call fails up
 * front with NP_ERR_NEED_MORE_SHARDS, detail {have, k, n} of the first such
 * payload, as np_reconstruct_batch_host does, and nothing is written.
 * Validation, before the context is touched, in this order: NULL ctx
 * (NP_ERR_INVALID_ARGUMENT); the code parameters; a zero or odd shard_len
 * (NP_ERR_EMPTY_SHARD); NULL shards or present, or batch_stride < n*shard_len
 * (NP_ERR_INVALID_ARGUMENT); nothing requested, mismatch without bad_rows, or
 * out with out_stride < (shard_len/2)*2k (NP_ERR_INVALID_ARGUMENT); batch == 0
 * returns NP_OK; then the mask check above.
 * Host memory: `shards` always goes through the context's pinned staging, also
 * when the caller pinned it; this call never registers caller memory, and
 * NP_PAGEABLE=pin is not honoured here.  An `out` the caller pinned is written
 * by DMA.  NP_PIPE_SLOTS and NP_PIPE_SB (payloads per sub-batch) are read per
 * call as in np_reconstruct_batch_host.  There are no separate restore-only or
 * verify-only host batch entries: they are this call with one request. */
int np_recover_batch_host(np_ctx* ctx, const np_code_params* params, uint8_t* shards, size_t shard_len,
                          size_t batch_stride, const uint8_t* present, size_t batch, uint8_t* out, size_t out_stride,
                          int restore, uint32_t* bad_rows, uint8_t* mismatch, np_payload_status* status);

/* ---- multi-GPU: one batch over several devices ------------------------------
 * payloads are independent, so `batch` splits into contiguous
 * ranges, one per context (np_batch_split: the first batch % nctx ranges hold
 * one payload more), with no exchange between devices and no collective.  One
 * host thread per context drives its range on that context's stream; every
 * call returns when all ranges are done (the first failing status is
 * returned, its detail in np_last_error_detail).  Replaces the caller-side
 * loop over payloads (mod.rs:117-239) across GPUs. */
void np_batch_split(size_t batch, size_t ndev, size_t i, size_t* begin, size_t* count);
/* Device memory: d_payloads[i] / d_shards[i] / d_present[i] / d_out[i] /
 * d_status[i] (d_status may be NULL) are device i's buffers holding its range,
 * laid out as in np_encode_batch_dev / np_reconstruct_batch_dev3 (payload
 * np_batch_split(...).begin of the batch at index 0). */
int np_encode_batch_multi(np_ctx* const* ctxs, size_t nctx, const np_code_params* params,
                          const uint8_t* const* d_payloads, size_t payload_len, size_t payload_stride, size_t batch,
                          uint8_t* const* d_shards, size_t batch_stride);
int np_reconstruct_batch_multi(np_ctx* const* ctxs, size_t nctx, const np_code_params* params,
                               const uint8_t* const* d_shards, size_t shard_len, size_t batch_stride,
                               const uint8_t* const* d_present, size_t batch, uint8_t* const* d_out,
                               size_t out_stride, np_payload_status* const* d_status);
/* Host memory: one whole batch as in np_encode_batch_host / np_reconstruct_batch_host,
 * each device copying and computing its range. */
int np_encode_batch_host_multi(np_ctx* const* ctxs, size_t nctx, const np_code_params* params,
                               const uint8_t* payloads, size_t payload_len, size_t payload_stride, size_t batch,
                               uint8_t* shards, size_t batch_stride);
int np_reconstruct_batch_host_multi(np_ctx* const* ctxs, size_t nctx, const np_code_params* params,
                                    const uint8_t* shards, size_t shard_len, size_t batch_stride,
                                    const uint8_t* present, size_t batch, uint8_t* out, size_t out_stride);
/* np_recover_batch_dev over several contexts: d_shards[i] / d_present[i] and,
 * where requested, d_out[i] / d_bad_rows[i] / d_mismatch[i] / d_status[i] are
 * device i's buffers holding its range.  A NULL array (d_out, d_bad_rows,
 * d_mismatch, d_status) means that output is not requested; validation per
 * range as np_recover_batch_dev.  The code parameters are checked first, also
 * at batch == 0. */
int np_recover_batch_multi(np_ctx* const* ctxs, size_t nctx, const np_code_params* params, uint8_t* const* d_shards,
                           size_t shard_len, size_t batch_stride, const uint8_t* const* d_present, size_t batch,
                           uint8_t* const* d_out, size_t out_stride, int restore, uint32_t* const* d_bad_rows,
                           uint8_t* const* d_mismatch, np_payload_status* const* d_status);
/* np_recover_batch_host over several contexts: each worker takes its range of
 * the one buffer set (no caller memory is registered, so neighbouring ranges
 * share nothing).  With status == NULL the mask check runs once over the whole
 * batch before any worker starts. */
int np_recover_batch_host_multi(np_ctx* const* ctxs, size_t nctx, const np_code_params* params, uint8_t* shards,
                                size_t shard_len, size_t batch_stride, const uint8_t* present, size_t batch,
                                uint8_t* out, size_t out_stride, int restore, uint32_t* bad_rows, uint8_t* mismatch,
                                np_payload_status* status);

/* ---- low-level parity hooks (device pointers, `cols` independent columns) ----
 * data layout: column c, position i at d_data[c*size + i] (uint16, plain values). */
/* inc_afft.rs:267-332 afft */
int np_afft_dev(np_ctx* ctx, uint16_t* d_data, size_t size, size_t index, size_t cols, void* stream);
/* inc_afft.rs:139-214 inverse_afft */
int np_inverse_afft_dev(np_ctx* ctx, uint16_t* d_data, size_t size, size_t index, size_t cols, void* stream);
/* inc_log_mul.rs:92-114 walsh, in place, one transform of `size` values */
int np_walsh_dev(np_ctx* ctx, uint16_t* d_data, size_t size, void* stream);
/* inc_log_mul.rs:42-49 mul: d_out[i] = d_a[i] * EXP[d_m[i]] (log-form multiplier) */
int np_mul_dev(np_ctx* ctx, const uint16_t* d_a, const uint16_t* d_m, uint16_t* d_out, size_t count,
               void* stream);
/* inc_encode.rs:15-48 encode_low on `cols` codewords: d_data cols x k, d_codeword cols x n */
int np_encode_low_dev(np_ctx* ctx, const uint16_t* d_data, size_t k, uint16_t* d_codeword, size_t n,
                      size_t cols, void* stream);
/* inc_reconstruct.rs:61-85 decode_main on `cols` codewords sharing one erasure pattern:
 * d_codeword cols x n (in/out), d_present n bytes, d_locator n uint16 */
int np_decode_main_dev(np_ctx* ctx, uint16_t* d_codeword, size_t recover_up_to, const uint8_t* d_present,
                       const uint16_t* d_locator, size_t n, size_t cols, void* stream);

/* Engine build/version string. */
const char* np_version(void);

#ifdef __cplusplus
}
#endif
#endif /* NOVELPOLY_H */
