/*
 * mirsha.h — C-ABI of the MI355X (gfx950) Actions.Hash engine for MirBFT.
 *
 * This is the ONLY native boundary of the drop-in.  Plain pointers and sizes,
 * no torch / HIP types in the signatures (a hipStream_t is passed as void*).
 * It replaces the arithmetic of the reference's hash loop
 *
 *     for i, req := range actions.Hash {            // processor.go:133
 *         h := p.Hasher()                           // processor.go:134 (sha256.New)
 *         for _, data := range req.Data { h.Write(data) }   // :135-137
 *         actionResults.Digests[i] = &HashResult{Request: req, Digest: h.Sum(nil)} // :139-142
 *     }
 *
 * and the equivalent loops in ProcessorWorkPool (processor.go:312-361, whose
 * completion-order output is NOT reproduced: every entry point here returns
 * digests in ORIGIN order) and testengine's Recording (testengine/recorder.go:441-455).
 * The Go-side binding a maintainer adds is in INTEGRATION.md.
 *
 * Conventions
 *   - Return value: MIRSHA_OK (0) or a negative MIRSHA_E* code; the message is
 *     available from mirsha_last_error(ctx).  The reference converts processor
 *     failures into panics (processor.go:75,81,85,91); the Go wrapper does the same.
 *   - Digests are 32 bytes each, written to digests_out[32*i] for request i.
 *   - Host-pointer entry points are synchronous: outputs are complete on return.
 *     Device-pointer entry points (*_device) are asynchronous on the context's
 *     stream; call mirsha_sync() (or synchronise the stream) before reading.
 *   - A context is single-caller (not re-entrant), like the reference
 *     Processor (serialised by its caller, processor.go:447-449).  Each call
 *     makes the context's device current (cgo may migrate OS threads).
 */
#ifndef MIRSHA_H
#define MIRSHA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MIRSHA_OK 0
#define MIRSHA_EINVAL (-1)   /* bad argument (NULL pointer, range outside arena, ...) */
#define MIRSHA_EHIP (-2)     /* HIP runtime error */
#define MIRSHA_ENOMEM (-3)   /* device or pinned allocation failed */
#define MIRSHA_ERANGE (-4)   /* size limit exceeded (see per-function notes) */
#define MIRSHA_ENODEV (-5)   /* no usable gfx950 device */

/* Null request marker inside a digest index list: contributes an EMPTY digest
 * (0 bytes), as a null request's RequestAck.Digest does (client_tracker.go:840-847). */
#define MIRSHA_NULL_INDEX 0xFFFFFFFFu

/* Largest single message and largest arena one device launch addresses. */
#define MIRSHA_MAX_MESSAGE_BYTES 0xFFFFFF00u
#define MIRSHA_MAX_DEVICE_ARENA_BYTES 0xFFFFFF00u

typedef struct mirsha_ctx mirsha_ctx;

int mirsha_version(void); /* (major << 16) | minor */

/* Number of visible devices (hipGetDeviceCount). */
int mirsha_device_count(int* count);

/* Create / destroy a context bound to one device.  Replaces the per-request
 * `p.Hasher()` factory (processor.go:21, :58) with one long-lived engine. */
int mirsha_ctx_create(int device, mirsha_ctx** out);
void mirsha_ctx_destroy(mirsha_ctx* ctx);
const char* mirsha_last_error(const mirsha_ctx* ctx);

/* Launch on an external stream (e.g. the caller's current HIP stream) instead
 * of the context-owned one.  NULL restores the context's own stream. */
int mirsha_ctx_set_stream(mirsha_ctx* ctx, void* hip_stream);
void* mirsha_ctx_stream(mirsha_ctx* ctx);

/* Kernel form for sha256 over packed messages (A/B measurement):
 * 0 = LDS-staged coalesced loader + generated-asm rounds (default; a launch
 *     of at most 512 64-message groups takes the producer/consumer pair
 *     kernel -- schedule and rounds of each compression on two waves on two
 *     SIMDs -- and one of at most 1024 groups (one wave per SIMD) the
 *     low-occupancy kernel: prefetching direct loads, no-yield rounds;
 *     MIRSHA_AB=1 MIRSHA_PAIR=0 in the environment disables the pair forms,
 *     an A/B knob read only with MIRSHA_AB=1),
 *     A launch of 1,025..4,096 groups (at most 4 per SIMD) takes the CU-block
 *     kernel: one workgroup of 4k waves per CU, exactly k waves per SIMD,
 *     each wave's next block DMA'd into its LDS tile during this block.
 * 1 = direct per-lane loads, 4 = the low-occupancy kernel at any size,
 * 5 = the LDS kernel at any size, 6 = the pair kernel at any size,
 * 10 = the CU-block kernel at any size (groups beyond 4 per SIMD run in
 *     later workgroups, one CU at a time).
 * All of these are bit-exact.  Anything else is EINVAL: 2, 3, 7, 8 (round-1
 * A/B forms) and 11-15 (earlier and diagnostic forms of the CU-block kernel)
 * are retired: no build holds them, whatever the environment says.
 * Under MIRSHA_HASHER_SHA512_256 the request launch reads the same value:
 * 6 = the SHA-512/256 pair kernel at any size, 1 and 5 = the one-lane kernel
 * at any size, every other accepted value = automatic (the pair kernel for at
 * most mirsha_sha512_pair_max_groups() groups, else the one-lane kernel).
 * The commit launches of SHA-512/256 checkpoint chains (mirsha_chains_absorb,
 * mirsha_chains_commit*, mirsha_chains_commit_submit*) read it in the same
 * way, when the call or the ticket is queued: one lane per active chain or per
 * segment, 64 of them a group. */
int mirsha_ctx_set_variant(mirsha_ctx* ctx, int variant);

/* Per-kernel device-time accounting with HIP events bound to each timed
 * launch's own dispatch (hipExtLaunchKernel): the kernel's start and end
 * timestamps, no marker packets (an event-bound launch still costs a few us
 * of stream time, so a benchmark times a sample of its launches).
 * kernel: 0 = message kernel, 1 = digest-list (batch) kernel, 2 = generator
 * and clock probe, 3 = batch-chain kernel, 4 = fused request -> batch kernel
 * (one persistent launch per run), 5 = overlapped-cycles kernel
 * (mirsha_pipeline_overlap_device), 6 = digest compare kernel (mirsha_verify_*),
 * 7 = select kernel of the mixed ring submissions (mirsha_submit_*_expect),
 * 8 = the kernels of the device-built bucket order (mirsha_bucket_order_device,
 * MIRSHA_ORDER_DEVICE): the count and the scatter kernel, two launches per
 * built order (rocPRIM's scan between them is not timed), or the one identity
 * launch, 9 = the streams kernels (mirsha_streams_run / _run_device, and the
 * segment kernel of mirsha_streams_submit / _submit_device): one launch per
 * call that has an active stream.
 * set_timing_mask: bit k on = kernel k is timed while timing is enabled
 * (default: all). */
int mirsha_ctx_set_timing(mirsha_ctx* ctx, int enable);
int mirsha_ctx_set_timing_mask(mirsha_ctx* ctx, uint32_t mask);
int mirsha_ctx_kernel_time(mirsha_ctx* ctx, int kernel, uint64_t* launches, double* total_ms);
int mirsha_ctx_reset_timing(mirsha_ctx* ctx);

/* Wait for all work queued on the context's stream. */
int mirsha_sync(mirsha_ctx* ctx);

/* ---------------------------------------------------------------- host API */

/* processor.go:129-143 over n requests whose bytes are already concatenated:
 * request i = arena[off[i] .. off[i]+len[i]).  Any byte alignment.  Lengths
 * are bucketed by block count internally (longest first); the digest of
 * request i always lands at digests_out[32*i]. */
int mirsha_hash_batch(mirsha_ctx* ctx, const uint8_t* arena, uint64_t arena_len,
                      const uint64_t* off, const uint32_t* len, uint32_t n,
                      uint8_t* digests_out);

/* The same for HashRequest.Data [][]byte (actions.go:157-164) without a
 * caller-side copy: request i = concat(slice_ptr[s] for s in
 * [slice_first[i], slice_first[i+1])), slice_first has n+1 entries.
 * A multi-slice Write sequence hashes exactly its concatenation. */
int mirsha_hash_slices(mirsha_ctx* ctx, const uint8_t* const* slice_ptr,
                       const uint64_t* slice_len, const uint32_t* slice_first, uint32_t n,
                       uint8_t* digests_out);

/* Content-addressed dedup of one Ready() cycle.  During an
 * epoch change every node hashes the same EpochChange payload once per
 * acknowledging source (applyEpochChangeAckMsg, epoch_target.go:459-477, with
 * epochChangeHashData, stateless.go:311-340): N sources x N origins requests,
 * N distinct payloads.  Requests whose concatenated bytes are equal are hashed
 * ONCE; every duplicate still gets its own digest at digests_out[32*i], in
 * origin order (equality is confirmed byte for byte; the fingerprint only
 * groups candidates).  *n_unique_out (may be NULL) = distinct requests hashed.
 * At most MIRSHA_MAX_DEVICE_ARENA_BYTES of distinct bytes per call. */
int mirsha_hash_slices_dedup(mirsha_ctx* ctx, const uint8_t* const* slice_ptr,
                             const uint64_t* slice_len, const uint32_t* slice_first, uint32_t n,
                             uint8_t* digests_out, uint32_t* n_unique_out);

/* Host-only (no device, no context): the dedup plan the call above uses.
 * rep_out[i] = smallest j <= i whose request bytes equal request i's
 * (rep_out[i] == i for the first of each distinct content). */
int mirsha_dedup_plan(const uint8_t* const* slice_ptr, const uint64_t* slice_len,
                      const uint32_t* slice_first, uint32_t n, uint32_t* rep_out,
                      uint32_t* n_unique_out);
/* Host-only as well: where each request's digest lies among the distinct
 * requests' digests on the device, which is what
 * mirsha_submit_slices_expect_dedup sends its select kernel.  row_out[i] in
 * [0, *n_unique_out); row_out[i] == row_out[j] exactly when requests i and j
 * have equal bytes.  The distinct requests of the scan's first segment take
 * the lowest rows in origin order (they are hashed first), those found later
 * follow.  Errors as mirsha_dedup_plan. */
int mirsha_dedup_rows(const uint8_t* const* slice_ptr, const uint64_t* slice_len,
                      const uint32_t* slice_first, uint32_t n, uint32_t* row_out,
                      uint32_t* n_unique_out);

/* Page-locked host memory for the caller's request arena.  The cgo binding
 * packs each Ready() cycle's request bytes into one C arena before the call
 * (INTEGRATION.md); allocated here (once, reused every cycle) that arena is
 * DMA'd to the GPU at PCIe rate, where a malloc'ed one goes through the
 * runtime's pageable staging.  mirsha_host_free releases it. */
int mirsha_host_alloc(mirsha_ctx* ctx, uint64_t bytes, void** out);
void mirsha_host_free(void* p);

/* ---------------------------------------- asynchronous, order-preserving */
/* Replaces the hash stage of ProcessorWorkPool (processor.go:312-361,
 * 447-470) without its completion-order output: the caller
 * submits a Ready() cycle's requests, goes on with the WAL writes and network
 * sends the cycle also carries (actions.go:22-23 lets hashing run beside
 * them), then waits for the digests.
 *   mirsha_submit_slices packs the requests into the context's pinned staging
 *     before it returns (the caller may reuse the slices at once), queues the
 *     H2D copy, the kernel and the D2H copy, and returns a ticket (> 0).
 *     digests_out must stay valid until that ticket is waited for: the
 *     digests land there, in origin order, inside mirsha_wait / mirsha_poll.
 *     flags: 0 or MIRSHA_SUBMIT_DEDUP.  Up to 4 submissions are in flight;
 *     a fifth first retires the oldest.
 *   mirsha_wait blocks until every submission up to `ticket` is complete and
 *     its digests are written (submissions complete in submission order).
 *   mirsha_poll sets *done = 1 (and writes the digests) if every submission
 *     up to `ticket` is complete, else 0 without blocking. */
#define MIRSHA_SUBMIT_DEDUP 1
int mirsha_submit_slices(mirsha_ctx* ctx, const uint8_t* const* slice_ptr,
                         const uint64_t* slice_len, const uint32_t* slice_first, uint32_t n,
                         uint8_t* digests_out, int flags, uint64_t* ticket_out);
int mirsha_wait(mirsha_ctx* ctx, uint64_t ticket);
int mirsha_poll(mirsha_ctx* ctx, uint64_t ticket, int* done);
/* The same ring over a caller arena (mirsha_hash_batch's arguments): request
 * i = arena[off[i] .. off[i]+len[i]).  For the Go binding's chunked HashBatch
 * (replaces processor.go:133-143 for one Ready() cycle): the
 * caller packs chunk k+1 of the cycle into a page-locked arena
 * (mirsha_host_alloc) while chunk k, already submitted, is DMA'd, hashed and
 * its digests copied back.
 *   off / len are read before the call returns (Go memory is fine there).
 *   A page-locked arena is DMA'd straight from the caller's memory: its bytes
 *     [min off, max off+len) must not change until the ticket retires.  A
 *     pageable arena is copied into the context's staging before the call
 *     returns.
 *   digests_out: C memory, valid until the ticket retires (as
 *     mirsha_submit_slices).  A page-locked (mirsha_host_alloc) digests_out
 *     is written by the hashing kernel itself, with no copy: its rows are
 *     final when the ticket retires (mirsha_wait / mirsha_poll).
 *   At most MIRSHA_MAX_DEVICE_ARENA_BYTES of request bytes per submission
 *   (else MIRSHA_ERANGE; submit the cycle in chunks).  Shares the ring (4 in
 *   flight) and the tickets of mirsha_submit_slices: mirsha_wait / mirsha_poll. */
int mirsha_submit_batch(mirsha_ctx* ctx, const uint8_t* arena, uint64_t arena_len,
                        const uint64_t* off, const uint32_t* len, uint32_t n,
                        uint8_t* digests_out, uint64_t* ticket_out);

/* Mixed hash-and-verify cycles.  A real cycle's actions.Hash mixes all five
 * origin kinds and only VerifyRequest (state_machine.go:408-417) and
 * VerifyBatch (batch_tracker.go:139-174) carry an expected digest: these are
 * mirsha_submit_slices / mirsha_submit_batch (same argument rules, error
 * codes, messages, arena routes, ring, tickets, mirsha_wait / mirsha_poll)
 * where each request may or may not carry an expectation.  The comparison
 * runs on the device behind the hashing kernel; the caller gets a verdict, and
 * digests only where it does not already hold them.
 *   expect_of       the m indices of the requests that carry an expectation:
 *                   strictly increasing, each < n (else MIRSHA_EINVAL);
 *   expected        32 m bytes, row k = the expectation of request
 *                   expect_of[k].  Both are read before the call returns and
 *                   travel H2D with the metadata;
 *   flags           must be 0 (MIRSHA_SUBMIT_DEDUP is MIRSHA_EINVAL here: a
 *                   deduplicated cycle that carries expectations is
 *                   mirsha_submit_slices_expect_dedup, below).
 * When the ticket retires (mirsha_wait, a mirsha_poll that reports done, or a
 * later submission reusing its ring slot):
 *   bits_out        (may be NULL) ceil(n / 64) words, bit i & 63 of word
 *                   i >> 6 set exactly when request i carries an expectation
 *                   and its digest differs from it in any bit; bits at or
 *                   beyond n are 0;
 *   *n_mismatch_out (required) the number of set bits;
 *   digests_out     row i holds request i's digest for every request WITHOUT
 *                   an expectation and for every MISMATCH.  The 32 bytes of a
 *                   matching request are not written (they keep the caller's
 *                   bytes): the caller holds that digest already, it equals
 *                   its expectation.
 * digests_out, bits_out and n_mismatch_out must stay valid until then.  A
 * page-locked, 16-byte aligned digests_out receives the kept rows from the
 * select kernel itself; otherwise the kernel stores them into the context's
 * page-locked rows and exactly the kept rows are copied out at retirement.
 * Either way a matching request's digest never crosses PCIe.  A validation
 * failure queues nothing and consumes no ticket.  n == 0: a valid ticket,
 * count 0.  m == 0: the plain submission, with an all-zero bitmap.
 * mirsha_ctx_host_profile: scatter = the copy of the kept rows plus the
 * verdict.  mirsha_hash_slices_expect = submit + wait. */
int mirsha_submit_slices_expect(mirsha_ctx* ctx, const uint8_t* const* slice_ptr,
                                const uint64_t* slice_len, const uint32_t* slice_first, uint32_t n,
                                const uint32_t* expect_of, const uint8_t* expected, uint32_t m,
                                uint8_t* digests_out, uint64_t* bits_out, uint32_t* n_mismatch_out,
                                int flags, uint64_t* ticket_out);
int mirsha_submit_batch_expect(mirsha_ctx* ctx, const uint8_t* arena, uint64_t arena_len,
                               const uint64_t* off, const uint32_t* len, uint32_t n,
                               const uint32_t* expect_of, const uint8_t* expected, uint32_t m,
                               uint8_t* digests_out, uint64_t* bits_out, uint32_t* n_mismatch_out,
                               uint64_t* ticket_out);
int mirsha_hash_slices_expect(mirsha_ctx* ctx, const uint8_t* const* slice_ptr,
                              const uint64_t* slice_len, const uint32_t* slice_first, uint32_t n,
                              const uint32_t* expect_of, const uint8_t* expected, uint32_t m,
                              uint8_t* digests_out, uint64_t* bits_out, uint32_t* n_mismatch_out);
/* The epoch-change cycle in ONE ticket: mirsha_submit_slices_expect (its
 * argument rules, codes, messages, ticket and retirement) over a cycle that is
 * deduplicated as mirsha_submit_slices(MIRSHA_SUBMIT_DEDUP) deduplicates it.
 * Requests whose bytes are equal are hashed once, whether or not they carry
 * an expectation; the select kernel reads request i's digest from the row of
 * its representative (mirsha_dedup_rows) and compares it with request i's OWN
 * expectation, so verdict and kept rows are exactly those of the plain mixed
 * submission: bit i set iff request i carries an expectation and SHA-256 of
 * its bytes differs from it; row i written for every request without an
 * expectation and for every mismatch, duplicates included; a match's 32 bytes
 * untouched.  No digest is copied back for the host to fan out.
 * *n_unique_out (may be NULL) = distinct requests hashed, written before the
 * call returns.  At most MIRSHA_MAX_DEVICE_ARENA_BYTES of distinct bytes per
 * launch (the scan's first segment; the rest), as mirsha_hash_slices_dedup.
 * mirsha_ctx_host_profile: validate = the scan plus the expectation plan,
 * plan = the dedup plan plus the rows, the rest as above.
 * mirsha_hash_slices_expect_dedup = submit + wait. */
int mirsha_submit_slices_expect_dedup(mirsha_ctx* ctx, const uint8_t* const* slice_ptr,
                                      const uint64_t* slice_len, const uint32_t* slice_first,
                                      uint32_t n, const uint32_t* expect_of, const uint8_t* expected,
                                      uint32_t m, uint8_t* digests_out, uint64_t* bits_out,
                                      uint32_t* n_mismatch_out, uint32_t* n_unique_out,
                                      uint64_t* ticket_out);
int mirsha_hash_slices_expect_dedup(mirsha_ctx* ctx, const uint8_t* const* slice_ptr,
                                    const uint64_t* slice_len, const uint32_t* slice_first,
                                    uint32_t n, const uint32_t* expect_of, const uint8_t* expected,
                                    uint32_t m, uint8_t* digests_out, uint64_t* bits_out,
                                    uint32_t* n_mismatch_out, uint32_t* n_unique_out);
/* Host-only (no device, no context), like mirsha_dedup_plan: the plan the
 * calls above send to the device.  has_out: ceil(n / 64) words, bit i & 63 of
 * word i >> 6 set exactly when request i is listed in expect_of; base_out[w] =
 * set bits in words 0..w-1, so request i's row of `expected` is
 * base[i >> 6] + popcount(has[i >> 6] & ((1 << (i & 63)) - 1)).  expect_of not
 * strictly increasing, an index >= n or m > n: MIRSHA_EINVAL. */
int mirsha_expect_plan(const uint32_t* expect_of, uint32_t m, uint32_t n, uint64_t* has_out,
                       uint32_t* base_out);

/* Host-side phases (milliseconds) of the context's last host-API call.
 * Slice submissions (mirsha_submit_slices / mirsha_hash_slices_dedup):
 * validate = slice lengths (dedup: the segmented scan -- validation plus a
 * fingerprint walk or a byte comparison per request); plan = dedup plan
 * (head assignment, the remaining byte-for-byte confirmations, resolution);
 * pack = gather into pinned staging + bucket order + queueing, over every
 * launch (dedup: the first segment's distinct requests are queued before the
 * rest is scanned, later ones in a second launch); device = first launch
 * queued -> complete (H2D, kernels, D2H, overlapping the dedup scan of the
 * later segments and any time the caller spent before waiting); scatter =
 * digests copied to the caller in origin order.
 * Synchronous calls (mirsha_hash_batch / _slices / _requests_then_batches /
 * mirsha_digest_lists): validate = arguments; pack = queueing the request
 * bytes (pinned arena: one DMA; else packing into pinned chunks behind their
 * DMA); plan = the metadata block; device = queue -> synchronised; scatter =
 * digests to the caller.  Large synchronous calls are pipelined (chunked
 * H2D, kernels and D2H overlap): there pack = host time spent packing, device
 * = host time spent waiting on the device, scatter = copying digests out, and
 * the phases overlap the DMA rather than add up.  total = the whole call.
 * Asynchronous submissions (mirsha_submit_slices): every phase belongs to the
 * most recently COMPLETED ticket (published when it retires: mirsha_wait,
 * mirsha_poll, or a later submission reusing its ring slot); total = 0.
 * Writes min(n, phases) entries; returns the number of phases. */
#define MIRSHA_PROF_VALIDATE 0
#define MIRSHA_PROF_PLAN 1
#define MIRSHA_PROF_PACK 2
#define MIRSHA_PROF_DEVICE 3
#define MIRSHA_PROF_SCATTER 4
#define MIRSHA_PROF_TOTAL 5
/* not a time: H2D chunks of the last synchronous call (0 = single-shot staging) */
#define MIRSHA_PROF_CHUNKS 6
#define MIRSHA_PROF_PHASES 7
int mirsha_ctx_host_profile(const mirsha_ctx* ctx, double* ms_out, int n);

/* Request digests, then the dependent batch digests computed ON DEVICE from
 * the device-resident request digests (no host round trip):
 *   batch b = SHA-256(concat(req_digest[idx[e]] for e in [batch_first[b], batch_first[b+1])))
 * idx[e] == MIRSHA_NULL_INDEX is a null request (0 bytes).  Mirrors
 * sequence.allocate (sequence.go:154-157) and batchTracker.applyForwardBatchMsg
 * (batch_tracker.go:147-150) feeding processResults (state_machine.go:394-397). */
int mirsha_hash_requests_then_batches(mirsha_ctx* ctx, const uint8_t* arena, uint64_t arena_len,
                                      const uint64_t* off, const uint32_t* len, uint32_t n_req,
                                      const uint32_t* idx, const uint32_t* batch_first,
                                      uint32_t n_batches, uint8_t* req_digests_out,
                                      uint8_t* batch_digests_out);

/* Digest lists over caller-provided 32-byte digests (host memory): batch /
 * VerifyBatch digests over known RequestAck digests, and the testengine
 * application checkpoint value = Sum of the running hash over the digests
 * committed since the last reset (testengine/recorder.go:213-256). */
int mirsha_digest_lists(mirsha_ctx* ctx, const uint8_t* digests, uint32_t n_digests,
                        const uint32_t* idx, const uint32_t* list_first, uint32_t n_lists,
                        uint8_t* digests_out);

/* ------------------------------------------------------ verify on the device */
/* Two hash origins carry the digest they expect: VerifyRequest compares with
 * RequestAck.Digest (state_machine.go:408-417), VerifyBatch with
 * ExpectedDigest (batch_tracker.go:139-174); a mismatch is the protocol's
 * byzantine signal.  These calls hash as their mirsha_hash_* counterparts do
 * (same arguments, checks, error codes and messages, `expected` standing
 * where the digest output stood), keep the digests on the device, compare
 * them there and return only a verdict:
 *   expected        exactly 32 bytes per item (a caller holding an expectation
 *                   of another length has a mismatch without asking: Go's
 *                   bytes.Equal) -- travels H2D with the call;
 *   bits_out        ceil(n / 64) words, bit i & 63 of word i >> 6 set exactly
 *                   when item i's digest differs from expected[32 i ..] in any
 *                   bit; bits at or beyond n are 0; may be NULL when only the
 *                   count is wanted;
 *   *n_mismatch_out number of set bits.
 * Synchronous.  No digest crosses PCIe: a call moves 8 + 8 ceil(n / 64) bytes
 * device -> host (count, bitmap), where the hash call moves 32 n.  Both
 * staging routes are covered (single-shot; pipelined above 32 MiB of request
 * bytes, one compare behind the last chunk).  mirsha_ctx_host_profile keeps
 * its phases; scatter = the verdict's copy to the caller. */
int mirsha_verify_slices(mirsha_ctx* ctx, const uint8_t* const* slice_ptr, const uint64_t* slice_len,
                         const uint32_t* slice_first, uint32_t n, const uint8_t* expected,
                         uint64_t* bits_out, uint32_t* n_mismatch_out);
int mirsha_verify_batch(mirsha_ctx* ctx, const uint8_t* arena, uint64_t arena_len,
                        const uint64_t* off, const uint32_t* len, uint32_t n, const uint8_t* expected,
                        uint64_t* bits_out, uint32_t* n_mismatch_out);
/* mirsha_digest_lists' arguments (MIRSHA_NULL_INDEX entries, empty lists), one
 * expected digest per list: the VerifyBatch flow (batch_tracker.go:147-150). */
int mirsha_verify_digest_lists(mirsha_ctx* ctx, const uint8_t* digests, uint32_t n_digests,
                               const uint32_t* idx, const uint32_t* list_first, uint32_t n_lists,
                               const uint8_t* expected, uint64_t* bits_out, uint32_t* n_mismatch_out);

/* -------------------------------------------------------------- device API */
/* Compare of n device-resident 32-byte digests with n expected ones; device
 * pointers, asynchronous on the context stream.  Every word of the
 * ceil(n / 64)-word bitmap is written (layout as bits_out above) and
 * *d_count_out is reset by the call itself before the mismatches are added,
 * so repeated calls do not accumulate.  n == 0: the count is written as 0 and
 * no kernel is launched.  d_digests and d_expected must be 16-byte aligned,
 * d_bits_out 8-byte aligned (else MIRSHA_EINVAL, nothing is launched). */
int mirsha_verify_digests_device(mirsha_ctx* ctx, const uint8_t* d_digests, const uint8_t* d_expected,
                                 uint32_t n, uint64_t* d_bits_out, uint32_t* d_count_out);

/* All pointers are device pointers; asynchronous on the context stream.
 * d_off and d_len live on the device, so the library cannot reject a message
 * that overhangs the arena as the host calls do; the loaders range-check
 * instead: reads at or past arena_len rounded up to a multiple of 4 return 0;
 * up to 3 bytes behind arena_len must be readable (loads are whole 32-bit
 * words, and an overhanging message hashes those bytes as they are).  Any
 * arena size: up to MIRSHA_MAX_DEVICE_ARENA_BYTES one 32-bit buffer descriptor
 * addresses it, and there a message's off + len must stay below 2^32 (a block
 * offset that crosses 2^32 wraps to the arena's start instead of reading 0);
 * beyond that (BASELINE config 5: ~123 GB per GPU in one launch) the loader
 * switches to 64-bit per-lane addresses.  order (may be NULL) lists message
 * indices in processing order, e.g. from mirsha_bucket_order (longest first:
 * with mixed sizes this keeps the long chains off the launch's tail); NULL =
 * identity. */
int mirsha_hash_batch_device(mirsha_ctx* ctx, const uint8_t* d_arena, uint64_t arena_len,
                             const uint64_t* d_off, const uint32_t* d_len,
                             const uint32_t* d_order, uint32_t n, uint8_t* d_digests_out);

/* d_digests holds n_digests 32-byte digests (< 2^27; reads are range-checked,
 * an out-of-range index reads zeros: every index in [n_digests,
 * MIRSHA_NULL_INDEX), whatever its value, contributes 32 zero bytes, where the
 * host call rejects it).  n_entries = d_list_first[n_lists] (the
 * caller knows it; it sizes the library's scratch for lists that contain
 * MIRSHA_NULL_INDEX entries). */
int mirsha_digest_lists_device(mirsha_ctx* ctx, const uint8_t* d_digests, uint32_t n_digests,
                               const uint32_t* d_idx, const uint32_t* d_list_first, uint32_t n_lists,
                               uint32_t n_entries, uint8_t* d_digests_out);

/* -------------------------------------------- request -> batch pipeline */
/* The batch digests of a Ready() cycle form sequential SHA chains over the
 * request digests (batch b = SHA-256(d_0 || ... || d_{n-1}), sequence.go:154-157).
 * A pipeline plan overlaps the dependent pass with the request pass.  It is
 * built once from the (host) index lists and reused for every run with the
 * same shape (device API below); a plan is single-stream, like its context.
 * len (may be NULL) = request lengths, for length bucketing.
 *   MIRSHA_PIPELINE_FUSED: ONE launch.  Requests are hashed in the order in
 *     which the lists first need them, one tile wave per SIMD so tiles finish
 *     in that order; chain waves, alone on a few CUs, advance each list chunk
 *     by chunk as device-side readiness counters report the feeding request
 *     tiles done (no host round trip, no second stream).  Pays for a few long
 *     chains (VerifyBatch of hundreds of digests).
 *   MIRSHA_PIPELINE_SEQUENTIAL: request kernel at full occupancy, then the
 *     list kernel.  Best for many short lists (BatchSize 20).
 *   MIRSHA_PIPELINE_AUTO (default): FUSED when the longest list is >= 64
 *     blocks (~126 digests) and there are <= 64 list groups, else SEQUENTIAL;
 *     mirsha_pipeline_mode() reports the choice.
 * (Modes 2 and 4 -- chain segments on a second stream, and an in-kernel
 * continuation form -- were measured slower and are retired: EINVAL.)
 * mirsha_pipeline_create reads MIRSHA_PIPELINE_MODE (auto | fused |
 * sequential; default auto). */
#define MIRSHA_PIPELINE_SEQUENTIAL 0
#define MIRSHA_PIPELINE_FUSED 1
#define MIRSHA_PIPELINE_AUTO 3
/* Deprecated (round 1; kept one release so old callers still compile): the
 * retired modes.  mirsha_pipeline_create_mode returns MIRSHA_EINVAL for them. */
#define MIRSHA_PIPELINE_STREAMS 2
#define MIRSHA_PIPELINE_CONT 4
typedef struct mirsha_pipeline mirsha_pipeline;
int mirsha_pipeline_create(mirsha_ctx* ctx, uint32_t n_req, const uint32_t* len, const uint32_t* idx,
                           const uint32_t* list_first, uint32_t n_lists, mirsha_pipeline** out);
int mirsha_pipeline_create_mode(mirsha_ctx* ctx, uint32_t n_req, const uint32_t* len, const uint32_t* idx,
                                const uint32_t* list_first, uint32_t n_lists, int mode, mirsha_pipeline** out);
/* A plan carries a hasher (MIRSHA_HASHER_*, "the context's hasher" below),
 * fixed when it is created:
 *   mirsha_pipeline_create / _create_mode: SHA-256 plans; refused with
 *     MIRSHA_EINVAL under a context whose hasher is not SHA-256.
 *   mirsha_pipeline_create_hasher: a plan of `hasher`, whatever the context's
 *     hasher is now; MIRSHA_PIPELINE_MODE is not read.  An unknown hasher is
 *     MIRSHA_EINVAL with a message that names it, *out = NULL.  With
 *     MIRSHA_HASHER_SHA256 it is mirsha_pipeline_create_mode: the same
 *     validation, builds, placement probe, launches and bytes.  With
 *     MIRSHA_HASHER_SHA512_256: SEQUENTIAL is built sequential (the SHA-512/256
 *     request kernel, then a list walk over the compacted lists, one lane per
 *     list); AUTO is built SEQUENTIAL (mirsha_pipeline_mode reports it,
 *     mirsha_pipeline_fallback 0); FUSED is MIRSHA_EINVAL with a message that
 *     names the mode and the hasher, nothing allocated (no fused SHA-512/256
 *     kernel is built).  _shape / _split_tiles / _trace / _status answer as for
 *     any sequential plan.
 *   mirsha_pipeline_hasher: the plan's hasher; MIRSHA_EINVAL for NULL.
 * mirsha_hash_requests_then_batches_device and mirsha_pipeline_overlap_device
 * are served when the context's hasher equals the plan's, else refused with
 * MIRSHA_EINVAL ahead of any other effect, the message naming the call and both
 * hashers.  A SHA-512/256 plan runs through one buffer descriptor: arena_len >
 * 0xFFFFFF00 or n_req >= 2^27 is MIRSHA_ERANGE from both calls, checked on the
 * host before anything is queued (there is no 64-bit-addressed SHA-512 form).
 * Its overlapped cycle is one launch too: the workgroups of the previous
 * cycle's lists first in the grid, then this cycle's request workgroups. */
int mirsha_pipeline_create_hasher(mirsha_ctx* ctx, uint32_t n_req, const uint32_t* len, const uint32_t* idx,
                                  const uint32_t* list_first, uint32_t n_lists, int mode, int hasher,
                                  mirsha_pipeline** out);
int mirsha_pipeline_hasher(const mirsha_pipeline* p);
void mirsha_pipeline_destroy(mirsha_pipeline* p);
int mirsha_pipeline_mode(const mirsha_pipeline* p);
/* 1 if a FUSED (or AUTO -> fused) plan was built SEQUENTIAL instead because
 * the placement probe at creation found the device not dealing a
 * workgroup's waves evenly over the SIMDs (the fused launch deals its static
 * roles by SIMD; its kernel stays correct under any placement, but stacked
 * waves would run slower than the sequential plan); 0 otherwise. */
int mirsha_pipeline_fallback(const mirsha_pipeline* p);
/* Synchronises the context stream and reports a fused run whose readiness
 * watchdog expired (MIRSHA_EHIP; never expected, the launch is deadlock-free
 * by construction).  MIRSHA_OK otherwise.
 * Fail closed: a list pair whose wait expired stores no digest of its lists
 * (d_batch_out keeps its old bytes there) and sets the plan's sticky error
 * word (host-mapped memory); from then on every run on the plan
 * (mirsha_hash_requests_then_batches_device, mirsha_pipeline_overlap_device)
 * returns MIRSHA_EHIP without launching, and so does this call.  The device
 * calls are asynchronous: a run's own expiry is reported by the next call on
 * the plan or by this call after it.  Destroy the plan and create a new one.
 * (MIRSHA_AB=1 MIRSHA_TEST_FUSED_WATCHDOG=<ticks of 100 MHz> at plan creation
 * shortens the 2 s watchdog; tests only.) */
int mirsha_pipeline_status(mirsha_ctx* ctx, mirsha_pipeline* p);
/* Diagnostics of a fused plan created with MIRSHA_AB=1 MIRSHA_FUSED_TRACE=1 in the
 * environment: the last run's timeline (s_memrealtime ticks, 100 MHz) --
 * per tile [start, end, info] at [3t, 3t+1, 3t+2] (info = HW_ID | XCC_ID << 32
 * | queue << 40 | slot << 44), per readiness chunk the time its list wave
 * passed the wait at [3 n_tiles + c] and finished the chunk's blocks at
 * [3 n_tiles + n_counters + n_groups + c], per list group its end at
 * [3 n_tiles + n_counters + g].  *words = total length (0 when tracing is off). */
int mirsha_pipeline_trace(mirsha_ctx* ctx, mirsha_pipeline* p, uint64_t* out, uint64_t cap, uint64_t* words);
int mirsha_pipeline_shape(const mirsha_pipeline* p, uint32_t* n_tiles, uint32_t* n_counters, uint32_t* n_groups);
/* Deprecated (round 1's chain-segment mode, retired): kept one release so old
 * callers still link.  Every plan is one segment: *n_segments = 1 and, if
 * cap >= 1, bounds[0] = 0. */
int mirsha_pipeline_segments(const mirsha_pipeline* p, uint32_t* n_segments, uint32_t* bounds, uint32_t cap);
/* Split tiles of a fused plan: request tiles beyond the launch's tile-wave
 * slots, each run as *segments_per_tile sequential block-range segments
 * spread one per SIMD (0, 0 when none). */
int mirsha_pipeline_split_tiles(const mirsha_pipeline* p, uint32_t* n_split, uint32_t* segments_per_tile);
/* Device-resident run: request digests to d_req_out (origin order), batch
 * digests to d_batch_out; asynchronous on the context stream. */
int mirsha_hash_requests_then_batches_device(mirsha_ctx* ctx, mirsha_pipeline* p, const uint8_t* d_arena,
                                             uint64_t arena_len, const uint64_t* d_off, const uint32_t* d_len,
                                             uint8_t* d_req_out, uint8_t* d_batch_out);

/* Overlapped cycles.  The state machine batches request digests it already holds, i.e.
 * results of EARLIER Ready() cycles (sequence.go:154-157), so in a stream of
 * cycles ONE launch hashes this cycle's requests (d_arena.. -> d_req_out, origin
 * order, as mirsha_hash_requests_then_batches_device) together with the batch
 * digests of the previous cycle over ITS request digests d_prev_req (p's lists)
 * into d_prev_batch_out.  Sequential plans (many short lists, BatchSize 20):
 * the chains run beside the request tiles at full occupancy instead of in a
 * second launch of lone chain waves.  Fused plans (long VerifyBatch chains):
 * the fused launch with its list pairs reading complete digests, so they
 * never wait on tiles.  d_req_out == NULL: chains only (the last cycle's
 * flush); d_prev_req == NULL: requests only (the first cycle).  d_prev_req must stay intact until the launch ends
 * (the context stream orders it).  Asynchronous on the context stream. */
int mirsha_pipeline_overlap_device(mirsha_ctx* ctx, mirsha_pipeline* p, const uint8_t* d_arena, uint64_t arena_len,
                                   const uint64_t* d_off, const uint32_t* d_len, uint8_t* d_req_out,
                                   const uint8_t* d_prev_req, uint8_t* d_prev_batch_out);

/* Host helper: order[] = message indices sorted by SHA-256 block count,
 * longest first (stable), so a wave's 64 lanes run equal-length chains.
 * Returns 1 if the order is the identity (all lengths in one bucket), else 0. */
int mirsha_bucket_order(const uint32_t* len, uint32_t n, uint32_t* order_out);

/* The same order built on the device, from lengths that are already there: a
 * counting sort in three launches in stream order (per-wave histograms of
 * `chunk` messages each, one exclusive scan of the bin-major counts, a stable
 * scatter).  The caller knows bounds on the lengths: with blocks(L) =
 * ceil((L + 9) / 64) there are bins = blocks(max_len) - blocks(min_len) + 1
 * bins and message i's bin is clamp(blocks(max_len) - blocks(len[i]), 0,
 * bins - 1).  A length outside [min_len, max_len] therefore sorts as the
 * nearest bound and the result is a permutation of 0..n-1 whatever the
 * lengths are; when every length lies inside the bounds it equals
 * mirsha_bucket_order's output element for element.
 * At most MIRSHA_ORDER_MAX_BINS bins (a wave's histogram lives in its LDS:
 * 16 KiB, block counts spread over 256 KiB of message length). */
#define MIRSHA_ORDER_MAX_BINS 4096

/* Host-only (no context): the shape of those launches for n messages with
 * lengths in [min_len, max_len].  *bins_out as above; MIRSHA_ERANGE when it
 * exceeds MIRSHA_ORDER_MAX_BINS (the other outputs are then 0).  chunk =
 * max(1024, bins rounded up to a multiple of 64) message indices per wave,
 * n_chunks = ceil(n / chunk) waves, scratch_bytes = 8 * bins * n_chunks (the
 * counts and their scan, u32 each) <= 8 n + 65536 because chunk >= bins; the
 * scan's own temporary storage (rocPRIM's, a few KiB) is not included.
 * MIRSHA_EINVAL: min_len > max_len or a NULL output. */
int mirsha_order_plan(uint32_t n, uint32_t min_len, uint32_t max_len, uint32_t* bins_out, uint32_t* chunk_out,
                      uint32_t* n_chunks_out, uint64_t* scratch_bytes_out);

/* Queues that sort on the context's stream, with no synchronisation (device
 * pointers, as the other _device forms): d_order_out[0, n) = the bucket order
 * of d_len[0, n).  The scratch is a grow-only buffer of the context, safe
 * because every call's launches run on one stream.
 * Returns 0, or 1 when bins == 1: one launch then writes the identity, and
 * the caller may pass NULL as d_order downstream.  n == 0 is valid, queues
 * nothing and returns 1.  MIRSHA_ERANGE: more than MIRSHA_ORDER_MAX_BINS bins,
 * nothing is queued and d_order_out is untouched.  MIRSHA_EINVAL: min_len >
 * max_len, or a NULL pointer with n > 0. */
int mirsha_bucket_order_device(mirsha_ctx* ctx, const uint32_t* d_len, uint32_t n, uint32_t min_len,
                               uint32_t max_len, uint32_t* d_order_out);

/* d_off_out[i] = d_len[0] + ... + d_len[i-1] (u64; the exclusive scan the
 * gapless host routes run), device pointers, queued on the context's stream
 * with no synchronisation.  With it the chain lengths -> offsets -> order ->
 * mirsha_hash_batch_device needs no host array.  n == 0 queues nothing;
 * MIRSHA_EINVAL: a NULL pointer with n > 0. */
int mirsha_offsets_device(mirsha_ctx* ctx, const uint32_t* d_len, uint32_t n, uint64_t* d_off_out);

/* Where mirsha_submit_batch / mirsha_submit_batch_expect build the bucket
 * order of a cycle whose block counts differ.
 *   MIRSHA_ORDER_HOST (default): mirsha_bucket_order on the submitting thread,
 *     the order's 4 n bytes cross PCIe with the metadata.
 *   MIRSHA_ORDER_DEVICE: the three launches above on the context's stream,
 *     behind the arrival of the lengths and ahead of the hashing kernel, with
 *     the validation pass's exact bounds: the same order, the same digests,
 *     no sort in the caller's time and 4 n bytes less over PCIe.  A cycle of
 *     one block count has the identity order and no order launch in either
 *     mode; one whose block counts spread over more than MIRSHA_ORDER_MAX_BINS
 *     takes the host route.
 * Every other entry point (slice submissions, the synchronous calls, the
 * mirsha_multi_* forms' own contexts unless set through mirsha_multi_ctx)
 * sorts on the host in both modes.  Anything else is MIRSHA_EINVAL.
 * mirsha_ctx_order_mode returns the mode (MIRSHA_EINVAL for a NULL context). */
#define MIRSHA_ORDER_HOST 0
#define MIRSHA_ORDER_DEVICE 1
int mirsha_ctx_set_order_mode(mirsha_ctx* ctx, int mode);
int mirsha_ctx_order_mode(const mirsha_ctx* ctx);

/* ------------------------------------------------- the context's hasher */
/* The reference's hash function is configuration: `Hasher func() hash.Hash`
 * of the Processor (processor.go:21,58; used at :134 and :313).  A context
 * hashes with one of:
 *   MIRSHA_HASHER_SHA256 (default): sha256.New.  Every call, launch and byte
 *     is what it is without this setting.
 *   MIRSHA_HASHER_SHA512_256: sha512.New512_256 (FIPS 180-4 §5.3.6.2, §6.7):
 *     32-byte digests of 128-byte blocks, so every consumer of digest rows
 *     (the verify and select kernels, the ring's retirement, the dedup scan,
 *     the bucket order) works unchanged.
 * The setting applies to kernels queued by calls made after it; tickets
 * already published keep the function they were queued with.
 * Calls that honour it (same validation, messages, routes and
 * mirsha_ctx_host_profile phases): mirsha_hash_batch, mirsha_hash_slices,
 * mirsha_hash_slices_dedup, mirsha_digest_lists,
 * mirsha_hash_requests_then_batches (under SHA-512/256 always the staged
 * route, whatever MIRSHA_PIPELINE_MODE says); mirsha_verify_batch,
 * mirsha_verify_slices, mirsha_verify_digest_lists; mirsha_hash_batch_device
 * (under SHA-512/256 MIRSHA_ERANGE for an arena beyond one buffer descriptor,
 * 0xFFFFFF00 bytes, or n >= 2^27: there is no 64-bit-addressed SHA-512 form,
 * and a host call that packs more than that into one launch fails with
 * MIRSHA_EHIP), mirsha_digest_lists_device; every hashing
 * submission of the ring (mirsha_submit_slices with and without
 * MIRSHA_SUBMIT_DEDUP, mirsha_submit_batch, mirsha_submit_slices_expect,
 * mirsha_submit_batch_expect, mirsha_hash_slices_expect,
 * mirsha_submit_slices_expect_dedup, mirsha_hash_slices_expect_dedup).
 * The checkpoint chains carry a hasher of their own, fixed when they are
 * created (mirsha_chains_create_hasher): mirsha_chains_absorb / _sum /
 * _commit / _commit_device / _commit_submit / _commit_submit_device are
 * served when the context's hasher equals the chains', and refused with
 * MIRSHA_EINVAL and a message that names the call and both hashers when it
 * does not (a log that hashes with another function than the requests is a
 * misconfiguration).  A commit ticket keeps the function it was queued with.
 * The streaming hash states carry a hasher of their own in the same way
 * (mirsha_streams_create_hasher): mirsha_streams_run / _run_device / _submit /
 * _submit_device / _export / _import are served when the context's hasher
 * equals the streams', and refused with MIRSHA_EINVAL and a message that names
 * the call and both hashers when it does not.  A stream ticket keeps the
 * function it was queued with.
 * The device plans carry a hasher of their own in the same way
 * (mirsha_pipeline_create_hasher): mirsha_hash_requests_then_batches_device and
 * mirsha_pipeline_overlap_device are served when the context's hasher equals
 * the plan's, and refused with MIRSHA_EINVAL and a message that names the call
 * and both hashers when it does not.
 * Calls built for SHA-256 only refuse any other hasher at entry with
 * MIRSHA_EINVAL and a message that names the call and the hasher.  Either
 * refusal comes ahead of any other effect (state, ring and tickets stay as
 * they were; there is no silent SHA-256 and no CPU path).  SHA-256 only:
 * mirsha_pipeline_create / _create_mode (they create SHA-256 plans; a
 * SHA-512/256 plan comes from mirsha_pipeline_create_hasher, sequential form
 * only).  The mirsha_multi_* forms own their contexts, which stay SHA-256.
 * mirsha_ctx_set_hasher: MIRSHA_EINVAL for a NULL context or an unknown value
 * (processor.go:21,58). */
#define MIRSHA_HASHER_SHA256 0
#define MIRSHA_HASHER_SHA512_256 1
int mirsha_ctx_set_hasher(mirsha_ctx* ctx, int hasher);
/* The context's hasher (processor.go:21,58); MIRSHA_EINVAL for a NULL context. */
int mirsha_ctx_hasher(const mirsha_ctx* ctx);
/* Go's Size() and BlockSize() of a hasher (processor.go:21,58): 32 / 64 for
 * MIRSHA_HASHER_SHA256, 32 / 128 for MIRSHA_HASHER_SHA512_256.  Host only, no
 * context; either pointer may be NULL.  MIRSHA_EINVAL: an unknown hasher. */
int mirsha_hasher_info(int hasher, uint32_t* digest_bytes, uint32_t* block_bytes);
/* The producer/consumer pair route of MIRSHA_HASHER_SHA512_256: a request,
 * list or sequential-plan list launch of at most this many 64-lane groups
 * (256 by default, one pair per CU: the largest measured count at which the
 * pair beat the one-lane kernels) splits every compression over
 * two waves, schedule and rounds; a larger launch takes the one-lane kernels.  Bit-exact either way.  Host only,
 * no context, like mirsha_hasher_info: the threshold in force (the A/B knobs
 * MIRSHA_SHA512_PAIR=0 and MIRSHA_SHA512_PAIR_MAX_GROUPS=n move it, read only
 * with MIRSHA_AB=1). */
int mirsha_sha512_pair_max_groups(void);
/* Pair launches (request, list and plan-list kernels) queued by this context
 * since its creation.  MIRSHA_EINVAL for a NULL context or a NULL out.  The
 * commit launches of checkpoint chains take the same route by the same
 * threshold (the walk of a chain's entries on the producer's side, h and the
 * rounds on the consumer's) but are counted per chains object, not here:
 * mirsha_chains_pair_launches. */
int mirsha_ctx_sha512_pair_launches(const mirsha_ctx* ctx, uint64_t* out);

/* ------------------------------------- streaming checkpoint chains (f4) */
/* Device-resident running hash states, one per application node: the
 * testengine application's checkpoint value is Sum() of a hash into which
 * every committed request digest is written (NodeState.Commit,
 * testengine/recorder.go:213-256: ActiveHash.Write :223, Sum :244) and which
 * restarts at each checkpoint (NodeState.Set, :186-207).  That log is made
 * with the node's Hasher, so a chains object has one, fixed at creation:
 *   mirsha_chains_create: SHA-256 chains, whatever the context's hasher.
 *   mirsha_chains_create_hasher: chains of `hasher` (MIRSHA_HASHER_*; an
 *     unknown value is MIRSHA_EINVAL).  SHA-512/256 chains keep h as 8 64-bit
 *     words, up to three pending digests (four fill a 128-byte block) and the
 *     digest count.
 *   mirsha_chains_hasher: the chains' hasher; MIRSHA_EINVAL for NULL.
 *   mirsha_chains_pair_launches: commit launches of these chains (absorb, the
 *     commit calls and the commit tickets below) that took the SHA-512/256
 *     producer/consumer pair kernels, counted since creation where the launch
 *     is queued.  Always 0 for SHA-256 chains.  MIRSHA_EINVAL for a NULL
 *     argument; *out is left as it was.
 * Every hashing call on the chains (absorb, sum, the commit calls below) needs
 * a context whose hasher is the chains' own, else MIRSHA_EINVAL ahead of any
 * other effect; mirsha_chains_reset hashes nothing and is served under either.
 *   mirsha_chains_absorb: ActiveHash.Write(digest) for m 32-byte digests, in
 *     order; digest i goes to chain chain_of[i].  A null request's digest is
 *     empty and its Write changes nothing: leave it out.
 *   mirsha_chains_sum: ActiveHash.Sum(nil) of chains which[0..k) into
 *     out[32*j]; like Go's Sum it leaves the states unchanged.
 *   mirsha_chains_reset: ActiveHash = Hasher() for chains which[0..k).
 * Synchronous; chain ids < n_chains (else MIRSHA_EINVAL). */
typedef struct mirsha_chains mirsha_chains;
int mirsha_chains_create(mirsha_ctx* ctx, uint32_t n_chains, mirsha_chains** out);
int mirsha_chains_create_hasher(mirsha_ctx* ctx, uint32_t n_chains, int hasher, mirsha_chains** out);
int mirsha_chains_hasher(const mirsha_chains* chains);
int mirsha_chains_pair_launches(const mirsha_chains* chains, uint64_t* out);
void mirsha_chains_destroy(mirsha_chains* chains);
int mirsha_chains_absorb(mirsha_ctx* ctx, mirsha_chains* chains, const uint8_t* digests, const uint32_t* chain_of,
                         uint32_t m);
int mirsha_chains_sum(mirsha_ctx* ctx, mirsha_chains* chains, const uint32_t* which, uint32_t k, uint8_t* out);
int mirsha_chains_reset(mirsha_ctx* ctx, mirsha_chains* chains, const uint32_t* which, uint32_t k);

/* ------------------------------- a cycle's Commits on the chains (one call) */
/* The commit loop of Processor.Process (processor.go:145-168): every
 * committed batch is applied to the application log (p.Log.Apply, :147) and
 * at a checkpoint the log's value goes into ActionResults.Checkpoints
 * (p.Log.Snap, :163-167).  With the testengine's log that is, per node,
 * ActiveHash.Write(request.Digest) for each request of each batch
 * (testengine/recorder.go:222-223) and, at a checkpoint, ActiveHash.Sum(nil)
 * (:244) followed by a fresh hasher (NodeState.Set, :186-207).  A cycle's
 * actions.Commits is an ordered mixture of the two; here it is ONE programme
 * of n_ops ops and ONE kernel launch over the running states.
 *
 * Op i acts on chain op_chain[i] (< n_chains); ops of one chain take effect
 * in op order.  op_digest[i] is
 *   an index < n_digests: Write(digests[32*idx .. +32)); any number of ops and
 *     chains may name the same index (N nodes committing one batch), the table
 *     is uploaded once;
 *   MIRSHA_NULL_INDEX: a null request's empty digest, a Write that changes
 *     nothing (as in the digest-list calls);
 *   MIRSHA_COMMIT_CHECKPOINT: Sum, then reset; the chain goes on with the ops
 *     that follow. */
#define MIRSHA_COMMIT_CHECKPOINT 0xFFFFFFFEu
/* Checkpoint flag of a plan entry; at most this many ops and digests a call. */
#define MIRSHA_COMMIT_ENTRY_CHECKPOINT 0x80000000u

/* Host-only (no device, no context), like mirsha_dedup_plan /
 * mirsha_expect_plan: exactly the arrays mirsha_chains_commit sends to the
 * device (recorder.go:213-256 turned into per-chain programmes).
 *   act_out[k], k < *n_active_out: the chains with at least one write or
 *     checkpoint, ascending.  A chain named only by null writes is not
 *     active: the kernel neither reads nor writes it.
 *   efirst_out[0 .. n_active]: chain act_out[k] runs entries
 *     ent_out[efirst_out[k] .. efirst_out[k+1]), in op order, null writes
 *     removed; efirst_out[0] = 0, efirst_out[n_active] = *n_entries_out.
 *   ent_out[e]: a digest index (< n_digests), or
 *     MIRSHA_COMMIT_ENTRY_CHECKPOINT | row, the row of the values output the
 *     checkpoint's Sum goes to: rows count the checkpoint ops in op order
 *     across all chains (origin order).
 *   *n_values_out: the number of checkpoint ops.
 * Capacities: act_out min(n_ops, n_chains), efirst_out one more, ent_out
 * n_ops entries.  MIRSHA_EINVAL: a NULL array with a non-zero count, a chain
 * id >= n_chains, a digest index >= n_digests that is neither marker; then
 * *bad_op_out (if given) is the first offending op, or UINT32_MAX.
 * MIRSHA_ERANGE: n_ops or n_digests above MIRSHA_COMMIT_ENTRY_CHECKPOINT.
 * MIRSHA_ENOMEM: no host memory for the per-chain counters. */
int mirsha_commit_plan(const uint32_t* op_chain, const uint32_t* op_digest, uint32_t n_ops, uint32_t n_chains,
                       uint32_t n_digests, uint32_t* act_out, uint32_t* efirst_out, uint32_t* ent_out,
                       uint32_t* n_active_out, uint32_t* n_entries_out, uint32_t* n_values_out,
                       uint32_t* bad_op_out);

/* Runs the programme (processor.go:145-168, see above).  values_out gets 32
 * bytes per checkpoint op, in op order across all chains; *n_values_out is
 * their number.  Synchronous like the other mirsha_chains_* calls; the state
 * left behind (midstate, pending digest, count) is the one mirsha_chains_absorb
 * / _sum / _reset use, so the calls mix freely on one mirsha_chains.  The
 * launch is timed as kernel id 1.  A validation failure (MIRSHA_EINVAL, the
 * message names the op; chains of another device) launches nothing and leaves
 * every state untouched.  n_ops == 0: MIRSHA_OK, *n_values_out = 0. */
int mirsha_chains_commit(mirsha_ctx* ctx, mirsha_chains* chains, const uint8_t* digests, uint32_t n_digests,
                         const uint32_t* op_chain, const uint32_t* op_digest, uint32_t n_ops, uint8_t* values_out,
                         uint32_t* n_values_out);
/* The same with the digest table in device memory (16-byte aligned), e.g. the
 * d_req_out a cycle's request hashing wrote: requests -> batches -> commits
 * without the digests leaving the GPU.  The table is read on the context's
 * stream, behind whatever was queued there.  The ops are host arrays and
 * values_out is host memory, as above. */
int mirsha_chains_commit_device(mirsha_ctx* ctx, mirsha_chains* chains, const uint8_t* d_digests, uint32_t n_digests,
                                const uint32_t* op_chain, const uint32_t* op_digest, uint32_t n_ops,
                                uint8_t* values_out, uint32_t* n_values_out);

/* ------------------------------ a cycle's Commits on the asynchronous ring */
/* ProcessorWorkPool.Process starts commitInParallel beside hashInParallel and
 * collects both at the end (processor.go:447-470, :363-394).  The ring form
 * of mirsha_chains_commit does the same: the programme is queued, the call
 * returns, and the values are complete when the ticket retires.
 *
 * After a checkpoint a chain restarts from Hasher(), so the stretches of one
 * chain between checkpoints are independent hashes.  The ring form cuts each
 * active chain's entries after every checkpoint entry into SEGMENTS and runs
 * one lane per segment: a cycle's commit costs its longest stretch, not their
 * sum. */
#define MIRSHA_COMMIT_SEG_FIRST 1u /* the chain's first segment: starts from the stored state */
#define MIRSHA_COMMIT_SEG_LAST 2u  /* holds the chain's final entry: stores the state it ends in */

/* Host-only, like mirsha_commit_plan, whose output it is built on (same
 * checks, codes and *bad_op_out; ent_out, *n_active_out, *n_entries_out and
 * *n_values_out are that plan's, unchanged).  Segment s, s < *n_seg_out:
 *   seg_chain_out[s]: its chain;
 *   entries ent_out[sfirst_out[s] .. sfirst_out[s+1]), sfirst_out[0] = 0,
 *     sfirst_out[n_seg] = *n_entries_out;
 *   seg_flags_out[s]: MIRSHA_COMMIT_SEG_FIRST starts from the chain's stored
 *     midstate, pending digest and count; every other segment starts from H0
 *     with nothing pending and count 0.  MIRSHA_COMMIT_SEG_LAST stores the
 *     state it ends in as the chain's.
 * A segment ends with a checkpoint entry or with the chain's final entry: a
 * chain whose entries end with a checkpoint gets no empty segment behind it
 * (its last segment leaves Hasher()).  Segments are chain-major (chains
 * ascending), in op order within a chain.  *n_seg_out = active chains +
 * checkpoint entries that are not their chain's final entry.
 * Capacities: seg_chain_out and seg_flags_out n_ops entries, sfirst_out one
 * more, ent_out n_ops. */
int mirsha_commit_seg_plan(const uint32_t* op_chain, const uint32_t* op_digest, uint32_t n_ops, uint32_t n_chains,
                           uint32_t n_digests, uint32_t* seg_chain_out, uint32_t* sfirst_out, uint32_t* seg_flags_out,
                           uint32_t* ent_out, uint32_t* n_seg_out, uint32_t* n_active_out, uint32_t* n_entries_out,
                           uint32_t* n_values_out, uint32_t* bad_op_out);

/* mirsha_chains_commit as a ring submission: arguments, checks, error codes
 * and messages are that call's.  Before the call returns every check has run
 * on the host, *n_values_out is written, and op_chain, op_digest and the
 * (host) digest table are copied into the ring slot's page-locked block: the
 * caller may reuse them at once.  The call takes the context's next ticket and
 * ring slot like mirsha_submit_*; the ticket is retired by mirsha_wait /
 * mirsha_poll in ticket order, mixed freely with hashing tickets, and a fifth
 * submission retires the oldest.  values_out (32 bytes per checkpoint op, op
 * order) must stay valid until the ticket retires and is complete then.  A
 * validation failure queues nothing, consumes no ticket and leaves every state
 * untouched.  n_ops == 0 or null writes only: a valid ticket, nothing
 * launched.
 *
 * The device work runs on a stream of the context's own for commits (created
 * at the first such call), so the one latency-bound commit wave does not queue
 * behind the hashing kernels on the context's stream, nor they behind it (their
 * device time beside it: DESIGN.md 1.4.1, measurement c): one H2D
 * copy of the slot's block, one launch of the segment kernel (timing id 1),
 * the slot's completion event.  When a chain's first and last segment fall
 * into different waves, a device-to-device copy of the states precedes the
 * launch (the first segments read that copy; without it a last segment's store
 * could overtake the first segment's load).  The kernel stores the values
 * straight into a page-locked, 16-byte aligned values_out, otherwise into
 * page-locked rows of the slot that are copied out at retirement: there is no
 * D2H copy.  Commit submissions run in submission order.  The synchronous
 * mirsha_chains_absorb / _sum / _reset / _commit on an object with a commit in
 * flight first make the context's stream wait for it, so both forms mix on
 * one object without the caller waiting; mirsha_chains_destroy waits for the
 * object's last queued commit.  mirsha_ctx_host_profile of a retired commit
 * ticket: validate = checks and plan, pack = the staging copy, device = queued
 * -> complete, scatter = the values' copy. */
int mirsha_chains_commit_submit(mirsha_ctx* ctx, mirsha_chains* chains, const uint8_t* digests, uint32_t n_digests,
                                const uint32_t* op_chain, const uint32_t* op_digest, uint32_t n_ops,
                                uint8_t* values_out, uint32_t* n_values_out, uint64_t* ticket_out);
/* The same with the table in device memory (16-byte aligned).  The commit
 * stream waits on an event recorded on the context's stream at submission, so
 * the table is read behind whatever was queued there (e.g. the hashing that
 * writes it); it must stay intact until the ticket retires. */
int mirsha_chains_commit_submit_device(mirsha_ctx* ctx, mirsha_chains* chains, const uint8_t* d_digests,
                                       uint32_t n_digests, const uint32_t* op_chain, const uint32_t* op_digest,
                                       uint32_t n_ops, uint8_t* values_out, uint32_t* n_values_out,
                                       uint64_t* ticket_out);

/* ------------------------- streaming hash states: Write / Sum / Reset (a2) */
/* The reference's hashing boundary is `type Hasher func() hash.Hash`
 * (processor.go:21): Write any bytes any number of times, Sum(nil) at any
 * point without disturbing the state, Reset.  Its application log is
 * application-defined: Log.Apply(*pb.QEntry) and Log.Snap (processor.go:28-31)
 * may cover sequence numbers, payloads or a serialised entry, not only whole
 * 32-byte digests as the chains above.  A mirsha_streams holds n_streams such
 * states on the device, kept across calls: the midstate h[8], the up to 63
 * bytes of the unfinished block, and the total byte count (u64, so the padded
 * bit length is 64-bit).  Every stream starts as Hasher().
 *
 * A hash.Hash is made by the node's Hasher, so a streams object has one, fixed
 * at creation, as the chains have:
 *   mirsha_streams_create: SHA-256 streams, whatever the context's hasher.
 *   mirsha_streams_create_hasher: streams of `hasher` (MIRSHA_HASHER_*; an
 *     unknown value is MIRSHA_EINVAL).  SHA-512/256 streams keep h as 8 64-bit
 *     words, the up to 127 bytes of the unfinished 128-byte block and the byte
 *     count (u64; the padded bit length is 128-bit, FIPS 180-4: above 2^61
 *     bytes Go's crypto/sha512 leaves its high 64 bits zero, this does not).
 *   mirsha_streams_hasher: the streams' hasher; MIRSHA_EINVAL for NULL.
 * The six calls below that run, queue, export or import need a context whose
 * hasher is the streams' own, else MIRSHA_EINVAL ahead of any other effect
 * (the states and the ring stay as they were; the same object is served again
 * once the context is set back).
 *
 * One call runs ONE programme of n_ops ops in ONE kernel launch (timing id
 * 9), one lane per active stream.  Op i acts on stream op_stream[i]
 * (< n_streams); ops of one stream take effect in op order, streams are
 * independent.  op_kind[i] is one of the kinds below; op_off[i] / op_len[i]
 * name the bytes of a WRITE (any byte alignment, any length) and are ignored
 * for every other kind. */
typedef struct mirsha_streams mirsha_streams;
int mirsha_streams_create(mirsha_ctx* ctx, uint32_t n_streams, mirsha_streams** out);
int mirsha_streams_create_hasher(mirsha_ctx* ctx, uint32_t n_streams, int hasher, mirsha_streams** out);
int mirsha_streams_hasher(const mirsha_streams* streams);
void mirsha_streams_destroy(mirsha_streams* streams);

#define MIRSHA_STREAM_WRITE 0u     /* Write(arena[op_off[i] .. op_off[i]+op_len[i])) */
#define MIRSHA_STREAM_SUM 1u       /* Sum(nil) -> next row of values_out; state unchanged (Go's Sum) */
#define MIRSHA_STREAM_SUM_RESET 2u /* Sum(nil), then Reset() (a checkpoint) */
#define MIRSHA_STREAM_RESET 3u
/* At most this many ops a call (a plan entry keeps its kind in 2 bits beside its value row). */
#define MIRSHA_STREAM_MAX_OPS 0x3FFFFFFFu
/* Bytes of one exported state (mirsha_streams_export) of SHA-256 streams, and
 * of SHA-512/256 streams. */
#define MIRSHA_STREAM_STATE_BYTES 108u
#define MIRSHA_STREAM_STATE_BYTES_SHA512 204u
/* The same by hasher: 108 for MIRSHA_HASHER_SHA256, 204 for
 * MIRSHA_HASHER_SHA512_256.  Host only, no context, like mirsha_hasher_info;
 * bytes_out may be NULL.  MIRSHA_EINVAL: an unknown hasher. */
int mirsha_stream_state_bytes(int hasher, uint32_t* bytes_out);

/* Host-only (no device, no context), with the role mirsha_commit_plan has for
 * the chains: exactly the arrays mirsha_streams_run* sends to the device.
 *   act_out[k], k < *n_active_out: the streams with at least one entry,
 *     ascending.  A zero-length write changes nothing and is dropped; a stream
 *     named only by such writes is not active: the kernel neither reads nor
 *     writes it.
 *   efirst_out[0 .. n_active]: stream act_out[k] runs entries
 *     [efirst_out[k], efirst_out[k+1]) in op order.
 *   ent_kind_out[e]: the kind in bits 0-1; for SUM / SUM_RESET the row of the
 *     values output above them: rows count those ops in op order across all
 *     streams.  ent_off_out[e] / ent_len_out[e]: the bytes of a WRITE entry
 *     (0 / 0 for every other kind).  pack == 0: the op's own offset (what
 *     mirsha_streams_run_device sends).  pack != 0: the offset of its bytes
 *     among the call's packed bytes (what mirsha_streams_run sends, with
 *     exactly those bytes): every distinct range (op_off, op_len) once, in the
 *     order of its first entry, without gaps; entries that name one range
 *     share its bytes (N nodes applying the same log entry).
 *   *n_values_out: the number of SUM / SUM_RESET ops; *n_bytes_out: pack == 0
 *     the bytes the write entries name, else the packed bytes.
 * (On the device the three entry arrays travel as one 16-byte record per
 * entry: kind, length, offset.)
 * Capacities: act_out min(n_ops, n_streams), efirst_out one more, the entry
 * arrays n_ops.  MIRSHA_EINVAL: a NULL array with a non-zero count, a stream
 * id >= n_streams, an unknown kind, a write with op_off + op_len > arena_len;
 * then *bad_op_out (if given) is the first offending op, or UINT32_MAX.
 * MIRSHA_ERANGE: n_ops above MIRSHA_STREAM_MAX_OPS.  MIRSHA_ENOMEM: no host
 * memory for the per-stream counters. */
int mirsha_stream_plan(const uint32_t* op_stream, const uint32_t* op_kind, const uint64_t* op_off,
                       const uint32_t* op_len, uint32_t n_ops, uint32_t n_streams, uint64_t arena_len, int pack,
                       uint32_t* act_out, uint32_t* efirst_out, uint32_t* ent_kind_out, uint64_t* ent_off_out,
                       uint32_t* ent_len_out, uint32_t* n_active_out, uint32_t* n_entries_out, uint32_t* n_values_out,
                       uint64_t* n_bytes_out, uint32_t* bad_op_out);

/* Runs the programme: one plan, one launch, one synchronisation; synchronous
 * like mirsha_chains_*.  values_out gets 32 bytes per SUM / SUM_RESET op, in
 * op order across all streams; *n_values_out is their number.  `arena` is host
 * memory of any kind (Go memory is fine) and may be sparse: only the bytes the
 * write ops name cross PCIe, each distinct range once, packed into page-locked
 * staging of the object with the offsets rewritten (mirsha_stream_plan,
 * pack).  At most
 * MIRSHA_MAX_DEVICE_ARENA_BYTES - 256 written bytes a call, else
 * MIRSHA_ERANGE.  Every check runs on the host before anything is queued:
 * MIRSHA_EINVAL (the message names the op) for a stream id >= n_streams, an
 * unknown kind, op_off + op_len > arena_len, or streams of another device; a
 * failing call leaves every state untouched.  n_ops == 0: MIRSHA_OK,
 * *n_values_out = 0. */
int mirsha_streams_run(mirsha_ctx* ctx, mirsha_streams* streams, const uint8_t* arena, uint64_t arena_len,
                       const uint32_t* op_stream, const uint32_t* op_kind, const uint64_t* op_off,
                       const uint32_t* op_len, uint32_t n_ops, uint8_t* values_out, uint32_t* n_values_out);
/* The same with the arena in device memory (any alignment), read where it lies
 * on the context's stream, behind whatever was queued there; arena_len at most
 * MIRSHA_MAX_DEVICE_ARENA_BYTES.  The kernel reads whole aligned 4-byte words:
 * up to 3 bytes on either side of the arena that share a word with it are
 * loaded and masked out.  The ops are host arrays and values_out is host
 * memory, as above. */
int mirsha_streams_run_device(mirsha_ctx* ctx, mirsha_streams* streams, const uint8_t* d_arena, uint64_t arena_len,
                              const uint32_t* op_stream, const uint32_t* op_kind, const uint64_t* op_off,
                              const uint32_t* op_len, uint32_t n_ops, uint8_t* values_out, uint32_t* n_values_out);

/* The states of streams which[0..k) as MIRSHA_STREAM_STATE_BYTES (108) bytes
 * each, in the layout of Go 1.14's crypto/sha256 MarshalBinary: the magic
 * "sha\x03", h[0..7] as big-endian u32, the buffered bytes zero-padded to 64,
 * the total length as big-endian u64.  With no Go toolchain at hand this
 * layout is pinned by that description only, not by a round trip through Go.
 * SHA-512/256 streams: MIRSHA_STREAM_STATE_BYTES_SHA512 (204) bytes each, Go
 * 1.14's crypto/sha512 MarshalBinary for New512_256: the magic "sha\x06",
 * h[0..7] as big-endian u64, the buffered bytes zero-padded to 128, the total
 * length as big-endian u64; pinned by this description only, in the same way.
 * _import sets the states from such rows (fill = length mod the block size) and
 * rejects a wrong magic (MIRSHA_EINVAL, the message names the row; nothing is
 * changed): a "sha\x03" row offered to SHA-512/256 streams is one, and so is a
 * "sha\x06" row offered to SHA-256 streams.
 * Synchronous; MIRSHA_EINVAL for a stream id >= n_streams.
 *
 * On an object with a stream ticket in flight (mirsha_streams_submit, below)
 * _run*, _export and _import first make the context's stream wait for it.
 *
 * Not built here: mirsha_multi_* forms, the C++ mirror, the Go files,
 * SHA-224, SHA-384 / SHA-512 / SHA-512/224. */
int mirsha_streams_export(mirsha_ctx* ctx, mirsha_streams* streams, const uint32_t* which, uint32_t k, uint8_t* out);
int mirsha_streams_import(mirsha_ctx* ctx, mirsha_streams* streams, const uint32_t* which, uint32_t k,
                          const uint8_t* in);

/* ----------------------- a stream programme on the asynchronous ring (a2.1) */
/* The ring form of mirsha_streams_run, as mirsha_chains_commit_submit is the
 * ring form of mirsha_chains_commit: the programme is queued, the call
 * returns, and the values are complete when the ticket retires.
 *
 * Behind a SUM_RESET or a RESET a stream restarts from Hasher(), so the
 * stretches of one stream between them are independent hashes.  The ring form
 * cuts each active stream's entries after every such entry into SEGMENTS and
 * runs one lane per segment: a stream with k Sum-then-Reset ops costs its
 * longest stretch, not their sum.  A plain SUM leaves the state as it was and
 * does not cut. */
#define MIRSHA_STREAM_SEG_FIRST 1u /* the stream's first segment: starts from the stored row */
#define MIRSHA_STREAM_SEG_LAST 2u  /* holds the stream's final entry: stores the state it ends in */

/* Host-only, like mirsha_stream_plan, whose output it is built on (same
 * checks, codes and *bad_op_out; the three entry arrays, *n_active_out,
 * *n_entries_out, *n_values_out and *n_bytes_out are that plan's, unchanged,
 * for either value of `pack`).  Segment s, s < *n_seg_out:
 *   seg_stream_out[s]: its stream;
 *   entries [sfirst_out[s], sfirst_out[s+1]) of the entry arrays,
 *     sfirst_out[0] = 0, sfirst_out[n_seg] = *n_entries_out;
 *   seg_flags_out[s]: MIRSHA_STREAM_SEG_FIRST starts from the stream's stored
 *     row; every other segment starts from Hasher(): H0, count 0, an all-zero
 *     block.  MIRSHA_STREAM_SEG_LAST stores the state it ends in as the
 *     stream's.
 * A segment ends with a SUM_RESET or RESET entry or with the stream's final
 * entry: a stream whose entries end with one of the two gets no empty segment
 * behind it (its last segment ends in that entry and stores Hasher()).
 * Segments are stream-major (streams ascending), in op order within a stream.
 * *n_seg_out = active streams + SUM_RESET / RESET entries that are not their
 * stream's final entry.  The writes of a segment that ends in a RESET without
 * a sum in it are dead work; they are not dropped.
 * Capacities: seg_stream_out and seg_flags_out n_ops entries, sfirst_out one
 * more, the entry arrays n_ops. */
int mirsha_stream_seg_plan(const uint32_t* op_stream, const uint32_t* op_kind, const uint64_t* op_off,
                           const uint32_t* op_len, uint32_t n_ops, uint32_t n_streams, uint64_t arena_len, int pack,
                           uint32_t* seg_stream_out, uint32_t* sfirst_out, uint32_t* seg_flags_out,
                           uint32_t* ent_kind_out, uint64_t* ent_off_out, uint32_t* ent_len_out, uint32_t* n_seg_out,
                           uint32_t* n_active_out, uint32_t* n_entries_out, uint32_t* n_values_out,
                           uint64_t* n_bytes_out, uint32_t* bad_op_out);

/* mirsha_streams_run as a ring submission: arguments, checks, error codes,
 * messages and the size limit are that call's.  Before the call returns every
 * check and the plan have run on the host, *n_values_out is written, and the
 * op arrays and every distinct written range of the (host) arena are copied
 * into the ring slot's page-locked block: the caller may reuse them at once.
 * The call takes the context's next ticket and ring slot like mirsha_submit_*
 * and mirsha_chains_commit_submit; the ticket is retired by mirsha_wait /
 * mirsha_poll in ticket order, mixed freely with hashing and commit tickets,
 * and a fifth submission retires the oldest.  values_out (32 bytes per SUM /
 * SUM_RESET op, op order) must stay valid until the ticket retires and is
 * complete then.  A validation failure queues nothing, consumes no ticket and
 * leaves every state untouched.  A programme without an active stream
 * (n_ops == 0, or zero-length writes only): a valid ticket, nothing launched.
 *
 * The device work runs on the context's commit stream (the one of
 * mirsha_chains_commit_submit, created at the first such call), so commit and
 * stream tickets run in submission order among themselves, beside the hashing
 * on the context's stream: one H2D copy of the slot's block, one launch of the
 * segment kernel (timing id 9), the slot's completion event.  When a stream's
 * first and last segment fall into different waves, a device-to-device copy of
 * the state rows precedes the launch (the first segments read that copy;
 * without it a last segment's store could overtake the first segment's load).
 * The kernel stores the values straight into a page-locked, 16-byte aligned
 * values_out, otherwise into page-locked rows of the slot that are copied out
 * at retirement: there is no D2H copy.  mirsha_streams_run* / _export /
 * _import on an object with a ticket in flight first make the context's
 * stream wait for it, so both forms mix on one object without the caller
 * waiting; mirsha_streams_destroy waits for the object's last queued ticket.
 * mirsha_ctx_host_profile of a retired stream ticket: validate = checks and
 * plan, pack = the staging copy, device = queued -> complete, scatter = the
 * values' copy. */
int mirsha_streams_submit(mirsha_ctx* ctx, mirsha_streams* streams, const uint8_t* arena, uint64_t arena_len,
                          const uint32_t* op_stream, const uint32_t* op_kind, const uint64_t* op_off,
                          const uint32_t* op_len, uint32_t n_ops, uint8_t* values_out, uint32_t* n_values_out,
                          uint64_t* ticket_out);
/* The same with the arena in device memory (any alignment).  The commit stream
 * waits on an event recorded on the context's stream at submission, so the
 * arena is read behind whatever was queued there (e.g. the hashing that
 * writes it); it must stay intact until the ticket retires. */
int mirsha_streams_submit_device(mirsha_ctx* ctx, mirsha_streams* streams, const uint8_t* d_arena, uint64_t arena_len,
                                 const uint32_t* op_stream, const uint32_t* op_kind, const uint64_t* op_off,
                                 const uint32_t* op_len, uint32_t n_ops, uint8_t* values_out, uint32_t* n_values_out,
                                 uint64_t* ticket_out);

/* ------------------------------------------------- multi-GPU (one process) */
/* Shards the n requests by contiguous range across ndev devices (balanced by
 * block count), one context per device, host gather into origin order.  No
 * collective: requests are independent (actions.go:22-23). */
int mirsha_hash_batch_multi(const int* devices, int ndev, const uint8_t* arena,
                            uint64_t arena_len, const uint64_t* off, const uint32_t* len,
                            uint32_t n, uint8_t* digests_out);
/* Contexts mirsha_hash_batch_multi keeps per device between calls: freed here
 * (optional; otherwise at process exit). */
void mirsha_multi_release(void);

/* The multi-GPU drop-in: a Go caller's Ready() cycle crosses PCIe at about
 * one link's rate per call (config 2: ~50 GB/s), so one device caps every
 * host-memory caller; the reference's pool scales with cores instead
 * (processor.go:401-410, HashWorkers = runtime.NumCPU()).  A mirsha_multi
 * holds one context per listed device (its own stream, pinned staging ring,
 * PCIe link) and one host worker per device with its own packing pool (an
 * equal share of the host threads).  Each call validates the slice lists,
 * cuts the requests into contiguous ranges of equal bytes (one per device;
 * ranges may be empty), and runs mirsha_hash_slices / mirsha_submit_slices
 * on every range in parallel; digests land at digests_out[32*i] in origin
 * order.  A device may be listed twice (two contexts on it: tests).  With
 * MIRSHA_SUBMIT_DEDUP each device deduplicates within its own range.
 * Single-caller, like a context.  At most 16 devices. */
typedef struct mirsha_multi mirsha_multi;
int mirsha_multi_create(const int* devices, int ndev, mirsha_multi** out);
void mirsha_multi_destroy(mirsha_multi* m);
const char* mirsha_multi_last_error(const mirsha_multi* m);
int mirsha_multi_devices(const mirsha_multi* m);
/* Context of device index k (0 <= k < ndev) for per-device settings and
 * diagnostics (mirsha_ctx_set_variant, timing); owned by m. */
mirsha_ctx* mirsha_multi_ctx(mirsha_multi* m, int k);
/* Request-range cut of the last call (every entry point cuts at the request
 * boundary nearest to k/ndev of the bytes): first_out[k] = first request of device
 * index k, first_out[ndev] = n.  Returns ndev + 1 (entries written: min(cap, ndev + 1)). */
int mirsha_multi_last_cut(const mirsha_multi* m, uint32_t* first_out, int cap);
int mirsha_hash_slices_multi(mirsha_multi* m, const uint8_t* const* slice_ptr,
                             const uint64_t* slice_len, const uint32_t* slice_first, uint32_t n,
                             uint8_t* digests_out);
/* The same over a caller arena (mirsha_hash_batch on every range): with a
 * page-locked arena from mirsha_multi_host_alloc every device DMAs its range
 * straight from it over its own link (the Go binding's GPUHasherMulti packs
 * one Ready() cycle into that arena with GOMAXPROCS goroutines). */
int mirsha_hash_arena_multi(mirsha_multi* m, const uint8_t* arena, uint64_t arena_len,
                            const uint64_t* off, const uint32_t* len, uint32_t n, uint8_t* digests_out);
/* Page-locked host memory usable by every device of m (portable); free with mirsha_host_free. */
int mirsha_multi_host_alloc(mirsha_multi* m, uint64_t bytes, void** out);
/* Asynchronous form (mirsha_submit_slices on every range): up to 4
 * submissions in flight; wait / poll cover every device's range of every
 * submission up to `ticket`.  The caller may reuse the slices when submit returns. */
int mirsha_submit_slices_multi(mirsha_multi* m, const uint8_t* const* slice_ptr,
                               const uint64_t* slice_len, const uint32_t* slice_first, uint32_t n,
                               uint8_t* digests_out, int flags, uint64_t* ticket_out);
/* mirsha_submit_batch over several devices: the requests cut into contiguous
 * ranges of equal bytes (as mirsha_hash_arena_multi), each range submitted to
 * its device's ring, DMA'd straight from a page-locked arena
 * (mirsha_multi_host_alloc) over that device's own link.  Tickets, wait and
 * poll as mirsha_submit_slices_multi. */
int mirsha_submit_arena_multi(mirsha_multi* m, const uint8_t* arena, uint64_t arena_len,
                              const uint64_t* off, const uint32_t* len, uint32_t n,
                              uint8_t* digests_out, uint64_t* ticket_out);
int mirsha_wait_multi(mirsha_multi* m, uint64_t ticket);
int mirsha_poll_multi(mirsha_multi* m, uint64_t ticket, int* done);
/* mirsha_ctx_host_profile of device index k's last call (its range only). */
int mirsha_multi_host_profile(const mirsha_multi* m, int k, double* ms_out, int n);

/* ------------------------------------------- benchmark / test utility only */
/* Device-side synthetic request stream, byte-identical to the
 * oracle generator: request i = LE64(i%16) || LE64(i/16) || data_len bytes of
 * splitmix64(splitmix64(seed ^ i) + j).  count messages packed densely. */
int mirsha_synth_requests_device(mirsha_ctx* ctx, uint64_t seed, uint64_t first, uint64_t count,
                                 uint32_t data_len, uint8_t* d_arena);
/* BASELINE config 5 stream (mixed 64 B - 64 KB): d_len[r] = message length
 * (16 + data_len) of request first + r, data_len log-uniform over the octaves
 * of [64, 65536) in integer arithmetic (identical to the oracle's
 * oracle_mixed_data_len); then the message bytes (same layout and data as
 * above) at d_arena + d_off[r], any byte alignment. */
int mirsha_synth_mixed_lengths_device(mirsha_ctx* ctx, uint64_t seed, uint64_t first, uint64_t count,
                                      uint32_t* d_len);
int mirsha_synth_mixed_device(mirsha_ctx* ctx, uint64_t seed, uint64_t first, uint64_t count,
                              const uint64_t* d_off, uint8_t* d_arena);

/* Clock probe (diagnostics; bench.py runs it right after its timed region):
 * every SIMD runs 8 waves of `iters` back-to-back register-only compressions
 * in the request kernel's round form.  *clock_ghz = median over waves of
 * shader cycles / 100 MHz reference ticks (the clock held under this load);
 * *cycles_per_wave_compression = launch span (first wave start to last wave
 * end, in shader cycles at that clock) / (iters x 8): the SIMD cycles one
 * 64-lane compression costs with no memory traffic at all (the measured
 * ceiling the request kernel is compared with).  Synchronous. */
int mirsha_clock_probe(mirsha_ctx* ctx, uint32_t iters, double* clock_ghz, double* cycles_per_wave_compression);

#ifdef __cplusplus
}
#endif
#endif /* MIRSHA_H */
