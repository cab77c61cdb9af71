// mirsha_async.hip — the asynchronous, order-preserving ring
// (mirsha_submit_slices / mirsha_wait / mirsha_poll, content-addressed dedup,
// mixed hash-and-verify cycles, and the two in one ticket):
// the hash stage of ProcessorWorkPool (processor.go:312-361, 447-470) without
// its completion-order output.
#include "mirsha_ctx.h"

namespace mirsha_api {

// ---- the slot lifecycle (mirsha_ctx.h) ---------------------------------------
int ensure_event(mirsha_ctx* c, hipEvent_t* e) {
    if (!*e) HIP_TRY(c, hipEventCreateWithFlags(e, hipEventDisableTiming));
    return MIRSHA_OK;
}

int ring_acquire(mirsha_ctx* c, AsyncSlot** slot) {
    if (int rc = use_device(c)) return rc;
    AsyncSlot& sl = c->slots[(c->next_ticket - 1) % kAsyncSlots];
    if (sl.busy)
        if (int rc = async_wait_upto(c, sl.ticket)) return rc;  // ring full: retire the oldest
    sl.retire = SlotRetire{};
    *slot = &sl;
    return ensure_event(c, &sl.done);
}

void ring_publish(mirsha_ctx* c, AsyncSlot& sl, RingQueued& queued, const double* ph, uint64_t* ticket_out) {
    queued.armed = false;
    sl.busy = true;
    sl.ticket = c->next_ticket++;
    for (int k = 0; k < MIRSHA_PROF_PHASES; k++) sl.prof[k] = ph[k];
    if (ticket_out) *ticket_out = sl.ticket;
}

uint8_t* host_rows(mirsha_ctx* c, void* p) {
    if (!p || (reinterpret_cast<uintptr_t>(p) & 15u) || !kernel_writable_host(p, c->device)) return nullptr;
    void* dp = nullptr;
    if (hipHostGetDevicePointer(&dp, p, 0) == hipSuccess) return static_cast<uint8_t*>(dp);
    (void)hipGetLastError();
    return nullptr;
}

int pinned_rows(mirsha_ctx* c, const PinnedBuf& b, uint8_t** rows) {
    void* dp = nullptr;
    HIP_TRY(c, hipHostGetDevicePointer(&dp, b.p, 0));
    *rows = static_cast<uint8_t*>(dp);
    return MIRSHA_OK;
}

// ---- mixed hash-and-verify cycles (mirsha_submit_*_expect) -------------------
// What a mixed submission adds to the plain one's arguments.
struct ExpectArgs {
    const uint32_t* expect_of;
    const uint8_t* expected;
    uint32_t m;
    uint64_t* bits_out;
    uint32_t* n_mismatch_out;
};

// The one check of a caller's submit flags: mirsha_submit_slices takes
// MIRSHA_SUBMIT_DEDUP, mirsha_submit_slices_expect (`mixed`) none.
static int check_submit_flags(mirsha_ctx* c, int flags, bool mixed) {
    if (mixed && (flags & MIRSHA_SUBMIT_DEDUP))
        return fail(c, MIRSHA_EINVAL,
                    "MIRSHA_SUBMIT_DEDUP does not combine with expectations here: "
                    "mirsha_submit_slices_expect_dedup");
    if (flags & ~(mixed ? 0 : MIRSHA_SUBMIT_DEDUP)) return fail(c, MIRSHA_EINVAL, "unknown submit flags 0x%x", flags);
    return MIRSHA_OK;
}

// The argument checks of a mixed submission, and its plan (mirsha_expect_plan)
// into the context's scratch.  Nothing is queued and no ticket is consumed.
static int expect_validate(mirsha_ctx* c, const ExpectArgs& xa, uint32_t n) {
    if (!xa.n_mismatch_out) return fail(c, MIRSHA_EINVAL, "n_mismatch_out is NULL");
    if (xa.m && (!xa.expect_of || !xa.expected)) return fail(c, MIRSHA_EINVAL, "NULL argument");
    if (xa.m > n) return fail(c, MIRSHA_EINVAL, "%u expectations for %u requests", xa.m, n);
    const uint32_t words = (uint32_t)(((uint64_t)n + 63u) >> 6);
    if (c->xp_has.size() < words) c->xp_has.resize(words);
    if (c->xp_base.size() < words) c->xp_base.resize(words);
    if (mirsha_expect_plan(xa.expect_of, xa.m, n, c->xp_has.data(), c->xp_base.data()) != MIRSHA_OK)
        return fail(c, MIRSHA_EINVAL, "expect_of must be strictly increasing with every index below %u", n);
    return MIRSHA_OK;
}

// Sizes the (free) slot's expectation staging, device block and verdict, and
// stages the plan.
static int expect_stage(mirsha_ctx* c, AsyncSlot& sl, const ExpectArgs& xa, uint32_t n, bool gather = false) {
    ExpectSlot& x = sl.xp;
    x.words = (uint32_t)(((uint64_t)n + 63u) >> 6);
    x.o_exp = align16(12ull * x.words);
    x.h2d = x.o_exp + 32ull * xa.m;
    x.o_row = align16(x.h2d);  // a deduplicated cycle's row_of[], sent on its own once it is resolved
    x.o_ver = gather ? align16(x.o_row + 4ull * n) : x.o_row;
    HIP_TRY(c, x.stage.ensure(std::max<uint64_t>(x.o_ver, 16)));
    HIP_TRY(c, x.verdict.ensure(8 + 8ull * x.words));
    HIP_TRY(c, x.dev.ensure(x.o_ver + 8 + 8ull * x.words));
    uint8_t* st = x.stage.as<uint8_t>();
    memcpy(st, c->xp_has.data(), 8ull * x.words);
    memcpy(st + 8ull * x.words, c->xp_base.data(), 4ull * x.words);
    return MIRSHA_OK;
}

// Copies the expected rows into the slot's staging (before the call returns:
// the caller may reuse them at once) and queues the expectation block's H2D.
// Called once the request bytes' DMA is queued, so the copy runs under it.
static int expect_h2d(mirsha_ctx* c, AsyncSlot& sl, const ExpectArgs& xa, hipStream_t s) {
    ExpectSlot& x = sl.xp;
    const uint64_t bytes = 32ull * xa.m;
    mirsha::host::pack_range(xa.expected, nullptr, nullptr, nullptr, 0, nullptr, 0, bytes,
                             x.stage.as<uint8_t>() + x.o_exp, mirsha::host::threads_for(bytes, 1u << 20), true);
    HIP_TRY(c, hipMemcpyAsync(x.dev.p, x.stage.p, x.h2d, hipMemcpyHostToDevice, s));
    return MIRSHA_OK;
}

// Behind the hashing kernel on c->stream: the count's reset,
// expect_select_kernel (timing id 7) over the n device digests, the kept rows
// stored to `rows` (host-visible, device address), and the verdict's copy.
// A deduplicated cycle (`gather`): expect_select_gather_kernel instead, which
// reads request i's digest from row row_of[i] (staged at o_row) of the
// representatives' digests, rows [0, m0) in d_digests and the rest in d_digests2.
static int expect_queue(mirsha_ctx* c, AsyncSlot& sl, const uint8_t* d_digests, uint32_t n, uint8_t* rows,
                        bool gather = false, const uint8_t* d_digests2 = nullptr, uint32_t m0 = 0) {
    ExpectSlot& x = sl.xp;
    uint8_t* xd = x.dev.as<uint8_t>();
    uint32_t* d_count = reinterpret_cast<uint32_t*>(xd + x.o_ver);
    uint64_t* d_bits = reinterpret_cast<uint64_t*>(xd + x.o_ver + 8);
    const uint64_t* d_has = reinterpret_cast<const uint64_t*>(xd);
    const uint32_t* d_base = reinterpret_cast<const uint32_t*>(xd + 8ull * x.words);
    HIP_TRY(c, hipMemsetAsync(d_count, 0, sizeof(uint32_t), c->stream));
    if (int rc = timed_launch(c, kTimerExpect, [&] {
            if (gather)
                return mirsha::launch_expect_select_gather(d_digests, d_digests2, m0,
                                                           reinterpret_cast<const uint32_t*>(xd + x.o_row),
                                                           xd + x.o_exp, d_has, d_base, n, rows, d_bits, d_count,
                                                           c->stream);
            return mirsha::launch_expect_select(d_digests, xd + x.o_exp, d_has, d_base, n, rows, d_bits, d_count,
                                                c->stream);
        }))
        return rc;
    HIP_TRY(c, hipMemcpyAsync(x.verdict.p, xd + x.o_ver, 8 + 8ull * x.words, hipMemcpyDeviceToHost, c->stream));
    return MIRSHA_OK;
}

// What a hashing ticket of n requests owes at retirement: its rows, and with
// expectations (`xa`) the verdict: the device's, or all zero when there was
// nothing to compare (m == 0: no expect_stage ran, so the words are set here).
static void owe(AsyncSlot& sl, SlotRows rows, uint8_t* out, uint32_t n, const ExpectArgs* xa) {
    SlotRetire& r = sl.retire;
    r.rows = rows;
    r.out = out;
    r.n = n;
    if (!xa) return;
    r.bits = xa->bits_out;
    r.count = xa->n_mismatch_out;
    r.verdict = xa->m ? SlotVerdict::kDevice : SlotVerdict::kAllZero;
    if (!xa->m) sl.xp.words = (uint32_t)(((uint64_t)n + 63u) >> 6);
}

// Retires a completed submission: its rows to the caller in origin order, then
// its verdict (sl.retire says which of either).
int async_complete(mirsha_ctx* c, AsyncSlot& sl) {
    HIP_TRY(c, hipEventSynchronize(sl.done));
    const auto t_done = Clock::now();
    sl.prof[MIRSHA_PROF_DEVICE] = std::chrono::duration<double, std::milli>(t_done - sl.t_queued).count();
    const SlotRetire& r = sl.retire;
    const ExpectSlot& x = sl.xp;
    const uint8_t* d = sl.dig.as<uint8_t>();
    const uint8_t* v = x.verdict.as<uint8_t>();  // [count u32, pad | mismatch bitmap]
    switch (r.rows) {
    case SlotRows::kInPlace:
        break;
    case SlotRows::kCopyAll:
        if (r.n) memcpy(r.out, d, 32ull * r.n);
        break;
    case SlotRows::kFanOut:
        for (uint32_t i = 0; i < r.n; i++) memcpy(r.out + 32ull * i, d + 32ull * sl.rank[i], 32);
        break;
    case SlotRows::kKept:  // requests without an expectation, and mismatches
        mirsha::host::copy_kept_rows(x.stage.as<uint64_t>(), reinterpret_cast<const uint64_t*>(v + 8), r.n, d, r.out);
        break;
    case SlotRows::kCommit:
        if (r.n) memcpy(r.out, sl.cm.rows.p, 32ull * r.n);
        break;
    }
    switch (r.verdict) {
    case SlotVerdict::kNone:
        break;
    case SlotVerdict::kAllZero:
        if (r.bits) memset(r.bits, 0, 8ull * x.words);
        *r.count = 0;
        break;
    case SlotVerdict::kDevice:
        if (r.bits) memcpy(r.bits, v + 8, 8ull * x.words);
        memcpy(r.count, v, sizeof(uint32_t));
        break;
    }
    sl.busy = false;
    c->done_ticket = std::max(c->done_ticket, sl.ticket);
    sl.prof[MIRSHA_PROF_SCATTER] = ms_since(t_done);
    sl.prof[MIRSHA_PROF_CHUNKS] = 0;
    // mirsha_ctx_host_profile: every phase of ONE submission, the most
    // recently completed (not one ticket's plan beside another's device time)
    for (int k = 0; k < MIRSHA_PROF_PHASES; k++) c->prof[k] = sl.prof[k];
    return MIRSHA_OK;
}

int async_wait_upto(mirsha_ctx* c, uint64_t ticket) {
    for (uint64_t t = c->done_ticket + 1; t <= ticket; t++) {
        AsyncSlot& sl = c->slots[(t - 1) % kAsyncSlots];
        if (sl.busy && sl.ticket == t)
            if (int rc = async_complete(c, sl)) return rc;
    }
    return MIRSHA_OK;
}

int async_submit(mirsha_ctx* c, const uint8_t* const* slice_ptr, const uint64_t* slice_len,
                 const uint32_t* slice_first, uint32_t n, uint8_t* out, bool want_dedup, uint64_t* ticket_out,
                 uint32_t* n_unique_out, const ExpectArgs* xa = nullptr) {
    auto t0 = Clock::now();
    if (xa)
        if (int rc = expect_validate(c, *xa, n)) return rc;
    // a deduplicated mixed cycle counts its expectation plan as validation
    const double t_xplan = xa && want_dedup ? ms_since(t0) : 0.0;
    t0 = Clock::now();
    // Which requests reach the GPU: all, or one per distinct content.  With
    // dedup the requests are scanned in segments in origin order
    // (mirsha::host::DedupScan): the first segment's heads (distinct
    // contents, each a final representative) are packed and queued as soon as
    // that segment is scanned, and the GPU hashes them while the host scans
    // and confirms the rest -- a request matching an earlier head is compared
    // byte for byte in the same walk, while its bytes are cache-warm.
    // Representatives found later (new contents of later segments, and
    // fingerprint collisions, rare) follow in one second launch.
    const bool dedup = want_dedup && n > 1;
    double ph[MIRSHA_PROF_PHASES] = {};
    std::vector<uint32_t>& len = c->sl_len;  // context scratch (single caller), grow-only
    if (dedup) {
        if (int rc = slice_args(c, slice_ptr, slice_len, slice_first, n, out)) return rc;
        if (len.size() < n) len.resize(n);  // each segment's lengths are set before it is queued
    } else if (n) {
        if (int rc = slice_lengths(c, slice_ptr, slice_len, slice_first, n, out, len)) return rc;
    }
    ph[MIRSHA_PROF_VALIDATE] = ms_since(t0) + t_xplan;
    t0 = Clock::now();
    AsyncSlot* slot = nullptr;
    if (int rc = ring_acquire(c, &slot)) return rc;
    AsyncSlot& sl = *slot;
    RingQueued queued(c->stream);
    HIP_TRY(c, sl.dig.ensure(32ull * std::max<uint32_t>(n, 1)));
    // Mixed submission with expectations: the select kernel stands where the
    // digests' D2H copy stood, storing the kept rows into a page-locked
    // digests_out or else into the slot's page-locked rows.
    // Deduplicated as well (`gather`): every launch keeps its representatives'
    // digests on the device, the expectation block goes H2D once behind the
    // first launch's request bytes, and ONE select launch behind the last
    // hashing launch reads request i's digest from row row_of[i].
    const bool sel = xa && xa->m;
    const bool gather = sel && dedup;
    const uint8_t* gather_dig[2] = {nullptr, nullptr};  // the launches' digest rows on the device
    uint8_t* sel_rows = nullptr;
    SlotRows rows = SlotRows::kCopyAll;
    if (sel) {
        if (int rc = expect_stage(c, sl, *xa, n, gather)) return rc;
        sel_rows = host_rows(c, out);
        rows = sel_rows ? SlotRows::kInPlace : SlotRows::kKept;
        if (!sel_rows)
            if (int rc = pinned_rows(c, sl.dig, &sel_rows)) return rc;
    }
    ph[MIRSHA_PROF_PLAN] = ms_since(t0);
    // Packs requests `ids` (identity when null) into `stage`, and queues their
    // digests into rows [row0, row0 + m) of sl.dig.
    auto queue = [&](const uint32_t* ids, uint32_t m, uint32_t row0, PinnedBuf& stage, DevBuf& dev) -> int {
        const auto tq = Clock::now();
        uint64_t bytes = 0;
        for (uint32_t k = 0; k < m; k++) bytes += len[ids ? ids[k] : k];
        if (bytes + kArenaSlack > MIRSHA_MAX_DEVICE_ARENA_BYTES)
            return fail(c, MIRSHA_ERANGE, "submission of %llu bytes exceeds one device arena (%u); split it",
                        (unsigned long long)bytes, MIRSHA_MAX_DEVICE_ARENA_BYTES);
        const uint64_t o_off = align8(bytes + kArenaSlack);
        const uint64_t o_len = o_off + 8ull * m, o_ord = o_len + 4ull * m;
        const uint64_t o_end = sel ? align16(o_ord + 4ull * m) : align8(o_ord + 4ull * m);  // select: 128-bit rows
        const uint64_t o_dig = o_end;
        HIP_TRY(c, stage.ensure(o_end));
        HIP_TRY(c, dev.ensure(o_dig + 32ull * std::max<uint32_t>(m, 1)));
        uint8_t* st = stage.as<uint8_t>();
        // offsets and lengths straight into the staged metadata (no temporaries)
        uint64_t* poff = reinterpret_cast<uint64_t*>(st + o_off);
        uint32_t* plen = reinterpret_cast<uint32_t*>(st + o_len);
        uint64_t p = 0;
        for (uint32_t k = 0; k < m; k++) {
            const uint32_t i = ids ? ids[k] : k;
            poff[k] = p;
            plen[k] = len[i];
            p += len[i];
        }
        mirsha::host::pack(slice_ptr, slice_len, slice_first, ids, m, poff, st, mirsha::host::threads_for(bytes, m),
                           true);
        const bool identity = bucket_order(plen, m, reinterpret_cast<uint32_t*>(st + o_ord));
        uint8_t* dv = dev.as<uint8_t>();
        if (m) {
            queued.arm();
            HIP_TRY(c, hipMemcpyAsync(dv, st, o_end, hipMemcpyHostToDevice, c->stream));
            if (sel && !(gather && row0))
                if (int rc = expect_h2d(c, sl, *xa, c->stream)) return rc;
            int rc = timed_launch(c, 0, [&] {
                return hasher_launch_msgs(c, dv, bytes, reinterpret_cast<const uint64_t*>(dv + o_off),
                                          reinterpret_cast<const uint32_t*>(dv + o_len),
                                          identity ? nullptr : reinterpret_cast<const uint32_t*>(dv + o_ord), m,
                                          dv + o_dig, c->stream);
            });
            if (rc) return rc;
            if (gather) {
                gather_dig[row0 ? 1 : 0] = dv + o_dig;
            } else if (sel) {
                if (int rc2 = expect_queue(c, sl, dv + o_dig, m, sel_rows)) return rc2;
            } else {
                HIP_TRY(c, hipMemcpyAsync(sl.dig.as<uint8_t>() + 32ull * row0, dv + o_dig, 32ull * m,
                                          hipMemcpyDeviceToHost, c->stream));
            }
        }
        ph[MIRSHA_PROF_PACK] += ms_since(tq);
        return MIRSHA_OK;
    };
    uint32_t m = n;
    if (!dedup) {
        if (int rc = queue(nullptr, n, 0, sl.stage, sl.dev)) return rc;
        sl.t_queued = Clock::now();
    } else {
        mirsha::host::DedupScan d(slice_ptr, slice_len, slice_first, n, MIRSHA_MAX_MESSAGE_BYTES);
        const std::vector<uint32_t> seg = d.segments();
        std::vector<uint32_t> first_heads, later;  // the first launch's rows, then the second's
        for (size_t k = 0; k + 1 < seg.size(); k++) {
            const uint32_t lo = seg[k], hi = seg[k + 1];
            t0 = Clock::now();
            const bool ok = d.scan(lo, hi);
            ph[MIRSHA_PROF_VALIDATE] += ms_since(t0);
            if (!ok) return slice_errors(c, d.err(), n);  // (a first launch already queued is drained: RingQueued)
            t0 = Clock::now();
            for (uint32_t i = lo; i < hi; i++) len[i] = (uint32_t)d.req_len()[i];
            d.assign(lo, hi, k == 0 ? first_heads : later);
            ph[MIRSHA_PROF_PLAN] += ms_since(t0);
            if (k == 0) {
                if (int rc = queue(first_heads.data(), (uint32_t)first_heads.size(), 0, sl.stage, sl.dev))
                    return rc;
                sl.t_queued = Clock::now();
            }
            t0 = Clock::now();
            d.confirm(lo, hi);
            ph[MIRSHA_PROF_PLAN] += ms_since(t0);
        }
        t0 = Clock::now();
        std::vector<uint32_t> rep(n);
        const uint32_t distinct = d.resolve(rep.data(), &later);  // collisions appended to `later`
        const uint32_t m0 = (uint32_t)first_heads.size();
        m = m0 + (uint32_t)later.size();
        if (m != distinct) return fail(c, MIRSHA_EHIP, "dedup: %u representatives for %u contents", m, distinct);
        // request -> row of the representatives' digests: for the host's fan-out
        // at retirement, or (gather) into the expectation staging for the kernel's
        uint32_t* row_of = nullptr;
        if (gather) {
            row_of = reinterpret_cast<uint32_t*>(sl.xp.stage.as<uint8_t>() + sl.xp.o_row);
        } else {
            if (sl.rank.size() < n) sl.rank.resize(n);
            row_of = sl.rank.data();
        }
        const bool identity = mirsha::host::dedup_rows(rep.data(), first_heads, later, n, row_of);
        if (gather) {  // the kernel's loads stay inside the m rows
            uint32_t top = 0;
            for (uint32_t i = 0; i < n; i++) top = std::max(top, row_of[i]);
            if (top >= m) return fail(c, MIRSHA_EHIP, "dedup: row %u of %u representatives", top, m);
        } else if (!identity) {  // (all distinct: the rows are in origin order already)
            rows = SlotRows::kFanOut;
        }
        ph[MIRSHA_PROF_PLAN] += ms_since(t0);
        if (!later.empty())
            if (int rc = queue(later.data(), (uint32_t)later.size(), m0, sl.stage2, sl.dev2)) return rc;
        if (gather) {
            const auto tq = Clock::now();
            HIP_TRY(c, hipMemcpyAsync(sl.xp.dev.as<uint8_t>() + sl.xp.o_row, row_of, 4ull * n, hipMemcpyHostToDevice,
                                      c->stream));
            if (int rc = expect_queue(c, sl, gather_dig[0], n, sel_rows, true, gather_dig[1], m0)) return rc;
            ph[MIRSHA_PROF_PACK] += ms_since(tq);
        }
    }
    if (n_unique_out) *n_unique_out = m;
    HIP_TRY(c, hipEventRecord(sl.done, c->stream));
    owe(sl, rows, out, n, xa);
    ring_publish(c, sl, queued, ph, ticket_out);
    return MIRSHA_OK;
}

// mirsha_submit_batch: n requests of a caller arena (request i =
// arena[off[i], off[i] + len[i])), one slot of the ring.  The off / len
// arrays are read before the call returns.  A dense range [lo, hi) of a
// page-locked arena is DMA'd straight from it (no host copy: the caller must
// leave those bytes alone until the ticket retires); a pageable or sparse one
// is copied into the slot's pinned staging first (packed back to back when
// sparse), so the caller may reuse it at once.  Digests land in a page-locked
// digests_out by DMA, else in the slot's pinned rows, copied out when the
// ticket retires.  The Go binding's chunked HashBatch packs
// chunk k + 1 of a Ready() cycle while chunk k's DMA, kernel and D2H run.
int async_submit_arena(mirsha_ctx* c, const uint8_t* arena, uint64_t arena_len, const uint64_t* off,
                       const uint32_t* len, uint32_t n, uint8_t* out, uint64_t* ticket_out,
                       const ExpectArgs* xa = nullptr) {
    auto t0 = Clock::now();
    const auto t_entry = t0;
    if (xa)
        if (int rc = expect_validate(c, *xa, n)) return rc;
    double ph[MIRSHA_PROF_PHASES] = {};
    // MIRSHA_SUBMIT_TRACE=1 (with MIRSHA_AB=1): a submission slower than 2 ms
    // prints where its time went (ms since entry at each step) on stderr.
    double tr[6] = {}, tq[8] = {};
    auto trace_done = [&](const char* how) {
        const double tot = ms_since(t_entry);
        if (tot > 2.0 && getenv_flag("MIRSHA_SUBMIT_TRACE"))
            fprintf(stderr,
                    "mirsha submit trace: %.3f ms (%s): slot wait %.3f, meta buffer %.3f, validate %.3f, "
                    "buffers %.3f, pack %.3f, queue %.3f [ev_in %.3f meta %.3f wait %.3f scan %.3f kernel %.3f "
                    "ev_kern %.3f d2h %.3f done %.3f]\n",
                    tot, how, tr[0], tr[1], tr[2], tr[3], tr[4], tr[5], tq[0], tq[1], tq[2], tq[3], tq[4], tq[5],
                    tq[6], tq[7]);
    };
    // One pass over the n entries on the calling thread (up to 2^18
    // requests: a chunk of the Go binding's HashBatch is ~120k requests and
    // its goroutines pack the NEXT chunk meanwhile): bounds, the span [lo,
    // hi), total bytes, block-count range, whether the requests are gapless,
    // and the lengths into the metadata block.  Offsets cross PCIe only when
    // the requests are not gapless (else the device rebuilds them by a scan
    // of the lengths), the bucket order only when block counts differ (and
    // not with MIRSHA_ORDER_DEVICE: the device then builds it): 4 B per
    // request instead of 16 in the common case (the metadata shares the
    // link with the request bytes and the digests).
    struct Part {
        uint64_t lo = UINT64_MAX, hi = 0, tot = 0;
        uint32_t bmin = UINT32_MAX, bmax = 0, bad = UINT32_MAX;
        bool gapless = true;
    };
    const int T = n < (1u << 18) ? 1
                                 : (int)std::min<uint32_t>((uint32_t)mirsha::host::max_threads(), n / (1u << 16));
    std::vector<Part> parts(T);
    const uint32_t step = n ? (n + (uint32_t)T - 1) / (uint32_t)T : 1;
    // Slot buffers: `stage2` = the metadata block [len u32 | order u32 | off
    // u64] (the device's copy has the same layout), `stage` = a copy of the
    // request bytes when they are not DMA'd from the caller, `dev` = [request
    // bytes + slack | metadata | digests].  The slot comes first: the pass
    // below writes the metadata block into it.
    AsyncSlot* slot = nullptr;
    if (int rc = ring_acquire(c, &slot)) return rc;
    AsyncSlot& sl = *slot;
    tr[0] = ms_since(t_entry);
    const uint64_t o_len = 0, o_ord = align8(4ull * n), o_off = align8(o_ord + 4ull * n), o_end = o_off + 8ull * n;
    HIP_TRY(c, sl.stage2.ensure(std::max<uint64_t>(o_end, 8)));
    tr[1] = ms_since(t_entry);
    uint8_t* mb = sl.stage2.as<uint8_t>();
    uint32_t* slen = reinterpret_cast<uint32_t*>(mb + o_len);
    uint32_t* sord = reinterpret_cast<uint32_t*>(mb + o_ord);
    uint64_t* soff = reinterpret_cast<uint64_t*>(mb + o_off);
    // The metadata block is page-locked host memory: written once, never
    // read back by the host.
    mirsha::host::parallel_for(n, T, [&](uint32_t a, uint32_t b) {
        Part& q = parts[a / step];
        for (uint32_t i = a; i < b; i++) {
            const uint64_t o = off[i];
            const uint32_t L = len[i];
            if (L > MIRSHA_MAX_MESSAGE_BYTES || o > arena_len || L > arena_len - o) {
                q.bad = i;
                return;
            }
            slen[i] = L;
            if (i > a && o != off[i - 1] + len[i - 1]) q.gapless = false;
            q.lo = std::min(q.lo, o);
            q.hi = std::max(q.hi, o + L);
            q.tot += L;
            const uint32_t k = host_blocks(L);
            q.bmin = std::min(q.bmin, k);
            q.bmax = std::max(q.bmax, k);
        }
    });
    Part all;
    for (int k = 0; k < T; k++) {
        const Part& q = parts[k];
        all.bad = std::min(all.bad, q.bad);
        all.lo = std::min(all.lo, q.lo);
        all.hi = std::max(all.hi, q.hi);
        all.tot += q.tot;
        all.bmin = std::min(all.bmin, q.bmin);
        all.bmax = std::max(all.bmax, q.bmax);
        all.gapless = all.gapless && q.gapless;
        const uint32_t a = (uint32_t)k * step;  // part boundaries
        if (k > 0 && a < n && off[a] != off[a - 1] + len[a - 1]) all.gapless = false;
    }
    if (all.bad != UINT32_MAX) {
        const uint32_t i = all.bad;
        if (len[i] > MIRSHA_MAX_MESSAGE_BYTES)
            return fail(c, MIRSHA_ERANGE, "message %u is %u bytes (max %u)", i, len[i], MIRSHA_MAX_MESSAGE_BYTES);
        return fail(c, MIRSHA_EINVAL, "message %u [%llu,+%u) outside arena of %llu bytes", i,
                    (unsigned long long)off[i], len[i], (unsigned long long)arena_len);
    }
    const uint64_t lo = n ? all.lo : 0, hi = n ? all.hi : 0, total = all.tot;
    const uint64_t span = hi - lo;
    const bool dense = span <= 2 * total + 4096;
    const uint64_t bytes = dense ? span : total;
    if (bytes + kArenaSlack > MIRSHA_MAX_DEVICE_ARENA_BYTES)
        return fail(c, MIRSHA_ERANGE, "submission of %llu bytes exceeds one device arena (%u); split it",
                    (unsigned long long)bytes, MIRSHA_MAX_DEVICE_ARENA_BYTES);
    // gapless => in order from lo = off[0]: the device scan of the lengths is the offsets
    const bool gapless = n && dense && all.gapless;
    if (!gapless && dense) {
        mirsha::host::parallel_for(n, T, [&](uint32_t a, uint32_t b) {
            for (uint32_t i = a; i < b; i++) soff[i] = off[i] - lo;
        });
    } else if (!dense) {  // packed back to back: off = exclusive scan of len
        uint64_t p = 0;
        for (uint32_t i = 0; i < n; i++) {
            soff[i] = p;
            p += len[i];
        }
    }
    // MIRSHA_ORDER_DEVICE: a cycle of several block counts gets its bucket
    // order from the device (queue_bucket_order, with this pass's exact bounds:
    // the host's order), written into the slot's device order region; neither
    // the sort nor the order's bytes are the submitting thread's.
    const bool dev_order = c->order_mode == MIRSHA_ORDER_DEVICE && n && all.bmin != all.bmax &&
                           all.bmax - all.bmin < MIRSHA_ORDER_MAX_BINS;
    const bool identity = n == 0 || all.bmin == all.bmax || (!dev_order && bucket_order(len, n, sord));
    // bytes of the metadata block that cross PCIe (a device order that is not
    // gapless: the lengths and the offsets, in two copies around the order region)
    const uint64_t meta_copy = dev_order ? 4ull * n : !gapless ? o_end : !identity ? o_ord + 4ull * n : 4ull * n;
    ph[MIRSHA_PROF_VALIDATE] = ms_since(t0);
    tr[2] = ms_since(t_entry);
    t0 = Clock::now();
    for (hipEvent_t* e : {&sl.ev_in, &sl.ev_kern})
        if (int rc = ensure_event(c, e)) return rc;
    // Request bytes in on xin, the kernel on the context stream; digests
    // stored by the kernel into a page-locked digests_out (metadata then on
    // xin too), else out on xout with the metadata on the kernel stream.
    // Submission k+1's DMA runs behind submission k's DMA, not behind its
    // kernel (PCIe is full duplex).
    if (!c->xin) HIP_TRY(c, hipStreamCreateWithFlags(&c->xin, hipStreamNonBlocking));
    if (!c->xout) HIP_TRY(c, hipStreamCreateWithFlags(&c->xout, hipStreamNonBlocking));
    const bool from_caller = dense && n && host_pinned(arena + lo);
    const bool direct = host_pinned(out);  // digests by DMA (or the kernel) straight into digests_out
    // A page-locked digests_out is written by the kernel itself (posted
    // writes over PCIe; visible when the kernel's completion is), and the
    // metadata follows the request bytes on xin: every SDMA copy of the
    // submission is then on one stream.  With copies on three streams (H2D,
    // metadata, D2H) the runtime now and then blocked a hipMemcpyAsync for
    // 8-15 ms (profiles/r05w: 13-22 ms calls of the chunked HashBatch); with
    // one copy stream no call stalled, at the same steady-state speed.
    uint8_t* const kout = direct && n ? host_rows(c, out) : nullptr;
    // Mixed submission with expectations: the hashing kernel keeps its digests
    // on the device, and the select kernel behind it stores the kept rows into
    // a kernel-writable digests_out, else into the slot's page-locked rows.
    const bool sel = xa && xa->m;
    uint8_t* sel_rows = kout;
    SlotRows rows = direct ? SlotRows::kInPlace : SlotRows::kCopyAll;
    if (!direct || (sel && !kout)) HIP_TRY(c, sl.dig.ensure(32ull * std::max<uint32_t>(n, 1)));
    if (sel) {
        if (int rc = expect_stage(c, sl, *xa, n)) return rc;
        rows = kout ? SlotRows::kInPlace : SlotRows::kKept;
        if (!kout)
            if (int rc = pinned_rows(c, sl.dig, &sel_rows)) return rc;
    }
    // device: [request bytes + slack | len u32 | order u32 | off u64 | digests]
    const uint64_t d_meta = align8(bytes + kArenaSlack);
    const uint64_t d_dig = sel ? align16(d_meta + o_end) : d_meta + o_end;  // select: 128-bit rows
    size_t scan_bytes = 0;
    if (gapless) {
        HIP_TRY(c, mirsha::launch_offsets_scan(nullptr, scan_bytes, nullptr, nullptr, n, c->stream));
        HIP_TRY(c, c->d_scan.ensure(std::max<size_t>(scan_bytes, 4)));
    }
    OrderShape order_shape;
    if (dev_order)
        if (int rc = order_buffers(c, n, all.bmin, all.bmax, &order_shape)) return rc;
    if (!from_caller) HIP_TRY(c, sl.stage.ensure(std::max<uint64_t>(bytes, 8)));
    HIP_TRY(c, sl.dev.ensure(d_dig + 32ull * n));
    uint8_t* st = sl.stage.as<uint8_t>();
    ph[MIRSHA_PROF_PLAN] = ms_since(t0);
    tr[3] = ms_since(t_entry);
    t0 = Clock::now();
    uint8_t* dv = sl.dev.as<uint8_t>();
    RingQueued queued(c->xin, c->stream, c->xout);
    if (from_caller) {
        queued.arm();
        HIP_TRY(c, hipMemcpyAsync(dv, arena + lo, bytes, hipMemcpyHostToDevice, c->xin));
    } else if (dense) {
        mirsha::host::pack_range(arena + lo, nullptr, nullptr, nullptr, 0, nullptr, 0, bytes, st,
                                 mirsha::host::threads_for(bytes, 1u << 20), true);
    } else {
        std::vector<const uint8_t*> sp(n);
        std::vector<uint64_t> sz(n);
        std::vector<uint32_t> sf(n + 1);
        for (uint32_t i = 0; i < n; i++) {
            sp[i] = arena + off[i];
            sz[i] = len[i];
            sf[i] = i;
        }
        sf[n] = n;
        mirsha::host::pack(sp.data(), sz.data(), sf.data(), nullptr, n, soff, st, mirsha::host::threads_for(bytes, n),
                           true);
    }
    tr[4] = ms_since(t_entry);
    // Queue the copies and the kernel (a failure part-way: RingQueued).
    auto meta_h2d = [&](hipStream_t s) -> int {
        HIP_TRY(c, hipMemcpyAsync(dv + d_meta, mb, meta_copy, hipMemcpyHostToDevice, s));
        if (dev_order && !gapless)  // the offsets lie behind the order region, which stays on the device
            HIP_TRY(c, hipMemcpyAsync(dv + d_meta + o_off, mb + o_off, 8ull * n, hipMemcpyHostToDevice, s));
        return MIRSHA_OK;
    };
    auto queue = [&]() -> int {
        if (n) {
            queued.arm();
            if (!from_caller && bytes) HIP_TRY(c, hipMemcpyAsync(dv, st, bytes, hipMemcpyHostToDevice, c->xin));
            // The metadata: behind the request bytes on xin when the kernel
            // stores the digests (one copy stream), else on the kernel stream.
            // (the expectations of a mixed submission travel with it)
            if (kout)
                if (int rc = meta_h2d(c->xin)) return rc;
            if (kout && sel)
                if (int rc = expect_h2d(c, sl, *xa, c->xin)) return rc;
            HIP_TRY(c, hipEventRecord(sl.ev_in, c->xin));
            tq[0] = ms_since(t_entry);
            if (!kout)
                if (int rc = meta_h2d(c->stream)) return rc;
            if (!kout && sel)
                if (int rc = expect_h2d(c, sl, *xa, c->stream)) return rc;
            tq[1] = ms_since(t_entry);
            HIP_TRY(c, hipStreamWaitEvent(c->stream, sl.ev_in, 0));
            tq[2] = ms_since(t_entry);
            uint64_t* d_off = reinterpret_cast<uint64_t*>(dv + d_meta + o_off);
            const uint32_t* d_len = reinterpret_cast<const uint32_t*>(dv + d_meta + o_len);
            if (gapless)  // off = exclusive scan of len, on the device (c->d_scan: c->stream's scratch)
                HIP_TRY(c, mirsha::launch_offsets_scan(c->d_scan.p, scan_bytes, d_len, d_off, n, c->stream));
            if (dev_order)
                if (int rc = queue_bucket_order(c, order_shape, d_len, n,
                                                reinterpret_cast<uint32_t*>(dv + d_meta + o_ord)))
                    return rc;
            tq[3] = ms_since(t_entry);
            if (int rc = timed_launch(c, 0, [&] {
                    return hasher_launch_msgs(c, dv, bytes, d_off, d_len,
                                              identity ? nullptr
                                                       : reinterpret_cast<const uint32_t*>(dv + d_meta + o_ord),
                                              n, kout && !sel ? kout : dv + d_dig, c->stream);
                }))
                return rc;
            tq[4] = ms_since(t_entry);
            if (sel) {  // kept rows and verdict are in host memory when the verdict's copy ends
                if (int rc = expect_queue(c, sl, dv + d_dig, n, sel_rows)) return rc;
                HIP_TRY(c, hipEventRecord(sl.done, c->stream));
                tq[7] = ms_since(t_entry);
                return MIRSHA_OK;
            }
            if (kout) {  // the digests are in host memory when the kernel ends
                HIP_TRY(c, hipEventRecord(sl.done, c->stream));
                tq[7] = ms_since(t_entry);
                return MIRSHA_OK;
            }
            HIP_TRY(c, hipEventRecord(sl.ev_kern, c->stream));
            HIP_TRY(c, hipStreamWaitEvent(c->xout, sl.ev_kern, 0));
            tq[5] = ms_since(t_entry);
            HIP_TRY(c, hipMemcpyAsync(direct ? out : sl.dig.as<uint8_t>(), dv + d_dig, 32ull * n,
                                      hipMemcpyDeviceToHost, c->xout));
            tq[6] = ms_since(t_entry);
        }
        HIP_TRY(c, hipEventRecord(sl.done, c->xout));
        tq[7] = ms_since(t_entry);
        return MIRSHA_OK;
    };
    if (int rc = queue()) return rc;
    sl.t_queued = Clock::now();
    ph[MIRSHA_PROF_PACK] = ms_since(t0);
    tr[5] = ms_since(t_entry);
    trace_done("arena");
    owe(sl, rows, out, n, xa);
    ring_publish(c, sl, queued, ph, ticket_out);
    return MIRSHA_OK;
}

}  // namespace mirsha_api

extern "C" {

int mirsha_hash_slices_dedup(mirsha_ctx* c, const uint8_t* const* slice_ptr, const uint64_t* slice_len,
                             const uint32_t* slice_first, uint32_t n, uint8_t* out, uint32_t* n_unique_out) {
    if (!c) return MIRSHA_EINVAL;
    if (n_unique_out) *n_unique_out = 0;
    if (n == 0) return MIRSHA_OK;
    uint64_t t = 0;
    if (int rc = async_submit(c, slice_ptr, slice_len, slice_first, n, out, true, &t, n_unique_out))
        return rc;
    return async_wait_upto(c, t);
}

int mirsha_submit_slices(mirsha_ctx* c, const uint8_t* const* slice_ptr, const uint64_t* slice_len,
                         const uint32_t* slice_first, uint32_t n, uint8_t* out, int flags, uint64_t* ticket_out) {
    if (!c || !ticket_out) return MIRSHA_EINVAL;
    if (int rc = check_submit_flags(c, flags, false)) return rc;
    return async_submit(c, slice_ptr, slice_len, slice_first, n, out, (flags & MIRSHA_SUBMIT_DEDUP) != 0, ticket_out,
                        nullptr);
}

int mirsha_submit_batch(mirsha_ctx* c, const uint8_t* arena, uint64_t arena_len, const uint64_t* off,
                        const uint32_t* len, uint32_t n, uint8_t* digests_out, uint64_t* ticket_out) {
    if (!c || !ticket_out) return MIRSHA_EINVAL;
    if (n && (!off || !len || !digests_out || (!arena && arena_len))) return fail(c, MIRSHA_EINVAL, "NULL argument");
    return async_submit_arena(c, arena, arena_len, off, len, n, digests_out, ticket_out);
}

int mirsha_submit_slices_expect(mirsha_ctx* c, const uint8_t* const* slice_ptr, const uint64_t* slice_len,
                                const uint32_t* slice_first, uint32_t n, const uint32_t* expect_of,
                                const uint8_t* expected, uint32_t m, uint8_t* digests_out, uint64_t* bits_out,
                                uint32_t* n_mismatch_out, int flags, uint64_t* ticket_out) {
    if (!c || !ticket_out) return MIRSHA_EINVAL;
    if (int rc = check_submit_flags(c, flags, true)) return rc;
    const ExpectArgs xa{expect_of, expected, m, bits_out, n_mismatch_out};
    return async_submit(c, slice_ptr, slice_len, slice_first, n, digests_out, false, ticket_out, nullptr, &xa);
}

int mirsha_submit_batch_expect(mirsha_ctx* c, const uint8_t* arena, uint64_t arena_len, const uint64_t* off,
                               const uint32_t* len, uint32_t n, const uint32_t* expect_of, const uint8_t* expected,
                               uint32_t m, uint8_t* digests_out, uint64_t* bits_out, uint32_t* n_mismatch_out,
                               uint64_t* ticket_out) {
    if (!c || !ticket_out) return MIRSHA_EINVAL;
    if (n && (!off || !len || !digests_out || (!arena && arena_len))) return fail(c, MIRSHA_EINVAL, "NULL argument");
    const ExpectArgs xa{expect_of, expected, m, bits_out, n_mismatch_out};
    return async_submit_arena(c, arena, arena_len, off, len, n, digests_out, ticket_out, &xa);
}

int mirsha_hash_slices_expect(mirsha_ctx* c, const uint8_t* const* slice_ptr, const uint64_t* slice_len,
                              const uint32_t* slice_first, uint32_t n, const uint32_t* expect_of,
                              const uint8_t* expected, uint32_t m, uint8_t* digests_out, uint64_t* bits_out,
                              uint32_t* n_mismatch_out) {
    if (!c) return MIRSHA_EINVAL;
    uint64_t t = 0;
    const ExpectArgs xa{expect_of, expected, m, bits_out, n_mismatch_out};
    if (int rc = async_submit(c, slice_ptr, slice_len, slice_first, n, digests_out, false, &t, nullptr, &xa)) return rc;
    return async_wait_upto(c, t);
}

int mirsha_submit_slices_expect_dedup(mirsha_ctx* c, const uint8_t* const* slice_ptr, const uint64_t* slice_len,
                                      const uint32_t* slice_first, uint32_t n, const uint32_t* expect_of,
                                      const uint8_t* expected, uint32_t m, uint8_t* digests_out, uint64_t* bits_out,
                                      uint32_t* n_mismatch_out, uint32_t* n_unique_out, uint64_t* ticket_out) {
    if (!c || !ticket_out) return MIRSHA_EINVAL;
    const ExpectArgs xa{expect_of, expected, m, bits_out, n_mismatch_out};
    return async_submit(c, slice_ptr, slice_len, slice_first, n, digests_out, true, ticket_out, n_unique_out, &xa);
}

int mirsha_hash_slices_expect_dedup(mirsha_ctx* c, const uint8_t* const* slice_ptr, const uint64_t* slice_len,
                                    const uint32_t* slice_first, uint32_t n, const uint32_t* expect_of,
                                    const uint8_t* expected, uint32_t m, uint8_t* digests_out, uint64_t* bits_out,
                                    uint32_t* n_mismatch_out, uint32_t* n_unique_out) {
    if (!c) return MIRSHA_EINVAL;
    uint64_t t = 0;
    const ExpectArgs xa{expect_of, expected, m, bits_out, n_mismatch_out};
    if (int rc = async_submit(c, slice_ptr, slice_len, slice_first, n, digests_out, true, &t, n_unique_out, &xa))
        return rc;
    return async_wait_upto(c, t);
}

int mirsha_wait(mirsha_ctx* c, uint64_t ticket) {
    if (!c) return MIRSHA_EINVAL;
    if (ticket == 0 || ticket >= c->next_ticket) return fail(c, MIRSHA_EINVAL, "unknown ticket %llu", (unsigned long long)ticket);
    if (ticket <= c->done_ticket) return MIRSHA_OK;
    if (int rc = use_device(c)) return rc;
    return async_wait_upto(c, ticket);
}

int mirsha_poll(mirsha_ctx* c, uint64_t ticket, int* done) {
    if (!c || !done) return MIRSHA_EINVAL;
    if (ticket == 0 || ticket >= c->next_ticket) return fail(c, MIRSHA_EINVAL, "unknown ticket %llu", (unsigned long long)ticket);
    *done = 0;
    if (ticket <= c->done_ticket) {
        *done = 1;
        return MIRSHA_OK;
    }
    if (int rc = use_device(c)) return rc;
    for (uint64_t t = c->done_ticket + 1; t <= ticket; t++) {
        AsyncSlot& sl = c->slots[(t - 1) % kAsyncSlots];
        const hipError_t q = hipEventQuery(sl.done);
        if (q == hipErrorNotReady) {
            (void)hipGetLastError();  // not an error (see run_pipelined)
            return MIRSHA_OK;
        }
        if (q != hipSuccess) return fail(c, MIRSHA_EHIP, "hipEventQuery: %s", hipGetErrorString(q));
    }
    if (int rc = async_wait_upto(c, ticket)) return rc;
    *done = 1;
    return MIRSHA_OK;
}

}  // extern "C"
