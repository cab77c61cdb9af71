// mirsha_api.hip — host side of the C-ABI declared in include/mirsha.h:
// contexts, timing, the device-pointer API (the digest compare of
// mirsha_verify_* among it, and the bucket order and the offsets built on the
// device), synthetic streams and the clock probe.  The other host units are
// listed in mirsha_ctx.h.
#include "mirsha_ctx.h"

namespace mirsha_api {

int fail(mirsha_ctx* c, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (c) c->err = buf;
    return code;
}

hipEvent_t take_event(KernelTimer& t) {
    if (!t.pool.empty()) {
        hipEvent_t e = t.pool.back();
        t.pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
}

int use_device(mirsha_ctx* c) {
    HIP_TRY(c, hipSetDevice(c->device));
    return MIRSHA_OK;
}

// Stable sort of message indices by block count, longest first.
bool bucket_order(const uint32_t* len, uint32_t n, uint32_t* order) {
    if (n == 0) return true;
    uint32_t lo = UINT32_MAX, hi = 0;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t b = host_blocks(len[i]);
        lo = std::min(lo, b);
        hi = std::max(hi, b);
    }
    if (lo == hi) {
        for (uint32_t i = 0; i < n; i++) order[i] = i;
        return true;
    }
    const uint64_t range = (uint64_t)hi - lo + 1;
    if (range <= (1u << 22)) {
        std::vector<uint32_t> count(range + 1, 0);
        for (uint32_t i = 0; i < n; i++) count[hi - host_blocks(len[i]) + 1]++;
        for (uint64_t k = 1; k <= range; k++) count[k] += count[k - 1];
        for (uint32_t i = 0; i < n; i++) order[count[hi - host_blocks(len[i])]++] = i;
    } else {
        for (uint32_t i = 0; i < n; i++) order[i] = i;
        std::stable_sort(order, order + n, [&](uint32_t a, uint32_t b) {
            return host_blocks(len[a]) > host_blocks(len[b]);
        });
    }
    return false;
}

int check_lists(mirsha_ctx* c, const uint32_t* idx, const uint32_t* first, uint32_t n_lists,
                uint32_t n_digests) {
    if (!first) return fail(c, MIRSHA_EINVAL, "list_first is NULL");
    if (n_digests > mirsha::kMaxListDigests) return fail(c, MIRSHA_ERANGE, "%u digests > %u", n_digests, mirsha::kMaxListDigests);
    if (first[0] != 0) return fail(c, MIRSHA_EINVAL, "list_first[0] must be 0");
    for (uint32_t b = 0; b < n_lists; b++)
        if (first[b + 1] < first[b]) return fail(c, MIRSHA_EINVAL, "list_first not monotone at %u", b);
    const uint32_t entries = first[n_lists];
    if (entries && !idx) return fail(c, MIRSHA_EINVAL, "idx is NULL");
    if (entries > mirsha::kMaxListEntries) return fail(c, MIRSHA_ERANGE, "%u list entries > %u", entries, mirsha::kMaxListEntries);
    std::atomic<uint32_t> bad{UINT32_MAX};
    mirsha::host::parallel_for(entries, mirsha::host::threads_for(4ull * entries, entries), [&](uint32_t a, uint32_t b) {
        for (uint32_t e = a; e < b; e++)
            if (idx[e] != MIRSHA_NULL_INDEX && idx[e] >= n_digests) {
                uint32_t cur = bad.load();
                while (e < cur && !bad.compare_exchange_weak(cur, e)) {}
                return;
            }
    });
    if (const uint32_t e = bad.load(); e != UINT32_MAX)
        return fail(c, MIRSHA_EINVAL, "idx[%u]=%u out of range (%u digests)", e, idx[e], n_digests);
    // 32 bytes per digest must fit a 32-bit message length.
    for (uint32_t b = 0; b < n_lists; b++)
        if ((uint64_t)(first[b + 1] - first[b]) * 32u > MIRSHA_MAX_MESSAGE_BYTES)
            return fail(c, MIRSHA_ERANGE, "list %u too long", b);
    return MIRSHA_OK;
}

int queue_verify(mirsha_ctx* c, const uint8_t* d_digests, const uint8_t* d_expected, uint32_t n, uint64_t* d_bits,
                 uint32_t* d_count) {
    HIP_TRY(c, hipMemsetAsync(d_count, 0, sizeof(uint32_t), c->stream));
    if (n == 0) return MIRSHA_OK;
    return timed_launch(c, kTimerVerify, [&] {
        return mirsha::launch_verify_digests(d_digests, d_expected, n, d_bits, d_count, c->stream);
    });
}

int order_buffers(mirsha_ctx* c, uint32_t n, uint32_t bmin, uint32_t bmax, OrderShape* shape) {
    OrderShape& sh = *shape;
    sh.bmax = bmax;
    sh.bins = bmax - bmin + 1u;
    sh.chunk = mirsha::host::order_chunk(sh.bins);
    sh.n_chunks = (uint32_t)(((uint64_t)n + sh.chunk - 1u) / sh.chunk);
    const size_t cells = (size_t)sh.bins * sh.n_chunks;
    sh.scan_bytes = 0;
    HIP_TRY(c, mirsha::launch_counts_scan(nullptr, sh.scan_bytes, nullptr, nullptr, cells, c->stream));
    HIP_TRY(c, c->d_scan.ensure(std::max<size_t>(sh.scan_bytes, 4)));
    HIP_TRY(c, c->d_order_counts.ensure(std::max<size_t>(8u * cells, 8)));
    return MIRSHA_OK;
}

int queue_bucket_order(mirsha_ctx* c, const OrderShape& sh, const uint32_t* d_len, uint32_t n, uint32_t* d_order) {
    uint32_t* counts = c->d_order_counts.as<uint32_t>();
    const size_t cells = (size_t)sh.bins * sh.n_chunks;
    uint32_t* base = counts + cells;
    if (int rc = timed_launch(c, kTimerOrder, [&] {
            return mirsha::launch_order_count(d_len, n, sh.bmax, sh.bins, sh.chunk, sh.n_chunks, counts, c->stream);
        }))
        return rc;
    size_t scan_bytes = sh.scan_bytes;
    HIP_TRY(c, mirsha::launch_counts_scan(c->d_scan.p, scan_bytes, counts, base, cells, c->stream));
    return timed_launch(c, kTimerOrder, [&] {
        return mirsha::launch_order_scatter(d_len, n, sh.bmax, sh.bins, sh.chunk, sh.n_chunks, base, d_order,
                                            c->stream);
    });
}

}  // namespace mirsha_api

extern "C" {

int mirsha_version(void) { return (0 << 16) | 2; }

int mirsha_device_count(int* count) {
    if (!count) return MIRSHA_EINVAL;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        n = 0;
    }
    *count = n;
    return MIRSHA_OK;
}

int mirsha_ctx_create(int device, mirsha_ctx** out) {
    if (!out) return MIRSHA_EINVAL;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        return MIRSHA_ENODEV;
    }
    if (device < 0 || device >= n) return MIRSHA_EINVAL;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return MIRSHA_EHIP;
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return MIRSHA_ENODEV;  // gfx950 code objects only
    mirsha_ctx* c = new mirsha_ctx();
    c->device = device;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&c->own, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return MIRSHA_EHIP;
    }
    c->stream = c->own;
    *out = c;
    return MIRSHA_OK;
}

void mirsha_ctx_destroy(mirsha_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    if (c->xin) (void)hipStreamSynchronize(c->xin);
    if (c->xout) (void)hipStreamSynchronize(c->xout);
    if (c->xcommit) (void)hipStreamSynchronize(c->xcommit);
    for (auto& t : c->timers) {
        for (auto& pr : t.pending) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
        for (auto e : t.pool) (void)hipEventDestroy(e);
    }
    c->d_arena.release(); c->d_off.release(); c->d_len.release(); c->d_order.release();
    c->d_out.release(); c->d_idx.release(); c->d_first.release(); c->d_out2.release(); c->d_scratch.release();
    c->d_scan.release();
    c->d_order_counts.release();
    for (int k = 0; k < kStageSlots; k++) {
        c->h_ring[k].release();
        if (c->ring_ev[k]) (void)hipEventDestroy(c->ring_ev[k]);
    }
    c->h_meta.release();
    c->h_outs.release();
    c->d_meta.release();
    c->h_expect.release(); c->h_verdict.release(); c->d_expect.release(); c->d_verdict.release();
    for (auto e : c->xev) (void)hipEventDestroy(e);
    if (c->xin) (void)hipStreamDestroy(c->xin);
    if (c->xout) (void)hipStreamDestroy(c->xout);
    if (c->xcommit) (void)hipStreamDestroy(c->xcommit);
    for (auto& sl : c->slots) {
        sl.stage.release(); sl.dig.release(); sl.dev.release(); sl.stage2.release(); sl.dev2.release();
        sl.xp.stage.release(); sl.xp.verdict.release(); sl.xp.dev.release();
        sl.cm.stage.release(); sl.cm.dev.release(); sl.cm.snap.release(); sl.cm.rows.release();
        if (sl.done) (void)hipEventDestroy(sl.done);
        if (sl.ev_in) (void)hipEventDestroy(sl.ev_in);
        if (sl.ev_kern) (void)hipEventDestroy(sl.ev_kern);
    }
    if (c->own) (void)hipStreamDestroy(c->own);
    delete c;
}

const char* mirsha_last_error(const mirsha_ctx* c) { return c ? c->err.c_str() : "null context"; }

int mirsha_ctx_set_stream(mirsha_ctx* c, void* s) {
    if (!c) return MIRSHA_EINVAL;
    c->stream = s ? static_cast<hipStream_t>(s) : c->own;
    return MIRSHA_OK;
}

void* mirsha_ctx_stream(mirsha_ctx* c) { return c ? static_cast<void*>(c->stream) : nullptr; }

int mirsha_ctx_set_variant(mirsha_ctx* c, int v) {
    if (!c || !mirsha::variant_valid(v)) return MIRSHA_EINVAL;
    c->variant = v;
    return MIRSHA_OK;
}

int mirsha_ctx_set_timing(mirsha_ctx* c, int enable) {
    if (!c) return MIRSHA_EINVAL;
    c->timing = enable != 0;
    return MIRSHA_OK;
}

int mirsha_ctx_kernel_time(mirsha_ctx* c, int which, uint64_t* launches, double* total_ms) {
    if (!c || which < 0 || which >= kKernelTimers) return MIRSHA_EINVAL;
    if (int rc = use_device(c)) return rc;
    KernelTimer& t = c->timers[which];
    for (auto& pr : t.pending) {
        HIP_TRY(c, hipEventSynchronize(pr.second));
        float ms = 0.f;
        HIP_TRY(c, hipEventElapsedTime(&ms, pr.first, pr.second));
        t.ms += ms;
        t.launches++;
        t.pool.push_back(pr.first);
        t.pool.push_back(pr.second);
    }
    t.pending.clear();
    if (launches) *launches = t.launches;
    if (total_ms) *total_ms = t.ms;
    return MIRSHA_OK;
}

int mirsha_ctx_set_timing_mask(mirsha_ctx* c, uint32_t mask) {
    if (!c) return MIRSHA_EINVAL;
    c->time_mask = mask;
    return MIRSHA_OK;
}

int mirsha_ctx_reset_timing(mirsha_ctx* c) {
    if (!c) return MIRSHA_EINVAL;
    for (int k = 0; k < kKernelTimers; k++) {
        int rc = mirsha_ctx_kernel_time(c, k, nullptr, nullptr);
        if (rc) return rc;
        c->timers[k].launches = 0;
        c->timers[k].ms = 0.0;
    }
    return MIRSHA_OK;
}

int mirsha_sync(mirsha_ctx* c) {
    if (!c) return MIRSHA_EINVAL;
    if (int rc = use_device(c)) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return MIRSHA_OK;
}

int mirsha_host_alloc(mirsha_ctx* c, uint64_t bytes, void** out) {
    if (!c || !out) return MIRSHA_EINVAL;
    *out = nullptr;
    if (int rc = use_device(c)) return rc;
    HIP_TRY(c, hipHostMalloc(out, std::max<uint64_t>(bytes, 1), hipHostMallocDefault));
    return MIRSHA_OK;
}

void mirsha_host_free(void* p) {
    if (p) (void)hipHostFree(p);
}

int mirsha_hash_batch_device(mirsha_ctx* c, const uint8_t* d_arena, uint64_t arena_len,
                             const uint64_t* d_off, const uint32_t* d_len, const uint32_t* d_order,
                             uint32_t n, uint8_t* d_out) {
    if (!c) return MIRSHA_EINVAL;
    if (n == 0) return MIRSHA_OK;
    if (!d_off || !d_len || !d_out || (!d_arena && arena_len)) return fail(c, MIRSHA_EINVAL, "NULL argument");
    if (c->hasher == MIRSHA_HASHER_SHA512_256 && (arena_len > mirsha::kMaxBufferArena || n >= mirsha::kMaxBufferMsgs))
        return fail(c, MIRSHA_ERANGE, "hasher sha512_256: arena_len %llu > %llu or n %u >= %u (one buffer descriptor)",
                    (unsigned long long)arena_len, (unsigned long long)mirsha::kMaxBufferArena, n,
                    mirsha::kMaxBufferMsgs);
    if (int rc = use_device(c)) return rc;
    return timed_launch(c, 0, [&] {
        return hasher_launch_msgs(c, d_arena, arena_len, d_off, d_len, d_order, n, d_out, c->stream);
    });
}

int mirsha_digest_lists_device(mirsha_ctx* c, const uint8_t* d_digests, uint32_t n_digests, const uint32_t* d_idx,
                               const uint32_t* d_first, uint32_t n_lists, uint32_t n_entries, uint8_t* d_out) {
    if (!c) return MIRSHA_EINVAL;
    if (n_lists == 0) return MIRSHA_OK;
    if (!d_idx || !d_first || !d_out) return fail(c, MIRSHA_EINVAL, "NULL argument");
    if (n_digests > mirsha::kMaxListDigests) return fail(c, MIRSHA_ERANGE, "n_digests %u too large", n_digests);
    if (n_entries > mirsha::kMaxListEntries) return fail(c, MIRSHA_ERANGE, "n_entries %u too large", n_entries);
    if (int rc = use_device(c)) return rc;
    HIP_TRY(c, c->d_scratch.ensure(sizeof(uint32_t) * std::max<uint32_t>(n_entries, 1)));
    return timed_launch(c, 1, [&] {
        return hasher_launch_lists(c, d_digests, n_digests, d_idx, n_entries, d_first, n_lists,
                                   c->d_scratch.as<uint32_t>(), d_out, c->stream);
    });
}

int mirsha_verify_digests_device(mirsha_ctx* c, const uint8_t* d_digests, const uint8_t* d_expected, uint32_t n,
                                 uint64_t* d_bits_out, uint32_t* d_count_out) {
    if (!c) return MIRSHA_EINVAL;
    if (!d_count_out) return fail(c, MIRSHA_EINVAL, "NULL argument");
    if (n && (!d_digests || !d_expected || !d_bits_out)) return fail(c, MIRSHA_EINVAL, "NULL argument");
    if (n && (((uintptr_t)d_digests | (uintptr_t)d_expected) & 15u))
        return fail(c, MIRSHA_EINVAL, "digest arrays must be 16-byte aligned");
    if (n && ((uintptr_t)d_bits_out & 7u)) return fail(c, MIRSHA_EINVAL, "bitmap must be 8-byte aligned");
    if ((uintptr_t)d_count_out & 3u) return fail(c, MIRSHA_EINVAL, "count must be 4-byte aligned");
    if (int rc = use_device(c)) return rc;
    return queue_verify(c, d_digests, d_expected, n, d_bits_out, d_count_out);
}

int mirsha_bucket_order(const uint32_t* len, uint32_t n, uint32_t* order_out) {
    if (n && (!len || !order_out)) return MIRSHA_EINVAL;
    return bucket_order(len, n, order_out) ? 1 : 0;
}

int mirsha_bucket_order_device(mirsha_ctx* c, const uint32_t* d_len, uint32_t n, uint32_t min_len, uint32_t max_len,
                               uint32_t* d_order_out) {
    if (!c) return MIRSHA_EINVAL;
    if (min_len > max_len) return fail(c, MIRSHA_EINVAL, "min_len %u > max_len %u", min_len, max_len);
    const uint32_t bmin = host_blocks(min_len), bmax = host_blocks(max_len);
    if (bmax - bmin >= MIRSHA_ORDER_MAX_BINS)
        return fail(c, MIRSHA_ERANGE, "%u block-count bins > %u", bmax - bmin + 1u, MIRSHA_ORDER_MAX_BINS);
    if (n == 0) return 1;
    if (!d_len || !d_order_out) return fail(c, MIRSHA_EINVAL, "NULL argument");
    if (int rc = use_device(c)) return rc;
    if (bmin == bmax) {
        if (int rc = timed_launch(c, kTimerOrder, [&] { return mirsha::launch_order_iota(d_order_out, n, c->stream); }))
            return rc;
        return 1;
    }
    OrderShape sh;
    if (int rc = order_buffers(c, n, bmin, bmax, &sh)) return rc;
    return queue_bucket_order(c, sh, d_len, n, d_order_out);
}

int mirsha_offsets_device(mirsha_ctx* c, const uint32_t* d_len, uint32_t n, uint64_t* d_off_out) {
    if (!c) return MIRSHA_EINVAL;
    if (n == 0) return MIRSHA_OK;
    if (!d_len || !d_off_out) return fail(c, MIRSHA_EINVAL, "NULL argument");
    if (int rc = use_device(c)) return rc;
    size_t scan_bytes = 0;
    HIP_TRY(c, mirsha::launch_offsets_scan(nullptr, scan_bytes, nullptr, nullptr, n, c->stream));
    HIP_TRY(c, c->d_scan.ensure(std::max<size_t>(scan_bytes, 4)));
    HIP_TRY(c, mirsha::launch_offsets_scan(c->d_scan.p, scan_bytes, d_len, d_off_out, n, c->stream));
    return MIRSHA_OK;
}

int mirsha_ctx_set_order_mode(mirsha_ctx* c, int mode) {
    if (!c) return MIRSHA_EINVAL;
    if (mode != MIRSHA_ORDER_HOST && mode != MIRSHA_ORDER_DEVICE)
        return fail(c, MIRSHA_EINVAL, "order mode %d (0 = host, 1 = device)", mode);
    c->order_mode = mode;
    return MIRSHA_OK;
}

int mirsha_ctx_order_mode(const mirsha_ctx* c) { return c ? c->order_mode : MIRSHA_EINVAL; }

int mirsha_ctx_set_hasher(mirsha_ctx* c, int hasher) {
    if (!c) return MIRSHA_EINVAL;
    if (mirsha_hasher_info(hasher, nullptr, nullptr) != MIRSHA_OK)
        return fail(c, MIRSHA_EINVAL, "hasher %d (0 = sha256, 1 = sha512_256)", hasher);
    c->hasher = hasher;
    return MIRSHA_OK;
}

int mirsha_ctx_hasher(const mirsha_ctx* c) { return c ? c->hasher : MIRSHA_EINVAL; }

int mirsha_hasher_info(int hasher, uint32_t* digest_bytes, uint32_t* block_bytes) {
    if (hasher != MIRSHA_HASHER_SHA256 && hasher != MIRSHA_HASHER_SHA512_256) return MIRSHA_EINVAL;
    if (digest_bytes) *digest_bytes = 32u;
    if (block_bytes) *block_bytes = hasher == MIRSHA_HASHER_SHA512_256 ? 128u : 64u;
    return MIRSHA_OK;
}

int mirsha_sha512_pair_max_groups(void) { return (int)mirsha::sha512_pair_max_groups(); }

int mirsha_ctx_sha512_pair_launches(const mirsha_ctx* c, uint64_t* out) {
    if (!c || !out) return MIRSHA_EINVAL;
    *out = c->sha512_pair_launches;
    return MIRSHA_OK;
}

int mirsha_synth_mixed_lengths_device(mirsha_ctx* c, uint64_t seed, uint64_t first, uint64_t count,
                                      uint32_t* d_len) {
    if (!c) return MIRSHA_EINVAL;
    if (count && !d_len) return fail(c, MIRSHA_EINVAL, "NULL length buffer");
    if (int rc = use_device(c)) return rc;
    return timed_launch(c, 2, [&] { return mirsha::launch_mixed_lengths(seed, first, count, d_len, c->stream); });
}

int mirsha_synth_mixed_device(mirsha_ctx* c, uint64_t seed, uint64_t first, uint64_t count, const uint64_t* d_off,
                              uint8_t* d_arena) {
    if (!c) return MIRSHA_EINVAL;
    if (count && (!d_off || !d_arena)) return fail(c, MIRSHA_EINVAL, "NULL argument");
    if (int rc = use_device(c)) return rc;
    return timed_launch(c, 2, [&] { return mirsha::launch_gen_mixed(seed, first, count, d_off, d_arena, c->stream); });
}

int mirsha_synth_requests_device(mirsha_ctx* c, uint64_t seed, uint64_t first, uint64_t count, uint32_t data_len,
                                 uint8_t* d_arena) {
    if (!c) return MIRSHA_EINVAL;
    if (count && !d_arena) return fail(c, MIRSHA_EINVAL, "NULL arena");
    if (int rc = use_device(c)) return rc;
    return timed_launch(c, 2, [&] { return mirsha::launch_gen_requests(seed, first, count, data_len, d_arena, c->stream); });
}

int mirsha_ctx_host_profile(const mirsha_ctx* c, double* ms_out, int n) {
    if (!c || !ms_out || n < 0) return MIRSHA_EINVAL;
    for (int k = 0; k < n && k < MIRSHA_PROF_PHASES; k++) ms_out[k] = c->prof[k];
    return MIRSHA_PROF_PHASES;
}

int mirsha_clock_probe(mirsha_ctx* c, uint32_t iters, double* clock_ghz, double* cycles_per_wave_compression) {
    if (!c || !clock_ghz || !cycles_per_wave_compression || iters == 0) return MIRSHA_EINVAL;
    if (int rc = use_device(c)) return rc;
    hipDeviceProp_t prop;
    HIP_TRY(c, hipGetDeviceProperties(&prop, c->device));
    // One 256-thread workgroup = one wave per SIMD of a CU; kProbeWavesPerSimd per CU
    // (MIRSHA_AB=1 MIRSHA_PROBE_WAVES=k: k per SIMD, occupancy A/B).
    uint32_t wps = mirsha::kProbeWavesPerSimd;
    if (const char* e = mirsha::ab_getenv("MIRSHA_PROBE_WAVES")) wps = std::min(8u, std::max(1u, (uint32_t)atoi(e)));
    const uint32_t blocks = (uint32_t)prop.multiProcessorCount * wps;
    const uint32_t waves = 4u * blocks;
    DevBuf stamps, sink;
    HIP_TRY(c, stamps.ensure(24ull * waves));
    HIP_TRY(c, sink.ensure(4ull * 256u * blocks));
    int rc = timed_launch(c, 2, [&] {
        return mirsha::launch_clock_probe(blocks, iters, stamps.as<unsigned long long>(), sink.as<uint32_t>(),
                                          c->stream);
    });
    std::vector<unsigned long long> h(3ull * waves);
    if (rc == MIRSHA_OK) {
        hipError_t e = hipMemcpyAsync(h.data(), stamps.p, 24ull * waves, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) rc = fail(c, MIRSHA_EHIP, "clock probe: %s", hipGetErrorString(e));
    }
    stamps.release();
    sink.release();
    if (rc) return rc;
    std::vector<double> ghz(waves);
    unsigned long long first = ~0ull, last = 0;
    for (uint32_t w = 0; w < waves; w++) {
        const unsigned long long r0 = h[3 * w + 1], r1 = h[3 * w + 2];
        ghz[w] = r1 > r0 ? 0.1 * (double)h[3 * w] / (double)(r1 - r0) : 0.0;
        first = std::min(first, r0);
        last = std::max(last, r1);
    }
    std::nth_element(ghz.begin(), ghz.begin() + waves / 2, ghz.end());
    *clock_ghz = ghz[waves / 2];
    // Span in shader cycles at that clock, per SIMD, per wave-compression.
    const double span_cycles = (double)(last - first) * 10.0 * *clock_ghz;
    *cycles_per_wave_compression = span_cycles / ((double)iters * wps);
    return MIRSHA_OK;
}

}  // extern "C"
