// mirsha_streams.hip — streaming SHA-256 states on the device: Write / Sum /
// Reset over any bytes (mirsha_streams_*, include/mirsha.h; the kernel's
// contract is in mirsha_streams.h).  The hash.Hash boundary of the reference
// (`type Hasher func() hash.Hash`, processor.go:21) and an application log
// that writes more than whole digests (Log.Apply / Log.Snap,
// processor.go:28-31).  A translation unit of its own, as
// mirsha_commit_ring.hip: the hashing kernels keep their code object.
#include "mirsha_ctx.h"
#include "mirsha_streams.h"

namespace mirsha {

namespace {

constexpr uint32_t kStreamWave = 64;  // one wave per workgroup: the waves spread over the CUs
constexpr uint32_t kStateQuads = kStreamStateBytes / 16u;

// The bytes of big-endian message word i (block bytes 4 i .. 4 i + 3) that lie
// at block positions >= x, as a mask; x in [0, 64].
__device__ __forceinline__ uint32_t bytes_from(uint32_t x, int i) {
    // compare-free (a clamp and a 64-bit shift): 33 of these per step would
    // otherwise each hold a lane mask in an SGPR pair
    const int d = min(max((int)x - 4 * i, 0), 4);
    return (uint32_t)(0xFFFFFFFFull >> (8 * d));
}

// The 17 aligned words that hold the 64-byte window at arena offset a (mod
// 2^32).  A word at or above `span` -- behind the arena, or before it: an
// offset below zero wraps to the top of the 32 bits, above every span -- and
// every word of a lane that is not writing takes ld_u32's dead offset, which
// is outside the descriptor's range and reads as zero.
__device__ __forceinline__ void load_window(__amdgpu_buffer_rsrc_t rs, uint32_t span, bool wr, uint32_t a,
                                            uint32_t d[17]) {
    const uint32_t a0 = a & ~3u;
#pragma unroll
    for (int i = 0; i < 17; i++) {
        const uint32_t o = a0 + 4u * (uint32_t)i;
        d[i] = ld_u32(rs, o, wr && o < span);
    }
}

}  // namespace

// A step of a lane, at most one compression:
//   WRITE at buffer fill b: t = min(64 - b, bytes left) bytes join the block;
//     it is compressed when that fills it, else the step has no compression.
//     The bytes come from the 64-byte window that is block-aligned in STREAM
//     coordinates, at arena offset (write position) - b: 17 aligned words,
//     shifted by the window's address & 3 with one v_perm each, then merged
//     word by word under the byte mask [b, b + t).  The window may begin
//     before the arena or end behind it: a word at or above `span` (an
//     offset below zero wraps to the top of the 32 bits, above every span) is
//     not loaded (ld_u32's dead offset, outside the descriptor's range, reads
//     as zero), and its bytes are masked out.
//     Single-word loads: a wider load that straddles the range's end would
//     read zero for its in-range words too (the note above issue_chunk,
//     mirsha_kernels.hip).
//   SUM pads a COPY of the state: block bytes [0, b), 0x80, zeros, and the
//     64-bit bit length when b < 56; else the length goes into a second,
//     otherwise empty block in the next step (the copy's midstate waits in
//     hs[]).  The row is stored; the state stays as it was.
//   SUM_RESET is a SUM that then leaves Hasher(); RESET leaves it at once.
// The block stays in 16 named registers with static indices throughout.
__global__ __launch_bounds__(kStreamWave) void streams_kernel(
    const uint32_t* __restrict__ arena_words, uint32_t shift, uint32_t span, const uint32_t* __restrict__ act,
    const uint4* __restrict__ ent, uint32_t n_active, uint4* __restrict__ state, uint4* __restrict__ out) {
    const uint32_t* efirst = act + n_active;
    const uint32_t k = blockIdx.x * kStreamWave + threadIdx.x;
    const bool valid = k < n_active;
    const uint32_t s = valid ? act[k] : 0u;
    uint32_t e = valid ? efirst[k] : 0u;
    const uint32_t end = valid ? efirst[k + 1] : 0u;
    uint32_t st[8], hs[8], bw[16];
    uint64_t n = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        st[i] = kH0[i];
        hs[i] = 0u;
    }
#pragma unroll
    for (int i = 0; i < 16; i++) bw[i] = 0u;
    // one row of kStateWords per stream, one address for the load and the store
    uint4* const row = state + (uint64_t)kStateQuads * s;
    if (valid) {
        const uint4* hp = row;
        const uint4* bp = row + 2;
#pragma unroll
        for (int q = 0; q < 2; q++) {
            const uint4 v = hp[q];
            st[4 * q] = v.x; st[4 * q + 1] = v.y; st[4 * q + 2] = v.z; st[4 * q + 3] = v.w;
        }
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const uint4 v = bp[q];
            bw[4 * q] = v.x; bw[4 * q + 1] = v.y; bw[4 * q + 2] = v.z; bw[4 * q + 3] = v.w;
        }
        const uint4 v = row[6];
        n = (uint64_t)v.y << 32 | v.x;
    }
    const __amdgpu_buffer_rsrc_t rs = buffer_rsrc(arena_words, span);
    // Straight-line steps: the lane's conditions select values, the rounds run
    // on every lane when any lane's step has a compression (a wave instruction
    // costs the same at any exec mask), and the only divergent branch inside a
    // step guards the row's store.  A lane past its
    // end idles (op 4) until the wave's last lane is done.  An entry's record
    // is loaded unguarded at an index clamped into the lane's own range (the
    // note on commit_fetch, mirsha_device.h), or at 0 for an idle lane: a
    // launch has at least one entry.
    // The walk runs one step ahead of the hashing, as commit_fetch: which bytes
    // a step takes depends on the entries and the byte count only, never on a
    // hash value, so the next step's window (and the entry behind the next) is
    // requested before this step's rounds and arrives during them.
    uint4 x = ent[e < end ? e : 0u];
    uint4 xn = ent[e + 1u < end ? e + 1u : 0u];  // e <= end <= 2^30: no wrap
    uint32_t pos = 0u;
    uint32_t sum2 = 0u;  // 1: the second step of a SUM whose padding takes two blocks
    uint32_t d[17];
    load_window(rs, span, e < end && (x.x & 3u) == MIRSHA_STREAM_WRITE, x.z + shift - ((uint32_t)n & 63u), d);
    while (__ballot(e < end) != 0ull) {
        const uint32_t kind = x.x, len = x.y;
        const uint32_t off = x.z + shift;  // x.w, the offset's high word, is 0: span < 2^32
        const uint32_t op = e < end ? (kind & 3u) : 4u;
        const bool wr = op == MIRSHA_STREAM_WRITE;
        const bool sm = op == MIRSHA_STREAM_SUM || op == MIRSHA_STREAM_SUM_RESET;
        const uint32_t b = (uint32_t)n & 63u;
        const uint32_t t = wr ? min(64u - b, len - pos) : 0u;
        // the window: block byte j = arena byte a + j (mod 2^32: see above)
        const uint32_t sel = be_sel((off + pos - b) & 3u);
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const uint32_t m = bytes_from(b, i) & ~bytes_from(b + t, i);  // t == 0: nothing
            bw[i] = (bw[i] & ~m) | (be_word(d[i + 1], d[i], sel) & m);
        }
        const bool full = wr && b + t == 64u;
        const bool second = sm && sum2 != 0u;
        const bool fin = sm && (sum2 != 0u || b < 56u);  // this step ends the SUM
        const uint64_t bits = n << 3;                    // of a SUM: n is the whole message
        uint32_t w[16], ts[8];
        // lane conditions as words, so the padding is bit arithmetic
        const uint32_t pad = sm ? 0xFFFFFFFFu : 0u;       // a SUM step: pad a copy of the block
        const uint32_t keep = second ? 0u : 0xFFFFFFFFu;  // its second block holds the length only
        const uint32_t lenw = fin ? 0xFFFFFFFFu : 0u;
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const uint32_t tail = bytes_from(b, i);                            // bytes at and behind b
            const uint32_t mark = tail & ~bytes_from(b + 1u, i) & 0x80808080u;  // 0x80 at byte b
            w[i] = ((bw[i] & ~(tail & pad)) | (mark & pad)) & keep;
        }
        w[14] |= (uint32_t)(bits >> 32) & lenw;  // b < 56 or the second block: words 14, 15 are zero
        w[15] |= (uint32_t)bits & lenw;
#pragma unroll
        for (int i = 0; i < 8; i++) ts[i] = second ? hs[i] : st[i];
        // where the lane stands after this step, and the loads of the next one
        const bool fresh = op == MIRSHA_STREAM_RESET || (fin && op == MIRSHA_STREAM_SUM_RESET);
        const bool adv = (wr && pos + t == len) || fin || op == MIRSHA_STREAM_RESET;
        n = fresh ? 0ull : n + t;
        pos = adv ? 0u : pos + t;
        e += adv ? 1u : 0u;
        sum2 = (sm && !fin) ? 1u : 0u;
        if (adv) x = xn;
        load_window(rs, span, e < end && (x.x & 3u) == MIRSHA_STREAM_WRITE,
                    x.z + shift + pos - ((uint32_t)n & 63u), d);  // d's old values are merged already
        xn = ent[e + 1u < end ? e + 1u : 0u];
        // wave-uniform: skipped when no lane's step has a compression (short writes only)
        if (__ballot(full || sm) != 0ull) compress_asm_lat(ts, w);
        if (fin) {
            uint4* o = out + 2ull * (kind >> 2);
            o[0] = make_uint4(__builtin_bswap32(ts[0]), __builtin_bswap32(ts[1]), __builtin_bswap32(ts[2]),
                              __builtin_bswap32(ts[3]));
            o[1] = make_uint4(__builtin_bswap32(ts[4]), __builtin_bswap32(ts[5]), __builtin_bswap32(ts[6]),
                              __builtin_bswap32(ts[7]));
        }
#pragma unroll
        for (int i = 0; i < 8; i++) {
            hs[i] = ts[i];  // read only by the second step of a SUM, which follows its first
            st[i] = fresh ? kH0[i] : (full ? ts[i] : st[i]);
        }
    }
    if (valid) {
        uint4* hp = row;
        uint4* bp = row + 2;
#pragma unroll
        for (int q = 0; q < 2; q++) hp[q] = make_uint4(st[4 * q], st[4 * q + 1], st[4 * q + 2], st[4 * q + 3]);
#pragma unroll
        for (int q = 0; q < 4; q++) bp[q] = make_uint4(bw[4 * q], bw[4 * q + 1], bw[4 * q + 2], bw[4 * q + 3]);
        row[6] = make_uint4((uint32_t)n, (uint32_t)(n >> 32), 0u, 0u);
    }
}

hipError_t launch_streams(const uint32_t* arena_words, uint32_t shift, uint32_t span, const uint32_t* act,
                          const uint32_t* ent, uint32_t n_active, uint8_t* state, uint8_t* out, hipStream_t s) {
    if (n_active == 0) return hipSuccess;
    const uint32_t grid = (n_active + kStreamWave - 1u) / kStreamWave;
    launch_k(streams_kernel, grid, kStreamWave, 0, s, arena_words, shift, span, act, reinterpret_cast<const uint4*>(ent),
             n_active, reinterpret_cast<uint4*>(state), reinterpret_cast<uint4*>(out));
    return hipGetLastError();
}

}  // namespace mirsha

// Streaming hash states (see mirsha.h, mirsha_streams_create).
struct mirsha_streams {
    int device = 0;
    uint32_t n = 0;
    DevBuf d_state;  // kStreamStateBytes per stream (mirsha_streams.h)
    // mirsha_stream_plan's arrays of the call being run (kept across calls)
    std::vector<uint32_t> act, efirst, kind, len;
    std::vector<uint64_t> off, poff;
    // The call's block [act | efirst | pad to 16 | entries {kind, len, off lo,
    // off hi} | the written bytes, each distinct range once (host form)]: ONE
    // H2D copy.
    PinnedBuf stage;
    DevBuf dev, d_out;
};

namespace mirsha_api {

namespace {

constexpr uint32_t kStateBytes = MIRSHA_STREAM_STATE_BYTES;
constexpr uint32_t kRowWords = mirsha::kStreamStateBytes / 4u;  // a stream's row on the device
const uint8_t kStateMagic[4] = {'s', 'h', 'a', 3};

inline void put_be32(uint8_t* p, uint32_t v) {
    p[0] = (uint8_t)(v >> 24); p[1] = (uint8_t)(v >> 16); p[2] = (uint8_t)(v >> 8); p[3] = (uint8_t)v;
}
inline uint32_t get_be32(const uint8_t* p) {
    return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | (uint32_t)p[3];
}

// Both forms of mirsha_streams_run.  Order: every check and the plan (on the
// host, before anything is queued), the block in one copy, one launch, the
// values back, one synchronisation.
int streams_run(mirsha_ctx* c, mirsha_streams* st, const uint8_t* arena, bool on_device, uint64_t arena_len,
                const uint32_t* op_stream, const uint32_t* op_kind, const uint64_t* op_off, const uint32_t* op_len,
                uint32_t n_ops, uint8_t* values_out, uint32_t* n_values_out) {
    if (!c || !st || !n_values_out) return MIRSHA_EINVAL;
    *n_values_out = 0;
    if (n_ops == 0) return MIRSHA_OK;
    if (!op_stream || !op_kind) return fail(c, MIRSHA_EINVAL, "NULL argument");
    if (st->device != c->device) return fail(c, MIRSHA_EINVAL, "streams belong to another device");
    if (on_device && arena_len > MIRSHA_MAX_DEVICE_ARENA_BYTES)
        return fail(c, MIRSHA_ERANGE, "device arena of %llu bytes > %u", (unsigned long long)arena_len,
                    MIRSHA_MAX_DEVICE_ARENA_BYTES);
    const uint32_t cap = std::min(n_ops, st->n);
    st->act.resize(cap);
    st->efirst.resize((size_t)cap + 1u);
    st->kind.resize(n_ops);
    st->len.resize(n_ops);
    st->off.resize(n_ops);
    uint32_t na = 0, entries = 0, values = 0, bad = UINT32_MAX;
    uint64_t bytes = 0;
    const int rc = mirsha_stream_plan(op_stream, op_kind, op_off, op_len, n_ops, st->n, arena_len, 0, st->act.data(),
                                      st->efirst.data(), st->kind.data(), st->off.data(), st->len.data(), &na,
                                      &entries, &values, &bytes, &bad);
    if (rc == MIRSHA_ERANGE) return fail(c, rc, "%u ops > %u", n_ops, MIRSHA_STREAM_MAX_OPS);
    if (rc != MIRSHA_OK) {
        if (bad == UINT32_MAX) return fail(c, rc, "stream plan failed (a NULL op array?)");
        if (op_stream[bad] >= st->n) return fail(c, rc, "op_stream[%u] = %u >= %u", bad, op_stream[bad], st->n);
        if (op_kind[bad] > MIRSHA_STREAM_RESET) return fail(c, rc, "op_kind[%u] = %u is no kind", bad, op_kind[bad]);
        return fail(c, rc, "op %u writes [%llu, +%u) of an arena of %llu bytes", bad, (unsigned long long)op_off[bad],
                    op_len[bad], (unsigned long long)arena_len);
    }
    if (bytes && !arena) return fail(c, MIRSHA_EINVAL, "NULL arena (%llu bytes to write)", (unsigned long long)bytes);
    if (values && !values_out) return fail(c, MIRSHA_EINVAL, "NULL values_out (%u sums)", values);
    if (!on_device) {  // what crosses PCIe: every distinct range once (mirsha_stream_plan, pack)
        st->poff.resize(n_ops);
        bytes = mirsha::host::stream_pack_offsets(st->off.data(), st->len.data(), entries, st->poff.data());
        if (bytes + kArenaSlack > MIRSHA_MAX_DEVICE_ARENA_BYTES)
            return fail(c, MIRSHA_ERANGE, "%llu written bytes > %u", (unsigned long long)bytes,
                        MIRSHA_MAX_DEVICE_ARENA_BYTES - (uint32_t)kArenaSlack);
    }
    if (na == 0) return MIRSHA_OK;  // zero-length writes only
    if (int r = use_device(c)) return r;
    const uint64_t o_first = 4ull * na, o_ent = align16(o_first + 4ull * (na + 1u)), o_bytes = o_ent + 16ull * entries;
    const uint64_t h2d = o_bytes + (on_device ? 0ull : bytes);
    HIP_TRY(c, st->stage.ensure(h2d));
    HIP_TRY(c, st->dev.ensure(h2d + kArenaSlack));  // the last word of the bytes lies inside
    HIP_TRY(c, st->d_out.ensure(32ull * std::max(values, 1u)));
    uint8_t* sg = st->stage.as<uint8_t>();
    if (!on_device) {
        uint64_t at = 0;
        for (uint32_t e = 0; e < entries; e++) {
            if (st->len[e] && st->poff[e] == at) {  // the range's first entry: its bytes go in here
                memcpy(sg + o_bytes + at, arena + st->off[e], st->len[e]);
                at += st->len[e];
            }
            st->off[e] = st->poff[e];
        }
    }
    memcpy(sg, st->act.data(), 4ull * na);
    memcpy(sg + o_first, st->efirst.data(), 4ull * (na + 1u));
    uint32_t* rec = reinterpret_cast<uint32_t*>(sg + o_ent);  // the plan's entry arrays, one 16-byte record each
    for (uint32_t e = 0; e < entries; e++) {
        rec[4ull * e] = st->kind[e];
        rec[4ull * e + 1] = st->len[e];
        rec[4ull * e + 2] = (uint32_t)st->off[e];
        rec[4ull * e + 3] = (uint32_t)(st->off[e] >> 32);
    }
    HIP_TRY(c, hipMemcpyAsync(st->dev.p, sg, h2d, hipMemcpyHostToDevice, c->stream));
    const uint8_t* dv = st->dev.as<uint8_t>();
    // aligned words only: a word never crosses a page, so the up to 3 bytes
    // beside a device arena that share a word with it are safe to load
    const uintptr_t base = on_device ? reinterpret_cast<uintptr_t>(arena) : reinterpret_cast<uintptr_t>(dv + o_bytes);
    const uint32_t shift = (uint32_t)(base & 3u);
    const uint64_t extent = on_device ? arena_len : bytes;
    const uint32_t span = extent ? (uint32_t)((shift + extent + 3u) & ~3ull) : 0u;
    if (int r = timed_launch(c, kTimerStreams, [&] {
            return mirsha::launch_streams(
                reinterpret_cast<const uint32_t*>(base - shift), shift, span, reinterpret_cast<const uint32_t*>(dv),
                reinterpret_cast<const uint32_t*>(dv + o_ent), na,
                st->d_state.as<uint8_t>(), st->d_out.as<uint8_t>(), c->stream);
        }))
        return r;
    if (values) HIP_TRY(c, hipMemcpyAsync(values_out, st->d_out.p, 32ull * values, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    *n_values_out = values;
    return MIRSHA_OK;
}

int streams_which(mirsha_ctx* c, mirsha_streams* st, const uint32_t* which, uint32_t k, const void* rows) {
    if (!which || !rows) return fail(c, MIRSHA_EINVAL, "NULL argument");
    if (st->device != c->device) return fail(c, MIRSHA_EINVAL, "streams belong to another device");
    for (uint32_t j = 0; j < k; j++)
        if (which[j] >= st->n) return fail(c, MIRSHA_EINVAL, "which[%u] = %u >= %u", j, which[j], st->n);
    return use_device(c);
}

}  // namespace

}  // namespace mirsha_api

extern "C" {

int mirsha_streams_create(mirsha_ctx* c, uint32_t n, mirsha_streams** out) {
    if (!c || !out) return MIRSHA_EINVAL;
    *out = nullptr;
    if (n == 0) return fail(c, MIRSHA_EINVAL, "n_streams must be > 0");
    if (int rc = use_device(c)) return rc;
    auto* st = new mirsha_streams();
    st->device = c->device;
    st->n = n;
    constexpr uint32_t kWords = mirsha::kStreamStateBytes / 4u;
    std::vector<uint32_t> rows((size_t)kWords * n, 0u);  // Hasher(): H0, nothing buffered, count 0
    for (uint32_t i = 0; i < n; i++)
        for (int j = 0; j < 8; j++) rows[(size_t)kWords * i + j] = mirsha::kH0[j];
    auto up = [&]() -> int {
        HIP_TRY(c, st->d_state.ensure(4ull * rows.size()));
        HIP_TRY(c, hipMemcpyAsync(st->d_state.p, rows.data(), 4ull * rows.size(), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        return MIRSHA_OK;
    };
    if (int rc = up()) {
        mirsha_streams_destroy(st);
        return rc;
    }
    *out = st;
    return MIRSHA_OK;
}

void mirsha_streams_destroy(mirsha_streams* st) {
    if (!st) return;
    (void)hipSetDevice(st->device);
    for (DevBuf* b : {&st->d_state, &st->dev, &st->d_out}) b->release();
    st->stage.release();
    delete st;
}

int mirsha_streams_run(mirsha_ctx* c, mirsha_streams* st, const uint8_t* arena, uint64_t arena_len,
                       const uint32_t* op_stream, const uint32_t* op_kind, const uint64_t* op_off,
                       const uint32_t* op_len, uint32_t n_ops, uint8_t* values_out, uint32_t* n_values_out) {
    return streams_run(c, st, arena, false, arena_len, op_stream, op_kind, op_off, op_len, n_ops, values_out,
                       n_values_out);
}

int mirsha_streams_run_device(mirsha_ctx* c, mirsha_streams* st, const uint8_t* d_arena, uint64_t arena_len,
                              const uint32_t* op_stream, const uint32_t* op_kind, const uint64_t* op_off,
                              const uint32_t* op_len, uint32_t n_ops, uint8_t* values_out, uint32_t* n_values_out) {
    return streams_run(c, st, d_arena, true, arena_len, op_stream, op_kind, op_off, op_len, n_ops, values_out,
                       n_values_out);
}

int mirsha_streams_export(mirsha_ctx* c, mirsha_streams* st, const uint32_t* which, uint32_t k, uint8_t* out) {
    if (!c || !st) return MIRSHA_EINVAL;
    if (k == 0) return MIRSHA_OK;
    if (int rc = streams_which(c, st, which, k, out)) return rc;
    std::vector<uint32_t> rows((size_t)kRowWords * k);
    for (uint32_t j = 0; j < k; j++)
        HIP_TRY(c, hipMemcpyAsync(&rows[(size_t)kRowWords * j], st->d_state.as<uint32_t>() + (uint64_t)kRowWords * which[j],
                                  4u * kRowWords, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (uint32_t j = 0; j < k; j++) {
        const uint32_t* r = &rows[(size_t)kRowWords * j];  // [h 8 | block 16 | count lo, hi | 0, 0]
        uint8_t* row = out + (uint64_t)kStateBytes * j;
        memcpy(row, kStateMagic, 4);
        for (int i = 0; i < 8; i++) put_be32(row + 4 + 4 * i, r[i]);
        const uint32_t fill = r[24] & 63u;
        for (int i = 0; i < 16; i++) put_be32(row + 36 + 4 * i, r[8 + i]);
        memset(row + 36 + fill, 0, 64u - fill);  // behind the fill the block's words are stale
        put_be32(row + 100, r[25]);
        put_be32(row + 104, r[24]);
    }
    return MIRSHA_OK;
}

int mirsha_streams_import(mirsha_ctx* c, mirsha_streams* st, const uint32_t* which, uint32_t k, const uint8_t* in) {
    if (!c || !st) return MIRSHA_EINVAL;
    if (k == 0) return MIRSHA_OK;
    if (int rc = streams_which(c, st, which, k, in)) return rc;
    for (uint32_t j = 0; j < k; j++)
        if (memcmp(in + (uint64_t)kStateBytes * j, kStateMagic, 4) != 0)
            return fail(c, MIRSHA_EINVAL, "state %u does not begin with \"sha\\x03\"", j);
    std::vector<uint32_t> rows((size_t)kRowWords * k, 0u);
    for (uint32_t j = 0; j < k; j++) {
        const uint8_t* row = in + (uint64_t)kStateBytes * j;
        uint32_t* r = &rows[(size_t)kRowWords * j];
        for (int i = 0; i < 8; i++) r[i] = get_be32(row + 4 + 4 * i);
        for (int i = 0; i < 16; i++) r[8 + i] = get_be32(row + 36 + 4 * i);
        r[25] = get_be32(row + 100);
        r[24] = get_be32(row + 104);
        HIP_TRY(c, hipMemcpyAsync(st->d_state.as<uint32_t>() + (uint64_t)kRowWords * which[j], r, 4u * kRowWords,
                                  hipMemcpyHostToDevice, c->stream));
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return MIRSHA_OK;
}

}  // extern "C"
