// mirsha_streams.h — the kernels of the streaming hash states
// (mirsha_streams.hip, mirsha_streams_ring.hip; mirsha_streams_* in
// include/mirsha.h): SHA-256 states that take Write / Sum / Reset over any
// bytes, as a hash.Hash does (processor.go:21), where the checkpoint chains
// take whole 32-byte digests.
//
// State of stream s, device-resident and kept across calls: row s of
// kStreamStateBytes bytes of one array (one address per lane for the load and
// the store), as u32 words
//   [0, 8)    the midstate
//   [8, 24)   the unfinished block as big-endian message words; only its
//             first count % 64 bytes mean anything
//   24, 25    the total bytes written (u64: low word, high word)
//   26, 27    unused (the row is a whole number of 16-byte accesses)
//
// One lane per active stream (streams_kernel) or per segment of one
// (streams_seg_kernel) walks its entries (mirsha_stream_plan's arrays) in
// steps of at most one compression (StreamLane::step, the one statement of the
// step), in a wave-uniform loop closed by a ballot: no atomics, no waiting, no
// cross-lane dependence.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mirsha.h"
#include "mirsha_device.h"

namespace mirsha {

constexpr uint32_t kStreamStateBytes = 112;
constexpr uint32_t kStreamWave = 64;  // one wave per workgroup: the waves spread over the CUs
constexpr uint32_t kStateQuads = kStreamStateBytes / 16u;

// arena_words: the arena's address rounded down to 4 bytes; `shift` (0-3) is
// what was rounded off and is added to every entry offset; `span` = the bytes
// from arena_words to the arena's end rounded up to 4 (at most 2^32 - 128):
// the kernel loads aligned 4-byte words inside [0, span) only, any other
// address reads as zero.  act[0, n_active) is followed by efirst[0, n_active];
// lane k runs entries [efirst[k], efirst[k + 1]) on stream act[k].  Entry e is
// the 16-byte record ent[4 e ..] = {ent_kind, ent_len, ent_off low, ent_off
// high} of mirsha_stream_plan's arrays (16-byte aligned: one load per entry).
// A SUM / SUM_RESET entry stores its 32-byte row of `out` (16-byte aligned),
// as is `state`.
hipError_t launch_streams(const uint32_t* arena_words, uint32_t shift, uint32_t span, const uint32_t* act,
                          const uint32_t* ent, uint32_t n_active, uint8_t* state, uint8_t* out, hipStream_t s);

// mirsha_streams_ring.hip.  The programme cut into segments
// (mirsha_stream_seg_plan's arrays), one lane per segment: lane k runs entries
// [sfirst[k], sfirst[k + 1]) on stream seg_stream[k].  A FIRST segment starts
// from its stream's row of state_in (the streams' own array, or a copy of it
// taken on the stream ahead of the launch), every other one from Hasher(); a
// LAST segment stores the state it ends in to its row of `state`.  The arena,
// the entries and `out` as above; `out` may be host-visible page-locked memory
// (plain vector stores).  `prio`: the issue priority (0-3) the waves take at
// entry.
hipError_t launch_streams_seg(const uint32_t* arena_words, uint32_t shift, uint32_t span, const uint32_t* seg_stream,
                              const uint32_t* sfirst, const uint32_t* seg_flags, const uint32_t* ent, uint32_t n_seg,
                              const uint8_t* state_in, uint8_t* state, uint8_t* out, uint32_t prio, hipStream_t s);

// What a hasher's streams are to the host (mirsha_streams.hip): the row's
// size, the exported state, and the launchers of its two kernels, which follow
// the contracts of launch_streams / launch_streams_seg above with rows of
// row_bytes.  The SHA-512/256 row's kernels: mirsha_sha512_streams.h.
struct StreamKernels {
    uint32_t row_bytes;     // a stream's row on the device (16-byte multiple)
    uint32_t export_bytes;  // one exported state (mirsha_stream_state_bytes)
    uint8_t magic[4];       // its first four bytes
    void (*row0)(uint8_t* row);                       // Hasher() as a device row
    void (*pack)(const uint8_t* row, uint8_t* out);   // a device row -> the exported state behind the magic
    void (*unpack)(const uint8_t* in, uint8_t* row);  // its inverse: every byte of the row is written
    decltype(&launch_streams) run;
    decltype(&launch_streams_seg) seg;
};
const StreamKernels& stream_kernels(int hasher);

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

// What a launch's lanes share: the arena's descriptor and the entry records.
struct StreamArgs {
    __amdgpu_buffer_rsrc_t rs;
    uint32_t span, shift;
    const uint4* ent;
};

// A lane's walk over entries [e, end) of one stream.
//
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
//
// Straight-line steps: the lane's conditions select values, the rounds run
// on every lane when any lane's step has a compression (a wave instruction
// costs the same at any exec mask), and the only divergent branch inside a
// step guards the row's store.  A lane past its end idles (op 4) until the
// wave's last lane is done.  An entry's record is loaded unguarded at an index
// clamped into the lane's own range (the note on commit_fetch,
// mirsha_chains.hip), or at 0 for an idle lane: a launch has at least one entry.
// The walk runs one step ahead of the hashing, as commit_fetch: which bytes a
// step takes depends on the entries and the byte count only, never on a hash
// value, so the next step's window (and the entry behind the next) is
// requested before this step's rounds and arrives during them.
struct StreamLane {
    uint32_t st[8], hs[8], bw[16];
    uint64_t n;
    uint32_t e, end;
    uint32_t pos;
    uint32_t sum2;  // 1: the second step of a SUM whose padding takes two blocks
    uint4 x, xn;
    uint32_t d[17];

    // Hasher() -- H0, count 0, an all-zero block -- before entries [e0, e1).
    __device__ __forceinline__ void fresh(uint32_t e0, uint32_t e1) {
#pragma unroll
        for (int i = 0; i < 8; i++) {
            st[i] = kH0[i];
            hs[i] = 0u;
        }
#pragma unroll
        for (int i = 0; i < 16; i++) bw[i] = 0u;
        n = 0;
        e = e0;
        end = e1;
        pos = 0u;
        sum2 = 0u;
    }

    // one row of kStateQuads per stream
    __device__ __forceinline__ void load_row(const uint4* row) {
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

    __device__ __forceinline__ void store_row(uint4* row) const {
        uint4* hp = row;
        uint4* bp = row + 2;
#pragma unroll
        for (int q = 0; q < 2; q++) hp[q] = make_uint4(st[4 * q], st[4 * q + 1], st[4 * q + 2], st[4 * q + 3]);
#pragma unroll
        for (int q = 0; q < 4; q++) bp[q] = make_uint4(bw[4 * q], bw[4 * q + 1], bw[4 * q + 2], bw[4 * q + 3]);
        row[6] = make_uint4((uint32_t)n, (uint32_t)(n >> 32), 0u, 0u);
    }

    __device__ __forceinline__ bool live() const { return e < end; }

    // The loads of the first step: its entry, the one behind it, its window.
    __device__ __forceinline__ void start(const StreamArgs& a) {
        x = a.ent[e < end ? e : 0u];
        xn = a.ent[e + 1u < end ? e + 1u : 0u];  // e <= end <= 2^30: no wrap
        load_window(a.rs, a.span, e < end && (x.x & 3u) == MIRSHA_STREAM_WRITE, x.z + a.shift - ((uint32_t)n & 63u), d);
    }

    __device__ __forceinline__ void step(const StreamArgs& a, uint4* out) {
        const uint32_t kind = x.x, len = x.y;
        const uint32_t off = x.z + a.shift;  // x.w, the offset's high word, is 0: span < 2^32
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
        const bool reset = op == MIRSHA_STREAM_RESET || (fin && op == MIRSHA_STREAM_SUM_RESET);
        const bool adv = (wr && pos + t == len) || fin || op == MIRSHA_STREAM_RESET;
        n = reset ? 0ull : n + t;
        pos = adv ? 0u : pos + t;
        e += adv ? 1u : 0u;
        sum2 = (sm && !fin) ? 1u : 0u;
        if (adv) x = xn;
        load_window(a.rs, a.span, e < end && (x.x & 3u) == MIRSHA_STREAM_WRITE,
                    x.z + a.shift + pos - ((uint32_t)n & 63u), d);  // d's old values are merged already
        xn = a.ent[e + 1u < end ? e + 1u : 0u];
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
            st[i] = reset ? kH0[i] : (full ? ts[i] : st[i]);
        }
    }
};

}  // namespace mirsha
