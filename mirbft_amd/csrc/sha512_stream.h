// sha512_stream.h — one step of a stream programme under SHA-512/256: the
// analogue of StreamLane::step (mirsha_streams.h) for a 128-byte block, a
// 64-bit state and a 128-bit length.  Plain C++ as sha512_chain.h, so the CPU
// suite proves it (tests/c/sha512_stream_unit.cpp); the kernels of
// mirsha_sha512_streams.hip add the loader and the walk.
//
// State per stream: h[8] (u64), the unfinished block as 32 big-endian 32-bit
// words bw[32] (only its first n % 128 bytes mean anything) and n, the total
// bytes written (u64).
//
// A step is at most one compression:
//   WRITE at fill b = n & 127: t = min(128 - b, bytes left) bytes join the
//     block; it is compressed when that fills it.  The bytes come from the
//     128-byte window that is block-aligned in STREAM coordinates, at arena
//     offset a = (write position) - b (mod 2^32): the 33 aligned words from
//     a & ~3 on, each realigned by a & 3 and merged word by word under the
//     byte mask [b, b + t).  The caller loads the 33 words (a word outside the
//     arena is anything: its bytes are never under the mask).
//   SUM pads a COPY of the state: block bytes [0, b), 0x80, zeros, and when
//     b < 112 the 128-bit big-endian bit length (w[14] = n >> 61,
//     w[15] = n << 3); else the length goes into a second, otherwise empty
//     block in the next step, and the copy's midstate waits in hs[].  The row
//     is digest_words() of the result; the state stays as it was.
//   SUM_RESET is a SUM that then leaves Hasher() (kH0, n 0); RESET leaves it
//     at once.
// Above n = 2^61 Go's crypto/sha512 writes zero into the high 64 bits of the
// length where FIPS 180-4 has n >> 61; this is FIPS.  (Not tested: no stream
// gets there.)
//
// Which bytes a step takes depends on the entries and the byte count only
// (stream_plan and StreamWalk::advance read no hash value), so a caller may
// request the next step's window before this step's rounds.  Conditions select
// values: the only data-dependent branch a caller needs is the one that guards
// the row's store.  Every array is indexed statically.
#pragma once
#include "sha512_device.h"

namespace mirsha {
namespace sha512 {

constexpr uint32_t kStreamWrite = 0u, kStreamSum = 1u, kStreamSumReset = 2u, kStreamReset = 3u;  // = MIRSHA_STREAM_*
constexpr uint32_t kStreamIdle = 4u;       // a lane past its end
constexpr int kStreamWindowWords = 33;     // the aligned words that hold any 128-byte window

// The bytes of big-endian block word i (block bytes 4 i .. 4 i + 3) that lie
// at block positions >= x, as a mask; x in [0, 128], i in [0, 32).
// Compare-free on the device (a clamp and a 64-bit shift).
MIRSHA512_HD uint32_t stream_bytes_from(uint32_t x, int i) {
    int d = (int)x - 4 * i;
    d = d < 0 ? 0 : d;
    d = d > 4 ? 4 : d;
    return (uint32_t)(0xFFFFFFFFull >> (8 * d));
}

// Big-endian block word from two neighbouring aligned words as they lie in
// (little-endian) memory, lo at the lower address, realigned by r = a & 3
// bytes: bytes r .. r + 3 of lo:hi, the first one most significant.
MIRSHA512_HD uint32_t stream_be_word(uint32_t hi, uint32_t lo, uint32_t r) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(hi, lo, 0x00010203u + r * 0x01010101u);
#else
    return __builtin_bswap32((uint32_t)((((uint64_t)hi << 32) | lo) >> (8u * r)));
#endif
}

// What a step does, from the entry and the walk's counters alone.
struct StreamStep {
    uint32_t op;     // the entry's kind, kStreamIdle for a lane past its end
    uint32_t b, t;   // the block's fill on entry; bytes this step writes
    uint32_t row;    // SUM / SUM_RESET: the output row
    bool wr, sm;     // a write step / a step of a SUM or SUM_RESET
    bool full;       // the write fills the block: compress it
    bool second;     // the SUM's second block (the length only)
    bool fin;        // this step ends the SUM: the row is stored
    bool reset;      // the state behind the step is Hasher()
    bool adv;        // the step is the entry's last
};

// The walk's counters: n, the position inside the current write and whether a
// SUM's second block is due.
struct StreamWalk {
    uint64_t n;
    uint32_t pos, sum2;

    // The step at an entry {kind | row << 2, len}; `live`: the lane has one.
    MIRSHA512_HD StreamStep plan(uint32_t kind, uint32_t len, bool live) const {
        StreamStep s;
        s.op = live ? (kind & 3u) : kStreamIdle;
        s.row = kind >> 2;
        s.wr = s.op == kStreamWrite;
        s.sm = s.op == kStreamSum || s.op == kStreamSumReset;
        s.b = (uint32_t)n & 127u;
        const uint32_t room = 128u - s.b, left = len - pos;
        s.t = s.wr ? (room < left ? room : left) : 0u;
        s.full = s.wr && s.b + s.t == 128u;
        s.second = s.sm && sum2 != 0u;
        s.fin = s.sm && (sum2 != 0u || s.b < 112u);
        s.reset = s.op == kStreamReset || (s.fin && s.op == kStreamSumReset);
        s.adv = (s.wr && pos + s.t == len) || s.fin || s.op == kStreamReset;
        return s;
    }

    // Moves past the step; s.adv tells the caller to go to the next entry.
    MIRSHA512_HD void advance(const StreamStep& s) {
        n = s.reset ? 0ull : n + s.t;
        pos = s.adv ? 0u : pos + s.t;
        sum2 = (s.sm && !s.fin) ? 1u : 0u;
    }

    // The arena offset (mod 2^32) of the window of the step that comes next at
    // a write entry with offset `off`: block byte j is arena byte result + j.
    MIRSHA512_HD uint32_t window(uint32_t off) const { return off + pos - ((uint32_t)n & 127u); }
};

// A write step's bytes into the block: d[] = the 33 aligned words from
// a & ~3 on, r = a & 3 (a = StreamWalk::window of this step).  t == 0 (every
// step that is no write): nothing changes.
MIRSHA512_HD void stream_merge(uint32_t bw[32], const uint32_t d[kStreamWindowWords], uint32_t r, const StreamStep& s) {
    MIRSHA512_UNROLL
    for (int i = 0; i < 32; i++) {
        const uint32_t m = stream_bytes_from(s.b, i) & ~stream_bytes_from(s.b + s.t, i);
        bw[i] = (bw[i] & ~m) | (stream_be_word(d[i + 1], d[i], r) & m);
    }
}

// The step's compression input: the block itself (a write), or the padded copy
// (a SUM), from the block after stream_merge and n BEFORE StreamWalk::advance;
// ts = the midstate it starts from (hs for a SUM's second block).
MIRSHA512_HD void stream_block(const uint32_t bw[32], const uint64_t st[8], const uint64_t hs[8], uint64_t n,
                               const StreamStep& s, uint64_t w[16], uint64_t ts[8]) {
    // lane conditions as words, so the padding is bit arithmetic
    const uint32_t pad = s.sm ? 0xFFFFFFFFu : 0u;       // a SUM step: pad a copy of the block
    const uint32_t keep = s.second ? 0u : 0xFFFFFFFFu;  // its second block holds the length only
    const uint64_t lenw = s.fin ? ~0ull : 0ull;
    uint32_t pw[32];
    MIRSHA512_UNROLL
    for (int i = 0; i < 32; i++) {
        const uint32_t tail = stream_bytes_from(s.b, i);                                  // bytes at and behind b
        const uint32_t mark = tail & ~stream_bytes_from(s.b + 1u, i) & 0x80808080u;       // 0x80 at byte b
        pw[i] = ((bw[i] & ~(tail & pad)) | (mark & pad)) & keep;
    }
    join_words(pw, w);
    w[14] |= (n >> 61) & lenw;  // b < 112 or the second block: words 14, 15 are zero
    w[15] |= (n << 3) & lenw;
    MIRSHA512_UNROLL
    for (int i = 0; i < 8; i++) ts[i] = s.second ? hs[i] : st[i];
}

// The conditions that outlive the rounds, as one word: on the device a VGPR,
// where three lane masks would each hold an SGPR pair across the 80 rounds,
// beside the round constants.
constexpr uint32_t kStreamFin = 1u, kStreamToH0 = 2u, kStreamFull = 4u;
MIRSHA512_HD uint32_t stream_after(const StreamStep& s) {
    return (s.fin ? kStreamFin : 0u) | (s.reset ? kStreamToH0 : 0u) | (s.full ? kStreamFull : 0u);
}

// Behind the compression of ts: the state and the SUM's waiting midstate.
// (after & kStreamFin: the caller stores digest_words(ts) as the row first.)
MIRSHA512_HD void stream_finish(uint64_t st[8], uint64_t hs[8], const uint64_t ts[8], uint32_t after) {
    MIRSHA512_UNROLL
    for (int i = 0; i < 8; i++) {
        hs[i] = ts[i];  // read only by the second step of a SUM, which follows its first
        st[i] = (after & kStreamToH0) ? kH0[i] : ((after & kStreamFull) ? ts[i] : st[i]);
    }
}

}  // namespace sha512
}  // namespace mirsha
