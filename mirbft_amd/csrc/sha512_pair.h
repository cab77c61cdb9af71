// sha512_pair.h — the SHA-512 compression split for a producer/consumer pair
// of waves (mirsha_sha512_pair.hip): the message schedule with the round
// constants added (K[j] + W[j], which never depends on the chaining state) on
// one side, the 80 rounds from those words on the other.
//
// The hand-over unit is a group of 16 rounds, the unit in which
// sha512::compress already stages K: five groups a block, 16 words = 128 bytes
// a lane, 8 KiB a wave.  A whole block of 80 words is 40 KiB a wave, so a ring
// of two such slots would not fit 64 KiB of static LDS; two group slots take
// 16 KiB.  The group index is a template argument, so every index into the
// window and into K is static.
//
// Plain C++ in the style of sha512_device.h, whose sigma / Sigma / Ch / Maj
// spellings and K staging it uses: compiles for the host as well, so the CPU
// suite proves it (tests/c/sha512_pair_unit.cpp), and includes nothing of HIP
// when the compiler is not hipcc.
#pragma once
#include "sha512_device.h"

namespace mirsha {
namespace sha512 {

constexpr int kPairGroups = 5;       // hand-overs a block
constexpr int kPairGroupWords = 16;  // KW words a hand-over

// Group G of a block's schedule: kw[i] = K[16 G + i] + W[16 G + i].  w[] holds
// the 16 message words before group 0 and is the rolling window afterwards, as
// in compress; groups are produced in order, 0 to 4.  The group's constants
// hang on compress's fence (tied to the window here), so they are fetched by
// scalar loads group by group and never hoisted out of the caller's loop.
template <int G>
MIRSHA512_HD void produce_group(uint64_t w[16], uint64_t kw[16]) {
    static_assert(G >= 0 && G < kPairGroups, "group of 16 rounds");
    KPtr kp = (KPtr)&MIRSHA512_K(0);
    uint64_t kc[16];
    MIRSHA512_K_FENCE(kp, w[0]);
    MIRSHA512_UNROLL
    for (int i = 0; i < 16; i++) kc[i] = kp[16 * G + i];
    MIRSHA512_UNROLL
    for (int i = 0; i < 16; i++) {
        // (the round's j is 16 G + i, so j & 15 == i)
        if (G > 0) w[i] += ssig1(w[(i + 14) & 15]) + w[(i + 9) & 15] + ssig0(w[(i + 1) & 15]);
        kw[i] = kc[i] + w[i];
    }
}

// 16 rounds on the working variables v[0..7] = a..h from one group's words.
// After 16 rounds the names are back where they started.
MIRSHA512_HD void consume_group(uint64_t v[8], const uint64_t kw[16]) {
    uint64_t a = v[0], b = v[1], c = v[2], d = v[3];
    uint64_t e = v[4], f = v[5], g = v[6], h = v[7];
#define MIRSHA512_KW_ROUND(a, b, c, d, e, f, g, h, i)                  \
    {                                                                  \
        const uint64_t t1 = h + bsig1(e) + ch(e, f, g) + kw[(i)];      \
        d += t1;                                                       \
        h = t1 + bsig0(a) + maj(a, b, c);                              \
    }
    MIRSHA512_UNROLL
    for (int i = 0; i < 16; i += 8) {
        MIRSHA512_KW_ROUND(a, b, c, d, e, f, g, h, i + 0);
        MIRSHA512_KW_ROUND(h, a, b, c, d, e, f, g, i + 1);
        MIRSHA512_KW_ROUND(g, h, a, b, c, d, e, f, i + 2);
        MIRSHA512_KW_ROUND(f, g, h, a, b, c, d, e, i + 3);
        MIRSHA512_KW_ROUND(e, f, g, h, a, b, c, d, i + 4);
        MIRSHA512_KW_ROUND(d, e, f, g, h, a, b, c, i + 5);
        MIRSHA512_KW_ROUND(c, d, e, f, g, h, a, b, i + 6);
        MIRSHA512_KW_ROUND(b, c, d, e, f, g, h, a, i + 7);
    }
#undef MIRSHA512_KW_ROUND
    v[0] = a; v[1] = b; v[2] = c; v[3] = d;
    v[4] = e; v[5] = f; v[6] = g; v[7] = h;
}

// The end of a block on the consumer's side: st += F only for a live block (a
// lane whose message is finished runs the rounds of whatever the producer
// handed over and drops them).
MIRSHA512_HD void finish_block(uint64_t st[8], const uint64_t v[8], bool live) {
    if (live) {
        MIRSHA512_UNROLL
        for (int i = 0; i < 8; i++) st[i] += v[i];
    }
}

// A whole block: the five groups in order.  produce_kw followed by consume_kw
// is sha512::compress bit for bit.
MIRSHA512_HD void produce_kw(uint64_t w[16], uint64_t kw[80]) {
    produce_group<0>(w, kw);
    produce_group<1>(w, kw + 16);
    produce_group<2>(w, kw + 32);
    produce_group<3>(w, kw + 48);
    produce_group<4>(w, kw + 64);
}

MIRSHA512_HD void consume_kw(uint64_t st[8], const uint64_t kw[80], bool live) {
    uint64_t v[8];
    MIRSHA512_UNROLL
    for (int i = 0; i < 8; i++) v[i] = st[i];
    MIRSHA512_UNROLL
    for (int g = 0; g < kPairGroups; g++) consume_group(v, kw + 16 * g);
    finish_block(st, v, live);
}

}  // namespace sha512
}  // namespace mirsha
