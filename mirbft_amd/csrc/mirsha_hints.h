// mirsha_hints.h — the hint set of a uniform request launch: one length, one
// stride and the wave-uniform scalars that follow from the length alone.  Plain
// C++ (no HIP): the host computes the set once where the lengths are already
// on the host (plan creation, the staged host calls) and the request kernel
// takes it as an argument.  A hint is never trusted: every wave proves it
// against the lengths and offsets it loaded and takes the unhinted code when
// the proof fails (hash_tile_uniform, mirsha_kernels.hip).
#pragma once
#include <stdint.h>

namespace mirsha {

// The scalars of the final-block tail form, in the order of TailWords
// (sha256_rounds_asm.h; tail_words() in sha256_device.h computes the same on
// the device).
struct HintTail {
    uint32_t kw4, kw14, kw15, c4, c14, c15, cs16, cs17, cs19, cs29, cs30;
};

struct UniformHint {
    uint32_t valid;       // 0: no hint (the launch takes the unhinted kernel)
    uint32_t len;         // L: every message's length
    uint32_t stride;      // off[i + 1] - off[i], a multiple of 4
    uint32_t nb;          // compressions per message: ceil((L + 9) / 64)
    uint32_t loop_nb;     // blocks staged through LDS (nb - 1 with the tail form)
    uint32_t tail;        // 1: the final block holds at most 16 message bytes (tail form)
    uint32_t tail_bytes;  // 1: ... and at least one (0: the block is padding only, nothing is fetched)
    uint32_t tail_pad;    // 1: the tail form's words 0..3 need keep / mark (fewer than 16 message bytes)
    uint32_t reach;       // bytes from a message's offset that its loads touch
    uint32_t keep[4], mark[4];  // the tail form's words 0..3: w = (w & keep) | mark
    HintTail tw;
};

namespace hint_detail {
constexpr uint32_t kK4 = 0x3956c25bu, kK14 = 0x9bdc06a7u, kK15 = 0xc19bf174u;  // FIPS 180-4 §4.2.2, K[4], K[14], K[15]
inline uint32_t rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
inline uint32_t ssig0(uint32_t x) { return rotr(x, 7) ^ rotr(x, 18) ^ (x >> 3); }
inline uint32_t ssig1(uint32_t x) { return rotr(x, 17) ^ rotr(x, 19) ^ (x >> 10); }
}  // namespace hint_detail

// The hint set of messages of L bytes, `stride` bytes apart.  valid == 0 when
// the stride rules the aligned loader out (not a multiple of 4).
inline UniformHint make_uniform_hint(uint32_t L, uint64_t stride) {
    using namespace hint_detail;
    UniformHint h{};
    if ((stride & 3u) != 0 || stride > 0xFFFFFFFFull) return h;
    h.valid = 1;
    h.len = L;
    h.stride = (uint32_t)stride;
    h.nb = (L + 72u) >> 6;
    const int32_t u = (int32_t)(L - 64u * (h.nb - 1u));  // message bytes in the final block (< 0: length-only block)
    h.tail = u <= 16 ? 1u : 0u;
    h.tail_bytes = (h.tail && u > 0) ? 1u : 0u;
    h.tail_pad = (h.tail && u < 16) ? 1u : 0u;
    h.loop_nb = h.tail ? h.nb - 1u : h.nb;
    h.reach = 64u * h.loop_nb + (h.tail_bytes ? 16u : 0u);
    for (int k = 0; k < 4; k++) {
        const int32_t t = u - 4 * k;  // message bytes left at word k of the final block
        const uint32_t sh = (uint32_t)(t & 3) << 3;
        h.keep[k] = t >= 4 ? 0xFFFFFFFFu : (t <= 0 ? 0u : ~(0xFFFFFFFFu >> sh));
        h.mark[k] = (t >= 0 && t < 4) ? 0x80000000u >> sh : 0u;
    }
    HintTail& w = h.tw;
    w.c4 = u == 16 ? 0x80000000u : 0u;
    w.c14 = L >> 29;
    w.c15 = L << 3;
    w.kw4 = kK4 + w.c4;
    w.kw14 = kK14 + w.c14;
    w.kw15 = kK15 + w.c15;
    w.cs16 = ssig1(w.c14);
    w.cs17 = ssig1(w.c15);
    w.cs19 = ssig0(w.c4);
    w.cs29 = ssig0(w.c14);
    w.cs30 = ssig0(w.c15) + w.c14;
    return h;
}

}  // namespace mirsha
