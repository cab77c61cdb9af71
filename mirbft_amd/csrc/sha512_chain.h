// sha512_chain.h — one step of a commit programme under SHA-512/256: the
// analogue of CommitStep / commit_fetch (mirsha_device.h) for a 128-byte block,
// which four 32-byte digests fill.  Plain C++ as sha512_device.h, so the CPU
// suite proves it (tests/c/sha512_chain_unit.cpp); the kernels of
// mirsha_sha512_chains.hip add the loaders.
//
// State per chain: h[8] (u64), the digests written since the last whole block
// as the block's first 12 big-endian words pend[12] (u64; rows past cnt % 4
// hold anything) and cnt, the digests written since the last reset.
//
// A step is at most one compression.  With p = cnt % 4 rows pending, the lane
// looks at its next entries (an entry is a row of the digest table to write,
// or kChainCheckpoint | output row):
//   full block   4 - p writes come first: they fill the block, nothing is
//                pending afterwards
//   checkpoint   a checkpoint comes after j < 4 - p writes: the final block is
//                the p + j rows, 0x80, zeros and the 128-bit bit length
//                256 (cnt + j); p + j <= 3 leaves bytes 96..127, so it is always
//                exactly one block.  The state becomes Hasher(), cnt 0
//   lane's end   the entries end after j < 4 - p writes: they join the pending
//                rows without a compression (a programme's last step only)
// Which entries a step takes depends on the entry kinds and cnt % 4 only,
// never on a hash value.
#pragma once
#include "sha512_device.h"

namespace mirsha {
namespace sha512 {

constexpr uint32_t kChainCheckpoint = 0x80000000u;  // = MIRSHA_COMMIT_ENTRY_CHECKPOINT
constexpr uint32_t kChainPendWords = 12;            // three rows of four 64-bit words

struct ChainStep {
    uint32_t id[4];     // block slot s takes table row id[s] where bit s of `take` is set
    uint32_t take;      // slots filled by this step's writes: [p, p + j)
    uint32_t p, j;      // pending rows on entry, writes taken
    uint32_t row;       // checkpoint: the output row
    uint32_t consumed;  // entries the step moves past (j, and the checkpoint)
    uint64_t count;     // checkpoint: digests of the message
    uint64_t n_after;   // the chain's count behind the step
    bool full, cp;      // compress a whole block / the final block
    bool keep;          // neither: j > 0 rows join the pending ones
    // none of the three: the lane has reached its end
};

// Plans the step of a lane whose next entries are x[0 .. avail) (x[i] for
// i >= avail is not looked at; avail may exceed 4) with n digests written.
MIRSHA512_HD ChainStep chain_plan(const uint32_t x[4], uint32_t avail, uint64_t n) {
    ChainStep s;
    const uint32_t p = (uint32_t)n & 3u, need = 4u - p;
    uint32_t j = 0u;
    bool open = true;  // every entry so far was a write
    MIRSHA512_UNROLL
    for (int i = 0; i < 4; i++) {
        open = open && (uint32_t)i < need && (uint32_t)i < avail && !(x[i] & kChainCheckpoint);
        j += open ? 1u : 0u;
    }
    uint32_t xj = 0u;  // the entry behind the writes (j < 4), if there is one
    MIRSHA512_UNROLL
    for (int i = 0; i < 4; i++) xj = (j == (uint32_t)i) ? x[i] : xj;
    s.full = j == need;
    s.cp = !s.full && j < avail && (xj & kChainCheckpoint) != 0u;
    s.keep = !s.full && !s.cp && j > 0u;
    s.p = p;
    s.j = j;
    s.row = xj & ~kChainCheckpoint;
    s.count = n + j;
    s.consumed = j + (s.cp ? 1u : 0u);
    s.n_after = s.cp ? 0u : n + j;
    s.take = 0u;
    MIRSHA512_UNROLL
    for (int sl = 0; sl < 4; sl++) {
        s.id[sl] = 0u;
        MIRSHA512_UNROLL
        for (int i = 0; i <= sl; i++) {
            const bool here = p + (uint32_t)i == (uint32_t)sl && (uint32_t)i < j;
            s.id[sl] = here ? x[i] : s.id[sl];
            s.take |= here ? 1u << sl : 0u;
        }
    }
    return s;
}

// The step's block: slots below p from the pending words, the taken slots
// from rows[s] (the raw row, 8 dwords as they lie in memory; anything in a
// slot that is not taken), and for a checkpoint 0x80 behind them and the bit
// length 256 count as a 128-bit big-endian number (w[14] = count >> 56,
// w[15] = count << 8).  Without a checkpoint the slots from p + j on are zero.
MIRSHA512_HD void chain_block(const uint64_t pend[kChainPendWords], const uint32_t rows[4][8], const ChainStep& s,
                              uint64_t w[16]) {
    const uint32_t filled = s.p + s.j;
    MIRSHA512_UNROLL
    for (int sl = 0; sl < 4; sl++) {
        MIRSHA512_UNROLL
        for (int i = 0; i < 4; i++) {
            const uint64_t fresh = ((uint64_t)__builtin_bswap32(rows[sl][2 * i]) << 32) |
                                   __builtin_bswap32(rows[sl][2 * i + 1]);
            const uint64_t mark = (s.cp && (uint32_t)sl == filled && i == 0) ? 0x8000000000000000ull : 0ull;
            uint64_t v = ((s.take >> sl) & 1u) ? fresh : mark;
            if (sl < 3) v = (uint32_t)sl < s.p ? pend[4 * sl + i] : v;
            w[4 * sl + i] = v;
        }
    }
    if (s.cp) {
        w[14] = s.count >> 56;
        w[15] = s.count << 8;
    }
}

// A step without a compression (`keep`): the block's first three slots are the
// pending rows from now on.
MIRSHA512_HD void chain_keep(const uint64_t w[16], uint64_t pend[kChainPendWords]) {
    MIRSHA512_UNROLL
    for (int i = 0; i < (int)kChainPendWords; i++) pend[i] = w[i];
}

// Sum() of a state: the final block of a checkpoint that takes no write.
MIRSHA512_HD ChainStep chain_sum_step(uint64_t n) {
    const uint32_t x[4] = {kChainCheckpoint, 0u, 0u, 0u};
    return chain_plan(x, 1u, n);
}

}  // namespace sha512
}  // namespace mirsha
