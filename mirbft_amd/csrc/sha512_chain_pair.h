// sha512_chain_pair.h — one step of a commit programme under SHA-512/256
// (sha512_chain.h) split for a producer/consumer pair of waves
// (mirsha_sha512_chains_pair.hip), in the way sha512_pair.h splits a
// compression.  Which entries a step takes never depends on a hash value, so
// one side does the whole walk and the other nothing but rounds:
//
//   producer   the entries, the plan of the step, its block, the pending
//              words and the count; per step and lane one control word
//   consumer   h: the 80 rounds from the handed-over K + W words, the state
//              addition, a checkpoint's row and the restart from Hasher()
//
// The two sides hold disjoint parts of a chain's state (pend and cnt / h).
// A `keep` step (a lane's end with rows left pending) compresses nothing and
// is the producer's alone.
//
// The control word of a lane's step is all the consumer learns about it:
//   0                          the lane compresses nothing in this step: the
//                              rounds it runs are dropped
//   kChainPairLive             a whole block: st += F
//   kChainCheckpoint | row     a final block: st += F, Sum() to `row`, restart
// (an output row is below 2^31, as in a plan entry; kChainPairLive is no
// checkpoint, so the two never collide).
//
// Plain C++ as sha512_chain.h and sha512_pair.h, so the CPU suite proves it
// (tests/c/sha512_chain_pair_unit.cpp); the kernels add the loaders, the ring
// and the barriers.
#pragma once
#include "sha512_chain.h"
#include "sha512_pair.h"

namespace mirsha {
namespace sha512 {

constexpr uint32_t kChainPairLive = 1u;

// The plan of the lane's step at entry e of [e, end) with n digests written
// (x[i] = ent[e + i] where e + i < end, as chain_plan takes them); e and n
// move past the step.
MIRSHA512_HD ChainStep chain_pair_plan(const uint32_t x[4], uint32_t end, uint32_t& e, uint64_t& n) {
    const ChainStep s = chain_plan(x, end - e, n);  // e <= end
    e += s.consumed;
    n = s.n_after;
    return s;
}

MIRSHA512_HD uint32_t chain_pair_ctl(const ChainStep& s) {
    return s.cp ? (kChainCheckpoint | s.row) : (s.full ? kChainPairLive : 0u);
}
MIRSHA512_HD bool chain_pair_live(uint32_t ctl) { return ctl != 0u; }
MIRSHA512_HD bool chain_pair_cp(uint32_t ctl) { return (ctl & kChainCheckpoint) != 0u; }
MIRSHA512_HD uint32_t chain_pair_row(uint32_t ctl) { return ctl & ~kChainCheckpoint; }

// The producer's step: the block into w (the schedule window of the five
// groups that follow when any lane of the group compresses), the pending words
// of a `keep` step, and the lane's control word.  A group of 64 lanes hands a
// step over when chain_pair_live holds for any of them; a step in which it
// holds for none is the walk's last (only a lane's last step is without a
// compression).
MIRSHA512_HD uint32_t chain_pair_produce(uint64_t pend[kChainPendWords], const uint32_t rows[4][8], const ChainStep& s,
                                         uint64_t w[16]) {
    chain_block(pend, rows, s, w);
    if (s.keep) chain_keep(w, pend);
    return chain_pair_ctl(s);
}

// The consumer's end of a step, v = the working variables after the step's 80
// rounds: the state addition where the lane's block is live and, for a
// checkpoint, the row's eight words (as digest_words leaves them: the bytes
// of the row in memory) and the restart.  Returns whether d holds a row, for
// output row chain_pair_row(ctl).
MIRSHA512_HD bool chain_pair_finish(uint64_t st[8], const uint64_t v[8], uint32_t ctl, uint32_t d[8]) {
    finish_block(st, v, chain_pair_live(ctl));
    const bool cp = chain_pair_cp(ctl);
    if (cp) {
        digest_words(st, d);
        MIRSHA512_UNROLL
        for (int i = 0; i < 8; i++) st[i] = kH0[i];
    }
    return cp;
}

}  // namespace sha512
}  // namespace mirsha
