// sha512_pair_ring.h — the hand-over of the SHA-512/256 producer/consumer pair
// kernels (mirsha_sha512_pair.hip, mirsha_sha512_chains_pair.hip): the LDS ring
// of two group slots, the two accesses to a slot, and which wave is which.  The
// loops that drive it are the units' own.  HIP only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sha512_pair.h"

namespace mirsha {

// Wave 0 produces, wave 1 consumes; 64 messages, lists or chains a workgroup.
constexpr uint32_t kSha512PairThreads = 128;

struct Sha512PairRing {
    // [slot][pair of KW words][lane]: 16 bytes a lane, consecutive lanes
    // consecutive, so every b128 access is conflict-free (as PairRing).
    ulonglong2 kw[2][sha512::kPairGroupWords / 2][64];
    // The walked loops' hand-over of "is there another block": per lane (lists
    // with nulls: whether the lane has the block; chains: the step's control
    // word, sha512_chain_pair.h), and for the whole group of 64.  [block & 1].
    uint32_t live[2][64];
    uint32_t more[2];
};
static_assert(sizeof(Sha512PairRing) <= 65536u, "static LDS only");

// One group of the schedule into a ring slot.
template <int G>
__device__ __forceinline__ void put_group(uint64_t w[16], ulonglong2 (*slot)[64], uint32_t lane) {
    uint64_t kw[16];
    sha512::produce_group<G>(w, kw);
#pragma unroll
    for (int q = 0; q < 8; q++) slot[q][lane] = make_ulonglong2(kw[2 * q], kw[2 * q + 1]);
}

// 16 rounds from a ring slot.
__device__ __forceinline__ void take_group(ulonglong2 (*slot)[64], uint32_t lane, uint64_t v[8]) {
    uint64_t kw[16];
#pragma unroll
    for (int q = 0; q < 8; q++) {
        const ulonglong2 x = slot[q][lane];
        kw[2 * q] = x.x;
        kw[2 * q + 1] = x.y;
    }
    sha512::consume_group(v, kw);
}

// Wave-uniform, and known to be: the branches on it are scalar.
__device__ __forceinline__ bool is_producer() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) == 0; }

}  // namespace mirsha
