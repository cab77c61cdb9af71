// mirsha_sha512_chains.h — launchers of the checkpoint-chain kernels of the
// second hasher, SHA-512/256 (mirsha_sha512_chains.hip): the SHA-512/256 row of
// chain_kernels (mirsha_chains.h), whose members' contracts they follow.  Not
// part of the C-ABI.
//
// State of n chains: h u64[8 n], pend u64[12 n] (the block's first three
// slots as big-endian words; sha512_chain.h), cnt u64[n]; all 16-byte aligned.
//
// The commit launchers come in two forms: the one-lane kernels themselves
// (mirsha_sha512_chains.hip) and, with `variant` and `pair_launches`, the
// routed form that chain_kernels holds (mirsha_sha512_chains_pair.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mirsha {

// Hasher() of a SHA-512/256 chain: the eight words of h (host code).
void sha512_chains_h0(void* h);

// `out` may be NULL when no entry is a checkpoint (mirsha_chains_absorb: a
// programme of writes).
hipError_t launch_sha512_chains_commit(const uint8_t* digests, const uint32_t* ent, const uint32_t* act,
                                       const uint32_t* efirst, uint32_t n_active, void* h, void* pend,
                                       uint64_t* cnt, uint8_t* out, hipStream_t s);
hipError_t launch_sha512_chains_sum(const uint32_t* which, uint32_t k, const void* h, const void* pend,
                                    const uint64_t* cnt, uint8_t* out, hipStream_t s);
hipError_t launch_sha512_chains_reset(const uint32_t* which, uint32_t k, void* h, uint64_t* cnt, hipStream_t s);
hipError_t launch_sha512_chains_commit_seg(const uint8_t* digests, const uint32_t* ent, const uint32_t* seg_chain,
                                           const uint32_t* sfirst, const uint32_t* seg_flags, uint32_t n_seg,
                                           const void* h_in, const void* pend_in, const uint64_t* cnt_in, void* h,
                                           void* pend, uint64_t* cnt, uint8_t* out, uint32_t prio, hipStream_t s);

// The routed launchers: a launch of at most sha512_pair_max_groups() 64-lane
// groups (mirsha_sha512_pair.h: the threshold and the A/B knobs of the request
// and list launches) takes the producer/consumer pair kernels, any other the
// one-lane kernels above.  `variant` as launch_sha512_msgs reads it:
// kVariantPair is the pair kernel at any size, kVariantDirect and
// kVariantLdsOnly the one-lane kernel at any size, anything else the automatic
// choice.  Each launches exactly one kernel (timed_launch) and adds 1 to
// *pair_launches (may be NULL) when that kernel is a pair kernel.
hipError_t launch_sha512_chains_commit(const uint8_t* digests, const uint32_t* ent, const uint32_t* act,
                                       const uint32_t* efirst, uint32_t n_active, void* h, void* pend,
                                       uint64_t* cnt, uint8_t* out, int variant, hipStream_t s,
                                       uint64_t* pair_launches);
hipError_t launch_sha512_chains_commit_seg(const uint8_t* digests, const uint32_t* ent, const uint32_t* seg_chain,
                                           const uint32_t* sfirst, const uint32_t* seg_flags, uint32_t n_seg,
                                           const void* h_in, const void* pend_in, const uint64_t* cnt_in, void* h,
                                           void* pend, uint64_t* cnt, uint8_t* out, uint32_t prio, int variant,
                                           hipStream_t s, uint64_t* pair_launches);

}  // namespace mirsha
