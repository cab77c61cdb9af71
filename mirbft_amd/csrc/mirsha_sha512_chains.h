// mirsha_sha512_chains.h — launchers of the checkpoint-chain kernels of the
// second hasher, SHA-512/256 (mirsha_sha512_chains.hip): what a mirsha_chains
// created with MIRSHA_HASHER_SHA512_256 runs where a SHA-256 one runs
// launch_chains_* (chains_launch_* in mirsha_ctx.h).  Not part of the C-ABI.
//
// State of n chains: h u64[8 n], pend u64[12 n] (the block's first three
// slots as big-endian words; sha512_chain.h), cnt u64[n]; all 16-byte aligned.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mirsha {

// Hasher() of a SHA-512/256 chain: the eight words of h (host code).
void sha512_chains_h0(uint64_t h0[8]);

// launch_chains_commit's arguments: one lane per active chain act[k] with
// entries ent[efirst[k] .. efirst[k + 1]).  `out` may be NULL when no entry is
// a checkpoint (mirsha_chains_absorb: a programme of writes).
hipError_t launch_sha512_chains_commit(const uint8_t* digests, const uint32_t* ent, const uint32_t* act,
                                       const uint32_t* efirst, uint32_t n_active, uint64_t* h, uint64_t* pend,
                                       uint64_t* cnt, uint8_t* out, hipStream_t s);
hipError_t launch_sha512_chains_sum(const uint32_t* which, uint32_t k, const uint64_t* h, const uint64_t* pend,
                                    const uint64_t* cnt, uint8_t* out, hipStream_t s);
hipError_t launch_sha512_chains_reset(const uint32_t* which, uint32_t k, uint64_t* h, uint64_t* cnt, hipStream_t s);
// launch_chains_commit_seg's arguments (mirsha_ctx.h).
hipError_t launch_sha512_chains_commit_seg(const uint8_t* digests, const uint32_t* ent, const uint32_t* seg_chain,
                                           const uint32_t* sfirst, const uint32_t* seg_flags, uint32_t n_seg,
                                           const uint64_t* h_in, const uint64_t* pend_in, const uint64_t* cnt_in,
                                           uint64_t* h, uint64_t* pend, uint64_t* cnt, uint8_t* out, uint32_t prio,
                                           hipStream_t s);

}  // namespace mirsha
