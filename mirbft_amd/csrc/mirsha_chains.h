// mirsha_chains.h — what the checkpoint-chain units share (mirsha_chains.hip:
// the SHA-256 kernels and every mirsha_chains_* entry point;
// mirsha_sha512_chains.hip: the SHA-512/256 kernels; mirsha_sha512_chains_pair.hip:
// their producer/consumer pair forms and the route between the two).  Not part
// of the C-ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mirsha {

// An entry of a commit programme (mirsha_commit_plan, mirsha_commit_seg_plan)
// is a row of the digest table to write, or kCommitEntryCheckpoint | the row
// of `out` that gets Sum() before the state restarts.
constexpr uint32_t kCommitEntryCheckpoint = 0x80000000u;

// What a hasher's chains are to the host: the state's sizes and the launchers
// of its kernels.  State of n chains: h, pend (h_bytes, pend_bytes per chain)
// and cnt u64[n], all 16-byte aligned; the launchers take them untyped.
struct ChainKernels {
    uint32_t h_bytes, pend_bytes;  // per chain
    void (*h0)(void* h);           // Hasher(): the h words of one chain
    // One lane per active chain act[k] with entries ent[efirst[k] ..
    // efirst[k + 1]); checkpoint values to 32-byte rows of `out` (NULL when no
    // entry is a checkpoint).  `variant` (the context's, mirsha_ctx_set_variant)
    // and `pair_launches` (the chains object's counter, may be NULL) are for a
    // hasher whose kernels have more than one form (mirsha_sha512_chains.h);
    // the SHA-256 row ignores both.  One kernel either way.
    hipError_t (*commit)(const uint8_t* digests, const uint32_t* ent, const uint32_t* act, const uint32_t* efirst,
                         uint32_t n_active, void* h, void* pend, uint64_t* cnt, uint8_t* out, int variant,
                         hipStream_t s, uint64_t* pair_launches);
    // mirsha_chains_absorb's grouped writes pos[afirst[k] .. afirst[k + 1]).
    // NULL: they run as a commit programme without checkpoints.
    hipError_t (*absorb)(const uint8_t* digests, const uint32_t* pos, const uint32_t* act, const uint32_t* afirst,
                         uint32_t n_active, void* h, void* pend, uint64_t* cnt, hipStream_t s);
    hipError_t (*sum)(const uint32_t* which, uint32_t k, const void* h, const void* pend, const uint64_t* cnt,
                      uint8_t* out, hipStream_t s);
    hipError_t (*reset)(const uint32_t* which, uint32_t k, void* h, uint64_t* cnt, hipStream_t s);
    // A cycle's commit programme cut into segments (mirsha_commit_seg_plan's
    // arrays), one lane per segment.  A FIRST segment starts from its chain's
    // state in h_in / pend_in / cnt_in (the chains' own arrays, or a copy of
    // them taken on the stream ahead of the launch), every other one from
    // Hasher(); a LAST segment stores the state it ends in to h / pend / cnt.
    // Checkpoint values go to 32-byte rows of `out` (16-byte aligned, device or
    // host-visible memory) with plain vector stores.  `prio`: the issue
    // priority (0-3) the waves take at entry.  `variant`, `pair_launches`: as
    // commit's.
    hipError_t (*commit_seg)(const uint8_t* digests, const uint32_t* ent, const uint32_t* seg_chain,
                             const uint32_t* sfirst, const uint32_t* seg_flags, uint32_t n_seg, const void* h_in,
                             const void* pend_in, const uint64_t* cnt_in, void* h, void* pend, uint64_t* cnt,
                             uint8_t* out, uint32_t prio, int variant, hipStream_t s, uint64_t* pair_launches);
};
const ChainKernels& chain_kernels(int hasher);

}  // namespace mirsha
