// mirsha_sha512_pair.h — the routed launchers of the SHA-512/256 request, list
// and plan-list launches (mirsha_sha512_pair.hip): a small launch takes the
// producer/consumer pair kernels, any other the one-lane kernels of
// mirsha_sha512.hip / mirsha_sha512_plan.hip.  These are what a context queues
// (hasher_launch_msgs / _lists, mirsha_ctx.h; kPlanSha512, mirsha_plan.hip).
// Not part of the C-ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mirsha {

// A launch of at most sha512_pair_max_groups() 64-lane groups takes the pair
// kernels.  Default kSha512PairMaxGroups: one pair per CU of the chip's 256.
// The derivation of kPairMaxGroups (mirsha_kernels.h) gives 512, half of the
// 1,024 SIMDs, so that both waves of every pair have a SIMD to themselves; as
// measured (profiles/hasher_pair) the pair wins by a third up
// to 256 groups and only ties the one-lane kernels at 512, so the automatic
// route stops at the largest measured count where it held.  Environment (A/B,
// read only with MIRSHA_AB=1): MIRSHA_SHA512_PAIR=0 turns the automatic choice
// off, MIRSHA_SHA512_PAIR_MAX_GROUPS=n moves the threshold.
constexpr uint32_t kSha512PairMaxGroups = 256;
uint32_t sha512_pair_max_groups();

// Each launches exactly one kernel (timed_launch) and adds 1 to *pair_launches
// (may be NULL) when that kernel is a pair kernel.
//
// launch_sha512_msgs with launch_msgs' `variant`: kVariantPair is the pair
// kernel at any size, kVariantDirect and kVariantLdsOnly the one-lane kernel at
// any size, anything else the automatic choice.  The one-descriptor limits of
// the one-lane launcher hold for both routes (hipErrorInvalidValue).
hipError_t launch_sha512_msgs(const uint8_t* arena, uint64_t arena_len, const uint64_t* off, const uint32_t* len,
                              const uint32_t* order, uint32_t n, uint8_t* out, int variant, hipStream_t s,
                              uint64_t* pair_launches);
hipError_t launch_sha512_lists(const uint8_t* digests, uint32_t n_digests, const uint32_t* idx, uint32_t n_entries,
                               const uint32_t* first, uint32_t n_lists, uint32_t* scratch, uint8_t* out, hipStream_t s,
                               uint64_t* pair_launches);
// The compacted lists of a sequential plan (launch_sha512_plan_lists' arguments).
hipError_t launch_sha512_plan_lists(const uint8_t* digests, uint32_t n_digests, const uint32_t* cidx,
                                    uint32_t n_entries, const uint32_t* cfirst, uint32_t n_lists, uint32_t uniform,
                                    uint8_t* out, hipStream_t s, uint64_t* pair_launches);

}  // namespace mirsha
