// mirsha_streams.h — the kernel of the streaming hash states
// (mirsha_streams.hip; mirsha_streams_* in include/mirsha.h): SHA-256 states
// that take Write / Sum / Reset over any bytes, as a hash.Hash does
// (processor.go:21), where the checkpoint chains take whole 32-byte digests.
//
// State of stream s, device-resident and kept across calls: row s of
// kStreamStateBytes bytes of one array (one address per lane for the load and
// the store), as u32 words
//   [0, 8)    the midstate
//   [8, 24)   the unfinished block as big-endian message words; only its
//             first count % 64 bytes mean anything
//   24, 25    the total bytes written (u64: low word, high word)
//   26, 27    unused (the row is a whole number of 16-byte accesses)
//
// One lane per active stream walks its entries (mirsha_stream_plan's arrays)
// in steps of at most one compression, in a wave-uniform loop closed by a
// ballot: no atomics, no waiting, no cross-lane dependence.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mirsha {

constexpr uint32_t kStreamStateBytes = 112;

// arena_words: the arena's address rounded down to 4 bytes; `shift` (0-3) is
// what was rounded off and is added to every entry offset; `span` = the bytes
// from arena_words to the arena's end rounded up to 4 (at most 2^32 - 128):
// the kernel loads aligned 4-byte words inside [0, span) only, any other
// address reads as zero.  act[0, n_active) is followed by efirst[0, n_active];
// lane k runs entries [efirst[k], efirst[k + 1]) on stream act[k].  Entry e is
// the 16-byte record ent[4 e ..] = {ent_kind, ent_len, ent_off low, ent_off
// high} of mirsha_stream_plan's arrays (16-byte aligned: one load per entry).
// A SUM / SUM_RESET entry stores its 32-byte row of `out` (16-byte aligned),
// as is `state`.
hipError_t launch_streams(const uint32_t* arena_words, uint32_t shift, uint32_t span, const uint32_t* act,
                          const uint32_t* ent, uint32_t n_active, uint8_t* state, uint8_t* out, hipStream_t s);

}  // namespace mirsha
