// mirsha_order.h — the bucket order built on the device (mirsha_order.hip, the
// u32 scan in mirsha_scan.hip): what mirsha_bucket_order builds on the host,
// from lengths that are already in HBM.
//
// Bucket order = message indices sorted by SHA-256 block count, longest first,
// stable within a block count.  With host-known bounds bmin = blocks(min_len),
// bmax = blocks(max_len) (blocks(L) = ceil((L + 9) / 64)) there are
// R = bmax - bmin + 1 bins and message i's bin is
// clamp(bmax - blocks(len[i]), 0, R - 1): a length outside the bounds sorts as
// the nearest bound, so the result is a permutation whatever the lengths are,
// and it is mirsha_bucket_order's result element for element when every
// length lies inside them.
//
// A counting sort in three launches in stream order (mirsha_order_plan sizes
// them: `chunk` message indices per wave, n_chunks waves):
//   order_count_kernel    wave c: histogram of chunk c -> counts[bin * n_chunks + c]
//   launch_counts_scan    one exclusive u32 scan over counts[R * n_chunks]
//                         (rocPRIM): bin-major, chunk-minor, so every (bin,
//                         chunk) cell's base lies behind all lower bins and,
//                         inside its bin, behind all lower chunks = stable
//   order_scatter_kernel  wave c: order[base + rank inside the cell] = i
// No atomics on global memory and no wave waits for another workgroup.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mirsha {

// counts[bin * n_chunks + c] = messages of chunk c = [c * chunk, min(n, (c + 1)
// * chunk)) in that bin.  chunk % 64 == 0, 1 <= bins <= MIRSHA_ORDER_MAX_BINS,
// n_chunks = ceil(n / chunk) > 0.
hipError_t launch_order_count(const uint32_t* len, uint32_t n, uint32_t bmax, uint32_t bins, uint32_t chunk,
                              uint32_t n_chunks, uint32_t* counts, hipStream_t s);
// base = the exclusive scan of counts (same layout); writes order[0, n).
hipError_t launch_order_scatter(const uint32_t* len, uint32_t n, uint32_t bmax, uint32_t bins, uint32_t chunk,
                                uint32_t n_chunks, const uint32_t* base, uint32_t* order, hipStream_t s);
// order[i] = i.
hipError_t launch_order_iota(uint32_t* order, uint32_t n, hipStream_t s);
// out[k] = in[0] + ... + in[k - 1] over m u32 values (mirsha_scan.hip; in != out).
// With tmp == nullptr only sets tmp_bytes, as launch_offsets_scan.
hipError_t launch_counts_scan(void* tmp, size_t& tmp_bytes, const uint32_t* in, uint32_t* out, size_t m,
                              hipStream_t s);

}  // namespace mirsha
