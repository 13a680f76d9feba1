// The two device-wide primitives of the voxel down-sample (voxel_kernels.hip), kept in a translation unit of their own
// (voxel_sort.hip) because they instantiate rocPRIM: nothing else of the library pays for its headers.
// Both follow rocPRIM's convention: tmp == nullptr only reports the temporary storage needed in *tmp_bytes; the caller
// brings the storage (the context's allocator), everything runs on the given stream, nothing synchronises.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace hgmm {

// STABLE least-significant-digit radix sort of (key, row) pairs by bits [0, end_bit) of the key: rows of equal keys keep
// their input order
hipError_t voxel_sort_pairs(void* tmp, size_t* tmp_bytes, const uint64_t* keys_in, uint64_t* keys_out,
                            const uint32_t* rows_in, uint32_t* rows_out, size_t n, unsigned end_bit, hipStream_t stream);

// heads_out: the positions i, ascending, at which a sorted key differs from its predecessor (position 0 included);
// *count_out (device): how many there are
hipError_t voxel_segment_heads(void* tmp, size_t* tmp_bytes, const uint64_t* sorted_keys, uint32_t* heads_out,
                               uint32_t* count_out, size_t n, hipStream_t stream);

}  // namespace hgmm
