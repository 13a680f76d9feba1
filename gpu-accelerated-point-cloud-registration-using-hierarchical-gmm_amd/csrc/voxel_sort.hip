// rocPRIM behind voxel_sort.h: the stable radix sort of (voxel key, row) and the compaction of the segment heads.
// (<cstring> first: rocPRIM's device pass uses memset without including it)
#include <cstring>
#include <rocprim/rocprim.hpp>

#include "voxel_sort.h"

namespace hgmm {

hipError_t voxel_sort_pairs(void* tmp, size_t* tmp_bytes, const uint64_t* keys_in, uint64_t* keys_out,
                            const uint32_t* rows_in, uint32_t* rows_out, size_t n, unsigned end_bit, hipStream_t stream) {
    return rocprim::radix_sort_pairs(tmp, *tmp_bytes, keys_in, keys_out, rows_in, rows_out, n, 0u, end_bit, stream);
}

namespace {
struct IsHead {
    const uint64_t* k;
    __host__ __device__ bool operator()(uint32_t i) const { return i == 0 || k[i] != k[i - 1]; }
};
}  // namespace

hipError_t voxel_segment_heads(void* tmp, size_t* tmp_bytes, const uint64_t* sorted_keys, uint32_t* heads_out,
                               uint32_t* count_out, size_t n, hipStream_t stream) {
    return rocprim::select(tmp, *tmp_bytes, rocprim::counting_iterator<uint32_t>(0), heads_out, count_out, n,
                           IsHead{sorted_keys}, stream);
}

}  // namespace hgmm
