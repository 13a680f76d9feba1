// The weighted slots of a batched flat fit (include/hgmm.h: hgmm_flat_train_batch_weighted, hgmm_flat_train_batch_voxels):
// flat_fused_pk_batch_kernel<NSLOT, true>, sixteen instantiations of the fused E+M body (flat_fused_body.h) with the WEIGHTED
// switch of the serial <NSLOT, true> kernels, over the second segment of the workgroup table (flat_batch_run,
// flat_kernels.hip).  A translation unit of its own: instantiated next to the serial kernels, the set made the compiler
// re-schedule the epilogue of one of them (profiles/flat_batch_weights.md), and the serial kernels are to stay the code they
// were, instruction for instruction.
#include "flat_fused_device.h"

#include <type_traits>
#include <utility>

using namespace hgmm;

// The same body text as flat_fused_pk_batch_kernel<NSLOT> (flat_kernels.hip); the second template parameter keeps the names
// apart.  SW is the
// slot's own array, indexed by the member's own rows, and nothing writes it while a fit runs: rebuilt as a pointer into the
// constant address space the row's weight arrives by scalar load with the row's coordinates, as behind the serial kernel's
// `const float* __restrict__ SW`.
template <int NSLOT, bool WEIGHTED>
__global__ __launch_bounds__(BLOCK) void flat_fused_pk_batch_kernel(
    const FlatBatchMember* __restrict__ members, const int2* __restrict__ wg_table, int J, int Jpad, int parity) {
    static_assert(WEIGHTED, "the unweighted instantiations are flat_fused_pk_batch_kernel<NSLOT>");
    const int2 me = wg_table[blockIdx.x];
    const FlatBatchMember& m = members[me.x];
    if (global_ptr(m.ctl)[parity ? 3 : 0]) return;
    const float* const X = constant_ptr(m.X);
    const float* const pack = global_ptr(m.pack);
    float* const partials = global_ptr(m.partials);
    double* const lpn_partials = global_ptr(m.lpn_partials);
    const float* const SW = constant_ptr(m.SW);
    const int64_t n = m.n;
    const unsigned block = (unsigned)me.y, nblocks = (unsigned)m.nblocks;
    constexpr int allow_const_shift = 1, comp_major = 0;
#define FLAT_FUSED_BLOCK block
#define FLAT_FUSED_ROW_RANGE(n, r0, nrows) wave_row_range_uniform(n, block, nblocks, r0, nrows)
#include "flat_fused_body.h"
#undef FLAT_FUSED_BLOCK
#undef FLAT_FUSED_ROW_RANGE
}

template <int... S>
static auto fused_batch_weighted_kernel_for(int slots, std::integer_sequence<int, S...>) {
    decltype(&flat_fused_pk_batch_kernel<1, true>) kernel = nullptr;
    ((slots == S + 1 ? (void)(kernel = flat_fused_pk_batch_kernel<S + 1, true>) : (void)0), ...);
    return kernel;
}

void hgmm::launch_fused_batch_weighted(int slots, unsigned grid, hipStream_t stream, const FlatBatchMember* members,
                                       const int2* wg_table, int J, int Jpad, int parity) {
    fused_batch_weighted_kernel_for(slots, std::make_integer_sequence<int, 16>())<<<grid, BLOCK, 0, stream>>>(members, wg_table, J,
                                                                                                            Jpad, parity);
}
