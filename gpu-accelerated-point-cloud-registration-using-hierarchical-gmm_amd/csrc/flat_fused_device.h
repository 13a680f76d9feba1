// Device pieces of the flat fused E+M kernels that more than one translation unit needs: flat_kernels.hip (the serial kernels,
// the unweighted batched set and every launcher) and flat_batch_weighted.hip (the weighted batched set, in a translation unit
// of its own so that its sixteen instantiations cannot re-schedule a serial kernel's code: profiles/flat_batch_weights.md).
// What flat_fused_body.h names and the including kernels use: the constants of the packed table, the log-sum-exp closing, the
// waves' row ranges, the zero-weight test and the pointer rebuilders of the batched kernels.
#pragma once
#include "hgmm_ctx.h"
#include "wave_ops.h"

namespace hgmm {

constexpr float NEG_INF = -__builtin_huge_valf();
constexpr float LOG2E = 1.4426950408889634f;
constexpr float LN2 = 0.6931471805599453f;
constexpr int PK_MU = 0, PK_G = 3, PK_C = 6, PK_W = 7;   // rows of the packed parameter table (PK_W: the raw weight, for the fused kernel's origin)
constexpr int PK_ROWS = 8;
typedef float f2 __attribute__((ext_vector_type(2)));
constexpr int WAVES_PER_BLOCK = 4;
constexpr int BLOCK = WAVES_PER_BLOCK * 64;
constexpr int FUSED_TRIP = 8;              // rows per straight-line trip of the fused kernels' constant-shift loop (8, 4 or 2)

// The reference's normaliser  log( sum_j exp(wlp_j) + eps )  (gmm_waymo gmm_impl.py:113, no
// max-shift there) from the wave maximum m2 and S = sum_j 2^(wl2_j - m2), all in log2 units:
//   lpn2 = mc + log2( S' + eps 2^-mc ),  mc = max(m2, -64),  S' = S (or 0 when m2 < -64: then
//   sum_j exp(wlp_j) < 1e-19 J is below float32 resolution of eps = 1e-8).
// inv_den satisfies  r_j = 2^(wl2_j - m2) * inv_den.
constexpr float CS_MAX_SHIFT = 60.0f;      // constant-shift log-sum-exp is used while max_j c2_j <= this (flat_fused_pk_kernel)
__device__ __forceinline__ float lpn2_from(float m2, float s, float& inv_den) {
    const bool tiny = m2 < -64.0f;
    const float mc = tiny ? -64.0f : m2;
    const float den = fmaf(FLAT_EPS, __builtin_amdgcn_exp2f(-mc), tiny ? 0.0f : s);
    inv_den = tiny ? 0.0f : __builtin_amdgcn_rcpf(den);
    return mc + __builtin_amdgcn_logf(den);
}

__device__ __forceinline__ void wave_row_range(int64_t n, int64_t& r0, int64_t& r1) {
    const int64_t nw = (int64_t)gridDim.x * WAVES_PER_BLOCK;
    const int64_t gw = (int64_t)blockIdx.x * WAVES_PER_BLOCK + wave_in_block();
    const int64_t per = (n + nw - 1) / nw;
    r0 = gw * per;
    r1 = r0 + per < n ? r0 + per : n;
    if (r0 > n) r0 = n;
}
// The same range as wave-uniform SCALARS: first row and row count.  The 64-bit division above goes through v_rcp and
// leaves r0 / r1 in vector registers although every lane holds the same value; a row loop that compares against them
// pays a v_cmp_*_i64 per comparison.  Read back through readfirstlane, the loop's counter, its prefetch clamp and its
// exit test are scalar instructions.  (A wave never owns 2^31 rows: the count is an int.)
__device__ __forceinline__ int64_t uniform_i64(int64_t v) {
    const int lo = __builtin_amdgcn_readfirstlane((int)(v & 0xffffffffLL)), hi = __builtin_amdgcn_readfirstlane((int)(v >> 32));
    return ((int64_t)hi << 32) | (int64_t)(unsigned int)lo;
}
__device__ __forceinline__ void wave_row_range_uniform(int64_t n, int64_t& r0, int& nrows) {
    int64_t r1;
    wave_row_range(n, r0, r1);
    r0 = uniform_i64(r0);
    nrows = (int)(uniform_i64(r1) - r0);                 // (r1 >= r0 always)
}

// (the same for workgroup `block` of the `nblocks` that share a cloud in a batched launch, flat_fused_pk_batch_kernel)
__device__ __forceinline__ void wave_row_range_uniform(int64_t n, unsigned block, unsigned nblocks, int64_t& r0, int& nrows) {
    const int64_t nw = (int64_t)nblocks * WAVES_PER_BLOCK;
    const int64_t gw = (int64_t)block * WAVES_PER_BLOCK + wave_in_block();
    const int64_t per = (n + nw - 1) / nw;
    int64_t a = gw * per;
    const int64_t b = a + per < n ? a + per : n;
    if (a > n) a = n;
    r0 = uniform_i64(a);
    nrows = (int)(uniform_i64(b) - r0);
}

__device__ __forceinline__ bool weight_is_zero(float s) { return (__float_as_uint(s) & 0x7fffffffu) == 0u; }


// A pointer read from memory is a generic pointer to the compiler, and a generic pointer is dereferenced by flat_load: no
// scalar loads for the row's coordinates, no global_load for the table.  The table holds device allocations only, so the
// pointer is rebuilt from its bits as a pointer into the global address space -- what a kernel argument is by itself.  (Through
// the integer: a cast to the global address space and back is folded away before the address spaces are inferred.)
template <class T>
__device__ __forceinline__ T* global_ptr(T* p) {
    typedef __attribute__((address_space(1))) T* gptr;
    return (T*)(gptr)(uintptr_t)p;
}
// ... and the cloud, which nothing writes while a fit runs, as a pointer into the CONSTANT address space: a wave-uniform load
// from it is a scalar load whatever else the kernel does (the serial kernel's `const float* __restrict__ X` argument says as
// much; behind a plain global pointer the row loop's compiler barrier counts as a possible store, and the row's coordinates
// arrive by vector loads into six more registers)
template <class T>
__device__ __forceinline__ const T* constant_ptr(const T* p) {
    typedef __attribute__((address_space(4))) const T* cptr;
    return (const T*)(cptr)(uintptr_t)p;
}


// (flat_batch_weighted.hip) the weighted segment of a batched fused launch: `grid` workgroups of wg_table, NSLOT = slots
void launch_fused_batch_weighted(int slots, unsigned grid, hipStream_t stream, const FlatBatchMember* members,
                                 const int2* wg_table, int J, int Jpad, int parity);

}  // namespace hgmm
