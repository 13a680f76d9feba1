// Batched HGMM: B independent clouds per launch set ("forest").
//
// The reference's unit of work is ONE scan pair -- registration_gmmtree(source, target): buildGMMTree of the source
// (src/python/hgmm/hgmm_gpu.py:466-548) + GMMTree.registration of the target (hgmm_gpu.py:754-768, E-step 550-577), called
// at hgmm_gpu.py:802-807.  A 40 k-point pair is ~350 launches whose dependent trips to memory leave an MI355X > 95 % idle
// (profiles/r05/kernel_trace_pair.txt); host threads driving several contexts top out near 1000 pairs/s.  Here B pairs
// share every launch:
//
//   hgmm_tree_build_batch      the B source clouds lie back to back in the context's resident cloud.  At level l the forest
//                              has B 8^l parent segments (segment p: cloud p >> 3 l); the partition kernels, the chunk table and
//                              the E-step work on segments and never notice; the moments, the log-likelihood and the stop rule
//                              find their cloud from the segment / the workgroup index and keep ONE state per cloud (stop
//                              flag, loop state, q shares, trace, progress word).  The levels run in lock-step: a cloud
//                              whose level has stopped costs a returned workgroup per launch until the last one stops.
//   hgmm_tree_set_targets_batch / hgmm_tree_register_batch
//                              the B targets back to back, one table entry per pair (transform, fixed-point encoding,
//                              active flag), one E-step launch + one normal-equations launch per iteration for ALL pairs,
//                              the B 6 x 6 solves on the host (north_star keeps the rigid solve there) between them.
//
// Every workgroup runs the arithmetic of the serial call for its cloud -- the device code is the SAME functions
// (csrc/tree_device.h), the chunks, blocks and orders of summation are the serial ones, the host steps are the same inline
// functions -- so trees, iteration counts, q traces and (R, t) are bitwise those of hgmm_tree_build / hgmm_tree_register
// (tests/test_tree_batch_gpu.py).
#include "tree_host.h"

namespace hgmm {

// ------------------------------------------------------------------------------------------
// kernels
// ------------------------------------------------------------------------------------------
__global__ void forest_prep_kernel(const double* __restrict__ pi, const double* __restrict__ mu,
                                   const double* __restrict__ cov, int64_t n_nodes, int T, double* __restrict__ prep,
                                   int* __restrict__ flags /*[B]*/) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_nodes) return;
    const double* c = cov + 9 * j;
    prep_node(pi[j], mu[3 * j], mu[3 * j + 1], mu[3 * j + 2], c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[8],
              prep + PREP_N * j, flags + j / T);
}

// (An XCD-aware work order -- XCD x taking the x-th contiguous eighth of the chunks instead of every eighth chunk, so that a
//  few clouds' node parameters stay in one XCD's scalar caches and L2 -- was built and measured in round 6: the build of 32
//  bunny scans went from 8.9 to 13.9 ms, 3650 -> 2740 pairs/s.  Eight widely spaced streams through the point arrays cost
//  more than the scalar loads' ~800-cycle misses; the grid order stays.)
// launch 0 of a level: the E-step of every chunk of every cloud
// (WEIGHTED: hgmm_tree_set_source_weights_batch -- ea.w, the forest's weights in the order of ea.xs)
template <bool HALF, bool WEIGHTED = false>
__global__ __launch_bounds__(CH, 7) void forest_estep_kernel(TreeEstepArgs ea, ForestArgs fa) {
    __shared__ double smem[tree_estep_lds<HALF>()];
    tree_estep_body<HALF, true, WEIGHTED>((int)blockIdx.x, ea, NO_FOLLOW, smem, &fa);
}

// One wave per child node of the level, all clouds: tree_moments_kernel with the cloud's own stop flag, point count and --
// from the level's second iteration on -- the cloud's own verdict on the previous iteration's q (tree_follow_wave: this
// launch is the one that follows the log-likelihood; the cloud's first wave speaks for it).
__global__ __launch_bounds__(64) void forest_moments_kernel(const double* __restrict__ partials,
                                                            const int* __restrict__ chunk_first, int n_level,
                                                            double* __restrict__ mom, int64_t lb, double ld, double* pi,
                                                            double* mu, double* cov, double* prep, int* __restrict__ flags,
                                                            ForestArgs fa, const double* __restrict__ block_q, int e) {
    const int cg = blockIdx.x;                       // forest-wide child index: cloud b's children are [b n_level, (b + 1) n_level)
    const int b = cg / n_level, cl = cg - b * n_level;
    const int seg = cg >> 3, k = cg & 7;             // (n_level is a multiple of 8: cg >> 3 = b 8^l + (cl >> 3), the parent segment)
    ForestCloud* fc = fa.clouds + b;
    const int stop_flag = fc->done;                  // (the cloud's entry and the chunk range: one trip)
    const int q_first = fc->q_first, q_count = fc->q_count;
    const double n_total = fc->n_total;
    const int c0 = chunk_first[seg], c1 = chunk_first[seg + 1];
    if (e >= 1 && c0 == c1 && cl != 0) return;      // (children of a parent without points: tree_moments_kernel)
    const TreeFollow follow = forest_follow(fa, b, e, block_q, q_first, q_count);
    TreeFollowLoads fl;
    if (e >= 1) fl = tree_follow_wave_load(follow);
    else if (stop_flag) return;
    double acc[NMOM];
    tree_moments_gather(partials, c0, c1, k, acc);
    if (e >= 1 && tree_follow_wave_verdict(follow, fl, stop_flag, cl == 0)) return;
#pragma unroll
    for (int m = 0; m < NMOM; ++m) acc[m] = wave_sum_f64(acc[m]);
    if (threadIdx.x == 0) {
        const int64_t node = (int64_t)b * fa.T + lb + cl;
#pragma unroll
        for (int m = 0; m < NMOM; ++m) mom[(size_t)node * NMOM + m] = acc[m];
        mstep_node(acc, node, n_total, ld, pi, mu, cov, prep, flags + b, /*with_complexity=*/false);
    }
}

// The same for the eight children of one parent per wave (tree_moments_gather8: the same sums bit for bit)
__global__ __launch_bounds__(64) void forest_moments8_kernel(const double* __restrict__ partials,
                                                             const int* __restrict__ chunk_first, int n_level,
                                                             double* __restrict__ mom, int64_t lb, double ld, double* pi,
                                                             double* mu, double* cov, double* prep, int* __restrict__ flags,
                                                             ForestArgs fa, const double* __restrict__ block_q, int e) {
    const int seg = blockIdx.x;                      // forest-wide parent segment; its children are cg = 8 seg + k
    const int b = (8 * seg) / n_level, cl0 = 8 * seg - b * n_level;
    ForestCloud* fc = fa.clouds + b;
    const int stop_flag = fc->done;
    const int q_first = fc->q_first, q_count = fc->q_count;
    const double n_total = fc->n_total;
    const int c0 = chunk_first[seg], c1 = chunk_first[seg + 1];
    if (e >= 1 && c0 == c1 && cl0 != 0) return;      // (children of a parent without points: tree_moments_kernel)
    const TreeFollow follow = forest_follow(fa, b, e, block_q, q_first, q_count);
    TreeFollowLoads fl;
    if (e >= 1) fl = tree_follow_wave_load(follow);
    else if (stop_flag) return;
    double acc[NMOM];
    tree_moments_gather8(partials, c0, c1, acc);
    if (e >= 1 && tree_follow_wave_verdict(follow, fl, stop_flag, cl0 == 0)) return;
    if ((threadIdx.x & 7) == 0) {
        const int64_t node = (int64_t)b * fa.T + lb + cl0 + ((int)threadIdx.x >> 3);
#pragma unroll
        for (int m = 0; m < NMOM; ++m) mom[(size_t)node * NMOM + m] = acc[m];
        mstep_node(acc, node, n_total, ld, pi, mu, cov, prep, flags + b, /*with_complexity=*/false);
    }
}

// Iteration e's log-likelihood of every cloud + (with_estep) iteration e + 1's speculative E-step of every chunk, as in
// tree_ll_estep_kernel.  Workgroups [0, B ll_stride): cloud w / ll_stride, point block w % ll_stride (clouds with fewer
// blocks return); the rest: chunks.
// (float64 pdfs: five waves per SIMD, 96 registers, no spills; 4 / 5 / 6 measured 14.2 / 13.9 / 14.4 ms per build of 32 bunny
//  scans -- the kernel keeps the fp64 pipe ~80 % busy at any of them, profiles/r06/pmc_sq_batch32.txt.  float32 pdfs: the
//  launch is latency chains of E-step workgroups for the larger part -- six waves at 80 registers, still without spills)
// F32: the log-likelihood workgroups evaluate their pdfs in float32 (hgmm_tree_set_precision; tree_loglik_f32_body)
// WEIGHTED: both halves read ea.w (the log-likelihood's points are the E-step's, in the same order)
template <bool F32, bool WEIGHTED = false>
__global__ __launch_bounds__(CH, F32 ? 6 : 5) void forest_ll_estep_kernel(const double* __restrict__ xs, int64_t n_pad,
                                                             const double* __restrict__ prep, int64_t lb, int n_level,
                                                             double* __restrict__ block_q, const int* __restrict__ flags,
                                                             ForestArgs fa, int ll_stride, TreeEstepArgs ea, int with_estep) {
    constexpr int LL_LDS = F32 ? tree_loglik_f32_lds() : tree_loglik_lds<false>();
    constexpr int LDS = LL_LDS > tree_estep_lds<true>() ? LL_LDS : tree_estep_lds<true>();
    __shared__ __attribute__((aligned(16))) double smem[LDS];
    const int w = (int)blockIdx.x;
    const int n_ll = fa.B * ll_stride;
    if (w < n_ll) {
        const int b = w / ll_stride, bx = w - b * ll_stride;
        const ForestCloud* fc = fa.clouds + b;
        const int gx = fc->ll_gx, gy = fc->ll_gy, per_chunk = fc->ll_per_chunk, pt_first = fc->pt_first,
                  pt_count = fc->pt_count, q_first = fc->q_first, q_count = fc->q_count, stop_flag = fc->done;
        if (bx >= gx || stop_flag) return;
        const TreeLoglikArgs la{xs, (int64_t)pt_first + pt_count, n_pad, prep, (int64_t)b * fa.T + lb, n_level, per_chunk,
                                nullptr, block_q + q_first, nullptr, nullptr, nullptr, NO_STOP, flags + b, nullptr, nullptr,
                                (int64_t)pt_first, q_count, WEIGHTED ? ea.w : nullptr};
        if constexpr (F32) tree_loglik_f32_body<2, true, WEIGHTED>(bx, 0, gx, gy, la, smem);
        else tree_loglik_body<2, false, true, WEIGHTED>(bx, 0, gx, gy, la, smem);
    } else if (with_estep) {
        tree_estep_body<true, true, WEIGHTED>(w - n_ll, ea, NO_FOLLOW, smem, &fa);
    }
}

// behind the budget's last iteration: one workgroup per cloud accounts for its q (tree_close_kernel)
__global__ __launch_bounds__(CH) void forest_close_kernel(ForestArgs fa, const double* __restrict__ block_q, int e) {
    __shared__ double sh4[4];
    const int b = blockIdx.x;
    ForestCloud* fc = fa.clouds + b;
    const int stop_flag = fc->done;
    const TreeFollow f = forest_follow(fa, b, e, block_q, fc->q_first, fc->q_count);
    (void)tree_follow(f, stop_flag, sh4, true);
}

// partition: tree_hist_kernel / tree_scatter_kernel with the assignment buffer of the chunk's OWN cloud (iteration e's
// E-step wrote buffer e & 1; a cloud whose level took `it` iterations keeps its assignment in buffer (it - 1) & 1)
__global__ __launch_bounds__(CH) void forest_hist_kernel(const int* __restrict__ cur0, const int* __restrict__ cur1,
                                                         const int* __restrict__ chunk_desc,
                                                         const int* __restrict__ n_chunks, int* __restrict__ hist,
                                                         ForestArgs fa) {
    const int c = blockIdx.x;
    if (c >= *n_chunks) return;
    const int seg = chunk_desc[3 * c], begin = chunk_desc[3 * c + 1], end = chunk_desc[3 * c + 2];
    const int it = fa.clouds[seg >> fa.shift].final_it;
    const int* __restrict__ cur = ((it - 1) & 1) ? cur1 : cur0;
    __shared__ int sh[CH / 64][8];
    tree_hist_waves(cur, begin, end, sh);
    __syncthreads();
    if (threadIdx.x < 8) {
        int t = 0;
        for (int ww = 0; ww < CH / 64; ++ww) t += sh[ww][threadIdx.x];
        hist[c * 8 + threadIdx.x] = t;
    }
}
// (WEIGHTED: the weights travel with the coordinates, as in tree_scatter_kernel)
template <bool WEIGHTED = false>
__global__ __launch_bounds__(CH) void forest_scatter_kernel(const double* __restrict__ xs, int64_t n_pad,
                                                            const int* __restrict__ cur0, const int* __restrict__ cur1,
                                                            const int* __restrict__ chunk_desc,
                                                            const int* __restrict__ n_chunks,
                                                            const int* __restrict__ chunk_off, double* __restrict__ xs_new,
                                                            ForestArgs fa, const double* __restrict__ wts = nullptr,
                                                            double* __restrict__ wts_new = nullptr) {
    const int c = blockIdx.x;
    if (c >= *n_chunks) return;
    const int seg = chunk_desc[3 * c], begin = chunk_desc[3 * c + 1], end = chunk_desc[3 * c + 2];
    const int it = fa.clouds[seg >> fa.shift].final_it;
    const int* __restrict__ cur = ((it - 1) & 1) ? cur1 : cur0;
    tree_scatter_body<WEIGHTED, false>(cur, c, begin, end, xs, n_pad, chunk_off, xs_new, nullptr, nullptr, wts, wts_new);
}

// targets: [n,3] rows -> the forest's structure of arrays at `first`, and the largest |x|^2 of the cloud (the same
// products and sums, in the same order, as hgmm_tree_set_target's host loop: no fused operations)
template <class IN>                                        // (double, or float widened here: the same float64 values either way)
__global__ void forest_target_kernel(const IN* __restrict__ aos, int64_t n, int64_t first, int64_t pad,
                                     double* __restrict__ soa, unsigned long long* __restrict__ r2max_bits) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    double r2 = 0.0;
    if (i < n) {
        const double x = (double)aos[3 * i], y = (double)aos[3 * i + 1], z = (double)aos[3 * i + 2];
        soa[first + i] = x;
        soa[pad + first + i] = y;
        soa[2 * pad + first + i] = z;
        r2 = __dadd_rn(__dadd_rn(__dmul_rn(x, x), __dmul_rn(y, y)), __dmul_rn(z, z));
        if (!(r2 >= 0.0)) r2 = 0.0;                  // (NaN coordinates: the host's `r2 > r2max` never takes them either)
    }
    // non-negative doubles order like their bit patterns
    unsigned long long bits = (unsigned long long)__double_as_longlong(r2);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(bits, off);
        bits = o > bits ? o : bits;
    }
    if (lane_id() == 0 && bits != 0ull) atomicMax(r2max_bits, bits);
}

// ---- registration and score of a SET of registrations (tree_host.h: RegSet) ------------------------------------------------
// One table entry per registration b: its pose, fixed-point encoding and loop state, and slice b of the [B][T][NMQ] sums.
// SHARED = false, the forest (hgmm_tree_register_batch / _score_batch): pair b has its own tree, `prep + PREP_N T b`, and
// its own target, at tg_first of the back-to-back targets.  SHARED = true, start poses of ONE pair (hgmm_tree_register_multi /
// _score_multi, hgmm_tree_register): `prep` is the one resident tree's table, every entry names the same target, which
// starts at 0 -- tg_first is not loaded.  A workgroup serves ONE registration either way: its LDS table of levels 0..2 would
// have to be flushed per start pose otherwise, and the 24 B / point a second pose would save come out of L2 anyway.
template <bool SHARED>
__device__ inline const double* reg_prep_of(const double* __restrict__ prep, int T, int b) {
    if constexpr (SHARED) return prep;
    else return prep + (size_t)PREP_N * T * b;
}

// (GATED: hgmm_tree_set_reg_gate's finite gate, tree_reg_estep_body; the gate-off instantiations do not read the argument)
// (WEIGHTED: hgmm_tree_set_target_weights[_batch]'s array w [tg_pad], indexed like the points; likewise never read without)
template <int NMQ, bool SHARED, bool GATED, bool WEIGHTED>
__global__ __launch_bounds__(CH) void forest_reg_estep_kernel(const double* __restrict__ tg, int64_t tg_pad,
                                                              const ForestRegPair* __restrict__ tab,
                                                              const double* __restrict__ prep, int T, int L,
                                                              double lambda_c, unsigned long long* __restrict__ momq, int gx,
                                                              double maha2_gate, const double* __restrict__ w) {
    __shared__ unsigned long long lds[REG_LDS_NODES * NMQ];
    const int item = (int)blockIdx.x;                  // (a one-dimensional grid of gx x B items: registration b, chunk bx)
    const int b = item / gx, bx = item - b * gx;
    const ForestRegPair* pr = tab + b;
    int first = 0;
    if constexpr (!SHARED) first = pr->tg_first;
    const int active = pr->active, count = pr->tg_count;
    if (!active || (int64_t)bx * CH >= count) return;
    const Rigid tf = pr->tf;
    const double inv_d = pr->inv_d, fix_scale = pr->fix_scale;
    const int64_t li = (int64_t)bx * CH + threadIdx.x;
    tree_reg_estep_body<NMQ, GATED, WEIGHTED>(first + li, li < count, tg, tg_pad, tf, reg_prep_of<SHARED>(prep, T, b), L, lambda_c,
                                              inv_d, fix_scale, momq + (size_t)NMQ * T * b, lds, maha2_gate, w);
}

// the score of every registration (tree_score_body), b's workgroups starting at its target's first point as in the kernel
// above -- the serial call's grouping, so its shares and its summary are the serial call's bit for bit.  Reads the pose and
// the target's place from the table, NOT `active`: every entry is scored.  partial: [B][gx][6]
template <bool SHARED, bool WEIGHTED>
__global__ __launch_bounds__(CH) void forest_score_kernel(const double* __restrict__ tg, int64_t tg_pad,
                                                          const ForestRegPair* __restrict__ tab,
                                                          const double* __restrict__ prep, int T, int L, double lambda_c,
                                                          double maha2_max, double* __restrict__ partial, int gx,
                                                          const double* __restrict__ w) {
    const int item = (int)blockIdx.x;
    const int b = item / gx, bx = item - b * gx;
    const ForestRegPair* pr = tab + b;
    int first = 0;
    if constexpr (!SHARED) first = pr->tg_first;
    const int count = pr->tg_count;
    if ((int64_t)bx * CH >= count) return;
    const Rigid tf = pr->tf;
    const int64_t li = (int64_t)bx * CH + threadIdx.x;
    tree_score_body<WEIGHTED>(first + li, li, li < count, tg, tg_pad, tf, reg_prep_of<SHARED>(prep, T, b), L, lambda_c, maha2_max,
                              nullptr, nullptr, nullptr, partial + (size_t)SCORE_NSUM * item, w);
}
// (nothing here depends on whose tree it was: one kernel for both kinds of set)
__global__ __launch_bounds__(CH) void forest_score_finish_kernel(const double* __restrict__ partial,
                                                                 const ForestRegPair* __restrict__ tab, int gx,
                                                                 double* __restrict__ summary) {
    const int b = blockIdx.x;
    const int count = tab[b].tg_count;
    // (tg_wtotal: the target's weight sum, (double)count without weights -- reg_pair)
    tree_score_finish_body(partial + (size_t)SCORE_NSUM * gx * b, (count + CH - 1) / CH, tab[b].tg_wtotal, summary + 8 * b);
}

template <bool SHARED>
__global__ __launch_bounds__(256) void forest_reg_normal_kernel(unsigned long long* __restrict__ momq,
                                                                const ForestRegPair* __restrict__ tab,
                                                                const double* __restrict__ prep, int T,
                                                                double* __restrict__ out, double* host_out,
                                                                unsigned long long* host_seq, unsigned long long seq) {
    const int b = blockIdx.x;
    const ForestRegPair* pr = tab + b;
    if (!pr->active) return;
    tree_reg_normal_body(momq + (size_t)4 * T * b, pr->d_ext, pr->inv_scale, reg_prep_of<SHARED>(prep, T, b), T, out + 28 * b,
                         host_out + 28 * b, host_seq + b, seq);
}

// reg_device_solve: the normal equations of registration b, then -- one thread -- the host's part of the iteration
// (reg_device_step) and b's progress word for the host: (left the loop << 32) | iterations done
template <bool SHARED>
__global__ __launch_bounds__(256) void forest_reg_solve_kernel(unsigned long long* __restrict__ momq, ForestRegPair* tab,
                                                               const double* __restrict__ prep, int T,
                                                               double* __restrict__ out, double tol, int max_iter,
                                                               double* __restrict__ trace, unsigned long long* host_words) {
    const int b = blockIdx.x;
    ForestRegPair* pr = tab + b;
    if (!pr->active) return;
    tree_reg_normal_body(momq + (size_t)4 * T * b, pr->d_ext, pr->inv_scale, reg_prep_of<SHARED>(prep, T, b), T, out + 28 * b,
                         nullptr, nullptr, 0ull);
    __syncthreads();                                         // (the 28 sums are in `out`, written by this workgroup)
    if (threadIdx.x == 0) {
        const int it = pr->it;
        reg_device_step(out + 28 * b, pr, tol, max_iter, trace ? trace + ((size_t)b * max_iter + it) * 13 : nullptr);
        __hip_atomic_store(host_words + b, ((unsigned long long)(pr->active ? 0 : 1) << 32) | (unsigned long long)(unsigned)pr->it,
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// ---- a third kind of set: R registrations OVER the resident forest (hgmm_tree_register_batch_multi / _score_batch_multi) --------
// Registration r reads the tree and the target of pair owner[r] -- `prep + PREP_N T owner`, and the table entry's tg_first /
// tg_count / tg_wtotal are that pair's -- and owns slice r of everything that is written: the sums, the table, the 28 numbers,
// the score's shares, its progress / sequence word.  The owner travels in the entry's spare word (ForestRegPair::owner).  These
// are kernels of their own over the same bodies, so that the forest's and the shared set's kernels above stay the code they
// were; a workgroup still serves one registration, and the grid is the one-dimensional gx x R.
template <bool GATED, bool WEIGHTED>
__global__ __launch_bounds__(CH) void forest_owned_reg_estep_kernel(const double* __restrict__ tg, int64_t tg_pad,
                                                                    const ForestRegPair* __restrict__ tab,
                                                                    const double* __restrict__ prep, int T, int L,
                                                                    double lambda_c, unsigned long long* __restrict__ momq,
                                                                    int gx, double maha2_gate, const double* __restrict__ w) {
    __shared__ unsigned long long lds[REG_LDS_NODES * 4];
    const int item = (int)blockIdx.x;                  // (gx x R items: registration r, chunk bx)
    const int r = item / gx, bx = item - r * gx;
    const ForestRegPair* pr = tab + r;
    const int first = pr->tg_first, active = pr->active, count = pr->tg_count, owner = pr->owner;
    if (!active || (int64_t)bx * CH >= count) return;
    const Rigid tf = pr->tf;
    const double inv_d = pr->inv_d, fix_scale = pr->fix_scale;
    const int64_t li = (int64_t)bx * CH + threadIdx.x;
    tree_reg_estep_body<4, GATED, WEIGHTED>(first + li, li < count, tg, tg_pad, tf, reg_prep_of<false>(prep, T, owner), L, lambda_c,
                                            inv_d, fix_scale, momq + (size_t)4 * T * r, lds, maha2_gate, w);
}

// partial: [R][gx][6]; forest_score_finish_kernel adds the shares of every entry as it does for the other sets
template <bool WEIGHTED>
__global__ __launch_bounds__(CH) void forest_owned_score_kernel(const double* __restrict__ tg, int64_t tg_pad,
                                                                const ForestRegPair* __restrict__ tab,
                                                                const double* __restrict__ prep, int T, int L, double lambda_c,
                                                                double maha2_max, double* __restrict__ partial, int gx,
                                                                const double* __restrict__ w) {
    const int item = (int)blockIdx.x;
    const int r = item / gx, bx = item - r * gx;
    const ForestRegPair* pr = tab + r;
    const int first = pr->tg_first, count = pr->tg_count, owner = pr->owner;
    if ((int64_t)bx * CH >= count) return;
    const Rigid tf = pr->tf;
    const int64_t li = (int64_t)bx * CH + threadIdx.x;
    tree_score_body<WEIGHTED>(first + li, li, li < count, tg, tg_pad, tf, reg_prep_of<false>(prep, T, owner), L, lambda_c, maha2_max,
                              nullptr, nullptr, nullptr, partial + (size_t)SCORE_NSUM * item, w);
}

__global__ __launch_bounds__(256) void forest_owned_reg_normal_kernel(unsigned long long* __restrict__ momq,
                                                                      const ForestRegPair* __restrict__ tab,
                                                                      const double* __restrict__ prep, int T,
                                                                      double* __restrict__ out, double* host_out,
                                                                      unsigned long long* host_seq, unsigned long long seq) {
    const int r = blockIdx.x;
    const ForestRegPair* pr = tab + r;
    if (!pr->active) return;
    tree_reg_normal_body(momq + (size_t)4 * T * r, pr->d_ext, pr->inv_scale, reg_prep_of<false>(prep, T, pr->owner), T, out + 28 * r,
                         host_out + 28 * r, host_seq + r, seq);
}

__global__ __launch_bounds__(256) void forest_owned_reg_solve_kernel(unsigned long long* __restrict__ momq, ForestRegPair* tab,
                                                                     const double* __restrict__ prep, int T,
                                                                     double* __restrict__ out, double tol, int max_iter,
                                                                     double* __restrict__ trace, unsigned long long* host_words) {
    const int r = blockIdx.x;
    ForestRegPair* pr = tab + r;
    if (!pr->active) return;
    tree_reg_normal_body(momq + (size_t)4 * T * r, pr->d_ext, pr->inv_scale, reg_prep_of<false>(prep, T, pr->owner), T, out + 28 * r,
                         nullptr, nullptr, 0ull);
    __syncthreads();                                         // (the 28 sums are in `out`, written by this workgroup)
    if (threadIdx.x == 0) {
        const int it = pr->it;
        reg_device_step(out + 28 * r, pr, tol, max_iter, trace ? trace + ((size_t)r * max_iter + it) * 13 : nullptr);
        __hip_atomic_store(host_words + r, ((unsigned long long)(pr->active ? 0 : 1) << 32) | (unsigned long long)(unsigned)pr->it,
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
// The E-step of a set's registration loops: shared tree or forest, gate off or on (hgmm_tree_set_reg_gate), without or with
// per-point weights of the target (hgmm_tree_set_target_weights[_batch]).  The one place a further flag is added.
struct RegEstepFamily { template <bool... FLAGS> static auto kernel() { return forest_reg_estep_kernel<4, FLAGS...>; } };
struct RegSolveFamily { template <bool SHARED> static auto kernel() { return forest_reg_solve_kernel<SHARED>; } };
struct ScoreFamily { template <bool SHARED, bool W> static auto kernel() { return forest_score_kernel<SHARED, W>; } };
// ... and of a set over the forest (RegSet::owned), whose kernels take the arguments of the others
struct OwnedRegEstepFamily { template <bool G, bool W> static auto kernel() { return forest_owned_reg_estep_kernel<G, W>; } };
struct OwnedScoreFamily { template <bool W> static auto kernel() { return forest_owned_score_kernel<W>; } };
static auto reg_estep_kernel_for(const hgmm_ctx* c, const RegSet& set) {
    const bool gated = std::isfinite(c->tree.reg_gate), weighted = set.w != nullptr;
    if (set.owned) return kernel_for<OwnedRegEstepFamily>(gated, weighted);
    return kernel_for<RegEstepFamily>(set.shared_tree, gated, weighted);
}
static auto reg_solve_kernel_for(const RegSet& set) {
    return set.owned ? forest_owned_reg_solve_kernel : kernel_for<RegSolveFamily>(set.shared_tree);
}
static auto reg_normal_kernel_for(const RegSet& set) {
    if (set.owned) return forest_owned_reg_normal_kernel;
    return set.shared_tree ? forest_reg_normal_kernel<true> : forest_reg_normal_kernel<false>;
}
static auto score_kernel_for(const RegSet& set) {
    return set.owned ? kernel_for<OwnedScoreFamily>(set.w != nullptr) : kernel_for<ScoreFamily>(set.shared_tree, set.w != nullptr);
}

// The registration loop of a set with the device on its own (reg_device_solve): every iteration is two launches -- the
// E-step of all registrations, then per registration the normal equations + reg_device_step -- enqueued by a host that only
// follows the progress words and keeps a few iterations ahead of the slowest running one; launches behind a registration's
// stop return at their first load.  The caller's arrays are filled at the end.  (register_set has opened the sums.)
static int forest_register_on_device(hgmm_ctx* c, const RegSet& set, double* rot, double* t, double scale, double lambda_c,
                                     int max_iter, double tol, double* q_prev_inout, int32_t* iters_out, int32_t* status_out,
                                     double* trace) {
    const int B = set.B(), T = set.T;
    for (int b = 0; b < B; ++b) { iters_out[b] = 0; status_out[b] = 0; }
    if (max_iter < 1) return HGMM_OK;
    RegTable tb;
    HGMM_TRY(reg_table(c, *set.table, B, &tb));
    const size_t trace_bytes = trace ? sizeof(double) * 13 * (size_t)max_iter * B : 0;
    if (trace) HGMM_TRY(ensure(c, c->fr_trace, trace_bytes));
    const auto estep_kernel = reg_estep_kernel_for(c, set);
    const auto solve_kernel = reg_solve_kernel_for(set);
    unsigned long long* momq = set.momq->as<unsigned long long>();
    double* d_trace = trace ? c->fr_trace.as<double>() : nullptr;
    HandOver* hand = nullptr;
    HGMM_TRY(hand_over(c, B, &hand));
    const HostDev<unsigned long long> words = hand->progress(0);
    std::vector<ForestRegPair> tab(B);
    for (int b = 0; b < B; ++b) {
        ForestRegPair& pr = tab[b] = reg_pair(set.regs[b]);
        reg_pair_fill(pr, rigid_from(rot + 9 * b, t + 3 * b, scale), set.regs[b]);
        pr.has_q = (q_prev_inout[b] == q_prev_inout[b]) ? 1 : 0;              // (NaN: no previous q)
        pr.q_prev = pr.has_q ? q_prev_inout[b] : 0.0;
        __atomic_store_n(words.host + b, 0ull, __ATOMIC_RELAXED);
    }
    HGMM_TRY(stage_h2d(c, tb.pairs, tab.data(), sizeof(ForestRegPair) * B));
    const unsigned gx = set.gx();
    const auto enqueue = [&](int) -> int {
        {
            ProfScope prof(c, HGMM_K_TREE_REG);
            estep_kernel<<<gx * (unsigned)B, CH, 0, c->stream>>>(set.tg, set.tg_pad, tb.pairs, set.prep, T, set.L, lambda_c, momq,
                                                                 (int)gx, c->tree.reg_gate, set.w);
        }
        solve_kernel<<<B, 256, 0, c->stream>>>(momq, tb.pairs, set.prep, T, tb.out, tol, max_iter, d_trace, words.dev);
        HGMM_HIP(c, hipGetLastError());
        return HGMM_OK;
    };
    const int ahead = 3;
    HGMM_TRY(follow_ahead(c, words.host, B, max_iter, ahead, enqueue, nothing_at_budget, nullptr, "registration (device loop)"));
    std::vector<double> trace_host(trace ? (size_t)13 * max_iter * B : 0);
    {
        StagedDownloads dl(c);
        dl.add(tab.data(), tb.pairs, sizeof(ForestRegPair) * B);
        if (trace) dl.add(trace_host.data(), d_trace, trace_bytes);
        HGMM_HIP(c, dl.finish());
    }
    for (int b = 0; b < B; ++b) {
        const ForestRegPair& pr = tab[b];
        for (int i = 0; i < 9; ++i) rot[9 * b + i] = pr.tf.r[i];
        for (int i = 0; i < 3; ++i) t[3 * b + i] = pr.tf.t[i];
        iters_out[b] = pr.it;
        status_out[b] = pr.status;
        if (pr.has_q) q_prev_inout[b] = pr.q_prev;
        if (trace) std::memcpy(trace + (size_t)13 * max_iter * b, trace_host.data() + (size_t)13 * max_iter * b, sizeof(double) * 13 * (size_t)pr.it);
    }
    return HGMM_OK;
}

// The registration loop of a set with the 6 x 6 solves on the host (the default): per iteration one E-step launch and one
// normal-equations launch for all registrations still running, each one's 28 numbers solved as soon as its sequence word
// arrives.  (register_set has opened the sums: every iteration's normal-equations kernel zeroes the words it read.)
static int forest_register_on_host(hgmm_ctx* c, const RegSet& set, double* rot, double* t, double scale, double lambda_c,
                                   int max_iter, double tol, double* q_prev_inout, int32_t* iters_out, int32_t* status_out,
                                   double* trace) {
    const int B = set.B(), T = set.T;
    HandOver* hand = nullptr;
    HGMM_TRY(hand_over(c, B, &hand));
    const HostDev<unsigned long long> words = hand->sequence(0);
    const HostDev<double> h_out = hand->out28(0);
    RegTable tb;
    HGMM_TRY(reg_table(c, *set.table, B, &tb));
    const auto estep_kernel = reg_estep_kernel_for(c, set);
    const auto normal_kernel = reg_normal_kernel_for(set);
    unsigned long long* momq = set.momq->as<unsigned long long>();
    std::vector<ForestRegPair> tab(B);
    std::vector<char> active(B, 1);
    for (int b = 0; b < B; ++b) {
        iters_out[b] = 0;
        status_out[b] = 0;                                        // 0: budget used up, 1: |dq| < tol, 2: host M-step needed
    }
    const unsigned gx = set.gx();
    int n_active = B;
    for (int it = 0; it < max_iter && n_active > 0; ++it) {
        for (int b = 0; b < B; ++b) {
            tab[b] = reg_pair(set.regs[b]);
            if (active[b]) reg_pair_fill(tab[b], rigid_from(rot + 9 * b, t + 3 * b, scale), set.regs[b]);
        }
        HGMM_TRY(stage_h2d(c, tb.pairs, tab.data(), sizeof(ForestRegPair) * B));
        const unsigned long long seq = ++hand->seq;
        {
            ProfScope prof(c, HGMM_K_TREE_REG);
            estep_kernel<<<gx * (unsigned)B, CH, 0, c->stream>>>(set.tg, set.tg_pad, tb.pairs, set.prep, T, set.L, lambda_c, momq,
                                                                 (int)gx, c->tree.reg_gate, set.w);
        }
        normal_kernel<<<B, 256, 0, c->stream>>>(momq, tb.pairs, set.prep, T, tb.out, h_out.dev, words.dev, seq);
        HGMM_HIP(c, hipGetLastError());
        // every active registration's normal equations arrive with its own sequence word; each is solved as soon as it is there
        std::vector<char> pending(active);
        int n_pending = n_active;
        unsigned spins = 0;
        while (n_pending > 0) {
            bool progressed = false;
            unsigned long long seen = 0;                   // signature of the sequence words as this pass read them
            for (int b = 0; b < B; ++b) {
                const unsigned long long w = __atomic_load_n(words.host + b, __ATOMIC_ACQUIRE);
                seen += w;
                if (!pending[b] || w != seq) continue;
                pending[b] = 0;
                --n_pending;
                progressed = true;
                double q = 0.0;
                const int stp = reg_host_step(h_out.host + 28 * b, rot + 9 * b, t + 3 * b, q_prev_inout + b, tol, &q);
                if (stp == 2) { status_out[b] = 2; active[b] = 0; --n_active; continue; }
                if (trace) {
                    double* tr = trace + ((size_t)b * max_iter + it) * 13;
                    for (int i = 0; i < 9; ++i) tr[i] = rot[9 * b + i];
                    for (int i = 0; i < 3; ++i) tr[9 + i] = t[3 * b + i];
                    tr[12] = q;
                }
                iters_out[b] = it + 1;
                if (stp == 1) { status_out[b] = 1; active[b] = 0; --n_active; }
            }
            if (progressed) { spins = 0; continue; }
            HGMM_TRY(device_watch(c, &spins, words.host, B, seen, "registration (batch): the normal-equation kernel (sequence %llu)", seq));
        }
    }
    return HGMM_OK;
}

int register_set(hgmm_ctx* c, const RegSet& set, double* rot, double* t, double scale, double lambda_c, int max_iter, double tol,
                 double* q_prev_inout, int32_t* iters_out, int32_t* status_out, double* trace) {
    MomqScope sums(*set.momq_clean);               // (one memset at the most; every later iteration finds the words zero)
    HGMM_TRY(sums.open(c, *set.momq, set.momq_bytes));
    const auto loop = c->cfg[CFG_REG_DEVICE_SOLVE] ? forest_register_on_device : forest_register_on_host;
    HGMM_TRY(loop(c, set, rot, t, scale, lambda_c, max_iter, tol, q_prev_inout, iters_out, status_out, trace));
    sums.consumed();                               // every iteration's normal-equations / solve kernel zeroed what its E-step had added
    return HGMM_OK;
}

int score_set(hgmm_ctx* c, const RegSet& set, const double* rot, const double* t, double scale, double lambda_c,
              double maha2_max, double* summary_out) {
    const int B = set.B();
    RegTable tb;
    HGMM_TRY(reg_table(c, *set.table, B, &tb));
    std::vector<ForestRegPair> tab(B);
    for (int b = 0; b < B; ++b) {
        tab[b] = reg_pair(set.regs[b]);
        tab[b].tf = rigid_from(rot ? rot + 9 * b : nullptr, t ? t + 3 * b : nullptr, scale);
    }
    const unsigned gx = set.gx();
    HGMM_TRY(ensure(c, c->scratch, sizeof(double) * ((size_t)SCORE_NSUM * gx + 8) * B));
    double* partial = c->scratch.as<double>();
    double* d_sum = partial + (size_t)SCORE_NSUM * gx * B;
    HGMM_TRY(stage_h2d(c, tb.pairs, tab.data(), sizeof(ForestRegPair) * B));
    {
        ProfScope prof(c, HGMM_K_TREE_SCORE);
        const auto kernel = score_kernel_for(set);
        kernel<<<gx * (unsigned)B, CH, 0, c->stream>>>(set.tg, set.tg_pad, tb.pairs, set.prep, set.T, set.L, lambda_c, maha2_max,
                                                      partial, (int)gx, set.w);
    }
    forest_score_finish_kernel<<<B, CH, 0, c->stream>>>(partial, tb.pairs, (int)gx, d_sum);
    HGMM_HIP(c, hipGetLastError());
    StagedDownloads dl(c);
    dl.add(summary_out, d_sum, sizeof(double) * 8 * B);
    HGMM_HIP(c, dl.finish());
    return HGMM_OK;
}

// ---- the kernel families of the forest build (kernel_for, hgmm_ctx.h; the last flag: WEIGHTED) ---------------------------
// (the forest's E-step is always the two-pass form)
struct ForestEstepFamily { template <bool W> static auto kernel() { return forest_estep_kernel<true, W>; } };
struct ForestLlEstepFamily { template <bool F32, bool W> static auto kernel() { return forest_ll_estep_kernel<F32, W>; } };
struct ForestScatterFamily { template <bool W> static auto kernel() { return forest_scatter_kernel<W>; } };

// ---- one level of the forest build (hgmm_tree_build's BuildLevel in its one mode: overlapped, follow) ---------------------
struct ForestLevel {
    hgmm_ctx* c;
    const BuildWorkspace& ws;
    int l, P;                        // the level and the forest's parent segments
    double ld;
    int max_iters;
    ForestArgs fa;
    int ll_stride;                   // log-likelihood workgroups per cloud (the longest cloud's); level 0: none
    int* d_flags;
    // ---- set by prepare() ----
    int64_t lb, parent_first;        // a cloud's first node of the level, n_level of them; ... of the level above
    int n_level;
    unsigned grid_chunks;

    void prepare() {
        lb = level_first(l);
        n_level = (int)(level_first(l + 1) - lb);
        parent_first = (l == 0) ? 0 : level_first(l - 1);
        tree_chunks_kernel<<<1, 1024, 0, c->stream>>>(ws.seg, P, ws.chunk_first, ws.chunk_desc, ws.n_chunks_dev);
        grid_chunks = (unsigned)(c->n / CH + P + 1);
    }
    int enqueue(int e) const {
        const bool weighted = ws.w != nullptr;
        const int64_t n_pad = c->n_pad;
        const int B = fa.B;
        double *d_pi = c->fr_pi.as<double>(), *d_mu = c->fr_mu.as<double>(), *d_cov = c->fr_cov.as<double>();
        double *d_prep = c->fr_prep.as<double>(), *d_mom = c->fr_mom.as<double>(), *block_q = c->fr_q.as<double>();
        const TreeEstepArgs ea_now{ws.xs, n_pad, d_prep, ws.chunk_desc, ws.n_chunks_dev, parent_first, l, ws.partials,
                                   ws.cur[e & 1], nullptr, nullptr, ws.w};
        const auto estep = kernel_for<ForestEstepFamily>(weighted);
        if (e == 0) {
            ProfScope prof(c, HGMM_K_TREE_ESTEP);
            estep<<<grid_chunks, CH, 0, c->stream>>>(ea_now, fa);
        }
        if (l > 0)
            forest_moments8_kernel<<<(unsigned)(B * n_level / 8), 64, 0, c->stream>>>(ws.partials, ws.chunk_first, n_level, d_mom, lb, ld,
                                                                                     d_pi, d_mu, d_cov, d_prep, d_flags, fa, block_q, e);
        else                                                    // (level 0: a wave per child, tree_moments8_kernel's note)
            forest_moments_kernel<<<(unsigned)(B * n_level), 64, 0, c->stream>>>(ws.partials, ws.chunk_first, n_level, d_mom, lb, ld,
                                                                                d_pi, d_mu, d_cov, d_prep, d_flags, fa, block_q, e);
        {
            ProfScope prof(c, HGMM_K_TREE_LOGLIK);
            // (level 0: behind the budget's last iteration the E-step runs for the shares of q alone)
            const int with_estep = (e + 1 < max_iters || l == 0) ? 1 : 0;
            const TreeEstepArgs ea_next{ws.xs, n_pad, d_prep, ws.chunk_desc, ws.n_chunks_dev, parent_first, l, ws.partials,
                                        ws.cur[(e + 1) & 1], nullptr, l == 0 ? block_q : nullptr, ws.w};
            const unsigned g = (unsigned)(B * ll_stride) + (with_estep ? grid_chunks : 0u);
            if (l == 0)
                // (level 0 is E-step workgroups only: the plain E-step kernel -- 72 registers instead of the fused kernel's
                //  92-96, one more wave per SIMD for a launch that is a chain of trips to memory)
                estep<<<grid_chunks, CH, 0, c->stream>>>(ea_next, fa);
            else {
                const auto fused = kernel_for<ForestLlEstepFamily>(c->tree.pdf_f32, weighted);
                fused<<<g, CH, 0, c->stream>>>(ws.xs, n_pad, d_prep, lb, n_level, block_q, d_flags, fa, ll_stride, ea_next, with_estep);
            }
        }
        const hipError_t le = hipGetLastError();
        if (le != hipSuccess) return fail(c, HGMM_ERR_HIP, "tree build (batch): kernel launch failed: %s", hipGetErrorString(le));
        return HGMM_OK;
    }
    // behind the budget's last iteration: one workgroup per cloud accounts for its q
    int close() const {
        forest_close_kernel<<<fa.B, CH, 0, c->stream>>>(fa, c->fr_q.as<double>(), max_iters);
        if (hipGetLastError() != hipSuccess) return fail(c, HGMM_ERR_HIP, "tree build (batch): launch failed");
        return HGMM_OK;
    }
};

}  // namespace hgmm

using namespace hgmm;

// hgmm_tree_build_batch (init_mu) and hgmm_tree_build_batch_rows (init_rows [B][T]: row numbers within each cloud, gathered
// on the device into the place init_mu is uploaded to): exactly one of the two is given
static int tree_build_batch(hgmm_ctx* c, int B, const int64_t* counts, int L, double ls, double ld,
                            const double* init_mu, const int64_t* init_rows, bool by_rows, double sig2, int max_iters_per_level,
                            double* pi_out, double* mu_out, double* cov_out, int32_t* iters_out, double* q_trace_out,
                            int q_capacity, int32_t* q_len_out) {
    HGMM_ENTER(c);
    if (!c->have_f64 || c->n <= 0) return fail(c, HGMM_ERR_STATE, "tree build (batch): set points first");
    if (B < 1 || B > 4096 || !counts) return fail(c, HGMM_ERR_ARG, "tree build (batch): B = %d clouds", B);
    if (L < 1 || L > 6) return fail(c, HGMM_ERR_ARG, "tree levels L = %d outside 1..6", L);
    if (by_rows ? !init_rows : !init_mu) return fail(c, HGMM_ERR_ARG, by_rows ? "init_rows is NULL" : "init_mu is NULL");
    if (c->comm_on()) return fail(c, HGMM_ERR_STATE, "tree build (batch): independent clouds take no communicator");
    if (c->n > 0x7fffffff - 1024) return fail(c, HGMM_ERR_ARG, "too many points for 32-bit indices");
    if (max_iters_per_level < 1) max_iters_per_level = 1;
    const int64_t n = c->n, n_pad = c->n_pad;
    {
        int64_t sum = 0;
        for (int b = 0; b < B; ++b) {
            if (counts[b] < 1) return fail(c, HGMM_ERR_ARG, "tree build (batch): cloud %d has no points", b);
            // (a cloud of >= 400 000 points fills the chip by itself and takes the serial build's four-points-per-thread
            //  log-likelihood, which this path does not reproduce)
            if (counts[b] >= 400000)
                return fail(c, HGMM_ERR_ARG, "tree build (batch): cloud %d has %lld points; clouds of >= 400000 points "
                            "go through hgmm_tree_build", b, (long long)counts[b]);
            sum += counts[b];
        }
        if (sum != n) return fail(c, HGMM_ERR_ARG, "tree build (batch): the counts add up to %lld, the resident cloud has %lld points",
                                  (long long)sum, (long long)n);
    }
    // hgmm_tree_set_source_weights_batch: the WEIGHTED instantiations, the weights on the coordinates' ping-pong
    const double* wsrc = c->forest.src_w.ptr();
    if (wsrc && (c->forest.src_counts.size() != (size_t)B || !std::equal(counts, counts + B, c->forest.src_counts.begin())))
        return fail(c, HGMM_ERR_ARG, "tree build (batch): the resident source weights were set for other cloud sizes");
    const int64_t T = level_first(L);
    const int64_t TT = T * B;
    if (by_rows)
        for (int64_t j = 0; j < TT; ++j)
            if (init_rows[j] < 0 || init_rows[j] >= counts[j / T])
                return fail(c, HGMM_ERR_ARG, "tree build (batch): init_rows[%lld][%lld] = %lld, but cloud %lld has %lld points",
                            (long long)(j / T), (long long)(j % T), (long long)init_rows[j], (long long)(j / T), (long long)counts[j / T]);
    int64_t P8 = 1;
    for (int i = 0; i < L - 1; ++i) P8 *= 8;                   // parents of one cloud at the last level
    const int64_t maxP = P8 * B;
    if (TT > 0x3fffffff || maxP > (1 << 24)) return fail(c, HGMM_ERR_ARG, "tree build (batch): %d clouds x %d levels is too large", B, L);
    // (one mode: every cloud is small, so every level is an overlapped follow-mode level of the serial build)
    const int ahead_iters = 2;                                  // iterations enqueued beyond the slowest running cloud (hgmm_tree_build)
    ForestState& F = c->forest;
    F.nodes_ready = false;
    HGMM_TRY(ensure(c, c->fr_pi, sizeof(double) * TT));
    HGMM_TRY(ensure(c, c->fr_mu, sizeof(double) * 3 * TT));
    HGMM_TRY(ensure(c, c->fr_cov, sizeof(double) * 9 * TT));
    HGMM_TRY(ensure(c, c->fr_prep, sizeof(double) * PREP_N * TT));
    HGMM_TRY(ensure(c, c->fr_mom, sizeof(double) * NMOM * TT));
    HGMM_TRY(ensure(c, c->fr_clouds, sizeof(ForestCloud) * B + sizeof(int) * (B + 1) + 256));
    HGMM_TRY(ensure(c, c->fr_q, sizeof(double) * (size_t)(n / CH + B + 8)));
    const int trace_cap = std::min(max_iters_per_level, 4096);
    HGMM_TRY(ensure(c, c->fr_trace, sizeof(double) * (size_t)trace_cap * L * B));
    HGMM_TRY(ensure(c, c->scratch, sizeof(double) * 3 * TT));
    BuildWorkspace ws;
    HGMM_TRY(ws.take(c, n, n_pad, maxP, L, c->x_soa64.as<double>(), wsrc));
    HandOver* hand = nullptr;
    HGMM_TRY(hand_over(c, B, &hand));
    const HostDev<unsigned long long> words = hand->progress(0);

    double *d_pi = c->fr_pi.as<double>(), *d_mu = c->fr_mu.as<double>(), *d_cov = c->fr_cov.as<double>();
    double* d_prep = c->fr_prep.as<double>();
    ForestCloud* d_clouds = c->fr_clouds.as<ForestCloud>();
    int* d_flags = reinterpret_cast<int*>(d_clouds + B);
    double* trace_base = c->fr_trace.as<double>();

    // node tables: pi = 1/8, mu = given, cov = sig2 I for every tree; per-cloud form flags start at zero
    if (by_rows) {
        std::vector<int64_t> first_row(B, 0);
        for (int b = 1; b < B; ++b) first_row[b] = first_row[b - 1] + counts[b - 1];
        HGMM_TRY(stage_init_rows(c, init_rows, TT, first_row.data(), T));
    } else {
        HGMM_HIP(c, hipMemcpyAsync(c->scratch.p, init_mu, sizeof(double) * 3 * TT, hipMemcpyHostToDevice, c->stream));
    }
    HGMM_HIP(c, hipMemsetAsync(d_flags, 0, sizeof(int) * (B + 1), c->stream));
    tree_init_nodes_kernel<<<nblk(TT, 256), 256, 0, c->stream>>>(c->scratch.as<double>(), sig2, TT, d_pi, d_mu, d_cov);
    forest_prep_kernel<<<nblk(TT, 256), 256, 0, c->stream>>>(d_pi, d_mu, d_cov, TT, (int)T, d_prep, d_flags);
    HGMM_HIP(c, hipGetLastError());
    std::vector<int> first(B + 1, 0);
    for (int b = 0; b < B; ++b) first[b + 1] = first[b] + (int)counts[b];
    HGMM_TRY(stage_h2d(c, ws.seg, first.data(), sizeof(int) * (B + 1)));

    int P = B;
    std::vector<int> level_iters((size_t)B * L, 0);
    std::vector<ForestCloud> table(B);
    int rc = HGMM_OK;
    for (int l = 0; l < L && rc == HGMM_OK; ++l) {
        const int n_level = (int)(level_first(l + 1) - level_first(l));
        // the clouds' entries for this level: the decomposition the serial build would use for each of them
        int q_at = 0, ll_stride = 1;
        for (int b = 0; b < B; ++b) {
            ForestCloud& fc = table[b];
            std::memset(&fc, 0, sizeof fc);
            fc.pt_first = first[b];
            fc.pt_count = (int)counts[b];
            const int llblocks = (int)nblk(counts[b], CH * 2);
            int chunks = 1, per_chunk = n_level;
            tree_ll_split(llblocks, n_level, c->cus, &chunks, &per_chunk);
            fc.ll_gx = llblocks;
            fc.ll_gy = chunks;
            fc.ll_per_chunk = per_chunk;
            fc.q_first = q_at;
            // (level 0: the E-step stores the shares, one per chunk -- a cloud's chunks are consecutive, TreeEstepArgs::q_shares)
            fc.q_count = (l == 0 || chunks > 1) ? (int)nblk(counts[b], CH) : llblocks;
            q_at += fc.q_count;
            fc.n_total = c->forest.src_w.total(counts[b], b);                      // (an unweighted member: its count)
            ll_stride = std::max(ll_stride, llblocks);
        }
        if (l == 0) ll_stride = 0;                              // no log-likelihood workgroups at level 0
        rc = stage_h2d(c, d_clouds, table.data(), sizeof(ForestCloud) * B);
        if (rc != HGMM_OK) break;
        const ForestArgs fa{d_clouds, B, (int)T, 3 * l, ls, max_iters_per_level, trace_base, trace_cap, L, l, words.dev};
        ForestLevel lv{c, ws, l, P, ld, max_iters_per_level, fa, ll_stride, d_flags};
        lv.prepare();
        for (int b = 0; b < B; ++b) __atomic_store_n(words.host + b, 0ull, __ATOMIC_RELAXED);
        rc = follow_ahead(c, words.host, B, max_iters_per_level, ahead_iters, [&lv](int e) { return lv.enqueue(e); },
                          [&lv] { return lv.close(); }, nullptr, "tree build (batch)");
        if (rc != HGMM_OK) {
            c->err += " (level " + std::to_string(l) + ")";
            break;
        }
        for (int b = 0; b < B; ++b)
            level_iters[(size_t)b * L + l] = (int)(__atomic_load_n(words.host + b, __ATOMIC_ACQUIRE) & 0xffffffffull);
        if (l + 1 < L) {
            // partition for the next level
            forest_hist_kernel<<<lv.grid_chunks, CH, 0, c->stream>>>(ws.cur[0], ws.cur[1], ws.chunk_desc, ws.n_chunks_dev, ws.hist, lv.fa);
            tree_offsets_kernel<<<P, OFF_BLOCK, 0, c->stream>>>(ws.hist, ws.chunk_first, ws.seg, P, ws.chunk_off, ws.seg_next);
            const auto scatter = kernel_for<ForestScatterFamily>(wsrc != nullptr);
            scatter<<<lv.grid_chunks, CH, 0, c->stream>>>(ws.xs, n_pad, ws.cur[0], ws.cur[1], ws.chunk_desc, ws.n_chunks_dev,
                                                          ws.chunk_off, ws.xs_next, lv.fa, ws.w, ws.w_next);
            if (hipGetLastError() != hipSuccess) { rc = fail(c, HGMM_ERR_HIP, "tree build (batch): partition launch failed"); break; }
            ws.advance();
            P *= 8;
        }
    }
    if (rc != HGMM_OK) {
        (void)ctx_stream_sync(c);
        return rc;
    }
    // The serial pair goes on through hgmm_tree_set_nodes: the finished tables are prepared once more, by tree_prep_kernel
    // (complexity ratio included).  The SAME kernel runs here over the whole forest, so that the registration reads the very
    // numbers it reads after a serial build (the per-iteration preparation inside the moments kernel is the same function
    // inlined elsewhere -- the compiler need not contract it alike).  Its one flags word is a scratch word behind the clouds'.
    tree_prep_kernel<<<nblk(TT, 256), 256, 0, c->stream>>>(d_pi, d_mu, d_cov, 0, TT, d_prep, d_flags + B);
    HGMM_HIP(c, hipGetLastError());
    // the means always come back (the registration's extent bound needs the largest |mu| per tree); the rest on request
    std::vector<double> mu_host;
    double* mu_dst = mu_out;
    if (!mu_dst) { mu_host.resize((size_t)3 * TT); mu_dst = mu_host.data(); }
    std::vector<double> trace_host;
    if (q_trace_out) trace_host.resize((size_t)trace_cap * L * B);
    {
        StagedDownloads dl(c);
        dl.add(mu_dst, d_mu, sizeof(double) * 3 * TT);
        dl.add(pi_out, d_pi, sizeof(double) * TT);
        dl.add(cov_out, d_cov, sizeof(double) * 9 * TT);
        if (q_trace_out) dl.add(trace_host.data(), trace_base, sizeof(double) * trace_host.size());
        HGMM_HIP(c, dl.finish());
    }
    F.B = B;
    F.L = L;
    F.T = (int)T;
    F.counts.assign(counts, counts + B);
    F.mu_rmax.resize(B);
    for (int b = 0; b < B; ++b) F.mu_rmax[b] = tree_mu_rmax(mu_dst + (size_t)3 * T * b, T);
    if (iters_out) std::copy(level_iters.begin(), level_iters.end(), iters_out);
    for (int b = 0; b < B; ++b) {
        const int q_len = gather_traces(&level_iters[(size_t)b * L], L, trace_cap, q_trace_out ? q_capacity : 0, [&](int at, int l, int take) {
            std::memcpy(q_trace_out + (size_t)b * q_capacity + at, trace_host.data() + ((size_t)b * L + l) * trace_cap, sizeof(double) * take);
        });
        if (q_len_out) q_len_out[b] = q_len < q_capacity ? q_len : q_capacity;
    }
    F.nodes_ready = true;
    return HGMM_OK;
}

extern "C" int hgmm_tree_build_batch(hgmm_ctx* c, int B, const int64_t* counts, int L, double ls, double ld,
                                     const double* init_mu, double sig2, int max_iters_per_level, double* pi_out,
                                     double* mu_out, double* cov_out, int32_t* iters_out, double* q_trace_out,
                                     int q_capacity, int32_t* q_len_out) {
    return tree_build_batch(c, B, counts, L, ls, ld, init_mu, nullptr, false, sig2, max_iters_per_level, pi_out, mu_out, cov_out,
                            iters_out, q_trace_out, q_capacity, q_len_out);
}
extern "C" int hgmm_tree_build_batch_rows(hgmm_ctx* c, int B, const int64_t* counts, int L, double ls, double ld,
                                          const int64_t* init_rows, double sig2, int max_iters_per_level, double* pi_out,
                                          double* mu_out, double* cov_out, int32_t* iters_out, double* q_trace_out,
                                          int q_capacity, int32_t* q_len_out) {
    return tree_build_batch(c, B, counts, L, ls, ld, nullptr, init_rows, true, sig2, max_iters_per_level, pi_out, mu_out, cov_out,
                            iters_out, q_trace_out, q_capacity, q_len_out);
}

extern "C" int hgmm_tree_get_nodes_batch(hgmm_ctx* c, int b, double* pi_out, double* mu_out, double* cov_out) {
    HGMM_ENTER(c);
    const ForestState& F = c->forest;
    if (!F.nodes_ready) return fail(c, HGMM_ERR_STATE, "no forest (hgmm_tree_build_batch first)");
    if (b < 0 || b >= F.B) return fail(c, HGMM_ERR_ARG, "tree %d of %d", b, F.B);
    const size_t T = (size_t)F.T;
    StagedDownloads dl(c);
    dl.add(pi_out, c->fr_pi.as<double>() + T * b, sizeof(double) * T);
    dl.add(mu_out, c->fr_mu.as<double>() + 3 * T * b, sizeof(double) * 3 * T);
    dl.add(cov_out, c->fr_cov.as<double>() + 9 * T * b, sizeof(double) * 9 * T);
    HGMM_HIP(c, dl.finish());
    return HGMM_OK;
}

template <class IN>
static int set_targets_batch(hgmm_ctx* c, int B, const IN* const* xyz, const int64_t* counts) {
    HGMM_ENTER(c);
    if (B < 1 || B > 4096 || !xyz || !counts) return fail(c, HGMM_ERR_ARG, "targets (batch): B = %d", B);
    forest_targets_begin(c);
    int64_t total = 0, longest = 0;
    for (int b = 0; b < B; ++b) {
        if (!xyz[b] || counts[b] < 1) return fail(c, HGMM_ERR_ARG, "targets (batch): target %d is empty", b);
        total += counts[b];
        longest = std::max(longest, counts[b]);
    }
    if (total > 0x7fffffff - 1024) return fail(c, HGMM_ERR_ARG, "too many target points for 32-bit indices");
    const int64_t pad = (total + 255) / 256 * 256;
    HGMM_TRY(ensure(c, c->fr_tg, sizeof(double) * 3 * pad));
    HGMM_TRY(ensure(c, c->scratch, sizeof(IN) * 3 * (size_t)total));
    RegTable tb;
    HGMM_TRY(reg_table(c, c->fr_reg, B, &tb));
    unsigned long long* r2bits = tb.r2max;
    HGMM_HIP(c, hipMemsetAsync(r2bits, 0, sizeof(unsigned long long) * B, c->stream));
    int64_t at = 0;
    IN* stage = c->scratch.as<IN>();
    for (int b = 0; b < B; ++b) {
        HGMM_HIP(c, hipMemcpyAsync(stage + 3 * at, xyz[b], sizeof(IN) * 3 * (size_t)counts[b], hipMemcpyHostToDevice, c->stream));
        forest_target_kernel<IN><<<nblk(counts[b], 256), 256, 0, c->stream>>>(stage + 3 * at, counts[b], at, pad, c->fr_tg.as<double>(),
                                                                             r2bits + b);
        at += counts[b];
    }
    HGMM_HIP(c, hipGetLastError());
    std::vector<unsigned long long> bits(B);
    {
        StagedDownloads dl(c);
        dl.add(bits.data(), r2bits, sizeof(unsigned long long) * B);
        HGMM_HIP(c, dl.finish());
    }
    forest_targets_publish(c, B, counts, bits.data(), pad, nullptr);
    return HGMM_OK;
}

extern "C" int hgmm_tree_set_targets_batch(hgmm_ctx* c, int B, const double* const* xyz, const int64_t* counts) {
    return set_targets_batch<double>(c, B, xyz, counts);
}
extern "C" int hgmm_tree_set_targets_batch_f32(hgmm_ctx* c, int B, const float* const* xyz, const int64_t* counts) {
    return set_targets_batch<float>(c, B, xyz, counts);
}

// per-point weights of the resident targets (include/hgmm.h): forest.tg_w [tg_pad] parallel to fr_tg (upload_weights)
extern "C" int hgmm_tree_set_target_weights_batch(hgmm_ctx* c, int B, const double* const* w, const int64_t* counts) {
    HGMM_ENTER(c);
    const char* what = "hgmm_tree_set_target_weights_batch";
    ForestState& F = c->forest;
    if (F.tg_B < 1) return fail(c, HGMM_ERR_STATE, "%s: no targets (call hgmm_tree_set_targets_batch first)", what);
    if (!w) { F.tg_w.drop(); return HGMM_OK; }
    if (B != F.tg_B) return fail(c, HGMM_ERR_ARG, "%s: B = %d, but %d targets are resident", what, B, F.tg_B);
    if (!counts) return fail(c, HGMM_ERR_ARG, "%s: counts is NULL", what);
    return upload_weights(c, what, "target", true, B, w, counts, F.tg_counts.data(), F.tg_pad, F.tg_w);
}

// per-point weights of the resident forest cloud (include/hgmm.h): forest.src_w [n_pad] parallel to x_soa64 (upload_weights)
extern "C" int hgmm_tree_set_source_weights_batch(hgmm_ctx* c, int B, const double* const* w, const int64_t* counts) {
    HGMM_ENTER(c);
    const char* what = "hgmm_tree_set_source_weights_batch";
    ForestState& F = c->forest;
    if (!c->have_f64 || c->n <= 0 || F.src_counts.empty())
        return fail(c, HGMM_ERR_STATE, "%s: no forest cloud (call hgmm_set_points_batch_f64 / _f32 first)", what);
    if (!w) { F.src_w.drop(); return HGMM_OK; }
    if (B != (int)F.src_counts.size())
        return fail(c, HGMM_ERR_ARG, "%s: B = %d, but %d clouds are resident", what, B, (int)F.src_counts.size());
    if (!counts) return fail(c, HGMM_ERR_ARG, "%s: counts is NULL", what);
    return upload_weights(c, what, "cloud", true, B, w, counts, F.src_counts.data(), c->n_pad, F.src_w);
}

extern "C" int hgmm_tree_register_batch(hgmm_ctx* c, int B, double* rot, double* t, double scale, double lambda_c,
                                        int max_iter, double tol, double* q_prev_inout, int32_t* iters_out,
                                        int32_t* status_out, double* trace) {
    HGMM_ENTER(c);
    if (!rot || !t || !q_prev_inout || !iters_out || !status_out) return fail(c, HGMM_ERR_ARG, "tree_register (batch): NULL argument");
    const ForestState& F = c->forest;
    if (!F.nodes_ready) return fail(c, HGMM_ERR_STATE, "registration (batch): no forest (hgmm_tree_build_batch first)");
    if (B != F.B || B != F.tg_B)
        return fail(c, HGMM_ERR_STATE, "registration (batch): %d pairs, but %d trees and %d targets are resident", B, F.B, F.tg_B);
    return register_set(c, reg_set_forest(c), rot, t, scale, lambda_c, max_iter, tol, q_prev_inout, iters_out, status_out, trace);
}

// hgmm_tree_score on every pair (tree b, target b) of the resident forest, summaries only: include/hgmm.h
extern "C" int hgmm_tree_score_batch(hgmm_ctx* c, int B, const double* rot, const double* t, double scale, double lambda_c,
                                     double maha2_max, double* summary_out) {
    HGMM_ENTER(c);
    if (!summary_out) return fail(c, HGMM_ERR_ARG, "tree_score (batch): summary_out is NULL");
    if (maha2_max != maha2_max) return fail(c, HGMM_ERR_ARG, "tree_score (batch): maha2_max is NaN");
    if (c->comm_on()) return fail(c, HGMM_ERR_STATE, "tree_score (batch): independent pairs take no communicator");
    const ForestState& F = c->forest;
    if (!F.nodes_ready) return fail(c, HGMM_ERR_STATE, "tree_score (batch): no forest (hgmm_tree_build_batch first)");
    if (B != F.B || B != F.tg_B)
        return fail(c, HGMM_ERR_STATE, "tree_score (batch): %d pairs, but %d trees and %d targets are resident", B, F.B, F.tg_B);
    return score_set(c, reg_set_forest(c), rot, t, scale, lambda_c, maha2_max, summary_out);
}

// ---- multi-start: K start poses of the SERIAL pair (hgmm_tree_build / _set_nodes + hgmm_tree_set_target): include/hgmm.h ------
// what both entries ask of the context
static int multi_state(hgmm_ctx* c, const char* what, int K) {
    if (c->comm_on()) return fail(c, HGMM_ERR_STATE, "%s: start poses of one pair take no communicator", what);
    if (!c->tree.nodes_ready) return fail(c, HGMM_ERR_STATE, "%s: no tree (build or set_nodes first)", what);
    if (c->tgt_n <= 0) return fail(c, HGMM_ERR_STATE, "%s: no target (call hgmm_tree_set_target first)", what);
    if (K < 1 || K > 4096) return fail(c, HGMM_ERR_ARG, "%s: K = %d start poses outside 1..4096", what, K);
    if ((uint64_t)nblk(c->tgt_n, CH) * (uint64_t)K > 0x7fffffffull)                // (the grid: one workgroup per pose and chunk)
        return fail(c, HGMM_ERR_ARG, "%s: %d start poses x %lld target points is too large", what, K, (long long)c->tgt_n);
    return HGMM_OK;
}

extern "C" int hgmm_tree_register_multi(hgmm_ctx* c, int K, double* rot, double* t, double scale, double lambda_c,
                                        int max_iter, double tol, double* q_prev_inout, int32_t* iters_out,
                                        int32_t* status_out, double* trace) {
    HGMM_ENTER(c);
    HGMM_TRY(multi_state(c, "tree_register (multi)", K));
    if (!rot || !t) return fail(c, HGMM_ERR_ARG, "tree_register (multi): rot / t is NULL (K start poses are the call's input)");
    if (!q_prev_inout || !iters_out || !status_out) return fail(c, HGMM_ERR_ARG, "tree_register (multi): NULL output argument");
    HGMM_TRY(tree_mu_rmax_resident(c));
    return register_set(c, reg_set_pair(c, K, true), rot, t, scale, lambda_c, max_iter, tol, q_prev_inout, iters_out, status_out,
                        trace);
}

extern "C" int hgmm_tree_score_multi(hgmm_ctx* c, int K, const double* rot, const double* t, double scale, double lambda_c,
                                     double maha2_max, double* summary_out) {
    HGMM_ENTER(c);
    HGMM_TRY(multi_state(c, "tree_score (multi)", K));
    if (!rot || !t) return fail(c, HGMM_ERR_ARG, "tree_score (multi): rot / t is NULL (K poses are the call's input)");
    if (!summary_out) return fail(c, HGMM_ERR_ARG, "tree_score (multi): summary_out is NULL");
    if (maha2_max != maha2_max) return fail(c, HGMM_ERR_ARG, "tree_score (multi): maha2_max is NaN");
    return score_set(c, reg_set_pair(c, K, true), rot, t, scale, lambda_c, maha2_max, summary_out);
}

// ---- batched multi-start: R hypotheses over the resident FOREST, hypothesis r on pair[r] (include/hgmm.h) ---------------------
// what both entries ask of the context and of `pair`; nothing resident has been touched when this refuses
static int batch_multi_state(hgmm_ctx* c, const char* what, int R, const int32_t* pair) {
    const ForestState& F = c->forest;
    if (c->comm_on()) return fail(c, HGMM_ERR_STATE, "%s: hypotheses over a forest take no communicator", what);
    if (!F.nodes_ready) return fail(c, HGMM_ERR_STATE, "%s: no forest (hgmm_tree_build_batch first)", what);
    if (F.tg_B < 1) return fail(c, HGMM_ERR_STATE, "%s: no targets (hgmm_tree_set_targets_batch first)", what);
    if (F.B != F.tg_B) return fail(c, HGMM_ERR_STATE, "%s: %d trees, but %d targets are resident", what, F.B, F.tg_B);
    if (R < 1) return fail(c, HGMM_ERR_ARG, "%s: R = %d hypotheses (at least one)", what, R);
    if (!pair) return fail(c, HGMM_ERR_ARG, "%s: pair is NULL", what);
    int64_t longest = 0;
    for (int r = 0; r < R; ++r) {
        if (pair[r] < 0 || pair[r] >= F.B)
            return fail(c, HGMM_ERR_ARG, "%s: pair[%d] = %d, but the forest has the pairs 0..%d", what, r, (int)pair[r], F.B - 1);
        longest = std::max(longest, F.tg_counts[pair[r]]);
    }
    if ((uint64_t)nblk(longest, CH) * (uint64_t)R > 0x7fffffffull)                 // (the grid: one workgroup per hypothesis and chunk)
        return fail(c, HGMM_ERR_ARG, "%s: %d hypotheses x %lld target points is more than 2^31 - 1 workgroups", what, R,
                    (long long)longest);
    // the sums: 32 T bytes per hypothesis (1.2 MB at L = 5, 9.6 MB at L = 6), capped so that a long list of hypotheses of a
    // deep forest is a refusal the caller can act on (split it: any subset is a valid call), not a failed allocation
    const uint64_t per = (uint64_t)sizeof(unsigned long long) * 4 * (uint64_t)F.T;
    if (per * (uint64_t)R > HGMM_TREE_BATCH_MULTI_MAX_BYTES)
        return fail(c, HGMM_ERR_ARG, "%s: the sums of R = %d hypotheses at L = %d take %llu bytes, more than the cap of %llu; "
                    "at most R = %llu hypotheses fit into one call", what, R, F.L, (unsigned long long)(per * (uint64_t)R),
                    (unsigned long long)HGMM_TREE_BATCH_MULTI_MAX_BYTES, (unsigned long long)(HGMM_TREE_BATCH_MULTI_MAX_BYTES / per));
    return HGMM_OK;
}

extern "C" int hgmm_tree_register_batch_multi(hgmm_ctx* c, int R, const int32_t* pair, double* rot, double* t, double scale,
                                              double lambda_c, int max_iter, double tol, double* q_prev_inout,
                                              int32_t* iters_out, int32_t* status_out, double* trace) {
    HGMM_ENTER(c);
    const char* what = "tree_register (batch multi)";
    HGMM_TRY(batch_multi_state(c, what, R, pair));
    if (!rot || !t) return fail(c, HGMM_ERR_ARG, "%s: rot / t is NULL (R start poses are the call's input)", what);
    if (!q_prev_inout || !iters_out || !status_out) return fail(c, HGMM_ERR_ARG, "%s: NULL output argument", what);
    return register_set(c, reg_set_forest_multi(c, R, pair), rot, t, scale, lambda_c, max_iter, tol, q_prev_inout, iters_out,
                        status_out, trace);
}

extern "C" int hgmm_tree_score_batch_multi(hgmm_ctx* c, int R, const int32_t* pair, const double* rot, const double* t,
                                           double scale, double lambda_c, double maha2_max, double* summary_out) {
    HGMM_ENTER(c);
    const char* what = "tree_score (batch multi)";
    HGMM_TRY(batch_multi_state(c, what, R, pair));
    if (!rot || !t) return fail(c, HGMM_ERR_ARG, "%s: rot / t is NULL (R poses are the call's input)", what);
    if (!summary_out) return fail(c, HGMM_ERR_ARG, "%s: summary_out is NULL", what);
    if (maha2_max != maha2_max) return fail(c, HGMM_ERR_ARG, "%s: maha2_max is NaN", what);
    return score_set(c, reg_set_forest_multi(c, R, pair), rot, t, scale, lambda_c, maha2_max, summary_out);
}
