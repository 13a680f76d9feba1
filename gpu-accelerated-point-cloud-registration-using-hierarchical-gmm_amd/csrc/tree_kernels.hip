// Hierarchical GMM (8-ary GMM tree, full 3x3 covariances) for gfx950, float64 arithmetic.
//
// Replaces the reference's Numba-CUDA kernels (src/python/hgmm/hgmm_gpu.py:107-115, 284-426:
// one thread per point, 3x3 inverse + determinant recomputed for every (point,node) pair,
// 104 global float atomics per point per iteration) and follows the semantics of its CPU twin
// (src/python/hgmm/hgmm_cupy_cpu_working.py:62-228), which is the canonical one.
//
//   tree_prep_kernel      once per M-step, per node: Sigma^-1 (6 unique), pi*coef, the
//                         log-likelihood weight (0 when pi < eps or det < eps) and the
//                         'complexity' ratio  -- instead of per pair.
//   partition (hist / offsets / scatter)
//                         the per-level recursion: after a level converges the points are
//                         regrouped (stable counting sort) by the child they were assigned to, so
//                         that at the next level every 256-point chunk shares ONE parent.
//   tree_estep_kernel     one workgroup per chunk, lanes across points; the 8 children's
//                         parameters are workgroup-uniform (scalar loads); responsibilities,
//                         arg-max and the 8 x 10 moment contributions are reduced with DPP wave
//                         reductions + LDS to one partial per chunk.  No atomics, deterministic.
//   tree_moments_kernel   fixed-order fp64 reduction of the chunk partials per node -> the
//                         buffer an RCCL all-reduce works on.
//   tree_mstep_kernel     ML estimate with the CPU twin's empty-node rule (m0 < ld).
//   tree_loglik_kernel    q = sum_i log max(sum_j pi_j N(x_i; j), eps) over ALL nodes of the
//                         level, node table tiled through LDS, wave-uniform skip of far nodes.
//   tree_reg_estep_kernel registration E-step: per target point descend the tree.
#include "tree_host.h"

#include <algorithm>
#include <numeric>
#include <type_traits>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace hgmm {

__global__ void tree_prep_kernel(const double* __restrict__ pi, const double* __restrict__ mu,
                                 const double* __restrict__ cov, int64_t j_begin, int64_t j_end,
                                 double* __restrict__ prep, int* __restrict__ flags) {
    const int64_t j = j_begin + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= j_end) return;
    const double* c = cov + 9 * j;
    prep_node(pi[j], mu[3 * j], mu[3 * j + 1], mu[3 * j + 2], c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[8],
              prep + PREP_N * j, flags);
}

// the 'complexity' ratios of nodes [j_begin, j_end) (prep[11]) from their covariances: one pass when a build is done
__global__ void tree_complexity_kernel(const double* __restrict__ cov, int64_t j_begin, int64_t j_end,
                                       double* __restrict__ prep) {
    const int64_t j = j_begin + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= j_end) return;
    const double* c = cov + 9 * j;
    prep[PREP_N * j + 11] = sym3_min_eig_over_trace(c[0], c[1], c[2], c[4], c[5], c[8]);
}

__global__ void tree_init_nodes_kernel(const double* __restrict__ init_mu, double sig2, int64_t T,
                                       double* pi, double* mu, double* cov) {
    // pi = 1/8, mu = given, cov = sig2 * I   (hgmm_cupy_cpu_working.py:132-136)
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= T) return;
    pi[j] = 1.0 / 8.0;
    for (int d = 0; d < 3; ++d) mu[3 * j + d] = init_mu[3 * j + d];
    for (int e = 0; e < 9; ++e) cov[9 * j + e] = (e % 4 == 0) ? sig2 : 0.0;
}

// ------------------------------------------------------------------------------------------
// chunk table: segment p (points of one parent, contiguous in sorted order) -> ceil(n_p/CH) chunks
// seg_start[P+1]; chunk_first[P+1] (first chunk id of each parent); chunk_desc[c] = {parent, begin, end}
// single workgroup (P <= 32768)
// ------------------------------------------------------------------------------------------
__global__ void tree_chunks_kernel(const int* __restrict__ seg_start, int P, int* __restrict__ chunk_first,
                                   int* __restrict__ chunk_desc, int* __restrict__ n_chunks_out) {
    __shared__ int carry;
    __shared__ int sh[1024];
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < P; base += 1024) {
        const int p = base + threadIdx.x;
        int cnt = 0;
        if (p < P) cnt = (seg_start[p + 1] - seg_start[p] + CH - 1) / CH;
        sh[threadIdx.x] = cnt;
        __syncthreads();
        // inclusive scan (Hillis-Steele)
        for (int off = 1; off < 1024; off <<= 1) {
            int v = (threadIdx.x >= (unsigned)off) ? sh[threadIdx.x - off] : 0;
            __syncthreads();
            sh[threadIdx.x] += v;
            __syncthreads();
        }
        if (p < P) chunk_first[p] = carry + sh[threadIdx.x] - cnt;
        __syncthreads();
        if (threadIdx.x == 1023) carry += sh[1023];
        __syncthreads();
    }
    const int total = carry;
    if (threadIdx.x == 0) {
        chunk_first[P] = total;
        *n_chunks_out = total;
    }
    __syncthreads();                       // chunk_first[] is complete and visible to this workgroup
    // descriptors: every thread takes chunks tid, tid + 1024, ... and finds the chunk's parent by bisection in
    // chunk_first (round 2 let the parent's thread write all of its chunks one after the other: level 0 of a
    // million-point cloud is ONE parent with 3907 chunks -- 165 us of a single thread's stores)
    for (int ch = threadIdx.x; ch < total; ch += 1024) {
        int lo = 0, hi = P - 1;            // last parent with chunk_first[p] <= ch (parents without points share a value)
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (chunk_first[mid] <= ch) lo = mid; else hi = mid - 1;
        }
        // (among parents with the same chunk_first only the last one owns chunks: the bisection lands on it)
        const int s0 = seg_start[lo], s1 = seg_start[lo + 1];
        const int k = ch - chunk_first[lo];
        int* d = chunk_desc + 3 * ch;
        d[0] = lo;
        d[1] = s0 + k * CH;
        d[2] = (s0 + (k + 1) * CH < s1) ? s0 + (k + 1) * CH : s1;
    }
}

__global__ __launch_bounds__(CH) void tree_close_kernel(TreeFollow f) {
    __shared__ double sh4[4];
    (void)tree_follow(f, *f.done, sh4, true);
}

// (WEIGHTED: hgmm_tree_set_source_weights' array w [n_pad] in the order of xs; the unweighted instantiations do not read it)
template <bool HALF, bool WEIGHTED = false>
__global__ __launch_bounds__(CH) void tree_estep_kernel(
    const double* __restrict__ xs, int64_t n_pad, const double* __restrict__ prep,
    const int* __restrict__ chunk_desc, const int* __restrict__ n_chunks, int64_t parent_level_first,
    int level, double* __restrict__ partials, int* __restrict__ cur_sorted, const int* __restrict__ done,
    TreeFollow follow = NO_FOLLOW, const double* __restrict__ w = nullptr) {
    __shared__ double smem[tree_estep_lds<HALF>()];
    tree_estep_body<HALF, false, WEIGHTED>(
        (int)blockIdx.x,
        TreeEstepArgs{xs, n_pad, prep, chunk_desc, n_chunks, parent_level_first, level, partials, cur_sorted, done, nullptr,
                      WEIGHTED ? w : nullptr},
        follow, smem);
}

// fixed-order reduction of the chunk partials of one node (64 threads); with `fuse` the same
// workgroup goes on to the node's M-step + preparation (single-GPU: no all-reduce in between)
__global__ __launch_bounds__(64) void tree_moments_kernel(const double* __restrict__ partials,
                                                          const int* __restrict__ chunk_first,
                                                          int n_level_nodes, double* __restrict__ mom,
                                                          int fuse, int64_t lb, double n_points_total, double ld,
                                                          double* pi, double* mu, double* cov, double* prep,
                                                          int* __restrict__ flags, const int* __restrict__ done,
                                                          TreeFollow follow = NO_FOLLOW) {
    const int cl = blockIdx.x;            // level-local child index
    if (cl >= n_level_nodes) return;
    const int p = cl >> 3, k = cl & 7;
    const int stop_flag = done ? *done : 0;                   // (requested together with the chunk range)
    const int c0 = chunk_first[p], c1 = chunk_first[p + 1];
    // (tree_ll_estep_kernel's launch order: this launch is the one that follows iteration e - 1's log-likelihood; if the
    //  level turns out to have stopped, the partial moments read here are the speculative E-step's and go nowhere)
    // (a parent without points has no chunks, at any iteration of the level: its children's tables were written by the
    //  level's first iteration -- pi = 0, mu = 0, cov = I -- and would be rewritten unchanged; wave 0 speaks for the loop)
    if (follow.q_blocks && c0 == c1 && blockIdx.x != 0) return;
    TreeFollowLoads fl;
    if (follow.q_blocks) fl = tree_follow_wave_load(follow);
    else if (stop_flag) return;
    double acc[NMOM];
    tree_moments_gather(partials, c0, c1, k, acc);
    if (follow.q_blocks && tree_follow_wave_verdict(follow, fl, stop_flag, blockIdx.x == 0)) return;
#pragma unroll
    for (int m = 0; m < NMOM; ++m) acc[m] = wave_sum_f64(acc[m]);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int m = 0; m < NMOM; ++m) mom[(size_t)cl * NMOM + m] = acc[m];
        if (fuse) mstep_node(acc, lb + cl, n_points_total, ld, pi, mu, cov, prep, flags, /*with_complexity=*/false);
    }
}
// the eight children of one parent per wave (tree_moments_gather8: the same sums bit for bit); overlapped builds
__global__ __launch_bounds__(64) void tree_moments8_kernel(const double* __restrict__ partials,
                                                           const int* __restrict__ chunk_first, double* __restrict__ mom,
                                                           int64_t lb, double n_points_total, double ld, double* pi, double* mu,
                                                           double* cov, double* prep, int* __restrict__ flags,
                                                           const int* __restrict__ done, TreeFollow follow) {
    const int p = blockIdx.x;             // level-local parent; its children are cl = 8 p + k
    const int stop_flag = done ? *done : 0;
    const int c0 = chunk_first[p], c1 = chunk_first[p + 1];
    if (follow.q_blocks && c0 == c1 && p != 0) return;
    TreeFollowLoads fl;
    if (follow.q_blocks) fl = tree_follow_wave_load(follow);
    else if (stop_flag) return;
    double acc[NMOM];
    tree_moments_gather8(partials, c0, c1, acc);
    if (follow.q_blocks && tree_follow_wave_verdict(follow, fl, stop_flag, p == 0)) return;
    if ((threadIdx.x & 7) == 0) {
        const int cl = 8 * p + ((int)threadIdx.x >> 3);
#pragma unroll
        for (int m = 0; m < NMOM; ++m) mom[(size_t)cl * NMOM + m] = acc[m];
        mstep_node(acc, lb + cl, n_points_total, ld, pi, mu, cov, prep, flags, /*with_complexity=*/false);
    }
}
__global__ void tree_mstep_kernel(const double* __restrict__ mom, int64_t lb, int n_level_nodes,
                                  double n_points_total, double ld, double* pi, double* mu, double* cov,
                                  double* prep, int* __restrict__ flags, const int* __restrict__ done = nullptr,
                                  int with_complexity = 1) {
    if (done && *done) return;
    const int cl = blockIdx.x * blockDim.x + threadIdx.x;
    if (cl >= n_level_nodes) return;
    mstep_node(mom + (size_t)cl * NMOM, lb + cl, n_points_total, ld, pi, mu, cov, prep, flags, with_complexity != 0);
}

template <int PTS, bool BIGTAB = false, bool WEIGHTED = false>
__global__ __launch_bounds__(CH) void tree_loglik_kernel(const double* __restrict__ xs, int64_t n,
                                                         int64_t n_pad, const double* __restrict__ prep,
                                                         int64_t lb, int n_level_nodes, int nodes_per_chunk,
                                                         double* __restrict__ partial,
                                                         double* __restrict__ block_q,
                                                         unsigned int* __restrict__ ticket,
                                                         double* __restrict__ q_out,
                                                         const int* __restrict__ done, TreeStop stop,
                                                         const int* __restrict__ flags,
                                                         unsigned long long* __restrict__ pair_count,
                                                         const double* __restrict__ exp2_tab = nullptr,
                                                         const double* __restrict__ w = nullptr) {
    __shared__ double smem[tree_loglik_lds<BIGTAB>()];
    tree_loglik_body<PTS, BIGTAB, false, WEIGHTED>(
        (int)blockIdx.x, (int)blockIdx.y, (int)gridDim.x, (int)gridDim.y,
        TreeLoglikArgs{xs, n, n_pad, prep, lb, n_level_nodes, nodes_per_chunk, partial, block_q, ticket, q_out, done, stop, flags,
                       pair_count, exp2_tab, 0, 0, WEIGHTED ? w : nullptr}, smem);
}

// (tree_loglik_f32_body, csrc/tree_device.h: the level log-likelihood with the pdfs in FLOAT32)
template <int PTS, bool WEIGHTED = false>
__global__ __launch_bounds__(CH) void tree_loglik_f32_kernel(TreeLoglikArgs a) {
    __shared__ __attribute__((aligned(16))) double smem[tree_loglik_f32_lds()];
    tree_loglik_f32_body<PTS, false, WEIGHTED>((int)blockIdx.x, (int)blockIdx.y, (int)gridDim.x, (int)gridDim.y, a, smem);
}

// One launch for two independent pieces of work on the same parameters (small clouds, single GPU): the level
// log-likelihood of iteration e and -- on workgroups of their own, behind them in the grid -- the E-step of iteration
// e + 1.  Both read the node parameters iteration e's M-step left; neither reads what the other writes.  The E-step is
// speculative: whether iteration e + 1 exists is decided by the q this very launch produces (the next launch, the
// moments kernel, adds it up and applies the stop rule, tree_follow_wave); if the level stops, the E-step's partial
// moments are never read and its assignment sits in the OTHER of two buffers (iteration e's E-step wrote buffer e & 1).
// What it buys: the E-step's chain of trips to memory (5 - 6 us at C4) runs beside the log-likelihood's instead of
// behind it, and a level-iteration is two or three launches instead of three or four.
// F32: the log-likelihood workgroups evaluate their pdfs in float32 (hgmm_tree_set_precision; tree_loglik_f32_body)
// WEIGHTED: both halves read the weights (la.w == ea.w: the same cloud in the same order)
template <int PTS, bool F32 = false, bool WEIGHTED = false>
__global__ __launch_bounds__(CH) void tree_ll_estep_kernel(TreeLoglikArgs la, int gx, int gy, TreeEstepArgs ea) {
    // (one LDS block for whichever of the two a workgroup turns out to be; the E-step in its two-pass form -- the same
    //  sums bit for bit -- so that both need ~23 KB and the launch's workgroups are all resident at once)
    constexpr int LL_LDS = F32 ? tree_loglik_f32_lds() : tree_loglik_lds<false>();
    constexpr int LDS = LL_LDS > tree_estep_lds<true>() ? LL_LDS : tree_estep_lds<true>();
    __shared__ __attribute__((aligned(16))) double smem[LDS];
    const int nll = gx * gy;
    const int b = (int)blockIdx.x;
    if (b < nll) {
        if constexpr (F32) tree_loglik_f32_body<PTS, false, WEIGHTED>(b % gx, b / gx, gx, gy, la, smem);
        else tree_loglik_body<PTS, false, false, WEIGHTED>(b % gx, b / gx, gx, gy, la, smem);
    } else
        tree_estep_body<true, false, WEIGHTED>(b - nll, ea, NO_FOLLOW, smem);
}

// FASTLOG: the float32-pdf mode's logarithm (log_pos_f64, as in tree_loglik_f32_body's own finish for forests)
// WEIGHTED: lq = w_i log(...) -- the split form's partial sums are unweighted (tree_loglik_body)
template <bool FASTLOG = false, bool WEIGHTED = false>
__global__ __launch_bounds__(CH) void tree_loglik_finish_kernel(const double* __restrict__ partial, int64_t n,
                                                                int64_t n_pad, int n_chunks,
                                                                double* __restrict__ block_q,
                                                                unsigned int* __restrict__ ticket,
                                                                double* __restrict__ q_out,
                                                                const int* __restrict__ done, TreeStop stop,
                                                                const double* __restrict__ wts = nullptr) {
    if (done && *done) return;
    __shared__ double shq[CH / 64];
    const int64_t i = (int64_t)blockIdx.x * CH + threadIdx.x;
    double lq = 0.0;
    if (i < n) {
        [[maybe_unused]] double wt = 0.0;
        if constexpr (WEIGHTED) wt = wts[i];                 // (requested with the partial sums)
        double tot = 0.0;
        for (int c = 0; c < n_chunks; ++c) tot += partial[(size_t)c * n_pad + i];
        lq = FASTLOG ? log_pos_f64(fmax(tot, TREE_EPS)) : log(fmax(tot, TREE_EPS));
        if constexpr (WEIGHTED) lq = weighted_log(wt, lq);
    }
    lq = wave_sum_f64(lq);
    if (lane_id() == 0) shq[wave_in_block()] = lq;
    __syncthreads();
    double t = 0.0;
    for (int w = 0; w < CH / 64; ++w) t += shq[w];
    store_block_q(t, block_q, (int)blockIdx.x, (int)gridDim.x, ticket, q_out, stop);
}

// Device-side stop rule of one tree level (buildGMMTree, hgmm_cupy_cpu_working.py:149-157): record q,
// stop when |q - prev_q| < ls (prev_q starts at 0) or after max_iters.  ctl = {done, iterations};
// prev_q sits behind it.  Lets the host enqueue several iterations per synchronisation: the kernels of
// an iteration that comes after the stop return at once.
__global__ void tree_ctl_kernel(const double* __restrict__ q_dev, TreeCtl* __restrict__ ctl, double ls,
                                int max_iters, double* __restrict__ trace, int trace_cap,
                                unsigned long long* host_word = nullptr) {
    if (ctl->done) return;
    tree_ctl_update(*q_dev, TreeStop{ctl, ls, max_iters, trace, trace_cap, host_word});
}

// (`done`: skip when the loop this launch belongs to has stopped; `stop`: apply the loop's stop rule to the sum)
__global__ __launch_bounds__(256) void tree_sum_kernel(const double* __restrict__ v, int n, double* out,
                                                       const int* __restrict__ done = nullptr,
                                                       TreeStop stop = NO_STOP) {
    // single workgroup, fixed order
    const int stop_flag = done ? *done : 0;                // (requested together with the shares)
    __shared__ double sh[4];
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) acc += v[i];
    if (stop_flag) return;
    acc = wave_sum_f64(acc);
    if (lane_id() == 0) sh[wave_in_block()] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double q = sh[0] + sh[1] + sh[2] + sh[3];
        *out = q;
        if (stop.ctl) tree_ctl_update(q, stop);
    }
}

// ------------------------------------------------------------------------------------------
// partition: regroup the (already parent-grouped) points by the child they were assigned to
// ------------------------------------------------------------------------------------------
// per chunk: 8-bin histogram of the child index
__global__ __launch_bounds__(CH) void tree_hist_kernel(const int* __restrict__ cur_sorted,
                                                       const int* __restrict__ chunk_desc,
                                                       const int* __restrict__ n_chunks,
                                                       int* __restrict__ hist /*[chunks][8]*/) {
    const int c = blockIdx.x;
    if (c >= *n_chunks) return;
    const int begin = chunk_desc[3 * c + 1], end = chunk_desc[3 * c + 2];
    __shared__ int sh[CH / 64][8];
    tree_hist_waves(cur_sorted, begin, end, sh);
    __syncthreads();
    if (threadIdx.x < 8) {
        int t = 0;
        for (int ww = 0; ww < CH / 64; ++ww) t += sh[ww][threadIdx.x];
        hist[c * 8 + threadIdx.x] = t;
    }
}

// one WORKGROUP per parent: new segment sizes + per-chunk write offsets (relative to the parent's segment start,
// children laid out k = 0..7 inside it).  Level 0 has ONE parent owning every chunk of the cloud (3907 at N = 1M):
// a thread per parent walked them one by one, 0.3 ms of dependent loads per pass; here the chunks are spread over
// the 256 threads, child totals by a reduction, offsets by a tiled scan.
__global__ __launch_bounds__(OFF_BLOCK) void tree_offsets_kernel(const int* __restrict__ hist,
                                                                 const int* __restrict__ chunk_first,
                                                                 const int* __restrict__ seg_start, int P,
                                                                 int* __restrict__ chunk_off /*[chunks][8]*/,
                                                                 int* __restrict__ new_seg_start /*[8P+1]*/) {
    const int p = blockIdx.x;
    if (p >= P) return;
    __shared__ int wsum[OFF_BLOCK / 64][8];
    const int tid = threadIdx.x, lane = lane_id(), w = wave_in_block();
    const int c0 = chunk_first[p], c1 = chunk_first[p + 1];
    // pass 1: children's totals
    int t[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) t[k] = 0;
    for (int c = c0 + tid; c < c1; c += OFF_BLOCK)
#pragma unroll
        for (int k = 0; k < 8; ++k) t[k] += hist[c * 8 + k];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int s = wave_reduce_i(t[k], OpAddInt());
        if (lane == 0) wsum[w][k] = s;
    }
    __syncthreads();
    int run[8];                                   // running write offset of child k (every thread keeps a copy)
    {
        int acc = seg_start[p];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            run[k] = acc;
            if (tid == 0) new_seg_start[8 * p + k] = acc;
            acc += (wsum[0][k] + wsum[1][k]) + (wsum[2][k] + wsum[3][k]);
        }
        if (tid == 0 && p == P - 1) new_seg_start[8 * P] = acc;
    }
    __syncthreads();
    // pass 2: exclusive prefix over the parent's chunks, 256 at a time
    for (int base = c0; base < c1; base += OFF_BLOCK) {
        const int c = base + tid;
        const bool ok = c < c1;
        int v[8], incl[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = ok ? hist[c * 8 + k] : 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            incl[k] = wave_scan_i32(v[k]);
            if (lane == 63) wsum[w][k] = incl[k];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            int off = 0;
            for (int ww = 0; ww < w; ++ww) off += wsum[ww][k];
            if (ok) chunk_off[c * 8 + k] = run[k] + off + incl[k] - v[k];
            run[k] += (wsum[0][k] + wsum[1][k]) + (wsum[2][k] + wsum[3][k]);
        }
        __syncthreads();
    }
}

// stable scatter of coordinates / permutation / (as the new parent) child index
// (WEIGHTED: the points' weights travel with their coordinates, wts_new[dst] = wts[i]; the unweighted instantiation reads neither)
template <bool WEIGHTED = false>
__global__ __launch_bounds__(CH) void tree_scatter_kernel(
    const double* __restrict__ xs, int64_t n_pad, const int* __restrict__ perm,
    const int* __restrict__ cur_sorted, const int* __restrict__ chunk_desc,
    const int* __restrict__ n_chunks, const int* __restrict__ chunk_off, double* __restrict__ xs_new,
    int* __restrict__ perm_new, const double* __restrict__ wts = nullptr, double* __restrict__ wts_new = nullptr) {
    const int c = blockIdx.x;
    if (c >= *n_chunks) return;
    const int begin = chunk_desc[3 * c + 1], end = chunk_desc[3 * c + 2];
    tree_scatter_body<WEIGHTED, true>(cur_sorted, c, begin, end, xs, n_pad, chunk_off, xs_new, perm, perm_new, wts, wts_new);
}

__global__ void tree_iota_kernel(int* perm, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) perm[i] = (int)i;
}
__global__ void tree_unsort_kernel(const int* __restrict__ perm, const int* __restrict__ cur_sorted,
                                   int64_t n, int* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[perm[i]] = cur_sorted[i];
}

// (GATED: hgmm_tree_set_reg_gate's finite gate, tree_reg_estep_body; the gate-off instantiations do not read the argument)
// (WEIGHTED: hgmm_tree_set_target_weights' array w [n_pad], likewise: the unweighted instantiations do not read the pointer)
template <int NMQ, bool GATED = false, bool WEIGHTED = false>
__global__ __launch_bounds__(CH) void tree_reg_estep_kernel(const double* __restrict__ tg, int64_t n,
                                                            int64_t n_pad, Rigid tf,
                                                            const double* __restrict__ prep, int L,
                                                            double lambda_c, double inv_d, double fix_scale,
                                                            unsigned long long* __restrict__ momq, double maha2_gate,
                                                            const double* __restrict__ w) {
    __shared__ unsigned long long tab[REG_LDS_NODES * NMQ];
    const int64_t i = (int64_t)blockIdx.x * CH + threadIdx.x;
    tree_reg_estep_body<NMQ, GATED, WEIGHTED>(i, i < n, tg, n_pad, tf, prep, L, lambda_c, inv_d, fix_scale, momq, tab,
                                              maha2_gate, w);
}
// the instantiation for the context's gate and weights
template <int NMQ>
struct TreeRegEstepFamily { template <bool GATED, bool W> static auto kernel() { return tree_reg_estep_kernel<NMQ, GATED, W>; } };
template <int NMQ>
static auto tree_reg_estep_kernel_for(bool gated, bool weighted) { return kernel_for<TreeRegEstepFamily<NMQ>>(gated, weighted); }

// score of the resident target against the resident tree (tree_score_body, csrc/tree_device.h): workgroup b writes its six
// sums to partial[b]; tree_score_finish_kernel (one workgroup) adds them in a fixed order into summary[8]
// (WEIGHTED: hgmm_tree_set_target_weights' array w [n_pad]; the unweighted instantiation does not read the pointer)
template <bool WEIGHTED = false>
__global__ __launch_bounds__(CH) void tree_score_kernel(const double* __restrict__ tg, int64_t n, int64_t n_pad, Rigid tf,
                                                        const double* __restrict__ prep, int L, double lambda_c,
                                                        double maha2_max, int32_t* __restrict__ node_out,
                                                        double* __restrict__ maha2_out, double* __restrict__ logp_out,
                                                        double* __restrict__ partial, const double* __restrict__ w) {
    const int64_t i = (int64_t)blockIdx.x * CH + threadIdx.x;
    tree_score_body<WEIGHTED>(i, i, i < n, tg, n_pad, tf, prep, L, lambda_c, maha2_max, node_out, maha2_out, logp_out,
                              partial + (size_t)SCORE_NSUM * blockIdx.x, w);
}
__global__ __launch_bounds__(CH) void tree_score_finish_kernel(const double* __restrict__ partial, int nb, double n_points,
                                                               double* __restrict__ summary) {
    tree_score_finish_body(partial, nb, n_points, summary);
}

// fixed point -> float64, still centred: cm[T][NMQ] = (m0, c1 = sum gamma (x - mu), C2 = sum gamma (x - mu)(x - mu)^T)
template <int NMQ>
__global__ void tree_reg_unpack_kernel(const unsigned long long* __restrict__ momq, int64_t T, double d,
                                       double inv_scale, double* __restrict__ cm) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= T * NMQ) return;
    const int m = (int)(e % NMQ);
    const double unit = (m == 0) ? inv_scale : (m < 4 ? d * inv_scale : d * d * inv_scale);
    cm[e] = (double)(long long)momq[e] * unit;
}
__global__ void tree_reg_clear_kernel(unsigned long long* __restrict__ momq, int64_t count) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < count) momq[e] = 0ull;
}

// centred moments -> the reference's raw layout m0[T], m1[T,3], m2[T,3,3] (momentsZero/One/Two, C:202-228):
//   m1 = c1 + m0 mu,  m2 = C2 + mu c1^T + c1 mu^T + m0 mu mu^T
__global__ void tree_reg_expand_kernel(const double* __restrict__ cm, const double* __restrict__ prep, int64_t T,
                                       double* m0, double* m1, double* m2) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= T) return;
    const double* c = cm + NMOM * j;
    const double u[3] = {prep[PREP_N * j + 6], prep[PREP_N * j + 7], prep[PREP_N * j + 8]};
    const double z = c[0];
    m0[j] = z;
    for (int a = 0; a < 3; ++a) m1[3 * j + a] = c[1 + a] + z * u[a];
    const int idx[3][3] = {{4, 5, 6}, {5, 7, 8}, {6, 8, 9}};
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b)
            m2[9 * j + 3 * a + b] = c[idx[a][b]] + u[a] * c[1 + b] + c[1 + a] * u[b] + z * u[a] * u[b];
}

// (the body: csrc/tree_device.h, shared with the batched registration)
__global__ __launch_bounds__(256) void tree_reg_normal_kernel(unsigned long long* __restrict__ momq /*[T][4]*/,
                                                              double d_ext, double inv_scale,
                                                              const double* __restrict__ prep, int64_t T,
                                                              double* __restrict__ out,
                                                              double* host_out = nullptr,
                                                              unsigned long long* host_seq = nullptr,
                                                              unsigned long long seq = 0) {
    tree_reg_normal_body(momq, d_ext, inv_scale, prep, T, out, host_out, host_seq, seq);
}

// expand the 10 unique moments into the reference layout m0[T], m1[T,3], m2[T,3,3]
__global__ void tree_expand_moments_kernel(const double* __restrict__ mom, int64_t T, double* m0,
                                           double* m1, double* m2) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= T) return;
    const double* m = mom + NMOM * j;
    m0[j] = m[0];
    m1[3 * j] = m[1]; m1[3 * j + 1] = m[2]; m1[3 * j + 2] = m[3];
    double* o = m2 + 9 * j;
    o[0] = m[4]; o[1] = m[5]; o[2] = m[6]; o[3] = m[5]; o[4] = m[7]; o[5] = m[8]; o[6] = m[6]; o[7] = m[8]; o[8] = m[9];
}

__global__ void tree_copy_cplx_kernel(const double* __restrict__ prep, int64_t T, double* out) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < T) out[j] = prep[PREP_N * j + 11];
}

// ------------------------------------------------------------------------------------------
// host driver
// ------------------------------------------------------------------------------------------

// node tables of T nodes + fresh tree flags
static int tree_alloc_tables(hgmm_ctx* c, int64_t T) {
    HGMM_TRY(ensure(c, c->t_pi, sizeof(double) * T));
    HGMM_TRY(ensure(c, c->t_mu, sizeof(double) * 3 * T));
    HGMM_TRY(ensure(c, c->t_cov, sizeof(double) * 9 * T));
    HGMM_TRY(ensure(c, c->t_prep, sizeof(double) * PREP_N * T));
    HGMM_TRY(ensure(c, c->t_mom, sizeof(double) * NMOM * T));
    HGMM_TRY(tree_flags(c, true));
    return HGMM_OK;
}
static int tree_alloc_nodes(hgmm_ctx* c, int L) {
    c->tree.L = L;
    c->tree.T = (int)level_first(L);
    return tree_alloc_tables(c, c->tree.T);
}

// tree flags (int[4]: bit 0 of [0] = some node's Sigma^-1 failed the Cholesky test) + the executed-pair counter of the
// level log-likelihood (uint64 at byte 16); `reset`: a new node table is about to be prepared
constexpr size_t TREE_FLAGS_BYTES = 64;
constexpr size_t TREE_TICKET_BYTES = sizeof(unsigned int) * TICKET_STRIDE * (1 + TICKET_GROUPS);   // the tickets of store_block_q
int tree_flags(hgmm_ctx* c, bool reset) {
    HGMM_TRY(ensure(c, c->t_flags, TREE_FLAGS_BYTES));
    const bool fresh_tickets = c->t_tickets.p == nullptr;
    HGMM_TRY(ensure(c, c->t_tickets, TREE_TICKET_BYTES));
    // (every launch leaves its counters at zero; a kernel that died mid-way is the exception -> cleared with the flags)
    if (fresh_tickets || reset) HGMM_HIP(c, hipMemsetAsync(c->t_tickets.p, 0, TREE_TICKET_BYTES, c->stream));
    if (reset) {
        HGMM_HIP(c, hipMemsetAsync(c->t_flags.p, 0, TREE_FLAGS_BYTES, c->stream));
        // tree_no_chol: take the symmetric-form fallback everywhere (lets the tests hold both forms to the oracle)
        // tree_rel: add the RELATIVE reach test of tree_loglik_kernel (bit 1).  Off by default: what the absolute
        // test skips is exactly 0 in float64 (q and the stop rule are bitwise those of the full sum), what the relative
        // test drops is "only" below 1e-20 of every point's sum.
        int preset = 0;
        if (c->cfg[CFG_TREE_NO_CHOL]) preset |= 1;
        if (c->cfg[CFG_TREE_REL]) preset |= 2;
        if (preset) HGMM_HIP(c, hipMemsetAsync(c->t_flags.p, preset, 1, c->stream));
    }
    return HGMM_OK;
}
static inline unsigned long long* pairs_ptr(hgmm_ctx* c) {
    return reinterpret_cast<unsigned long long*>(c->t_flags.as<char>() + 16);
}
static inline unsigned int* tickets_ptr(hgmm_ctx* c) { return c->t_tickets.as<unsigned int>(); }

// 2^(j / 2048), j = 0 .. 2047, correctly rounded (formed in the x87 80-bit format), once per context
int ensure_exp_tab2(hgmm_ctx* c) {
    if (c->exp_tab2.p) return HGMM_OK;
    HGMM_TRY(ensure(c, c->exp_tab2, sizeof(double) * EXP_TAB2_N));
    std::vector<double> h(EXP_TAB2_N);
    for (int j = 0; j < EXP_TAB2_N; ++j) h[j] = (double)exp2l((long double)j / (long double)EXP_TAB2_N);
    HGMM_HIP(c, hipMemcpyAsync(c->exp_tab2.p, h.data(), sizeof(double) * EXP_TAB2_N, hipMemcpyHostToDevice, c->stream));
    HGMM_HIP(c, ctx_stream_sync(c));              // `h` is pageable host memory
    return HGMM_OK;
}

// tree_loglik_kernel takes the fields of TreeLoglikArgs one by one
template <class K>
static void ll_positional(K kernel, dim3 grid, hipStream_t stream, const TreeLoglikArgs& a, const double* exp2_tab) {
    kernel<<<grid, CH, 0, stream>>>(a.xs, a.n, a.n_pad, a.prep, a.lb, a.n_level_nodes, a.nodes_per_chunk, a.partial, a.block_q,
                                    a.ticket, a.q_out, a.done, a.stop, a.flags, a.pair_count, exp2_tab, a.w);
}

static int tree_prep(hgmm_ctx* c, int64_t jb, int64_t je) {
    tree_prep_kernel<<<nblk(je - jb, 256), 256, 0, c->stream>>>(c->t_pi.as<double>(), c->t_mu.as<double>(),
                                                               c->t_cov.as<double>(), jb, je,
                                                               c->t_prep.as<double>(), flags_ptr(c));
    HGMM_HIP(c, hipGetLastError());
    return HGMM_OK;
}

// ---- the kernel families of the build (kernel_for, hgmm_ctx.h; the last flag: WEIGHTED, hgmm_tree_set_source_weights) ----
struct EstepFamily { template <bool HALF, bool W> static auto kernel() { return tree_estep_kernel<HALF, W>; } };
// (two points per thread: `overlap` excludes the four-point form)
struct LlEstepFamily { template <bool F32, bool W> static auto kernel() { return tree_ll_estep_kernel<2, F32, W>; } };
struct LoglikF32Family { template <bool FOUR, bool W> static auto kernel() { return tree_loglik_f32_kernel<FOUR ? 4 : 2, W>; } };
// (four points per thread come with the large exp table)
struct LoglikFamily { template <bool FOUR, bool W> static auto kernel() { return tree_loglik_kernel<FOUR ? 4 : 2, FOUR, W>; } };
struct LoglikFinishFamily { template <bool FASTLOG, bool W> static auto kernel() { return tree_loglik_finish_kernel<FASTLOG, W>; } };
struct ScatterFamily { template <bool W> static auto kernel() { return tree_scatter_kernel<W>; } };

// ---- how hgmm_tree_build runs a cloud: the five modes, decided here and nowhere else -------------------------------------
struct BuildPlan { int ll_pts; bool estep_half; int batch_iters, ahead_iters; bool use_follow, overlap; };
static BuildPlan build_plan(hgmm_ctx* c) {
    BuildPlan p;
    const int64_t n = c->n;
    // points per thread in the log-likelihood kernel (N = 1e6, L = 4 build: 10.2 / 8.4 / 8.0 ms with 1 / 2 / 4)
    // (one point per thread for small clouds was tried in round 3: C4 level 0 / 1 got slower, 11.5 / 16.0 vs 9.2 / 15.4 us --
    //  these launches are chains of memory round trips, not arithmetic)
    p.ll_pts = n >= 400000 ? 4 : 2;
    // (a 64-point / node-split form of the log-likelihood for small clouds -- four waves of a workgroup sharing 64 points and
    //  splitting the nodes, no finish pass -- was built and measured in round 3 and lost at every C4 level: 16.9 / 17.7 /
    //  20.2 / 49 us per iteration against 8.9 / 14.8 / 19.1 / 22.4 for this form: eight times as many workgroups each read
    //  the level's whole node table for the reach test; removed again, commit 7d926ef)
    // the E-step's LDS transpose in two passes (half the LDS, twice the resident workgroups) once a level has more chunks
    // than the chip holds at a time
    p.estep_half = n / CH > (int64_t)3 * c->cus;
    // iterations enqueued per batch.  Round 2 (host waits at every batch boundary): 1/2/4/8/16 -> 6.8/6.3/5.6/5.1/5.3 ms @C4.
    // With the host one batch ahead (run_batches) a level that stops at iteration k still has (ceil(k / B) + 1) B - k
    // iterations enqueued behind the stop (46 over C4's four levels at B = 8, 22 at B = 4) -- but each of those is three
    // launches that return at their first load, and a batch boundary (control-word copy + event) costs more than it
    // saves: 2/4/8 -> 3.67/3.60/3.46 ms @C4, 5.12/5.07/5.02 @1M on one box.
    p.batch_iters = 8;
    // single GPU: progress word in pinned host memory, polled (follow_ahead); HGMM_TREE_AHEAD=0 -> the batch scheme
    // (C4, one box: batch scheme 3.16-3.6 ms; 1 / 2 / 3 / 4 / 6 iterations ahead: 3.39 / 2.88 / 3.0 / 2.94 / 2.97 ms -- with one
    //  the device waits for the host after every iteration; the host needs ~10 us to enqueue what the device runs in ~25)
    // (under a communicator too, round 6: every rank reads the same reduced q, so every rank's stop rule says the same and
    //  every rank's host can follow its own device's progress word)
    p.ahead_iters = c->cfg[CFG_TREE_AHEAD];
    // the stop rule inside the next launch (tree_follow) instead of a ticketed tail of the log-likelihood: needs the
    // polled scheme with >= 2 iterations ahead (the verdict on iteration e is reached by launch e + 1)
    p.use_follow = !c->comm_on() && p.ahead_iters >= 2 && !c->cfg[CFG_TREE_TICKETS];
    // small clouds: iteration e + 1's (speculative) E-step rides in iteration e's log-likelihood launch and the moments
    // kernel takes over the stop rule (tree_ll_estep_kernel); HGMM_TREE_OVERLAP=0 -> one launch each, as for large clouds
    p.overlap = p.use_follow && p.ahead_iters > 0 && !p.estep_half && p.ll_pts != 4 && c->cfg[CFG_TREE_OVERLAP];
    return p;
}

// ---- one level of the serial build: everything an iteration's launches take, and the iteration itself ------------------
// The stop rule runs on the device; the host enqueues iterations ahead of it (follow_ahead / run_batches), so launches
// overlap execution.  Kernels of iterations enqueued past the stop return immediately.  With a communicator the
// all-reduces of the enqueued iterations cannot be predicated, so they run out of place: rank-local moments / q stay where
// the (skipped) kernels left them, the reduced copies are rebuilt identically, the M-step and the stop rule read the
// copies -- surplus iterations are idempotent and no per-iteration host round trip is needed.
struct BuildLevel {
    hgmm_ctx* c;
    const BuildPlan& plan;
    const BuildWorkspace& ws;
    int l, P;                        // the level and its parent segments
    double ls, ld, n_total;
    int max_iters, trace_cap;
    unsigned long long* host_word_dev;   // the progress word of the polled scheme; NULL: the batch scheme
    // ---- set by prepare() ----
    int64_t lb, parent_first;        // the level's first node, n_level of them; the first node of the level above
    int n_level;
    unsigned grid_chunks;
    // small clouds do not have enough 256-point blocks to fill the chip: the level's nodes are split over gridDim.y of the
    // log-likelihood launch (`chunks` of per_chunk nodes) and the per-chunk sums added in a second (fixed-order) kernel
    int pblocks, llblocks;           // point blocks; the log-likelihood grid: ll_pts points per thread
    int chunks, per_chunk;
    double *ll_partial, *block_q, *q_dev, *trace_dev;
    TreeCtl* ctl;
    TreeLoopState* loop_state;       // two slots (tree_follow), right behind ctl
    int* curbuf[2];                  // (overlap: iteration e's assignment is curbuf[e & 1]; else always the same buffer)
    double *mom_g, *q_g;             // communicator: the reduced copies of the moments and of q

    // the level's chunk table, its buffers, and a fresh stop rule
    int prepare() {
        const int64_t n = c->n;
        lb = level_first(l);
        n_level = (int)(level_first(l + 1) - lb);
        parent_first = (l == 0) ? 0 : level_first(l - 1);
        tree_chunks_kernel<<<1, 1024, 0, c->stream>>>(ws.seg, P, ws.chunk_first, ws.chunk_desc, ws.n_chunks_dev);
        grid_chunks = (unsigned)(n / CH + P + 1);
        pblocks = (int)nblk(n, CH);
        llblocks = (int)nblk(n, CH * plan.ll_pts);
        tree_ll_split(llblocks, n_level, c->cus, &chunks, &per_chunk);
        ll_partial = nullptr;
        if (chunks > 1) {
            HGMM_TRY(ensure(c, c->t_llp, sizeof(double) * (size_t)chunks * c->n_pad));
            ll_partial = c->t_llp.as<double>();
        }
        block_q = c->t_q.as<double>();
        q_dev = block_q + pblocks;
        ctl = reinterpret_cast<TreeCtl*>(q_dev + 2);
        loop_state = reinterpret_cast<TreeLoopState*>(q_dev + 4);
        trace_dev = c->t_qtrace.as<double>() + (size_t)l * trace_cap;
        curbuf[0] = ws.cur[0];
        curbuf[1] = plan.overlap ? ws.cur[1] : ws.cur[0];
        // (ctl and the two loop-state slots of tree_follow behind it: 48 contiguous bytes)
        HGMM_HIP(c, hipMemsetAsync(ctl, 0, sizeof(TreeCtl) + 2 * sizeof(TreeLoopState), c->stream));
        mom_g = nullptr;
        q_g = q_dev;
        if (c->comm_on()) {
            HGMM_TRY(ensure(c, c->comm_buf, sizeof(double) * ((size_t)NMOM * n_level + 8)));
            mom_g = c->comm_buf.as<double>();
            q_g = mom_g + (size_t)NMOM * n_level;
        }
        return HGMM_OK;
    }
    // level 0 of an overlapped build: q comes out of the (next iteration's) E-step, one share per chunk (TreeEstepArgs)
    bool fused0() const { return plan.overlap && l == 0; }
    // follow mode (single GPU, polled look-ahead): launch e of the E-step adds up the shares of q that iteration e - 1
    // left behind and applies the stop rule itself (tree_follow); the log-likelihood kernels only store their shares
    TreeFollow follow_of(int e) const {
        const int q_shares = (fused0() || chunks > 1) ? pblocks : llblocks;
        return TreeFollow{block_q, q_shares, loop_state + ((e - 1) & 1), loop_state + (e & 1), &ctl->done, ls,
                          max_iters, trace_dev, trace_cap, host_word_dev};
    }
    // One EM iteration of the level, enqueued (every kernel looks at ctl->done first and returns at once when it has stopped)
    int enqueue(int e) const {
        const bool weighted = ws.w != nullptr;
        const int64_t n = c->n, n_pad = c->n_pad;
        double *d_pi = c->t_pi.as<double>(), *d_mu = c->t_mu.as<double>(), *d_cov = c->t_cov.as<double>();
        double *d_prep = c->t_prep.as<double>(), *d_mom = c->t_mom.as<double>();
        const bool overlap = plan.overlap, use_follow = plan.use_follow;
        if (!overlap || e == 0) {
            ProfScope prof(c, HGMM_K_TREE_ESTEP);
            const TreeFollow fol = (use_follow && e >= 1) ? follow_of(e) : NO_FOLLOW;
            const auto estep = kernel_for<EstepFamily>(plan.estep_half, weighted);
            estep<<<grid_chunks, CH, 0, c->stream>>>(
                ws.xs, n_pad, d_prep, ws.chunk_desc, ws.n_chunks_dev, parent_first, l, ws.partials, curbuf[e & 1], &ctl->done, fol, ws.w);
        }
        // single GPU: reduction, M-step and preparation of a node in one launch; with a communicator the all-reduce of the
        // moments sits between reduction and M-step
        // (small clouds below level 0: a wave per parent, same bits.  Level 0 is ONE parent with all of the cloud's chunks:
        //  eight waves gathering side by side are 3 us quicker than one wave taking the eight rows in turn)
        if (overlap && l > 0)
            tree_moments8_kernel<<<n_level / 8, 64, 0, c->stream>>>(ws.partials, ws.chunk_first, d_mom + NMOM * lb, lb, n_total,
                                                                    ld, d_pi, d_mu, d_cov, d_prep, flags_ptr(c), &ctl->done,
                                                                    e >= 1 ? follow_of(e) : NO_FOLLOW);
        else
            tree_moments_kernel<<<n_level, 64, 0, c->stream>>>(ws.partials, ws.chunk_first, n_level, d_mom + NMOM * lb,
                                                               c->comm_on() ? 0 : 1, lb, n_total, ld, d_pi, d_mu, d_cov,
                                                               d_prep, flags_ptr(c), &ctl->done,
                                                               (overlap && e >= 1) ? follow_of(e) : NO_FOLLOW);
        if (c->comm_on()) {
            HGMM_TRY(allreduce_f64_oop(c, d_mom + NMOM * lb, mom_g, (size_t)NMOM * n_level));
            tree_mstep_kernel<<<nblk(n_level, 256), 256, 0, c->stream>>>(mom_g, lb, n_level, n_total, ld, d_pi,
                                                                         d_mu, d_cov, d_prep, flags_ptr(c), &ctl->done, 0);
        }
        {
            ProfScope prof(c, HGMM_K_TREE_LOGLIK);
            // the last workgroup to finish adds up the per-block shares of q (store_block_q) ... and, on a single GPU, applies
            // the level's stop rule (with a communicator q is all-reduced first and tree_ctl_kernel does it)
            const TreeStop stop = (c->comm_on() || use_follow)
                                      ? NO_STOP
                                      : TreeStop{ctl, ls, max_iters, trace_dev, trace_cap, host_word_dev};
            // follow mode: plain stores of the shares  (the tickets: zeroed by tree_flags; every launch leaves them zero)
            unsigned int* q_ticket = use_follow ? nullptr : tickets_ptr(c);
            // (the positional kernels take the same list, field by field)
            TreeLoglikArgs la{ws.xs, n, n_pad, d_prep, lb, n_level, per_chunk, ll_partial, block_q, q_ticket,
                              q_dev, &ctl->done, chunks > 1 ? NO_STOP : stop, flags_ptr(c), pairs_ptr(c), nullptr,
                              0, 0, ws.w};
            const dim3 ll_grid(llblocks, chunks);
            const bool four = plan.ll_pts == 4;
            if (overlap && (e + 1 < max_iters || fused0())) {
                // (level 0: no log-likelihood workgroups at all -- the E-step stores the shares of q; behind the
                //  budget's last iteration it runs for those alone, its moments and assignment are never read)
                la.stop = NO_STOP;
                const TreeEstepArgs ea{ws.xs, n_pad, d_prep, ws.chunk_desc, ws.n_chunks_dev, parent_first, l, ws.partials,
                                       curbuf[(e + 1) & 1], &ctl->done, fused0() ? block_q : nullptr, ws.w};
                const int gx = fused0() ? 0 : llblocks, gy = fused0() ? 0 : chunks;
                const unsigned g = (unsigned)(gx * gy) + grid_chunks;
                const auto fused = kernel_for<LlEstepFamily>(c->tree.pdf_f32, weighted);
                fused<<<g, CH, 0, c->stream>>>(la, gx, gy, ea);
            } else if (c->tree.pdf_f32) {
                const auto ll = kernel_for<LoglikF32Family>(four, weighted);
                ll<<<ll_grid, CH, 0, c->stream>>>(la);
            } else {
                ll_positional(kernel_for<LoglikFamily>(four, weighted), ll_grid, c->stream, la,
                              four ? c->exp_tab2.as<double>() : nullptr);
            }
            if (chunks > 1 && !fused0()) {
                const auto finish = kernel_for<LoglikFinishFamily>(c->tree.pdf_f32, weighted);
                finish<<<pblocks, CH, 0, c->stream>>>(ll_partial, n, n_pad, chunks, block_q, q_ticket, q_dev, &ctl->done, stop, ws.w);
            }
        }
        if (c->comm_on()) {
            HGMM_TRY(allreduce_f64_oop(c, q_dev, q_g, 1));
            tree_ctl_kernel<<<1, 1, 0, c->stream>>>(q_g, ctl, ls, max_iters, trace_dev, trace_cap, host_word_dev);
        }
        // a launch the runtime rejected (LDS / grid limits of another chip) would leave the progress word untouched
        // for ever: the host loops must hear about it here
        const hipError_t le = hipGetLastError();
        if (le != hipSuccess) return fail(c, HGMM_ERR_HIP, "tree build: kernel launch failed: %s", hipGetErrorString(le));
        return HGMM_OK;
    }
    // follow mode: nobody follows the budget's last iteration -- one workgroup accounts for its q
    int close() const {
        tree_close_kernel<<<1, CH, 0, c->stream>>>(follow_of(max_iters));
        if (hipGetLastError() != hipSuccess) return fail(c, HGMM_ERR_HIP, "tree build: launch failed");
        return HGMM_OK;
    }
};

}  // namespace hgmm

using namespace hgmm;

// hgmm_tree_build (init_mu) and hgmm_tree_build_rows (init_rows: the initial means are rows of the resident cloud, gathered on
// the device into the place init_mu is uploaded to): exactly one of the two is given
static int tree_build(hgmm_ctx* c, int L, double ls, double ld, const double* init_mu, const int64_t* init_rows, bool by_rows,
                      double sig2, int max_iters_per_level, double* pi_out, double* mu_out,
                      double* cov_out, int32_t* leaf_idx_out, int32_t* iters_per_level_out,
                      double* q_trace_out, int q_capacity, int* q_len_out) {
    HGMM_ENTER(c);
    if (!c->have_f64 || c->n <= 0) return fail(c, HGMM_ERR_STATE, "tree build: set points first");
    if (L < 1 || L > 6) return fail(c, HGMM_ERR_ARG, "tree levels L = %d outside 1..6", L);
    if (by_rows ? !init_rows : !init_mu) return fail(c, HGMM_ERR_ARG, by_rows ? "init_rows is NULL" : "init_mu is NULL");
    if (by_rows)
        for (int64_t j = 0, T_ = level_first(L); j < T_; ++j)
            if (init_rows[j] < 0 || init_rows[j] >= c->n)
                return fail(c, HGMM_ERR_ARG, "tree build: init_rows[%lld] = %lld, but the resident cloud has %lld points",
                            (long long)j, (long long)init_rows[j], (long long)c->n);
    if (c->n > 0x7fffffff - 1024) return fail(c, HGMM_ERR_ARG, "too many points for 32-bit indices");
    // hgmm_tree_set_source_weights: the WEIGHTED instantiations of the level's kernels, the weights on the coordinates' ping-pong
    const double* wsrc = c->src.ptr();
    const bool weighted = wsrc != nullptr;
    if (weighted && c->comm_on())
        return fail(c, HGMM_ERR_STATE, "tree build: source weights are resident and the context has a communicator; sharded "
                    "weighted builds are not supported (hgmm_tree_set_source_weights(ctx, NULL, 0) takes the weights off)");
    if (max_iters_per_level < 1) max_iters_per_level = 1;
    HGMM_HIP(c, hipSetDevice(c->device));
    HGMM_TRY(tree_alloc_nodes(c, L));
    const BuildPlan plan = build_plan(c);
    if (plan.ll_pts == 4) HGMM_TRY(ensure_exp_tab2(c));

    const int64_t T = c->tree.T;
    const int64_t n = c->n, n_pad = c->n_pad;
    int64_t maxP = 1;
    for (int i = 0; i < L - 1; ++i) maxP *= 8;                 // parents at the last level
    BuildWorkspace ws;
    HGMM_TRY(ws.take(c, n, n_pad, maxP, L, c->x_soa64.as<double>(), wsrc));
    HGMM_TRY(ensure(c, c->scratch, sizeof(double) * 3 * T));
    HGMM_TRY(ensure(c, c->t_perm, sizeof(int) * 2 * n_pad));                 // ping-pong
    HGMM_TRY(ensure(c, c->t_q, sizeof(double) * (nblk(n, CH) + 8)));
    const int trace_cap = std::min(max_iters_per_level, 1 << 20);
    HGMM_TRY(ensure(c, c->t_qtrace, sizeof(double) * (size_t)trace_cap * L));     // one segment per level, read back at the end
    HandOver* hand = nullptr;
    HGMM_TRY(hand_over(c, 1, &hand));
    const HostDev<unsigned long long> word = hand->progress(0);       // the polled scheme's progress word
    double *d_pi = c->t_pi.as<double>(), *d_mu = c->t_mu.as<double>(), *d_cov = c->t_cov.as<double>();
    int* perm_cur = c->t_perm.as<int>();
    int* perm_next = perm_cur + n_pad;
    double* trace_base = c->t_qtrace.as<double>();

    if (by_rows) HGMM_TRY(stage_init_rows(c, init_rows, T, nullptr, 1));
    else HGMM_HIP(c, hipMemcpyAsync(c->scratch.p, init_mu, sizeof(double) * 3 * T, hipMemcpyHostToDevice, c->stream));
    tree_init_nodes_kernel<<<nblk(T, 256), 256, 0, c->stream>>>(c->scratch.as<double>(), sig2, T, d_pi, d_mu, d_cov);
    HGMM_TRY(tree_prep(c, 0, T));
    tree_iota_kernel<<<nblk(n, 256), 256, 0, c->stream>>>(perm_cur, n);
    const int seg0[2] = {0, (int)n};
    HGMM_HIP(c, hipMemcpyAsync(ws.seg, seg0, sizeof seg0, hipMemcpyHostToDevice, c->stream));
    HGMM_HIP(c, hipGetLastError());

    // global point count (pi = m0 / N_total); with weights their sum: point i counts as w_i points
    double n_total = c->src.total(n);
    if (c->comm_on()) HGMM_TRY(hgmm_comm_allreduce_f64(c, &n_total, 1, 0));

    std::vector<int> level_iters(L, 0);
    int P = 1, rc = HGMM_OK;
    for (int l = 0; l < L && rc == HGMM_OK; ++l) {
        BuildLevel lv{c, plan, ws, l, P, ls, ld, n_total, max_iters_per_level, trace_cap, plan.ahead_iters > 0 ? word.dev : nullptr};
        rc = lv.prepare();
        if (rc != HGMM_OK) break;
        const auto enqueue = [&lv](int e) { return lv.enqueue(e); };
        int it = 0;
        if (plan.ahead_iters > 0) {
            // (the word is reset here: every launch that could write it belongs to this level)
            __atomic_store_n(word.host, 0ull, __ATOMIC_RELAXED);
            int enq = 0;
            const auto close = [&lv, &plan] { return plan.use_follow ? lv.close() : HGMM_OK; };
            rc = follow_ahead(c, word.host, 1, max_iters_per_level, plan.ahead_iters, enqueue, close, &enq, "tree build");
            const unsigned long long w = __atomic_load_n(word.host, __ATOMIC_RELAXED);
            it = (int)(w & 0xffffffffull);
            // Under a communicator every rank must have enqueued the SAME collectives when it leaves the level.
            // How far a rank's host had got when it saw the stop is a matter of timing; min(it + ahead, budget)
            // is not: each rank tops its queue up to exactly that many iterations (the surplus ones return at
            // their first load, their all-reduces run out of place on unchanged operands).  Round 5 looked at
            // the stop word once per 8 iterations, one batch behind: up to 15 surplus iterations per level,
            // 46 over C4's four levels; now `ahead` (2) per level, whatever the backend.
            if (rc == HGMM_OK && c->comm_on()) {
                const int must = std::min(it + plan.ahead_iters, max_iters_per_level);
                while (rc == HGMM_OK && enq < must) rc = lv.enqueue(enq++);
                c->tree.surplus_iterations += (unsigned long long)(enq - it);
            }
        } else {
            rc = run_batches(c, lv.ctl, hand, max_iters_per_level, plan.batch_iters, enqueue, &it, "tree build");
        }
        if (rc != HGMM_OK) {
            c->err += " (level " + std::to_string(l) + ")";
            break;
        }
        level_iters[l] = it;
        int* cur = lv.curbuf[(it - 1) & 1];                    // the assignment of the last iteration that counted
        if (iters_per_level_out) iters_per_level_out[l] = it;
        if (l + 1 < L) {
            // partition for the next level
            tree_hist_kernel<<<lv.grid_chunks, CH, 0, c->stream>>>(cur, ws.chunk_desc, ws.n_chunks_dev, ws.hist);
            tree_offsets_kernel<<<P, OFF_BLOCK, 0, c->stream>>>(ws.hist, ws.chunk_first, ws.seg, P, ws.chunk_off, ws.seg_next);
            const auto scatter = kernel_for<ScatterFamily>(weighted);
            scatter<<<lv.grid_chunks, CH, 0, c->stream>>>(
                ws.xs, n_pad, perm_cur, cur, ws.chunk_desc, ws.n_chunks_dev, ws.chunk_off, ws.xs_next, perm_next, ws.w, ws.w_next);
            HGMM_HIP(c, hipGetLastError());
            ws.advance();
            std::swap(perm_cur, perm_next);
            P *= 8;
        } else if (leaf_idx_out) {
            tree_unsort_kernel<<<nblk(n, 256), 256, 0, c->stream>>>(perm_cur, cur, n, perm_next);
            if (hipMemcpyAsync(leaf_idx_out, perm_next, sizeof(int) * n, hipMemcpyDeviceToHost, c->stream) != hipSuccess)
                rc = fail(c, HGMM_ERR_HIP, "tree build: leaf index download failed");
        }
    }
    if (rc == HGMM_OK) {
        // the per-iteration M-steps skip the 'complexity' ratio (registration only): all nodes at once, now
        tree_complexity_kernel<<<nblk(T, 256), 256, 0, c->stream>>>(d_cov, 0, T, c->t_prep.as<double>());
        // The node tables and the q traces come back through the context's pinned ring: every copy is a DMA packet that
        // queues at once, ONE synchronisation, then plain memcpys.  (Copied straight into the caller's pageable arrays
        // each of the 3 + L copies blocked the host for ~20 us while the runtime staged it: 5 % of a C4 build.)  Tables
        // too large for the ring (L >= 5) are copied directly.
        StagedDownloads dl(c, STAGE_RING_BYTES);                   // (no per-array limit: at L = 4 the 337 KB covariance table is staged)
        dl.add(pi_out, d_pi, sizeof(double) * T);
        dl.add(mu_out, d_mu, sizeof(double) * 3 * T);
        dl.add(cov_out, d_cov, sizeof(double) * 9 * T);
        gather_traces(level_iters.data(), L, trace_cap, q_trace_out ? q_capacity : 0, [&](int at, int l, int take) {
            dl.add(q_trace_out + at, trace_base + (size_t)l * trace_cap, sizeof(double) * take);
        });
        const hipError_t e = dl.finish();
        if (e != hipSuccess) rc = fail(c, HGMM_ERR_HIP, "tree build: download failed: %s", hipGetErrorString(e));
    } else {
        (void)ctx_stream_sync(c);
    }
    const int q_len = std::accumulate(level_iters.begin(), level_iters.end(), 0);      // (of the levels that finished)
    if (q_len_out) *q_len_out = q_len < q_capacity ? q_len : q_capacity;
    if (rc == HGMM_OK) { c->tree.nodes_ready = true; c->tree.mu_rmax = -1.0; }
    return rc;
}

extern "C" int hgmm_tree_build(hgmm_ctx* c, int L, double ls, double ld, const double* init_mu,
                               double sig2, int max_iters_per_level, double* pi_out, double* mu_out,
                               double* cov_out, int32_t* leaf_idx_out, int32_t* iters_per_level_out,
                               double* q_trace_out, int q_capacity, int* q_len_out) {
    return tree_build(c, L, ls, ld, init_mu, nullptr, false, sig2, max_iters_per_level, pi_out, mu_out, cov_out, leaf_idx_out,
                      iters_per_level_out, q_trace_out, q_capacity, q_len_out);
}
extern "C" int hgmm_tree_build_rows(hgmm_ctx* c, int L, double ls, double ld, const int64_t* init_rows,
                                    double sig2, int max_iters_per_level, double* pi_out, double* mu_out,
                                    double* cov_out, int32_t* leaf_idx_out, int32_t* iters_per_level_out,
                                    double* q_trace_out, int q_capacity, int* q_len_out) {
    return tree_build(c, L, ls, ld, nullptr, init_rows, true, sig2, max_iters_per_level, pi_out, mu_out, cov_out, leaf_idx_out,
                      iters_per_level_out, q_trace_out, q_capacity, q_len_out);
}

extern "C" int hgmm_tree_set_precision(hgmm_ctx* c, int precision) {
    HGMM_ENTER(c);
    if (precision != HGMM_PRECISION_F64 && precision != HGMM_PRECISION_F32_PDF)
        return fail(c, HGMM_ERR_ARG, "hgmm_tree_set_precision: unknown precision %d", precision);
    c->tree.pdf_f32 = precision == HGMM_PRECISION_F32_PDF;
    return HGMM_OK;
}

extern "C" int hgmm_tree_set_reg_gate(hgmm_ctx* c, double maha2_gate) {
    HGMM_ENTER(c);
    if (!(maha2_gate > 0.0))                                      // (NaN fails the comparison too)
        return fail(c, HGMM_ERR_ARG, "hgmm_tree_set_reg_gate: the gate must be > 0 (+inf: off), got %g", maha2_gate);
    c->tree.reg_gate = maha2_gate;
    return HGMM_OK;
}
extern "C" int hgmm_tree_get_reg_gate(hgmm_ctx* c, double* maha2_gate_out) {
    HGMM_ENTER(c);
    if (!c || !maha2_gate_out) return c ? fail(c, HGMM_ERR_ARG, "maha2_gate_out is NULL") : HGMM_ERR_ARG;
    *maha2_gate_out = c->tree.reg_gate;
    return HGMM_OK;
}

extern "C" int hgmm_tree_set_nodes(hgmm_ctx* c, int L, const double* pi, const double* mu, const double* cov) {
    HGMM_ENTER(c);
    if (!c || !pi || !mu || !cov) return c ? fail(c, HGMM_ERR_ARG, "NULL node table") : HGMM_ERR_ARG;
    if (L < 1 || L > 6) return fail(c, HGMM_ERR_ARG, "tree levels L = %d outside 1..6", L);
    HGMM_HIP(c, hipSetDevice(c->device));
    HGMM_TRY(tree_alloc_nodes(c, L));
    const int64_t T = c->tree.T;
    HGMM_HIP(c, hipMemcpyAsync(c->t_pi.p, pi, sizeof(double) * T, hipMemcpyHostToDevice, c->stream));
    HGMM_HIP(c, hipMemcpyAsync(c->t_mu.p, mu, sizeof(double) * 3 * T, hipMemcpyHostToDevice, c->stream));
    HGMM_HIP(c, hipMemcpyAsync(c->t_cov.p, cov, sizeof(double) * 9 * T, hipMemcpyHostToDevice, c->stream));
    HGMM_TRY(tree_prep(c, 0, T));
    HGMM_HIP(c, ctx_stream_sync(c));
    c->tree.mu_rmax = tree_mu_rmax(mu, T);
    c->tree.nodes_ready = true;
    return HGMM_OK;
}

extern "C" int hgmm_tree_set_target(hgmm_ctx* c, const double* xyz, int64_t n) {
    HGMM_ENTER(c);
    if (!c || !xyz) return c ? fail(c, HGMM_ERR_ARG, "xyz is NULL") : HGMM_ERR_ARG;
    if (n <= 0) return fail(c, HGMM_ERR_ARG, "target must have at least one point");
    HGMM_HIP(c, hipSetDevice(c->device));
    const int64_t n_pad = (n + 255) / 256 * 256;
    target_begin(c);
    HGMM_TRY(ensure(c, c->tgt_soa64, sizeof(double) * 3 * n_pad));
    std::vector<double> soa((size_t)3 * n_pad, 0.0);
    double r2max = 0.0;                                         // largest |x|^2: bounds the extent of the moved cloud
    for (int64_t i = 0; i < n; ++i) {
        double r2 = 0.0;
        for (int d = 0; d < 3; ++d) { soa[(size_t)d * n_pad + i] = xyz[3 * i + d]; r2 += xyz[3 * i + d] * xyz[3 * i + d]; }
        if (r2 > r2max) r2max = r2;
    }
    HGMM_HIP(c, hipMemcpyAsync(c->tgt_soa64.p, soa.data(), sizeof(double) * soa.size(), hipMemcpyHostToDevice, c->stream));
    HGMM_HIP(c, ctx_stream_sync(c));
    target_publish(c, n, n_pad, r2max, nullptr);
    return HGMM_OK;
}

// per-point weights of the resident target (include/hgmm.h): tgt_w [tgt_pad] parallel to tgt_soa64
extern "C" int hgmm_tree_set_target_weights(hgmm_ctx* c, const double* w, int64_t n) {
    HGMM_ENTER(c);
    const char* what = "hgmm_tree_set_target_weights";
    if (c->tgt_n <= 0) return fail(c, HGMM_ERR_STATE, "%s: no target (call hgmm_tree_set_target first)", what);
    if (!w) { c->tgt_w.drop(); return HGMM_OK; }
    return upload_weights(c, what, "target", false, 1, &w, &n, &c->tgt_n, c->tgt_pad, c->tgt_w);
}

// per-point weights of the resident cloud (include/hgmm.h): src [n_pad] parallel to x_soa64; hgmm_tree_build alone reads them
extern "C" int hgmm_tree_set_source_weights(hgmm_ctx* c, const double* w, int64_t n) {
    HGMM_ENTER(c);
    const char* what = "hgmm_tree_set_source_weights";
    if (!c->have_f64 || c->n <= 0) return fail(c, HGMM_ERR_STATE, "%s: no cloud (set or bind points first)", what);
    if (!w) { c->src.drop(); return HGMM_OK; }
    return upload_weights(c, what, "cloud", false, 1, &w, &n, &c->n, c->n_pad, c->src);
}

// fixed-point moments of the resident target under (rot, t, scale) -> c->t_momq [T][NMQ] (all-reduced over the
// ranks as integers: still exact); *d_out / *f_out = extent and fractional bits of the encoding
template <int NMQ>
static int reg_estep_fixed(hgmm_ctx* c, MomqScope& sums, const double* rot, const double* t, double scale, double lambda_c,
                           double* d_out, int* f_out) {
    if (!c->tree.nodes_ready) return fail(c, HGMM_ERR_STATE, "registration E-step: no tree (build or set_nodes first)");
    if (c->tgt_n <= 0) return fail(c, HGMM_ERR_STATE, "registration E-step: call hgmm_tree_set_target first");
    HGMM_HIP(c, hipSetDevice(c->device));
    const int64_t T = c->tree.T;
    const Rigid tf = rigid_from(rot, t, scale);
    // extent: |s R x + t - mu| <= |s| (Frobenius bound on R) max|x| + |t| + max|mu|, rounded up to a power of two
    HGMM_TRY(tree_mu_rmax_resident(c));
    double ext = reg_extent(tf, c->tgt_rmax, c->tree.mu_rmax);
    if (c->comm_on()) {                                           // every rank must use the same encoding
        double e = ext;
        HGMM_TRY(hgmm_comm_allreduce_f64(c, &e, 1, 1));
        ext = e;
    }
    double n_all = c->tgt_w.total(c->tgt_n);                             // (weights: this rank's shard's, like its points)
    if (c->comm_on()) HGMM_TRY(hgmm_comm_allreduce_f64(c, &n_all, 1, 0));
    double D = 1.0;
    int F = 0;
    reg_encoding(ext, n_all, &D, &F);
    HGMM_TRY(sums.open(c, c->t_momq, sizeof(unsigned long long) * NMOM * T));
    unsigned long long* mq = c->t_momq.as<unsigned long long>();
    {
        ProfScope prof(c, HGMM_K_TREE_REG);
        const double gate = c->tree.reg_gate;
        const double* w = c->tgt_w.ptr();
        const auto kernel = tree_reg_estep_kernel_for<NMQ>(std::isfinite(gate), w != nullptr);
        kernel<<<nblk(c->tgt_n, CH), CH, 0, c->stream>>>(c->tgt_soa64.as<double>(), c->tgt_n, c->tgt_pad, tf,
                                                         c->t_prep.as<double>(), c->tree.L, lambda_c, 1.0 / D,
                                                         std::ldexp(1.0, F), mq, gate, w);
    }
    HGMM_HIP(c, hipGetLastError());
    if (c->comm_on()) HGMM_TRY(allreduce_i64_dev(c, reinterpret_cast<long long*>(mq), (size_t)NMQ * T));
    *d_out = D;
    *f_out = F;
    return HGMM_OK;
}

extern "C" int hgmm_tree_reg_estep(hgmm_ctx* c, const double* rot, const double* t, double scale,
                                   double lambda_c, double* m0_out, double* m1_out, double* m2_out) {
    HGMM_ENTER(c);
    double D = 1.0;
    int F = 0;
    MomqScope sums(c->tree.momq_clean);                    // (no consumer: the [T][10] sums stay behind)
    HGMM_TRY(reg_estep_fixed<NMOM>(c, sums, rot, t, scale, lambda_c, &D, &F));
    const int64_t T = c->tree.T;
    double* cm = c->t_mom.as<double>();
    tree_reg_unpack_kernel<NMOM><<<nblk(T * NMOM, 256), 256, 0, c->stream>>>(c->t_momq.as<unsigned long long>(), T, D,
                                                                            std::ldexp(1.0, -F), cm);
    HGMM_TRY(ensure(c, c->scratch, sizeof(double) * 13 * T));
    double* e0 = c->scratch.as<double>();
    double* e1 = e0 + T;
    double* e2 = e1 + 3 * T;
    tree_reg_expand_kernel<<<nblk(T, 256), 256, 0, c->stream>>>(cm, c->t_prep.as<double>(), T, e0, e1, e2);
    HGMM_HIP(c, hipGetLastError());
    StagedDownloads dl(c);                                 // (three pageable copies were 90 us around 17 us of kernels)
    dl.add(m0_out, e0, sizeof(double) * T);
    dl.add(m1_out, e1, sizeof(double) * 3 * T);
    dl.add(m2_out, e2, sizeof(double) * 9 * T);
    HGMM_HIP(c, dl.finish());
    return HGMM_OK;
}

extern "C" int hgmm_tree_reg_normal(hgmm_ctx* c, const double* rot, const double* t, double scale,
                                    double lambda_c, double* out28) {
    HGMM_ENTER(c);
    if (!c || !out28) return c ? fail(c, HGMM_ERR_ARG, "out28 is NULL") : HGMM_ERR_ARG;
    double D = 1.0;
    int F = 0;
    MomqScope sums(c->tree.momq_clean);
    HGMM_TRY(reg_estep_fixed<4>(c, sums, rot, t, scale, lambda_c, &D, &F));
    const int64_t T = c->tree.T;
    HGMM_TRY(ensure(c, c->scratch, sizeof(double) * 32));
    // The 28 numbers come back through coherent pinned memory: the kernel stores them there and then a sequence
    // number the host polls (a D2H copy packet + a stream synchronisation cost ~20 us of every ~60 us iteration).
    HandOver* hand = nullptr;
    HGMM_TRY(hand_over(c, 1, &hand));
    const HostDev<unsigned long long> seq_word = hand->sequence(0);
    const HostDev<double> out = hand->out28(0);
    const unsigned long long seq = ++hand->seq;
    tree_reg_normal_kernel<<<1, 256, 0, c->stream>>>(c->t_momq.as<unsigned long long>(), D, std::ldexp(1.0, -F),
                                                    c->t_prep.as<double>(), T, c->scratch.as<double>(), out.dev, seq_word.dev, seq);
    HGMM_HIP(c, hipGetLastError());
    unsigned spins = 0;
    for (unsigned long long w; (w = __atomic_load_n(seq_word.host, __ATOMIC_ACQUIRE)) != seq;)
        HGMM_TRY(device_watch(c, &spins, seq_word.host, 1, w, "registration: the normal-equation kernel (sequence %llu)", seq));
    sums.consumed();                                              // the kernel has run: it zeroed the [T][4] words it consumed
    std::memcpy(out28, out.host, sizeof(double) * 28);
    return HGMM_OK;
}

extern "C" int hgmm_tree_register(hgmm_ctx* c, double* rot, double* t, double scale, double lambda_c, int max_iter,
                                  double tol, double* q_prev_inout, int* iters_out, int* status_out,
                                  double* trace /*[max_iter][13] or NULL*/) {
    HGMM_ENTER(c);
    if (!c || !rot || !t || !q_prev_inout || !iters_out || !status_out)
        return c ? fail(c, HGMM_ERR_ARG, "tree_register: NULL argument") : HGMM_ERR_ARG;
    *iters_out = 0;
    *status_out = 0;                                  // 0: iteration budget used up, 1: |dq| < tol, 2: host M-step needed
    if (c->cfg[CFG_REG_DEVICE_SOLVE] && !c->comm_on()) {
        // the loop on the device alone (register_set: one start pose of this context's pair, on the serial call's buffers)
        if (!c->tree.nodes_ready) return fail(c, HGMM_ERR_STATE, "registration: no tree (build or set_nodes first)");
        if (c->tgt_n <= 0) return fail(c, HGMM_ERR_STATE, "registration: call hgmm_tree_set_target first");
        HGMM_TRY(tree_mu_rmax_resident(c));
        int32_t it32 = 0, st32 = 0;
        HGMM_TRY(register_set(c, reg_set_pair(c, 1, false), rot, t, scale, lambda_c, max_iter, tol, q_prev_inout, &it32, &st32,
                              trace));
        *iters_out = it32;
        *status_out = st32;
        return HGMM_OK;
    }
    for (int it = 0; it < max_iter; ++it) {
        double o[28];
        HGMM_TRY(hgmm_tree_reg_normal(c, rot, t, scale, lambda_c, o));
        double q = 0.0;
        // too ill-conditioned for normal equations: the caller takes the reference's stacked least-squares M-step
        const int st = reg_host_step(o, rot, t, q_prev_inout, tol, &q);
        if (st == 2) { *status_out = 2; return HGMM_OK; }
        if (trace) {
            double* tr = trace + (size_t)13 * it;
            for (int i = 0; i < 9; ++i) tr[i] = rot[i];
            for (int i = 0; i < 3; ++i) tr[9 + i] = t[i];
            tr[12] = q;
        }
        *iters_out = it + 1;
        if (st == 1) { *status_out = 1; return HGMM_OK; }
    }
    return HGMM_OK;
}

// Score of the resident target, moved by (rot, t, scale), against the resident tree: include/hgmm.h.  The descent is the
// registration E-step's (gmmTreeRegESTep, hgmm_cupy_cpu_working.py:202-228); the score has no counterpart in the reference.
extern "C" int hgmm_tree_score(hgmm_ctx* c, const double* rot, const double* t, double scale, double lambda_c,
                               double maha2_max, int32_t* node_out, double* maha2_out, double* logp_out,
                               double* summary_out) {
    HGMM_ENTER(c);
    if (!summary_out) return fail(c, HGMM_ERR_ARG, "tree_score: summary_out is NULL");
    if (maha2_max != maha2_max) return fail(c, HGMM_ERR_ARG, "tree_score: maha2_max is NaN");
    if (c->comm_on()) return fail(c, HGMM_ERR_STATE, "tree_score: sharded targets are not scored (no communicator)");
    if (!c->tree.nodes_ready) return fail(c, HGMM_ERR_STATE, "tree_score: no tree (build or set_nodes first)");
    if (c->tgt_n <= 0) return fail(c, HGMM_ERR_STATE, "tree_score: call hgmm_tree_set_target first");
    const Rigid tf = rigid_from(rot, t, scale);
    const int64_t n = c->tgt_n, n_pad = c->tgt_pad;
    const unsigned nb = nblk(n, CH);
    // scratch: [nb][6] shares | summary[8] | maha2[n_pad] | logp[n_pad] | node[n_pad]  (each array only when asked for)
    const size_t head = (size_t)SCORE_NSUM * nb + 8;
    HGMM_TRY(ensure(c, c->scratch, sizeof(double) * (head + (maha2_out ? n_pad : 0) + (logp_out ? n_pad : 0)) +
                                       sizeof(int32_t) * (node_out ? n_pad : 0)));
    double* partial = c->scratch.as<double>();
    double* d_sum = partial + (size_t)SCORE_NSUM * nb;
    double* at = d_sum + 8;
    double* d_maha = nullptr;
    double* d_logp = nullptr;
    if (maha2_out) { d_maha = at; at += n_pad; }
    if (logp_out) { d_logp = at; at += n_pad; }
    int32_t* d_node = node_out ? reinterpret_cast<int32_t*>(at) : nullptr;
    {
        ProfScope prof(c, HGMM_K_TREE_SCORE);
        const double* w = c->tgt_w.ptr();
        const auto kernel = w ? tree_score_kernel<true> : tree_score_kernel<false>;
        kernel<<<nb, CH, 0, c->stream>>>(c->tgt_soa64.as<double>(), n, n_pad, tf, c->t_prep.as<double>(), c->tree.L, lambda_c,
                                         maha2_max, d_node, d_maha, d_logp, partial, w);
    }
    tree_score_finish_kernel<<<1, CH, 0, c->stream>>>(partial, (int)nb, c->tgt_w.total(n), d_sum);
    HGMM_HIP(c, hipGetLastError());
    StagedDownloads dl(c);
    dl.add(summary_out, d_sum, sizeof(double) * 8);
    dl.add(node_out, d_node, sizeof(int32_t) * n);
    dl.add(maha2_out, d_maha, sizeof(double) * n);
    dl.add(logp_out, d_logp, sizeof(double) * n);
    HGMM_HIP(c, dl.finish());
    return HGMM_OK;
}

extern "C" int hgmm_tree_node_complexity(hgmm_ctx* c, double* cplx_out) {
    HGMM_ENTER(c);
    if (!c || !cplx_out) return c ? fail(c, HGMM_ERR_ARG, "cplx_out is NULL") : HGMM_ERR_ARG;
    if (!c->tree.nodes_ready) return fail(c, HGMM_ERR_STATE, "no tree");
    const int64_t T = c->tree.T;
    HGMM_TRY(ensure(c, c->t_cplx, sizeof(double) * T));
    tree_copy_cplx_kernel<<<nblk(T, 256), 256, 0, c->stream>>>(c->t_prep.as<double>(), T, c->t_cplx.as<double>());
    HGMM_HIP(c, hipGetLastError());
    HGMM_HIP(c, hipMemcpyAsync(cplx_out, c->t_cplx.p, sizeof(double) * T, hipMemcpyDeviceToHost, c->stream));
    HGMM_HIP(c, ctx_stream_sync(c));
    return HGMM_OK;
}

// ==========================================================================================
// Stand-alone tree steps with the reference's function granularity (the pieces buildGMMTree is
// made of, callable one at a time):
//   hgmm_tree_estep   <- gmmTreeEStep()        hgmm_cupy_cpu_working.py:162-191 (arbitrary parentIdx)
//   hgmm_tree_mstep   <- gmmTreeMStep()        hgmm_cupy_cpu_working.py:193-198 (+ mlEstimator 109-119)
//   hgmm_tree_loglik  <- logLikelihoodValue()  hgmm_cupy_cpu_working.py:72-85
// The E-step here takes ANY parent assignment (no partition state), so lanes gather their own
// parent's children; lanes of a wave that share a parent are combined (leader rounds) before the
// float64 HBM atomics.  hgmm_tree_build uses the partitioned, atomic-free kernels instead.
// ==========================================================================================
namespace hgmm {

__global__ __launch_bounds__(CH) void tree_estep_generic_kernel(const double* __restrict__ xs, int64_t n,
                                                                int64_t n_pad, const double* __restrict__ prep,
                                                                const int* __restrict__ parent, int64_t T,
                                                                double inv_d, double fix_scale,
                                                                unsigned long long* __restrict__ momq,
                                                                int* __restrict__ cur) {
    // Fixed-point moment sums about each child's mean, as in tree_reg_estep_kernel: deterministic for any parent
    // assignment.  This entry point feeds an M-step directly (mu = m1 / m0 also for nodes of mass 1e-4), so every
    // contribution is carried in TWO words: hi = round(v 2^F), lo = round((v 2^F - hi) 2^32) -- resolution
    // 2^-(F+32) of the extent, far below float64 round-off of the sums themselves.  momq = [T][NMOM][2].
    // Nodes of the first two levels are summed in LDS and flushed once per workgroup.
    constexpr int LDS_NODES = 72;
    constexpr int NW = 2 * NMOM;
    __shared__ unsigned long long tab[LDS_NODES * NW];
    const int lds_nodes = (int)(T < LDS_NODES ? T : LDS_NODES);
    for (int e = threadIdx.x; e < lds_nodes * NW; e += CH) tab[e] = 0ull;
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * CH + threadIdx.x;
    const bool active = i < n;
    double x0 = 0.0, x1 = 0.0, x2 = 0.0;
    int64_t j0 = 0;
    if (active) {
        x0 = xs[i]; x1 = xs[n_pad + i]; x2 = xs[2 * n_pad + i];
        j0 = 8 * ((int64_t)parent[i] + 1);
    }
    const bool valid = active && j0 >= 0 && j0 + 8 <= T;
    double g[8];
    double den = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        g[k] = 0.0;
        if (valid) {
            const double* pr = prep + PREP_N * (j0 + k);
            const double wE = pr[9];
            if (wE != 0.0) {
                const double d0 = x0 - pr[6], d1 = x1 - pr[7], d2 = x2 - pr[8];
                const double q = sym3_quad(pr[0], pr[1], pr[2], pr[3], pr[4], pr[5], d0, d1, d2);
                g[k] = wE * exp(-0.5 * q);
            }
        }
        den += g[k];
    }
    const bool good = den > TREE_EPS;
    int am = 0;
    double best = -1.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        g[k] = good ? g[k] / den : 0.0;
        if (g[k] > best) { best = g[k]; am = k; }
        if (g[k] < TREE_EPS) g[k] = 0.0;
    }
    if (valid) cur[i] = (int)(j0 + am);
    if (valid) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (g[k] == 0.0) continue;
            const int64_t node = j0 + k;
            const double* pr = prep + PREP_N * node;
            const double u0 = (x0 - pr[6]) * inv_d, u1 = (x1 - pr[7]) * inv_d, u2 = (x2 - pr[8]) * inv_d;
            const double gq = g[k] * fix_scale;
            const double v[NMOM] = {gq, gq * u0, gq * u1, gq * u2, gq * u0 * u0, gq * u0 * u1, gq * u0 * u2,
                                    gq * u1 * u1, gq * u1 * u2, gq * u2 * u2};
            // (two typed paths instead of one pointer that may name LDS or HBM: the latter compiles to flat-address
            //  atomics, 320 of them per lane; these are ds_add_u64 resp. global_atomic_add_x2)
            if (node < lds_nodes) {
                unsigned long long* dst = tab + NW * node;
#pragma unroll
                for (int m = 0; m < NMOM; ++m) {
                    const long long hi = __double2ll_rn(v[m]);
                    const long long lo = __double2ll_rn((v[m] - (double)hi) * 4294967296.0);     // exact remainder x 2^32
                    atomicAdd(dst + 2 * m, (unsigned long long)hi);
                    atomicAdd(dst + 2 * m + 1, (unsigned long long)lo);
                }
            } else {
                unsigned long long* dst = momq + NW * node;
#pragma unroll
                for (int m = 0; m < NMOM; ++m) {
                    const long long hi = __double2ll_rn(v[m]);
                    const long long lo = __double2ll_rn((v[m] - (double)hi) * 4294967296.0);
                    atomicAdd(dst + 2 * m, (unsigned long long)hi);
                    atomicAdd(dst + 2 * m + 1, (unsigned long long)lo);
                }
            }
        }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < lds_nodes * NW; e += CH) {
        const unsigned long long v = tab[e];
        if (v != 0ull) atomicAdd(momq + e, v);
    }
}

// two-word fixed point -> float64, still centred (cm[T][NMOM])
__global__ void tree_unpack2_kernel(const unsigned long long* __restrict__ momq, int64_t T, double d,
                                    double inv_scale, double* __restrict__ cm) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= T * NMOM) return;
    const int m = (int)(e % NMOM);
    const double unit = (m == 0) ? inv_scale : (m < 4 ? d * inv_scale : d * d * inv_scale);
    const double hi = (double)(long long)momq[2 * e], lo = (double)(long long)momq[2 * e + 1];
    cm[e] = (hi + lo * (1.0 / 4294967296.0)) * unit;
}

// largest |x|^2 over the resident cloud (bit pattern of a non-negative double is order-preserving as uint64)
__global__ void tree_rmax_kernel(const double* __restrict__ xs, int64_t n, int64_t n_pad, unsigned long long* out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    double r2 = 0.0;
    if (i < n) r2 = xs[i] * xs[i] + xs[n_pad + i] * xs[n_pad + i] + xs[2 * n_pad + i] * xs[2 * n_pad + i];
    r2 = wave_max_f64(r2);
    if (lane_id() == 0 && r2 > 0.0) atomicMax(out, (unsigned long long)__double_as_longlong(r2));
}

__global__ void tree_compact_moments_kernel(const double* __restrict__ m0, const double* __restrict__ m1,
                                            const double* __restrict__ m2, int64_t T, double* __restrict__ mom) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= T) return;
    double* m = mom + NMOM * j;
    m[0] = m0[j];
    m[1] = m1[3 * j]; m[2] = m1[3 * j + 1]; m[3] = m1[3 * j + 2];
    const double* s = m2 + 9 * j;
    m[4] = s[0]; m[5] = s[1]; m[6] = s[2]; m[7] = s[4]; m[8] = s[5]; m[9] = s[8];
}

}  // namespace hgmm

static int tree_upload_nodes(hgmm_ctx* c, int64_t T, const double* pi, const double* mu, const double* cov) {
    HGMM_TRY(tree_alloc_tables(c, T));
    HGMM_HIP(c, hipMemcpyAsync(c->t_pi.p, pi, sizeof(double) * T, hipMemcpyHostToDevice, c->stream));
    HGMM_HIP(c, hipMemcpyAsync(c->t_mu.p, mu, sizeof(double) * 3 * T, hipMemcpyHostToDevice, c->stream));
    HGMM_HIP(c, hipMemcpyAsync(c->t_cov.p, cov, sizeof(double) * 9 * T, hipMemcpyHostToDevice, c->stream));
    tree_prep_kernel<<<nblk(T, 256), 256, 0, c->stream>>>(c->t_pi.as<double>(), c->t_mu.as<double>(),
                                                         c->t_cov.as<double>(), 0, T, c->t_prep.as<double>(), flags_ptr(c));
    HGMM_HIP(c, hipGetLastError());
    c->tree.nodes_ready = false;       // tables no longer describe a complete L-level tree
    return HGMM_OK;
}

extern "C" int hgmm_tree_estep(hgmm_ctx* c, int64_t T, const double* pi, const double* mu, const double* cov,
                               const int32_t* parent_idx, double* m0_out, double* m1_out, double* m2_out,
                               int32_t* current_idx_out) {
    HGMM_ENTER(c);
    if (!c || !pi || !mu || !cov || !parent_idx) return c ? fail(c, HGMM_ERR_ARG, "NULL argument") : HGMM_ERR_ARG;
    if (!c->have_f64 || c->n <= 0) return fail(c, HGMM_ERR_STATE, "tree E-step: set points first");
    if (T < 8) return fail(c, HGMM_ERR_ARG, "node table must hold at least 8 nodes");
    HGMM_HIP(c, hipSetDevice(c->device));
    HGMM_TRY(tree_upload_nodes(c, T, pi, mu, cov));
    HGMM_TRY(ensure(c, c->t_current, sizeof(int) * 2 * c->n_pad));
    int* par = c->t_current.as<int>();
    int* cur = par + c->n_pad;
    HGMM_HIP(c, hipMemcpyAsync(par, parent_idx, sizeof(int) * c->n, hipMemcpyHostToDevice, c->stream));
    HGMM_HIP(c, hipMemsetAsync(cur, 0, sizeof(int) * c->n, c->stream));
    // extent of the fixed-point encoding: max |x| (device reduction) + max |mu| (host), a power of two
    MomqScope sums(c->tree.momq_clean);                    // (no consumer that clears: the sums stay behind)
    HGMM_TRY(sums.open(c, c->t_momq, sizeof(unsigned long long) * (2 * NMOM * T + 1)));
    unsigned long long* mq = c->t_momq.as<unsigned long long>();
    tree_rmax_kernel<<<nblk(c->n, 256), 256, 0, c->stream>>>(c->x_soa64.as<double>(), c->n, c->n_pad, mq + 2 * NMOM * T);
    unsigned long long r2bits = 0;
    HGMM_HIP(c, hipMemcpyAsync(&r2bits, mq + 2 * NMOM * T, sizeof r2bits, hipMemcpyDeviceToHost, c->stream));
    HGMM_HIP(c, ctx_stream_sync(c));
    double r2 = 0.0;
    memcpy(&r2, &r2bits, sizeof r2);
    double ext = std::sqrt(r2) + tree_mu_rmax(mu, T);
    double n_all = (double)c->n;
    if (c->comm_on()) {
        HGMM_TRY(hgmm_comm_allreduce_f64(c, &ext, 1, 1));
        HGMM_TRY(hgmm_comm_allreduce_f64(c, &n_all, 1, 0));
    }
    double D = 1.0;
    int F = 0;
    reg_encoding(ext, n_all, &D, &F);
    {
        ProfScope prof(c, HGMM_K_TREE_ESTEP);
        tree_estep_generic_kernel<<<nblk(c->n, CH), CH, 0, c->stream>>>(c->x_soa64.as<double>(), c->n, c->n_pad,
                                                                       c->t_prep.as<double>(), par, T, 1.0 / D,
                                                                       std::ldexp(1.0, F), mq, cur);
    }
    HGMM_HIP(c, hipGetLastError());
    if (c->comm_on()) HGMM_TRY(allreduce_i64_dev(c, reinterpret_cast<long long*>(mq), (size_t)2 * NMOM * T));
    double* mom = c->t_mom.as<double>();
    tree_unpack2_kernel<<<nblk(T * NMOM, 256), 256, 0, c->stream>>>(mq, T, D, std::ldexp(1.0, -F), mom);
    HGMM_TRY(ensure(c, c->scratch, sizeof(double) * 13 * T));
    double* e0 = c->scratch.as<double>();
    double* e1 = e0 + T;
    double* e2 = e1 + 3 * T;
    tree_reg_expand_kernel<<<nblk(T, 256), 256, 0, c->stream>>>(mom, c->t_prep.as<double>(), T, e0, e1, e2);
    HGMM_HIP(c, hipGetLastError());
    StagedDownloads dl(c);
    dl.add(m0_out, e0, sizeof(double) * T);
    dl.add(m1_out, e1, sizeof(double) * 3 * T);
    dl.add(m2_out, e2, sizeof(double) * 9 * T);
    dl.add(current_idx_out, cur, sizeof(int) * c->n);
    HGMM_HIP(c, dl.finish());
    return HGMM_OK;
}

extern "C" int hgmm_tree_mstep(hgmm_ctx* c, int64_t T, const double* m0, const double* m1, const double* m2,
                               int64_t j_begin, int64_t j_end, double n_points, double ld, double* pi_inout,
                               double* mu_inout, double* cov_inout) {
    HGMM_ENTER(c);
    if (!c || !m0 || !m1 || !m2 || !pi_inout || !mu_inout || !cov_inout)
        return c ? fail(c, HGMM_ERR_ARG, "NULL argument") : HGMM_ERR_ARG;
    if (j_begin < 0 || j_end > T || j_begin >= j_end) return fail(c, HGMM_ERR_ARG, "bad node range");
    HGMM_HIP(c, hipSetDevice(c->device));
    HGMM_TRY(tree_upload_nodes(c, T, pi_inout, mu_inout, cov_inout));
    HGMM_TRY(ensure(c, c->scratch, sizeof(double) * 13 * T));
    double* e0 = c->scratch.as<double>();
    double* e1 = e0 + T;
    double* e2 = e1 + 3 * T;
    HGMM_HIP(c, hipMemcpyAsync(e0, m0, sizeof(double) * T, hipMemcpyHostToDevice, c->stream));
    HGMM_HIP(c, hipMemcpyAsync(e1, m1, sizeof(double) * 3 * T, hipMemcpyHostToDevice, c->stream));
    HGMM_HIP(c, hipMemcpyAsync(e2, m2, sizeof(double) * 9 * T, hipMemcpyHostToDevice, c->stream));
    double* mom = c->t_mom.as<double>();
    tree_compact_moments_kernel<<<nblk(T, 256), 256, 0, c->stream>>>(e0, e1, e2, T, mom);
    const int n_level = (int)(j_end - j_begin);
    tree_mstep_kernel<<<nblk(n_level, 256), 256, 0, c->stream>>>(mom + NMOM * j_begin, j_begin, n_level, n_points, ld,
                                                                 c->t_pi.as<double>(), c->t_mu.as<double>(),
                                                                 c->t_cov.as<double>(), nullptr, nullptr);
    HGMM_HIP(c, hipGetLastError());
    StagedDownloads dl(c);
    dl.add(pi_inout, c->t_pi.p, sizeof(double) * T);
    dl.add(mu_inout, c->t_mu.p, sizeof(double) * 3 * T);
    dl.add(cov_inout, c->t_cov.p, sizeof(double) * 9 * T);
    HGMM_HIP(c, dl.finish());
    return HGMM_OK;
}

extern "C" int hgmm_tree_loglik(hgmm_ctx* c, int64_t T, const double* pi, const double* mu, const double* cov,
                                int64_t j_begin, int64_t j_end, double* q_out) {
    HGMM_ENTER(c);
    if (!c || !pi || !mu || !cov || !q_out) return c ? fail(c, HGMM_ERR_ARG, "NULL argument") : HGMM_ERR_ARG;
    if (!c->have_f64 || c->n <= 0) return fail(c, HGMM_ERR_STATE, "tree log-likelihood: set points first");
    if (j_begin < 0 || j_end > T || j_begin >= j_end) return fail(c, HGMM_ERR_ARG, "bad node range");
    HGMM_HIP(c, hipSetDevice(c->device));
    HGMM_TRY(tree_upload_nodes(c, T, pi, mu, cov));
    const int pblocks = (int)nblk(c->n, CH);
    HGMM_TRY(ensure(c, c->t_q, sizeof(double) * (pblocks + 8)));
    double* block_q = c->t_q.as<double>();
    double* q_dev = block_q + pblocks;
    const int n_level = (int)(j_end - j_begin);
    {
        ProfScope prof(c, HGMM_K_TREE_LOGLIK);
        tree_loglik_kernel<1><<<dim3(pblocks, 1), CH, 0, c->stream>>>(c->x_soa64.as<double>(), c->n, c->n_pad,
                                                                  c->t_prep.as<double>(), j_begin, n_level,
                                                                  (n_level + LL_TILE - 1) / LL_TILE * LL_TILE, nullptr,
                                                                  block_q, nullptr, nullptr, nullptr,
                                                                  NO_STOP, flags_ptr(c), nullptr);
    }
    tree_sum_kernel<<<1, 256, 0, c->stream>>>(block_q, pblocks, q_dev);
    HGMM_HIP(c, hipGetLastError());
    if (c->comm_on()) HGMM_TRY(allreduce_f64_dev(c, q_dev, 1));
    HGMM_HIP(c, hipMemcpyAsync(q_out, q_dev, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HGMM_HIP(c, ctx_stream_sync(c));
    return HGMM_OK;
}

extern "C" int hgmm_tree_stats(hgmm_ctx* c, unsigned long long* pairs_out, int* flags_out) {
    HGMM_ENTER(c);
    HGMM_HIP(c, hipSetDevice(c->device));
    HGMM_TRY(tree_flags(c, false));
    unsigned char h[64];
    HGMM_HIP(c, hipMemcpyAsync(h, c->t_flags.p, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HGMM_HIP(c, ctx_stream_sync(c));
    if (flags_out) memcpy(flags_out, h, sizeof(int));
    if (pairs_out) memcpy(pairs_out, h + 16, sizeof(unsigned long long));
    return HGMM_OK;
}
