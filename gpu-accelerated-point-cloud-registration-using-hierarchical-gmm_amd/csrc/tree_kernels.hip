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
#include "tree_device.h"

#include <algorithm>
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

template <bool HALF>
__global__ __launch_bounds__(CH) void tree_estep_kernel(
    const double* __restrict__ xs, int64_t n_pad, const double* __restrict__ prep,
    const int* __restrict__ chunk_desc, const int* __restrict__ n_chunks, int64_t parent_level_first,
    int level, double* __restrict__ partials, int* __restrict__ cur_sorted, const int* __restrict__ done,
    TreeFollow follow = TreeFollow{nullptr, 0, nullptr, nullptr, nullptr, 0.0, 0, nullptr, 0, nullptr}) {
    __shared__ double smem[tree_estep_lds<HALF>()];
    tree_estep_body<HALF>((int)blockIdx.x,
                          TreeEstepArgs{xs, n_pad, prep, chunk_desc, n_chunks, parent_level_first, level, partials, cur_sorted, done},
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
                                                          TreeFollow follow = TreeFollow{nullptr, 0, nullptr, nullptr, nullptr, 0.0,
                                                                                         0, nullptr, 0, nullptr}) {
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

template <int PTS, bool BIGTAB = false>
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
                                                         const double* __restrict__ exp2_tab = nullptr) {
    __shared__ double smem[tree_loglik_lds<BIGTAB>()];
    tree_loglik_body<PTS, BIGTAB>((int)blockIdx.x, (int)blockIdx.y, (int)gridDim.x, (int)gridDim.y,
                                  TreeLoglikArgs{xs, n, n_pad, prep, lb, n_level_nodes, nodes_per_chunk, partial, block_q, ticket,
                                                 q_out, done, stop, flags, pair_count, exp2_tab}, smem);
}

// (tree_loglik_f32_body, csrc/tree_device.h: the level log-likelihood with the pdfs in FLOAT32)
template <int PTS>
__global__ __launch_bounds__(CH) void tree_loglik_f32_kernel(TreeLoglikArgs a) {
    __shared__ __attribute__((aligned(16))) double smem[tree_loglik_f32_lds()];
    tree_loglik_f32_body<PTS, false>((int)blockIdx.x, (int)blockIdx.y, (int)gridDim.x, (int)gridDim.y, a, smem);
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
template <int PTS, bool F32 = false>
__global__ __launch_bounds__(CH) void tree_ll_estep_kernel(TreeLoglikArgs la, int gx, int gy, TreeEstepArgs ea) {
    // (one LDS block for whichever of the two a workgroup turns out to be; the E-step in its two-pass form -- the same
    //  sums bit for bit -- so that both need ~23 KB and the launch's workgroups are all resident at once)
    constexpr int LL_LDS = F32 ? tree_loglik_f32_lds() : tree_loglik_lds<false>();
    constexpr int LDS = LL_LDS > tree_estep_lds<true>() ? LL_LDS : tree_estep_lds<true>();
    __shared__ __attribute__((aligned(16))) double smem[LDS];
    const int nll = gx * gy;
    const int b = (int)blockIdx.x;
    if (b < nll) {
        if constexpr (F32) tree_loglik_f32_body<PTS, false>(b % gx, b / gx, gx, gy, la, smem);
        else tree_loglik_body<PTS, false>(b % gx, b / gx, gx, gy, la, smem);
    } else
        tree_estep_body<true>(b - nll, ea, TreeFollow{nullptr, 0, nullptr, nullptr, nullptr, 0.0, 0, nullptr, 0, nullptr}, smem);
}


// FASTLOG: the float32-pdf mode's logarithm (log_pos_f64, as in tree_loglik_f32_body's own finish for forests)
template <bool FASTLOG = false>
__global__ __launch_bounds__(CH) void tree_loglik_finish_kernel(const double* __restrict__ partial, int64_t n,
                                                                int64_t n_pad, int n_chunks,
                                                                double* __restrict__ block_q,
                                                                unsigned int* __restrict__ ticket,
                                                                double* __restrict__ q_out,
                                                                const int* __restrict__ done, TreeStop stop) {
    if (done && *done) return;
    __shared__ double shq[CH / 64];
    const int64_t i = (int64_t)blockIdx.x * CH + threadIdx.x;
    double lq = 0.0;
    if (i < n) {
        double tot = 0.0;
        for (int c = 0; c < n_chunks; ++c) tot += partial[(size_t)c * n_pad + i];
        lq = FASTLOG ? log_pos_f64(fmax(tot, TREE_EPS)) : log(fmax(tot, TREE_EPS));
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
                                                       TreeStop stop = TreeStop{nullptr, 0.0, 0, nullptr, 0}) {
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
    const int i = begin + (int)threadIdx.x;
    const int key = (i < end) ? (cur_sorted[i] & 7) : -1;
    __shared__ int sh[CH / 64][8];
    const int w = wave_in_block();
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const unsigned long long m = __ballot(key == k);
        if (lane_id() == 0) sh[w][k] = __popcll(m);
    }
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
__global__ __launch_bounds__(CH) void tree_scatter_kernel(
    const double* __restrict__ xs, int64_t n_pad, const int* __restrict__ perm,
    const int* __restrict__ cur_sorted, const int* __restrict__ chunk_desc,
    const int* __restrict__ n_chunks, const int* __restrict__ chunk_off, double* __restrict__ xs_new,
    int* __restrict__ perm_new) {
    const int c = blockIdx.x;
    if (c >= *n_chunks) return;
    const int begin = chunk_desc[3 * c + 1], end = chunk_desc[3 * c + 2];
    const int i = begin + (int)threadIdx.x;
    const bool active = i < end;
    const int key = active ? (cur_sorted[i] & 7) : -1;
    __shared__ int sh[CH / 64][8];
    const int w = wave_in_block(), lane = lane_id();
    int rank_in_wave = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const unsigned long long m = __ballot(key == k);
        if (key == k) rank_in_wave = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) sh[w][k] = __popcll(m);
    }
    __syncthreads();
    if (!active) return;
    int before = 0;
    for (int ww = 0; ww < w; ++ww) before += sh[ww][key];
    const int dst = chunk_off[c * 8 + key] + before + rank_in_wave;
    xs_new[dst] = xs[i];
    xs_new[n_pad + dst] = xs[n_pad + i];
    xs_new[2 * n_pad + dst] = xs[2 * n_pad + i];
    perm_new[dst] = perm[i];
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


template <int NMQ>
__global__ __launch_bounds__(CH) void tree_reg_estep_kernel(const double* __restrict__ tg, int64_t n,
                                                            int64_t n_pad, Rigid tf,
                                                            const double* __restrict__ prep, int L,
                                                            double lambda_c, double inv_d, double fix_scale,
                                                            unsigned long long* __restrict__ momq) {
    __shared__ unsigned long long tab[REG_LDS_NODES * NMQ];
    const int64_t i = (int64_t)blockIdx.x * CH + threadIdx.x;
    tree_reg_estep_body<NMQ>(i, i < n, tg, n_pad, tf, prep, L, lambda_c, inv_d, fix_scale, momq, tab);
}

// score of the resident target against the resident tree (tree_score_body, csrc/tree_device.h): workgroup b writes its six
// sums to partial[b]; tree_score_finish_kernel (one workgroup) adds them in a fixed order into summary[8]
__global__ __launch_bounds__(CH) void tree_score_kernel(const double* __restrict__ tg, int64_t n, int64_t n_pad, Rigid tf,
                                                        const double* __restrict__ prep, int L, double lambda_c,
                                                        double maha2_max, int32_t* __restrict__ node_out,
                                                        double* __restrict__ maha2_out, double* __restrict__ logp_out,
                                                        double* __restrict__ partial) {
    const int64_t i = (int64_t)blockIdx.x * CH + threadIdx.x;
    tree_score_body(i, i, i < n, tg, n_pad, tf, prep, L, lambda_c, maha2_max, node_out, maha2_out, logp_out,
                    partial + (size_t)SCORE_NSUM * blockIdx.x);
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

static int tree_flags(hgmm_ctx* c, bool reset);
static int tree_alloc_nodes(hgmm_ctx* c, int L) {
    const int64_t T = level_first(L);
    c->tree.L = L;
    c->tree.T = (int)T;
    HGMM_TRY(ensure(c, c->t_pi, sizeof(double) * T));
    HGMM_TRY(ensure(c, c->t_mu, sizeof(double) * 3 * T));
    HGMM_TRY(ensure(c, c->t_cov, sizeof(double) * 9 * T));
    HGMM_TRY(ensure(c, c->t_prep, sizeof(double) * PREP_N * T));
    HGMM_TRY(ensure(c, c->t_mom, sizeof(double) * NMOM * T));
    HGMM_TRY(tree_flags(c, true));
    return HGMM_OK;
}

// tree flags (int[4]: bit 0 of [0] = some node's Sigma^-1 failed the Cholesky test) + the executed-pair counter of the
// level log-likelihood (uint64 at byte 16); `reset`: a new node table is about to be prepared
constexpr size_t TREE_FLAGS_BYTES = 64;
constexpr size_t TREE_TICKET_BYTES = sizeof(unsigned int) * TICKET_STRIDE * (1 + TICKET_GROUPS);   // the tickets of store_block_q
static int tree_flags(hgmm_ctx* c, bool reset) {
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
static inline int* flags_ptr(hgmm_ctx* c) { return c->t_flags.as<int>(); }
static inline unsigned long long* pairs_ptr(hgmm_ctx* c) {
    return reinterpret_cast<unsigned long long*>(c->t_flags.as<char>() + 16);
}
static inline unsigned int* tickets_ptr(hgmm_ctx* c) { return c->t_tickets.as<unsigned int>(); }

// 2^(j / 2048), j = 0 .. 2047, correctly rounded (formed in the x87 80-bit format), once per context
static int ensure_exp_tab2(hgmm_ctx* c) {
    if (c->exp_tab2.p) return HGMM_OK;
    HGMM_TRY(ensure(c, c->exp_tab2, sizeof(double) * EXP_TAB2_N));
    std::vector<double> h(EXP_TAB2_N);
    for (int j = 0; j < EXP_TAB2_N; ++j) h[j] = (double)exp2l((long double)j / (long double)EXP_TAB2_N);
    HGMM_HIP(c, hipMemcpyAsync(c->exp_tab2.p, h.data(), sizeof(double) * EXP_TAB2_N, hipMemcpyHostToDevice, c->stream));
    HGMM_HIP(c, ctx_stream_sync(c));              // `h` is pageable host memory
    return HGMM_OK;
}

// pinned {done, iterations} slots + events for the build's look-ahead batches
static int tree_host_ctl(hgmm_ctx* c, TreeCtl** out) {
    if (!c->tree_hctl) {
        // (coherent = fine-grained: a system-scope store of a running kernel is visible to the polling host at once)
        // layout: [0, 32) two control-word slots of the batch scheme, [64] the polled progress word of the tree build,
        // [128] sequence number + [256, 480) the 28 numbers of the registration loop's hand-over
        HGMM_HIP(c, hipHostMalloc(&c->tree_hctl, 1024, hipHostMallocMapped | hipHostMallocCoherent));
        std::memset(c->tree_hctl, 0, 1024);
        HGMM_HIP(c, hipEventCreateWithFlags(&c->tree_ev[0], hipEventDisableTiming));
        HGMM_HIP(c, hipEventCreateWithFlags(&c->tree_ev[1], hipEventDisableTiming));
    }
    *out = static_cast<TreeCtl*>(c->tree_hctl);
    return HGMM_OK;
}

static int tree_prep(hgmm_ctx* c, int64_t jb, int64_t je) {
    tree_prep_kernel<<<nblk(je - jb, 256), 256, 0, c->stream>>>(c->t_pi.as<double>(), c->t_mu.as<double>(),
                                                               c->t_cov.as<double>(), jb, je,
                                                               c->t_prep.as<double>(), flags_ptr(c));
    HGMM_HIP(c, hipGetLastError());
    return HGMM_OK;
}

}  // namespace hgmm

using namespace hgmm;

extern "C" int hgmm_tree_build(hgmm_ctx* c, int L, double ls, double ld, const double* init_mu,
                               double sig2, int max_iters_per_level, double* pi_out, double* mu_out,
                               double* cov_out, int32_t* leaf_idx_out, int32_t* iters_per_level_out,
                               double* q_trace_out, int q_capacity, int* q_len_out) {
    HGMM_ENTER(c);
    if (!c->have_f64 || c->n <= 0) return fail(c, HGMM_ERR_STATE, "tree build: set points first");
    if (L < 1 || L > 6) return fail(c, HGMM_ERR_ARG, "tree levels L = %d outside 1..6", L);
    if (!init_mu) return fail(c, HGMM_ERR_ARG, "init_mu is NULL");
    if (c->n > 0x7fffffff - 1024) return fail(c, HGMM_ERR_ARG, "too many points for 32-bit indices");
    if (max_iters_per_level < 1) max_iters_per_level = 1;
    HGMM_HIP(c, hipSetDevice(c->device));
    HGMM_TRY(tree_alloc_nodes(c, L));
    const int64_t T = c->tree.T;
    const int64_t n = c->n, n_pad = c->n_pad;
    int64_t maxP = 1;
    for (int i = 0; i < L - 1; ++i) maxP *= 8;                 // parents at the last level
    const int64_t max_chunks = n / CH + maxP + 8;
    // buffers
    HGMM_TRY(ensure(c, c->scratch, sizeof(double) * 3 * T));
    HGMM_TRY(ensure(c, c->t_current, sizeof(int) * 2 * n_pad));              // two assignments (tree_ll_estep_kernel)
    HGMM_TRY(ensure(c, c->t_perm, sizeof(int) * 2 * n_pad));                 // ping-pong
    HGMM_TRY(ensure(c, c->t_parent, sizeof(double) * 3 * n_pad));            // second coordinate buffer
    HGMM_TRY(ensure(c, c->t_seg, sizeof(int) * (2 * (8 * maxP + 2) + 2 * (maxP + 2) + 8)));
    HGMM_TRY(ensure(c, c->t_chunks, sizeof(int) * (size_t)(3 + 8 + 8) * max_chunks));
    HGMM_TRY(ensure(c, c->t_partials, sizeof(double) * (size_t)8 * NMOM * max_chunks));
    HGMM_TRY(ensure(c, c->t_q, sizeof(double) * (nblk(n, CH) + 8)));

    double* d_pi = c->t_pi.as<double>();
    double* d_mu = c->t_mu.as<double>();
    double* d_cov = c->t_cov.as<double>();
    double* d_prep = c->t_prep.as<double>();
    double* d_mom = c->t_mom.as<double>();
    // coordinate ping-pong: A = x_soa64 (original order == sorted order at level 0), B = t_parent
    double* xs_a = c->x_soa64.as<double>();
    double* xs_b = c->t_parent.as<double>();
    int* perm_a = c->t_perm.as<int>();
    int* perm_b = perm_a + n_pad;
    int* cur = c->t_current.as<int>();
    int* seg_a = c->t_seg.as<int>();
    int* seg_b = seg_a + (8 * maxP + 2);
    int* chunk_first = seg_b + (8 * maxP + 2);
    int* n_chunks_dev = chunk_first + (maxP + 2) * 2;
    int* chunk_desc = c->t_chunks.as<int>();
    int* hist = chunk_desc + 3 * max_chunks;
    int* chunk_off = hist + 8 * max_chunks;
    double* partials = c->t_partials.as<double>();
    double* block_q = c->t_q.as<double>();
    double* q_dev = block_q + nblk(n, CH);
    unsigned int* q_ticket_buf = tickets_ptr(c);              // (zeroed by tree_alloc_nodes -> tree_flags; every launch leaves them zero)
    TreeCtl* ctl = reinterpret_cast<TreeCtl*>(q_dev + 2);
    TreeLoopState* loop_state = reinterpret_cast<TreeLoopState*>(q_dev + 4);     // two slots (tree_follow), right behind ctl
    const int trace_cap = std::min(max_iters_per_level, 1 << 20);
    HGMM_TRY(ensure(c, c->t_qtrace, sizeof(double) * (size_t)trace_cap * L));     // one segment per level, read back at the end
    double* trace_base = c->t_qtrace.as<double>();
    std::vector<int> level_iters(L, 0);
    // points per thread in the log-likelihood kernel (N = 1e6, L = 4 build: 10.2 / 8.4 / 8.0 ms with 1 / 2 / 4)
    // (one point per thread for small clouds was tried in round 3: C4 level 0 / 1 got slower, 11.5 / 16.0 vs 9.2 / 15.4 us --
    //  these launches are chains of memory round trips, not arithmetic)
    const int ll_pts = n >= 400000 ? 4 : 2;
    // (a 64-point / node-split form of the log-likelihood for small clouds -- four waves of a workgroup sharing 64 points and
    //  splitting the nodes, no finish pass -- was built and measured in round 3 and lost at every C4 level: 16.9 / 17.7 /
    //  20.2 / 49 us per iteration against 8.9 / 14.8 / 19.1 / 22.4 for this form: eight times as many workgroups each read
    //  the level's whole node table for the reach test; removed again, commit 7d926ef)
    if (ll_pts == 4) HGMM_TRY(ensure_exp_tab2(c));
    // the E-step's LDS transpose in two passes (half the LDS, twice the resident workgroups) once a level has more chunks
    // than the chip holds at a time
    const bool estep_half = n / CH > (int64_t)3 * c->cus;
    // iterations enqueued per batch.  Round 2 (host waits at every batch boundary): 1/2/4/8/16 -> 6.8/6.3/5.6/5.1/5.3 ms @C4.
    // With the host one batch ahead (below) a level that stops at iteration k still has (ceil(k / B) + 1) B - k
    // iterations enqueued behind the stop (46 over C4's four levels at B = 8, 22 at B = 4) -- but each of those is three
    // launches that return at their first load, and a batch boundary (control-word copy + event) costs more than it
    // saves: 2/4/8 -> 3.67/3.60/3.46 ms @C4, 5.12/5.07/5.02 @1M on one box.
    const int batch_iters = 8;
    // single GPU: progress word in pinned host memory, polled (see the level loop); HGMM_TREE_AHEAD=0 -> the batch scheme
    // (C4, one box: batch scheme 3.16-3.6 ms; 1 / 2 / 3 / 4 / 6 iterations ahead: 3.39 / 2.88 / 3.0 / 2.94 / 2.97 ms -- with one
    //  the device waits for the host after every iteration; the host needs ~10 us to enqueue what the device runs in ~25)
    const int ahead_iters = c->cfg[CFG_TREE_AHEAD];
    // the stop rule inside the next launch (tree_follow) instead of a ticketed tail of the log-likelihood: needs the
    // polled scheme with >= 2 iterations ahead (the verdict on iteration e is reached by launch e + 1)
    const bool use_follow = !c->comm_on() && ahead_iters >= 2 && !c->cfg[CFG_TREE_TICKETS];
    // small clouds: iteration e + 1's (speculative) E-step rides in iteration e's log-likelihood launch and the moments
    // kernel takes over the stop rule (tree_ll_estep_kernel); HGMM_TREE_OVERLAP=0 -> one launch each, as for large clouds
    const bool overlap = use_follow && ahead_iters > 0 && !estep_half && ll_pts != 4 && c->cfg[CFG_TREE_OVERLAP];
    int* curbuf[2] = {cur, overlap ? cur + n_pad : cur};
    unsigned long long* host_word = nullptr;                   // host address / device address of the same pinned word
    unsigned long long* host_word_dev = nullptr;
    // (under a communicator too, round 6: every rank reads the same reduced q, so every rank's stop rule says the same and
    //  every rank's host can follow its own device's progress word -- see the level loop)
    if (ahead_iters > 0) {
        TreeCtl* hp0 = nullptr;
        HGMM_TRY(tree_host_ctl(c, &hp0));
        host_word = reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(hp0) + 64);
        void* dp = nullptr;
        HGMM_HIP(c, hipHostGetDevicePointer(&dp, host_word, 0));
        host_word_dev = static_cast<unsigned long long*>(dp);
    }

    HGMM_HIP(c, hipMemcpyAsync(c->scratch.p, init_mu, sizeof(double) * 3 * T, hipMemcpyHostToDevice, c->stream));
    tree_init_nodes_kernel<<<nblk(T, 256), 256, 0, c->stream>>>(c->scratch.as<double>(), sig2, T, d_pi, d_mu, d_cov);
    HGMM_TRY(tree_prep(c, 0, T));
    tree_iota_kernel<<<nblk(n, 256), 256, 0, c->stream>>>(perm_a, n);
    const int seg0[2] = {0, (int)n};
    HGMM_HIP(c, hipMemcpyAsync(seg_a, seg0, sizeof seg0, hipMemcpyHostToDevice, c->stream));
    HGMM_HIP(c, hipGetLastError());

    // global point count (pi = m0 / N_total)
    double n_total = (double)n;
    if (c->comm_on()) {
        HGMM_TRY(hgmm_comm_allreduce_f64(c, &n_total, 1, 0));
    }

    // the resident cloud (x_soa64 = level-0 order) is never overwritten: the first scatter goes
    // A -> B, later ones alternate between B and a third buffer C
    double* xs_c = nullptr;
    if (L > 2) {
        HGMM_TRY(ensure(c, c->t_xs3, sizeof(double) * 3 * n_pad));
        xs_c = c->t_xs3.as<double>();
    }
    auto cleanup = [&]() {};

    const double* xs_cur = xs_a;
    int* perm_cur = perm_a;
    int* seg_cur = seg_a;
    int P = 1;
    int q_len = 0;
    int rc = HGMM_OK;
    for (int l = 0; l < L && rc == HGMM_OK; ++l) {
        const int64_t lb = level_first(l), le = level_first(l + 1);
        const int n_level = (int)(le - lb);
        const int64_t parent_first = (l == 0) ? 0 : level_first(l - 1);
        double* trace_dev = trace_base + (size_t)l * trace_cap;
        tree_chunks_kernel<<<1, 1024, 0, c->stream>>>(seg_cur, P, chunk_first, chunk_desc, n_chunks_dev);
        const unsigned grid_chunks = (unsigned)(n / CH + P + 1);
        // small clouds do not have enough 256-point blocks to fill the chip: split the level's nodes
        // over gridDim.y and add the per-chunk sums in a second (fixed-order) kernel
        const int pblocks = (int)nblk(n, CH);
        const int llblocks = (int)nblk(n, CH * ll_pts);        // log-likelihood grid: ll_pts points per thread
        int chunks = 1, per_chunk = n_level;
        tree_ll_split(llblocks, n_level, c->cus, &chunks, &per_chunk);
        double* ll_partial = nullptr;
        if (chunks > 1) {
            rc = ensure(c, c->t_llp, sizeof(double) * (size_t)chunks * n_pad);
            if (rc != HGMM_OK) break;
            ll_partial = c->t_llp.as<double>();
        }
        // The stop rule runs on the device (tree_ctl_kernel); the host enqueues `batch` iterations per
        // synchronisation and reads {done, iterations} back, so launches overlap execution.  Kernels of
        // iterations enqueued past the stop return immediately.  With a communicator the all-reduces of the
        // enqueued iterations cannot be predicated, so they run out of place: rank-local moments / q stay where
        // the (skipped) kernels left them, the reduced copies are rebuilt identically, the M-step and the stop
        // rule read the copies -- surplus iterations are idempotent and no per-iteration host round trip is needed.
        // (ctl and the two loop-state slots of tree_follow behind it: 48 contiguous bytes)
        HGMM_HIP(c, hipMemsetAsync(ctl, 0, sizeof(TreeCtl) + 2 * sizeof(TreeLoopState), c->stream));
        const int batch = batch_iters;
        double* mom_g = nullptr;
        double* q_g = q_dev;
        if (c->comm_on()) {
            rc = ensure(c, c->comm_buf, sizeof(double) * ((size_t)NMOM * n_level + 8));
            if (rc != HGMM_OK) break;
            mom_g = c->comm_buf.as<double>();
            q_g = mom_g + (size_t)NMOM * n_level;
        }
        // One EM iteration of the level, enqueued (every kernel looks at ctl->done first and returns at once when the level
        // has stopped).
        // follow mode (single GPU, polled look-ahead): launch e of the E-step adds up the shares of q that iteration e - 1
        // left behind and applies the stop rule itself (tree_follow); the log-likelihood kernels only store their shares
        // level 0 of an overlapped build: q comes out of the (next iteration's) E-step, one share per chunk (TreeEstepArgs)
        const bool fused0 = overlap && l == 0;
        const int q_shares = (fused0 || chunks > 1) ? pblocks : llblocks;
        auto follow_of = [&](int e) {
            return TreeFollow{block_q, q_shares, loop_state + ((e - 1) & 1), loop_state + (e & 1), &ctl->done, ls,
                              max_iters_per_level, trace_dev, trace_cap, host_word_dev};
        };
        auto enqueue_iteration = [&](int e) -> int {
            int rc = HGMM_OK;
            const TreeFollow no_follow{nullptr, 0, nullptr, nullptr, nullptr, 0.0, 0, nullptr, 0, nullptr};
            int* cur = curbuf[e & 1];                                      // (overlap: iteration e's assignment; else always the same)
                if (!overlap || e == 0) {
                    ProfScope prof(c, HGMM_K_TREE_ESTEP);
                    const TreeFollow fol = (use_follow && e >= 1) ? follow_of(e) : no_follow;
                    if (estep_half)
                        tree_estep_kernel<true><<<grid_chunks, CH, 0, c->stream>>>(xs_cur, n_pad, d_prep, chunk_desc,
                                                                                  n_chunks_dev, parent_first, l, partials, cur,
                                                                                  &ctl->done, fol);
                    else
                        tree_estep_kernel<false><<<grid_chunks, CH, 0, c->stream>>>(xs_cur, n_pad, d_prep, chunk_desc,
                                                                                   n_chunks_dev, parent_first, l, partials, cur,
                                                                                   &ctl->done, fol);
                }
                // single GPU: reduction, M-step and preparation of a node in one launch; with a
                // communicator the all-reduce of the moments sits between reduction and M-step
                // (small clouds below level 0: a wave per parent, same bits.  Level 0 is ONE parent with all of the cloud's chunks:
                //  eight waves gathering side by side are 3 us quicker than one wave taking the eight rows in turn)
                if (overlap && l > 0)
                    tree_moments8_kernel<<<n_level / 8, 64, 0, c->stream>>>(partials, chunk_first, d_mom + NMOM * lb, lb, n_total,
                                                                            ld, d_pi, d_mu, d_cov, d_prep, flags_ptr(c), &ctl->done,
                                                                            e >= 1 ? follow_of(e) : no_follow);
                else
                    tree_moments_kernel<<<n_level, 64, 0, c->stream>>>(partials, chunk_first, n_level, d_mom + NMOM * lb,
                                                                       c->comm_on() ? 0 : 1, lb, n_total, ld, d_pi, d_mu, d_cov,
                                                                       d_prep, flags_ptr(c), &ctl->done,
                                                                       (overlap && e >= 1) ? follow_of(e) : no_follow);
                if (c->comm_on()) {
                    rc = allreduce_f64_oop(c, d_mom + NMOM * lb, mom_g, (size_t)NMOM * n_level);
                    if (rc != HGMM_OK) return rc;
                    tree_mstep_kernel<<<nblk(n_level, 256), 256, 0, c->stream>>>(mom_g, lb, n_level, n_total, ld, d_pi,
                                                                                 d_mu, d_cov, d_prep, flags_ptr(c), &ctl->done, 0);
                }
                {
                    ProfScope prof(c, HGMM_K_TREE_LOGLIK);
                    // the last workgroup to finish adds up the per-block shares of q (store_block_q)
                    // ... and, on a single GPU, applies the level's stop rule (with a communicator q is all-reduced
                    // first and tree_ctl_kernel does it)
                    const TreeStop no_stop{nullptr, 0.0, 0, nullptr, 0};
                    const TreeStop stop = (c->comm_on() || use_follow)
                                              ? no_stop
                                              : TreeStop{ctl, ls, max_iters_per_level, trace_dev, trace_cap, host_word_dev};
                    unsigned int* q_ticket = use_follow ? nullptr : q_ticket_buf;     // follow mode: plain stores of the shares
#define LL_LAUNCH(PTS)                                                                                     \
    tree_loglik_kernel<PTS><<<dim3(llblocks, chunks), CH, 0, c->stream>>>(                                 \
        xs_cur, n, n_pad, d_prep, lb, n_level, per_chunk, ll_partial, block_q, q_ticket, q_dev, &ctl->done, \
        chunks > 1 ? no_stop : stop, flags_ptr(c), pairs_ptr(c))
                    if (overlap && (e + 1 < max_iters_per_level || fused0)) {
                        // (level 0: no log-likelihood workgroups at all -- the E-step stores the shares of q; behind the
                        //  budget's last iteration it runs for those alone, its moments and assignment are never read)
                        const TreeLoglikArgs la{xs_cur, n, n_pad, d_prep, lb, n_level, per_chunk, ll_partial, block_q, q_ticket,
                                                q_dev, &ctl->done, no_stop, flags_ptr(c), pairs_ptr(c), nullptr};
                        const TreeEstepArgs ea{xs_cur, n_pad, d_prep, chunk_desc, n_chunks_dev, parent_first, l, partials,
                                               curbuf[(e + 1) & 1], &ctl->done, fused0 ? block_q : nullptr};
                        const int gx = fused0 ? 0 : llblocks, gy = fused0 ? 0 : chunks;
                        const unsigned g = (unsigned)(gx * gy) + grid_chunks;
                        if (ll_pts == 2 && c->tree.pdf_f32) tree_ll_estep_kernel<2, true><<<g, CH, 0, c->stream>>>(la, gx, gy, ea);
                        else if (ll_pts == 2) tree_ll_estep_kernel<2><<<g, CH, 0, c->stream>>>(la, gx, gy, ea);
                        else tree_ll_estep_kernel<1><<<g, CH, 0, c->stream>>>(la, gx, gy, ea);
                    } else if (c->tree.pdf_f32 && ll_pts >= 2) {
                        const TreeLoglikArgs la{xs_cur, n, n_pad, d_prep, lb, n_level, per_chunk, ll_partial, block_q, q_ticket,
                                                q_dev, &ctl->done, chunks > 1 ? no_stop : stop, flags_ptr(c), pairs_ptr(c), nullptr};
                        if (ll_pts == 4) tree_loglik_f32_kernel<4><<<dim3(llblocks, chunks), CH, 0, c->stream>>>(la);
                        else tree_loglik_f32_kernel<2><<<dim3(llblocks, chunks), CH, 0, c->stream>>>(la);
                    } else if (ll_pts == 4)
                        tree_loglik_kernel<4, true><<<dim3(llblocks, chunks), CH, 0, c->stream>>>(
                            xs_cur, n, n_pad, d_prep, lb, n_level, per_chunk, ll_partial, block_q, q_ticket, q_dev, &ctl->done,
                            chunks > 1 ? no_stop : stop, flags_ptr(c), pairs_ptr(c), c->exp_tab2.as<double>());
                    else if (ll_pts == 2) LL_LAUNCH(2);
                    else LL_LAUNCH(1);
#undef LL_LAUNCH
                    if (chunks > 1 && !fused0) {
                        if (c->tree.pdf_f32 && ll_pts >= 2)
                            tree_loglik_finish_kernel<true><<<pblocks, CH, 0, c->stream>>>(ll_partial, n, n_pad, chunks, block_q,
                                                                                          q_ticket, q_dev, &ctl->done, stop);
                        else
                            tree_loglik_finish_kernel<false><<<pblocks, CH, 0, c->stream>>>(ll_partial, n, n_pad, chunks, block_q,
                                                                                           q_ticket, q_dev, &ctl->done, stop);
                    }
                }
                if (c->comm_on()) {
                    rc = allreduce_f64_oop(c, q_dev, q_g, 1);
                    if (rc != HGMM_OK) return rc;
                    tree_ctl_kernel<<<1, 1, 0, c->stream>>>(q_g, ctl, ls, max_iters_per_level, trace_dev, trace_cap, host_word_dev);
                }
            // a launch the runtime rejected (LDS / grid limits of another chip) would leave the progress word untouched
            // for ever: the loops below must hear about it here
            const hipError_t le = hipGetLastError();
            if (le != hipSuccess) return fail(c, HGMM_ERR_HIP, "tree build: kernel launch failed: %s", hipGetErrorString(le));
            return HGMM_OK;
        };
        // The host stays ONE BATCH AHEAD of the device: batch k + 1 is enqueued before the host waits for batch k's
        // verdict (an asynchronous copy of {done, iterations} into pinned memory + an event), so the device never idles
        // at a batch boundary (round 2: enqueue, copy, synchronise, enqueue -- 30-40 us of idle device per batch, a
        // quarter of C4's build).  The price: when a level stops, the batch enqueued ahead runs as skipped launches
        // (~1 us each).  No batch is enqueued beyond the level's iteration budget.
        int it = 0;
        if (host_word) {
            // Single GPU: the stop rule's last thread also stores (done << 32 | iterations) into a word of pinned HOST
            // memory, and the host keeps `ahead` iterations enqueued beyond the last one it has seen finished -- no copy, no
            // event, no synchronisation inside a level, and at most `ahead` iterations of skipped launches behind a stop
            // (the batch scheme below: 46 of them over C4's four levels, ~0.25 ms of a 3.1 ms build, plus a control-word
            // copy per batch).  The word is reset here: every launch that could write it belongs to this level.
            __atomic_store_n(host_word, 0ull, __ATOMIC_RELAXED);
            int enq = 0;
            unsigned spins = 0;
            while (rc == HGMM_OK) {
                const unsigned long long w = __atomic_load_n(host_word, __ATOMIC_RELAXED);
                it = (int)(w & 0xffffffffull);
                if (w >> 32) {                                                // the level has stopped after `it` iterations
                    // Under a communicator every rank must have enqueued the SAME collectives when it leaves the level.
                    // How far a rank's host had got when it saw the stop is a matter of timing; min(it + ahead, budget)
                    // is not: each rank tops its queue up to exactly that many iterations (the surplus ones return at
                    // their first load, their all-reduces run out of place on unchanged operands).  Round 5 looked at
                    // the stop word once per 8 iterations, one batch behind: up to 15 surplus iterations per level,
                    // 46 over C4's four levels; now `ahead` (2) per level, whatever the backend.
                    if (c->comm_on()) {
                        const int must = std::min(it + ahead_iters, max_iters_per_level);
                        while (rc == HGMM_OK && enq < must) rc = enqueue_iteration(enq++);
                        c->tree.surplus_iterations += (unsigned long long)(enq - it);
                    }
                    break;
                }
                if (enq < max_iters_per_level && enq - it < ahead_iters) {
                    rc = enqueue_iteration(enq);
                    ++enq;
                    if (use_follow && rc == HGMM_OK && enq == max_iters_per_level) {
                        // nobody follows the budget's last iteration: one workgroup accounts for its q
                        tree_close_kernel<<<1, CH, 0, c->stream>>>(follow_of(enq));
                        if (hipGetLastError() != hipSuccess) rc = fail(c, HGMM_ERR_HIP, "tree build: launch failed");
                    }
                    spins = 0;
                    continue;
                }
                if (enq >= max_iters_per_level && it >= enq) {                // cannot happen (the budget's last iteration stops)
                    rc = fail(c, HGMM_ERR_STATE, "tree build: level %d did not stop within its budget", l);
                    break;
                }
                __builtin_ia32_pause();
                if ((++spins & 0x3fff) == 0) {                                // every ~16k polls: is the device still alive?
                    const hipError_t qe = hipStreamQuery(c->stream);
                    if (qe != hipSuccess && qe != hipErrorNotReady)
                        rc = fail(c, HGMM_ERR_HIP, "tree build: device error: %s", hipGetErrorString(qe));
                    else if (qe == hipSuccess && __atomic_load_n(host_word, __ATOMIC_ACQUIRE) == w)
                        // the stream is idle -- everything enqueued has run -- and the word has not moved: nothing is left
                        // that could move it (the old batch scheme ended in the same error here)
                        rc = fail(c, HGMM_ERR_STATE, "tree build: level %d made no progress (%d iterations enqueued, %d seen)",
                                  l, enq, it);
                }
            }
        } else {
            TreeCtl* hp = nullptr;
            rc = tree_host_ctl(c, &hp);
            int enq = 0, slot = 0;
            auto enqueue_batch = [&](int s) -> int {
                const int cnt = std::min(batch, max_iters_per_level - enq);
                for (int b = 0; b < cnt; ++b) {
                    const int r = enqueue_iteration(enq + b);
                    if (r != HGMM_OK) return r;
                }
                enq += cnt;
                if (hipMemcpyAsync(&hp[s], ctl, sizeof(TreeCtl), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
                    hipEventRecord(c->tree_ev[s], c->stream) != hipSuccess)
                    return fail(c, HGMM_ERR_HIP, "tree build: device error: %s", hipGetErrorString(hipGetLastError()));
                return HGMM_OK;
            };
            if (rc == HGMM_OK) rc = enqueue_batch(slot);
            while (rc == HGMM_OK) {
                const bool ahead = enq < max_iters_per_level;
                if (ahead) rc = enqueue_batch(slot ^ 1);
                if (rc != HGMM_OK) break;
                if (hipEventSynchronize(c->tree_ev[slot]) != hipSuccess) {
                    rc = fail(c, HGMM_ERR_HIP, "tree build: device error: %s", hipGetErrorString(hipGetLastError()));
                    break;
                }
                it = hp[slot].it;
                if (hp[slot].done != 0) break;
                if (!ahead) {                      // cannot happen (the budget's last iteration sets done); never spin
                    rc = fail(c, HGMM_ERR_STATE, "tree build: level %d did not stop within its budget", l);
                    break;
                }
                slot ^= 1;
            }
        }
        level_iters[l] = it;
        if (rc != HGMM_OK) break;
        int* cur = curbuf[(it - 1) & 1];                       // the assignment of the last iteration that counted
        q_len += it;
        if (iters_per_level_out) iters_per_level_out[l] = it;
        if (l + 1 < L) {
            // partition for the next level
            tree_hist_kernel<<<grid_chunks, CH, 0, c->stream>>>(cur, chunk_desc, n_chunks_dev, hist);
            int* seg_next = (seg_cur == seg_a) ? seg_b : seg_a;
            tree_offsets_kernel<<<P, OFF_BLOCK, 0, c->stream>>>(hist, chunk_first, seg_cur, P, chunk_off, seg_next);
            double* xs_next = (xs_cur == xs_b) ? xs_c : xs_b;     // A -> B -> C -> B -> ...
            int* perm_next = (perm_cur == perm_a) ? perm_b : perm_a;
            tree_scatter_kernel<<<grid_chunks, CH, 0, c->stream>>>(xs_cur, n_pad, perm_cur, cur, chunk_desc, n_chunks_dev,
                                                                  chunk_off, xs_next, perm_next);
            HGMM_HIP(c, hipGetLastError());
            xs_cur = xs_next;
            perm_cur = perm_next;
            seg_cur = seg_next;
            P *= 8;
        } else if (leaf_idx_out) {
            int* out_dev = (perm_cur == perm_a) ? perm_b : perm_a;
            tree_unsort_kernel<<<nblk(n, 256), 256, 0, c->stream>>>(perm_cur, cur, n, out_dev);
            if (hipMemcpyAsync(leaf_idx_out, out_dev, sizeof(int) * n, hipMemcpyDeviceToHost, c->stream) != hipSuccess)
                rc = fail(c, HGMM_ERR_HIP, "tree build: leaf index download failed");
        }
    }
    if (rc == HGMM_OK) {
        // the per-iteration M-steps skip the 'complexity' ratio (registration only): all nodes at once, now
        tree_complexity_kernel<<<nblk(T, 256), 256, 0, c->stream>>>(d_cov, 0, T, d_prep);
        // The node tables and the q traces come back through the context's pinned ring: every copy is a DMA packet that
        // queues at once, ONE synchronisation, then plain memcpys.  (Copied straight into the caller's pageable arrays
        // each of the 3 + L copies blocked the host for ~20 us while the runtime staged it: 5 % of a C4 build.)  Tables
        // too large for the ring (L >= 5) are copied directly.
        hipError_t e = hipSuccess;
        struct Pending { void* dst; const void* src; size_t bytes; };
        std::vector<Pending> pending;
        size_t staged = 0;
        auto download = [&](void* dst, const void* dev_src, size_t bytes) {
            if (e != hipSuccess || !dst || bytes == 0) return;
            void* st = nullptr;
            if (staged + bytes + 256 <= STAGE_RING_BYTES / 2 && stage_reserve(c, bytes, &st) == HGMM_OK) {
                staged += (bytes + 255) & ~(size_t)255;
                e = hipMemcpyAsync(st, dev_src, bytes, hipMemcpyDeviceToHost, c->stream);
                pending.push_back({dst, st, bytes});
            } else {
                e = hipMemcpyAsync(dst, dev_src, bytes, hipMemcpyDeviceToHost, c->stream);
            }
        };
        download(pi_out, d_pi, sizeof(double) * T);
        download(mu_out, d_mu, sizeof(double) * 3 * T);
        download(cov_out, d_cov, sizeof(double) * 9 * T);
        if (q_trace_out) {                                          // the levels' q traces, back to back
            int at = 0;
            for (int l = 0; l < L && e == hipSuccess; ++l) {
                const int take = std::min(std::min(level_iters[l], trace_cap), q_capacity - at);
                if (take > 0) download(q_trace_out + at, trace_base + (size_t)l * trace_cap, sizeof(double) * take);
                at += level_iters[l];
                if (at >= q_capacity) break;
            }
        }
        if (e == hipSuccess) e = ctx_stream_sync(c);
        if (e != hipSuccess) rc = fail(c, HGMM_ERR_HIP, "tree build: download failed: %s", hipGetErrorString(e));
        else
            for (const Pending& pd : pending) std::memcpy(pd.dst, pd.src, pd.bytes);
    } else {
        (void)ctx_stream_sync(c);
    }
    cleanup();
    if (q_len_out) *q_len_out = q_len < q_capacity ? q_len : q_capacity;
    if (rc == HGMM_OK) { c->tree.nodes_ready = true; c->tree.mu_rmax = -1.0; }
    return rc;
}

extern "C" int hgmm_tree_set_precision(hgmm_ctx* c, int precision) {
    HGMM_ENTER(c);
    if (precision != HGMM_PRECISION_F64 && precision != HGMM_PRECISION_F32_PDF)
        return fail(c, HGMM_ERR_ARG, "hgmm_tree_set_precision: unknown precision %d", precision);
    c->tree.pdf_f32 = precision == HGMM_PRECISION_F32_PDF;
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
    double m2max = 0.0;
    for (int64_t j = 0; j < T; ++j) {
        const double v = mu[3 * j] * mu[3 * j] + mu[3 * j + 1] * mu[3 * j + 1] + mu[3 * j + 2] * mu[3 * j + 2];
        if (v > m2max) m2max = v;
    }
    c->tree.mu_rmax = std::sqrt(m2max);
    c->tree.nodes_ready = true;
    return HGMM_OK;
}

extern "C" int hgmm_tree_set_target(hgmm_ctx* c, const double* xyz, int64_t n) {
    HGMM_ENTER(c);
    if (!c || !xyz) return c ? fail(c, HGMM_ERR_ARG, "xyz is NULL") : HGMM_ERR_ARG;
    if (n <= 0) return fail(c, HGMM_ERR_ARG, "target must have at least one point");
    HGMM_HIP(c, hipSetDevice(c->device));
    const int64_t n_pad = (n + 255) / 256 * 256;
    HGMM_TRY(ensure(c, c->tgt_soa64, sizeof(double) * 3 * n_pad));
    std::vector<double> soa((size_t)3 * n_pad, 0.0);
    double r2max = 0.0;                                         // largest |x|^2: bounds the extent of the moved cloud
    for (int64_t i = 0; i < n; ++i) {
        double r2 = 0.0;
        for (int d = 0; d < 3; ++d) { soa[(size_t)d * n_pad + i] = xyz[3 * i + d]; r2 += xyz[3 * i + d] * xyz[3 * i + d]; }
        if (r2 > r2max) r2max = r2;
    }
    c->tgt_rmax = std::sqrt(r2max);
    HGMM_HIP(c, hipMemcpyAsync(c->tgt_soa64.p, soa.data(), sizeof(double) * soa.size(), hipMemcpyHostToDevice, c->stream));
    HGMM_HIP(c, ctx_stream_sync(c));
    c->tgt_n = n;
    c->tgt_pad = n_pad;
    return HGMM_OK;
}

// fixed-point moments of the resident target under (rot, t, scale) -> c->t_momq [T][NMQ] (all-reduced over the
// ranks as integers: still exact); *d_out / *f_out = extent and fractional bits of the encoding
template <int NMQ>
static int reg_estep_fixed(hgmm_ctx* c, const double* rot, const double* t, double scale, double lambda_c,
                           double* d_out, int* f_out) {
    if (!c->tree.nodes_ready) return fail(c, HGMM_ERR_STATE, "registration E-step: no tree (build or set_nodes first)");
    if (c->tgt_n <= 0) return fail(c, HGMM_ERR_STATE, "registration E-step: call hgmm_tree_set_target first");
    HGMM_HIP(c, hipSetDevice(c->device));
    const int64_t T = c->tree.T;
    Rigid tf;
    for (int i = 0; i < 9; ++i) tf.r[i] = rot ? rot[i] : ((i % 4 == 0) ? 1.0 : 0.0);
    for (int i = 0; i < 3; ++i) tf.t[i] = t ? t[i] : 0.0;
    tf.s = scale;
    // extent: |s R x + t - mu| <= |s| (Frobenius bound on R) max|x| + |t| + max|mu|, rounded up to a power of two
    if (c->tree.mu_rmax < 0.0) {                                  // tree built on the device: means not seen by the host
        std::vector<double> mu((size_t)3 * T);
        HGMM_HIP(c, hipMemcpyAsync(mu.data(), c->t_mu.p, sizeof(double) * 3 * T, hipMemcpyDeviceToHost, c->stream));
        HGMM_HIP(c, ctx_stream_sync(c));
        c->tree.mu_rmax = tree_mu_rmax(mu.data(), T);
    }
    double ext = reg_extent(tf, c->tgt_rmax, c->tree.mu_rmax);
    if (c->comm_on()) {                                           // every rank must use the same encoding
        double e = ext;
        HGMM_TRY(hgmm_comm_allreduce_f64(c, &e, 1, 1));
        ext = e;
    }
    double n_all = (double)c->tgt_n;
    if (c->comm_on()) HGMM_TRY(hgmm_comm_allreduce_f64(c, &n_all, 1, 0));
    double D = 1.0;
    int F = 0;
    reg_encoding(ext, n_all, &D, &F);
    // Invariant: momq_dirty == false  <=>  EVERY word of the buffer (its whole capacity, not just the words of the
    // current tree) is zero.  Earlier uses may have been larger (hgmm_tree_estep writes 2 NMOM T + 1 two-word sums,
    // hgmm_tree_reg_estep leaves [T][10] behind, a deeper tree has more nodes): clearing only this tree's words and
    // then calling the buffer clean would let a later, larger use add onto stale sums.
    const size_t want = sizeof(unsigned long long) * NMOM * T;
    if (c->t_momq.cap < want || !c->t_momq.p || c->tree.momq_dirty) {
        HGMM_TRY(ensure(c, c->t_momq, want));
        HGMM_HIP(c, hipMemsetAsync(c->t_momq.p, 0, c->t_momq.cap, c->stream));
        c->tree.momq_dirty = false;
    }
    unsigned long long* mq = c->t_momq.as<unsigned long long>();
    {
        ProfScope prof(c, HGMM_K_TREE_REG);
        tree_reg_estep_kernel<NMQ><<<nblk(c->tgt_n, CH), CH, 0, c->stream>>>(
            c->tgt_soa64.as<double>(), c->tgt_n, c->tgt_pad, tf, c->t_prep.as<double>(), c->tree.L, lambda_c, 1.0 / D,
            std::ldexp(1.0, F), mq);
    }
    HGMM_HIP(c, hipGetLastError());
    c->tree.momq_dirty = true;                                    // until a consumer has cleared what it read
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
    HGMM_TRY(reg_estep_fixed<NMOM>(c, rot, t, scale, lambda_c, &D, &F));
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
    HGMM_TRY(reg_estep_fixed<4>(c, rot, t, scale, lambda_c, &D, &F));
    const int64_t T = c->tree.T;
    HGMM_TRY(ensure(c, c->scratch, sizeof(double) * 32));
    // The 28 numbers come back through coherent pinned memory: the kernel stores them there and then a sequence
    // number the host polls (a D2H copy packet + a stream synchronisation cost ~20 us of every ~60 us iteration).
    TreeCtl* hp = nullptr;
    HGMM_TRY(tree_host_ctl(c, &hp));
    char* hbase = reinterpret_cast<char*>(hp);
    unsigned long long* h_seq = reinterpret_cast<unsigned long long*>(hbase + 128);
    double* h_out = reinterpret_cast<double*>(hbase + 256);
    void *d_seq = nullptr, *d_out = nullptr;
    HGMM_HIP(c, hipHostGetDevicePointer(&d_seq, h_seq, 0));
    HGMM_HIP(c, hipHostGetDevicePointer(&d_out, h_out, 0));
    const unsigned long long seq = ++c->tree.reg_seq;
    tree_reg_normal_kernel<<<1, 256, 0, c->stream>>>(c->t_momq.as<unsigned long long>(), D, std::ldexp(1.0, -F),
                                                    c->t_prep.as<double>(), T, c->scratch.as<double>(),
                                                    static_cast<double*>(d_out), static_cast<unsigned long long*>(d_seq), seq);
    HGMM_HIP(c, hipGetLastError());
    c->tree.momq_dirty = false;                                   // the kernel zeroed the [T][4] words it consumed
    unsigned spins = 0;
    while (__atomic_load_n(h_seq, __ATOMIC_ACQUIRE) != seq) {
        __builtin_ia32_pause();
        if ((++spins & 0x3fff) == 0) {                            // is the device still alive?  has the stream drained?
            const hipError_t qe = hipStreamQuery(c->stream);
            if (qe != hipSuccess && qe != hipErrorNotReady)
                return fail(c, HGMM_ERR_HIP, "registration: device error: %s", hipGetErrorString(qe));
            // idle stream and still no sequence number: the kernel that writes it never ran
            if (qe == hipSuccess && __atomic_load_n(h_seq, __ATOMIC_ACQUIRE) != seq)
                return fail(c, HGMM_ERR_STATE, "registration: the normal-equation kernel did not report (sequence %llu)", seq);
        }
    }
    std::memcpy(out28, h_out, sizeof(double) * 28);
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
        // the loop on the device alone (forest_register_on_device: one pair on this context's tree and target)
        if (!c->tree.nodes_ready) return fail(c, HGMM_ERR_STATE, "registration: no tree (build or set_nodes first)");
        if (c->tgt_n <= 0) return fail(c, HGMM_ERR_STATE, "registration: call hgmm_tree_set_target first");
        const int64_t T = c->tree.T;
        if (c->tree.mu_rmax < 0.0) {
            std::vector<double> mu((size_t)3 * T);
            HGMM_HIP(c, hipMemcpyAsync(mu.data(), c->t_mu.p, sizeof(double) * 3 * T, hipMemcpyDeviceToHost, c->stream));
            HGMM_HIP(c, ctx_stream_sync(c));
            c->tree.mu_rmax = tree_mu_rmax(mu.data(), T);
        }
        const size_t want = sizeof(unsigned long long) * NMOM * T;
        if (c->t_momq.cap < want || !c->t_momq.p || c->tree.momq_dirty) {      // (reg_estep_fixed's invariant)
            HGMM_TRY(ensure(c, c->t_momq, want));
            HGMM_HIP(c, hipMemsetAsync(c->t_momq.p, 0, c->t_momq.cap, c->stream));
            c->tree.momq_dirty = false;
        }
        const int64_t first = 0, count = c->tgt_n;
        int32_t it32 = 0, st32 = 0;
        HGMM_TRY(forest_register_on_device(c, 1, c->tgt_soa64.as<double>(), c->tgt_pad, &first, &count, &c->tgt_rmax,
                                           &c->tree.mu_rmax, c->t_prep.as<double>(), (int)T, c->tree.L,
                                           c->t_momq.as<unsigned long long>(), rot, t, scale, lambda_c, max_iter, tol,
                                           q_prev_inout, &it32, &st32, trace));
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
    Rigid tf;
    for (int i = 0; i < 9; ++i) tf.r[i] = rot ? rot[i] : ((i % 4 == 0) ? 1.0 : 0.0);
    for (int i = 0; i < 3; ++i) tf.t[i] = t ? t[i] : 0.0;
    tf.s = scale;
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
        tree_score_kernel<<<nb, CH, 0, c->stream>>>(c->tgt_soa64.as<double>(), n, n_pad, tf, c->t_prep.as<double>(), c->tree.L,
                                                    lambda_c, maha2_max, d_node, d_maha, d_logp, partial);
    }
    tree_score_finish_kernel<<<1, CH, 0, c->stream>>>(partial, (int)nb, (double)n, d_sum);
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
// Flat FULL-covariance EM  ==  ONE tree level with branching J  (the CPU twin run
// with its module global n_node = J and maxTreeLevel = 1, hgmm_cupy_cpu_working.py:30,122-198).
// float64.  Per iteration:
//   full_pass_kernel     lanes across points, the J components tiled through LDS: for every
//                        point  den_i = sum_j pi_j N(x_i; j),  arg-max_j,  and the level
//                        log-likelihood term  log max(sum_{pi_j >= eps} pi_j N, eps).
//   full_moments_kernel  the 10 sufficient statistics per component as a dense contraction
//                        M[J,10] = Gamma^T [N,J] . F[N,10],  F_i = (1, x, y, z, xx, xy, xz, yy, yz, zz),
//                        on the fp64 matrix cores (v_mfma_f64_16x16x4_f64): per wave a 16-component
//                        x 16-feature accumulator tile stays in registers across all of the
//                        workgroup's points; gamma and F are transposed through LDS.
//   full_reduce_kernel   fixed-order sum of the per-workgroup partials -> mom[J][10] (the
//                        buffer the RCCL all-reduce works on), then tree_mstep/tree_prep.
// ==========================================================================================
namespace hgmm {

constexpr int FULL_LD = 66;          // LDS row stride (doubles): conflict-free 16x4 fragment reads
constexpr int FULL_WAVES = 2;        // waves per workgroup of the moments kernel (LDS: 2 x 2 x 8.4 KB)
constexpr int FULL_BLOCK = FULL_WAVES * 64;
typedef double double4_t __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(CH) void full_pass_kernel(const double* __restrict__ xs, int64_t n, int64_t n_pad,
                                                       const double* __restrict__ prep, int J,
                                                       double* __restrict__ den_out, int* __restrict__ label_out,
                                                       double* __restrict__ block_q) {
    __shared__ double tile[LL_TILE][11];
    __shared__ double shq[CH / 64];
    const int64_t i = (int64_t)blockIdx.x * CH + threadIdx.x;
    const bool active = i < n;
    double x0 = 0.0, x1 = 0.0, x2 = 0.0;
    if (active) { x0 = xs[i]; x1 = xs[n_pad + i]; x2 = xs[2 * n_pad + i]; }
    double den = 0.0, tot = 0.0, best = -1.0;
    int am = 0;
    for (int base = 0; base < J; base += LL_TILE) {
        const int cnt = (J - base < LL_TILE) ? J - base : LL_TILE;
        __syncthreads();
        for (int t = threadIdx.x; t < cnt * 11; t += CH) {
            const int node = t / 11, fidx = t % 11;
            tile[node][fidx] = prep[PREP_N * (base + node) + fidx];
        }
        __syncthreads();
        for (int node = 0; node < cnt; ++node) {
            const double wE = tile[node][9];
            if (wE == 0.0) continue;                                    // workgroup-uniform
            const double d0 = x0 - tile[node][6], d1 = x1 - tile[node][7], d2 = x2 - tile[node][8];
            const double q = sym3_quad(tile[node][0], tile[node][1], tile[node][2], tile[node][3], tile[node][4],
                                       tile[node][5], d0, d1, d2);
            double g = 0.0;
            if (__any(q < 1500.0)) g = wE * exp(-0.5 * q);
            den += g;
            if (tile[node][10] != 0.0) tot += g;      // pi >= eps: counts towards the log-likelihood
            if (g > best) { best = g; am = base + node; }
        }
    }
    if (active) {
        den_out[i] = den;
        label_out[i] = (den > TREE_EPS) ? am : 0;   // all gammas zero -> argmax = 0 (C:178,184)
    }
    double lq = active ? log(fmax(tot, TREE_EPS)) : 0.0;
    lq = wave_sum_f64(lq);
    if (lane_id() == 0) shq[wave_in_block()] = lq;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int w = 0; w < CH / 64; ++w) t += shq[w];
        block_q[blockIdx.x] = t;
    }
}

// grid = persistent workgroups, each owning a contiguous range of 64-point groups
__global__ __launch_bounds__(FULL_BLOCK) void full_moments_kernel(const double* __restrict__ xs, int64_t n, int64_t n_pad,
                                                          const double* __restrict__ prep, int J16,
                                                          const double* __restrict__ den_in,
                                                          double* __restrict__ partials /*[grid][J16][NMOM]*/) {
    __shared__ double G[FULL_WAVES][16][FULL_LD];    // gamma, component-major, per wave
    __shared__ double F[FULL_WAVES][16][FULL_LD];    // features, feature-major, per wave
    __shared__ double red[FULL_WAVES][16][16];
    const int w = wave_in_block(), lane = lane_id();
    const int64_t groups = (n + 63) / 64;
    const int64_t nw = (int64_t)gridDim.x * FULL_WAVES;
    const int64_t per = (groups + nw - 1) / nw;
    const int64_t gw = (int64_t)blockIdx.x * FULL_WAVES + w;
    const int64_t g0 = gw * per, g1 = (g0 + per < groups) ? g0 + per : groups;
    const int a_idx = lane & 15, b_idx = lane >> 4;

    for (int tile = 0; tile < J16; tile += 16) {
        double4_t acc = {0.0, 0.0, 0.0, 0.0};
        for (int64_t grp = g0; grp < g1; ++grp) {
            const int64_t i = grp * 64 + lane;
            const bool active = i < n;
            double x0 = 0.0, x1 = 0.0, x2 = 0.0, inv_den = 0.0;
            if (active) {
                x0 = xs[i]; x1 = xs[n_pad + i]; x2 = xs[2 * n_pad + i];
                const double den = den_in[i];
                inv_den = (den > TREE_EPS) ? 1.0 / den : 0.0;
            }
            // features of this lane's point, feature-major
            F[w][0][lane] = 1.0; F[w][1][lane] = x0; F[w][2][lane] = x1; F[w][3][lane] = x2;
            F[w][4][lane] = x0 * x0; F[w][5][lane] = x0 * x1; F[w][6][lane] = x0 * x2;
            F[w][7][lane] = x1 * x1; F[w][8][lane] = x1 * x2; F[w][9][lane] = x2 * x2;
#pragma unroll
            for (int f = 10; f < 16; ++f) F[w][f][lane] = 0.0;
#pragma unroll
            for (int cc = 0; cc < 16; ++cc) {
                const double* pr = prep + PREP_N * (tile + cc);     // wave-uniform
                const double wE = pr[9];
                double gam = 0.0;
                if (wE != 0.0) {
                    const double d0 = x0 - pr[6], d1 = x1 - pr[7], d2 = x2 - pr[8];
                    const double q = sym3_quad(pr[0], pr[1], pr[2], pr[3], pr[4], pr[5], d0, d1, d2);
                    if (__any(q < 1500.0)) gam = wE * exp(-0.5 * q) * inv_den;
                    // reference: gamma = g / den (C:176); accumulate() drops gamma < eps (C:100)
                    if (gam < TREE_EPS || !active) gam = 0.0;
                }
                G[w][cc][lane] = gam;
            }
            __builtin_amdgcn_s_waitcnt(0xc07f);      // lgkmcnt(0): this wave's LDS writes landed
            __builtin_amdgcn_wave_barrier();
            // 16 MFMAs: D[comp][feat] += sum over the 4 points of sub-group s
#pragma unroll
            for (int s = 0; s < 16; ++s) {
                const double a = G[w][a_idx][4 * s + b_idx];
                const double b = F[w][a_idx][4 * s + b_idx];
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
            }
            __builtin_amdgcn_wave_barrier();
        }
        // D layout (f64 16x16x4): row (component) = (lane >> 4) + 4 r, col (feature) = lane & 15
#pragma unroll
        for (int r = 0; r < 4; ++r) red[w][b_idx + 4 * r][a_idx] = acc[r];
        __syncthreads();
        // fixed-order combination of the workgroup's waves, one partial per workgroup
        for (int e = threadIdx.x; e < 16 * NMOM; e += FULL_BLOCK) {
            const int comp = e / NMOM, feat = e % NMOM;
            double t = 0.0;
#pragma unroll
            for (int ww = 0; ww < FULL_WAVES; ++ww) t += red[ww][comp][feat];
            partials[((size_t)blockIdx.x * J16 + tile + comp) * NMOM + feat] = t;
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------
// One-pass E-step of the flat full-covariance EM: every pdf (an fp64 exp) is evaluated ONCE.
//
// full_pass_kernel + full_moments_kernel evaluate every pi_j N(x_i; j) twice (once for the denominators, once
// more for the statistics) and the second kernel re-streams all points once per 16-component tile.  Here a
// workgroup (8 waves) takes FT_P = 16 points at a time and keeps the tile's un-normalised
// g[p][j] = pi_j N(x_p; j) in LDS (16 x (J16 + 16) doubles = 104 KB at J = 800):
//   phase A  lanes across components (<= 2 per lane, their (Sigma^-1, mu, pi coef) in registers), the tile's
//            points wave-uniform (scalar loads): g -> LDS, point-major (conflict-free writes)
//   phase B  each wave owns 2 of the 16 points: row sum = denominator, first arg-max, the log-likelihood
//            term (components with pi >= eps only), the point's 10 features -> LDS
//   phase C  M[j][f] += sum_p gamma[p][j] F[p][f] on the fp64 matrix cores (v_mfma_f64_16x16x4_f64, A = gamma
//            read back from LDS, normalised and thresholded on the fly; B = features); wave w owns the
//            16-component tiles w, w + 8, ... and keeps their accumulators in registers across ALL of the
//            workgroup's points.
// Deterministic (fixed tile -> workgroup map, fixed accumulation order); one partial per workgroup, summed by
// full_reduce_kernel.  LDS row stride J16 + 16 == 16 (mod 32) makes the A-fragment reads conflict-free.
// ------------------------------------------------------------------------------------------
constexpr int FT_P = 16;                 // points per tile
constexpr int FT_WAVES = 8;
constexpr int FT_BLOCK = FT_WAVES * 64;
constexpr int FT_LDF = 18;               // feature rows: 16 points + 2 (conflict-free B-fragment reads)
constexpr int FT_MAX_J16 = 1024;

__host__ __device__ inline int ft_ldg(int J16) {        // doubles per point row of g: == 16 (mod 32), and room
    return (J16 + 127) / 128 * 128 + 16;                // for whole 128-column steps (tail columns stay 0)
}
inline size_t ft_lds_bytes(int J16) {
    return sizeof(double) * ((size_t)FT_P * ft_ldg(J16) + 16 * FT_LDF + 3 * FT_P + J16 + 4 * 3 * FT_P + EXP_TAB2_N);
}

// The kernel's body, specialised at compile time on the form of the exponent:
//   CHOL   triangular form -|R (x - o) - R (mu - o)|^2 with R^T R = Sigma^-1 / 2 (prep[12..17]) and o = the cloud's first
//          point: 9 fma / mul per pair against 14 for 3 subtractions + the symmetric form; R (mu - o) is formed once per
//          component at the start.  (All points share ONE origin -- the flat fit's cloud is not spatially sorted --, so the
//          form carries a relative error of ~ eps |x - o| / sigma in the exponent: 1e-13 for millimetre clusters in a
//          metre-sized cloud, far inside the parity tolerances.)
//   !CHOL  the symmetric form, for node tables with a Sigma^-1 that failed the Cholesky test (flags bit 0).
template <int CPL, bool CHOL>
__device__ __forceinline__ void full_fused_body(
    const double* __restrict__ xs, int64_t n, int64_t n_pad, const double* __restrict__ prep, int J16,
    int* __restrict__ label_out, double* __restrict__ block_q, double* __restrict__ partials /*[grid][J16][NMOM]*/,
    int want_stats, long long* __restrict__ dbg, double* lds, const double* __restrict__ exp2_tab) {
    long long tA = 0, tB = 0, tC = 0, tW = 0, tm = 0;
#define FT_TICK(acc) do { if (dbg) { const long long now_ = clock64(); acc += now_ - tm; tm = now_; } } while (0)
    const int LDG = ft_ldg(J16);
    double* G = lds;                              // [FT_P][LDG]
    double* F = G + (size_t)FT_P * LDG;           // [16 features][FT_LDF]
    double* INV = F + 16 * FT_LDF;                // [FT_P] 1 / denominator (0: dead point)
    double* TOT = INV + FT_P;                     // [2][FT_P] sum over the components with pi >= eps (-1: dead point), by tile parity
    double* WL = TOT + 2 * FT_P;                  // [J16] 1.0 where pi_j >= eps (the component counts towards q)
    double* XS = WL + J16;                        // [2][3][FT_P] the tile's coordinates relative to the origin, double-buffered
    double* XA = XS + 2 * 3 * FT_P;               // [2][3][FT_P] ... and as given (the statistics' features)
    double* EXPT = XA + 2 * 3 * FT_P;             // [2048] 2^(j/2048) for exp_t11_4
    const int w = wave_in_block(), lane = lane_id();
    const int tid = (int)threadIdx.x;
    exp_tab2_load(EXPT, exp2_tab);                // (the barrier behind the WL / G initialisation covers it)

    // this lane's components: slot 0 = tid; slot 1 (J16 > 512) = tid + 512.  When the last wave of slot 1 has at
    // most 32 components left, they are a TAIL BLOCK of 32 components x 16 points that is dealt out over the waves
    // behind the full ones (which have nothing else in slot 1): each of `nw` such waves holds the same 32 components
    // in both half-waves and evaluates them for 16 / (2 nw) points per half-wave.  J = 800: waves 0-3 take 64 second
    // components each, waves 4-7 the tail, 2 points per lane -- every SIMD (waves w and w + 4) then carries 50 of
    // the tile's 200 wave-evaluations (round 2: one wave took the whole tail, its SIMD 56: phase A waited for it).
    const int R = (CPL == 2) ? J16 - FT_BLOCK : 0;
    const int w_r = R / 64, rem = R % 64;
    const bool tail_exists = CPL == 2 && rem > 0 && rem <= 32;
    const int free_w = FT_WAVES - w_r;                                   // waves without a full second block (>= 1)
    const int nw = tail_exists ? (free_w >= 8 ? 8 : (free_w >= 4 ? 4 : (free_w >= 2 ? 2 : 1))) : 0;
    const bool tail_wave = tail_exists && w >= w_r && w < w_r + nw;      // wave-uniform
    const int tail_pts = tail_exists ? FT_P / (2 * nw) : 0;              // points per half-wave: 8, 4, 2 or 1
    const int tail_p0 = tail_wave ? (w - w_r) * 2 * tail_pts + (lane >> 5) * tail_pts : 0;
    int jc[CPL];
    jc[0] = tid;
    if (CPL == 2) jc[1] = tail_wave ? FT_BLOCK + 64 * w_r + (lane & 31) : tid + FT_BLOCK;
    const double o0 = xs[0], o1 = xs[n_pad], o2 = xs[2 * n_pad];
    // CHOL: s* = R, m* = -R (mu - o);   !CHOL: s* = -Sigma^-1 / 2, m* = mu - o
    double s00[CPL], s01[CPL], s02[CPL], s11[CPL], s12[CPL], s22[CPL], m0[CPL], m1[CPL], m2[CPL], wE[CPL];
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
        const int j = jc[c];
        wE[c] = 0.0;
        s00[c] = s01[c] = s02[c] = s11[c] = s12[c] = s22[c] = m0[c] = m1[c] = m2[c] = 0.0;
        if (j < J16) {
            const double* pr = prep + PREP_N * j;
            const double u0 = pr[6] - o0, u1 = pr[7] - o1, u2 = pr[8] - o2;
            if (CHOL) {
                s00[c] = pr[PREP_R]; s01[c] = pr[PREP_R + 1]; s02[c] = pr[PREP_R + 2];
                s11[c] = pr[PREP_R + 3]; s12[c] = pr[PREP_R + 4]; s22[c] = pr[PREP_R + 5];
                m0[c] = -fma(s02[c], u2, fma(s01[c], u1, s00[c] * u0));
                m1[c] = -fma(s12[c], u2, s11[c] * u1);
                m2[c] = -(s22[c] * u2);
            } else {
                s00[c] = -0.5 * pr[0]; s01[c] = -0.5 * pr[1]; s02[c] = -0.5 * pr[2];
                s11[c] = -0.5 * pr[3]; s12[c] = -0.5 * pr[4]; s22[c] = -0.5 * pr[5];
                m0[c] = u0; m1[c] = u1; m2[c] = u2;
            }
            wE[c] = pr[9];
        }
    }
    // components with 0 < pi < eps take part in the E-step but not in q (C:80): rare enough that the second row
    // sum is only formed when one exists (workgroup-uniform flag)
    int my_small = 0;
    for (int j = tid; j < J16; j += FT_BLOCK) {
        const double wl = prep[PREP_N * j + 10], we = prep[PREP_N * j + 9];
        WL[j] = (wl != 0.0) ? 1.0 : 0.0;
        if (wl == 0.0 && we != 0.0) my_small = 1;
    }
    for (int e = tid; e < FT_P * LDG; e += FT_BLOCK) G[e] = 0.0;   // phase B reads whole 128-column steps
    const bool any_small = __syncthreads_or(my_small) != 0;
    // accumulator tiles of this wave
    const int ntiles = J16 / 16;
    constexpr int MAXT = (FT_MAX_J16 / 16 + FT_WAVES - 1) / FT_WAVES;     // 8
    double acc[MAXT][3];                          // per tile: three 4-feature blocks (4 x 4 x 4 products)
#pragma unroll
    for (int t = 0; t < MAXT; ++t) acc[t][0] = acc[t][1] = acc[t][2] = 0.0;
    const int a_idx = lane & 15, b_idx = lane >> 4;

    const int64_t tiles = (n + FT_P - 1) / FT_P;
    const int64_t per = (tiles + gridDim.x - 1) / gridDim.x;
    const int64_t t0 = (int64_t)blockIdx.x * per;
    const int64_t t1 = (t0 + per < tiles) ? t0 + per : tiles;
    // the wave that takes the tiles' log-likelihood terms: with the tail block dealt out, the waves behind the full second
    // blocks carry 16 + 2 evaluations per lane against 32 of the first ones -- but those share their SIMDs; measured,
    // wave 1 (32 evaluations, SIMD 1) finishes phase A 0.2 M cycles ahead of the critical wave and has room for the logs
    constexpr int LQ_WAVE = 1;
    double lq = 0.0;                              // wave LQ_WAVE: sum of the workgroup's log-likelihood terms

    // coordinates of a tile -> LDS buffer `buf` (threads 0..47; rows past the end repeat the last point)
    const int st_d = tid / FT_P, st_p = tid % FT_P;                      // the staging threads' (coordinate, point)
    const double st_o = (tid < 3 * FT_P) ? xs[(size_t)st_d * n_pad] : 0.0;    // ... and their coordinate of the origin
    auto stage = [&](int64_t tile, int buf) {
        if (tid < 3 * FT_P) {
            int64_t i = tile * FT_P + st_p;
            i = i < n ? i : n - 1;
            const double v = xs[(size_t)st_d * n_pad + i];
            XA[(buf * 3 + st_d) * FT_P + st_p] = v;
            XS[(buf * 3 + st_d) * FT_P + st_p] = v - st_o;
        }
    };
    // the log-likelihood terms of one tile (its TOT row), 16 lanes at once; taken by wave LQ_WAVE at the START of the
    // next tile's phase A, i.e. off the critical path of phase C
    auto tile_loglik = [&](int par) {
        const double tv = (lane < FT_P) ? TOT[par * FT_P + lane] : -1.0;
        double term = (tv >= 0.0) ? log(fmax(tv, TREE_EPS)) : 0.0;
        term = wave_sum_f64(term);
        lq += term;
    };
    if (t0 < t1) stage(t0, 0);
    __syncthreads();
    for (int64_t tile = t0; tile < t1; ++tile) {
        const int64_t base = tile * FT_P;
        const int buf = (int)((tile - t0) & 1);
        const double* X = XS + buf * 3 * FT_P;
        if (dbg) tm = clock64();
        if (w == LQ_WAVE && tile > t0) tile_loglik(buf ^ 1);
        // ---- phase A: g[p][j] for the lane's components, all 16 points (branch-free: a component with
        //      pi = 0 or a singular covariance has wE = 0 and S = 0, q >= 1500 gives exp -> 0 anyway) ----------
        // four (point, component) pairs per step
        auto eval4 = [&](const int (&pt)[4], auto c_of) {
            double y[4], e[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int c = c_of(k);
                const double a0 = X[pt[k]], a1 = X[FT_P + pt[k]], a2 = X[2 * FT_P + pt[k]];
                if (CHOL) {
                    const double z0 = fma(s02[c], a2, fma(s01[c], a1, fma(s00[c], a0, m0[c])));
                    const double z1 = fma(s12[c], a2, fma(s11[c], a1, m1[c]));
                    const double z2 = fma(s22[c], a2, m2[c]);
                    y[k] = -fma(z2, z2, fma(z1, z1, z0 * z0));
                } else {
                    y[k] = sym3_quad(s00[c], s01[c], s02[c], s11[c], s12[c], s22[c], a0 - m0[c], a1 - m1[c], a2 - m2[c]);
                }
            }
            exp_t11_4<CHOL>(y, e, EXPT);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int c = c_of(k);
                // (a lane's first component always exists when it has two: J16 > FT_BLOCK)
                if ((CPL == 2 && c == 0) || jc[c] < J16) G[(size_t)pt[k] * LDG + jc[c]] = wE[c] * e[k];
            }
        };
        // two pairs of the tail block (one or two of its points, second component)
        auto eval2 = [&](int pa, int pb) {
            constexpr int c = CPL - 1;
            double y[4], e[4];
            const int pt[2] = {pa, pb};
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const double a0 = X[pt[k]], a1 = X[FT_P + pt[k]], a2 = X[2 * FT_P + pt[k]];
                if (CHOL) {
                    const double z0 = fma(s02[c], a2, fma(s01[c], a1, fma(s00[c], a0, m0[c])));
                    const double z1 = fma(s12[c], a2, fma(s11[c], a1, m1[c]));
                    const double z2 = fma(s22[c], a2, m2[c]);
                    y[k] = -fma(z2, z2, fma(z1, z1, z0 * z0));
                } else {
                    y[k] = sym3_quad(s00[c], s01[c], s02[c], s11[c], s12[c], s22[c], a0 - m0[c], a1 - m1[c], a2 - m2[c]);
                }
            }
            y[2] = y[3] = y[1];
            exp_t11_4<CHOL>(y, e, EXPT);
            if (jc[c] < J16) {
                G[(size_t)pa * LDG + jc[c]] = wE[c] * e[0];
                if (pb != pa) G[(size_t)pb * LDG + jc[c]] = wE[c] * e[1];
            }
        };
        // four (point, component) pairs per step, the exponentials in three stages: the four table look-ups are in flight
        // while the polynomials are evaluated (see exp_t11_head; eight per step needs 3 registers more than there are)
        auto eval4s = [&](const int (&pt)[4], auto c_of) {
            ExpHead hd[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int c = c_of(k);
                const double a0 = X[pt[k]], a1 = X[FT_P + pt[k]], a2 = X[2 * FT_P + pt[k]];
                double y;
                if (CHOL) {
                    const double z0 = fma(s02[c], a2, fma(s01[c], a1, fma(s00[c], a0, m0[c])));
                    const double z1 = fma(s12[c], a2, fma(s11[c], a1, m1[c]));
                    const double z2 = fma(s22[c], a2, m2[c]);
                    y = -fma(z2, z2, fma(z1, z1, z0 * z0));
                } else {
                    y = sym3_quad(s00[c], s01[c], s02[c], s11[c], s12[c], s22[c], a0 - m0[c], a1 - m1[c], a2 - m2[c]);
                }
                hd[k] = exp_t11_head<CHOL>(y, EXPT);
            }
            double pa[4];
            exp_t11_poly4(hd[0].r, hd[1].r, hd[2].r, hd[3].r, pa);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int c = c_of(k);
                const double e = exp_t11_tail(hd[k], pa[k]);
                if ((CPL == 2 && c == 0) || jc[c] < J16) G[(size_t)pt[k] * LDG + jc[c]] = wE[c] * e;
            }
        };
        const bool full2 = CPL == 2 && !tail_wave && (w * 64 + FT_BLOCK < J16);     // wave-uniform
        if (full2) {
#pragma unroll 2
            for (int p0 = 0; p0 < FT_P; p0 += 2) {
                const int pt[4] = {p0, p0, p0 + 1, p0 + 1};
                eval4s(pt, [](int k) { return k & 1; });
            }
        } else {
#pragma unroll 2
            for (int p0 = 0; p0 < FT_P; p0 += 4) {
                const int pt[4] = {p0, p0 + 1, p0 + 2, p0 + 3};
                eval4s(pt, [](int) { return 0; });
            }
            if (tail_wave) {                                              // (tail_pts is workgroup-uniform)
                if (tail_pts >= 4) {
                    for (int p0 = 0; p0 < tail_pts; p0 += 4) {
                        const int pt[4] = {tail_p0 + p0, tail_p0 + p0 + 1, tail_p0 + p0 + 2, tail_p0 + p0 + 3};
                        eval4(pt, [](int) { return CPL - 1; });
                    }
                } else if (tail_pts == 2) {
                    eval2(tail_p0, tail_p0 + 1);
                } else {
                    eval2(tail_p0, tail_p0);
                }
            }
        }
        if (tile + 1 < t1) stage(tile + 1, buf ^ 1);     // read two barriers from now, overwritten two barriers after
        FT_TICK(tA);
        __syncthreads();
        FT_TICK(tW);
        // ---- phase B: wave w owns points 2w, 2w + 1 ---------------------------------------------------------
        {
            // half-wave h = lane >> 5 owns point 2 w + h: 32 lanes stride through the row (two 32-lane groups read two
            // rows: conflict-free), one 5-step DPP reduction serves both points (results in lanes 31 and 63).
            // Per 128 columns a lane takes 4 values: row sum, running maximum and -- instead of an index per value --
            // the 128-column step in which its maximum was last raised (strictly: the first such step wins); the step's
            // four values are looked at again afterwards.  9 VALU instructions per 4 values (round 2: ~25).
            const int h = lane >> 5, sub = lane & 31;
            const int p = w * 2 + h;
            const double* Gp = G + (size_t)p * LDG;
            const int J128 = (J16 + 127) & ~127;                       // the row is zero beyond J16
            double den = 0.0, tot = 0.0, best = -1.0;
            int jbest = 0;
            // (requesting the whole row before using any of it -- 16 predicated loads per batch -- was tried and is
            //  slower: 1.05-1.19 M cycles per wave for this phase against 0.80-0.93 M for the plain loop)
            for (int jb = 0; jb < J128; jb += 128) {                   // four 32-column steps at a time, loads first
                double gv[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) gv[u] = Gp[jb + 32 * u + sub];
                const double m4 = fmax(fmax(gv[0], gv[1]), fmax(gv[2], gv[3]));
                den += (gv[0] + gv[1]) + (gv[2] + gv[3]);
                jbest = (m4 > best) ? jb : jbest;
                best = fmax(best, m4);
                if (any_small) {
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int j = jb + 32 * u + sub;
                        tot = fma(gv[u], (j < J16) ? WL[j] : 0.0, tot);
                    }
                }
            }
            // the lane's first column holding its maximum: the first of the step's four values equal to it
            int am;
            {
                const double g0 = Gp[jbest + sub], g1 = Gp[jbest + 32 + sub], g2 = Gp[jbest + 64 + sub];
                am = jbest + sub + ((g0 == best) ? 0 : ((g1 == best) ? 32 : ((g2 == best) ? 64 : 96)));
            }
            double den0, den1, bm0, bm1;
            halfwave_sum_f64(den, den0, den1);
            halfwave_max_f64(best, bm0, bm1);
            const double den_h = h ? den1 : den0, bm_h = h ? bm1 : bm0;
            // first arg-max of the row: the largest value, then the smallest index among its holders
            int c0, c1;
            halfwave_min_i32((best == bm_h) ? am : 0x7fffffff, c0, c1);
            double tot_h = den_h;
            if (any_small) {
                double t0s, t1s;
                halfwave_sum_f64(tot, t0s, t1s);
                tot_h = h ? t1s : t0s;
            }
            const double inv = 1.0 / den_h;
            if (sub == 0) {
                const bool live = base + p < n;
                const bool good = den_h > TREE_EPS;
                INV[p] = (live && good) ? inv : 0.0;
                TOT[buf * FT_P + p] = live ? tot_h : -1.0;             // its log is taken during the next tile's phase A
                if (live) label_out[base + p] = good ? (h ? c1 : c0) : 0;   // all gammas zero -> argmax = 0 (C:178,184)
            }
            if (sub < 16) {
                const double* A = XA + buf * 3 * FT_P;                 // cloud coordinates
                const double x0 = A[p], x1 = A[FT_P + p], x2 = A[2 * FT_P + p];
                double f = 0.0;
                switch (sub) {
                    case 0: f = 1.0; break;
                    case 1: f = x0; break;
                    case 2: f = x1; break;
                    case 3: f = x2; break;
                    case 4: f = x0 * x0; break;
                    case 5: f = x0 * x1; break;
                    case 6: f = x0 * x2; break;
                    case 7: f = x1 * x1; break;
                    case 8: f = x1 * x2; break;
                    case 9: f = x2 * x2; break;
                    default: f = 0.0;
                }
                F[sub * FT_LDF + p] = f;
            }
        }
        FT_TICK(tB);
        __syncthreads();
        FT_TICK(tW);
        // ---- phase C: statistics on the matrix cores ---------------------------------------------------------
        // v_mfma_f64_4x4x4_4b_f64: four independent 4 x 4 x 4 products per instruction.  Operand layout measured with
        // tools/mfma_layout.hip (profiles/r03/mfma_f64_4x4x4_layout.txt): A[b][i][k] in lane i + 4 b + 16 k,
        // B[b][k][j] in lane j + 4 b + 16 k, D[b][i][j] in lane j + 4 b + 16 i.  Block b = components 4 b .. 4 b + 3 of the
        // wave's 16-component tile, i = component, k = point, j = feature: the A operand is read from G exactly as
        // the 16 x 16 x 4 form read it (column 16 ct + (lane & 15), row 4 s + (lane >> 4)) and serves THREE products,
        // one per block of four features -- 10 features cost 12 columns instead of 16: 48 instead of 64 matrix cycles
        // per (tile, four points), and 3 instead of 4 accumulator registers per tile.
        double bfrag[3][4], ifrag[4];
        if (want_stats) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            ifrag[s] = INV[4 * s + b_idx];
#pragma unroll
            for (int fb = 0; fb < 3; ++fb) bfrag[fb][s] = F[(4 * fb + (lane & 3)) * FT_LDF + 4 * s + b_idx];
        }
        // (the next tile's four A values are requested before the current tile's are consumed: round 3's first version
        //  read one value, waited for it, used it -- 28 LDS round trips in a row per wave and phase)
        double araw[2][4];
        auto load_a = [&](int ct, double (&dst)[4]) {
#pragma unroll
            for (int s = 0; s < 4; ++s) dst[s] = G[(size_t)(4 * s + b_idx) * LDG + 16 * ct + a_idx];
        };
        if (w < ntiles) load_a(w, araw[0]);
#pragma unroll
        for (int t = 0; t < MAXT; ++t) {
            const int ct = w + t * FT_WAVES;                           // wave-uniform
            if (ct < ntiles) {
                if (t + 1 < MAXT && ct + FT_WAVES < ntiles) load_a(ct + FT_WAVES, araw[(t + 1) & 1]);
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    // reference: gamma = g / den (C:176); accumulate() drops gamma < eps (C:100)
                    double a = araw[t & 1][s] * ifrag[s];
                    if (a < TREE_EPS) a = 0.0;
#pragma unroll
                    for (int fb = 0; fb < 3; ++fb)
                        acc[t][fb] = __builtin_amdgcn_mfma_f64_4x4x4f64(a, bfrag[fb][s], acc[t][fb], 0, 0, 0);
                }
            }
        }
        }
        FT_TICK(tC);
        __syncthreads();                                               // G is overwritten by the next tile
        FT_TICK(tW);
    }
    if (w == LQ_WAVE && t0 < t1) tile_loglik((int)((t1 - 1 - t0) & 1));      // the last tile's terms
    if (dbg && lane == 0 && blockIdx.x == 7) {
        dbg[w * 4 + 0] = tA; dbg[w * 4 + 1] = tB; dbg[w * 4 + 2] = tC; dbg[w * 4 + 3] = tW;
    }
    // D layout (f64 4x4x4, 4 blocks): lane = j + 4 b + 16 i  ->  component 16 ct + 4 b + i, feature 4 fb + j
#pragma unroll
    for (int t = 0; t < MAXT; ++t) {
        const int ct = w + t * FT_WAVES;
        if (ct < ntiles) {
            const int comp = 16 * ct + 4 * ((lane >> 2) & 3) + (lane >> 4);
#pragma unroll
            for (int fb = 0; fb < 3; ++fb) {
                const int feat = 4 * fb + (lane & 3);
                if (feat < NMOM) partials[((size_t)blockIdx.x * J16 + comp) * NMOM + feat] = acc[t][fb];
            }
        }
    }
    if (w == LQ_WAVE && lane == 0) block_q[blockIdx.x] = lq;
#undef FT_TICK
}

template <int CPL>
__global__ __launch_bounds__(FT_BLOCK) void full_fused_kernel(
    const double* __restrict__ xs, int64_t n, int64_t n_pad, const double* __restrict__ prep, int J16,
    int* __restrict__ label_out, double* __restrict__ block_q, double* __restrict__ partials /*[grid][J16][NMOM]*/,
    int want_stats, const int* __restrict__ flags, const double* __restrict__ exp2_tab,
    long long* __restrict__ dbg = nullptr, const int* __restrict__ done = nullptr) {
    extern __shared__ double lds[];
    if (done && *done) return;                     // the loop stopped in an earlier iteration of this batch
    if (flags && (*flags & 1))                     // kernel-uniform: some Sigma^-1 failed the Cholesky test
        full_fused_body<CPL, false>(xs, n, n_pad, prep, J16, label_out, block_q, partials, want_stats, dbg, lds, exp2_tab);
    else
        full_fused_body<CPL, true>(xs, n, n_pad, prep, J16, label_out, block_q, partials, want_stats, dbg, lds, exp2_tab);
}

// ------------------------------------------------------------------------------------------
// The one-pass E-step with a FLOAT32 TILE (hgmm_tree_set_precision(ctx, HGMM_PRECISION_F32_PDF): the type of the
// reference's GPU file, hgmm/hgmm_gpu.py:472, 478-484 -- float32 points, float32 node and moment arrays; round 6).
// Same three phases on a tile of 16 points, g[p][j] kept in LDS as float (52 KB at J = 800 instead of 117: TWO
// workgroups per CU at <= 128 registers, whose phases run out of step):
//   phase A  a lane's TWO ADJACENT components as one float2: the exponent from head + tail DIFFERENCES
//            d = (x_head - m_head) + (x_tail - m_tail) of coordinates and means relative to the cloud's first point (the
//            cloud is not spatially sorted: the plain float32 difference would carry 6e-8 of the cloud's extent, this
//            carries 6e-8 of |x - mu|), z = R d with R pre-scaled by sqrt(log2 e), 2^(-|z|^2) by v_exp_f32: 21 packed
//            instructions + 2 transcendental per point for two components (float64: 48 + two table exponentials)
//   phase B  row sums, first arg-max, the log-likelihood's row sum: float32 reads, four values per lane and step added in
//            float32, the steps and the lanes in float64; 1 / den and log() in float64
//   phase C  statistics on v_mfma_f32_16x16x4_f32 about the cloud's first point o (features 1, d, d d^T of d = x - o in
//            float32), gamma = g (1 / den) thresholded at eps as in float64.  The accumulators are float32: a workgroup
//            hands them over every FF_SEG tiles (1024 points) as one float partial per segment, and
//            full_reduce_f32_kernel adds the segments in float64 and moves the moments from o to the cloud's own origin.
//            Measured on the reference's kind of data (tools/fullcov_f32_stats_error.py: uniform cube, sigma = 0.03):
//            covariances to 3e-6 of sigma^2 -- the float32 REFERENCE accumulates all N points in float32.
// Triangular form only (a table with a failed factorisation takes the float64 kernel), J16 <= 1024.
// ------------------------------------------------------------------------------------------
constexpr int FF_P = 16, FF_WAVES = 8, FF_BLOCK = FF_WAVES * 64, FF_SEG = 16;
// The origin of the float32 statistics: the cloud's CENTROID (the float32 second moments are accumulated about it and
// moved to the cloud's own frame in float64: their rounding is relative to |x - o|^2, and no point is closer to all
// others).  FF_OPARTS workgroups leave partial coordinate sums; the consumers add them in one fixed order (ff_origin,
// one wave), so the fused kernel and the reduction use the same o bit for bit.
constexpr int FF_OPARTS = 256;
__global__ __launch_bounds__(256) void full_origin_parts_kernel(const double* __restrict__ xs, int64_t n, int64_t n_pad,
                                                                double* __restrict__ parts /*[FF_OPARTS][3]*/) {
    __shared__ double sh[4][3];
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)FF_OPARTS * 256) {
        a0 += xs[i]; a1 += xs[n_pad + i]; a2 += xs[2 * n_pad + i];
    }
    a0 = wave_sum_f64(a0); a1 = wave_sum_f64(a1); a2 = wave_sum_f64(a2);
    if (lane_id() == 0) { sh[wave_in_block()][0] = a0; sh[wave_in_block()][1] = a1; sh[wave_in_block()][2] = a2; }
    __syncthreads();
    if (threadIdx.x < 3) parts[blockIdx.x * 3 + threadIdx.x] = (sh[0][threadIdx.x] + sh[1][threadIdx.x]) + (sh[2][threadIdx.x] + sh[3][threadIdx.x]);
}
// all 64 lanes of ONE wave: the centroid's coordinate d (every lane returns it)
__device__ __forceinline__ double ff_origin(const double* __restrict__ parts, int d, double inv_n) {
    double a = 0.0;
#pragma unroll
    for (int k = 0; k < FF_OPARTS / 64; ++k) a += parts[(lane_id() + 64 * k) * 3 + d];
    return wave_sum_f64(a) * inv_n;
}
__host__ __device__ inline int ff_ld(int J16) {            // floats per point row: == 16 or 48 (mod 64) -> the four rows of an
    int ld = J16 + 16;                                      // A fragment fall into four different 16-bank groups
    while ((ld & 63) != 16 && (ld & 63) != 48) ld += 16;
    return ld;
}
inline size_t ff_lds_bytes(int J16) {
    return sizeof(float) * ((size_t)FF_P * ff_ld(J16) + 16 * FF_P + FF_P + J16 + 2 * 2 * 3 * FF_P * 2) + sizeof(double) * (2 * FF_P + 2);
}

__global__ __launch_bounds__(FF_BLOCK, 4) void full_fused_f32_kernel(
    const double* __restrict__ xs, int64_t n, int64_t n_pad, const double* __restrict__ prep, int J16,
    int* __restrict__ label_out, double* __restrict__ block_q, float* __restrict__ partials /*[segments][J16][NMOM]*/,
    int segs_per_wg, int want_stats, const int* __restrict__ flags, const int* __restrict__ done,
    const double* __restrict__ origin_parts, long long* __restrict__ dbg) {
    extern __shared__ double lds_raw[];
    if (done && *done) return;
    const bool use_chol = !(flags && (*flags & 1));        // kernel-uniform: some Sigma^-1 failed its factorisation -> symmetric form
    long long tA = 0, tB = 0, tC = 0, tW = 0, tm = 0;
#define FF_TICK(acc) do { if (dbg) { const long long now_ = clock64(); acc += now_ - tm; tm = now_; } } while (0)
    const int LD = ff_ld(J16);
    double* TOT = lds_raw;                                  // [2][FF_P] row sums over the components with pi >= eps (-1: dead point)
    float* G = reinterpret_cast<float*>(TOT + 2 * FF_P + 2);      // [FF_P][LD]
    float* F = G + (size_t)FF_P * LD;                       // [FF_P points][16 features]
    float* INV = F + 16 * FF_P;                             // [FF_P] 1 / denominator (0: dead point)
    float* WL = INV + FF_P;                                 // [J16] 1 where pi_j >= eps
    f2t* XH = reinterpret_cast<f2t*>(WL + J16);             // [2][3][FF_P] {v, v}: head of x - o, double-buffered
    f2t* XT = XH + 2 * 3 * FF_P;                            // ... and its tail
    const int w = wave_in_block(), lane = lane_id();
    const int tid = (int)threadIdx.x;
    const int npair = J16 / 2;
    const bool mine = tid < npair;
    // the origin: wave 0 adds the partial sums up, everybody reads the three numbers from LDS (TOT's row 0 is not used
    // before the first tile's phase B, two barriers from here)
    if (tid < 64) {
        const double inv_n = 1.0 / (double)n;
        const double c0 = ff_origin(origin_parts, 0, inv_n), c1 = ff_origin(origin_parts, 1, inv_n), c2 = ff_origin(origin_parts, 2, inv_n);
        if (tid == 0) { TOT[0] = c0; TOT[1] = c1; TOT[2] = c2; }
    }
    __syncthreads();
    const double o0 = TOT[0], o1 = TOT[1], o2 = TOT[2];
    __syncthreads();
    // this lane's two components 2 tid, 2 tid + 1
    f2t r00 = {0.f, 0.f}, r01 = r00, r02 = r00, r11 = r00, r12 = r00, r22 = r00, nh0 = r00, nh1 = r00, nh2 = r00, nt0 = r00,
        nt1 = r00, nt2 = r00, we = r00;
    if (mine) {
        float v[2][13];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const double* pr = prep + PREP_N * (2 * tid + c);
            // triangular form: sqrt(log2 e) R;  symmetric form: (log2 e / 2) Sigma^-1
            const double S = use_chol ? LLF_SQRT_LOG2E : 0.5 * LLF_LOG2E;
            const int fo = use_chol ? PREP_R : 0;
            const double u0 = pr[6] - o0, u1 = pr[7] - o1, u2 = pr[8] - o2;
            v[c][0] = llf_f32(S * pr[fo]); v[c][1] = llf_f32(S * pr[fo + 1]); v[c][2] = llf_f32(S * pr[fo + 2]);
            v[c][3] = llf_f32(S * pr[fo + 3]); v[c][4] = llf_f32(S * pr[fo + 4]); v[c][5] = llf_f32(S * pr[fo + 5]);
            const float h0 = (float)u0, h1 = (float)u1, h2 = (float)u2;
            v[c][6] = -h0; v[c][7] = -h1; v[c][8] = -h2;
            v[c][9] = -(float)(u0 - (double)h0); v[c][10] = -(float)(u1 - (double)h1); v[c][11] = -(float)(u2 - (double)h2);
            v[c][12] = (float)pr[9];
        }
        r00 = f2t{v[0][0], v[1][0]}; r01 = f2t{v[0][1], v[1][1]}; r02 = f2t{v[0][2], v[1][2]};
        r11 = f2t{v[0][3], v[1][3]}; r12 = f2t{v[0][4], v[1][4]}; r22 = f2t{v[0][5], v[1][5]};
        nh0 = f2t{v[0][6], v[1][6]}; nh1 = f2t{v[0][7], v[1][7]}; nh2 = f2t{v[0][8], v[1][8]};
        nt0 = f2t{v[0][9], v[1][9]}; nt1 = f2t{v[0][10], v[1][10]}; nt2 = f2t{v[0][11], v[1][11]};
        we = f2t{v[0][12], v[1][12]};
    }
    int my_small = 0;
    for (int j = tid; j < J16; j += FF_BLOCK) {
        const double wl = prep[PREP_N * j + 10], wev = prep[PREP_N * j + 9];
        WL[j] = (wl != 0.0) ? 1.f : 0.f;
        if (wl == 0.0 && wev != 0.0) my_small = 1;
    }
    for (int e = tid; e < FF_P * LD; e += FF_BLOCK) G[e] = 0.f;
    const bool any_small = __syncthreads_or(my_small) != 0;
    const int ntiles = J16 / 16;
    constexpr int MAXT = (FT_MAX_J16 / 16 + FF_WAVES - 1) / FF_WAVES;      // 8
    f4t acc[MAXT];
#pragma unroll
    for (int t = 0; t < MAXT; ++t) acc[t] = f4t{0.f, 0.f, 0.f, 0.f};
    const int a_idx = lane & 15, b_idx = lane >> 4;

    const int64_t tiles = (n + FF_P - 1) / FF_P;
    const int64_t per = (int64_t)segs_per_wg * FF_SEG;
    const int64_t t0 = (int64_t)blockIdx.x * per;
    const int64_t t1 = (t0 + per < tiles) ? t0 + per : tiles;
    constexpr int LQ_WAVE = 7;                             // (the wave with the fewest components at J = 800)
    double lq = 0.0;
    const int st_d = tid / FF_P, st_p = tid % FF_P;
    const double st_o = st_d == 0 ? o0 : (st_d == 1 ? o1 : o2);
    auto stage = [&](int64_t tile, int buf) {
        if (tid < 3 * FF_P) {
            int64_t i = tile * FF_P + st_p;
            i = i < n ? i : n - 1;
            const double dv = xs[(size_t)st_d * n_pad + i] - st_o;
            const float h = (float)dv, tl = (float)(dv - (double)h);
            XH[(buf * 3 + st_d) * FF_P + st_p] = f2t{h, h};
            XT[(buf * 3 + st_d) * FF_P + st_p] = f2t{tl, tl};
        }
    };
    auto tile_loglik = [&](int par) {
        const double tv = (lane < FF_P) ? TOT[par * FF_P + lane] : -1.0;
        double term = (tv >= 0.0) ? log_pos_f64(fmax(tv, TREE_EPS)) : 0.0;
        term = wave_sum_f64(term);
        lq += term;
    };
    auto flush = [&](int64_t seg) {                        // the wave's accumulator tiles -> the segment's float partial
        // (the segment index is made opaque: otherwise the eight tiles' addresses are formed ahead of the tile loop and kept
        //  in registers through it -- 199 registers instead of 86)
        int seg_lo = (int)seg;
        asm volatile("" : "+s"(seg_lo));
        seg = seg_lo;
#pragma unroll
        for (int t = 0; t < MAXT; ++t) {
            const int ct = w + t * FF_WAVES;
            if (ct < ntiles) {
                if (a_idx < NMOM) {
                    // D layout (f32 16x16x4): row (component) = 4 (lane >> 4) + r, column (feature) = lane & 15
                    float* dst = partials + ((size_t)seg * J16 + 16 * ct + 4 * b_idx) * NMOM + a_idx;
                    dst[0] = acc[t].x; dst[NMOM] = acc[t].y; dst[2 * NMOM] = acc[t].z; dst[3 * NMOM] = acc[t].w;
                }
                acc[t] = f4t{0.f, 0.f, 0.f, 0.f};
            }
        }
    };
    if (t0 < t1) stage(t0, 0);
    __syncthreads();
    for (int64_t seg0 = t0; seg0 < t1; seg0 += FF_SEG) {
    const int64_t seg1 = (seg0 + FF_SEG < t1) ? seg0 + FF_SEG : t1;
    for (int64_t tile = seg0; tile < seg1; ++tile) {
        const int64_t base = tile * FF_P;
        const int buf = (int)((tile - t0) & 1);
        if (dbg) tm = clock64();
        if (w == LQ_WAVE && tile > t0) tile_loglik(buf ^ 1);
        // ---- phase A ----------------------------------------------------------------------------------------------
        if (mine) {
            const f2t* xh = XH + buf * 3 * FF_P;
            const f2t* xt = XT + buf * 3 * FF_P;
#pragma unroll 4
            for (int p = 0; p < FF_P; ++p) {
                const f2t d0 = (xh[p] + nh0) + (xt[p] + nt0);
                const f2t d1 = (xh[FF_P + p] + nh1) + (xt[FF_P + p] + nt1);
                const f2t d2 = (xh[2 * FF_P + p] + nh2) + (xt[2 * FF_P + p] + nt2);
                f2t q;
                if (use_chol) {
                    const f2t z0 = llf_fma(r02, d2, llf_fma(r01, d1, r00 * d0));
                    const f2t z1 = llf_fma(r12, d2, r11 * d1);
                    const f2t z2 = r22 * d2;
                    q = llf_fma(z2, z2, llf_fma(z1, z1, z0 * z0));
                } else {
                    const f2t t0 = llf_fma(llf_bc(2.f), llf_fma(r02, d2, r01 * d1), r00 * d0);
                    const f2t t1 = llf_fma(llf_bc(2.f), r12 * d2, r11 * d1);
                    q = llf_fma(d2, r22 * d2, llf_fma(d1, t1, d0 * t0));
                }
                const f2t e = f2t{__builtin_amdgcn_exp2f(-q.x), __builtin_amdgcn_exp2f(-q.y)};
                *reinterpret_cast<f2t*>(G + (size_t)p * LD + 2 * tid) = we * e;
            }
        }
        if (tile + 1 < t1) stage(tile + 1, buf ^ 1);
        FF_TICK(tA);
        __syncthreads();
        FF_TICK(tW);
        // ---- phase B: wave w owns points 2 w, 2 w + 1 (one per half-wave) ---------------------------------------------
        {
            const int h = lane >> 5, sub = lane & 31;
            const int p = w * 2 + h;
            const float* Gp = G + (size_t)p * LD;
            const int J128 = (J16 + 127) & ~127;                       // (the row is zero beyond J16: LD >= J16 + 16 ... see below)
            double den = 0.0, tot = 0.0;
            float best = -1.f;
            int jbest = 0;
            for (int jb = 0; jb < J128; jb += 128) {
                const int j = jb + 4 * sub;
                f4t gv = f4t{0.f, 0.f, 0.f, 0.f};
                if (j < J16) gv = *reinterpret_cast<const f4t*>(Gp + j);
                const float m4 = fmaxf(fmaxf(gv.x, gv.y), fmaxf(gv.z, gv.w));
                den += (double)((gv.x + gv.y) + (gv.z + gv.w));
                jbest = (m4 > best) ? j : jbest;
                best = fmaxf(best, m4);
                if (any_small && j < J16) {
                    const f4t wl = *reinterpret_cast<const f4t*>(WL + j);
                    tot += (double)((gv.x * wl.x + gv.y * wl.y) + (gv.z * wl.z + gv.w * wl.w));
                }
            }
            int am;
            {
                const f4t gv = *reinterpret_cast<const f4t*>(Gp + jbest);
                am = jbest + ((gv.x == best) ? 0 : ((gv.y == best) ? 1 : ((gv.z == best) ? 2 : 3)));
            }
            double den0, den1, bm0, bm1;
            halfwave_sum_f64(den, den0, den1);
            halfwave_max_f64((double)best, bm0, bm1);
            const double den_h = h ? den1 : den0;
            const float bm_h = (float)(h ? bm1 : bm0);
            int c0, c1;
            halfwave_min_i32((best == bm_h) ? am : 0x7fffffff, c0, c1);
            double tot_h = den_h;
            if (any_small) {
                double t0s, t1s;
                halfwave_sum_f64(tot, t0s, t1s);
                tot_h = h ? t1s : t0s;
            }
            const double inv = 1.0 / den_h;
            if (sub == 0) {
                const bool live = base + p < n;
                const bool good = den_h > TREE_EPS;
                INV[p] = (live && good) ? (float)inv : 0.f;
                TOT[buf * FF_P + p] = live ? tot_h : -1.0;
                if (live) label_out[base + p] = good ? (h ? c1 : c0) : 0;
            }
            if (sub < 16) {
                const f2t* xh = XH + buf * 3 * FF_P;
                const float x0 = xh[p].x, x1 = xh[FF_P + p].x, x2 = xh[2 * FF_P + p].x;
                float f = 0.f;
                switch (sub) {
                    case 0: f = 1.f; break;
                    case 1: f = x0; break;
                    case 2: f = x1; break;
                    case 3: f = x2; break;
                    case 4: f = x0 * x0; break;
                    case 5: f = x0 * x1; break;
                    case 6: f = x0 * x2; break;
                    case 7: f = x1 * x1; break;
                    case 8: f = x1 * x2; break;
                    case 9: f = x2 * x2; break;
                    default: f = 0.f;
                }
                F[p * 16 + sub] = f;
            }
        }
        FF_TICK(tB);
        __syncthreads();
        FF_TICK(tW);
        // ---- phase C: v_mfma_f32_16x16x4_f32, A[i][k] in lane i + 16 k, B[k][j] in lane j + 16 k ----------------------
        if (want_stats) {
            float bfrag[4], ifrag[4];
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                ifrag[s] = INV[4 * s + b_idx];
                bfrag[s] = F[(4 * s + b_idx) * 16 + a_idx];
            }
            // (the next tile's four A values are requested before the current tile's are consumed; the fences keep the
            //  compiler from requesting ALL tiles' values at once -- 168 registers instead of 84 for the rest of the kernel)
            float araw[2][4];
            const int row_off = b_idx * LD + a_idx, srow = 4 * LD;
            auto load_a = [&](int ct, float (&dst)[4]) {
                // (the tile's offset is made opaque: left alone the compiler forms all 28 addresses ahead of the loop, spills
                //  them and reloads four per tile from scratch)
                int off = row_off + 16 * ct;
                asm volatile("" : "+v"(off));
#pragma unroll
                for (int s = 0; s < 4; ++s) dst[s] = G[off + s * srow];
            };
            if (w < ntiles) load_a(w, araw[0]);
#pragma unroll
            for (int t = 0; t < MAXT; ++t) {
                const int ct = w + t * FF_WAVES;                       // wave-uniform
                if (ct < ntiles) {
                    if (t + 1 < MAXT && ct + FF_WAVES < ntiles) load_a(ct + FF_WAVES, araw[(t + 1) & 1]);
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        float a = araw[t & 1][s] * ifrag[s];
                        if (a < 1.0e-15f) a = 0.f;                     // accumulate() drops gamma < eps (C:100)
                        acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bfrag[s], acc[t], 0, 0, 0);
                    }
                    asm volatile("" ::: "memory");
                }
            }
        }
        FF_TICK(tC);
        __syncthreads();                                               // G is overwritten by the next tile
        FF_TICK(tW);
    }
    if (want_stats) flush((int64_t)blockIdx.x * segs_per_wg + (seg0 - t0) / FF_SEG);
    }
    if (w == LQ_WAVE && t0 < t1) tile_loglik((int)((t1 - 1 - t0) & 1));
    if (dbg && lane == 0 && blockIdx.x == 7) {
        dbg[w * 4 + 0] = tA; dbg[w * 4 + 1] = tB; dbg[w * 4 + 2] = tC; dbg[w * 4 + 3] = tW;
    }
    if (w == LQ_WAVE && lane == 0) block_q[blockIdx.x] = lq;
#undef FF_TICK
}

// The segments' float partials -> float64 moments, in two fixed-order stages (one wave per component walking all ~4000
// segments was 350 us -- strided 40-byte reads; this is ~35):
//   stage 1  FF_RB workgroups; workgroup b adds segments b, b + FF_RB, ... element by element in float64 (coalesced reads
//            of whole [J16][NMOM] rows) -> part64 [FF_RB][J16 NMOM]
//   stage 2  one wave per component: lane = 16 slice + feature, slice s adds blocks s, s + 4, ...; then the moments are
//            moved from the centroid o to the cloud's own origin: M1 = M1' + o M0, M2 = M2' + o M1'^T + M1' o^T + o o^T M0
constexpr int FF_RB = 128;
__global__ __launch_bounds__(256) void full_reduce_f32_stage1_kernel(const float* __restrict__ partials, int nseg,
                                                                     int segs_per_wg, int64_t tiles, int J16,
                                                                     double* __restrict__ part64,
                                                                     const int* __restrict__ done = nullptr) {
    // grid = (element chunks of 1024, FF_RB): a thread owns four consecutive elements (one 16-byte load per segment)
    if (done && *done) return;
    const int E = J16 * NMOM;                                          // a multiple of 4 (J16 is one of 16)
    const int e = ((int)blockIdx.x * 256 + (int)threadIdx.x) * 4;
    if (e >= E) return;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    for (int sgm = blockIdx.y; sgm < nseg; sgm += FF_RB) {
        // (segment s = the (s mod segs_per_wg)-th of workgroup s / segs_per_wg; a workgroup's segments beyond the cloud's
        //  last tile were never written)
        const int64_t first_tile = ((int64_t)(sgm / segs_per_wg) * segs_per_wg + sgm % segs_per_wg) * FF_SEG;
        if (first_tile >= tiles) continue;
        const f4t v = *reinterpret_cast<const f4t*>(partials + (size_t)sgm * E + e);
        a0 += (double)v.x; a1 += (double)v.y; a2 += (double)v.z; a3 += (double)v.w;
    }
    double* dst = part64 + (size_t)blockIdx.y * E + e;
    dst[0] = a0; dst[1] = a1; dst[2] = a2; dst[3] = a3;
}
__global__ __launch_bounds__(64) void full_reduce_f32_kernel(const double* __restrict__ part64, int J, int J16,
                                                             const double* __restrict__ origin_parts, int64_t n,
                                                             double* __restrict__ mom,
                                                             const int* __restrict__ done = nullptr) {
    const int j = blockIdx.x;
    if (j >= J) return;
    if (done && *done) return;
    __shared__ double sh[4][16];
    const double inv_n = 1.0 / (double)n;
    const double oc0 = ff_origin(origin_parts, 0, inv_n), oc1 = ff_origin(origin_parts, 1, inv_n), oc2 = ff_origin(origin_parts, 2, inv_n);
    const int feat = (int)threadIdx.x & 15, slice = (int)threadIdx.x >> 4;
    double a = 0.0;
    if (feat < NMOM)
        for (int b = slice; b < FF_RB; b += 4) a += part64[((size_t)b * J16 + j) * NMOM + feat];
    sh[slice][feat] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        double m[NMOM];
#pragma unroll
        for (int f = 0; f < NMOM; ++f) m[f] = (sh[0][f] + sh[1][f]) + (sh[2][f] + sh[3][f]);
        const double o[3] = {oc0, oc1, oc2};
        const double m0 = m[0], d[3] = {m[1], m[2], m[3]};
        double* dst = mom + (size_t)j * NMOM;
        dst[0] = m0;
        for (int k = 0; k < 3; ++k) dst[1 + k] = d[k] + o[k] * m0;
        const int ia[6] = {0, 0, 0, 1, 1, 2}, ib[6] = {0, 1, 2, 1, 2, 2};
        for (int k = 0; k < 6; ++k) {
            const int r = ia[k], c2 = ib[k];
            dst[4 + k] = m[4 + k] + o[r] * d[c2] + d[r] * o[c2] + o[r] * o[c2] * m0;
        }
    }
}

// one wave per component: fixed-order sum over the workgroups' partials
__global__ __launch_bounds__(64) void full_reduce_kernel(const double* __restrict__ partials, int nblocks,
                                                         int J, int J16, double* __restrict__ mom,
                                                         const int* __restrict__ done = nullptr) {
    const int j = blockIdx.x;
    if (j >= J) return;
    if (done && *done) return;
    double acc[NMOM];
#pragma unroll
    for (int m = 0; m < NMOM; ++m) acc[m] = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += 64) {
        const double* src = partials + ((size_t)b * J16 + j) * NMOM;
#pragma unroll
        for (int m = 0; m < NMOM; ++m) acc[m] += src[m];
    }
#pragma unroll
    for (int m = 0; m < NMOM; ++m) {
        const double v = wave_sum_f64(acc[m]);
        if (threadIdx.x == 0) mom[(size_t)j * NMOM + m] = v;
    }
}

__global__ void full_init_nodes_kernel(const double* __restrict__ init_mu, double sig2, int J, int J16,
                                       double* pi, double* mu, double* cov) {
    // pi = 1/J (n_node = J), mu = given, cov = sig2 I; padding components get pi = 0
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= J16) return;
    pi[j] = (j < J) ? 1.0 / (double)J : 0.0;
    for (int d = 0; d < 3; ++d) mu[3 * j + d] = (j < J) ? init_mu[3 * j + d] : 0.0;
    for (int e = 0; e < 9; ++e) cov[9 * j + e] = (e % 4 == 0) ? ((j < J) ? sig2 : 1.0) : 0.0;
}

}  // namespace hgmm

static int fullcov_alloc(hgmm_ctx* c, int J, int* J16_out, int* grid_out) {
    const int J16 = (J + 15) / 16 * 16;
    *J16_out = J16;
    const int64_t groups = (c->n + 63) / 64;
    int64_t grid = (groups + FULL_WAVES - 1) / FULL_WAVES;
    if (grid > 4 * c->cus) grid = 4 * c->cus;
    if (grid < 1) grid = 1;
    *grid_out = (int)grid;
    HGMM_TRY(ensure(c, c->t_pi, sizeof(double) * J16));
    HGMM_TRY(ensure(c, c->t_mu, sizeof(double) * 3 * J16));
    HGMM_TRY(ensure(c, c->t_cov, sizeof(double) * 9 * J16));
    HGMM_TRY(ensure(c, c->t_prep, sizeof(double) * PREP_N * J16));
    HGMM_TRY(ensure(c, c->t_mom, sizeof(double) * NMOM * J16));
    const size_t pblocks = std::max<size_t>((size_t)grid, (size_t)c->cus * 2);          // (the one-pass kernels: <= 2 workgroups per CU)
    HGMM_TRY(ensure(c, c->t_partials, sizeof(double) * pblocks * J16 * NMOM));
    HGMM_TRY(ensure(c, c->t_q, sizeof(double) * (nblk(c->n, CH) + 2 * c->cus + 8)));      // per-workgroup q (<= 2 per CU) + the sum
    HGMM_TRY(ensure(c, c->t_current, sizeof(int) * 2 * c->n_pad));
    HGMM_TRY(ensure(c, c->t_parent, sizeof(double) * c->n_pad));     // den
    HGMM_TRY(tree_flags(c, true));
    c->tree.nodes_ready = false;
    return HGMM_OK;
}

static int fullcov_moments(hgmm_ctx* c, int J, int J16, int grid) {
    {
        ProfScope prof(c, HGMM_K_FULL_MOMENTS);
        full_moments_kernel<<<grid, FULL_BLOCK, 0, c->stream>>>(c->x_soa64.as<double>(), c->n, c->n_pad, c->t_prep.as<double>(),
                                                       J16, c->t_parent.as<double>(), c->t_partials.as<double>());
    }
    full_reduce_kernel<<<J, 64, 0, c->stream>>>(c->t_partials.as<double>(), grid, J, J16, c->t_mom.as<double>());
    HGMM_HIP(c, hipGetLastError());
    if (c->comm_on()) HGMM_TRY(allreduce_f64_dev(c, c->t_mom.as<double>(), (size_t)NMOM * J));
    return HGMM_OK;
}

// one-pass E-step (J16 <= FT_MAX_J16): denominators, arg-max, q and the statistics from ONE evaluation of the pdfs
static bool fullcov_one_pass(const hgmm_ctx* c, int J16) {
    if (c->cfg[CFG_FULLCOV_TWO_PASS]) return false;
    return J16 <= FT_MAX_J16;
}
// `ctl` (device): the launches look at ctl->done first and the sum of q applies the stop rule `stop` -- for a loop whose
// iterations are enqueued ahead of the host's knowledge (hgmm_fullcov_fit); then nothing is copied to the host here.
static int fullcov_fused(hgmm_ctx* c, int J, int J16, int* labels, double* q_host, bool want_stats = true,
                         const int* done = nullptr, TreeStop stop = TreeStop{nullptr, 0.0, 0, nullptr, 0}) {
    const int64_t tiles = (c->n + FT_P - 1) / FT_P;
    const int grid = (int)std::min<int64_t>(tiles, c->cus);             // 100+ KB of LDS: one workgroup per CU
    double* block_q = c->t_q.as<double>();
    double* q_dev = block_q + nblk(c->n, CH) + 2 * c->cus;                // (the loop's q lives here whichever kernel runs)
    if (c->tree.pdf_f32) {
        // float32 tile (hgmm_tree_set_precision): two workgroups per CU, float partials per segment of FF_SEG tiles
        const int64_t tiles16 = (c->n + FF_P - 1) / FF_P;
        const int want_wgs = 2 * c->cus;
        const int segs_per_wg = (int)std::max<int64_t>(1, ((tiles16 + want_wgs - 1) / want_wgs + FF_SEG - 1) / FF_SEG);
        const int grid32 = (int)((tiles16 + (int64_t)segs_per_wg * FF_SEG - 1) / ((int64_t)segs_per_wg * FF_SEG));
        const int nseg = grid32 * segs_per_wg;
        // [segments][J16][NMOM] floats, then stage 1's [FF_RB][J16][NMOM] doubles (8-byte aligned: an even number of floats)
        HGMM_TRY(ensure(c, c->t_partials, sizeof(float) * (size_t)nseg * J16 * NMOM + sizeof(double) * (size_t)FF_RB * J16 * NMOM + 8));
        // (grid32 <= 2 CUs: the workgroups' shares of q fit in front of q_dev, where hgmm_fullcov_fit's loop expects it)
        const size_t lds32 = ff_lds_bytes(J16);
        HGMM_TRY(ensure(c, c->ff_origin, sizeof(double) * 3 * FF_OPARTS));
        double* oparts = c->ff_origin.as<double>();
        full_origin_parts_kernel<<<FF_OPARTS, 256, 0, c->stream>>>(c->x_soa64.as<double>(), c->n, c->n_pad, oparts);
        {
            ProfScope prof(c, HGMM_K_FULL_FUSED);
            HGMM_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&full_fused_f32_kernel),
                                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds32));
            full_fused_f32_kernel<<<grid32, FF_BLOCK, lds32, c->stream>>>(c->x_soa64.as<double>(), c->n, c->n_pad,
                                                                         c->t_prep.as<double>(), J16, labels, block_q,
                                                                         c->t_partials.as<float>(), segs_per_wg,
                                                                         want_stats ? 1 : 0, flags_ptr(c), done, oparts,
                                                                         c->ff_clocks_on ? c->ff_clocks.as<long long>() : nullptr);
        }
        HGMM_HIP(c, hipGetLastError());
        if (want_stats) {
            double* part64 = reinterpret_cast<double*>(c->t_partials.as<float>() + (size_t)nseg * J16 * NMOM);
            full_reduce_f32_stage1_kernel<<<dim3(nblk((int64_t)J16 * NMOM, 1024), FF_RB), 256, 0, c->stream>>>(
                c->t_partials.as<float>(), nseg, segs_per_wg, tiles16, J16, part64, done);
            full_reduce_f32_kernel<<<J, 64, 0, c->stream>>>(part64, J, J16, oparts, c->n, c->t_mom.as<double>(), done);
        }
        tree_sum_kernel<<<1, 256, 0, c->stream>>>(block_q, grid32, q_dev, done, stop);
        HGMM_HIP(c, hipGetLastError());
        if (c->comm_on()) {
            HGMM_TRY(allreduce_f64_dev(c, c->t_mom.as<double>(), (size_t)NMOM * J));
            HGMM_TRY(allreduce_f64_dev(c, q_dev, 1));
        }
        if (q_host) {
            HGMM_HIP(c, hipMemcpyAsync(q_host, q_dev, sizeof(double), hipMemcpyDeviceToHost, c->stream));
            HGMM_HIP(c, ctx_stream_sync(c));
        }
        return HGMM_OK;
    }
    const size_t lds = ft_lds_bytes(J16);
    HGMM_TRY(ensure_exp_tab2(c));
    // (a 16-wave form of this kernel -- 1024 threads, one component per lane, 128 registers -- was built and measured in
    //  round 3: 1.83 vs 1.76 ms, phase A no shorter with four waves per SIMD than with two; removed again, commit b7f6218,
    //  profiles/r03/fullcov_accounting.md.  Round 4: four-wave workgroups on 8-point tiles, TWO workgroups per CU so that
    //  the two waves of a SIMD run out of step -- up to 4 components per lane, 13 statistics tiles per wave: parity green,
    //  2.04 ms against 1.73; it needs 281 registers where two waves per SIMD leave 256 (40 spilled), phase B is a latency
    //  chain per TILE, not per point (3.5 k cycles per 8-point tile against 3.2 k per 16-point tile), phase C 6.1 k per
    //  8 points against 4.5 k per 16; removed again, commit 875bec9, profiles/r04/fullcov_accounting_r04.md)
    {
        ProfScope prof(c, HGMM_K_FULL_FUSED);
        if (J16 <= FT_BLOCK) {
            HGMM_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&full_fused_kernel<1>),
                                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            full_fused_kernel<1><<<grid, FT_BLOCK, lds, c->stream>>>(c->x_soa64.as<double>(), c->n, c->n_pad,
                                                                   c->t_prep.as<double>(), J16, labels, block_q,
                                                                   c->t_partials.as<double>(), want_stats ? 1 : 0,
                                                                   flags_ptr(c), c->exp_tab2.as<double>(), nullptr, done);
        } else {
            HGMM_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&full_fused_kernel<2>),
                                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            // (last kernel argument: phase clocks per wave, a debugging aid that is off)
            full_fused_kernel<2><<<grid, FT_BLOCK, lds, c->stream>>>(c->x_soa64.as<double>(), c->n, c->n_pad,
                                                                   c->t_prep.as<double>(), J16, labels, block_q,
                                                                   c->t_partials.as<double>(), want_stats ? 1 : 0,
                                                                   flags_ptr(c), c->exp_tab2.as<double>(),
                                                                   c->ff_clocks_on ? c->ff_clocks.as<long long>() : nullptr, done);
        }
    }
    HGMM_HIP(c, hipGetLastError());
    // (the statistics before the sum: the sum may set the stop flag, and a loop that stops still wants THIS launch's q --
    //  its statistics are not needed any more, but the reduction has looked at the flag before it is raised)
    if (want_stats)
        full_reduce_kernel<<<J, 64, 0, c->stream>>>(c->t_partials.as<double>(), grid, J, J16, c->t_mom.as<double>(), done);
    tree_sum_kernel<<<1, 256, 0, c->stream>>>(block_q, grid, q_dev, done, stop);
    HGMM_HIP(c, hipGetLastError());
    if (c->comm_on()) {
        HGMM_TRY(allreduce_f64_dev(c, c->t_mom.as<double>(), (size_t)NMOM * J));
        HGMM_TRY(allreduce_f64_dev(c, q_dev, 1));
    }
    if (q_host) {
        HGMM_HIP(c, hipMemcpyAsync(q_host, q_dev, sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HGMM_HIP(c, ctx_stream_sync(c));
    }
    return HGMM_OK;
}

static int fullcov_pass(hgmm_ctx* c, int J, int* labels, double* q_host) {
    double* block_q = c->t_q.as<double>();
    double* q_dev = block_q + nblk(c->n, CH);
    {
        ProfScope prof(c, HGMM_K_FULL_PASS);
        full_pass_kernel<<<nblk(c->n, CH), CH, 0, c->stream>>>(c->x_soa64.as<double>(), c->n, c->n_pad,
                                                             c->t_prep.as<double>(), J, c->t_parent.as<double>(),
                                                             labels, block_q);
    }
    tree_sum_kernel<<<1, 256, 0, c->stream>>>(block_q, (int)nblk(c->n, CH), q_dev);
    HGMM_HIP(c, hipGetLastError());
    if (c->comm_on()) HGMM_TRY(allreduce_f64_dev(c, q_dev, 1));
    if (q_host) {
        HGMM_HIP(c, hipMemcpyAsync(q_host, q_dev, sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HGMM_HIP(c, ctx_stream_sync(c));
    }
    return HGMM_OK;
}

extern "C" int hgmm_fullcov_fit(hgmm_ctx* c, int J, double ls, double ld, const double* init_mu, double sig2,
                                int max_iters, double* pi_out, double* mu_out, double* cov_out,
                                int32_t* labels_out, double* q_trace_out, int q_capacity, int* q_len_out) {
    HGMM_ENTER(c);
    if (!c->have_f64 || c->n <= 0) return fail(c, HGMM_ERR_STATE, "full-covariance fit: set points first");
    if (J < 1 || J > 4096) return fail(c, HGMM_ERR_ARG, "J = %d outside 1..4096", J);
    if (!init_mu) return fail(c, HGMM_ERR_ARG, "init_mu is NULL");
    if (max_iters < 1) max_iters = 1;
    HGMM_HIP(c, hipSetDevice(c->device));
    int J16 = 0, grid = 0;
    HGMM_TRY(fullcov_alloc(c, J, &J16, &grid));
    HGMM_TRY(ensure(c, c->scratch, sizeof(double) * 3 * J16));
    double* d_pi = c->t_pi.as<double>();
    double* d_mu = c->t_mu.as<double>();
    double* d_cov = c->t_cov.as<double>();
    double* d_prep = c->t_prep.as<double>();
    int* lab_a = c->t_current.as<int>();
    int* lab_b = lab_a + c->n_pad;
    HGMM_HIP(c, hipMemcpyAsync(c->scratch.p, init_mu, sizeof(double) * 3 * J, hipMemcpyHostToDevice, c->stream));
    full_init_nodes_kernel<<<nblk(J16, 256), 256, 0, c->stream>>>(c->scratch.as<double>(), sig2, J, J16, d_pi, d_mu, d_cov);
    tree_prep_kernel<<<nblk(J16, 256), 256, 0, c->stream>>>(d_pi, d_mu, d_cov, 0, J16, d_prep, flags_ptr(c));
    double n_total = (double)c->n;
    if (c->comm_on()) HGMM_TRY(hgmm_comm_allreduce_f64(c, &n_total, 1, 0));
    // E-step quantities of the initial parameters
    const bool one_pass = fullcov_one_pass(c, J16);
    if (one_pass) HGMM_TRY(fullcov_fused(c, J, J16, lab_a, nullptr));
    else HGMM_TRY(fullcov_pass(c, J, lab_a, nullptr));
    int* lab_cur = lab_a;      // arg-max of the most recent E-step
    int* lab_nxt = lab_b;
    double prev_q = 0.0;
    int it = 0, q_len = 0;
    if (one_pass && !c->comm_on()) {
        // The stop rule on the device, the host one batch of iterations ahead (the scheme of hgmm_tree_build): the
        // launches of an iteration look at ctl->done first, the sum of q applies |q - prev_q| < ls / the budget, and the
        // host reads {done, iterations} through a pinned copy + an event while the next batch is already queued.
        // (Waiting for q after every iteration left the device idle for ~0.1 ms per 1.7 ms iteration at N = 1e6.)
        double* q_dev = c->t_q.as<double>() + nblk(c->n, CH) + 2 * c->cus;
        TreeCtl* ctl = reinterpret_cast<TreeCtl*>(q_dev + 2);
        const int trace_cap = std::min(max_iters, 1 << 20);
        HGMM_TRY(ensure(c, c->t_qtrace, sizeof(double) * (size_t)trace_cap));
        double* trace_dev = c->t_qtrace.as<double>();
        HGMM_HIP(c, hipMemsetAsync(ctl, 0, sizeof(TreeCtl), c->stream));
        const TreeStop stop{ctl, ls, max_iters, trace_dev, trace_cap};
        TreeCtl* hp = nullptr;
        HGMM_TRY(tree_host_ctl(c, &hp));
        const int batch = 4;
        int enq = 0, slot = 0, rc = HGMM_OK;
        auto enqueue_batch = [&](int s) -> int {
            const int cnt = std::min(batch, max_iters - enq);
            for (int b = 0; b < cnt; ++b) {
                const int k = enq + b;                         // iteration k: labels into buffer (k + 1) & 1
                tree_mstep_kernel<<<nblk(J, 256), 256, 0, c->stream>>>(c->t_mom.as<double>(), 0, J, n_total, ld, d_pi, d_mu,
                                                                       d_cov, d_prep, flags_ptr(c), &ctl->done);
                const int r = fullcov_fused(c, J, J16, ((k + 1) & 1) ? lab_b : lab_a, nullptr, k + 1 < max_iters,
                                            &ctl->done, stop);
                if (r != HGMM_OK) return r;
            }
            enq += cnt;
            if (hipMemcpyAsync(&hp[s], ctl, sizeof(TreeCtl), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
                hipEventRecord(c->tree_ev[s], c->stream) != hipSuccess)
                return fail(c, HGMM_ERR_HIP, "full-covariance fit: device error: %s", hipGetErrorString(hipGetLastError()));
            return HGMM_OK;
        };
        rc = enqueue_batch(slot);
        while (rc == HGMM_OK) {
            const bool ahead = enq < max_iters;
            if (ahead) rc = enqueue_batch(slot ^ 1);
            if (rc != HGMM_OK) break;
            if (hipEventSynchronize(c->tree_ev[slot]) != hipSuccess) {
                rc = fail(c, HGMM_ERR_HIP, "full-covariance fit: device error: %s", hipGetErrorString(hipGetLastError()));
                break;
            }
            it = hp[slot].it;
            if (hp[slot].done != 0) break;
            if (!ahead) { rc = fail(c, HGMM_ERR_STATE, "full-covariance fit did not stop within its budget"); break; }
            slot ^= 1;
        }
        HGMM_TRY(rc);
        q_len = it;
        lab_cur = ((it - 1) & 1) ? lab_b : lab_a;              // the arg-max of the E-step whose statistics the last M-step took
        if (q_trace_out && q_len > 0)
            HGMM_HIP(c, hipMemcpyAsync(q_trace_out, trace_dev, sizeof(double) * std::min(std::min(q_len, q_capacity), trace_cap),
                                       hipMemcpyDeviceToHost, c->stream));
    } else
    while (true) {
        if (!one_pass) HGMM_TRY(fullcov_moments(c, J, J16, grid));                    // E (moments)
        tree_mstep_kernel<<<nblk(J, 256), 256, 0, c->stream>>>(c->t_mom.as<double>(), 0, J, n_total, ld, d_pi, d_mu,
                                                               d_cov, d_prep, flags_ptr(c));    // M (+ prep)
        double q = 0.0;
        // q of the new parameters; one pass: the same launch already holds the next iteration's statistics
        // (the statistics of a call that is known to be the last one -- iteration budget reached -- are not formed)
        if (one_pass) HGMM_TRY(fullcov_fused(c, J, J16, lab_nxt, &q, it + 1 < max_iters));
        else HGMM_TRY(fullcov_pass(c, J, lab_nxt, &q));                               // q (+ next E-step's den)
        ++it;
        if (q_trace_out && q_len < q_capacity) q_trace_out[q_len] = q;
        ++q_len;
        if (fabs(q - prev_q) < ls || it >= max_iters) break;
        prev_q = q;
        int* t = lab_cur; lab_cur = lab_nxt; lab_nxt = t;
    }
    {
        StagedDownloads dl(c);
        dl.add(labels_out, lab_cur, sizeof(int) * c->n);
        dl.add(pi_out, d_pi, sizeof(double) * J);
        dl.add(mu_out, d_mu, sizeof(double) * 3 * J);
        dl.add(cov_out, d_cov, sizeof(double) * 9 * J);
        HGMM_HIP(c, dl.finish());
    }
    if (q_len_out) *q_len_out = q_len < q_capacity ? q_len : q_capacity;
    return HGMM_OK;
}

extern "C" int hgmm_fullcov_phase_clocks(hgmm_ctx* c, int enable, int64_t* clocks_out) {
    HGMM_ENTER(c);
    if (enable) {
        HGMM_TRY(ensure(c, c->ff_clocks, sizeof(long long) * 32));
        HGMM_HIP(c, hipMemsetAsync(c->ff_clocks.p, 0, sizeof(long long) * 32, c->stream));
        c->ff_clocks_on = true;
        return HGMM_OK;
    }
    c->ff_clocks_on = false;
    if (clocks_out) {
        if (!c->ff_clocks.p) return fail(c, HGMM_ERR_STATE, "phase clocks were never armed");
        static_assert(sizeof(long long) == sizeof(int64_t), "clock words");
        HGMM_HIP(c, hipMemcpyAsync(clocks_out, c->ff_clocks.p, sizeof(long long) * 32, hipMemcpyDeviceToHost, c->stream));
        HGMM_HIP(c, ctx_stream_sync(c));
    }
    return HGMM_OK;
}

extern "C" int hgmm_fullcov_estep(hgmm_ctx* c, int J, const double* pi, const double* mu, const double* cov,
                                  double* m0_out, double* m1_out, double* m2_out, int32_t* labels_out,
                                  double* q_out) {
    HGMM_ENTER(c);
    if (!c || !pi || !mu || !cov) return c ? fail(c, HGMM_ERR_ARG, "NULL parameter table") : HGMM_ERR_ARG;
    if (!c->have_f64 || c->n <= 0) return fail(c, HGMM_ERR_STATE, "full-covariance E-step: set points first");
    if (J < 1 || J > 4096) return fail(c, HGMM_ERR_ARG, "J = %d outside 1..4096", J);
    HGMM_HIP(c, hipSetDevice(c->device));
    int J16 = 0, grid = 0;
    HGMM_TRY(fullcov_alloc(c, J, &J16, &grid));
    HGMM_HIP(c, hipMemsetAsync(c->t_pi.p, 0, sizeof(double) * J16, c->stream));
    HGMM_HIP(c, hipMemsetAsync(c->t_mu.p, 0, sizeof(double) * 3 * J16, c->stream));
    HGMM_HIP(c, hipMemsetAsync(c->t_cov.p, 0, sizeof(double) * 9 * J16, c->stream));
    HGMM_HIP(c, hipMemcpyAsync(c->t_pi.p, pi, sizeof(double) * J, hipMemcpyHostToDevice, c->stream));
    HGMM_HIP(c, hipMemcpyAsync(c->t_mu.p, mu, sizeof(double) * 3 * J, hipMemcpyHostToDevice, c->stream));
    HGMM_HIP(c, hipMemcpyAsync(c->t_cov.p, cov, sizeof(double) * 9 * J, hipMemcpyHostToDevice, c->stream));
    tree_prep_kernel<<<nblk(J16, 256), 256, 0, c->stream>>>(c->t_pi.as<double>(), c->t_mu.as<double>(),
                                                           c->t_cov.as<double>(), 0, J16, c->t_prep.as<double>(), flags_ptr(c));
    int* lab = c->t_current.as<int>();
    double q = 0.0;
    if (fullcov_one_pass(c, J16)) {
        HGMM_TRY(fullcov_fused(c, J, J16, lab, &q));
    } else {
        HGMM_TRY(fullcov_pass(c, J, lab, &q));
        HGMM_TRY(fullcov_moments(c, J, J16, grid));
    }
    HGMM_TRY(ensure(c, c->scratch, sizeof(double) * 13 * J16));
    double* e0 = c->scratch.as<double>();
    double* e1 = e0 + J16;
    double* e2 = e1 + 3 * J16;
    tree_expand_moments_kernel<<<nblk(J, 256), 256, 0, c->stream>>>(c->t_mom.as<double>(), J, e0, e1, e2);
    HGMM_HIP(c, hipGetLastError());
    {
        StagedDownloads dl(c);
        dl.add(m0_out, e0, sizeof(double) * J);
        dl.add(m1_out, e1, sizeof(double) * 3 * J);
        dl.add(m2_out, e2, sizeof(double) * 9 * J);
        dl.add(labels_out, lab, sizeof(int) * c->n);
        HGMM_HIP(c, dl.finish());
    }
    if (q_out) *q_out = q;
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
    HGMM_TRY(ensure(c, c->t_pi, sizeof(double) * T));
    HGMM_TRY(ensure(c, c->t_mu, sizeof(double) * 3 * T));
    HGMM_TRY(ensure(c, c->t_cov, sizeof(double) * 9 * T));
    HGMM_TRY(ensure(c, c->t_prep, sizeof(double) * PREP_N * T));
    HGMM_TRY(ensure(c, c->t_mom, sizeof(double) * NMOM * T));
    HGMM_TRY(tree_flags(c, true));
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
    HGMM_TRY(ensure(c, c->t_momq, sizeof(unsigned long long) * (2 * NMOM * T + 1)));
    unsigned long long* mq = c->t_momq.as<unsigned long long>();
    HGMM_HIP(c, hipMemsetAsync(mq, 0, sizeof(unsigned long long) * (2 * NMOM * T + 1), c->stream));
    c->tree.momq_dirty = true;
    tree_rmax_kernel<<<nblk(c->n, 256), 256, 0, c->stream>>>(c->x_soa64.as<double>(), c->n, c->n_pad, mq + 2 * NMOM * T);
    unsigned long long r2bits = 0;
    HGMM_HIP(c, hipMemcpyAsync(&r2bits, mq + 2 * NMOM * T, sizeof r2bits, hipMemcpyDeviceToHost, c->stream));
    HGMM_HIP(c, ctx_stream_sync(c));
    double r2 = 0.0;
    memcpy(&r2, &r2bits, sizeof r2);
    double m2max = 0.0;
    for (int64_t j = 0; j < T; ++j) {
        const double v = mu[3 * j] * mu[3 * j] + mu[3 * j + 1] * mu[3 * j + 1] + mu[3 * j + 2] * mu[3 * j + 2];
        if (v > m2max && std::isfinite(v)) m2max = v;
    }
    double ext = std::sqrt(r2) + std::sqrt(m2max);
    double n_all = (double)c->n;
    if (c->comm_on()) {
        HGMM_TRY(hgmm_comm_allreduce_f64(c, &ext, 1, 1));
        HGMM_TRY(hgmm_comm_allreduce_f64(c, &n_all, 1, 0));
    }
    if (!(ext > 0.0) || !std::isfinite(ext)) ext = 1.0;
    int e2x = 0;
    (void)std::frexp(ext, &e2x);
    const double D = std::ldexp(1.0, e2x);
    int nbits = 1;
    while (std::ldexp(1.0, nbits) <= n_all) ++nbits;
    const int F = 62 - nbits;
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
                                                                  TreeStop{nullptr, 0.0, 0, nullptr, 0}, flags_ptr(c), nullptr);
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
