// Flat full-covariance EM (hgmm_fullcov_fit / hgmm_fullcov_estep / hgmm_fullcov_phase_clocks) for gfx950.  One tree level
// with branching J: it shares the node preparation, the M-step and the node tables (t_*) with the tree build
// (tree_kernels.hip, declared in tree_host.h) and nothing else.  The batched fit (hgmm_fullcov_fit_batch: B clouds per launch
// set, on the one-pass kernel's body) is fullcov_batch.h, included at the end of this file.
#include "tree_host.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

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

// The bodies of full_pass_kernel, full_moments_kernel and full_fused_f32_kernel are in fullcov_body.h, included once per kernel
// under `constexpr bool WEIGHTED` and `wsrc` (hgmm_fullcov_*_weighted: the points' weights [n], parallel to xs): the unweighted
// kernels are compiled from the text they always had.  The weight multiplies the point's log-likelihood term in the pass and
// its feature row in the moments; gamma, its floor and the arg-max never see it.
__global__ __launch_bounds__(CH) void full_pass_kernel(const double* __restrict__ xs, int64_t n, int64_t n_pad,
                                                       const double* __restrict__ prep, int J,
                                                       double* __restrict__ den_out, int* __restrict__ label_out,
                                                       double* __restrict__ block_q) {
    constexpr bool WEIGHTED = false;
    const double* const wsrc = nullptr;
#define FULLCOV_BODY 1
#include "fullcov_body.h"
#undef FULLCOV_BODY
}
__global__ __launch_bounds__(CH) void full_pass_w_kernel(const double* __restrict__ xs, int64_t n, int64_t n_pad,
                                                         const double* __restrict__ prep, int J,
                                                         double* __restrict__ den_out, int* __restrict__ label_out,
                                                         double* __restrict__ block_q, const double* __restrict__ wsrc) {
    constexpr bool WEIGHTED = true;
#define FULLCOV_BODY 1
#include "fullcov_body.h"
#undef FULLCOV_BODY
}

// grid = persistent workgroups, each owning a contiguous range of 64-point groups
__global__ __launch_bounds__(FULL_BLOCK) void full_moments_kernel(const double* __restrict__ xs, int64_t n, int64_t n_pad,
                                                          const double* __restrict__ prep, int J16,
                                                          const double* __restrict__ den_in,
                                                          double* __restrict__ partials /*[grid][J16][NMOM]*/) {
    constexpr bool WEIGHTED = false;
    const double* const wsrc = nullptr;
#define FULLCOV_BODY 2
#include "fullcov_body.h"
#undef FULLCOV_BODY
}
__global__ __launch_bounds__(FULL_BLOCK) void full_moments_w_kernel(const double* __restrict__ xs, int64_t n, int64_t n_pad,
                                                            const double* __restrict__ prep, int J16,
                                                            const double* __restrict__ den_in,
                                                            double* __restrict__ partials /*[grid][J16][NMOM]*/,
                                                            const double* __restrict__ wsrc) {
    constexpr bool WEIGHTED = true;
#define FULLCOV_BODY 2
#include "fullcov_body.h"
#undef FULLCOV_BODY
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
inline size_t ft_lds_bytes(int J16, bool weighted = false) {      // (weighted: + the tiles' weights, see WX / WT)
    return sizeof(double) * ((size_t)FT_P * ft_ldg(J16) + 16 * FT_LDF + 3 * FT_P + J16 + 4 * 3 * FT_P + EXP_TAB2_N +
                             (weighted ? 4 * FT_P : 0));
}

// The kernel's body, specialised at compile time on the form of the exponent:
//   CHOL   triangular form -|R (x - o) - R (mu - o)|^2 with R^T R = Sigma^-1 / 2 (prep[12..17]) and o = the cloud's first
//          point: 9 fma / mul per pair against 14 for 3 subtractions + the symmetric form; R (mu - o) is formed once per
//          component at the start.  (All points share ONE origin -- the flat fit's cloud is not spatially sorted --, so the
//          form carries a relative error of ~ eps |x - o| / sigma in the exponent: 1e-13 for millimetre clusters in a
//          metre-sized cloud, far inside the parity tolerances.)
//   !CHOL  the symmetric form, for node tables with a Sigma^-1 that failed the Cholesky test (flags bit 0).
// ... and on WEIGHTED (hgmm_fullcov_*_weighted; `wsrc` [n] parallel to xs): the tile's weights are staged next to its
// coordinates (0 for the rows past the cloud's end), phase B writes the feature row of point p as w_p f -- the weight rides in
// the B operand of the matrix product, the A operand (gamma and its floor) and the arg-max are what they are without it --
// and the point's log-likelihood term is multiplied by w_p.
// FT_WG of FT_NWG: the workgroup's place in the launch of THIS cloud -- blockIdx.x of gridDim.x for the serial kernels (the
// text they always had); BATCH: the local block and the serial grid of the member, handed in by hgmm_fullcov_fit_batch's
// kernel (fullcov_batch.h), whose launch holds many clouds.
template <int CPL, bool CHOL, bool WEIGHTED, bool BATCH = false>
__device__ __forceinline__ void full_fused_body(
    const double* __restrict__ xs, int64_t n, int64_t n_pad, const double* __restrict__ prep, int J16,
    int* __restrict__ label_out, double* __restrict__ block_q, double* __restrict__ partials /*[grid][J16][NMOM]*/,
    int want_stats, long long* __restrict__ dbg, double* lds, const double* __restrict__ exp2_tab,
    const double* __restrict__ wsrc, const unsigned wg_arg = 0, const unsigned nwg_arg = 0) {
#define FT_WG (BATCH ? wg_arg : blockIdx.x)
#define FT_NWG (BATCH ? nwg_arg : gridDim.x)
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
    double* WX = EXPT + EXP_TAB2_N;               // (WEIGHTED) [2][FT_P] the tile's weights, double-buffered like XA
    double* WT = WX + 2 * FT_P;                   // (WEIGHTED) [2][FT_P] ... by tile parity like TOT, for its log terms
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
    const int64_t per = (tiles + FT_NWG - 1) / FT_NWG;
    const int64_t t0 = (int64_t)FT_WG * per;
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
        if (WEIGHTED) {
            // threads 48..63 bring the points' weights (past the end: 0) by the SAME load instruction as the coordinates: a
            // branch of their own put a second memory round trip behind the first one at the end of wave 0's phase A
            if (tid < 4 * FT_P) {
                const int64_t i = tile * FT_P + st_p;
                const int64_t ic = i < n ? i : n - 1;
                const bool is_w = st_d == 3;
                const double v = *(is_w ? wsrc + ic : xs + (size_t)st_d * n_pad + ic);
                if (is_w) {
                    WX[buf * FT_P + st_p] = i < n ? v : 0.0;
                } else {
                    XA[(buf * 3 + st_d) * FT_P + st_p] = v;
                    XS[(buf * 3 + st_d) * FT_P + st_p] = v - st_o;
                }
            }
        } else if (tid < 3 * FT_P) {
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
        if (WEIGHTED) term *= (lane < FT_P) ? WT[par * FT_P + lane] : 0.0;
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
                if (WEIGHTED) WT[buf * FT_P + p] = WX[buf * FT_P + p];
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
                if (WEIGHTED) f *= WX[buf * FT_P + p];
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
    if (dbg && lane == 0 && FT_WG == 7) {
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
                if (feat < NMOM) partials[((size_t)FT_WG * J16 + comp) * NMOM + feat] = acc[t][fb];
            }
        }
    }
    if (w == LQ_WAVE && lane == 0) block_q[FT_WG] = lq;
#undef FT_TICK
#undef FT_WG
#undef FT_NWG
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
        full_fused_body<CPL, false, false>(xs, n, n_pad, prep, J16, label_out, block_q, partials, want_stats, dbg, lds, exp2_tab, nullptr);
    else
        full_fused_body<CPL, true, false>(xs, n, n_pad, prep, J16, label_out, block_q, partials, want_stats, dbg, lds, exp2_tab, nullptr);
}
// ... under the weights `wsrc` (hgmm_fullcov_fit_weighted / hgmm_fullcov_estep_weighted)
template <int CPL>
__global__ __launch_bounds__(FT_BLOCK) void full_fused_w_kernel(
    const double* __restrict__ xs, int64_t n, int64_t n_pad, const double* __restrict__ prep, int J16,
    int* __restrict__ label_out, double* __restrict__ block_q, double* __restrict__ partials /*[grid][J16][NMOM]*/,
    int want_stats, const int* __restrict__ flags, const double* __restrict__ exp2_tab,
    long long* __restrict__ dbg, const int* __restrict__ done, const double* __restrict__ wsrc) {
    extern __shared__ double lds[];
    if (done && *done) return;
    if (flags && (*flags & 1))
        full_fused_body<CPL, false, true>(xs, n, n_pad, prep, J16, label_out, block_q, partials, want_stats, dbg, lds, exp2_tab, wsrc);
    else
        full_fused_body<CPL, true, true>(xs, n, n_pad, prep, J16, label_out, block_q, partials, want_stats, dbg, lds, exp2_tab, wsrc);
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
inline size_t ff_lds_bytes(int J16, bool weighted = false) {       // (weighted: + the tiles' weights, see WX / WT)
    return sizeof(float) * ((size_t)FF_P * ff_ld(J16) + 16 * FF_P + FF_P + J16 + 2 * 2 * 3 * FF_P * 2) +
           sizeof(double) * (2 * FF_P + 2 + (weighted ? 4 * FF_P : 0));
}

// WEIGHTED (hgmm_fullcov_*_weighted; `wsrc` [n] parallel to xs): the tile's weights are staged with its coordinates (0 past the
// cloud's end); phase B converts w_p to float32 once and writes the feature row about the centroid as w_p f, and the point's
// log term is multiplied by w_p in float64.  The origin stays the UNWEIGHTED centroid: it is a reference point only, and the
// move back in full_reduce_f32_kernel holds for any o because it uses the (weighted) m0.
__global__ __launch_bounds__(FF_BLOCK, 4) void full_fused_f32_kernel(
    const double* __restrict__ xs, int64_t n, int64_t n_pad, const double* __restrict__ prep, int J16,
    int* __restrict__ label_out, double* __restrict__ block_q, float* __restrict__ partials /*[segments][J16][NMOM]*/,
    int segs_per_wg, int want_stats, const int* __restrict__ flags, const int* __restrict__ done,
    const double* __restrict__ origin_parts, long long* __restrict__ dbg) {
    constexpr bool WEIGHTED = false;
    const double* const wsrc = nullptr;
#define FULLCOV_BODY 3
#include "fullcov_body.h"
#undef FULLCOV_BODY
}
__global__ __launch_bounds__(FF_BLOCK, 4) void full_fused_f32_w_kernel(
    const double* __restrict__ xs, int64_t n, int64_t n_pad, const double* __restrict__ prep, int J16,
    int* __restrict__ label_out, double* __restrict__ block_q, float* __restrict__ partials /*[segments][J16][NMOM]*/,
    int segs_per_wg, int want_stats, const int* __restrict__ flags, const int* __restrict__ done,
    const double* __restrict__ origin_parts, long long* __restrict__ dbg, const double* __restrict__ wsrc) {
    constexpr bool WEIGHTED = true;
#define FULLCOV_BODY 3
#include "fullcov_body.h"
#undef FULLCOV_BODY
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

using namespace hgmm;

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

// `wsrc` (here and below): the resident source weights for the _weighted entries -- the WEIGHTED instantiation of the launch's
// E-step kernel --, NULL for the unweighted ones, whose launches are what they were
static int fullcov_moments(hgmm_ctx* c, int J, int J16, int grid, const double* wsrc) {
    {
        ProfScope prof(c, HGMM_K_FULL_MOMENTS);
        if (wsrc)
            full_moments_w_kernel<<<grid, FULL_BLOCK, 0, c->stream>>>(c->x_soa64.as<double>(), c->n, c->n_pad,
                                                                       c->t_prep.as<double>(), J16, c->t_parent.as<double>(),
                                                                       c->t_partials.as<double>(), wsrc);
        else
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
static int fullcov_fused(hgmm_ctx* c, int J, int J16, int* labels, double* q_host, const double* wsrc, bool want_stats = true,
                         const int* done = nullptr, TreeStop stop = NO_STOP) {
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
        const size_t lds32 = ff_lds_bytes(J16, wsrc != nullptr);
        HGMM_TRY(ensure(c, c->ff_origin, sizeof(double) * 3 * FF_OPARTS));
        double* oparts = c->ff_origin.as<double>();
        full_origin_parts_kernel<<<FF_OPARTS, 256, 0, c->stream>>>(c->x_soa64.as<double>(), c->n, c->n_pad, oparts);
        {
            ProfScope prof(c, HGMM_K_FULL_FUSED);
            if (wsrc) {
                HGMM_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&full_fused_f32_w_kernel),
                                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds32));
                full_fused_f32_w_kernel<<<grid32, FF_BLOCK, lds32, c->stream>>>(
                    c->x_soa64.as<double>(), c->n, c->n_pad, c->t_prep.as<double>(), J16, labels, block_q, c->t_partials.as<float>(),
                    segs_per_wg, want_stats ? 1 : 0, flags_ptr(c), done, oparts,
                    c->ff_clocks_on ? c->ff_clocks.as<long long>() : nullptr, wsrc);
            } else {
            HGMM_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&full_fused_f32_kernel),
                                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds32));
            full_fused_f32_kernel<<<grid32, FF_BLOCK, lds32, c->stream>>>(c->x_soa64.as<double>(), c->n, c->n_pad,
                                                                         c->t_prep.as<double>(), J16, labels, block_q,
                                                                         c->t_partials.as<float>(), segs_per_wg,
                                                                         want_stats ? 1 : 0, flags_ptr(c), done, oparts,
                                                                         c->ff_clocks_on ? c->ff_clocks.as<long long>() : nullptr);
            }
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
    const size_t lds = ft_lds_bytes(J16, wsrc != nullptr);
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
        long long* clocks = c->ff_clocks_on ? c->ff_clocks.as<long long>() : nullptr;
        if (wsrc && J16 <= FT_BLOCK) {
            HGMM_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&full_fused_w_kernel<1>),
                                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            full_fused_w_kernel<1><<<grid, FT_BLOCK, lds, c->stream>>>(
                c->x_soa64.as<double>(), c->n, c->n_pad, c->t_prep.as<double>(), J16, labels, block_q, c->t_partials.as<double>(),
                want_stats ? 1 : 0, flags_ptr(c), c->exp_tab2.as<double>(), nullptr, done, wsrc);
        } else if (wsrc) {
            HGMM_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&full_fused_w_kernel<2>),
                                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            full_fused_w_kernel<2><<<grid, FT_BLOCK, lds, c->stream>>>(
                c->x_soa64.as<double>(), c->n, c->n_pad, c->t_prep.as<double>(), J16, labels, block_q, c->t_partials.as<double>(),
                want_stats ? 1 : 0, flags_ptr(c), c->exp_tab2.as<double>(), clocks, done, wsrc);
        } else if (J16 <= FT_BLOCK) {
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
                                                                   flags_ptr(c), c->exp_tab2.as<double>(), clocks, done);
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

static int fullcov_pass(hgmm_ctx* c, int J, int* labels, double* q_host, const double* wsrc) {
    double* block_q = c->t_q.as<double>();
    double* q_dev = block_q + nblk(c->n, CH);
    {
        ProfScope prof(c, HGMM_K_FULL_PASS);
        if (wsrc)
            full_pass_w_kernel<<<nblk(c->n, CH), CH, 0, c->stream>>>(c->x_soa64.as<double>(), c->n, c->n_pad,
                                                                     c->t_prep.as<double>(), J, c->t_parent.as<double>(),
                                                                     labels, block_q, wsrc);
        else
        full_pass_kernel<<<nblk(c->n, CH), CH, 0, c->stream>>>(c->x_soa64.as<double>(), c->n, c->n_pad,
                                                             c->t_prep.as<double>(), J, c->t_parent.as<double>(),
                                                             labels, block_q);
    }
    tree_sum_kernel<<<1, 256, 0, c->stream>>>(block_q, (int)nblk(c->n, CH), q_dev, nullptr, NO_STOP);
    HGMM_HIP(c, hipGetLastError());
    if (c->comm_on()) HGMM_TRY(allreduce_f64_dev(c, q_dev, 1));
    if (q_host) {
        HGMM_HIP(c, hipMemcpyAsync(q_host, q_dev, sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HGMM_HIP(c, ctx_stream_sync(c));
    }
    return HGMM_OK;
}

// hgmm_fullcov_fit (weighted = false) and hgmm_fullcov_fit_weighted: the weighted level's three statements -- the E-step
// kernels' WEIGHTED instantiations (moments and log-likelihood) and pi = m0 / W with W = the source weights' sum
static int fullcov_fit(hgmm_ctx* c, bool weighted, int J, double ls, double ld, const double* init_mu, double sig2,
                       int max_iters, double* pi_out, double* mu_out, double* cov_out,
                       int32_t* labels_out, double* q_trace_out, int q_capacity, int* q_len_out) {
    HGMM_ENTER(c);
    if (!c->have_f64 || c->n <= 0) return fail(c, HGMM_ERR_STATE, "full-covariance fit: set points first");
    // (the source weights are never written by a tree build: the level-0 order of x_soa64, BuildWorkspace in tree_host.h)
    const double* wsrc = nullptr;
    if (weighted) HGMM_TRY(source_weights_ready(c, "hgmm_fullcov_fit_weighted", &wsrc));
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
    double n_total = weighted ? c->src.total(c->n) : (double)c->n;   // pi = m0 / N; with weights their sum
    if (c->comm_on()) HGMM_TRY(hgmm_comm_allreduce_f64(c, &n_total, 1, 0));
    // E-step quantities of the initial parameters
    const bool one_pass = fullcov_one_pass(c, J16);
    if (one_pass) HGMM_TRY(fullcov_fused(c, J, J16, lab_a, nullptr, wsrc));
    else HGMM_TRY(fullcov_pass(c, J, lab_a, nullptr, wsrc));
    int* lab_cur = lab_a;      // arg-max of the most recent E-step
    int* lab_nxt = lab_b;
    double prev_q = 0.0;
    int it = 0, q_len = 0;
    if (one_pass && !c->comm_on()) {
        // The stop rule on the device, the host one batch of iterations ahead (run_batches): the launches of an iteration look
        // at ctl->done first, the sum of q applies |q - prev_q| < ls / the budget.
        // (Waiting for q after every iteration left the device idle for ~0.1 ms per 1.7 ms iteration at N = 1e6.)
        double* q_dev = c->t_q.as<double>() + nblk(c->n, CH) + 2 * c->cus;
        TreeCtl* ctl = reinterpret_cast<TreeCtl*>(q_dev + 2);
        const int trace_cap = std::min(max_iters, 1 << 20);
        HGMM_TRY(ensure(c, c->t_qtrace, sizeof(double) * (size_t)trace_cap));
        double* trace_dev = c->t_qtrace.as<double>();
        HGMM_HIP(c, hipMemsetAsync(ctl, 0, sizeof(TreeCtl), c->stream));
        const TreeStop stop{ctl, ls, max_iters, trace_dev, trace_cap};
        HandOver* hand = nullptr;
        HGMM_TRY(hand_over(c, 1, &hand));
        const int batch = 4;
        const auto enqueue_one = [&](int k) -> int {               // iteration k: labels into buffer (k + 1) & 1
            tree_mstep_kernel<<<nblk(J, 256), 256, 0, c->stream>>>(c->t_mom.as<double>(), 0, J, n_total, ld, d_pi, d_mu,
                                                                   d_cov, d_prep, flags_ptr(c), &ctl->done, 1);
            return fullcov_fused(c, J, J16, ((k + 1) & 1) ? lab_b : lab_a, nullptr, wsrc, k + 1 < max_iters, &ctl->done, stop);
        };
        HGMM_TRY(run_batches(c, ctl, hand, max_iters, batch, enqueue_one, &it, "full-covariance fit"));
        q_len = it;
        lab_cur = ((it - 1) & 1) ? lab_b : lab_a;              // the arg-max of the E-step whose statistics the last M-step took
        if (q_trace_out && q_len > 0)
            HGMM_HIP(c, hipMemcpyAsync(q_trace_out, trace_dev, sizeof(double) * std::min(std::min(q_len, q_capacity), trace_cap),
                                       hipMemcpyDeviceToHost, c->stream));
    } else
    while (true) {
        if (!one_pass) HGMM_TRY(fullcov_moments(c, J, J16, grid, wsrc));              // E (moments)
        tree_mstep_kernel<<<nblk(J, 256), 256, 0, c->stream>>>(c->t_mom.as<double>(), 0, J, n_total, ld, d_pi, d_mu,
                                                               d_cov, d_prep, flags_ptr(c), nullptr, 1);    // M (+ prep)
        double q = 0.0;
        // q of the new parameters; one pass: the same launch already holds the next iteration's statistics
        // (the statistics of a call that is known to be the last one -- iteration budget reached -- are not formed)
        if (one_pass) HGMM_TRY(fullcov_fused(c, J, J16, lab_nxt, &q, wsrc, it + 1 < max_iters));
        else HGMM_TRY(fullcov_pass(c, J, lab_nxt, &q, wsrc));                         // q (+ next E-step's den)
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

extern "C" int hgmm_fullcov_fit(hgmm_ctx* c, int J, double ls, double ld, const double* init_mu, double sig2,
                                int max_iters, double* pi_out, double* mu_out, double* cov_out,
                                int32_t* labels_out, double* q_trace_out, int q_capacity, int* q_len_out) {
    return fullcov_fit(c, false, J, ls, ld, init_mu, sig2, max_iters, pi_out, mu_out, cov_out, labels_out, q_trace_out,
                       q_capacity, q_len_out);
}

extern "C" int hgmm_fullcov_fit_weighted(hgmm_ctx* c, int J, double ls, double ld, const double* init_mu, double sig2,
                                         int max_iters, double* pi_out, double* mu_out, double* cov_out,
                                         int32_t* labels_out, double* q_trace_out, int q_capacity, int* q_len_out) {
    return fullcov_fit(c, true, J, ls, ld, init_mu, sig2, max_iters, pi_out, mu_out, cov_out, labels_out, q_trace_out,
                       q_capacity, q_len_out);
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

static int fullcov_estep(hgmm_ctx* c, bool weighted, int J, const double* pi, const double* mu, const double* cov,
                         double* m0_out, double* m1_out, double* m2_out, int32_t* labels_out, double* q_out) {
    HGMM_ENTER(c);
    if (!c || !pi || !mu || !cov) return c ? fail(c, HGMM_ERR_ARG, "NULL parameter table") : HGMM_ERR_ARG;
    if (!c->have_f64 || c->n <= 0) return fail(c, HGMM_ERR_STATE, "full-covariance E-step: set points first");
    const double* wsrc = nullptr;
    if (weighted) HGMM_TRY(source_weights_ready(c, "hgmm_fullcov_estep_weighted", &wsrc));
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
        HGMM_TRY(fullcov_fused(c, J, J16, lab, &q, wsrc));
    } else {
        HGMM_TRY(fullcov_pass(c, J, lab, &q, wsrc));
        HGMM_TRY(fullcov_moments(c, J, J16, grid, wsrc));
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

extern "C" int hgmm_fullcov_estep(hgmm_ctx* c, int J, const double* pi, const double* mu, const double* cov,
                                  double* m0_out, double* m1_out, double* m2_out, int32_t* labels_out,
                                  double* q_out) {
    return fullcov_estep(c, false, J, pi, mu, cov, m0_out, m1_out, m2_out, labels_out, q_out);
}

extern "C" int hgmm_fullcov_estep_weighted(hgmm_ctx* c, int J, const double* pi, const double* mu, const double* cov,
                                           double* m0_out, double* m1_out, double* m2_out, int32_t* labels_out,
                                           double* q_out) {
    return fullcov_estep(c, true, J, pi, mu, cov, m0_out, m1_out, m2_out, labels_out, q_out);
}

#include "fullcov_batch.h"
