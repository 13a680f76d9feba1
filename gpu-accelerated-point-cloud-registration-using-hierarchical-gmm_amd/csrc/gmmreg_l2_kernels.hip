// Fused rigid L2 cost of the GMMReg registration over RESIDENT mixtures for gfx950, float64: R poses per launch set.
//
// hgmm_gauss_transform (gmmreg_kernels.hip) serves one cost evaluation with three uploads, one launch, a download of
// splits x 4 x J_s partial sums and NumPy behind it.  During a BFGS solve the mixtures never change and only seven
// numbers do, so here the mixtures of B pairs stay on the device (hgmm_l2_set_pairs) and an evaluation
// (hgmm_l2_cost) uploads 128 bytes per hypothesis, runs two kernels and reads 13 doubles per hypothesis back:
//   l2_cost_kernel    one wave per (hypothesis, block of 64 source centres, split of <= 256 target centres): poses the
//                     source centres, tiles the targets through LDS, and reduces  f, sum_i grad_i, sum_i grad_i (x) x_i
//                     over its lanes in the fixed order of wave_sum_f64 -> one record of 13 doubles
//   l2_finish_kernel  adds a hypothesis' records in (source block, target split) order -> [R][13] in pinned host memory
// Every output is linear in the per-centre sums (g0, g1), so a split only adds partial records.  The map of a
// hypothesis onto workgroups depends on (J_s, J_t) alone and nothing is accumulated with atomics: hypothesis r of any
// call has the bits of the R = 1 call.
//
// The arithmetic follows RigidCostFunction.__call__ / compute_l2_dist on the host (gmmreg_gpu/cost_functions.py) step by
// step -- the same divisions where the host divides, differences taken axis by axis, no contraction into fused
// multiply-adds except the pose's own dot products -- so that what remains between the two is the summation order and the
// exponential's last bit.
#include "hgmm_ctx.h"
#include "wave_ops.h"

#include <cmath>
#include <cstring>
#include <vector>

namespace hgmm {

constexpr int L2_BLOCK = 64;          // source centres per workgroup (one wave)
constexpr int L2_TILE = 128;          // target centres per LDS tile
constexpr int L2_SPLIT = 256;         // target centres per workgroup (two tiles)
constexpr int L2_NOUT = HGMM_L2_NOUT;
constexpr int L2_ROW = 8;             // doubles per tile row: mu (3), phi / z, phi mu / z (3), one pad (16-byte rows)
constexpr unsigned long long L2_MAX_RECORD_BYTES = 1ull << 30;

// one hypothesis as it travels to the device: everything that depends on sigma is worked out once, on the host
struct L2Hyp {
    double rot[9], t[3];
    double neg_h2;                    // -(h h), h = sqrt(2) sigma: the exponent is d2 / neg_h2 (transforms.py: kernel_matrix)
    double z;                         // (2 pi sigma^2)^(3/2)
    double two_s2;                    // 2 sigma^2
    int pair, pad;
};
static_assert(sizeof(L2Hyp) == 128, "L2Hyp is 16 words");

inline int l2_blocks(int Js) { return (Js + L2_BLOCK - 1) / L2_BLOCK; }
__host__ __device__ inline int l2_splits(int Jt) { return (Jt + L2_SPLIT - 1) / L2_SPLIT; }

__global__ __launch_bounds__(L2_BLOCK) void l2_cost_kernel(
    const double* __restrict__ mu_s, const double* __restrict__ phi_s, const double* __restrict__ mu_t,
    const double* __restrict__ phi_t, const L2Pair* __restrict__ pairs, const L2Hyp* __restrict__ hyps, int wg_max,
    double* __restrict__ records /*[R][wg_max][13]*/) {
#pragma clang fp contract(off)
    __shared__ double tile[L2_TILE][L2_ROW];
    const int r = blockIdx.y;
    const L2Hyp& h = hyps[r];
    const L2Pair p = pairs[h.pair];
    const int nsp = l2_splits(p.Jt);
    const int w = blockIdx.x;
    if (w >= ((p.Js + L2_BLOCK - 1) / L2_BLOCK) * nsp) return;      // (uniform: the whole workgroup leaves)
    const int sb = w / nsp, sp = w - sb * nsp;
    const int i = sb * L2_BLOCK + (int)threadIdx.x;
    const bool live = i < p.Js;
    double x0 = 0.0, x1 = 0.0, x2 = 0.0, ps = 0.0;
    if (live) {
        const double* x = mu_s + 3 * (size_t)(p.s_first + i);
        x0 = x[0]; x1 = x[1]; x2 = x[2];
        ps = phi_s[p.s_first + i];
    }
    // y = rot x + t, each dot product one multiply and two fused multiply-adds in the order of the columns
    const double y0 = fma(x2, h.rot[2], fma(x1, h.rot[1], x0 * h.rot[0])) + h.t[0];
    const double y1 = fma(x2, h.rot[5], fma(x1, h.rot[4], x0 * h.rot[3])) + h.t[1];
    const double y2 = fma(x2, h.rot[8], fma(x1, h.rot[7], x0 * h.rot[6])) + h.t[2];
    const double neg_h2 = h.neg_h2, z = h.z;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;                  // g0, g1[3] of this split
    const int c_begin = sp * L2_SPLIT;
    const int c_end = min(p.Jt, c_begin + L2_SPLIT);
    for (int base = c_begin; base < c_end; base += L2_TILE) {
        const int cnt = min(L2_TILE, c_end - base);
        __syncthreads();
        for (int j = (int)threadIdx.x; j < cnt; j += L2_BLOCK) {
            const double* m = mu_t + 3 * (size_t)(p.t_first + base + j);
            const double ph = phi_t[p.t_first + base + j];
            const double m0 = m[0], m1 = m[1], m2 = m[2];
            tile[j][0] = m0; tile[j][1] = m1; tile[j][2] = m2;
            tile[j][3] = ph / z;
            tile[j][4] = (ph * m0) / z; tile[j][5] = (ph * m1) / z; tile[j][6] = (ph * m2) / z;
        }
        __syncthreads();
        for (int j = 0; j < cnt; ++j) {
            const double d0 = y0 - tile[j][0], d1 = y1 - tile[j][1], d2 = y2 - tile[j][2];
            const double e = exp((d0 * d0 + d1 * d1 + d2 * d2) / neg_h2);
            a0 += tile[j][3] * e;
            a1 += tile[j][4] * e;
            a2 += tile[j][5] * e;
            a3 += tile[j][6] * e;
        }
    }
    // a lane without a centre adds exact zeros, whatever the pose is (0 x NaN would not)
    double v[L2_NOUT];
    const double g0 = live ? (ps * (a0 * y0 - a1)) / h.two_s2 : 0.0;
    const double g1 = live ? (ps * (a0 * y1 - a2)) / h.two_s2 : 0.0;
    const double g2 = live ? (ps * (a0 * y2 - a3)) / h.two_s2 : 0.0;
    v[0] = live ? -(ps * a0) : 0.0;
    v[1] = g0; v[2] = g1; v[3] = g2;
    v[4] = g0 * x0; v[5] = g0 * x1; v[6] = g0 * x2;
    v[7] = g1 * x0; v[8] = g1 * x1; v[9] = g1 * x2;
    v[10] = g2 * x0; v[11] = g2 * x1; v[12] = g2 * x2;
    double* rec = records + ((size_t)r * wg_max + w) * L2_NOUT;
#pragma unroll
    for (int k = 0; k < L2_NOUT; ++k) {
        const double s = wave_sum_f64(v[k]);
        if (threadIdx.x == 0) rec[k] = s;
    }
}

// one thread per (hypothesis, output): the hypothesis' records in (source block, target split) order
__global__ __launch_bounds__(256) void l2_finish_kernel(const L2Pair* __restrict__ pairs, const L2Hyp* __restrict__ hyps,
                                                        int R, int wg_max, const double* __restrict__ records,
                                                        double* __restrict__ out /*[R][13], pinned host memory*/) {
#pragma clang fp contract(off)
    const int e = blockIdx.x * 256 + (int)threadIdx.x;
    if (e >= R * L2_NOUT) return;
    const int r = e / L2_NOUT, k = e - r * L2_NOUT;
    const L2Pair p = pairs[hyps[r].pair];
    const int nwg = ((p.Js + L2_BLOCK - 1) / L2_BLOCK) * l2_splits(p.Jt);
    const double* rec = records + (size_t)r * wg_max * L2_NOUT + k;
    double s = rec[0];
    for (int w = 1; w < nwg; ++w) s += rec[(size_t)w * L2_NOUT];
    out[e] = s;
}

}  // namespace hgmm

using namespace hgmm;

extern "C" int hgmm_l2_set_pairs(hgmm_ctx* c, int B, const int32_t* Js, const double* mu_s, const double* phi_s,
                                 const int32_t* Jt, const double* mu_t, const double* phi_t) {
    HGMM_ENTER(c);
    if (!Js || !mu_s || !phi_s || !Jt || !mu_t || !phi_t) return fail(c, HGMM_ERR_ARG, "l2 set pairs: NULL argument");
    if (B < 1 || B > HGMM_L2_MAX_PAIRS)
        return fail(c, HGMM_ERR_ARG, "l2 set pairs: B = %d outside 1..%d", B, HGMM_L2_MAX_PAIRS);
    std::vector<L2Pair> pairs((size_t)B);
    long long ns = 0, nt = 0;
    int wg_max = 0;
    for (int b = 0; b < B; ++b) {
        if (Js[b] < 1 || Jt[b] < 1)
            return fail(c, HGMM_ERR_ARG, "l2 set pairs: J < 1 (pair %d has %d source and %d target components)", b,
                        (int)Js[b], (int)Jt[b]);
        pairs[(size_t)b] = {(int)ns, (int)Js[b], (int)nt, (int)Jt[b]};
        ns += Js[b];
        nt += Jt[b];
        if (ns + nt > 2147483647LL) return fail(c, HGMM_ERR_ARG, "l2 set pairs: more than 2^31 - 1 centres in all");
        const long long nwg = (long long)l2_blocks(Js[b]) * l2_splits(Jt[b]);
        if (nwg > 2147483647LL) return fail(c, HGMM_ERR_ARG, "l2 set pairs: pair %d is too large for one launch", b);
        if ((int)nwg > wg_max) wg_max = (int)nwg;
    }
    // (nothing resident has been touched so far; from here on the previous set is gone)
    const size_t doubles = 4 * (size_t)(ns + nt);
    c->l2.B = 0;
    HGMM_TRY(ensure(c, c->l2.mix, sizeof(double) * doubles + sizeof(L2Pair) * (size_t)B));
    double* d = c->l2.mix.as<double>();
    HGMM_HIP(c, hipMemcpyAsync(d, mu_s, sizeof(double) * 3 * (size_t)ns, hipMemcpyHostToDevice, c->stream));
    HGMM_HIP(c, hipMemcpyAsync(d + 3 * (size_t)ns, phi_s, sizeof(double) * (size_t)ns, hipMemcpyHostToDevice, c->stream));
    HGMM_HIP(c, hipMemcpyAsync(d + 4 * (size_t)ns, mu_t, sizeof(double) * 3 * (size_t)nt, hipMemcpyHostToDevice, c->stream));
    HGMM_HIP(c, hipMemcpyAsync(d + 4 * (size_t)ns + 3 * (size_t)nt, phi_t, sizeof(double) * (size_t)nt, hipMemcpyHostToDevice,
                               c->stream));
    HGMM_HIP(c, hipMemcpyAsync(d + doubles, pairs.data(), sizeof(L2Pair) * (size_t)B, hipMemcpyHostToDevice, c->stream));
    HGMM_HIP(c, ctx_stream_sync(c));                     // the caller's arrays and `pairs` are free again
    if (!c->l2.pin) {
        void* p = nullptr;
        void* pd = nullptr;
        HGMM_HIP(c, hipHostMalloc(&p, (sizeof(L2Hyp) + sizeof(double) * L2_NOUT) * HGMM_L2_MAX_HYP, hipHostMallocMapped));
        if (hipHostGetDevicePointer(&pd, p, 0) != hipSuccess) {
            (void)hipHostFree(p);
            return fail(c, HGMM_ERR_HIP, "l2 set pairs: no device address for the pinned result block");
        }
        c->l2.pin = static_cast<char*>(p);
        c->l2.pin_dev = static_cast<char*>(pd);
    }
    c->l2.pairs = std::move(pairs);
    c->l2.wg_max = wg_max;
    c->l2.B = B;
    return HGMM_OK;
}

extern "C" int hgmm_l2_cost(hgmm_ctx* c, int R, const int32_t* pair, const double* rot, const double* t, const double* sigma,
                            double* out) {
    HGMM_ENTER(c);
    if (!pair || !rot || !t || !sigma || !out) return fail(c, HGMM_ERR_ARG, "l2 cost: NULL argument");
    if (c->l2.B < 1) return fail(c, HGMM_ERR_STATE, "l2 cost: no resident pairs (call hgmm_l2_set_pairs first)");
    if (R < 1 || R > HGMM_L2_MAX_HYP) return fail(c, HGMM_ERR_ARG, "l2 cost: R = %d outside 1..%d", R, HGMM_L2_MAX_HYP);
    for (int r = 0; r < R; ++r) {
        if (pair[r] < 0 || pair[r] >= c->l2.B)
            return fail(c, HGMM_ERR_ARG, "l2 cost: pair out of range (hypothesis %d names pair %d of %d)", r, (int)pair[r], c->l2.B);
        if (!(sigma[r] > 0.0))
            return fail(c, HGMM_ERR_ARG, "l2 cost: sigma not positive (hypothesis %d: %g)", r, sigma[r]);
    }
    const int wg_max = c->l2.wg_max;
    const unsigned long long rec_bytes = (unsigned long long)R * (unsigned long long)wg_max * L2_NOUT * sizeof(double);
    if (rec_bytes > L2_MAX_RECORD_BYTES)
        return fail(c, HGMM_ERR_ARG, "l2 cost: the records of %d hypotheses x %d workgroups exceed %llu bytes; call with fewer",
                    R, wg_max, L2_MAX_RECORD_BYTES);
    HGMM_TRY(ensure(c, c->l2.work, sizeof(L2Hyp) * (size_t)R + (size_t)rec_bytes));
    L2Hyp* hyp_host = reinterpret_cast<L2Hyp*>(c->l2.pin);
    for (int r = 0; r < R; ++r) {
        L2Hyp& h = hyp_host[r];
        std::memcpy(h.rot, rot + 9 * (size_t)r, sizeof h.rot);
        std::memcpy(h.t, t + 3 * (size_t)r, sizeof h.t);
        const double s = sigma[r], hh = std::sqrt(2.0) * s;
        h.neg_h2 = -(hh * hh);
        h.z = std::pow((2.0 * M_PI) * (s * s), 1.5);
        h.two_s2 = 2.0 * (s * s);
        h.pair = pair[r];
        h.pad = 0;
    }
    L2Hyp* d_hyp = c->l2.work.as<L2Hyp>();
    double* d_rec = reinterpret_cast<double*>(d_hyp + R);
    HGMM_HIP(c, hipMemcpyAsync(d_hyp, hyp_host, sizeof(L2Hyp) * (size_t)R, hipMemcpyHostToDevice, c->stream));
    long long ns = 0, nt = 0;
    for (const L2Pair& p : c->l2.pairs) { ns += p.Js; nt += p.Jt; }
    const double* d_mu_s = c->l2.mix.as<double>();
    const double* d_phi_s = d_mu_s + 3 * (size_t)ns;
    const double* d_mu_t = d_phi_s + (size_t)ns;
    const double* d_phi_t = d_mu_t + 3 * (size_t)nt;
    const L2Pair* d_pairs = reinterpret_cast<const L2Pair*>(d_phi_t + (size_t)nt);
    const size_t out_off = sizeof(L2Hyp) * HGMM_L2_MAX_HYP;
    double* out_dev = reinterpret_cast<double*>(c->l2.pin_dev + out_off);
    l2_cost_kernel<<<dim3((unsigned)wg_max, (unsigned)R), L2_BLOCK, 0, c->stream>>>(d_mu_s, d_phi_s, d_mu_t, d_phi_t, d_pairs,
                                                                                  d_hyp, wg_max, d_rec);
    HGMM_HIP(c, hipGetLastError());
    l2_finish_kernel<<<(R * L2_NOUT + 255) / 256, 256, 0, c->stream>>>(d_pairs, d_hyp, R, wg_max, d_rec, out_dev);
    HGMM_HIP(c, hipGetLastError());
    HGMM_HIP(c, ctx_stream_sync(c));
    std::memcpy(out, c->l2.pin + out_off, sizeof(double) * L2_NOUT * (size_t)R);
    return HGMM_OK;
}
