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
//
// THE DEVICE SOLVE (hgmm_l2_solve): the whole BFGS solve of R hypotheses on the resident mixtures, in lock-step, two
// launches per evaluation and no host between them:
//   l2_solve_cost_kernel  l2_cost_kernel's body (l2_cost_body.h) over the hypotheses' CURRENT trial poses; the workgroups
//                         of a hypothesis that has left the loop return at their first load
//   l2_solve_step_kernel  one wave per hypothesis: adds its records as l2_finish_kernel does -- the 13 sums have the bits
//                         hgmm_l2_cost returns for that pose -- then lane 0 does the serial part (l2_device.h: pose and
//                         dR/dq from the quaternion, the 7-gradient, one transition of SciPy's dcsrch / BFGS state machine,
//                         the next trial pose) and stores the progress word (left << 32 | evaluations) into pinned host
//                         memory at system scope.  The state (L2SolveState) never leaves the device before the end.
// The host enqueues a few evaluations ahead of the slowest running hypothesis (tree_host.h: follow_ahead).
#include "hgmm_ctx.h"
#include "tree_host.h"
#include "wave_ops.h"
#include "l2_device.h"

#include <cmath>
#include <cstring>
#include <vector>

namespace hgmm {

static_assert(L2_NOUT == HGMM_L2_NOUT, "l2_device.h");

__global__ __launch_bounds__(L2_BLOCK) void l2_cost_kernel(
    const double* __restrict__ mu_s, const double* __restrict__ phi_s, const double* __restrict__ mu_t,
    const double* __restrict__ phi_t, const L2Pair* __restrict__ pairs, const L2Hyp* __restrict__ hyps, int wg_max,
    double* __restrict__ records /*[R][wg_max][13]*/) {
#pragma clang fp contract(off)
    __shared__ double tile[L2_TILE][L2_ROW];
    const int r = blockIdx.y;
    const L2Hyp& h = hyps[r];
#include "l2_cost_body.h"
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

// ---- the device solve --------------------------------------------------------------------------------------------------
// l2_cost_kernel over the trial poses the step kernel left in `hyps`; L2Hyp::pad != 0: the hypothesis has left the loop
__global__ __launch_bounds__(L2_BLOCK) void l2_solve_cost_kernel(
    const double* __restrict__ mu_s, const double* __restrict__ phi_s, const double* __restrict__ mu_t,
    const double* __restrict__ phi_t, const L2Pair* __restrict__ pairs, const L2Hyp* __restrict__ hyps, int wg_max,
    double* __restrict__ records /*[R][wg_max][13]*/) {
#pragma clang fp contract(off)
    __shared__ double tile[L2_TILE][L2_ROW];
    const int r = blockIdx.y;
    const L2Hyp& h = hyps[r];
    if (h.pad != 0) return;                                         // (uniform: the whole workgroup leaves)
#include "l2_cost_body.h"
}

// the pose of a quaternion into a hypothesis' slot
__device__ inline void l2_solve_pose(const double* theta, L2Hyp* h) {
    L2Quat qt;
    l2_quat_terms(theta, false, qt);
    for (int i = 0; i < 9; ++i) h->rot[i] = qt.rot[i];
    for (int i = 0; i < 3; ++i) h->t[i] = theta[4 + i];
}

// the start poses: one thread per hypothesis (the same code that forms every later trial pose)
__global__ __launch_bounds__(L2_BLOCK) void l2_solve_init_kernel(L2Hyp* hyps, const L2SolveState* __restrict__ states, int R) {
    const int r = blockIdx.x * L2_BLOCK + (int)threadIdx.x;
    if (r < R) l2_solve_pose(states[r].x, hyps + r);
}

// one wave per hypothesis: lanes 0..12 add its records in (source block, target split) order, as l2_finish_kernel does;
// lane 0 then does the serial part of the evaluation (l2_solve_step) on a copy of the state, writes the next trial pose or
// the "left" mark, and stores the progress word for the host
__global__ __launch_bounds__(L2_BLOCK) void l2_solve_step_kernel(const L2Pair* __restrict__ pairs, L2Hyp* hyps,
                                                                 L2SolveState* states, int wg_max,
                                                                 const double* __restrict__ records,
                                                                 unsigned long long* host_words) {
#pragma clang fp contract(off)
    __shared__ double sums[L2_NOUT];
    const int r = blockIdx.x;
    L2Hyp* h = hyps + r;
    if (h->pad != 0) return;
    const int k = (int)threadIdx.x;
    if (k < L2_NOUT) {
        const L2Pair p = pairs[h->pair];
        const int nwg = ((p.Js + L2_BLOCK - 1) / L2_BLOCK) * l2_splits(p.Jt);
        const double* rec = records + (size_t)r * wg_max * L2_NOUT + k;
        double s = rec[0];
        for (int w = 1; w < nwg; ++w) s += rec[(size_t)w * L2_NOUT];
        sums[k] = s;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double out[L2_NOUT];
    for (int i = 0; i < L2_NOUT; ++i) out[i] = sums[i];
    L2SolveState s = states[r];
    l2_solve_step(s, out);
    states[r] = s;
    if (s.left) h->pad = 1;
    else l2_solve_pose(s.xt, h);
    __hip_atomic_store(host_words + r, ((unsigned long long)(s.left ? 1 : 0) << 32) | (unsigned long long)(unsigned)s.nfev,
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
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

// ---- hgmm_l2_solve / hgmm_l2_solve_each -----------------------------------------------------------------------------------
namespace hgmm {

constexpr int L2_SOLVE_AHEAD = 4;      // evaluations the host keeps enqueued beyond the slowest hypothesis still running

// max_iter_of(r), gtol_of(r): the hypothesis' own limits (hgmm_l2_solve: the same for all)
template <class MaxIterOf, class GtolOf>
static int l2_solve_run(hgmm_ctx* c, int R, const int32_t* pair, const double* theta0, const double* sigma, MaxIterOf&& max_iter_of,
                        GtolOf&& gtol_of, double* theta_out, double* f_out, double* grad_out, int32_t* nit_out, int32_t* nfev_out,
                        int32_t* status_out) {
    if (c->l2.B < 1) return fail(c, HGMM_ERR_STATE, "l2 solve: no resident pairs (call hgmm_l2_set_pairs first)");
    if (R < 1 || R > HGMM_L2_MAX_HYP) return fail(c, HGMM_ERR_ARG, "l2 solve: R = %d outside 1..%d", R, HGMM_L2_MAX_HYP);
    long long budget = 1;
    for (int r = 0; r < R; ++r) {
        if (pair[r] < 0 || pair[r] >= c->l2.B)
            return fail(c, HGMM_ERR_ARG, "l2 solve: pair out of range (hypothesis %d names pair %d of %d)", r, (int)pair[r], c->l2.B);
        if (!(sigma[r] > 0.0))
            return fail(c, HGMM_ERR_ARG, "l2 solve: sigma not positive (hypothesis %d: %g)", r, sigma[r]);
        if (max_iter_of(r) < 1)
            return fail(c, HGMM_ERR_ARG, "l2 solve: max_iter < 1 (hypothesis %d: %d)", r, (int)max_iter_of(r));
        if (!(gtol_of(r) >= 0.0))
            return fail(c, HGMM_ERR_ARG, "l2 solve: gtol negative or NaN (hypothesis %d: %g)", r, gtol_of(r));
        // a line search that has not ended after L2_LS_MAX evaluations has failed: the budget is exact
        budget = std::max(budget, 1 + (long long)L2_LS_MAX * max_iter_of(r));
    }
    const int wg_max = c->l2.wg_max;
    const unsigned long long rec_bytes = (unsigned long long)R * (unsigned long long)wg_max * L2_NOUT * sizeof(double);
    if (rec_bytes > L2_MAX_RECORD_BYTES)
        return fail(c, HGMM_ERR_ARG, "l2 solve: the records of %d hypotheses x %d workgroups exceed %llu bytes; call with fewer",
                    R, wg_max, L2_MAX_RECORD_BYTES);
    const size_t head_bytes = (sizeof(L2Hyp) + sizeof(L2SolveState)) * (size_t)R;
    HGMM_TRY(ensure(c, c->l2.work, head_bytes + (size_t)rec_bytes));
    HandOver* hand = nullptr;
    HGMM_TRY(hand_over(c, R, &hand));
    const HostDev<unsigned long long> words = hand->progress(0);
    L2Hyp* hyp_host = reinterpret_cast<L2Hyp*>(c->l2.pin);
    std::vector<L2SolveState> states((size_t)R);
    std::memset(states.data(), 0, sizeof(L2SolveState) * (size_t)R);
    for (int r = 0; r < R; ++r) {
        L2Hyp& h = hyp_host[r];
        std::memset(&h, 0, sizeof h);
        const double s = sigma[r], hh = std::sqrt(2.0) * s;             // (as hgmm_l2_cost forms them)
        h.neg_h2 = -(hh * hh);
        h.z = std::pow((2.0 * M_PI) * (s * s), 1.5);
        h.two_s2 = 2.0 * (s * s);
        h.pair = pair[r];
        h.pad = 0;
        std::memcpy(states[r].x, theta0 + 7 * (size_t)r, sizeof states[r].x);
        states[r].max_iter = max_iter_of(r);
        states[r].gtol = gtol_of(r);
        __atomic_store_n(words.host + r, 0ull, __ATOMIC_RELAXED);
    }
    L2Hyp* d_hyp = c->l2.work.as<L2Hyp>();
    L2SolveState* d_state = reinterpret_cast<L2SolveState*>(d_hyp + R);
    double* d_rec = reinterpret_cast<double*>(d_state + R);
    HGMM_HIP(c, hipMemcpyAsync(d_hyp, hyp_host, sizeof(L2Hyp) * (size_t)R, hipMemcpyHostToDevice, c->stream));
    HGMM_HIP(c, hipMemcpyAsync(d_state, states.data(), sizeof(L2SolveState) * (size_t)R, hipMemcpyHostToDevice, c->stream));
    long long ns = 0, nt = 0;
    for (const L2Pair& p : c->l2.pairs) { ns += p.Js; nt += p.Jt; }
    const double* d_mu_s = c->l2.mix.as<double>();
    const double* d_phi_s = d_mu_s + 3 * (size_t)ns;
    const double* d_mu_t = d_phi_s + (size_t)ns;
    const double* d_phi_t = d_mu_t + 3 * (size_t)nt;
    const L2Pair* d_pairs = reinterpret_cast<const L2Pair*>(d_phi_t + (size_t)nt);
    l2_solve_init_kernel<<<(R + L2_BLOCK - 1) / L2_BLOCK, L2_BLOCK, 0, c->stream>>>(d_hyp, d_state, R);
    HGMM_HIP(c, hipGetLastError());
    HGMM_HIP(c, ctx_stream_sync(c));                     // (`states` and the pinned hypotheses are free again)
    const auto enqueue = [&](int) -> int {
        l2_solve_cost_kernel<<<dim3((unsigned)wg_max, (unsigned)R), L2_BLOCK, 0, c->stream>>>(d_mu_s, d_phi_s, d_mu_t, d_phi_t,
                                                                                            d_pairs, d_hyp, wg_max, d_rec);
        l2_solve_step_kernel<<<R, L2_BLOCK, 0, c->stream>>>(d_pairs, d_hyp, d_state, wg_max, d_rec, words.dev);
        HGMM_HIP(c, hipGetLastError());
        return HGMM_OK;
    };
    const int budget_int = (int)std::min(budget, 2147483647LL);
    const int rc = follow_ahead(c, words.host, R, budget_int, L2_SOLVE_AHEAD, enqueue, nothing_at_budget, nullptr,
                                "l2 solve");
    if (rc != HGMM_OK) {
        (void)ctx_stream_sync(c);                        // nothing of this call is left in flight
        return rc;
    }
    {
        StagedDownloads dl(c);
        dl.add(states.data(), d_state, sizeof(L2SolveState) * (size_t)R);
        HGMM_HIP(c, dl.finish());
    }
    for (int r = 0; r < R; ++r) {
        const L2SolveState& s = states[r];
        std::memcpy(theta_out + 7 * (size_t)r, s.x, sizeof s.x);
        f_out[r] = s.f;
        if (grad_out) std::memcpy(grad_out + 7 * (size_t)r, s.g, sizeof s.g);
        nit_out[r] = s.nit;
        nfev_out[r] = s.nfev;
        status_out[r] = s.status;
    }
    return HGMM_OK;
}

}  // namespace hgmm

extern "C" int hgmm_l2_solve_each(hgmm_ctx* c, int R, const int32_t* pair, const double* theta0, const double* sigma,
                                  const int32_t* max_iter, const double* gtol, double* theta_out, double* f_out, double* grad_out,
                                  int32_t* nit_out, int32_t* nfev_out, int32_t* status_out) {
    HGMM_ENTER(c);
    if (!pair || !theta0 || !sigma || !max_iter || !gtol || !theta_out || !f_out || !nit_out || !nfev_out || !status_out)
        return fail(c, HGMM_ERR_ARG, "l2 solve: NULL argument");
    return l2_solve_run(c, R, pair, theta0, sigma, [&](int r) { return (int)max_iter[r]; }, [&](int r) { return gtol[r]; },
                        theta_out, f_out, grad_out, nit_out, nfev_out, status_out);
}

extern "C" int hgmm_l2_solve(hgmm_ctx* c, int R, const int32_t* pair, const double* theta0, const double* sigma, int max_iter,
                             double gtol, double* theta_out, double* f_out, double* grad_out, int32_t* nit_out, int32_t* nfev_out,
                             int32_t* status_out) {
    HGMM_ENTER(c);
    if (!pair || !theta0 || !sigma || !theta_out || !f_out || !nit_out || !nfev_out || !status_out)
        return fail(c, HGMM_ERR_ARG, "l2 solve: NULL argument");
    return l2_solve_run(c, R, pair, theta0, sigma, [&](int) { return max_iter; }, [&](int) { return gtol; }, theta_out, f_out,
                        grad_out, nit_out, nfev_out, status_out);
}
