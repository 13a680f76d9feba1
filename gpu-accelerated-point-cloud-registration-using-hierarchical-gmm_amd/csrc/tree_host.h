// Host side shared by the drivers of the tree, forest and full-covariance kernels (tree_kernels.hip, tree_batch.hip,
// fullcov_kernels.hip): the pinned hand-over block, the watch of a host that follows the device through it, the guard
// of the fixed-point moment sums, and the small blocks every registration entry point needs.  Host code only.
#pragma once
#include "tree_device.h"

namespace hgmm {

// ---- defined in tree_kernels.hip, used by fullcov_kernels.hip as well ------------------------------------------------
__global__ void tree_mstep_kernel(const double* __restrict__ mom, int64_t lb, int n_level_nodes,
                                  double n_points_total, double ld, double* pi, double* mu, double* cov,
                                  double* prep, int* __restrict__ flags, const int* __restrict__ done,
                                  int with_complexity);
__global__ __launch_bounds__(256) void tree_sum_kernel(const double* __restrict__ v, int n, double* out,
                                                       const int* __restrict__ done, TreeStop stop);
__global__ void tree_expand_moments_kernel(const double* __restrict__ mom, int64_t T, double* m0,
                                           double* m1, double* m2);
int tree_flags(hgmm_ctx* c, bool reset);
int ensure_exp_tab2(hgmm_ctx* c);
inline int* flags_ptr(hgmm_ctx* c) { return c->t_flags.as<int>(); }

// ---- the pinned hand-over block (layout and accessors: hgmm_ctx.h, HandOver) -----------------------------------------
// The block for B pairs / clouds (the serial paths: B = 1).  It only grows; the device aliases are resolved here, once.
// (coherent = fine-grained: a system-scope store of a running kernel is visible to the polling host at once)
static_assert(sizeof(TreeCtl) == 16, "HandOver::ctl_slot");
inline int hand_over(hgmm_ctx* c, int B, HandOver** out) {
    HandOver& h = c->hand;
    if (!h.host || h.B < B) {
        HGMM_HIP(c, ctx_stream_sync(c));
        if (h.host) HGMM_HIP(c, hipHostFree(h.host));
        h.host = h.dev = nullptr;
        h.B = 0;
        void *hp = nullptr, *dp = nullptr;
        HGMM_HIP(c, hipHostMalloc(&hp, HandOver::bytes(B), hipHostMallocMapped | hipHostMallocCoherent));
        std::memset(hp, 0, HandOver::bytes(B));
        HGMM_HIP(c, hipHostGetDevicePointer(&dp, hp, 0));
        h.host = static_cast<char*>(hp);
        h.dev = static_cast<char*>(dp);
        h.cap = HandOver::bytes(B);
        h.B = B;
    }
    *out = &h;
    return HGMM_OK;
}
// the two events of the batch scheme (a copy of the control words into slot s, then event s)
inline int tree_batch_events(hgmm_ctx* c) {
    for (hipEvent_t& e : c->tree_ev)
        if (!e) HGMM_HIP(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    return HGMM_OK;
}

// ---- a host that follows the device through words of the block --------------------------------------------------------
// B progress words (stopped << 32 | iterations): has every loop stopped, the fewest iterations among those still
// running, and a signature of all the words for device_watch
struct Progress { bool all_done; int it_min; unsigned long long sig; };
inline Progress scan_progress(const unsigned long long* words, int B) {
    Progress p{true, 0x7fffffff, 0};
    for (int b = 0; b < B; ++b) {
        const unsigned long long w = __atomic_load_n(words + b, __ATOMIC_RELAXED);
        p.sig += w;
        if (w >> 32) continue;
        p.all_done = false;
        p.it_min = std::min(p.it_min, (int)(w & 0xffffffffull));
    }
    return p;
}
inline unsigned long long words_signature(const unsigned long long* words, int B) {
    unsigned long long sig = 0;
    for (int b = 0; b < B; ++b) sig += __atomic_load_n(words + b, __ATOMIC_ACQUIRE);
    return sig;
}
// The slow branch of every polling loop -- the words held nothing to act on: pause, and every ~16k polls ask the stream
// whether the device is still alive.  An idle stream has run everything that was enqueued: if the words' signature is
// still `seen` (what the caller read before it decided to wait), nothing is left that could move them.  HGMM_OK: keep
// polling; otherwise the error, named by the printf-style label.  The caller zeroes `spins` whenever it made progress.
__attribute__((format(printf, 6, 7))) inline int device_watch(hgmm_ctx* c, unsigned* spins, const unsigned long long* words,
                                                              int B, unsigned long long seen, const char* label, ...) {
    __builtin_ia32_pause();
    if ((++*spins & 0x3fff) != 0) return HGMM_OK;
    const hipError_t qe = hipStreamQuery(c->stream);
    if (qe == hipErrorNotReady) return HGMM_OK;
    if (qe == hipSuccess && words_signature(words, B) != seen) return HGMM_OK;
    char what[256];
    va_list ap;
    va_start(ap, label);
    vsnprintf(what, sizeof what, label, ap);
    va_end(ap);
    if (qe != hipSuccess) return fail(c, HGMM_ERR_HIP, "%s: device error: %s", what, hipGetErrorString(qe));
    return fail(c, HGMM_ERR_STATE, "%s: no progress (the stream is idle and the device has not reported)", what);
}

// ---- the fixed-point moment sums (t_momq, fr_momq) --------------------------------------------------------------------
// Invariant: clean == true  <=>  EVERY word of the buffer (its whole capacity, not just the words of the current tree)
// is zero.  Earlier uses may have been larger (hgmm_tree_estep writes 2 NMOM T + 1 two-word sums, hgmm_tree_reg_estep
// leaves [T][10] behind, a deeper tree has more nodes): clearing only this tree's words and then calling the buffer
// clean would let a later, larger use add onto stale sums.
// One scope per use: open() right before the first adding kernel is enqueued, consumed() once the host knows that the
// consumer -- which zeroes what it read -- has run for everything that was added.  Whatever returns in between leaves
// "not clean" behind, and the next use pays one memset instead of summing onto stale words.
struct MomqScope {
    bool& clean;
    explicit MomqScope(bool& flag) : clean(flag) {}
    // capacity >= want and every word zero; not clean from here on
    int open(hgmm_ctx* c, DevBuf& buf, size_t want) {
        const bool zero = clean && buf.p && buf.cap >= want;
        clean = false;
        if (!zero) {
            HGMM_TRY(ensure(c, buf, want));
            HGMM_HIP(c, hipMemsetAsync(buf.p, 0, buf.cap, c->stream));
        }
        return HGMM_OK;
    }
    void consumed() { clean = true; }
};

// ---- small blocks of the registration entry points ---------------------------------------------------------------------
// (rot, t, scale) of the C ABI; NULL: identity / no translation
inline Rigid rigid_from(const double* rot, const double* t, double scale) {
    Rigid tf;
    for (int i = 0; i < 9; ++i) tf.r[i] = rot ? rot[i] : ((i % 4 == 0) ? 1.0 : 0.0);
    for (int i = 0; i < 3; ++i) tf.t[i] = t ? t[i] : 0.0;
    tf.s = scale;
    return tf;
}
// a pair's table entry: its target's slice, everything else zero (a pair that takes no part)
// (tg_wsum: the targets' weight sums, NULL without weights -- the count then, as a double)
inline ForestRegPair reg_pair(int64_t tg_first, int64_t tg_count, const double* tg_wsum = nullptr, int b = 0) {
    ForestRegPair pr;
    std::memset(&pr, 0, sizeof pr);
    pr.tg_first = (int)tg_first;
    pr.tg_count = (int)tg_count;
    pr.tg_wsum = tg_wsum ? tg_wsum[b] : (double)tg_count;
    return pr;
}
// ... of a pair that takes part: its transform and the fixed-point encoding of its next E-step
inline void reg_pair_fill(ForestRegPair& pr, const Rigid& tf, double tg_rmax, double mu_rmax) {
    pr.active = 1;
    pr.tf = tf;
    double D = 1.0;
    int F = 0;
    reg_encoding(reg_extent(tf, tg_rmax, mu_rmax), pr.tg_wsum, &D, &F);
    pr.inv_d = 1.0 / D;
    pr.fix_scale = std::ldexp(1.0, F);
    pr.d_ext = D;
    pr.inv_scale = std::ldexp(1.0, -F);
    pr.tg_rmax = tg_rmax;
    pr.mu_rmax = mu_rmax;
}
// (tree_kernels.hip) one cloud's weights for hgmm_tree_set_target_weights[_batch] and hgmm_tree_set_source_weights[_batch]:
// finite, >= 0, not all zero; their sum
int check_target_weights(hgmm_ctx* c, const char* what, const double* w, int64_t n, double* sum_out);
// largest |mu_j| of the resident tree; a tree built on the device has not shown its means to the host yet
inline int tree_mu_rmax_resident(hgmm_ctx* c) {
    if (c->tree.mu_rmax >= 0.0) return HGMM_OK;
    const int64_t T = c->tree.T;
    std::vector<double> mu((size_t)3 * T);
    HGMM_HIP(c, hipMemcpyAsync(mu.data(), c->t_mu.p, sizeof(double) * 3 * T, hipMemcpyDeviceToHost, c->stream));
    HGMM_HIP(c, ctx_stream_sync(c));
    c->tree.mu_rmax = tree_mu_rmax(mu.data(), T);
    return HGMM_OK;
}

}  // namespace hgmm
