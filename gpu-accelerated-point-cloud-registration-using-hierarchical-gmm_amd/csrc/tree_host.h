// Host side shared by the drivers of the tree, forest and full-covariance kernels (tree_kernels.hip, tree_batch.hip,
// fullcov_kernels.hip): the pinned hand-over block and the watch of a host that follows the device through it, the
// picker of a kernel's instantiation, the two host loops of a device-side stop rule (follow_ahead, run_batches), the
// workspace and the trace hand-out of both builds, the guard of the fixed-point moment sums, and the small blocks every
// registration entry point needs.  Host code only.
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
// a launch that follows nothing / applies no stop rule
constexpr TreeFollow NO_FOLLOW{nullptr, 0, nullptr, nullptr, nullptr, 0.0, 0, nullptr, 0, nullptr};
constexpr TreeStop NO_STOP{nullptr, 0.0, 0, nullptr, 0};

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

// ---- the two host loops of every device-side stop rule -----------------------------------------------------------------
// The polled look-ahead loop (hgmm_tree_build: B = 1, ahead = tree_ahead; hgmm_tree_build_batch: 2; forest_register_on_device:
// 3).  Every member's stop rule stores (stopped << 32 | iterations) into its progress word of pinned HOST memory; the host
// keeps `ahead` iterations enqueued beyond the slowest member still running -- no copy, no event, no synchronisation, at
// most `ahead` iterations of skipped launches behind a stop (run_batches below: 46 of them over C4's four levels, ~0.25 ms
// of a 3.1 ms build, plus a control-word copy per batch) -- and returns once all have stopped.  The caller resets the
// words before the loop's first launch (every launch that could write them is this loop's) and reads the counts from them
// afterwards.  enqueue(e) -> status: iteration e, *enqueued (may be NULL) of them in all; on_budget_enqueued() fires once, right
// after iteration budget - 1 (the builds' close launch).  A launch the runtime rejected would leave the words untouched for
// ever: enqueue reports it (hipGetLastError) and the loop returns it before it polls again.  `what` names the loop.
template <class Enqueue, class AtBudget>
inline int follow_ahead(hgmm_ctx* c, const unsigned long long* words, int B, int budget, int ahead, Enqueue&& enqueue,
                        AtBudget&& on_budget_enqueued, int* enqueued, const char* what) {
    int enq = 0, rc = HGMM_OK;
    unsigned spins = 0;
    while (rc == HGMM_OK) {
        const Progress pg = scan_progress(words, B);
        if (pg.all_done) break;
        if (enq < budget && enq - pg.it_min < ahead) {
            rc = enqueue(enq);
            ++enq;
            if (rc == HGMM_OK && enq == budget) rc = on_budget_enqueued();
            spins = 0;
            continue;
        }
        if (enq >= budget && pg.it_min >= enq)                  // cannot happen (the budget's last iteration stops)
            rc = fail(c, HGMM_ERR_STATE, "%s did not stop within its budget", what);
        else                                                    // (seen: of the slowest member still running)
            rc = device_watch(c, &spins, words, B, pg.sig, "%s (%d iterations enqueued, %d seen)", what, enq, pg.it_min);
    }
    if (enqueued) *enqueued = enq;
    return rc;
}
inline int nothing_at_budget() { return HGMM_OK; }

// The batch scheme (hgmm_tree_build with tree_ahead = 0: batches of 8; hgmm_fullcov_fit: of 4).  The control word {done,
// iterations} stays on the device; the host enqueues `batch` iterations (enqueue_one(e) -> status, never beyond the budget),
// a copy of the word into slot s of the pinned block and event s.  It stays ONE BATCH AHEAD: batch k + 1 is enqueued before
// the host waits for batch k's verdict, so the device never idles at a batch boundary (round 2: enqueue, copy, synchronise,
// enqueue -- 30-40 us of idle device per batch, a quarter of C4's build).  The price: when the loop stops, the batch enqueued
// ahead runs as skipped launches (~1 us each).  *it: the iterations the loop took.
template <class EnqueueOne>
inline int run_batches(hgmm_ctx* c, const TreeCtl* ctl_dev, HandOver* hand, int budget, int batch, EnqueueOne&& enqueue_one, int* it,
                       const char* what) {
    for (hipEvent_t& e : c->tree_ev)                            // (one event per slot, made on first use)
        if (!e) HGMM_HIP(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    TreeCtl* hp = hand->ctl_slot(0);
    int enq = 0, slot = 0;
    auto enqueue_batch = [&](int s) -> int {
        const int cnt = std::min(batch, budget - enq);
        for (int b = 0; b < cnt; ++b) HGMM_TRY(enqueue_one(enq + b));
        enq += cnt;
        if (hipMemcpyAsync(&hp[s], ctl_dev, sizeof(TreeCtl), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
            hipEventRecord(c->tree_ev[s], c->stream) != hipSuccess)
            return fail(c, HGMM_ERR_HIP, "%s: device error: %s", what, hipGetErrorString(hipGetLastError()));
        return HGMM_OK;
    };
    HGMM_TRY(enqueue_batch(slot));
    while (true) {
        const bool ahead = enq < budget;
        if (ahead) HGMM_TRY(enqueue_batch(slot ^ 1));
        if (hipEventSynchronize(c->tree_ev[slot]) != hipSuccess)
            return fail(c, HGMM_ERR_HIP, "%s: device error: %s", what, hipGetErrorString(hipGetLastError()));
        *it = hp[slot].it;
        if (hp[slot].done != 0) return HGMM_OK;
        if (!ahead) return fail(c, HGMM_ERR_STATE, "%s did not stop within its budget", what);      // cannot happen; never spin
        slot ^= 1;
    }
}

// ---- the workspace of a tree build, serial or forest ----------------------------------------------------------------------
// The partition's tables and the buffers the points travel through, for n points (n_pad: the arrays' stride) in at most
// maxP parent segments at the last of L levels.  The resident cloud (level-0 order == sorted order at level 0) and its
// weights are never overwritten: the first scatter goes A -> B (t_parent), later ones alternate between B and a third
// buffer C (t_xs3); the weights' buffers (t_w2, t_w3) pair up with the coordinates'.
struct BuildWorkspace {
    int *chunk_first, *n_chunks_dev;            // t_seg: two segment tables [8 maxP + 2], chunk_first [2 (maxP + 2)], the chunk count
    int *chunk_desc, *hist, *chunk_off;         // t_chunks: [max_chunks][3], then [max_chunks][8] twice
    double* partials;                           // t_partials: [max_chunks][8][NMOM]
    int* cur[2];                                // t_current: two assignments (iteration e of an overlapped level writes buffer e & 1)
    // this level's points, weights (NULL: none) and segment table, and where the partition puts the next level's
    const double *xs, *w;
    double *xs_next, *w_next;
    int *seg, *seg_next;
    double *xs_b, *xs_c, *w_b, *w_c;            // the buffers B and C of the points and of the weights

    // xs0 / w0: the resident cloud and its weights (w0 == NULL: an unweighted build)
    int take(hgmm_ctx* c, int64_t n, int64_t n_pad, int64_t maxP, int L, const double* xs0, const double* w0) {
        const bool weighted = w0 != nullptr;
        const int64_t max_chunks = n / CH + maxP + 8;
        HGMM_TRY(ensure(c, c->t_current, sizeof(int) * 2 * n_pad));
        HGMM_TRY(ensure(c, c->t_parent, sizeof(double) * 3 * n_pad));
        if (weighted) HGMM_TRY(ensure(c, c->t_w2, sizeof(double) * n_pad));
        HGMM_TRY(ensure(c, c->t_seg, sizeof(int) * (2 * (8 * maxP + 2) + 2 * (maxP + 2) + 8)));
        HGMM_TRY(ensure(c, c->t_chunks, sizeof(int) * (size_t)(3 + 8 + 8) * max_chunks));
        HGMM_TRY(ensure(c, c->t_partials, sizeof(double) * (size_t)8 * NMOM * max_chunks));
        if (L > 2) HGMM_TRY(ensure(c, c->t_xs3, sizeof(double) * 3 * n_pad));
        if (L > 2 && weighted) HGMM_TRY(ensure(c, c->t_w3, sizeof(double) * n_pad));
        seg = c->t_seg.as<int>();
        seg_next = seg + (8 * maxP + 2);
        chunk_first = seg_next + (8 * maxP + 2);
        n_chunks_dev = chunk_first + (maxP + 2) * 2;
        chunk_desc = c->t_chunks.as<int>();
        hist = chunk_desc + 3 * max_chunks;
        chunk_off = hist + 8 * max_chunks;
        partials = c->t_partials.as<double>();
        cur[0] = c->t_current.as<int>();
        cur[1] = cur[0] + n_pad;
        xs_b = c->t_parent.as<double>();
        xs_c = L > 2 ? c->t_xs3.as<double>() : nullptr;
        w_b = weighted ? c->t_w2.as<double>() : nullptr;
        w_c = (weighted && L > 2) ? c->t_w3.as<double>() : nullptr;
        xs = xs0;
        w = w0;
        xs_next = xs_b;
        w_next = w_b;
        return HGMM_OK;
    }
    // the partition has been enqueued: the next level's buffers become the current ones (A -> B -> C -> B -> ...)
    void advance() {
        xs = xs_next;
        w = w_next;
        std::swap(seg, seg_next);
        xs_next = (xs == xs_b) ? xs_c : xs_b;
        w_next = (xs == xs_b) ? w_c : w_b;
    }
};

// The levels' q traces back to back, as both builds hand them out: copy(at, l, take) puts the first `take` = min(iters[l],
// trace_cap) values of level l at position `at` of the caller's array, as far as q_capacity reaches.  Returns sum iters.
template <class Copy>
inline int gather_traces(const int* iters, int L, int trace_cap, int q_capacity, Copy&& copy) {
    int at = 0;
    for (int l = 0; l < L; ++l) {
        const int take = std::min(std::min(iters[l], trace_cap), q_capacity - at);
        if (take > 0) copy(at, l, take);
        at += iters[l];
    }
    return at;
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

// ---- a set of B registrations: what the E-step, normal-equation, solve and score launches of tree_batch.hip work on ------
// Either the pairs of the resident forest (hgmm_tree_register_batch / _score_batch) or B start poses of the serial pair
// (hgmm_tree_register_multi / _score_multi; hgmm_tree_register's device loop with B = 1), or R hypotheses over the forest,
// each naming its pair (hgmm_tree_register_batch_multi / _score_batch_multi).
struct RegSet {
    struct One {
        int64_t first, count;                  // its target's slice of `tg`
        double rmax, mu_rmax;                  // largest |x| of the target, largest |mu_j| of the tree: reg_extent
        double wsum;                           // sum of the target's weights; (double)count without
        int owner = 0;                         // (owned sets) the forest pair whose tree and target these are
    };
    bool owned = false;                        // hypotheses over the forest: prep is [F.B][T], member r reads tree regs[r].owner
    bool shared_tree = false;                  // one tree and one target for all (the SHARED kernels): prep is [T], not [B][T]
    std::vector<One> regs;                     // [B]
    const double* tg = nullptr;                // device: the targets' structure of arrays [3][tg_pad]
    int64_t tg_pad = 0;
    const double* w = nullptr;                 // device, parallel to tg: the targets' weights; NULL: none
    const double* prep = nullptr;              // device: the node tables
    int T = 0, L = 0;
    DevBuf* momq = nullptr;                    // the fixed-point sums, slice b = [T][4] ...
    bool* momq_clean = nullptr;                // ... their MomqScope flag ...
    size_t momq_bytes = 0;                     // ... and what a use opens them at
    DevBuf* table = nullptr;                   // RegTable
    int B() const { return (int)regs.size(); }
    unsigned gx() const {                      // chunks of the longest target: the launches are gx x B workgroups
        int64_t longest = 0;
        for (const One& r : regs) longest = std::max(longest, r.count);
        return nblk(longest, CH);
    }
};
// the resident forest's pairs (the caller has checked nodes_ready and B == F.B == F.tg_B)
inline RegSet reg_set_forest(hgmm_ctx* c) {
    const ForestState& F = c->forest;
    RegSet s;
    for (int b = 0; b < F.B; ++b)
        s.regs.push_back({F.tg_first[b], F.tg_counts[b], F.tg_rmax[b], F.mu_rmax[b], F.tg_w.total(F.tg_counts[b], b)});
    s.tg = c->fr_tg.as<double>();
    s.tg_pad = F.tg_pad;
    s.w = F.tg_w.ptr();
    s.prep = c->fr_prep.as<double>();
    s.T = F.T;
    s.L = F.L;
    s.momq = &c->fr_momq;
    s.momq_clean = &c->forest.momq_clean;
    s.momq_bytes = sizeof(unsigned long long) * 4 * (size_t)F.T * F.B;
    s.table = &c->fr_reg;
    return s;
}
// R hypotheses over the resident forest, hypothesis r on (tree pair[r], target pair[r]) (the caller has checked the state and
// every pair[r]): on fm_momq / fm_reg, which leaves the sums and the table of hgmm_tree_register_batch alone
inline RegSet reg_set_forest_multi(hgmm_ctx* c, int R, const int32_t* pair) {
    const ForestState& F = c->forest;
    RegSet s = reg_set_forest(c);
    const std::vector<RegSet::One> pairs = std::move(s.regs);
    s.regs.clear();
    for (int r = 0; r < R; ++r) {
        s.regs.push_back(pairs[pair[r]]);
        s.regs.back().owner = pair[r];
    }
    s.owned = true;
    s.momq = &c->fm_momq;
    s.momq_clean = &c->forest.multi_momq_clean;
    s.momq_bytes = sizeof(unsigned long long) * 4 * (size_t)F.T * R;
    s.table = &c->fm_reg;
    return s;
}
// K start poses of the serial pair (the caller has checked the tree and the target; tree.mu_rmax: tree_mu_rmax_resident,
// which the score does not need).  multi: on tm_momq / tm_reg, which leaves the serial call's state alone; otherwise
// hgmm_tree_register's own buffers, K = 1 -- t_momq at the [T][NMOM] words every other use of it opens it at, and fr_reg.
inline RegSet reg_set_pair(hgmm_ctx* c, int K, bool multi) {
    RegSet s;
    s.shared_tree = true;
    s.regs.assign(K, {0, c->tgt_n, c->tgt_rmax, c->tree.mu_rmax, c->tgt_w.total(c->tgt_n)});
    s.tg = c->tgt_soa64.as<double>();
    s.tg_pad = c->tgt_pad;
    s.w = c->tgt_w.ptr();
    s.prep = c->t_prep.as<double>();
    s.T = c->tree.T;
    s.L = c->tree.L;
    s.momq = multi ? &c->tm_momq : &c->t_momq;
    s.momq_clean = multi ? &c->tree.multi_momq_clean : &c->tree.momq_clean;
    s.momq_bytes = sizeof(unsigned long long) * (multi ? 4 * (size_t)K : (size_t)NMOM) * s.T;
    s.table = multi ? &c->tm_reg : &c->fr_reg;
    return s;
}
// (tree_batch.hip) up to max_iter iterations of every registration of the set from (rot [B][9], t [B][3]), on the host's
// solve or -- reg_device_solve -- the device's; the arguments are hgmm_tree_register_batch's.  Opens and closes the sums.
int register_set(hgmm_ctx* c, const RegSet& set, double* rot, double* t, double scale, double lambda_c, int max_iter, double tol,
                 double* q_prev_inout, int32_t* iters_out, int32_t* status_out, double* trace);
// (tree_batch.hip) hgmm_tree_score's summary of every registration of the set at (rot, t; NULL: identity) -> summary_out [B][8]
int score_set(hgmm_ctx* c, const RegSet& set, const double* rot, const double* t, double scale, double lambda_c,
              double maha2_max, double* summary_out);

// the device table of B registrations: [B entries][28 B doubles: the normal equations][B words: forest_target_kernel's r2max]
struct RegTable {
    ForestRegPair* pairs;
    double* out;
    unsigned long long* r2max;
};
inline int reg_table(hgmm_ctx* c, DevBuf& buf, int B, RegTable* tb) {
    HGMM_TRY(ensure(c, buf, (sizeof(ForestRegPair) + 28 * sizeof(double) + sizeof(unsigned long long)) * (size_t)B + 512));
    tb->pairs = buf.as<ForestRegPair>();
    tb->out = reinterpret_cast<double*>(tb->pairs + B);
    tb->r2max = reinterpret_cast<unsigned long long*>(tb->out + (size_t)28 * B);
    return HGMM_OK;
}
// a registration's table entry: its target's slice and weight sum, everything else zero (one that takes no part)
inline ForestRegPair reg_pair(const RegSet::One& r) {
    ForestRegPair pr;
    std::memset(&pr, 0, sizeof pr);
    pr.tg_first = (int)r.first;
    pr.tg_count = (int)r.count;
    pr.tg_wtotal = r.wsum;
    pr.owner = r.owner;
    return pr;
}
// ... of one that takes part: its transform and the fixed-point encoding of its next E-step
inline void reg_pair_fill(ForestRegPair& pr, const Rigid& tf, const RegSet::One& r) {
    pr.active = 1;
    pr.tf = tf;
    double D = 1.0;
    int F = 0;
    reg_encoding(reg_extent(tf, r.rmax, r.mu_rmax), pr.tg_wtotal, &D, &F);
    pr.inv_d = 1.0 / D;
    pr.fix_scale = std::ldexp(1.0, F);
    pr.d_ext = D;
    pr.inv_scale = std::ldexp(1.0, -F);
    pr.tg_rmax = r.rmax;
    pr.mu_rmax = r.mu_rmax;
}
// What the four weight entries (hgmm_tree_set_target_weights[_batch], hgmm_tree_set_source_weights[_batch]) do once their own
// state checks have passed and w is not NULL.  `what`: the entry's name; `noun`: "target" / "cloud"; batch: the messages name
// the member (the serial entries: B = 1, no index).  The B members lie back to back in an array of `pad` doubles, resident[b]
// points each.  In this order: counts[b] against resident[b]; every w[b] finite, >= 0 and not all zero (a NULL member: 1.0
// per point, its count as the sum -- gamma * 1.0 is gamma, so it keeps its unweighted bits); a refusal up to here leaves the
// previous weights in force.  Then set.drop(): what is left to fail is the device, and then no weights are in force.  Upload
// into set.buf and publish the sums (all members NULL: the set stays off).
inline int upload_weights(hgmm_ctx* c, const char* what, const char* noun, bool batch, int B, const double* const* w,
                   const int64_t* counts, const int64_t* resident, int64_t pad, WeightSet<double>& set) {
    std::vector<double> sum(B), padded((size_t)pad, 0.0);
    bool any = false;
    int64_t at = 0;
    for (int b = 0; b < B; at += counts[b], ++b) {
        if (counts[b] != resident[b])
            return batch ? fail(c, HGMM_ERR_ARG, "%s: counts[%d] = %lld, but the resident %s %d has %lld points", what, b,
                                (long long)counts[b], noun, b, (long long)resident[b])
                         : fail(c, HGMM_ERR_ARG, "%s: %lld weights, but the resident %s has %lld points", what,
                                (long long)counts[b], noun, (long long)resident[b]);
        double* slot = padded.data() + at;
        if (!w[b]) {
            std::fill(slot, slot + counts[b], 1.0);
            sum[b] = (double)counts[b];
            continue;
        }
        char label[96];
        if (batch) snprintf(label, sizeof label, "%s (%s %d)", what, noun, b);
        HGMM_TRY(check_point_weights(c, batch ? label : what, w[b], counts[b], &sum[b]));
        std::copy(w[b], w[b] + counts[b], slot);
        any = true;
    }
    set.drop();
    if (!any) return HGMM_OK;
    HGMM_TRY(ensure(c, set.buf, sizeof(double) * padded.size()));
    HGMM_HIP(c, hipMemcpyAsync(set.buf.p, padded.data(), sizeof(double) * padded.size(), hipMemcpyHostToDevice, c->stream));
    HGMM_HIP(c, ctx_stream_sync(c));
    set.publish(sum);
    return HGMM_OK;
}

// ---- a new target: begin, the upload or hand-over launches of the caller, publish -----------------------------------------
// the serial target (hgmm_tree_set_target, hgmm_voxel_to_target).  From begin on a failure leaves no target, and the previous
// target's weights are gone whatever happens.  publish: n points in tgt_soa64 [3][pad], r2max their largest |x|^2; wsum: the
// sum of the weights the caller has put into tgt_w.buf, NULL: none
inline void target_begin(hgmm_ctx* c) { c->tgt_n = 0; c->tgt_w.drop(); }
inline void target_publish(hgmm_ctx* c, int64_t n, int64_t pad, double r2max, const double* wsum) {
    c->tgt_rmax = std::sqrt(r2max);
    c->tgt_n = n;
    c->tgt_pad = pad;
    if (wsum) c->tgt_w.publish({*wsum});
}
inline double r2_of_bits(unsigned long long bits) {        // (forest_target_kernel / handover_kernel: bits of a double >= 0)
    double r2;
    std::memcpy(&r2, &bits, sizeof r2);
    return r2;
}
// the forest's targets (hgmm_tree_set_targets_batch[_f32], hgmm_voxel_to_targets_batch), likewise: B targets of counts[b]
// points back to back in fr_tg [3][pad], r2bits[b] the bits of their largest |x|^2, wsums [B] or NULL
inline void forest_targets_begin(hgmm_ctx* c) { c->forest.tg_B = 0; c->forest.tg_w.drop(); }
inline void forest_targets_publish(hgmm_ctx* c, int B, const int64_t* counts, const unsigned long long* r2bits, int64_t pad,
                                   const double* wsums) {
    ForestState& F = c->forest;
    F.tg_counts.assign(counts, counts + B);
    F.tg_first.resize((size_t)B);
    F.tg_rmax.resize((size_t)B);
    int64_t at = 0;
    for (int b = 0; b < B; at += counts[b], ++b) {
        F.tg_first[b] = at;
        F.tg_rmax[b] = std::sqrt(r2_of_bits(r2bits[b]));
    }
    F.tg_pad = pad;
    F.tg_B = B;
    if (wsums) F.tg_w.publish(std::vector<double>(wsums, wsums + B));
}

}  // namespace hgmm
