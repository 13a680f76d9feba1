// Host side of hgmm_kmeans_fit_batch's tables (kmeans_batch.h): the serial grids of every member and where its pieces lie in
// the batch's buffers, and the (member, local index) entry of every workgroup of the four launches whose grid depends on the
// clouds' sizes.  Plain C++17, nothing of HIP or of the library: tests/kmeans_batch_plan_main.cpp builds it with the host
// compiler under the address and undefined-behaviour sanitizers and checks what the kernels rely on.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace hgmm {

// (kmeans_kernels.hip's KM_BLOCK, KM_GROUP, KM_MAX_TRIALS: kmeans_batch.h asserts that they are these)
constexpr int KMB_BLOCK = 256;                     // points per block
constexpr int KMB_GROUP = 16;                      // blocks per seeding workgroup
constexpr int KMB_TRIALS = 16;                     // candidate slots per centre

struct KmBatchWg { int member, local; };

struct KmBatchPlan {
    int64_t n, n_pad, src_first;                   // n_pad = G * 4096; src_first: the member's first row in the resident cloud
    int B, G, nb_assign, nb_acc;                   // blocks, seeding / assignment / accumulator workgroups of a cloud of n points
    size_t row0;                                   // first row in the per-point buffers (the cloud copy: 3 * row0 doubles)
    size_t blk0;                                   // first double of its block / group / candidate tables
    size_t partial0, inertia0;                     // ... of its per-cluster partial sums, of its inertia partials
};

struct KmBatchLayout {
    std::vector<KmBatchPlan> plan;                 // [B]
    std::vector<KmBatchWg> tab;                    // first | step | assign | accum, each member after member
    size_t rows = 0, blk = 0, npartial = 0, ninertia = 0;          // the buffers' sizes, in elements
    size_t wg_first = 0, wg_step = 0, wg_assign = 0, wg_acc = 0;   // the four launches' grids
    int maxG = 0;
    static size_t blk_doubles(int B, int G) {      // bsum [B] | part [2][T][B] | part16 [2][T][G] | g0 [G] | gprefix [G]
        return (size_t)B + 2 * (size_t)(B + G) * KMB_TRIALS + 2 * (size_t)G;
    }
};

// counts [B] >= 1 each; k_alloc: centres per partial table; acc_lds: the LDS accumulator (one workgroup per CU, else two)
inline KmBatchLayout km_batch_layout(int B, const int64_t* counts, int k_alloc, bool acc_lds, int cus) {
    KmBatchLayout L;
    L.plan.resize((size_t)B);
    int64_t src_at = 0;
    for (int b = 0; b < B; ++b) {
        KmBatchPlan& p = L.plan[b];
        p.n = counts[b];
        p.src_first = src_at;
        src_at += p.n;
        p.B = (int)((p.n + KMB_BLOCK - 1) / KMB_BLOCK);
        p.G = (p.B + KMB_GROUP - 1) / KMB_GROUP;
        p.n_pad = (int64_t)p.G * KMB_GROUP * KMB_BLOCK;
        p.nb_assign = (int)((p.n + 2 * KMB_BLOCK - 1) / (2 * KMB_BLOCK));
        p.nb_acc = (int)std::min<int64_t>((acc_lds ? 1 : 2) * (int64_t)cus, p.B);
        p.row0 = L.rows;
        L.rows += (size_t)p.n_pad;
        p.blk0 = L.blk;
        L.blk += KmBatchLayout::blk_doubles(p.B, p.G);
        p.partial0 = L.npartial;
        L.npartial += 4 * (size_t)k_alloc * p.nb_acc;
        p.inertia0 = L.ninertia;
        L.ninertia += (size_t)p.nb_assign;
        L.wg_first += p.B; L.wg_step += p.G; L.wg_assign += p.nb_assign; L.wg_acc += p.nb_acc;
        L.maxG = std::max(L.maxG, p.G);
    }
    L.tab.resize(L.wg_first + L.wg_step + L.wg_assign + L.wg_acc);
    size_t a = 0, s = L.wg_first, as = s + L.wg_step, ac = as + L.wg_assign;
    for (int b = 0; b < B; ++b) {
        const KmBatchPlan& p = L.plan[b];
        for (int i = 0; i < p.B; ++i) L.tab[a++] = {b, i};
        for (int i = 0; i < p.G; ++i) L.tab[s++] = {b, i};
        for (int i = 0; i < p.nb_assign; ++i) L.tab[as++] = {b, i};
        for (int i = 0; i < p.nb_acc; ++i) L.tab[ac++] = {b, i};
    }
    return L;
}

}  // namespace hgmm
