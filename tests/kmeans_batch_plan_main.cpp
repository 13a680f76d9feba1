// Exercises the host side of hgmm_kmeans_fit_batch's tables (csrc/kmeans_batch_plan.h: km_batch_layout) -- plain C++17, no
// HIP -- and checks what the batched kernels rely on.  Built with the address and undefined-behaviour sanitizers and run by
// tests/test_kmeans_batch_cpu.py.
//   kmeans_batch_plan k_alloc acc_lds cus n_0 n_1 ...
// Prints one line "ok B=.. rows=.. wg=../../../.." or the first violated condition (exit status 1).
#include "kmeans_batch_plan.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

#define REQUIRE(cond)                                                        \
    do {                                                                     \
        if (!(cond)) { std::printf("violated: %s (member %d)\n", #cond, b); return 1; } \
    } while (0)

int main(int argc, char** argv) {
    if (argc < 5) return 2;
    const int k_alloc = std::atoi(argv[1]), acc_lds = std::atoi(argv[2]), cus = std::atoi(argv[3]);
    std::vector<int64_t> counts;
    for (int i = 4; i < argc; ++i) counts.push_back(std::atoll(argv[i]));
    const int B = (int)counts.size();
    const hgmm::KmBatchLayout L = hgmm::km_batch_layout(B, counts.data(), k_alloc, acc_lds != 0, cus);
    int b = -1;
    REQUIRE((int)L.plan.size() == B);
    REQUIRE(L.tab.size() == L.wg_first + L.wg_step + L.wg_assign + L.wg_acc);
    size_t rows = 0, blk = 0, partial = 0, inertia = 0;
    int64_t src = 0;
    // every member: the serial grids of a cloud of its size, pieces that follow each other without overlap
    for (b = 0; b < B; ++b) {
        const hgmm::KmBatchPlan& p = L.plan[b];
        const int64_t n = counts[b];
        REQUIRE(p.n == n && p.src_first == src);
        REQUIRE((int64_t)p.B * 256 >= n && (int64_t)(p.B - 1) * 256 < n);
        REQUIRE(p.G * 16 >= p.B && (p.G - 1) * 16 < p.B);
        REQUIRE(p.n_pad == (int64_t)p.G * 4096 && p.n_pad >= n && p.n_pad - n < 4096);
        REQUIRE((int64_t)p.nb_assign * 512 >= n && (int64_t)(p.nb_assign - 1) * 512 < n);
        REQUIRE(p.nb_acc >= 1 && p.nb_acc <= p.B && p.nb_acc <= (acc_lds ? 1 : 2) * cus);
        REQUIRE(p.nb_acc == p.B || p.nb_acc == (acc_lds ? 1 : 2) * cus);
        REQUIRE(p.row0 == rows && p.row0 % 4096 == 0 && p.blk0 == blk && p.partial0 == partial && p.inertia0 == inertia);
        rows += (size_t)p.n_pad;
        blk += hgmm::KmBatchLayout::blk_doubles(p.B, p.G);
        partial += 4 * (size_t)k_alloc * p.nb_acc;
        inertia += (size_t)p.nb_assign;
        src += n;
    }
    b = -1;
    REQUIRE(rows == L.rows && blk == L.blk && partial == L.npartial && inertia == L.ninertia);
    // every launch's table: member after member, local indices 0 .. grid_b - 1, nothing else
    size_t at = 0;
    for (int launch = 0; launch < 4; ++launch) {
        size_t total = 0;
        for (b = 0; b < B; ++b) {
            const hgmm::KmBatchPlan& p = L.plan[b];
            const int grid = launch == 0 ? p.B : launch == 1 ? p.G : launch == 2 ? p.nb_assign : p.nb_acc;
            for (int i = 0; i < grid; ++i, ++at) REQUIRE(at < L.tab.size() && L.tab[at].member == b && L.tab[at].local == i);
            total += (size_t)grid;
        }
        b = -1;
        REQUIRE(total == (launch == 0 ? L.wg_first : launch == 1 ? L.wg_step : launch == 2 ? L.wg_assign : L.wg_acc));
    }
    REQUIRE(at == L.tab.size());
    int maxG = 0;
    for (const hgmm::KmBatchPlan& p : L.plan) maxG = p.G > maxG ? p.G : maxG;
    REQUIRE(maxG == L.maxG);
    std::printf("ok B=%d rows=%zu wg=%zu/%zu/%zu/%zu\n", B, L.rows, L.wg_first, L.wg_step, L.wg_assign, L.wg_acc);
    return 0;
}
