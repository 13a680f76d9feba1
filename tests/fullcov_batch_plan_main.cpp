// Exercises the host side of hgmm_fullcov_fit_batch's tables (csrc/fullcov_batch_plan.h: fc_batch_layout) -- plain C++17, no
// HIP -- and checks what the batched kernels rely on.  Built with the address and undefined-behaviour sanitizers and run by
// tests/test_fullcov_batch_cpu.py.
//   fullcov_batch_plan J cus n_0 n_1 ...
// Prints one line "ok B=.. rows=.. wgs=.. J16=.." or the first violated condition (exit status 1).
#include "fullcov_batch_plan.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

#define REQUIRE(cond)                                                        \
    do {                                                                     \
        if (!(cond)) { std::printf("violated: %s (member %d)\n", #cond, b); return 1; } \
    } while (0)

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    const int J = std::atoi(argv[1]), cus = std::atoi(argv[2]);
    std::vector<int64_t> counts;
    for (int i = 3; i < argc; ++i) counts.push_back(std::atoll(argv[i]));
    const int B = (int)counts.size();
    const hgmm::FcBatchLayout L = hgmm::fc_batch_layout(B, counts.data(), J, cus);
    int b = -1;
    REQUIRE((int)L.plan.size() == B);
    REQUIRE(L.J16 % 16 == 0 && L.J16 >= J && L.J16 - J < 16);
    int64_t rows = 0, wgs = 0;
    int max_grid = 0;
    // every member: the serial grid of a cloud of its size, pieces that follow each other without overlap, and the serial
    // tile-to-workgroup map covering each of its tiles exactly once, in order
    for (b = 0; b < B; ++b) {
        const hgmm::FcBatchPlan& p = L.plan[b];
        const int64_t n = counts[b];
        REQUIRE(p.n == n && p.first == rows);
        REQUIRE(p.tiles * 16 >= n && (p.tiles - 1) * 16 < n);
        REQUIRE(p.grid == (p.tiles < cus ? (int)p.tiles : cus));
        REQUIRE(p.wg0 == wgs && p.table0 == (size_t)b * L.J16);
        int64_t next = 0;
        for (int blk = 0; blk < p.grid; ++blk) {
            int64_t t0 = -1, t1 = -1;
            hgmm::fc_batch_tiles(p, blk, &t0, &t1);
            if (t0 >= t1) continue;                              // (the serial map leaves the last blocks idle when tiles % grid is small)
            REQUIRE(t0 == next && t1 <= p.tiles);
            next = t1;
        }
        REQUIRE(next == p.tiles);
        {
            int64_t t0 = -1, t1 = -1;
            hgmm::fc_batch_tiles(p, 0, &t0, &t1);               // (a member without a workgroup: an empty range, no division)
            REQUIRE(p.grid > 0 || (t0 == 0 && t1 == 0));
        }
        rows += n;
        wgs += p.grid;
        max_grid = p.grid > max_grid ? p.grid : max_grid;
    }
    b = -1;
    REQUIRE(rows == L.rows && wgs == L.wgs && max_grid == L.max_grid);
    REQUIRE(L.components == (size_t)B * L.J16);
    REQUIRE(L.partial_doubles == (size_t)L.wgs * L.J16 * 10);
    // the fused launch's table: member after member, local blocks 0 .. grid_b - 1, nothing else
    size_t at = 0;
    for (b = 0; b < B; ++b)
        for (int i = 0; i < L.plan[b].grid; ++i, ++at) REQUIRE(at < L.tab.size() && L.tab[at].member == b && L.tab[at].local == i);
    b = -1;
    REQUIRE(at == L.tab.size() && at == (size_t)L.wgs);
    std::printf("ok B=%d rows=%lld wgs=%lld J16=%d\n", B, (long long)L.rows, (long long)L.wgs, L.J16);
    return 0;
}
