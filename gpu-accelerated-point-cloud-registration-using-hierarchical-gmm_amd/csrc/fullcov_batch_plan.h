// Host side of hgmm_fullcov_fit_batch's tables (fullcov_batch.h): the serial grid of every member's one-pass launch, where its
// workgroups lie in the batch's fused launch, where its pieces lie in the batch's buffers, and the (member, local block)
// entry of every workgroup of the fused launch.  Plain C++17, nothing of HIP or of the library:
// tests/fullcov_batch_plan_main.cpp builds it with the host compiler under the address and undefined-behaviour sanitizers
// and checks what the kernels rely on.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace hgmm {

// (fullcov_kernels.hip's FT_P, NMOM of tree_device.h: fullcov_batch.h asserts that they are these)
constexpr int FCB_TILE = 16;                       // points per tile of the one-pass kernel
constexpr int FCB_NMOM = 10;                       // statistics per component

struct FcBatchWg { int member, local; };

struct FcBatchPlan {
    int64_t n, first;                              // the member's points and its first row in the resident batch cloud
    int64_t tiles;                                 // ceil(n / 16)
    int grid;                                      // min(tiles, CUs): the workgroups of the serial launch on this cloud alone
    int64_t wg0;                                   // the prefix table: its workgroups are [wg0, wg0 + grid) of the fused launch,
                                                   // which is also its first block of partials ([J16][NMOM] doubles each) and
                                                   // its first share of q
    size_t table0;                                 // first component of its slices of the parameter, moment and prep tables
};

struct FcBatchLayout {
    std::vector<FcBatchPlan> plan;                 // [B]
    std::vector<FcBatchWg> tab;                    // [wgs], member after member
    int J16 = 0;
    int64_t wgs = 0;                               // the fused launch's grid = sum of the members' grids
    int64_t rows = 0;                              // sum of the members' points
    size_t components = 0;                         // B * J16: the length of every per-component table
    size_t partial_doubles = 0;                    // wgs * J16 * NMOM
    int max_grid = 0;
};

// counts [B] >= 1 each (a member without points has no tile, no workgroup and no origin: the entry refuses it); J >= 1
inline FcBatchLayout fc_batch_layout(int B, const int64_t* counts, int J, int cus) {
    FcBatchLayout L;
    L.J16 = (J + 15) / 16 * 16;
    L.plan.resize((size_t)B);
    for (int b = 0; b < B; ++b) {
        FcBatchPlan& p = L.plan[b];
        p.n = counts[b];
        p.first = L.rows;
        L.rows += p.n;
        p.tiles = (p.n + FCB_TILE - 1) / FCB_TILE;
        p.grid = (int)std::min<int64_t>(p.tiles, cus);
        p.wg0 = L.wgs;
        L.wgs += p.grid;
        p.table0 = (size_t)b * L.J16;
        L.max_grid = std::max(L.max_grid, p.grid);
    }
    L.components = (size_t)B * L.J16;
    L.partial_doubles = (size_t)L.wgs * L.J16 * FCB_NMOM;
    L.tab.resize((size_t)L.wgs);
    size_t at = 0;
    for (int b = 0; b < B; ++b)
        for (int i = 0; i < L.plan[b].grid; ++i) L.tab[at++] = {b, i};
    return L;
}

// the tiles [t0, t1) of local block `blk` of a member: the serial kernel's tile-to-workgroup map (full_fused_body)
inline void fc_batch_tiles(const FcBatchPlan& p, int blk, int64_t* t0, int64_t* t1) {
    if (p.grid < 1) { *t0 = *t1 = 0; return; }     // (a member without points: no workgroup ever asks)
    const int64_t per = (p.tiles + p.grid - 1) / p.grid;
    *t0 = (int64_t)blk * per;
    *t1 = std::min(*t0 + per, p.tiles);
}

}  // namespace hgmm
