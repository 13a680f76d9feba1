// Batched KMeans initialiser (hgmm_kmeans_fit_batch): B clouds seeded and clustered by the same launches.  Included once, at
// the end of kmeans_kernels.hip.
//
// Every kernel of the serial chain has a twin here that runs the SAME BODY (kmeans_body.h, kmpp_tail_body) for many clouds:
// a workgroup looks up its member and its place in that member's launch -- one (member, local index) entry per workgroup
// for the four launches whose grid depends on the cloud's size, blockIdx.y for those whose grid depends on k alone --,
// declares the serial kernel's arguments as locals from the member's row of KmBatchMember, and runs the body with KM_WG /
// KM_NWG naming what the serial launch of that cloud alone would have given it.  Everything a member's workgroups read or
// write is the member's own: its copy of the cloud, closest[], labels, block / group / candidate tables (double-buffered by
// centre parity, as in the serial chain), partials, sums, control word, changed counter.  The fused seeding launch's one
// shared-while-written array, `closest`, is therefore shared among one member's workgroups only, and the argument above
// kmpp_fused_kernel holds member by member.
//
// THE CLOUD COPY.  The members lie packed in the resident batch cloud: member b starts at an arbitrary row and the rows
// behind its last one are member b + 1's.  The serial kernels see row 0 at the start of a buffer and rows that read as the
// origin up to a multiple of 256.  kmb_pack_kernel therefore copies every member, in one launch, into a buffer of the batch's
// own where it starts at a multiple of 4096 rows (one seeding workgroup) and is followed by zero rows up to the next one:
// each member sees what the serial cloud shows, at a cost of at most 4095 rows.
#include "kmeans_batch_plan.h"

namespace hgmm {

static_assert(KMB_BLOCK == KM_BLOCK && KMB_GROUP == KM_GROUP && KMB_TRIALS == KM_MAX_TRIALS, "kmeans_batch_plan.h");

struct KmBatchMember {
    const double* xs;                 // double [3][n_pad]: the member's copy of its cloud
    int64_t n, n_pad;                 // n_pad = G * 4096
    int64_t src_first;                // its first row in the resident batch cloud
    int64_t first_id;                 // seeding: the first centre
    double tol_abs;
    double* closest;                  // double [n_pad]
    int32_t* labels;                  // int32 [n_pad]
    double* mind2;                    // double [n_pad]
    double* bsum;                     // double [B]          the first kernel's block sums
    double* part;                     // double [2][KM_MAX_TRIALS][B]
    double* part16;                   // double [2][KM_MAX_TRIALS][G]
    double* g0;                       // double [G]
    double* gprefix;                  // double [G]          (unused by the one-launch form; the tail body's argument)
    double* seeds;                    // double [k][3]       the seeding's `centres`
    double* c3;                       // double [k][3]       the Lloyd loop's centres
    double* c4;                       // double [k][4]
    double* cand_xyz;                 // double [2][KM_MAX_TRIALS][3]
    int64_t* ids;                     // int64 [k]
    int64_t* cand;                    // int64 [2][KM_MAX_TRIALS]
    const double* rand;               // double [k - 1][n_trials]
    double* partial;                  // double [nb_acc][k_alloc][4]
    double* out;                      // double [4 k + 2]
    double* inertia_part;             // double [nb_assign]
    unsigned long long* changed;
    KmCtl* ctl;
    int B, G, nb_assign, nb_acc;      // the serial grids of a cloud of n points
};
// (KmBatchWg, a workgroup's (member, local index): kmeans_batch_plan.h)

// A pointer read from the member table is a generic pointer to the compiler and would be dereferenced by flat loads, a
// wave-uniform centre never by a scalar load; the table holds device allocations only, so the pointer is rebuilt from its bits
// as one into the global address space -- what the serial kernels' arguments are by themselves (flat_fused_device.h does the same)
template <class T>
__device__ __forceinline__ T* km_global(T* p) {
    typedef __attribute__((address_space(1))) T* gptr;
    return (T*)(gptr)(uintptr_t)p;
}

#undef KM_WG
#undef KM_NWG
#define KM_WG km_wg
#define KM_NWG km_nwg

// grid: the seeding workgroups of all members (G_b each), 1024 threads, four rows per thread
__global__ __launch_bounds__(KM_STEP_BLOCK) void kmb_pack_kernel(const KmBatchMember* __restrict__ mem,
                                                                 const KmBatchWg* __restrict__ tab,
                                                                 const double* __restrict__ src, int64_t src_pad) {
    const KmBatchWg wg = tab[blockIdx.x];
    const KmBatchMember& m = mem[wg.member];
    double* xs = const_cast<double*>(km_global(m.xs));
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int64_t i = (int64_t)wg.local * (KM_GROUP * KM_BLOCK) + q * KM_STEP_BLOCK + threadIdx.x;   // < n_pad
        const bool ok = i < m.n;
        const int64_t s = m.src_first + (ok ? i : 0);
        const double x = src[s], y = src[src_pad + s], z = src[2 * src_pad + s];
        xs[i] = ok ? x : 0.0;
        xs[m.n_pad + i] = ok ? y : 0.0;
        xs[2 * m.n_pad + i] = ok ? z : 0.0;
        km_global(m.labels)[i] = -1;
    }
}

__global__ __launch_bounds__(KM_BLOCK) void kmb_first_kernel(const KmBatchMember* __restrict__ mem,
                                                             const KmBatchWg* __restrict__ tab) {
    const KmBatchWg wg = tab[blockIdx.x];
    const KmBatchMember& m = mem[wg.member];
    const unsigned km_wg = (unsigned)wg.local;
    constexpr bool WEIGHTED = false;
    const double* wts = nullptr;
    const double* __restrict__ xs = km_global(m.xs);
    const int64_t n = m.n, n_pad = m.n_pad, first = m.first_id;
    double* __restrict__ closest = km_global(m.closest);
    double* __restrict__ bsum = km_global(m.bsum);
    double* __restrict__ centres = km_global(m.seeds);
    int64_t* __restrict__ ids = km_global(m.ids);
#define KMEANS_BODY 1
#include "kmeans_body.h"
#undef KMEANS_BODY
}

// grid (ceil(max G / 256), B)
__global__ void kmb_group_kernel(const KmBatchMember* __restrict__ mem) {
    const KmBatchMember& m = mem[blockIdx.y];
    const int B = m.B, G = m.G;
    const double* __restrict__ bsum = km_global(m.bsum);
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    double s = 0.0;
    for (int q = 0; q < KM_GROUP; ++q) s += (g * KM_GROUP + q < B) ? bsum[g * KM_GROUP + q] : 0.0;
    km_global(m.g0)[g] = s;
}

// the member's buffers of centre j's candidates (parity j & 1), as km_plusplus's cand_b / xyz_b / part_b / part16_b
#define KMB_CAND(j) (km_global(m.cand) + (size_t)((j) & 1) * KM_MAX_TRIALS)
#define KMB_XYZ(j) (km_global(m.cand_xyz) + (size_t)((j) & 1) * 3 * KM_MAX_TRIALS)
#define KMB_PART(j) (km_global(m.part) + (size_t)((j) & 1) * m.B * KM_MAX_TRIALS)
#define KMB_PART16(j) (km_global(m.part16) + (size_t)((j) & 1) * m.G * KM_MAX_TRIALS)

// grid B: one tail workgroup per member
template <int TMAX>
__global__ __launch_bounds__(1024) void kmb_tail_kernel(const KmBatchMember* __restrict__ mem, int T, int j, int select,
                                                        int draw, int64_t rand_off) {
    const KmBatchMember& m = mem[blockIdx.x];
    __shared__ KmTailShared ts;
    double pcx, pcy, pcz;
    kmpp_tail_body<TMAX>(km_global(m.xs), m.n, m.n_pad, nullptr, km_global(m.closest), KMB_PART(j), KMB_PART16(j), m.G,
                         km_global(m.bsum), km_global(m.g0), m.B, T, j, select, draw,
                         draw ? km_global(m.rand) + rand_off : nullptr, KMB_CAND(j), KMB_XYZ(j), KMB_CAND(j + 1), KMB_XYZ(j + 1),
                         km_global(m.seeds), km_global(m.ids), km_global(m.gprefix), true, nullptr, pcx, pcy, pcz, ts);
}

// grid: the seeding workgroups of all members
template <int TMAX>
__global__ __launch_bounds__(KM_STEP_BLOCK) void kmb_step_kernel(const KmBatchMember* __restrict__ mem,
                                                                 const KmBatchWg* __restrict__ tab, int fold, int T, int j) {
    const KmBatchWg wg = tab[blockIdx.x];
    const KmBatchMember& m = mem[wg.member];
    const unsigned km_wg = (unsigned)wg.local, km_nwg = (unsigned)m.G;
    constexpr bool WEIGHTED = false;
    const double* wts = nullptr;
    const double* __restrict__ xs = km_global(m.xs);
    const int64_t n = m.n, n_pad = m.n_pad;
    double* __restrict__ closest = km_global(m.closest);
    const double* __restrict__ centres = km_global(m.seeds);
    const double* __restrict__ cand_xyz = KMB_XYZ(j);
    double* __restrict__ part = KMB_PART(j);
    double* __restrict__ part16 = KMB_PART16(j);
    const int B = m.B;
#define KMEANS_BODY 2
#include "kmeans_body.h"
#undef KMEANS_BODY
}

template <int TMAX>
__global__ __launch_bounds__(KM_STEP_BLOCK) void kmb_fused_kernel(const KmBatchMember* __restrict__ mem,
                                                                  const KmBatchWg* __restrict__ tab, int T, int j,
                                                                  int64_t rand_off) {
    const KmBatchWg wg = tab[blockIdx.x];
    const KmBatchMember& m = mem[wg.member];
    const unsigned km_wg = (unsigned)wg.local, km_nwg = (unsigned)m.G;
    constexpr bool WEIGHTED = false;
    const double* wts = nullptr;
    const double* __restrict__ xs = km_global(m.xs);
    const int64_t n = m.n, n_pad = m.n_pad;
    double* closest = km_global(m.closest);
    const double* __restrict__ part_prev = KMB_PART(j - 1);
    const double* __restrict__ part16_prev = KMB_PART16(j - 1);
    double* __restrict__ part_next = KMB_PART(j);
    double* __restrict__ part16_next = KMB_PART16(j);
    const int G = m.G, B = m.B;
    const double* __restrict__ rand_c = km_global(m.rand) + rand_off;
    const int64_t* cand_prev = KMB_CAND(j - 1);
    const double* cand_xyz_prev = KMB_XYZ(j - 1);
    int64_t* cand_next = KMB_CAND(j);
    double* cand_xyz_next = KMB_XYZ(j);
    double* __restrict__ centres = km_global(m.seeds);
    int64_t* __restrict__ ids = km_global(m.ids);
    unsigned long long* dbg = nullptr;
#define KMEANS_BODY 3
#include "kmeans_body.h"
#undef KMEANS_BODY
}

// grid B: the Lloyd loop starts from the seeds (copied here: the seeds stay for the download) or from the caller's centres
// (uploaded into `seeds`, which then reports the start); control word and changed counter cleared
__global__ void kmb_start_kernel(const KmBatchMember* __restrict__ mem, int k) {
    const KmBatchMember& m = mem[blockIdx.x];
    for (int e = threadIdx.x; e < 3 * k; e += blockDim.x) km_global(m.c3)[e] = km_global(m.seeds)[e];
    if (threadIdx.x == 0) {
        *km_global(m.ctl) = KmCtl{};
        *km_global(m.changed) = 0ull;
    }
}

// grid (ceil(k / 256), B)
__global__ void kmb_pad_centres_kernel(const KmBatchMember* __restrict__ mem, int k) {
    const KmBatchMember& m = mem[blockIdx.y];
    if (km_global(m.ctl)->done) return;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= k) return;
    km_global(m.c4)[4 * j] = km_global(m.c3)[3 * j];
    km_global(m.c4)[4 * j + 1] = km_global(m.c3)[3 * j + 1];
    km_global(m.c4)[4 * j + 2] = km_global(m.c3)[3 * j + 2];
    km_global(m.c4)[4 * j + 3] = 0.0;
}

// grid: the assignment workgroups of all members (512 points each)
__global__ __launch_bounds__(KM_BLOCK) void kmb_assign_kernel(const KmBatchMember* __restrict__ mem,
                                                              const KmBatchWg* __restrict__ tab, int k) {
    const KmBatchWg wg = tab[blockIdx.x];
    const KmBatchMember& m = mem[wg.member];
    const unsigned km_wg = (unsigned)wg.local;
    constexpr bool WEIGHTED = false;
    const double* wts = nullptr;
    const double* __restrict__ xs = km_global(m.xs);
    const int64_t n = m.n, n_pad = m.n_pad;
    const double* __restrict__ c4 = km_global(m.c4);
    int32_t* __restrict__ labels = km_global(m.labels);
    double* __restrict__ mind2 = km_global(m.mind2);
    double* __restrict__ inertia_part = km_global(m.inertia_part);
    unsigned long long* __restrict__ n_changed = km_global(m.changed);
    const int* __restrict__ done = &km_global(m.ctl)->done;
#define KMEANS_BODY 4
#include "kmeans_body.h"
#undef KMEANS_BODY
}

// grid: the accumulator workgroups of all members (nb_acc_b each, the member's contiguous runs)
template <int NSLOT>
__global__ __launch_bounds__(KM_BLOCK) void kmb_accum_kernel(const KmBatchMember* __restrict__ mem,
                                                             const KmBatchWg* __restrict__ tab, int slot0, int k_alloc) {
    const KmBatchWg wg = tab[blockIdx.x];
    const KmBatchMember& m = mem[wg.member];
    const unsigned km_wg = (unsigned)wg.local, km_nwg = (unsigned)m.nb_acc;
    constexpr bool WEIGHTED = false;
    const double* wts = nullptr;
    const double* __restrict__ xs = km_global(m.xs);
    const int64_t n = m.n, n_pad = m.n_pad;
    const int32_t* __restrict__ labels = km_global(m.labels);
    double* __restrict__ partial = km_global(m.partial);
    const int* __restrict__ done = &km_global(m.ctl)->done;
#define KMEANS_BODY 5
#include "kmeans_body.h"
#undef KMEANS_BODY
}
__global__ __launch_bounds__(KM_BLOCK) void kmb_accum_lds_kernel(const KmBatchMember* __restrict__ mem,
                                                                 const KmBatchWg* __restrict__ tab, int k_alloc) {
    const KmBatchWg wg = tab[blockIdx.x];
    const KmBatchMember& m = mem[wg.member];
    const unsigned km_wg = (unsigned)wg.local, km_nwg = (unsigned)m.nb_acc;
    constexpr bool WEIGHTED = false;
    const double* wts = nullptr;
    const double* __restrict__ xs = km_global(m.xs);
    const int64_t n = m.n, n_pad = m.n_pad;
    const int32_t* __restrict__ labels = km_global(m.labels);
    double* __restrict__ partial = km_global(m.partial);
    const int* __restrict__ done = &km_global(m.ctl)->done;
#define KMEANS_BODY 6
#include "kmeans_body.h"
#undef KMEANS_BODY
}

// grid (ceil(4 k / 32), B)
__global__ __launch_bounds__(KM_BLOCK) void kmb_reduce_kernel(const KmBatchMember* __restrict__ mem, int k_alloc, int k) {
    const KmBatchMember& m = mem[blockIdx.y];
    const unsigned km_wg = blockIdx.x;
    const double* __restrict__ partial = km_global(m.partial);
    const int nb = m.nb_acc, nib = m.nb_assign;
    const double* __restrict__ inertia_part = km_global(m.inertia_part);
    const unsigned long long* __restrict__ n_changed = km_global(m.changed);
    double* __restrict__ out = km_global(m.out);
    const int* __restrict__ done = &km_global(m.ctl)->done;
#define KMEANS_BODY 7
#include "kmeans_body.h"
#undef KMEANS_BODY
}

// grid B
__global__ __launch_bounds__(256) void kmb_update_kernel(const KmBatchMember* __restrict__ mem, int k, int max_iter) {
    const KmBatchMember& m = mem[blockIdx.x];
    const double* __restrict__ out = km_global(m.out);
    const double tol_abs = m.tol_abs;
    double* __restrict__ c3 = km_global(m.c3);
    unsigned long long* __restrict__ changed = km_global(m.changed);
    KmCtl* __restrict__ ctl = km_global(m.ctl);
#define KMEANS_BODY 8
#include "kmeans_body.h"
#undef KMEANS_BODY
}

// grid ceil(B / 256), after the loop: a member that did not stop strictly (and did not leave for an empty cluster) takes one
// more assignment against its final centres, as KMeans.fit does; the others' workgroups return at their `done` word
__global__ void kmb_final_gate_kernel(const KmBatchMember* __restrict__ mem, int nB) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nB) return;
    KmCtl* ctl = mem[b].ctl;
    ctl->done = (ctl->strict || ctl->needs_host) ? 1 : 0;
}
// ... and that assignment's inertia, member after member (0 where none was made)
__global__ void kmb_inertia_kernel(const KmBatchMember* __restrict__ mem, int nB, int k, double* __restrict__ res) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nB) return;
    res[b] = mem[b].ctl->done ? 0.0 : mem[b].out[4 * k];
}
// grid: the first kernel's workgroups of all members: labels packed as the members lie in the resident cloud
__global__ __launch_bounds__(KM_BLOCK) void kmb_labels_kernel(const KmBatchMember* __restrict__ mem,
                                                              const KmBatchWg* __restrict__ tab,
                                                              int32_t* __restrict__ packed) {
    const KmBatchWg wg = tab[blockIdx.x];
    const KmBatchMember& m = mem[wg.member];
    const int64_t i = (int64_t)wg.local * KM_BLOCK + threadIdx.x;
    if (i < m.n) packed[m.src_first + i] = km_global(m.labels)[i];
}

#undef KMB_CAND
#undef KMB_XYZ
#undef KMB_PART
#undef KMB_PART16
#undef KM_WG
#undef KM_NWG
#define KM_WG blockIdx.x
#define KM_NWG gridDim.x

}  // namespace hgmm

using namespace hgmm;

extern "C" int hgmm_kmeans_fit_batch(hgmm_ctx* c, int B, const int64_t* counts, int k, const int64_t* first_ids,
                                     const double* rand_vals, int n_trials, const double* init_centres, int max_iter,
                                     const double* tol_abs, int64_t* ids_out, double* seeds_out, double* centres_out,
                                     int32_t* n_iter_out, int32_t* strict_out, int32_t* status_out, double* inertia_out,
                                     int32_t* labels_out) {
    HGMM_ENTER(c);
    const char* what = "hgmm_kmeans_fit_batch";
    // ---- refusals: nothing resident is touched ----
    if (B < 1 || B > KM_BATCH_MAX) return fail(c, HGMM_ERR_ARG, "%s: B = %d outside 1..%d", what, B, KM_BATCH_MAX);
    if (!counts || !tol_abs || !centres_out || !n_iter_out || !strict_out || !status_out || !inertia_out)
        return fail(c, HGMM_ERR_ARG, "%s: NULL argument (counts, tol_abs, centres_out, n_iter_out, strict_out, status_out and "
                    "inertia_out are required)", what);
    const bool seeded = init_centres == nullptr;
    if (!seeded && (first_ids || rand_vals))
        return fail(c, HGMM_ERR_ARG, "%s: both seeding inputs (first_ids / rand_vals) and init_centres are given; an explicit "
                    "start skips the seeding", what);
    if (seeded && !first_ids)
        return fail(c, HGMM_ERR_ARG, "%s: neither first_ids nor init_centres is given", what);
    if (k < 1 || k > KM_MAX_K) return fail(c, HGMM_ERR_ARG, "%s: k = %d outside 1..%d", what, k, KM_MAX_K);
    if (seeded && (n_trials < 1 || n_trials > KM_MAX_TRIALS))
        return fail(c, HGMM_ERR_ARG, "%s: n_trials = %d outside 1..%d", what, n_trials, KM_MAX_TRIALS);
    if (seeded && k > 1 && !rand_vals) return fail(c, HGMM_ERR_ARG, "%s: rand_vals is NULL", what);
    if (seeded && (!ids_out || !seeds_out)) return fail(c, HGMM_ERR_ARG, "%s: ids_out / seeds_out is NULL", what);
    if (max_iter < 0) return fail(c, HGMM_ERR_ARG, "%s: max_iter = %d is negative", what, max_iter);
    const ForestState& F = c->forest;
    if (!c->have_f64 || c->n <= 0 || F.src_counts.empty())
        return fail(c, HGMM_ERR_STATE, "%s: no batch cloud is resident (call hgmm_set_points_batch_f64 / _f32 first)", what);
    if (c->comm_on())
        return fail(c, HGMM_ERR_STATE, "%s: the context has a communicator; the batched initialiser is single-rank", what);
    if (B != (int)F.src_counts.size())
        return fail(c, HGMM_ERR_STATE, "%s: B = %d, but %d clouds are resident", what, B, (int)F.src_counts.size());
    for (int b = 0; b < B; ++b)
        if (counts[b] != F.src_counts[b])
            return fail(c, HGMM_ERR_STATE, "%s: member %d: counts[%d] = %lld, but the resident cloud has %lld points", what, b,
                        b, (long long)counts[b], (long long)F.src_counts[b]);
    if (c->n > 0x7fffffff - 1024)
        return fail(c, HGMM_ERR_ARG, "%s: the batch cloud's %lld points are too many for 32-bit indices", what, (long long)c->n);
    for (int b = 0; b < B; ++b) {
        if (k > counts[b])
            return fail(c, HGMM_ERR_ARG, "%s: member %d: k = %d exceeds its %lld points", what, b, k, (long long)counts[b]);
        if (counts[b] > (int64_t)KM_TAIL_LDS_GROUPS * KM_GROUP * KM_BLOCK)
            return fail(c, HGMM_ERR_ARG, "%s: member %d: %lld points exceed the one-launch-per-centre seeding form (%lld points)",
                        what, b, (long long)counts[b], (long long)KM_TAIL_LDS_GROUPS * KM_GROUP * KM_BLOCK);
        if (seeded && (first_ids[b] < 0 || first_ids[b] >= counts[b]))
            return fail(c, HGMM_ERR_ARG, "%s: member %d: first_id = %lld out of range (its cloud has %lld points)", what, b,
                        (long long)first_ids[b], (long long)counts[b]);
    }
    // ---- the plan: every member's serial grids and its pieces of the batch's buffers ----
    const int nslot = k <= 256 ? 4 : KM_ACC_SLOTS;
    const int k_alloc = (k + 64 * nslot - 1) / (64 * nslot) * (64 * nslot);
    const bool acc_lds = k <= 1024 && !c->cfg[CFG_KMEANS_ACC_REGS];
    const int T = seeded ? n_trials : 1;
    const KmBatchLayout lay = km_batch_layout(B, counts, k_alloc, acc_lds, c->cus);
    const std::vector<KmBatchPlan>& plan = lay.plan;
    const size_t rows = lay.rows, blk = lay.blk, npartial = lay.npartial, ninertia = lay.ninertia;
    const size_t wg_first = lay.wg_first, wg_step = lay.wg_step, wg_assign = lay.wg_assign, wg_acc = lay.wg_acc;
    const int maxG = lay.maxG;
    if (sizeof(double) * npartial > KM_BATCH_MAX_PARTIALS)
        return fail(c, HGMM_ERR_ARG, "%s: the members' per-cluster partial sums take %.1f GiB together, above the limit of %.0f GiB",
                    what, (double)(sizeof(double) * npartial) / (1ull << 30), (double)KM_BATCH_MAX_PARTIALS / (1ull << 30));
    // ---- buffers of the batch's own ----
    const size_t per_small = 10 * (size_t)k + 2 * 3 * KM_MAX_TRIALS + (4 * (size_t)k + 2) + (size_t)std::max(1, (k - 1) * T);
    const size_t n_wg = wg_first + wg_step + wg_assign + wg_acc;
    HGMM_TRY(ensure(c, c->kb_tab, sizeof(KmBatchMember) * (size_t)B + sizeof(KmBatchWg) * n_wg));
    HGMM_TRY(ensure(c, c->kb_x, sizeof(double) * 3 * rows));
    HGMM_TRY(ensure(c, c->kb_points, (sizeof(double) * 2 + sizeof(int32_t)) * rows + sizeof(int32_t) * (size_t)c->n_pad));
    HGMM_TRY(ensure(c, c->kb_blocks, sizeof(double) * (blk + ninertia)));
    HGMM_TRY(ensure(c, c->kb_partial, sizeof(double) * npartial));
    HGMM_TRY(ensure(c, c->kb_small, sizeof(double) * (per_small * B + (size_t)B) +
                                        (sizeof(int64_t) * ((size_t)k + 2 * KM_MAX_TRIALS) + sizeof(KmCtl) + 8) * (size_t)B));
    KmBatchMember* mem_dev = c->kb_tab.as<KmBatchMember>();
    KmBatchWg* tab_dev = reinterpret_cast<KmBatchWg*>(mem_dev + B);
    KmBatchWg* tab_first = tab_dev;
    KmBatchWg* tab_step = tab_first + wg_first;
    KmBatchWg* tab_assign = tab_step + wg_step;
    KmBatchWg* tab_acc = tab_assign + wg_assign;
    double* xs_all = c->kb_x.as<double>();
    double* closest_all = c->kb_points.as<double>();
    double* mind2_all = closest_all + rows;
    int32_t* labels_all = reinterpret_cast<int32_t*>(mind2_all + rows);
    int32_t* labels_packed = labels_all + rows;                              // int32 [resident n_pad]
    double* blk_all = c->kb_blocks.as<double>();
    double* inertia_all = blk_all + blk;
    // kb_small: double  seeds [B][3k] | c3 [B][3k] | c4 [B][4k] | cand_xyz [B][96] | out [B][4k + 2] | rand [B][(k-1) T] | res [B]
    //           int64   ids [B][k] | cand [B][32]      KmCtl ctl [B]      uint64 changed [B]
    double* seeds_all = c->kb_small.as<double>();
    double* c3_all = seeds_all + 3 * (size_t)k * B;
    double* c4_all = c3_all + 3 * (size_t)k * B;
    double* xyz_all = c4_all + 4 * (size_t)k * B;
    double* out_all = xyz_all + (size_t)2 * 3 * KM_MAX_TRIALS * B;
    double* rand_all = out_all + (4 * (size_t)k + 2) * B;
    const size_t per_rand = (size_t)std::max(1, (k - 1) * T);
    double* res_all = rand_all + per_rand * B;
    int64_t* ids_all = reinterpret_cast<int64_t*>(res_all + B);
    int64_t* cand_all = ids_all + (size_t)k * B;
    KmCtl* ctl_all = reinterpret_cast<KmCtl*>(cand_all + (size_t)2 * KM_MAX_TRIALS * B);
    unsigned long long* changed_all = reinterpret_cast<unsigned long long*>(ctl_all + B);
    static_assert(sizeof(KmCtl) == 24, "the control words are downloaded as an array");

    std::vector<KmBatchMember> mem((size_t)B);
    const std::vector<KmBatchWg>& tab = lay.tab;
    for (int b = 0; b < B; ++b) {
        const KmBatchPlan& p = plan[b];
        KmBatchMember& m = mem[b];
        m.xs = xs_all + 3 * p.row0;
        m.n = p.n; m.n_pad = p.n_pad; m.src_first = p.src_first;
        m.first_id = seeded ? first_ids[b] : 0;
        m.tol_abs = tol_abs[b];
        m.closest = closest_all + p.row0;
        m.labels = labels_all + p.row0;
        m.mind2 = mind2_all + p.row0;
        m.bsum = blk_all + p.blk0;
        m.part = m.bsum + p.B;
        m.part16 = m.part + 2 * (size_t)p.B * KM_MAX_TRIALS;
        m.g0 = m.part16 + 2 * (size_t)p.G * KM_MAX_TRIALS;
        m.gprefix = m.g0 + p.G;
        m.seeds = seeds_all + 3 * (size_t)k * b;
        m.c3 = c3_all + 3 * (size_t)k * b;
        m.c4 = c4_all + 4 * (size_t)k * b;
        m.cand_xyz = xyz_all + (size_t)2 * 3 * KM_MAX_TRIALS * b;
        m.ids = ids_all + (size_t)k * b;
        m.cand = cand_all + (size_t)2 * KM_MAX_TRIALS * b;
        m.rand = rand_all + per_rand * b;
        m.partial = c->kb_partial.as<double>() + p.partial0;
        m.out = out_all + (4 * (size_t)k + 2) * b;
        m.inertia_part = inertia_all + p.inertia0;
        m.changed = changed_all + b;
        m.ctl = ctl_all + b;
        m.B = p.B; m.G = p.G; m.nb_assign = p.nb_assign; m.nb_acc = p.nb_acc;
    }
    HGMM_TRY(upload_table(c, mem_dev, mem.data(), sizeof(KmBatchMember) * mem.size()));
    HGMM_TRY(upload_table(c, tab_dev, tab.data(), sizeof(KmBatchWg) * tab.size()));
    if (seeded && k > 1)
        HGMM_HIP(c, hipMemcpyAsync(rand_all, rand_vals, sizeof(double) * per_rand * B, hipMemcpyHostToDevice, c->stream));
    if (!seeded)
        HGMM_HIP(c, hipMemcpyAsync(seeds_all, init_centres, sizeof(double) * 3 * (size_t)k * B, hipMemcpyHostToDevice, c->stream));
    hipStream_t st = c->stream;
    kmb_pack_kernel<<<(unsigned)wg_step, KM_STEP_BLOCK, 0, st>>>(mem_dev, tab_step, c->x_soa64.as<double>(), c->n_pad);
    // ---- seeding: km_plusplus's one-launch-per-centre chain, every launch over all members ----
    if (seeded) {
        kmb_first_kernel<<<(unsigned)wg_first, KM_BLOCK, 0, st>>>(mem_dev, tab_first);
        if (k > 1) {
            const bool t8 = T <= 8;
            auto tail = [&](int jj, int select, int draw, int64_t off) {
                if (t8) kmb_tail_kernel<8><<<B, 1024, 0, st>>>(mem_dev, T, jj, select, draw, off);
                else kmb_tail_kernel<KM_MAX_TRIALS><<<B, 1024, 0, st>>>(mem_dev, T, jj, select, draw, off);
            };
            kmb_group_kernel<<<dim3(km_nblk(maxG, 256), B), 256, 0, st>>>(mem_dev);
            tail(0, 0, 1, 0);
            if (t8) kmb_step_kernel<8><<<(unsigned)wg_step, KM_STEP_BLOCK, 0, st>>>(mem_dev, tab_step, -1, T, 1);
            else kmb_step_kernel<KM_MAX_TRIALS><<<(unsigned)wg_step, KM_STEP_BLOCK, 0, st>>>(mem_dev, tab_step, -1, T, 1);
            for (int j = 2; j < k; ++j) {
                const int64_t off = (int64_t)(j - 1) * T;
                if (t8) kmb_fused_kernel<8><<<(unsigned)wg_step, KM_STEP_BLOCK, 0, st>>>(mem_dev, tab_step, T, j, off);
                else kmb_fused_kernel<KM_MAX_TRIALS><<<(unsigned)wg_step, KM_STEP_BLOCK, 0, st>>>(mem_dev, tab_step, T, j, off);
            }
            tail(k - 1, 1, 0, 0);
        }
    }
    kmb_start_kernel<<<B, 256, 0, st>>>(mem_dev, k);
    HGMM_HIP(c, hipGetLastError());
    // ---- Lloyd: the five launches of km_enqueue + kmeans_update_kernel per iteration, eight iterations per synchronisation ----
    const size_t lds = sizeof(double) * ((size_t)4 * 4 * k_alloc + 4 * 256);
    if (acc_lds)
        HGMM_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&kmb_accum_lds_kernel),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    auto enqueue = [&]() {
        kmb_pad_centres_kernel<<<dim3(km_nblk(k, 256), B), 256, 0, st>>>(mem_dev, k);
        kmb_assign_kernel<<<(unsigned)wg_assign, KM_BLOCK, 0, st>>>(mem_dev, tab_assign, k);
        if (acc_lds)
            kmb_accum_lds_kernel<<<(unsigned)wg_acc, KM_BLOCK, lds, st>>>(mem_dev, tab_acc, k_alloc);
        else
            for (int slot0 = 0; slot0 * 64 < k; slot0 += nslot) {
                if (nslot == 4) kmb_accum_kernel<4><<<(unsigned)wg_acc, KM_BLOCK, 0, st>>>(mem_dev, tab_acc, slot0, k_alloc);
                else kmb_accum_kernel<KM_ACC_SLOTS><<<(unsigned)wg_acc, KM_BLOCK, 0, st>>>(mem_dev, tab_acc, slot0, k_alloc);
            }
        kmb_reduce_kernel<<<dim3(km_nblk(4 * (int64_t)k, 32), B), KM_BLOCK, 0, st>>>(mem_dev, k_alloc, k);
    };
    std::vector<KmCtl> h((size_t)B);
    if (max_iter >= 1) {
        const int batch = 8;
        bool all_done = false;
        while (!all_done) {
            for (int it = 0; it < batch; ++it) {
                enqueue();
                kmb_update_kernel<<<B, 256, 0, st>>>(mem_dev, k, max_iter);
            }
            HGMM_HIP(c, hipGetLastError());
            HGMM_HIP(c, hipMemcpyAsync(h.data(), ctl_all, sizeof(KmCtl) * B, hipMemcpyDeviceToHost, st));
            HGMM_HIP(c, ctx_stream_sync(c));
            all_done = true;
            for (int b = 0; b < B; ++b) all_done = all_done && h[b].done;
        }
    }
    // ---- the last assignment of the members that did not stop strictly, then one group of downloads ----
    kmb_final_gate_kernel<<<km_nblk(B, 256), 256, 0, st>>>(mem_dev, B);
    enqueue();
    kmb_inertia_kernel<<<km_nblk(B, 256), 256, 0, st>>>(mem_dev, B, k, res_all);
    if (labels_out) kmb_labels_kernel<<<(unsigned)wg_first, KM_BLOCK, 0, st>>>(mem_dev, tab_first, labels_packed);
    HGMM_HIP(c, hipGetLastError());
    {
        StagedDownloads dl(c);
        if (seeded) dl.add(ids_out, ids_all, sizeof(int64_t) * (size_t)k * B);
        dl.add(seeds_out, seeds_all, sizeof(double) * 3 * (size_t)k * B);        // (an explicit start: the start, if asked for)
        dl.add(centres_out, c3_all, sizeof(double) * 3 * (size_t)k * B);
        dl.add(inertia_out, res_all, sizeof(double) * B);
        dl.add(h.data(), ctl_all, sizeof(KmCtl) * B);
        if (labels_out) dl.add(labels_out, labels_packed, sizeof(int32_t) * (size_t)c->n);
        HGMM_HIP(c, dl.finish());
    }
    for (int b = 0; b < B; ++b) {
        // (after the gate `done` says "no last assignment"; iterations, strictness and the empty cluster are untouched)
        n_iter_out[b] = h[b].it;
        strict_out[b] = h[b].strict;
        status_out[b] = h[b].needs_host;
    }
    return HGMM_OK;
}
