// Batched flat full-covariance fit (hgmm_fullcov_fit_batch / _rows): B clouds fitted by the same launches.  Included once, at
// the end of fullcov_kernels.hip.
//
// Every launch of the serial one-pass loop (fullcov_fit: tree_mstep_kernel, full_fused_kernel, full_reduce_kernel,
// tree_sum_kernel) has a twin here that does the SAME work for many clouds: a workgroup looks up its member -- one (member,
// local block) entry per workgroup for the fused launch, whose grid depends on the clouds' sizes; blockIdx.y for the M-step
// and the reduction, whose grids depend on J alone; blockIdx.x for the sum of q -- and runs the serial code on the member's
// row of FcBatchMember: full_fused_body with the member's local block and serial grid for blockIdx.x / gridDim.x,
// mstep_node / prep_node / tree_ctl_update as the serial kernels call them, the serial kernels' summation orders.
// Everything a member's workgroups read or write is the member's own: its piece of the forest cloud (and of the weights), its
// slices of the parameter, prep and moment tables, its partials and shares of q, its control word, q trace, progress word
// and Cholesky flag.
//
// THE CLOUD.  The members lie packed in the resident forest cloud [3][n_pad]: member b starts at row first_b, which is no
// multiple of anything.  full_fused_body reads coordinates and weights one double at a time (the origin and the staging
// threads' loads: scalar or 8-byte vector loads) and writes labels one int at a time, so a member is simply the pointer
// xs + first_b with the forest's stride n_pad: no aligned copy is needed.  Rows past a member's end are never read (the
// staging clamps to n - 1), so the next member's rows behind it do not matter.
#include "fullcov_batch_plan.h"

namespace hgmm {

static_assert(FCB_TILE == FT_P && FCB_NMOM == NMOM, "fullcov_batch_plan.h");

#ifndef FCB_AHEAD
#define FCB_AHEAD 4            // iterations the host keeps enqueued beyond the slowest member still running (follow_ahead)
#endif
constexpr int FC_BATCH_MAX = 4096;                                // members per call
constexpr unsigned long long FC_BATCH_MAX_PARTIALS = 8ull << 30;  // bytes of all members' partials together

struct FcBatchMember {
    const double* xs;                 // the member's piece of the forest cloud: x_soa64 + first (stride: the forest's n_pad)
    const double* w;                  // ... of the forest's source weights, or NULL (weighted == 0)
    int64_t n;
    double n_total;                   // what pi = m0 / W divides by: the count, or the member's weight sum
    const double* init_mu;            // double [J][3]
    double *pi, *mu, *cov, *prep, *mom;   // double [J16], [J16][3], [J16][9], [J16][PREP_N], [J16][NMOM]
    double* partials;                 // double [grid][J16][NMOM]
    double* block_q;                  // double [grid]
    double* q;                        // the latest sum of the shares
    double* trace;                    // double [trace_cap]
    int32_t* labels;                  // buffer 0 of its rows' arg-max (buffer 1: + the forest's n_pad)
    int* flags;                       // bit 0: some Sigma^-1 of THIS member failed the Cholesky test
    TreeCtl* ctl;
    unsigned long long* host_word;    // its progress word in the pinned hand-over block
    int grid;                         // min(tiles, CUs): the serial launch's grid
};

// A pointer read from the member table is a generic pointer to the compiler and would be dereferenced by flat loads, a
// wave-uniform origin never by a scalar load; the table holds device allocations only, so the pointer is rebuilt from its bits
// as one into the global address space -- what the serial kernels' arguments are by themselves (kmeans_batch.h does the same)
template <class T>
__device__ __forceinline__ T* fc_global(T* p) {
    typedef __attribute__((address_space(1))) T* gptr;
    return (T*)(gptr)(uintptr_t)p;
}

// grid (J16 / 256, B): full_init_nodes_kernel per member
__global__ void fcb_init_kernel(const FcBatchMember* __restrict__ mem, double sig2, int J, int J16) {
    const FcBatchMember& m = mem[blockIdx.y];
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= J16) return;
    const double* init_mu = fc_global(m.init_mu);
    double *pi = fc_global(m.pi), *mu = fc_global(m.mu), *cov = fc_global(m.cov);
    pi[j] = (j < J) ? 1.0 / (double)J : 0.0;
    for (int d = 0; d < 3; ++d) mu[3 * j + d] = (j < J) ? init_mu[3 * j + d] : 0.0;
    for (int e = 0; e < 9; ++e) cov[9 * j + e] = (e % 4 == 0) ? ((j < J) ? sig2 : 1.0) : 0.0;
}
// ... and tree_prep_kernel (a launch of its own, as in the serial fit: it reads the tables back from memory)
__global__ void fcb_prep_kernel(const FcBatchMember* __restrict__ mem, int J16) {
    const FcBatchMember& m = mem[blockIdx.y];
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= J16) return;
    const double *pi = fc_global(m.pi), *mu = fc_global(m.mu);
    const double* c = fc_global(m.cov) + 9 * j;
    prep_node(pi[j], mu[3 * j], mu[3 * j + 1], mu[3 * j + 2], c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[8],
              fc_global(m.prep) + PREP_N * j, fc_global(m.flags));
}

// grid (J / 256, B): tree_mstep_kernel per member
__global__ void fcb_mstep_kernel(const FcBatchMember* __restrict__ mem, int J, double ld, int with_complexity) {
    const FcBatchMember& m = mem[blockIdx.y];
    if (fc_global(m.ctl)->done) return;
    const int cl = blockIdx.x * blockDim.x + threadIdx.x;
    if (cl >= J) return;
    mstep_node(fc_global(m.mom) + (size_t)cl * NMOM, cl, m.n_total, ld, fc_global(m.pi), fc_global(m.mu), fc_global(m.cov),
               fc_global(m.prep), fc_global(m.flags), with_complexity != 0);
}

// grid: the sum of the members' serial grids; `slot`: the arg-max buffer this launch writes
template <int CPL, bool WEIGHTED>
__global__ __launch_bounds__(FT_BLOCK) void fcb_fused_kernel(const FcBatchMember* __restrict__ mem,
                                                             const FcBatchWg* __restrict__ tab, int64_t n_pad, int J16,
                                                             int slot, int want_stats, const double* __restrict__ exp2_tab) {
    extern __shared__ double lds[];
    const FcBatchWg wg = tab[blockIdx.x];                       // (wave-uniform: scalar loads)
    const FcBatchMember& m = mem[wg.member];
    if (fc_global(m.ctl)->done) return;                         // the member's loop stopped in an earlier iteration
    const double* xs = fc_global(m.xs);
    const double* wsrc = WEIGHTED ? fc_global(m.w) : nullptr;
    const double* prep = fc_global(m.prep);
    int* labels = fc_global(m.labels) + (size_t)slot * n_pad;
    double* block_q = fc_global(m.block_q);
    double* partials = fc_global(m.partials);
    if (*fc_global(m.flags) & 1)                                // member-uniform: some Sigma^-1 of this member failed the test
        full_fused_body<CPL, false, WEIGHTED, true>(xs, m.n, n_pad, prep, J16, labels, block_q, partials, want_stats, nullptr,
                                                    lds, exp2_tab, wsrc, (unsigned)wg.local, (unsigned)m.grid);
    else
        full_fused_body<CPL, true, WEIGHTED, true>(xs, m.n, n_pad, prep, J16, labels, block_q, partials, want_stats, nullptr,
                                                   lds, exp2_tab, wsrc, (unsigned)wg.local, (unsigned)m.grid);
}

// grid (J, B), one wave per component: full_reduce_kernel per member
__global__ __launch_bounds__(64) void fcb_reduce_kernel(const FcBatchMember* __restrict__ mem, int J, int J16) {
    const FcBatchMember& m = mem[blockIdx.y];
    const int j = blockIdx.x;
    if (j >= J) return;
    if (fc_global(m.ctl)->done) return;
    const double* partials = fc_global(m.partials);
    const int nblocks = m.grid;
    double acc[NMOM];
#pragma unroll
    for (int k = 0; k < NMOM; ++k) acc[k] = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += 64) {
        const double* src = partials + ((size_t)b * J16 + j) * NMOM;
#pragma unroll
        for (int k = 0; k < NMOM; ++k) acc[k] += src[k];
    }
    double* mom = fc_global(m.mom);
#pragma unroll
    for (int k = 0; k < NMOM; ++k) {
        const double v = wave_sum_f64(acc[k]);
        if (threadIdx.x == 0) mom[(size_t)j * NMOM + k] = v;
    }
}

// grid B: tree_sum_kernel per member, each applying its member's stop rule
__global__ __launch_bounds__(256) void fcb_sum_kernel(const FcBatchMember* __restrict__ mem, double ls, int max_iters,
                                                      int trace_cap) {
    const FcBatchMember& m = mem[blockIdx.x];
    TreeCtl* ctl = fc_global(m.ctl);
    const int stop_flag = ctl->done;                            // (requested together with the shares)
    const double* v = fc_global(m.block_q);
    const int n = m.grid;
    __shared__ double sh[4];
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) acc += v[i];
    if (stop_flag) return;
    acc = wave_sum_f64(acc);
    if (lane_id() == 0) sh[wave_in_block()] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double q = sh[0] + sh[1] + sh[2] + sh[3];
        *fc_global(m.q) = q;
        tree_ctl_update(q, TreeStop{ctl, ls, max_iters, fc_global(m.trace), trace_cap, m.host_word});
    }
}

// the members' labels -> one array on the forest cloud's rows: member b's are those of the E-step whose statistics its last
// M-step took, buffer (it_b - 1) & 1 (fullcov_fit's lab_cur)
__global__ __launch_bounds__(256) void fcb_labels_kernel(const FcBatchMember* __restrict__ mem, const int64_t* __restrict__ first,
                                                         int B, int64_t n, int64_t n_pad, const int32_t* __restrict__ lab,
                                                         int32_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int b = find_cloud(first, B, i);
    const int it = fc_global(mem[b].ctl)->it;
    out[i] = lab[(size_t)((it - 1) & 1) * n_pad + i];
}

template <int CPL, bool WEIGHTED>
static int fcb_launch_fused(hgmm_ctx* c, unsigned grid, size_t lds, const FcBatchMember* mem, const FcBatchWg* tab, int J16,
                            int slot, int want_stats) {
    fcb_fused_kernel<CPL, WEIGHTED><<<grid, FT_BLOCK, lds, c->stream>>>(mem, tab, c->n_pad, J16, slot, want_stats,
                                                                         c->exp_tab2.as<double>());
    return HGMM_OK;
}

}  // namespace hgmm

using namespace hgmm;

// hgmm_fullcov_fit_batch (init_mu) and hgmm_fullcov_fit_batch_rows (init_rows [B][J]: row numbers within each member, gathered
// on the device into the place init_mu is uploaded to): exactly one of the two is given
static int fullcov_fit_batch(hgmm_ctx* c, const char* what, int B, const int64_t* counts, int J, double ls, double ld,
                             const double* init_mu, const int64_t* init_rows, bool by_rows, double sig2, int max_iters,
                             int weighted, double* pi_out, double* mu_out, double* cov_out, int32_t* labels_out,
                             double* q_trace_out, int q_capacity, int32_t* q_len_out) {
    HGMM_ENTER(c);
    // ---- refusals: nothing resident is touched ----
    if (B < 1 || B > FC_BATCH_MAX) return fail(c, HGMM_ERR_ARG, "%s: B = %d outside 1..%d", what, B, FC_BATCH_MAX);
    if (!counts || !pi_out || !mu_out || !cov_out || !q_len_out)
        return fail(c, HGMM_ERR_ARG, "%s: NULL argument (counts, pi_out, mu_out, cov_out and q_len_out are required)", what);
    if (by_rows ? !init_rows : !init_mu) return fail(c, HGMM_ERR_ARG, "%s: %s is NULL", what, by_rows ? "init_rows" : "init_mu");
    if (J < 1 || J > 4096) return fail(c, HGMM_ERR_ARG, "%s: J = %d outside 1..4096", what, J);
    const int J16 = (J + 15) / 16 * 16;
    if (J16 > FT_MAX_J16)
        return fail(c, HGMM_ERR_ARG, "%s: J = %d (J16 = %d > %d) takes the two-pass path of hgmm_fullcov_fit; the batch is the "
                    "one-pass float64 kernel only", what, J, J16, FT_MAX_J16);
    if (c->cfg[CFG_FULLCOV_TWO_PASS])
        return fail(c, HGMM_ERR_STATE, "%s: the fullcov_two_pass option is set; the batch is the one-pass float64 kernel only", what);
    if (c->tree.pdf_f32)
        return fail(c, HGMM_ERR_STATE, "%s: hgmm_tree_set_precision(HGMM_PRECISION_F32_PDF) is in force; the batch has no float32 "
                    "tile (set HGMM_PRECISION_F64, or fit the members with hgmm_fullcov_fit)", what);
    const ForestState& F = c->forest;
    if (!c->have_f64 || c->n <= 0 || F.src_counts.empty())
        return fail(c, HGMM_ERR_STATE, "%s: no batch cloud is resident (call hgmm_set_points_batch_f64 / _f32 or "
                    "hgmm_voxel_to_points_batch first)", what);
    if (c->comm_on())
        return fail(c, HGMM_ERR_STATE, "%s: the context has a communicator; independent clouds take none", what);
    if (B != (int)F.src_counts.size())
        return fail(c, HGMM_ERR_STATE, "%s: B = %d, but %d clouds are resident", what, B, (int)F.src_counts.size());
    for (int b = 0; b < B; ++b)
        if (counts[b] != F.src_counts[b] || counts[b] < 1)
            return fail(c, HGMM_ERR_ARG, "%s: member %d: counts[%d] = %lld, but the resident cloud has %lld points", what, b, b,
                        (long long)counts[b], (long long)F.src_counts[b]);
    if (c->n > 0x7fffffff - 1024)
        return fail(c, HGMM_ERR_ARG, "%s: the batch cloud's %lld points are too many for 32-bit indices", what, (long long)c->n);
    const double* wsrc = nullptr;
    if (weighted) {
        wsrc = F.src_w.ptr();
        if (!wsrc || F.src_w.buf.cap < sizeof(double) * (size_t)c->n_pad || F.src_w.sums.size() != (size_t)B)
            return fail(c, HGMM_ERR_STATE, "%s: weighted = 1, but no source weights of the batch cloud are resident (set them with "
                        "hgmm_tree_set_source_weights_batch or hgmm_voxel_to_points_batch(..., HGMM_VOXEL_W_TREE), or pass "
                        "weighted = 0)", what);
    }
    if (by_rows)
        for (int64_t e = 0; e < (int64_t)B * J; ++e)
            if (init_rows[e] < 0 || init_rows[e] >= counts[e / J])
                return fail(c, HGMM_ERR_ARG, "%s: init_rows[%lld][%lld] = %lld, but member %lld has %lld points", what,
                            (long long)(e / J), (long long)(e % J), (long long)init_rows[e], (long long)(e / J),
                            (long long)counts[e / J]);
    // ---- the plan: every member's serial grid and its pieces of the batch's buffers ----
    const FcBatchLayout lay = fc_batch_layout(B, counts, J, c->cus);
    if (sizeof(double) * (unsigned long long)lay.partial_doubles > FC_BATCH_MAX_PARTIALS)
        return fail(c, HGMM_ERR_ARG, "%s: the members' partial statistics take %.1f GiB together, above the limit of %.0f GiB",
                    what, (double)(sizeof(double) * lay.partial_doubles) / (1ull << 30), (double)FC_BATCH_MAX_PARTIALS / (1ull << 30));
    if (max_iters < 1) max_iters = 1;
    if (q_capacity < 0) q_capacity = 0;
    // (a member's trace is handed out up to min(iterations, q_capacity): nothing behind q_capacity is kept)
    const int trace_cap = std::max(1, std::min(std::min(max_iters, 1 << 20), q_trace_out ? q_capacity : 1));
    const int64_t n = c->n, n_pad = c->n_pad;
    const size_t TC = lay.components, wgs = (size_t)lay.wgs;
    // ---- buffers of the batch's own ----
    HGMM_TRY(ensure(c, c->fc_tab, sizeof(FcBatchMember) * (size_t)B + sizeof(int64_t) * (size_t)B + sizeof(FcBatchWg) * wgs));
    HGMM_TRY(ensure(c, c->fc_tables, sizeof(double) * TC * (1 + 3 + 9 + PREP_N + NMOM)));
    HGMM_TRY(ensure(c, c->fc_partials, sizeof(double) * lay.partial_doubles));
    HGMM_TRY(ensure(c, c->fc_small, sizeof(double) * (wgs + (size_t)B + (size_t)B * trace_cap) + (sizeof(TreeCtl) + sizeof(int)) * (size_t)B));
    HGMM_TRY(ensure(c, c->fc_labels, sizeof(int32_t) * 3 * (size_t)n_pad));
    HGMM_TRY(ensure_exp_tab2(c));
    HandOver* hand = nullptr;
    HGMM_TRY(hand_over(c, B, &hand));
    const HostDev<unsigned long long> words = hand->progress(0);
    FcBatchMember* mem_dev = c->fc_tab.as<FcBatchMember>();
    int64_t* first_dev = reinterpret_cast<int64_t*>(mem_dev + B);
    FcBatchWg* tab_dev = reinterpret_cast<FcBatchWg*>(first_dev + B);
    double* d_pi = c->fc_tables.as<double>();
    double* d_mu = d_pi + TC;
    double* d_cov = d_mu + 3 * TC;
    double* d_prep = d_cov + 9 * TC;
    double* d_mom = d_prep + (size_t)PREP_N * TC;
    double* bq_all = c->fc_small.as<double>();
    double* q_all = bq_all + wgs;
    double* trace_all = q_all + B;
    TreeCtl* ctl_all = reinterpret_cast<TreeCtl*>(trace_all + (size_t)B * trace_cap);
    int* flags_all = reinterpret_cast<int*>(ctl_all + B);
    int32_t* lab_all = c->fc_labels.as<int32_t>();
    int32_t* lab_packed = lab_all + 2 * (size_t)n_pad;
    // the initial means: [B][J][3] in scratch
    if (by_rows) {
        std::vector<int64_t> first_row((size_t)B);
        for (int b = 0; b < B; ++b) first_row[b] = lay.plan[b].first;
        HGMM_TRY(stage_init_rows(c, init_rows, (int64_t)B * J, first_row.data(), J));
    } else {
        HGMM_TRY(ensure(c, c->scratch, sizeof(double) * 3 * (size_t)B * J));
        HGMM_HIP(c, hipMemcpyAsync(c->scratch.p, init_mu, sizeof(double) * 3 * (size_t)B * J, hipMemcpyHostToDevice, c->stream));
    }
    std::vector<FcBatchMember> mem((size_t)B);
    std::vector<int64_t> first((size_t)B);
    for (int b = 0; b < B; ++b) {
        const FcBatchPlan& p = lay.plan[b];
        FcBatchMember& m = mem[b];
        first[b] = p.first;
        m.xs = c->x_soa64.as<double>() + p.first;
        m.w = wsrc ? wsrc + p.first : nullptr;
        m.n = p.n;
        m.n_total = wsrc ? F.src_w.total(p.n, b) : (double)p.n;   // pi = m0 / N; with weights their sum (a NULL member: its count)
        m.init_mu = c->scratch.as<double>() + 3 * (size_t)J * b;
        m.pi = d_pi + p.table0;
        m.mu = d_mu + 3 * p.table0;
        m.cov = d_cov + 9 * p.table0;
        m.prep = d_prep + (size_t)PREP_N * p.table0;
        m.mom = d_mom + (size_t)NMOM * p.table0;
        m.partials = c->fc_partials.as<double>() + (size_t)p.wg0 * lay.J16 * NMOM;
        m.block_q = bq_all + p.wg0;
        m.q = q_all + b;
        m.trace = trace_all + (size_t)b * trace_cap;
        m.labels = lab_all + p.first;
        m.flags = flags_all + b;
        m.ctl = ctl_all + b;
        m.host_word = words.dev + b;
        m.grid = p.grid;
    }
    HGMM_TRY(upload_table(c, mem_dev, mem.data(), sizeof(FcBatchMember) * mem.size()));
    HGMM_TRY(upload_table(c, first_dev, first.data(), sizeof(int64_t) * first.size()));
    HGMM_TRY(upload_table(c, tab_dev, lay.tab.data(), sizeof(FcBatchWg) * lay.tab.size()));
    HGMM_HIP(c, hipMemsetAsync(ctl_all, 0, (sizeof(TreeCtl) + sizeof(int)) * (size_t)B, c->stream));   // control words and flags
    // (tree_no_chol: every member starts on the symmetric form, as tree_flags presets the serial fit's word)
    const std::vector<int> preset((size_t)B, 1);
    if (c->cfg[CFG_TREE_NO_CHOL]) HGMM_TRY(upload_table(c, flags_all, preset.data(), sizeof(int) * (size_t)B));
    for (int b = 0; b < B; ++b) __atomic_store_n(words.host + b, 0ull, __ATOMIC_RELAXED);
    hipStream_t st = c->stream;
    const size_t lds = ft_lds_bytes(J16, wsrc != nullptr);
    const bool cpl1 = J16 <= FT_BLOCK;
    int (*launch_fused)(hgmm_ctx*, unsigned, size_t, const FcBatchMember*, const FcBatchWg*, int, int, int) =
        wsrc ? (cpl1 ? &fcb_launch_fused<1, true> : &fcb_launch_fused<2, true>)
             : (cpl1 ? &fcb_launch_fused<1, false> : &fcb_launch_fused<2, false>);
    const void* fused_fn = wsrc ? (cpl1 ? reinterpret_cast<const void*>(&fcb_fused_kernel<1, true>)
                                        : reinterpret_cast<const void*>(&fcb_fused_kernel<2, true>))
                                : (cpl1 ? reinterpret_cast<const void*>(&fcb_fused_kernel<1, false>)
                                        : reinterpret_cast<const void*>(&fcb_fused_kernel<2, false>));
    HGMM_HIP(c, hipFuncSetAttribute(fused_fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    // ---- the initial parameters and their E-step (arg-max into buffer 0) ----
    fcb_init_kernel<<<dim3(nblk(J16, 256), B), 256, 0, st>>>(mem_dev, sig2, J, J16);
    fcb_prep_kernel<<<dim3(nblk(J16, 256), B), 256, 0, st>>>(mem_dev, J16);
    launch_fused(c, (unsigned)wgs, lds, mem_dev, tab_dev, J16, 0, 1);
    fcb_reduce_kernel<<<dim3(J, B), 64, 0, st>>>(mem_dev, J, J16);
    HGMM_HIP(c, hipGetLastError());
    // ---- the loop: four launches per iteration of all members, the host FCB_AHEAD iterations ahead of the slowest ----
    const auto enqueue = [&](int k) -> int {                    // iteration k: arg-max into buffer (k + 1) & 1
        const int want_stats = k + 1 < max_iters ? 1 : 0;       // (the budget's last iteration forms no statistics)
        fcb_mstep_kernel<<<dim3(nblk(J, 256), B), 256, 0, st>>>(mem_dev, J, ld, 1);
        launch_fused(c, (unsigned)wgs, lds, mem_dev, tab_dev, J16, (k + 1) & 1, want_stats);
        if (want_stats) fcb_reduce_kernel<<<dim3(J, B), 64, 0, st>>>(mem_dev, J, J16);
        fcb_sum_kernel<<<B, 256, 0, st>>>(mem_dev, ls, max_iters, trace_cap);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return fail(c, HGMM_ERR_HIP, "%s: launch failed: %s", what, hipGetErrorString(e));
        return HGMM_OK;
    };
    const int rc = follow_ahead(c, words.host, B, max_iters, FCB_AHEAD, enqueue, nothing_at_budget, nullptr, what);
    if (rc != HGMM_OK) {
        (void)ctx_stream_sync(c);
        return rc;
    }
    // ---- results ----
    if (labels_out) fcb_labels_kernel<<<nblk(n, 256), 256, 0, st>>>(mem_dev, first_dev, B, n, n_pad, lab_all, lab_packed);
    HGMM_HIP(c, hipGetLastError());
    const bool dense = J == J16;                                // the tables' slices are the outputs' rows
    std::vector<double> h_tab;
    if (!dense) h_tab.resize(13 * TC);
    std::vector<double> h_trace;
    if (q_trace_out) h_trace.resize((size_t)B * trace_cap);
    std::vector<TreeCtl> h_ctl((size_t)B);
    {
        StagedDownloads dl(c);
        dl.add(dense ? pi_out : h_tab.data(), d_pi, sizeof(double) * TC);
        dl.add(dense ? mu_out : h_tab.data() + TC, d_mu, sizeof(double) * 3 * TC);
        dl.add(dense ? cov_out : h_tab.data() + 4 * TC, d_cov, sizeof(double) * 9 * TC);
        dl.add(h_ctl.data(), ctl_all, sizeof(TreeCtl) * (size_t)B);
        if (q_trace_out) dl.add(h_trace.data(), trace_all, sizeof(double) * h_trace.size());
        if (labels_out) dl.add(labels_out, lab_packed, sizeof(int32_t) * (size_t)n);
        HGMM_HIP(c, dl.finish());
    }
    for (int b = 0; b < B; ++b) {
        if (!dense) {
            std::memcpy(pi_out + (size_t)J * b, h_tab.data() + (size_t)J16 * b, sizeof(double) * J);
            std::memcpy(mu_out + 3 * (size_t)J * b, h_tab.data() + TC + 3 * (size_t)J16 * b, sizeof(double) * 3 * J);
            std::memcpy(cov_out + 9 * (size_t)J * b, h_tab.data() + 4 * TC + 9 * (size_t)J16 * b, sizeof(double) * 9 * J);
        }
        const int q_len = h_ctl[b].it;
        if (q_trace_out && q_len > 0)
            std::memcpy(q_trace_out + (size_t)b * q_capacity, h_trace.data() + (size_t)b * trace_cap,
                        sizeof(double) * std::min(std::min(q_len, q_capacity), trace_cap));
        q_len_out[b] = q_len < q_capacity ? q_len : q_capacity;
    }
    return HGMM_OK;
}

extern "C" int hgmm_fullcov_fit_batch(hgmm_ctx* c, int B, const int64_t* counts, int J, double ls, double ld,
                                      const double* init_mu, double sig2, int max_iters, int weighted, double* pi_out,
                                      double* mu_out, double* cov_out, int32_t* labels_out, double* q_trace_out,
                                      int q_capacity, int32_t* q_len_out) {
    return fullcov_fit_batch(c, "hgmm_fullcov_fit_batch", B, counts, J, ls, ld, init_mu, nullptr, false, sig2, max_iters, weighted,
                             pi_out, mu_out, cov_out, labels_out, q_trace_out, q_capacity, q_len_out);
}
extern "C" int hgmm_fullcov_fit_batch_rows(hgmm_ctx* c, int B, const int64_t* counts, int J, double ls, double ld,
                                           const int64_t* init_rows, double sig2, int max_iters, int weighted, double* pi_out,
                                           double* mu_out, double* cov_out, int32_t* labels_out, double* q_trace_out,
                                           int q_capacity, int32_t* q_len_out) {
    return fullcov_fit_batch(c, "hgmm_fullcov_fit_batch_rows", B, counts, J, ls, ld, nullptr, init_rows, true, sig2, max_iters,
                             weighted, pi_out, mu_out, cov_out, labels_out, q_trace_out, q_capacity, q_len_out);
}
