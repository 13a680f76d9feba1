// The voxel result handed to its consumers on the device (include/hgmm.h: hgmm_voxel_result_info, hgmm_voxel_to_*,
// hgmm_points_rows_f64; the row gather of hgmm_tree_build_rows / _batch_rows).  The down-sample leaves centroids and counts
// in vx_cent / vx_cnt; every consumer of them -- the resident cloud with its tree and flat weights, the serial target with
// its weights, the forest cloud, the forest's targets -- used to be fed from host arrays that were those buffers'
// download.  Here ONE launch per call, whatever B is, copies member rows to where the existing setters put them:
//   handover_kernel   one thread per destination row up to the pad: the three float64 planes, the float32 row, the count as
//                     a double and / or a float, the zero padding the existing uploads leave behind; the target variants
//                     reduce |x|^2 over the wave and issue one integer atomicMax per wave on the bits of the non-negative
//                     double (forest_target_kernel's definition, the same products and sums as hgmm_tree_set_target's loop)
//   gather_rows_kernel  one thread per requested row, structure of arrays -> [k][3]
// Each entry is DEFINED by a sequence of existing entries (the header names them) and leaves the context in that sequence's
// state, bit for bit.  The weight sums need no device sum: counts are integers >= 1 that add up to the member's raw point
// count, which the host has kept since the down-sample, and integer sums below 2^53 are exact in any order.
// No floating-point atomics; contraction off, so r2 has the host's bits.
#include "hgmm_ctx.h"
#include "tree_device.h"
#include "tree_host.h"

#include <algorithm>

#pragma clang fp contract(off)

namespace hgmm {

constexpr int HO_BLOCK = 256;

struct HandoverArgs {
    const double* cent;           // vx_cent [M][3]
    const int64_t* cnt;           // vx_cnt [M]
    const int64_t* dst_first;     // (B > 1) destination first rows [B + 1]; dst_first[B] = total
    const int64_t* src_first;     // (B > 1) first voxel of the member that fills slot b [B]
    int64_t src_first0;           // (B == 1) the member's first voxel
    int B;
    int64_t total, pad;           // destination rows in use / rows of a plane
    double* soa;                  // double [3][pad]
    float* aos;                   // float [total][3], or NULL
    double* wd;                   // double [pad]: the counts (zero beyond total), or NULL
    float* wf;                    // float [total]: the counts, or NULL
    unsigned long long* r2bits;   // (TARGET) [B] largest |x|^2 per slot, bits of a non-negative double; zeroed before the launch
    unsigned long long* wf_sum;   // sum of the integers (float)count over all rows, or NULL; zeroed before the launch
};

template <bool TARGET>
__global__ __launch_bounds__(HO_BLOCK) void handover_kernel(HandoverArgs a) {
    const int64_t i = (int64_t)blockIdx.x * HO_BLOCK + threadIdx.x;       // (the grid covers the pad exactly: no early return,
    const bool row = i < a.total;                                         //  every lane reaches the shuffles)
    int b = 0;
    double x = 0.0, y = 0.0, z = 0.0;
    int64_t count = 0;
    if (row) {
        int64_t src = a.src_first0 + i;
        if (a.B > 1) {
            b = find_cloud(a.dst_first, a.B, i);
            src = a.src_first[b] + (i - a.dst_first[b]);
        }
        x = a.cent[3 * src];
        y = a.cent[3 * src + 1];
        z = a.cent[3 * src + 2];
        count = a.cnt[src];
    }
    // rows between the last point and the pad are written as zeros: what hgmm_set_points_*, hgmm_tree_set_target and
    // upload_weights leave there.  (hgmm_tree_set_targets_batch leaves the pad of fr_tg unwritten -- no kernel reads it --;
    // the hand-over zeroes it like the others, on purpose: one rule for every destination.)
    a.soa[i] = x;
    a.soa[a.pad + i] = y;
    a.soa[2 * a.pad + i] = z;
    if (a.wd) a.wd[i] = (double)count;
    if (row) {
        if (a.aos) {
            a.aos[3 * i] = (float)x;
            a.aos[3 * i + 1] = (float)y;
            a.aos[3 * i + 2] = (float)z;
        }
        if (a.wf) a.wf[i] = (float)count;
    }
    if (a.wf_sum) {                                    // (float)count is an integer: summed as one, exact in any order
        unsigned long long s = row ? (unsigned long long)(float)count : 0ull;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
        if (lane_id() == 0 && s != 0ull) atomicAdd(a.wf_sum, s);
    }
    if (TARGET) {
        double r2 = 0.0;
        if (row) {
            r2 = __dadd_rn(__dadd_rn(__dmul_rn(x, x), __dmul_rn(y, y)), __dmul_rn(z, z));
            if (!(r2 >= 0.0)) r2 = 0.0;
        }
        // non-negative doubles order like their bit patterns
        unsigned long long bits = (unsigned long long)__double_as_longlong(r2);
        const int b0 = __shfl(b, 0);                   // (rows ascend with the lane: lane 0 holds a row if any lane does)
        if (__any(row && b != b0)) {
            // the wave's rows belong to more than one slot (at most B - 1 waves): every row for itself
            if (row && bits != 0ull) atomicMax(a.r2bits + b, bits);
        } else {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const unsigned long long o = __shfl_xor(bits, off);
                bits = o > bits ? o : bits;
            }
            if (lane_id() == 0 && bits != 0ull) atomicMax(a.r2bits + b0, bits);
        }
    }
}

// The hand-over to the batched flat fit (hgmm_flat_train_batch_voxels): what handover_kernel writes for the flat fit and
// nothing else -- the float32 row (float)centroid and the weight (float)count, by the same conversions -- slot after slot into
// buffers of the batch's own.  One thread per destination row; no float64 planes, no pad, no sums.
__global__ __launch_bounds__(HO_BLOCK) void handover_flat_kernel(const double* __restrict__ cent, const int64_t* __restrict__ cnt,
                                                                  const int64_t* __restrict__ dst_first,
                                                                  const int64_t* __restrict__ src_first, int B, int64_t total,
                                                                  float* __restrict__ aos, float* __restrict__ wf) {
    const int64_t i = (int64_t)blockIdx.x * HO_BLOCK + threadIdx.x;
    if (i >= total) return;
    const int b = find_cloud(dst_first, B, i);
    const int64_t src = src_first[b] + (i - dst_first[b]);
    aos[3 * i] = (float)cent[3 * src];
    aos[3 * i + 1] = (float)cent[3 * src + 1];
    aos[3 * i + 2] = (float)cent[3 * src + 2];
    if (wf) wf[i] = (float)cnt[src];
}

__global__ __launch_bounds__(HO_BLOCK) void gather_rows_kernel(const double* __restrict__ soa, int64_t n_pad,
                                                                const int64_t* __restrict__ rows, int64_t k,
                                                                double* __restrict__ out) {
    const int64_t j = (int64_t)blockIdx.x * HO_BLOCK + threadIdx.x;
    if (j >= k) return;
    const int64_t r = rows[j];
    for (int d = 0; d < 3; ++d) out[3 * j + d] = soa[(size_t)d * n_pad + r];
}

int gather_rows(hgmm_ctx* c, const int64_t* dev_rows, int64_t k, double* dev_out) {
    if (k <= 0) return HGMM_OK;
    gather_rows_kernel<<<(unsigned)((k + HO_BLOCK - 1) / HO_BLOCK), HO_BLOCK, 0, c->stream>>>(c->x_soa64.as<double>(), c->n_pad,
                                                                                             dev_rows, k, dev_out);
    HGMM_HIP(c, hipGetLastError());
    return HGMM_OK;
}

// scratch: [k][3] doubles (what the builds' tree_init_nodes_kernel reads), then the k row numbers.  The table travels
// through the pinned ring, not through scratch, and scratch has its final size before the first copy is enqueued (ensure
// frees and synchronises only when it grows): nothing between the gather and the builds' kernel touches the [k][3] block.
int stage_init_rows(hgmm_ctx* c, const int64_t* rows, int64_t k, const int64_t* first, int64_t per) {
    HGMM_TRY(ensure(c, c->scratch, (sizeof(double) * 3 + sizeof(int64_t)) * (size_t)k));
    int64_t* d_rows = reinterpret_cast<int64_t*>(c->scratch.as<double>() + 3 * (size_t)k);
    if (first) {
        std::vector<int64_t> abs_rows((size_t)k);
        for (int64_t j = 0; j < k; ++j) abs_rows[j] = rows[j] + first[j / per];
        HGMM_TRY(upload_table(c, d_rows, abs_rows.data(), sizeof(int64_t) * (size_t)k));
        if (sizeof(int64_t) * (size_t)k > (256u << 10)) HGMM_HIP(c, ctx_stream_sync(c));     // (abs_rows leaves scope)
    } else {
        HGMM_TRY(upload_table(c, d_rows, rows, sizeof(int64_t) * (size_t)k));
    }
    return gather_rows(c, d_rows, k, c->scratch.as<double>());
}

// ---- what every hand-over checks before anything resident is touched -------------------------------------------------------
static int check_result(hgmm_ctx* c, const char* what) {
    if (!c->vx_have) return fail(c, HGMM_ERR_STATE, "%s: no voxel result (no down-sample has succeeded on this context)", what);
    return HGMM_OK;
}
static int check_member(hgmm_ctx* c, const char* what, int member) {
    const int B = (int)c->vx_mb.size();
    if (member < 0 || member >= B) return fail(c, HGMM_ERR_ARG, "%s: member %d, but the voxel result has %d member%s", what, member, B, B == 1 ? "" : "s");
    return HGMM_OK;
}
static int check_members(hgmm_ctx* c, const char* what, int B, const int32_t* members, int max_B) {
    if (B < 1 || (max_B > 0 && B > max_B)) return fail(c, HGMM_ERR_ARG, "%s: B = %d", what, B);
    if (!members) return fail(c, HGMM_ERR_ARG, "%s: members is NULL", what);
    const int have = (int)c->vx_mb.size();
    for (int b = 0; b < B; ++b)
        if (members[b] < 0 || members[b] >= have)
            return fail(c, HGMM_ERR_ARG, "%s: members[%d] = %d, but the voxel result has %d member%s", what, b, members[b], have,
                        have == 1 ? "" : "s");
    return HGMM_OK;
}

// the weight sums of B slots filled from `members`: counts are integers that add up to the member's raw point count
static std::vector<double> raw_counts(const hgmm_ctx* c, int B, const int32_t* members) {
    std::vector<double> sums((size_t)B);
    for (int b = 0; b < B; ++b) sums[b] = (double)c->vx_nb[members[b]];
    return sums;
}

// the launch: B slots filled from `members` (B == 1: no table), the words of `zeroed` cleared in front of it
template <bool TARGET>
static int launch_handover(hgmm_ctx* c, HandoverArgs a, int B, const int32_t* members, unsigned long long* zeroed, int n_zeroed) {
    a.cent = c->vx_cent.as<double>();
    a.cnt = c->vx_cnt.as<int64_t>();
    a.B = B;
    if (B > 1) {
        std::vector<int64_t> tab((size_t)2 * B + 1);
        int64_t at = 0;
        for (int b = 0; b < B; ++b) {
            tab[b] = at;
            tab[(size_t)B + 1 + b] = c->vx_first[members[b]];
            at += c->vx_mb[members[b]];
        }
        tab[B] = at;
        HGMM_TRY(ensure(c, c->vx_hand, sizeof(int64_t) * tab.size() + 64));
        HGMM_TRY(upload_table(c, c->vx_hand.p, tab.data(), sizeof(int64_t) * tab.size()));
        if (sizeof(int64_t) * tab.size() > (256u << 10)) HGMM_HIP(c, ctx_stream_sync(c));    // (tab leaves scope)
        a.dst_first = c->vx_hand.as<int64_t>();
        a.src_first = a.dst_first + B + 1;
        a.src_first0 = 0;
    } else {
        a.dst_first = a.src_first = nullptr;
        a.src_first0 = c->vx_first[members[0]];
    }
    if (n_zeroed > 0) HGMM_HIP(c, hipMemsetAsync(zeroed, 0, sizeof(unsigned long long) * (size_t)n_zeroed, c->stream));
    handover_kernel<TARGET><<<(unsigned)(a.pad / HO_BLOCK), HO_BLOCK, 0, c->stream>>>(a);
    HGMM_HIP(c, hipGetLastError());
    return HGMM_OK;
}

}  // namespace hgmm

using namespace hgmm;

extern "C" int hgmm_voxel_result_info(hgmm_ctx* c, int* B_out, int64_t* m_out, int64_t* n_out, uint64_t* serial_out) {
    HGMM_ENTER(c);
    HGMM_TRY(check_result(c, "hgmm_voxel_result_info"));
    if (B_out) *B_out = (int)c->vx_mb.size();
    if (m_out) std::copy(c->vx_mb.begin(), c->vx_mb.end(), m_out);
    if (n_out) std::copy(c->vx_nb.begin(), c->vx_nb.end(), n_out);
    if (serial_out) *serial_out = (uint64_t)c->vx_serial;
    return HGMM_OK;
}

extern "C" int hgmm_voxel_to_points(hgmm_ctx* c, int member, int weights) {
    HGMM_ENTER(c);
    const char* what = "hgmm_voxel_to_points";
    HGMM_TRY(check_result(c, what));
    HGMM_TRY(check_member(c, what, member));
    if (weights & ~(HGMM_VOXEL_W_TREE | HGMM_VOXEL_W_FLAT))
        return fail(c, HGMM_ERR_ARG, "%s: weights = %d has bits other than HGMM_VOXEL_W_TREE | HGMM_VOXEL_W_FLAT", what, weights);
    const bool w_tree = (weights & HGMM_VOXEL_W_TREE) != 0, w_flat = (weights & HGMM_VOXEL_W_FLAT) != 0;
    const int64_t m = c->vx_mb[member], n_raw = c->vx_nb[member];
    // ---- the arguments are good: from here on a failure is the runtime's and leaves nothing bound ----
    bind_points(c, nullptr);
    hgmm_points* p = &c->own_points;
    HGMM_TRY(points_alloc(c, p, m));
    if (w_tree) HGMM_TRY(ensure(c, c->src.buf, sizeof(double) * (size_t)p->n_pad));
    if (w_flat) HGMM_TRY(ensure(c, c->flat_w.buf, sizeof(float) * (size_t)m));
    // (float)count == count while count < 2^24, and no count exceeds the member's raw points: only a member of 2^24 raw
    // points or more can hold a count that rounds, and only then is the sum of the float32 weights taken on the device
    const bool sum_on_device = w_flat && n_raw >= ((int64_t)1 << 24);
    if (sum_on_device) HGMM_TRY(ensure(c, c->vx_hand, 64));
    HandoverArgs a{};
    a.total = m;
    a.pad = p->n_pad;
    a.soa = p->x_soa64.as<double>();
    a.aos = p->x_aos.as<float>();
    a.wd = w_tree ? c->src.buf.as<double>() : nullptr;
    a.wf = w_flat ? c->flat_w.buf.as<float>() : nullptr;
    // (B == 1 launches use no table: the first word of vx_hand is free for the sum)
    a.wf_sum = sum_on_device ? c->vx_hand.as<unsigned long long>() : nullptr;
    const int32_t mem = member;
    HGMM_TRY(launch_handover<false>(c, a, 1, &mem, a.wf_sum, sum_on_device ? 1 : 0));
    double flat_sum = (double)n_raw;
    if (sum_on_device) {
        unsigned long long s = 0;
        StagedDownloads dl(c);
        dl.add(&s, a.wf_sum, sizeof s);
        HGMM_HIP(c, dl.finish());
        flat_sum = (double)s;
    }
    bind_points(c, p);
    if (w_tree) c->src.publish({(double)n_raw});
    if (w_flat) c->flat_w.publish({flat_sum});
    return HGMM_OK;
}

extern "C" int hgmm_voxel_to_target(hgmm_ctx* c, int member, int weighted) {
    HGMM_ENTER(c);
    const char* what = "hgmm_voxel_to_target";
    HGMM_TRY(check_result(c, what));
    HGMM_TRY(check_member(c, what, member));
    const int64_t m = c->vx_mb[member];
    const int64_t pad = (m + 255) / 256 * 256;
    // ---- the arguments are good: from here on a failure is the runtime's and leaves no target ----
    target_begin(c);
    HGMM_TRY(ensure(c, c->tgt_soa64, sizeof(double) * 3 * (size_t)pad));
    if (weighted) HGMM_TRY(ensure(c, c->tgt_w.buf, sizeof(double) * (size_t)pad));
    HGMM_TRY(ensure(c, c->vx_hand, 64));
    HandoverArgs a{};
    a.total = m;
    a.pad = pad;
    a.soa = c->tgt_soa64.as<double>();
    a.wd = weighted ? c->tgt_w.buf.as<double>() : nullptr;
    a.r2bits = c->vx_hand.as<unsigned long long>();          // (B == 1 launches use no table)
    const int32_t mem = member;
    HGMM_TRY(launch_handover<true>(c, a, 1, &mem, a.r2bits, 1));
    unsigned long long bits = 0;
    {
        StagedDownloads dl(c);
        dl.add(&bits, a.r2bits, sizeof bits);
        HGMM_HIP(c, dl.finish());
    }
    const double wsum = (double)c->vx_nb[member];
    target_publish(c, m, pad, r2_of_bits(bits), weighted ? &wsum : nullptr);
    return HGMM_OK;
}

extern "C" int hgmm_voxel_to_points_batch(hgmm_ctx* c, int B, const int32_t* members, int weighted) {
    HGMM_ENTER(c);
    const char* what = "hgmm_voxel_to_points_batch";
    HGMM_TRY(check_result(c, what));
    HGMM_TRY(check_members(c, what, B, members, 0));
    int64_t total = 0;
    for (int b = 0; b < B; ++b) total += c->vx_mb[members[b]];
    // ---- the arguments are good: from here on a failure is the runtime's and leaves nothing bound ----
    bind_points(c, nullptr);
    hgmm_points* p = &c->own_points;
    HGMM_TRY(points_alloc(c, p, total));
    ForestState& F = c->forest;
    if (weighted) HGMM_TRY(ensure(c, F.src_w.buf, sizeof(double) * (size_t)p->n_pad));
    HandoverArgs a{};
    a.total = total;
    a.pad = p->n_pad;
    a.soa = p->x_soa64.as<double>();
    a.wd = weighted ? F.src_w.buf.as<double>() : nullptr;
    HGMM_TRY(launch_handover<false>(c, a, B, members, nullptr, 0));
    bind_points(c, p);
    c->have_f32 = false;                                    // (a forest cloud has no float32 rows: hgmm_set_points_batch_*)
    F.src_counts.resize((size_t)B);
    for (int b = 0; b < B; ++b) F.src_counts[b] = c->vx_mb[members[b]];
    if (weighted) F.src_w.publish(raw_counts(c, B, members));
    return HGMM_OK;
}

extern "C" int hgmm_voxel_to_targets_batch(hgmm_ctx* c, int B, const int32_t* members, int weighted) {
    HGMM_ENTER(c);
    const char* what = "hgmm_voxel_to_targets_batch";
    HGMM_TRY(check_result(c, what));
    HGMM_TRY(check_members(c, what, B, members, 4096));
    std::vector<int64_t> counts((size_t)B);
    int64_t total = 0;
    for (int b = 0; b < B; ++b) { counts[b] = c->vx_mb[members[b]]; total += counts[b]; }
    if (total > 0x7fffffff - 1024) return fail(c, HGMM_ERR_ARG, "%s: too many target points for 32-bit indices", what);
    // ---- the arguments are good: from here on a failure is the runtime's and leaves no targets ----
    forest_targets_begin(c);
    const int64_t pad = (total + 255) / 256 * 256;
    HGMM_TRY(ensure(c, c->fr_tg, sizeof(double) * 3 * (size_t)pad));
    if (weighted) HGMM_TRY(ensure(c, c->forest.tg_w.buf, sizeof(double) * (size_t)pad));
    RegTable tb;
    HGMM_TRY(reg_table(c, c->fr_reg, B, &tb));
    HandoverArgs a{};
    a.total = total;
    a.pad = pad;
    a.soa = c->fr_tg.as<double>();
    a.wd = weighted ? c->forest.tg_w.buf.as<double>() : nullptr;
    a.r2bits = tb.r2max;
    HGMM_TRY(launch_handover<true>(c, a, B, members, tb.r2max, B));
    std::vector<unsigned long long> bits((size_t)B);
    {
        StagedDownloads dl(c);
        dl.add(bits.data(), tb.r2max, sizeof(unsigned long long) * (size_t)B);
        HGMM_HIP(c, dl.finish());
    }
    const std::vector<double> wsums = raw_counts(c, B, members);
    forest_targets_publish(c, B, counts.data(), bits.data(), pad, weighted ? wsums.data() : nullptr);
    return HGMM_OK;
}

extern "C" int hgmm_flat_train_batch_voxels(hgmm_ctx* c, int B, const int32_t* members, int weighted, int cov_type, int variant,
                                            int J, int max_iter, float tol, float* mu, float* cov, float* w,
                                            float* inv_std_out, float* lls_out, int32_t* n_iter_out, int32_t* converged_out) {
    HGMM_ENTER(c);
    const char* what = "hgmm_flat_train_batch_voxels";
    // ---- refusals: all of them before anything is touched ----
    HGMM_TRY(check_result(c, what));
    HGMM_TRY(check_members(c, what, B, members, FLAT_BATCH_MAX));
    HGMM_TRY(flat_batch_check(c, what, B, cov_type, variant, J, max_iter, mu, cov, w, n_iter_out, converged_out));
    int64_t total = 0;
    for (int b = 0; b < B; ++b) {
        const int64_t m = c->vx_mb[members[b]];
        if (m < 1) return fail(c, HGMM_ERR_ARG, "%s: members[%d] = %d holds no points", what, b, members[b]);
        // S_b is the member's raw point count (hgmm_voxel_to_points' rule), which is the sum of the float32 weights only
        // while no count rounds
        if (weighted && c->vx_nb[members[b]] >= ((int64_t)1 << 24))
            return fail(c, HGMM_ERR_ARG, "%s: members[%d] = %d stands for %lld raw points, 2^24 or more: a count may round as "
                        "a float32 weight; hand it over with hgmm_voxel_to_points(member, HGMM_VOXEL_W_FLAT), which sums such "
                        "counts on the device, and fit it with hgmm_flat_train", what, b, members[b],
                        (long long)c->vx_nb[members[b]]);
        total += m;
    }
    // ---- ONE hand-over launch, whatever B is: rows and weights of every slot into fb_x / fb_sw ----
    HGMM_TRY(ensure(c, c->fb_x, sizeof(float) * 3 * (size_t)total + 64));
    if (weighted) HGMM_TRY(ensure(c, c->fb_sw, sizeof(float) * (size_t)total + 64));
    std::vector<int64_t> tab((size_t)2 * B + 1);
    std::vector<FlatBatchSlot> slots((size_t)B);
    int64_t at = 0;
    for (int b = 0; b < B; ++b) {
        const int64_t m = c->vx_mb[members[b]];
        tab[b] = at;
        tab[(size_t)B + 1 + b] = c->vx_first[members[b]];
        slots[b].X = c->fb_x.as<float>() + 3 * at;
        slots[b].n = m;
        slots[b].SW = weighted ? c->fb_sw.as<float>() + at : nullptr;
        slots[b].wn = weighted ? (double)c->vx_nb[members[b]] : (double)m;
        at += m;
    }
    tab[B] = at;
    HGMM_TRY(ensure(c, c->vx_hand, sizeof(int64_t) * tab.size() + 64));
    HGMM_TRY(upload_table(c, c->vx_hand.p, tab.data(), sizeof(int64_t) * tab.size()));
    if (sizeof(int64_t) * tab.size() > (256u << 10)) HGMM_HIP(c, ctx_stream_sync(c));    // (tab leaves scope)
    const int64_t* d_first = c->vx_hand.as<int64_t>();
    handover_flat_kernel<<<(unsigned)((total + HO_BLOCK - 1) / HO_BLOCK), HO_BLOCK, 0, c->stream>>>(
        c->vx_cent.as<double>(), c->vx_cnt.as<int64_t>(), d_first, d_first + B + 1, B, total, c->fb_x.as<float>(),
        weighted ? c->fb_sw.as<float>() : nullptr);
    HGMM_HIP(c, hipGetLastError());
    return flat_batch_run(c, what, B, slots.data(), cov_type, variant, J, max_iter, tol, mu, cov, w, inv_std_out, lls_out,
                          n_iter_out, converged_out);
}

extern "C" int hgmm_points_rows_f64(hgmm_ctx* c, const int64_t* rows, int64_t k, double* out) {
    HGMM_ENTER(c);
    const char* what = "hgmm_points_rows_f64";
    if (!c->have_f64 || c->n <= 0) return fail(c, HGMM_ERR_STATE, "%s: no cloud with a float64 view (set or bind points first)", what);
    if (k < 0 || !rows || !out) return fail(c, HGMM_ERR_ARG, "%s: k = %lld, or a NULL argument", what, (long long)k);
    for (int64_t j = 0; j < k; ++j)
        if (rows[j] < 0 || rows[j] >= c->n)
            return fail(c, HGMM_ERR_ARG, "%s: rows[%lld] = %lld, but the resident cloud has %lld points", what, (long long)j,
                        (long long)rows[j], (long long)c->n);
    if (k == 0) return HGMM_OK;
    HGMM_TRY(stage_init_rows(c, rows, k, nullptr, 1));
    StagedDownloads dl(c);
    dl.add(out, c->scratch.p, sizeof(double) * 3 * (size_t)k);
    HGMM_HIP(c, dl.finish());
    return HGMM_OK;
}
