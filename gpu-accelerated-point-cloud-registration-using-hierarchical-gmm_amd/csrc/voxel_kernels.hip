// Voxel-grid down-sample on the device: centroids + counts of one cloud or of B clouds in the same launches
// (include/hgmm.h: hgmm_voxel_downsample_*).  The definition is pointcloud_io.voxel_down_sample on float64 -- origin
// min - v / 2, index floor((p - origin) / v), voxels in lexicographic (ix, iy, iz) order, centroid = the float64 sum of the
// voxel's points in ascending point index, started from +0.0 and divided once by the count -- and every step below is
// chosen so that the result has that function's bits:
//   1 voxel_bbox_kernel      min / max per cloud and axis (exact in any order: integer atomics on the order-preserving
//                            encoding of a double) + the first non-finite row (integer atomicMin)
//     host                   6 doubles per cloud -> origin, extents, key bits; the refusals
//   2 voxel_keys_kernel      key = (ix ny + iy) nz + iz, the cloud number above the largest cloud's key bits; one IEEE
//                            subtraction, one IEEE division, one floor per axis -- no reciprocal, no fused multiply-add
//   3 voxel_sort_pairs       STABLE radix sort of (key, row) over the bits in use (voxel_sort.hip)
//   4 voxel_segment_heads    positions where the sorted key changes, compacted: M and the voxels' first positions
//   5 voxel_centroid_kernel  one thread per voxel walks its rows in sorted order = ascending row index
// No floating-point atomics.  A voxel with very many points makes the walk of step 5 long (one thread adds them one after
// the other): accepted, the order of summation is not traded for speed.
// The buffers (hgmm_ctx.h: vx_*) are the call's own: the resident cloud, its weights, a forest, a target or a tree are
// neither read nor written.
#include "hgmm_ctx.h"
#include "voxel_sort.h"

#include <cfloat>
#include <climits>

#pragma clang fp contract(off)

namespace hgmm {

struct VoxelBox {                       // per cloud, filled by voxel_bbox_kernel
    unsigned long long mn[3], mx[3];    // order-preserving encodings (ord_enc) of the smallest / largest coordinate
    int bad;                            // first row (within the cloud) with a non-finite coordinate; INT_MAX: none
    int pad;
};
struct VoxelGrid {                      // per cloud, formed on the host from the box
    double origin[3];
    int64_t ny, nz;
};
constexpr int VX_BLOCK = 256;
constexpr int VX_BBOX_ROWS = 2048;      // rows per workgroup of the bounding-box pass

// u < v as doubles <=> ord_enc(u) < ord_enc(v) as integers (-0.0 below +0.0, which no result depends on: origin and
// extents come out the same for either)
__host__ __device__ inline unsigned long long ord_enc(double x) {
    unsigned long long u;
    memcpy(&u, &x, 8);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
inline double ord_dec(unsigned long long e) {
    const unsigned long long u = (e >> 63) ? (e & 0x7fffffffffffffffull) : ~e;
    double x;
    memcpy(&x, &u, 8);
    return x;
}

__device__ inline void box_point(VoxelBox* bx, double x, int d) {
    atomicMin(&bx->mn[d], ord_enc(x));
    atomicMax(&bx->mx[d], ord_enc(x));
}

template <class IN>
__global__ __launch_bounds__(VX_BLOCK) void voxel_bbox_kernel(const IN* __restrict__ in, int64_t total,
                                                               const int64_t* __restrict__ first, int B,
                                                               VoxelBox* __restrict__ box) {
    const int64_t lo = (int64_t)blockIdx.x * VX_BBOX_ROWS;
    const int64_t hi = lo + VX_BBOX_ROWS < total ? lo + VX_BBOX_ROWS : total;
    const int b0 = find_cloud(first, B, lo);
    if (first[b0 + 1] < hi) {
        // the workgroup's rows belong to more than one cloud (at most B - 1 workgroups): every point for itself
        for (int64_t i = lo + threadIdx.x; i < hi; i += VX_BLOCK) {
            const int b = find_cloud(first, B, i);
            for (int d = 0; d < 3; ++d) {
                const double x = (double)in[3 * i + d];
                if (!(fabs(x) <= DBL_MAX)) atomicMin(&box[b].bad, (int)(i - first[b]));
                else box_point(&box[b], x, d);
            }
        }
        return;
    }
    double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    int bad = INT_MAX;
    for (int64_t i = lo + threadIdx.x; i < hi; i += VX_BLOCK)
        for (int d = 0; d < 3; ++d) {
            const double x = (double)in[3 * i + d];
            if (!(fabs(x) <= DBL_MAX)) { const int r = (int)(i - first[b0]); bad = r < bad ? r : bad; }
            else { mn[d] = fmin(mn[d], x); mx[d] = fmax(mx[d], x); }
        }
    for (int off = 32; off > 0; off >>= 1) {
        for (int d = 0; d < 3; ++d) {
            mn[d] = fmin(mn[d], __shfl_xor(mn[d], off));
            mx[d] = fmax(mx[d], __shfl_xor(mx[d], off));
        }
        const int o = __shfl_xor(bad, off);
        bad = o < bad ? o : bad;
    }
    if ((threadIdx.x & 63) == 0) {
        for (int d = 0; d < 3; ++d)
            if (mn[d] <= mx[d]) { atomicMin(&box[b0].mn[d], ord_enc(mn[d])); atomicMax(&box[b0].mx[d], ord_enc(mx[d])); }
        if (bad != INT_MAX) atomicMin(&box[b0].bad, bad);
    }
}

template <class IN>
__global__ __launch_bounds__(VX_BLOCK) void voxel_keys_kernel(const IN* __restrict__ in, int64_t total,
                                                               const int64_t* __restrict__ first, int B,
                                                               const VoxelGrid* __restrict__ grid, double v, unsigned key_bits,
                                                               unsigned long long* __restrict__ keys, uint32_t* __restrict__ rows) {
    const int64_t i = (int64_t)blockIdx.x * VX_BLOCK + threadIdx.x;
    if (i >= total) return;
    const int b = B > 1 ? find_cloud(first, B, i) : 0;
    const VoxelGrid g = grid[b];
    unsigned long long idx[3];
    for (int d = 0; d < 3; ++d) idx[d] = (unsigned long long)(long long)floor(((double)in[3 * i + d] - g.origin[d]) / v);
    unsigned long long key = (idx[0] * (unsigned long long)g.ny + idx[1]) * (unsigned long long)g.nz + idx[2];
    if (B > 1) key |= (unsigned long long)b << key_bits;
    keys[i] = key;
    rows[i] = (uint32_t)i;
}

// out[0] = M (from voxel_segment_heads); out[1 + b] <- the first voxel of cloud b (every cloud has one)
template <class IN>
__global__ __launch_bounds__(VX_BLOCK) void voxel_centroid_kernel(const IN* __restrict__ in, int64_t total,
                                                                   const int64_t* __restrict__ first, int B,
                                                                   const uint32_t* __restrict__ heads,
                                                                   const uint32_t* __restrict__ sorted_rows, uint32_t M,
                                                                   uint32_t* __restrict__ out, double* __restrict__ cent,
                                                                   int64_t* __restrict__ cnt) {
    const int64_t vx = (int64_t)blockIdx.x * VX_BLOCK + threadIdx.x;
    if (vx >= (int64_t)M) return;
    const int64_t s = heads[vx];
    const int64_t e = vx + 1 < (int64_t)M ? (int64_t)heads[vx + 1] : total;
    if (vx == 0) out[1] = 0;
    else if (B > 1) {
        const int b = find_cloud(first, B, s);
        if (find_cloud(first, B, heads[vx - 1]) != b) out[1 + b] = (uint32_t)vx;
    }
    double sum[3] = {0.0, 0.0, 0.0};
    for (int64_t r = s; r < e; ++r) {
        const int64_t row = sorted_rows[r];
        for (int d = 0; d < 3; ++d) sum[d] += (double)in[3 * row + d];
    }
    const double n = (double)(e - s);
    for (int d = 0; d < 3; ++d) cent[3 * vx + d] = sum[d] / n;
    cnt[vx] = e - s;
}

static unsigned bits_of(unsigned long long x) {         // bits needed to write x
    unsigned b = 0;
    while (x) { ++b; x >>= 1; }
    return b;
}

template <class IN>
static int voxel_downsample(hgmm_ctx* c, int B, const IN* const* xyz, const int64_t* counts, double v, int64_t* m_out) {
    HGMM_ENTER(c);
    if (B < 1 || !xyz || !counts) return fail(c, HGMM_ERR_ARG, "voxel down-sample: B = %d, or a NULL argument", B);
    if (!(v > 0.0) || !(v <= DBL_MAX)) return fail(c, HGMM_ERR_ARG, "voxel down-sample: the voxel size must be finite and > 0, got %g", v);
    std::vector<int64_t> first((size_t)B + 1, 0);
    for (int b = 0; b < B; ++b) {
        if (!xyz[b] || counts[b] < 1) return fail(c, HGMM_ERR_ARG, "voxel down-sample: cloud %d is empty (n = %lld)", b, (long long)counts[b]);
        if (counts[b] >= ((int64_t)1 << 31) || first[b] + counts[b] >= ((int64_t)1 << 31))
            return fail(c, HGMM_ERR_ARG, "voxel down-sample: 2^31 points or more (rows are 32-bit indices)");
        first[b + 1] = first[b] + counts[b];
    }
    const int64_t total = first[B];

    // the table block: first rows, boxes, grids, M + first voxels
    const size_t off_box = sizeof(int64_t) * ((size_t)B + 1);
    const size_t off_grid = off_box + sizeof(VoxelBox) * (size_t)B;
    const size_t off_out = off_grid + sizeof(VoxelGrid) * (size_t)B;
    const size_t tab_bytes = off_out + sizeof(uint32_t) * ((size_t)B + 2);
    HGMM_TRY(ensure(c, c->vx_tab, tab_bytes));
    HGMM_TRY(ensure(c, c->vx_in, sizeof(IN) * 3 * (size_t)total));
    char* tab = c->vx_tab.as<char>();
    const int64_t* d_first = reinterpret_cast<const int64_t*>(tab);
    VoxelBox* d_box = reinterpret_cast<VoxelBox*>(tab + off_box);
    VoxelGrid* d_grid = reinterpret_cast<VoxelGrid*>(tab + off_grid);
    uint32_t* d_out = reinterpret_cast<uint32_t*>(tab + off_out);
    const IN* d_in = c->vx_in.as<IN>();

    std::vector<char> h_head(off_grid);
    memcpy(h_head.data(), first.data(), off_box);
    for (int b = 0; b < B; ++b) {
        VoxelBox bx;
        for (int d = 0; d < 3; ++d) { bx.mn[d] = ~0ull; bx.mx[d] = 0ull; }
        bx.bad = INT_MAX;
        bx.pad = 0;
        memcpy(h_head.data() + off_box + sizeof(VoxelBox) * (size_t)b, &bx, sizeof bx);
    }
    HGMM_TRY(upload_table(c, tab, h_head.data(), off_grid));
    for (int b = 0; b < B; ++b)
        HGMM_HIP(c, hipMemcpyAsync(c->vx_in.as<IN>() + 3 * first[b], xyz[b], sizeof(IN) * 3 * (size_t)counts[b],
                                   hipMemcpyHostToDevice, c->stream));

    ProfScope prof(c, HGMM_K_VOXEL);
    // 1 ---- bounding boxes ------------------------------------------------------------------------------------------
    voxel_bbox_kernel<IN><<<(unsigned)((total + VX_BBOX_ROWS - 1) / VX_BBOX_ROWS), VX_BLOCK, 0, c->stream>>>(d_in, total, d_first, B, d_box);
    HGMM_HIP(c, hipGetLastError());
    std::vector<VoxelBox> box((size_t)B);
    StagedDownloads dl(c);
    dl.add(box.data(), d_box, sizeof(VoxelBox) * (size_t)B);
    HGMM_HIP(c, dl.finish());
    std::vector<VoxelGrid> grid((size_t)B);
    unsigned key_bits = 1;
    for (int b = 0; b < B; ++b) {
        if (box[b].bad != INT_MAX)
            return B == 1 ? fail(c, HGMM_ERR_ARG, "voxel down-sample: row %d has a non-finite coordinate", box[b].bad)
                          : fail(c, HGMM_ERR_ARG, "voxel down-sample: cloud %d, row %d has a non-finite coordinate", b, box[b].bad);
        unsigned __int128 cells = 1;
        int64_t ext[3] = {1, 1, 1};
        for (int d = 0; d < 3; ++d) {
            const double mn = ord_dec(box[b].mn[d]), mx = ord_dec(box[b].mx[d]);
            const double half = 0.5 * v;
            grid[b].origin[d] = mn - half;
            const double last = floor((mx - grid[b].origin[d]) / v);          // the index of the largest coordinate
            if (!(last < 9223372036854775807.0)) cells = ~(unsigned __int128)0;
            else ext[d] = (int64_t)last + 1;
            if (cells < ((unsigned __int128)1 << 63)) cells *= (unsigned __int128)ext[d];
        }
        if (cells >= ((unsigned __int128)1 << 63))
            return fail(c, HGMM_ERR_ARG, "voxel down-sample: the voxel grid of cloud %d has 2^63 cells or more at voxel size %g "
                                         "(its keys do not fit 64 bits)", b, v);
        grid[b].ny = ext[1];
        grid[b].nz = ext[2];
        const unsigned kb = bits_of((unsigned long long)cells - 1);
        key_bits = kb > key_bits ? kb : key_bits;
    }
    const unsigned cloud_bits = bits_of((unsigned long long)B - 1);
    if (key_bits + cloud_bits > 64)
        return fail(c, HGMM_ERR_ARG, "voxel down-sample: the voxel grid needs %u key bits and the batch %u cloud bits: more than 64",
                    key_bits, cloud_bits);

    // ---- from here on the call succeeds unless the runtime fails: the buffers of the result may be touched ----------------
    HGMM_TRY(ensure(c, c->vx_keys, sizeof(uint64_t) * (size_t)total));
    HGMM_TRY(ensure(c, c->vx_keys2, sizeof(uint64_t) * (size_t)total));
    HGMM_TRY(ensure(c, c->vx_rows, sizeof(uint32_t) * (size_t)total));
    HGMM_TRY(ensure(c, c->vx_rows2, sizeof(uint32_t) * (size_t)total));
    HGMM_TRY(ensure(c, c->vx_heads, sizeof(uint32_t) * (size_t)total));
    size_t tmp_sort = 0, tmp_heads = 0;
    HGMM_HIP(c, voxel_sort_pairs(nullptr, &tmp_sort, nullptr, nullptr, nullptr, nullptr, (size_t)total, key_bits + cloud_bits, c->stream));
    HGMM_HIP(c, voxel_segment_heads(nullptr, &tmp_heads, nullptr, nullptr, nullptr, (size_t)total, c->stream));
    HGMM_TRY(ensure(c, c->vx_tmp, tmp_sort > tmp_heads ? tmp_sort : tmp_heads));
    HGMM_TRY(upload_table(c, d_grid, grid.data(), sizeof(VoxelGrid) * (size_t)B));
    // 2 ---- keys ----------------------------------------------------------------------------------------------------------
    unsigned long long* keys = c->vx_keys.as<unsigned long long>();
    unsigned long long* keys2 = c->vx_keys2.as<unsigned long long>();
    voxel_keys_kernel<IN><<<(unsigned)((total + VX_BLOCK - 1) / VX_BLOCK), VX_BLOCK, 0, c->stream>>>(
        d_in, total, d_first, B, d_grid, v, key_bits, keys, c->vx_rows.as<uint32_t>());
    HGMM_HIP(c, hipGetLastError());
    // 3, 4 ---- sort, segment heads ----------------------------------------------------------------------------------------
    HGMM_HIP(c, voxel_sort_pairs(c->vx_tmp.p, &tmp_sort, reinterpret_cast<const uint64_t*>(keys), reinterpret_cast<uint64_t*>(keys2),
                                 c->vx_rows.as<uint32_t>(), c->vx_rows2.as<uint32_t>(), (size_t)total, key_bits + cloud_bits, c->stream));
    HGMM_HIP(c, voxel_segment_heads(c->vx_tmp.p, &tmp_heads, reinterpret_cast<const uint64_t*>(keys2), c->vx_heads.as<uint32_t>(),
                                    d_out, (size_t)total, c->stream));
    uint32_t M = 0;
    dl.add(&M, d_out, sizeof M);
    HGMM_HIP(c, dl.finish());
    if (M < (uint32_t)B || (int64_t)M > total) return fail(c, HGMM_ERR_HIP, "voxel down-sample: %u segments for %lld points", M, (long long)total);
    c->vx_have = false;                          // (a runtime failure below leaves no result rather than a mixed one)
    HGMM_TRY(ensure(c, c->vx_cent, sizeof(double) * 3 * (size_t)M));
    HGMM_TRY(ensure(c, c->vx_cnt, sizeof(int64_t) * (size_t)M));
    // 5 ---- centroids -----------------------------------------------------------------------------------------------------
    voxel_centroid_kernel<IN><<<(unsigned)((M + VX_BLOCK - 1) / VX_BLOCK), VX_BLOCK, 0, c->stream>>>(
        d_in, total, d_first, B, c->vx_heads.as<uint32_t>(), c->vx_rows2.as<uint32_t>(), M, d_out, c->vx_cent.as<double>(),
        c->vx_cnt.as<int64_t>());
    HGMM_HIP(c, hipGetLastError());
    std::vector<uint32_t> h_out((size_t)B + 1);
    dl.add(h_out.data(), d_out, sizeof(uint32_t) * ((size_t)B + 1));
    HGMM_HIP(c, dl.finish());
    c->vx_m = (int64_t)M;
    c->vx_mb.resize((size_t)B);
    c->vx_first.resize((size_t)B);
    for (int b = 0; b < B; ++b) {
        c->vx_first[b] = (int64_t)h_out[1 + b];
        c->vx_mb[b] = (int64_t)(b + 1 < B ? h_out[2 + b] : M) - (int64_t)h_out[1 + b];
    }
    c->vx_nb.assign(counts, counts + B);
    ++c->vx_serial;
    c->vx_have = true;
    if (m_out)
        for (int b = 0; b < B; ++b) m_out[b] = c->vx_mb[b];
    return HGMM_OK;
}

}  // namespace hgmm

using namespace hgmm;

extern "C" int hgmm_voxel_downsample_f64(hgmm_ctx* c, const double* xyz, int64_t n, double voxel, int64_t* m_out) {
    return voxel_downsample<double>(c, 1, &xyz, &n, voxel, m_out);
}
extern "C" int hgmm_voxel_downsample_f32(hgmm_ctx* c, const float* xyz, int64_t n, double voxel, int64_t* m_out) {
    return voxel_downsample<float>(c, 1, &xyz, &n, voxel, m_out);
}
extern "C" int hgmm_voxel_downsample_batch_f64(hgmm_ctx* c, int B, const double* const* xyz, const int64_t* counts, double voxel,
                                               int64_t* m_out) {
    return voxel_downsample<double>(c, B, xyz, counts, voxel, m_out);
}
extern "C" int hgmm_voxel_downsample_batch_f32(hgmm_ctx* c, int B, const float* const* xyz, const int64_t* counts, double voxel,
                                               int64_t* m_out) {
    return voxel_downsample<float>(c, B, xyz, counts, voxel, m_out);
}

extern "C" int hgmm_voxel_downsample_get(hgmm_ctx* c, double* centroids_out, int64_t* counts_out) {
    HGMM_ENTER(c);
    if (!c->vx_have) return fail(c, HGMM_ERR_STATE, "hgmm_voxel_downsample_get: no down-sample has succeeded on this context");
    StagedDownloads dl(c);
    dl.add(centroids_out, c->vx_cent.p, sizeof(double) * 3 * (size_t)c->vx_m);
    dl.add(counts_out, c->vx_cnt.p, sizeof(int64_t) * (size_t)c->vx_m);
    HGMM_HIP(c, dl.finish());
    return HGMM_OK;
}
