// The body of the fused L2 cost kernels (gmmreg_l2_kernels.hip), included inside the kernel's braces as flat_fused_body.h,
// fullcov_body.h and kmeans_body.h are: l2_cost_kernel (hgmm_l2_cost) and l2_solve_cost_kernel (hgmm_l2_solve), which only
// differs by leaving at its first load when its hypothesis has left the solve.  An include and not a function: l2_cost_kernel
// is then compiled from the very text it had, and its code object stays what it was (tools/isa_diff.py).
// The including kernel has `#pragma clang fp contract(off)` in force and defines next to its arguments
//   __shared__ double tile[L2_TILE][L2_ROW]
//   const int r                   the hypothesis (blockIdx.y)
//   const L2Hyp& h                hyps[r]
// No include guard: the file is meant to be included more than once.
    const L2Pair p = pairs[h.pair];
    const int nsp = l2_splits(p.Jt);
    const int w = blockIdx.x;
    if (w >= ((p.Js + L2_BLOCK - 1) / L2_BLOCK) * nsp) return;      // (uniform: the whole workgroup leaves)
    const int sb = w / nsp, sp = w - sb * nsp;
    const int i = sb * L2_BLOCK + (int)threadIdx.x;
    const bool live = i < p.Js;
    double x0 = 0.0, x1 = 0.0, x2 = 0.0, ps = 0.0;
    if (live) {
        const double* x = mu_s + 3 * (size_t)(p.s_first + i);
        x0 = x[0]; x1 = x[1]; x2 = x[2];
        ps = phi_s[p.s_first + i];
    }
    // y = rot x + t, each dot product one multiply and two fused multiply-adds in the order of the columns
    const double y0 = fma(x2, h.rot[2], fma(x1, h.rot[1], x0 * h.rot[0])) + h.t[0];
    const double y1 = fma(x2, h.rot[5], fma(x1, h.rot[4], x0 * h.rot[3])) + h.t[1];
    const double y2 = fma(x2, h.rot[8], fma(x1, h.rot[7], x0 * h.rot[6])) + h.t[2];
    const double neg_h2 = h.neg_h2, z = h.z;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;                  // g0, g1[3] of this split
    const int c_begin = sp * L2_SPLIT;
    const int c_end = min(p.Jt, c_begin + L2_SPLIT);
    for (int base = c_begin; base < c_end; base += L2_TILE) {
        const int cnt = min(L2_TILE, c_end - base);
        __syncthreads();
        for (int j = (int)threadIdx.x; j < cnt; j += L2_BLOCK) {
            const double* m = mu_t + 3 * (size_t)(p.t_first + base + j);
            const double ph = phi_t[p.t_first + base + j];
            const double m0 = m[0], m1 = m[1], m2 = m[2];
            tile[j][0] = m0; tile[j][1] = m1; tile[j][2] = m2;
            tile[j][3] = ph / z;
            tile[j][4] = (ph * m0) / z; tile[j][5] = (ph * m1) / z; tile[j][6] = (ph * m2) / z;
        }
        __syncthreads();
        for (int j = 0; j < cnt; ++j) {
            const double d0 = y0 - tile[j][0], d1 = y1 - tile[j][1], d2 = y2 - tile[j][2];
            const double e = exp((d0 * d0 + d1 * d1 + d2 * d2) / neg_h2);
            a0 += tile[j][3] * e;
            a1 += tile[j][4] * e;
            a2 += tile[j][5] * e;
            a3 += tile[j][6] * e;
        }
    }
    // a lane without a centre adds exact zeros, whatever the pose is (0 x NaN would not)
    double v[L2_NOUT];
    const double g0 = live ? (ps * (a0 * y0 - a1)) / h.two_s2 : 0.0;
    const double g1 = live ? (ps * (a0 * y1 - a2)) / h.two_s2 : 0.0;
    const double g2 = live ? (ps * (a0 * y2 - a3)) / h.two_s2 : 0.0;
    v[0] = live ? -(ps * a0) : 0.0;
    v[1] = g0; v[2] = g1; v[3] = g2;
    v[4] = g0 * x0; v[5] = g0 * x1; v[6] = g0 * x2;
    v[7] = g1 * x0; v[8] = g1 * x1; v[9] = g1 * x2;
    v[10] = g2 * x0; v[11] = g2 * x1; v[12] = g2 * x2;
    double* rec = records + ((size_t)r * wg_max + w) * L2_NOUT;
#pragma unroll
    for (int k = 0; k < L2_NOUT; ++k) {
        const double s = wave_sum_f64(v[k]);
        if (threadIdx.x == 0) rec[k] = s;
    }
