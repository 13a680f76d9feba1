// The bodies of eight kernels of the KMeans initialiser (kmeans_kernels.hip), included once per kernel -- plain and _w --
// inside the kernel's braces, as fullcov_body.h and flat_fused_body.h are: KMEANS_BODY selects the body (1 kmpp_first_kernel,
// 2 kmpp_step_kernel, 3 kmpp_fused_kernel, 4 kmeans_assign_kernel, 5 kmeans_accum_kernel, 6 kmeans_accum_lds_kernel, and the
// two that have no _w form: 7 kmeans_reduce_kernel, 8 kmeans_update_kernel).  The including kernel defines
//   constexpr bool WEIGHTED       the points carry weights (hgmm_kmeans_plusplus_weighted / _step_weighted / _lloyd_weighted)
//   const double* wts             ... [n_pad], on the row index of xs (NULL without)
// next to its own arguments.  An include and not a template: the unweighted kernels are then compiled from the very text they
// had before the weights, and their code objects stay what they were, instruction for instruction (tools/isa_diff.py).
// The BATCHED kernels (kmeans_batch.h: many clouds through one launch) include the same bodies once more: they declare the
// kernel's arguments as locals read from their member's row of a table, and the two names a body knows its place in the
// launch by,
//   KM_WG                         the workgroup's index within ITS CLOUD's launch   (serial kernels: blockIdx.x)
//   KM_NWG                        the workgroups that launch has for the cloud      (serial kernels: gridDim.x)
// as what the serial launch of that cloud alone would have given this workgroup.  Same text, same operations in the same
// order: a member's numbers are the serial kernels' bit for bit.
// No include guard: the file is meant to be included more than once.
#if KMEANS_BODY == 1    // kmpp_first_kernel
    __shared__ double sh[4];
    const int64_t i = (int64_t)KM_WG * KM_BLOCK + threadIdx.x;
    const double cx = xs[first], cy = xs[n_pad + first], cz = xs[2 * n_pad + first];
    double d = 0.0;
    if (i < n) d = dist2(xs[i], xs[n_pad + i], xs[2 * n_pad + i], cx, cy, cz);
    closest[i] = d;
    double term = d;
    if constexpr (WEIGHTED) term = i < n ? wts[i] * d : 0.0;
    const double t = block_sum_256(term, sh);
    if (threadIdx.x == 0) {
        bsum[KM_WG] = t;
        if (KM_WG == 0) {
            centres[0] = cx; centres[1] = cy; centres[2] = cz;
            ids[0] = first;
        }
    }
#elif KMEANS_BODY == 2    // kmpp_step_kernel
    __shared__ double shg[KM_MAX_TRIALS][KM_GROUP];
    const int lane = lane_id();
    const int64_t blk = (int64_t)KM_WG * KM_GROUP + wave_in_block();     // 256-point block of this wave
    const bool have = blk < B;
    const int64_t i0 = (have ? blk : 0) * KM_BLOCK + 4 * lane;                 // n_pad is a multiple of 256
    // every candidate's coordinates through ONE batch of scalar loads (index clamped, not branched on, so that the
    // loads can leave the per-candidate blocks): the tail's CU wrote them a moment ago and each cache line of them
    // is a trip through the fabric -- a load per loop iteration would chain those trips
    // (issued before the points' loads so that the two kinds of trip overlap)
    double cc[TMAX][3];
#pragma unroll
    for (int t = 0; t < TMAX; ++t) {
        const int tt = t < T ? t : T - 1;
        cc[t][0] = cand_xyz[3 * tt]; cc[t][1] = cand_xyz[3 * tt + 1]; cc[t][2] = cand_xyz[3 * tt + 2];
    }
    double x[4], y[4], z[4], cl[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) { x[q] = xs[i0 + q]; y[q] = xs[n_pad + i0 + q]; z[q] = xs[2 * n_pad + i0 + q]; cl[q] = closest[i0 + q]; }
    double wt[4] = {1.0, 1.0, 1.0, 1.0};                                       // (WEIGHTED) one more coalesced load per point
    if constexpr (WEIGHTED) {
#pragma unroll
        for (int q = 0; q < 4; ++q) wt[q] = wts[i0 + q];
    }
    if (fold >= 0 && have) {
        const double fx = centres[3 * fold], fy = centres[3 * fold + 1], fz = centres[3 * fold + 2];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const double d = dist2(x[q], y[q], z[q], fx, fy, fz);
            if (i0 + q < n && d < cl[q]) { cl[q] = d; closest[i0 + q] = d; }   // few points move once j is large
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) if (!have || !(i0 + q < n)) cl[q] = 0.0;      // padding contributes min(0, d) = 0
    if constexpr (WEIGHTED) {
#pragma unroll
        for (int q = 0; q < 4; ++q) if (!have || !(i0 + q < n)) wt[q] = 0.0;  // (whatever the weights' padding holds)
    }
#pragma unroll
    for (int t = 0; t < TMAX; ++t) {
        if (t < T) {
            const double cx = cc[t][0], cy = cc[t][1], cz = cc[t][2];
            double sacc = 0.0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const double m = fmin(cl[q], dist2(x[q], y[q], z[q], cx, cy, cz));
                if constexpr (WEIGHTED) sacc += wt[q] * m; else sacc += m;
            }
            const double w = wave_sum_f64(sacc);
            if (lane == 0) {
                if (have) part[(size_t)t * B + blk] = w;
                shg[t][wave_in_block()] = have ? w : 0.0;
            }
        }
    }
    __syncthreads();
    // the workgroup's 16 block sums, added in block order: what the tail's winner selection and group search read
    if ((int)threadIdx.x < T) {
        double s = 0.0;
#pragma unroll
        for (int q = 0; q < KM_GROUP; ++q) s += shg[threadIdx.x][q];
        part16[(size_t)threadIdx.x * KM_NWG + KM_WG] = s;
    }
#elif KMEANS_BODY == 3    // kmpp_fused_kernel
    const unsigned long long t_start = dbg ? (unsigned long long)wall_clock64() : 0ull;
    static_assert(KM_STEP_BLOCK == 1024, "the tail body is written for 1024 threads");
    __shared__ double shg[KM_MAX_TRIALS][KM_GROUP];
    __shared__ double sh_cand[3 * KM_MAX_TRIALS];
    __shared__ KmTailShared ts;
    const int lane = lane_id();
    const int64_t blk = (int64_t)KM_WG * KM_GROUP + wave_in_block();     // 256-point block of this wave
    const bool have = blk < B;
    const int64_t i0 = (have ? blk : 0) * KM_BLOCK + 4 * lane;                 // n_pad is a multiple of 256
    // the pass's operands do not depend on the tail: requested inside its first round of loads (see there)
    double pts[WEIGHTED ? 20 : 16];
    double fx, fy, fz;
    kmpp_tail_body<TMAX, WEIGHTED>(xs, n, n_pad, wts, closest, part_prev, part16_prev, G, nullptr, nullptr, B, T, j - 1, 1, 1,
                            rand_c, cand_prev, cand_xyz_prev, cand_next, cand_xyz_next, centres, ids, nullptr,
                            KM_WG == 0, sh_cand, fx, fy, fz, ts, dbg, t_start, pts, i0);
    __syncthreads();                                         // sh_cand
    km_stamp(dbg, 7, t_start);
    double x[4], y[4], z[4], cl[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) { x[q] = pts[q]; y[q] = pts[4 + q]; z[q] = pts[8 + q]; cl[q] = pts[12 + q]; }
    if (have) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const double d = dist2(x[q], y[q], z[q], fx, fy, fz);
            if (i0 + q < n && d < cl[q]) { cl[q] = d; closest[i0 + q] = d; }
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) if (!have || !(i0 + q < n)) cl[q] = 0.0;      // padding contributes min(0, d) = 0
    double wt[4] = {1.0, 1.0, 1.0, 1.0};
    if constexpr (WEIGHTED) {
#pragma unroll
        for (int q = 0; q < 4; ++q) wt[q] = (!have || !(i0 + q < n)) ? 0.0 : pts[16 + q];
    }
#pragma unroll
    for (int t = 0; t < TMAX; ++t) {
        if (t < T) {
            const double cx = sh_cand[3 * t], cy = sh_cand[3 * t + 1], cz = sh_cand[3 * t + 2];
            double sacc = 0.0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const double m = fmin(cl[q], dist2(x[q], y[q], z[q], cx, cy, cz));
                if constexpr (WEIGHTED) sacc += wt[q] * m; else sacc += m;
            }
            const double w = wave_sum_f64(sacc);
            if (lane == 0) {
                if (have) part_next[(size_t)t * B + blk] = w;
                shg[t][wave_in_block()] = have ? w : 0.0;
            }
        }
    }
    km_stamp(dbg, 9, t_start);
    __syncthreads();
    if ((int)threadIdx.x < T) {
        double s2 = 0.0;
#pragma unroll
        for (int q = 0; q < KM_GROUP; ++q) s2 += shg[threadIdx.x][q];
        part16_next[(size_t)threadIdx.x * KM_NWG + KM_WG] = s2;
    }
    km_stamp(dbg, 8, t_start);
#elif KMEANS_BODY == 4    // kmeans_assign_kernel
    if (done && *done) return;
    __shared__ double sh[4];
    __shared__ int shc[4];
    const int64_t i0 = (int64_t)KM_WG * (2 * KM_BLOCK) + threadIdx.x;
    const int64_t i1 = i0 + KM_BLOCK;
    const bool l0 = i0 < n, l1 = i1 < n;
    const int64_t j0 = l0 ? i0 : 0, j1 = l1 ? i1 : 0;
    const double x0 = xs[j0], y0 = xs[n_pad + j0], z0 = xs[2 * n_pad + j0];
    const double x1 = xs[j1], y1 = xs[n_pad + j1], z1 = xs[2 * n_pad + j1];
    double w0 = 1.0, w1 = 1.0;
    if constexpr (WEIGHTED) { w0 = wts[j0]; w1 = wts[j1]; }
    // Four centres at a time: their minimum (3 v_min_f64) is compared with the running best once, and only the
    // group's first index is recorded (1 compare + 3 selects per FOUR pairs instead of per pair: 7.75 instead of 10
    // lane-operations per pair); which of the four it was is settled afterwards by evaluating the winning group
    // again -- same arithmetic, so the same values, and the first index that attains the minimum wins as before.
    double b0 = INFINITY, b1 = INFINITY;
    int a0 = 0, a1 = 0;
    const int k4 = k & ~3;
    for (int j = 0; j < k4; j += 4) {
        double e0[4], e1[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const double cx = c4[4 * (j + u)], cy = c4[4 * (j + u) + 1], cz = c4[4 * (j + u) + 2];
            e0[u] = dist2(x0, y0, z0, cx, cy, cz);
            e1[u] = dist2(x1, y1, z1, cx, cy, cz);
        }
        const double m0 = fmin(fmin(e0[0], e0[1]), fmin(e0[2], e0[3]));
        const double m1 = fmin(fmin(e1[0], e1[1]), fmin(e1[2], e1[3]));
        if (m0 < b0) { b0 = m0; a0 = j; }
        if (m1 < b1) { b1 = m1; a1 = j; }
    }
    if (k4 > 0) {
        // the member of the winning group (divergent group index: vector loads, once per point)
        int w0 = a0, w1 = a1;
#pragma unroll
        for (int u = 3; u >= 0; --u) {
            const double* p0 = c4 + 4 * (a0 + u);
            const double* p1 = c4 + 4 * (a1 + u);
            if (dist2(x0, y0, z0, p0[0], p0[1], p0[2]) == b0) w0 = a0 + u;
            if (dist2(x1, y1, z1, p1[0], p1[1], p1[2]) == b1) w1 = a1 + u;
        }
        a0 = w0; a1 = w1;
    }
    for (int j = k4; j < k; ++j) {
        const double cx = c4[4 * j], cy = c4[4 * j + 1], cz = c4[4 * j + 2];
        const double d0 = dist2(x0, y0, z0, cx, cy, cz);
        const double d1 = dist2(x1, y1, z1, cx, cy, cz);
        if (d0 < b0) { b0 = d0; a0 = j; }
        if (d1 < b1) { b1 = d1; a1 = j; }
    }
    int changed = 0;
    double in = 0.0;
    if (l0) {
        changed += labels[i0] != a0;
        labels[i0] = a0;
        mind2[i0] = b0;
        if constexpr (WEIGHTED) in += w0 * b0; else in += b0;
    }
    if (l1) {
        changed += labels[i1] != a1;
        labels[i1] = a1;
        mind2[i1] = b1;
        if constexpr (WEIGHTED) in += w1 * b1; else in += b1;
    }
    const int wc = wave_reduce_i(changed, OpAddI());
    if (lane_id() == 0) shc[wave_in_block()] = wc;
    const double t = block_sum_256(in, sh);
    if (threadIdx.x == 0) {
        inertia_part[KM_WG] = t;
        const int tc = shc[0] + shc[1] + shc[2] + shc[3];
        if (tc) atomicAdd(n_changed, (unsigned long long)tc);
    }
#elif KMEANS_BODY == 5    // kmeans_accum_kernel
    if (done && *done) return;
    __shared__ double sh[4][64][4];
    const int lane = lane_id(), wave = wave_in_block();
    double ax[NSLOT], ay[NSLOT], az[NSLOT], ac[NSLOT];
#pragma unroll
    for (int s = 0; s < NSLOT; ++s) ax[s] = ay[s] = az[s] = ac[s] = 0.0;
    const int64_t waves = (int64_t)KM_NWG * 4;
    const int64_t per = ((n + waves - 1) / waves + 63) / 64 * 64;
    const int64_t gw = (int64_t)KM_WG * 4 + wave;
    const int64_t begin = gw * per;
    const int64_t end = begin + per < n ? begin + per : n;
    for (int64_t base = begin; base < end; base += 64) {
        const int64_t i = base + lane;
        const bool ok = i < end;
        const int64_t ii = ok ? i : 0;
        const int rel = ok ? labels[ii] - slot0 * 64 : -1;
        double x = xs[ii], y = xs[n_pad + ii], z = xs[2 * n_pad + ii];
        double wgt = 1.0;
        if constexpr (WEIGHTED) { wgt = wts[ii]; x *= wgt; y *= wgt; z *= wgt; }
        const int cnt = (int)(end - base < 64 ? end - base : 64);
        for (int t = 0; t < cnt; ++t) {
            const int r = __builtin_amdgcn_readlane(rel, t);
            if (r < 0 || r >= NSLOT * 64) continue;
            const double px = readlane_f64(x, t), py = readlane_f64(y, t), pz = readlane_f64(z, t);
            double pw = 1.0;
            if constexpr (WEIGHTED) pw = readlane_f64(wgt, t);
            const int s = r >> 6;
            if (lane == (r & 63)) {
#pragma unroll
                for (int u = 0; u < NSLOT; ++u)
                    if (u == s) { ax[u] += px; ay[u] += py; az[u] += pz; ac[u] += pw; }
            }
        }
    }
    double* out = partial + (size_t)KM_WG * k_alloc * 4;
#pragma unroll
    for (int s = 0; s < NSLOT; ++s) {
        sh[wave][lane][0] = ax[s];
        sh[wave][lane][1] = ay[s];
        sh[wave][lane][2] = az[s];
        sh[wave][lane][3] = ac[s];
        __syncthreads();
        const int l = threadIdx.x >> 2, f = threadIdx.x & 3;
        out[((size_t)(slot0 + s) * 64 + l) * 4 + f] = (sh[0][l][f] + sh[1][l][f]) + (sh[2][l][f] + sh[3][l][f]);
        __syncthreads();
    }
#elif KMEANS_BODY == 6    // kmeans_accum_lds_kernel
    if (done && *done) return;
    extern __shared__ double km_lds[];
    const int lane = lane_id(), wave = wave_in_block();
    const int tsz = k_alloc * 4;
    double* T = km_lds + (size_t)wave * tsz;              // this wave's sums
    double* S = km_lds + (size_t)4 * tsz + wave * 256;    // [64 points][4] staging of the current batch
    for (int e = lane; e < tsz; e += 64) T[e] = 0.0;
    // Wave-level ordering contract, stated instead of assumed: lanes 0..3 read what OTHER lanes of this wave stored
    // (the staging tile, the cleared table).  The hardware executes one wave's LDS operations in order, but the
    // compiler may reorder accesses it cannot prove to alias; a wavefront-scope release / acquire fence pair plus the
    // (free) wave barrier pins the order in the generated code.
    auto wave_lds_sync = [] {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    };
    wave_lds_sync();                                      // table cleared before the first ds_add
    const int64_t waves = (int64_t)KM_NWG * 4;
    const int64_t per = ((n + waves - 1) / waves + 63) / 64 * 64;
    const int64_t gw = (int64_t)KM_WG * 4 + wave;
    const int64_t begin = gw * per;
    const int64_t end = begin + per < n ? begin + per : n;
    const int f = lane & 3;
    for (int64_t base = begin; base < end; base += 64) {
        const int64_t i = base + lane;
        const bool ok = i < end;
        const int64_t ii = ok ? i : 0;
        const int lab = ok ? labels[ii] : 0;
        const double x = xs[ii], y = xs[n_pad + ii], z = xs[2 * n_pad + ii];
        wave_lds_sync();                                  // the previous batch has been consumed
        if constexpr (WEIGHTED) {
            const double wgt = wts[ii];
            S[lane * 4 + 0] = wgt * x; S[lane * 4 + 1] = wgt * y; S[lane * 4 + 2] = wgt * z; S[lane * 4 + 3] = wgt;
        } else {
            S[lane * 4 + 0] = x; S[lane * 4 + 1] = y; S[lane * 4 + 2] = z; S[lane * 4 + 3] = 1.0;
        }
        wave_lds_sync();                                  // all 64 lanes' stores before lanes 0..3 read them
        const int cnt = (int)(end - base < 64 ? end - base : 64);
        if (lane < 4) {
            int t = 0;
            for (; t + 8 <= cnt; t += 8) {
                double v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = S[(t + u) * 4 + f];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int r = __builtin_amdgcn_readlane(lab, t + u);
                    (void)__hip_atomic_fetch_add(&T[r * 4 + f], v[u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            }
            for (; t < cnt; ++t) {
                const int r = __builtin_amdgcn_readlane(lab, t);
                (void)__hip_atomic_fetch_add(&T[r * 4 + f], S[t * 4 + f], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
    }
    __syncthreads();
    double* out = partial + (size_t)KM_WG * tsz;
    for (int e = threadIdx.x; e < tsz; e += KM_BLOCK)
        out[e] = (km_lds[e] + km_lds[tsz + e]) + (km_lds[2 * tsz + e] + km_lds[3 * tsz + e]);
#elif KMEANS_BODY == 7    // kmeans_reduce_kernel
    if (done && *done) return;
    __shared__ double sh[8][32];
    __shared__ double shi[4];
    const int e_loc = threadIdx.x & 31, slice = threadIdx.x >> 5;
    const int e = KM_WG * 32 + e_loc;
    double s = 0.0;
    if (e < 4 * k) {
        const int per = (nb + 7) / 8;
        const int b0 = slice * per, b1 = min(nb, b0 + per);
        for (int b = b0; b < b1; ++b) s += partial[(size_t)b * k_alloc * 4 + e];
    }
    sh[slice][e_loc] = s;
    __syncthreads();
    if (slice == 0 && e < 4 * k) {
        double t = 0.0;
#pragma unroll
        for (int q = 0; q < 8; ++q) t += sh[q][e_loc];
        out[e] = t;
    }
    if (KM_WG == 0) {
        double v = 0.0;
        for (int b = threadIdx.x; b < nib; b += KM_BLOCK) v += inertia_part[b];
        const double t = block_sum_256(v, shi);
        if (threadIdx.x == 0) {
            out[4 * k] = t;
            out[4 * k + 1] = (double)n_changed[0];
        }
    }
#elif KMEANS_BODY == 8    // kmeans_update_kernel
    if (ctl->done) return;
    __shared__ double sh[4];
    __shared__ int sh_empty;
    if (threadIdx.x == 0) sh_empty = 0;
    __syncthreads();
    int empty = 0;
    for (int j = threadIdx.x; j < k; j += 256) empty |= out[4 * j + 3] == 0.0;
    if (empty) sh_empty = 1;
    __syncthreads();
    if (sh_empty) {
        if (threadIdx.x == 0) { ctl->needs_host = 1; ctl->done = 1; }
        return;
    }
    double shift = 0.0;
    for (int j = threadIdx.x; j < k; j += 256) {
        const double alpha = 1.0 / out[4 * j + 3];
        const double n0 = out[4 * j] * alpha, n1 = out[4 * j + 1] * alpha, n2 = out[4 * j + 2] * alpha;
        const double d0 = n0 - c3[3 * j], d1 = n1 - c3[3 * j + 1], d2 = n2 - c3[3 * j + 2];
        const double nrm = sqrt((d0 * d0 + d1 * d1) + d2 * d2);
        shift += nrm * nrm;
        c3[3 * j] = n0; c3[3 * j + 1] = n1; c3[3 * j + 2] = n2;
    }
    const double tot = block_sum_256(shift, sh);
    if (threadIdx.x == 0) {
        const int it = ctl->it + 1;
        ctl->it = it;
        if (out[4 * k + 1] == 0.0) { ctl->strict = 1; ctl->done = 1; }
        else if (tot <= tol_abs || it >= max_iter) ctl->done = 1;
        *changed = 0ull;                                   // next iteration's counter
    }
#endif
