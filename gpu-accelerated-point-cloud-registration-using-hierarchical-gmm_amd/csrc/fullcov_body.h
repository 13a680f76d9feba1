// The bodies of three E-step kernels of the flat full-covariance fit (fullcov_kernels.hip), included once per kernel -- plain and
// _w -- inside the kernel's braces, as flat_fused_body.h is: FULLCOV_BODY selects the body (1 full_pass_kernel, 2
// full_moments_kernel, 3 full_fused_f32_kernel).  The including kernel defines
//   constexpr bool WEIGHTED       the points carry weights (hgmm_fullcov_fit_weighted / hgmm_fullcov_estep_weighted)
//   const double* wsrc            ... [n], parallel to xs (NULL without)
// next to its own arguments.  An include and not a template: the unweighted kernels are then compiled from the very text they
// had before the weights, and their code objects stay what they were, instruction for instruction (tools/isa_diff.py).
// No include guard: the file is meant to be included more than once.
#if FULLCOV_BODY == 1
    __shared__ double tile[LL_TILE][11];
    __shared__ double shq[CH / 64];
    const int64_t i = (int64_t)blockIdx.x * CH + threadIdx.x;
    const bool active = i < n;
    double x0 = 0.0, x1 = 0.0, x2 = 0.0;
    if (active) { x0 = xs[i]; x1 = xs[n_pad + i]; x2 = xs[2 * n_pad + i]; }
    double den = 0.0, tot = 0.0, best = -1.0;
    int am = 0;
    for (int base = 0; base < J; base += LL_TILE) {
        const int cnt = (J - base < LL_TILE) ? J - base : LL_TILE;
        __syncthreads();
        for (int t = threadIdx.x; t < cnt * 11; t += CH) {
            const int node = t / 11, fidx = t % 11;
            tile[node][fidx] = prep[PREP_N * (base + node) + fidx];
        }
        __syncthreads();
        for (int node = 0; node < cnt; ++node) {
            const double wE = tile[node][9];
            if (wE == 0.0) continue;                                    // workgroup-uniform
            const double d0 = x0 - tile[node][6], d1 = x1 - tile[node][7], d2 = x2 - tile[node][8];
            const double q = sym3_quad(tile[node][0], tile[node][1], tile[node][2], tile[node][3], tile[node][4],
                                       tile[node][5], d0, d1, d2);
            double g = 0.0;
            if (__any(q < 1500.0)) g = wE * exp(-0.5 * q);
            den += g;
            if (tile[node][10] != 0.0) tot += g;      // pi >= eps: counts towards the log-likelihood
            if (g > best) { best = g; am = base + node; }
        }
    }
    if (active) {
        den_out[i] = den;
        label_out[i] = (den > TREE_EPS) ? am : 0;   // all gammas zero -> argmax = 0 (C:178,184)
    }
    double lq = active ? log(fmax(tot, TREE_EPS)) : 0.0;
    if (WEIGHTED) lq *= active ? wsrc[i] : 0.0;
    lq = wave_sum_f64(lq);
    if (lane_id() == 0) shq[wave_in_block()] = lq;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int w = 0; w < CH / 64; ++w) t += shq[w];
        block_q[blockIdx.x] = t;
    }
#elif FULLCOV_BODY == 2
    __shared__ double G[FULL_WAVES][16][FULL_LD];    // gamma, component-major, per wave
    __shared__ double F[FULL_WAVES][16][FULL_LD];    // features, feature-major, per wave
    __shared__ double red[FULL_WAVES][16][16];
    const int w = wave_in_block(), lane = lane_id();
    const int64_t groups = (n + 63) / 64;
    const int64_t nw = (int64_t)gridDim.x * FULL_WAVES;
    const int64_t per = (groups + nw - 1) / nw;
    const int64_t gw = (int64_t)blockIdx.x * FULL_WAVES + w;
    const int64_t g0 = gw * per, g1 = (g0 + per < groups) ? g0 + per : groups;
    const int a_idx = lane & 15, b_idx = lane >> 4;

    for (int tile = 0; tile < J16; tile += 16) {
        double4_t acc = {0.0, 0.0, 0.0, 0.0};
        for (int64_t grp = g0; grp < g1; ++grp) {
            const int64_t i = grp * 64 + lane;
            const bool active = i < n;
            double x0 = 0.0, x1 = 0.0, x2 = 0.0, inv_den = 0.0;
            if (active) {
                x0 = xs[i]; x1 = xs[n_pad + i]; x2 = xs[2 * n_pad + i];
                const double den = den_in[i];
                inv_den = (den > TREE_EPS) ? 1.0 / den : 0.0;
            }
            // features of this lane's point, feature-major
            if (WEIGHTED) {                          // ... times the point's weight (an inactive lane: 0)
                const double wp = active ? wsrc[i] : 0.0;
                F[w][0][lane] = wp; F[w][1][lane] = wp * x0; F[w][2][lane] = wp * x1; F[w][3][lane] = wp * x2;
                F[w][4][lane] = wp * (x0 * x0); F[w][5][lane] = wp * (x0 * x1); F[w][6][lane] = wp * (x0 * x2);
                F[w][7][lane] = wp * (x1 * x1); F[w][8][lane] = wp * (x1 * x2); F[w][9][lane] = wp * (x2 * x2);
            } else {
            F[w][0][lane] = 1.0; F[w][1][lane] = x0; F[w][2][lane] = x1; F[w][3][lane] = x2;
            F[w][4][lane] = x0 * x0; F[w][5][lane] = x0 * x1; F[w][6][lane] = x0 * x2;
            F[w][7][lane] = x1 * x1; F[w][8][lane] = x1 * x2; F[w][9][lane] = x2 * x2;
            }
#pragma unroll
            for (int f = 10; f < 16; ++f) F[w][f][lane] = 0.0;
#pragma unroll
            for (int cc = 0; cc < 16; ++cc) {
                const double* pr = prep + PREP_N * (tile + cc);     // wave-uniform
                const double wE = pr[9];
                double gam = 0.0;
                if (wE != 0.0) {
                    const double d0 = x0 - pr[6], d1 = x1 - pr[7], d2 = x2 - pr[8];
                    const double q = sym3_quad(pr[0], pr[1], pr[2], pr[3], pr[4], pr[5], d0, d1, d2);
                    if (__any(q < 1500.0)) gam = wE * exp(-0.5 * q) * inv_den;
                    // reference: gamma = g / den (C:176); accumulate() drops gamma < eps (C:100)
                    if (gam < TREE_EPS || !active) gam = 0.0;
                }
                G[w][cc][lane] = gam;
            }
            __builtin_amdgcn_s_waitcnt(0xc07f);      // lgkmcnt(0): this wave's LDS writes landed
            __builtin_amdgcn_wave_barrier();
            // 16 MFMAs: D[comp][feat] += sum over the 4 points of sub-group s
#pragma unroll
            for (int s = 0; s < 16; ++s) {
                const double a = G[w][a_idx][4 * s + b_idx];
                const double b = F[w][a_idx][4 * s + b_idx];
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
            }
            __builtin_amdgcn_wave_barrier();
        }
        // D layout (f64 16x16x4): row (component) = (lane >> 4) + 4 r, col (feature) = lane & 15
#pragma unroll
        for (int r = 0; r < 4; ++r) red[w][b_idx + 4 * r][a_idx] = acc[r];
        __syncthreads();
        // fixed-order combination of the workgroup's waves, one partial per workgroup
        for (int e = threadIdx.x; e < 16 * NMOM; e += FULL_BLOCK) {
            const int comp = e / NMOM, feat = e % NMOM;
            double t = 0.0;
#pragma unroll
            for (int ww = 0; ww < FULL_WAVES; ++ww) t += red[ww][comp][feat];
            partials[((size_t)blockIdx.x * J16 + tile + comp) * NMOM + feat] = t;
        }
        __syncthreads();
    }
#elif FULLCOV_BODY == 3
// WEIGHTED: the tile's weights are staged with its coordinates (0 past the cloud's end); phase B converts w_p to float32 once
// and writes the feature row about the centroid as w_p f, and the point's log term is multiplied by w_p in float64.  The origin
// stays the UNWEIGHTED centroid: it is a reference point only, and the move back in full_reduce_f32_kernel holds for any o
// because it uses the (weighted) m0.
    extern __shared__ double lds_raw[];
    if (done && *done) return;
    const bool use_chol = !(flags && (*flags & 1));        // kernel-uniform: some Sigma^-1 failed its factorisation -> symmetric form
    long long tA = 0, tB = 0, tC = 0, tW = 0, tm = 0;
#define FF_TICK(acc) do { if (dbg) { const long long now_ = clock64(); acc += now_ - tm; tm = now_; } } while (0)
    const int LD = ff_ld(J16);
    double* TOT = lds_raw;                                  // [2][FF_P] row sums over the components with pi >= eps (-1: dead point)
    double* WX = TOT + 2 * FF_P + 2;                        // (WEIGHTED) [2][FF_P] the tile's weights, double-buffered like XH
    double* WT = WX + 2 * FF_P;                             // (WEIGHTED) [2][FF_P] ... by tile parity like TOT, for its log terms
    float* G = reinterpret_cast<float*>(TOT + 2 * FF_P + 2 + (WEIGHTED ? 4 * FF_P : 0));      // [FF_P][LD]
    float* F = G + (size_t)FF_P * LD;                       // [FF_P points][16 features]
    float* INV = F + 16 * FF_P;                             // [FF_P] 1 / denominator (0: dead point)
    float* WL = INV + FF_P;                                 // [J16] 1 where pi_j >= eps
    f2t* XH = reinterpret_cast<f2t*>(WL + J16);             // [2][3][FF_P] {v, v}: head of x - o, double-buffered
    f2t* XT = XH + 2 * 3 * FF_P;                            // ... and its tail
    const int w = wave_in_block(), lane = lane_id();
    const int tid = (int)threadIdx.x;
    const int npair = J16 / 2;
    const bool mine = tid < npair;
    // the origin: wave 0 adds the partial sums up, everybody reads the three numbers from LDS (TOT's row 0 is not used
    // before the first tile's phase B, two barriers from here)
    if (tid < 64) {
        const double inv_n = 1.0 / (double)n;
        const double c0 = ff_origin(origin_parts, 0, inv_n), c1 = ff_origin(origin_parts, 1, inv_n), c2 = ff_origin(origin_parts, 2, inv_n);
        if (tid == 0) { TOT[0] = c0; TOT[1] = c1; TOT[2] = c2; }
    }
    __syncthreads();
    const double o0 = TOT[0], o1 = TOT[1], o2 = TOT[2];
    __syncthreads();
    // this lane's two components 2 tid, 2 tid + 1
    f2t r00 = {0.f, 0.f}, r01 = r00, r02 = r00, r11 = r00, r12 = r00, r22 = r00, nh0 = r00, nh1 = r00, nh2 = r00, nt0 = r00,
        nt1 = r00, nt2 = r00, we = r00;
    if (mine) {
        float v[2][13];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const double* pr = prep + PREP_N * (2 * tid + c);
            // triangular form: sqrt(log2 e) R;  symmetric form: (log2 e / 2) Sigma^-1
            const double S = use_chol ? LLF_SQRT_LOG2E : 0.5 * LLF_LOG2E;
            const int fo = use_chol ? PREP_R : 0;
            const double u0 = pr[6] - o0, u1 = pr[7] - o1, u2 = pr[8] - o2;
            v[c][0] = llf_f32(S * pr[fo]); v[c][1] = llf_f32(S * pr[fo + 1]); v[c][2] = llf_f32(S * pr[fo + 2]);
            v[c][3] = llf_f32(S * pr[fo + 3]); v[c][4] = llf_f32(S * pr[fo + 4]); v[c][5] = llf_f32(S * pr[fo + 5]);
            const float h0 = (float)u0, h1 = (float)u1, h2 = (float)u2;
            v[c][6] = -h0; v[c][7] = -h1; v[c][8] = -h2;
            v[c][9] = -(float)(u0 - (double)h0); v[c][10] = -(float)(u1 - (double)h1); v[c][11] = -(float)(u2 - (double)h2);
            v[c][12] = (float)pr[9];
        }
        r00 = f2t{v[0][0], v[1][0]}; r01 = f2t{v[0][1], v[1][1]}; r02 = f2t{v[0][2], v[1][2]};
        r11 = f2t{v[0][3], v[1][3]}; r12 = f2t{v[0][4], v[1][4]}; r22 = f2t{v[0][5], v[1][5]};
        nh0 = f2t{v[0][6], v[1][6]}; nh1 = f2t{v[0][7], v[1][7]}; nh2 = f2t{v[0][8], v[1][8]};
        nt0 = f2t{v[0][9], v[1][9]}; nt1 = f2t{v[0][10], v[1][10]}; nt2 = f2t{v[0][11], v[1][11]};
        we = f2t{v[0][12], v[1][12]};
    }
    int my_small = 0;
    for (int j = tid; j < J16; j += FF_BLOCK) {
        const double wl = prep[PREP_N * j + 10], wev = prep[PREP_N * j + 9];
        WL[j] = (wl != 0.0) ? 1.f : 0.f;
        if (wl == 0.0 && wev != 0.0) my_small = 1;
    }
    for (int e = tid; e < FF_P * LD; e += FF_BLOCK) G[e] = 0.f;
    const bool any_small = __syncthreads_or(my_small) != 0;
    const int ntiles = J16 / 16;
    constexpr int MAXT = (FT_MAX_J16 / 16 + FF_WAVES - 1) / FF_WAVES;      // 8
    f4t acc[MAXT];
#pragma unroll
    for (int t = 0; t < MAXT; ++t) acc[t] = f4t{0.f, 0.f, 0.f, 0.f};
    const int a_idx = lane & 15, b_idx = lane >> 4;

    const int64_t tiles = (n + FF_P - 1) / FF_P;
    const int64_t per = (int64_t)segs_per_wg * FF_SEG;
    const int64_t t0 = (int64_t)blockIdx.x * per;
    const int64_t t1 = (t0 + per < tiles) ? t0 + per : tiles;
    constexpr int LQ_WAVE = 7;                             // (the wave with the fewest components at J = 800)
    double lq = 0.0;
    const int st_d = tid / FF_P, st_p = tid % FF_P;
    const double st_o = st_d == 0 ? o0 : (st_d == 1 ? o1 : o2);
    auto stage = [&](int64_t tile, int buf) {
        if (WEIGHTED) {
            // threads 48..63 bring the points' weights (past the end: 0) by the SAME load instruction as the coordinates
            if (tid < 4 * FF_P) {
                const int64_t i = tile * FF_P + st_p;
                const int64_t ic = i < n ? i : n - 1;
                const bool is_w = st_d == 3;
                const double v = *(is_w ? wsrc + ic : xs + (size_t)st_d * n_pad + ic);
                if (is_w) {
                    WX[buf * FF_P + st_p] = i < n ? v : 0.0;
                } else {
                    const double dv = v - st_o;
                    const float h = (float)dv, tl = (float)(dv - (double)h);
                    XH[(buf * 3 + st_d) * FF_P + st_p] = f2t{h, h};
                    XT[(buf * 3 + st_d) * FF_P + st_p] = f2t{tl, tl};
                }
            }
        } else if (tid < 3 * FF_P) {
            int64_t i = tile * FF_P + st_p;
            i = i < n ? i : n - 1;
            const double dv = xs[(size_t)st_d * n_pad + i] - st_o;
            const float h = (float)dv, tl = (float)(dv - (double)h);
            XH[(buf * 3 + st_d) * FF_P + st_p] = f2t{h, h};
            XT[(buf * 3 + st_d) * FF_P + st_p] = f2t{tl, tl};
        }
    };
    auto tile_loglik = [&](int par) {
        const double tv = (lane < FF_P) ? TOT[par * FF_P + lane] : -1.0;
        double term = (tv >= 0.0) ? log_pos_f64(fmax(tv, TREE_EPS)) : 0.0;
        if (WEIGHTED) term *= (lane < FF_P) ? WT[par * FF_P + lane] : 0.0;
        term = wave_sum_f64(term);
        lq += term;
    };
    auto flush = [&](int64_t seg) {                        // the wave's accumulator tiles -> the segment's float partial
        // (the segment index is made opaque: otherwise the eight tiles' addresses are formed ahead of the tile loop and kept
        //  in registers through it -- 199 registers instead of 86)
        int seg_lo = (int)seg;
        asm volatile("" : "+s"(seg_lo));
        seg = seg_lo;
#pragma unroll
        for (int t = 0; t < MAXT; ++t) {
            const int ct = w + t * FF_WAVES;
            if (ct < ntiles) {
                if (a_idx < NMOM) {
                    // D layout (f32 16x16x4): row (component) = 4 (lane >> 4) + r, column (feature) = lane & 15
                    float* dst = partials + ((size_t)seg * J16 + 16 * ct + 4 * b_idx) * NMOM + a_idx;
                    dst[0] = acc[t].x; dst[NMOM] = acc[t].y; dst[2 * NMOM] = acc[t].z; dst[3 * NMOM] = acc[t].w;
                }
                acc[t] = f4t{0.f, 0.f, 0.f, 0.f};
            }
        }
    };
    if (t0 < t1) stage(t0, 0);
    __syncthreads();
    for (int64_t seg0 = t0; seg0 < t1; seg0 += FF_SEG) {
    const int64_t seg1 = (seg0 + FF_SEG < t1) ? seg0 + FF_SEG : t1;
    for (int64_t tile = seg0; tile < seg1; ++tile) {
        const int64_t base = tile * FF_P;
        const int buf = (int)((tile - t0) & 1);
        if (dbg) tm = clock64();
        if (w == LQ_WAVE && tile > t0) tile_loglik(buf ^ 1);
        // ---- phase A ----------------------------------------------------------------------------------------------
        if (mine) {
            const f2t* xh = XH + buf * 3 * FF_P;
            const f2t* xt = XT + buf * 3 * FF_P;
#pragma unroll 4
            for (int p = 0; p < FF_P; ++p) {
                const f2t d0 = (xh[p] + nh0) + (xt[p] + nt0);
                const f2t d1 = (xh[FF_P + p] + nh1) + (xt[FF_P + p] + nt1);
                const f2t d2 = (xh[2 * FF_P + p] + nh2) + (xt[2 * FF_P + p] + nt2);
                f2t q;
                if (use_chol) {
                    const f2t z0 = llf_fma(r02, d2, llf_fma(r01, d1, r00 * d0));
                    const f2t z1 = llf_fma(r12, d2, r11 * d1);
                    const f2t z2 = r22 * d2;
                    q = llf_fma(z2, z2, llf_fma(z1, z1, z0 * z0));
                } else {
                    const f2t t0 = llf_fma(llf_bc(2.f), llf_fma(r02, d2, r01 * d1), r00 * d0);
                    const f2t t1 = llf_fma(llf_bc(2.f), r12 * d2, r11 * d1);
                    q = llf_fma(d2, r22 * d2, llf_fma(d1, t1, d0 * t0));
                }
                const f2t e = f2t{__builtin_amdgcn_exp2f(-q.x), __builtin_amdgcn_exp2f(-q.y)};
                *reinterpret_cast<f2t*>(G + (size_t)p * LD + 2 * tid) = we * e;
            }
        }
        if (tile + 1 < t1) stage(tile + 1, buf ^ 1);
        FF_TICK(tA);
        __syncthreads();
        FF_TICK(tW);
        // ---- phase B: wave w owns points 2 w, 2 w + 1 (one per half-wave) ---------------------------------------------
        {
            const int h = lane >> 5, sub = lane & 31;
            const int p = w * 2 + h;
            const float* Gp = G + (size_t)p * LD;
            const int J128 = (J16 + 127) & ~127;                       // (the row is zero beyond J16: LD >= J16 + 16 ... see below)
            double den = 0.0, tot = 0.0;
            float best = -1.f;
            int jbest = 0;
            for (int jb = 0; jb < J128; jb += 128) {
                const int j = jb + 4 * sub;
                f4t gv = f4t{0.f, 0.f, 0.f, 0.f};
                if (j < J16) gv = *reinterpret_cast<const f4t*>(Gp + j);
                const float m4 = fmaxf(fmaxf(gv.x, gv.y), fmaxf(gv.z, gv.w));
                den += (double)((gv.x + gv.y) + (gv.z + gv.w));
                jbest = (m4 > best) ? j : jbest;
                best = fmaxf(best, m4);
                if (any_small && j < J16) {
                    const f4t wl = *reinterpret_cast<const f4t*>(WL + j);
                    tot += (double)((gv.x * wl.x + gv.y * wl.y) + (gv.z * wl.z + gv.w * wl.w));
                }
            }
            int am;
            {
                const f4t gv = *reinterpret_cast<const f4t*>(Gp + jbest);
                am = jbest + ((gv.x == best) ? 0 : ((gv.y == best) ? 1 : ((gv.z == best) ? 2 : 3)));
            }
            double den0, den1, bm0, bm1;
            halfwave_sum_f64(den, den0, den1);
            halfwave_max_f64((double)best, bm0, bm1);
            const double den_h = h ? den1 : den0;
            const float bm_h = (float)(h ? bm1 : bm0);
            int c0, c1;
            halfwave_min_i32((best == bm_h) ? am : 0x7fffffff, c0, c1);
            double tot_h = den_h;
            if (any_small) {
                double t0s, t1s;
                halfwave_sum_f64(tot, t0s, t1s);
                tot_h = h ? t1s : t0s;
            }
            const double inv = 1.0 / den_h;
            if (sub == 0) {
                const bool live = base + p < n;
                const bool good = den_h > TREE_EPS;
                INV[p] = (live && good) ? (float)inv : 0.f;
                TOT[buf * FF_P + p] = live ? tot_h : -1.0;
                if (live) label_out[base + p] = good ? (h ? c1 : c0) : 0;
                if (WEIGHTED) WT[buf * FF_P + p] = WX[buf * FF_P + p];
            }
            if (sub < 16) {
                const f2t* xh = XH + buf * 3 * FF_P;
                const float x0 = xh[p].x, x1 = xh[FF_P + p].x, x2 = xh[2 * FF_P + p].x;
                float f = 0.f;
                switch (sub) {
                    case 0: f = 1.f; break;
                    case 1: f = x0; break;
                    case 2: f = x1; break;
                    case 3: f = x2; break;
                    case 4: f = x0 * x0; break;
                    case 5: f = x0 * x1; break;
                    case 6: f = x0 * x2; break;
                    case 7: f = x1 * x1; break;
                    case 8: f = x1 * x2; break;
                    case 9: f = x2 * x2; break;
                    default: f = 0.f;
                }
                if (WEIGHTED) f *= (float)WX[buf * FF_P + p];
                F[p * 16 + sub] = f;
            }
        }
        FF_TICK(tB);
        __syncthreads();
        FF_TICK(tW);
        // ---- phase C: v_mfma_f32_16x16x4_f32, A[i][k] in lane i + 16 k, B[k][j] in lane j + 16 k ----------------------
        if (want_stats) {
            float bfrag[4], ifrag[4];
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                ifrag[s] = INV[4 * s + b_idx];
                bfrag[s] = F[(4 * s + b_idx) * 16 + a_idx];
            }
            // (the next tile's four A values are requested before the current tile's are consumed; the fences keep the
            //  compiler from requesting ALL tiles' values at once -- 168 registers instead of 84 for the rest of the kernel)
            float araw[2][4];
            const int row_off = b_idx * LD + a_idx, srow = 4 * LD;
            auto load_a = [&](int ct, float (&dst)[4]) {
                // (the tile's offset is made opaque: left alone the compiler forms all 28 addresses ahead of the loop, spills
                //  them and reloads four per tile from scratch)
                int off = row_off + 16 * ct;
                asm volatile("" : "+v"(off));
#pragma unroll
                for (int s = 0; s < 4; ++s) dst[s] = G[off + s * srow];
            };
            if (w < ntiles) load_a(w, araw[0]);
#pragma unroll
            for (int t = 0; t < MAXT; ++t) {
                const int ct = w + t * FF_WAVES;                       // wave-uniform
                if (ct < ntiles) {
                    if (t + 1 < MAXT && ct + FF_WAVES < ntiles) load_a(ct + FF_WAVES, araw[(t + 1) & 1]);
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        float a = araw[t & 1][s] * ifrag[s];
                        if (a < 1.0e-15f) a = 0.f;                     // accumulate() drops gamma < eps (C:100)
                        acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bfrag[s], acc[t], 0, 0, 0);
                    }
                    asm volatile("" ::: "memory");
                }
            }
        }
        FF_TICK(tC);
        __syncthreads();                                               // G is overwritten by the next tile
        FF_TICK(tW);
    }
    if (want_stats) flush((int64_t)blockIdx.x * segs_per_wg + (seg0 - t0) / FF_SEG);
    }
    if (w == LQ_WAVE && t0 < t1) tile_loglik((int)((t1 - 1 - t0) & 1));
    if (dbg && lane == 0 && blockIdx.x == 7) {
        dbg[w * 4 + 0] = tA; dbg[w * 4 + 1] = tB; dbg[w * 4 + 2] = tC; dbg[w * 4 + 3] = tW;
    }
    if (w == LQ_WAVE && lane == 0) block_q[blockIdx.x] = lq;
#undef FF_TICK
#else
#error "FULLCOV_BODY must be 1, 2 or 3"
#endif
