// The body of the fused E+M kernel (flat_kernels.hip), stated ONCE and included TEXTUALLY by the kernel of one cloud
// (flat_fused_pk_kernel) and by the batched kernels (flat_fused_pk_batch_kernel<NSLOT> there, <NSLOT, true> in
// flat_batch_weighted.hip; what the text names beyond the kernel's own: flat_fused_device.h).  Not a header: no include
// guard, included inside a kernel's braces.  The including kernel provides
//   NSLOT, WEIGHTED                 compile-time constants
//   X, pack, n, J, Jpad, partials, lpn_partials, allow_const_shift, comp_major, SW     what the serial kernel's arguments are
//   FLAT_FUSED_BLOCK                the workgroup's number among those that share the cloud X [n]
//   FLAT_FUSED_ROW_RANGE(n, r0, nrows)   the wave's rows among them (wave_row_range_uniform)
// -- the three places where the serial kernel reads blockIdx.x / gridDim.x: the wave's rows, the partial block's address and
// the index of the log-normaliser partial.
// (Why text and not a __forceinline__ device function: inlined, the same statements compiled to a different instruction
//  order in 30 of the 32 serial instantiations -- equal counts, commuted operands and a re-scheduled epilogue -- and the
//  serial kernels are to stay the code they were, instruction for instruction; profiles/flat_batch.md.)
    constexpr int K = NSLOT;
    constexpr int KP = K / 2;          // full pairs
    constexpr bool ODD = (K & 1) != 0; // one trailing single component
    const int lane = lane_id();
    f2 mu0[KP + 1], mu1[KP + 1], mu2[KP + 1], g0[KP + 1], g1[KP + 1], g2[KP + 1], cc[KP + 1];
    f2 s0[KP + 1], a0[KP + 1], a1[KP + 1], a2[KP + 1], b0[KP + 1], b1[KP + 1], b2[KP + 1];
    float mu0s = 0.f, mu1s = 0.f, mu2s = 0.f, g0s = 0.f, g1s = 0.f, g2s = 0.f, cs = NEG_INF;
    float s0s = 0.f, a0s = 0.f, a1s = 0.f, a2s = 0.f, b0s = 0.f, b1s = 0.f, b2s = 0.f;
#pragma unroll
    for (int p = 0; p < KP; ++p) {
        const int ja = (2 * p) * 64 + lane, jb = (2 * p + 1) * 64 + lane;
        mu0[p] = f2{pack[(PK_MU + 0) * Jpad + ja], pack[(PK_MU + 0) * Jpad + jb]};
        mu1[p] = f2{pack[(PK_MU + 1) * Jpad + ja], pack[(PK_MU + 1) * Jpad + jb]};
        mu2[p] = f2{pack[(PK_MU + 2) * Jpad + ja], pack[(PK_MU + 2) * Jpad + jb]};
        g0[p] = f2{pack[(PK_G + 0) * Jpad + ja], pack[(PK_G + 0) * Jpad + jb]};
        g1[p] = f2{pack[(PK_G + 1) * Jpad + ja], pack[(PK_G + 1) * Jpad + jb]};
        g2[p] = f2{pack[(PK_G + 2) * Jpad + ja], pack[(PK_G + 2) * Jpad + jb]};
        cc[p] = f2{pack[PK_C * Jpad + ja], pack[PK_C * Jpad + jb]};
        s0[p] = a0[p] = a1[p] = a2[p] = b0[p] = b1[p] = b2[p] = f2{0.f, 0.f};
    }
    if (ODD) {
        const int j = (K - 1) * 64 + lane;
        mu0s = pack[(PK_MU + 0) * Jpad + j]; mu1s = pack[(PK_MU + 1) * Jpad + j]; mu2s = pack[(PK_MU + 2) * Jpad + j];
        g0s = pack[(PK_G + 0) * Jpad + j]; g1s = pack[(PK_G + 1) * Jpad + j]; g2s = pack[(PK_G + 2) * Jpad + j];
        cs = pack[PK_C * Jpad + j];
    }

    // largest constant of the table = upper bound of every wl2 (identical in every wave)
    // (m0 and the origin below are derived by EVERY wave, from the table it has just loaded, and not once by the kernel
    //  that writes the table: flat_finalize_kernel, flat_boundary_kernel, flat_finalize_mb_kernel and flat_pack_kernel
    //  all write it from several workgroups, so one wave could only derive them behind a cross-workgroup hand-off --
    //  a ticket and agent-scope fences, microseconds on the latency chain between two iterations -- or in one more
    //  launch, against ~130 vector instructions per wave here, less than one of its ~1000 rows)
    float m0 = cs;
#pragma unroll
    for (int p = 0; p < KP; ++p) m0 = fmaxf(m0, fmaxf(cc[p].x, cc[p].y));
    m0 = wave_max_dpp(m0);
    // (false for NaN as well; below -64 the row-maximum loop's "tiny" rule applies, see lpn2_from)
    const bool small_shift = allow_const_shift && m0 <= CS_MAX_SHIFT && m0 >= -64.0f;

    // row range and loop control in scalar registers (wave_row_range_uniform)
    int64_t r0;
    int nrows;
    FLAT_FUSED_ROW_RANGE(n, r0, nrows);
    const float* const xw = X + 3 * r0;
    double lsum = 0.0;
    // First moments are summed about ONE origin for all components and moved to the component's mean when the wave is
    // done:  sum r (x - mu) = sum r (x - o) - (mu - o) sum r.  The row's x - o is a wave-uniform operand, so the update
    // is one packed FMA per axis -- and the squares (x - mu)^2 the quadratic form needs anyway are what the second
    // moments need: the per-component differences themselves do not have to survive the row's reduction.  18 instead of
    // 21 packed instructions per pair of components (round 4: 0.374 -> 0.33 ms at C3).  The origin is the weighted mean
    // of the component means (every wave derives the same one from the table) -- inside the model whatever the
    // coordinates' offset and whatever outliers the cloud has.  The price: a first moment's
    // rounding error is relative to the MODEL's extent instead of the component's, 2^-24 |x - o| per addition -- the
    // reference's own float32 resp.T @ X has it relative to |x| (tests: test_fit_far_from_the_origin,
    // test_train_far_points_and_mixed_scales).
    // ... WEIGHTED by the mixing weights (table row PK_W; 0 for padding, dead and non-finite components): a component
    // that has lost its points sits wherever its last M-step left it -- at the coordinate origin, which for a cloud in
    // map coordinates is kilometres outside the model -- and must not pull the common origin (and with it every
    // component's rounding error) towards itself.
    float o0 = 0.f, o1 = 0.f, o2 = 0.f, ow = 0.f;
#pragma unroll
    for (int p = 0; p < KP; ++p) {
        const float wa = pack[PK_W * Jpad + (2 * p) * 64 + lane], wb = pack[PK_W * Jpad + (2 * p + 1) * 64 + lane];
        o0 = fmaf(wa, mu0[p].x, fmaf(wb, mu0[p].y, o0));
        o1 = fmaf(wa, mu1[p].x, fmaf(wb, mu1[p].y, o1));
        o2 = fmaf(wa, mu2[p].x, fmaf(wb, mu2[p].y, o2));
        ow += wa + wb;
    }
    if (ODD) {
        const float ws = pack[PK_W * Jpad + (K - 1) * 64 + lane];
        o0 = fmaf(ws, mu0s, o0); o1 = fmaf(ws, mu1s, o1); o2 = fmaf(ws, mu2s, o2);
        ow += ws;
    }
    {
        ow = wave_sum_dpp(ow);
        const float inv_w = ow > 0.f ? 1.0f / ow : 0.f;      // (no usable component at all: the coordinate origin)
        o0 = wave_sum_dpp(o0) * inv_w; o1 = wave_sum_dpp(o1) * inv_w; o2 = wave_sum_dpp(o2) * inv_w;
        if (!(fabsf(o0) < 3.0e38f)) o0 = 0.f;
        if (!(fabsf(o1) < 3.0e38f)) o1 = 0.f;
        if (!(fabsf(o2) < 3.0e38f)) o2 = 0.f;
    }
    // the row loop exists twice in this kernel, once per log-sum-exp variant; the choice is uniform
    // over the whole grid (every wave derives the same m0 from the table)
    auto rows = [&](auto cs_tag) {
    constexpr bool CS = decltype(cs_tag)::value;
    if (CS) {
        const f2 M0 = f2{m0, m0};
#pragma unroll
        for (int p = 0; p < KP; ++p) cc[p] = cc[p] - M0;
        cs -= m0;
    }
    const float eps_scale = __builtin_amdgcn_exp2f(-m0);
    // FLAT_EPS in a vector register: the denominator's FMA below then reads the row's sum straight from the scalar
    // register the wave reduction left it in (one v_fma_f32; an inline literal would need the sum copied to a VGPR first)
    float eps_v = FLAT_EPS;
    asm volatile("" : "+v"(eps_v));
    float lacc = 0.f;                      // sum of log2(den) of the rows since the last flush
    double swsum = 0.0;                    // (WEIGHTED) sum of the weights of this wave's rows
    // One row's E and M phase: everything a row does but fetch its coordinates and flush lacc, which belong to the loops below.
    auto row_em = [&](const float x0, const float x1, const float x2, const float sw) __attribute__((always_inline)) {
        // (WEIGHTED) a row of weight zero is absent, whatever its coordinates: a wave-uniform branch round the row's work
        if (!WEIGHTED || !weight_is_zero(sw)) {
            const f2 X0 = f2{x0, x0}, X1 = f2{x1, x1}, X2 = f2{x2, x2};
            const float xo0 = x0 - o0, xo1 = x1 - o1, xo2 = x2 - o2;
            const f2 XO0 = f2{xo0, xo0}, XO1 = f2{xo1, xo1}, XO2 = f2{xo2, xo2};

            f2 wl[KP + 1];
            f2 q0[KP + 1], q1[KP + 1], q2[KP + 1];
            float q0s = 0.f, q1s = 0.f, q2s = 0.f;
            float wls = NEG_INF;
            float m = NEG_INF;
            f2 sacc = f2{0.f, 0.f};
#pragma unroll
            for (int p = 0; p < KP; ++p) {
                const f2 d0 = X0 - mu0[p], d1 = X1 - mu1[p], d2 = X2 - mu2[p];
                q0[p] = d0 * d0; q1[p] = d1 * d1; q2[p] = d2 * d2;
                f2 a = cc[p] - g0[p] * q0[p];
                a = a - g1[p] * q1[p];
                a = a - g2[p] * q2[p];
                if (CS) {
                    wl[p] = f2{__builtin_amdgcn_exp2f(a.x), __builtin_amdgcn_exp2f(a.y)};
                    // (the first pair starts the sum: 0 + 2^a is 2^a bit for bit -- an exponential is never -0 --
                    //  and one packed addition fewer)
                    sacc = p == 0 ? wl[p] : sacc + wl[p];
                } else {
                    wl[p] = a;
                    m = fmaxf(m, fmaxf(a.x, a.y));
                }
            }
            if (ODD) {
                const float d0 = x0 - mu0s, d1 = x1 - mu1s, d2 = x2 - mu2s;
                q0s = d0 * d0; q1s = d1 * d1; q2s = d2 * d2;
                float a = fmaf(-g0s, q0s, cs);
                a = fmaf(-g1s, q1s, a);
                a = fmaf(-g2s, q2s, a);
                wls = CS ? __builtin_amdgcn_exp2f(a) : a;
                m = fmaxf(m, a);
            }
            if (CS) {
                m = m0;
            } else {
                m = wave_max_dpp(m);
                if (m == NEG_INF) m = 0.f;
                const f2 M = f2{m, m};
#pragma unroll
                for (int p = 0; p < KP; ++p) {
                    const f2 t = wl[p] - M;
                    wl[p] = f2{__builtin_amdgcn_exp2f(t.x), __builtin_amdgcn_exp2f(t.y)};
                    sacc = p == 0 ? wl[p] : sacc + wl[p];
                }
                if (ODD) wls = __builtin_amdgcn_exp2f(wls - m);
            }
            float s = sacc.x + sacc.y;
            if (ODD) s += wls;
            s = wave_sum_dpp(s);
            float inv_den;
            if (CS) {
                // lpn2_from with m = m0 in [-64, CS_MAX_SHIFT]: no "tiny" case, eps 2^-m0 is loop-invariant;
                // the log-normalisers are summed in float32 over 8 rows before they join the float64 total
                const float den = fmaf(eps_v, eps_scale, s);
                inv_den = __builtin_amdgcn_rcpf(den);
                if constexpr (WEIGHTED) lacc = fmaf(sw, __builtin_amdgcn_logf(den), lacc);
                else lacc += __builtin_amdgcn_logf(den);
            } else {
                const float lpn2 = lpn2_from(m, s, inv_den);
                if constexpr (WEIGHTED) lsum += (double)sw * (double)(lpn2 * LN2);
                else lsum += (double)(lpn2 * LN2);
            }
            if constexpr (WEIGHTED) inv_den *= sw;
            const f2 INV = f2{inv_den, inv_den};
#pragma unroll
            for (int p = 0; p < KP; ++p) {
                const f2 rr = wl[p] * INV;
                s0[p] += rr;
                a0[p] += rr * XO0; a1[p] += rr * XO1; a2[p] += rr * XO2;
                b0[p] += rr * q0[p]; b1[p] += rr * q1[p]; b2[p] += rr * q2[p];
            }
            if (ODD) {
                const float rr = wls * inv_den;
                // (unweighted: spelt as the fused multiply-add the compiler makes of s0 += rr everywhere else in this loop --
                //  left to it, this one addition can be paired with lacc's instead, and the sum is then rounded twice.
                //  Weighted, lacc's update is a fused multiply-add itself: spelt alike the two are paired into one packed
                //  instruction whose operands cost <13, true> its 256th register and its second wave per SIMD.)
                if constexpr (WEIGHTED) s0s += rr;
                else s0s = fmaf(wls, inv_den, s0s);
                a0s = fmaf(rr, xo0, a0s); a1s = fmaf(rr, xo1, a1s); a2s = fmaf(rr, xo2, a2s);
                b0s = fmaf(rr, q0s, b0s); b1s = fmaf(rr, q1s, b1s); b2s = fmaf(rr, q2s, b2s);
            }
        }
    };
    // The constant-shift loop runs FUSED_TRIP rows per trip, straight-line: a full trip has no prefetch clamp, no exit test
    // and no flush test per row -- one compare and one branch per trip, and the float64 flush of lacc at its end.  The wave
    // counts its rows from zero and a trip starts at a multiple of FUSED_TRIP, so the flush falls after the rows with
    // (row & 7) == 7, the same eight rows per float32 sum as when every row tested for it; rows, operations and operands are
    // in the order they were.
    // The coordinates (and weights) arrive by wide scalar loads, half a trip at a time, into the registers of the half
    // consumed before: the second half of this trip is fetched behind the first row of the first half, the first half of
    // the next trip behind the first row of the second (this trip's again when no full trip follows: the address stays
    // inside the wave's rows).  Scalar loads return out of order, so a wait is a wait for all of them: a fetch issued before
    // the half in flight is first read would be waited for at once.  The three rows between a fetch and its first use are
    // what the trip is for: with the same trip fetching one row ahead, as the one-row loop does, the kernel is as fast as
    // it was without trips (N = 1e6, J = 800: 3137 against 3129 it/s), with them 3274 (profiles/fused_row_trip.md).
    // What keeps a row's instructions between its neighbours': the empty asm statements -- a row's coordinates exist from
    // its first statement on, the odd slot's sums are complete at its last -- and the scheduling barrier.  Without them the
    // vectoriser pairs the odd slot's scalar operations of one row with the next row's and the scheduler interleaves rows,
    // and both keep the values in between in registers the kernel does not have (<13, false>: 256 + 85 and scratch).
    // (NSLOT > 13 keeps one row per trip: those kernels run one wave per SIMD with part of their sums in AGPRs, and the
    //  straight-line trip's allocation spilt to scratch at NSLOT = 15 and 16)
    constexpr int TRIP = NSLOT <= 13 ? FUSED_TRIP : 1;
    int row = 0;                                            // (row: counted from the wave's first one)
    if constexpr (CS && TRIP > 1) {
        constexpr int HALF = TRIP > 1 ? TRIP / 2 : 1;       // (TRIP == 1: this block is discarded, but it is still parsed)
        static_assert(8 % TRIP == 0, "a flush every eight rows falls at the end of a trip");
        if (nrows >= TRIP) {
            float xa[3 * HALF], xb[3 * HALF], wa[HALF], wb[HALF];
            // HALF rows from `have`; behind the first of them, the fetch of the HALF rows from row `next` into `into`
            auto half_trip = [&](const float (&have)[3 * HALF], const float (&whave)[HALF], float (&into)[3 * HALF],
                                 float (&winto)[HALF], const int next) __attribute__((always_inline)) {
#pragma unroll
                for (int t = 0; t < HALF; ++t) {
                    float c0 = have[3 * t], c1 = have[3 * t + 1], c2 = have[3 * t + 2];
                    asm volatile("" : "+s"(c0), "+s"(c1), "+s"(c2));
                    row_em(c0, c1, c2, whave[t]);
                    if (ODD) asm volatile("" : : "v"(s0s), "v"(a0s), "v"(a1s), "v"(a2s), "v"(b0s), "v"(b1s), "v"(b2s));
                    __builtin_amdgcn_sched_barrier(0);
                    if (t == 0) {
                        const float* xn = xw + 3 * (int64_t)next;
#pragma unroll
                        for (int i = 0; i < 3 * HALF; ++i) into[i] = xn[i];
                        if constexpr (WEIGHTED) {
#pragma unroll
                            for (int i = 0; i < HALF; ++i) winto[i] = SW[r0 + next + i];
                        }
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
            };
#pragma unroll
            for (int i = 0; i < 3 * HALF; ++i) xa[i] = xw[i];
#pragma unroll
            for (int i = 0; i < HALF; ++i) wa[i] = wb[i] = 1.f;
            if constexpr (WEIGHTED) {
#pragma unroll
                for (int i = 0; i < HALF; ++i) wa[i] = SW[r0 + i];
            }
            for (; nrows - row >= TRIP; row += TRIP) {
                half_trip(xa, wa, xb, wb, row + HALF);
                half_trip(xb, wb, xa, wa, nrows - row >= 2 * TRIP ? row + TRIP : row);
                if (TRIP == 8 || ((row + TRIP) & 7) == 0) {
                    lsum += (double)lacc;
                    lacc = 0.f;
                }
            }
        }
    }
    // the last nrows % TRIP rows, and every row of the row-maximum variant: one row per trip, the next row's
    // coordinates prefetched behind a clamp
    float x0 = 0.f, x1 = 0.f, x2 = 0.f;
    float sw = 1.f;                        // (WEIGHTED) this row's weight
    if (row < nrows) {
        const float* xr = xw + 3 * (int64_t)row;
        x0 = xr[0]; x1 = xr[1]; x2 = xr[2];
        if (WEIGHTED) sw = SW[r0 + row];
    }
    for (; row < nrows; ++row) {
        const int nrow = (row + 1 < nrows) ? row + 1 : row;
        const float* xn = xw + 3 * (int64_t)nrow;
        const float nx0 = xn[0], nx1 = xn[1], nx2 = xn[2];
        float nsw = 1.f;
        if constexpr (WEIGHTED) nsw = SW[r0 + nrow];
        row_em(x0, x1, x2, sw);
        // the 8-row flush of lacc, on the rows' schedule whether this one was skipped or not; with eight rows per trip the
        // rows left over start at a multiple of eight and are fewer than eight: none of them is a row 7
        if (CS && TRIP != 8 && (row & 7) == 7) {
            asm volatile("" ::: "memory");                  // keeps this a (wave-uniform) branch, not selects
            lsum += (double)lacc;
            lacc = 0.f;
        }
        x0 = nx0; x1 = nx1; x2 = nx2;
        if constexpr (WEIGHTED) sw = nsw;
    }
    if constexpr (WEIGHTED) {
        // the closing term's sum of the wave's weights, float64, taken here and not in the loop (two registers the loop
        // does not have); zero weights add nothing
        if (CS) {
            for (int64_t i = r0 + lane; i < r0 + nrows; i += 64) swsum += (double)SW[i];
            swsum = wave_sum_f64(swsum);
        }
    }
    if (CS) lsum = (lsum + (double)lacc + (WEIGHTED ? swsum : (double)nrows) * (double)m0) * (double)LN2;
    };
    if (small_shift) rows(std::true_type{});
    else rows(std::false_type{});
    // first moments: from the common origin to the component's mean
    {
        const f2 O0 = f2{o0, o0}, O1 = f2{o1, o1}, O2 = f2{o2, o2};
#pragma unroll
        for (int p = 0; p < KP; ++p) {
            a0[p] -= (mu0[p] - O0) * s0[p]; a1[p] -= (mu1[p] - O1) * s0[p]; a2[p] -= (mu2[p] - O2) * s0[p];
        }
        if (ODD) {
            a0s = fmaf(-(mu0s - o0), s0s, a0s); a1s = fmaf(-(mu1s - o1), s0s, a1s); a2s = fmaf(-(mu2s - o2), s0s, a2s);
        }
    }

    // (a statistic's LDS row is padded by 8 words: the component-major copy below has a wave read 8 components x 8
    //  rows at once, and NSLOT * 64 words apart all rows of a component would share one bank)
    // The four waves' sums meet in the fixed order ((w0 + w1) + w2) + w3 -- what makes a partial reproducible -- over THREE
    // LDS copies of the block: waves 0, 2 and 3 store theirs side by side, wave 1 then adds into wave 0's copy, and the
    // output loop adds the three copies in that order on its way out.  Two barriers where four turns on one copy took
    // four, and the same bits.  (Four copies and one barrier do not fit: 4 x 23.5 KB at NSLOT = 13, twice per CU, is
    // more than the 160 KB; three copies leave every NSLOT the workgroups per CU its registers allow.)
    constexpr int ST = NSLOT * 64, STP = ST + 8, CP = FLAT_NSTAT * STP;
    __shared__ float sh[3 * CP];
    __shared__ double shl[WAVES_PER_BLOCK];
    const int w = wave_in_block();
    if (lane == 0) shl[w] = lsum;
    auto put = [&](float* base, int k, bool first, float v0, float v1, float v2, float v3, float v4, float v5, float v6) {
        float* q = base + k * 64 + lane;
        if (first) { q[0 * STP] = v0; q[1 * STP] = v1; q[2 * STP] = v2; q[3 * STP] = v3; q[4 * STP] = v4; q[5 * STP] = v5; q[6 * STP] = v6; }
        else { q[0 * STP] += v0; q[1 * STP] += v1; q[2 * STP] += v2; q[3 * STP] += v3; q[4 * STP] += v4; q[5 * STP] += v5; q[6 * STP] += v6; }
    };
    auto put_all = [&](float* base, bool first) {
#pragma unroll
        for (int p = 0; p < KP; ++p) {
            put(base, 2 * p, first, s0[p].x, a0[p].x, a1[p].x, a2[p].x, b0[p].x, b1[p].x, b2[p].x);
            put(base, 2 * p + 1, first, s0[p].y, a0[p].y, a1[p].y, a2[p].y, b0[p].y, b1[p].y, b2[p].y);
        }
        if (ODD) put(base, K - 1, first, s0s, a0s, a1s, a2s, b0s, b1s, b2s);
    };
    if (w != 1) put_all(sh + (w == 0 ? 0 : w - 1) * CP, true);
    __syncthreads();
    if (w == 1) put_all(sh, false);
    __syncthreads();
    auto total = [&](int i) { return (sh[i] + sh[CP + i]) + sh[2 * CP + i]; };
    if (comp_major) {
        // [block][Jpad][8]: a component's 7 statistics + one pad word are 32 contiguous bytes, 8 components -- what a
        // workgroup of flat_boundary_kernel owns -- 256 (the train loop without a communicator; kernel-uniform)
        float* outp = partials + (size_t)FLAT_FUSED_BLOCK * FLAT_CM_STRIDE * Jpad;
        for (int idx = threadIdx.x; idx < FLAT_CM_STRIDE * ST; idx += BLOCK) {
            const int j = idx / FLAT_CM_STRIDE, st = idx % FLAT_CM_STRIDE;
            outp[idx] = st < FLAT_NSTAT ? total(st * STP + j) : 0.f;
        }
    } else {
        float* outp = partials + (size_t)FLAT_FUSED_BLOCK * FLAT_NSTAT * Jpad;
        for (int idx = threadIdx.x; idx < FLAT_NSTAT * ST; idx += BLOCK) {
            const int st = idx / ST, j = idx % ST;
            outp[st * Jpad + j] = total(st * STP + j);
        }
    }
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int i = 0; i < WAVES_PER_BLOCK; ++i) t += shl[i];
        lpn_partials[FLAT_FUSED_BLOCK] = t;
    }
