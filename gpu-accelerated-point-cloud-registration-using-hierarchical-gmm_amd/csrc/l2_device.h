// What the kernels of the resident L2 GMMReg cost and of its device solve share (gmmreg_l2_kernels.hip): the launch shape,
// a hypothesis as it travels to the device, and the SERIAL part of the BFGS solve on the device (hgmm_l2_solve) -- the
// quaternion's pose and Jacobian, the chain rule, one transition of the line search / BFGS state machine.
//
// THE ARITHMETIC IS THE CONTRACT.  Everything below is float64 with contraction off and uses + - x / sqrt, comparisons and
// sign changes only, in the order it is written in; tests/_l2_solve_model.py restates it in scalar Python and the device
// has to meet that bit for bit.  The optimiser is SciPy 1.15's BFGS (_optimize.py: _minimize_bfgs) with its first line
// search (_linesearch.py: line_search_wolfe1 / scalar_search_wolfe1 over _dcsrch.py: DCSRCH, dcstep), restated with its
// constants: gtol on the infinity norm; old_old_fval = f0 + |g|_2 / 2; first trial step min(1, 1.01 * 2 (phi0 - old_phi0) /
// derphi0), 1 if that is negative; c1 = 1e-4, c2 = 0.9, xtol = 1e-14, amin = 1e-100, amax = 1e100; at most 100 evaluations
// per line search; the accepted point's gradient is the one the line search evaluated last; rhok = 1000 when yk.sk == 0;
// Hk = A1 (Hk A2) + rhok sk sk^T; its NaN and non-finite-f endings.  Where SciPy's comparisons decide what a NaN does
// (Python's min / max keep their first argument unless the next one compares smaller / larger; np.clip and np.amax
// propagate a NaN), the same comparisons are written out here.
// ONE DELIBERATE DIFFERENCE: when dcsrch fails SciPy tries a second line search (line_search_wolfe2) and only if that
// fails too ends with status 2 at the last accepted iterate; here the solve ends there at once with status 2
// (profiles/l2_device_solve.md: on the multi-start scenario the second search rescued 0 of 25 failures and cost 12-14
// evaluations each time).  nfev therefore differs from SciPy's by design.
// Host and device code: the header compiles without HIP as well (L2_HD empty); tests/test_l2_device_host_cpu.py builds it
// for the host and holds this very text to the Python model bit for bit, without a GPU.
#pragma once

#if defined(__HIPCC__)
#define L2_HD __host__ __device__ inline
#else
#define L2_HD inline
#endif

namespace hgmm {

constexpr int L2_BLOCK = 64;          // source centres per workgroup (one wave)
constexpr int L2_TILE = 128;          // target centres per LDS tile
constexpr int L2_SPLIT = 256;         // target centres per workgroup (two tiles)
constexpr int L2_NOUT = 13;           // (HGMM_L2_NOUT)
constexpr int L2_ROW = 8;             // doubles per tile row: mu (3), phi / z, phi mu / z (3), one pad (16-byte rows)
constexpr unsigned long long L2_MAX_RECORD_BYTES = 1ull << 30;

// one hypothesis as it travels to the device: everything that depends on sigma is worked out once, on the host
struct L2Hyp {
    double rot[9], t[3];
    double neg_h2;                    // -(h h), h = sqrt(2) sigma: the exponent is d2 / neg_h2 (transforms.py: kernel_matrix)
    double z;                         // (2 pi sigma^2)^(3/2)
    double two_s2;                    // 2 sigma^2
    int pair;
    int pad;                          // hgmm_l2_cost: 0.  hgmm_l2_solve: 1 once the hypothesis has left the loop
};
static_assert(sizeof(L2Hyp) == 128, "L2Hyp is 16 words");

inline int l2_blocks(int Js) { return (Js + L2_BLOCK - 1) / L2_BLOCK; }
L2_HD int l2_splits(int Jt) { return (Jt + L2_SPLIT - 1) / L2_SPLIT; }

// ---- the device solve ---------------------------------------------------------------------------------------------------
constexpr int L2_LS_MAX = 100;        // DCSRCH.__call__: maxiter (calls of _iterate per line search, the START call included)
enum L2Task { L2_TASK_FG = 0, L2_TASK_CONV = 1, L2_TASK_WARN = 2, L2_TASK_ERROR = 3 };
enum L2Status { L2_ST_OK = 0, L2_ST_MAXITER = 1, L2_ST_LINESEARCH = 2, L2_ST_NAN = 3 };

// a hypothesis' whole state; it stays on the device from the first launch to the download at the end
struct L2SolveState {
    double x[7], g[7];                // the accepted iterate and its gradient
    double pk[7], xt[7];              // the search direction and the trial point that is being evaluated
    double H[49];                     // the inverse Hessian estimate, row-major
    double f, old_old;                // old_fval, old_old_fval
    double derphi0, gnorm;
    // DCSRCH's attributes
    double stp, finit, ginit, gtest, gx, gy, fx, fy, stx, sty, stmin, stmax, width, width1;
    double gtol;
    int stage, brackt, ls_calls;      // ls_calls: calls of _iterate in this line search so far
    int nit, nfev, status, left, max_iter;
    int started;                      // 0: the evaluation under way is the start point's
    int pad;
};
// copied to the device and back by size, and laid out between L2Hyp [R] and the records' doubles in one buffer
static_assert(sizeof(L2SolveState) == 808 && sizeof(L2SolveState) % sizeof(double) == 0, "L2SolveState is 96 doubles and 10 words");

struct L2Quat {
    double rot[9];                    // so.quaternion_matrix: the pose
    double d[4][9];                   // so.diff_rot_from_quaternion with the reference's quirks: dR/dq_k, row-major
};

// q = (w, x, y, z).  n = |q|^2 summed left to right; pose I + (2 / n) A(q), the identity when n < 4 eps; the Jacobian from
// the same n and A, WITHOUT that rule (n = 0 makes it NaN, as on the host).  `jac` false: d is left alone.
L2_HD void l2_quat_terms(const double* q, bool jac, L2Quat& o) {
#pragma clang fp contract(off)
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    const double n = ((w * w + x * x) + y * y) + z * z;
    const double a[9] = {-(y * y + z * z), x * y - w * z, x * z + w * y,
                         x * y + w * z, -(x * x + z * z), y * z - w * x,
                         x * z - w * y, y * z + w * x, -(x * x + y * y)};
    const double s = 2.0 / n;
    double raw[9];
    for (int i = 0; i < 9; ++i) raw[i] = (i % 4 == 0) ? 1.0 + s * a[i] : s * a[i];
    const bool tiny = n < 4.0 * 2.220446049250313e-16;
    for (int i = 0; i < 9; ++i) o.rot[i] = tiny ? ((i % 4 == 0) ? 1.0 : 0.0) : raw[i];
    if (!jac) return;
    const double zero = 0.0;
    const double da[4][9] = {{zero, -z, y, z, zero, -x, -y, x, zero},
                             {zero, y, z, y, -2.0 * x, -w, z, w, -2.0 * x},
                             {-2.0 * y, x, w, x, zero, z, -w, z, -2.0 * y},
                             {-2.0 * z, -w, x, w, -2.0 * z, y, x, y, zero}};
    const double nn = n * n;
    const double c4 = 4.0 / nn, c2 = 2.0 / nn;
    for (int k = 0; k < 4; ++k)
        for (int i = 0; i < 9; ++i) {
            const double first = s * da[k][i];
            o.d[k][i] = (i % 4 == 0) ? first - (c4 * q[k]) * a[i] : first - (c2 * q[k]) * raw[i];
        }
    o.d[2][8] = ((-4.0 * y) * (x * x + y * y)) / nn;        // (so.py:23-24: the two swapped squared terms)
    o.d[3][8] = ((4.0 * z) * (z * z + w * w)) / nn;
}

// the 7-gradient from the 13 sums (f, sum_i grad_i (3), M = sum_i grad_i (x) x_i row-major) and dR/dq
L2_HD void l2_chain_rule(const double* out, const L2Quat& qt, double* g) {
#pragma clang fp contract(off)
    for (int k = 0; k < 4; ++k) {
        double acc = out[4] * qt.d[k][0];
        for (int i = 1; i < 9; ++i) acc = acc + out[4 + i] * qt.d[k][i];
        g[k] = acc;
    }
    g[4] = out[1]; g[5] = out[2]; g[6] = out[3];
}

L2_HD double l2_abs(double v) { return v < 0.0 ? -v : (v == 0.0 ? 0.0 : v); }       // (|-0| = 0, a NaN stays)
L2_HD bool l2_isnan(double v) { return v != v; }
L2_HD bool l2_isfinite(double v) { return (v - v) == 0.0; }
L2_HD double l2_sign(double v) { return v > 0.0 ? 1.0 : (v < 0.0 ? -1.0 : (v == 0.0 ? 0.0 : v)); }
L2_HD double l2_max3(double a, double b, double c) { double m = a; if (b > m) m = b; if (c > m) m = c; return m; }
L2_HD double l2_clip(double v, double lo, double hi) { if (v < lo) v = lo; if (v > hi) v = hi; return v; }
L2_HD double l2_dot7(const double* a, const double* b) {
#pragma clang fp contract(off)
    double acc = a[0] * b[0];
    for (int i = 1; i < 7; ++i) acc = acc + a[i] * b[i];
    return acc;
}
L2_HD double l2_norm2(const double* a) { return __builtin_sqrt(l2_dot7(a, a)); }
L2_HD double l2_norm_inf(const double* a) {               // np.amax(np.abs(a)): a NaN stays
    double m = l2_abs(a[0]);
    for (int i = 1; i < 7; ++i) {
        const double v = l2_abs(a[i]);
        if (!l2_isnan(m) && !(v <= m)) m = v;
    }
    return m;
}

// _dcsrch.py: dcstep.  -> the new step; the bracket is updated in place
L2_HD double l2_dcstep(double& stx, double& fx, double& dx, double& sty, double& fy, double& dy, double stp, double fp, double dp,
                       int& brackt, double stpmin, double stpmax) {
#pragma clang fp contract(off)
    const double sgnd = l2_sign(dp) * l2_sign(dx);
    double stpf;
    if (fp > fx) {
        const double theta = (3.0 * (fx - fp)) / (stp - stx) + dx + dp;
        const double s = l2_max3(l2_abs(theta), l2_abs(dx), l2_abs(dp));
        const double ts = theta / s;
        double gamma = s * __builtin_sqrt(ts * ts - (dx / s) * (dp / s));
        if (stp < stx) gamma = -gamma;
        const double p = (gamma - dx) + theta;
        const double q = ((gamma - dx) + gamma) + dp;
        const double r = p / q;
        const double stpc = stx + r * (stp - stx);
        const double stpq = stx + ((dx / ((fx - fp) / (stp - stx) + dx)) / 2.0) * (stp - stx);
        if (l2_abs(stpc - stx) <= l2_abs(stpq - stx)) stpf = stpc;
        else stpf = stpc + (stpq - stpc) / 2.0;
        brackt = 1;
    } else if (sgnd < 0.0) {
        const double theta = (3.0 * (fx - fp)) / (stp - stx) + dx + dp;
        const double s = l2_max3(l2_abs(theta), l2_abs(dx), l2_abs(dp));
        const double ts = theta / s;
        double gamma = s * __builtin_sqrt(ts * ts - (dx / s) * (dp / s));
        if (stp > stx) gamma = -gamma;
        const double p = (gamma - dp) + theta;
        const double q = ((gamma - dp) + gamma) + dx;
        const double r = p / q;
        const double stpc = stp + r * (stx - stp);
        const double stpq = stp + (dp / (dp - dx)) * (stx - stp);
        if (l2_abs(stpc - stp) > l2_abs(stpq - stp)) stpf = stpc;
        else stpf = stpq;
        brackt = 1;
    } else if (l2_abs(dp) < l2_abs(dx)) {
        const double theta = (3.0 * (fx - fp)) / (stp - stx) + dx + dp;
        const double s = l2_max3(l2_abs(theta), l2_abs(dx), l2_abs(dp));
        const double ts = theta / s;
        const double under = ts * ts - (dx / s) * (dp / s);
        double gamma = s * __builtin_sqrt(under > 0.0 ? under : 0.0);
        if (stp > stx) gamma = -gamma;
        const double p = (gamma - dp) + theta;
        const double q = (gamma + (dx - dp)) + gamma;
        const double r = p / q;
        double stpc;
        if (r < 0.0 && gamma != 0.0) stpc = stp + r * (stx - stp);
        else if (stp > stx) stpc = stpmax;
        else stpc = stpmin;
        const double stpq = stp + (dp / (dp - dx)) * (stx - stp);
        if (brackt) {
            if (l2_abs(stpc - stp) < l2_abs(stpq - stp)) stpf = stpc;
            else stpf = stpq;
            const double lim = stp + 0.66 * (sty - stp);
            if (stp > stx) { if (stpf < lim) {} else stpf = lim; }          // min(lim, stpf): lim unless stpf < lim
            else { if (stpf > lim) {} else stpf = lim; }                    // max(lim, stpf)
        } else {
            if (l2_abs(stpc - stp) > l2_abs(stpq - stp)) stpf = stpc;
            else stpf = stpq;
            stpf = l2_clip(stpf, stpmin, stpmax);
        }
    } else {
        if (brackt) {
            const double theta = (3.0 * (fp - fy)) / (sty - stp) + dy + dp;
            const double s = l2_max3(l2_abs(theta), l2_abs(dy), l2_abs(dp));
            const double ts = theta / s;
            double gamma = s * __builtin_sqrt(ts * ts - (dy / s) * (dp / s));
            if (stp > sty) gamma = -gamma;
            const double p = (gamma - dp) + theta;
            const double q = ((gamma - dp) + gamma) + dy;
            const double r = p / q;
            stpf = stp + r * (sty - stp);
        } else if (stp > stx) stpf = stpmax;
        else stpf = stpmin;
    }
    if (fp > fx) {
        sty = stp; fy = fp; dy = dp;
    } else {
        if (sgnd < 0.0) { sty = stx; fy = fx; dy = dx; }
        stx = stp; fx = fp; dx = dp;
    }
    return stpf;
}

constexpr double L2_FTOL = 1e-4, L2_GTOL = 0.9, L2_XTOL = 1e-14, L2_STPMIN = 1e-100, L2_STPMAX = 1e100;

// DCSRCH._iterate with task START: the step s.stp, the function f and the derivative g at 0
L2_HD int l2_dcsrch_start(L2SolveState& s, double f, double g) {
#pragma clang fp contract(off)
    if (s.stp < L2_STPMIN || s.stp > L2_STPMAX || g >= 0.0) return L2_TASK_ERROR;
    s.brackt = 0;
    s.stage = 1;
    s.finit = f;
    s.ginit = g;
    s.gtest = L2_FTOL * s.ginit;
    s.width = L2_STPMAX - L2_STPMIN;
    s.width1 = s.width / 0.5;
    s.stx = 0.0; s.fx = s.finit; s.gx = s.ginit;
    s.sty = 0.0; s.fy = s.finit; s.gy = s.ginit;
    s.stmin = 0.0;
    s.stmax = s.stp + 4.0 * s.stp;
    return L2_TASK_FG;
}

// DCSRCH._iterate afterwards: f and g are the function and the derivative at s.stp; FG leaves the next step in s.stp
L2_HD int l2_dcsrch_iterate(L2SolveState& s, double f, double g) {
#pragma clang fp contract(off)
    double stp = s.stp;
    const double ftest = s.finit + stp * s.gtest;
    if (s.stage == 1 && f <= ftest && g >= 0.0) s.stage = 2;
    int task = L2_TASK_FG;
    if (s.brackt && (stp <= s.stmin || stp >= s.stmax)) task = L2_TASK_WARN;
    if (s.brackt && s.stmax - s.stmin <= L2_XTOL * s.stmax) task = L2_TASK_WARN;
    if (stp == L2_STPMAX && f <= ftest && g <= s.gtest) task = L2_TASK_WARN;
    if (stp == L2_STPMIN && (f > ftest || g >= s.gtest)) task = L2_TASK_WARN;
    if (f <= ftest && l2_abs(g) <= L2_GTOL * -s.ginit) task = L2_TASK_CONV;
    if (task != L2_TASK_FG) return task;
    if (s.stage == 1 && f <= s.fx && f > ftest) {
        const double fm = f - stp * s.gtest;
        double fxm = s.fx - s.stx * s.gtest;
        double fym = s.fy - s.sty * s.gtest;
        const double gm = g - s.gtest;
        double gxm = s.gx - s.gtest;
        double gym = s.gy - s.gtest;
        stp = l2_dcstep(s.stx, fxm, gxm, s.sty, fym, gym, stp, fm, gm, s.brackt, s.stmin, s.stmax);
        s.fx = fxm + s.stx * s.gtest;
        s.fy = fym + s.sty * s.gtest;
        s.gx = gxm + s.gtest;
        s.gy = gym + s.gtest;
    } else {
        stp = l2_dcstep(s.stx, s.fx, s.gx, s.sty, s.fy, s.gy, stp, f, g, s.brackt, s.stmin, s.stmax);
    }
    if (s.brackt) {
        if (l2_abs(s.sty - s.stx) >= 0.66 * s.width1) stp = s.stx + 0.5 * (s.sty - s.stx);
        s.width1 = s.width;
        s.width = l2_abs(s.sty - s.stx);
    }
    if (s.brackt) {
        s.stmin = s.sty < s.stx ? s.sty : s.stx;
        s.stmax = s.sty > s.stx ? s.sty : s.stx;
    } else {
        s.stmin = stp + 1.1 * (stp - s.stx);
        s.stmax = stp + 4.0 * (stp - s.stx);
    }
    stp = l2_clip(stp, L2_STPMIN, L2_STPMAX);
    if ((s.brackt && (stp <= s.stmin || stp >= s.stmax)) || (s.brackt && s.stmax - s.stmin <= L2_XTOL * s.stmax)) stp = s.stx;
    s.stp = stp;
    return L2_TASK_FG;
}

// the hypothesis leaves the loop.  forced: the line search failed or f is not finite (warnflag 2); otherwise SciPy's order
L2_HD void l2_solve_leave(L2SolveState& s, bool forced) {
    bool nan = l2_isnan(s.gnorm) || l2_isnan(s.f);
    for (int i = 0; i < 7; ++i) nan = nan || l2_isnan(s.x[i]);
    s.status = forced ? L2_ST_LINESEARCH : (s.nit >= s.max_iter ? L2_ST_MAXITER : (nan ? L2_ST_NAN : L2_ST_OK));
    s.left = 1;
}

// One transition: `out` are the 13 sums of the evaluation under way (at s.x before the solve has started, at s.xt
// afterwards).  On return the hypothesis has either left the loop (s.left) or s.xt is the next point to evaluate.
L2_HD void l2_solve_step(L2SolveState& s, const double* out) {
#pragma clang fp contract(off)
    L2Quat qt;
    double ge[7];
    l2_quat_terms(s.started ? s.xt : s.x, true, qt);
    l2_chain_rule(out, qt, ge);
    const double fe = out[0];
    s.nfev += 1;
    if (!s.started) {
        s.started = 1;
        s.f = fe;
        for (int i = 0; i < 7; ++i) s.g[i] = ge[i];
        for (int i = 0; i < 49; ++i) s.H[i] = (i % 8 == 0) ? 1.0 : 0.0;
        s.old_old = s.f + l2_norm2(s.g) / 2.0;
        s.gnorm = l2_norm_inf(s.g);
    } else {
        const double derphi = l2_dot7(ge, s.pk);
        int task;
        if (s.ls_calls >= L2_LS_MAX) task = L2_TASK_WARN;                  // (the loop of DCSRCH.__call__ has run out)
        else {
            task = l2_dcsrch_iterate(s, fe, derphi);
            s.ls_calls += 1;
            if (!l2_isfinite(s.stp)) task = L2_TASK_WARN;
        }
        if (task == L2_TASK_FG) {
            for (int i = 0; i < 7; ++i) s.xt[i] = s.x[i] + s.stp * s.pk[i];
            return;
        }
        if (task != L2_TASK_CONV) { l2_solve_leave(s, true); return; }
        // the step is accepted: _minimize_bfgs from `sk = alpha_k * pk` on
        const double alpha = s.stp;
        double sk[7], yk[7];
        s.old_old = s.f;
        s.f = fe;
        for (int i = 0; i < 7; ++i) {
            sk[i] = alpha * s.pk[i];
            s.x[i] = s.x[i] + sk[i];
            yk[i] = ge[i] - s.g[i];
            s.g[i] = ge[i];
        }
        s.nit += 1;
        s.gnorm = l2_norm_inf(s.g);
        if (s.gnorm <= s.gtol) { l2_solve_leave(s, false); return; }
        if (alpha * l2_norm2(s.pk) <= 0.0 * (0.0 + l2_norm2(s.x))) { l2_solve_leave(s, false); return; }     // (xrtol = 0)
        if (!l2_isfinite(s.f)) { l2_solve_leave(s, true); return; }
        const double rhok_inv = l2_dot7(yk, sk);
        const double rhok = rhok_inv == 0.0 ? 1000.0 : 1.0 / rhok_inv;
        double T[49];
        for (int i = 0; i < 7; ++i)
            for (int j = 0; j < 7; ++j) {                                  // Hk A2,  A2 = I - yk sk^T rhok
                double acc = 0.0;
                for (int k = 0; k < 7; ++k) {
                    const double a2 = ((k == j) ? 1.0 : 0.0) - (yk[k] * sk[j]) * rhok;
                    const double term = s.H[7 * i + k] * a2;
                    acc = (k == 0) ? term : acc + term;
                }
                T[7 * i + j] = acc;
            }
        for (int i = 0; i < 7; ++i)
            for (int j = 0; j < 7; ++j) {                                  // A1 (Hk A2) + rhok sk sk^T,  A1 = I - sk yk^T rhok
                double acc = 0.0;
                for (int k = 0; k < 7; ++k) {
                    const double a1 = ((i == k) ? 1.0 : 0.0) - (sk[i] * yk[k]) * rhok;
                    const double term = a1 * T[7 * k + j];
                    acc = (k == 0) ? term : acc + term;
                }
                s.H[7 * i + j] = acc + (rhok * sk[i]) * sk[j];
            }
    }
    // the head of _minimize_bfgs' loop
    if (!(s.gnorm > s.gtol && s.nit < s.max_iter)) { l2_solve_leave(s, false); return; }
    for (int i = 0; i < 7; ++i) s.pk[i] = -l2_dot7(s.H + 7 * i, s.g);
    s.derphi0 = l2_dot7(s.g, s.pk);
    double alpha1 = 1.0;
    if (s.derphi0 != 0.0) {
        const double a = ((1.01 * 2.0) * (s.f - s.old_old)) / s.derphi0;
        alpha1 = a < 1.0 ? a : 1.0;
        if (alpha1 < 0.0) alpha1 = 1.0;
    }
    s.stp = alpha1;
    s.ls_calls = 1;
    if (l2_dcsrch_start(s, s.f, s.derphi0) != L2_TASK_FG || !l2_isfinite(s.stp)) { l2_solve_leave(s, true); return; }
    for (int i = 0; i < 7; ++i) s.xt[i] = s.x[i] + s.stp * s.pk[i];
}

}  // namespace hgmm
