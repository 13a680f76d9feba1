"""The written-down arithmetic of the device BFGS solve of the L2 GMMReg path (hgmm_l2_solve, csrc/l2_device.h), in Python
floats only: no NumPy reductions, no ``np.dot``, no ``einsum`` -- loops in the order the device uses, every operation one
of + - x / sqrt, a comparison or a sign change.  The device has to meet it bit for bit
(tests/test_gmmreg_device_solve_gpu.py); against SciPy itself it is held on the CPU
(tests/test_gmmreg_device_solve_cpu.py).

The optimiser is SciPy 1.15's BFGS (``_optimize.py::_minimize_bfgs``) over its first line search
(``_linesearch.py::line_search_wolfe1`` / ``scalar_search_wolfe1``, ``_dcsrch.py``), with ONE deliberate difference: when
dcsrch fails the solve ends at once with status 2 at the last accepted iterate, where SciPy first tries a second line search
(``line_search_wolfe2``).  ``nfev`` therefore differs from SciPy's by design.

``solve(evaluate, theta0, pair, sigma, max_iter, gtol)`` is parameterised by ``evaluate((rot [9], t [3]), pair, sigma) -> 13
numbers``: f, the gradient's column sums (3) and g.T @ mu_source (9, row-major), what ``hgmm_l2_cost`` returns for a pose.
"""
import math

NAN, INF = float("nan"), float("inf")
EPS = 2.220446049250313e-16
FTOL, GTOL, XTOL, STPMIN, STPMAX = 1e-4, 0.9, 1e-14, 1e-100, 1e100
LS_MAX = 100
FG, CONV, WARN, ERROR = 0, 1, 2, 3


def _div(a, b):
    """IEEE division (Python raises on a zero divisor)."""
    if b == 0.0:
        if a != a or a == 0.0:
            return NAN
        return -INF if (math.copysign(1.0, a) < 0.0) != (math.copysign(1.0, b) < 0.0) else INF
    return a / b


def _sqrt(a):
    """IEEE square root (Python raises on a negative argument)."""
    if a != a or a < 0.0:
        return NAN
    return math.sqrt(a)


def _abs(v):
    return -v if v < 0.0 else (0.0 if v == 0.0 else v)


def _isfinite(v):
    return (v - v) == 0.0


def _sign(v):
    return 1.0 if v > 0.0 else (-1.0 if v < 0.0 else (0.0 if v == 0.0 else v))


def _max3(a, b, c):
    m = a
    if b > m:
        m = b
    if c > m:
        m = c
    return m


def _clip(v, lo, hi):
    if v < lo:
        v = lo
    if v > hi:
        v = hi
    return v


def _dot(a, b):
    acc = a[0] * b[0]
    for i in range(1, len(a)):
        acc = acc + a[i] * b[i]
    return acc


def _norm2(a):
    return _sqrt(_dot(a, a))


def _norm_inf(a):
    m = _abs(a[0])
    for i in range(1, len(a)):
        v = _abs(a[i])
        if m == m and not (v <= m):
            m = v
    return m


def quat_terms(q):
    """-> (rot [9], d [4][9]): so.quaternion_matrix (identity when |q|^2 < 4 eps) and so.diff_rot_from_quaternion with the
    reference's quirks, from one n = |q|^2 summed left to right."""
    w, x, y, z = q
    n = ((w * w + x * x) + y * y) + z * z
    a = [-(y * y + z * z), x * y - w * z, x * z + w * y,
         x * y + w * z, -(x * x + z * z), y * z - w * x,
         x * z - w * y, y * z + w * x, -(x * x + y * y)]
    s = _div(2.0, n)
    raw = [1.0 + s * a[i] if i % 4 == 0 else s * a[i] for i in range(9)]
    if n < 4.0 * EPS:
        rot = [1.0 if i % 4 == 0 else 0.0 for i in range(9)]
    else:
        rot = list(raw)
    da = [[0.0, -z, y, z, 0.0, -x, -y, x, 0.0],
          [0.0, y, z, y, -2.0 * x, -w, z, w, -2.0 * x],
          [-2.0 * y, x, w, x, 0.0, z, -w, z, -2.0 * y],
          [-2.0 * z, -w, x, w, -2.0 * z, y, x, y, 0.0]]
    nn = n * n
    c4, c2 = _div(4.0, nn), _div(2.0, nn)
    d = [[0.0] * 9 for _ in range(4)]
    for k in range(4):
        for i in range(9):
            first = s * da[k][i]
            d[k][i] = first - (c4 * q[k]) * a[i] if i % 4 == 0 else first - (c2 * q[k]) * raw[i]
    d[2][8] = _div((-4.0 * y) * (x * x + y * y), nn)
    d[3][8] = _div((4.0 * z) * (z * z + w * w), nn)
    return rot, d


def chain_rule(out, d):
    g = [0.0] * 7
    for k in range(4):
        acc = out[4] * d[k][0]
        for i in range(1, 9):
            acc = acc + out[4 + i] * d[k][i]
        g[k] = acc
    g[4], g[5], g[6] = out[1], out[2], out[3]
    return g


class Dcsrch(object):
    """``_dcsrch.py::DCSRCH`` with ftol = 1e-4, gtol = 0.9, xtol = 1e-14, stpmin = 1e-100, stpmax = 1e100."""

    def start(self, stp, f, g):
        self.stp = stp
        if stp < STPMIN or stp > STPMAX or g >= 0.0:
            return ERROR
        self.brackt = False
        self.stage = 1
        self.finit = f
        self.ginit = g
        self.gtest = FTOL * self.ginit
        self.width = STPMAX - STPMIN
        self.width1 = self.width / 0.5
        self.stx, self.fx, self.gx = 0.0, self.finit, self.ginit
        self.sty, self.fy, self.gy = 0.0, self.finit, self.ginit
        self.stmin = 0.0
        self.stmax = stp + 4.0 * stp
        return FG

    def iterate(self, f, g):
        stp = self.stp
        ftest = self.finit + stp * self.gtest
        if self.stage == 1 and f <= ftest and g >= 0.0:
            self.stage = 2
        task = FG
        if self.brackt and (stp <= self.stmin or stp >= self.stmax):
            task = WARN
        if self.brackt and self.stmax - self.stmin <= XTOL * self.stmax:
            task = WARN
        if stp == STPMAX and f <= ftest and g <= self.gtest:
            task = WARN
        if stp == STPMIN and (f > ftest or g >= self.gtest):
            task = WARN
        if f <= ftest and _abs(g) <= GTOL * -self.ginit:
            task = CONV
        if task != FG:
            return task
        if self.stage == 1 and f <= self.fx and f > ftest:
            fm = f - stp * self.gtest
            fxm = self.fx - self.stx * self.gtest
            fym = self.fy - self.sty * self.gtest
            gm = g - self.gtest
            gxm = self.gx - self.gtest
            gym = self.gy - self.gtest
            self.stx, fxm, gxm, self.sty, fym, gym, stp, self.brackt = dcstep(
                self.stx, fxm, gxm, self.sty, fym, gym, stp, fm, gm, self.brackt, self.stmin, self.stmax)
            self.fx = fxm + self.stx * self.gtest
            self.fy = fym + self.sty * self.gtest
            self.gx = gxm + self.gtest
            self.gy = gym + self.gtest
        else:
            self.stx, self.fx, self.gx, self.sty, self.fy, self.gy, stp, self.brackt = dcstep(
                self.stx, self.fx, self.gx, self.sty, self.fy, self.gy, stp, f, g, self.brackt, self.stmin, self.stmax)
        if self.brackt:
            if _abs(self.sty - self.stx) >= 0.66 * self.width1:
                stp = self.stx + 0.5 * (self.sty - self.stx)
            self.width1 = self.width
            self.width = _abs(self.sty - self.stx)
        if self.brackt:
            self.stmin = self.sty if self.sty < self.stx else self.stx
            self.stmax = self.sty if self.sty > self.stx else self.stx
        else:
            self.stmin = stp + 1.1 * (stp - self.stx)
            self.stmax = stp + 4.0 * (stp - self.stx)
        stp = _clip(stp, STPMIN, STPMAX)
        if (self.brackt and (stp <= self.stmin or stp >= self.stmax)) or \
                (self.brackt and self.stmax - self.stmin <= XTOL * self.stmax):
            stp = self.stx
        self.stp = stp
        return FG


def dcstep(stx, fx, dx, sty, fy, dy, stp, fp, dp, brackt, stpmin, stpmax):
    sgnd = _sign(dp) * _sign(dx)
    if fp > fx:
        theta = _div(3.0 * (fx - fp), stp - stx) + dx + dp
        s = _max3(_abs(theta), _abs(dx), _abs(dp))
        ts = _div(theta, s)
        gamma = s * _sqrt(ts * ts - _div(dx, s) * _div(dp, s))
        if stp < stx:
            gamma = -gamma
        p = (gamma - dx) + theta
        q = ((gamma - dx) + gamma) + dp
        r = _div(p, q)
        stpc = stx + r * (stp - stx)
        stpq = stx + (_div(dx, _div(fx - fp, stp - stx) + dx) / 2.0) * (stp - stx)
        if _abs(stpc - stx) <= _abs(stpq - stx):
            stpf = stpc
        else:
            stpf = stpc + (stpq - stpc) / 2.0
        brackt = True
    elif sgnd < 0.0:
        theta = _div(3.0 * (fx - fp), stp - stx) + dx + dp
        s = _max3(_abs(theta), _abs(dx), _abs(dp))
        ts = _div(theta, s)
        gamma = s * _sqrt(ts * ts - _div(dx, s) * _div(dp, s))
        if stp > stx:
            gamma = -gamma
        p = (gamma - dp) + theta
        q = ((gamma - dp) + gamma) + dx
        r = _div(p, q)
        stpc = stp + r * (stx - stp)
        stpq = stp + _div(dp, dp - dx) * (stx - stp)
        if _abs(stpc - stp) > _abs(stpq - stp):
            stpf = stpc
        else:
            stpf = stpq
        brackt = True
    elif _abs(dp) < _abs(dx):
        theta = _div(3.0 * (fx - fp), stp - stx) + dx + dp
        s = _max3(_abs(theta), _abs(dx), _abs(dp))
        ts = _div(theta, s)
        under = ts * ts - _div(dx, s) * _div(dp, s)
        gamma = s * _sqrt(under if under > 0.0 else 0.0)
        if stp > stx:
            gamma = -gamma
        p = (gamma - dp) + theta
        q = (gamma + (dx - dp)) + gamma
        r = _div(p, q)
        if r < 0.0 and gamma != 0.0:
            stpc = stp + r * (stx - stp)
        elif stp > stx:
            stpc = stpmax
        else:
            stpc = stpmin
        stpq = stp + _div(dp, dp - dx) * (stx - stp)
        if brackt:
            if _abs(stpc - stp) < _abs(stpq - stp):
                stpf = stpc
            else:
                stpf = stpq
            lim = stp + 0.66 * (sty - stp)
            if stp > stx:
                stpf = stpf if stpf < lim else lim
            else:
                stpf = stpf if stpf > lim else lim
        else:
            if _abs(stpc - stp) > _abs(stpq - stp):
                stpf = stpc
            else:
                stpf = stpq
            stpf = _clip(stpf, stpmin, stpmax)
    else:
        if brackt:
            theta = _div(3.0 * (fp - fy), sty - stp) + dy + dp
            s = _max3(_abs(theta), _abs(dy), _abs(dp))
            ts = _div(theta, s)
            gamma = s * _sqrt(ts * ts - _div(dy, s) * _div(dp, s))
            if stp > sty:
                gamma = -gamma
            p = (gamma - dp) + theta
            q = ((gamma - dp) + gamma) + dy
            r = _div(p, q)
            stpf = stp + r * (sty - stp)
        elif stp > stx:
            stpf = stpmax
        else:
            stpf = stpmin
    if fp > fx:
        sty, fy, dy = stp, fp, dp
    else:
        if sgnd < 0.0:
            sty, fy, dy = stx, fx, dx
        stx, fx, dx = stp, fp, dp
    return stx, fx, dx, sty, fy, dy, stpf, brackt


def first_step(phi0, old_phi0, derphi0):
    """scalar_search_wolfe1's alpha1."""
    if derphi0 != 0.0:
        a = _div((1.01 * 2.0) * (phi0 - old_phi0), derphi0)
        alpha1 = a if a < 1.0 else 1.0
        if alpha1 < 0.0:
            alpha1 = 1.0
        return alpha1
    return 1.0


def line_search(phi_derphi, alpha1, phi0, derphi0):
    """``DCSRCH.__call__`` over ``phi_derphi(stp) -> (phi, derphi)`` -> (task, stp, phi at stp, steps evaluated).  The task
    is CONV, or WARN / ERROR for a failed search."""
    ls = Dcsrch()
    steps = []
    task = ls.start(alpha1, phi0, derphi0)
    calls = 1
    if task == FG and not _isfinite(ls.stp):
        task = WARN
    phi1 = phi0
    while task == FG:
        phi1, derphi1 = phi_derphi(ls.stp)
        steps.append(ls.stp)
        if calls >= LS_MAX:
            task = WARN
            break
        task = ls.iterate(phi1, derphi1)
        calls += 1
        if not _isfinite(ls.stp):
            task = WARN
    return task, ls.stp, phi1, steps


def solve(evaluate, theta0, pair, sigma, max_iter, gtol):
    """-> dict(x, f, grad, nit, nfev, status): status 0 gtol met, 1 max_iter, 2 line search failed, 3 NaN."""
    nfev = [0]
    last = {}

    def fg(xv):
        rot, d = quat_terms(xv[:4])
        out = [float(v) for v in evaluate((rot, [xv[4], xv[5], xv[6]]), pair, sigma)]
        nfev[0] += 1
        return out[0], chain_rule(out, d)

    x = [float(v) for v in theta0]
    gtol = float(gtol)
    f, g = fg(x)
    H = [1.0 if i % 8 == 0 else 0.0 for i in range(49)]
    old_old = f + _norm2(g) / 2.0
    gnorm = _norm_inf(g)
    nit = 0
    forced = False
    while gnorm > gtol and nit < max_iter:
        pk = [-_dot(H[7 * i:7 * i + 7], g) for i in range(7)]
        derphi0 = _dot(g, pk)

        def phi_derphi(stp, x=x, pk=pk):
            xt = [x[i] + stp * pk[i] for i in range(7)]
            ft, gt = fg(xt)
            last["g"] = gt
            return ft, _dot(gt, pk)

        task, alpha, fe, _ = line_search(phi_derphi, first_step(f, old_old, derphi0), f, derphi0)
        if task != CONV:
            forced = True
            break
        ge = last["g"]
        old_old = f
        f = fe
        sk = [alpha * pk[i] for i in range(7)]
        x = [x[i] + sk[i] for i in range(7)]
        yk = [ge[i] - g[i] for i in range(7)]
        g = ge
        nit += 1
        gnorm = _norm_inf(g)
        if gnorm <= gtol:
            break
        if alpha * _norm2(pk) <= 0.0 * (0.0 + _norm2(x)):
            break
        if not _isfinite(f):
            forced = True
            break
        rhok_inv = _dot(yk, sk)
        rhok = 1000.0 if rhok_inv == 0.0 else _div(1.0, rhok_inv)
        T = [0.0] * 49
        for i in range(7):
            for j in range(7):
                acc = 0.0
                for k in range(7):
                    a2 = (1.0 if k == j else 0.0) - (yk[k] * sk[j]) * rhok
                    term = H[7 * i + k] * a2
                    acc = term if k == 0 else acc + term
                T[7 * i + j] = acc
        Hn = [0.0] * 49
        for i in range(7):
            for j in range(7):
                acc = 0.0
                for k in range(7):
                    a1 = (1.0 if i == k else 0.0) - (sk[i] * yk[k]) * rhok
                    term = a1 * T[7 * k + j]
                    acc = term if k == 0 else acc + term
                Hn[7 * i + j] = acc + (rhok * sk[i]) * sk[j]
        H = Hn
    if forced:
        status = 2
    elif nit >= max_iter:
        status = 1
    elif gnorm != gnorm or f != f or any(v != v for v in x):
        status = 3
    else:
        status = 0
    return {"x": x, "f": f, "grad": g, "nit": nit, "nfev": nfev[0], "status": status}
