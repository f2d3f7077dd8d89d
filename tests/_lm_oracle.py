"""The Levenberg-Marquardt driver of xmris_amd/csrc/xm_lm.h (lm_fit_item) restated once for any
(model, Jacobian) pair, and the standard least-squares problems on which tests/test_lm.py and tests/test_gpu_lm.py run
it.  Plain numpy; it does not import xmris_amd.

A problem has Q physical parameters p, bounded by lmfit's transforms (internal variables u), 2 n real residuals
r = x - x^(p) (two per point) and the Jacobian d x^ / d p.  The closed-form problems (More, Garbow, Hillstrom, "Testing
unconstrained optimization software", 1981) have x = 0, x^ = -f.  The iteration: lambda_0 = 1e-3, D_j the largest squared
column norm so far (1 for a column that has always been zero), trial step (J^T J + lambda D) dl = J^T r, accepted when
the cost is finite and falls; then lambda *= max(1/3, 1 - (2 rho - 1)^3), nu = 2; else lambda *= nu, nu *= 2.  A trial
whose system cannot be solved counts and is a rejection.  Stop: (F - Ft) <= ftol F on an accepted step,
|D^(1/2) dl| <= xtol (|D^(1/2) u| + xtol) on any solved trial, lambda not finite, or the cap.
"""
import numpy as np

EPS = float(np.finfo(np.float64).eps)
FIXED, FREE, LO, HI, TWO = 0, 1, 2, 3, 4  # XM_WG_* of xm_wg.h
KINDS = ("rosenbrock", "powell", "freudenstein", "helical", "brown_dennis", "box3d", "exp2", "table", "wall")  # WGP_*
BRANCHES = ("cholesky_failed", "lambda_overflow", "nonfinite_cost_rejected", "xconv_on_rejection", "zero_column_scale",
            "crlb_failed")


# ---- bound transforms ---------------------------------------------------------------------------------------------------------
def bound_type(lo, hi, fixed=False):
    if fixed:
        return FIXED
    fl, fh = np.isfinite(lo), np.isfinite(hi)
    return TWO if fl and fh else LO if fl else HI if fh else FREE


def to_internal(bt, v, lo, hi):
    if bt == TWO:
        return float(np.arcsin(np.clip(2.0 * (v - lo) / (hi - lo) - 1.0, -1.0, 1.0)))
    if bt == LO:
        return float(np.sqrt((v - lo + 1.0) ** 2 - 1.0))
    if bt == HI:
        return float(np.sqrt((hi - v + 1.0) ** 2 - 1.0))
    return float(v)


def from_internal(bt, u, lo, hi):
    """(p, dp/du); on a two-sided bound (sin u = +-1) the slope is exactly 0 and the value is the bound."""
    if bt == TWO:
        s = np.sin(u)
        p = hi if s == 1.0 else lo + (s + 1.0) * (hi - lo) * 0.5
        return p, (0.0 if abs(s) == 1.0 else np.cos(u) * (hi - lo) * 0.5)
    if bt == LO:
        r = np.sqrt(u * u + 1.0)
        return lo - 1.0 + r, u / r
    if bt == HI:
        r = np.sqrt(u * u + 1.0)
        return hi + 1.0 - r, -u / r
    return u, 1.0


# ---- the problems: (x^ [2n], x [2n], d x^ / d p [2n, Q]) at p ----------------------------------------------------------------
def _closed(f, df):
    f, df = np.asarray(f, dtype=np.float64), np.asarray(df, dtype=np.float64)
    if f.size % 2:  # an odd number of residuals: the last point's second row is a zero row
        f, df = np.append(f, 0.0), np.vstack([df, np.zeros(df.shape[1])])
    return -f, np.zeros(f.size), -df


def _rosenbrock(p, tab):
    return _closed([10.0 * (p[1] - p[0] * p[0]), 1.0 - p[0]], [[-20.0 * p[0], 10.0], [-1.0, 0.0]])


def _wall(p, tab):
    with np.errstate(invalid="ignore"):
        beyond = 0.0 * np.sqrt(tab[0] - p[0])  # 0 on this side of the wall, NaN beyond it
    return _closed([10.0 * (p[1] - p[0] * p[0]), 1.0 - p[0], beyond], [[-20.0 * p[0], 10.0], [-1.0, 0.0], [0.0, 0.0]])


def _powell(p, tab):
    a, b, s5, s10 = p[1] - 2.0 * p[2], p[0] - p[3], np.sqrt(5.0), np.sqrt(10.0)
    return _closed([p[0] + 10.0 * p[1], s5 * (p[2] - p[3]), a * a, s10 * (b * b)],
                   [[1.0, 10.0, 0.0, 0.0], [0.0, 0.0, s5, -s5], [0.0, 2.0 * a, -4.0 * a, 0.0],
                    [2.0 * s10 * b, 0.0, 0.0, -2.0 * s10 * b]])


def _freudenstein(p, tab):
    return _closed([-13.0 + p[0] + ((5.0 - p[1]) * p[1] - 2.0) * p[1], -29.0 + p[0] + ((p[1] + 1.0) * p[1] - 14.0) * p[1]],
                   [[1.0, 10.0 * p[1] - 3.0 * p[1] * p[1] - 2.0], [1.0, 3.0 * p[1] * p[1] + 2.0 * p[1] - 14.0]])


def _helical(p, tab):
    with np.errstate(all="ignore"):
        r2 = p[0] * p[0] + p[1] * p[1]
        r = np.sqrt(r2)
        th = np.arctan(p[1] / p[0]) / (2.0 * np.pi) + (0.5 if p[0] < 0.0 else 0.0)
        return _closed([10.0 * (p[2] - 10.0 * th), 10.0 * (r - 1.0), p[2]],
                       [[100.0 * p[1] / (2.0 * np.pi * r2), -100.0 * p[0] / (2.0 * np.pi * r2), 10.0],
                        [10.0 * p[0] / r, 10.0 * p[1] / r, 0.0], [0.0, 0.0, 1.0]])


def _brown_dennis(p, tab):
    t = np.arange(1, 21) / 5.0
    a, b = p[0] + t * p[1] - np.exp(t), p[2] + p[3] * np.sin(t) - np.cos(t)
    return _closed(a * a + b * b, np.stack([2.0 * a, 2.0 * a * t, 2.0 * b, 2.0 * b * np.sin(t)], axis=1))


def _box3d(p, tab):
    t = 0.1 * np.arange(1, 11)
    with np.errstate(over="ignore"):
        e0, e1, c = np.exp(-t * p[0]), np.exp(-t * p[1]), np.exp(-t) - np.exp(-10.0 * t)
    return _closed(e0 - e1 - p[2] * c, np.stack([-t * e0, t * e1, -c], axis=1))


def _exp2(p, tab):
    n_res = int(tab[0])
    t, y = tab[1:1 + 2 * n_res:2], tab[2:2 + 2 * n_res:2]
    with np.errstate(over="ignore"):
        e0, e1 = np.exp(-p[1] * t), np.exp(-p[3] * t)
    m, j = p[0] * e0 + p[2] * e1, np.stack([e0, -p[0] * t * e0, e1, -p[2] * t * e1], axis=1)
    if n_res % 2:
        m, y, j = np.append(m, 0.0), np.append(y, 0.0), np.vstack([j, np.zeros(4)])
    return m, y, j


def _table(p, tab):
    Q = p.size
    rows = tab[1:].reshape(-1, Q + 1)
    a = rows[:, :Q]
    j = a.copy()
    j[:, 0] = j[:, 0] + tab[0]  # jadd: 0, or NaN for a Jacobian that is not finite where the cost is
    with np.errstate(all="ignore"):
        return a @ p, rows[:, Q].copy(), j


_FUN = {"rosenbrock": _rosenbrock, "powell": _powell, "freudenstein": _freudenstein, "helical": _helical,
        "brown_dennis": _brown_dennis, "box3d": _box3d, "exp2": _exp2, "table": _table, "wall": _wall}


def evaluate(kind, p, tab=None):
    """(x^, x, d x^ / d p) of problem `kind` at the physical parameters p."""
    return _FUN[kind](np.asarray(p, dtype=np.float64), None if tab is None else np.asarray(tab, dtype=np.float64))


def table_of(a, y, jadd=0.0):
    """The data table of a `table` problem: A [2n, Q], y [2n]."""
    return np.concatenate([[jadd], np.concatenate([a, y[:, None]], axis=1).ravel()])


# ---- the two solvers ----------------------------------------------------------------------------------------------------------
def cholesky(h):
    """Lower factor of h, or None where a pivot is not positive and finite (wg_cholesky's rule)."""
    P = h.shape[0]
    L = np.zeros_like(h)
    with np.errstate(all="ignore"):
        for j in range(P):
            s = h[j, j] - L[j, :j] @ L[j, :j]
            if not (s > 0.0) or not np.isfinite(s):
                return None
            L[j, j] = np.sqrt(s)
            L[j + 1:, j] = (h[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def _solve_normal(H, g, lam, D, jr, rr):
    L = cholesky(H + lam * np.diag(D))
    if L is None:
        return None
    P = g.size
    with np.errstate(all="ignore"):
        y = np.zeros(P)
        for j in range(P):
            y[j] = (g[j] - L[j, :j] @ y[:j]) / L[j, j]
        for j in range(P - 1, -1, -1):
            y[j] = (y[j] - L[j + 1:, j] @ y[j + 1:]) / L[j, j]
    return y if np.all(np.isfinite(y)) else None


def lstsq_longdouble(a, b):
    """Least squares by Householder reflections in numpy.longdouble; None where it does not come out finite."""
    a, b = np.array(a, dtype=np.longdouble), np.array(b, dtype=np.longdouble)
    m, n = a.shape
    with np.errstate(all="ignore"):
        for k in range(n):
            x = a[k:, k]
            nx = np.sqrt(x @ x)
            if not np.isfinite(nx) or nx == 0:
                return None
            v = x.copy()
            v[0] += nx if x[0] >= 0 else -nx
            v /= np.sqrt(v @ v)
            a[k:, k:] -= 2 * np.outer(v, v @ a[k:, k:])
            b[k:] -= 2 * v * (v @ b[k:])
        x = np.zeros(n, dtype=np.longdouble)
        for k in range(n - 1, -1, -1):
            x[k] = (b[k] - a[k, k + 1:n] @ x[k + 1:]) / a[k, k]
    x = x.astype(np.float64)
    return x if np.all(np.isfinite(x)) else None


def _solve_lstsq(H, g, lam, D, jr, rr):
    P = g.size
    if not (np.all(np.isfinite(jr)) and np.all(np.isfinite(rr)) and np.isfinite(lam)):
        return None
    # A column that is exactly zero (a parameter on its bound, slope 0) decouples: its step is exactly 0, as forward and
    # back substitution give it.  Reflections would leave a rounding-sized step there, which moves the parameter off
    # its bound.
    on = np.any(jr != 0.0, axis=0)
    dl = np.zeros(P)
    if on.any():
        sub = lstsq_longdouble(np.concatenate([jr[:, on], np.diag(np.sqrt(lam * D[on]))]),
                               np.concatenate([rr, np.zeros(int(on.sum()))]))
        if sub is None:
            return None
        dl[on] = sub
    return dl


# ---- the driver ---------------------------------------------------------------------------------------------------------------
class Case:
    """One listed problem: kind, physical start [Q], bounds and fixed mask [Q], data table, tolerances, the number of
    amplitudes (the first NA parameters) and their factors."""

    def __init__(self, name, kind, start, lo=None, hi=None, fixed=None, tab=None, ftol=1e-10, xtol=1e-10, n_amp=None,
                 factor=None, expect=None):
        self.name, self.kind = name, kind
        self.start = np.asarray(start, dtype=np.float64)
        Q = self.Q = self.start.size
        self.lo = np.full(Q, -np.inf) if lo is None else np.asarray(lo, dtype=np.float64)
        self.hi = np.full(Q, np.inf) if hi is None else np.asarray(hi, dtype=np.float64)
        self.fixed = np.zeros(Q, bool) if fixed is None else np.asarray(fixed, bool)
        self.bt = np.array([bound_type(self.lo[q], self.hi[q], self.fixed[q]) for q in range(Q)], dtype=np.int32)
        self.free = np.flatnonzero(~self.fixed)
        self.P = self.free.size
        self.tab = np.zeros(1) if tab is None else np.asarray(tab, dtype=np.float64)
        self.ftol, self.xtol = ftol, xtol
        self.NA = Q if n_amp is None else n_amp
        # never 1, so that a dropped factor shows
        self.factor = 1.5 + (0.25 * np.arange(self.NA)) % 2.0 if factor is None else np.asarray(factor, dtype=np.float64)
        self.expect = expect or {}
        with np.errstate(all="ignore"):
            self.n_points = evaluate(kind, self.start, self.tab)[0].size // 2

    def start_vector(self):
        """[Q] as the probe takes it: the internal start value of a free parameter, the physical value of a fixed one."""
        return np.array([self.start[q] if self.fixed[q] else to_internal(self.bt[q], self.start[q], self.lo[q], self.hi[q])
                         for q in range(self.Q)])

    def physical(self, u):
        p, s = self.start.copy(), np.zeros(self.Q)
        with np.errstate(all="ignore"):
            for j, q in enumerate(self.free):
                p[q], s[q] = from_internal(self.bt[q], u[j], self.lo[q], self.hi[q])
        return p, s

    def cost(self, p):
        with np.errstate(all="ignore"):
            m, x, _ = evaluate(self.kind, p, self.tab)
            return float(np.sum((x - m) ** 2))


def crlb(case, p):
    """(sd [NA], cond, failed): sqrt(diag((J^T J)^{-1})) factor over the physical free columns at p (0 for a fixed
    amplitude; NaN for every free one where the factorisation fails) from an SVD of the column-scaled Jacobian, and
    the 2-norm condition number of J^T J."""
    with np.errstate(all="ignore"):
        j = evaluate(case.kind, p, case.tab)[2][:, case.free]
        failed = cholesky(j.T @ j) is None
    sd = np.zeros(case.Q)
    cond = np.inf
    if failed or not np.all(np.isfinite(j)):
        sd[case.free] = np.nan
    else:
        sv = np.linalg.svd(j, compute_uv=False)
        cond = float((sv[0] / sv[-1]) ** 2) if sv[-1] > 0 else np.inf
        c = np.linalg.norm(j, axis=0)
        _, s, vt = np.linalg.svd(j / c, full_matrices=False)
        with np.errstate(all="ignore"):
            sd[case.free] = np.sqrt(np.sum((vt.T / s) ** 2, axis=1)) / c
    return sd[:case.NA] * case.factor, cond, failed


def lm_fit(case, max_iter=200, route="normal"):
    """lm_fit_item on `case`.  route: "normal" (fp64 normal equations and a Cholesky solve, as the kernel forms them) or
    "lstsq" (least squares on the augmented Jacobian [J; sqrt(lambda D)] in longdouble; J^T J is never formed).

    Returns a dict: u [P], params [Q], rss, iters, status (0 converged, 1 cap or lambda overflow, 2 not finite), asd [NA],
    fit [2n], trials (list of (accepted, margin (F - Ft) / F, reason)), path [Q] and path_u [P] (sums of |change| over
    the accepted steps), branches (a counter per name of BRANCHES), crlb_cond."""
    solve = {"normal": _solve_normal, "lstsq": _solve_lstsq}[route]
    br = dict.fromkeys(BRANCHES, 0)
    u = case.start_vector()[case.free]
    P = case.P
    p, s = case.physical(u)
    F = case.cost(p)
    status = 1 if np.isfinite(F) else 2
    dsc = np.zeros(P)
    lam, nu, it = 1e-3, 2.0, 0
    need_jac, trials = True, []
    path, path_u = np.zeros(case.Q), np.zeros(P)
    while status == 1 and it < max_iter:
        if need_jac:
            p, s = case.physical(u)
            with np.errstate(all="ignore"):
                m, x, j = evaluate(case.kind, p, case.tab)
                jr, rr = j[:, case.free] * s[case.free], x - m
                H, g = jr.T @ jr, jr.T @ rr
                dsc = np.fmax(dsc, np.diag(H))  # fmax: a NaN norm leaves the scale as it was
            need_jac = False
        it += 1
        D = np.where(dsc > 0, dsc, 1.0)
        if np.any(~(dsc > 0)):
            br["zero_column_scale"] += 1
        dl = solve(H, g, lam, D, jr, rr)
        if dl is None:
            br["cholesky_failed"] += 1
            trials.append((False, -np.inf, "no_solve"))
            lam *= nu
            nu *= 2.0
            if not np.isfinite(lam):
                br["lambda_overflow"] += 1
                break
            continue
        dn, un = np.sqrt(np.sum(D * dl * dl)), np.sqrt(np.sum(D * u * u))
        pred = float(dl @ (lam * D * dl + g))
        xconv = bool(dn <= case.xtol * (un + case.xtol))
        ut = u + dl
        pt, _ = case.physical(ut)
        Ft = case.cost(pt)
        if np.isfinite(Ft) and Ft < F:
            trials.append((True, (F - Ft) / F, "accepted"))
            rho = min(max((F - Ft) / pred, 0.0), 1.0)
            fconv = (F - Ft) <= case.ftol * F
            path += np.abs(pt - p)
            path_u += np.abs(ut - u)
            u, F, p = ut, Ft, pt
            q = 2.0 * rho - 1.0
            lam *= max(1.0 / 3.0, 1.0 - q * q * q)
            nu = 2.0
            need_jac = True
            if fconv or xconv:
                status = 0
        else:
            if not np.isfinite(Ft):
                br["nonfinite_cost_rejected"] += 1
                trials.append((False, -np.inf, "nonfinite_cost"))
            elif np.array_equal(ut, u):
                # a step of exactly zero: Ft is F computed again at the same point, nothing to compare
                trials.append((False, -np.inf, "zero_step"))
            else:
                trials.append((False, (F - Ft) / F if F > 0 else -np.inf, "cost_rose"))
            lam *= nu
            nu *= 2.0
            if xconv:
                br["xconv_on_rejection"] += 1
                status = 0
            if not np.isfinite(lam):
                br["lambda_overflow"] += 1
                break
    p, _ = case.physical(u)
    if not (np.all(np.isfinite(p)) and np.isfinite(F)):
        status = 2
    out = {"u": u, "iters": it, "status": status, "trials": trials, "path": path, "path_u": path_u, "branches": br}
    if status == 2:  # a row that is not finite: all zeros, NaN rss
        out.update(params=np.zeros(case.Q), rss=np.nan, asd=np.zeros(case.NA), fit=np.zeros(2 * case.n_points),
                   crlb_cond=np.inf)
        return out
    sd, cond, failed = crlb(case, p)
    br["crlb_failed"] += int(failed)
    with np.errstate(all="ignore"):
        fit = evaluate(case.kind, p, case.tab)[0]
    out.update(params=p, rss=F, asd=sd, fit=fit, crlb_cond=cond)
    return out


def caps(stop):
    """max_iter of the trajectory tests: 1, 2, 3, 5, 8, 13, ... up to and past the stopping trial."""
    out, a, b = [], 1, 2
    while not out or out[-1] <= stop:
        out.append(a)
        a, b = b, a + b
    return out


# ---- the listed cases ---------------------------------------------------------------------------------------------------------
def table_data(P_free, n_points, seed, Q=None, fixed=(), zero_cols=(), noise=0.05):
    """Seeded linear problem: A [2 n_points, Q] with column norms spread over two decades, y = A truth + noise."""
    Q = P_free + len(fixed) if Q is None else Q
    rng = np.random.default_rng([seed, Q, n_points])
    a = rng.standard_normal((2 * n_points, Q)) * 10.0 ** rng.uniform(-1.0, 1.0, Q)
    a[:, list(zero_cols)] = 0.0
    truth = rng.uniform(0.5, 2.0, Q)
    y = a @ truth + noise * rng.standard_normal(2 * n_points)
    return a, y, truth


def _exp2_tab(n_res, seed):
    rng = np.random.default_rng(seed)
    t = np.linspace(0.0, 3.0, n_res)
    y = 4.0 * np.exp(-1.0 * t) + 2.0 * np.exp(-5.0 * t) + 0.01 * rng.standard_normal(n_res)
    pad = np.zeros(2 * (n_res % 2))  # the table holds 2 n_points entries; the one past n_res is not read
    return np.concatenate([[float(n_res)], np.stack([t, y], axis=1).ravel(), pad])


def cases():
    """The list of tests/test_lm.py and tests/test_gpu_lm.py.  `expect`: what a branch-only case must end as."""
    inf = np.inf
    a5, y5, _ = table_data(5, 12, 1)
    a6, y6, _ = table_data(6, 9, 2)
    az, yz, _ = table_data(4, 8, 3, zero_cols=(2,))
    an, yn, _ = table_data(3, 6, 4)
    return [
        Case("rosenbrock", "rosenbrock", [-1.2, 1.0]),
        Case("rosenbrock_lo_hi", "rosenbrock", [-1.2, 1.0], lo=[-2.0, -inf], hi=[inf, 5.0]),
        Case("powell_lo", "powell", [3.0, -1.0, 0.0, 1.0], lo=[-10.0] * 4, xtol=1e-3),
        Case("freudenstein", "freudenstein", [0.5, -2.0], ftol=1e-7),
        Case("helical", "helical", [-1.0, 0.0, 0.0]),
        Case("brown_dennis", "brown_dennis", [25.0, 5.0, -5.0, -1.0], ftol=1e-3),
        Case("box3d_two", "box3d", [0.0, 10.0, 20.0], lo=[-10.0, -10.0, -10.0], hi=[30.0, 30.0, 30.0]),
        Case("exp2_lo", "exp2", [3.0, 0.5, 3.0, 3.0], lo=[-inf, 0.0, -inf, 0.0], tab=_exp2_tab(41, 5), ftol=1e-4),
        Case("exp2_fixed", "exp2", [3.0, 0.5, 2.0, 3.0], fixed=[False, False, True, False], tab=_exp2_tab(40, 6), n_amp=3,
             ftol=1e-4),
        Case("table5", "table", [10.0, -10.0, 5.0, 0.0, 3.0], tab=table_of(a5, y5), ftol=1e-6),
        Case("table6_on_bound", "table", [1.0, 4.0, 1.0, -3.0, 2.0, 1.0], lo=[-inf, -inf, -inf, -inf, 0.0, -inf],
             hi=[inf, 4.0, inf, inf, 2.0, inf], tab=table_of(a6, y6), ftol=1e-2),
        Case("table_zero_column", "table", [3.0, -2.0, 1.0, 4.0], tab=table_of(az, yz), ftol=1e-6,
             expect={"asd_nan": True}),
        Case("wall", "wall", [-1.2, 1.0], tab=[-0.9], xtol=0.05, expect={"status": 0}),
        Case("nan_jacobian", "table", [1.0, 2.0, 3.0], tab=table_of(an, yn, jadd=np.nan),
             expect={"status": 1, "asd_nan": True, "all_no_solve": True}),
        Case("infinite_start", "rosenbrock", [1e200, 1.0], expect={"status": 2, "iters": 0}),
    ]


# ---- staging rounds and CRLB rounds (`table` problems) ------------------------------------------------------------------------
def q_pts(P):
    """lm_q_pts of xm_lm.h at lda = P + 1: points per staging round."""
    q = 128
    while q > 32 and 2 * q * (P + 1) * 8 > 65536:
        q >>= 1
    return q


STAGING_P = (1, 63, 64, 65, 80)  # either side of q_pts = 64 / 32 and of cap = 2 q_pts (P + 1) / P = 64


def staging_points(P):
    q = q_pts(P)
    return ((P + 1) // 2, q - 1, q, q + 1, 3 * q + 5)


def staging_case(P, n_points, n_amp=None, n_fixed=0):
    """All P columns free, every parameter an amplitude unless n_amp says otherwise; n_fixed further parameters, fixed,
    spread among the free ones so that both CRLB rounds hold some."""
    Q = P + n_fixed
    fixed = np.zeros(Q, bool)
    if n_fixed:
        fixed[np.round(np.linspace(1, Q - 2, n_fixed)).astype(int)] = True
        assert fixed.sum() == n_fixed
    a, y, truth = table_data(P, n_points, 7, Q=Q)
    start = truth + 0.3 * np.cos(np.arange(Q))
    return Case(f"table_P{P}_n{n_points}_Q{Q}_NA{n_amp or Q}", "table", start, fixed=fixed, tab=table_of(a, y), ftol=1e-6,
                n_amp=n_amp)


def crlb_round_cases():
    """P = 80 (cap = 64): amplitudes either side of one round, and 120 amplitudes of which 40 are fixed."""
    return [staging_case(80, 60, n_amp=64), staging_case(80, 60, n_amp=65), staging_case(80, 60, n_amp=80),
            staging_case(80, 60, n_amp=120, n_fixed=40)]
