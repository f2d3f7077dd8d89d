"""TEST ORACLE (not product code): the rate model of DESIGN.md section 19 in numpy / scipy, fp64, the yardstick of
k_kinetics_fit.  It does not import xmris_amd.

One item is a (voxel, product) pair: substrate samples S [T], product samples Y [T], weights w [T] (0: a missing point,
whose sample is not read), times t [T] (seconds, increasing), flip angles ths [T] and thp [T] (radians), and three
parameters in the order k (rate), rho (decay), z (magnetisation before the first excitation):

    Zs_n = S_n / sin ths[n],   Zs+_n = Zs_n cos ths[n],   D_n = t[n+1] - t[n],   x = rho D_n
    Z_0 = z,   Z_{n+1} = e^{-x} cos thp[n] Z_n + k (w0_n Zs+_n + w1_n Zs_{n+1})
    w1_n = D_n (x - 1 + e^{-x}) / x^2,   w0_n = D_n (1 - e^{-x}) / x - w1_n,   model_n = Z_n sin thp[n]
    cost = sum_n w_n^2 (Y_n - model_n)^2

Bounds: lmfit's transforms (tests/_amares_oracle.py).  The model is stated twice: `forward` is the plain sequential
recurrence, `forward_scan` the same numbers in the order of an affine prefix scan over 64 lanes.
"""
import math

import numpy as np
from scipy.optimize import least_squares

from _amares_oracle import from_internal, to_internal

EPS = 2.0 ** -52
SERIES_X = 0.5  # x = rho D below this: power series; from it on: closed forms on expm1
TERMS = 16
NAMES = ("k", "rho", "z")


# ---- the weights -----------------------------------------------------------------------------------------------------
def _series(x, den, num):
    """sum_{i < TERMS} num(i) / (i + den)! (-x)^i by Horner's rule."""
    acc = np.zeros_like(x)
    for i in range(TERMS - 1, -1, -1):
        acc = acc * (-x) + num(i) / math.factorial(i + den)
    return acc


def weights_series(rho, D):
    x = rho * D
    return (D * _series(x, 2, lambda i: i + 1.0), D * _series(x, 2, lambda i: 1.0),
            D * D * _series(x, 3, lambda i: -(i + 1.0) * (i + 2.0)), D * D * _series(x, 3, lambda i: -(i + 1.0)))


def weights_closed(rho, D):
    x = rho * D
    em = np.expm1(-x)
    f2 = (x + em) / (x * x)
    df1 = (x + (x + 1.0) * em) / (x * x)
    df2 = -(2.0 * x + (x + 2.0) * em) / (x * x * x)
    return D * (-em / x - f2), D * f2, D * D * (df1 - df2), D * D * df2


def weights(rho, D):
    """(E, w0, w1, dE, dw0, dw1) for the intervals D [T - 1] at rho; the d are derivatives with respect to rho."""
    D = np.asarray(D, dtype=np.float64)
    x = rho * D
    small = x < SERIES_X
    with np.errstate(all="ignore"):
        s, c = weights_series(rho, D), weights_closed(rho, D)
    w0, w1, dw0, dw1 = (np.where(small, a, b) for a, b in zip(s, c))
    E = np.exp(-x)
    return E, w0, w1, -D * E, dw0, dw1


def _pieces(p, S, t, ths, thp):
    """a [T - 1], c [T - 1] (Z_{n+1} = a_n Z_n + k c_n) and their rho derivatives."""
    S, t, ths, thp = (np.asarray(v, dtype=np.float64) for v in (S, t, ths, thp))
    zs = S / np.sin(ths)
    zsp = zs * np.cos(ths)
    E, w0, w1, dE, dw0, dw1 = weights(p[1], np.diff(t))
    cp = np.cos(thp[:-1])
    return E * cp, w0 * zsp[:-1] + w1 * zs[1:], dE * cp, dw0 * zsp[:-1] + dw1 * zs[1:]


def forward(p, S, t, ths, thp):
    """(Z [T], dZ [T, 3]): the magnetisation before each excitation and its derivatives by k, rho, z, sequentially."""
    k, _, z = p
    a, c, da, dc = _pieces(p, S, t, ths, thp)
    T = len(t)
    Z, dZ = np.zeros(T), np.zeros((T, 3))
    Z[0], dZ[0, 2] = z, 1.0
    for n in range(T - 1):
        Z[n + 1] = a[n] * Z[n] + k * c[n]
        dZ[n + 1, 0] = a[n] * dZ[n, 0] + c[n]
        dZ[n + 1, 1] = a[n] * dZ[n, 1] + da[n] * Z[n] + k * dc[n]
        dZ[n + 1, 2] = a[n] * dZ[n, 2]
    return Z, dZ


def _scan(a, c):
    """B_j = a_j B_{j-1} + c_j from B = 0 in scan order: element j of lane j // C, C = ceil(len / 64); each lane composes
    its maps, an inclusive Hillis-Steele scan runs over the 64 lane totals, each lane applies its exclusive prefix."""
    n = len(a)
    C = -(-n // 64)
    a = np.concatenate([a, np.ones(64 * C - n)]).reshape(64, C)
    c = np.concatenate([c, np.zeros(64 * C - n)]).reshape(64, C)
    at, ct = np.ones(64), np.zeros(64)
    for j in range(C):
        ct = a[:, j] * ct + c[:, j]
        at = a[:, j] * at
    d = 1
    while d < 64:
        a2, c2 = np.roll(at, d), np.roll(ct, d)
        hit = np.arange(64) >= d
        ct = np.where(hit, at * c2 + ct, ct)
        at = np.where(hit, at * a2, at)
        d *= 2
    pa = np.concatenate([[1.0], at[:-1]])
    pc = np.concatenate([[0.0], ct[:-1]])
    A, B = np.zeros((64, C)), np.zeros((64, C))
    for j in range(C):
        pa = a[:, j] * pa
        pc = a[:, j] * pc + c[:, j]
        A[:, j], B[:, j] = pa, pc
    return A.reshape(-1)[:n], B.reshape(-1)[:n]


def forward_scan(p, S, t, ths, thp):
    """`forward` in the order of the scan: Z = z A + k B, then the rho column from a second scan."""
    k, _, z = p
    a, c, da, dc = _pieces(p, S, t, ths, thp)
    a1, c1 = np.concatenate([[1.0], a]), np.concatenate([[0.0], c])  # element 0 is the identity: A_0 = 1, B_0 = 0
    A, B = _scan(a1, c1)
    Z = z * A + k * B
    h = np.concatenate([[0.0], da * Z[:-1] + k * dc])
    _, G = _scan(a1, h)
    return Z, np.stack([B, G, A], axis=1)


def model(p, S, t, ths, thp):
    return forward(p, S, t, ths, thp)[0] * np.sin(thp)


def model_jacobian(p, S, t, ths, thp):
    """d model / d (k, rho, z): [T, 3]."""
    return forward(p, S, t, ths, thp)[1] * np.sin(thp)[:, None]


def jacobian_central(p, S, t, ths, thp, rel=1e-6):
    p = np.asarray(p, dtype=np.float64)
    J = np.zeros((len(t), 3))
    for q in range(3):
        h = rel * max(abs(p[q]), 1e-2)
        up, dn = p.copy(), p.copy()
        up[q] += h
        dn[q] -= h
        J[:, q] = (model(up, S, t, ths, thp) - model(dn, S, t, ths, thp)) / (2.0 * h)
    return J


def simulate(S_mag, t, ths, thp, k, rho, z=0.0):
    """Noise-free samples (S [T], Y [T]) from a substrate magnetisation S_mag [T] (before each excitation)."""
    S = np.asarray(S_mag, dtype=np.float64) * np.sin(ths)
    return S, model((k, rho, z), S, t, ths, thp)


def auc_ratio(S, Y, w, t):
    """Trapezoid area over t of Y divided by that of S, both over the points of positive weight."""
    on = np.flatnonzero(np.asarray(w) > 0)
    if on.size < 2:
        return np.nan
    tt = np.asarray(t, dtype=np.float64)[on]
    area = lambda v: np.sum(0.5 * np.diff(tt) * (v[on][1:] + v[on][:-1]))  # noqa: E731
    with np.errstate(all="ignore"):  # (numpy's division: a zero area gives inf or NaN, as on the device)
        return float(area(np.asarray(Y, dtype=np.float64)) / area(np.asarray(S, dtype=np.float64)))


# ---- bounds and starts -----------------------------------------------------------------------------------------------
def _split(lo, hi, fixed):
    lo, hi = (np.asarray(v, dtype=np.float64).ravel() for v in (lo, hi))
    fixed = np.zeros(3, bool) if fixed is None else np.asarray(fixed, bool).ravel()
    fixed = fixed | (lo == hi)
    return lo, hi, fixed, np.flatnonzero(~fixed)


def start_values(Y, w, thp, init, lo, hi, fixed=None):
    """(v0 [3], u0 [P]): a NaN start of a free z is |Y_j| / sin thp[j] at the first repetition j of positive weight (0
    when there is none); everything is clipped into its bounds."""
    lo, hi, fixed, free = _split(lo, hi, fixed)
    v0 = np.asarray(init, dtype=np.float64).ravel().copy()
    if np.isnan(v0[2]) and not fixed[2]:
        on = np.flatnonzero(np.asarray(w) > 0)
        v0[2] = abs(Y[on[0]]) / np.sin(thp[on[0]]) if on.size else 0.0
    v0 = np.clip(v0, lo, hi)
    return v0, np.array([to_internal(v0[q], lo[q], hi[q]) for q in free])


def physical(u, v0, lo, hi, fixed=None):
    lo, hi, fixed, free = _split(lo, hi, fixed)
    p, s = np.array(v0, dtype=np.float64).copy(), np.zeros(3)
    for j, q in enumerate(free):
        p[q], s[q] = from_internal(u[j], lo[q], hi[q])
    return p, s


def _resid(p, c):
    on = c["w"] > 0
    r = np.zeros(len(c["t"]))
    r[on] = c["w"][on] * (c["Y"][on] - model(p, c["S"], c["t"], c["ths"], c["thp"])[on])
    return r


def cost(p, c):
    r = _resid(p, c)
    return float(r @ r)


def _wjac(p, c):
    return np.where(c["w"] > 0, c["w"], 0.0)[:, None] * model_jacobian(p, c["S"], c["t"], c["ths"], c["thp"])


def covariance_sd(p, c):
    """(sd [3], cond): sqrt(diag((J^T W J)^{-1}) rss / (T_w - P)) over the physical free columns at p (0 for a fixed
    parameter; NaN when a column vanishes or T_w = P), from an SVD of the column-scaled Jacobian, with the 2-norm
    condition number of the scaled J^T W J."""
    lo, hi, fixed, free = _split(c["lo"], c["hi"], c["fixed"])
    jr = _wjac(p, c)[:, free]
    tw = int(np.count_nonzero(c["w"] > 0))
    sd = np.zeros(3)
    norms = np.linalg.norm(jr, axis=0)
    if tw <= free.size or not np.all(norms > 0):
        sd[free] = np.nan
        return sd, np.inf
    _, s, vt = np.linalg.svd(jr / norms, full_matrices=False)
    with np.errstate(divide="ignore", invalid="ignore"):
        sd[free] = np.sqrt(np.sum((vt.T / s) ** 2, axis=1)) / norms * np.sqrt(cost(p, c) / (tw - free.size))
        cond = float((s[0] / s[-1]) ** 2) if s[-1] > 0 else np.inf
    return sd, cond


def item(case, v, m):
    """The fit (voxel v, product m) of a case of `kinetic_case` as the dict the functions below take."""
    w = case["w"][v, m] if case["w"] is not None else np.ones(len(case["t"]))
    return {"S": case["S"][v], "Y": case["Y"][v, m], "w": w, "t": case["t"], "ths": case["ths"], "thp": case["thp"][m],
            "init": case["init"][m], "lo": case["lo"][m], "hi": case["hi"][m], "fixed": case["fixed"][m]}


# ---- the iteration ---------------------------------------------------------------------------------------------------
def lm_steps_kinetics(c, max_iter=200, ftol=1e-10, xtol=1e-10, solver="normal"):
    """The iteration of DESIGN.md section 8 restated for this model, exactly as tests/_basis_oracle.lm_steps_basis
    states it (lambda_0 = 1e-3, D_j the largest squared column norm so far, accept when the cost falls, lambda *=
    max(1/3, 1 - (2 rho - 1)^3) and nu = 2 on acceptance, lambda *= nu and nu *= 2 on rejection, the same stopping rules;
    `iters` counts trials), with status 3 (nothing done) when fewer points have weight than parameters are free.
    solver: "normal" or "qr" (least squares on the augmented Jacobian).

    Returns a dict: params [3], rss, iters, status, trials (list of (accepted, (F - Ft) / F)), path [3]."""
    lo, hi, fixed, free = _split(c["lo"], c["hi"], c["fixed"])
    P = free.size
    if np.count_nonzero(c["w"] > 0) < P:
        return {"params": np.zeros(3), "rss": np.nan, "iters": 0, "status": 3, "trials": [], "path": np.zeros(3)}
    v0, u = start_values(c["Y"], c["w"], c["thp"], c["init"], lo, hi, fixed)
    p, s = physical(u, v0, lo, hi, fixed)
    with np.errstate(all="ignore"):
        F = cost(p, c)
    dsc = np.zeros(P)
    lam, nu, it = 1e-3, 2.0, 0
    status = 1 if np.isfinite(F) else 2
    need_jac, trials, path = True, [], np.zeros(3)
    while status == 1 and it < max_iter:
        if need_jac:
            p, s = physical(u, v0, lo, hi, fixed)
            jr = _wjac(p, c)[:, free] * s[free]
            rr = _resid(p, c)
            H, g = jr.T @ jr, jr.T @ rr
            dsc = np.maximum(dsc, np.diag(H))
            need_jac = False
        it += 1
        D = np.where(dsc > 0, dsc, 1.0)
        try:
            with np.errstate(all="ignore"):
                if solver == "qr":
                    aug = np.concatenate([jr, np.diag(np.sqrt(lam * D))])
                    dl = np.linalg.lstsq(aug, np.concatenate([rr, np.zeros(P)]), rcond=None)[0]
                else:
                    dl = np.linalg.solve(H + lam * np.diag(D), g)
            ok = bool(np.all(np.isfinite(dl)))
        except np.linalg.LinAlgError:
            ok = False
        if not ok:
            trials.append((False, -np.inf))
            lam *= nu
            nu *= 2.0
            if not np.isfinite(lam):
                break
            continue
        dn = np.sqrt(np.sum(D * dl * dl))
        un = np.sqrt(np.sum(D * u * u))
        pred = float(dl @ (lam * D * dl + g))
        xconv = dn <= xtol * (un + xtol)
        ut = u + dl
        pt, _ = physical(ut, v0, lo, hi, fixed)
        with np.errstate(all="ignore"):
            Ft = cost(pt, c)
        margin = (F - Ft) / F if F > 0 and np.isfinite(Ft) else -np.inf
        if np.isfinite(Ft) and Ft < F:
            trials.append((True, margin))
            rho = min(max((F - Ft) / pred, 0.0), 1.0)
            fconv = (F - Ft) <= ftol * F
            path += np.abs(pt - p)
            u, F, p = ut, Ft, pt
            q = 2.0 * rho - 1.0
            lam *= max(1.0 / 3.0, 1.0 - q * q * q)
            nu = 2.0
            need_jac = True
            if fconv or xconv:
                status = 0
        else:
            trials.append((False, margin))
            lam *= nu
            nu *= 2.0
            if xconv:
                status = 0
            if not np.isfinite(lam):
                break
    p = physical(u, v0, lo, hi, fixed)[0]
    if not (np.all(np.isfinite(p)) and np.isfinite(F)):
        status = 2
    return {"params": p, "rss": F, "iters": it, "status": status, "trials": trials, "path": path}


def fit_scipy(c, tol=1e-14):
    """One item by scipy.optimize.least_squares (trust-region reflective, bounds on the physical parameters, analytic
    Jacobian).  Returns params [3], sd [3], rss, success."""
    lo, hi, fixed, free = _split(c["lo"], c["hi"], c["fixed"])
    v0, _ = start_values(c["Y"], c["w"], c["thp"], c["init"], lo, hi, fixed)

    def full(x):
        p = v0.copy()
        p[free] = x
        return p

    sol = least_squares(lambda x: _resid(full(x), c), v0[free], jac=lambda x: -_wjac(full(x), c)[:, free],
                        bounds=(lo[free], hi[free]), method="trf", x_scale="jac", xtol=tol, ftol=tol, gtol=tol,
                        max_nfev=2000)
    p = full(sol.x)
    return {"params": p, "sd": covariance_sd(p, c)[0], "rss": cost(p, c), "success": bool(sol.success) and sol.status > 0}


# ---- seeded cases ----------------------------------------------------------------------------------------------------
K_BOUNDS, RHO_BOUNDS = (0.0, 1.0), (1.0 / 60.0, 1.0 / 10.0)


def parameters(M, rho_free=True, z_free=False, k_start=0.02, rho_fixed=None):
    """(init, lo, hi, fixed) [M, 3]: k in [0, 1] from k_start; rho in [1/60, 1/10] from the middle, or fixed at
    rho_fixed [M]; z >= 0 from the automatic start (NaN), or fixed at 0."""
    init, lo, hi = np.zeros((M, 3)), np.zeros((M, 3)), np.zeros((M, 3))
    fixed = np.zeros((M, 3), bool)
    init[:, 0], lo[:, 0], hi[:, 0] = k_start, *K_BOUNDS
    lo[:, 1], hi[:, 1] = RHO_BOUNDS
    init[:, 1] = 0.5 * (RHO_BOUNDS[0] + RHO_BOUNDS[1]) if rho_free else rho_fixed
    fixed[:, 1] = not rho_free
    hi[:, 2] = np.inf
    init[:, 2] = np.nan if z_free else 0.0
    fixed[:, 2] = not z_free
    return init, lo, hi, fixed


def kinetic_case(T, M, seed, n_vox=2, noise=0.01, rho_free=True, z_free=False, uniform=True, flip_per_rep=False,
                 missing=0.0, sigma_weights=False):
    """Seeded case: times over min(2 (T - 1), 80) seconds (uniform, or each interval stretched by 0.6 ... 1.4), a
    gamma-variate substrate peaking at 100 after 8 s, products from the model at k in 0.01 ... 0.06, rho in 1/40 ... 1/15
    and (z_free) z in 2 ... 8, noise of `noise` times each trajectory's largest value on substrate and products, voxels
    that differ in amplitude (0.5 ... 2) and noise.  missing: the fraction of points with weight 0 (their samples NaN).
    sigma_weights: weights 1 / sigma, not 1.  Returns a dict: S [n_vox, T], Y, w [n_vox, M, T] (w None: all 1), t, ths
    [T], thp [M, T], truth [M, 3], init, lo, hi, fixed [M, 3]."""
    rng = np.random.default_rng([seed, T, M])
    span = min(2.0 * (T - 1), 80.0)
    D = np.full(T - 1, span / (T - 1))
    if not uniform:
        D = D * rng.uniform(0.6, 1.4, T - 1)
    t = np.concatenate([[0.0], np.cumsum(D)])
    ths = np.deg2rad(10.0) * (np.linspace(0.8, 1.6, T) if flip_per_rep else np.ones(T))
    thp = np.deg2rad(np.linspace(25.0, 15.0, M))[:, None] * (np.linspace(0.9, 1.3, T) if flip_per_rep else np.ones(T))
    truth = np.stack([rng.uniform(0.01, 0.06, M), rng.uniform(1 / 40, 1 / 15, M),
                      rng.uniform(2.0, 8.0, M) if z_free else np.zeros(M)], axis=1)
    tt = (t + 2.0) / 8.0
    mag = 100.0 * tt ** 2 * np.exp(2.0 * (1.0 - tt))
    S = np.zeros((n_vox, T))
    Y = np.zeros((n_vox, M, T))
    scale = rng.uniform(0.5, 2.0, n_vox)
    sig = np.zeros((n_vox, M))
    for v in range(n_vox):
        s0, _ = simulate(scale[v] * mag, t, ths, thp[0], 0.0, 0.1)
        for m in range(M):
            _, y = simulate(scale[v] * mag, t, ths, thp[m], truth[m, 0], truth[m, 1], scale[v] * truth[m, 2])
            sig[v, m] = noise * np.abs(y).max()
            Y[v, m] = y + sig[v, m] * rng.standard_normal(T)
        S[v] = s0 + noise * np.abs(s0).max() * rng.standard_normal(T)
    w = None
    if missing > 0 or sigma_weights:
        w = np.ones((n_vox, M, T)) / (np.where(sig > 0, sig, 1.0)[:, :, None] if sigma_weights else 1.0)
        if missing > 0:
            off = rng.random((n_vox, M, T)) < missing
            w[off] = 0.0
            Y[off] = np.nan
    init, lo, hi, fixed = parameters(M, rho_free, z_free, rho_fixed=truth[:, 1])
    return {"S": S, "Y": Y, "w": w, "t": t, "ths": ths, "thp": thp, "truth": truth, "init": init, "lo": lo, "hi": hi,
            "fixed": fixed, "T": T, "M": M}


T_LIST = (2, 3, 63, 64, 65, 129, 256)


def free_for(T):
    """(rho_free, z_free) of the cases at T repetitions: as many free parameters as T points can carry."""
    return (T >= 3, T >= 63)


def step_cases():
    """(name, kinetic_case arguments) of the cases on which the first trial steps are compared one by one: every lane
    and per-lane-count boundary, M = 1 and 4, uniform and stretched times, constant and per-repetition flip angles."""
    out = []
    for i, T in enumerate(T_LIST):
        rf, zf = free_for(T)
        out.append((f"T{T}_M{1 if i % 2 else 4}", dict(T=T, M=1 if i % 2 else 4, seed=70 + i, rho_free=rf, z_free=zf,
                                                       uniform=i % 3 != 1, flip_per_rep=i % 2 == 0)))
    return out


# ---- what xm_kinetics_fit must refuse before any HIP call (CPU and GPU tests share the list) -----------------------------
ABI_ORDER = ("substrate", "products", "weights", "n_batch", "M", "T", "times", "flip_s", "flip_p", "init", "lower",
             "upper", "fixed", "max_iter", "ftol", "xtol", "params", "param_sd", "rss", "status", "iters", "fit",
             "auc_ratio")
ABI_HOST = ("times", "flip_s", "flip_p", "init", "lower", "upper", "fixed")


def abi_ok(M=2, T=5):
    """A valid argument set with made-up device addresses (a refusal comes before any of them is touched)."""
    init, lo, hi, fixed = parameters(M, rho_fixed=np.full(M, 0.04))
    a = {"substrate": 1 << 20, "products": 2 << 20, "weights": 3 << 20, "n_batch": 3, "M": M, "T": T,
         "times": 2.0 * np.arange(T), "flip_s": np.full(T, 0.2), "flip_p": np.full((M, T), 0.4), "init": init,
         "lower": lo, "upper": hi, "fixed": fixed.astype(np.int32), "max_iter": 50, "ftol": 1e-10, "xtol": 1e-10}
    for i, k in enumerate(ABI_ORDER[16:]):
        a[k] = (4 + i) << 20
    return a


def _set(key, index, value):
    def change(a):
        v = np.array(a[key], dtype=np.float64 if key != "fixed" else np.int32)
        v[index] = value
        a[key] = v
    return change


def _many(*changes):
    def change(a):
        for c in changes:
            c(a)
    return change


def _shape(M, T):
    def change(a):
        a.update({k: v for k, v in abi_ok(M, T).items() if k in ABI_HOST or k in ("M", "T")})
    return change


REFUSALS = (
    ("T = 1", _shape(2, 1)), ("T = 257", _shape(2, 257)), ("M = 0", lambda a: a.update(M=0)), ("M = 9", _shape(9, 5)),
    ("n_batch < 0", lambda a: a.update(n_batch=-1)),
    ("equal times", _set("times", 2, 2.0)), ("decreasing times", _set("times", 4, 1.0)),
    ("NaN time", _set("times", 0, np.nan)), ("infinite time", _set("times", 4, np.inf)),
    ("substrate flip 0", _set("flip_s", 1, 0.0)), ("substrate flip pi/2", _set("flip_s", 1, np.pi / 2)),
    ("product flip negative", _set("flip_p", (1, 4), -0.1)), ("product flip NaN", _set("flip_p", (0, 0), np.nan)),
    ("NaN lower bound", _set("lower", (0, 0), np.nan)), ("NaN upper bound", _set("upper", (1, 2), np.nan)),
    ("lower > upper", _set("lower", (1, 0), 2.0)),
    ("infinite bound of a free k", _set("upper", (0, 0), np.inf)),
    ("infinite bound of a free rho", _set("upper", (1, 1), np.inf)),
    ("infinite lower bound of a free k", _set("lower", (0, 0), -np.inf)),
    ("negative lower bound of rho", _set("lower", (0, 1), -0.01)),
    ("negative lower bound of a fixed rho", _many(_set("lower", (0, 1), -0.01), _set("fixed", (0, 1), 1))),
    ("infinite start", _set("init", (0, 0), np.inf)), ("NaN start of k", _set("init", (1, 0), np.nan)),
    ("NaN start of a fixed z", _many(_set("init", (0, 2), np.nan), _set("fixed", (0, 2), 1))),
    ("every parameter fixed", _set("fixed", (1, slice(None)), 1)),
    ("max_iter = 0", lambda a: a.update(max_iter=0)), ("negative ftol", lambda a: a.update(ftol=-1.0)),
    ("NaN xtol", lambda a: a.update(xtol=np.nan)),
    ("null substrate", lambda a: a.update(substrate=0)), ("null products", lambda a: a.update(products=0)),
    ("null params", lambda a: a.update(params=0)), ("null param_sd", lambda a: a.update(param_sd=0)),
    ("null rss", lambda a: a.update(rss=0)), ("null status", lambda a: a.update(status=0)),
    ("null iters", lambda a: a.update(iters=0)), ("null auc_ratio", lambda a: a.update(auc_ratio=0)),
    ("null times", lambda a: a.update(times=None)), ("null fixed", lambda a: a.update(fixed=None)),
)


def abi_arguments(a, stream=0):
    """The positional arguments of xm_kinetics_fit for the dict `a`, and the host arrays they point into."""
    keep, args = [], []
    for k in ABI_ORDER:
        v = a[k]
        if k in ABI_HOST and v is not None:
            v = np.ascontiguousarray(v, dtype=np.int32 if k == "fixed" else np.float64)
            keep.append(v)
            v = v.ctypes.data
        args.append(v if v != 0 or k in ("n_batch", "M", "T", "max_iter", "ftol", "xtol") else None)
    return args + [stream], keep
