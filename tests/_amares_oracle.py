"""Independent numpy / scipy statement of the AMARES estimator of DESIGN.md ("Quantification: AMARES"), the yardstick
of the HIP kernel.  It does not import xmris_amd: the prior knowledge comes in as plain arrays.

Parameters of a peak, in fitting units: amplitude a, frequency f [Hz], damping d [1/s], phase phi [rad], lineshape g.
Model: x^(t) = sum_k a_k e^{i phi_k} exp(-d_k (1 - g_k + g_k t) t) e^{i 2 pi f_k t}.
Bounds: lmfit's transforms to an internal variable u; fit: MINPACK lmder (scipy.optimize.leastsq) in u with the analytic
Jacobian; CRLB / SNR from the physical Jacobian at the solution.
"""
import numpy as np
from scipy.optimize import leastsq

NAMES = ("amplitude", "frequency", "damping", "phase", "g")


def model(params, t):
    """params [K, 5] -> complex128 FID at times t."""
    p = np.asarray(params, dtype=np.float64).reshape(-1, 5)
    a, f, d, ph, g = (p[:, c] for c in range(5))
    tc = np.asarray(t, dtype=np.float64)[:, None]
    return np.sum(a * np.exp(-d * (1.0 - g + g * tc) * tc) * np.exp(1j * (ph + 2.0 * np.pi * f * tc)), axis=1)


def model_jacobian(params, t):
    """d model / d params: complex [n, K*5] (column 5k + c)."""
    p = np.asarray(params, dtype=np.float64).reshape(-1, 5)
    tc = np.asarray(t, dtype=np.float64)[:, None]
    a, f, d, ph, g = (p[:, c] for c in range(5))
    base = np.exp(-d * (1.0 - g + g * tc) * tc) * np.exp(1j * (ph + 2.0 * np.pi * f * tc))
    term = a * base
    cols = np.stack([base, 2j * np.pi * tc * term, -(1.0 - g + g * tc) * tc * term, 1j * term,
                     d * tc * (1.0 - tc) * term], axis=2)
    return cols.reshape(len(tc), -1)


# ---- lmfit's bound transforms ------------------------------------------------------------------------------------------
def to_internal(v, lo, hi):
    if np.isfinite(lo) and np.isfinite(hi):
        return float(np.arcsin(np.clip(2.0 * (v - lo) / (hi - lo) - 1.0, -1.0, 1.0)))
    if np.isfinite(lo):
        return float(np.sqrt((v - lo + 1.0) ** 2 - 1.0))
    if np.isfinite(hi):
        return float(np.sqrt((hi - v + 1.0) ** 2 - 1.0))
    return float(v)


def from_internal(u, lo, hi):
    """(p, dp/du).  On a two-sided bound (sin u = +-1) the slope is exactly zero."""
    if np.isfinite(lo) and np.isfinite(hi):
        s = np.sin(u)
        slope = 0.0 if abs(s) == 1.0 else np.cos(u) * (hi - lo) / 2.0
        return lo + (s + 1.0) * (hi - lo) / 2.0, slope
    if np.isfinite(lo):
        r = np.sqrt(u * u + 1.0)
        return lo - 1.0 + r, u / r
    if np.isfinite(hi):
        r = np.sqrt(u * u + 1.0)
        return hi + 1.0 - r, -u / r
    return u, 1.0


def fit(x, t, init, lo, hi, fixed=None, xtol=1e-12, ftol=1e-12, maxfev=4000):
    """One voxel.  init / lo / hi / fixed: [K, 5] in fitting units.  Returns a dict with params [K, 5], sd [K, 5]
    (square roots of the diagonal of sigma^2 (J^T J)^{-1}, 0 for fixed parameters), rss, sigma, crlb [K], snr [K]."""
    x = np.asarray(x, dtype=np.complex128)
    t = np.asarray(t, dtype=np.float64)
    init, lo, hi = (np.asarray(v, dtype=np.float64).ravel() for v in (init, lo, hi))
    fixed = np.zeros(init.size, bool) if fixed is None else np.asarray(fixed, bool).ravel()
    fixed = fixed | (lo == hi)
    v0 = np.clip(init, lo, hi)
    free = np.flatnonzero(~fixed)

    def physical(u):
        p, s = v0.copy(), np.zeros(v0.size)
        for j, q in enumerate(free):
            p[q], s[q] = from_internal(u[j], lo[q], hi[q])
        return p, s

    def fun(u):
        r = x - model(physical(u)[0], t)
        return np.concatenate([r.real, r.imag])

    def jac(u):
        p, s = physical(u)
        jm = model_jacobian(p, t)[:, free] * s[free]
        return -np.concatenate([jm.real, jm.imag])

    u0 = np.array([to_internal(v0[q], lo[q], hi[q]) for q in free])
    u, _, _, _, ier = leastsq(fun, u0, Dfun=jac, full_output=True, xtol=xtol, ftol=ftol, maxfev=maxfev)
    p = physical(u)[0]
    r = fun(u)
    rss = float(r @ r)
    n2 = 2 * len(t)
    sigma = np.sqrt(rss / (n2 - free.size))
    jm = model_jacobian(p, t)[:, free]
    jr = np.concatenate([jm.real, jm.imag])
    cov = sigma ** 2 * np.linalg.inv(jr.T @ jr)
    sd = np.zeros(init.size)
    sd[free] = np.sqrt(np.diag(cov))
    P, SD = p.reshape(-1, 5), sd.reshape(-1, 5)
    a = P[:, 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        crlb = np.where(a != 0, 100.0 * SD[:, 0] / np.abs(a), 0.0)
    return {"params": P, "sd": SD, "rss": rss, "sigma": sigma, "crlb": crlb, "snr": a / sigma, "ier": ier}


# ---- the notebook's dataset and prior knowledge (docs/notebooks/fitting/pyamares.md:85-154) --------------------------
def notebook_dataset():
    """5 voxels x 1024 points, sw 10 kHz, 120 MHz: PCr (0 ppm, 15 Hz, amplitude 10 ... 50) + ATP (-7.5 ppm, 20 Hz, 5),
    noise sigma 0.5 per channel from default_rng(42).  Returns (data [5, 1024] complex128, time, mhz)."""
    n, sw, mhz = 1024, 10000.0, 120.0
    t = np.arange(n) / sw
    rng = np.random.default_rng(seed=42)
    data = np.zeros((5, n), dtype=complex)
    for v in range(5):
        sig = 10.0 * (v + 1) * np.exp(-15.0 * np.pi * t) + 5.0 * np.exp(-20.0 * np.pi * t) * np.exp(
            1j * 2 * np.pi * (-7.5 * mhz) * t)
        data[v] = sig + rng.normal(0, 0.5, n) + 1j * rng.normal(0, 0.5, n)
    return data, t, mhz


def notebook_pk(mhz):
    """(init, lo, hi) [2, 5] in fitting units for the notebook's PCr / ATP prior knowledge."""
    deg = np.pi / 180.0
    init = np.array([[10.0, 0.0 * mhz, 15.0 * np.pi, 0.0, 0.0], [5.0, -7.5 * mhz, 20.0 * np.pi, 0.0, 0.0]])
    lo = np.array([[0.0, -0.5 * mhz, 5.0 * np.pi, -180 * deg, 0.0], [0.0, -8.0 * mhz, 10.0 * np.pi, -180 * deg, 0.0]])
    hi = np.array([[np.inf, 0.5 * mhz, 30.0 * np.pi, 180 * deg, 1.0], [np.inf, -7.0 * mhz, 40.0 * np.pi, 180 * deg, 1.0]])
    return init, lo, hi


# ---- a 31P-like MRSI workload: PCr, Pi, gamma-, alpha-, beta-ATP ---------------------------------------------------
P31_NAMES = ("PCr", "Pi", "gATP", "aATP", "bATP")
P31_PPM = (0.0, 4.9, -2.5, -7.5, -16.2)
P31_LW = (12.0, 18.0, 25.0, 25.0, 30.0)
P31_AMP = (20.0, 6.0, 8.0, 8.0, 6.0)


def p31_pk_csv() -> str:
    """Prior knowledge of the workload in the notebook's CSV layout (g starts on its bound: held at 0)."""
    cols = ",".join(P31_NAMES)
    row = lambda name, vals: f"{name}," + ",".join(vals)  # noqa: E731
    lines = [f"Index,{cols}", "Initial Values" + "," * len(P31_NAMES),
             row("amplitude", [str(a) for a in P31_AMP]), row("chemicalshift", [str(c) for c in P31_PPM]),
             row("linewidth", [str(w) for w in P31_LW]), row("phase", ["0"] * 5), row("g", ["0"] * 5),
             "Bounds" + "," * len(P31_NAMES), row("amplitude", ['"(0, "'] * 5),
             row("chemicalshift", [f'"({c - 0.4}, {c + 0.4})"' for c in P31_PPM]),
             row("linewidth", ['"(4, 60)"'] * 5), row("phase", ['"(-180, 180)"'] * 5), row("g", ['"(0, 1)"'] * 5)]
    return "\n".join(lines) + "\n"


def p31_pk(mhz):
    """(init, lo, hi) [5, 5] in fitting units, the same prior knowledge as p31_pk_csv()."""
    deg = np.pi / 180.0
    ppm = np.array(P31_PPM)
    init = np.stack([np.array(P31_AMP), ppm * mhz, np.array(P31_LW) * np.pi, np.zeros(5), np.zeros(5)], axis=1)
    lo = np.stack([np.zeros(5), (ppm - 0.4) * mhz, np.full(5, 4 * np.pi), np.full(5, -180 * deg), np.zeros(5)], axis=1)
    hi = np.stack([np.full(5, np.inf), (ppm + 0.4) * mhz, np.full(5, 60 * np.pi), np.full(5, 180 * deg), np.ones(5)],
                  axis=1)
    return init, lo, hi


def p31_workload(n_vox, n=2048, sw=10000.0, mhz=120.0, seed=0, noise=0.5):
    """Seeded per-voxel truth around the prior knowledge: (data [n_vox, n] complex128, truth [n_vox, 5, 5], t)."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / sw
    truth = np.zeros((n_vox, 5, 5))
    truth[:, :, 0] = np.array(P31_AMP) * rng.uniform(0.6, 1.4, (n_vox, 5))
    truth[:, :, 1] = (np.array(P31_PPM) + rng.uniform(-0.15, 0.15, (n_vox, 5))) * mhz
    truth[:, :, 2] = np.array(P31_LW) * rng.uniform(0.8, 1.2, (n_vox, 5)) * np.pi
    truth[:, :, 3] = rng.uniform(-0.3, 0.3, (n_vox, 1))
    data = np.stack([model(truth[v], t) for v in range(n_vox)])
    data = data + noise * (rng.standard_normal(data.shape) + 1j * rng.standard_normal(data.shape))
    return data, truth, t


# ---- pieces that judge the kernel away from the converged solution (tests/test_amares_kernel.py) ---------------------
def _split(lo, hi, fixed, init=None):
    lo, hi = (np.asarray(v, dtype=np.float64).ravel() for v in (lo, hi))
    fixed = np.zeros(lo.size, bool) if fixed is None else np.asarray(fixed, bool).ravel()
    fixed = fixed | (lo == hi)
    return lo, hi, fixed, np.flatnonzero(~fixed)


def real_rows(z):
    """complex [n, ...] -> real [2n, ...]: real parts, then imaginary parts (the 2n real residuals of n points)."""
    return np.concatenate([z.real, z.imag])


def start_values(init, lo, hi, fixed=None):
    """(v0, u0): the start clipped into the bounds (all 5K parameters) and the internal start of the free ones."""
    lo, hi, fixed, free = _split(lo, hi, fixed)
    v0 = np.clip(np.asarray(init, dtype=np.float64).ravel(), lo, hi)
    return v0, np.array([to_internal(v0[q], lo[q], hi[q]) for q in free])


def physical(u, v0, lo, hi, fixed=None):
    """(p, s): all 5K physical values and slopes dp/du at the internal vector u; fixed parameters keep v0, slope 0."""
    lo, hi, fixed, free = _split(lo, hi, fixed)
    p, s = np.array(v0, dtype=np.float64).ravel().copy(), np.zeros(lo.size)
    for j, q in enumerate(free):
        p[q], s[q] = from_internal(u[j], lo[q], hi[q])
    return p, s


def _normal(x, t, p, scale, free):
    jr = real_rows(model_jacobian(p, t)[:, free] * scale)
    r = real_rows(np.asarray(x, dtype=np.complex128) - model(p, t))
    return jr.T @ jr, jr.T @ r, float(r @ r), jr, r


def normal_equations(x, t, params, lo, hi, fixed=None, internal=False):
    """(H, g, F) at the physical point `params` over the free columns: H = J^T J, g = J^T r, F = |r|^2 with
    r = x - model (2n real residuals) and J = d model / d parameter -- so that the Gauss-Newton step solves H delta = g.
    internal: J with respect to the internal variables, i.e. chained through from_internal's slope at
    u = to_internal(params)."""
    lo, hi, fixed, free = _split(lo, hi, fixed)
    p = np.asarray(params, dtype=np.float64).ravel()
    scale = np.ones(free.size)
    if internal:
        scale = np.array([from_internal(to_internal(p[q], lo[q], hi[q]), lo[q], hi[q])[1] for q in free])
    return _normal(x, t, p, scale, free)[:3]


def amplitude_sd(t, params, lo, hi, fixed=None):
    """(sd [K], cond): sqrt(diag((J^T J)^{-1})) of the amplitudes over the physical free columns at `params` (0 for a
    fixed amplitude), from an SVD of the column-scaled Jacobian, and the 2-norm condition number of the unscaled
    J^T J (what the kernel factors)."""
    lo, hi, fixed, free = _split(lo, hi, fixed)
    jr = real_rows(model_jacobian(params, t)[:, free])
    sv = np.linalg.svd(jr, compute_uv=False)
    with np.errstate(divide="ignore"):
        cond = float((sv[0] / sv[-1]) ** 2) if sv[-1] > 0 else np.inf
    c = np.linalg.norm(jr, axis=0)
    sd = np.zeros(lo.size)
    if np.all(c > 0):
        _, s, vt = np.linalg.svd(jr / c, full_matrices=False)
        with np.errstate(divide="ignore", invalid="ignore"):
            sd[free] = np.sqrt(np.sum((vt.T / s) ** 2, axis=1)) / c
    else:
        sd[free] = np.nan
    return sd.reshape(-1, 5)[:, 0], cond


def lm_steps(x, t, init, lo, hi, fixed=None, max_iter=200, ftol=1e-10, xtol=1e-10, solver="normal"):
    """The iteration of DESIGN.md section 8, restated: Levenberg-Marquardt in the internal variables from the clipped
    start; lambda_0 = 1e-3; D_j the largest squared column norm so far (1 for an always-zero column); a trial solves
    (H + lambda D) delta = g; accepted when the cost falls, then lambda *= max(1/3, 1 - (2 rho - 1)^3), nu = 2;
    rejected (also when the system cannot be solved): lambda *= nu, nu *= 2.  Stops: |sqrt(D) delta| <=
    xtol (|sqrt(D) u| + xtol) (tested on every trial), or an accepted step reduces the cost by <= ftol relative; the
    trial cap leaves status 1.  `iters` counts trials.

    solver: "normal" -- numpy.linalg.solve on the fp64 normal equations; "qr" -- least squares (LAPACK, orthogonal
    factorisation) on the augmented Jacobian [J; sqrt(lambda D)], which never forms J^T J.

    Returns a dict: params [K, 5], u, rss, iters, status, trials (list of (accepted, (F - Ft) / F)), path [5K] (the sum
    of |change| of every parameter over the accepted steps: the scale in which two trajectories are compared)."""
    x = np.asarray(x, dtype=np.complex128)
    t = np.asarray(t, dtype=np.float64)
    lo, hi, fixed, free = _split(lo, hi, fixed)
    v0, u = start_values(init, lo, hi, fixed)
    P = free.size
    p, s = physical(u, v0, lo, hi, fixed)
    r = x - model(p, t)
    F = float(np.sum(r.real ** 2 + r.imag ** 2))
    dsc = np.zeros(P)
    lam, nu, it = 1e-3, 2.0, 0
    status = 1 if np.isfinite(F) else 2
    need_jac, trials, path = True, [], np.zeros(lo.size)
    while status == 1 and it < max_iter:
        if need_jac:
            p, s = physical(u, v0, lo, hi, fixed)
            H, g, _, jr, rr = _normal(x, t, p, s[free], free)
            dsc = np.maximum(dsc, np.diag(H))
            need_jac = False
        it += 1
        D = np.where(dsc > 0, dsc, 1.0)
        try:
            with np.errstate(all="ignore"):
                if solver == "qr":
                    a = np.concatenate([jr, np.diag(np.sqrt(lam * D))])
                    dl = np.linalg.lstsq(a, np.concatenate([rr, np.zeros(P)]), rcond=None)[0]
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
            rt = x - model(pt, t)
            Ft = float(np.sum(rt.real ** 2 + rt.imag ** 2))
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
    return {"params": p.reshape(-1, 5), "u": u, "rss": F, "iters": it, "status": status, "trials": trials,
            "path": path}


def kernel_case(K, n, seed, dt=1e-4, t0=5e-4, noise=0.2, n_vox=1, fix_g=False, fix_phase=False, on_bound=()):
    """Seeded K well-separated Voigt peaks with dead time and noise, a start perturbed away from the truth and bounds
    of all four types: amplitude lower-only (0, inf); frequency two-sided (+-60 Hz); damping upper-only (-inf, 400) on
    even peaks and lower-only (2, inf) on odd ones; phase unbounded on even peaks and two-sided (-pi, pi) on odd ones;
    g two-sided (0, 1).  n_vox voxels share truth and prior knowledge and differ in their noise.
    fix_g: g held through fixed[] at its start value; fix_phase: phases held through lo == hi.
    on_bound: (peak, column, "lo" | "hi") triples whose start value is put exactly on that bound.
    Only cases whose J^T J (physical, at the truth) has 64 eps cond <= 1e-4 are emitted: a seed that misses is
    re-drawn deterministically.  Records shorter than 25 ms cannot meet that (the peaks have hardly decayed: cond is
    4e10 at K = 1, n = 80) and are emitted as drawn.  Returns a dict: x [n_vox, n] complex128, t, dt, t0, truth, init, lo, hi, fixed [K, 5]."""
    t = np.arange(n) * dt + t0
    for attempt in range(50):
        rng = np.random.default_rng([seed, K, n, attempt])
        truth = np.zeros((K, 5))
        truth[:, 0] = rng.uniform(5.0, 20.0, K)
        centre = np.linspace(-3500.0, 3500.0, K) if K > 1 else np.zeros(1)
        truth[:, 1] = centre + rng.uniform(-20.0, 20.0, K)
        truth[:, 2] = rng.uniform(30.0, 90.0, K)
        truth[:, 3] = rng.uniform(-0.5, 0.5, K)
        truth[:, 4] = rng.uniform(0.2, 0.8, K)
        init = truth.copy()
        init[:, 0] *= rng.uniform(0.8, 1.2, K)
        init[:, 1] += rng.uniform(-4.0, 4.0, K)
        init[:, 2] *= rng.uniform(0.85, 1.15, K)
        init[:, 3] += rng.uniform(-0.2, 0.2, K)
        init[:, 4] = np.clip(truth[:, 4] + rng.uniform(-0.15, 0.15, K), 0.1, 0.9)
        lo, hi = np.full((K, 5), -np.inf), np.full((K, 5), np.inf)
        lo[:, 0] = 0.0
        lo[:, 1], hi[:, 1] = centre - 60.0, centre + 60.0
        hi[0::2, 2] = 400.0
        lo[1::2, 2] = 2.0
        lo[1::2, 3], hi[1::2, 3] = -np.pi, np.pi
        lo[:, 4], hi[:, 4] = 0.0, 1.0
        fixed = np.zeros((K, 5), bool)
        if fix_g:
            fixed[:, 4] = True
            init[:, 4] = truth[:, 4]
        if fix_phase:
            lo[:, 3] = hi[:, 3] = init[:, 3] = truth[:, 3]
        for k, c, side in on_bound:
            init[k, c] = lo[k, c] if side == "lo" else hi[k, c]
        z = rng.standard_normal((n_vox, n)) + 1j * rng.standard_normal((n_vox, n))
        x = model(truth, t)[None] + noise * z
        if n * dt < 0.025 or 64 * np.finfo(np.float64).eps * amplitude_sd(t, truth, lo, hi, fixed)[1] <= 1e-4:
            break
    else:
        raise RuntimeError(f"kernel_case({K}, {n}, {seed}): no well-conditioned draw")
    return {"x": x, "t": t, "dt": dt, "t0": t0, "truth": truth, "init": init, "lo": lo, "hi": hi, "fixed": fixed}


def step_cases():
    """(name, kernel_case arguments) of the cases on which the first trial steps are compared one by one: every staging
    tier at a ragged record length, and two 2-peak cases in which parameters of every bounded type start exactly on a
    bound (the others start inside)."""
    return [
        ("K1_n257", dict(K=1, n=257, seed=31, n_vox=2)),
        ("K6_n1000", dict(K=6, n=1000, seed=32, n_vox=2)),
        ("K7_n1000", dict(K=7, n=1000, seed=33, n_vox=2)),
        ("K13_n1500", dict(K=13, n=1500, seed=34, n_vox=2)),
        ("K16_n3001", dict(K=16, n=3001, seed=35, n_vox=2)),
        ("K16_fixed_g_n1000", dict(K=16, n=1000, seed=36, n_vox=2, fix_g=True)),
        # frequency (two-sided) on hi, damping (upper only) on hi, phase (two-sided) on lo, g (two-sided) on lo
        ("K2_on_bound_a", dict(K=2, n=700, seed=37, n_vox=2,
                               on_bound=((1, 1, "hi"), (0, 2, "hi"), (1, 3, "lo"), (0, 4, "lo")))),
        # amplitude (lower only) on lo, damping (lower only) on lo, g (two-sided) on hi
        ("K2_on_bound_b", dict(K=2, n=700, seed=38, n_vox=2, on_bound=((0, 0, "lo"), (1, 2, "lo"), (1, 4, "hi")))),
    ]
