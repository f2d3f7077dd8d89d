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
