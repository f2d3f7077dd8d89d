"""numpy restatement of the alignment definition, the oracle of tests/test_align.py and
tests/test_gpu_align.py.  Two routes to f*: the safeguarded Newton iteration of the definition in fp64, and
``scipy.optimize.brentq`` on P' over the same bracket with every sum (and every phase) in ``np.longdouble``."""
import numpy as np

EPS = np.finfo(np.float64).eps
STEPS = 40
LD = np.longdouble


def grid(L, dt, max_shift):
    delta = 1.0 / (4.0 * L * dt)
    return delta, (int(np.floor(max_shift / delta)) if L >= 2 else 0)


PI_LD = LD("3.14159265358979323846264338327950288")


def _split(a):
    c = 134217729.0 * a  # Veltkamp: 2^27 + 1
    hi = c - (c - a)
    return hi, a - hi


def frac_turns(f, tau):
    """f tau minus its nearest integer, from the exact product (Dekker), rounded once: what fma(f, tau, -k) gives."""
    p = f * tau
    fh, fl = _split(np.float64(f))
    th, tl = _split(tau)
    err = ((fh * th - p) + fh * tl + fl * th) + fl * tl
    return (p - np.rint(p)) + err


def _sums(z, tau, f, ld=False):
    """C, S1, S2 at f (S_k = sum tau^k z e^{-2 pi i f tau}); fp64 with the turn count reduced, or long double."""
    if ld:
        zz, tt = z.astype(np.clongdouble), tau.astype(LD)
        turns = LD(f) * tt
        a = 2 * PI_LD * (turns - np.rint(turns))
        u = zz * (np.cos(a) - 1j * np.sin(a))
        return u.sum(), (tt * u).sum(), (tt * tt * u).sum()
    a = 2.0 * np.pi * frac_turns(f, tau)
    u = z * (np.cos(a) - 1j * np.sin(a))
    return u.sum(), (tau * u).sum(), (tau * tau * u).sum()


def _d1(c, s1):
    return (np.conj(c) * s1).imag  # P' / 4 pi


def _d2(c, s1, s2):
    return abs(s1) ** 2 - (np.conj(c) * s2).real  # P'' / 8 pi^2


def align(x, r, dt, t0=0.0, max_shift=20.0, L=None, route="newton"):
    """One transient.  dict(y, shift, phase, quality, status) and what the tests scale their bounds with: u_f, u_phi,
    u_q (units of rounding), margin, one_sign_change, g, delta, tau."""
    x = np.asarray(x, dtype=np.complex128)
    r = np.asarray(r, dtype=np.complex128)
    N = x.shape[0]
    L = min(N, r.shape[0]) if L is None else L
    tau = t0 + np.arange(N) * dt
    out = dict(y=np.zeros(N, complex), shift=np.nan, phase=np.nan, quality=np.nan, status=2, u_f=np.nan, u_phi=np.nan,
               u_q=np.nan, margin=np.nan, one_sign_change=False, g=0, tau=tau)
    xl, rl, tl = x[:L], r[:L], tau[:L]
    delta, G = grid(L, dt, max_shift)
    out["delta"] = delta
    with np.errstate(all="ignore"):
        z = rl * np.conj(xl)
        nr2, nx2 = float(np.sum(np.abs(rl) ** 2)), float(np.sum(np.abs(xl) ** 2))
        gs = np.arange(-G, G + 1)
        P = np.array([abs(_sums(z, tl, g * delta)[0]) ** 2 for g in gs])
    if not (np.all(np.isfinite(xl)) and np.all(np.isfinite(rl)) and np.isfinite(nr2) and np.isfinite(nx2)
            and np.all(np.isfinite(P))):
        return out
    order = np.argsort(np.abs(gs) * 2 + (gs > 0), kind="stable")  # 0, -1, +1, -2, +2, ...
    g = int(gs[order][np.argmax(P[order])])
    out["g"] = g
    if not P[g + G] > 0.0:
        out.update(y=x.copy(), shift=0.0, phase=0.0, quality=0.0, status=3)
        return out
    far = np.abs(gs - g) > 2
    out["margin"] = 1.0 - (P[far].max() / P[g + G] if far.any() else 0.0)
    status, f = 0, g * delta
    a, b = max((g - 1) * delta, -max_shift), min((g + 1) * delta, max_shift)
    ld = route == "brentq"
    d1_at = lambda ff: float(_d1(*_sums(z, tl, ff, ld)[:2]))  # noqa: E731
    out["one_sign_change"] = G == 0  # (no bracket: f* = 0)
    if G > 0:
        sub = np.array([d1_at(v) for v in np.linspace(a, b, 64)])
        sg = np.sign(sub[sub != 0])
        out["one_sign_change"] = bool(np.count_nonzero(sg[1:] != sg[:-1]) == 1 and sg[0] > 0)
        refine = True
        if abs(g) == G:
            e = max_shift if g > 0 else -max_shift
            d1 = d1_at(e)
            if (d1 > 0) if g > 0 else (d1 < 0):
                status, f, refine = 1, e, False
        if refine and route == "brentq":
            from scipy.optimize import brentq

            f = float(brentq(d1_at, a, b, xtol=1e-300, rtol=4 * EPS, maxiter=200)) if d1_at(a) * d1_at(b) < 0 else np.nan
        elif refine:
            tol, status = delta * 2.0 ** -40, 4
            for _ in range(STEPS):
                c, s1, s2 = _sums(z, tl, f)
                d1, d2 = _d1(c, s1), _d2(c, s1, s2)
                if d1 > 0:
                    a = f
                elif d1 < 0:
                    b = f
                else:
                    status = 0
                    break
                fn = f - d1 / (2.0 * np.pi * d2) if d2 < 0 else np.nan
                if not (a <= fn <= b):
                    fn = 0.5 * (a + b)
                step, f = abs(fn - f), fn
                if step <= tol:
                    status = 0
                    break
    c, s1, s2 = _sums(z, tl, f, ld)
    phi = float(np.arctan2(c.imag, c.real))
    az = np.abs(z)
    sa, sat = float(az.sum()), float((az * np.abs(tl)).sum())
    p2 = abs(float(_d2(c, s1, s2))) * 8 * np.pi ** 2
    u_f = EPS * sa * 4 * np.pi * sat / p2 if p2 > 0 else 0.0
    u_phi = EPS * sa / abs(c) + 2 * np.pi * (sat / sa) * u_f
    q = float(abs(c)) / (np.sqrt(nr2) * np.sqrt(nx2))
    ang = 2 * PI_LD * (LD(f) * tau.astype(LD)) + LD(phi)
    y = (x.astype(np.clongdouble) * (np.cos(ang) + 1j * np.sin(ang))).astype(np.complex128)
    out.update(y=y, shift=float(f), phase=phi, quality=q, status=status, u_f=u_f, u_phi=u_phi,
               u_q=EPS * (sa / (np.sqrt(nr2) * np.sqrt(nx2)) + q))
    return out


KEYS = ("shift", "phase", "quality", "status", "u_f", "u_phi", "u_q", "margin", "one_sign_change", "g")


def align_batch(x, ref, dt, t0=0.0, max_shift=20.0, L=None, route="newton"):
    """x (n_outer, A, n_inner, N), ref (n_outer, n_inner, N_r) or (N_r,): per-transient arrays (n_outer, A, n_inner)."""
    no, A, ni, N = x.shape
    res = {k: np.empty((no, A, ni), dtype=int if k in ("status", "g") else bool if k == "one_sign_change" else float)
           for k in KEYS}
    res["y"] = np.empty(x.shape, complex)
    for o in range(no):
        for a in range(A):
            for i in range(ni):
                one = align(x[o, a, i], ref if ref.ndim == 1 else ref[o, i], dt, t0, max_shift, L, route)
                res["y"][o, a, i] = one["y"]
                for k in KEYS:
                    res[k][o, a, i] = one[k]
    return res


def average(y, status, quality, min_quality=0.0):
    """Ordered mean over the average axis (axis 1) of the y with status != 2 and quality >= min_quality."""
    no, A, ni, N = y.shape
    s = np.zeros((no, ni, N), complex)
    n = np.zeros((no, ni), int)
    for a in range(A):
        keep = (status[:, a] != 2) & (quality[:, a] >= min_quality)
        s[keep] = s[keep] + y[:, a][keep]
        n += keep
    d = np.where(n > 0, n, 1)[..., None]
    return (s.real / d) + 1j * (s.imag / d), n


def make_data(n_outer, A, n_inner, N, seed, dt=5e-4, max_shift=20.0, snr=(2.0, 10.0), clean=False):
    """(x, ref): per voxel a two-peak damped FID r (N points, times t dt); every transient is r shifted by a frequency
    drawn from +-0.6 max_shift and turned by a phase from +-pi, plus complex noise at a per-sample SNR (rms of the
    signal over the noise's standard deviation) drawn from `snr`."""
    rng = np.random.default_rng(seed)
    t = np.arange(N) * dt
    T = max(N, 16) * dt
    vox = (n_outer, 1, n_inner, 1)
    f1, f2 = rng.uniform(2, 6, vox) / T, rng.uniform(-9, -4, vox) / T
    r = np.exp((-2.0 / T + 2j * np.pi * f1) * t) + 0.6 * np.exp((-3.0 / T + 2j * np.pi * f2) * t + 0.7j)
    per = (n_outer, A, n_inner, 1)
    fs, ph = rng.uniform(-0.6, 0.6, per) * max_shift, rng.uniform(-np.pi, np.pi, per)
    sig = r * np.exp(1j * (2 * np.pi * fs * t + ph))
    rms = np.sqrt(np.mean(np.abs(sig) ** 2, axis=3, keepdims=True))
    noise = (rng.standard_normal(sig.shape) + 1j * rng.standard_normal(sig.shape)) / np.sqrt(2.0)
    x = sig if clean else sig + rms / rng.uniform(snr[0], snr[1], per) * noise
    return x, r[:, 0], fs[..., 0], ph[..., 0]


DT = 5e-4


def shift_for(G, L, dt=DT):
    """A max_shift in the middle of the range that gives G grid points each side."""
    return (G + 0.5) / (4.0 * L * dt)


# name -> (n_outer, A, n_inner, N, L, G): N = 1, 2, 33, 64, 255, 256, 257, 2048; L = N and N / 2; A = 1, 2, 5, 37;
# n_inner 1, 3; n_outer 1, 4; G = 0, 1, about 16 (two coarse rounds and a tail), and the cap 512 (4 L > 1024, so that
# the grid stays inside one period 1 / dt of P)
PARITY_CASES = {
    "n1_a2": (1, 2, 1, 1, 1, 16),
    "n2_a5": (1, 5, 1, 2, 2, 1),
    "n33_a37_g0": (1, 37, 1, 33, 33, 0),
    "n33_a5_inner3": (1, 5, 3, 33, 33, 1),
    "n64_a5_half": (4, 5, 1, 64, 32, 1),
    "n255_a2_outer4": (4, 2, 3, 255, 255, 16),
    "n256_a37": (1, 37, 1, 256, 256, 16),
    "n256_a1_half": (1, 1, 3, 256, 128, 13),
    "n257_a5": (1, 5, 1, 257, 257, 17),
    "n2048_a5": (1, 5, 1, 2048, 2048, 16),
    "n2048_a2_half": (1, 2, 1, 2048, 1024, 16),
    "n2048_a2_cap": (1, 2, 1, 2048, 1024, 512),
}


def parity_case(name):
    """(x, ref, dt, max_shift, L) of a parity case."""
    no, A, ni, N, L, G = PARITY_CASES[name]
    ms = shift_for(G, L)
    x, r, _, _ = make_data(no, A, ni, N, seed=2000 + sum(map(ord, name)), max_shift=ms)
    return x, r, DT, ms, L


def phase_gap(a, b):
    """|a - b| of two angles, the short way round."""
    return np.abs(np.angle(np.exp(1j * (np.asarray(a) - np.asarray(b)))))


def route_gap_units(a, b):
    """Largest disagreement of two results in f* (units of u_f) and phi* (units of u_phi); the worst transient."""
    uf = np.abs(a["shift"] - b["shift"]) / np.where(a["u_f"] > 0, a["u_f"], 1.0)
    up = phase_gap(a["phase"], b["phase"]) / a["u_phi"]
    return float(np.max(uf)), float(np.max(up))
