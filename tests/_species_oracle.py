"""numpy restatement of the species-separation definition, the oracle of tests/test_species.py and
tests/test_gpu_species.py.  Known field: the factorised estimate, and per-row ``numpy.linalg.lstsq`` on A_r.  Fitted
field: the grid, the tie rule and the safeguarded Newton iteration step by step in fp64, and ``scipy.optimize.brentq``
on G' over the same bracket as an independent route."""
import numpy as np

EPS = np.finfo(np.float64).eps
STEPS = 40
LD = np.longdouble
FREQS = (0.0, 390.0, -320.0, 185.0, 610.0, -150.0, 480.0, -560.0)  # Hz
DECAYS = (12.0, 30.0, 8.0, 20.0, 5.0, 40.0, 16.0, 25.0)  # 1/s


# ---- the model ----------------------------------------------------------------------------------------------------------
def a0(te, f, r):
    return np.exp((2j * np.pi * np.asarray(f) - np.asarray(r))[None, :] * np.asarray(te)[:, None])


def projector(A):
    q = np.linalg.qr(A)[0]
    return q @ q.conj().T


def frac_turns(f, t):
    """f t minus its nearest integer, from the (all but) exact product, rounded once: what fma(f, t, -k) gives."""
    p = LD(1) * np.asarray(f, dtype=LD) * np.asarray(t, dtype=LD)
    k = np.rint(np.asarray(f, dtype=np.float64) * np.asarray(t, dtype=np.float64))
    return np.asarray(p - k, dtype=np.float64)


def unit(f, t):
    """e^{2 pi i f t} with the turn count reduced first."""
    x = 2.0 * frac_turns(f, t)
    return np.cos(np.pi * x) + 1j * np.sin(np.pi * x)


def forward(rho, te, f, r, tau, psi):
    """y [R, E, C] of rho [R, M, C], tau [R], psi [R]."""
    t = np.asarray(te)[None, :] + np.asarray(tau)[:, None]  # [R, E]
    a = np.exp((2j * np.pi * np.asarray(f) - np.asarray(r))[None, None, :] * t[:, :, None])  # [R, E, M]
    return np.einsum("rem,rmc->rec", a, rho) * np.exp(2j * np.pi * np.asarray(psi)[:, None] * t)[:, :, None]


def known(y, te, f, r, tau, psi, reverse=False):
    """The factorised estimate rho [R, M, C] of y [R, E, C] (complex128); `reverse`: the echo sum in descending order."""
    te, f, r = np.asarray(te, dtype=np.float64), np.asarray(f, dtype=np.float64), np.asarray(r, dtype=np.float64)
    p0 = np.linalg.pinv(a0(te, f, r))  # [M, E]
    t = te[None, :] + np.asarray(tau, dtype=np.float64)[:, None]
    d = np.conj(unit(np.asarray(psi, dtype=np.float64)[:, None], t))  # [R, E]
    z = d[:, :, None] * y
    order = range(len(te) - 1, -1, -1) if reverse else range(len(te))
    acc = np.zeros((y.shape[0], len(f), y.shape[2]), dtype=np.complex128)
    for e in order:
        acc += p0[None, :, e, None] * z[:, e, None, :]
    tau = np.asarray(tau, dtype=np.float64)
    c = np.conj(unit(f[None, :], tau[:, None])) * np.exp(r[None, :] * tau[:, None])  # [R, M]
    return c[:, :, None] * acc


def lstsq_rows(y, te, f, r, tau, psi):
    """Per-row numpy.linalg.lstsq on A_r = D_r A0 C_r built directly."""
    out = np.zeros((y.shape[0], len(f), y.shape[2]), dtype=np.complex128)
    for i in range(y.shape[0]):
        t = np.asarray(te) + tau[i]
        A = np.exp((2j * np.pi * np.asarray(f) - np.asarray(r))[None, :] * t[:, None]) * np.exp(2j * np.pi * psi[i] * t)[:, None]
        out[i] = np.linalg.lstsq(A, y[i], rcond=None)[0]
    return out


# ---- the field fit of one row ----------------------------------------------------------------------------------------------
def grid(te, max_field):
    te = np.asarray(te, dtype=np.float64)
    delta = 1.0 / (4.0 * (te.max() - te.min()))
    return delta, int(np.floor(max_field / delta))


def pairs(E):
    iu = np.triu_indices(E, 1)
    return iu[0], iu[1]


def gram_w(y, Pi, reverse=False):
    """(w0, W over the pairs e < e', syy, Delta is the caller's) of one row y [E, C]; `reverse`: columns descending."""
    E, C = y.shape
    pe, pf = pairs(E)
    cols = range(C - 1, -1, -1) if reverse else range(C)
    s = np.zeros(len(pe), dtype=np.complex128)
    syy = 0.0
    w0 = 0.0
    for c in cols:
        s += y[pe, c] * np.conj(y[pf, c])
        for e in range(E):
            n = y[e, c].real ** 2 + y[e, c].imag ** 2
            syy += n
            w0 += Pi[e, e].real * n
    return w0, Pi[pf, pe] * s, syy


def sums(psi, W, dl):
    """(sum Re, sum Delta Im, sum Delta^2 Re) of W e^{2 pi i psi Delta} over the pairs in ascending order."""
    u = W * unit(psi, dl)
    return float(np.sum(u.real)), float(np.sum(dl * u.imag)), float(np.sum(dl * dl * u.real))


def G(psi, w0, W, dl):
    return w0 + 2.0 * sums(psi, W, dl)[0]


def better(p1, g1, p2, g2):
    if p1 != p2:
        return p1 > p2
    return abs(g1) < abs(g2) if abs(g1) != abs(g2) else g1 < g2


def coarse(w0, W, dl, delta, Gn):
    """(g*, G on the grid as an array over g = -Gn ... Gn)."""
    gs = np.arange(-Gn, Gn + 1)
    vals = np.array([G(float(g) * delta, w0, W, dl) for g in gs])
    best, gb = vals[Gn], 0
    for g, v in zip(gs, vals):
        if better(v, int(g), best, gb):
            best, gb = v, int(g)
    return gb, vals


def refine(w0, W, dl, g, delta, Gn, max_field):
    """The safeguarded Newton iteration -> (psi*, status, G(psi*), evaluations, (a, b) of the first bracket)."""
    a, b = max((g - 1) * delta, -max_field), min((g + 1) * delta, max_field)
    bracket = (a, b)
    f, tol, status, evals = float(g) * delta, delta * 2.0 ** -40, 0, 0
    if Gn > 0 and abs(g) == Gn:
        end = max_field if g > 0 else -max_field
        s0, d1, _ = sums(end, W, dl)
        evals += 1
        if (d1 < 0.0) if g > 0 else (d1 > 0.0):  # G' = -4 pi d1 points out of the window
            return end, 1, w0 + 2.0 * s0, evals, bracket
    steps = 0
    while True:
        s0, d1, d2 = sums(f, W, dl)
        evals += 1
        if d1 < 0.0:
            a = f
        elif d1 > 0.0:
            b = f
        else:
            return f, status, w0 + 2.0 * s0, evals, bracket
        fn = f - d1 / (2.0 * np.pi * d2) if d2 > 0.0 else np.nan
        if not (a <= fn <= b):
            fn = 0.5 * (a + b)
        step = abs(fn - f)
        f = fn
        if step <= tol:
            break
        steps += 1
        if steps == STEPS:
            status = 4
            break
    return f, status, w0 + 2.0 * sums(f, W, dl)[0], evals + 1, bracket


def fit_row(y, te, f, r, tau, max_field, Pi=None, reverse=False):
    """One row y [E, C] -> dict(field, status, residual, species [M, C], g, grid values, margin, evaluations)."""
    te = np.asarray(te, dtype=np.float64)
    M, C = len(f), y.shape[1]
    out = dict(species=np.zeros((M, C), dtype=np.complex128), field=np.nan, residual=np.nan, status=2, g=0, vals=None,
               evals=0, bracket=None)
    if not (np.all(np.isfinite(y.view(np.float64))) and np.isfinite(tau)):
        return out
    Pi = projector(a0(te, f, r)) if Pi is None else Pi
    pe, pf = pairs(len(te))
    dl = te[pf] - te[pe]
    w0, W, syy = gram_w(y, Pi, reverse)
    delta, Gn = grid(te, max_field)
    g, vals = coarse(w0, W, dl, delta, Gn)
    out.update(g=g, vals=vals)
    if not (np.all(np.isfinite(vals)) and np.isfinite(syy)):
        return out
    if not vals[g + Gn] > 0.0:
        out.update(field=0.0, residual=0.0, status=3)
        return out
    psi, status, gfin, evals, bracket = refine(w0, W, dl, g, delta, Gn, max_field)
    out.update(field=psi, status=status, residual=max(0.0, 1.0 - gfin / syy), evals=evals, bracket=bracket, w0=w0, W=W,
               dl=dl, syy=syy, species=known(y[None], te, f, r, np.array([tau]), np.array([psi]))[0])
    return out


def brent_row(y, te, f, r, max_field, g, Pi=None):
    """psi* and residual by scipy's brentq on G' over the bracket of grid point g, W summed over the columns in
    descending order: the independent route.  None when G' does not change sign over the bracket (a window end)."""
    from scipy.optimize import brentq

    te = np.asarray(te, dtype=np.float64)
    Pi = projector(a0(te, f, r)) if Pi is None else Pi
    pe, pf = pairs(len(te))
    dl = te[pf] - te[pe]
    w0, W, syy = gram_w(y, Pi, reverse=True)
    delta, _ = grid(te, max_field)
    a, b = max((g - 1) * delta, -max_field), min((g + 1) * delta, max_field)
    d1 = lambda p: -sums(p, W, dl)[1]  # noqa: E731 -- G' / 4 pi
    if not d1(a) > 0.0 > d1(b):
        return None
    psi = brentq(d1, a, b, xtol=1e-18 * delta, rtol=4 * EPS, maxiter=200)
    return psi, max(0.0, 1.0 - G(psi, w0, W, dl) / syy)


def margin(vals, g, Gn):
    """How far the best grid value exceeds every grid value outside g* +- 1, relative to itself (inf: no such point)."""
    gs = np.arange(-Gn, Gn + 1)
    far = vals[np.abs(gs - g) > 1]
    return np.inf if far.size == 0 else (vals[g + Gn] - far.max()) / vals[g + Gn]


# ---- the cases -------------------------------------------------------------------------------------------------------------
def echo_times(E, rng):
    """Non-uniform echo times around a spacing of 1.1 ms, in unsorted order."""
    te = 0.9e-3 + 1.1e-3 * np.arange(E) + rng.uniform(-0.25e-3, 0.25e-3, E)
    return te[rng.permutation(E)]


def make_case(E, M, rows, cols, seed, max_field=None, noise=1e-3, psi_max=300.0):
    """A parity case: y [R, E, C] complex128 with its model.  `max_field` None: a known field up to +-psi_max Hz and
    delays up to 5 ms; else the field lies within 0.8 max_field."""
    rng = np.random.default_rng(seed)
    te = echo_times(E, rng)
    f, r = np.array(FREQS[:M]), np.array(DECAYS[:M])
    rho = (rng.standard_normal((rows, M, cols)) + 1j * rng.standard_normal((rows, M, cols))) * rng.uniform(0.5, 2.0, (1, M, 1))
    tau = rng.uniform(0.0, 5e-3, rows)
    psi = rng.uniform(-psi_max, psi_max, rows) if max_field is None else rng.uniform(-0.8, 0.8, rows) * max_field
    y = forward(rho, te, f, r, tau, psi)
    y = y + noise * (rng.standard_normal(y.shape) + 1j * rng.standard_normal(y.shape))
    return dict(E=E, M=M, te=te, f=f, r=r, rho=rho, tau=tau, psi=psi, y=y, max_field=max_field)


KNOWN_EM = ((2, 1), (2, 2), (3, 2), (8, 3), (16, 8), (32, 8))
KNOWN_ROWS = (1, 63, 64, 65, 257)
KNOWN_COLS = (1, 3, 5)
FIT_EM = ((2, 1), (3, 2), (8, 3), (16, 8))
FIT_GRIDS = (1, 3, 25, 1025)
FIT_SHAPES = ((1, 1), (64, 4), (65, 5))


def fit_max_field(te, n_grid):
    """A window whose coarse grid has n_grid points: (n_grid - 1) / 2 + 0.5 grid spacings (0.6 of one for one point)."""
    delta = 1.0 / (4.0 * (np.max(te) - np.min(te)))
    return 0.6 * delta if n_grid == 1 else ((n_grid - 1) / 2 + 0.5) * delta


def fit_cases():
    """(name, E, M, rows, cols, n_grid, seed): every (E, M) with every grid size, the shapes in turn.  Two echoes make G
    a single cosine of period 4 delta, so a grid of more than 3 points holds exact copies of its maximum: E = 2 takes
    the grids of 1 and 3 points only."""
    out, k = [], 0
    for E, M in FIT_EM:
        for n_grid in FIT_GRIDS:
            if E == 2 and n_grid > 3:
                continue
            rows, cols = FIT_SHAPES[k % 3]
            out.append((f"E{E}M{M}g{n_grid}r{rows}c{cols}", E, M, rows, cols, n_grid, 100 + k))
            k += 1
    return out


def make_fit_case(E, M, rows, cols, n_grid, seed):
    rng = np.random.default_rng(seed)
    mf = fit_max_field(echo_times(E, rng), n_grid)  # (make_case draws the same echo times first)
    return make_case(E, M, rows, cols, seed, max_field=mf)
