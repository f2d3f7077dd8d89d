"""numpy restatement of remove_water's definition: HSVD of one FID, removal of the components in
a frequency band.  Two routes to the signal subspace: "eigh" (eigen-decomposition of G = H^H H) and "svd" (singular
vectors of the Hankel matrix H itself); both then take Q by lstsq, the poles by eigvals and the amplitudes by lstsq.
Also the generator of the test FIDs and the parity cases of tests/test_hsvd.py and tests/test_gpu_hsvd.py."""
import numpy as np

EPS = float(np.finfo(np.float64).eps)
DT = 2e-4
BAND = (-50.0, 50.0)
FIELDS = ("frequency", "damping", "amplitude", "phase")


def hankel(x, n_cols):
    """H[l, j] = x[l + j], N - M + 1 rows."""
    return np.lib.stride_tricks.sliding_window_view(np.asarray(x), n_cols)


def _nan_result(x, k, status, y):
    out = {f: np.full(k, np.nan) for f in FIELDS}
    out.update(y=y, removed=np.zeros(k, np.int32), n_removed=0, status=status, z=np.full(k, np.nan + 0j),
               a=np.full(k, np.nan + 0j), cond=np.nan)
    return out


def hsvd(x, n_cols, rank, dt=DT, band=BAND, route="eigh"):
    """One FID.  Returns y, the components sorted by frequency (frequency Hz, damping 1/s, amplitude, phase rad,
    removed 0/1), n_removed, status, and for the tests the poles z, the complex amplitudes a and cond(B)."""
    x = np.asarray(x, dtype=np.complex128)
    n, m, k = x.size, int(n_cols), int(rank)
    if not np.all(np.isfinite(x)):
        return _nan_result(x, k, 2, np.zeros_like(x))
    if not x.any():
        return _nan_result(x, k, 1, x.copy())
    h = hankel(x, m)
    try:
        with np.errstate(all="ignore"):
            if route == "eigh":
                g = h.conj().T @ h
                if not np.all(np.isfinite(g)):
                    return _nan_result(x, k, 2, np.zeros_like(x))
                _, vec = np.linalg.eigh(g)
                w = vec[:, ::-1][:, :k].conj()
            elif route == "svd":
                _, s, vh = np.linalg.svd(h, full_matrices=False)
                if not np.all(np.isfinite(s)):
                    return _nan_result(x, k, 2, np.zeros_like(x))
                w = vh.T[:, :k]
            else:
                raise ValueError(route)
        if not 1.0 - np.sum(np.abs(w[-1]) ** 2) > 0.0:
            return _nan_result(x, k, 4, x.copy())
        q = np.linalg.lstsq(w[:-1], w[1:], rcond=None)[0]
        z = np.linalg.eigvals(q)
    except np.linalg.LinAlgError:  # an iteration of LAPACK's that did not converge: the kernel's caps
        return _nan_result(x, k, 3, x.copy())
    with np.errstate(all="ignore"):
        logz = np.log(z)
        f = logz.imag / (2 * np.pi * dt)
        order = np.argsort(f, kind="stable")
        z, logz, f = z[order], logz[order], f[order]
        d = -logz.real / dt
        b = np.exp(np.arange(n)[:, None] * logz[None, :])
    if not np.all(np.isfinite(b)):
        return _nan_result(x, k, 4, x.copy())
    a, _, rk, sv = np.linalg.lstsq(b, x, rcond=None)
    if rk < k or not np.all(np.isfinite(a)):
        return _nan_result(x, k, 4, x.copy())
    sel = (f >= band[0]) & (f <= band[1])
    out = dict(frequency=f, damping=d, amplitude=np.abs(a), phase=np.angle(a), removed=sel.astype(np.int32),
               n_removed=int(sel.sum()), status=0 if sel.any() else 1, z=z, a=a, cond=float(sv[0] / sv[-1]))
    out["y"] = x - b[:, sel] @ a[sel] if sel.any() else x.copy()
    return out


def hsvd_rows(x, n_cols, rank, dt=DT, band=BAND, route="eigh"):
    """Every row of x[..., N]; the outputs stacked."""
    x = np.asarray(x)
    rows = [hsvd(r, n_cols, rank, dt, band, route) for r in x.reshape(-1, x.shape[-1])]
    lead = x.shape[:-1]
    out = {}
    for key in rows[0]:
        v = np.stack([np.asarray(r[key]) for r in rows])
        out[key] = v.reshape(lead + v.shape[1:])
    return out


# ---- the generator --------------------------------------------------------------------------------------------------
def make_fid(n, seed, n_vox=1, dt=DT, noise=0.02, water=True, metabolites=True):
    """(x, clean metabolite-only FID, parameters): three metabolite peaks (largest amplitude 1), three water-band
    components within +-15 Hz at 6 ... 40 times the largest peak, complex noise of standard deviation `noise` per part."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) * dt
    x = np.zeros((n_vox, n), complex)
    met = np.zeros((n_vox, n), complex)
    pars = []
    for v in range(n_vox):
        fm = np.array([260.0, 430.0, 640.0]) + rng.uniform(-20, 20, 3)
        am = np.array([1.0, rng.uniform(0.4, 0.9), rng.uniform(0.4, 0.9)]) * np.exp(1j * rng.uniform(-np.pi, np.pi, 3))
        dm = rng.uniform(15.0, 40.0, 3)
        fw = np.array([-11.0, 1.0, 12.0]) + rng.uniform(-3, 3, 3)
        aw = rng.uniform(6.0, 40.0, 3) * np.exp(1j * rng.uniform(-np.pi, np.pi, 3))
        dw = rng.uniform(20.0, 60.0, 3)
        met[v] = (am * np.exp((2j * np.pi * fm - dm) * t[:, None])).sum(axis=1)
        wat = (aw * np.exp((2j * np.pi * fw - dw) * t[:, None])).sum(axis=1)
        x[v] = (met[v] if metabolites else 0) + (wat if water else 0)
        x[v] += noise * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
        pars.append(dict(fm=fm, am=am, dm=dm, fw=fw, aw=aw, dw=dw))
    return x, met, pars


# name -> (N, M, K, seed, voxels): the smallest shapes at which the kernel takes another path (M = 2, 3: one block of
# padding; 16 / 17: one / two 16-row blocks a side and the time-sliced Gram; 63 / 64: all 36 blocks; N = 2 M, 2 M + 1:
# the shortest rows; 255 ... 257: around one staged tile; 2048: the flagship; K = 1, 2, M - 1, 32).  The seeds are the
# first for which both routes of the oracle meet the conditions of tests/test_hsvd.py.
PARITY_CASES = {}


def _case(n, m, k, seed, vox=2):
    PARITY_CASES[f"N{n}-M{m}-K{k}"] = (n, m, k, seed, vox)


_case(4, 2, 1, 1, 2)
_case(5, 2, 1, 1, 2)
_case(6, 3, 1, 1, 2)
_case(7, 3, 2, 1, 2)
_case(32, 16, 1, 1, 2)
_case(33, 16, 2, 1, 2)
_case(255, 16, 15, 3, 2)
_case(256, 16, 2, 1, 2)
_case(34, 17, 16, 2, 2)
_case(35, 17, 2, 1, 2)
_case(257, 17, 16, 1, 2)
_case(66, 33, 32, 6, 2)
_case(126, 63, 32, 1, 2)
_case(127, 63, 2, 1, 2)
_case(255, 63, 20, 1, 2)
_case(2048, 63, 20, 1, 2)
_case(128, 64, 32, 1, 2)
_case(129, 64, 1, 1, 2)
_case(256, 64, 25, 1, 2)
_case(257, 64, 20, 1, 2)
_case(2048, 64, 12, 1, 2)
_case(2048, 64, 20, 1, 2)
_case(2048, 64, 25, 1, 2)
_case(2048, 64, 32, 1, 2)
_case(2048, 32, 8, 1, 2)
_case(1024, 48, 10, 1, 2)
_case(512, 32, 6, 1, 2)
_case(16384, 64, 20, 1, 1)


def parity_case(name):
    n, m, k, seed, vox = PARITY_CASES[name]
    x, met, _ = make_fid(n, seed, vox)
    return x, met, m, k


def gap(a, b, x):
    """The disagreement of two results on the same rows x: y in units of max |x| per row, and over the in-band
    components (the same set in both, or inf) arg z in radians, ln |z|, and |a - a'| / |a|."""
    if not np.array_equal(a["removed"], b["removed"]):
        return dict(y=np.inf, f=np.inf, d=np.inf, a=np.inf)
    sel = a["removed"].astype(bool)
    scale = np.abs(x).max(axis=-1, keepdims=True)
    dt_f = np.abs(np.angle(a["z"][sel] * np.conj(b["z"][sel])))
    dt_d = np.abs(np.log(np.abs(a["z"][sel])) - np.log(np.abs(b["z"][sel])))
    da = np.abs(a["a"][sel] - b["a"][sel]) / np.abs(a["a"][sel])
    mx = lambda v: float(v.max()) if v.size else 0.0  # noqa: E731
    return dict(y=float((np.abs(a["y"] - b["y"]) / scale).max()), f=mx(dt_f), d=mx(dt_d), a=mx(da))


def with_poles(res, dt=DT):
    """z and a of a result that has only frequency, damping, amplitude and phase (the kernel's outputs)."""
    out = dict(res)
    out["z"] = np.exp((-np.asarray(res["damping"]) + 2j * np.pi * np.asarray(res["frequency"])) * dt)
    out["a"] = np.asarray(res["amplitude"]) * np.exp(1j * np.asarray(res["phase"]))
    return out


def route_gap(name):
    """gap() of the oracle's two routes on a parity case, and the two results."""
    x, _, m, k = parity_case(name)
    a, b = (hsvd_rows(x, m, k, route=rt) for rt in ("eigh", "svd"))
    return gap(a, b, x), a, b


# ---- noise-free model FIDs ------------------------------------------------------------------------------------------
def model_fid(f, d, a, n, dt=DT):
    """sum_k a_k exp((2 pi i f_k - d_k) t dt), t < n: no noise, so the Hankel matrix has rank len(f) exactly."""
    f, d, a = (np.atleast_1d(np.asarray(v)) for v in (f, d, a))
    t = np.arange(n) * dt
    return (a * np.exp((2j * np.pi * f - d) * t[:, None])).sum(axis=1)


# name -> (f Hz, d 1/s, a, N, M, band): K = len(f), the true number of components.  Component-wise parity with the oracle
# is not defined here (clustered poles, cond(B) large, a dynamic range of 1e6, conjugate pairs, a growing pole); the GPU
# tests check that the kernel's outputs follow from the components it returns.  Every band edge is at least 0.5 Hz
# (EDGE_HZ of tests/test_hsvd.py) from every true pole.
MODEL_CASES = {
    "pair-1Hz": ((0.0, 1.0, 300.0), (30.0, 35.0, 25.0), (3.0, 2.0 * np.exp(0.7j), 1.0), 512, 32, (-50.0, 50.0)),
    "pair-0.2Hz": ((0.0, 0.2, 300.0), (30.0, 35.0, 25.0), (3.0, 2.0 * np.exp(0.7j), 1.0), 512, 32, (-50.0, 50.0)),
    "range-1e6": ((2.0, 300.0, 520.0), (40.0, 25.0, 30.0), (1e6, 1.0, 0.7 * np.exp(-1.1j)), 512, 32, (-50.0, 50.0)),
    "real-valued": ((-400.0, -20.0, 20.0, 400.0), (30.0, 20.0, 20.0, 30.0), (0.5, 1.5, 1.5, 0.5), 256, 24, (-50.0, 50.0)),
    "growing": ((5.0, 310.0), (-20.0, 30.0), (2.0, 1.0), 256, 16, (-50.0, 50.0)),
}


def model_case(name):
    """(x, M, K, band, f, d, a) of a MODEL_CASES entry."""
    f, d, a, n, m, band = MODEL_CASES[name]
    return model_fid(f, d, a, n), m, len(f), band, np.asarray(f), np.asarray(d), np.asarray(a, complex)


def model_residual(x, res, dt=DT):
    """max |x - B a| / max |x| of the full model rebuilt from a result's frequency, damping, amplitude and phase."""
    r = with_poles(res, dt)
    b = np.exp(np.arange(x.size)[:, None] * np.log(r["z"])[None, :])
    return float(np.abs(x - b @ r["a"]).max() / np.abs(x).max())


# ---- sparse combs: inputs with exact zeros in Q ----------------------------------------------------------------------------
def comb_fid(p, n, rho, theta):
    """Exact zeros except at t = 0, P, 2 P, ...: x[t] = rho^(t / P) e^{i theta t} there.  The sum of P components of
    amplitude 1 / P with poles rho^(1 / P) e^{i (theta + 2 pi k / P)}: G couples only indices of the same residue mod P,
    Jacobi skips every other pair, and Q is a weighted cyclic permutation with a zero diagonal."""
    x = np.zeros(n, complex)
    t = np.arange(0, n, p)
    x[t] = rho ** (t // p) * np.exp(1j * theta * t)
    return x


def comb_theta(p):
    return 2 * np.pi * 0.3 / p  # no pole at arg z = +-pi: the sort by frequency is unambiguous


def comb_truth(p, n, rho, theta, dt=DT):
    """(z sorted by frequency, a, index of the in-band pole, band): every amplitude 1 / P, the band fs / (4 P) either
    side of the pole k = 0."""
    z = rho ** (1.0 / p) * np.exp(1j * (theta + 2 * np.pi * np.arange(p) / p))
    f = np.angle(z) / (2 * np.pi * dt)
    order = np.argsort(f, kind="stable")
    f0 = theta / (2 * np.pi * dt)
    half = 1.0 / (4 * p * dt)
    return z[order], np.full(p, 1.0 / p, complex), int(np.nonzero(order == 0)[0][0]), (f0 - half, f0 + half)


# name -> (P, M, N, rho); K = P
COMB_CASES = {f"P{p}-M{m}-N{n}-rho{rho}": (p, m, n, rho) for p, m, n, rho in (
    (2, 4, 16, 0.9), (3, 6, 24, 0.9), (4, 8, 40, 0.9), (5, 16, 64, 0.9), (8, 16, 80, 0.9), (16, 17, 67, 0.8),
    (16, 32, 160, 0.8), (31, 63, 250, 0.8), (32, 64, 320, 0.8), (32, 64, 320, 1.0))}


def grid_fid(k1, k2, amp, n, dt=DT):
    """A two-level comb on a grid: G = K1 + K2 undamped poles e^{i (theta + 2 pi k / G)}, the first K1 of amplitude
    `amp`, the others 1.  With M and N - M + 1 multiples of G the Vandermonde vectors are orthogonal, the Hankel matrix
    has the two singular values amp sqrt(R M) and sqrt(R M), K1- and K2-fold, and Q is unitary with degenerate groups.
    Returns (x, z sorted by frequency, a in that order, index of pole 0, band: fs / (4 G) either side of pole 0)."""
    g = k1 + k2
    th = comb_theta(g)
    z = np.exp(1j * (th + 2 * np.pi * np.arange(g) / g))
    a = np.where(np.arange(g) < k1, amp, 1.0).astype(complex)
    x = (a * z[None, :] ** np.arange(n)[:, None]).sum(axis=1)
    order = np.argsort(np.angle(z), kind="stable")
    f0, half = th / (2 * np.pi * dt), 1.0 / (4 * g * dt)
    return x, z[order], a[order], int(np.nonzero(order == 0)[0][0]), (f0 - half, f0 + half)


# name -> (K1, K2, amplitude, M, N); K = K1 + K2.  The one case of the search in tests/test_hsvd.py on which the restated
# iteration deflates in the middle of the matrix (an active window that starts below row 0, l > 0 in hs_qr).
GRID_CASES = {"G1+3-A2-M8-N23": (1, 3, 2.0, 8, 23)}
# every candidate of that search
GRID_SEARCH = ((2, 2, 2.0, 8, 23), (12, 4, 2.0, 32, 95), (4, 4, 2.0, 16, 47), (8, 8, 2.0, 32, 95), (3, 3, 2.0, 12, 35),
               (6, 2, 2.0, 16, 47), (1, 3, 2.0, 8, 23), (2, 6, 2.0, 16, 47))
# name -> (P, M, N, rho), theta = 0 (P odd: no pole at arg z = +-pi): a real-valued comb.  Q is real, every product
# with an exact zero stays one, and Wilkinson's shift is exactly zero step after step: without the exceptional shift the
# restated iteration runs into its cap of 30 K steps on both (tests/test_hsvd.py), with it it ends in 22.
REAL_COMBS = {"P5-M16-N64-rho0.9-real": (5, 16, 64, 0.9), "P5-M16-N64-rho1.0-real": (5, 16, 64, 1.0)}
VALUE_CASES = list(COMB_CASES) + list(REAL_COMBS) + list(GRID_CASES)


def comb_case(name):
    """(x, M, K, band, z true, a true, in-band index, y true) of a COMB_CASES, REAL_COMBS or GRID_CASES entry."""
    if name in GRID_CASES:
        k1, k2, amp, m, n = GRID_CASES[name]
        x, z, a, k0, band = grid_fid(k1, k2, amp, n)
        return x, m, k1 + k2, band, z, a, k0, x - a[k0] * z[k0] ** np.arange(n)
    p, m, n, rho = REAL_COMBS[name] if name in REAL_COMBS else COMB_CASES[name]
    th = 0.0 if name in REAL_COMBS else comb_theta(p)
    x = comb_fid(p, n, rho, th)
    z, a, k0, band = comb_truth(p, n, rho, th)
    return x, m, p, band, z, a, k0, x - a[k0] * z[k0] ** np.arange(n)


def comb_routes(name):
    """The oracle's two routes on a comb case, their gap(), and each route's truth_gap()."""
    x, m, k, band, z, a, k0, y = comb_case(name)
    r = {rt: hsvd(x, m, k, band=band, route=rt) for rt in ("eigh", "svd")}
    rows = {rt: {key: np.asarray(v)[None] for key, v in r[rt].items()} for rt in r}
    return gap(rows["eigh"], rows["svd"], x[None]), r, {rt: truth_gap(r[rt], x, z, a, k0, y) for rt in r}


def model_routes(name):
    """The oracle's two routes on a model case and each route's model_residual()."""
    x, m, k, band = model_case(name)[:4]
    r = {rt: hsvd(x, m, k, band=band, route=rt) for rt in ("eigh", "svd")}
    return r, {rt: model_residual(x, r[rt]) for rt in r}


def truth_gap(res, x, z, a, k0, y):
    """The distance of a result (z, a, y) from the analytic truth: "pole" max |dz|, "amp" the amplitudes relative,
    "sig" y in units of max |x|."""
    return dict(pole=float(np.abs(res["z"] - z).max()), amp=float((np.abs(res["a"] - a) / np.abs(a)).max()),
                sig=float(np.abs(res["y"] - y).max() / np.abs(x).max()))


# ---- the kernel's pole iteration restated (xm_wg.h: wg_jacobi; xm_hsvd.h: hs_select, hs_shift_matrix, hs_hessenberg, hs_qr) -------
def jacobi_w(x, n_cols, rank, sweeps=30):
    """W (M x K) as the kernel forms it: cyclic Jacobi in the kernel's round-robin order on sum_l h_l h_l^H, a pair with
    G_pq = 0 skipped (so exact zeros stay exact), then the eigenvectors of the K largest diagonal entries, the largest
    first, a tie going to the lower index.  Sequential within a step, which the disjoint pairs of a step allow."""
    h = hankel(np.asarray(x, complex), n_cols)
    g = np.einsum("li,lj->ij", h, h.conj())  # (no BLAS: the same bits whatever the number of threads)
    c = g.shape[0]
    v = np.eye(c, dtype=complex)
    fro2 = float((np.abs(g) ** 2).sum())
    n_pairs = (c + 1) // 2
    players = 2 * n_pairs
    for sweep in range(sweeps + 1):
        off2 = float((np.abs(g - np.diag(np.diag(g))) ** 2).sum())
        if not off2 > EPS * EPS * fro2:
            break
        if sweep == sweeps:
            raise np.linalg.LinAlgError("Jacobi sweep cap")
        for step in range(players - 1):
            for t in range(n_pairs):
                a = players - 1 if t == 0 else (step + t) % (players - 1)
                b = step if t == 0 else (step - t + players - 1) % (players - 1)
                p, q = min(a, b), max(a, b)
                if q >= c or g[p, q] == 0:
                    continue
                hh = abs(g[p, q])
                tau = (g[q, q].real - g[p, p].real) / (2 * hh)
                tt = (1.0 if tau >= 0 else -1.0) / (abs(tau) + np.sqrt(1 + tau * tau))
                cs = 1 / np.sqrt(1 + tt * tt)
                sn = tt * cs
                e = g[p, q] / hh
                j = np.array([[cs, sn * e], [-sn * np.conj(e), cs]])  # columns p, q <- (columns p, q) J
                gpp, gqq = g[p, p].real - tt * hh, g[q, q].real + tt * hh
                g[:, [p, q]] = g[:, [p, q]] @ j
                v[:, [p, q]] = v[:, [p, q]] @ j
                g[[p, q], :] = j.conj().T @ g[[p, q], :]
                g[p, p], g[q, q], g[p, q], g[q, p] = gpp, gqq, 0.0, 0.0
    lam = np.diag(g).real
    order = np.argsort(-lam, kind="stable")[:rank]
    return v[:, order]


def shift_matrix(w):
    """hs_shift_matrix: Q = (I + w w^H / (1 - ||w||^2)) Wup^H Wdown, w^H the last row of W."""
    pm = w[:-1].conj().T @ w[1:]
    last = w[-1]
    den = 1.0 - float((np.abs(last) ** 2).sum())
    if not den > 0.0:
        raise np.linalg.LinAlgError("1 - ||w||^2 <= 0")
    return pm + np.outer(last.conj(), last @ pm) / den


def _abs1(v):
    return abs(v.real) + abs(v.imag)


def _hz_sqrt(a):
    m = np.hypot(a.real, a.imag)
    if m == 0.0:
        return 0j
    u = np.sqrt(0.5 * (m + abs(a.real)))
    v = a.imag / (2.0 * u)
    return complex(u, v) if a.real >= 0.0 else complex(abs(v), u if a.imag >= 0.0 else -u)


def _hz_div(a, b):
    s = 1.0 / (abs(b.real) + abs(b.imag))
    br, bi = b.real * s, b.imag * s
    d = br * br + bi * bi
    return complex(((a.real * s) * br + (a.imag * s) * bi) / d, ((a.imag * s) * br - (a.real * s) * bi) / d)


def hessenberg(q, count):
    """hs_hessenberg on a copy of Q; count["sigma0"]: columns with nothing below the subdiagonal, skipped."""
    h = np.array(q, complex)
    k_ = h.shape[0]
    for k in range(k_ - 2):
        sigma = float((np.abs(h[k + 2:, k]) ** 2).sum())
        if sigma == 0.0:
            count["sigma0"] += 1
            continue
        x0 = h[k + 1, k]
        a0 = np.hypot(x0.real, x0.imag)
        nrm = np.sqrt(a0 * a0 + sigma)
        alpha = x0 * (-nrm / a0) if a0 > 0.0 else complex(-nrm, 0.0)
        v = h[k + 1:, k].copy()
        v[0] = x0 - alpha
        v /= np.sqrt(abs(v[0]) ** 2 + sigma)
        h[k + 1:, :] -= np.outer(v, 2.0 * (v.conj() @ h[k + 1:, :]))
        h[:, k + 1:] -= np.outer(2.0 * (h[:, k + 1:] @ v), v.conj())
    return h


def qr_poles(h, hnorm, count, exceptional=True):
    """hs_qr on a copy of the Hessenberg matrix: single-shift QR, Wilkinson's shift, an exceptional shift at the 10th
    and 20th step of a deflation, the active window [l, hi] alone updated.  Raises LinAlgError at the cap of 30 K steps.
    count: "steps", "exceptional", "max_its", "l_positive" (steps on a window that starts below row 0), "hnorm" (deflation
    tests whose two diagonal entries were both zero).  `exceptional=False` is for the mutation check only."""
    h = np.array(h, complex)
    k_ = h.shape[0]
    z = np.zeros(k_, complex)
    hi, its, total = k_ - 1, 0, 0
    while hi >= 0:
        l = hi
        while l > 0:
            sub = _abs1(h[l, l - 1])
            tst = _abs1(h[l - 1, l - 1]) + _abs1(h[l, l])
            if tst == 0.0:
                tst = hnorm
                count["hnorm"] += 1
            if sub <= EPS * tst:
                break
            l -= 1
        if l == hi:
            z[hi] = h[hi, hi]
            hi -= 1
            its = 0
            continue
        if total == 30 * k_:
            raise np.linalg.LinAlgError("QR iteration cap")
        total += 1
        its += 1
        count["steps"] += 1
        count["max_its"] = max(count["max_its"], its)
        count["l_positive"] += l > 0
        a, b, c, d = h[hi - 1, hi - 1], h[hi - 1, hi], h[hi, hi - 1], h[hi, hi]
        if exceptional and its in (10, 20):
            count["exceptional"] += 1
            s = complex(abs(c.real) + (abs(h[hi - 1, hi - 2].real) if hi - 2 >= l else 0.0), 0.0)
        else:
            dl = (a - d) * 0.5
            bc = b * c
            disc = _hz_sqrt(dl * dl + bc)
            if dl.real * disc.real + dl.imag * disc.imag < 0.0:
                disc = -disc
            den = dl + disc
            s = d if den == 0 else d - _hz_div(bc, den)
        idx = np.arange(l, hi + 1)
        h[idx, idx] -= s
        rots = []
        for k in range(l, hi):  # from the left: columns k ... hi
            x, y = h[k, k], h[k + 1, k]
            r = np.hypot(np.hypot(x.real, x.imag), np.hypot(y.real, y.imag))
            p, q = (np.conj(x) / r, np.conj(y) / r) if r != 0.0 else (1.0 + 0j, 0j)
            top, bot = h[k, k:hi + 1].copy(), h[k + 1, k:hi + 1].copy()
            h[k, k:hi + 1] = p * top + q * bot
            h[k + 1, k:hi + 1] = np.conj(p) * bot - np.conj(q) * top
            rots.append((p, q))
        for k in range(l, hi):  # from the right: rows l ... min(k + 1, hi)
            p, q = rots[k - l]
            x, y = h[l:k + 2, k].copy(), h[l:k + 2, k + 1].copy()
            h[l:k + 2, k] = x * np.conj(p) + y * np.conj(q)
            h[l:k + 2, k + 1] = y * p - x * q
        h[idx, idx] += s
    return z


def new_count():
    return dict(steps=0, exceptional=0, max_its=0, l_positive=0, sigma0=0, hnorm=0)


def restated_poles(w, exceptional=True):
    """(z, Q, counters) of the kernel's route from W to the poles."""
    count = new_count()
    q = shift_matrix(np.asarray(w, complex))
    hnorm = float(np.sqrt((q.real ** 2 + q.imag ** 2).sum()))
    return qr_poles(hessenberg(q, count), hnorm, count, exceptional), q, count


def oracle_w(x, n_cols, rank):
    """W of the oracle's route "eigh"."""
    h = hankel(np.asarray(x, complex), n_cols)
    _, vec = np.linalg.eigh(h.conj().T @ h)
    return vec[:, ::-1][:, :rank].conj()


def match_sets(a, b):
    """max |a_i - b_pi(i)| with pi the greedy nearest matching of two equally large sets of complex numbers."""
    b = list(b)
    worst = 0.0
    for v in a:
        j = int(np.argmin([abs(v - u) for u in b]))
        worst = max(worst, abs(v - b.pop(j)))
    return worst
