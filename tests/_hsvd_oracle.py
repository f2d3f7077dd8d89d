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
