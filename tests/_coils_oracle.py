"""numpy restatement of the coil-combination definition, the oracle of tests/test_coils.py and
tests/test_gpu_coils.py.  Two independent routes to the direction u: ``np.linalg.eigh`` of the whitened Gram matrix G,
and ``np.linalg.svd`` of the whitened reference L^-1 R (G is never formed)."""
import numpy as np

EPS = np.finfo(np.float64).eps
Q = 64  # time points per staged tile of k_coil_combine (XM_CC_Q)


def linv_of(psi):
    """L^-1 of Psi = L L^H."""
    c = psi.shape[0]
    return np.linalg.solve(np.linalg.cholesky(psi.astype(np.complex128)), np.eye(c, dtype=np.complex128))


def combine(X, R=None, psi=None, method="svd", n_points=1, route="eigh"):
    """One voxel.  X [C, N], R [C, N_R] or None, psi [C, C] or None -> dict(y, w, quality, lam1, lam2, status)."""
    X = np.asarray(X, dtype=np.complex128)
    R = X if R is None else np.asarray(R, dtype=np.complex128)
    c = X.shape[0]
    if not (np.all(np.isfinite(R)) and np.all(np.isfinite(X))):
        return dict(y=np.zeros(X.shape[1], complex), w=np.zeros(c, complex), quality=np.nan, lam1=np.nan, lam2=np.nan,
                    status=2)
    if not np.any(R):
        return dict(y=np.zeros(X.shape[1], complex), w=np.zeros(c, complex), quality=0.0, lam1=0.0, lam2=0.0, status=1)
    li = np.eye(c, dtype=np.complex128) if psi is None else linv_of(psi)
    Rw = li @ R
    lam2 = 0.0
    if method == "first_point":
        m = li @ R[:, :n_points].mean(axis=1)
        u = m / np.linalg.norm(m)
        trace = float(np.sum(np.abs(Rw) ** 2))
        lam1 = float(np.sum(np.abs(u.conj() @ Rw) ** 2))
    elif route == "eigh":
        G = Rw @ Rw.conj().T
        lam, V = np.linalg.eigh(G)
        u, lam1, trace = V[:, -1], float(lam[-1]), float(np.trace(G).real)
        lam2 = float(lam[-2]) if c > 1 else 0.0
    else:
        U, s, _ = np.linalg.svd(Rw, full_matrices=False)
        u, lam1, trace = U[:, 0], float(s[0] ** 2), float(np.sum(s ** 2))
        lam2 = float(s[1] ** 2) if len(s) > 1 else 0.0
    w = li.conj().T @ u
    s0 = np.vdot(w, R[:, 0])
    if abs(s0) > 0:
        w = w * (s0 / abs(s0))
    return dict(y=w.conj() @ X, w=w, quality=lam1 / trace, lam1=lam1, lam2=lam2, status=0)


def combine_batch(x, ref=None, coil_axis=-2, **kw):
    """Every voxel of x [..., C, ..., N] (time last): y [..., N], w [..., C], quality, lam1, lam2, status [...]."""
    xm = np.moveaxis(x, coil_axis, -2)
    rm = None if ref is None else np.moveaxis(ref, coil_axis, -2)
    lead = xm.shape[:-2]
    outs = [combine(xm[i], None if rm is None else rm[i], **kw) for i in np.ndindex(*lead)]
    pack = lambda k, tail: np.array([o[k] for o in outs]).reshape(lead + tail)  # noqa: E731
    return dict(y=pack("y", (xm.shape[-1],)), w=pack("w", (xm.shape[-2],)), quality=pack("quality", ()),
                lam1=pack("lam1", ()), lam2=pack("lam2", ()), status=pack("status", ()))


def make_data(n_outer, c, n_inner, n, seed, snr=(1.0, 5.0)):
    """(n_outer, c, n_inner, n) complex128: per voxel a random complex sensitivity vector times a two-peak damped FID,
    plus complex noise.  Per-sample SNR, drawn per voxel from `snr`: the rms of the voxel's signal over all its coils
    and points divided by the standard deviation of a complex noise sample."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / max(n, 32)
    vox = (n_outer, 1, n_inner, 1)
    f1, f2 = rng.uniform(2, 6, vox), rng.uniform(-9, -4, vox)
    fid = np.exp((-2.0 + 2j * np.pi * f1) * t) + 0.6 * np.exp((-3.0 + 2j * np.pi * f2) * t + 0.7j)
    sens = rng.standard_normal((n_outer, c, n_inner, 1)) + 1j * rng.standard_normal((n_outer, c, n_inner, 1))
    sig = sens * fid
    rms = np.sqrt(np.mean(np.abs(sig) ** 2, axis=(1, 3), keepdims=True))
    sigma = rms / rng.uniform(snr[0], snr[1], vox)
    noise = (rng.standard_normal(sig.shape) + 1j * rng.standard_normal(sig.shape)) / np.sqrt(2.0)
    return sig + sigma * noise


# name -> (n_outer, C, n_inner, N): the smallest shapes at which each part of the kernel can go wrong -- C = 1, 2, 3
# (Jacobi bye, plain-FMA Gram), 8 and 16 (first MFMA tiles, time split over the waves), 33 (padded rows), 64 (LDS maximum);
# N = 1, 33, Q - 1, Q, Q + 1, 2048; coil next to time and not; 1 voxel and 37
PARITY_CASES = {
    "c1_n33_v37": (37, 1, 1, 33),
    "c2_n65_v37": (37, 2, 1, Q + 1),
    "c3_n64_v37": (37, 3, 1, Q),
    "c3_n1_v1": (1, 3, 1, 1),
    "c3_n2048_v1": (1, 3, 1, 2048),
    "c8_n63_v37": (37, 8, 1, Q - 1),
    "c8_n1_inner3": (2, 8, 3, 1),
    "c16_n33_inner3": (5, 16, 3, 33),
    "c16_n2048_v1": (1, 16, 1, 2048),
    "c33_n65_inner3": (2, 33, 3, Q + 1),
    "c64_n63_v37": (37, 64, 1, Q - 1),
    "c64_n2048_v1": (1, 64, 1, 2048),
}


def parity_case(name):
    no, c, ni, n = PARITY_CASES[name]
    return make_data(no, c, ni, n, seed=1000 + sum(map(ord, name)))


SWEEP_COILS = range(1, 65)  # every coil count the kernel accepts


def sweep_case(c):
    """Three voxels of c coils and 65 points, one full staged tile and a ragged one.  Cases of their own: COIL_TOL is
    pinned to PARITY_CASES."""
    return make_data(3, c, 1, Q + 1, seed=7000 + c)


def random_psd(c, seed):
    """A random Hermitian positive-definite C x C matrix with a condition number of a few tens."""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((c, 2 * c)) + 1j * rng.standard_normal((c, 2 * c))
    return a @ a.conj().T / (2 * c) + 0.2 * np.eye(c)


def route_gap_units(a, b):
    """Largest disagreement of two results in units of eps lam1 / (lam1 - lam2), relative to max |y| (y), to
    max |w| (w) and absolute (quality, which is <= 1), per voxel; the worst voxel."""
    gain = EPS * a["lam1"] / (a["lam1"] - a["lam2"])
    dy = np.abs(a["y"] - b["y"]).max(axis=-1) / np.abs(a["y"]).max(axis=-1)
    dw = np.abs(a["w"] - b["w"]).max(axis=-1) / np.abs(a["w"]).max(axis=-1)
    dq = np.abs(a["quality"] - b["quality"])
    return float(np.max(dy / gain)), float(np.max(dw / gain)), float(np.max(dq / gain))
