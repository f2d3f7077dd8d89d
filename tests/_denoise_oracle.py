"""numpy restatement of the patch PCA denoising definition, the oracle of tests/test_denoise.py and
tests/test_gpu_denoise.py.  Two independent routes to the eigenpairs of G = X X^H: ``np.linalg.eigh`` of G, and
``np.linalg.svd`` of the window matrix X itself (G is never formed)."""
import itertools

import numpy as np

EPS = np.finfo(np.float64).eps
Q = 64  # time points per staged tile of k_denoise (XM_CC_Q)
NOISE_SD = 0.05


def window_start(i, p, s):
    """Start of the window of voxel index i along a dim of size s with patch size p: full, shifted inward at an edge."""
    return min(max(i - p // 2, 0), s - p)


def mp_rank(lam, n, rank=None):
    """lam [M] descending, n time points -> (r, sigma, margin).  `rank` None: the Marchenko-Pastur rule, the first p with
    sigma2^2(p) < sigma1^2(p) (M when no p qualifies).  margin: the smallest relative distance
    |sigma2^2 - sigma1^2| / max(sigma2^2, sigma1^2) over the comparisons the scan evaluated (inf with a given rank)."""
    m = len(lam)
    suf = np.zeros(m)
    s = 0.0
    for i in range(m - 1, -1, -1):  # accumulated from i = M - 1 downwards
        s += lam[i]
        suf[i] = s
    margin = np.inf
    if rank is None:
        r = m
        for p in range(m):
            s1 = suf[p] / (m - p)
            s2 = (lam[p] - lam[m - 1]) / (4.0 * np.sqrt((m - p) / n))
            big = max(s1, s2)
            margin = min(margin, abs(s2 - s1) / big if big > 0 else 0.0)
            if s2 < s1:
                r = p
                break
    else:
        r = int(rank)
    sigma = float(np.sqrt(suf[r] / (m - r))) if r < m else 0.0
    return r, sigma, float(margin)


def denoise_window(X, c, rank=None, route="eigh"):
    """One voxel.  X [P, N] the window's FIDs, c the row of the voxel itself -> dict(y, rank, sigma, status, lam,
    margin)."""
    X = np.asarray(X, dtype=np.complex128)
    p, n = X.shape
    bad = dict(y=np.zeros(n, complex), rank=0, sigma=np.nan, status=2, lam=np.full(p, np.nan), margin=np.inf)
    if not np.all(np.isfinite(X)):
        return bad
    if not np.any(X):
        return dict(bad, sigma=0.0, status=1, lam=np.zeros(p))
    try:
        with np.errstate(over="ignore", invalid="ignore"):
            if route == "eigh":
                G = X @ X.conj().T
                if not (np.all(np.isfinite(G)) and np.isfinite(np.sum(np.abs(G) ** 2))):
                    return bad
                e, U = np.linalg.eigh(G)
                e, U = e[::-1], U[:, ::-1]
            else:
                if not np.isfinite(np.sum(np.abs(X) ** 2) ** 2):
                    return bad
                U, s, _ = np.linalg.svd(X, full_matrices=False)
                e = s ** 2
    except np.linalg.LinAlgError:  # an iteration of LAPACK's that did not converge: the kernel's sweep cap
        return dict(bad, y=X[c].copy(), status=3)
    lam = np.maximum(e, 0.0) / n
    r, sigma, margin = mp_rank(lam, n, rank)
    w = U[c, :r] @ U[:, :r].conj().T
    return dict(y=w @ X, rank=r, sigma=sigma, status=0, lam=lam, margin=margin)


def windows(grid, patch):
    """For every voxel of `grid` (row-major): (index tuple, list of the window's voxel index tuples in row-major order of
    the offsets, c)."""
    for idx in np.ndindex(*grid):
        o = [window_start(i, p, s) for i, p, s in zip(idx, patch, grid)]
        rows = [tuple(a + d for a, d in zip(o, off)) for off in itertools.product(*(range(p) for p in patch))]
        yield idx, rows, rows.index(tuple(idx))


def denoise(x, patch, rank=None, route="eigh"):
    """x [..., s_1 ... s_d, N] with d = len(patch) patch dims in front of time, every dim before them batch.  Returns
    dict(y like x (complex128), rank, sigma, status, margin [..., s_1 ... s_d], lam [..., s_1 ... s_d, P])."""
    x = np.asarray(x)
    d = len(patch)
    grid, n = x.shape[-1 - d:-1], x.shape[-1]
    lead = x.shape[:-1 - d]
    P = int(np.prod(patch))
    out = dict(y=np.zeros(x.shape, np.complex128), rank=np.zeros(lead + grid, np.int32), sigma=np.zeros(lead + grid),
               status=np.zeros(lead + grid, np.int32), margin=np.zeros(lead + grid), lam=np.zeros(lead + grid + (P,)))
    win = list(windows(grid, patch))
    for b in np.ndindex(*lead):
        xb = x[b]
        for idx, rows, c in win:
            r = denoise_window(np.stack([xb[j] for j in rows]), c, rank, route)
            for k in out:
                out[k][b + idx] = r[k]
    return out


def make_data(grid, n, k, seed, n_outer=None, noise=NOISE_SD):
    """(clean, noisy), each [n_outer,] grid..., n complex128: K Gaussian-shaped amplitude maps times damped exponentials,
    plus complex noise of standard deviation `noise` (real and imaginary parts sqrt(1/2) of it each)."""
    rng = np.random.default_rng(seed)
    lead = () if n_outer is None else (n_outer,)
    t = np.arange(n) / max(n, 32)
    axes = np.meshgrid(*(np.arange(s, dtype=float) for s in grid), indexing="ij")
    clean = np.zeros(lead + tuple(grid) + (n,), complex)
    for b in np.ndindex(*lead):
        for _ in range(k):
            cen = [rng.uniform(0, max(s - 1, 0)) for s in grid]
            wid = [rng.uniform(0.3, 0.6) * max(s, 2) for s in grid]
            amp = rng.uniform(0.5, 1.0) * np.exp(1j * rng.uniform(-np.pi, np.pi))
            m = amp * np.exp(-sum(((a - c0) / w0) ** 2 for a, c0, w0 in zip(axes, cen, wid)))
            fid = np.exp((-rng.uniform(2.0, 6.0) + 2j * np.pi * rng.uniform(-12.0, 12.0)) * t)
            clean[b] += m[..., None] * fid
    z = (rng.standard_normal(clean.shape) + 1j * rng.standard_normal(clean.shape)) / np.sqrt(2.0)
    return clean, clean + noise * z


# name -> (grid, patch, N, K, n_outer or None): P = 2, 6, 7, 8 (FMA / matrix-core border), 9, 25, 27, 49, 64; N around
# one staged tile (63, 64, 65), the shortest (N = P + 1 at P = 6) and 2048; 1, 2 and 3 patch dims; even patch sizes; a
# patch that is the whole grid; a batch in front
PARITY_CASES = {
    "g4x3_p2x3_n7": ((4, 3), (2, 3), 7, 1, None),
    "g9_p5_n40": ((9,), (5,), 40, 2, None),
    "g9_p7_n40": ((9,), (7,), 40, 2, None),
    "g6x5_p2x4_n40": ((6, 5), (2, 4), 40, 2, None),
    "g6x7_p3x3_n63": ((6, 7), (3, 3), Q - 1, 2, None),
    "g6x7_p3x3_n64": ((6, 7), (3, 3), Q, 2, None),
    "g6x7_p3x3_n65": ((6, 7), (3, 3), Q + 1, 2, None),
    "g6x7_p3x3_n2048": ((6, 7), (3, 3), 2048, 3, None),
    "g5x5x4_p3x3x3_n128": ((5, 5, 4), (3, 3, 3), 128, 3, None),
    "g8x8_p5x5_n256": ((8, 8), (5, 5), 256, 3, None),
    "g8x8_p7x7_n512": ((8, 8), (7, 7), 512, 4, None),
    "g8x8_p8x8_n2048": ((8, 8), (8, 8), 2048, 4, None),
    "g3x3_p1x2_n16": ((3, 3), (1, 2), 16, 1, None),
    "o3_g4x5_p3x3_n96": ((4, 5), (3, 3), 96, 2, 3),
}
MIN_MARGIN = 1e-3  # every comparison of the rank scan is decided by at least this, relatively


def conditions(a, b):
    """The conditions a case must meet to be a parity case, for the results a, b of the two routes: status 0, the same
    rank at every voxel, every comparison of the scan decided by a relative margin >= MIN_MARGIN."""
    return bool(np.all(a["status"] == 0) and np.all(b["status"] == 0) and np.array_equal(a["rank"], b["rank"])
                and min(a["margin"].min(), b["margin"].min()) >= MIN_MARGIN)


# P -> the same tuple: every patch size the kernel accepts, as a 1-D patch (P,) on a grid (P + 1,) with N = 96, K = 2 --
# two windows, each voxel's own row at either end and in the middle.  A list of its own: PARITY_CASES is the set whose
# route gap tests/test_denoise.py pins DENOISE_TOL to.
SWEEP_CASES = {p: ((p + 1,), (p,), 96, 2, None) for p in range(2, 65)}

_cache = {}


def _first_seed(key, case):
    """(clean, noisy, eigh result, svd result, seed) of `case`; the seed is the first that meets `conditions`.  Computed
    once per process and shared: do not modify."""
    if key not in _cache:
        grid, patch, n, k, n_outer = case
        for seed in range(64):
            clean, x = make_data(grid, n, k, seed, n_outer)
            a, b = (denoise(x, patch, route=rt) for rt in ("eigh", "svd"))
            if conditions(a, b):
                break
        else:
            raise AssertionError(f"{key}: no seed below 64 meets the conditions")
        for arr in (clean, x, *a.values(), *b.values()):
            arr.setflags(write=False)
        _cache[key] = (clean, x, a, b, seed)
    return _cache[key]


def parity_case(name):
    """(clean, noisy, eigh result, svd result, seed) of a parity case; the seed is the first that meets `conditions`.
    Computed once per process and shared: do not modify."""
    return _first_seed(name, PARITY_CASES[name])


def sweep_case(p):
    """The same for the patch size p of SWEEP_CASES."""
    return _first_seed(("sweep", p), SWEEP_CASES[p])


def units(res, x):
    """Per voxel, the unit y is measured in: eps max(1, lam_0 / (lam_{r-1} - lam_r)) max |x| (the conditioning of the
    top-r subspace); eps max |x| where r = 0 or r = P."""
    lam, r = res["lam"], res["rank"]
    P = lam.shape[-1]
    gain = np.ones(r.shape)
    it = np.nditer(r, flags=["multi_index"])
    for rv in it:
        rv = int(rv)
        if 0 < rv < P:
            l = lam[it.multi_index]
            gap = l[rv - 1] - l[rv]
            gain[it.multi_index] = max(1.0, l[0] / gap) if gap > 0 else np.inf
    return EPS * gain * np.abs(x).max()


def route_gap(a, b, x):
    """Largest disagreement of two results: y in `units`, sigma relative to itself; the worst voxel of each."""
    dy = np.abs(a["y"] - b["y"]).max(axis=-1) / units(a, x)
    sg = np.where(a["sigma"] > 0, a["sigma"], 1.0)
    return float(dy.max()), float((np.abs(a["sigma"] - b["sigma"]) / sg).max())
