"""numpy restatement of remove_lipids: test code, not product code.

M (T x N_l) holds the lipid FIDs as columns (the rows of L, transposed), M = U S V^H;
beta = 1 / (level s_1)^2, w_k = beta s_k^2 / (1 + beta s_k^2); out = y - sum_k u_k w_k (u_k^H y) = (I + beta M M^H)^-1 y
at full rank.  Two routes to (s, U): the Hermitian eigen-decomposition of the smaller Gram matrix (the product's) and the
SVD of M; a dense route for the result; the phantom; the parity case lists."""
import functools

import numpy as np

MIN_WEIGHT = 2.0 ** -20
MAX_RANK = 64

ROWS = (1, 15, 16, 17, 33)
POINTS = (2, 6, 64, 250, 257, 1026)
RANKS = (1, 2, 7, 8, 9, 33, 64)
CASES = tuple((n, T, r) for n in ROWS for T in POINTS for r in RANKS if r <= T)
# ... and the ranks at which the kernel changes the registers that hold the next chunk of its table (16 | 17, 32 | 33)
CLASS_CASES = tuple((17, 257, r) for r in (16, 17, 32))


def subspace_eig(L):
    """(s, U): every singular value, descending with ties to the lower index, and the left vectors of M = L^T, from the
    eigen-decomposition of the smaller of M M^H and M^H M."""
    L = np.asarray(L, dtype=np.complex128)
    n, T = L.shape
    M = L.T
    if T <= n:
        g = M @ M.conj().T
    else:
        g = M.conj().T @ M
    ev, vec = np.linalg.eigh(0.5 * (g + g.conj().T))
    order = np.argsort(-ev, kind="stable")
    s = np.sqrt(np.maximum(ev[order], 0.0))
    v = vec[:, order]
    if T <= n:
        return s, v
    inv = np.where(s > 0, 1.0 / np.where(s > 0, s, 1.0), 0.0)
    return s, (M @ v) * inv[None, :]


def subspace_svd(L):
    """(s, U) from the SVD of M = L^T."""
    u, s, _ = np.linalg.svd(np.asarray(L, dtype=np.complex128).T, full_matrices=False)
    return s, u


def weights(s, level):
    q = (np.asarray(s, dtype=np.float64) / (level * s[0])) ** 2
    return 1.0 / (level * s[0]) ** 2, q / (1.0 + q)


def pick_rank(w, rank=None, avail=None):
    """(r, dropped_weight) of the rank rule."""
    avail = min(len(w), MAX_RANK) if avail is None else min(avail, len(w), MAX_RANK)
    r = max(1, min(int(np.count_nonzero(w >= MIN_WEIGHT)), avail)) if rank is None else int(rank)
    return r, (float(w[r]) if r < len(w) else 0.0)


def basis(L, level=0.01, rank=None, route="eig"):
    """dict(U [T, r], w [r], s (all), beta, rank, dropped_weight)."""
    s, u = (subspace_eig if route == "eig" else subspace_svd)(L)
    beta, w = weights(s, level)
    r, dropped = pick_rank(w, rank, u.shape[1])
    return dict(U=np.ascontiguousarray(u[:, :r]), w=w[:r].copy(), s=s, beta=beta, rank=r, dropped_weight=dropped)


def apply(y, U, w, reverse=False):
    """out[t] = y[t] - sum_k U[t, k] w_k c_k, c_k = sum_t conj(U[t, k]) y[t], rows of y [n, T]; both sums one chain each,
    ascending (or descending with `reverse`)."""
    y = np.asarray(y, dtype=np.complex128)
    T, r = U.shape
    c = np.zeros((y.shape[0], r), dtype=np.complex128)
    for t in (range(T - 1, -1, -1) if reverse else range(T)):
        c += np.conj(U[t])[None, :] * y[:, t, None]
    d = c * w[None, :]
    s = np.zeros_like(y)
    for k in (range(r - 1, -1, -1) if reverse else range(r)):
        s += U[None, :, k] * d[:, k, None]
    return y - s


def dense(y, L, level=0.01):
    """solve(I + beta M M^H, y) per row: the full-rank result without any factorisation of M."""
    L = np.asarray(L, dtype=np.complex128)
    M = L.T
    s1 = np.linalg.norm(M, 2)
    beta = 1.0 / (level * s1) ** 2
    A = np.eye(M.shape[0]) + beta * (M @ M.conj().T)
    return np.linalg.solve(A, np.asarray(y, dtype=np.complex128).T).T


def projector(U, w):
    return (U * w[None, :]) @ U.conj().T


def rel_err(a, b, y):
    """max over rows of max_t |a - b| / max_t |y| (the output is the small remainder of a cancellation: the input's
    magnitude is the scale of every rounding)."""
    scale = np.abs(y).max(axis=-1)
    return float(np.max(np.abs(a - b).max(axis=-1) / np.where(scale > 0, scale, 1.0)))


@functools.lru_cache(maxsize=None)
def make_case(n_rows, T, rank, dynamic=1.0):
    """One parity case, computed once and never changed: N_l = rank lipid rows with singular values over three decades
    (so full rank is `rank` and the weights run from 1 to 1/2 and below), and n_rows data rows: unit noise plus `dynamic`
    times a combination of the lipid rows' components in proportion to their singular values."""
    rng = np.random.default_rng(100000 * n_rows + 100 * T + rank)
    cplx = lambda *s: (rng.standard_normal(s) + 1j * rng.standard_normal(s)) / np.sqrt(2.0)  # noqa: E731
    q1 = np.linalg.qr(cplx(rank, rank))[0]
    q2 = np.linalg.qr(cplx(T, rank))[0]
    sv = 10.0 ** (-3.0 * np.arange(rank) / max(rank - 1, 1))
    L = 7.0 * (q1 * sv[None, :]) @ q2.T  # [rank, T]
    mix = cplx(n_rows, rank)
    lip = (mix * sv[None, :]) @ (q2.T * np.sqrt(T))  # (a strong component of the basis is a strong one of the rows)
    y = cplx(n_rows, T) + dynamic * lip / np.sqrt(rank)
    for a in (L, y):
        a.setflags(write=False)
    return dict(L=L, y=y, level=0.01)


@functools.lru_cache(maxsize=None)
def case_reference(n_rows, T, rank, dtype="complex128", dynamic=1.0):
    """(x, basis, out): the case's rows rounded to `dtype` (the kernel's own input), its basis of `rank` components and
    the oracle's result, computed once."""
    c = make_case(n_rows, T, rank, dynamic)
    x = c["y"].astype(dtype)
    b = basis(c["L"], c["level"], rank)
    out = apply(x, b["U"], b["w"])
    x.setflags(write=False)
    out.setflags(write=False)
    return x, b, out


@functools.lru_cache(maxsize=None)
def phantom(n=12, T=256, bleed=9.0, noise=0.02, seed=2014):
    """A 2-D slice: a disc of brain voxels with four damped lines, a ring of scalp voxels with broad lipid lines whose
    frequency, width, phase and amplitude jitter per voxel; a random complex mixing matrix bleeds lipid into the brain at
    `bleed` times the metabolite norm; complex noise of `noise` times the metabolites' rms.
    dict(data [n, n, T], truth [n, n, T] (metabolites only), scalp, brain [n, n] bool, dt)."""
    rng = np.random.default_rng(seed)
    dt = 1.0 / 2000.0
    t = np.arange(T) * dt
    yy, xx = np.mgrid[:n, :n]
    rad = np.hypot(yy - (n - 1) / 2.0, xx - (n - 1) / 2.0)
    brain = rad <= 0.33 * n
    scalp = (rad > 0.40 * n) & (rad <= 0.52 * n)
    truth = np.zeros((n, n, T), dtype=np.complex128)
    lines = ((-310.0, 6.0, 1.0), (-240.0, 8.0, 0.6), (-215.0, 8.0, 0.5), (-95.0, 10.0, 0.3))  # Hz, 1/s width, amplitude
    for iy, ix in zip(*np.nonzero(brain)):
        for f, d, a in lines:
            truth[iy, ix] += a * (1.0 + 0.2 * rng.standard_normal()) * np.exp((2j * np.pi * f - np.pi * d) * t)
    ns = int(scalp.sum())
    lip = np.zeros((ns, T), dtype=np.complex128)
    for i in range(ns):
        for f, d, a in ((-420.0, 40.0, 1.0), (-445.0, 55.0, 0.5), (-385.0, 50.0, 0.15)):
            f = f + 8.0 * rng.standard_normal()
            d = d * (1.0 + 0.25 * rng.standard_normal())
            a = a * (1.0 + 0.3 * rng.standard_normal())
            lip[i] += a * np.exp(1j * 0.4 * rng.standard_normal()) * np.exp((2j * np.pi * f - np.pi * abs(d)) * t)
    nb = int(brain.sum())
    mix = (rng.standard_normal((nb, ns)) + 1j * rng.standard_normal((nb, ns)))
    leak = mix @ lip
    met = truth[brain]
    leak *= bleed * np.linalg.norm(met) / np.linalg.norm(leak)
    data = np.zeros_like(truth)
    data[brain] = met + leak
    data[scalp] = 30.0 * lip
    sigma = noise * np.sqrt(np.mean(np.abs(met) ** 2))
    data += sigma * (rng.standard_normal(data.shape) + 1j * rng.standard_normal(data.shape)) / np.sqrt(2.0)
    for a in (data, truth, scalp, brain):
        a.setflags(write=False)
    return dict(data=data, truth=truth, scalp=scalp, brain=brain, dt=dt)


def phantom_error(out, ph):
    """|| out - truth || / || truth || over the brain voxels."""
    b = ph["brain"]
    return float(np.linalg.norm(out[b] - ph["truth"][b]) / np.linalg.norm(ph["truth"][b]))


def remove(data, scalp, level=0.01, rank=None, apply_mask=None):
    """The public call on a [ny, nx, T] array: (out, basis)."""
    b = basis(data[scalp], level, rank)
    flat = data.reshape(-1, data.shape[-1])
    out = apply(flat, b["U"], b["w"]).reshape(data.shape)
    if apply_mask is not None:
        out[~apply_mask] = data[~apply_mask]
    return out, b


# ---- the C ABI: a valid argument set and the changes that must be refused before any HIP call ---------------------------
ABI_ORDER = ("x", "y", "n_rows", "xs", "ys", "T", "rank", "tables", "apply", "status", "dtype")
# (pointers of a call without a device: aligned numbers that are never dereferenced)
ABI_OK = dict(x=1 << 20, y=1 << 21, n_rows=4, xs=64, ys=64, T=64, rank=8, tables=1 << 22, apply=None, status=1 << 23,
              dtype=0)
REFUSALS = (dict(T=1), dict(T=65537, xs=65537, ys=65537), dict(rank=0), dict(rank=65), dict(n_rows=-1), dict(x=None),
            dict(y=None), dict(tables=None), dict(status=None), dict(dtype=2), dict(dtype=0x800), dict(xs=63),
            dict(ys=63), dict(tables=(1 << 22) + 8), dict(x=(1 << 20) + 4), dict(y=(1 << 20) + 8),
            dict(y=1 << 20, ys=128), dict(y=(1 << 20) + 64 * 8 * 3))
