"""ORACLE (not product code): non-Cartesian gridding restated in numpy complex128 straight from the definition (DESIGN.md
section 17), with explicit loops over samples and cells and nothing imported from the package.

* `dense_matrix`: the gridding matrix A [cells, S] entry by entry.
* two product routes along an axis: `apply_csr` (every output the sum of its row's non-zero entries in ascending column,
  one term at a time) and `apply_dense` (one matrix product); their largest disagreement in units of `unit` is what the
  kernel tolerance is made from (tests/tool_grid_tolerance.py).
* `adjoint_exact`: the sum the NUFFT approximates; `nufft_adjoint`: the oracle's own chain (dense A, then the [m, G]
  tables); `pipe`: Pipe-Menon on the dense matrix.
* seeded trajectories: `radial`, `random`, `cartesian`."""
import itertools
import math

import numpy as np

EPS = float(np.finfo(np.float64).eps)
EPS32 = float(np.finfo(np.float32).eps)


# ---- trajectories ---------------------------------------------------------------------------------------------------------
def radial(m, spokes, per_spoke):
    """`spokes` diameters of `per_spoke` samples through the centre of a 2-D k-space, golden-angle increments."""
    r = (np.arange(per_spoke) - per_spoke / 2) / per_spoke * m  # [-m/2, m/2)
    out = []
    for s in range(spokes):
        a = s * math.pi * (math.sqrt(5.0) - 1.0) / 2.0
        out.append(np.stack([r * math.cos(a), r * math.sin(a)], axis=1))
    return np.concatenate(out)


def random(m, S, d, seed):
    ms = (m,) * d if np.ndim(m) == 0 else tuple(m)
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-mm / 2, mm / 2, S) for mm in ms], axis=1)


def wrapping(m, S, seed):
    """3-D random samples whose first coordinate lies in (0.275 m, m / 2): at oversampling 2 and W = 4 every footprint
    runs over the upper edge of the grid and wraps."""
    k = random(m, S, 3, seed)
    k[:, 0] = np.random.default_rng(seed + 100).uniform(0.275 * m, np.nextafter(m / 2, 0), S)
    return k


def cartesian(m, d):
    ms = (m,) * d if np.ndim(m) == 0 else tuple(m)
    axes = [np.arange(mm) - mm // 2 for mm in ms]
    return np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, d).astype(np.float64)


def make(shape, seed, dtype=np.complex128):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(dtype)


# ---- the definition -------------------------------------------------------------------------------------------------------
def per_dim(v, d):
    return (v,) * d if np.ndim(v) == 0 else tuple(v)


def oversampled(m, a0):
    G = int(math.ceil(a0 * m))
    return G + G % 2


def beta_of(W, alpha):
    return math.pi * math.sqrt((W / alpha) ** 2 * (alpha - 0.5) ** 2 - 0.8)


def kb(t, W, beta):
    return float(np.i0(beta * math.sqrt(max(1.0 - (2.0 * t / W) ** 2, 0.0))) / np.i0(beta))


def dense_matrix(traj, matrix, a0=2.0, W=4, dens=None):
    """A [cells, S] (C-order cells over the dims) and the per-dim G."""
    traj = np.asarray(traj, dtype=np.float64)
    S, d = traj.shape
    ms = per_dim(matrix, d)
    Gs = tuple(oversampled(m, a0) for m in ms)
    A = np.zeros((int(np.prod(Gs)), S))
    for j in range(S):
        per = []
        for a in range(d):
            m, G = ms[a], Gs[a]
            beta = beta_of(W, G / m)
            u = traj[j, a] * G / m + G // 2
            g0 = math.ceil(u - W / 2.0)
            per.append([((g0 + q) % G, kb((g0 + q) - u, W, beta)) for q in range(W)])
        for combo in itertools.product(*per):
            cell, v = 0, 1.0
            for a, (g, w) in enumerate(combo):
                cell = cell * Gs[a] + g
                v = v * w
            A[cell, j] += v * (1.0 if dens is None else float(dens[j]))
    return A, Gs


def apply_dense(M, x, axis):
    """M @ x along `axis` as one matrix product."""
    y = np.tensordot(M.astype(np.complex128), np.asarray(x, dtype=np.complex128), axes=([1], [axis]))
    return np.moveaxis(y, 0, axis)


def apply_csr(M, x, axis):
    """M @ x along `axis`: every output row the sum of its non-zero entries, ascending column, one term at a time."""
    xm = np.moveaxis(np.asarray(x, dtype=np.complex128), axis, 0)
    y = np.zeros((M.shape[0],) + xm.shape[1:], dtype=np.complex128)
    for r in range(M.shape[0]):
        acc = np.zeros(xm.shape[1:], dtype=np.complex128)
        for j in np.flatnonzero(M[r]):
            acc = acc + M[r, j] * xm[j]
        y[r] = acc
    return np.moveaxis(y, 0, axis)


def unit(M, x, axis):
    """U per output: eps64 sum_e |val_e| |x_e|."""
    y = np.tensordot(np.abs(M), np.abs(np.asarray(x, dtype=np.complex128)), axes=([1], [axis]))
    return EPS * np.moveaxis(y, 0, axis)


def gap(a, b, u):
    """max |a - b| / U over the outputs with U > 0 (an output with U = 0 must agree exactly)."""
    diff = np.abs(np.asarray(a, dtype=np.complex128) - b)
    assert np.all(diff[u == 0] == 0)
    return float((diff[u > 0] / u[u > 0]).max()) if np.any(u > 0) else 0.0


def deapodization(m, G, W, beta):
    c = np.zeros(m)
    for p in range(m):
        z = np.sqrt(complex(beta ** 2 - (math.pi * W * (p - m // 2) / G) ** 2))
        ratio = 1.0 if abs(z) < 1e-8 else (z / np.sinh(z)).real
        c[p] = math.sqrt(G / m) * float(np.i0(beta)) * ratio / W
    return c


def image_table(m, G, W):
    """F [m, G]."""
    c = deapodization(m, G, W, beta_of(W, G / m))
    F = np.zeros((m, G), dtype=np.complex128)
    for p in range(m):
        for g in range(G):
            F[p, g] = c[p] * np.exp(2j * math.pi * (((g - G // 2) * (p - m // 2)) % G) / G) / math.sqrt(G)
    return F


def nufft_adjoint(x, traj, matrix, a0=2.0, W=4, dens=None, axis=0):
    """The oracle's chain: dense gridding, then F along every gridded dim.  `axis`: the sample axis of x."""
    d = np.asarray(traj).shape[1]
    ms = per_dim(matrix, d)
    A, Gs = dense_matrix(traj, matrix, a0, W, dens)
    y = apply_dense(A, x, axis)
    y = y.reshape(y.shape[:axis] + Gs + y.shape[axis + 1:])
    for a in range(d):
        y = apply_dense(image_table(ms[a], Gs[a], W), y, axis + a)
    return y


def nufft_forward(img, traj, matrix, a0=2.0, W=4, axis=0):
    """The Hermitian transpose of `nufft_adjoint` with unit density; `axis`: the first image axis."""
    d = np.asarray(traj).shape[1]
    ms = per_dim(matrix, d)
    A, Gs = dense_matrix(traj, matrix, a0, W)
    y = np.asarray(img, dtype=np.complex128)
    for a in range(d):
        y = apply_dense(image_table(ms[a], Gs[a], W).conj().T, y, axis + a)
    y = y.reshape(y.shape[:axis] + (A.shape[0],) + y.shape[axis + d:])
    return apply_dense(A.T, y, axis)


def adjoint_exact(x, traj, matrix, dens=None, axis=0):
    """(1 / sqrt(prod m)) sum_j dens_j x_j exp(2 pi i k_j . (p - m // 2) / m), the image dims in place of `axis`."""
    traj = np.asarray(traj, dtype=np.float64)
    S, d = traj.shape
    ms = per_dim(matrix, d)
    E = np.ones((1, S), dtype=np.complex128)
    for a in range(d):
        p = np.arange(ms[a]) - ms[a] // 2
        Ea = np.exp(2j * np.pi * np.outer(p, traj[:, a]) / ms[a])  # [m_a, S]
        E = (E[:, None, :] * Ea[None, :, :]).reshape(-1, S)
    E = E * (1.0 if dens is None else np.asarray(dens, dtype=np.float64)[None, :]) / math.sqrt(float(np.prod(ms)))
    y = apply_dense_complex(E, x, axis)
    return y.reshape(y.shape[:axis] + ms + y.shape[axis + 1:])


def apply_dense_complex(M, x, axis):
    y = np.tensordot(M, np.asarray(x, dtype=np.complex128), axes=([1], [axis]))
    return np.moveaxis(y, 0, axis)


def pipe(traj, matrix, a0=2.0, W=4, iterations=10):
    A1, _ = dense_matrix(traj, matrix, a0, W)
    w = np.ones(A1.shape[1])
    for _ in range(iterations):
        w = w / (A1.T @ (A1 @ w))
    return w


# ---- the cases of tests/tool_grid_tolerance.py ----------------------------------------------------------------------------
# name: (trajectory, matrix, oversampling, W, shape of x, sample axis); the GPU parity tests run the same cases
PARITY_CASES = {
    "2d_random": (lambda: random(6, 37, 2, 1), 6, 2.0, 4, (3, 37, 5), 1),
    "1d_w6": (lambda: random(8, 20, 1, 2), 8, 2.0, 6, (2, 20, 3), 1),
    "3d_wraps": (lambda: wrapping(4, 50, 3), 4, 2.0, 4, (50, 4), 0),
    "2d_w5_odd": (lambda: random((5, 6), 31, 2, 4), (5, 6), 2.0, 5, (2, 3, 31), 2),
    "radial": (lambda: radial(8, 7, 16), 8, 2.0, 4, (3, 112, 5), 1),
}


def parity_case(name, dtype=np.complex128):
    """(x rounded to dtype, trajectory, matrix, a0, W, axis, dense A, A x by the CSR route, unit)."""
    tr, matrix, a0, W, shape, axis = PARITY_CASES[name]
    traj = tr()
    x = make(shape, seed=len(name), dtype=dtype)
    A, _ = dense_matrix(traj, matrix, a0, W)
    return x, traj, matrix, a0, W, axis, A, apply_csr(A, x, axis), unit(A, x, axis)


def worst_route_gap():
    worst = 0.0
    for name in PARITY_CASES:
        x, traj, matrix, a0, W, axis, A, y, u = parity_case(name)
        worst = max(worst, gap(y, apply_dense(A, x, axis), u))
        xs = apply_dense(A.T, y, axis)  # (degridding: the transpose on the gridded data)
        worst = max(worst, gap(apply_csr(A.T, y, axis), xs, unit(A.T, y, axis)))
    return worst


# name: (trajectory, matrix, W); oversampling 2, unit density, x = make((S, 3), seed 7)
ACCURACY_CASES = {
    "radial_m16_w4": (lambda: radial(16, 26, 32), 16, 4),
    "radial_m16_w6": (lambda: radial(16, 26, 32), 16, 6),
    "random_m16_w4": (lambda: random(16, 400, 2, 5), 16, 4),
    "random_m16_w6": (lambda: random(16, 400, 2, 5), 16, 6),
    "cartesian_m8_w4": (lambda: cartesian(8, 2), 8, 4),
    "cartesian_m8_w6": (lambda: cartesian(8, 2), 8, 6),
}


def accuracy_case(name):
    """(x [S, 3], trajectory, matrix, W, the exact sum [m, m, 3])."""
    tr, matrix, W = ACCURACY_CASES[name]
    traj = tr()
    x = make((len(traj), 3), seed=7)
    return x, traj, matrix, W, adjoint_exact(x, traj, matrix)


def accuracy(got, exact):
    return float(np.abs(got - exact).max() / np.abs(exact).max())


# ---- what xm_axis_sparse must refuse before any HIP call (CPU and GPU tests share the list) --------------------------------
# changes to a valid call (x, y, rowptr, col, val, n_outer, n, n_rows, n_inner, dtype); a pointer entry is None (null),
# "x" (the same address as x) or an integer offset in bytes from the valid pointer
REFUSALS = [dict(n=0), dict(n=1 << 31), dict(n_rows=0), dict(n_rows=1 << 31), dict(x=None), dict(y=None), dict(rowptr=None),
            dict(col=None), dict(val=None), dict(y="x"), dict(dtype=2), dict(dtype=-1), dict(n_outer=-1), dict(n_inner=-1),
            dict(n_outer=1 << 40, n_inner=1 << 40), dict(n_outer=1 << 31, n_inner=1), dict(x=4), dict(y=4),
            dict(dtype=1, x=8), dict(dtype=1, y=8)]
