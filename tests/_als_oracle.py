"""TEST ORACLE (not product code): the AsLS baseline of DESIGN.md (rank 4, `xm_baseline_als`) in numpy, in 80-bit
`np.longdouble` by default: per iteration the pentadiagonal system (W + lam D'D) z = W y by band LDL', then
w = p (y > z) + (1 - p) (y < z).  The same function run in float64 gives the rounding error of the recurrence itself,
which the GPU bound is taken from (tests/tool_als_tolerance.py, profiles/als/tolerance.txt).

A row with fewer than two non-zero weights has the singular matrix lam D'D (plus at most one weight): y == z held at
all but one point, the row has converged, and z keeps its value (the AsLS text; `k_als_solve` does the same).

The weight margin of a row is the smallest |y - z| at any point after any iteration.  A comparison y > z that the
kernel decides the other way moves z by far more than rounding, so a case is only usable when its margin lies far above
the bound (tests/test_baseline_als.py asserts 64 x)."""
import functools

import numpy as np

assert np.finfo(np.longdouble).eps <= 2.0 ** -63, (
    "tests/_als_oracle.py needs an extended-precision np.longdouble (eps <= 2^-63); this platform's is "
    f"{np.finfo(np.longdouble).eps!r}")


def _band_solve(y, w, lam):
    """(W + lam D'D) z = W y for rows [n_batch, n]: LDL' of the band, unit lower L with l1 = L[i][i-1], l2 = L[i][i-2].
    D'D has the diagonal 1, 5, 6 ... 6, 5, 1, the first off-diagonal -2, -4 ... -4, -2 and the second 1."""
    nb, n = y.shape
    dt = y.dtype.type
    l1s, l2s, v = np.zeros_like(y), np.zeros_like(y), np.zeros_like(y)
    d1 = d2 = np.ones(nb, y.dtype)
    l1p = u1 = u2 = np.zeros(nb, y.dtype)
    for i in range(n):
        c0 = dt(1 if i in (0, n - 1) else (5 if i in (1, n - 2) else 6))
        a1 = dt(-2 if i in (1, n - 1) else -4) * lam
        di = w[:, i] + lam * c0
        l2 = lam / d2 if i >= 2 else np.zeros(nb, y.dtype)
        l1 = (a1 - l2 * l1p * d2) / d1 if i >= 1 else np.zeros(nb, y.dtype)
        dd = di - l1 * l1 * d1 - l2 * l2 * d2
        u = w[:, i] * y[:, i] - l1 * u1 - l2 * u2
        l1s[:, i], l2s[:, i], v[:, i] = l1, l2, u / dd
        d2, d1, l1p, u2, u1 = d1, dd, l1, u1, u
    z = np.zeros_like(y)
    for i in range(n - 1, -1, -1):
        zi = v[:, i]
        if i + 1 < n:
            zi = zi - l1s[:, i + 1] * z[:, i + 1]
        if i + 2 < n:
            zi = zi - l2s[:, i + 2] * z[:, i + 2]
        z[:, i] = zi
    return z


def als_reference(y, lam, p, n_iter, dtype=np.longdouble):
    """(z [n_batch, n], margin [n_batch]) for real rows y [n_batch, n]: the baseline after n_iter iterations and the
    smallest |y - z| at any point after any iteration.  lam and p enter as the float64 values the kernel receives, and
    1 - p as the float64 difference it forms."""
    y = np.atleast_2d(np.asarray(y, dtype=np.float64)).astype(dtype)
    nb, n = y.shape
    assert n >= 4 and n_iter >= 1
    lam_t, p_t, q_t = dtype(np.float64(lam)), dtype(np.float64(p)), dtype(np.float64(1.0) - np.float64(p))
    z = np.zeros_like(y)
    w = np.ones_like(y)
    live = np.ones(nb, bool)
    margin = np.full(nb, np.inf, dtype)
    for it in range(n_iter):
        if it > 0:
            w = p_t * (y > z) + q_t * (y < z)
            live &= np.count_nonzero(w, axis=1) >= 2
        with np.errstate(all="ignore"):  # the rows that are no longer live divide 0 by 0; their result is dropped
            z = np.where(live[:, None], _band_solve(y, w, lam_t), z)
        margin = np.minimum(margin, np.abs(y - z).min(axis=1))
    return z, margin


# ---- cases ------------------------------------------------------------------------------------------------------------
LINES = ((10.0, 30.0, 616.0), (5.0, 40.0, -308.0), (35.0, 1200.0, 369.6), (45.0, 1800.0, 61.6), (30.0, 1500.0, -184.8))


def make(n, n_batch, seed, sw=2000.0):
    """[n_batch, n] complex128 spectra: two sharp lines on three very broad ones (the generator of
    tests/test_baseline_als.py), row v scaled by 1 + 0.1 v, each with its own noise."""
    t = np.arange(n) / sw
    rng = np.random.default_rng(seed)
    clean = sum(a * np.exp(-d * t) * np.exp(2j * np.pi * f * t) for a, d, f in LINES)
    fid = clean[None, :] * (1 + 0.1 * np.arange(n_batch))[:, None]
    fid = fid + 0.05 * (rng.standard_normal((n_batch, n)) + 1j * rng.standard_normal((n_batch, n)))
    fid[:, 0] *= 0.5
    return np.roll(np.fft.fft(fid, axis=1, norm="ortho"), n // 2, axis=1)


PARAMS = ((1e5, 0.01, 10), (1e5, 0.001, 10), (1e7, 0.001, 3), (1e9, 0.001, 10), (1e2, 0.1, 1))  # (lam, p, n_iter)

# (n, n_batch, (lam, p, n_iter), seed).  Every n of {4, 5, 6, 31, 32, 33, 37, 1000} (the smallest legal lengths, one
# short of / equal to / one past the 32-wide tile, two tiles with a ragged second one, 32 tiles with a ragged last one)
# and every batch of {1, 31, 32, 33, 63, 64, 65, 131} (around one and two 32-row tiles and one 64-thread block of
# k_als_solve, and five tiles / three blocks) appears.  The long rows come with few spectra and the large batches with
# short rows: a case needs every point of every row to keep its distance from the baseline.  The seed of a case is the
# first of 1, 2, 3 ... whose weight margin is at least 64 x the bound of its (lam, p), for the float64 and the float32
# rounding of the spectra both (tests/tool_als_tolerance.py prints the margins).
CASES = (
    (4, 131, PARAMS[0], 1),
    (5, 1, PARAMS[3], 1),
    (5, 33, PARAMS[3], 1),
    (6, 31, PARAMS[4], 1),
    (31, 32, PARAMS[1], 1),
    (32, 64, PARAMS[2], 1),
    (32, 63, PARAMS[1], 2),
    (33, 33, PARAMS[2], 1),
    (37, 65, PARAMS[0], 1),
    (1000, 1, PARAMS[1], 3),
    (1000, 1, PARAMS[2], 1),
    (1000, 3, PARAMS[0], 2),
    (1000, 1, PARAMS[4], 1),
)


def case_id(case):
    n, nb, (lam, p, n_iter), seed = case
    return f"n{n}-b{nb}-lam{lam:g}-p{p:g}-it{n_iter}-s{seed}"


def case_rows(case, single=False):
    """The real rows [n_batch, n] (float64) of a case; `single`: rounded to float32 first, what a complex64 or float32
    input holds."""
    n, nb, _, seed = case
    y = make(n, nb, seed).real
    return y.astype(np.float32).astype(np.float64) if single else y


def scale(y):
    return np.abs(y).max(axis=-1)


@functools.lru_cache(maxsize=None)
def case_reference(case, single=False):
    """(y, z, margin) of a case in long double, computed once and shared; the arrays are read-only."""
    y = case_rows(case, single)
    _, _, (lam, p, n_iter), _ = case
    z, margin = als_reference(y, lam, p, n_iter)
    for a in (y, z, margin):
        a.setflags(write=False)
    return y, z, margin


def figures(case, single, als_core):
    """(e64, scipy, margin) of a case, relative to max |y| of the row: the float64 run of the recurrence and `als_core`
    (the scipy oracle of oracle/xmris_oracle.py) against the long-double run, the largest row of each; the weight margin
    of the long-double run, the smallest row."""
    import warnings

    y, z, margin = case_reference(case, single)
    z64, _ = als_reference(y, *case[2], dtype=np.float64)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        zs = np.stack([als_core(r, *case[2]) for r in y])
    return float(row_gap(z64, z, y).max()), float(row_gap(zs, z, y).max()), float((margin / scale(y)).min())


def row_gap(got, want, y):
    """Per row: the largest |got - want| relative to the row's scale max |y|."""
    d = np.abs(np.asarray(got, dtype=np.longdouble) - np.asarray(want, dtype=np.longdouble)).max(axis=-1)
    return (d / scale(y)).astype(np.float64)


# ---- the GPU bound: 16 x the largest e64 (float64 recurrence against long double, relative to max |y| of the row) among
# the cases with the same (lam, p), rounded up to two digits.  Source: profiles/als/tolerance.txt, written by
# tests/tool_als_tolerance.py on the CPU; no figure here comes from a GPU run.  16 covers what numpy does not reproduce:
# FMA contraction and the order of the operations.
BOUND = {  # (lam, p): largest e64 -> bound
    (1e5, 0.01): 1.2e-9,  # 7.197e-11 (n 1000, 3 rows)
    (1e5, 0.001): 1.9e-8,  # 1.135e-09 (n 1000)
    (1e7, 0.001): 9.0e-9,  # 5.610e-10 (n 32, 64 rows)
    (1e9, 0.001): 3.1e-6,  # 1.919e-07 (n 5, 33 rows)
    (1e2, 0.1): 1.9e-13,  # 1.156e-14 (n 6, 31 rows)
}


def bound(case):
    _, _, (lam, p, _), _ = case
    return BOUND[(lam, p)]
