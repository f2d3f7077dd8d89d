"""CPU tests of tests/_wg_oracle.py, the numpy restatement of the workgroup toolbox (xmris_amd/csrc/xm_wg.h): every piece
is pinned here before tests/test_gpu_wg.py judges a kernel by it, the matrix families meet the conditions the GPU tests
rely on, and the bounds of the GPU tests are the figures of tests/tool_wg_tolerance.py
(profiles/wg_toolbox/tolerance.txt).  Nothing here imports the package."""
import os
import re

import numpy as np
import pytest

import _wg_oracle as orc

# the worst figures numpy shows on the oracle's own matrices (tests/tool_wg_tolerance.py) and 16 x them, the project's
# margin for a third summation order of the same algorithm.  Jacobi: residual in units of eps ||G||_F, orthonormality
# in units of eps; Cholesky: factor in units of eps ||H + lam D||_F, solution in units of eps cond max |x|.
JACOBI_REF = {"residual": 3.667, "orthonormality": 80.889}
JACOBI_TOL = {"residual": 58.7, "orthonormality": 1294.2}
CHOL_REF = {"factor": 1.359, "solution": 0.451}
CHOL_TOL = {"factor": 21.7, "solution": 7.22}
# derivations, not measurements.  off(G) <= eps ||G||_F is the kernel's own stopping rule; the factor 2 covers the
# rounding of the two norms it compares.  The longest transform (TWO: sincos, +1, hi - lo, two products, the sum; its
# inverse: v - lo, hi - lo, the quotient, x 2, -1, asin) has at most 8 roundings; doubled.
OFF_TOL = 2.0
TRANSFORM_TOL = 16.0
MAX_COND = 1e12  # below this the longdouble Cholesky reference (eps 1.08e-19) is exact to fp64
# the sizes at which the slow part of the tool, the oracle's Jacobi, is re-derived here
JACOBI_RECHECK = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 33, 64)

TOLERANCE_TXT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "wg_toolbox",
                             "tolerance.txt")


# ---- block sum ----------------------------------------------------------------------------------------------------------
def test_tree_sum_is_the_pairwise_tree():
    rng = np.random.default_rng(0)
    x = rng.standard_normal((3, orc.NT))
    want = [sum(float(v) for v in row) for row in x]  # (any order agrees to a few eps here)
    assert np.allclose(orc.tree_sum(x), want, rtol=0, atol=64 * orc.EPS * np.abs(x).sum(axis=1).max())
    one = np.zeros(orc.NT)
    one[[0, 128]] = 1e16, -1e16  # partners of the first level: they cancel before anything else is added
    one[1] = 1.0
    assert orc.tree_sum(one[None])[0] == 1.0
    one[[0, 128, 2, 1]] = 1e16, 0.0, 1.0, -1e16  # red[0] + red[2] rounds the 1 away, then red[0] + red[1] cancels
    assert orc.tree_sum(one[None])[0] == 0.0
    ints = np.arange(orc.NT, dtype=float)
    assert orc.tree_sum(ints[None])[0] == orc.NT * (orc.NT - 1) / 2


# ---- maps -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", range(1, orc.MAXC + 1))
def test_entry_map_is_the_row_major_upper_triangle(c):
    ci, cj = orc.gram_entries(c)
    ne = c * (c + 1) // 2
    assert ne <= orc.NT * orc.MAXE
    flat = [(int(ci[t, m]), int(cj[t, m])) for m in range(orc.MAXE) for t in range(orc.NT)]  # entry number t + 256 m
    assert flat[:ne] == [(i, j) for i in range(c) for j in range(i, c)]
    assert all(p == (0, 0) for p in flat[ne:])


@pytest.mark.parametrize("nb", range(1, orc.MAXC // 8 + 1))
def test_item_map_covers_every_block_and_slice_once(nb):
    nblk, s = orc.gram_slices(nb)
    assert (s == 4) == (nblk < 4) and s in (1, 4)
    nitems = nblk * s
    assert nitems <= 4 * orc.MAXB
    bi, bj, sl = orc.gram_items(nb)
    seen = [(int(bi[v, m]), int(bj[v, m]), int(sl[v, m])) for m in range(orc.MAXB) for v in range(4) if v + 4 * m < nitems]
    want = [(i, j, k) for k in range(s) for i in range(nb) for j in range(i, nb)]
    assert seen == want  # item number v + 4 m = slice * nblk + block
    assert np.all((bi <= bj) & (bj < nb))  # the slots past the items hold valid blocks too


@pytest.mark.parametrize("c", range(1, orc.MAXC + 1))
def test_pairing_visits_every_pair_once_per_sweep(c):
    steps = orc.pairing(c)
    n_pairs = (c + 1) // 2
    assert len(steps) == max(2 * n_pairs - 1, 0) and all(len(s) == n_pairs for s in steps)
    real = [pq for s in steps for pq in s if pq[1] < c]
    assert sorted(real) == [(p, q) for p in range(c) for q in range(p + 1, c)]
    for s in steps:
        players = [x for pq in s for x in pq]
        assert len(set(players)) == 2 * n_pairs  # the rotations of a step touch disjoint rows and columns
        byes = [pq for pq in s if pq[1] >= c]
        assert len(byes) == c % 2 and all(pq[1] == c for pq in byes)  # an odd c rests one player per step
    if c % 2:
        assert sorted(pq[0] for s in steps for pq in s if pq[1] >= c) == list(range(c))  # ... each player once


# ---- Jacobi ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [1, 2, 5, 16, 33])
def test_matrix_families_meet_their_conditions(c):
    gs = orc.jacobi_cases(c)
    assert gs.shape == (4, c, c) and np.all(np.isfinite(gs.view(np.float64)))
    for name, g in zip(orc.FAMILIES, gs):
        assert np.array_equal(g, g.conj().T) and not np.diagonal(g).imag.any(), name
    gram, rank_one, imag, graded = gs
    assert np.linalg.eigvalsh(gram).min() > 0
    lam = np.linalg.eigvalsh(rank_one)
    assert np.allclose(lam[:-1], 1e-3, rtol=0, atol=1e-12 * lam[-1]) and (c == 1 or lam[-1] > 0.1)
    upper = np.triu_indices(c, 1)
    assert not imag[upper].real.any() and imag[upper].imag.all()
    d = np.sqrt(np.diagonal(graded).real)
    assert np.all(np.log2(d[:-1] / d[1:]) > 0.3) if c > 1 else True  # graded: about a binade per row
    unscaled = graded / np.outer(d, d)
    assert np.linalg.cond(unscaled) < 100


def test_oracle_jacobi_diagonalises():
    for c in (1, 2, 3, 8):
        gs = orc.jacobi_cases(c, seed=3)
        lam, v, done = orc.jacobi(gs)
        for k in range(4):
            want = np.linalg.eigvalsh(gs[k])
            scale = max(np.abs(want).max(), 1e-300)
            assert np.allclose(np.sort(lam[k]), want, rtol=0, atol=64 * orc.EPS * scale)
            res, orth = orc.eig_quality(gs[k], lam[k], v[k])
            assert res < 64 and orth < 64
        assert np.all(done <= orc.SWEEPS) and (c == 1) == (done.max() == 0)
    # a matrix that is diagonal already: no sweep, V the identity
    lam, v, done = orc.jacobi(np.diag([3.0, -1.0, 0.0]).astype(complex)[None])
    assert done[0] == 0 and np.array_equal(v[0], np.eye(3)) and list(lam[0]) == [3.0, -1.0, 0.0]


def test_eig_quality_sees_a_wrong_answer():
    g = orc.jacobi_cases(6)[0]
    lam, v = np.linalg.eigh(g)
    good = orc.eig_quality(g, lam, v)
    assert good[0] < 16 and good[1] < 16
    assert orc.eig_quality(g, lam * (1 + 1e-12), v)[0] > 1e3
    assert orc.eig_quality(g, lam, v * (1 + 1e-12))[1] > 1e3
    assert orc.off_units(g, np.diag(lam).astype(complex)) == 0.0 and orc.off_units(g, g) > 1e10


def _recorded():
    text = open(TOLERANCE_TXT).read()
    jac = {int(c): (float(r), float(o), int(s)) for c, r, o, s in
           re.findall(r"jacobi C=\s*(\d+)\s+residual\s+([0-9.]+)\s+orthonormality\s+([0-9.]+)\s+oracle sweeps (\d+)", text)}
    cho = {int(p): (float(f), float(s), float(c)) for p, f, s, c in
           re.findall(r"cholesky P=\s*(\d+)\s+factor\s+([0-9.]+)\s+solution\s+([0-9.e+-]+)\s+cond\s+([0-9.e+-]+)", text)}
    tol = {name: {k: float(v) for k, v in re.findall(r'"(\w+)": ([0-9.e+-]+)', body)}
           for name, body in re.findall(r"(JACOBI_TOL|CHOL_TOL) = \{(.*)\}", text)}
    return jac, cho, tol


def test_tolerance_constants_match_their_tool():
    jac, cho, tol = _recorded()
    assert sorted(jac) == list(range(1, orc.MAXC + 1)) and sorted(cho) == list(range(1, orc.MAXP + 1))
    assert tol == {"JACOBI_TOL": JACOBI_TOL, "CHOL_TOL": CHOL_TOL}
    for k, col in (("residual", 0), ("orthonormality", 1)):
        assert max(v[col] for v in jac.values()) == pytest.approx(JACOBI_REF[k], abs=2e-3)
        assert JACOBI_TOL[k] == pytest.approx(16 * JACOBI_REF[k], abs=0.06)  # (printed to one decimal)
    for k, col in (("factor", 0), ("solution", 1)):
        assert max(v[col] for v in cho.values()) == pytest.approx(CHOL_REF[k], abs=2e-3)
        assert CHOL_TOL[k] == pytest.approx(16 * CHOL_REF[k], abs=0.06)
    assert max(v[2] for v in jac.values()) <= orc.SWEEPS


def test_recorded_jacobi_figures_are_rederived():
    """The oracle's Jacobi takes half a minute over all 64 sizes: re-derived here at the sizes around every change of
    the pairing and the maps, the rest stands as the tool wrote it."""
    jac, _, _ = _recorded()
    for c in JACOBI_RECHECK:
        res, orth, sweeps = orc.jacobi_reference(c)
        assert (res, orth) == pytest.approx(jac[c][:2], abs=2e-3), c
        assert sweeps == jac[c][2], c


def test_recorded_cholesky_figures_are_rederived_and_well_conditioned():
    _, cho, _ = _recorded()
    for p in range(1, orc.MAXP + 1):
        fac, sol, cond = orc.cholesky_reference(p)
        assert fac == pytest.approx(cho[p][0], abs=2e-3) and sol == pytest.approx(cho[p][1], rel=0.01, abs=1e-9), p
        assert cond == pytest.approx(cho[p][2], rel=0.01) and cond <= MAX_COND, (p, cond)


# ---- Cholesky ---------------------------------------------------------------------------------------------------------------
def test_cholesky_cases_are_what_the_probe_takes():
    up, hd, dsc, g, lam = orc.cholesky_cases(7)
    assert up.shape == (6, 7, 7) and list(lam) == list(orc.CHOL_LAMS) * 2
    low = np.tril(np.ones((7, 7), bool))
    assert np.isnan(up[:, low]).all() and np.isfinite(up[:, ~low]).all()  # on and below the diagonal: never read
    assert np.array_equal(hd, dsc) and np.all(hd > 0)
    decades = np.log10(hd.max(axis=1) / hd.min(axis=1))
    assert np.all(decades > 7) and np.all(decades < 9.5)  # Marquardt's scales over eight decades
    h, _ = orc.cholesky_case(7, 0)
    m = orc.damped(up[1], hd[1], dsc[1], lam[1])
    assert np.array_equal(m.astype(float), h + 1e-3 * np.diag(np.diagonal(h)))
    # a column that has always been zero is scaled by 1 (MINPACK)
    z = orc.damped(np.zeros((2, 2)), np.array([4.0, 0.0]), np.array([4.0, 0.0]), 0.5)
    assert np.array_equal(z.astype(float), [[6.0, 0.0], [0.0, 0.5]])


def test_longdouble_cholesky_solves():
    assert np.finfo(orc.LD).eps < 2e-19  # 80-bit here; with a 64-bit long double the reference would prove nothing
    up, hd, dsc, g, lam = orc.cholesky_cases(12)
    for k in range(len(lam)):
        m = orc.damped(up[k], hd[k], dsc[k], lam[k])
        low = orc.cholesky_ld(m)
        assert np.abs(low @ low.T - m).max() <= 64 * np.finfo(orc.LD).eps * np.abs(m).max()
        x = orc.solve_ld(m, g[k])
        r = np.abs(m @ x - g[k].astype(orc.LD)).max()
        assert r <= 1e3 * np.finfo(orc.LD).eps * np.abs(m).max() * np.abs(x).max()
        fac, sol, _ = orc.cholesky_quality(m, g[k], low.astype(float), x.astype(float))
        assert fac <= 1.0 and sol <= 1.0  # the longdouble answer rounded to fp64: within a rounding
        assert orc.cholesky_quality(m, g[k], low.astype(float) * (1 + 1e-9), x.astype(float))[0] > 1e3


# ---- normal equations -------------------------------------------------------------------------------------------------------
def test_lm_q_pts_tiers_are_the_staging_budget():
    for p in range(1, orc.MAXP + 1):
        q = orc.lm_q_pts(p)
        assert q in (128, 64, 32) and (q == 32 or 2 * q * (p + 1) * 8 <= orc.LM_STAGE_BYTES)
        assert q == 128 or 2 * (2 * q) * (p + 1) * 8 > orc.LM_STAGE_BYTES  # the largest tier that fits
    assert [orc.lm_q_pts(p) for p in orc.LM_NORMAL_P] == [128, 128, 128, 128, 64, 64, 32, 32]
    ne = [(p + 1) * (p + 2) // 2 - 1 for p in orc.LM_NORMAL_P]
    assert [-(-e // orc.NT) for e in ne] == [1, 1, 2, 3, 3, 9, 9, 13] and ne[1] == 252 and ne[2] == 275 and ne[-1] == 3320


@pytest.mark.parametrize("p", orc.LM_NORMAL_P)
def test_lm_normal_oracle_is_the_product_of_the_staged_rows(p):
    """Against A^T A of the staged rows A = [J | r].  Both are sums of the same n products in some order: each is within
    gamma_n sum |a_ri a_rj| of the exact sum (gamma_n < n eps), so they differ by at most 2 n eps (|A|^T |A|)_ij."""
    q = orc.lm_q_pts(p)
    for n_points in (1, q, q + 1):
        cases = orc.lm_normal_cases(p, n_points)
        assert cases.shape == (3, n_points, 2, p + 1)
        decades = np.log10(np.abs(cases).max(axis=(1, 2)))
        assert p < 8 or np.all(decades.max(axis=1) - decades.min(axis=1) > 2)  # the columns span decades
        for case in cases:
            a = case.reshape(2 * n_points, p + 1)
            got = orc.lm_normal(a)
            assert np.array_equal(got, got.T)
            bound = 2 * len(a) * orc.EPS * (np.abs(a).T @ np.abs(a))
            assert np.all(np.abs(got - a.T @ a) <= bound)
            if n_points > 1:  # a dropped row or a transposed pair of columns is far outside the bound
                assert np.all(np.abs(orc.lm_normal(a[1:]) - a.T @ a) > bound)
    one = orc.lm_normal(np.array([[3.0, 0.1, 7.0]]))  # one row: the rounded products themselves
    assert np.array_equal(one, np.outer([3.0, 0.1, 7.0], [3.0, 0.1, 7.0]))
    two = orc.lm_normal(np.array([[1e16, 1.0], [1.0, 1.0], [-1e16, 1.0]]))  # row after row: (1e16 + 1) - 1e16 = 0
    assert two[0, 1] == 0.0 and two[1, 1] == 3.0


# ---- transforms -------------------------------------------------------------------------------------------------------------
def test_transforms_are_lmfits_and_invert_each_other():
    bt, u, lo, hi, v = orc.transform_grid()
    assert set(bt) == {orc.FIXED, orc.FREE, orc.LO, orc.HI, orc.TWO} and np.all(lo < hi)
    assert np.array_equal(np.isfinite(lo), np.isin(bt, (orc.LO, orc.HI, orc.TWO))) and np.array_equal(np.isfinite(lo), np.isfinite(hi))
    assert np.abs(u).max() == 1e8 and {1e-6, 1e6} <= set(np.abs(lo)) and {1e-6} <= set(np.abs(hi))
    assert (lo > 0).any() and (hi < 0).any() and ((lo < 0) & (hi > 0)).any()
    p, s = orc.from_internal(bt, u, lo, hi)
    ld_eps = np.finfo(orc.LD).eps
    two, one, other = bt == orc.TWO, bt == orc.LO, bt == orc.HI
    slack = 4 * ld_eps * np.maximum(np.maximum(np.abs(lo), np.abs(hi)), 1.0)
    assert np.all(p[two] >= (lo - slack)[two]) and np.all(p[two] <= (hi + slack)[two])
    assert np.all(p[one] >= (lo - slack)[one]) and np.all(p[other] <= (hi + slack)[other])
    free = ~(two | one | other)
    assert np.array_equal(p[free], u[free].astype(orc.LD)) and np.all(s[free] == 1)
    # hand values: u = 0 is the middle of a two-sided interval, the bound itself of a one-sided one
    p0, s0 = orc.from_internal([orc.TWO, orc.LO, orc.HI], [0.0, 0.0, 0.0], [2.0, 2.0, 2.0], [6.0, 6.0, 6.0])
    assert list(p0) == [4.0, 2.0, 6.0] and list(s0) == [2.0, 0.0, 0.0]
    # the slope is the derivative
    mid = (np.abs(u) > 1e-3) & (np.abs(u) < 10)
    du = np.ldexp(1.0, -20)
    pa, _ = orc.from_internal(bt[mid], u[mid] - du, lo[mid], hi[mid])
    pb, _ = orc.from_internal(bt[mid], u[mid] + du, lo[mid], hi[mid])
    scale = (orc.transform_scale(lo, hi) / orc.EPS)[mid]  # (p cancels at eps_ld |p| / du)
    assert np.all(np.abs((pb - pa) / (2 * du) - s[mid]) <= 1e-9 * scale)
    # round trip through the inverse, v clipped into its bounds
    ui = orc.to_internal(bt, v, lo, hi)
    back, _ = orc.from_internal(bt, ui.astype(np.float64), lo, hi)
    vc = np.clip(v, lo, hi)
    assert np.all(np.abs(back - vc) <= 4 * orc.transform_scale(lo, hi, vc))
    assert (v < lo)[two | one].any() and (v > hi)[two | other].any() and (v == lo)[two].any() and (v == hi)[two].any()


def test_the_formula_alone_leaves_the_upper_bound():
    """Why wg_from_internal returns hi itself at sin u = 1: in fp64, lo + (1 + 1) (hi - lo) / 2 is not always hi."""
    lo, hi = np.float64(-1e6), np.float64(1e-6)
    assert lo + (np.float64(1.0) + 1.0) * (hi - lo) * 0.5 > hi
