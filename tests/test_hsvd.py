"""CPU tests of remove_water: the oracle's two routes agree within the figures HSVD_TOL is made from, every GPU parity
case meets the conditions that make the comparison meaningful (the same in-band set, no pole near a band edge, status 0,
cond(B) <= 1e4), the oracle has the properties of the definition, and every validation error
fires before the library is reached.

The tests of the oracle alone import nothing from the package and pass without the feature; the validation, ABI and
vocabulary tests fail without it."""
import functools
import os
import re

import numpy as np
import pytest

import _hsvd_oracle as orc

# the largest disagreement of the oracle's two routes (eigh of G against the SVD of H) over orc.PARITY_CASES, per
# quantity -- tests/tool_hsvd_tolerance.py, recorded in profiles/hsvd/tolerance.txt -- and 16 x that: y in units of
# max |x|, f as arg z (radians per sample), d as ln |z|, a in units of |a_k|, the last three over in-band components
ROUTE_GAP = {"y": 4.67e-08, "f": 3.46e-09, "d": 1.24e-09, "a": 5.16e-07}
HSVD_TOL = {"y": 7.5e-07, "f": 5.5e-08, "d": 2.0e-08, "a": 8.3e-06}
EDGE_HZ = 0.5
MAX_COND = 1e4
CLEAN_RMS = 1.8e-9  # noise-free N = 512, M = 32, K = 6, route eigh: rms |y - metabolites| (the same tool)
# the oracle's largest distance from the closed-form truth over orc.VALUE_CASES and both routes (the same tool and file):
# "pole" max |dz|, "amp" the amplitudes relative, "sig" y in units of max |x| -- and 16 x that, the bound of the kernel's
# distance from the same truth (its Jacobi and QR against LAPACK: two roundings of one answer)
COMB_GAP = {"pole": 3.86e-15, "amp": 3.78e-13, "sig": 8.88e-15}
COMB_TOL = {"pole": 6.2e-14, "amp": 6.1e-12, "sig": 1.4e-13}
# max |x - B a| / max |x| of the oracle's full model on orc.MODEL_CASES, the larger of the two routes (the same tool)
MODEL_RESIDUAL = {"pair-1Hz": 6.7e-12, "pair-0.2Hz": 5.3e-11, "range-1e6": 1.1e-09, "real-valued": 2.8e-14, "growing": 7.0e-14}


@functools.lru_cache(maxsize=None)
def routes(name):
    return orc.route_gap(name)


@pytest.mark.parametrize("name", list(orc.PARITY_CASES))
def test_routes_agree_and_cases_meet_the_conditions(name):
    g, a, b = routes(name)
    print(name, g, a["cond"].max())
    for key in HSVD_TOL:
        assert g[key] <= HSVD_TOL[key] / 16 * 1.01, (key, g[key])
    assert np.array_equal(a["removed"], b["removed"])
    for r in (a, b):
        assert np.all(r["status"] == 0) and np.all(r["n_removed"] >= 1)
        f = r["frequency"]
        assert np.min(np.minimum(np.abs(f - orc.BAND[0]), np.abs(f - orc.BAND[1]))) >= EDGE_HZ
        assert np.all(r["cond"] <= MAX_COND), r["cond"].max()


def test_tolerance_constants_match_their_tool():
    worst = {k: max(routes(name)[0][k] for name in orc.PARITY_CASES) for k in HSVD_TOL}
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "hsvd", "tolerance.txt")).read()
    recorded = dict(re.findall(r'"([yfda])": ([0-9.e+-]+)', text.split("HSVD_TOL =")[1]))
    for k in HSVD_TOL:
        assert worst[k] == pytest.approx(ROUTE_GAP[k], rel=0.02), (k, worst[k])
        assert HSVD_TOL[k] == pytest.approx(16 * worst[k], rel=0.02)
        assert float(recorded[k]) == HSVD_TOL[k]


def test_comb_and_model_constants_match_their_tool():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "hsvd", "tolerance.txt")).read()
    worst = {k: max(comb_routes(name)[2][rt][k] for name in orc.VALUE_CASES for rt in ("eigh", "svd")) for k in COMB_TOL}
    recorded = dict(re.findall(r'"(pole|amp|sig)": ([0-9.e+-]+)', text.split("COMB_TOL =")[1].split("\n")[0]))
    for k in COMB_TOL:
        assert worst[k] == pytest.approx(COMB_GAP[k], rel=0.02), (k, worst[k])
        assert COMB_TOL[k] == pytest.approx(16 * worst[k], rel=0.02)
        assert float(recorded[k]) == COMB_TOL[k]
    recorded = dict(re.findall(r'"([^"]+)": ([0-9.e+-]+)', text.split("MODEL_RESIDUAL =")[1].split("\n")[0]))
    assert set(recorded) == set(MODEL_RESIDUAL) == set(orc.MODEL_CASES)
    for name in orc.MODEL_CASES:
        larger = max(model_routes(name)[1].values())
        assert larger == pytest.approx(MODEL_RESIDUAL[name], rel=0.02), (name, larger)
        assert float(recorded[name]) == MODEL_RESIDUAL[name]


# ---- the kernel's pole iteration restated: what it computes, and which of its branches a case enters --------------------
@functools.lru_cache(maxsize=None)
def comb_routes(name):
    return orc.comb_routes(name)


@functools.lru_cache(maxsize=None)
def model_routes(name):
    return orc.model_routes(name)


@functools.lru_cache(maxsize=None)
def restated(name, row=0):
    """(z, Q, counters) of the restated iteration: W from the zero-skipping Jacobi on a comb case, from the oracle's eigh
    on a row of a parity case."""
    if name in orc.PARITY_CASES:
        x, _, m, k = orc.parity_case(name)
        return orc.restated_poles(orc.oracle_w(x[row], m, k))
    x, m, k = orc.comb_case(name)[:3]
    return orc.restated_poles(orc.jacobi_w(x, m, k))


def eigenvalue_bound(q, steps):
    """How far the restated eigenvalues may lie from numpy's, to first order.  Every QR step and every Householder step
    is a unitary similarity, so ||H||_F = ||Q||_F throughout and the computed result is exact for Q + E.  A QR step
    passes every entry through at most 2 rotations from the left and 2 from the right, each a complex p x + q y of at
    most 3 eps relative to the pair's norm, and moves the diagonal by the shift twice (2 eps): 14 eps ||Q||_F a step.
    A reflection from one side is a dot product of at most K terms, a scaling and an update, (K + 4) eps ||Q||_F; two
    sides, K - 2 columns.  So ||E||_F <= (14 steps + 2 (K + 4) (K - 2)) eps ||Q||_F; LAPACK's own Hessenberg-QR is
    allowed the same, and an eigenvalue moves by at most its condition number 1 / |y^H x| times ||E||."""
    k = q.shape[0]
    _, vec = np.linalg.eig(q)
    s = np.linalg.norm(np.linalg.inv(vec), axis=1) * np.linalg.norm(vec, axis=0)
    return 2.0 * float(s.max()) * (14 * steps + 2 * (k + 4) * max(k - 2, 0)) * orc.EPS * float(np.linalg.norm(q))


@pytest.mark.parametrize("name", list(orc.PARITY_CASES) + orc.VALUE_CASES)
def test_restated_pole_iteration_finds_the_eigenvalues(name):
    rows = range(orc.PARITY_CASES[name][4]) if name in orc.PARITY_CASES else (0,)
    for row in rows:
        z, q, count = restated(name, row)
        err, bound = orc.match_sets(z, np.linalg.eigvals(q)), eigenvalue_bound(q, count["steps"])
        print(name, row, count, f"{err:.2e} = {err / (orc.EPS * np.linalg.norm(q)):.1f} eps ||Q||_F, bound {bound:.2e}")
        assert err <= bound
        if name in orc.PARITY_CASES:  # noisy FIDs: Wilkinson's shift alone, from the top of the matrix, no exact zero
            assert count["exceptional"] == count["l_positive"] == count["sigma0"] == count["hnorm"] == 0 and count["max_its"] <= 8


# what the restated iteration does on every comb case: (QR steps, exceptional shifts, largest `its`, steps on a window
# with l > 0, Householder columns skipped for sigma == 0, deflation tests that fell back on hnorm)
COMB_COUNTS = {
    "P2-M4-N16-rho0.9": (1, 0, 1, 0, 0, 1),
    "P3-M6-N24-rho0.9": (12, 1, 11, 0, 0, 0),
    "P4-M8-N40-rho0.9": (19, 1, 14, 0, 1, 3),
    "P5-M16-N64-rho0.9": (22, 1, 15, 0, 2, 21),
    "P8-M16-N80-rho0.9": (31, 1, 15, 0, 1, 7),
    "P16-M17-N67-rho0.8": (57, 1, 16, 0, 0, 29),
    "P16-M32-N160-rho0.8": (57, 1, 16, 0, 1, 46),
    "P31-M63-N250-rho0.8": (104, 1, 18, 0, 2, 224),
    "P32-M64-N320-rho0.8": (107, 1, 18, 0, 1, 213),
    "P32-M64-N320-rho1.0": (94, 1, 18, 0, 1, 199),
    "P5-M16-N64-rho0.9-real": (22, 1, 15, 0, 2, 40),
    "P5-M16-N64-rho1.0-real": (22, 1, 15, 0, 2, 40),
    "G1+3-A2-M8-N23": (5, 0, 4, 5, 0, 0),
}


@pytest.mark.parametrize("name", orc.VALUE_CASES)
def test_comb_cases_reach_the_branches_the_noisy_cases_never_do(name):
    """The counters are those of the restatement, with W from a sequential Jacobi; the kernel's parallel ordering may
    order tied eigenvalues of G otherwise, and then take a few steps more or fewer.  What does not depend on that order:
    Q is a weighted cyclic permutation (exact zeros, zero diagonal).  What the counters show is that these branches are
    entered, not that their results matter: any shift leaves the eigenvalues alone, so a wrong value of the exceptional
    shift can only cost steps, and on the complex combs the iteration converges without it too (in up to 2.7 times the
    steps, `its` up to 44, rounding errors breaking the symmetry).  Only the real-valued combs need the branch, see
    test_real_combs_do_not_converge_without_the_exceptional_shift.  No committed case reaches the second exceptional
    shift (`its` == 20; the largest is 18, and a search over P <= 32, rho in (0.8, 0.9, 1) found none), and wherever
    these matrices have tst == 0 the subdiagonal entry is an exact zero too, so the deflation is the same with or
    without the hnorm fallback: the `its` == 20 arm and the fallback's value stay unverified."""
    z, q, c = restated(name)
    got = (c["steps"], c["exceptional"], c["max_its"], c["l_positive"], c["sigma0"], c["hnorm"])
    print(name, c)
    assert got == COMB_COUNTS[name]
    if name in orc.COMB_CASES or name in orc.REAL_COMBS:
        p = dict(orc.COMB_CASES, **orc.REAL_COMBS)[name][0]
        assert np.count_nonzero(q) == p and not np.diag(q).any()  # a weighted cyclic permutation
        if p >= 3:
            assert c["exceptional"] >= 1 and c["max_its"] >= 10
        if p >= 4:
            assert c["hnorm"] >= 1
    truth = orc.comb_case(name)[4]
    assert orc.match_sets(z, truth) <= COMB_TOL["pole"]


@pytest.mark.parametrize("name", list(orc.REAL_COMBS))
def test_real_combs_do_not_converge_without_the_exceptional_shift(name):
    """The mutation check, committed: on a real-valued comb Wilkinson's shift is exactly zero at every step and an
    unshifted step maps a weighted cyclic permutation to another one, exact zeros included, so with the exceptional
    branch disabled the restated iteration reaches its cap of 30 K steps (the kernel's status 3); with it, 22 steps.
    The GPU tests run these cases and require status 0 and the closed-form poles."""
    x, m, k = orc.comb_case(name)[:3]
    w = orc.jacobi_w(x, m, k)
    with pytest.raises(np.linalg.LinAlgError, match="cap"):
        orc.restated_poles(w, exceptional=False)
    assert restated(name)[2]["exceptional"] == 1 and not shift_q_imag(w)


def shift_q_imag(w):
    return np.abs(orc.shift_matrix(w).imag).max()


def test_some_comb_case_skips_a_householder_column_and_one_grid_case_deflates_mid_matrix():
    assert sum(COMB_COUNTS[n][4] >= 1 for n in orc.COMB_CASES) >= 6  # sigma == 0 (not P = 2, 3: nothing to reduce; nor
    # every P >= 4: whether a column below the subdiagonal is empty depends on where hs_select puts the classes)
    assert all(COMB_COUNTS[n][3] >= 1 for n in orc.GRID_CASES)  # l > 0


def test_search_for_a_window_that_starts_below_row_zero():
    """The two-level combs on a grid (orc.grid_fid) are the candidates for a deflation in the middle of the matrix:
    Q is unitary with two degenerate groups.  Of the eight tried, the restated iteration meets l > 0 on one, which is
    orc.GRID_CASES.  Inside a degenerate group of G the kernel's eigenvector basis may differ from the restatement's, and
    with it Q's Hessenberg form: that the kernel meets l > 0 on this case is likely, not proven."""
    found = []
    for k1, k2, amp, m, n in orc.GRID_SEARCH:
        x = orc.grid_fid(k1, k2, amp, n)[0]
        count = orc.restated_poles(orc.jacobi_w(x, m, k1 + k2))[2]
        if count["l_positive"]:
            found.append((k1, k2, amp, m, n))
    assert found == list(orc.GRID_CASES.values())


@pytest.mark.parametrize("name", orc.VALUE_CASES)
def test_comb_cases_meet_the_parity_conditions(name):
    g, r, tg = comb_routes(name)
    x, m, k, band, z, a, k0, y = orc.comb_case(name)
    print(name, g, tg)
    for key in HSVD_TOL:
        assert g[key] <= HSVD_TOL[key] / 16, (key, g[key])
    assert np.array_equal(r["eigh"]["removed"], r["svd"]["removed"])
    for rt in r:
        assert r[rt]["status"] == 0 and r[rt]["n_removed"] == 1 and r[rt]["removed"][k0] == 1
        f = r[rt]["frequency"]
        assert np.min(np.minimum(np.abs(f - band[0]), np.abs(f - band[1]))) >= EDGE_HZ
        assert r[rt]["cond"] <= MAX_COND
        assert all(tg[rt][key] <= COMB_GAP[key] * 1.01 for key in COMB_GAP)


@pytest.mark.parametrize("name", list(orc.MODEL_CASES))
def test_model_cases_are_decomposed_by_both_routes_and_stay_clear_of_the_band_edges(name):
    x, m, k, band, f, d, a = orc.model_case(name)
    r, res = model_routes(name)
    print(name, res, [r[rt]["cond"] for rt in r])
    assert np.all(np.minimum(np.abs(f - band[0]), np.abs(f - band[1])) >= EDGE_HZ)
    want = ((f >= band[0]) & (f <= band[1]))[np.argsort(f, kind="stable")].astype(np.int32)
    for rt in r:
        assert r[rt]["status"] == 0 and np.array_equal(r[rt]["removed"], want)
    if name == "real-valued":
        assert not x.imag.any()


@pytest.mark.parametrize("route", ["eigh", "svd"])
def test_noise_free_peaks_come_back_and_the_metabolites_stay(route):
    n, m = 512, 32
    x, met, pars = orc.make_fid(n, 11, 1, noise=0.0)
    p = pars[0]
    r = orc.hsvd(x[0], m, 6, route=route)
    assert r["status"] == 0 and r["n_removed"] == 3
    f_true = np.concatenate([p["fw"], p["fm"]])
    d_true = np.concatenate([p["dw"], p["dm"]])
    a_true = np.concatenate([p["aw"], p["am"]])
    o = np.argsort(f_true)
    z_true = np.exp((2j * np.pi * f_true[o] - d_true[o]) * orc.DT)
    rms = np.sqrt(np.mean(np.abs(r["y"] - met[0]) ** 2))
    print(route, "rms", rms, "poles", np.abs(r["z"] - z_true).max(), "amplitudes", (np.abs(r["a"] - a_true[o]) / np.abs(a_true[o])).max())
    assert rms <= 16 * CLEAN_RMS
    assert np.abs(r["z"] - z_true).max() <= HSVD_TOL["f"]
    assert np.all(np.abs(r["a"] - a_true[o]) <= HSVD_TOL["a"] * np.abs(a_true[o]))
    assert list(r["removed"]) == [1, 1, 1, 0, 0, 0]


def test_removing_water_leaves_the_metabolites():
    x, met, _ = orc.make_fid(2048, 1, 1)
    r = orc.hsvd(x[0], 64, 20)
    rms = lambda v: float(np.sqrt(np.mean(np.abs(v) ** 2)))  # noqa: E731
    assert r["status"] == 0 and rms(r["y"] - met[0]) < 0.1 and rms(x[0] - met[0]) > 1.0


def test_status_cases(monkeypatch):
    x, _, _ = orc.make_fid(64, 3, 1)
    x = x[0]
    far = orc.hsvd(x, 16, 4, band=(1000.0, 1100.0))  # no pole there
    assert far["status"] == 1 and far["n_removed"] == 0 and np.array_equal(far["y"], x) and np.all(np.isfinite(far["frequency"]))
    zero = orc.hsvd(np.zeros(64, complex), 16, 4)
    assert zero["status"] == 1 and not zero["y"].any() and np.isnan(zero["frequency"]).all() and zero["n_removed"] == 0
    for bad_value in (np.nan, np.inf):
        bad = x.copy()
        bad[7] = bad_value
        o = orc.hsvd(bad, 16, 4)
        assert o["status"] == 2 and not o["y"].any() and np.isnan(o["amplitude"]).all() and not o["removed"].any()
    assert orc.hsvd(x * 1e200, 16, 4)["status"] == 2  # G overflows
    one = np.zeros(64, complex)
    one[0] = 1.0  # G = e_0 e_0^T: the pole is zero, z^t is not finite
    o = orc.hsvd(one, 16, 1)
    assert o["status"] == 4 and np.array_equal(o["y"], one) and np.isnan(o["damping"]).all()

    def no_convergence(*a, **k):
        raise np.linalg.LinAlgError("Eigenvalues did not converge")

    monkeypatch.setattr(np.linalg, "eigvals", no_convergence)
    o = orc.hsvd(x, 16, 4)
    assert o["status"] == 3 and np.array_equal(o["y"], x) and np.isnan(o["phase"]).all()


# ---- validation: every error fires before any native call -----------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    from xmris_amd import _lib
    from xmris_amd import device as dev

    def boom(*a, **k):
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "call", boom)
    monkeypatch.setattr(dev, "to_device", boom)
    monkeypatch.setattr(dev, "hsvd_rows", boom)


def _la(shape=(3, 200), dims=("x", "time"), time=True, dtype=complex, dt=2e-4):
    from xmris_amd import LabeledArray

    rng = np.random.default_rng(1)
    v = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    v = v.real.copy() if dtype is float else v.astype(dtype)
    coords = {"time": np.arange(shape[dims.index("time")]) * dt} if time and "time" in dims else {}
    return LabeledArray(v, dims, coords)


@pytest.mark.parametrize("kw, word", [
    (dict(dim="t"), "dim"),
    (dict(band=(50.0, -50.0)), "band"),
    (dict(band=(0.0, np.inf)), "band"),
    (dict(band=5.0), "band"),
    (dict(n_cols=1), "n_cols"),
    (dict(n_cols=65), "n_cols"),
    (dict(n_cols=32.5), "n_cols"),
    (dict(rank=0), "rank"),
    (dict(rank=33), "rank"),
    (dict(rank=16, n_cols=16), "rank"),
    (dict(rank=2.5), "rank"),
    (dict(n_cols=64, rank=4), "n_cols"),  # on 100 points: fewer than 2 * 64
    (dict(dt=0.0), "dt"),
    (dict(dt=-1e-3), "dt"),
    (dict(dt=np.nan), "dt"),
])
def test_validation_errors_name_their_argument(no_library, kw, word):
    from xmris_amd import remove_water

    da = _la((3, 100)) if kw.get("n_cols") == 64 else _la()
    with pytest.raises(ValueError, match=word):
        remove_water(da, **kw)
    with pytest.raises(ValueError, match=word):
        da.xmr.remove_water(**kw)


def test_validation_of_input_length_and_time_coordinate(no_library):
    from xmris_amd import remove_water

    with pytest.raises(ValueError, match="n_cols"):
        remove_water(_la((2, 127)))  # < 2 * 64
    with pytest.raises(ValueError, match="16384"):
        remove_water(_la((1, 16385)))
    with pytest.raises(ValueError, match="dt"):
        remove_water(_la(time=False))
    uneven = _la()
    uneven.coords["time"].values[3] += 1e-4
    with pytest.raises(ValueError, match="uniform"):
        remove_water(uneven)
    with pytest.raises(ValueError, match="complex"):
        remove_water(_la(dtype=float))
    with pytest.raises(TypeError):
        remove_water(np.zeros((2, 200), complex))


def test_c_abi_refusals_without_gpu():
    from xmris_amd import _lib

    lib = _lib.load()
    ok = dict(x=1, rs=128, y=1, f=1, d=1, a=1, p=1, r=1, nr=1, s=1, nb=2, N=128, M=64, K=20, dt=2e-4, lo=-50.0, hi=50.0,
              dtype=0, ws=1)
    for change in (dict(x=None), dict(f=None), dict(d=None), dict(a=None), dict(p=None), dict(r=None), dict(nr=None),
                   dict(s=None), dict(ws=None), dict(M=1), dict(M=65), dict(K=0), dict(K=33), dict(M=16, K=16),
                   dict(N=127), dict(N=16385, rs=16385), dict(rs=127), dict(dt=0.0), dict(dt=-1.0), dict(dt=float("nan")),
                   dict(lo=1.0, hi=0.0), dict(hi=float("inf")), dict(lo=float("nan")), dict(dtype=2), dict(dtype=0x1000),
                   dict(dtype=0xa00), dict(nb=-1)):
        a = dict(ok, **change)
        rc = lib.xm_hsvd_rows(a["x"], a["rs"], a["y"], a["f"], a["d"], a["a"], a["p"], a["r"], a["nr"], a["s"], a["nb"],
                              a["N"], a["M"], a["K"], a["dt"], a["lo"], a["hi"], a["dtype"], a["ws"], None)
        assert rc == _lib.XM_ERR_INVALID_ARG, change
        assert b"hsvd_rows" in lib.xm_last_error_string()
    # no rows: nothing to do, whatever the pointers hold
    assert lib.xm_hsvd_rows(1, 128, None, 1, 1, 1, 1, 1, 1, 1, 0, 128, 64, 20, 2e-4, -50.0, 50.0, 0, 1, None) == 0


def test_vocabulary_and_exports():
    import xmris_amd
    from xmris_amd import ATTRS, processing
    from xmris_amd import device as dev

    assert (ATTRS.water_band, ATTRS.water_rank, ATTRS.water_n_cols) == ("water_band", "water_rank", "water_n_cols")
    assert xmris_amd.remove_water is processing.remove_water and "remove_water" in xmris_amd.__all__
    assert "remove_water" in processing.__all__ and hasattr(xmris_amd.XmrisAccessor, "remove_water")
    assert (dev.HSVD_MAX_COLS, dev.HSVD_MAX_RANK, dev.HSVD_MAX_POINTS) == (64, 32, 16384)
