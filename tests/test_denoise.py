"""CPU tests of denoise_mppca: the oracle's two routes agree within the figures DENOISE_TOL is made from, every GPU
parity case meets the conditions that make the comparison meaningful (the same rank on both routes, every comparison of
the rank scan decided by a margin, status 0), the oracle has the properties of the definition, and
every validation error fires before the library is reached.

The tests of the oracle alone import nothing from the package and pass without the feature; the validation, ABI and
vocabulary tests fail without it."""
import os
import re

import numpy as np
import pytest

import _denoise_oracle as orc

# the largest disagreement of the oracle's two routes (eigh of G against the SVD of X) over orc.PARITY_CASES --
# tests/tool_denoise_tolerance.py, recorded in profiles/denoise/tolerance.txt -- and 16 x that: y in units of
# eps max(1, lam_0 / (lam_{r-1} - lam_r)) max |x| (orc.units), sigma relative to itself
ROUTE_GAP = {"y": 4.15, "sigma": 9.67e-15}
DENOISE_TOL = {"y": 66.4, "sigma": 1.5e-13}


def y_bound(res, x, dtype=np.complex128):
    """Per voxel, the bound on |y - oracle's y|: DENOISE_TOL in the oracle's units; complex64 adds the one rounding of y
    to fp32 (half an ulp of each part: at most eps32 / 2 of |y|)."""
    b = DENOISE_TOL["y"] * orc.units(res, x)
    if np.dtype(dtype) == np.complex64:
        b = b + 0.5 * np.finfo(np.float32).eps * np.abs(res["y"]).max(axis=-1)
    return b


@pytest.mark.parametrize("name", list(orc.PARITY_CASES))
def test_routes_agree_and_cases_meet_the_conditions(name):
    clean, x, a, b, seed = orc.parity_case(name)
    gy, gs = orc.route_gap(a, b, x)
    print(name, "seed", seed, "y", gy, "sigma", gs, "margin", a["margin"].min(), b["margin"].min())
    assert gy <= DENOISE_TOL["y"] / 16 * 1.01 and gs <= DENOISE_TOL["sigma"] / 16 * 1.05
    assert orc.conditions(a, b)
    assert np.array_equal(a["rank"], b["rank"])
    for r in (a, b):
        assert np.all(r["status"] == 0) and r["margin"].min() >= orc.MIN_MARGIN
    # the seed is the first that meets the conditions
    grid, patch, n, k, n_outer = orc.PARITY_CASES[name]
    for s in range(seed):
        _, xs = orc.make_data(grid, n, k, s, n_outer)
        assert not orc.conditions(*(orc.denoise(xs, patch, route=rt) for rt in ("eigh", "svd")))


def test_every_patch_size_of_the_sweep_meets_the_conditions():
    """The inputs of tests/test_gpu_denoise.py's sweep over P = 2 ... 64: a seed below 64 meets the conditions at every P
    (orc.sweep_case raises otherwise: none is skipped), and the oracle's two routes agree within DENOISE_TOL."""
    assert list(orc.SWEEP_CASES) == list(range(2, 65)) and not set(orc.SWEEP_CASES) & set(orc.PARITY_CASES)
    worst = [0.0, 0.0]
    for p, (grid, patch, n, k, n_outer) in orc.SWEEP_CASES.items():
        assert (grid, patch, n, k, n_outer) == ((p + 1,), (p,), 96, 2, None)
        _, x, a, b, seed = orc.sweep_case(p)
        assert orc.conditions(a, b) and 0 <= seed < 64, p
        gy, gs = orc.route_gap(a, b, x)
        worst = [max(worst[0], gy), max(worst[1], gs)]
        assert gy <= DENOISE_TOL["y"] and gs <= DENOISE_TOL["sigma"], (p, gy, gs)
    print("sweep: routes differ by y", worst[0], "units, sigma", worst[1], "; bounds", DENOISE_TOL)


def test_parity_cases_cover_the_kernel_paths():
    ps = {int(np.prod(c[1])) for c in orc.PARITY_CASES.values()}
    ns = {c[2] for c in orc.PARITY_CASES.values()}
    assert {2, 6, 7, 8, 9, 25, 27, 49, 64} <= ps and {orc.Q - 1, orc.Q, orc.Q + 1, 2048} <= ns
    assert any(c[4] == 3 for c in orc.PARITY_CASES.values())
    assert {len(c[0]) for c in orc.PARITY_CASES.values()} == {1, 2, 3}


def test_tolerance_constants_match_their_tool():
    gaps = [orc.route_gap(a, b, x) for _, x, a, b, _ in map(orc.parity_case, orc.PARITY_CASES)]
    worst = {"y": max(g[0] for g in gaps), "sigma": max(g[1] for g in gaps)}
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "denoise", "tolerance.txt")).read()
    recorded = dict(re.findall(r'"(y|sigma)": ([0-9.e+-]+)', text.split("DENOISE_TOL =")[1]))
    for k in DENOISE_TOL:
        assert worst[k] == pytest.approx(ROUTE_GAP[k], rel=0.02), (k, worst[k])
        assert DENOISE_TOL[k] == pytest.approx(16 * worst[k], rel=0.04)
        assert float(recorded[k]) == DENOISE_TOL[k]


@pytest.mark.parametrize("route", ["eigh", "svd"])
def test_hand_checkable_ranks(route):
    _, x, _, _, _ = orc.parity_case("g6x7_p3x3_n64")
    zero = orc.denoise(x, (3, 3), rank=0, route=route)
    assert not zero["y"].any() and np.all(zero["rank"] == 0) and np.all(zero["status"] == 0)
    lam = zero["lam"]
    assert np.allclose(zero["sigma"], np.sqrt(lam.mean(axis=-1)), rtol=1e-13)  # the mean of all lam
    full = orc.denoise(x, (3, 3), rank=9, route=route)
    assert np.abs(full["y"] - x).max() <= 64 * orc.EPS * np.abs(x).max()
    assert np.all(full["rank"] == 9) and not full["sigma"].any()
    # a noise-free grid of K components has rank K: keeping K gives the input back
    k = 3
    clean, _ = orc.make_data((6, 7), 64, k, seed=5, noise=0.0)
    keep = orc.denoise(clean, (3, 3), rank=k, route=route)
    assert np.all(np.abs(keep["y"] - clean).max(axis=-1) <= 64 * orc.units(keep, clean))  # (the unit holds lam_0 / lam_{K-1})
    assert np.abs(orc.denoise(clean, (3, 3), rank=k - 1, route=route)["y"] - clean).max() > 1e-6


def test_marchenko_pastur_rule_on_a_hand_made_spectrum():
    # M = 4, N = 16: gamma_p = (4 - p) / 16, 4 sqrt(gamma_p) = 2, sqrt(3), sqrt(2), 1
    lam = np.array([10.0, 4.0, 1.0, 1.0])
    # p = 0: s1 = 16 / 4 = 4, s2 = 9 / 2 = 4.5 (not below); p = 1: s1 = 6 / 3 = 2, s2 = 3 / sqrt(3) = 1.73 < 2 -> r = 1
    r, sigma, margin = orc.mp_rank(lam, 16)
    assert r == 1 and sigma == pytest.approx(np.sqrt(2.0)) and margin == pytest.approx(0.5 / 4.5)
    # a flat spectrum is all noise: r = 0, sigma^2 its level
    r, sigma, _ = orc.mp_rank(np.full(5, 0.25), 100)
    assert r == 0 and sigma == pytest.approx(0.5)
    # p = 0: s1 = 103 / 4, s2 = 99 / 2; p = 1: s1 = 1, s2 = 0 -> r = 1
    assert orc.mp_rank(np.array([100.0, 1.0, 1.0, 1.0]), 16)[0] == 1
    # a zero tail: no p qualifies (0 < 0 never holds), everything is kept and no noise is reported
    assert orc.mp_rank(np.array([3.0, 0.0, 0.0]), 16)[:2] == (3, 0.0)
    # a given rank: sigma from the tail's mean, 0 for the full rank
    assert orc.mp_rank(lam, 16, rank=2)[:2] == (2, 1.0) and orc.mp_rank(lam, 16, rank=4)[:2] == (4, 0.0)


def test_edge_windows_are_full_and_shifted_inward():
    for p, s in ((5, 8), (3, 7), (4, 6), (2, 3), (8, 8), (1, 3)):
        starts = [orc.window_start(i, p, s) for i in range(s)]
        assert all(0 <= o and o + p <= s and o <= i < o + p for i, o in enumerate(starts))
        assert starts[0] == starts[p // 2] == 0 and starts[-1] == s - p
        assert all(o == i - p // 2 for i, o in enumerate(starts) if p // 2 <= i <= s - p + p // 2)
    win = {idx: (rows, c) for idx, rows, c in orc.windows((8, 8), (5, 5))}
    assert win[(0, 0)][0] == win[(2, 2)][0] and win[(0, 0)][1] == 0 and win[(2, 2)][1] == 12
    assert win[(7, 7)][0] == win[(5, 5)][0] and win[(7, 7)][1] == 24
    assert win[(3, 4)][0][0] == (1, 2) and win[(3, 4)][0][1] == (1, 3) and len(win[(3, 4)][0]) == 25


def test_denoising_improves_and_sigma_is_the_noise_level():
    clean, x, a, _, _ = orc.parity_case("g8x8_p5x5_n256")
    rms = lambda z: float(np.sqrt(np.mean(np.abs(z) ** 2)))  # noqa: E731
    print("rms", rms(x - clean), "->", rms(a["y"] - clean), "mean sigma", a["sigma"].mean())
    assert rms(a["y"] - clean) <= 0.5 * rms(x - clean)
    assert abs(a["sigma"].mean() - orc.NOISE_SD) <= 0.05 * orc.NOISE_SD


def test_a_voxel_depends_on_its_window_only():
    _, x, a, _, _ = orc.parity_case("g6x7_p3x3_n64")
    x2 = x.copy()
    x2[5, 6] += 1.0  # seen by the windows of rows 4, 5 and columns 5, 6 (they start at row 3, column 4)
    b = orc.denoise(x2, (3, 3))
    same = np.ones((6, 7), bool)
    same[4:, 5:] = False
    assert np.array_equal(a["y"][same], b["y"][same]) and np.array_equal(a["sigma"][same], b["sigma"][same])
    assert np.all(np.abs(a["y"][~same] - b["y"][~same]).max(axis=-1) > 0)


def test_status_cases(monkeypatch):
    _, x, _, _, _ = orc.parity_case("g6x7_p3x3_n64")
    x = x.copy()
    x[:3, :3] = 0.0  # the window of voxels (0, 0), (0, 1), (1, 0), (1, 1) is all zero; others only hold some zeros
    o = orc.denoise(x, (3, 3))
    expect = np.zeros((6, 7), int)
    expect[:2, :2] = 1
    assert np.array_equal(o["status"], expect)
    assert not o["y"][:2, :2].any() and not o["sigma"][:2, :2].any() and not o["rank"][:2, :2].any()
    for bad_value in (np.nan, np.inf):
        bad = x.copy()
        bad[5, 6, 7] = bad_value
        o = orc.denoise(bad, (3, 3))
        expect2 = expect.copy()
        expect2[4:, 5:] = 2
        assert np.array_equal(o["status"], expect2)
        assert not o["y"][4:, 5:].any() and np.isnan(o["sigma"][4:, 5:]).all() and not o["rank"][4:, 5:].any()
    for route in ("eigh", "svd"):
        assert np.all(orc.denoise(x * 1e200, (3, 3), route=route)["status"][2:, 2:] == 2)  # G overflows

    def no_convergence(*a, **k):
        raise np.linalg.LinAlgError("Eigenvalues did not converge")

    monkeypatch.setattr(np.linalg, "eigh", no_convergence)
    o = orc.denoise(x, (3, 3))
    cap = expect == 0
    assert np.all(o["status"][cap] == 3) and np.array_equal(o["y"][cap], x[cap]) and np.isnan(o["sigma"][cap]).all()
    assert not o["rank"].any() and np.array_equal(o["status"][~cap], expect[~cap])


# ---- validation: every error fires before any native call -----------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    from xmris_amd import _lib
    from xmris_amd import device as dev

    def boom(*a, **k):
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "call", boom)
    monkeypatch.setattr(dev, "to_device", boom)
    monkeypatch.setattr(dev, "denoise_patches", boom)


def _la(shape=(6, 7, 40), dims=("x", "y", "time"), dtype=complex):
    from xmris_amd import LabeledArray

    rng = np.random.default_rng(1)
    v = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    v = v.real.copy() if dtype is float else v.astype(dtype)
    return LabeledArray(v, dims, {"time": np.arange(shape[dims.index("time")]) * 1e-3})


@pytest.mark.parametrize("kw, word", [
    (dict(dims=("x", "q"), patch=3), "dims"),  # unknown
    (dict(dims=("x", "time"), patch=3), "dims"),  # the time dim
    (dict(dims=("x", "x"), patch=2), "dims"),  # repeated
    (dict(dims=(), patch=3), "dims"),
    (dict(dims=("x", "y"), patch=3, time_dim="t"), "time_dim"),
    (dict(dims=("x", "y"), patch=(3, 8)), "patch"),  # larger than its dim
    (dict(dims=("x", "y"), patch=(0, 3)), "patch"),
    (dict(dims=("x", "y"), patch=(3, 3, 3)), "patch"),  # one size too many
    (dict(dims=("x", "y"), patch=2.5), "patch"),
    (dict(dims=("x", "y"), patch="wide"), "patch"),
    (dict(dims=("x", "y"), patch=1), "patch"),  # P = 1
    (dict(dims=("x", "y"), patch=(6, 7)), "time_dim"),  # P = 42 > N = 40
    (dict(dims=("x", "y"), patch=3, rank=-1), "rank"),
    (dict(dims=("x", "y"), patch=3, rank=10), "rank"),
    (dict(dims=("x", "y"), patch=3, rank=2.5), "rank"),
])
def test_validation_errors_name_their_argument(no_library, kw, word):
    from xmris_amd import denoise_mppca

    with pytest.raises(ValueError, match=word):
        denoise_mppca(_la(), **kw)
    with pytest.raises(ValueError, match=word):
        _la().xmr.denoise_mppca(**kw)


def test_validation_of_sizes_and_dtype(no_library):
    from xmris_amd import denoise_mppca

    with pytest.raises(ValueError, match="dims"):  # more than three
        denoise_mppca(_la((2, 2, 2, 2, 40), ("a", "b", "c", "d", "time")), ("a", "b", "c", "d"), 2)
    with pytest.raises(ValueError, match="patch.*64"):  # P = 81
        denoise_mppca(_la((9, 9, 100)), ("x", "y"), 9)
    with pytest.raises(ValueError, match="16384"):
        denoise_mppca(_la((2, 2, 16385)), ("x", "y"), 2)
    with pytest.raises(ValueError, match="complex"):
        denoise_mppca(_la(dtype=float), ("x", "y"), 3)
    with pytest.raises(TypeError):
        denoise_mppca(np.zeros((6, 7, 40), complex), ("x", "y"), 3)


def test_c_abi_refusals_without_gpu():
    from xmris_amd import _lib

    lib = _lib.load()
    ok = dict(x=1, y=2, r=1, sg=1, st=1, no=2, s1=1, s2=6, s3=7, p1=1, p2=3, p3=3, N=40, rank=-1, dtype=0, ws=1)
    for change in (dict(x=None), dict(y=None), dict(r=None), dict(sg=None), dict(st=None), dict(ws=None), dict(y=1),
                   dict(s1=0), dict(p1=0), dict(p2=7), dict(p3=8), dict(p1=2), dict(p2=1, p3=1), dict(s2=9, s3=9, p2=9, p3=9, N=100),
                   dict(p2=6, p3=7), dict(N=8), dict(N=16385), dict(rank=-2), dict(rank=10), dict(dtype=2),
                   dict(dtype=0x800), dict(dtype=0x600), dict(no=-1), dict(no=1 << 40, s2=1 << 20, p2=3)):
        a = dict(ok, **change)
        rc = lib.xm_denoise_patches(a["x"], a["y"], a["r"], a["sg"], a["st"], a["no"], a["s1"], a["s2"], a["s3"], a["p1"],
                                    a["p2"], a["p3"], a["N"], a["rank"], a["dtype"], a["ws"], None)
        assert rc == _lib.XM_ERR_INVALID_ARG, change
        assert b"denoise_patches" in lib.xm_last_error_string()
    # no voxels: nothing to do, whatever the pointers hold
    assert lib.xm_denoise_patches(1, 2, 1, 1, 1, 0, 1, 6, 7, 1, 3, 3, 40, -1, 0, 1, None) == 0


def test_vocabulary_and_exports():
    import xmris_amd
    from xmris_amd import ATTRS, processing
    from xmris_amd import device as dev

    assert (ATTRS.denoise_dims, ATTRS.denoise_patch, ATTRS.denoise_rank) == ("denoise_dims", "denoise_patch", "denoise_rank")
    assert xmris_amd.denoise_mppca is processing.denoise_mppca and "denoise_mppca" in xmris_amd.__all__
    assert "denoise_mppca" in processing.__all__ and hasattr(xmris_amd.XmrisAccessor, "denoise_mppca")
    assert (dev.DENOISE_MAX_PATCH, dev.DENOISE_MAX_POINTS) == (64, 16384)
    assert xmris_amd._lib.XM_DENOISE_WORKSPACE_BYTES == 256
