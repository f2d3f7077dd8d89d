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
