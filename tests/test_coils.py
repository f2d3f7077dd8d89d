"""CPU tests of combine_coils: the oracle's two routes agree within the bound COIL_TOL is made from, the oracle has the
properties of the definition, every GPU case has a wide spectral gap, and every validation error
fires before the library is reached.

The tests of the oracle alone (routes, properties, degenerate voxels) import nothing from the package and therefore
pass without the feature; the validation, ABI and vocabulary tests fail without it."""
import functools

import numpy as np
import pytest

import _coils_oracle as orc

EPS = orc.EPS
# 16 x 5.48, the largest disagreement in y of the oracle's two routes (eigh of G against svd of the whitened
# reference) over orc.PARITY_CASES in units of eps lam1 / (lam1 - lam2) relative to max |y|: tests/tool_coil_tolerance.py
ROUTE_UNITS = 5.48
W_ROUTE_UNITS = 16.14  # the same for w (relative to max |w|); the GPU tests hold w to COIL_TOL like y
COIL_TOL = 88.0
MIN_GAP = 0.5


@functools.lru_cache(maxsize=None)
def routes(name):
    x = orc.parity_case(name)
    return tuple(orc.combine_batch(x, coil_axis=1, route=r) for r in ("eigh", "svd"))


@pytest.mark.parametrize("name", list(orc.PARITY_CASES))
def test_routes_agree_and_gap_is_wide(name):
    a, b = routes(name)
    uy, uw, uq = orc.route_gap_units(a, b)
    print(name, uy, uw, uq)
    assert uy <= ROUTE_UNITS * 1.005 and uq <= ROUTE_UNITS * 1.005, (uy, uq)
    assert uw <= W_ROUTE_UNITS * 1.005, uw
    gap = (a["lam1"] - a["lam2"]) / a["lam1"]
    assert np.all(gap >= MIN_GAP), gap.min()
    assert np.all(a["status"] == 0)


def test_every_coil_count_of_the_sweep_has_a_wide_gap():
    """The inputs of tests/test_gpu_coils.py's sweep over C = 1 ... 64: the gap that makes the comparison meaningful, and
    the oracle's two routes within the bound the kernel is held to."""
    worst, smallest = (0.0, 0.0, 0.0), 1.0
    for c in orc.SWEEP_COILS:
        x = orc.sweep_case(c)
        assert x.shape == (3, c, 1, orc.Q + 1)
        a, b = (orc.combine_batch(x, coil_axis=1, route=r) for r in ("eigh", "svd"))
        gap = (a["lam1"] - a["lam2"]) / a["lam1"]
        assert np.all(gap >= MIN_GAP) and np.all(a["status"] == 0), (c, gap.min())
        smallest = min(smallest, float(gap.min()))
        worst = tuple(max(w, u) for w, u in zip(worst, orc.route_gap_units(a, b)))
    print("smallest gap", smallest, "routes differ by (y, w, quality)", worst, "units; bound", COIL_TOL)
    assert max(worst) <= COIL_TOL


def test_tolerance_constant_matches_its_tool():
    assert COIL_TOL == pytest.approx(16 * ROUTE_UNITS, abs=0.5)


@pytest.mark.parametrize("method", ["svd", "first_point"])
def test_oracle_properties(method):
    x = orc.make_data(6, 5, 1, 40, seed=3)[:, :, 0, :]
    psi = orc.random_psd(5, 4)
    chol = np.linalg.cholesky(psi)
    for v in range(x.shape[0]):
        o = orc.combine(x[v], psi=psi, method=method, n_points=3)
        assert abs(np.linalg.norm(chol.conj().T @ o["w"]) - 1.0) < 64 * EPS
        y0 = np.vdot(o["w"], x[v][:, 0])
        assert abs(y0.imag) <= 64 * EPS * abs(y0) and y0.real > 0
        assert 0.0 < o["quality"] <= 1.0 + 64 * EPS


def test_oracle_rank_one_and_single_coil():
    rng = np.random.default_rng(0)
    s = rng.standard_normal(4) + 1j * rng.standard_normal(4)
    f = np.exp((-1 + 9j) * np.arange(20) / 20)
    for route in ("eigh", "svd"):
        assert abs(orc.combine(np.outer(s, f), route=route)["quality"] - 1.0) < 64 * EPS
    x = rng.standard_normal((1, 20)) + 1j * rng.standard_normal((1, 20))
    o = orc.combine(x)
    want = x[0] * np.conj(x[0, 0]) / abs(x[0, 0])
    assert np.abs(o["y"] - want).max() <= 8 * EPS * np.abs(want).max() and abs(o["quality"] - 1.0) < 8 * EPS


def test_oracle_degenerate_voxels():
    z = orc.combine(np.zeros((3, 8)))
    assert z["status"] == 1 and z["quality"] == 0.0 and not z["y"].any() and not z["w"].any()
    x = np.ones((3, 8), complex)
    x[1, 4] = np.nan
    n = orc.combine(x)
    assert n["status"] == 2 and np.isnan(n["quality"]) and not n["y"].any() and not n["w"].any()


# ---- validation: every error fires before any native call -----------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    from xmris_amd import _lib
    from xmris_amd import device as dev

    def boom(*a, **k):
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "call", boom)
    monkeypatch.setattr(dev, "to_device", boom)
    monkeypatch.setattr(dev, "coil_combine", boom)


def _la(shape=(3, 4, 16), dims=("x", "coil", "time")):
    from xmris_amd import LabeledArray

    rng = np.random.default_rng(1)
    return LabeledArray(rng.standard_normal(shape) + 1j * rng.standard_normal(shape), dims)


@pytest.mark.parametrize("kw, word", [
    (dict(dim="channel"), "dim"),
    (dict(time_dim="t"), "time_dim"),
    (dict(method="sos"), "method"),
    (dict(n_points=0), "n_points"),
    (dict(n_points=17), "n_points"),
    (dict(noise_cov=np.eye(3)), "noise_cov"),
    (dict(noise_cov=-np.eye(4)), "noise_cov"),
    (dict(noise_cov=np.array([[1, 2, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1.0]])), "noise_cov"),
    (dict(noise_cov="head"), "noise_cov"),
])
def test_validation_errors_name_their_argument(no_library, kw, word):
    from xmris_amd import combine_coils

    with pytest.raises(ValueError, match=word):
        combine_coils(_la(), **kw)
    with pytest.raises(ValueError, match=word):
        _la().xmr.combine_coils(**kw)


def test_validation_of_coil_count_and_reference(no_library):
    from xmris_amd import combine_coils

    with pytest.raises(ValueError, match="dim"):
        combine_coils(_la((2, 65, 4)))
    for bad in (_la((3, 5, 16)), _la((2, 4, 16)), _la((4, 3, 16), ("coil", "x", "time"))):
        with pytest.raises(ValueError, match="reference"):
            combine_coils(_la(), reference=bad)
    with pytest.raises(ValueError, match="n_points"):  # the range follows the reference's length
        combine_coils(_la(), reference=_la((3, 4, 2)), n_points=3)


def test_c_abi_refusals_without_gpu():
    from xmris_amd import _lib

    lib = _lib.load()
    ok = dict(x=1, ref=None, y=1, w=1, q=1, s=1, no=1, C=4, ni=1, N=8, NR=8, linv=None, method=0, npts=1, c128=0, ws=1)
    for change in (dict(C=0), dict(C=65), dict(N=0), dict(NR=0), dict(NR=9), dict(npts=0), dict(npts=9), dict(method=3),
                   dict(method=-1), dict(x=None), dict(y=None), dict(w=None), dict(q=None), dict(s=None), dict(ws=None),
                   dict(no=-1)):
        a = dict(ok, **change)
        rc = lib.xm_coil_combine(a["x"], a["ref"], a["y"], a["w"], a["q"], a["s"], a["no"], a["C"], a["ni"], a["N"], a["NR"],
                                 a["linv"], a["method"], a["npts"], a["c128"], a["ws"], None)
        assert rc == _lib.XM_ERR_INVALID_ARG, change
        assert b"coil_combine" in lib.xm_last_error_string()


def test_vocabulary_and_exports():
    import xmris_amd
    from xmris_amd import ATTRS, processing

    assert ATTRS.coil_combine_method == "coil_combine_method" and ATTRS.coil_combine_dim == "coil_combine_dim"
    assert xmris_amd.combine_coils is processing.combine_coils
    assert hasattr(xmris_amd.XmrisAccessor, "combine_coils")
    assert processing.coils.tail_points(2048) == 409 and processing.coils.tail_points(30) == 10
