"""CPU tests of align_averages: the oracle's two routes agree within the bound ALIGN_TOL is made from, every GPU parity
case is well conditioned (margin, one sign change of P', status 0), the oracle has the properties of the definition
(DESIGN.md section 11), and every validation error fires before the library is reached.

The tests of the oracle alone import nothing from the package and pass without the feature; the validation, ABI and
vocabulary tests fail without it."""
import functools

import numpy as np
import pytest

import _align_oracle as orc

EPS = orc.EPS
# 16 x 2.51, the largest disagreement of the oracle's two routes (safeguarded Newton in fp64 against brentq on P' in
# long double) over orc.PARITY_CASES: f* 2.51 units of u_f, phi* 1.91 units of u_phi -- tests/tool_align_tolerance.py
ROUTE_UNITS = 2.51
ALIGN_TOL = 40.0
MIN_MARGIN = 0.2


@functools.lru_cache(maxsize=None)
def routes(name):
    x, r, dt, ms, L = orc.parity_case(name)
    return tuple(orc.align_batch(x, r, dt, 0.0, ms, L, route=rt) for rt in ("newton", "brentq"))


@pytest.mark.parametrize("name", list(orc.PARITY_CASES))
def test_routes_agree_and_cases_are_well_conditioned(name):
    a, b = routes(name)
    uf, up = orc.route_gap_units(a, b)
    print(name, uf, up, a["margin"].min())
    assert uf <= ALIGN_TOL / 16 * 1.005 and up <= ALIGN_TOL / 16 * 1.005, (uf, up)
    assert np.all(a["margin"] >= MIN_MARGIN), a["margin"].min()
    assert np.all(a["one_sign_change"]) and np.all(a["status"] == 0)


def test_tolerance_constant_matches_its_tool():
    """ALIGN_TOL is 16 x the worst figure of the routes over all parity cases, measured here again (cached), and the
    figure is the one profiles/align/tolerance.txt records from tests/tool_align_tolerance.py."""
    worst = max(max(orc.route_gap_units(*routes(name))) for name in orc.PARITY_CASES)
    assert worst == pytest.approx(ROUTE_UNITS, abs=0.005), worst
    assert ALIGN_TOL == pytest.approx(16 * worst, abs=0.5)
    import os
    import re

    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "align", "tolerance.txt")).read()
    assert float(re.search(r"ALIGN_TOL = (\d+)", text).group(1)) == ALIGN_TOL


def test_known_shift_and_phase_come_back_negated():
    n, dt, f0, p0 = 200, 5e-4, 3.7, 0.9
    _, r, _, _ = orc.make_data(1, 1, 1, n, seed=5, dt=dt, clean=True)
    r = r[0, 0]
    t = 0.002 + np.arange(n) * dt
    x = r * np.exp(1j * (2 * np.pi * f0 * t + p0))
    o = orc.align(x, r, dt, t0=0.002, max_shift=10.0)
    assert o["status"] == 0 and abs(o["quality"] - 1.0) <= 64 * EPS
    assert abs(o["shift"] + f0) <= ALIGN_TOL * o["u_f"] and orc.phase_gap(o["phase"], -p0) <= ALIGN_TOL * o["u_phi"]
    bound = np.abs(x) * (2 * np.pi * np.abs(t) * ALIGN_TOL * o["u_f"] + ALIGN_TOL * o["u_phi"] + 4 * EPS)
    assert np.all(np.abs(o["y"] - r) <= bound)


def test_status_cases():
    n, dt = 64, 5e-4
    x, r, _, _ = orc.make_data(1, 1, 1, n, seed=6, dt=dt, clean=True, max_shift=0.0)
    x, r = x[0, 0, 0], r[0, 0]
    t = np.arange(n) * dt
    delta, _ = orc.grid(n, dt, 1.0)
    far = orc.align(x * np.exp(2j * np.pi * 6 * delta * t), r, dt, max_shift=3.3 * delta)  # the maximum lies at -6 delta
    assert far["status"] == 1 and far["shift"] == -3.3 * delta and 0 < far["quality"] < 1
    bad = x.copy()
    bad[5] = np.nan
    for o in (orc.align(bad, r, dt), orc.align(x, bad, dt), orc.align(x * 1e200, r * 1e200, dt)):
        assert o["status"] == 2 and not o["y"].any() and np.isnan([o["shift"], o["phase"], o["quality"]]).all()
    late = x.copy()
    late[40] = np.inf  # beyond the L points: not looked at
    assert orc.align(late, r, dt, L=32)["status"] == 0
    z = orc.align(x, np.zeros(n), dt)
    assert z["status"] == 3 and np.array_equal(z["y"], x) and z["shift"] == z["phase"] == z["quality"] == 0.0


def test_grid_tie_goes_to_the_smaller_and_then_the_negative_index():
    # z = delta at t = 0: P is the same at every grid point
    x = np.zeros(8, complex)
    x[0] = 1.0
    o = orc.align(x, x, 1e-3, max_shift=100.0)
    assert o["g"] == 0 and o["status"] == 0
    # a pure tone half way between -1 and +1 mirrored: P(-g) = P(+g) exactly for a real z
    xr = np.cos(2 * np.pi * 3 * np.arange(16) / 16.0) + 0j
    o = orc.align(np.ones(16, complex), xr, 1.0 / 64, max_shift=20.0)
    assert o["g"] < 0


def test_alignment_raises_the_summed_peak():
    x, r, _, _ = orc.make_data(1, 16, 1, 512, seed=7, max_shift=12.0)
    res = orc.align_batch(x, r, orc.DT, 0.0, 12.0)
    peak = lambda a: np.abs(np.fft.fft(a.sum(axis=1)[0, 0])).max()  # noqa: E731
    assert peak(res["y"]) > 1.5 * peak(x)


# ---- validation: every error fires before any native call -----------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    from xmris_amd import _lib
    from xmris_amd import device as dev

    def boom(*a, **k):
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "call", boom)
    monkeypatch.setattr(dev, "to_device", boom)
    monkeypatch.setattr(dev, "align_rows", boom)


def _la(shape=(3, 4, 16), dims=("x", "average", "time"), time=True, dtype=complex, dt=1e-3):
    from xmris_amd import LabeledArray

    rng = np.random.default_rng(1)
    v = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    v = v.real.copy() if dtype is float else v.astype(dtype)
    coords = {"time": np.arange(shape[dims.index("time")]) * dt} if time and "time" in dims else {}
    return LabeledArray(v, dims, coords)


@pytest.mark.parametrize("kw, word", [
    (dict(dim="repetition"), "repetition"),
    (dict(time_dim="t"), "'t'"),
    (dict(reference="median"), "reference"),
    (dict(reference=7), "reference"),
    (dict(passes=2, reference="first"), "passes"),
    (dict(passes=0), "passes"),
    (dict(n_points=0), "n_points"),
    (dict(n_points=17), "n_points"),
    (dict(t_max=-1.0), "t_max"),
    (dict(max_shift=-1.0), "max_shift"),
    (dict(max_shift=1e5), "max_shift.*t_max"),
])
def test_validation_errors_name_their_argument(no_library, kw, word):
    from xmris_amd import align_averages

    with pytest.raises(ValueError, match=word):
        align_averages(_la(), **kw)
    with pytest.raises(ValueError, match=word):
        _la().xmr.align_averages(**kw)


def test_validation_of_input_time_coordinate_reference_and_caps(no_library):
    from xmris_amd import align_averages

    with pytest.raises(ValueError, match="time_dim"):
        align_averages(_la(time=False))
    uneven = _la()
    uneven.coords["time"].values[3] += 4e-4
    with pytest.raises(ValueError, match="uniform"):
        align_averages(uneven)
    with pytest.raises(ValueError, match="complex"):
        align_averages(_la(dtype=float))
    for bad in (_la((3, 4, 16)), _la((2, 16), ("x", "time")), _la((3, 4), ("x", "y"), time=False)):
        with pytest.raises(ValueError, match="reference"):
            align_averages(_la(), reference=bad)
    with pytest.raises(ValueError, match="n_points"):  # the range follows the reference's length
        align_averages(_la(), reference=_la((8,), ("time",)), n_points=9)
    with pytest.raises(ValueError, match="t_max"):
        align_averages(_la((1, 2, 9000), dt=1e-5), max_shift=1.0)


def test_c_abi_refusals_without_gpu():
    from xmris_amd import _lib

    lib = _lib.load()
    ok = dict(x=1, r=1, rs=8, y=1, mean=None, sh=1, ph=1, q=1, s=1, na=None, no=1, A=2, ni=1, N=8, NR=8, L=8, dt=1e-3,
              t0=0.0, ms=20.0, mq=0.0, dtype=0, ws=1)
    for change in (dict(x=None), dict(r=None), dict(y=None), dict(sh=None), dict(ph=None), dict(q=None), dict(s=None),
                   dict(ws=None), dict(mean=1), dict(L=0), dict(L=9), dict(NR=7), dict(N=9000, NR=9000, L=8193),
                   dict(ms=1e6), dict(ms=1e6, L=2), dict(dt=0.0), dict(dt=-1e-3), dict(ms=-1.0), dict(dtype=2), dict(dtype=0x800),
                   dict(rs=3), dict(A=0), dict(no=-1)):
        a = dict(ok, **change)
        rc = lib.xm_align_rows(a["x"], a["r"], a["rs"], a["y"], a["mean"], a["sh"], a["ph"], a["q"], a["s"], a["na"], a["no"],
                               a["A"], a["ni"], a["N"], a["NR"], a["L"], a["dt"], a["t0"], a["ms"], a["mq"], a["dtype"],
                               a["ws"], None)
        assert rc == _lib.XM_ERR_INVALID_ARG, change
        assert b"align_rows" in lib.xm_last_error_string()
    assert lib.xm_align_workspace_bytes(4, 5, 3, 2048) == _lib.XM_ALIGN_WORKSPACE_BYTES


def test_vocabulary_and_exports():
    import xmris_amd
    from xmris_amd import ATTRS, processing

    assert (ATTRS.align_dim, ATTRS.align_reference, ATTRS.align_max_shift) == ("align_dim", "align_reference", "align_max_shift")
    assert xmris_amd.align_averages is processing.align_averages
    assert hasattr(xmris_amd.XmrisAccessor, "align_averages")
    from xmris_amd import device as dev

    assert dev.align_grid(1024, 2e-4, 20.0) == orc.grid(1024, 2e-4, 20.0)
    assert dev.align_grid(1, 2e-4, 1e9) == orc.grid(1, 2e-4, 1e9) and dev.align_grid(1, 2e-4, 1e9)[1] == 0
