"""CPU tests of grappa_calibrate / grappa_fill: the oracle's own sums and routes agree within the figures GRAPPA_TOL and
GRAPPA_CAL_TOL are made from, the chosen cases meet the conditions of DESIGN.md section 20, ``grappa_calibrate`` agrees
with both routes of the oracle, the Python layer (on a numpy stand-in for ``device.grappa_fill`` built from the oracle)
reconstructs the missing lines, keeps the acquired ones bit for bit and keeps dims, coordinates, attrs and names as
specified, every validation error fires before the library is reached, and xm_grappa_fill refuses bad arguments
without a GPU.

The tests of the oracle alone import nothing from the package and pass without the feature; all others fail without it."""
import ctypes
import os
import re

import numpy as np
import pytest

import _grappa_oracle as orc

# tests/tool_grappa_tolerance.py, recorded in profiles/grappa/tolerance.txt: the largest gap between the ascending-order
# float64 sum and the long-double sum over orc.APPLY_CASES in units of eps sum |W| |a|, and 16 x that; the largest gap of
# the two calibration routes over orc.E2E_CASES in units of eps kappa max |W|, and 16 x that
APPLY_GAP = 0.958
GRAPPA_TOL = 15.3
ROUTE_GAP = 0.990
GRAPPA_CAL_TOL = 15.8
SCORE_ORACLE = 0.2  # every end-to-end case in the oracle
SCORE_PACKAGE = 0.25  # ... and through the package; zeros in the missing lines score 1.0


def bound(want, dtype=np.complex128):
    """On |y - oracle|: GRAPPA_TOL units; complex64 adds the one rounding the definition makes, eps32 |y|."""
    b = GRAPPA_TOL * want["unit"]
    if np.dtype(dtype) == np.complex64:
        b = b + orc.EPS32 * np.abs(want["y"])
    return b


def check(y, want, dtype=np.complex128, what=""):
    """y against an oracle result: the acquired lines exact, the others within the bound; returns the worst fraction."""
    acq = want["acquired"]
    assert np.array_equal(y[:, acq], want["y"][:, acq].astype(dtype)), what
    b = bound(want, dtype)[:, ~acq]
    d = np.abs(y[:, ~acq] - want["y"][:, ~acq])
    assert not d[b == 0].any(), what
    fr = float((d[b > 0] / b[b > 0]).max()) if (b > 0).any() else 0.0
    print(f"{what}: y {fr:.3f} of the bound")
    assert fr <= 1.0, (what, fr)
    return fr


# ---- the oracle -----------------------------------------------------------------------------------------------------------
def test_sampling_and_source_rules():
    for n, r in ((16, 2), (11, 3), (3, 2), (3, 3), (1, 2), (5, 4)):
        kept = orc.kept_lines(n, r)
        assert np.array_equal(kept, (r * n) // 2 + r * (np.arange(n) - n // 2))  # the rule of section 16
        for j in range(r * n):
            l, o = orc.split(j, n, r)
            assert 0 <= o < r and j == orc.first_line(n, r) + r * l + o and -1 <= l < n
            assert (o == 0) == (j in kept)
    assert orc.split(0, 3, 2) == (-1, 1)  # j0 = 1: the floor, not a truncation
    assert orc.type_offsets((2, 3)) == [(0, 1), (0, 2), (1, 0), (1, 1), (1, 2)]
    assert [orc.type_index(o, (2, 3)) for o in orc.type_offsets((2, 3))] == [0, 1, 2, 3, 4]
    assert orc.neighbours((2, 3)) == [(0, -1), (0, 0), (0, 1), (1, -1), (1, 0), (1, 1)]  # b = 2 straddles, b = 3 is centred
    assert orc.neighbours((4,)) == [(-1,), (0,), (1,), (2,)]
    assert orc.sources((0,), (1,), (2,), (4,)) == (0, [(2, (0,))])  # l = -1: only s = 1 is a kept line
    assert orc.sources((1,), (1,), (2,), (4,)) == (-1, [(0, (0,))])


@pytest.mark.parametrize("name", list(orc.APPLY_CASES))
def test_ascending_sum_against_long_double(name):
    r = orc.apply_case(name)[4]
    g = orc.gap(r["y"], r["alt"], r["unit"])
    print(name, g)
    assert g <= GRAPPA_TOL / 16 * 1.01


def test_tolerance_constants_match_their_tool():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "grappa", "tolerance.txt")).read()
    assert orc.worst_apply_gap() == pytest.approx(APPLY_GAP, rel=0.02)
    assert GRAPPA_TOL == pytest.approx(16 * APPLY_GAP, rel=0.04) and float(re.search(r"GRAPPA_TOL = ([0-9.]+)", text).group(1)) == GRAPPA_TOL
    assert orc.worst_calibration_gap() == pytest.approx(ROUTE_GAP, rel=0.02)
    assert GRAPPA_CAL_TOL == pytest.approx(16 * ROUTE_GAP, rel=0.04)
    assert float(re.search(r"GRAPPA_CAL_TOL = ([0-9.]+)", text).group(1)) == GRAPPA_CAL_TOL


def test_case_selection():
    """The four cases of the issue, none excluded, and the conditions on them."""
    want = {((16, 32), (2, 1), (2, 3), 8, (12, 12), 1e-6), ((16, 16), (2, 2), (2, 2), 12, (14, 14), 1e-6),
            ((16, 16), (2, 2), (4, 3), 8, (16, 16), 1e-4), ((11, 30), (3, 1), (2, 3), 8, (14, 14), 1e-6)}
    assert set(orc.E2E_CASES.values()) == want and orc.E2E_POINTS == 3
    for name, case in orc.E2E_CASES.items():
        cal, res, sc = orc.e2e_oracle(name)
        k = case[3] * int(np.prod(case[2]))
        print(name, sc, max(cal["kappa"]), cal["n_eq"], k)
        assert case[5] >= 1e-6 and max(cal["kappa"]) <= 1e8 and min(cal["n_eq"]) >= 2 * k
        assert sc <= SCORE_ORACLE
        assert orc.score(np.where(res["acquired"][None, ..., None], res["y"], 0.0), orc.e2e_case(name)["full"], res["acquired"]) == 1.0
        assert orc.calibration_gap(cal, orc.e2e_oracle(name, "lstsq")[0]) <= GRAPPA_CAL_TOL / 16 * 1.01


def test_oracle_apply_on_exactly_interpolable_data():
    """Weights that copy the nearest kept line of the same coil: every missing line becomes that line, bit for bit."""
    a = orc.make((3, 4, 5), 3)
    w = np.zeros((1, 3, 2, 3), dtype=complex)
    w[0, :, 0, :] = np.eye(3)  # s = 0: the kept line below
    r = orc.fill(a, w, (2,), (2,))
    assert np.array_equal(r["y"][:, 0::2], a) and np.array_equal(r["y"][:, 1::2], a) and np.array_equal(r["y"], r["alt"])
    assert np.array_equal(r["acquired"], [True, False] * 4)


# ---- the Python layer on the numpy stand-in ----------------------------------------------------------------------------
def np_grappa_fill(x, weights, coil_axis, spatial_axes, time_axis, accel, kernel):
    """``device.grappa_fill`` from the oracle: the input's axis order with time last, every spatial axis grown."""
    nd = x.ndim
    coil_axis, time_axis = coil_axis % nd, time_axis % nd
    axes = [a % nd for a in spatial_axes]
    batch = [a for a in range(nd) if a not in (coil_axis, time_axis, *axes)]
    xv = np.transpose(x, batch + [coil_axis] + axes + [time_axis])
    bshape = xv.shape[:len(batch)]
    full = [r * x.shape[a] for r, a in zip(accel, axes)]
    y = np.zeros((*bshape, x.shape[coil_axis], *full, x.shape[time_axis]), dtype=x.dtype)
    w = np.zeros((0,)) if weights is None else np.asarray(weights)
    for i in np.ndindex(*bshape):
        y[i] = orc.fill(xv[i], w, tuple(accel), tuple(kernel))["y"].astype(x.dtype)
    have = batch + [coil_axis] + axes
    order = [a for a in range(nd) if a != time_axis]
    return np.ascontiguousarray(np.transpose(y, [have.index(a) for a in order] + [len(have)]))


@pytest.fixture
def numpy_device(monkeypatch):
    import _numpy_device
    from xmris_amd import device as dev

    _numpy_device.install(monkeypatch)
    calls = []

    def fill(*a, **k):
        calls.append("grappa_fill")
        return np_grappa_fill(*a, **k)

    monkeypatch.setattr(dev, "grappa_fill", fill)
    return calls


def labeled_case(name, dtype=np.complex128, dk=0.25):
    """(kept lines as a LabeledArray (coil, kx, ky, time), the ACS block as a LabeledArray, the case)."""
    from xmris_amd import LabeledArray

    cs = orc.e2e_case(name)
    kept = cs["kept"]
    coords = {d: orc.kept_lines(n, r) * dk - (r * n // 2) * dk for d, n, r in zip(("kx", "ky"), kept.shape[1:], cs["accel"])}
    coords["time"] = np.arange(kept.shape[-1]) * 1e-3
    la = LabeledArray(kept.astype(dtype), ("coil", "kx", "ky", "time"), coords, {"note": "kept"}, "csi")
    return la, LabeledArray(cs["acs"], ("coil", "kx", "ky", "time")), cs


@pytest.mark.parametrize("name", list(orc.E2E_CASES))
@pytest.mark.parametrize("route", ["normal", "lstsq"])
def test_calibrate_against_the_oracle(name, route):
    from xmris_amd import GrappaWeights, grappa_calibrate

    _, acs, cs = labeled_case(name)
    want = orc.e2e_oracle(name, route)[0]
    got = grappa_calibrate(acs, cs["accel"], cs["kernel"], regularization=cs["lam"])
    assert isinstance(got, GrappaWeights) and got.weights.shape == want["w"].shape and got.weights.dtype == np.complex128
    assert got.accel == cs["accel"] and got.kernel == cs["kernel"] and got.dims == ("kx", "ky") and got.coils == cs["coils"]
    assert got.n_equations == tuple(want["n_eq"]) and got.regularization == cs["lam"]
    fr = max(float(np.abs(g - w).max()) / u for g, w, u in zip(got.weights, want["w"], want["unit"]))
    print(f"{name} {route}: weights {fr / GRAPPA_CAL_TOL:.3f} of the bound")
    assert fr <= GRAPPA_CAL_TOL
    assert np.allclose(got.kappa, want["kappa"], rtol=1e-3) and np.allclose(got.residual, want["residual"], rtol=1e-3, atol=1e-12)


@pytest.mark.parametrize("name", list(orc.E2E_CASES))
def test_end_to_end_reconstructs_the_missing_lines(numpy_device, name):
    from xmris_amd import ATTRS

    la, acs, cs = labeled_case(name)
    out, rec = la.xmr.grappa_fill(acs=acs, accel=cs["accel"], kernel=cs["kernel"], regularization=cs["lam"], return_weights=True)
    assert numpy_device == ["grappa_fill"] and out.dims == la.dims and out.shape == cs["full"].shape
    acquired = orc.e2e_oracle(name)[1]["acquired"]
    sc = orc.score(out.values, cs["full"], acquired)
    print(f"{name}: score {sc:.4f} (oracle {orc.e2e_oracle(name)[2]:.4f})")
    assert sc <= SCORE_PACKAGE
    assert np.array_equal(out.values[:, acquired], cs["kept"].reshape(cs["coils"], -1, 3))  # the acquired lines, bit for bit
    assert out.attrs[ATTRS.grappa_kernel] == cs["kernel"] and out.attrs[ATTRS.grappa_regularization] == cs["lam"]
    # weights= gives what acs= gave
    again = la.xmr.grappa_fill(rec)
    assert np.array_equal(again.values, out.values) and again.attrs == out.attrs
    assert np.array_equal(la.values, cs["kept"])  # the input is untouched


@pytest.mark.parametrize("shape, accel, kernel", [((4, 10, 10, 3), (2, 1), (1, 3)), ((4, 10, 10, 3), (2, 2), (1, 2)),
                                                  ((4, 10, 10, 3), (3, 2), (1, 1)), ((4, 9, 10, 3), (2, 2), (3, 1))])
@pytest.mark.parametrize("route", ["normal", "lstsq"])
def test_calibrate_with_one_line_along_an_accelerated_dim(shape, accel, kernel, route):
    """b = 1 at R > 1: the only source lies below the target, so the block's last lines are targets no more."""
    from xmris_amd import grappa_calibrate

    acs = orc.make(shape, 5)
    want = orc.calibrate(acs, accel, kernel, lam=1e-4, route=route)
    got = grappa_calibrate(acs, accel, kernel)
    assert got.n_equations == tuple(want["n_eq"]) and got.weights.shape == want["w"].shape
    fr = max(float(np.abs(g - w).max()) / u for g, w, u in zip(got.weights, want["w"], want["unit"]))
    print(f"accel {accel} kernel {kernel} {route}: weights {fr / GRAPPA_CAL_TOL:.3f} of the bound")
    assert fr <= GRAPPA_CAL_TOL


def test_fill_with_one_line_along_an_accelerated_dim(numpy_device):
    from xmris_amd import LabeledArray, grappa_fill

    la, acs, cs = labeled_case("16x32_r2x1_b2x3_c8")
    out, rec = grappa_fill(la, acs=acs, accel=(2, 1), kernel=(1, 3), regularization=1e-6, return_weights=True)
    assert rec.kernel == (1, 3) and rec.weights.shape == (1, 8, 3, 8) and out.shape == (8, 32, 32, 3)
    want = orc.fill(cs["kept"], orc.calibrate(cs["acs"], (2, 1), (1, 3), lam=1e-6)["w"], (2, 1), (1, 3))
    assert np.array_equal(out.values[:, want["acquired"]], cs["kept"].reshape(8, -1, 3))
    assert orc.score(out.values, cs["full"], want["acquired"]) == pytest.approx(orc.score(want["y"], cs["full"], want["acquired"]), rel=1e-6)


def test_default_kernel_and_acs_without_time(numpy_device):
    from xmris_amd import LabeledArray, grappa_calibrate, grappa_fill

    la, acs, cs = labeled_case("16x32_r2x1_b2x3_c8")
    rec = grappa_calibrate(acs, (2, 1), regularization=1e-6)
    assert rec.kernel == (2, 3)  # 2 along an accelerated dim, 3 along the other
    assert grappa_calibrate(acs, 2).kernel == (2, 2) and grappa_calibrate(acs, 2).regularization == 1e-4
    flat = LabeledArray(acs.values[..., 0], ("coil", "kx", "ky"))
    one = grappa_calibrate(flat, (2, 1), regularization=1e-6)
    assert one.n_equations == (100,) and one.weights.shape == (1, 8, 6, 8)
    w1 = orc.calibrate(acs.values[..., :1], (2, 1), (2, 3), lam=1e-6)
    assert max(float(np.abs(g - w).max()) / u for g, w, u in zip(one.weights, w1["w"], w1["unit"])) <= GRAPPA_CAL_TOL
    assert grappa_calibrate(acs, (2, 1), acs_points=1, regularization=1e-6).n_equations == (100,)
    # plain arrays in the order (coil, *dims, time) and transposed labeled blocks give the same weights
    assert np.array_equal(grappa_calibrate(acs.values, (2, 1), regularization=1e-6).weights, rec.weights)
    moved = LabeledArray(np.ascontiguousarray(np.transpose(acs.values, (3, 2, 0, 1))), ("time", "ky", "coil", "kx"))
    assert np.array_equal(grappa_calibrate(moved, (2, 1), regularization=1e-6).weights, rec.weights)
    out = grappa_fill(la, acs=flat, accel=(2, 1), regularization=1e-6)
    assert out.shape == (8, 32, 32, 3)


def test_accel_one_is_the_identity(numpy_device):
    la, acs, _ = labeled_case("16x32_r2x1_b2x3_c8", np.complex64)
    out = la.xmr.grappa_fill(acs=acs, accel=1)
    assert np.array_equal(out.values, la.values) and out.values.dtype == np.complex64 and out.dims == la.dims
    assert all(np.array_equal(out.coords[d].values, la.coords[d].values) for d in ("kx", "ky", "time"))


def test_coordinates_attrs_and_layouts(numpy_device):
    from xmris_amd import ATTRS, LabeledArray, grappa_calibrate, grappa_fill

    la, acs, cs = labeled_case("16x16_r2x2_b2x2_c12")
    rec = grappa_calibrate(acs, 2, 2, regularization=1e-6)
    extra = dict(la.coords)
    extra["ky_label"] = ("ky", np.arange(16))
    extra["coil"] = np.arange(12)
    src = LabeledArray(la.values, la.dims, extra, la.attrs, la.name)
    out = grappa_fill(src, rec)
    assert out.attrs == {"note": "kept", ATTRS.grappa_dims: ("kx", "ky"), ATTRS.grappa_accel: (2, 2), ATTRS.grappa_kernel: (2, 2),
                         ATTRS.grappa_regularization: 1e-6}
    assert src.attrs == {"note": "kept"} and out.name == "csi" and out.dims == ("coil", "kx", "ky", "time")
    for d in ("kx", "ky"):  # the coordinate of the full grid: (arange(N) - N // 2) dk, dk = the input's spacing over accel
        assert np.allclose(out.coords[d].values, (np.arange(32) - 16) * 0.25, rtol=1e-14, atol=0) and out.coords[d].dim == d
        assert np.allclose(out.coords[d].values[orc.kept_lines(16, 2)], la.coords[d].values, rtol=1e-14, atol=0)
    assert "ky_label" not in out.coords and np.array_equal(out.coords["coil"].values, np.arange(12))
    assert np.array_equal(out.coords["time"].values, la.coords["time"].values)
    # a repetition axis, the coil axis between the dims, time not last, the dims in the other order
    rep = np.stack([la.values, 2 * la.values])  # (rep, coil, kx, ky, time)
    moved = LabeledArray(np.ascontiguousarray(np.transpose(rep, (4, 2, 1, 0, 3))), ("time", "kx", "coil", "rep", "ky"))
    got = grappa_fill(moved, rec)
    assert got.dims == ("time", "kx", "coil", "rep", "ky") and got.shape == (3, 32, 12, 2, 32)
    back = np.transpose(got.values, (3, 2, 1, 4, 0))
    assert np.array_equal(back[0], out.values) and np.array_equal(back[1], 2 * out.values)
    sw = grappa_calibrate(LabeledArray(np.swapaxes(acs.values, 1, 2), ("coil", "ky", "kx", "time")), 2, 2, dims=("ky", "kx"),
                          regularization=1e-6)
    assert sw.dims == ("ky", "kx")
    swapped = grappa_fill(la, sw)  # dims from the weights
    assert swapped.attrs[ATTRS.grappa_dims] == ("ky", "kx") and swapped.dims == la.dims
    # the same equations and the same terms in another order: each weight within the calibration bound of the oracle's,
    # times at most K source samples; and the two sums within the apply bound
    cal, want, _ = orc.e2e_oracle("16x16_r2x2_b2x2_c12")
    tol = 2 * GRAPPA_CAL_TOL * max(cal["unit"]) * 48 * np.abs(la.values).max() + 2 * GRAPPA_TOL * want["unit"]
    assert np.all(np.abs(swapped.values - out.values) <= tol)
    single = LabeledArray(la.values[:, :1], la.dims, {"kx": [3.0]})
    assert np.array_equal(grappa_fill(single, acs=acs, accel=(2, 1), regularization=1e-6).coords["kx"].values, [-0.5, 0.0])


def test_dataset_member_and_dataarray_bridge(numpy_device, monkeypatch):
    import _fake_xarray

    xr = _fake_xarray.install(monkeypatch)
    import xmris_amd
    from xmris_amd.fitting.dataset import LabeledDataset

    xmris_amd.register_xarray_accessor(force=True)
    la, acs, cs = labeled_case("11x30_r3x1_b2x3_c8")
    want = la.xmr.grappa_fill(acs=acs, accel=(3, 1), regularization=1e-6)
    ds = LabeledDataset({"k": la, "centre": acs}, {"study": 1})
    got = ds["k"].xmr.grappa_fill(acs=ds["centre"], accel=(3, 1), regularization=1e-6)
    assert np.array_equal(got.values, want.values) and got.dims == want.dims
    da = xr.DataArray(la.values, dims=la.dims, coords={"kx": la.coords["kx"].values}, attrs={"a": 1}, name="k")
    ax = xr.DataArray(acs.values, dims=acs.dims)
    out = xmris_amd.grappa_fill(da, acs=ax, accel=(3, 1), regularization=1e-6)
    assert type(out) is xr.DataArray and out.dims == la.dims and out.name == "k" and out.attrs["a"] == 1
    assert isinstance(out.values, np.ndarray) and out.shape == (8, 33, 30, 3) and np.array_equal(out.values, want.values)
    assert np.array_equal(da.xmr.grappa_fill(acs=acs.values, accel=(3, 1), regularization=1e-6).values, out.values)


# ---- validation: every error fires before any native call -----------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    from xmris_amd import _lib
    from xmris_amd import device as dev

    def boom(*a, **k):
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "call", boom)
    for name in ("to_device", "grappa_fill"):
        monkeypatch.setattr(dev, name, boom)


def _la(shape=(4, 3, 5, 6), dims=("coil", "kx", "ky", "time")):
    from xmris_amd import LabeledArray

    return LabeledArray(orc.make(shape, 1), dims)


_ACS = orc.make((4, 8, 8, 2), 2)


def _weights(**kw):
    from xmris_amd import grappa_calibrate

    return grappa_calibrate(_ACS, **dict(dict(accel=2), **kw))


@pytest.mark.parametrize("kw, word", [
    (dict(), "weights"),  # neither weights nor acs
    (dict(weights="w", acs=_ACS, accel=2), "weights"),  # both
    (dict(weights=np.ones((3, 4, 4, 4))), "weights"),  # not a GrappaWeights
    (dict(acs=_ACS), "accel"),
    (dict(acs=_ACS, accel=(2, 2, 2)), "accel"),
    (dict(acs=_ACS, accel=0), "accel"),
    (dict(acs=_ACS, accel=(2, -1)), "accel"),
    (dict(acs=_ACS, accel=2.5), "accel"),
    (dict(acs=_ACS, accel="two"), "accel"),
    (dict(acs=_ACS, accel=(4, 8)), "accel"),  # R = 32
    (dict(acs=_ACS, accel=2, kernel=0), "kernel"),
    (dict(acs=_ACS, accel=2, kernel=(2, 2, 2)), "kernel"),
    (dict(acs=_ACS, accel=2, kernel=1.5), "kernel"),
    (dict(acs=_ACS, accel=2, kernel=(9, 8)), "kernel"),  # S = 72
    (dict(acs=_ACS, accel=2, acs_points=0), "acs_points"),
    (dict(acs=_ACS, accel=2, acs_points=1.5), "acs_points"),
    (dict(acs=_ACS, accel=2, regularization=-0.1), "regularization"),
    (dict(acs=_ACS, accel=2, regularization=float("nan")), "regularization"),
    (dict(acs=_ACS, accel=2, regularization="much"), "regularization"),
    (dict(acs=_ACS[:3], accel=2), "acs"),  # 3 coils, the data has 4
    (dict(acs=_ACS[:, :, :, 0, None, None], accel=2), "acs"),  # too many axes
    (dict(acs=_ACS[:, :3, :3], accel=2), "acs"),  # 2 x 2 positions x 2 points: fewer equations than 16 unknowns
    (dict(acs=np.zeros((4, 8, 8, 2)), accel=2, regularization=0), "acs"),  # singular
    (dict(acs=np.where(np.arange(8)[:, None] == 3, np.nan, _ACS), accel=2), "acs"),  # not finite
    (dict(acs=_ACS, accel=2, dims=("kx", "coil")), "coil_dim"),
    (dict(acs=_ACS, accel=2, dims=("kx", "time")), "time_dim"),
    (dict(acs=_ACS, accel=2, coil_dim="channel"), "coil_dim"),
    (dict(acs=_ACS, accel=2, time_dim="t"), "time_dim"),
    (dict(acs=_ACS, accel=2, dims=("kx", "kx")), "dims"),
    (dict(acs=_ACS, accel=2, dims=()), "dims"),
])
def test_validation_errors_name_their_argument(no_library, kw, word):
    from xmris_amd import grappa_fill

    with pytest.raises(ValueError, match=word):
        grappa_fill(_la(), **kw)
    with pytest.raises(ValueError, match=word):
        _la().xmr.grappa_fill(**kw)


def test_weights_that_disagree_with_the_data_are_refused(no_library):
    from xmris_amd import LabeledArray, grappa_calibrate, grappa_fill

    w = _weights()
    for kw in (dict(accel=(2, 1)), dict(kernel=3), dict(dims=("ky", "kx")), dict(dims="kx")):
        with pytest.raises(ValueError, match="weights"):
            grappa_fill(_la(), w, **kw)
    with pytest.raises(ValueError, match="weights"):  # 5 coils, calibrated for 4
        grappa_fill(_la((5, 3, 5, 6)), w)
    with pytest.raises(ValueError, match=r"Method 'grappa_fill' attempted to operate on missing dimension\(s\): \['kz'\]"):
        grappa_fill(_la(), acs=_ACS, accel=2, dims=("kx", "kz"))
    with pytest.raises(ValueError, match="coil_dim"):  # 65 coils
        grappa_fill(_la((65, 3, 5, 2)), acs=orc.make((65, 8, 8, 2), 1), accel=2)
    with pytest.raises(ValueError, match="kernel"):  # 64 coils x 32 neighbours
        grappa_fill(_la((64, 3, 5, 2)), acs=orc.make((64, 8, 8, 2), 1), accel=2, kernel=(4, 8))
    with pytest.raises(ValueError, match="acs"):  # a labeled block with other dims
        grappa_fill(_la(), acs=LabeledArray(_ACS, ("coil", "kx", "kz", "time")), accel=2)
    with pytest.raises(ValueError, match="2\\^26.*acs_points"):  # 1024 x (66 x 66 positions x 16 points) entries
        grappa_calibrate(np.ones((16, 80, 80, 16), dtype=complex), 2, (8, 8), acs_points=16)
    with pytest.raises(TypeError):
        grappa_fill(np.zeros((4, 3, 5, 6), complex), w)


def _abi_call(lib, a):
    i32 = ctypes.c_int32 * 3
    vec = lambda v, t: None if v is None else t(*v)  # noqa: E731
    return lib.xm_grappa_fill(a["a"], a["y"], a["w"], a["no"], a["C"], vec(a["n"], i32), vec(a["accel"], i32), vec(a["kernel"], i32),
                              a["Nt"], vec(a["as"], ctypes.c_int64 * 5), vec(a["ys"], ctypes.c_int64 * 5), a["dtype"], None)


# a (2, 4, 3, 4, 8) -> y (2, 4, 6, 8, 8): two repetitions, 4 coils, 3 x 4 kept lines filled 2 x 2, 8 points
ABI_OK = {"a": 16, "y": 32, "w": 48, "no": 2, "C": 4, "n": (1, 3, 4), "accel": (1, 2, 2), "kernel": (1, 2, 2), "Nt": 8,
          "as": (384, 96, 0, 32, 8), "ys": (1536, 384, 0, 64, 8), "dtype": 0}
ABI_BAD = (dict(a=None), dict(y=None), dict(w=None), dict(n=None), dict(accel=None), dict(kernel=None), {"as": None},
           dict(ys=None), dict(C=0), dict(C=65), dict(accel=(1, 0, 2)), dict(accel=(1, -2, 2)), dict(accel=(2, 3, 3)),
           dict(accel=(1, 1, 17)), dict(kernel=(1, 0, 2)), dict(kernel=(1, -2, 2)), dict(kernel=(1, 9, 8)), dict(kernel=(5, 5, 3)),
           dict(C=64, kernel=(1, 4, 8)), dict(C=17, kernel=(1, 8, 8)), dict(n=(1, 0, 4)), dict(n=(0, 3, 4)), dict(Nt=0),
           dict(dtype=2), dict(dtype=-1), dict(y=16), dict(no=-1), dict(no=1 << 40), dict(n=(1, 1 << 15, 1 << 15)),
           dict(no=1 << 20, Nt=1 << 20))


def test_c_abi_refusals_without_gpu():
    from xmris_amd import _lib

    lib = _lib.load()
    assert lib.xm_version() >= 500
    for change in ABI_BAD:
        rc = _abi_call(lib, dict(ABI_OK, **change))
        assert rc == _lib.XM_ERR_INVALID_ARG, change
        assert b"grappa_fill" in lib.xm_last_error_string()
    assert _abi_call(lib, dict(ABI_OK, no=0)) == 0  # a zero-sized problem launches nothing, whatever the pointers hold
    assert _abi_call(lib, dict(ABI_OK, no=0, w=None, accel=(1, 1, 1))) == 0  # R = 1 takes no weights


def test_vocabulary_and_exports():
    import xmris_amd
    from xmris_amd import ATTRS, processing
    from xmris_amd import device as dev

    assert (ATTRS.grappa_dims, ATTRS.grappa_accel, ATTRS.grappa_kernel, ATTRS.grappa_regularization) == (
        "grappa_dims", "grappa_accel", "grappa_kernel", "grappa_regularization")
    for name in ("grappa_calibrate", "grappa_fill", "GrappaWeights"):
        assert getattr(xmris_amd, name) is getattr(processing, name) and name in xmris_amd.__all__ and name in processing.__all__
    assert hasattr(xmris_amd.XmrisAccessor, "grappa_fill")
    assert (dev.GRAPPA_MAX_COILS, dev.GRAPPA_MAX_ACCEL, dev.GRAPPA_MAX_SOURCES, dev.GRAPPA_MAX_TERMS) == (64, 16, 64, 1024)
    from xmris_amd.processing import grappa

    assert (grappa.MAX_COILS, grappa.MAX_ACCEL, grappa.MAX_SOURCES, grappa.MAX_TERMS) == (64, 16, 64, 1024)  # the device's own
    assert "xm_grappa_fill" in xmris_amd._lib.SIGNATURES
