"""CPU tests of unfold_sense / sense_maps: the oracle's two routes agree within the figure SENSE_TOL is made from, the
aliasing model of the definition is what to_kspace -> kept lines -> to_image gives, the parity
cases are well conditioned, the Python layer (on a numpy stand-in for ``device.unfold_sense`` built from the oracle)
keeps dims, coordinates, attrs and names as specified, every validation error fires before the library is reached, and
xm_sense_unfold refuses bad arguments without a GPU.

The tests of the oracle alone import nothing from the package and pass without the feature; all others fail without it."""
import ctypes
import os
import re

import numpy as np
import pytest

import _coils_oracle as corc
import _mrsi_oracle as morc
import _sense_oracle as orc
from test_mrsi import MRSI_TOL

# the largest disagreement of the oracle's two routes (normal equations + Cholesky against the pseudo-inverse of the
# stacked system) over orc.PARITY_CASES, in units of eps kappa sum |U| |a| -- tests/tool_sense_tolerance.py, recorded in
# profiles/sense/tolerance.txt -- and 16 x that
ROUTE_GAP = 3.782
SENSE_TOL = 60.5


def bound(want, dtype=np.complex128):
    """On |rho - oracle|: SENSE_TOL units; complex64 adds the one rounding the definition makes, eps32 |rho|."""
    b = SENSE_TOL * want["unit"]
    if np.dtype(dtype) == np.complex64:
        b = b + orc.EPS32 * np.abs(want["rho"])
    return b


def check(rho, g, status, want, dtype=np.complex128, what="", extra=0.0):
    """rho, g and status against an oracle result; returns the worst fractions of the bounds (rho, g)."""
    assert np.array_equal(status, want["status"]), (what, status, want["status"])
    b = bound(want, dtype) + extra
    d = np.abs(rho - want["rho"])
    assert not d[b == 0].any(), what
    fr = float((d[b > 0] / b[b > 0]).max()) if (b > 0).any() else 0.0
    ok = want["status"] == 0
    assert np.array_equal(np.isnan(g), want["status"] >= 2) and not g[want["status"] == 1].any(), what
    gb = SENSE_TOL * want["gunit"][ok]
    fg = float((np.abs(g[ok] - want["g"][ok]) / gb).max()) if ok.any() else 0.0
    print(f"{what}: rho {fr:.3f}  g {fg:.3f} of the bound")
    assert fr <= 1.0 and fg <= 1.0, (what, fr, fg)
    return fr, fg


# ---- the oracle -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(orc.PARITY_CASES))
def test_routes_agree(name):
    gr, gg = orc.route_gaps(name)
    print(name, gr, gg)
    assert max(gr, gg) <= SENSE_TOL / 16 * 1.01


def test_tolerance_constant_matches_its_tool():
    worst = orc.worst_route_gap()
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "sense", "tolerance.txt")).read()
    recorded = float(re.search(r"SENSE_TOL = ([0-9.]+)", text).group(1))
    assert worst == pytest.approx(ROUTE_GAP, rel=0.02), worst
    assert SENSE_TOL == pytest.approx(16 * worst, rel=0.04) and recorded == SENSE_TOL


def test_case_selection():
    """The cases of the issue, none excluded: every group is well conditioned and no Cholesky pivot is near zero, so
    status 3 is never a coin toss."""
    want = {((4, 5), (2, 1), 4), ((5, 3), (2, 3), 12), ((3, 4), (3, 2), 8), ((2, 2), (4, 4), 32), ((2, 3, 2), (2, 2, 2), 16),
            ((7, 5), (1, 1), 64), ((3,), (1,), 1)}
    assert {c[:3] for c in orc.PARITY_CASES.values()} == want
    for name in orc.PARITY_CASES:
        a = orc.parity_routes(name)[0]
        assert np.all(a["status"] == 0) and np.all(a["kappa"] <= 1e6), (name, np.nanmax(a["kappa"]))
        assert np.all(a["pivot"] > 1e-9), (name, np.nanmin(a["pivot"]))


def _kspace_route(name):
    """(aliased images by to_kspace -> kept lines -> to_image on the oracle of section 14, a bound on their error)."""
    rho, sens, a, rs = orc.parity_case(name)
    axes = list(range(1, 1 + len(rs)))
    full = sens[..., None] * rho[None]
    k = morc.reconstruct(full, axes, sign=-1)
    dk = MRSI_TOL * np.broadcast_to(morc.unit(full, axes), k.shape)
    ku, dku = orc.undersample(k, axes, rs), orc.undersample(dk, axes, rs)
    img = morc.reconstruct(ku, axes, sign=1)
    err = MRSI_TOL * morc.unit(ku, axes) + morc.unit(dku, axes) / morc.EPS
    return img, np.broadcast_to(err, img.shape)


@pytest.mark.parametrize("name", list(orc.PARITY_CASES))
def test_aliasing_identity(name):
    """to_image of the kept lines is the sum over the group divided by sqrt(R), with no extra phase, at every parity."""
    a = orc.parity_case(name)[2]
    img, err = _kspace_route(name)
    fwd = orc.EPS * np.abs(a) * 16  # the forward model's own sums: at most 16 terms
    print(name, float((np.abs(img - a) / (err + fwd)).max()))
    assert np.all(np.abs(img - a) <= err + fwd)


@pytest.mark.parametrize("name", list(orc.PARITY_CASES))
def test_oracle_returns_the_truth(name):
    rho, sens, a, rs = orc.parity_case(name)
    fwd = orc.EPS * 16 * np.sqrt(np.prod(rs)) * np.einsum("c...,...t->c...t", np.abs(sens), np.abs(rho))  # per term
    da = np.zeros(a.shape)
    for p, qq in orc.groups(a.shape[1:-1], rs):
        da[(slice(None), *p)] = sum(fwd[(slice(None), *q)] for q in qq) / np.prod(rs)
    for route in ("chol", "lstsq"):
        got = orc.unfold(a, sens, rs, route=route, da=da)
        assert np.all(np.abs(got["rho"] - rho) <= SENSE_TOL * got["unit"] + got["prop"]), (name, route)


def test_oracle_status_rules_and_g():
    rho, sens, a, rs = orc.parity_case("3x4_r3x2_c8")
    s = sens.copy()
    s[:, 0, 0] = 0.0  # one masked member
    grp = list(orc.groups((3, 4), rs))[5][1]
    for q in grp:
        s[(slice(None), *q)] = 0.0  # a group fully masked
    got = orc.unfold(a, s, rs)
    assert got["status"][0, 0] == 1 and got["g"][0, 0] == 0 and not got["rho"][0, 0].any()
    assert all(got["status"][q] == 1 for q in grp)
    assert (got["status"] == 1).sum() == 1 + len(grp) and (got["status"] == 0).sum() == s[0].size - 1 - len(grp)
    bad = np.array(a)
    bad[2, 1, 1, 3] = np.nan
    got = orc.unfold(bad, sens, rs)
    grp = [q for p, qq in orc.groups((3, 4), rs) if p == (1, 1) for q in qq]
    assert all(got["status"][q] == 2 and np.isnan(got["g"][q]) and not got["rho"][q].any() for q in grp)
    assert (got["status"] == 2).sum() == 6
    # more members than coils at lambda = 0 is status 3; a regularised system is solvable
    one = orc.unfold(a[:1], sens[:1], rs)
    assert np.all(one["status"] == 3) and np.all(np.isnan(one["g"]))
    assert np.all(orc.unfold(a[:1], sens[:1], rs, lam=0.01)["status"] == 0)
    # g = 1 at R = 1, >= 1 at lambda = 0 (Cauchy-Schwarz)
    assert np.allclose(orc.parity_routes("7x5_r1x1_c64")[0]["g"], 1.0, atol=1e-14)
    assert np.all(orc.parity_routes("5x3_r2x3_c12")[0]["g"] >= 1.0 - 1e-12)


# ---- the Python layer on the numpy stand-in ----------------------------------------------------------------------------
class _Result:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def np_unfold_sense(x, sens, coil_axis, spatial_axes, time_axis, accel, linv=None, regularization=0.0, workspace=None):
    """``device.unfold_sense`` from the oracle: y in the input's axis order without the coil axis, time last; g and status
    with the batch axes in front and the spatial axes in the order given."""
    nd = x.ndim
    coil_axis, time_axis = coil_axis % nd, time_axis % nd
    axes = [a % nd for a in spatial_axes]
    batch = [a for a in range(nd) if a not in (coil_axis, time_axis, *axes)]
    xv = np.transpose(x, batch + [coil_axis] + axes + [time_axis])
    bshape = xv.shape[:len(batch)]
    full = [r * x.shape[a] for r, a in zip(accel, axes)]
    y = np.zeros((*bshape, *full, x.shape[time_axis]), dtype=x.dtype)
    g, status = np.zeros((*bshape, *full)), np.zeros((*bshape, *full), dtype=np.int32)
    for i in np.ndindex(*bshape):
        r = orc.unfold(xv[i], np.asarray(sens), accel, lam=regularization, w=linv)
        y[i], g[i], status[i] = r["rho"].astype(x.dtype), r["g"], r["status"]
    have = batch + axes
    order = [a for a in range(nd) if a not in (coil_axis, time_axis)]
    return _Result(y=np.ascontiguousarray(np.transpose(y, [have.index(a) for a in order] + [len(have)])), g=g, status=status)


def np_coil_combine(x, coil_axis, time_axis, method="svd", reference=None, linv=None, n_points=1, workspace=None):
    assert time_axis % x.ndim == x.ndim - 1 and reference is None
    psi = None
    if linv is not None:
        chol = np.linalg.inv(linv)
        psi = chol @ chol.conj().T
    r = corc.combine_batch(x, coil_axis=coil_axis, psi=psi, method=method, n_points=n_points)
    return _Result(y=r["y"], weights=r["w"], quality=r["quality"], status=r["status"])


@pytest.fixture
def numpy_device(monkeypatch):
    import _numpy_device
    from test_mrsi import np_axis_dft
    from xmris_amd import device as dev

    _numpy_device.install(monkeypatch)
    calls = []

    def unfold(*a, **k):
        calls.append("unfold_sense")
        return np_unfold_sense(*a, **k)

    monkeypatch.setattr(dev, "unfold_sense", unfold)
    monkeypatch.setattr(dev, "coil_combine", np_coil_combine)
    monkeypatch.setattr(dev, "axis_dft", np_axis_dft)
    return calls


DIMS3 = ("x", "y", "z")


def labeled_case(name, dtype=np.complex128, dx=0.5):
    """(aliased LabeledArray (coil, dims..., time), sensitivities LabeledArray, accel, dims, truth)."""
    from xmris_amd import LabeledArray

    rho, sens, a, rs = orc.parity_case(name)
    dims = DIMS3[:len(rs)]
    coords = {d: (np.arange(n) - n // 2) * dx * r for d, n, r in zip(dims, a.shape[1:], rs)}
    coords["time"] = np.arange(a.shape[-1]) * 1e-3
    la = LabeledArray(a.astype(dtype), ("coil", *dims, "time"), coords, {"note": "kept"}, "csi")
    return la, LabeledArray(np.array(sens), ("coil", *dims)), rs, dims, rho


@pytest.mark.parametrize("name", list(orc.PARITY_CASES))
def test_python_layer_matches_the_oracle_on_the_stand_in(numpy_device, name):
    import xmris_amd

    la, sens, rs, dims, _ = labeled_case(name)
    want = orc.parity_routes(name)[0]
    ds = xmris_amd.unfold_sense(la, sens, rs, dims=dims, return_maps=True)
    assert numpy_device == ["unfold_sense"]
    assert ds["unfolded"].dims == (*dims, "time") and ds["g_factor"].dims == dims == ds["status"].dims
    check(ds["unfolded"].values, ds["g_factor"].values, ds["status"].values, want, what=name)
    assert np.array_equal(la.values, orc.parity_case(name)[2])  # the input is untouched


@pytest.mark.parametrize("name", list(orc.PARITY_CASES))
def test_round_trip_through_kspace(numpy_device, name):
    """truth -> to_kspace -> the kept lines -> to_image -> unfold_sense gives the truth back."""
    from xmris_amd import LabeledArray, to_image, to_kspace

    rho, sens, a, rs = orc.parity_case(name)
    dims = DIMS3[:len(rs)]
    kdims = tuple("k" + d for d in dims)
    full = LabeledArray(sens[..., None] * rho[None], ("coil", *dims, "time"), {d: np.arange(float(n)) for d, n in zip(dims, rho.shape)})
    k = to_kspace(full, dim=dims)
    kept = orc.undersample(k.values, list(range(1, 1 + len(rs))), rs)
    ku = LabeledArray(kept, ("coil", *kdims, "time"), {d: orc.kept_lines(n, r) * 1.0 for d, n, r in zip(kdims, kept.shape[1:], rs)})
    img = to_image(ku, dim=kdims)
    got = img.xmr.unfold_sense(sens, rs, dims=dims, return_maps=True)
    _, err = _kspace_route(name)
    want = orc.unfold(img.values, sens, rs, da=2 * err + orc.EPS * 16 * np.abs(a))
    d = np.abs(got["unfolded"].values - rho)
    assert np.all(got["status"].values == 0) and got["unfolded"].shape == rho.shape
    print(name, float((d / (SENSE_TOL * want["unit"] + want["prop"])).max()))
    assert np.all(d <= SENSE_TOL * want["unit"] + want["prop"])


def test_accel_one_with_sense_maps_is_combine_coils(numpy_device):
    from xmris_amd import LabeledArray, sense_maps, unfold_sense

    x = corc.make_data(6, 8, 1, 40, seed=61).reshape(2, 3, 8, 40)  # (x, y, coil, time)
    la = LabeledArray(x, ("x", "y", "coil", "time"), {"x": np.arange(2.0), "y": np.arange(3.0)})
    for psi in (None, corc.random_psd(8, 5)):
        want = corc.combine_batch(x, coil_axis=2, psi=psi)
        maps = sense_maps(la, noise_cov=psi, threshold=0.0)
        assert maps.dims == ("coil", "x", "y") and maps.values.dtype == np.complex128
        out = unfold_sense(la, maps, 1, noise_cov=psi, return_maps=True)
        assert out["unfolded"].dims == ("x", "y", "time") and np.all(out["status"].values == 0)
        # U = w^H to rounding: ||w||_1 max |x| eps per sample, times the 16 of the project's margin
        tol = 16 * 8 * orc.EPS * np.abs(want["w"]).sum(-1, keepdims=True) * np.abs(x).max(axis=2)
        assert np.all(np.abs(out["unfolded"].values - want["y"]) <= tol)
        assert np.allclose(out["g_factor"].values, 1.0, atol=1e-12)
    # voxels below the threshold are zero in every coil, and unfold_sense masks them
    weak = x.copy()
    weak[1, 2] *= 1e-3
    lw = LabeledArray(weak, la.dims, la.coords)
    maps = sense_maps(lw)
    assert not maps.values[:, 1, 2].any() and np.all(np.abs(maps.values).sum(0)[:1] > 0)
    out = unfold_sense(lw, maps, (1, 1), return_maps=True)
    assert out["status"].values[1, 2] == 1 and not out["unfolded"].values[1, 2].any() and out["status"].values.sum() == 1


def test_coordinates_equal_those_of_the_full_kspace(numpy_device):
    from xmris_amd import LabeledArray, to_image, unfold_sense

    rs, ns, c, t = (2, 3), (5, 4), 3, 4
    dk = (0.25, 0.5)
    big = [n * r for n, r in zip(ns, rs)]
    kfull = LabeledArray(orc.make((c, *big, t), 3), ("coil", "kx", "ky", "time"),
                         {"kx": (np.arange(big[0]) - big[0] // 2) * dk[0], "ky": (np.arange(big[1]) - big[1] // 2) * dk[1],
                          "ky_label": ("ky", np.arange(big[1])), "time": np.arange(t) * 1e-3, "coil": np.arange(c)})
    kept = orc.undersample(kfull.values, [1, 2], rs)
    ku = LabeledArray(kept, kfull.dims, {"kx": kfull.coords["kx"].values[orc.kept_lines(ns[0], rs[0])],
                                         "ky": kfull.coords["ky"].values[orc.kept_lines(ns[1], rs[1])],
                                         "ky_label": ("ky", np.arange(ns[1])), "time": kfull.coords["time"].values,
                                         "coil": np.arange(c)})
    want, img = to_image(kfull), to_image(ku)
    out = unfold_sense(img, orc.make_sens(c, big, 1), rs)
    assert out.dims == ("x", "y", "time") and out.shape == (*big, t)
    for d in ("x", "y"):
        assert np.allclose(out.coords[d].values, want.coords[d].values, rtol=1e-14, atol=0) and out.coords[d].dim == d
    assert "ky_label" not in out.coords and "coil" not in out.coords  # its dim changed size / is gone
    assert np.array_equal(out.coords["time"].values, kfull.coords["time"].values)
    # accel 1 along a dim: its coordinates stay as they are, labels included; a single point: step 1
    one = unfold_sense(img, orc.make_sens(c, (big[0], ns[1]), 1), (2, 1))
    assert np.array_equal(one.coords["y"].values, img.coords["y"].values) and "ky_label" in one.coords
    single = LabeledArray(img.values[:, :1], img.dims, {"x": [3.0]})
    assert np.array_equal(unfold_sense(single, orc.make_sens(c, (2, ns[1]), 1), (2, 1)).coords["x"].values, [-1.0, 0.0])


def test_metadata_layouts_and_dataset(numpy_device):
    from xmris_amd import ATTRS, LabeledArray, unfold_sense

    la, sens, rs, dims, _ = labeled_case("5x3_r2x3_c12")
    want = orc.parity_routes("5x3_r2x3_c12")[0]
    out = la.xmr.unfold_sense(sens, rs, regularization=0)
    assert out.attrs == {"note": "kept", ATTRS.sense_dims: ("x", "y"), ATTRS.sense_accel: (2, 3), ATTRS.sense_regularization: 0.0}
    assert la.attrs == {"note": "kept"} and out.name == "csi" and out.dims == ("x", "y", "time")
    # the coil axis between the spatial dims, a repetition axis, time not last, sensitivities in another order
    rep = np.stack([la.values, 2 * la.values, la.values])  # (rep, coil, x, y, time)
    moved = LabeledArray(np.ascontiguousarray(np.transpose(rep, (4, 2, 1, 0, 3))), ("time", "x", "coil", "rep", "y"))
    st = LabeledArray(np.ascontiguousarray(np.transpose(sens.values, (2, 0, 1))), ("y", "coil", "x"))
    ds = unfold_sense(moved, st, (3, 2), dims=("y", "x"), return_maps=True)
    assert ds["unfolded"].dims == ("time", "x", "rep", "y") and ds["g_factor"].dims == ("y", "x") == ds["status"].dims
    assert set(ds.data_vars) == {"unfolded", "g_factor", "status"} and ds.attrs[ATTRS.sense_accel] == (3, 2)
    # the member order follows `dims`, so the numbers differ from the (x, y) call by rounding only
    got = np.transpose(ds["unfolded"].values, (2, 1, 3, 0))  # (rep, x, y, time)
    for i, f in enumerate((1.0, 2.0, 1.0)):
        assert np.all(np.abs(got[i] - f * want["rho"]) <= f * SENSE_TOL * want["unit"])
    assert np.all(np.abs(ds["g_factor"].values.T - want["g"]) <= SENSE_TOL * want["gunit"])
    # status and g over the dims alone: the highest status over the other axes
    bad = rep.copy()
    bad[1, 0, 2, 1, 0] = np.inf
    ds = unfold_sense(LabeledArray(bad, ("rep", "coil", "x", "y", "time")), sens, rs, return_maps=True)
    grp = [q for p, qq in orc.groups((5, 3), rs) if p == (2, 1) for q in qq]
    assert all(ds["status"].values[q] == 2 and np.isnan(ds["g_factor"].values[q]) for q in grp)
    assert (ds["status"].values == 2).sum() == 6 and not ds["unfolded"].values[1][grp[0]].any()
    assert np.array_equal(ds["unfolded"].values[0], ds["unfolded"].values[2]) and ds["unfolded"].values[0][grp[0]].any()


def test_dataarray_bridge(numpy_device, monkeypatch):
    import _fake_xarray

    xr = _fake_xarray.install(monkeypatch)
    import xmris_amd

    xmris_amd.register_xarray_accessor(force=True)
    la, sens, rs, dims, _ = labeled_case("4x5_r2x1_c4")
    da = xr.DataArray(la.values, dims=la.dims, coords={"x": la.coords["x"].values}, attrs={"a": 1}, name="k")
    sx = xr.DataArray(sens.values, dims=sens.dims)
    out = xmris_amd.unfold_sense(da, sx, rs)
    assert type(out) is xr.DataArray and out.dims == ("x", "y", "time") and out.name == "k" and out.attrs["a"] == 1
    assert isinstance(out.values, np.ndarray) and out.shape == (8, 5, 9)
    assert np.array_equal(da.xmr.unfold_sense(sens.values, rs).values, out.values)
    check(out.values, *(orc.parity_routes("4x5_r2x1_c4")[0][k] for k in ("g", "status")), orc.parity_routes("4x5_r2x1_c4")[0])


# ---- validation: every error fires before any native call -----------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    from xmris_amd import _lib
    from xmris_amd import device as dev

    def boom(*a, **k):
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "call", boom)
    for name in ("to_device", "unfold_sense", "coil_combine"):
        monkeypatch.setattr(dev, name, boom)


def _la(shape=(4, 3, 5, 6), dims=("coil", "x", "y", "time")):
    from xmris_amd import LabeledArray

    return LabeledArray(orc.make(shape, 1), dims)


_S = np.ones((4, 6, 10), dtype=complex)


@pytest.mark.parametrize("kw, word", [
    (dict(accel=(2, 2, 2)), "accel"),
    (dict(accel=0), "accel"),
    (dict(accel=(2, -1)), "accel"),
    (dict(accel=2.5), "accel"),
    (dict(accel="two"), "accel"),
    (dict(accel=(4, 8), sensitivities=np.ones((4, 12, 40))), "accel"),  # R = 32
    (dict(sensitivities=np.ones((4, 6, 5))), "sensitivities"),
    (dict(sensitivities=np.ones((3, 6, 10))), "sensitivities"),
    (dict(sensitivities=np.ones((6, 10, 4))), "sensitivities"),
    (dict(regularization=-0.1), "regularization"),
    (dict(regularization=float("nan")), "regularization"),
    (dict(regularization=float("inf")), "regularization"),
    (dict(regularization="much"), "regularization"),
    (dict(noise_cov=np.eye(3)), "noise_cov"),
    (dict(noise_cov=-np.eye(4)), "noise_cov"),
    (dict(noise_cov="head"), "noise_cov"),
    (dict(dims=("x", "coil")), "coil_dim"),
    (dict(dims=("x", "time")), "time_dim"),
    (dict(coil_dim="channel"), "coil_dim"),
    (dict(time_dim="t"), "time_dim"),
    (dict(dims=("x", "x")), "dims"),
    (dict(dims=()), "dims"),
])
def test_validation_errors_name_their_argument(no_library, kw, word):
    from xmris_amd import unfold_sense

    args = dict(sensitivities=_S, accel=2)
    args.update(kw)
    with pytest.raises(ValueError, match=word):
        unfold_sense(_la(), **args)
    with pytest.raises(ValueError, match=word):
        _la().xmr.unfold_sense(**args)


def test_validation_of_dims_and_types(no_library):
    from xmris_amd import LabeledArray, sense_maps, unfold_sense

    with pytest.raises(ValueError, match=r"Method 'unfold_sense' attempted to operate on missing dimension\(s\): \['z'\]"):
        unfold_sense(_la(), _S, 2, dims=("x", "z"))
    with pytest.raises(ValueError, match="dims"):  # more than three
        unfold_sense(_la((2, 2, 2, 2, 2, 3), ("coil", "a", "b", "c", "d", "time")), _S, 1, dims=("a", "b", "c", "d"))
    with pytest.raises(ValueError, match="coil_dim"):  # 65 coils
        unfold_sense(_la((65, 3, 5, 2)), np.ones((65, 6, 10)), 2)
    with pytest.raises(ValueError, match="sensitivities"):  # a labeled array with other dims
        unfold_sense(_la(), LabeledArray(_S, ("coil", "x", "z")), 2)
    with pytest.raises(TypeError):
        unfold_sense(np.zeros((4, 3, 5, 6), complex), _S, 2)
    for kw, word in ((dict(dim="channel"), "dim"), (dict(time_dim="t"), "time_dim"), (dict(threshold=2.0), "threshold"),
                     (dict(noise_cov=np.eye(3)), "noise_cov")):
        with pytest.raises(ValueError, match=word):
            sense_maps(_la(), **kw)


def _abi_call(lib, a):
    i32 = ctypes.c_int32 * 3
    n = None if a["n"] is None else i32(*a["n"])
    r = None if a["accel"] is None else i32(*a["accel"])
    ast = None if a["as"] is None else (ctypes.c_int64 * 5)(*a["as"])
    yst = None if a["ys"] is None else (ctypes.c_int64 * 4)(*a["ys"])
    return lib.xm_sense_unfold(a["a"], a["y"], a["sens"], a["linv"], a["g"], a["st"], a["no"], a["C"], n, r, a["Nt"], ast, yst,
                               a["reg"], a["dtype"], a["ws"], None)


# a (2, 4, 3, 4, 8) -> y (2, 6, 8, 8): two repetitions, 4 coils, 3 x 4 voxels unfolded 2 x 2, 8 points
ABI_OK = {"a": 16, "y": 32, "sens": 48, "linv": None, "g": 64, "st": 80, "no": 2, "C": 4, "n": (1, 3, 4), "accel": (1, 2, 2),
          "Nt": 8, "as": (384, 96, 0, 32, 8), "ys": (384, 0, 64, 8), "reg": 0.0, "dtype": 0, "ws": 96}
ABI_BAD = (dict(a=None), dict(y=None), dict(sens=None), dict(ws=None), dict(n=None), dict(accel=None), {"as": None},
           dict(ys=None), dict(C=0), dict(C=65), dict(accel=(1, 0, 2)), dict(accel=(1, -2, 2)), dict(accel=(2, 3, 3)),
           dict(accel=(1, 1, 17)), dict(n=(1, 0, 4)), dict(n=(0, 3, 4)), dict(Nt=0), dict(reg=-1.0), dict(reg=float("nan")),
           dict(reg=float("inf")), dict(dtype=2), dict(dtype=-1), dict(y=16), dict(no=-1), dict(no=1 << 40, n=(1, 1 << 15, 1 << 15)))


def test_c_abi_refusals_without_gpu():
    from xmris_amd import _lib

    lib = _lib.load()
    for change in ABI_BAD:
        rc = _abi_call(lib, dict(ABI_OK, **change))
        assert rc == _lib.XM_ERR_INVALID_ARG, change
        assert b"sense_unfold" in lib.xm_last_error_string()
    assert _abi_call(lib, dict(ABI_OK, no=0)) == 0  # a zero-sized problem launches nothing, whatever the pointers hold


def test_vocabulary_and_exports():
    import xmris_amd
    from xmris_amd import ATTRS, processing
    from xmris_amd import device as dev

    assert (ATTRS.sense_dims, ATTRS.sense_accel, ATTRS.sense_regularization) == ("sense_dims", "sense_accel", "sense_regularization")
    for name in ("unfold_sense", "sense_maps"):
        assert getattr(xmris_amd, name) is getattr(processing, name) and name in xmris_amd.__all__ and name in processing.__all__
    assert hasattr(xmris_amd.XmrisAccessor, "unfold_sense")
    assert dev.SENSE_MAX_COILS == 64 and dev.SENSE_MAX_ACCEL == 16 and "xm_sense_unfold" in xmris_amd._lib.SIGNATURES
    assert xmris_amd._lib.XM_SENSE_WORKSPACE_BYTES == 256
