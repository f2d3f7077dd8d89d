"""CPU tests of to_image / to_kspace: the oracle's two routes agree within the figure MRSI_TOL is made from, the oracle
has the properties of the definition, the Python layer (both routes, on the numpy stand-in for the
device plus a numpy ``axis_dft``) matches the oracle and keeps dims, coordinates, attrs and names as specified, every
validation error fires before the library is reached, and xm_axis_dft refuses bad arguments without a GPU.

The tests of the oracle alone import nothing from the package and pass without the feature; all others fail without it."""
import os
import re

import numpy as np
import pytest

import _mrsi_oracle as orc

# the largest disagreement of the oracle's two routes (table product against numpy's FFT) over orc.PARITY_CASES, in units
# of the pencil's U (orc.unit) -- tests/tool_mrsi_tolerance.py, recorded in profiles/mrsi/tolerance.txt -- and 16 x that
ROUTE_GAP = 1.850
MRSI_TOL = 29.6


def bound(u, dtype=np.complex128, passes=1):
    """On |result - oracle|: MRSI_TOL U; complex64 adds the roundings the definition itself makes, one per pass:
    passes eps32 U / eps64."""
    b = MRSI_TOL * u
    if np.dtype(dtype) == np.complex64:
        b = b + passes * orc.EPS32 * u / orc.EPS
    return b


# ---- the oracle -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(orc.PARITY_CASES))
def test_routes_agree(name):
    x, axes, matrix, filters, shifts, sign, a, b, u = orc.parity_case(name)
    g = orc.gap(a, b, u)
    print(name, g)
    assert a.shape == b.shape and g <= MRSI_TOL / 16 * 1.01


def test_tolerance_constant_matches_its_tool():
    worst = orc.worst_route_gap()
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "mrsi", "tolerance.txt")).read()
    recorded = float(re.search(r"MRSI_TOL = ([0-9.]+)", text).group(1))
    assert worst == pytest.approx(ROUTE_GAP, rel=0.02), worst
    assert MRSI_TOL == pytest.approx(16 * worst, rel=0.04) and recorded == MRSI_TOL


def test_parity_cases_cover_parities_and_signs():
    nm = set()
    for shape, dims, tdims, matrix, *_ in orc.PARITY_CASES.values():
        ns = [shape[dims.index(d)] for d in tdims]
        ms = ns if matrix is None else ([matrix] * len(ns) if np.ndim(matrix) == 0 else matrix)
        nm |= {(n % 2, m % 2, m > n) for n, m in zip(ns, ms)}
    assert {(0, 0, True), (1, 0, True), (0, 1, True), (1, 1, True), (0, 0, False), (1, 1, False)} <= nm
    assert {c[6] for c in orc.PARITY_CASES.values()} == {1, -1}
    assert {len(c[2]) for c in orc.PARITY_CASES.values()} == {1, 2, 3}


@pytest.mark.parametrize("route", ["table", "fft"])
@pytest.mark.parametrize("n, m", [(7, 16), (8, 8), (6, 9), (5, 5), (12, 33)])
def test_constant_kspace_peaks_at_the_centre(route, n, m):
    y = orc.reconstruct(np.ones((n, 2)), [0], m, route=route)
    assert np.all(np.argmax(np.abs(y), axis=0) == m // 2)
    assert np.allclose(y[m // 2], n / np.sqrt(m), rtol=1e-13)


@pytest.mark.parametrize("route", ["table", "fft"])
def test_integer_shift_is_a_roll(route):
    x = orc.make((7, 6, 3), seed=3)
    plain = orc.reconstruct(x, [0, 1], (16, 9), "hamming", None, route=route)
    moved = orc.reconstruct(x, [0, 1], (16, 9), "hamming", (3, -2), route=route)
    want = np.roll(plain, (3, -2), axis=(0, 1))
    assert np.abs(moved - want).max() <= 64 * orc.unit(x, [0, 1], (16, 9), "hamming").max()
    half = orc.reconstruct(x, [0, 1], (16, 9), "hamming", (0.5, 0.0), route=route)
    assert np.abs(half - plain).max() > 1e-3


@pytest.mark.parametrize("shape", [(7, 6, 3), (8, 5, 2), (1, 4, 2)])
def test_to_kspace_undoes_to_image(shape):
    x = orc.make(shape, seed=4)
    back = orc.reconstruct(orc.reconstruct(x, [0, 1], sign=1), [0, 1], sign=-1)
    assert np.abs(back - x).max() <= 64 * orc.EPS * np.abs(x).max()


def test_seven_to_sixteen_keeps_dc_on_the_centre():
    # a k-space that holds its DC sample (index 7 // 2) alone is a constant image; the pad m // 2 - n // 2 = 5 puts it on
    # 16 // 2 = 8, where the transform's centre is.  The reference's symmetric pad (16 - 7) // 2 = 4 puts it on 7
    k = np.zeros(7)
    k[3] = 1.0
    for route in ("table", "fft"):
        assert np.allclose(orc.reconstruct(k, [0], 16, route=route), 0.25, atol=1e-15)
    off = np.fft.fftshift(np.fft.ifft(np.fft.ifftshift(np.pad(k, (4, 5))), norm="ortho"))
    assert np.abs(off - 0.25).max() > 0.1  # (a phase ramp)
    assert 16 // 2 - 7 // 2 == 5 and all(m // 2 - n // 2 == (m - n) // 2 for n, m in ((8, 16), (7, 9), (6, 9), (8, 11)))


def test_filter_weights():
    for name, alpha in (("hamming", 0.54), ("hann", 0.5)):
        for n in (8, 7, 1):
            w = orc.weights(name, n)
            assert w[n // 2] == 1.0 and np.argmax(w) == n // 2  # centred on the DC sample
            assert np.allclose(w[1:], w[1:][::-1]) if n % 2 == 0 else np.allclose(w, w[::-1])  # symmetric about it
        assert orc.weights(name, 8)[0] == pytest.approx(2 * alpha - 1)  # the edge of an even grid: cos(-pi)
        assert orc.weights(name, 7)[0] == pytest.approx(alpha + (1 - alpha) * np.cos(2 * np.pi * 3 / 7))
    assert np.array_equal(orc.weights(None, 5), np.ones(5))


# ---- the Python layer on the numpy stand-in ----------------------------------------------------------------------------
def np_axis_dft(x, axis, table):
    return orc.apply_table(x, axis, np.asarray(table)).astype(x.dtype)


@pytest.fixture
def numpy_device(monkeypatch):
    import _numpy_device
    from xmris_amd import device as dev

    _numpy_device.install(monkeypatch)
    calls = []

    def axis_dft(x, axis, table):
        calls.append("axis_dft")
        return np_axis_dft(x, axis, table)

    monkeypatch.setattr(dev, "axis_dft", axis_dft)
    for name in ("phase_apply", "zero_fill", "fft"):
        def wrap(*a, _f=getattr(dev, name), _n=name, **k):
            calls.append(_n)
            return _f(*a, **k)

        monkeypatch.setattr(dev, name, wrap)
    return calls


def labeled_case(name, dtype=np.complex128):
    """(LabeledArray, keyword arguments, the function's name, oracle result, unit, passes) of a parity case."""
    from xmris_amd import LabeledArray

    shape, dims, tdims, matrix, _, shifts, sign = orc.PARITY_CASES[name]
    x, axes, matrix, filters, shifts, sign, a, _, u = orc.parity_case(name)
    coords = {d: (np.arange(n) - n // 2) * 0.5 for d, n in zip(dims, shape) if d in tdims}
    coords["time"] = np.arange(shape[dims.index("time")]) * 1e-3
    la = LabeledArray(x.astype(dtype), dims, coords, {"note": "kept"}, "mrsi")
    kw = dict(dim=tdims if len(tdims) > 1 else tdims[0], matrix=matrix, filter=filters, shift=shifts)
    if dtype == np.complex64:  # the oracle on the rounded input
        a = orc.reconstruct(la.values.astype(np.complex128), axes, matrix, filters, shifts, sign)
        u = orc.unit(la.values, axes, matrix, filters)
    return la, kw, "to_image" if sign > 0 else "to_kspace", a, u, len(tdims)


@pytest.mark.parametrize("staged", [False, True])
@pytest.mark.parametrize("name", list(orc.PARITY_CASES))
def test_both_routes_match_the_oracle_on_the_stand_in(numpy_device, name, staged):
    import xmris_amd

    la, kw, fn, want, u, d = labeled_case(name)
    got = getattr(xmris_amd, fn)(la, _staged=staged, **kw)
    g = orc.gap(np.asarray(got.values), want, u)
    print(name, "staged" if staged else "kernel", g, numpy_device)
    assert got.shape == want.shape and g <= MRSI_TOL
    assert ("axis_dft" in numpy_device) != staged and ("fft" in numpy_device) == staged
    assert np.array_equal(la.values, orc.parity_case(name)[0])  # the input is untouched


def test_a_matrix_above_64_takes_the_staged_calls(numpy_device):
    from xmris_amd import LabeledArray, to_image

    x = orc.make((6, 5, 4), seed=11)
    la = LabeledArray(x, ("kx", "ky", "time"), {"kx": np.arange(6.0), "ky": np.arange(5.0)})
    got = to_image(la, matrix=(96, 5), filter="hamming", shift=(0.5, 0.0))
    assert numpy_device == ["phase_apply", "zero_fill", "fft", "axis_dft"]  # kx staged, ky the kernel
    want = orc.reconstruct(x, [0, 1], (96, 5), "hamming", (0.5, 0.0))
    assert orc.gap(got.values, want, orc.unit(x, [0, 1], (96, 5), "hamming")) <= MRSI_TOL
    del numpy_device[:]
    to_image(la, dim="ky", out_dim="y")  # no filter, shift or zero fill: the staged route is the transform alone
    to_image(la, dim="ky", out_dim="y", _staged=True)
    assert numpy_device == ["axis_dft", "fft"]


def test_metadata(numpy_device):
    from xmris_amd import ATTRS, LabeledArray, to_image, to_kspace

    x = orc.make((3, 7, 12, 5), seed=12)
    coords = {"kx": (np.arange(7) - 3) * 0.25, "ky": (np.arange(12) - 6) * 0.5, "time": np.arange(5) * 1e-3,
              "coil": np.arange(3), "ky_label": ("ky", np.arange(12) * 10.0, {"units": "a.u."}), "kx_label": ("kx", np.arange(7))}
    la = LabeledArray(x, ("coil", "kx", "ky", "time"), coords, {"note": "kept"}, "csi")
    img = to_image(la, matrix=(16, 12), filter="hamming", shift=(0.25, -1.5))
    assert img.dims == ("coil", "x", "y", "time") and img.shape == (3, 16, 12, 5) and img.name == "csi"
    assert np.allclose(img.coords["x"].values, np.roll(np.fft.fftfreq(16, d=0.25), 8))
    assert np.allclose(img.coords["y"].values, np.roll(np.fft.fftfreq(12, d=0.5), 6))
    assert img.coords["x"].attrs == {} and img.coords["x"].dim == "x" and "kx" not in img.coords and "ky" not in img.coords
    assert "kx_label" not in img.coords  # its dim changed size
    assert img.coords["ky_label"].dim == "y" and np.array_equal(img.coords["ky_label"].values, np.arange(12) * 10.0)
    assert img.coords["ky_label"].attrs == {"units": "a.u."}
    assert np.array_equal(img.coords["time"].values, coords["time"]) and np.array_equal(img.coords["coil"].values, np.arange(3))
    assert img.attrs == {"note": "kept", ATTRS.mrsi_dims: ("kx", "ky"), ATTRS.mrsi_matrix: (16, 12),
                         ATTRS.mrsi_filter: "hamming", ATTRS.mrsi_shift: (0.25, -1.5)}
    assert la.attrs == {"note": "kept"} and la.dims == ("coil", "kx", "ky", "time")
    # the accessor, the defaults of to_kspace, a single point, explicit names
    back = img.xmr.to_kspace()
    assert back.dims == ("coil", "kx", "ky", "time") and back.attrs[ATTRS.mrsi_filter] == "none"
    assert back.attrs[ATTRS.mrsi_shift] == (0.0, 0.0) and back.attrs[ATTRS.mrsi_matrix] == (16, 12)
    one = LabeledArray(x[:, :1], ("coil", "kx", "ky", "time"), {"kx": [2.0], "ky": coords["ky"]})
    assert np.allclose(to_image(one, dim="kx", matrix=4).coords["x"].values, np.roll(np.fft.fftfreq(4, d=1.0), 2))
    named = la.xmr.to_image(dim=("coil", "ky"), out_dim=("channel", "row"), filter=[None, orc.custom_filter(12)])
    assert named.dims == ("channel", "kx", "row", "time") and named.attrs[ATTRS.mrsi_filter] == "custom"
    # real input is taken as complex
    real = LabeledArray(x.real.copy(), la.dims, coords)
    assert np.iscomplexobj(to_image(real).values)
    assert orc.gap(to_image(real).values, orc.reconstruct(x.real, [1, 2]), orc.unit(x.real, [1, 2])) <= MRSI_TOL


def test_dataarray_bridge(numpy_device, monkeypatch):
    import _fake_xarray

    xr = _fake_xarray.install(monkeypatch)
    import xmris_amd

    xmris_amd.register_xarray_accessor(force=True)
    x = orc.make((6, 5, 4), seed=13)
    da = xr.DataArray(x, dims=("kx", "ky", "time"), coords={"kx": np.arange(6.0), "ky": np.arange(5.0)}, attrs={"a": 1}, name="k")
    out = xmris_amd.to_image(da, matrix=8, filter="hann")
    assert type(out) is xr.DataArray and out.dims == ("x", "y", "time") and out.name == "k" and out.attrs["a"] == 1
    assert isinstance(out.values, np.ndarray) and out.shape == (8, 8, 4)
    assert orc.gap(out.values, orc.reconstruct(x, [0, 1], 8, "hann"), orc.unit(x, [0, 1], 8, "hann")) <= MRSI_TOL
    assert np.array_equal(da.xmr.to_image(matrix=8, filter="hann").values, out.values)


# ---- validation: every error fires before any native call -----------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    from xmris_amd import _lib
    from xmris_amd import device as dev

    def boom(*a, **k):
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "call", boom)
    for name in ("to_device", "axis_dft", "phase_apply", "zero_fill", "fft"):
        monkeypatch.setattr(dev, name, boom)


def _la(shape=(6, 7, 5, 4), dims=("kx", "ky", "kz", "time")):
    from xmris_amd import LabeledArray

    return LabeledArray(orc.make(shape, seed=1), dims, {d: np.arange(float(n)) for d, n in zip(dims, shape)})


@pytest.mark.parametrize("kw, word", [
    (dict(dim=()), "dim"),
    (dict(dim=("kx", "kx")), "dim"),
    (dict(dim=("kx", "time")), "out_dim"),  # no default name for time
    (dict(out_dim="x"), "out_dim"),  # one name for two dims
    (dict(out_dim=("x", "x")), "out_dim"),
    (dict(out_dim=("x", "time")), "out_dim"),  # the name of another dim
    (dict(matrix=5), "matrix"),  # smaller than kx
    (dict(matrix=(8, 6)), "matrix"),  # smaller than ky
    (dict(matrix=(8, 8, 8)), "matrix"),
    (dict(matrix=8.5), "matrix"),
    (dict(matrix="big"), "matrix"),
    (dict(filter="gauss"), "filter"),
    (dict(filter=["hamming"]), "filter"),  # one entry for two dims
    (dict(filter=[np.ones(5), None]), "filter"),  # wrong length
    (dict(filter=[np.ones(6) * 1j, None]), "filter"),  # not real
    (dict(filter=[np.ones((6, 1)), None]), "filter"),
    (dict(filter=["hamming", "gauss"]), "filter"),
    (dict(filter=3), "filter"),
    (dict(shift=(1.0,)), "shift"),
    (dict(shift=(1.0, float("nan"))), "shift"),
    (dict(shift="left"), "shift"),
])
def test_validation_errors_name_their_argument(no_library, kw, word):
    from xmris_amd import to_image

    with pytest.raises(ValueError, match=word):
        to_image(_la(), **kw)
    with pytest.raises(ValueError, match=word):
        _la().xmr.to_image(**kw)


def test_validation_of_dims_and_coordinates(no_library):
    from xmris_amd import LabeledArray, to_image, to_kspace

    with pytest.raises(ValueError, match=r"Method 'to_image' attempted to operate on missing dimension\(s\): \['x'\]"):
        to_image(_la(), dim=("kx", "x"))
    with pytest.raises(ValueError, match=r"Method 'to_kspace' attempted to operate on missing dimension\(s\): \['x', 'y'\]"):
        to_kspace(_la())
    with pytest.raises(ValueError, match="dim"):  # more than three
        to_image(_la((2, 2, 2, 2, 3), ("a", "b", "c", "d", "time")), dim=("a", "b", "c", "d"), out_dim=("e", "f", "g", "h"))
    with pytest.raises(KeyError):
        to_image(LabeledArray(orc.make((4, 4, 3), 1), ("kx", "ky", "time"), {"kx": np.arange(4.0)}))
    with pytest.raises(TypeError):
        to_image(np.zeros((4, 4, 3), complex))


def test_c_abi_refusals_without_gpu():
    from xmris_amd import _lib

    lib = _lib.load()
    ok = dict(x=16, y=32, t=48, no=2, n=7, m=16, ni=3, dtype=0)
    for change in (dict(n=0), dict(n=65), dict(m=65), dict(m=0), dict(x=None), dict(y=None), dict(t=None), dict(y=16),
                   dict(dtype=2), dict(dtype=-1), dict(no=-1), dict(ni=-1), dict(no=1 << 40, ni=1 << 40)):
        a = dict(ok, **change)
        rc = lib.xm_axis_dft(a["x"], a["y"], a["t"], a["no"], a["n"], a["m"], a["ni"], a["dtype"], None)
        assert rc == _lib.XM_ERR_INVALID_ARG, change
        assert b"axis_dft" in lib.xm_last_error_string()
    # a zero-sized problem launches nothing, whatever the pointers hold
    assert lib.xm_axis_dft(16, 32, 48, 0, 7, 16, 3, 0, None) == 0
    assert lib.xm_axis_dft(16, 32, 48, 2, 7, 16, 0, 1, None) == 0


def test_vocabulary_and_exports():
    import xmris_amd
    from xmris_amd import ATTRS, processing
    from xmris_amd import device as dev

    assert (ATTRS.mrsi_dims, ATTRS.mrsi_matrix, ATTRS.mrsi_filter, ATTRS.mrsi_shift) == ("mrsi_dims", "mrsi_matrix", "mrsi_filter", "mrsi_shift")
    for name in ("to_image", "to_kspace"):
        assert getattr(xmris_amd, name) is getattr(processing, name) and name in xmris_amd.__all__
        assert name in processing.__all__ and hasattr(xmris_amd.XmrisAccessor, name)
    assert dev.AXIS_DFT_MAX == 64 and "xm_axis_dft" in xmris_amd._lib.SIGNATURES
    from xmris_amd.processing import mrsi

    t = mrsi.axis_table(7, 16, orc.weights("hamming", 7), 0.25, 1.0)
    assert np.abs(t - orc.table(7, 16, "hamming", 0.25, 1)).max() <= 8 * orc.EPS
