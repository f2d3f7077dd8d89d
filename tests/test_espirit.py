"""CPU tests of espirit_maps: the oracle meets the conditions an ESPIRiT calibration has to meet, the
tolerance constants are what their tool recorded, the Python layer (on the numpy stand-in for the device, with
``axis_dft`` as a matrix product and ``espirit_eig`` as ``numpy.linalg.eigh`` followed by the kernel's selection, phase and
crop rules) reproduces the oracle and meets the same conditions, keeps dims, coordinates and attrs as specified, every
validation error names its argument before the library is reached, and xm_espirit_eig refuses bad arguments without a
GPU.

The tests of the oracle alone import nothing from the package; all others fail without the feature."""
import os
import re

import numpy as np
import pytest

import _espirit_oracle as orc
import _mrsi_oracle as mrsi_orc
import _wg_oracle as wg

# tests/tool_espirit_tolerance.py, recorded in profiles/espirit/tolerance.txt: 16 x the largest disagreement of two routes
# to H (an entry), and of Jacobi against eigh (an eigenvalue, a residual relative to ||H||_F, a map component)
ESP_TOL_H = 7.230e-13
ESP_TOL_VALUE = 2.665e-14
ESP_TOL_RESIDUAL = 2.995e-14
ESP_TOL_MAP = 7.290e-14
# the oracle against the truth (same tool): the largest map error inside the object and the error of a SENSE unfolding at
# accel 2 relative to max |object|, maps cropped at 0.9; the package is allowed 2 x these
MAP_ERROR = {"disc2d": 4.856e-02, "rect2d": 7.729e-02, "line1d": 2.524e-02, "box3d": 3.129e-02}
UNFOLD_ERROR = {"disc2d": 6.660e-02, "rect2d": 8.726e-02, "line1d": 2.463e-02, "box3d": 4.246e-02}
PROFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "espirit", "tolerance.txt")
K_DIMS = ("kx", "ky", "kz")


def value_tol(c):
    """A whole call against the oracle: Jacobi against eigh, and Weyl's bound on what the two routes to H may differ by."""
    return ESP_TOL_VALUE + c * ESP_TOL_H


def map_tol(c):
    """... and the sin-theta bound at the gap of 0.5 that the conditions demand inside the object."""
    return ESP_TOL_MAP + c * ESP_TOL_H / 0.5


def check_conditions(name, f):
    """The conditions an ESPIRiT calibration of a case has to meet, oracle and package alike."""
    print(name, f)
    assert f["left_out"] == 0.0
    assert f["lam1_min"] >= 0.98 and f["gap_min"] >= 0.5
    assert f["map_error"] <= 2 * MAP_ERROR[name] and f["unfold_error"] <= 2 * UNFOLD_ERROR[name]
    assert f["unfold_error"] < 0.1


# ---- the oracle -----------------------------------------------------------------------------------------------------------
def test_tolerance_constants_match_their_tool():
    text = open(PROFILE).read()
    for key, const in (("ESP_TOL_H", ESP_TOL_H), ("ESP_TOL_VALUE", ESP_TOL_VALUE), ("ESP_TOL_RESIDUAL", ESP_TOL_RESIDUAL),
                       ("ESP_TOL_MAP", ESP_TOL_MAP)):
        assert float(re.search(key + r" = ([0-9.e+-]+)", text).group(1)) == const
    for key, const in (("largest H disagreement", ESP_TOL_H), ("largest eigenvalue disagreement", ESP_TOL_VALUE),
                       ("largest residual", ESP_TOL_RESIDUAL), ("largest map disagreement", ESP_TOL_MAP)):
        assert const == pytest.approx(16 * float(re.search(key + r": ([0-9.e+-]+)", text).group(1)), rel=0.01)
    rec = {m.group(1): (float(m.group(2)), float(m.group(3)))
           for m in re.finditer(r"truth (\w+) .* map error ([0-9.e+-]+) unfolding error ([0-9.e+-]+)", text)}
    assert rec == {n: (MAP_ERROR[n], UNFOLD_ERROR[n]) for n in orc.CASES}


@pytest.mark.parametrize("name", list(orc.CASES))
def test_oracle_meets_the_conditions(name):
    c = orc.case(name)
    ref = orc.reference(name, crop=0.0)
    f = orc.figures(c, ref["maps"], ref["values"])
    check_conditions(name, f)
    assert f["map_error"] == pytest.approx(MAP_ERROR[name], rel=0.02) and f["unfold_error"] == pytest.approx(UNFOLD_ERROR[name], rel=0.02)
    assert 0 < ref["n_kernels"] < ref["sigma"].size // 2  # the signal space is a small part of the windows' space
    lam = np.linalg.eigvalsh(ref["H"])
    assert lam.min() >= -1e-12 and lam.max() <= 1 + 1e-12
    # outside the object nothing is promised, and the crop takes voxels away there
    assert np.any(ref["values"][0][~c.mask] < 0.9) or name == "line1d"


def test_oracle_conventions_conjugate_and_sign():
    """Of the four combinations of conjugate and sign in g_j(q) only the specified one finds the maps: the others give
    the conjugate or the mirror image, whose map error is beyond what the package is allowed."""
    c = orc.case("rect2d")
    v, _ = orc.singular_vectors(c.acs, c.kernel, 8, c.threshold)

    def error(conjugate, sign):
        g = np.conj(v) if conjugate else v
        for axis, n in enumerate(c.mat):
            e = np.exp(sign * 2j * np.pi * np.outer(np.arange(n) - n // 2, np.arange(g.shape[1 + axis])) / n)
            g = np.moveaxis(np.tensordot(e, g, axes=([1], [1 + axis])), 0, 1 + axis)
        h = np.einsum("j...c,j...d->...cd", g, np.conj(g)) / int(np.prod(c.kernel))
        maps, _ = orc.select(*np.linalg.eigh(h), 1, 0, 0.0)
        return orc.map_error(c, maps[0])

    errs = {(cj, sg): error(cj, sg) for cj in (True, False) for sg in (1.0, -1.0)}
    print(errs)
    assert errs[(True, 1.0)] <= 2 * MAP_ERROR["rect2d"]
    assert min(errs[k] for k in errs if k != (True, 1.0)) > 2 * MAP_ERROR["rect2d"]


# ---- the Python layer on the numpy stand-in -----------------------------------------------------------------------------
def np_espirit_eig(h, n_coils, n_maps=1, phase_ref=0, crop=0.8):
    """``device.espirit_eig`` by eigh: h [V, E] -> maps [M, C, V], values [M, V], status [V]."""
    from xmris_amd.device import EspiritEig

    h = np.asarray(h)
    full = np.zeros((h.shape[0], n_coils, n_coils), dtype=np.complex128)
    iu, ju = np.triu_indices(n_coils)
    full[:, iu, ju] = h
    lam, vec = np.linalg.eigh(wg.hermitian(full))
    maps, values = orc.select(lam, vec, n_maps, phase_ref, crop)
    return EspiritEig(maps=maps, values=values, status=np.zeros(h.shape[0], np.int32))


@pytest.fixture
def numpy_device(monkeypatch):
    import _numpy_device
    from xmris_amd import device as dev

    _numpy_device.install(monkeypatch)
    calls = []

    def axis_dft(x, axis, table):
        calls.append("axis_dft")
        assert max(np.asarray(table).shape) <= dev.AXIS_DFT_MAX
        return mrsi_orc.apply_table(x, axis, np.asarray(table)).astype(x.dtype)

    def espirit_eig(*a, **k):
        calls.append("espirit_eig")
        return np_espirit_eig(*a, **k)

    monkeypatch.setattr(dev, "axis_dft", axis_dft)
    monkeypatch.setattr(dev, "espirit_eig", espirit_eig)
    for name in ("zero_fill", "fft"):
        def wrap(*a, _f=getattr(dev, name), _n=name, **k):
            calls.append(_n)
            return _f(*a, **k)

        monkeypatch.setattr(dev, name, wrap)
    return calls


def labeled_acs(c, **coords):
    from xmris_amd import LabeledArray

    return LabeledArray(np.array(c.acs), ("coil",) + K_DIMS[:c.d] + ("time",), coords, {"note": "kept"}, "acs")


def run(c, **kw):
    from xmris_amd import espirit_maps

    kw = dict(dict(kernel=c.kernel, dims=K_DIMS[:c.d], threshold=c.threshold), **kw)
    return espirit_maps(labeled_acs(c), c.mat, **kw)


def compare_with_oracle(c, ds, ref):
    """Eigenvalues everywhere, the first map on the object: a dataset of a two-map run against the oracle's."""
    lam, maps = np.asarray(ds["eigenvalues"].values), np.asarray(ds["maps"].values)
    dv = float(np.abs(lam - ref["values"]).max())
    dm = float(np.abs(maps[0] - ref["maps"][0])[:, c.mask].max())
    print(c.name, "values", dv, "of", value_tol(c.C), "map", dm, "of", map_tol(c.C))
    assert dv <= value_tol(c.C) and dm <= map_tol(c.C)
    # the second map: lambda_2 and lambda_3 may coincide, so by its residual against the oracle's H
    h = ref["H"].reshape(-1, c.C, c.C)
    x = np.moveaxis(maps[1].reshape(c.C, -1), 0, -1)
    res = np.linalg.norm(np.einsum("vcd,vd->vc", h, x) - lam[1].reshape(-1, 1) * x, axis=-1)
    fro = np.sqrt((np.abs(h) ** 2).sum(axis=(1, 2)))
    assert float((res / fro).max()) <= ESP_TOL_RESIDUAL + c.C * ESP_TOL_H
    return dv, dm


@pytest.mark.parametrize("name", list(orc.CASES))
def test_python_layer_reproduces_the_oracle_on_the_stand_in(numpy_device, name):
    c = orc.case(name)
    ds = run(c, crop=0.0, n_maps=2, return_eigenvalues=True)
    ref = orc.reference(name, crop=0.0)
    compare_with_oracle(c, ds, ref)
    assert ds.attrs["n_kernels"] == ref["n_kernels"] and np.allclose(ds.attrs["singular_values"], ref["sigma"], rtol=1e-6, atol=1e-9)
    assert numpy_device == ["axis_dft"] * c.d + ["espirit_eig"]
    check_conditions(name, orc.figures(c, np.asarray(ds["maps"].values), np.asarray(ds["eigenvalues"].values)))
    # one map, the default crop: what the two-map run gives, cropped
    one = run(c)
    want = np.where((ref["values"][0] < 0.8)[None], 0.0, np.asarray(ds["maps"].values)[0])
    assert one.dims == ("coil",) + ("x", "y", "z")[:c.d] and np.array_equal(one.values, want)


def test_staged_route_above_the_table_limit(numpy_device):
    c = orc.case("line1d")
    from xmris_amd import espirit_maps

    ds = espirit_maps(labeled_acs(c), 72, kernel=c.kernel, dims="kx", threshold=c.threshold, crop=0.0, n_maps=2,
                      return_eigenvalues=True)
    assert numpy_device == ["zero_fill", "fft", "espirit_eig"]
    want = orc.espirit(c.acs, (72,), c.kernel, threshold=c.threshold, crop=0.0, n_maps=2)
    assert float(np.abs(np.asarray(ds["eigenvalues"].values) - want["values"]).max()) <= value_tol(c.C)
    big = want["values"][0] - want["values"][1] >= 0.5
    assert big.sum() > 36 and float(np.abs(np.asarray(ds["maps"].values)[0] - want["maps"][0])[:, big].max()) <= map_tol(c.C)


def test_whitening_round_trip(numpy_device):
    """A block mixed by L with noise_cov = L L^H is whitened back to the block itself: the maps are L times its maps."""
    c = orc.case("rect2d")
    rng = np.random.default_rng(5)
    m = rng.standard_normal((c.C, c.C)) + 1j * rng.standard_normal((c.C, c.C))
    psi = m @ m.conj().T + c.C * np.eye(c.C)
    chol = np.linalg.cholesky(psi)
    from xmris_amd import espirit_maps

    kw = dict(kernel=c.kernel, threshold=c.threshold, crop=0.9)
    plain = espirit_maps(c.acs, c.mat, **kw)
    mixed = espirit_maps(np.einsum("cd,d...->c...", chol, c.acs), c.mat, noise_cov=psi, **kw)
    want = np.einsum("cd,d...->c...", chol, plain.values)
    assert plain.dims == ("coil", "x", "y") and np.abs(want).max() > 1
    assert float(np.abs(mixed.values - want).max()) <= 1e-10 * np.abs(want).max()
    assert np.array_equal(np.any(mixed.values != 0, axis=0), np.any(plain.values != 0, axis=0))


def test_metadata_and_dataset_layout(numpy_device):
    from xmris_amd import LabeledArray
    from xmris_amd.fitting.dataset import LabeledDataset

    c = orc.case("rect2d")
    dk = 1.0 / 0.2
    coords = dict(coil=np.arange(c.C) + 10, kx=(np.arange(12) - 6) * dk, ky=(np.arange(10) - 5) * dk, time=np.arange(2) * 1e-3)
    la = labeled_acs(c, **coords)
    moved = LabeledArray(np.ascontiguousarray(np.transpose(c.acs, (3, 2, 0, 1))), ("time", "ky", "coil", "kx"), coords, {}, "acs")
    ds = la.xmr.espirit_maps(c.mat, kernel=c.kernel, threshold=c.threshold, crop=0.9, n_maps=2, return_eigenvalues=True)
    assert isinstance(ds, LabeledDataset) and set(ds.data_vars) == {"maps", "eigenvalues", "status"}
    maps = ds["maps"]
    assert maps.dims == ("map", "coil", "x", "y") and maps.shape == (2, c.C, 24, 20) and maps.values.dtype == np.complex128
    assert ds["eigenvalues"].dims == ("map", "x", "y") and ds["eigenvalues"].values.dtype == np.float64
    assert ds["status"].dims == ("x", "y") and ds["status"].values.dtype == np.int32 and not ds["status"].values.any()
    assert np.array_equal(maps.coords["coil"].values, coords["coil"])
    assert np.allclose(maps.coords["x"].values, np.roll(np.fft.fftfreq(24, d=dk), 12))
    assert np.allclose(maps.coords["y"].values, np.roll(np.fft.fftfreq(20, d=dk), 10))
    assert "time" not in maps.coords and "kx" not in maps.coords and set(ds["status"].coords) == {"x", "y"}
    assert set(ds.attrs) == {"n_kernels", "singular_values", "threshold", "crop", "kernel"}
    assert ds.attrs["kernel"] == (4, 3) and ds.attrs["threshold"] == 0.03 and ds.attrs["crop"] == 0.9
    assert ds.attrs["singular_values"].shape == (60,) and np.all(np.diff(ds.attrs["singular_values"]) <= 0)
    assert la.attrs == {"note": "kept"} and la.dims == ("coil", "kx", "ky", "time")
    lam = ds["eigenvalues"].values
    assert np.all(lam[0] >= lam[1]) and np.all(maps.values[0][:, lam[0] < 0.9] == 0) and np.all(maps.values[1][:, lam[1] < 0.9] == 0)
    kept = lam[0] >= 0.9
    assert np.allclose((np.abs(maps.values[0]) ** 2).sum(axis=0)[kept], 1.0, atol=1e-12)
    assert np.all(maps.values[0][0].imag == 0) and np.all(maps.values[0][0].real >= 0)
    # any dim order gives the same maps; the default kernel is min(6, the block); phase_ref picks the real coil
    again = moved.xmr.espirit_maps(c.mat, kernel=c.kernel, threshold=c.threshold, crop=0.9, n_maps=2)
    assert again.dims == maps.dims and np.array_equal(again.values, maps.values)
    default = la.xmr.espirit_maps(c.mat, return_eigenvalues=True)
    assert default.attrs["kernel"] == (6, 6) and default["maps"].dims == ("coil", "x", "y")
    turned = la.xmr.espirit_maps(c.mat, kernel=c.kernel, threshold=c.threshold, crop=0.9, phase_ref=2)
    assert np.all(turned.values[2].imag == 0) and np.allclose(np.abs(turned.values), np.abs(maps.values[0]), atol=1e-12)
    # a time axis is optional, and acs_points limits the rows
    first = la.xmr.espirit_maps(c.mat, kernel=c.kernel, acs_points=1, return_eigenvalues=True)
    flat = LabeledArray(np.array(c.acs[..., 0]), ("coil", "kx", "ky"), {}, {}, None)
    assert np.array_equal(flat.xmr.espirit_maps(c.mat, kernel=c.kernel).values, first["maps"].values)


def test_dataarray_bridge(numpy_device, monkeypatch):
    import _fake_xarray

    xr = _fake_xarray.install(monkeypatch)
    import xmris_amd

    xmris_amd.register_xarray_accessor(force=True)
    c = orc.case("line1d")
    da = xr.DataArray(np.array(c.acs), dims=("coil", "kx", "time"), coords={"coil": np.arange(3)}, name="k")
    out = xmris_amd.espirit_maps(da, c.mat, dims="kx")
    assert type(out) is xr.DataArray and out.dims == ("coil", "x") and out.name == "k"
    assert np.array_equal(da.xmr.espirit_maps(c.mat, dims="kx").values, out.values)
    # the maps feed unfold_sense's argument check as they are
    from xmris_amd.processing.sense import _sens_values

    assert _sens_values(xmris_amd.espirit_maps(labeled_acs(c), c.mat, dims="kx"), "coil", ("x",), 3, [30]).shape == (3, 30)


# ---- validation: every error fires before any native call -----------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    from xmris_amd import _lib
    from xmris_amd import device as dev

    def boom(*a, **k):
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "call", boom)
    for name in ("to_device", "axis_dft", "zero_fill", "fft", "espirit_eig"):
        monkeypatch.setattr(dev, name, boom)


ACS = orc.case("rect2d").acs  # [5, 12, 10, 2]


def _with(index, value):
    a = np.array(ACS)
    a[index] = value
    return a


@pytest.mark.parametrize("kw, word", [
    (dict(kernel=(13, 3)), "kernel"),  # larger than the block
    (dict(kernel=(4, 11)), "kernel"),
    (dict(kernel=0), "kernel"),
    (dict(kernel=(4, 3, 2)), "kernel"),
    (dict(kernel=2.5), "kernel"),
    (dict(matrix=(24, 4), kernel=(4, 3)), "matrix"),  # 2 b - 1 = 5 > 4
    (dict(matrix=(6, 20), kernel=(4, 3)), "matrix"),
    (dict(matrix=(24, 20, 8)), "matrix"),
    (dict(matrix=None), "matrix"),
    (dict(matrix=0), "matrix"),
    (dict(acs=np.ones((64, 12, 10)), kernel=(9, 9)), "kernel"),  # K = 5184 > 4096
    (dict(acs=np.ones((8, 200, 200, 8)), kernel=(6, 6)), "acs_points"),  # more than 2^26 entries
    (dict(acs=np.zeros((5, 12, 10, 2))), "acs"),
    (dict(acs=_with((2, 3, 4, 1), np.nan)), "acs"),
    (dict(acs=_with((0, 0, 0, 0), np.inf)), "acs"),
    (dict(acs=np.ones((65, 12, 10))), "acs"),
    (dict(acs=np.ones((12, 10))), "acs"),
    (dict(acs_points=0), "acs_points"),
    (dict(acs_points=1.5), "acs_points"),
    (dict(threshold=-0.1), "threshold"),
    (dict(threshold=1.5), "threshold"),
    (dict(threshold="low"), "threshold"),
    (dict(crop=float("nan")), "crop"),
    (dict(crop=2.0), "crop"),
    (dict(n_maps=0), "n_maps"),
    (dict(n_maps=3), "n_maps"),
    (dict(n_maps=True), "n_maps"),
    (dict(acs=np.ones((1, 12, 10)), n_maps=2), "n_maps"),
    (dict(phase_ref=5), "phase_ref"),
    (dict(phase_ref=-1), "phase_ref"),
    (dict(phase_ref=1.0), "phase_ref"),
    (dict(noise_cov=np.eye(4)), "noise_cov"),
    (dict(noise_cov=-np.eye(5)), "noise_cov"),
    (dict(noise_cov="tail"), "noise_cov"),
    (dict(dims=("kx", "kx")), "dims"),
    (dict(dims=("kx", "sample")), "dims"),
    (dict(dims=("kx", "coil")), "coil_dim"),
    (dict(coil_dim="time"), "coil_dim"),
])
def test_validation_errors_name_their_argument(no_library, kw, word):
    from xmris_amd import espirit_maps

    args = dict(dict(acs=np.array(ACS), matrix=(24, 20)), **kw)
    with pytest.raises(ValueError, match=word):
        espirit_maps(**args)


def test_validation_of_labeled_dims(no_library):
    from xmris_amd import LabeledArray

    la = LabeledArray(np.array(ACS), ("coil", "kx", "ky", "time"), {}, {}, None)
    with pytest.raises(ValueError, match="acs: dims"):
        la.xmr.espirit_maps((24, 20), dims=("kx", "kz"))
    with pytest.raises(ValueError, match="acs: dims"):
        la.xmr.espirit_maps((24, 20), coil_dim="channel")


# ---- the C ABI ----------------------------------------------------------------------------------------------------------
def test_c_abi_refusals_without_gpu():
    import ctypes

    from xmris_amd import _lib

    lib = _lib.load()

    def call(a):
        return lib.xm_espirit_eig(*[ctypes.c_double(a[k]) if k == "crop" else a[k] for k in orc.EIG_ORDER], None)

    for change in orc.EIG_REFUSALS:
        rc = call(dict(orc.EIG_OK, **change))
        assert rc == _lib.XM_ERR_INVALID_ARG, change
        assert b"espirit_eig" in lib.xm_last_error_string()


def test_vocabulary_and_exports():
    import xmris_amd
    from xmris_amd import processing
    from xmris_amd.processing import espirit

    assert xmris_amd.espirit_maps is processing.espirit_maps is espirit.espirit_maps
    assert "espirit_maps" in xmris_amd.__all__ and "espirit_maps" in processing.__all__
    assert hasattr(xmris_amd.XmrisAccessor, "espirit_maps")
    assert "xm_espirit_eig" in xmris_amd._lib.SIGNATURES
    assert xmris_amd.device.ESPIRIT_MAX_COILS == 64 and xmris_amd.device.espirit_entries(5) == 15
    assert espirit.MAP_DIM == "map" and espirit.MAX_TERMS == 4096 and espirit.MAX_SYSTEM == 1 << 26
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "xmris_hip.h")).read()
    assert "int xm_espirit_eig(" in header
