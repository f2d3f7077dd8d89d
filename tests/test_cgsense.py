"""CPU tests of recon_cg_sense: the oracle converges to the direct solve and its closed-form lambda
is the mean diagonal of the normal matrix, the tolerance constants are what their tool recorded, the Python layer (on the
numpy stand-in for the device, with numpy versions of ``axis_sparse``, ``axis_dft`` and ``cg_sense``) reproduces the oracle
and keeps dims, coordinates, attrs and names as specified, every validation error fires before the library is reached, and
the xm_cgs_* entry points refuse bad arguments without a GPU.

The tests of the oracle alone import nothing from the package; all others fail without the feature."""
import os
import re

import numpy as np
import pytest

import _cgsense_oracle as orc
import _grid_oracle as grid_orc
import _mrsi_oracle as mrsi_orc

# tests/tool_cgsense_tolerance.py, recorded in profiles/cgsense/tolerance.txt: the largest disagreement of two routes of
# the oracle after 6 iterations relative to max |x| and 16 x that, in complex128 (dense against stage-by-stage CSR) and
# with every coil-sized intermediate rounded to complex64
ROUTE_GAP128, CGS_TOL128 = 1.221e-15, 1.954e-14
ROUTE_GAP64, CGS_TOL64 = 1.291e-07, 2.066e-06
# the oracle's distance to the direct solve after 30 iterations (same tool); the GPU test allows 4 x these
DISTANCE30 = {"radial2d": 4.507e-06, "masked2d": 1.608e-08, "random3d": 8.922e-12, "line1d": 7.384e-16, "long1d": 9.884e-14,
              "odd2d": 6.754e-14}
# fully sampled Cartesian 8 x 8, one coil, s = 1, regularization 0, pipe density, 10 iterations: the normal matrix is
# mu I to the accuracy of the gridding kernel (mu = sum_j w_j / V), so mu x is nufft_adjoint of the data.  The largest
# |mu x - nufft_adjoint| / max |nufft_adjoint| per kernel width W, measured with the dense oracle; the tests allow 2 x
FULL_SAMPLING = {4: 5.931e-03, 6: 2.355e-05}
PROFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "cgsense", "tolerance.txt")


# ---- the oracle -----------------------------------------------------------------------------------------------------------
def test_tolerance_constants_match_their_tool():
    text = open(PROFILE).read()
    assert float(re.search(r"CGS_TOL128 = ([0-9.e+-]+)", text).group(1)) == CGS_TOL128
    assert float(re.search(r"CGS_TOL64 = ([0-9.e+-]+)", text).group(1)) == CGS_TOL64
    assert float(re.search(r"largest route disagreement: ([0-9.e+-]+)", text).group(1)) == ROUTE_GAP128
    assert float(re.search(r"largest complex64 rounding gap: ([0-9.e+-]+)", text).group(1)) == ROUTE_GAP64
    assert CGS_TOL128 == pytest.approx(16 * ROUTE_GAP128, rel=0.01) and CGS_TOL64 == pytest.approx(16 * ROUTE_GAP64, rel=0.01)
    recorded = {m.group(1): float(m.group(2)) for m in re.finditer(r"convergence (\w+) .* 30 iterations ([0-9.e+-]+)", text)}
    assert recorded == DISTANCE30
    c = orc.case("radial2d")  # the case that sets CGS_TOL64, recomputed
    y64 = orc.c64(c.y)
    gap = orc.rel(orc.cg(c.staged(rnd=orc.c64), c.rhs(y64, rnd=orc.c64), 6)[0], orc.cg(c.staged(), c.rhs(y64), 6)[0])
    assert gap == pytest.approx(ROUTE_GAP64, rel=0.02)


@pytest.mark.parametrize("name", ["radial2d", "masked2d", "random3d", "odd2d"])
def test_oracle_converges_to_the_direct_solve(name):
    c = orc.case(name)
    b = c.rhs()
    x, residual, n_iter, status = orc.cg(c.dense(), b, 30)
    d = orc.rel(x, c.solve(b))
    print(name, d, residual)
    assert d == pytest.approx(DISTANCE30[name], rel=0.05) and d <= 1e-5 and np.all(n_iter == 30) and np.all(status == 0)
    assert orc.rel(orc.cg(c.dense(), b, 6)[0], c.solve(b)) > 100 * d  # 6 iterations are not yet there: 30 did the work
    if name == "masked2d":
        dead = (np.abs(c.sv) ** 2).sum(axis=0) == 0
        assert dead.sum() > 8 and np.all(x[dead] == 0)


def test_oracle_freezes_a_column_that_has_converged_exactly():
    """line1d has 8 unknowns: conjugate gradients are exact after 8 steps, and without the floor of 1e-14 the next step
    would divide vanishing numbers."""
    c = orc.case("line1d")
    x, residual, n_iter, status = orc.cg(c.dense(), c.rhs(), 20)
    assert np.all(status == 1) and np.all(n_iter <= 9) and np.all(np.isfinite(x)) and np.all(residual <= orc.FLOOR)
    # a zero column converges at once, a column that is not finite is refused; neither touches its neighbours
    b = c.rhs().copy()
    b[:, 1] = 0
    x0, _, n0, s0 = orc.cg(c.dense(), b, 20)
    assert np.all(x0[:, 1] == 0) and n0[1] == 0 and s0[1] == 1 and np.array_equal(x0[:, 0], x[:, 0])
    b[3, 1] = np.nan
    xn, rn, nn, sn = orc.cg(c.dense(), b, 20)
    assert sn[1] == 3 and np.all(np.isnan(xn[:, 1])) and np.array_equal(xn[:, 2], x[:, 2])


@pytest.mark.parametrize("name", ["radial2d", "random3d", "line1d"])
def test_closed_form_lambda_is_the_mean_diagonal(name):
    c = orc.case(name)
    print(name, c.scale(), c.mean_diagonal())
    assert c.lam == pytest.approx(c.reg * c.mean_diagonal(), rel=1e-3)
    assert c.scale() == pytest.approx({"radial2d": 0.3742, "random3d": 0.3063, "line1d": 1.5}[name], rel=2e-4)


# ---- the Python layer on the numpy stand-in -----------------------------------------------------------------------------
def np_axis_sparse(x, axis, table):
    xm = np.moveaxis(np.asarray(x, dtype=np.complex128), axis, 0)
    y = np.zeros((table.n_rows,) + xm.shape[1:], dtype=np.complex128)
    rows = np.repeat(np.arange(table.n_rows), np.diff(table.rowptr))
    np.add.at(y, rows, table.val.reshape((-1,) + (1,) * (xm.ndim - 1)) * xm[table.col])
    return np.ascontiguousarray(np.moveaxis(y, 0, axis)).astype(x.dtype)


def np_cg_sense(y, s, adjoint, forward, lam, iterations, tol):
    """The loop of ``device.cg_sense`` on the oracle's recurrences and the package's own two chains."""
    from xmris_amd.device import CgSense

    c, v = s.shape
    b = orc.reduce_coils(s, adjoint(y).reshape(c, v, -1).astype(np.complex128))

    def op(p):
        u = (s[:, :, None] * p[None, :, :]).astype(y.dtype)
        return orc.reduce_coils(s, adjoint(forward(u)).reshape(c, v, -1).astype(np.complex128)) + lam * p

    x, residual, n_iter, status = orc.cg(op, b, iterations, tol)
    return CgSense(x=x, residual=residual, iterations=n_iter, status=status)


@pytest.fixture
def numpy_device(monkeypatch):
    import _numpy_device
    from xmris_amd import device as dev

    _numpy_device.install(monkeypatch)
    calls = []

    def axis_sparse(x, axis, table):
        calls.append("axis_sparse")
        return np_axis_sparse(x, axis, table)

    def axis_dft(x, axis, table):
        calls.append("axis_dft")
        return mrsi_orc.apply_table(x, axis, np.asarray(table)).astype(x.dtype)

    def cg_sense(*a):
        calls.append("cg_sense")
        return np_cg_sense(*a)

    monkeypatch.setattr(dev, "axis_sparse", axis_sparse)
    monkeypatch.setattr(dev, "axis_dft", axis_dft)
    monkeypatch.setattr(dev, "cg_sense", cg_sense)
    for name in ("phase_apply", "zero_fill", "fft"):
        def wrap(*a, _f=getattr(dev, name), _n=name, **k):
            calls.append(_n)
            return _f(*a, **k)

        monkeypatch.setattr(dev, name, wrap)
    return calls


def labeled(x, dims, **coords):
    from xmris_amd import LabeledArray

    return LabeledArray(x, dims, coords, {"note": "kept"}, "fid")


def recon(c, iterations=6, tol=0.0, **kw):
    from xmris_amd import recon_cg_sense

    kw = dict(dict(regularization=c.reg, density=c.density, width=c.W), **kw)
    return recon_cg_sense(labeled(c.y, ("coil", "sample", "time")), c.traj, c.s, iterations=iterations, tol=tol, **kw)


@pytest.mark.parametrize("name", list(orc.CASES))
def test_python_layer_reproduces_the_oracle_on_the_stand_in(numpy_device, name):
    """The operator the package assembles from its tables (grid_table, the image tables, lambda) is the oracle's: 6
    iterations agree to rounding.  long1d: the staged transform (fft, phase_apply, zero_fill) stands in for the table."""
    c = orc.case(name)
    img = recon(c)
    want = orc.cg(c.dense(), c.rhs(), 6)[0].reshape(c.ms + (c.T,))
    print(name, orc.rel(img.values, want))
    assert img.dims == ("x", "y", "z")[:len(c.ms)] + ("time",) and img.values.dtype == np.complex128
    assert orc.rel(img.values, want) <= 1e-12
    assert ("fft" in numpy_device) == (name == "long1d")


def test_chunks_whitening_and_layouts_on_the_stand_in(numpy_device):
    from xmris_amd import recon_cg_sense

    c = orc.case("radial2d", 5)
    whole = recon(c).values
    assert np.array_equal(recon(c, chunk=2).values, whole) and numpy_device.count("cg_sense") == 1 + 3
    # coil and sample anywhere: one permuting copy, the image dims in place of the sample dim
    moved = labeled(np.ascontiguousarray(np.transpose(c.y, (2, 1, 0))), ("time", "sample", "coil"))
    img = recon_cg_sense(moved, c.traj, c.s, iterations=6, tol=0.0, regularization=c.reg, density="pipe")
    assert img.dims == ("time", "x", "y") and np.array_equal(np.moveaxis(img.values, 0, -1), whole)
    # whitening: data and maps through L^-1; with Psi = a^2 I the solution is unchanged (lambda scales with the maps)
    psi = 4.0 * np.eye(c.C)
    assert orc.rel(recon(c, noise_cov=psi).values, whole) <= 1e-12
    # a general Psi solves the whitened system
    rng = np.random.default_rng(3)
    m = rng.standard_normal((c.C, c.C)) + 1j * rng.standard_normal((c.C, c.C))
    psi = m @ m.conj().T + c.C * np.eye(c.C)
    li = np.linalg.inv(np.linalg.cholesky(psi))
    got = recon(c, noise_cov=psi, iterations=30).values
    sw, yw = np.einsum("cd,dv->cv", li, c.sv), np.einsum("cd,dst->cst", li, c.y)
    G = c.N.conj().T @ (c.w[:, None] * c.N)
    M = sum(np.conj(sw[k])[:, None] * G * sw[k][None, :] for k in range(c.C))
    e = (np.abs(sw) ** 2).sum(axis=0)
    lam = c.reg * c.w.sum() / c.V * e.mean()
    b = sum(np.conj(sw[k])[:, None] * (c.N.conj().T @ (c.w[:, None] * yw[k])) for k in range(c.C))
    want = np.linalg.solve(M + lam * np.eye(c.V), b).reshape(8, 8, 5)
    assert orc.rel(got, want) <= 1e-4


def full_sampling_case(W):
    """(data [1, 64, 3], trajectory, maps, mu) of the FULL_SAMPLING figures."""
    traj = grid_orc.cartesian(8, 2)
    y = grid_orc.make((64, 3), seed=7)[None]
    return y, traj, np.ones((1, 8, 8), dtype=np.complex128), float(grid_orc.pipe(traj, 8, 2.0, W).sum() / 64)


@pytest.mark.parametrize("W", [4, 6])
def test_full_sampling_approaches_nufft_adjoint(numpy_device, W):
    from xmris_amd import nufft_adjoint, recon_cg_sense

    y, traj, sens, mu = full_sampling_case(W)
    la = labeled(y, ("coil", "sample", "time"))
    x = recon_cg_sense(la, traj, sens, iterations=10, tol=0.0, density="pipe", width=W).values
    adj = nufft_adjoint(la, traj, 8, width=W, density="pipe").values[0]
    print(W, orc.rel(mu * x, adj))
    assert orc.rel(mu * x, adj) == pytest.approx(FULL_SAMPLING[W], rel=0.01)


def test_metadata_and_dataset_layout(numpy_device):
    from xmris_amd import ATTRS, LabeledArray
    from xmris_amd.fitting.dataset import LabeledDataset

    c = orc.case("radial2d", 6)
    y = c.y.reshape(c.C, c.S, 2, 3)
    la = labeled(y, ("coil", "sample", "rep", "time"), coil=np.arange(c.C), time=np.arange(3) * 1e-3, rep=np.arange(2),
                 readout=("sample", np.arange(c.S) * 2.0), label=("time", np.arange(3) * 10.0, {"units": "a.u."}))
    sens = LabeledArray(np.ascontiguousarray(np.moveaxis(c.s, 0, -1)), ("x", "y", "coil"), {}, {}, None)
    ds = la.xmr.recon_cg_sense(c.traj, sens, iterations=6, tol=0.0, regularization=0.05, density="pipe", fov=(0.2, 0.25),
                               return_info=True)
    assert isinstance(ds, LabeledDataset) and set(ds.data_vars) == {"image", "residual", "iterations", "status"}
    img = ds["image"]
    assert img.dims == ("x", "y", "rep", "time") and img.shape == (8, 8, 2, 3) and img.name == "fid"
    assert np.allclose(img.coords["x"].values, (np.arange(8) - 4) * 0.2 / 8)
    assert np.allclose(img.coords["y"].values, (np.arange(8) - 4) * 0.25 / 8)
    assert "readout" not in img.coords and "sample" not in img.coords and "coil" not in img.coords
    assert img.coords["label"].attrs == {"units": "a.u."} and np.array_equal(img.coords["time"].values, la.coords["time"].values)
    beta = grid_orc.beta_of(4, 2.0)
    assert img.attrs == {"note": "kept", ATTRS.grid_dims: ("x", "y"), ATTRS.grid_matrix: (8, 8), ATTRS.grid_oversampled: (16, 16),
                         ATTRS.grid_width: 4, ATTRS.grid_beta: (beta, beta), ATTRS.grid_density: "pipe",
                         ATTRS.cgsense_iterations: 6, ATTRS.cgsense_tol: 0.0, ATTRS.cgsense_regularization: 0.05}
    assert ds.attrs == img.attrs and la.attrs == {"note": "kept"} and la.dims == ("coil", "sample", "rep", "time")
    for name, kind in (("residual", np.float64), ("iterations", np.int32), ("status", np.int32)):
        v = ds[name]
        assert v.dims == ("rep", "time") and v.shape == (2, 3) and v.values.dtype == kind and set(v.coords) == {"rep", "time", "label"}
    assert np.all(ds["iterations"].values == 6) and np.all(ds["status"].values == 0) and np.all(ds["residual"].values < 0.1)
    want = orc.cg(c.dense(), c.rhs(), 6)[0].reshape(8, 8, 2, 3)
    assert orc.rel(img.values, want) <= 1e-12
    # matrix given and agreeing; explicit names; another sample dim
    from xmris_amd import recon_cg_sense

    named = recon_cg_sense(labeled(y, ("coil", "shot", "rep", "time")), c.traj, c.s, matrix=(8, 8), iterations=6, tol=0.0,
                           regularization=0.05, density="pipe", dim="shot", out_dim=("u", "v"))
    assert named.dims == ("u", "v", "rep", "time") and np.array_equal(named.values, img.values)
    assert named.attrs[ATTRS.grid_dims] == ("u", "v")
    # no column dim at all
    one = recon_cg_sense(labeled(c.y[:, :, 0], ("coil", "sample")), c.traj, c.s, iterations=6, tol=0.0, regularization=0.05,
                         density="pipe", return_info=True)
    assert one["image"].dims == ("x", "y") and one["status"].dims == () and np.array_equal(one["image"].values, img.values[:, :, 0, 0])


def test_dataarray_bridge(numpy_device, monkeypatch):
    import _fake_xarray

    xr = _fake_xarray.install(monkeypatch)
    import xmris_amd

    xmris_amd.register_xarray_accessor(force=True)
    c = orc.case("line1d")
    da = xr.DataArray(c.y, dims=("coil", "sample", "time"), coords={"time": np.arange(3.0)}, attrs={"a": 1}, name="k")
    out = xmris_amd.recon_cg_sense(da, c.traj, c.s, regularization=0.05, width=6)
    assert type(out) is xr.DataArray and out.dims == ("x", "time") and out.name == "k" and out.attrs["a"] == 1
    assert np.array_equal(da.xmr.recon_cg_sense(c.traj, c.s, regularization=0.05, width=6).values, out.values)


# ---- validation: every error fires before any native call -----------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    from xmris_amd import _lib
    from xmris_amd import device as dev

    def boom(*a, **k):
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "call", boom)
    for name in ("to_device", "axis_sparse", "axis_dft", "phase_apply", "zero_fill", "fft", "cg_sense", "cgs_expand", "cgs_reduce",
                 "cgs_step", "shift_time"):
        monkeypatch.setattr(dev, name, boom)


TRAJ = grid_orc.random(6, 37, 2, 1)
SENS = orc.maps((6, 6), 3)


def _bad(i, j, v):
    k = TRAJ.copy()
    k[i, j] = v
    return k


@pytest.mark.parametrize("kw, word", [
    (dict(iterations=-1), "iterations"),
    (dict(iterations=2.0), "iterations"),
    (dict(iterations=True), "iterations"),
    (dict(tol=-1e-3), "tol"),
    (dict(tol=float("nan")), "tol"),
    (dict(tol="small"), "tol"),
    (dict(regularization=-0.1), "regularization"),
    (dict(regularization=float("inf")), "regularization"),
    (dict(sensitivities=SENS[:2]), "sensitivities"),  # fewer coils than the data
    (dict(sensitivities=SENS[:, 0]), "sensitivities"),  # one spatial dim for a 2-D trajectory
    (dict(sensitivities=SENS[0]), "sensitivities"),
    (dict(matrix=(6, 5)), "matrix"),
    (dict(matrix=7), "matrix"),
    (dict(matrix=(6, 6, 6)), "matrix"),
    (dict(noise_cov=np.eye(2)), "noise_cov"),
    (dict(noise_cov=-np.eye(3)), "noise_cov"),
    (dict(noise_cov="tail"), "noise_cov"),
    (dict(chunk=0), "chunk"),
    (dict(chunk=1.5), "chunk"),
    (dict(coil_dim="sample"), "coil_dim"),
    (dict(trajectory=TRAJ[:30]), "trajectory"),
    (dict(trajectory=_bad(5, 1, np.nan)), "sample 5"),
    (dict(trajectory=_bad(11, 1, 3.0 + 1e-9)), "sample 11"),
    (dict(width=9), "width"),
    (dict(oversampling=0.9), "oversampling"),
    (dict(density=np.ones(36)), "density"),
    (dict(density="voronoi"), "density"),
    (dict(out_dim=("x",)), "out_dim"),
    (dict(out_dim=("x", "time")), "out_dim"),
    (dict(fov=0.0), "fov"),
])
def test_validation_errors_name_their_argument(no_library, kw, word):
    from xmris_amd import recon_cg_sense

    la = labeled(grid_orc.make((3, 37, 4), seed=1), ("coil", "sample", "time"))
    args = dict(dict(trajectory=TRAJ, sensitivities=SENS), **kw)
    with pytest.raises(ValueError, match=word):
        recon_cg_sense(la, **args)
    with pytest.raises(ValueError, match=word):
        la.xmr.recon_cg_sense(**args)


def test_validation_of_dims_and_coils(no_library):
    from xmris_amd import LabeledArray, recon_cg_sense

    la = labeled(grid_orc.make((3, 37, 4), seed=1), ("coil", "sample", "time"))
    with pytest.raises(ValueError, match=r"Method 'recon_cg_sense' attempted to operate on missing dimension\(s\): \['shot'\]"):
        recon_cg_sense(la, TRAJ, SENS, dim="shot")
    with pytest.raises(ValueError, match="missing dimension"):
        recon_cg_sense(la, TRAJ, SENS, coil_dim="channel")
    many = labeled(grid_orc.make((65, 37), seed=1), ("coil", "sample"))
    with pytest.raises(ValueError, match="coil_dim: 65 coils"):
        recon_cg_sense(many, TRAJ, orc.maps((6, 6), 65))
    with pytest.raises(ValueError, match="sensitivities: dims"):
        recon_cg_sense(la, TRAJ, LabeledArray(SENS, ("coil", "x", "z"), {}, {}, None))
    with pytest.raises(TypeError):
        recon_cg_sense(np.zeros((3, 37), complex), TRAJ, SENS)


def test_default_chunk_keeps_the_grid_within_its_scratch():
    from xmris_amd.processing.cgsense import SCRATCH_BYTES, default_chunk

    assert SCRATCH_BYTES == 1 << 30
    assert default_chunk(16, (64, 64), 8, 2048) == 2048  # 512 KiB per column: exactly 1 GiB
    assert default_chunk(16, (64, 64), 16, 2048) == 1024
    assert default_chunk(8, (32, 32, 32), 8, 2048) == 512
    assert default_chunk(3, (64, 64), 8, 100000) % 2 == 0
    assert default_chunk(64, (128, 128, 128), 16, 7) == 1  # a column larger than the scratch still runs, alone
    for args in ((16, (64, 64), 8, 2048), (5, (20, 22), 16, 99999), (3, (64, 64), 8, 100000)):
        assert args[0] * int(np.prod(args[1])) * args[2] * default_chunk(*args) <= SCRATCH_BYTES


# ---- the C ABI ----------------------------------------------------------------------------------------------------------
def _refusals(fn, order, ok, changes, who):
    import ctypes

    from xmris_amd import _lib

    lib = _lib.load()
    ptrs = [k for k, v in ok.items() if isinstance(v, int) and v >= 1024]

    def args(a):
        return [ctypes.c_double(a[k]) if k in ("lam", "tol") else a[k] for k in order] + [None]

    for change in changes:
        a = dict(ok)
        for k, v in change.items():
            a[k] = ok[v] if isinstance(v, str) else (ok[k] + v if k in ptrs and isinstance(v, int) else v)
        rc = getattr(lib, fn)(*args(a))
        assert rc == _lib.XM_ERR_INVALID_ARG, (fn, change)
        assert who.encode() in lib.xm_last_error_string()


def test_c_abi_refusals_without_gpu():
    _refusals("xm_cgs_expand", orc.EXPAND_ORDER, orc.EXPAND_OK, orc.EXPAND_REFUSALS, "cgs_expand")
    _refusals("xm_cgs_reduce", orc.REDUCE_ORDER, orc.REDUCE_OK, orc.REDUCE_REFUSALS, "cgs_reduce")
    _refusals("xm_cgs_step", orc.STEP_ORDER, orc.STEP_OK, orc.STEP_REFUSALS, "cgs_step")


def test_vocabulary_and_exports():
    import xmris_amd
    from xmris_amd import ATTRS, processing

    assert (ATTRS.cgsense_iterations, ATTRS.cgsense_tol, ATTRS.cgsense_regularization) == (
        "cgsense_iterations", "cgsense_tol", "cgsense_regularization")
    assert xmris_amd.recon_cg_sense is processing.recon_cg_sense
    assert "recon_cg_sense" in xmris_amd.__all__ and "recon_cg_sense" in processing.__all__
    assert hasattr(xmris_amd.XmrisAccessor, "recon_cg_sense")
    for name in ("xm_cgs_expand", "xm_cgs_reduce", "xm_cgs_step"):
        assert name in xmris_amd._lib.SIGNATURES
    assert xmris_amd.device.CGS_VOXELS == 16 and xmris_amd.device.cgs_blocks(48) == 3 and xmris_amd.device.cgs_blocks(49) == 4
