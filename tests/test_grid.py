"""CPU tests of grid_kspace / degrid_kspace / nufft_adjoint / nufft_forward / density_weights: `grid_table` equals the
oracle's dense matrix entry by entry, the approximation error of the NUFFT stays within the recorded
figures, the Python layer (on the numpy stand-in for the device plus numpy versions of ``axis_sparse`` and ``axis_dft``)
keeps dims, coordinates, attrs and names as specified, every validation error fires before the library is reached,
`SparseTable` refuses what would read out of bounds, and xm_axis_sparse refuses bad arguments without a GPU.

The tests of the oracle alone import nothing from the package and pass without the feature; all others fail without it."""
import os
import re

import numpy as np
import pytest

import _grid_oracle as orc
import _mrsi_oracle as mrsi_orc

# the largest disagreement of the oracle's two product routes over orc.PARITY_CASES, both directions, in units of the
# output's U (orc.unit) -- tests/tool_grid_tolerance.py, recorded in profiles/grid/tolerance.txt -- and 16 x that
ROUTE_GAP = 1.746
GRID_TOL = 27.9
# relative error of nufft_adjoint against the exact sum (same tool, same file); the tests allow 2 x these
ACCURACY = {"radial_m16_w4": 7.046e-04, "radial_m16_w6": 8.899e-06, "random_m16_w4": 9.142e-04,
            "random_m16_w6": 1.039e-05, "cartesian_m8_w4": 2.968e-03, "cartesian_m8_w6": 2.201e-05}
PROFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "grid", "tolerance.txt")


def bound(u, y=None, dtype=np.complex128):
    """On |result - oracle|: GRID_TOL U; complex64 adds the final rounding eps32 |y|."""
    b = GRID_TOL * u
    if np.dtype(dtype) == np.complex64:
        b = b + orc.EPS32 * np.abs(y)
    return b


# ---- the oracle -----------------------------------------------------------------------------------------------------------
def test_tolerance_constants_match_their_tool():
    text = open(PROFILE).read()
    assert float(re.search(r"GRID_TOL = ([0-9.]+)", text).group(1)) == GRID_TOL
    assert float(re.search(r"largest disagreement: ([0-9.]+)", text).group(1)) == ROUTE_GAP
    assert GRID_TOL == pytest.approx(16 * ROUTE_GAP, rel=0.01)
    recorded = {m.group(1): float(m.group(2)) for m in re.finditer(r"accuracy (\w+) .* relative error ([0-9.e+-]+)", text)}
    assert recorded == ACCURACY
    assert orc.worst_route_gap() == pytest.approx(ROUTE_GAP, rel=0.02)


@pytest.mark.parametrize("name", list(orc.ACCURACY_CASES))
def test_oracle_accuracy_is_what_was_recorded(name):
    x, traj, matrix, W, exact = orc.accuracy_case(name)
    err = orc.accuracy(orc.nufft_adjoint(x, traj, matrix, 2.0, W), exact)
    print(name, err)
    assert err == pytest.approx(ACCURACY[name], rel=0.01)


def test_exact_sum_of_a_cartesian_trajectory_is_to_image():
    x = orc.make((8, 6, 3), seed=2)
    exact = orc.adjoint_exact(x.reshape(48, 3), orc.cartesian((8, 6), 2), (8, 6))
    want = mrsi_orc.reconstruct(x, [0, 1])
    assert np.abs(exact - want).max() <= 64 * orc.EPS * np.abs(want).max()


def test_every_sample_of_the_wrapping_case_wraps():
    traj = orc.PARITY_CASES["3d_wraps"][0]()
    A, Gs = orc.dense_matrix(traj, 4, 2.0, 4)
    first = np.add.reduce(A.reshape(Gs + (len(traj),)) != 0, axis=(1, 2)) > 0  # [G0, S]: planes a sample touches
    assert np.all(first[0] & first[-1]) and np.all((A != 0).sum(axis=0) == 64)


# ---- grid_table against the oracle ------------------------------------------------------------------------------------------
def edge_trajectory(ms):
    """Samples on the wrap edge (k = -m/2, k just below m/2), on the lattice (integer and half-integer u) and in between."""
    rows = []
    for m in ms:
        rows.append(np.clip([-m / 2, np.nextafter(m / 2, 0), 0.0, 1.0, -1.5, 0.25, m / 2 - 0.5, 0.3, -m / 2 + 1e-9, m / 4],
                            -m / 2, m / 2))
    k = np.array(rows).T
    mixed = np.stack([np.roll(k[:, a], 3 + 2 * a) for a in range(len(ms))], axis=1)  # the dims out of step
    return np.concatenate([k, mixed])


TABLE_CASES = {
    "1d_odd_m": ((7,), 2.0, 4),
    "1d_w6": ((8,), 2.0, 6),
    "2d_odd_even": ((5, 6), 2.0, 4),
    "2d_w5_alpha_1_25": ((8, 7), 1.25, 5),
    "3d": ((4, 3, 5), 2.0, 4),
    "3d_w2": ((3, 3, 2), 1.5, 2),
}


def dense_of(table):
    M = np.zeros((table.n_rows, table.n))
    rows = np.repeat(np.arange(table.n_rows), np.diff(table.rowptr))
    assert len(set(zip(rows.tolist(), table.col.tolist()))) == len(rows)  # no entry twice
    M[rows, table.col] = table.val
    return M


@pytest.mark.parametrize("name", list(TABLE_CASES))
def test_grid_table_equals_the_oracle(name):
    from xmris_amd import grid_table

    ms, a0, W = TABLE_CASES[name]
    traj = edge_trajectory(ms)
    dens = 0.5 + np.arange(len(traj)) / 7.0
    t = grid_table(traj, ms, a0, W, density=dens)
    A, Gs = orc.dense_matrix(traj, ms, a0, W, dens)
    assert t.oversampled == Gs and all(G % 2 == 0 and G >= a0 * m and G - 2 < a0 * m for G, m in zip(Gs, ms))
    got = dense_of(t.grid)
    assert np.array_equal(got != 0, A != 0)  # the same sparsity pattern
    assert np.all(np.abs(got - A) <= 8 * orc.EPS * np.abs(A))
    assert np.all((A != 0).sum(axis=0) == W ** len(ms))  # exactly W cells per dim, wrapped or not
    for r in range(t.grid.n_rows):  # each row's entries in ascending sample index
        assert np.all(np.diff(t.grid.col[t.grid.rowptr[r]:t.grid.rowptr[r + 1]]) > 0)
    # the degrid table is the exact transpose of the unit-density matrix, rows in ascending cell
    unit_density = grid_table(traj, ms, a0, W)
    assert np.array_equal(dense_of(t.degrid), dense_of(unit_density.grid).T)
    assert np.array_equal(t.degrid.rowptr, np.arange(len(traj) + 1) * W ** len(ms))
    assert np.all(np.diff(t.degrid.col.reshape(len(traj), -1), axis=1) > 0)
    for a, (m, G) in enumerate(zip(ms, Gs)):
        beta = orc.beta_of(W, G / m)
        assert t.beta[a] == pytest.approx(beta, rel=1e-15)
        assert np.allclose(t.deapodization[a], orc.deapodization(m, G, W, beta), rtol=1e-13, atol=0)
    if W % 2 == 0:  # the lattice-aligned sample k = 0 holds the edge value 1 / I0(beta) (the support is half open)
        col = dense_of(unit_density.grid)[:, 2]
        edge = np.prod([1.0 / np.i0(orc.beta_of(W, G / m)) for m, G in zip(ms, Gs)])
        assert np.isclose(col[col > 0].min(), edge, rtol=1e-14)


# ---- the Python layer on the numpy stand-in -----------------------------------------------------------------------------
def np_axis_sparse(x, axis, table):
    """The CSR sum in its stored order, complex128, rounded once to x's dtype."""
    from xmris_amd.device import SparseTable

    assert isinstance(table, SparseTable) and x.shape[axis] == table.n
    xm = np.moveaxis(np.asarray(x, dtype=np.complex128), axis, 0)
    y = np.zeros((table.n_rows,) + xm.shape[1:], dtype=np.complex128)
    rows = np.repeat(np.arange(table.n_rows), np.diff(table.rowptr))
    np.add.at(y, rows, table.val.reshape((-1,) + (1,) * (xm.ndim - 1)) * xm[table.col])
    return np.ascontiguousarray(np.moveaxis(y, 0, axis)).astype(x.dtype)


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

    monkeypatch.setattr(dev, "axis_sparse", axis_sparse)
    monkeypatch.setattr(dev, "axis_dft", axis_dft)
    for name in ("phase_apply", "zero_fill", "fft"):
        def wrap(*a, _f=getattr(dev, name), _n=name, **k):
            calls.append(_n)
            return _f(*a, **k)

        monkeypatch.setattr(dev, name, wrap)
    return calls


def labeled(x, dims, **coords):
    from xmris_amd import LabeledArray

    return LabeledArray(x, dims, coords, {"note": "kept"}, "fid")


@pytest.mark.parametrize("name", list(orc.PARITY_CASES))
def test_grid_and_degrid_match_the_oracle_on_the_stand_in(numpy_device, name):
    from xmris_amd import degrid_kspace, grid_kspace

    x, traj, matrix, a0, W, axis, A, want, u = orc.parity_case(name)
    dims = ["a", "b", "c"][:x.ndim]
    dims[axis] = "sample"
    g = grid_kspace(labeled(x, dims), traj, matrix, a0, W)
    d = traj.shape[1]
    flat = g.values.reshape(want.shape)
    print(name, orc.gap(flat, want, u))
    assert g.dims == tuple(dims[:axis]) + ("kx", "ky", "kz")[:d] + tuple(dims[axis + 1:])
    assert orc.gap(flat, want, u) <= GRID_TOL
    back = degrid_kspace(g, traj, matrix, a0, W)
    ref = orc.apply_csr(A.T, flat, axis)
    assert back.dims == tuple(dims) and orc.gap(back.values, ref, orc.unit(A.T, flat, axis)) <= GRID_TOL
    assert numpy_device == ["axis_sparse", "axis_sparse"]
    # k dims that are neither adjacent nor in order are gathered first: the same values
    if d == 2:
        moved = labeled(np.moveaxis(g.values, (axis, axis + 1), (-1, 0)), ["ky"] + dims[:axis] + dims[axis + 1:] + ["kx"])
        again = degrid_kspace(moved, traj, matrix, a0, W)
        assert np.array_equal(np.moveaxis(again.values, again.get_axis_num("sample"), axis), back.values)


@pytest.mark.parametrize("name", list(orc.ACCURACY_CASES))
def test_nufft_adjoint_stays_within_the_recorded_error(numpy_device, name):
    from xmris_amd import nufft_adjoint

    x, traj, matrix, W, exact = orc.accuracy_case(name)
    img = nufft_adjoint(labeled(x, ("sample", "time")), traj, matrix, width=W)
    err = orc.accuracy(img.values, exact)
    print(name, err)
    assert img.dims == ("x", "y", "time") and err <= 2 * ACCURACY[name]
    # ... and equals the oracle's own chain to rounding
    assert np.abs(img.values - orc.nufft_adjoint(x, traj, matrix, 2.0, W)).max() <= 1e-12 * np.abs(exact).max()


@pytest.mark.parametrize("W", [4, 6])
def test_cartesian_trajectory_matches_to_image(numpy_device, W):
    from xmris_amd import nufft_adjoint, to_image

    x, traj, matrix, _, _ = orc.accuracy_case(f"cartesian_m8_w{W}")
    k = labeled(x.reshape(8, 8, 3), ("kx", "ky", "time"), kx=np.arange(8.0) - 4, ky=np.arange(8.0) - 4)
    want = to_image(k).values
    got = nufft_adjoint(labeled(x, ("sample", "time")), traj, 8, width=W).values
    assert orc.accuracy(got, want) <= 2 * ACCURACY[f"cartesian_m8_w{W}"]


def test_large_grids_take_the_staged_transform(numpy_device):
    from xmris_amd import nufft_adjoint, nufft_forward

    traj = orc.random((40, 6), 90, 2, 9)  # G = (80, 12): dim 0 is beyond axis_dft
    x = orc.make((2, 90), seed=3)
    img = nufft_adjoint(labeled(x, ("coil", "sample")), traj, (40, 6))
    assert numpy_device == ["axis_sparse", "fft", "phase_apply", "axis_dft"]
    want = orc.nufft_adjoint(x, traj, (40, 6), axis=1)
    assert img.shape == (2, 40, 6) and np.abs(img.values - want).max() <= 1e-12 * np.abs(want).max()
    del numpy_device[:]
    back = nufft_forward(img, traj)
    assert numpy_device == ["phase_apply", "zero_fill", "fft", "axis_dft", "axis_sparse"]
    ref = orc.nufft_forward(img.values, traj, (40, 6), axis=1)
    assert back.dims == ("coil", "sample") and np.abs(back.values - ref).max() <= 1e-12 * np.abs(ref).max()


def test_forward_is_the_hermitian_transpose_of_adjoint(numpy_device):
    from xmris_amd import nufft_adjoint, nufft_forward

    traj = orc.random((6, 5), 37, 2, 1)
    x, img = orc.make((37, 2), seed=5), orc.make((6, 5, 2), seed=6)
    ax = nufft_adjoint(labeled(x, ("sample", "time")), traj, (6, 5)).values
    fi = nufft_forward(labeled(img, ("x", "y", "time")), traj).values
    lhs, rhs = np.vdot(img, ax), np.vdot(fi, x)
    assert abs(lhs - rhs) <= 1e-13 * np.linalg.norm(img) * np.linalg.norm(ax)
    assert np.abs(fi - orc.nufft_forward(img, traj, (6, 5))).max() <= 1e-12 * np.abs(fi).max()


def test_density_weights():
    from xmris_amd import density_weights, grid_table

    for traj, m in ((orc.radial(8, 7, 16), 8), (orc.random((5, 6), 31, 2, 4), (5, 6)), (orc.random(4, 20, 3, 3), 4)):
        w = density_weights(traj, m)
        assert np.allclose(w, orc.pipe(traj, m), rtol=1e-12, atol=0)
        assert np.array_equal(grid_table(traj, m, density="pipe").density, w)
        assert np.allclose(density_weights(traj, m, iterations=3), orc.pipe(traj, m, iterations=3), rtol=1e-12, atol=0)
    w = density_weights(orc.cartesian(8, 2), 8)
    assert np.all(np.abs(w - w[0]) <= 1e-12 * w[0])
    w = density_weights(orc.radial(8, 7, 16), 8)
    assert w[8] < 0.5 * w[0]  # the centre of a spoke is sampled more densely than its end


def test_metadata(numpy_device):
    from xmris_amd import ATTRS, DIMS, grid_kspace, nufft_adjoint

    traj = orc.random((6, 5), 37, 2, 1)
    x = orc.make((3, 37, 4), seed=8)
    la = labeled(x, ("coil", "sample", "time"), coil=np.arange(3), time=np.arange(4) * 1e-3,
                 readout=("sample", np.arange(37) * 2.0), label=("time", np.arange(4) * 10.0, {"units": "a.u."}))
    g = grid_kspace(la, traj, (6, 5), fov=(0.2, 0.25))
    assert DIMS.sample == "sample" and g.dims == ("coil", "kx", "ky", "time") and g.shape == (3, 12, 10, 4) and g.name == "fid"
    assert np.allclose(g.coords["kx"].values, (np.arange(12) - 6) * (6 / 12) / 0.2)
    assert np.allclose(g.coords["ky"].values, (np.arange(10) - 5) * (5 / 10) / 0.25)
    assert "readout" not in g.coords and "sample" not in g.coords
    assert g.coords["label"].attrs == {"units": "a.u."} and np.array_equal(g.coords["time"].values, la.coords["time"].values)
    beta = orc.beta_of(4, 2.0)
    assert g.attrs == {"note": "kept", ATTRS.grid_dims: ("kx", "ky"), ATTRS.grid_matrix: (6, 5), ATTRS.grid_oversampled: (12, 10),
                       ATTRS.grid_width: 4, ATTRS.grid_beta: (beta, beta), ATTRS.grid_density: "none"}
    assert la.attrs == {"note": "kept"} and la.dims == ("coil", "sample", "time")
    # to_image's reciprocal rule on the gridded k-space gives voxel positions spaced fov / m
    img = g.xmr.to_image()
    assert np.allclose(np.diff(img.coords["x"].values), 0.2 / 6) and np.allclose(np.diff(img.coords["y"].values), 0.25 / 5)
    # nufft_adjoint: image dims, their coordinates, the density label; the accessor; explicit names; another sample dim
    img = la.xmr.nufft_adjoint(traj, (6, 5), density="pipe", fov=0.2)
    assert img.dims == ("coil", "x", "y", "time") and img.shape == (3, 6, 5, 4) and img.attrs[ATTRS.grid_density] == "pipe"
    assert np.allclose(img.coords["x"].values, (np.arange(6) - 3) * 0.2 / 6)
    assert np.allclose(img.coords["y"].values, (np.arange(5) - 2) * 0.2 / 5)
    assert img.attrs[ATTRS.grid_dims] == ("x", "y")
    named = grid_kspace(labeled(x, ("coil", "shot", "time")), traj, (6, 5), density=np.ones(37), dim="shot", out_dim=("ka", "kb"))
    assert named.dims == ("coil", "ka", "kb", "time") and named.attrs[ATTRS.grid_density] == "custom"
    assert np.array_equal(named.values, g.values)
    back = named.xmr.degrid_kspace(traj, (6, 5), dim=("ka", "kb"), out_dim="shot")
    assert back.dims == ("coil", "shot", "time") and np.array_equal(back.coords["shot"].values, np.arange(37))
    fwd = img.xmr.nufft_forward(traj)
    assert fwd.dims == ("coil", "sample", "time") and fwd.attrs[ATTRS.grid_matrix] == (6, 5)
    # real input is taken as complex
    assert np.iscomplexobj(grid_kspace(labeled(x.real.copy(), ("coil", "sample", "time")), traj, (6, 5)).values)


def test_dataarray_bridge(numpy_device, monkeypatch):
    import _fake_xarray

    xr = _fake_xarray.install(monkeypatch)
    import xmris_amd

    xmris_amd.register_xarray_accessor(force=True)
    traj = orc.random(6, 37, 2, 1)
    x = orc.make((37, 4), seed=13)
    da = xr.DataArray(x, dims=("sample", "time"), coords={"time": np.arange(4.0)}, attrs={"a": 1}, name="k")
    out = xmris_amd.nufft_adjoint(da, traj, 6)
    assert type(out) is xr.DataArray and out.dims == ("x", "y", "time") and out.name == "k" and out.attrs["a"] == 1
    assert np.array_equal(da.xmr.nufft_adjoint(traj, 6).values, out.values)


# ---- validation: every error fires before any native call -----------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    from xmris_amd import _lib
    from xmris_amd import device as dev

    def boom(*a, **k):
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "call", boom)
    for name in ("to_device", "axis_sparse", "axis_dft", "phase_apply", "zero_fill", "fft"):
        monkeypatch.setattr(dev, name, boom)


def _la():
    return labeled(orc.make((3, 37, 4), seed=1), ("coil", "sample", "time"))


TRAJ = orc.random(6, 37, 2, 1)


def _bad(i, j, v):
    k = TRAJ.copy()
    k[i, j] = v
    return k


@pytest.mark.parametrize("kw, word", [
    (dict(trajectory=TRAJ[:, 0]), "trajectory"),  # not [S, d]
    (dict(trajectory=np.zeros((37, 4))), "trajectory"),  # d = 4
    (dict(trajectory=TRAJ * 1j), "trajectory"),  # not real
    (dict(trajectory=TRAJ[:30]), "trajectory"),  # fewer samples than the dim
    (dict(trajectory=_bad(5, 1, np.nan)), "sample 5"),
    (dict(trajectory=_bad(7, 0, np.inf)), "sample 7"),
    (dict(trajectory=_bad(11, 1, 3.0 + 1e-9)), "sample 11"),  # |k| > m / 2
    (dict(trajectory=_bad(12, 0, -3.5)), "sample 12"),
    (dict(matrix=(6, 6, 6)), "matrix"),
    (dict(matrix=6.5), "matrix"),
    (dict(matrix=0), "matrix"),
    (dict(width=1), "width"),
    (dict(width=9), "width"),
    (dict(width=4.0), "width"),
    (dict(oversampling=0.9), "oversampling"),
    (dict(oversampling=float("nan")), "oversampling"),
    (dict(oversampling="two"), "oversampling"),
    (dict(matrix=(6, 2), oversampling=1.0, width=4), "width"),  # W > G
    (dict(density=np.ones(36)), "density"),
    (dict(density=np.ones(37) * 1j), "density"),
    (dict(density=np.full(37, np.inf)), "density"),
    (dict(density="voronoi"), "density"),
    (dict(density="pipe", iterations=-1), "iterations"),
    (dict(out_dim=("kx",)), "out_dim"),
    (dict(out_dim=("kx", "time")), "out_dim"),
    (dict(fov=0.0), "fov"),
    (dict(fov=(1.0, 1.0, 1.0)), "fov"),
])
def test_validation_errors_name_their_argument(no_library, kw, word):
    from xmris_amd import grid_kspace, nufft_adjoint

    args = dict(dict(trajectory=TRAJ, matrix=6), **kw)
    for fn in (grid_kspace, nufft_adjoint):
        with pytest.raises(ValueError, match=word):
            fn(_la(), **args)
    with pytest.raises(ValueError, match=word):
        _la().xmr.nufft_adjoint(**args)


def test_validation_of_dims(no_library):
    from xmris_amd import degrid_kspace, grid_kspace, nufft_forward

    with pytest.raises(ValueError, match=r"Method 'grid_kspace' attempted to operate on missing dimension\(s\): \['shot'\]"):
        grid_kspace(_la(), TRAJ, 6, dim="shot")
    g = labeled(orc.make((12, 12, 2), seed=1), ("kx", "ky", "time"))
    with pytest.raises(ValueError, match=r"Method 'degrid_kspace' attempted to operate on missing dimension"):
        degrid_kspace(g, orc.random(6, 9, 3, 1), 6)
    with pytest.raises(ValueError, match="matrix"):  # the k dims are not the trajectory's oversampled grid
        degrid_kspace(g, TRAJ, 7)
    with pytest.raises(ValueError, match="dim"):
        degrid_kspace(g, TRAJ, 6, dim=("kx",))
    with pytest.raises(ValueError, match="out_dim"):
        degrid_kspace(g, TRAJ, 6, out_dim="time")
    with pytest.raises(ValueError, match="matrix"):
        nufft_forward(labeled(orc.make((6, 6, 2), seed=1), ("x", "y", "time")), TRAJ, matrix=(6, 7))
    with pytest.raises(TypeError):
        grid_kspace(np.zeros((37, 3), complex), TRAJ, 6)


# ---- SparseTable: the only door to the kernel ---------------------------------------------------------------------------
def test_sparse_table_refuses_what_would_read_out_of_bounds():
    from xmris_amd.device import SparseTable, axis_sparse

    ok = dict(rowptr=[0, 2, 2, 3], col=[0, 4, 1], val=[1.0, 2.0, 3.0], n=5)
    t = SparseTable(**ok)
    assert (t.n, t.n_rows, t.nnz) == (5, 3, 3) and t.rowptr.dtype == np.int32 and t.col.dtype == np.int32 and t.val.dtype == np.float64
    for change, word in ((dict(col=[0, 5, 1]), "col"), (dict(col=[0, -1, 1]), "col"), (dict(rowptr=[0, 2, 1, 3]), "rowptr"),
                         (dict(rowptr=[1, 2, 2, 3]), "rowptr"), (dict(rowptr=[0, 2, 2, 4]), "rowptr"), (dict(rowptr=[0, 2, 2, 2]), "rowptr"),
                         (dict(val=[1.0, np.nan, 3.0]), "val"), (dict(val=[1.0, np.inf, 3.0]), "val"), (dict(val=[1.0, 2.0]), "val"),
                         (dict(val=[1.0, 2j, 3.0]), "val"), (dict(col=[0.0, 4.0, 1.0]), "col"), (dict(n=0), "n"), (dict(rowptr=[0]), "n_rows")):
        with pytest.raises(ValueError, match=word):
            SparseTable(**dict(ok, **change))
    # bound to its n and n_rows, frozen
    with pytest.raises(ValueError):
        t.col[1] = 7
    with pytest.raises(AttributeError):
        t.n = 9
    # no path takes raw index arrays
    for raw in ((t.rowptr, t.col, t.val), dict(rowptr=t.rowptr, col=t.col, val=t.val), None):
        with pytest.raises(TypeError, match="SparseTable"):
            axis_sparse(np.zeros((5, 2), complex), 0, raw)


def test_c_abi_refusals_without_gpu():
    from xmris_amd import _lib

    lib = _lib.load()
    ok = dict(x=64, y=128, rowptr=192, col=256, val=320, n_outer=2, n=7, n_rows=16, n_inner=3, dtype=0)
    order = ("x", "y", "rowptr", "col", "val", "n_outer", "n", "n_rows", "n_inner", "dtype")
    for change in orc.REFUSALS:
        a = dict(ok)
        for k, v in change.items():
            a[k] = ok["x"] if v == "x" else (ok[k] + v if k in ("x", "y") and isinstance(v, int) else v)
        rc = lib.xm_axis_sparse(*[a[k] for k in order], None)
        assert rc == _lib.XM_ERR_INVALID_ARG, change
        assert b"axis_sparse" in lib.xm_last_error_string()
    # a zero-sized problem launches nothing, whatever the pointers hold
    assert lib.xm_axis_sparse(64, 128, 192, 256, 320, 0, 7, 16, 3, 0, None) == 0
    assert lib.xm_axis_sparse(64, 128, 192, 256, 320, 2, 7, 16, 0, 1, None) == 0


def test_vocabulary_and_exports():
    import xmris_amd
    from xmris_amd import ATTRS, DIMS, processing

    assert (ATTRS.grid_dims, ATTRS.grid_matrix, ATTRS.grid_oversampled, ATTRS.grid_width, ATTRS.grid_beta, ATTRS.grid_density) == (
        "grid_dims", "grid_matrix", "grid_oversampled", "grid_width", "grid_beta", "grid_density")
    assert DIMS.sample == "sample"
    for name in ("grid_kspace", "degrid_kspace", "nufft_adjoint", "nufft_forward", "density_weights", "grid_table"):
        assert getattr(xmris_amd, name) is getattr(processing, name) and name in xmris_amd.__all__ and name in processing.__all__
    for name in ("grid_kspace", "degrid_kspace", "nufft_adjoint", "nufft_forward"):
        assert hasattr(xmris_amd.XmrisAccessor, name)
    assert "xm_axis_sparse" in xmris_amd._lib.SIGNATURES
