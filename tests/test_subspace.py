"""CPU tests of recon_subspace / temporal_basis: the oracle's operator is Hermitian and positive, the
folded conjugate gradients meet the direct solve, full sampling with an orthonormal basis is per-column CG-SENSE of the
projected data, kappa is the kept fraction, temporal_basis is numpy's SVD, the Python layer on the numpy stand-in
(tests/_subspace_device.py) reproduces the oracle and keeps dims, coordinates and attrs, every validation error fires
before the library is reached, the xm_sub_* entry points refuse bad arguments without a GPU, and the subspace solve of
quarter-sampled data beats the zero-filled per-column route.  Every test imports a name the feature adds."""
import os
import re

import numpy as np
import pytest

import _cgsense_oracle as cg
import _grid_oracle as grid_orc
import _subspace_oracle as orc
from test_cgsense import _refusals, labeled

# tests/tool_subspace_tolerance.py, recorded in profiles/subspace/tolerance.txt: the largest disagreement of two routes of
# the oracle after 6 iterations relative to max |x| and 16 x that, in complex128 (dense against staged) and with every
# coil-sized intermediate rounded to complex64; and the errors against the truth on radial2d with a quarter kept
ROUTE_GAP128, SUB_TOL128 = 1.809e-15, 2.895e-14
ROUTE_GAP64, SUB_TOL64 = 1.316e-07, 2.106e-06
BENEFIT = dict(subspace=0.272, full=0.237, zero_filled=0.820)
PROFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "subspace", "tolerance.txt")
NINE = [(name, keep) for name in ("radial2d", "odd2d", "line1d") for keep in orc.KEEPS]


def test_tolerance_constants_match_their_tool():
    from xmris_amd import recon_subspace  # noqa: F401  (the constants belong to the feature)

    text = open(PROFILE).read()
    assert float(re.search(r"SUB_TOL128 = ([0-9.e+-]+)", text).group(1)) == SUB_TOL128
    assert float(re.search(r"SUB_TOL64 = ([0-9.e+-]+)", text).group(1)) == SUB_TOL64
    assert float(re.search(r"largest route disagreement: ([0-9.e+-]+)", text).group(1)) == ROUTE_GAP128
    assert float(re.search(r"largest complex64 rounding gap: ([0-9.e+-]+)", text).group(1)) == ROUTE_GAP64
    assert SUB_TOL128 == pytest.approx(16 * ROUTE_GAP128, rel=0.01) and SUB_TOL64 == pytest.approx(16 * ROUTE_GAP64, rel=0.01)
    m = re.search(r"benefit radial2d keep 0.25: subspace ([0-9.]+) fully sampled ([0-9.]+) zero-filled ([0-9.]+)", text)
    assert tuple(float(g) for g in m.groups()) == (BENEFIT["subspace"], BENEFIT["full"], BENEFIT["zero_filled"])
    p = orc.problem("radial2d", 0.5, 1)  # one setting recomputed
    y64 = cg.c64(p.y)
    gap = cg.rel(p.image(p.folded(p.staged(cg.c64), p.staged_rhs(cg.c64, y64), 6)[0]),
                 p.image(p.folded(p.staged(), p.staged_rhs(y=y64), 6)[0]))
    print(gap)
    assert gap <= ROUTE_GAP64 * 1.02


# ---- the oracle -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, keep", NINE)
def test_operator_is_hermitian_positive_and_cg_meets_the_direct_solve(name, keep):
    """The folded recurrence is conjugate gradients on one Hermitian positive system per frame: its distance to the direct
    solve is at most cond(M) x the relative residual it stopped at."""
    from xmris_amd import recon_subspace  # noqa: F401

    p = orc.problem(name, keep)
    M = p.normal_matrix()
    ev = np.linalg.eigvalsh(M)
    assert np.abs(M - M.conj().T).max() <= 4e-16 * np.abs(M).max() and ev.min() > 0
    U = p.solve()
    Uc, residual, n_iter, status = p.folded(p.dense(), p.rhs(), 60, 1e-10)
    d = float(np.linalg.norm(Uc - U) / np.linalg.norm(U))
    print(name, keep, d, residual, n_iter, status, ev.max() / ev.min())
    assert status[0] in (0, 1) and (status[0] == 1) == (residual[0] <= 1e-10) and n_iter[0] <= 60
    assert d <= (ev.max() / ev.min()) * max(residual[0], 1e-14)
    staged = p.folded(p.staged(), p.staged_rhs(), 6)[0]
    assert cg.rel(staged, p.folded(p.dense(), p.rhs(), 6)[0]) <= 1e-12  # the staged operator is the dense one


@pytest.mark.parametrize("name", ["radial2d", "odd2d", "line1d"])
def test_full_sampling_is_per_column_cg_sense_of_the_projected_data(name):
    from xmris_amd import recon_subspace  # noqa: F401

    p = orc.problem(name, 1.0)
    c = p.c
    assert np.abs(p.K - np.eye(p.R)[None]).max() <= 1e-14 and p.kappa == pytest.approx(1.0, abs=1e-14)
    b = orc.project(p.y, p.V, None)  # [C, S, R, 1]
    rhs = cg.reduce_coils(c.sv, c.adjoint(b.reshape(c.C, c.S, p.R)))
    each = np.linalg.solve(c.normal_matrix(), rhs)  # [V, R]: CG-SENSE's own system, every coefficient on its own
    assert cg.rel(p.solve()[:, :, 0], each) <= 1e-12


@pytest.mark.parametrize("name, keep", NINE)
def test_kappa_is_the_kept_fraction(name, keep):
    """tr K_s = the number of kept points x the mean |V|^2 over them: for orthonormal rows kappa is the density-weighted
    kept fraction up to the sampling noise of sum_t m |V|^2, a few standard deviations of sqrt(keep (1 - keep) / T)."""
    from xmris_amd import recon_subspace  # noqa: F401

    p = orc.problem(name, keep)
    print(name, keep, p.kappa, p.m.mean())
    assert abs(p.kappa - keep) <= 4 * np.sqrt(keep * (1 - keep) / p.T) + 1e-12


def test_temporal_basis_is_numpys_svd():
    from xmris_amd import TemporalBasis, temporal_basis

    rng = np.random.default_rng(3)
    train = (rng.standard_normal((5, 6, 3)) + 1j * rng.standard_normal((5, 6, 3))) @ \
        (rng.standard_normal((3, 40)) + 1j * rng.standard_normal((3, 40)))
    train = train + 1e-3 * rng.standard_normal(train.shape)
    tb = temporal_basis(labeled(np.moveaxis(train, -1, 1), ("x", "time", "y")), 3)
    _, sigma, vh = np.linalg.svd(train.reshape(30, 40), full_matrices=False)
    assert isinstance(tb, TemporalBasis) and tb.rank == 3 and tb.n_time == 40 and tb.vectors.dtype == np.complex128
    assert np.allclose(tb.singular_values, sigma, rtol=1e-12)
    for k in range(3):  # up to the phase of each vector
        assert abs(abs(np.vdot(vh[k], tb.vectors[k])) - 1.0) <= 1e-10
    assert tb.energy == pytest.approx(float((sigma[:3] ** 2).sum() / (sigma ** 2).sum()), rel=1e-12) and tb.energy > 0.999
    assert abs(abs(np.vdot(temporal_basis(train, 2).vectors[1], tb.vectors[1])) - 1.0) <= 1e-10  # array-like: time last
    for bad, word in ((0, "rank"), (33, "rank"), (41, "rank"), (2.0, "rank"), (True, "rank")):
        with pytest.raises(ValueError, match=word):
            temporal_basis(train, bad)
    with pytest.raises(ValueError, match="rank"):
        temporal_basis(train[:1, :2], 3)  # two rows
    with pytest.raises(ValueError, match="finite"):
        temporal_basis(np.where(np.arange(40) == 3, np.nan, train), 2)
    with pytest.raises(ValueError, match="missing dimension"):
        temporal_basis(labeled(train, ("x", "y", "time")), 2, dim="t")


# ---- the Python layer on the numpy stand-in -----------------------------------------------------------------------------
@pytest.fixture
def numpy_device(monkeypatch):
    import _subspace_device

    return _subspace_device.install(monkeypatch)


def recon(p, y=None, iterations=6, tol=0.0, dims=("coil", "sample", "rep", "time"), basis=None, **kw):
    from xmris_amd import recon_subspace

    c = p.c
    kw = dict(dict(regularization=c.reg, density=c.density, width=c.W, sampling=p.m), **kw)
    return recon_subspace(labeled(p.y if y is None else y, dims), c.traj, c.s, p.V if basis is None else basis, iterations=iterations,
                          tol=tol, **kw)


@pytest.mark.parametrize("name, keep, frames", [("radial2d", 0.5, 1), ("masked2d", 1.0, 4), ("odd2d", 0.25, 1), ("line1d", 0.5, 4),
                                                ("random3d", 0.5, 1)])
def test_python_layer_reproduces_the_oracle_on_the_stand_in(numpy_device, name, keep, frames):
    """The system the package assembles (tables, K, kappa, lambda, the folding) is the oracle's: 6 iterations agree to
    rounding, and the launches are the expected ones."""
    p = orc.problem(name, keep, frames)
    ds = recon(p, return_info=True, return_coefficients=True, sampling=None if keep == 1.0 else p.m)
    want = p.folded(p.dense(), p.rhs(), 6)
    d = cg.rel(ds["image"].values.reshape(p.c.V, frames, p.T), p.image(want[0]))
    print(name, keep, frames, d)
    assert d <= 1e-11
    assert cg.rel(ds["coefficients"].values.reshape(p.c.V, p.R, frames), want[0]) <= 1e-11
    assert np.array_equal(ds["iterations"].values, want[2]) and np.array_equal(ds["status"].values, want[3])
    assert numpy_device.count("sub_project") == 1 and numpy_device.count("sub_expand") == 1 and numpy_device.count("cg_sense") == 1
    assert numpy_device.count("sub_mix") == 6 * frames  # (the stand-in's conjugate gradients take one frame at a time)
    if name == "masked2d":
        dead = (np.abs(p.c.sv) ** 2).sum(axis=0) == 0
        assert dead.sum() > 8 and np.all(ds["image"].values.reshape(p.c.V, -1)[dead] == 0)


def test_chunks_layouts_and_garbage_on_the_stand_in(numpy_device):
    p = orc.problem("radial2d", 0.5, 4)
    ref = recon(p).values
    assert np.array_equal(recon(p, chunk=1).values, ref) and numpy_device.count("cg_sense") == 5
    # the frames first; the sampling labelled and transposed; garbage where nothing was sampled
    from xmris_amd import LabeledArray

    junk = np.where(p.m[None, :, None, :], p.y, np.nan)
    m = LabeledArray(np.ascontiguousarray(p.m.T), ("time", "sample"), {}, {}, None)
    out = recon(p, y=np.ascontiguousarray(np.moveaxis(junk, 2, 0)), dims=("rep", "coil", "sample", "time"), sampling=m)
    assert out.dims == ("rep", "x", "y", "time") and np.array_equal(out.values, np.moveaxis(ref, 2, 0))
    # all-false sampling: a zero image, converged at once
    ds = recon(p, sampling=np.zeros_like(p.m), return_info=True)
    assert np.all(ds["image"].values == 0) and np.all(ds["status"].values == 1) and np.all(ds["iterations"].values == 0)
    assert ds["image"].attrs["subspace_sampled_fraction"] == 0.0
    # a basis that is not orthonormal spans the same images (line1d: 24 unknowns, conjugate gradients end exactly)
    q = orc.problem("line1d", 0.5, 4)
    mixed = np.array([[1.0, 0.3, 0], [0, 2.0, 0.1j], [0.2, 0, 0.5]]) @ q.V
    kw = dict(iterations=200, tol=1e-13, regularization=0.0)
    assert cg.rel(recon(q, basis=mixed, **kw).values, recon(q, **kw).values) <= 1e-8


def test_metadata_and_dataset_layout(numpy_device):
    from xmris_amd import ATTRS, DIMS, LabeledArray, TemporalBasis
    from xmris_amd.fitting.dataset import LabeledDataset

    p = orc.problem("radial2d", 0.5, 4)
    c = p.c
    y = p.y.reshape(c.C, c.S, 2, 2, p.T)
    la = labeled(y, ("coil", "sample", "rep", "avg", "time"), coil=np.arange(c.C), time=np.arange(p.T) * 1e-3, rep=np.arange(2),
                 readout=("sample", np.arange(c.S) * 2.0), ppm=("time", np.arange(p.T) * 10.0, {"units": "a.u."}))
    sens = LabeledArray(np.ascontiguousarray(np.moveaxis(c.s, 0, -1)), ("x", "y", "coil"), {}, {}, None)
    tb = TemporalBasis(vectors=p.V)
    ds = la.xmr.recon_subspace(c.traj, sens, tb, sampling=p.m, iterations=6, tol=0.0, regularization=0.05, density="pipe",
                               fov=(0.2, 0.25), return_info=True, return_coefficients=True)
    assert isinstance(ds, LabeledDataset) and set(ds.data_vars) == {"image", "coefficients", "residual", "iterations", "status"}
    img = ds["image"]
    assert img.dims == ("x", "y", "rep", "avg", "time") and img.shape == (8, 8, 2, 2, p.T) and img.name == "fid"
    assert img.values.dtype == np.complex128
    assert np.allclose(img.coords["x"].values, (np.arange(8) - 4) * 0.2 / 8)
    assert "readout" not in img.coords and "coil" not in img.coords and img.coords["ppm"].attrs == {"units": "a.u."}
    assert np.array_equal(img.coords["time"].values, la.coords["time"].values)
    beta = grid_orc.beta_of(4, 2.0)
    assert img.attrs == {"note": "kept", ATTRS.grid_dims: ("x", "y"), ATTRS.grid_matrix: (8, 8), ATTRS.grid_oversampled: (16, 16),
                         ATTRS.grid_width: 4, ATTRS.grid_beta: (beta, beta), ATTRS.grid_density: "pipe",
                         ATTRS.subspace_rank: 3, ATTRS.subspace_sampled_fraction: float(p.m.mean()),
                         ATTRS.cgsense_iterations: 6, ATTRS.cgsense_tol: 0.0, ATTRS.cgsense_regularization: 0.05}
    assert la.attrs == {"note": "kept"}
    for name, kind in (("residual", np.float64), ("iterations", np.int32), ("status", np.int32)):
        v = ds[name]
        assert v.dims == ("rep", "avg") and v.shape == (2, 2) and v.values.dtype == kind and set(v.coords) == {"rep"}
    co = ds["coefficients"]
    assert co.dims == ("x", "y", DIMS.coefficient, "rep", "avg") and co.shape == (8, 8, 3, 2, 2) and DIMS.coefficient == "coefficient"
    assert cg.rel(img.values, np.einsum("xyrab,rt->xyabt", co.values, p.V)) <= 1e-14
    want = p.image(p.folded(p.dense(), p.rhs(), 6)[0]).reshape(8, 8, 2, 2, p.T)
    assert cg.rel(img.values, want) <= 1e-11
    # time in the middle, another sample dim, explicit names, no frame dim at all
    from xmris_amd import recon_subspace

    one = recon_subspace(labeled(np.ascontiguousarray(np.moveaxis(y[:, :, 0, 0], 2, 0)), ("time", "coil", "shot")), c.traj, c.s, p.V,
                         sampling=p.m, iterations=6, tol=0.0, regularization=0.05, density="pipe", dim="shot", out_dim=("u", "v"),
                         return_info=True)
    assert one["image"].dims == ("time", "u", "v") and one["status"].dims == () and set(one.data_vars) == {"image", "residual", "iterations", "status"}
    assert np.array_equal(np.moveaxis(one["image"].values, 0, -1), img.values[:, :, 0, 0])
    only = recon_subspace(la, c.traj, c.s, p.V, sampling=p.m, iterations=6, tol=0.0, regularization=0.05, density="pipe",
                          return_coefficients=True)
    assert set(only.data_vars) == {"image", "coefficients"}


def test_dataarray_bridge(numpy_device, monkeypatch):
    import _fake_xarray

    xr = _fake_xarray.install(monkeypatch)
    import xmris_amd

    xmris_amd.register_xarray_accessor(force=True)
    p = orc.problem("line1d", 0.5, 1)
    c = p.c
    da = xr.DataArray(p.y[:, :, 0], dims=("coil", "sample", "time"), coords={"time": np.arange(float(p.T))}, attrs={"a": 1}, name="k")
    out = xmris_amd.recon_subspace(da, c.traj, c.s, p.V, sampling=p.m, regularization=0.05, width=6)
    assert type(out) is xr.DataArray and out.dims == ("x", "time") and out.name == "k" and out.attrs["a"] == 1
    assert np.array_equal(da.xmr.recon_subspace(c.traj, c.s, p.V, sampling=p.m, regularization=0.05, width=6).values, out.values)


# ---- validation: every error fires before any native call -----------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    from xmris_amd import _lib
    from xmris_amd import device as dev

    def boom(*a, **k):
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "call", boom)
    for name in ("to_device", "axis_sparse", "axis_dft", "phase_apply", "zero_fill", "fft", "cg_sense", "sub_project", "sub_mix",
                 "sub_expand", "subspace_setup", "subspace_sense"):
        monkeypatch.setattr(dev, name, boom)


TRAJ = grid_orc.random(6, 37, 2, 1)
SENS = cg.maps((6, 6), 3)
BASIS = orc.basis_of(grid_orc.make((4, 12), seed=2), 3)


@pytest.mark.parametrize("kw, word", [
    (dict(basis=BASIS[:, :11]), "basis"),  # another T
    (dict(basis=np.ones((33, 12))), "basis"),
    (dict(basis=np.ones((13, 12))[:, :12]), "basis"),  # R > T
    (dict(basis=np.where(np.arange(12) == 5, np.inf, BASIS)), "basis"),
    (dict(basis=BASIS[0]), "basis"),
    (dict(basis="navigator"), "basis"),
    (dict(sampling=np.ones((37, 11), bool)), "sampling"),
    (dict(sampling=np.ones((12, 37), bool)), "sampling"),
    (dict(sampling=np.ones((37, 12))), "sampling"),
    (dict(sampling=np.ones((37, 12), np.uint8)), "sampling"),
    (dict(time_dim="sample"), "time_dim"),
    (dict(time_dim="coil"), "time_dim"),
    (dict(iterations=-1), "iterations"),
    (dict(tol=float("nan")), "tol"),
    (dict(regularization=-0.1), "regularization"),
    (dict(chunk=0), "chunk"),
    (dict(sensitivities=SENS[:2]), "sensitivities"),
    (dict(matrix=(6, 5)), "matrix"),
    (dict(trajectory=TRAJ[:30]), "trajectory"),
    (dict(out_dim=("x", "time")), "out_dim"),
])
def test_validation_errors_name_their_argument(no_library, kw, word):
    from xmris_amd import recon_subspace

    la = labeled(grid_orc.make((3, 37, 12), seed=1), ("coil", "sample", "time"))
    args = dict(dict(trajectory=TRAJ, sensitivities=SENS, basis=BASIS), **kw)
    with pytest.raises(ValueError, match=word):
        recon_subspace(la, **args)
    with pytest.raises(ValueError, match=word):
        la.xmr.recon_subspace(**args)


def test_validation_of_dims_and_labelled_sampling(no_library):
    from xmris_amd import LabeledArray, recon_subspace

    la = labeled(grid_orc.make((3, 37, 12), seed=1), ("coil", "sample", "time"))
    with pytest.raises(ValueError, match=r"missing dimension\(s\): \['t'\]"):
        recon_subspace(la, TRAJ, SENS, BASIS, time_dim="t")
    with pytest.raises(ValueError, match="sampling: dims"):
        recon_subspace(la, TRAJ, SENS, BASIS, sampling=LabeledArray(np.ones((37, 12), bool), ("sample", "rep"), {}, {}, None))
    with pytest.raises(TypeError):
        recon_subspace(la, TRAJ, SENS, BASIS, readout_time=np.zeros(37))  # deliberately not a parameter


# ---- the C ABI ----------------------------------------------------------------------------------------------------------
def test_c_abi_refusals_without_gpu():
    _refusals("xm_sub_project", orc.PROJECT_ORDER, orc.PROJECT_OK, orc.PROJECT_REFUSALS, "sub_project")
    _refusals("xm_sub_mix", orc.MIX_ORDER, orc.MIX_OK, orc.MIX_REFUSALS, "sub_mix")
    _refusals("xm_sub_expand", orc.EXPAND_ORDER, orc.EXPAND_OK, orc.EXPAND_REFUSALS, "sub_expand")


def test_vocabulary_and_exports():
    import xmris_amd
    from xmris_amd import ATTRS, DIMS, processing

    assert (ATTRS.subspace_rank, ATTRS.subspace_sampled_fraction, DIMS.coefficient) == (
        "subspace_rank", "subspace_sampled_fraction", "coefficient")
    for name in ("recon_subspace", "temporal_basis", "TemporalBasis"):
        assert getattr(xmris_amd, name) is getattr(processing, name) and name in xmris_amd.__all__ and name in processing.__all__
    assert hasattr(xmris_amd.XmrisAccessor, "recon_subspace")
    for name in ("xm_sub_project", "xm_sub_mix", "xm_sub_expand"):
        assert name in xmris_amd._lib.SIGNATURES
    assert xmris_amd.device.SUB_MAX_RANK == 32 == xmris_amd._lib.XM_SUB_MAX_RANK


# ---- the benefit ----------------------------------------------------------------------------------------------------------
def test_subspace_beats_the_zero_filled_per_column_route():
    """radial2d with a random quarter of the (sample, time) positions kept: the subspace solve is closer to the truth than
    half the zero-filled per-column solve's error, and within 1.25 x the per-column solve of the fully sampled data."""
    from xmris_amd import recon_subspace  # noqa: F401

    p = orc.problem("radial2d", 0.25)
    sub, full, zf = (orc.err(x, p.truth) for x in (p.image(p.solve()), p.per_column(p.full), p.per_column(p.y)))
    print(sub, full, zf)
    assert (round(sub, 3), round(full, 3), round(zf, 3)) == (BENEFIT["subspace"], BENEFIT["full"], BENEFIT["zero_filled"])
    assert sub < 0.5 * zf and sub < 1.25 * full
