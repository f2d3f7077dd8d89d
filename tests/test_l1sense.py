"""CPU tests of recon_l1_sense: the oracle's Psi is orthonormal and the same in both of its forms,
its shrink is the prox of the penalty, FISTA reaches what ISTA reaches and the linear solve when the penalty is off, the
measured step safety keeps tau below 1 / lambda_max, the penalty pays on the undersampled case; the constants are what
their tool recorded; the Python layer (on the numpy stand-in for the device, with numpy versions of ``axis_sparse``,
``axis_dft``, ``l1_sense`` and ``l1_lipschitz``) reproduces the oracle and keeps dims, coordinates, attrs and names as
specified; every validation error fires before the library is reached, and the xm_l1_* entry points refuse bad arguments
without a GPU.

The tests of the oracle alone import nothing from the package; all others fail without the feature."""
import os
import re

import numpy as np
import pytest

import _cgsense_oracle as cgs_orc
import _grid_oracle as grid_orc
import _l1sense_oracle as orc
import _mrsi_oracle as mrsi_orc
from test_cgsense import _refusals, labeled, np_axis_sparse, np_cg_sense

# tests/tool_l1sense_tolerance.py, recorded in profiles/l1sense/tolerance.txt: the largest disagreement of two routes of the
# oracle after 10 steps relative to max |x| and 16 x that, in complex128 (dense against stage-by-stage CSR) and with every
# coil-sized intermediate rounded to complex64
ROUTE_GAP128, L1_TOL128 = 1.209e-15, 1.934e-14
ROUTE_GAP64, L1_TOL64 = 7.950e-08, 1.272e-06
# 1 + 2 x the largest shortfall of 20 power steps, rounded up to two digits
SHORTFALL, STEP_SAFETY = 8.861e-02, 1.2
# sparsity 0, tikhonov 0.05 on radial2d: the oracle's distance to the direct solve after 200 steps
DISTANCE200 = 4.284e-06
# the benefit case: |x - truth| / |truth| of 30 CG iterations (regularization 0.05), of 100 FISTA steps at sparsity 0.02,
# and of the same at sparsity 0
BENEFIT = {"cg": 0.337, "l1": 0.090, "l1_off": 0.408}
PROFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "l1sense", "tolerance.txt")
PARITY = ["radial2d", "masked2d", "random3d", "odd2d", "line1d"]
LEVEL_TUPLES = [((8,), (3,)), ((8, 6), (2, 1)), ((4, 4, 4), (1, 1, 1)), ((8, 8), (2, 2)), ((8, 8), (0, 0)), ((16, 16), (2, 2)),
                ((4, 4, 4), (2, 2, 0)), ((8,), (2,)), ((8, 6), (0, 1))]


def tau_of(c, safety=STEP_SAFETY, lam=None):
    M0 = c.normal_matrix(0.0)
    return 1.0 / (safety * orc.power(lambda v: M0 @ v, c.mask, 20) + (c.lam if lam is None else lam))


# ---- the oracle -----------------------------------------------------------------------------------------------------------
def test_tolerance_constants_match_their_tool():
    text = open(PROFILE).read()
    assert float(re.search(r"L1_TOL128 = ([0-9.e+-]+)", text).group(1)) == L1_TOL128
    assert float(re.search(r"L1_TOL64 = ([0-9.e+-]+)", text).group(1)) == L1_TOL64
    assert float(re.search(r"largest route disagreement: ([0-9.e+-]+)", text).group(1)) == ROUTE_GAP128
    assert float(re.search(r"largest complex64 rounding gap: ([0-9.e+-]+)", text).group(1)) == ROUTE_GAP64
    assert L1_TOL128 == pytest.approx(16 * ROUTE_GAP128, rel=0.01) and L1_TOL64 == pytest.approx(16 * ROUTE_GAP64, rel=0.01)
    assert float(re.search(r"largest shortfall: ([0-9.e+-]+)", text).group(1)) == SHORTFALL
    assert float(re.search(r"STEP_SAFETY = ([0-9.]+)", text).group(1)) == STEP_SAFETY
    assert 1 + 2 * SHORTFALL <= STEP_SAFETY < 1 + 2 * SHORTFALL + 0.1
    assert float(re.search(r"direct solve at 200 steps ([0-9.e+-]+)", text).group(1)) == DISTANCE200
    assert float(re.search(r"30 CG iterations.*error ([0-9.]+)", text).group(1)) == BENEFIT["cg"]
    assert float(re.search(r"sparsity 0.02: error ([0-9.]+)", text).group(1)) == BENEFIT["l1"]
    assert float(re.search(r"sparsity 0.0: error ([0-9.]+)", text).group(1)) == BENEFIT["l1_off"]
    # the gaps of 40 steps are not above those of 10: rounding is not amplified
    for m in re.finditer(r"complex64 rounding ([0-9.e+-]+) \(10 steps\) ([0-9.e+-]+) \(40\)", text):
        assert float(m.group(2)) <= 16 * ROUTE_GAP64
    c = orc.case("radial2d")  # the case that sets L1_TOL64, recomputed
    y64 = orc.c64(c.y)
    args = (c.ms, c.levels, 0.02, tau_of(c), 10)
    gap = orc.rel(orc.fista(c.staged(rnd=orc.c64), c.rhs(y64, rnd=orc.c64), *args, mask=c.mask).x,
                  orc.fista(c.staged(), c.rhs(y64), *args, mask=c.mask).x)
    assert gap == pytest.approx(ROUTE_GAP64, rel=0.02)


@pytest.mark.parametrize("ms, levels", LEVEL_TUPLES)
def test_psi_is_orthonormal_and_both_forms_agree(ms, levels):
    V = int(np.prod(ms))
    for shift in (None, tuple((3 * (d + 1)) % (1 << l) for d, l in enumerate(levels))):
        P = orc.psi_matrix(ms, levels, shift)
        assert np.abs(P.T @ P - np.eye(V)).max() <= 1e-14
        w = grid_orc.make((V, 3), seed=V)
        coeff = orc.haar(w, ms, levels, shift)
        assert np.abs(coeff - (P @ w)[orc.standard_index(ms, levels)]).max() <= 1e-14
        assert np.abs(orc.haar(coeff, ms, levels, shift, inverse=True) - w).max() <= 1e-14
        theta = np.array([0.3, 0.0, 5.0])
        assert np.abs(orc.prox(w, ms, levels, theta, shift=shift) - orc.prox(w, ms, levels, theta, shift=shift, kron=True)).max() <= 1e-14
    pen = orc.penalised(ms, levels)
    assert np.array_equal(pen[orc.standard_index(ms, levels)], pen)
    assert (~pen).sum() == (0 if not any(levels) else V >> sum(levels))


def test_shrink_is_the_prox_of_the_penalty():
    """x = prox(w) minimises 1/2 |x - w|^2 + theta |pen . Psi x|_1: with c = Psi x, d = Psi w, a penalised c != 0 has
    c - d + theta c / |c| = 0, a penalised c = 0 has |d| <= theta, and the others c = d."""
    ms, levels, theta = (8, 8), (2, 2), 1.2
    w = grid_orc.make((64, 4), seed=5)
    pen = orc.penalised(ms, levels)
    d = orc.haar(w, ms, levels)
    c = orc.shrink(d, theta, pen)
    assert np.abs(orc.haar(orc.prox(w, ms, levels, theta), ms, levels) - c).max() <= 1e-14
    live = pen[:, None] & (c != 0)
    dead = pen[:, None] & (c == 0)
    assert live.sum() > 20 and dead.sum() > 20
    assert np.abs((c - d + theta * c / np.where(c != 0, np.abs(c), 1.0))[live]).max() <= 1e-14
    assert np.all(np.abs(d[dead]) <= theta) and np.array_equal(c[~pen], d[~pen])


def test_sparsity_zero_is_the_linear_solve():
    c = orc.case("radial2d")
    r = orc.fista(c.dense(), c.rhs(), c.ms, c.levels, 0.0, tau_of(c), 200, mask=c.mask)
    d = orc.rel(r.x, c.solve())
    print("distance at 200 steps", d)
    assert d == pytest.approx(DISTANCE200, rel=0.05) and d <= 1e-5 and np.all(r.status == 0)


def test_ista_and_fista_reach_the_same_objective():
    c = orc.case("odd2d")
    args = (c.dense(), c.rhs(), c.ms, c.levels, 0.02, tau_of(c))
    slow = orc.fista(*args, 1500, mask=c.mask, accelerate=False)
    fast = orc.fista(*args, 300, mask=c.mask)
    for t in range(c.T):
        steps = np.diff(slow.objective[t])
        assert np.all(steps <= 1e-13 * abs(slow.objective[t][-1]))  # ISTA never goes up
        assert fast.objective[t][-1] == pytest.approx(slow.objective[t][-1], rel=1e-8)
    assert orc.rel(fast.x, slow.x) <= 1e-3


@pytest.mark.parametrize("name", list(orc.CASES))
def test_measured_safety_keeps_the_step_below_one_over_lambda_max(name):
    c = orc.case(name)
    assert tau_of(c) <= 1.0 / c.lambda_max()
    assert tau_of(c, safety=1.0) > 1.0 / c.lambda_max()  # the estimate alone is a lower bound of lambda_max


def test_default_levels():
    from xmris_amd.processing.l1sense import default_levels

    assert default_levels((8, 8)) == (2, 2) and default_levels((8, 6)) == (2, 1) and default_levels((7, 12)) == (0, 2)
    assert default_levels((4, 4, 4)) == (2, 2, 0) and default_levels((16, 16, 2)) == (2, 2, 0) and default_levels((8,)) == (2,)
    assert default_levels((16, 2, 6)) == (2, 1, 1)
    for name in orc.CASES:
        assert default_levels(orc.CASES[name][1]) == orc.LEVELS[name]


# ---- the Python layer on the numpy stand-in -----------------------------------------------------------------------------
def np_l1_sense(y, s, adjoint, forward, mask, matrix, levels, lam2, sparsity, tau, iterations, tol, cycle_spin=False):
    """The loop of ``device.l1_sense`` on the oracle's iteration and the package's own two chains."""
    from xmris_amd.device import L1Sense

    c, v = s.shape
    b = cgs_orc.reduce_coils(s, adjoint(y).reshape(c, v, -1).astype(np.complex128))

    def op(p):
        u = (s[:, :, None] * p[None, :, :]).astype(y.dtype)
        return cgs_orc.reduce_coils(s, adjoint(forward(u)).reshape(c, v, -1).astype(np.complex128)) + lam2 * p

    r = orc.fista(op, b, tuple(matrix), tuple(levels), sparsity, tau, iterations, tol, np.asarray(mask) != 0, cycle_spin)
    return L1Sense(x=r.x, change=r.change, iterations=r.n_iter, status=r.status)


def np_l1_lipschitz(s, adjoint, forward, mask, power_iterations, dtype):
    c, v = s.shape

    def op(p):
        u = (s[:, :, None] * p[None, :, :]).astype(dtype)
        return cgs_orc.reduce_coils(s, adjoint(forward(u)).reshape(c, v, -1).astype(np.complex128))

    return orc.power(op, np.asarray(mask) != 0, power_iterations)


@pytest.fixture
def numpy_device(monkeypatch):
    import _numpy_device
    from xmris_amd import device as dev

    _numpy_device.install(monkeypatch)
    calls = []

    def axis_dft(x, axis, table):
        return mrsi_orc.apply_table(x, axis, np.asarray(table)).astype(x.dtype)

    def l1_sense(*a):
        calls.append("l1_sense")
        return np_l1_sense(*a)

    def l1_lipschitz(*a):
        calls.append("l1_lipschitz")
        return np_l1_lipschitz(*a)

    monkeypatch.setattr(dev, "axis_sparse", np_axis_sparse)
    monkeypatch.setattr(dev, "axis_dft", axis_dft)
    monkeypatch.setattr(dev, "l1_sense", l1_sense)
    monkeypatch.setattr(dev, "l1_lipschitz", l1_lipschitz)
    return calls


def recon(c, y=None, iterations=10, tol=0.0, **kw):
    from xmris_amd import recon_l1_sense

    kw = dict(dict(tikhonov=c.reg, density=c.density, width=c.W, levels=c.levels), **kw)
    return recon_l1_sense(labeled(c.y if y is None else y, ("coil", "sample", "time")), c.traj, c.s, iterations=iterations,
                          tol=tol, **kw)


@pytest.mark.parametrize("dtype", ["complex128", "complex64"])
@pytest.mark.parametrize("name", PARITY)
def test_python_layer_reproduces_the_oracle_on_the_stand_in(numpy_device, name, dtype):
    """The operator, the mask, lambda2, the step from the power estimate and the levels the package assembles are the
    oracle's: 10 steps agree within L1_TOL."""
    c = orc.case(name)
    y = c.y.astype(dtype)
    img = recon(c, y)
    y128 = y.astype(np.complex128)
    want = orc.fista(c.dense(), c.rhs(y128), c.ms, c.levels, 0.02, tau_of(c), 10, mask=c.mask).x
    err = orc.rel(img.values.reshape(c.V, c.T), want)
    print(name, dtype, err)
    assert img.dims == ("x", "y", "z")[:len(c.ms)] + ("time",) and img.values.dtype == np.complex128
    assert err <= (L1_TOL64 if dtype == "complex64" else L1_TOL128)
    assert img.attrs["l1sense_step"] == pytest.approx(tau_of(c), rel=1e-6 if dtype == "complex64" else 1e-12)
    assert numpy_device == ["l1_lipschitz", "l1_sense"]
    if name == "masked2d":
        assert (~c.mask).sum() > 8 and np.all(img.values.reshape(c.V, c.T)[~c.mask] == 0)


def test_benefit_of_the_penalty(numpy_device, monkeypatch):
    """The undersampled 16 x 16 radial case (S / V = 0.75): the penalty more than halves the error of conjugate gradients
    with Tikhonov alone, and without the penalty there is no such gain."""
    from xmris_amd import device as dev
    from xmris_amd import recon_cg_sense

    c = orc.case("benefit")
    monkeypatch.setattr(dev, "cg_sense", np_cg_sense)
    la = labeled(c.y, ("coil", "sample", "time"))
    x_cg = recon_cg_sense(la, c.traj, c.s, iterations=30, tol=0.0, regularization=0.05, density="pipe").values
    e_cg = orc.error(x_cg.reshape(c.V, c.T), c.obj)
    e_l1 = orc.error(recon(c, iterations=100, sparsity=0.02).values.reshape(c.V, c.T), c.obj)
    e_off = orc.error(recon(c, iterations=100, sparsity=0.0).values.reshape(c.V, c.T), c.obj)
    print(f"benefit: cg {e_cg:.3f}  l1 {e_l1:.3f}  sparsity 0 {e_off:.3f}")
    assert e_l1 < e_cg and e_l1 < 0.5 * e_cg and e_off >= e_cg
    assert e_cg == pytest.approx(BENEFIT["cg"], rel=0.05) and e_l1 == pytest.approx(BENEFIT["l1"], rel=0.05)
    assert e_off == pytest.approx(BENEFIT["l1_off"], rel=0.05)


def test_chunks_zero_and_nan_columns_and_stopping(numpy_device):
    c = orc.case("radial2d", 5)
    whole = recon(c, return_info=True)
    img = whole["image"].values
    parts = recon(c, chunk=2, return_info=True)
    assert np.array_equal(parts["image"].values, img) and numpy_device.count("l1_sense") == 1 + 3
    assert np.array_equal(parts["change"].values, whole["change"].values)
    assert np.all(whole["iterations"].values == 10) and np.all(whole["status"].values == 0)
    z = c.y.copy()
    z[:, :, 1] = 0
    ds = recon(c, z, return_info=True)
    keep = [0, 2, 3, 4]
    assert np.all(ds["image"].values[..., 1] == 0) and ds["status"].values[1] == 1 and ds["iterations"].values[1] == 1
    assert ds["change"].values[1] == 0 and np.array_equal(ds["image"].values[..., keep], img[..., keep])
    z[1, 3, 1] = np.nan
    ds = recon(c, z, return_info=True)
    assert ds["status"].values[1] == 3 and np.all(np.isnan(ds["image"].values[..., 1])) and ds["iterations"].values[1] == 0
    assert np.array_equal(ds["image"].values[..., keep], img[..., keep]) and np.all(ds["status"].values[keep] == 0)
    # a tol that no step's change comes near: the columns stop where the oracle's ratios say
    ref = orc.fista(c.dense(), c.rhs(), c.ms, c.levels, 0.02, tau_of(c), 40, mask=c.mask)
    tol = 3e-3
    assert orc.clear_of(ref.ratios, tol)
    ds = recon(c, iterations=40, tol=tol, return_info=True)
    want = [next(k + 1 for k, r in enumerate(col) if r <= tol) for col in ref.ratios]
    assert ds["iterations"].values.tolist() == want and np.all(ds["status"].values == 1) and max(want) < 40
    assert np.all(ds["change"].values <= tol)
    # cycle spinning and a given step reach the library as given
    spun = recon(c, cycle_spin=True, step=0.5)
    want = orc.fista(c.dense(), c.rhs(), c.ms, c.levels, 0.02, 0.5, 10, mask=c.mask, cycle_spin=True).x
    assert orc.rel(spun.values.reshape(c.V, c.T), want) <= L1_TOL128 and spun.attrs["l1sense_step"] == 0.5
    assert orc.rel(spun.values, img) > 1e-3


def test_metadata_and_dataset_layout(numpy_device):
    from xmris_amd import ATTRS, LabeledArray
    from xmris_amd.fitting.dataset import LabeledDataset

    c = orc.case("radial2d", 6)
    y = c.y.reshape(c.C, c.S, 2, 3)
    la = labeled(y, ("coil", "sample", "rep", "time"), coil=np.arange(c.C), time=np.arange(3) * 1e-3, rep=np.arange(2),
                 readout=("sample", np.arange(c.S) * 2.0), label=("time", np.arange(3) * 10.0, {"units": "a.u."}))
    sens = LabeledArray(np.ascontiguousarray(np.moveaxis(c.s, 0, -1)), ("x", "y", "coil"), {}, {}, None)
    ds = la.xmr.recon_l1_sense(c.traj, sens, iterations=10, tol=0.0, sparsity=0.03, density="pipe", fov=(0.2, 0.25),
                               return_info=True)
    assert isinstance(ds, LabeledDataset) and set(ds.data_vars) == {"image", "change", "iterations", "status"}
    img = ds["image"]
    assert img.dims == ("x", "y", "rep", "time") and img.shape == (8, 8, 2, 3) and img.name == "fid"
    assert np.allclose(img.coords["x"].values, (np.arange(8) - 4) * 0.2 / 8)
    assert np.allclose(img.coords["y"].values, (np.arange(8) - 4) * 0.25 / 8)
    assert "readout" not in img.coords and "sample" not in img.coords and "coil" not in img.coords
    assert img.coords["label"].attrs == {"units": "a.u."} and np.array_equal(img.coords["time"].values, la.coords["time"].values)
    beta = grid_orc.beta_of(4, 2.0)
    tau = tau_of(c, lam=0.0)
    own = {k: img.attrs[k] for k in (ATTRS.l1sense_step, ATTRS.l1sense_lipschitz)}
    assert own[ATTRS.l1sense_step] == pytest.approx(tau, rel=1e-12) and own[ATTRS.l1sense_lipschitz] == pytest.approx(1 / tau, rel=1e-12)
    assert img.attrs == {"note": "kept", ATTRS.grid_dims: ("x", "y"), ATTRS.grid_matrix: (8, 8), ATTRS.grid_oversampled: (16, 16),
                         ATTRS.grid_width: 4, ATTRS.grid_beta: (beta, beta), ATTRS.grid_density: "pipe",
                         ATTRS.l1sense_sparsity: 0.03, ATTRS.l1sense_levels: (2, 2), ATTRS.l1sense_iterations: 10,
                         ATTRS.l1sense_tol: 0.0, **own}
    assert ds.attrs == img.attrs and la.attrs == {"note": "kept"} and la.dims == ("coil", "sample", "rep", "time")
    for name, kind in (("change", np.float64), ("iterations", np.int32), ("status", np.int32)):
        v = ds[name]
        assert v.dims == ("rep", "time") and v.shape == (2, 3) and v.values.dtype == kind and set(v.coords) == {"rep", "time", "label"}
    M0 = c.normal_matrix(0.0)  # (tikhonov is 0 in this call)
    want = orc.fista(lambda v: M0 @ v, c.rhs(), c.ms, (2, 2), 0.03, tau, 10, mask=c.mask).x.reshape(8, 8, 2, 3)
    assert orc.rel(img.values, want) <= L1_TOL128
    from xmris_amd import recon_l1_sense

    named = recon_l1_sense(labeled(y, ("coil", "shot", "rep", "time")), c.traj, c.s, matrix=(8, 8), iterations=10, tol=0.0,
                           sparsity=0.03, density="pipe", dim="shot", out_dim=("u", "v"), levels=2)
    assert named.dims == ("u", "v", "rep", "time") and np.array_equal(named.values, img.values)
    one = recon_l1_sense(labeled(c.y[:, :, 0], ("coil", "sample")), c.traj, c.s, iterations=10, tol=0.0, sparsity=0.03,
                         density="pipe", return_info=True)
    assert one["image"].dims == ("x", "y") and one["status"].dims == () and np.array_equal(one["image"].values, img.values[:, :, 0, 0])


def test_dataarray_bridge(numpy_device, monkeypatch):
    import _fake_xarray

    xr = _fake_xarray.install(monkeypatch)
    import xmris_amd

    xmris_amd.register_xarray_accessor(force=True)
    c = orc.case("line1d")
    da = xr.DataArray(c.y, dims=("coil", "sample", "time"), coords={"time": np.arange(3.0)}, attrs={"a": 1}, name="k")
    out = xmris_amd.recon_l1_sense(da, c.traj, c.s, width=6)
    assert type(out) is xr.DataArray and out.dims == ("x", "time") and out.name == "k" and out.attrs["a"] == 1
    assert np.array_equal(da.xmr.recon_l1_sense(c.traj, c.s, width=6).values, out.values)


# ---- validation: every error fires before any native call -----------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    from xmris_amd import _lib
    from xmris_amd import device as dev

    def boom(*a, **k):
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "call", boom)
    for name in ("to_device", "axis_sparse", "axis_dft", "phase_apply", "zero_fill", "fft", "l1_sense", "l1_lipschitz", "l1_start",
                 "l1_prox", "cgs_expand", "cgs_reduce", "shift_time"):
        monkeypatch.setattr(dev, name, boom)


TRAJ = grid_orc.random(6, 37, 2, 1)
SENS = cgs_orc.maps((6, 6), 3)


@pytest.mark.parametrize("kw, word", [
    (dict(iterations=-1), "iterations"),
    (dict(iterations=2.0), "iterations"),
    (dict(iterations=True), "iterations"),
    (dict(power_iterations=-1), "power_iterations"),
    (dict(power_iterations=1.5), "power_iterations"),
    (dict(tol=-1e-3), "tol"),
    (dict(tol=float("nan")), "tol"),
    (dict(sparsity=-0.1), "sparsity"),
    (dict(sparsity=float("inf")), "sparsity"),
    (dict(sparsity="some"), "sparsity"),
    (dict(tikhonov=-0.1), "tikhonov"),
    (dict(tikhonov=float("nan")), "tikhonov"),
    (dict(step=0.0), "step"),
    (dict(step=-1.0), "step"),
    (dict(step=float("inf")), "step"),
    (dict(step_safety=0.0), "step_safety"),
    (dict(step_safety=float("nan")), "step_safety"),
    (dict(cycle_spin=1), "cycle_spin"),
    (dict(levels=(1,)), "levels"),
    (dict(levels=(1, 1, 1)), "levels"),
    (dict(levels=(-1, 1)), "levels"),
    (dict(levels=(1.0, 1)), "levels"),
    (dict(levels=(2, 1)), "not divisible"),  # 6 = 2 x 3
    (dict(levels=2), "not divisible"),
    (dict(levels=(3, 2), sensitivities=cgs_orc.maps((8, 8), 3), trajectory=grid_orc.random(8, 37, 2, 1)), "16"),
    (dict(sensitivities=SENS[:2]), "sensitivities"),
    (dict(sensitivities=SENS[0]), "sensitivities"),
    (dict(matrix=(6, 5)), "matrix"),
    (dict(noise_cov=np.eye(2)), "noise_cov"),
    (dict(chunk=0), "chunk"),
    (dict(chunk=1.5), "chunk"),
    (dict(coil_dim="sample"), "coil_dim"),
    (dict(trajectory=TRAJ[:30]), "trajectory"),
    (dict(width=9), "width"),
    (dict(oversampling=0.9), "oversampling"),
    (dict(density="voronoi"), "density"),
    (dict(out_dim=("x", "time")), "out_dim"),
    (dict(fov=0.0), "fov"),
])
def test_validation_errors_name_their_argument(no_library, kw, word):
    from xmris_amd import recon_l1_sense

    la = labeled(grid_orc.make((3, 37, 4), seed=1), ("coil", "sample", "time"))
    args = dict(dict(trajectory=TRAJ, sensitivities=SENS), **kw)
    with pytest.raises(ValueError, match=word):
        recon_l1_sense(la, **args)
    with pytest.raises(ValueError, match=word):
        la.xmr.recon_l1_sense(**args)


def test_validation_of_dims(no_library):
    from xmris_amd import recon_l1_sense

    la = labeled(grid_orc.make((3, 37, 4), seed=1), ("coil", "sample", "time"))
    with pytest.raises(ValueError, match=r"Method 'recon_l1_sense' attempted to operate on missing dimension\(s\): \['shot'\]"):
        recon_l1_sense(la, TRAJ, SENS, dim="shot")
    with pytest.raises(TypeError):
        recon_l1_sense(np.zeros((3, 37), complex), TRAJ, SENS)


# ---- the C ABI ----------------------------------------------------------------------------------------------------------
def test_c_abi_refusals_without_gpu():
    import ctypes

    from xmris_amd import _lib

    _refusals("xm_l1_start", orc.START_ORDER, orc.START_OK, orc.START_REFUSALS, "l1_start")
    lib = _lib.load()
    ptrs = orc.PROX_ORDER[:14]
    for change in orc.PROX_REFUSALS:
        a = dict(orc.PROX_OK)
        for k, v in change.items():
            a[k] = orc.PROX_OK[v] if isinstance(v, str) else (orc.PROX_OK[k] + v if k in ptrs and isinstance(v, int) else v)
        args = [ctypes.c_double(a[k]) if k in orc.PROX_DOUBLES else a[k] for k in orc.PROX_ORDER] + [None]
        assert lib.xm_l1_prox(*args) == _lib.XM_ERR_INVALID_ARG, change
        assert b"l1_prox" in lib.xm_last_error_string()


def test_vocabulary_and_exports():
    import xmris_amd
    from xmris_amd import ATTRS, processing

    for name in ("sparsity", "levels", "iterations", "tol", "step", "lipschitz"):
        assert getattr(ATTRS, "l1sense_" + name) == "l1sense_" + name
    assert xmris_amd.recon_l1_sense is processing.recon_l1_sense
    assert "recon_l1_sense" in xmris_amd.__all__ and "recon_l1_sense" in processing.__all__
    assert hasattr(xmris_amd.XmrisAccessor, "recon_l1_sense")
    assert "xm_l1_start" in xmris_amd._lib.SIGNATURES and "xm_l1_prox" in xmris_amd._lib.SIGNATURES
    assert xmris_amd.device.L1_MAX_BLOCK == 16 and xmris_amd.device.l1_blocks((8, 6), (2, 1)) == 6
    assert processing.l1sense.STEP_SAFETY == STEP_SAFETY
    assert xmris_amd.device.fista_momentum(3) == orc.momentum(3)
