"""CPU tests: the C-ABI library loads and exports every symbol of include/xmris_hip.h, argument
validation works without a GPU, and the host layer reproduces the reference's metadata semantics
(checked against the oracle with a numpy test double standing in for the device kernels)."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    from xmris_amd import _lib

    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "xmris_hip.h")).read()
    declared = set(re.findall(r"\b(xm_[a-z0-9_]+)\s*\(", header))
    declared -= {"xm_fft_supported)"}  # (none) keep the regex honest
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.xm_version() >= 100


def test_plan_predicates_without_gpu():
    from xmris_amd import _lib

    lib = _lib.load()
    for n in (2, 16, 512, 1024, 2048, 4096, 8192, 1536, 3072, 640, 1531, 1000, 4095):
        assert lib.xm_fft_supported(n, _lib.XM_C64) == 1, n
    assert lib.xm_fft_supported(16384, _lib.XM_C64) == 1
    assert lib.xm_fft_supported(16384, _lib.XM_C128) == 1  # four-step over global memory (xm_bigfft.inc)
    assert lib.xm_fft_supported(65536, _lib.XM_C128) == 1 and lib.xm_fft_supported(10007, _lib.XM_C128) == 1
    assert lib.xm_fft_supported((1 << 22) + 1, _lib.XM_C64) == 0
    assert lib.xm_fft_supported(9001, _lib.XM_C64) == 1  # chirp-z of length 32768 on top of the four-step path
    assert lib.xm_fft_supported(0, _lib.XM_C64) == 0


def test_invalid_arguments_return_status_not_crash():
    from xmris_amd import _lib

    lib = _lib.load()
    # null pointers / bad geometry are rejected before any HIP call is made
    assert lib.xm_zero_fill(None, None, 4, 8, 16, 0, _lib.XM_C64, None) == _lib.XM_ERR_INVALID_ARG
    assert lib.xm_pipeline_fused(None, 8, None, None, None, 1, 8, 4, 0, 0, None, None, _lib.XM_C64, None) \
        == _lib.XM_ERR_INVALID_ARG
    assert lib.xm_fft1d_batched(8, 16, 1, (1 << 22) + 1, 0, _lib.XM_C64, None) == _lib.XM_ERR_UNSUPPORTED_N
    assert b"4194305" in lib.xm_last_error_string()
    assert lib.xm_apodize(1, 1, 1, 1, 8, 7, None) == _lib.XM_ERR_INVALID_ARG  # bad dtype
    with pytest.raises(_lib.XmrisHipError):
        _lib.call("xm_roll", 1, 1, 1, 8, 1, _lib.XM_C64, None)  # in == out


def test_no_cpu_fallback():
    import torch

    from xmris_amd import device

    with pytest.raises(RuntimeError, match="no CPU path"):
        device.fft(torch.zeros(2, 8, dtype=torch.complex64), 1)


# ---------------------------------------------------------------------------------------------
# host metadata logic vs the oracle (device kernels replaced by the numpy test double)
# ---------------------------------------------------------------------------------------------
@pytest.fixture
def host(monkeypatch):
    import _numpy_device

    import xmris_amd

    _numpy_device.install(monkeypatch)
    return xmris_amd


def _same(a, o, phase_tol=0.0):
    """xmris_amd.LabeledArray `a` vs oracle.Labeled `o`: dims, coords (values + attrs), attrs, name.
    phase_tol > 0: the solver's (p0, p1) attrs and the phased values are compared approximately (the
    product's objectives are native code: equal to the numpy ones to rounding, not bit for bit, and the
    ROI scores are non-smooth, so their polished optimum moves by ~1e-4 degrees)."""
    assert a.dims == o.dims
    assert set(a.coords) == set(o.coords)
    for k in o.coords:
        assert a.coords[k].dim == o.coords[k].dim
        np.testing.assert_array_equal(a.coords[k].values, o.coords[k].values)
        assert a.coords[k].attrs == o.coords[k].attrs, k
    if phase_tol:
        assert set(a.attrs) == set(o.attrs)
        for k, v in o.attrs.items():
            if k in ("phase_p0", "phase_p1"):
                assert abs(a.attrs[k] - v) < phase_tol, (k, a.attrs[k], v)
            else:
                assert a.attrs[k] == v, k
        np.testing.assert_allclose(a.values, o.values, rtol=0, atol=phase_tol * np.abs(o.values).max())
    else:
        assert a.attrs == o.attrs
        np.testing.assert_allclose(a.values, o.values, rtol=1e-12, atol=1e-12)
    assert a.name == o.name


def _pair(host, oracle, values, dims, coords, attrs, name=None):
    a = host.LabeledArray(values, dims, coords, attrs, name)
    o = oracle.Labeled(values, dims, {k: oracle.Coord(k, np.asarray(v)) for k, v in coords.items()}, dict(attrs), name)
    return a, o


def test_quickstart_chain_metadata(host, oracle):
    rng = np.random.default_rng(42)
    t = np.linspace(0, 1, 1024)
    x = rng.standard_normal((5, 1024)) + 1j * rng.standard_normal((5, 1024))
    a, o = _pair(host, oracle, x, ("voxel", "time"), {"voxel": np.arange(5), "time": t}, {"MHz": 120.0, "sw": 10000.0})
    a1, o1 = a.xmr.zero_fill(target_points=2048), oracle.zero_fill(o, target_points=2048)
    _same(a1, o1)
    a2, o2 = a1.xmr.apodize_exp(lb=5.0), oracle.apodize_exp(o1, lb=5.0)
    _same(a2, o2)
    a3, o3 = a2.xmr.to_spectrum(), oracle.to_spectrum(o2)
    _same(a3, o3)
    assert a3.coords["frequency"].attrs == {"long_name": "Frequency", "units": "Hz"}
    a4 = a3.xmr.phase(p0=30.0, p1=-60.0)
    o4 = oracle.phase(o3, p0=30.0, p1=-60.0)
    _same(a4, o4)
    assert "zero_fill_target" not in a.attrs  # inputs never mutated
    # no-op zero fill: plain copy, no lineage (fid.py:235-236)
    _same(a.xmr.zero_fill(target_points=512), oracle.zero_fill(o, target_points=512))
    # symmetric on another axis + custom dim keeps the old coord attrs
    b = host.LabeledArray(x[:, :32], ("ky", "kx"), {"kx": host.Coordinate("kx", np.linspace(-16, 15, 32), {"u": 1})})
    ob = oracle.Labeled(x[:, :32], ("ky", "kx"), {"kx": oracle.Coord("kx", np.linspace(-16, 15, 32), {"u": 1})})
    _same(b.xmr.zero_fill(dim="kx", target_points=128, position="symmetric"),
          oracle.zero_fill(ob, dim="kx", target_points=128, position="symmetric"))


def test_fourier_family_metadata(host, oracle):
    rng = np.random.default_rng(1)
    for n in (8, 7):
        x = rng.standard_normal((3, n)) + 1j * rng.standard_normal((3, n))
        a, o = _pair(host, oracle, x, ("rep", "time"), {"time": np.arange(n) * 0.5}, {"k": 1})
        _same(a.xmr.fft(), oracle.fft(o))
        _same(a.xmr.fft(out_dim="frequency"), oracle.fft(o, out_dim="frequency"))
        _same(a.xmr.fft(out_dim="f"), oracle.fft(o, out_dim="f"))
        s, so = a.xmr.to_spectrum(), oracle.to_spectrum(o)
        _same(s, so)
        _same(s.xmr.to_fid(), oracle.to_fid(so))
        _same(s.xmr.ifft(), oracle.ifft(so))
        _same(a.xmr.fftshift("time"), oracle.fftshift(o, "time"))
        _same(a.xmr.ifftshift("time"), oracle.ifftshift(o, "time"))
        _same(a.xmr.fftc(out_dim="frequency"), oracle.fftc(o, out_dim="frequency"))
        _same(s.xmr.ifftc(out_dim="time"), oracle.ifftc(so, out_dim="time"))
    k = np.linspace(-4, 3, 8)
    y = rng.standard_normal((8, 8)) + 0j
    a, o = _pair(host, oracle, y, ("kx", "ky"), {"kx": k, "ky": k}, {})
    _same(a.xmr.ifftc(dim=["kx", "ky"], out_dim=["x", "y"]), oracle.ifftc(o, dim=["kx", "ky"], out_dim=["x", "y"]))
    with pytest.raises(ValueError, match="same length"):
        a.xmr.fft(dim=["kx", "ky"], out_dim=["x"])


def test_errors_match_reference_wording(host, oracle):
    a = host.LabeledArray(np.zeros(4, complex), ("x",), {"x": np.arange(4)})
    for call, name in [(lambda: a.xmr.zero_fill(), "zero_fill"), (lambda: a.xmr.apodize_exp(), "apodize_exp"),
                       (lambda: a.xmr.to_spectrum(), "to_spectrum"), (lambda: a.xmr.autophase(), "autophase"),
                       (lambda: a.xmr.phase(), "phase"), (lambda: a.xmr.fft(), "fft"),
                       (lambda: a.xmr.fftshift("time"), "fftshift")]:
        with pytest.raises(ValueError) as e:
            call()
        msg = str(e.value)
        assert f"Method '{name}'" in msg and "missing dimension" in msg and "['x']" in msg and "rename" in msg
        assert "attempted to operate on" in msg and "Available dimensions are" in msg  # core/utils.py:14-21
    with pytest.raises(ValueError, match="`position` must be either 'end' or 'symmetric'."):
        a.xmr.zero_fill(dim="x", target_points=16, position="middle")
    b = host.LabeledArray(np.zeros((2, 4), complex), ("v", "time"))  # no time coordinate
    with pytest.raises(KeyError):
        b.xmr.apodize_exp()
    with pytest.raises(KeyError):
        b.xmr.to_spectrum()
    s = host.LabeledArray(np.ones((2, 4), complex), ("v", "frequency"), {"frequency": np.arange(4.0)})
    with pytest.raises(NotImplementedError, match="is not yet implemented"):
        s.xmr.autophase(mode="all")
    with pytest.raises(ValueError, match="Mode must be 'single' or 'all'."):
        s.xmr.autophase(mode="some")
    with pytest.raises(ValueError, match="Method must be 'acme', 'peak_minima', or 'positivity'"):
        s.xmr.autophase(method="nope")


def test_accessor_defaults_contract(host):
    """tests/test_core.py:497-552 of the reference: default arguments of the accessor methods."""
    import inspect

    acc = host.XmrisAccessor
    sig = lambda f: {k: v.default for k, v in inspect.signature(f).parameters.items() if k != "self"}  # noqa: E731
    assert sig(acc.zero_fill) == {"dim": "time", "target_points": 1024, "position": "end"}
    assert sig(acc.apodize_exp) == {"dim": "time", "lb": 1.0}
    assert sig(acc.apodize_lg) == {"dim": "time", "lb": 1.0, "gb": 1.0}
    assert sig(acc.to_spectrum) == {"dim": "time", "out_dim": "frequency"}
    assert sig(acc.to_fid) == {"dim": "frequency", "out_dim": "time"}
    assert sig(acc.phase) == {"dim": "frequency", "p0": 0.0, "p1": 0.0, "pivot": None}
    ap = sig(acc.autophase)
    assert (ap["dim"], ap["method"], ap["peak_width"], ap["lb"], ap["temp_time_dim"]) == \
        ("frequency", "acme", 100, 0.0, "time")
    assert sig(acc.fft) == {"dim": "time", "out_dim": None}
    assert sig(acc.ifft) == {"dim": "frequency", "out_dim": None}
    assert host.DIMS.time == "time" and host.COORDS.frequency.unit == "Hz"
    assert host.ATTRS.phase_pivot_coord == "phase_pivot_coord" and host.COORDS.chemical_shift.long_name == "Chemical Shift"


def test_autophase_and_phase_warning(host, oracle):
    n, sw = 512, 2000.0
    t = np.arange(n) / sw
    rng = np.random.default_rng(3)
    rows = [a * np.exp(-20 * t) * np.exp(2j * np.pi * 150 * t) + 0.05 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
            for a in (1.0, 3.0, 2.0)]
    a, o = _pair(host, oracle, np.stack(rows), ("rep", "time"), {"time": t, "rep": np.arange(3)}, {"seq": "x"})
    s, so = a.xmr.to_spectrum(), oracle.to_spectrum(o)
    r = s.xmr.autophase(method="positivity", peak_width=50.0)
    ro = oracle.autophase(so, method="positivity", peak_width=50.0)
    _same(r, ro, phase_tol=1e-2)
    r = s.xmr.autophase(p0_only=True, target_coord=150.0, lb=2.0)  # accessor default peak_width=100, acme
    ro = oracle.autophase(so, peak_width=100, p0_only=True, target_coord=150.0, lb=2.0)
    _same(r, ro, phase_tol=1e-6)
    assert r.attrs["phase_p1"] == 0.0 and r.attrs["phase_pivot"] == 150.0
    ppm = host.LabeledArray(r.values, ("rep", "chemical_shift"),
                            {"chemical_shift": r.coords["frequency"].values / 100.0}, r.attrs)
    with pytest.warns(UserWarning, match="previous phase operations"):
        ppm.xmr.phase(dim="chemical_shift", p0=1.0, pivot=0.0)


def test_sharding_helpers():
    from xmris_amd import sharding

    assert [sharding.shard_bounds(10, 4, r) for r in range(4)] == [(0, 2), (2, 5), (5, 7), (7, 10)]
    assert sharding.pick_winner([(1.0, 50), (3.0, 999), (3.0, 120), (2.0, 1)]) == (2, 120, 3.0)
    assert sharding.exchange_argmax(2.5, 77) == (0, 77, 2.5)
    assert sharding.broadcast_params([1.0, 2.0], 0) == [1.0, 2.0]


def test_native_solver_replicates_scipy_differential_evolution():
    """libxmris_hip.so's host solver (xm_solver_de) visits exactly the trial vectors scipy's
    DifferentialEvolutionSolver does (numpy RandomState(42) stream, latin hypercube, best1bin,
    immediate updating, std/mean convergence): same x, fun, nfev -- bit for bit -- as
    scipy.optimize.differential_evolution driven by the same native objective; and on the golden ACME
    slice it lands on the same (p0, p1) as the numpy-objective route the reference takes."""
    import scipy.optimize

    from xmris_amd import autophase_solver as aps

    g = np.load(os.path.join(ROOT, "tests", "golden", "scores.npz"))
    c3 = np.load(os.path.join(ROOT, "tests", "golden", "c3_three_peak.npz"))
    sl, fr, pv, ti, iw = g["slice"], g["freq"], float(g["pivot"]), int(g["target_idx"]), int(g["index_width"])
    for i, p in enumerate(g["points"]):  # native objectives == numpy objectives to rounding
        for m, ref in (("acme", g["acme"][i]), ("peak_minima", g["peak_minima"][i]), ("positivity", g["positivity"][i])):
            assert aps.NativeObjective(sl, fr, pv, ti, iw, m)(p) == pytest.approx(ref, rel=1e-12, abs=1e-15)
    for method in aps.METHODS:
        for p0_only in (False, True):
            # (polish="native": scipy's L-BFGS-B core on the SAME native objective scipy is driven with below)
            p0, p1, opt = aps.solve(sl, fr, pv, ti, iw, method=method, p0_only=p0_only, polish="native")
            obj = aps.NativeObjective(sl, fr, pv, ti, iw, method)
            bounds = [(-180.0, 180.0)] if p0_only else [(-180.0, 180.0), (-4000.0, 4000.0)]
            r = scipy.optimize.differential_evolution(obj, bounds=bounds, strategy="best1bin", tol=0.01, seed=42)
            assert np.array_equal(r.x, opt.x) and r.fun == opt.fun and r.nfev == opt.nfev, (method, p0_only)
            assert p1 == (0.0 if p0_only else opt.x[1])
    p0, p1, _ = aps.solve(sl, fr, pv, ti, iw)
    q0, q1, _ = aps.solve(sl, fr, pv, ti, iw, engine="scipy")
    assert p0 == q0 and p1 == q1  # polish="exact": the reference's route wherever the polish does anything
    assert abs(p0 - float(c3["p0"])) < 1e-9 and abs(p1 - float(c3["p1"])) < 1e-9
    # thread count does not change the objective value (fixed-order chunk sums)
    obj = aps.NativeObjective(sl, fr, pv, ti, iw, "acme")
    vals = []
    for thr in (1, 2, 0):
        obj.set_threads(thr)
        vals.append(obj([12.5, -321.0]))
    assert vals[0] == vals[1] == vals[2]


def test_native_solver_speculative_batches_do_not_change_the_search():
    """xm_solver_de evaluates up to XM_SOLVER_BATCH trials speculatively per hand-off and commits them in
    scipy's order: x, fun, nfev and nit must not depend on the batch size (1 = the sequential schedule) nor
    on the team size, and xm_solver_score_batch must return xm_solver_score's values."""
    from xmris_amd import autophase_solver as aps

    g = np.load(os.path.join(ROOT, "tests", "golden", "scores.npz"))
    sl, fr, pv, ti, iw = g["slice"], g["freq"], float(g["pivot"]), int(g["target_idx"]), int(g["index_width"])
    old = os.environ.get("XM_SOLVER_BATCH")
    try:
        for method in aps.METHODS:
            runs = []
            for batch, threads in ((1, 1), (4, 0), (7, 3), (30, 0)):
                os.environ["XM_SOLVER_BATCH"] = str(batch)  # read when the solver handle is created
                obj = aps.NativeObjective(sl, fr, pv, ti, iw, method)
                obj.set_threads(threads)
                for p0_only in (False, True):
                    before = obj.evaluations()
                    rc, x, fun, nfev, nit = obj.de(p0_only)
                    assert obj.evaluations() - before >= nfev
                    runs.append((batch, p0_only, rc, tuple(x), fun, nfev, nit))
            ref = {r[1]: r[2:] for r in runs if r[0] == 1}
            for r in runs:
                assert r[2:] == ref[r[1]], (method, r[0], r[1])
            obj = aps.NativeObjective(sl, fr, pv, ti, iw, method)
            pts = np.array([[12.5, -321.0], [-170.0, 3999.0], [0.0, 0.0], [33.3, 47.1], [179.0, -3999.0]])
            assert np.array_equal(obj.score_batch(pts), np.array([obj(p) for p in pts]))
    finally:
        if old is None:
            os.environ.pop("XM_SOLVER_BATCH", None)
        else:
            os.environ["XM_SOLVER_BATCH"] = old


def test_native_acme_objective_on_a_non_uniform_axis_and_ragged_lengths():
    """The ACME objective has two code paths: the rotation recurrence for a uniformly spaced coordinate (what
    the path produces) and per-sample sin/cos for any other coordinate; the last 256-sample chunk may be
    ragged.  Both must match the numpy objective (phasing.py:100-122)."""
    from xmris_amd import autophase_solver as aps

    rng = np.random.default_rng(3)
    for n in (2, 17, 255, 256, 257, 1531, 2048, 4099):
        sl = rng.standard_normal(n) + 1j * rng.standard_normal(n)
        uniform = np.roll(np.fft.fftfreq(n, d=2e-4), n // 2)
        warped = uniform + 3.0 * np.sin(np.arange(n))  # same range order, not evenly spaced
        for coords in (uniform, warped):
            k = int(np.argmax(np.abs(sl)))
            obj = aps.NativeObjective(sl, coords, float(coords[k]), k, 1, "acme")
            for p in ([0.0, 0.0], [12.5, -321.0], [-170.0, 3999.0], [179.0, -3999.0]):
                ref = aps.acme_score(p, sl, coords, float(coords[k]))
                assert obj(p) == pytest.approx(ref, rel=2e-12, abs=1e-15), (n, p)


def test_xarray_bridge_through_a_test_double(oracle, monkeypatch):
    """The xarray face of the drop-in (reference core/accessor.py:691-710 registers `.xmr` on xr.DataArray): with a
    module named `xarray` in place (tests/_fake_xarray.py -- the real one is not installed here),
    register_xarray_accessor / as_labeled / like_input and a chained `.xmr` call must take and return DataArrays with
    the reference's dims, coords (incl. attrs), lineage attrs and name; multi-dimensional coordinates are refused
    loudly instead of being dropped."""
    import _fake_xarray
    import _numpy_device

    import xmris_amd as xm
    from xmris_amd import accessor, labeled

    xr = _fake_xarray.install(monkeypatch)
    _numpy_device.install(monkeypatch)
    assert accessor.register_xarray_accessor() is True
    assert accessor.register_xarray_accessor() is False  # the name is taken now (e.g. by the reference package)
    assert accessor.register_xarray_accessor(force=True) is True
    rng = np.random.default_rng(3)
    t = np.linspace(0, 1, 64)
    x = rng.standard_normal((3, 64)) + 1j * rng.standard_normal((3, 64))
    da = xr.DataArray(x, dims=("voxel", "time"), coords={"time": xr.Variable("time", t, {"units": "s"}), "voxel": [10, 11, 12]},
                      attrs={"B0": 3.0}, name="fid")
    assert labeled.is_xarray(da) and isinstance(da.xmr, accessor.XmrisAccessor)
    got = da.xmr.zero_fill(target_points=128).xmr.apodize_exp(lb=5.0).xmr.to_spectrum()
    assert isinstance(got, xr.DataArray), "xarray in -> xarray out"
    ref = oracle.to_spectrum(oracle.apodize_exp(oracle.zero_fill(
        oracle.Labeled(x, ("voxel", "time"), {"time": oracle.Coord("time", t, {"units": "s"}),
                                              "voxel": oracle.Coord("voxel", np.array([10, 11, 12]))}, {"B0": 3.0}, "fid"),
        target_points=128), lb=5.0))
    assert got.dims == ref.dims and got.attrs == ref.attrs and got.name == ref.name
    np.testing.assert_allclose(got.values, ref.values, rtol=0, atol=1e-12 * np.abs(ref.values).max())
    assert set(got.coords) == set(ref.coords)
    for k, c in ref.coords.items():
        np.testing.assert_array_equal(got.coords[k].values, c.values)
        assert got.coords[k].attrs == c.attrs and got.coords[k].dims == (c.dim,)
    assert da.attrs == {"B0": 3.0} and da.values is not got.values  # the input is untouched
    # SURVEY 8f rank 2 on the reference's own container: every step of the chain came back as a DataArray around a
    # duck array (xarray's protocol: `is_duck_array`) that is still a RECORDED step -- shape / dtype / coords / attrs
    # known, nothing computed -- and `.values` / numpy functions / arithmetic compute it
    z = da.xmr.zero_fill(target_points=128)
    assert isinstance(z, xr.DataArray) and isinstance(z.data, labeled.LazyDuck) and xr.is_duck_array(z.data)
    assert z.data.node.is_deferred and z.shape == (3, 128) and z.dtype == np.complex128 and z.attrs["zero_fill_target"] == 128
    a2 = z.xmr.apodize_exp(lb=5.0)
    assert isinstance(a2.data, labeled.LazyDuck) and a2.data.node.is_deferred
    steps, chain_root = a2.data.node.pending_chain()
    assert [s_[0] for s_ in steps] == ["apodize_exp", "zero_fill"] and not chain_root.is_deferred  # ONE chain across the DataArrays
    assert z.data.node.is_deferred  # ... and asking for the later step did not compute the earlier one's DataArray
    np.testing.assert_allclose(np.abs(a2.data).max(), np.abs(oracle.apodize_exp(oracle.zero_fill(
        oracle.Labeled(x, ("voxel", "time"), {"time": oracle.Coord("time", t)}), target_points=128), lb=5.0).values).max(), rtol=1e-12)
    assert np.asarray(z.data).shape == (3, 128) and (z.data + 0).dtype == np.complex128 and z.data[0, :4].shape == (4,)
    # an edit on an intermediate DataArray is honoured by the next call (the chain takes the DataArray's metadata)
    z.attrs["note"] = "edited"
    assert z.xmr.apodize_exp(lb=5.0).attrs["note"] == "edited"
    monkeypatch.setenv("XMRIS_AMD_XARRAY_EAGER", "1")
    assert isinstance(da.xmr.zero_fill(target_points=128).data, np.ndarray)
    monkeypatch.delenv("XMRIS_AMD_XARRAY_EAGER")
    # functions take DataArrays too, and hand back the caller's container type
    assert isinstance(xm.to_spectrum(da), xr.DataArray)
    assert isinstance(xm.to_spectrum(labeled.as_labeled(da)), xm.LabeledArray)
    bad = xr.DataArray(x, dims=("voxel", "time"), coords={"time": t, "pos": xr.Variable(("voxel", "time"), x.real)})
    with pytest.raises(NotImplementedError, match="spans 2 dimensions"):
        bad.xmr.to_spectrum()
    with pytest.raises(TypeError):
        labeled.as_labeled(np.zeros(3))


def _sweep_spectrum(aps, seed):
    """Spectrum `seed` of the divergence sweep: (spectrum, frequency axis, pivot, arg-max index, index width)."""
    n, sw = 2048, 5000.0
    t = np.arange(n) / sw
    freq = np.roll(np.fft.fftfreq(n, d=1 / sw), n // 2)
    rng = np.random.default_rng(1000 + seed)
    k = int(rng.integers(3, 6))
    fid = np.zeros(n, complex)
    for _ in range(k):
        fid += rng.uniform(0.3, 1.0) * np.exp(-rng.uniform(15.0, 60.0) * t) * np.exp(2j * np.pi * rng.uniform(-2000, 2000) * t)
    fid += 0.01 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    spec = np.roll(np.fft.fft(fid * np.exp(-np.pi * 3.0 * t), norm="ortho"), n // 2)
    kmax = int(np.argmax(np.abs(spec)))
    pivot = float(freq[kmax])
    spec = spec * np.exp(1j * aps.phase_angles(freq, rng.uniform(-150, 150), rng.uniform(-600, 600), pivot))
    return spec, freq, pivot, kmax, aps.index_width_of(freq, 100)


def test_native_search_vs_scipy_divergence_sweep():
    """How often does the native search end somewhere else than the reference's route
    (scipy.optimize.differential_evolution on the numpy objective, phasing.py:276-284)?  60 seeded spectra of 3-5
    Lorentzian lines with a random (p0, p1) distortion and noise, three scores.

    The generations are the same search evaluation for evaluation (equal nfev).  scipy's final L-BFGS-B polish
    usually does nothing -- the projected gradient at the best member is below pgtol, nit = 0, the member is kept --
    and the default polish="exact" makes that test natively and hands every search that does NOT pass it to the
    reference's own route (scipy's minimiser on the numpy objective).  So, accepted polishes included:
      * ACME: (p0, p1) within 1e-4 degrees of the reference's route in EVERY case (round 3, native polish: up to
        8e-4 / 4e-3 degrees where a polish iterated), identical wherever no polish ran;
      * the two piecewise ROI scores (min over a window / sums over sign sets: plateaus and kinks -- whole regions
        score exactly 0, ties between members decide the generations, "the same parameters" is not defined) are held
        to SURVEY section 7.3 contract (iii): an objective no worse than scipy's, to 1e-7 relative.
    polish="native" (what round 3's streaming executor ran) is measured beside it and only held to contract (iii)."""
    from xmris_amd import autophase_solver as aps

    stats = {m: dict(n=0, identical=0, polished=0, route_numpy=0, dp0=0.0, dp1=0.0, dfun=0.0, native_dp0=0.0, native_dp1=0.0)
             for m in aps.METHODS}
    for seed in range(60):
        spec, freq, pivot, kmax, iw = _sweep_spectrum(aps, seed)
        method = aps.METHODS[seed % 3]
        p0n, p1n, on = aps.solve(spec, freq, pivot, kmax, iw, method=method, engine="native")  # polish="exact"
        p0s, p1s, os_ = aps.solve(spec, freq, pivot, kmax, iw, method=method, engine="scipy")
        p0v, p1v, ov = aps.solve(spec, freq, pivot, kmax, iw, method=method, engine="native", polish="native")
        st = stats[method]
        dp0, dp1 = abs(p0n - p0s), abs(p1n - p1s)
        floor = 1e-12 * float(np.abs(spec).max())  # (the ROI scores are in data units and can be exactly 0)
        dfun = (on.fun - os_.fun) / max(abs(os_.fun), floor * 1e7)
        st["n"] += 1
        st["identical"] += int(dp0 == 0.0 and dp1 == 0.0)
        st["polished"] += int(bool(on.get("polished")))
        st["route_numpy"] += int(on.get("polish_route") == "numpy")
        st["dp0"], st["dp1"], st["dfun"] = max(st["dp0"], dp0), max(st["dp1"], dp1), max(st["dfun"], dfun)
        st["native_dp0"], st["native_dp1"] = max(st["native_dp0"], abs(p0v - p0s)), max(st["native_dp1"], abs(p1v - p1s))
        if method == "acme":
            assert on.nfev == os_.nfev, (seed, method, on.nfev, os_.nfev)
            assert dp0 < 1e-4 and dp1 < 1e-4, (seed, method, p0n, p0s, p1n, p1s, on.get("polish_route"))
        assert dfun <= 1e-7, (seed, method, on.fun, os_.fun)
        assert (ov.fun - os_.fun) / max(abs(os_.fun), floor * 1e7) <= 1e-7, (seed, method, ov.fun, os_.fun)
    print("native vs scipy route per method:", stats)
    assert stats["acme"]["identical"] >= stats["acme"]["n"] - stats["acme"]["polished"]


def test_reference_polish_is_public_minimize_on_the_public_scores_to_the_bit():
    """`polish_reference` -- the one polish on the reference's route, whoever asks for it (a single accessor call, the
    streaming executor, a worker process): the lean L-BFGS-B driver on the objective object.  It must be what
    `differential_evolution` does for the reference (phasing.py:276-284): the public `scipy.optimize.minimize` on the
    public score function, then scipy's acceptance rule -- identical x, fun, nfev and accepted flag.  The 60 spectra
    of the divergence sweep, every method, one and two parameters, a seeded random start each; every method must accept
    a polish that iterated (otherwise nothing was compared but the start)."""
    import scipy.optimize

    from xmris_amd import autophase_solver as aps

    iterated = {m: 0 for m in aps.METHODS}
    for seed in range(60):
        spec, freq, pivot, kmax, iw = _sweep_spectrum(aps, seed)
        rng = np.random.default_rng(5000 + seed)
        start = np.array([rng.uniform(-180, 180), rng.uniform(-4000, 4000)])
        for method, fn in (("acme", aps.acme_score), ("peak_minima", aps.peak_minima_score), ("positivity", aps.roi_positivity_score)):
            args = (spec, freq, pivot) + (() if method == "acme" else (kmax, iw))
            for p0_only in (False, True):
                bounds = [(-180.0, 180.0)] if p0_only else [(-180.0, 180.0), (-4000.0, 4000.0)]
                x0 = start[:len(bounds)]
                fun0 = float(fn(x0, *args))
                ref = scipy.optimize.minimize(fn, np.copy(x0), args=args, method="L-BFGS-B", bounds=bounds)
                accepted = bool(ref.fun < fun0 and ref.success and all(lo <= v <= hi for v, (lo, hi) in zip(ref.x, bounds)))
                want_x, want_fun = (ref.x, float(ref.fun)) if accepted else (x0, fun0)
                x, fun, nfev, polished = aps.polish_reference(spec, freq, pivot, kmax, iw, method, p0_only, np.copy(start))
                tag = (seed, method, p0_only)
                assert np.array_equal(x, want_x) and fun == want_fun and nfev == ref.nfev and polished == accepted, tag
                iterated[method] += int(accepted and ref.nit >= 1)
    print("accepted polishes that iterated, of 120 per method:", iterated)
    assert all(v >= 1 for v in iterated.values()), iterated


def test_polish_worker_child_imports_neither_torch_nor_the_hip_library():
    """A polish worker is numpy, scipy and the objective statements: importing its module (what the child's
    `python -c` does) and the objective it serves must leave torch out of `sys.modules` and libxmris_hip / the HIP
    runtime out of the process's loaded libraries."""
    import subprocess
    import sys

    code = ("import sys; from xmris_amd import polish_workers as w; from xmris_amd import autophase_solver\n"
            "assert callable(w.main) and 'torch' not in sys.modules, sorted(m for m in sys.modules if 'torch' in m)\n"
            "libs = [ln.split()[-1] for ln in open('/proc/self/maps') if 'libxmris_hip' in ln or 'libamdhip' in ln]\n"
            "assert not libs, libs\n")
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120,
                         cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert res.returncode == 0, res.stderr[-2000:]


def test_deferred_chain_metadata_matches_materialised_data(monkeypatch):
    """The recorded (not yet computed) steps of the accessor chain must announce exactly the shape and dtype their
    data has once computed (numpy's promotion included), keep coordinates / attrs available without computing, and
    compute on first use -- on the numpy test double of the device layer."""
    import _numpy_device

    import xmris_amd as xm

    _numpy_device.install(monkeypatch)
    t = np.linspace(0, 0.1, 50)
    for dt_in in (np.complex64, np.complex128, np.float32, np.float64):
        x = (np.random.default_rng(1).standard_normal((3, 50))).astype(dt_in)
        a = xm.LabeledArray(x, ("v", "time"), {"time": t}, {"k": 1})
        zf = a.xmr.zero_fill(target_points=128)
        ap = zf.xmr.apodize_exp(lb=2.0)
        sp = ap.xmr.to_spectrum()
        assert zf.is_deferred and ap.is_deferred and sp.is_deferred
        steps, root = sp.pending_chain()
        assert [s_[0] for s_ in steps] == ["to_spectrum", "apodize_exp", "zero_fill"] and root is a
        assert sp.dims == ("v", "frequency") and sp.attrs["apodization_lb"] == 2.0 and len(sp.coords["frequency"]) == 128
        for node in (zf, ap, sp):
            shape, dtype = node.shape, node.dtype
            v = node.values  # computes (and, recursively, its parents)
            assert not node.is_deferred and v.shape == shape and v.dtype == dtype, (dt_in, shape, dtype, v.dtype)
    monkeypatch.setenv("XMRIS_AMD_EAGER", "1")
    assert not xm.LabeledArray(x, ("v", "time"), {"time": t}).xmr.zero_fill(target_points=128).is_deferred


@pytest.mark.parametrize("fg", ["native", "numpy"])
def test_lean_polish_is_scipys_minimize_to_the_bit(oracle, monkeypatch, fg):
    """`autophase_solver.polish_lbfgsb` drives scipy's compiled L-BFGS-B core itself (no ScalarFunction / bounds
    front end) with a restated forward-difference gradient: x, fun, jac, nfev, nit, success must equal
    `scipy.optimize.minimize(..., method="L-BFGS-B", bounds=...)` -- the polish `differential_evolution` runs for the
    reference (phasing.py:276-284) -- bit for bit, for all three objectives, one and two parameters, starts inside,
    ON the bounds (the difference step flips there) and next to them, converged at once or after tens of iterations.
    `fg`: the f-and-gradient requests answered by one native call (`xm_solver_fg`, the default) or spelled out in numpy."""
    import scipy.optimize

    from xmris_amd import autophase_solver as aps

    if fg == "numpy":
        monkeypatch.setenv("XM_POLISH_NUMPY_FG", "1")
    else:
        monkeypatch.delenv("XM_POLISH_NUMPY_FG", raising=False)

    rng = np.random.default_rng(3)
    n_iter = []
    for case in range(6):
        nt = int(rng.choice([256, 1024, 2048]))
        t = np.arange(nt) / 5000.0
        f0, d, a = rng.uniform(-2000, 2000, 3), rng.uniform(10, 60, 3), rng.uniform(0.2, 1.0, 3)
        x = sum(ai * np.exp(-di * t) * np.exp(2j * np.pi * fi * t + 1j * rng.uniform(-3, 3)) for ai, di, fi in zip(a, d, f0))
        x = (x + 0.02 * (rng.standard_normal(nt) + 1j * rng.standard_normal(nt)))[None, :]
        _, inf = oracle.pipeline_values(x, t, 2 * nt, 5.0, solve=False)
        sl, fr, pv, ti = inf["slice"], inf["freq"], inf["pivot"], inf["target_idx"]
        for method in aps.METHODS:
            obj = aps.NativeObjective(sl, fr, pv, ti, aps.index_width_of(fr, 100), method)
            for p0_only in (False, True):
                bounds = [(-180.0, 180.0)] if p0_only else [(-180.0, 180.0), (-4000.0, 4000.0)]
                starts = [np.array([rng.uniform(-180, 180)] + ([] if p0_only else [rng.uniform(-4000, 4000)])) for _ in range(2)]
                starts += [np.array([180.0] + ([] if p0_only else [4000.0])), np.array([-180.0] + ([] if p0_only else [-4000.0])),
                           np.array([179.999999995] + ([] if p0_only else [12.0]))]
                for x0 in starts:
                    ref = scipy.optimize.minimize(obj, np.copy(x0), method="L-BFGS-B", bounds=bounds)
                    got = aps.polish_lbfgsb(obj, np.copy(x0), bounds)
                    tag = (case, method, p0_only, x0)
                    assert np.array_equal(ref.x, got.x) and ref.fun == got.fun and np.array_equal(ref.jac, got.jac), tag
                    assert (ref.nfev, ref.nit, ref.success, ref.status) == (got.nfev, got.nit, got.success, got.status), tag
                    n_iter.append(ref.nit)
    assert max(n_iter) >= 10 and min(n_iter) == 0  # both regimes were exercised
    # the fallback is the public entry point itself
    fb = aps.polish_lbfgsb(obj, np.copy(x0), bounds, force_scipy=True)
    assert np.array_equal(fb.x, ref.x) and fb.nfev == ref.nfev


def test_coarse_spectra_factorisation_used_by_the_matrix_core_kernel():
    """The algebra of `csrc/xm_coarse.h` in numpy: the 1024-bin DFT of 512 samples as two 32-point stages with the
    kernel's index maps -- n = 32 n1 + n2 (n1 < 16), k = k1 + 32 k2; D1[n2, k1] = sum_n1 x[32 n1 + n2] W32^(n1 k1),
    Z = D1 * W1024^(n2 k1), X[k1 + 32 k2] = sum_n2 W32^(n2 k2) Z[n2, k1] -- including the PERMUTED contraction order in
    which an MFMA accumulator tile presents its rows to the next product (element j of lane half h at k-step s is row
    16 s + 8 (j >> 2) + 4 h + (j & 3)): summing the second stage in that order, with the constant operand permuted the
    same way, must give the plain DFT."""
    rng = np.random.default_rng(1)
    x = rng.standard_normal(512) + 1j * rng.standard_normal(512)
    ref = np.fft.fft(x, n=1024)
    w32 = lambda m: np.exp(-2j * np.pi * (m % 32) / 32)  # noqa: E731
    w1024 = lambda m: np.exp(-2j * np.pi * (m % 1024) / 1024)  # noqa: E731
    n1, n2, k1, k2 = np.arange(16), np.arange(32), np.arange(32), np.arange(32)
    a1 = x.reshape(16, 32).T                                   # A1[n2, n1] = x[32 n1 + n2]
    d1 = a1 @ w32(np.outer(n1, k1))                            # D1[n2, k1]
    z = d1 * w1024(np.outer(n2, k1))
    d2 = np.zeros((32, 32), dtype=complex)                     # D2[k2, k1]
    for s in range(2):                                         # two k-steps of 16, in the accumulator tile's row order
        for h in range(2):
            for j in range(8):
                row = 16 * s + 8 * (j >> 2) + 4 * h + (j & 3)
                d2 += np.outer(w32(row * k2), z[row])
    got = np.empty(1024, dtype=complex)
    got[(k1[None, :] + 32 * k2[:, None])] = d2
    assert np.allclose(got, ref, rtol=0, atol=1e-10 * np.abs(ref).max())
    rows = sorted(16 * s + 8 * (j >> 2) + 4 * h + (j & 3) for s in range(2) for h in range(2) for j in range(8))
    assert rows == list(range(32))  # every row of Z exactly once


@pytest.mark.parametrize("dtype", ["complex128", "complex64"])
@pytest.mark.parametrize("n_in,target,lb", [(1024, 2048, 5.0), (1536, 1536, 5.0), (1972, 4096, 0.0), (4096, 8192, 12.5), (1000, 1024, 3.0)])
def test_winner_spectrum_is_the_reference_slice_bit_for_bit(oracle, dtype, n_in, target, lb):
    """`pipeline.winner_spectrum` -- the slice the (p0, p1) search runs on -- restates fid.py:251, fid.py:136-139,
    fourier.py:153 and fourier.py:31-32 on ONE row; it must equal, bit for bit, the row the oracle (= the reference's
    statements on the whole batch) slices out of its spectra: numpy's FFT of a row of a batch and of the row alone are
    the same bits, complex64 storage is promoted at the apodisation as numpy promotes it; zero fill to 2x, to an odd
    ratio, none; lb = 0 (all-ones weights)."""
    import torch

    from xmris_amd import pipeline as pl

    rng = np.random.default_rng(n_in + target)
    t = 3e-4 + np.arange(n_in) * 2e-4
    x = (rng.standard_normal((7, n_in)) + 1j * rng.standard_normal((7, n_in))).astype(dtype)
    x[4] *= 3.0
    ref, info = oracle.pipeline_values(x, t, target, lb, peak_width=100, solve=False)
    row = info["flat_idx"] // info["freq"].size
    plan = pl.make_plan(torch.from_numpy(x), t, target, lb)
    got = pl.winner_spectrum(plan, x[row].astype(np.complex128))
    assert got.dtype == np.complex128 and np.array_equal(got, info["slice"])
    assert int(np.argmax(np.abs(got))) == info["target_idx"]


def test_polish_workers_never_make_a_caller_wait_for_their_start(oracle):
    """`polish_workers.PolishWorkers` (children: `polish_workers.main`): a request submitted before any worker has reported ready is polished by the
    future's own thread; once the workers are up they answer with the same (x, fun, nfev) to the bit -- the polish is
    the reference's route either way (phasing.py:276-284 with scipy's defaults) -- and a worker that dies is replaced by
    the in-thread polish, not waited for."""
    import time

    from xmris_amd import autophase_solver as aps

    rng = np.random.default_rng(11)
    nt = 512
    t = np.arange(nt) / 5000.0
    x = sum(a * np.exp(-d * t) * np.exp(2j * np.pi * f * t + 1j * ph) for a, d, f, ph in
            ((1.0, 25.0, 310.0, 0.4), (0.6, 40.0, -900.0, -1.1)))
    x = (x + 0.05 * (rng.standard_normal(nt) + 1j * rng.standard_normal(nt)))[None, :]
    _, inf = oracle.pipeline_values(x, t, 2 * nt, 5.0, solve=False)
    sl, fr, pv, ti = inf["slice"], inf["freq"], inf["pivot"], inf["target_idx"]
    args = (sl, fr, pv, ti, aps.index_width_of(fr, 100), "acme", False, np.array([12.0, 150.0]))
    want = aps.polish_reference(*args)

    def same(got):
        return np.array_equal(got[0], want[0]) and got[1] == want[1] and got[2] == want[2]

    pw = aps.PolishWorkers(2, lazy=True)
    try:
        assert not pw._started and pw._free.qsize() == 0
        t0 = time.perf_counter()
        assert same(pw.submit(*args).result(timeout=60))  # starts the children, is answered without them
        first = time.perf_counter() - t0
        assert pw._started
        deadline = time.time() + 120
        while pw._free.qsize() < 2 and time.time() < deadline:
            time.sleep(0.05)
        assert pw._free.qsize() == 2, "the workers did not report ready"
        futs = [pw.submit(*args) for _ in range(6)]
        assert all(same(f.result(timeout=60)) for f in futs)
        assert pw._free.qsize() == 2  # both back on the free list
        pw._procs[0].kill()
        pw._procs[0].wait()
        futs = [pw.submit(*args) for _ in range(4)]
        assert all(same(f.result(timeout=60)) for f in futs)
        assert first < 30.0
        pw._procs[1].kill()  # ... and with the last one gone nobody waits for a worker any more
        pw._procs[1].wait()
        futs = [pw.submit(*args) for _ in range(3)]
        assert all(same(f.result(timeout=60)) for f in futs)
        assert pw._alive == 0 and pw._free.qsize() == 0
    finally:
        pw.close()


@pytest.mark.parametrize("breakage", ["module_gone", "other_signature", "other_release"])
def test_polish_falls_back_to_public_minimize_when_scipy_internals_change(oracle, monkeypatch, breakage):
    """`polish_lbfgsb` follows a PRIVATE entry point of scipy 1.15 (`scipy.optimize._lbfgsb.setulb`); the reference's
    lock file pins scipy 1.17 for newer interpreters, where that module is a C rewrite with another signature
    (`uv.lock:2908-2909`).  Any such change must end in the public `scipy.optimize.minimize` with the same bits:
    the private module gone (ImportError), its entry point taking other arguments (TypeError on the first call),
    another release number."""
    import sys

    import scipy
    import scipy.optimize

    from xmris_amd import autophase_solver as aps

    rng = np.random.default_rng(8)
    nt = 512
    t = np.arange(nt) / 5000.0
    x = sum(a * np.exp(-d * t) * np.exp(2j * np.pi * f * t + 1j * p) for a, d, f, p in
            ((1.0, 25.0, 410.0, 0.4), (0.5, 40.0, -700.0, -2.0)))
    x = (x + 0.02 * (rng.standard_normal(nt) + 1j * rng.standard_normal(nt)))[None, :]
    _, inf = oracle.pipeline_values(x, t, 2 * nt, 5.0, solve=False)
    sl, fr, pv, ti = inf["slice"], inf["freq"], inf["pivot"], inf["target_idx"]
    obj = aps.NativeObjective(sl, fr, pv, ti, 1, "acme")
    bounds = [(-180.0, 180.0), (-4000.0, 4000.0)]
    x0 = np.array([35.0, -250.0])
    ref = scipy.optimize.minimize(obj, np.copy(x0), method="L-BFGS-B", bounds=bounds)
    lean = aps.polish_lbfgsb(obj, np.copy(x0), bounds)
    assert ref.nit >= 2 and np.array_equal(lean.x, ref.x)  # the lean route is in use and iterates here
    if breakage == "module_gone":
        monkeypatch.setitem(sys.modules, "scipy.optimize._lbfgsb", None)  # `from scipy.optimize import _lbfgsb` fails
        monkeypatch.delattr(scipy.optimize, "_lbfgsb", raising=False)
    elif breakage == "other_signature":
        from scipy.optimize import _lbfgsb

        real_setulb = _lbfgsb.setulb

        def setulb(*args, **kwargs):  # scipy 1.17's C rewrite takes other arguments than this package passes
            if sys._getframe(1).f_globals.get("__name__") == aps.polish_lbfgsb.__module__:
                raise TypeError("setulb() takes 12 positional arguments but 17 were given")
            return real_setulb(*args, **kwargs)  # (scipy's own front end knows its own core)

        monkeypatch.setattr(_lbfgsb, "setulb", setulb)
    else:
        monkeypatch.setattr(scipy, "__version__", "1.17.0")
    got = aps.polish_lbfgsb(obj, np.copy(x0), bounds)
    assert np.array_equal(got.x, ref.x) and got.fun == ref.fun and (got.nfev, got.nit) == (ref.nfev, ref.nit), breakage


def test_solver_team_survives_a_member_that_is_not_there():
    """A team member that is asleep or descheduled must not stall the search: the searching thread waits a grace
    period, then computes the missing share itself (`xm_solver_obj.cpp`, "Stragglers").  With the test hook that
    puts member 2 to sleep for 3 ms before every fifth job, a 4-thread search returns EXACTLY what the serial search
    returns (every work unit has one value, whoever computes it), takes nowhere near the sum of the naps, and the
    backup counter moves.  (Own process: the hook is read when the pool is created.)"""
    import subprocess
    import sys

    code = r"""
import time, json, numpy as np
from xmris_amd import autophase_solver as aps, _lib
rng = np.random.default_rng(5)
n = 8192
t = np.arange(n // 2) / 5000.0
x = sum(a * np.exp(-d * t) * np.exp(2j * np.pi * f * t + 1j * p) for a, d, f, p in ((1.0, 20.0, 310.0, 0.7), (0.6, 35.0, -820.0, -1.1)))
x = x + 0.02 * (rng.standard_normal(t.size) + 1j * rng.standard_normal(t.size))
sl = np.fft.fftshift(np.fft.fft(np.pad(x, (0, n - t.size)), norm="ortho"))
fr = np.fft.fftshift(np.fft.fftfreq(n, 1 / 5000.0))
k = int(np.argmax(np.abs(sl)))
out = {}
for th in (1, 4):
    t0 = time.perf_counter()
    p0, p1, opt = aps.solve(sl, fr, float(fr[k]), k, 1, threads=th)
    out[th] = (p0, p1, float(opt.fun), int(opt.nfev), int(opt.nit), time.perf_counter() - t0)
print(json.dumps({"serial": out[1], "team": out[4], "backups": int(_lib.load().xm_solver_pool_backups())}))
"""
    env = dict(os.environ, XM_SOLVER_TEST_STALL="2,3000")
    env.pop("XM_SOLVER_THREADS", None)
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env,
                         cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert res.returncode == 0, res.stderr[-2000:]
    import json

    got = json.loads(res.stdout.strip().splitlines()[-1])
    assert got["serial"][:5] == got["team"][:5]  # p0, p1, fun, nfev, nit: bit for bit
    assert got["backups"] >= 5
    jobs = got["team"][3] / 4  # at least a quarter of the evaluations as hand-offs... each fifth one napped 3 ms
    assert got["team"][5] < 0.25 * (jobs / 5) * 3e-3 + 0.5, got  # far below the sum of the naps


def test_solver_pool_back_to_back_searches_with_a_late_member():
    """A member that missed the last batches of search A wakes into search B on the same pool with `seen < gen` and
    finds A's last descriptor still in the ring -- A's solver may already be destroyed (advisor, round 3).  Jobs carry
    the pool phase of the search that published them and a member discards any other.  300 searches back to back on
    DIFFERENT slices (each solver freed before the next starts), member 1 napping 200 us before every fifth job it
    takes: every search must return exactly the serial result for ITS slice."""
    import subprocess
    import sys

    code = r"""
import json, numpy as np
from xmris_amd import autophase_solver as aps
n = 2048
fr = np.fft.fftshift(np.fft.fftfreq(n, 1 / 5000.0))
t = np.arange(n // 2) / 5000.0
bad = 0
for i in range(300):
    rng = np.random.default_rng(100 + i)
    x = sum(a * np.exp(-d * t) * np.exp(2j * np.pi * f * t + 1j * p) for a, d, f, p in
            ((1.0, 20.0 + i % 7, 310.0 + 3 * i, 0.7), (0.6, 35.0, -820.0 + i, -1.1)))
    x = x + 0.02 * (rng.standard_normal(t.size) + 1j * rng.standard_normal(t.size))
    sl = np.fft.fftshift(np.fft.fft(np.pad(x, (0, n - t.size)), norm="ortho"))
    k = int(np.argmax(np.abs(sl)))
    obj = aps.NativeObjective(sl, fr, float(fr[k]), k, 1, "acme")
    obj.set_threads(3)
    team = obj.de(False)
    del obj  # the solver is destroyed before the next search activates the pool again
    if i % 10 == 0:
        ref = aps.NativeObjective(sl, fr, float(fr[k]), k, 1, "acme")
        ref.set_threads(1)
        serial = ref.de(False)
        bad += int(not (np.array_equal(team[1], serial[1]) and team[2:] == serial[2:]))
print(json.dumps({"bad": bad}))
"""
    env = dict(os.environ, XM_SOLVER_TEST_STALL="1,200")
    env.pop("XM_SOLVER_THREADS", None)
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env,
                         cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert res.returncode == 0, res.stderr[-2000:]
    import json

    assert json.loads(res.stdout.strip().splitlines()[-1])["bad"] == 0


def test_restated_xarray_semantics_one_by_one(monkeypatch):
    """The reference leans on four xarray behaviours that this package has to restate for its own container (and
    that `tests/_fake_xarray.py` cannot vouch for -- it only carries data in and out).  One assertion each, against
    xarray's DOCUMENTED semantics (xarray 2025.6 API reference / user guide), on the host layer alone:

    * `DataArray.pad` (fid.py:251): "coordinates will be padded with ... the 'constant' mode with fill_value
      dtypes.NA" -- every coordinate along the padded dimension is NaN-filled; the reference then overwrites the
      dimension coordinate only when it has more than one entry (fid.py:254-263);
    * `DataArray.roll(roll_coords=True)` (fourier.py:31-32): "roll_coords: indicates whether to roll the coordinates
      by the offset too" -- ALL coordinates along the rolled dimension move with the data, attrs kept;
    * binary arithmetic (fid.py:139, phasing.py:73): the result's name is kept only "if all operands share it"
      (`xarray.core.utils.result_name`): the other operand is the coordinate of `dim`, named `dim`;
    * `DataArray.isel({d: i})` with integers (phasing.py:241-242): the dimension is dropped, the result is the
      1-D slice through that position -- autophase searches on exactly that slice."""
    import _numpy_device

    from xmris_amd import processing
    from xmris_amd.labeled import Coordinate, LabeledArray

    _numpy_device.install(monkeypatch)
    rng = np.random.default_rng(1)
    x = rng.standard_normal((2, 6)) + 1j * rng.standard_normal((2, 6))
    t = np.arange(6) * 0.5
    aux = np.arange(6) * 10.0  # a second, non-dimension coordinate along `time`
    da = LabeledArray(x, ("voxel", "time"), {"time": Coordinate("time", t, {"units": "s"}),
                                             "echo": Coordinate("time", aux, {"note": "aux"})}, {"k": 1}, "fid")
    # pad: the dimension coordinate is extrapolated (more than one entry), the other coordinate along it is NaN-filled
    zf = processing.fid.zero_fill(da, target_points=10, position="symmetric")
    np.testing.assert_array_equal(zf.coords["time"].values, (t[0] - 2 * 0.5) + np.arange(10) * 0.5)
    np.testing.assert_array_equal(zf.coords["echo"].values, np.r_[np.nan, np.nan, aux, np.nan, np.nan])
    assert zf.coords["echo"].attrs == {"note": "aux"} and zf.name == "fid"  # pad keeps the name
    one = LabeledArray(x[:, :1], ("voxel", "time"), {"time": Coordinate("time", t[:1])}, {}, None)
    zf1 = processing.fid.zero_fill(one, target_points=3)  # one entry: nothing to extrapolate from, the NaN fill stays
    np.testing.assert_array_equal(zf1.coords["time"].values, np.r_[t[0], np.nan, np.nan])
    # roll(roll_coords=True): both coordinates along the dimension are rolled by n // 2, attrs untouched
    sh = processing.fourier.fftshift(da, "time")
    np.testing.assert_array_equal(sh.values, np.roll(x, 3, axis=1))
    np.testing.assert_array_equal(sh.coords["time"].values, np.roll(t, 3))
    np.testing.assert_array_equal(sh.coords["echo"].values, np.roll(aux, 3))
    assert sh.coords["time"].attrs == {"units": "s"} and sh.attrs == {"k": 1} and sh.name == "fid"
    ish = processing.fourier.ifftshift(LabeledArray(x[:, :5], ("voxel", "time"), {"time": Coordinate("time", t[:5])}), "time")
    np.testing.assert_array_equal(ish.coords["time"].values, np.roll(t[:5], 3))  # (n + 1) // 2 for odd n
    # binary-op name rule: "fid" * (coordinate named "time") -> None;  "time" * "time" -> "time"
    assert processing.fid.apodize_exp(da, lb=1.0).name is None
    named = LabeledArray(x, ("voxel", "time"), {"time": Coordinate("time", t)}, {}, "time")
    assert processing.fid.apodize_exp(named, lb=1.0).name == "time"
    spec = LabeledArray(x, ("voxel", "frequency"), {"frequency": Coordinate("frequency", t - 1.0)}, {}, "frequency")
    assert processing.phasing.phase(spec, p0=10.0).name == "frequency"
    assert processing.phasing.phase(LabeledArray(x, ("voxel", "frequency"), {"frequency": Coordinate("frequency", t - 1.0)},
                                                 {}, "spectrum"), p0=10.0).name is None
    # isel: autophase works on the 1-D slice through the global arg-max of every OTHER dimension
    y = 0.01 * x
    y[1, 4] = 5.0 + 0.0j
    got = processing.phasing.autophase(LabeledArray(y, ("voxel", "frequency"), {"frequency": Coordinate("frequency", t - 1.0)}),
                                       p0_only=True)
    assert got.attrs["phase_pivot"] == (t - 1.0)[4]  # the pivot is the coordinate at the arg-max ALONG dim ...
    ref_p0 = __import__("xmris_amd.autophase_solver", fromlist=["solve"]).solve(
        y[1].astype(np.complex128), t - 1.0, (t - 1.0)[4], 4, 1, p0_only=True, polish="numpy")[0]
    assert got.attrs["phase_p0"] == ref_p0  # ... and the search ran on row 1 (the slice isel would return), not row 0


def test_solver_team_budget(monkeypatch):
    """`default_threads` / `burst_threads` / `scarce_cpus`: one rank takes half of its CPU share (power of two, at most
    16) and the whole share for a lone search; several ranks on a node reserve one core per rank and give the rest to
    the searches in flight on the node (16 CPUs, 8 ranks: 8 -- round 2's rule left one thread); few cores per rank ->
    blocking event waits."""
    from xmris_amd import autophase_solver as aps
    from xmris_amd import cpu_budget

    for var in ("XM_SOLVER_THREADS", "XM_BLOCKING_SYNC", "LOCAL_WORLD_SIZE"):
        monkeypatch.delenv(var, raising=False)
    share = {"n": 16}
    monkeypatch.setattr(cpu_budget, "cpu_share", lambda: share["n"])
    assert (aps.default_threads(), aps.burst_threads(), aps.scarce_cpus()) == (8, 16, False)
    # a streaming call: three quarters of the share for two searches in flight (each busy half of its two device
    # periods), half of it when the host paces the steps (every team spins all the time)
    from xmris_amd import pipeline as pipe

    assert (aps.stream_threads(), aps.stream_threads(host_paced=True)) == (12, 16)
    assert (pipe._search_team(2), pipe._search_team(3), pipe._search_team(4)) == (6, 4, 4)
    share["n"] = 6
    assert (aps.default_threads(), aps.burst_threads()) == (2, 4)
    share["n"] = 256
    assert (aps.default_threads(), aps.burst_threads()) == (16, 16)
    monkeypatch.setenv("LOCAL_WORLD_SIZE", "8")
    share["n"] = 16
    assert (aps.default_threads(), aps.burst_threads(), aps.scarce_cpus()) == (8, 8, True)
    assert (aps.stream_threads(), pipe._search_team(2), pipe._search_team(3), pipe._search_team(4)) == (8, 4, 2, 2)  # the node's budget, evenly
    share["n"] = 128
    assert (aps.default_threads(), aps.scarce_cpus()) == (16, False)
    share["n"] = 8
    assert aps.default_threads() == 1  # (never zero)
    monkeypatch.setenv("XM_SOLVER_THREADS", "5")
    assert aps.default_threads() == aps.burst_threads() == 5


def test_bench_dump_outputs_and_arguments_without_gpu(tmp_path):
    """bench.dump_outputs on host tensors: a fixed row sample within its byte budget, float arrays only, the winner's
    row where the global flat index puts it; and bench.py refuses a step count below one before it touches a GPU."""
    import subprocess
    import sys
    from types import SimpleNamespace

    import torch

    sys.path.insert(0, ROOT)
    import bench

    rng = np.random.default_rng(3)
    for cdt, rd in ((torch.complex64, np.float32), (torch.complex128, np.float64)):
        spec = torch.from_numpy((rng.standard_normal((300, 64)) + 1j * rng.standard_normal((300, 64))).astype(np.complex128)).to(cdt)
        res = SimpleNamespace(p0=12.5, p1=-3.25, pivot=0.5, flat_index=1000 * 64 + 17, target_idx=17, max_abs=2.0)
        d = tmp_path / str(rd.__name__)
        bench.dump_outputs(torch, str(d), spec, res, row_offset=800, budget_bytes=100 * 64 * 2 * np.dtype(rd).itemsize)
        sample, rows = np.load(d / "spectra_sample.npy"), np.load(d / "spectra_sample_rows.npy")
        assert sample.dtype == rd and sample.shape == (100, 64, 2) and rows.dtype == np.float64
        assert np.all(np.diff(rows) > 0) and rows.min() >= 0 and rows.max() < 300
        assert np.array_equal(sample, torch.view_as_real(spec).numpy()[rows.astype(int)])
        assert np.array_equal(np.load(d / "spectrum_winner.npy"), torch.view_as_real(spec[200]).numpy())
        assert np.array_equal(np.load(d / "autophase.npy"), [12.5, -3.25, 0.5, 1000 * 64 + 17, 17, 2.0])
        bench.dump_outputs(torch, str(d / "again"), spec, res, row_offset=800, budget_bytes=100 * 64 * 2 * np.dtype(rd).itemsize)
        assert np.array_equal(np.load(d / "again" / "spectra_sample_rows.npy"), rows)
        bench.dump_outputs(torch, str(d / "other_rank"), spec, res, row_offset=0)  # the winning row lives elsewhere
        assert not (d / "other_rank" / "spectrum_winner.npy").exists()
        assert np.load(d / "other_rank" / "spectra_sample.npy").shape == (300, 64, 2)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 2 and "--steps" in r.stderr
