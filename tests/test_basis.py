"""fit_basis without a GPU: the numpy oracle (tests/_basis_oracle.py) is pinned first -- model and Jacobian against
finite differences, the automatic start, the restated iteration against scipy -- then the Python layer of
xmris_amd.fitting.basis: groups, refusals (every ValueError is raised before native code), and the result's dims,
coords and attrs with the launch replaced by the oracle.  The last tests pin the selection of the GPU cases."""
import functools

import numpy as np
import pytest

import _basis_oracle as orc
from xmris_amd import LabeledArray
from xmris_amd.fitting import basis as fb

STEP_M = (1, 2, 3, 5)
TIE = 1e-9  # accept / reject margins below this are too close to call
PARITY = {"M5G2": dict(M=5, G=2, n=512, seed=51, n_vox=64), "M16G2": dict(M=16, G=2, n=1024, seed=52, n_vox=16)}


# ---- the oracle ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lineshape,fit_phase", [("voigt", True), ("lorentzian", False)])
def test_jacobian_against_central_differences(lineshape, fit_phase):
    c = orc.kernel_case(5, 2, 200, 3, lineshape=lineshape, fit_phase=fit_phase)
    p = c["truth"].copy()
    p[0] = 0.0  # the amplitude columns do not need a_m
    J = orc.model_jacobian(p, c["B"], c["group"], c["dt"])
    assert J.shape == (200, 5 + 3 * 2 + 1)
    steps = np.concatenate([np.full(5, 1e-6), np.full(2, 1e-5), np.full(2, 1e-4), np.full(2, 1e-2), [1e-6]])  # a, f, d, s, phi
    for q in range(p.size):
        h = steps[q]
        e = np.zeros(p.size)
        e[q] = h
        fd = (orc.model(p + e, c["B"], c["group"], c["dt"]) - orc.model(p - e, c["B"], c["group"], c["dt"])) / (2 * h)
        scale = max(np.abs(J[:, q]).max(), 1e-300)
        assert np.abs(fd - J[:, q]).max() <= 1e-7 * scale, q


def test_model_is_the_stated_sum():
    c = orc.kernel_case(4, 3, 64, 5)
    p, B, g, dt = c["truth"], c["B"], c["group"], c["dt"]
    M, G = 4, 3
    t = np.arange(64) * dt
    ref = np.zeros(64, complex)
    for m in range(M):
        k = g[m]
        ref += p[m] * B[m] * np.exp(-p[M + G + k] * t - p[M + 2 * G + k] * t * t + 2j * np.pi * p[M + k] * t)
    ref *= np.exp(1j * p[-1])
    np.testing.assert_allclose(orc.model(p, B, g, dt), ref, rtol=1e-13, atol=1e-15)
    assert sorted(set(g.tolist())) == [0, 1, 2] and list(g) == [0, 1, 2, 0]  # interleaved groups


def test_bound_transforms_and_automatic_start():
    c = orc.kernel_case(3, 2, 128, 7, skip=5)
    x, B = c["x"][0], c["B"]
    a = orc.automatic_amplitudes(x, B, skip=5)
    ref = np.linalg.norm(x[5:]) / (3 * np.linalg.norm(B[:, 5:], axis=1))
    np.testing.assert_allclose(a, ref, rtol=1e-14)
    assert np.all(a > 0)
    np.testing.assert_allclose(orc.automatic_amplitudes(7.0 * x, B, 5), 7.0 * a, rtol=1e-14)  # scale-covariant
    assert not orc.automatic_amplitudes(np.zeros(128), B, 5).any()
    v0, u0 = orc.start_values(x, B, c["init"], c["lo"], c["hi"], c["fixed"], 5)
    p, s = orc.physical(u0, v0, c["lo"], c["hi"], c["fixed"])
    np.testing.assert_allclose(p, v0, rtol=1e-12)
    free = ~(c["fixed"] | (c["lo"] == c["hi"]))
    assert np.all(s[free] != 0) and not s[~free].any()  # nothing starts on a bound with zero slope
    assert np.all((v0[free] > c["lo"][free]) & (v0[free] < c["hi"][free]))
    # amplitude_start overrides the automatic one
    init = c["init"].copy()
    init[:3] = [1.0, 2.0, 3.0]
    assert np.array_equal(orc.start_values(x, B, init, c["lo"], c["hi"], c["fixed"], 5)[0][:3], [1.0, 2.0, 3.0])


def test_gaussian_width_is_the_fwhm():
    s = float(orc.gaussian_damping(4.0))
    f = np.linspace(-20, 20, 400001)
    line = np.exp(-(np.pi * f) ** 2 / s)  # Fourier transform of exp(-s t^2), up to a factor
    half = f[line >= 0.5]
    assert abs((half[-1] - half[0]) - 4.0) < 1e-3
    np.testing.assert_allclose(fb.gaussian_fwhm(fb.gaussian_damping(4.0)), 4.0, rtol=1e-14)
    np.testing.assert_allclose(fb.gaussian_damping(4.0), s, rtol=1e-14)


@functools.lru_cache(maxsize=None)
def _step_case(name):
    return orc.kernel_case(**dict(orc.step_cases())[name])


def _args(c):
    return (c["B"], c["group"], c["dt"], c["init"], c["lo"], c["hi"], c["fixed"], c["skip"])


@functools.lru_cache(maxsize=None)
def _step_ref(name, v, m):
    c = _step_case(name)
    return orc.lm_steps_basis(c["x"][v], *_args(c), max_iter=m)


@pytest.mark.parametrize("name", ["M3G3_lorentz_n1000", "M12G2_skip5_n1500"])
def test_lm_steps_basis_converges_to_scipy(name):
    c = _step_case(name)
    for x in c["x"]:
        o = orc.fit(x, *_args(c))
        assert o["success"]
        for solver in ("normal", "qr"):
            r = orc.lm_steps_basis(x, *_args(c), solver=solver)
            assert r["status"] == 0 and r["iters"] < 200 and len(r["trials"]) == r["iters"]
            free = o["sd"] > 0
            assert np.all(np.abs(r["params"] - o["params"])[free] <= 1e-3 * o["sd"][free]), solver
            assert np.array_equal(r["params"][~free], o["params"][~free])
            assert abs(r["rss"] - o["rss"]) <= 1e-9 * o["rss"]


def test_amplitude_sd_against_the_inverse():
    c = _step_case("M12G2_skip5_n1500")
    p = c["truth"]
    sd, cond = orc.amplitude_sd(c["B"], c["group"], c["dt"], p, c["lo"], c["hi"], c["fixed"], c["skip"])
    free = np.flatnonzero(~(c["fixed"] | (c["lo"] == c["hi"])))
    jr = orc.real_rows(orc.model_jacobian(p, c["B"], c["group"], c["dt"])[c["skip"]:, free])
    ref = np.sqrt(np.diag(np.linalg.inv(jr.T @ jr)))[:12]
    np.testing.assert_allclose(sd, ref, rtol=1e-6)
    assert np.isfinite(cond) and cond > 1
    p0 = p.copy()
    p0[3] = 0.0  # nothing singular about one absent metabolite: its own column E B_m does not vanish
    assert np.all(np.isfinite(orc.amplitude_sd(c["B"], c["group"], c["dt"], p0, c["lo"], c["hi"], c["fixed"])[0]))
    p0[:12] = 0.0  # every amplitude 0: the f, d, s and phi columns vanish
    assert np.all(np.isnan(orc.amplitude_sd(c["B"], c["group"], c["dt"], p0, c["lo"], c["hi"], c["fixed"])[0]))


# ---- the Python layer ---------------------------------------------------------------------------------------------------
def test_groups_parsing():
    names = ["NAA", "Cr", "Cho", "Lac"]
    assert fb.parse_groups(None, names)[1] == ["all"] and not fb.parse_groups(None, names)[0].any()
    idx, labels = fb.parse_groups("each", names)
    assert list(idx) == [0, 1, 2, 3] and labels == names
    idx, labels = fb.parse_groups(["s", "m", "s", "x"], names)
    assert list(idx) == [0, 1, 0, 2] and labels == ["s", "m", "x"] and idx.dtype == np.int32
    with pytest.raises(ValueError, match="one label per metabolite"):
        fb.parse_groups(["a", "b"], names)
    with pytest.raises(ValueError, match="'each'"):
        fb.parse_groups("every", names)


@pytest.mark.parametrize("kw", [{}, {"lineshape": "lorentzian"}, {"fit_phase": False},
                                {"amplitude_start": [1.0, 2.0, 3.0, 4.0, 5.0]},
                                {"max_shift": 3.0, "max_broadening": 9.0, "broadening_start": 1.0, "max_gaussian": 7.0,
                                 "gaussian_start": 0.5}])
def test_parameters_are_the_designs_table(kw):
    got = fb.basis_parameters(5, 2, **kw)
    ref = orc.parameters(5, 2, **kw)
    for a, b in zip(got, ref):
        assert np.array_equal(a, b, equal_nan=True)
    init, lo, hi, fixed = got
    free = ~fixed
    assert np.count_nonzero(free) == 5 + (2 if kw.get("lineshape") == "lorentzian" else 3) * 2 + kw.get("fit_phase", True)
    nl = slice(5, 11)
    assert np.all((init[nl][free[nl]] > lo[nl][free[nl]]) & (init[nl][free[nl]] < hi[nl][free[nl]]))  # strictly inside
    assert np.all(lo[:5] == 0) and np.all(np.isinf(hi[:5])) and np.isinf(lo[-1]) and np.isinf(hi[-1])


def test_parameter_refusals():
    for kw in ({"lineshape": "gauss"}, {"broadening_start": 0.0}, {"broadening_start": 20.0}, {"gaussian_start": 25.0},
               {"max_shift": 0.0}, {"amplitude_start": [1.0]}, {"amplitude_start": [1.0, -1.0, 1.0]},
               {"amplitude_start": [1.0, np.nan, 1.0]}):
        with pytest.raises(ValueError):
            fb.basis_parameters(3, 1, **kw)
    fb.basis_parameters(3, 1, lineshape="lorentzian", gaussian_start=25.0)  # not read without a Gaussian part


def _data(shape=(3, 64), dims=("voxel", "time"), dt=2.5e-4, dtype=np.complex128):
    rng = np.random.default_rng(0)
    x = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(dtype)
    coords = {"time": np.arange(shape[dims.index("time")]) * dt}
    for d in dims:
        if d != "time":
            coords[d] = np.arange(shape[dims.index(d)]) * 10.0
    return LabeledArray(x, dims, coords, {"MHz": 123.2})


def _basis(M=3, n=64, dt=2.5e-4, names=None):
    coords = {"time": np.arange(n) * dt}
    if names is not None:
        coords["metabolite"] = np.array(names)
    return LabeledArray(orc.make_basis(M, n, dt, 1), ("metabolite", "time"), coords)


def _no_launch(*a, **k):
    raise AssertionError("native code reached")


def test_refusals_come_before_native_code(monkeypatch):
    monkeypatch.setattr(fb, "_run_fit", _no_launch)
    da = _data()
    with pytest.raises(ValueError, match="Dimension 'fid' missing"):
        fb.fit_basis(da, _basis(), dim="fid")
    with pytest.raises(ValueError, match=r"0\.0005.*0\.00025"):  # both dwell times are named
        fb.fit_basis(da, _basis(dt=5e-4))
    with pytest.raises(ValueError, match="has 60 points along 'time', fewer than the data's 64"):
        fb.fit_basis(da, _basis(n=60))
    with pytest.raises(ValueError, match="coordinate 'time'"):
        fb.fit_basis(da, LabeledArray(orc.make_basis(3, 64, 2.5e-4, 1), ("metabolite", "time")))
    with pytest.raises(ValueError, match="coordinate 'time'"):
        fb.fit_basis(LabeledArray(np.zeros((3, 64), complex), ("voxel", "time")), _basis())
    with pytest.raises(ValueError, match="81 free parameters"):  # 20 + 3 * 20 + 1
        fb.fit_basis(_data((2, 128)), _basis(M=20, n=128), groups="each")
    fb_ok = fb.basis_parameters(20, 20, "lorentzian")  # ... while the same basis fits with 61
    assert np.count_nonzero(~fb_ok[3]) == 61
    with pytest.raises(ValueError, match="skip=55 leaves 9 of 64 points for 10 free parameters"):
        fb.fit_basis(da, _basis(), groups=["a", "a", "b"], skip=55)
    with pytest.raises(ValueError, match="skip=-1"):
        fb.fit_basis(da, _basis(), skip=-1)
    bad = _basis()
    vals = np.array(bad.values)
    vals[1, 7] = np.nan
    with pytest.raises(ValueError, match="non-finite sample"):
        fb.fit_basis(da, LabeledArray(vals, bad.dims, bad.coords))
    vals[1, 7] = complex(0.0, np.inf)
    with pytest.raises(ValueError, match="non-finite sample"):
        fb.fit_basis(da, LabeledArray(vals, bad.dims, bad.coords))
    with pytest.raises(ValueError, match="one name per metabolite"):
        fb.fit_basis(da, _basis(), names=["a", "b"])
    with pytest.raises(ValueError, match="one label per metabolite"):
        fb.fit_basis(da, _basis(), groups=["a", "b"])
    with pytest.raises(ValueError, match="lineshape"):
        fb.fit_basis(da, _basis(), lineshape="gauss")
    with pytest.raises(ValueError, match="max_iter"):
        fb.fit_basis(da, _basis(), max_iter=0)


def _oracle_launch(calls):
    """A stand-in for the launch: the restated iteration on the CPU, outputs shaped as device.basis_fit shapes them."""

    def run(src, axis, basis, group, init, lo, hi, fixed, dt, skip, max_iter, want_fit):
        calls.append(dict(axis=axis, basis=basis, group=group, init=init, lo=lo, hi=hi, fixed=fixed, dt=dt, skip=skip,
                          max_iter=max_iter, want_fit=want_fit))
        x = np.moveaxis(np.asarray(src.values), axis, -1)
        lead, n = x.shape[:-1], x.shape[-1]
        rows = x.reshape(-1, n).astype(np.complex128)
        M = basis.shape[0]
        out = {"params": [], "amp_sd": [], "rss": [], "status": [], "iters": [], "fit": []}
        for r in rows:
            o = orc.lm_steps_basis(r, basis, group, dt, init, lo, hi, fixed, skip, max_iter=max_iter)
            out["params"].append(o["params"])
            out["amp_sd"].append(orc.amplitude_sd(basis, group, dt, o["params"], lo, hi, fixed, skip)[0])
            out["rss"].append(o["rss"])
            out["status"].append(o["status"])
            out["iters"].append(o["iters"])
            out["fit"].append(orc.model(o["params"], basis, group, dt))
        res = {k: np.array(v).reshape(lead + np.array(v).shape[1:]) for k, v in out.items()}
        res["status"], res["iters"] = res["status"].astype(np.int32), res["iters"].astype(np.int32)
        if not want_fit:
            res["fit"] = None
        res["n_free"] = int(np.count_nonzero(~(np.asarray(fixed, bool) | (lo == hi))))
        return res

    return run


@pytest.mark.parametrize("dims,shape", [(("x", "y", "time"), (2, 3, 96)), (("time", "voxel"), (96, 4))])
def test_result_dims_coords_attrs_and_input_untouched(monkeypatch, dims, shape):
    calls = []
    monkeypatch.setattr(fb, "_run_fit", _oracle_launch(calls))
    n, dt = 96, 2.5e-4
    names = ["NAA", "Cr", "Cho"]
    B = _basis(3, 120, dt, names)  # longer than the data: the extra points are cut
    truth = np.concatenate([[1.0, 2.0, 0.5], [2.0, -1.0], np.pi * np.array([3.0, 4.0]), orc.gaussian_damping([2.0, 3.0]),
                            [np.deg2rad(200.0)]])
    group = np.array([0, 1, 0], dtype=np.int32)
    fid = orc.model(truth, np.asarray(B.values)[:, :n], group, dt)
    axis = dims.index("time")
    x = np.moveaxis(np.broadcast_to(fid, tuple(s for i, s in enumerate(shape) if i != axis) + (n,)), -1, axis).copy()
    coords = {d: np.arange(shape[i]) * (dt if d == "time" else 2.0) for i, d in enumerate(dims)}
    da = LabeledArray(x, dims, coords, {"MHz": 123.2})
    before = x.copy()
    ds = da.xmr.fit_basis(B, groups=["s", "m", "s"], skip=2)
    assert np.array_equal(da.values, before) and da.attrs == {"MHz": 123.2}
    call = calls[0]
    assert call["axis"] == axis and call["basis"].shape == (3, n) and call["basis"].dtype == np.complex128
    assert list(call["group"]) == [0, 1, 0] and call["skip"] == 2 and call["dt"] == pytest.approx(dt, rel=1e-12)
    other = tuple(d for d in dims if d != "time")
    for k in ("amplitude", "crlb", "snr"):
        assert ds[k].dims == other + ("metabolite",), k
    for k in ("shift", "linewidth", "gaussian"):
        assert ds[k].dims == other + ("group",), k
    for k in ("phase", "rss", "status", "iters"):
        assert ds[k].dims == other, k
    for k in ("fit_data", "residuals", "raw_data"):
        assert ds[k].dims == dims and ds[k].shape == shape, k
    assert list(ds.coords["metabolite"].values) == names and list(ds.coords["group"].values) == ["s", "m"]
    for d in other:
        assert np.array_equal(ds["amplitude"].coords[d].values, coords[d])
    assert np.array_equal(ds["fit_data"].coords["time"].values, coords["time"])
    assert ds.attrs == {"MHz": 123.2, "n_free_parameters": 10, "lineshape": "voigt", "skip": 2}
    # noiseless data: the truth comes back, in the reported units, the phase wrapped into (-180, 180]
    assert np.all(ds["status"].values == 0)
    np.testing.assert_allclose(ds["amplitude"].values, np.broadcast_to(truth[:3], ds["amplitude"].shape), rtol=1e-6)
    np.testing.assert_allclose(ds["shift"].values[..., :], np.broadcast_to([2.0, -1.0], ds["shift"].shape), atol=1e-6)
    np.testing.assert_allclose(ds["linewidth"].values, np.broadcast_to([3.0, 4.0], ds["shift"].shape), rtol=1e-5)
    np.testing.assert_allclose(ds["gaussian"].values, np.broadcast_to([2.0, 3.0], ds["shift"].shape), rtol=1e-5)
    np.testing.assert_allclose(ds["phase"].values, -160.0, atol=1e-6)
    np.testing.assert_array_equal(ds["raw_data"].values, before)
    np.testing.assert_array_equal(ds["residuals"].values, before - ds["fit_data"].values)
    assert np.abs(ds["residuals"].values).max() < 1e-6
    # without the fit: the three arrays are left out, everything else stays
    ds2 = fb.fit_basis(da, B, groups=["s", "m", "s"], skip=2, return_fit=False, lineshape="lorentzian", fit_phase=False)
    assert not {"fit_data", "residuals", "raw_data"} & set(ds2.data_vars) and calls[-1]["want_fit"] is False
    assert ds2.attrs["n_free_parameters"] == 7 and ds2.attrs["lineshape"] == "lorentzian"
    assert not ds2["gaussian"].values.any() and not ds2["phase"].values.any()


def test_plain_and_transposed_bases_and_crlb(monkeypatch):
    calls = []
    monkeypatch.setattr(fb, "_run_fit", _oracle_launch(calls))
    c = orc.kernel_case(3, 1, 256, 9, n_vox=2, noise=0.05)
    da = LabeledArray(c["x"], ("voxel", "time"), {"time": np.arange(256) * c["dt"]})
    ds = fb.fit_basis(da, c["B"])  # a plain array is on the data's grid; names m0 ...; one common group
    assert list(ds.coords["metabolite"].values) == ["m0", "m1", "m2"] and list(ds.coords["group"].values) == ["all"]
    Bt = LabeledArray(c["B"].T.copy(), ("time", "metabolite"), {"time": np.arange(256) * c["dt"],
                                                                "metabolite": np.array(["a", "b", "c"])})
    ds_t = fb.fit_basis(da, Bt)
    assert list(ds_t.coords["metabolite"].values) == ["a", "b", "c"]
    assert np.array_equal(ds_t["amplitude"].values, ds["amplitude"].values)
    assert np.array_equal(calls[0]["basis"], calls[1]["basis"])
    for v in range(2):
        o = orc.fit(c["x"][v], c["B"], np.zeros(3, np.int32), c["dt"], *orc.parameters(3, 1))
        np.testing.assert_allclose(ds["crlb"].values[v], o["crlb"], rtol=1e-3)
        np.testing.assert_allclose(ds["snr"].values[v], o["snr"], rtol=1e-6)
    one = fb.fit_basis(da, LabeledArray(c["B"][0], ("time",), {"time": np.arange(256) * c["dt"]}), names=["only"])
    assert one["amplitude"].dims == ("voxel", "metabolite") and one["amplitude"].shape == (2, 1)


# ---- the selection of the GPU cases ---------------------------------------------------------------------------------------
def test_step_cases_have_no_ties_and_cover_the_tile():
    """No (case, m) pair may hinge on an accept / reject decision too close to call: the cap on excluded trials in
    tests/test_gpu_basis.py is 0."""
    frees = set()
    for name, kw in orc.step_cases():
        c = _step_case(name)
        frees.add(int(np.count_nonzero(~(c["fixed"] | (c["lo"] == c["hi"])))))
        for v in range(c["x"].shape[0]):
            for m in STEP_M:
                ref = _step_ref(name, v, m)
                assert ref["iters"] == m and ref["status"] == 1, (name, v, m)
                assert not any(abs(margin) < TIE for _, margin in ref["trials"]), (name, v, m)
    assert min(frees) + 1 <= 16 < max(frees) + 1 and max(frees) == 80 and frees >= {5, 10, 19, 22, 80}


@pytest.mark.parametrize("name", list(PARITY))
def test_scipy_converges_on_the_parity_cases(name):
    c = orc.kernel_case(**PARITY[name])
    for v in range(c["x"].shape[0]):
        o = orc.fit(c["x"][v], *_args(c))
        assert o["success"] and o["status"] in (1, 2, 3, 4), (v, o["status"])
        assert np.all(np.isfinite(o["sd"])) and np.all(o["sd"][:c["M"]] > 0)
        assert np.all(o["params"][:c["M"]] > 0)  # no amplitude ends on its bound: the standard deviations mean something


def test_shapes_of_the_second_crlb_round_are_conditioned():
    """M70G3 and M100G2 with 30 fixed amplitudes (tests/test_gpu_basis.py: more amplitudes than one round of the CRLB pass
    hands out) at the truth, over every variant and every n of N_LIST: 64 eps cond(J^T J) < 1, so _check_invariants
    compares every deviation of these shapes, those of the second round included, and does not skip."""
    import test_gpu_basis as g

    eps = np.finfo(np.float64).eps
    for shape, span in (("M70G3", (1e-11, 2.7e-2)), ("M100G2", (1e-12, 1.2e-3))):
        M, G = g.SHAPES[shape]
        held = g.FIXED_AMPLITUDES.get(shape, 0)
        seen = []
        for vi, (lineshape, fit_phase, skip, _) in enumerate(g.VARIANTS):
            P = M - held + (3 if lineshape == "voigt" else 2) * G + int(fit_phase)
            assert 65 <= P <= 80 and M > 2 * 32 * (P + 1) // P  # q_pts = 32: a second round
            for n in g.N_LIST:
                nn = P + skip if n == "P" else n
                c = orc.kernel_case(M, G, nn, 100 + vi, lineshape=lineshape, fit_phase=fit_phase, skip=skip, n_vox=2,
                                    fixed_amplitudes=held)
                free = ~(c["fixed"] | (c["lo"] == c["hi"]))
                assert np.count_nonzero(free) == P and np.count_nonzero(~free[:M]) == held
                sd, cond = orc.amplitude_sd(c["B"], c["group"], c["dt"], c["truth"], c["lo"], c["hi"], c["fixed"], skip)
                assert np.all(sd[free[:M]] > 0) and np.all(sd[~free[:M]] == 0)
                seen.append(64 * eps * cond)
        assert span[0] <= min(seen) and max(seen) <= span[1], (shape, min(seen), max(seen))
