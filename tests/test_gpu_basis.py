"""k_basis_fit (csrc/xm_basis.h) on the GPU against tests/_basis_oracle.py: invariants of every returned voxel, the first
trial steps against the restated iteration, converged parity with scipy, batch independence and degenerate voxels, and
the interface (refusals of the C ABI, the accessor, basis_model).  tests/test_basis.py pins the oracle and the selection
of the cases on the CPU."""
import functools

import numpy as np
import pytest

import _basis_oracle as orc
from test_basis import PARITY, STEP_M, TIE, _step_case, _step_ref

EPS = np.finfo(np.float64).eps

# Largest disagreement between lm_steps_basis solved by the fp64 normal equations and by least squares on the augmented
# Jacobian, per parameter in units of that parameter's path length, over orc.step_cases() x m in STEP_M: 2.46e-10
# (M = 40, G = 13, n = 2049, m = 3; tests/tool_basis_tolerance.py -> profiles/basis/tolerance.txt, CPU only, the kernel
# is not involved).  The kernel is a third summation order and a Cholesky solve of the same equations: 16 x that.
STEP_TOL_MEASURED = 2.46e-10
STEP_TOL = 16 * STEP_TOL_MEASURED
# The same two runs disagree in rss by at most 1.62e-11 relative (same tool); on top of 16 x that, the kernel's own
# summation order of the cost: the bound for rss at equal parameters that tests/test_amares.py uses.
STEP_RSS_TOL = 16 * 1.62e-11 + 1e-9

# M70G3 (P = 76 ... 80) and M100G2 with 30 amplitudes fixed (P = 74 ... 77): more than the 64 amplitudes that one round of the
# CRLB pass hands out at P >= 65 (xm_lm.h: cap = 2 q_pts lda / P), so the pass runs a second round
SHAPES = {"M1G1": (1, 1), "M3G3": (3, 3), "M12G2": (12, 2), "M40G13": (40, 13), "M70G3": (70, 3), "M100G2": (100, 2)}
FIXED_AMPLITUDES = {"M100G2": 30}
# (lineshape, fit_phase, skip, dtype): both lineshapes, the phase on and off, skip 0 and 5, both sample types
VARIANTS = (("voigt", True, 0, "complex128"), ("lorentzian", False, 5, "complex64"),
            ("voigt", False, 5, "complex128"), ("lorentzian", True, 0, "complex64"))
N_LIST = ("P", 129, 300, 2048)


def _free(c):
    return ~(c["fixed"] | (c["lo"] == c["hi"]))


def _fit(x, c, max_iter=200, ftol=1e-10, xtol=1e-10, want_fit=True):
    import torch
    from xmris_amd import device as dev

    r = dev.basis_fit(torch.from_numpy(np.ascontiguousarray(x)).to("cuda"), 1, torch.from_numpy(c["B"]).to("cuda"),
                      c["group"], c["init"], c["lo"], c["hi"], c["fixed"], dt=c["dt"], skip=c["skip"],
                      max_iter=max_iter, ftol=ftol, xtol=xtol, want_fit=want_fit)
    assert "k_basis_fit" in dev.last_kernel()
    out = {k: getattr(r, k).cpu().numpy() for k in ("params", "amp_sd", "rss", "status", "iters")}
    out["fit"] = r.fit.cpu().numpy() if want_fit else None
    assert r.n_free == np.count_nonzero(_free(c))
    return out


def _same(a, b):
    return all((a[k] is None and b[k] is None) or np.array_equal(a[k], b[k], equal_nan=True) for k in a)


def _check_invariants(out, x, c, max_iter, rows=None):
    """Every output of a voxel with status 0 / 1 recomputed from its returned parameters.  Returns the voxels checked."""
    B, group, dt, skip, lo, hi = c["B"], c["group"], c["dt"], c["skip"], c["lo"], c["hi"]
    M, free = c["M"], _free(c)
    checked = 0
    for v in (range(x.shape[0]) if rows is None else rows):
        st = int(out["status"][v])
        assert st in (0, 1, 2), (v, st)
        if st == 2:
            continue
        checked += 1
        p = out["params"][v]
        assert np.all(np.isfinite(p)), (v, p)
        v0 = orc.start_values(x[v], B, c["init"], lo, hi, c["fixed"], skip)[0]
        assert np.array_equal(p[~free], v0[~free]), (v, "a fixed parameter moved")
        assert np.all((p[free] >= lo[free]) & (p[free] <= hi[free])), (v, "outside the bounds", p)
        ref = orc.model(p, B, group, dt)
        if out["fit"] is not None:
            assert np.abs(out["fit"][v] - ref).max() <= 1e-12 * np.abs(ref).max(), (v, "fit")
        rss = float(np.sum(np.abs((x[v].astype(np.complex128) - ref)[skip:]) ** 2))
        assert abs(out["rss"][v] - rss) <= 1e-9 * rss, (v, "rss", out["rss"][v], rss)
        sd, cond = orc.amplitude_sd(B, group, dt, p, lo, hi, c["fixed"], skip)
        bound = 64 * EPS * cond
        got = out["amp_sd"][v]
        assert np.all(got[~free[:M]] == 0.0), (v, "a fixed amplitude reports a deviation")
        if bound < 1.0:  # otherwise eps cond(J^T J) promises no digit (tiny records) and the factorisation may fail
            fa = free[:M]
            err = np.abs(got[fa] - sd[fa]) / sd[fa]
            assert np.all(err <= bound), (v, "amp_sd", err.max(), bound, cond)
        assert 0 < out["iters"][v] <= max_iter
    return checked


# ---- 1. invariants of every returned voxel --------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", N_LIST, ids=[f"n{n}" for n in N_LIST])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_outputs_follow_from_returned_parameters(shape, n):
    M, G = SHAPES[shape]
    held = FIXED_AMPLITUDES.get(shape, 0)
    checked = 0
    for vi, (lineshape, fit_phase, skip, dtype) in enumerate(VARIANTS):
        P = M - held + (3 if lineshape == "voigt" else 2) * G + int(fit_phase)
        nn = P + skip if n == "P" else n  # "P": as many fitted points as free columns
        c = orc.kernel_case(M, G, nn, 100 + vi, lineshape=lineshape, fit_phase=fit_phase, skip=skip, n_vox=2,
                            fixed_amplitudes=held)
        assert np.count_nonzero(_free(c)) == P and nn - skip >= P
        x = c["x"].astype(dtype)
        for max_iter in (1, 3, 200):
            out = _fit(x, c, max_iter=max_iter)
            checked += _check_invariants(out, x, c, max_iter)
            if max_iter == 1:
                assert np.all(out["iters"] == 1) and np.all(out["status"] != 2)
            if nn == 2048 and max_iter == 200:
                assert np.all(out["status"] == 0), out["status"]
            if dtype == "complex64" and max_iter == 3:
                # complex64 samples are widened on load: bitwise what the host-widened samples give
                assert _same(out, _fit(x.astype(np.complex128), c, max_iter=max_iter))
                assert not _same(out, _fit(c["x"], c, max_iter=max_iter))
    assert checked >= 2 * len(VARIANTS)  # the max_iter = 1 launches at least


def _raw_fit(first_ptr, stride, nb, n, c, code, work, basis_dev, max_iter=200, want_fit=False, out=None, **over):
    import torch
    from xmris_amd import _lib

    M, Q = c["M"], c["init"].size
    o = out or {"params": torch.empty((nb, Q), dtype=torch.float64, device="cuda"),
                "amp_sd": torch.empty((nb, M), dtype=torch.float64, device="cuda"),
                "rss": torch.empty(nb, dtype=torch.float64, device="cuda"),
                "status": torch.empty(nb, dtype=torch.int32, device="cuda"),
                "iters": torch.empty(nb, dtype=torch.int32, device="cuda"),
                "fit": torch.empty((nb, n), dtype=torch.complex128, device="cuda") if want_fit else None}
    a = dict(group=c["group"], n_groups=c["G"], n_metab=M, init=c["init"], lo=c["lo"], hi=c["hi"], skip=c["skip"])
    a.update(over)
    host = [np.ascontiguousarray(a[k], dtype=np.float64) for k in ("init", "lo", "hi")]
    fixed = np.ascontiguousarray(c["fixed"], dtype=np.int32)
    group = np.ascontiguousarray(a["group"], dtype=np.int32)
    _lib.call("xm_basis_fit", first_ptr, stride, nb, n, float(c["dt"]), int(a["skip"]), basis_dev.data_ptr(),
              int(a["n_metab"]), group.ctypes.data, int(a["n_groups"]), *[h.ctypes.data for h in host], fixed.ctypes.data,
              max_iter, 1e-10, 1e-10, o["params"].data_ptr(), o["amp_sd"].data_ptr(), o["rss"].data_ptr(),
              o["status"].data_ptr(), o["iters"].data_ptr(), o["fit"].data_ptr() if o["fit"] is not None else None,
              work.data_ptr(), work.numel() * work.element_size(), code, torch.cuda.current_stream().cuda_stream)
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in o.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["complex64", "complex128"])
@pytest.mark.parametrize("shape,n", [("M3G3", 257), ("M12G2", 300)])
def test_strided_rows_through_the_c_abi(shape, n, dtype):
    """in_row_stride = n + 24, the first row 5 elements into the buffer, fit_data null."""
    import torch
    from xmris_amd import _lib

    M, G = SHAPES[shape]
    nb, stride = 5, n + 24
    c = orc.kernel_case(M, G, n, 42, n_vox=nb, skip=5)
    rng = np.random.default_rng(n)
    wide = (1e3 * (rng.standard_normal((nb, stride)) + 1j * rng.standard_normal((nb, stride)))).astype(dtype)
    wide[:, 5:5 + n] = c["x"].astype(dtype)
    x = np.ascontiguousarray(wide[:, 5:5 + n])
    wd = torch.from_numpy(wide).to("cuda")
    bd = torch.from_numpy(c["B"]).to("cuda")
    work = torch.zeros(256 + 8 * M, dtype=torch.uint8, device="cuda")
    code = _lib.XM_C64 if dtype == "complex64" else _lib.XM_C128
    for max_iter in (2, 200):
        got = _raw_fit(wd.data_ptr() + 5 * wd.element_size(), stride, nb, n, c, code, work, bd, max_iter=max_iter)
        ref = _fit(x, c, max_iter=max_iter, want_fit=False)
        assert _same(got, ref)
        assert _check_invariants(got, x, c, max_iter) == nb


# ---- 2. the first trial steps against the restated iteration ------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", [name for name, _ in orc.step_cases()])
def test_first_steps_match_the_restated_iteration(name):
    """params, rss, iters and status after m = 1, 2, 3, 5 trials against orc.lm_steps_basis with the same cap.  Per
    parameter the disagreement is bounded in units of the parameter's path length (sum of |change| over the accepted
    steps).  tests/test_basis.py shows that no trial of these cases is too close to call: none is excluded."""
    c = _step_case(name)
    for m in STEP_M:
        out = _fit(c["x"], c, max_iter=m)
        for v in range(c["x"].shape[0]):
            ref = _step_ref(name, v, m)
            assert not any(abs(margin) < TIE for _, margin in ref["trials"])
            assert out["iters"][v] == ref["iters"] == m and out["status"][v] == ref["status"] == 1, (m, v)
            d = np.abs(out["params"][v] - ref["params"])
            worst = np.max(np.where(ref["path"] > 0, d / np.where(ref["path"] > 0, ref["path"], 1.0), 0.0))
            print(f"{name} m={m} voxel {v}: worst |dp| / path {worst:.3e} (bound {STEP_TOL:.3e}), rss rel "
                  f"{abs(out['rss'][v] - ref['rss']) / ref['rss']:.3e}")
            assert np.all(d <= STEP_TOL * ref["path"]), (m, v, worst, np.argmax(d - STEP_TOL * ref["path"]))
            assert abs(out["rss"][v] - ref["rss"]) <= STEP_RSS_TOL * ref["rss"], (m, v)


# ---- 3. parity with the scipy oracle -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _parity_ref(name):
    c = orc.kernel_case(**PARITY[name])
    args = (c["B"], c["group"], c["dt"], c["init"], c["lo"], c["hi"], c["fixed"], c["skip"])
    return c, [orc.fit(x, *args) for x in c["x"]]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PARITY))
def test_converged_fit_matches_scipy(name):
    import xmris_amd as xm

    c, refs = _parity_ref(name)
    M, G = c["M"], c["G"]
    raw = _fit(c["x"], c)
    assert np.all(raw["status"] == 0) and np.all(raw["iters"] < 200), (raw["status"], raw["iters"])
    n = c["x"].shape[1]
    time = np.arange(n) * c["dt"]
    ds = xm.fit_basis(xm.LabeledArray(c["x"], ("voxel", "time"), {"time": time}),
                      xm.LabeledArray(c["B"], ("metabolite", "time"), {"time": time}),
                      groups=[f"g{k}" for k in c["group"]])
    np.testing.assert_array_equal(raw["params"][:, :M], ds["amplitude"].values)
    worst = 0.0
    for v, o in enumerate(refs):
        free = o["sd"] > 0
        dev_sd = np.abs(raw["params"][v] - o["params"])[free] / o["sd"][free]
        worst = max(worst, float(dev_sd.max()))
        assert np.all(dev_sd <= 1e-3), (v, dev_sd.max(), np.argmax(dev_sd))
        assert np.array_equal(raw["params"][v][~free], o["params"][~free])
        assert abs(raw["rss"][v] - o["rss"]) <= 1e-9 * o["rss"], v
        np.testing.assert_allclose(ds["crlb"].values[v], o["crlb"], rtol=1e-3, err_msg=f"voxel {v}")
        np.testing.assert_allclose(ds["snr"].values[v], o["snr"], rtol=1e-6, err_msg=f"voxel {v}")
        np.testing.assert_allclose(ds["linewidth"].values[v], o["params"][M + G:M + 2 * G] / np.pi, rtol=1e-6)
    print(f"{name}: worst |dp| / sd {worst:.3e} (bound 1e-3)")


# ---- 4. batch independence and degenerate voxels -------------------------------------------------------------------------
@pytest.mark.gpu
def test_ticket_counter_over_many_rounds():
    """5003 voxels of the smallest footprint (M = 1, n = 96): many tickets per resident workgroup; every row bitwise the
    7-voxel launch's row i % 7; twice through the C ABI on one workspace, whose counters the kernel leaves at zero."""
    import torch
    from xmris_amd import _lib

    c = orc.kernel_case(1, 1, 96, 6, n_vox=7)
    small = _fit(c["x"], c)
    assert np.all(small["status"] != 2) and len({float(r) for r in small["rss"]}) == 7
    idx = np.arange(5003) % 7
    tiled = np.ascontiguousarray(c["x"][idx])
    out = _fit(tiled, c)
    for k in small:
        assert np.array_equal(out[k], small[k][idx], equal_nan=True), k
    xd = torch.from_numpy(tiled).to("cuda")
    bd = torch.from_numpy(c["B"]).to("cuda")
    work = torch.full((66,), 0, dtype=torch.int32, device="cuda")  # 256 + 8 M bytes
    for _ in range(2):
        got = _raw_fit(xd.data_ptr(), 96, 5003, 96, c, _lib.XM_C128, work, bd, want_fit=True)
        for k in small:
            assert np.array_equal(got[k], small[k][idx], equal_nan=True), k
        assert not work.cpu().numpy()[:64].any()


@pytest.mark.gpu
def test_degenerate_voxels():
    """Zeros, a NaN sample, a metabolite that is not in the data: the kernel ends with a status and the outputs of
    DESIGN.md section 8; neighbours do not notice."""
    import xmris_amd as xm

    c = orc.kernel_case(5, 2, 300, 8, n_vox=4, absent=(3,))
    good = c["x"]
    zero = np.zeros((1, 300), complex)
    nan = good[:1].copy()
    nan[0, 17] = complex(np.nan, 0.0)
    big = np.concatenate([good[:1], zero, good[1:3], nan, good[3:]])
    keep = [0, 2, 3, 5]
    base, out = _fit(good, c), _fit(big, c)
    for k in base:
        assert np.array_equal(out[k][keep], base[k], equal_nan=True), k  # bitwise
    assert np.all(base["status"] == 0)
    assert _check_invariants(out, big, c, 200, rows=keep) == 4
    # the all-zero voxel starts and ends at zero amplitudes with status 0
    assert out["status"][1] == 0 and out["iters"][1] >= 1 and out["rss"][1] == 0.0
    assert not out["params"][1, :5].any() and np.all(np.isfinite(out["params"][1])) and not out["fit"][1].any()
    assert np.all(np.isnan(out["amp_sd"][1]))  # f, d, s and phi columns vanish: J^T J is singular
    # non-finite data: status 2, zeros, rss NaN
    assert out["status"][4] == 2 and np.isnan(out["rss"][4])
    assert not out["params"][4].any() and not out["amp_sd"][4].any() and not out["fit"][4].any()
    # the absent metabolite: a finite amplitude near 0 (the others are 0.5 ... 2), never below its bound
    a3 = base["params"][:, 3]
    assert np.all(np.isfinite(a3)) and np.all(a3 >= 0.0) and np.all(a3 < 0.05), a3

    n = 300
    time = np.arange(n) * c["dt"]
    ds = xm.fit_basis(xm.LabeledArray(big, ("voxel", "time"), {"time": time}),
                      xm.LabeledArray(c["B"], ("metabolite", "time"), {"time": time}),
                      groups=[f"g{k}" for k in c["group"]])
    crlb, snr, amp = ds["crlb"].values, ds["snr"].values, ds["amplitude"].values
    np.testing.assert_array_equal(amp, out["params"][:, :5])
    assert np.array_equal(np.isnan(crlb), np.isnan(out["amp_sd"]))  # NaN exactly where J^T J could not be factored
    assert np.all(np.isfinite(crlb[keep])) and np.all(crlb[keep][amp[keep] > 0] > 0)
    assert np.all(crlb[keep][amp[keep] == 0] == 0)
    assert np.all(crlb[4] == 0) and np.all(snr[4] == 0) and ds["phase"].values[4] == 0  # failed voxel: zeros
    assert np.all(np.isnan(crlb[1])) and np.all(snr[1] == 0)
    assert list(ds["status"].values) == [0, 0, 0, 0, 2, 0]


# ---- 5. interface --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals_leave_outputs_and_counters_untouched():
    import torch
    from xmris_amd import _lib

    M, G, n, nb = 3, 2, 64, 2
    c = orc.kernel_case(M, G, n, 4, n_vox=nb)
    xd = torch.from_numpy(c["x"]).to("cuda")
    bd = torch.from_numpy(c["B"]).to("cuda")
    work = torch.full((64 + 2 * M,), 7, dtype=torch.int32, device="cuda")
    Q = M + 3 * G + 1

    def sentinel():
        return {"params": torch.full((nb, Q), -3.5, dtype=torch.float64, device="cuda"),
                "amp_sd": torch.full((nb, M), -3.5, dtype=torch.float64, device="cuda"),
                "rss": torch.full((nb,), -3.5, dtype=torch.float64, device="cuda"),
                "status": torch.full((nb,), -9, dtype=torch.int32, device="cuda"),
                "iters": torch.full((nb,), -9, dtype=torch.int32, device="cuda"),
                "fit": torch.full((nb, n), -3.5, dtype=torch.complex128, device="cuda")}

    def bounds(q, lo=None, hi=None):
        a, b = c["lo"].copy(), c["hi"].copy()
        if lo is not None:
            a[q] = lo
        if hi is not None:
            b[q] = hi
        return dict(lo=a, hi=b)

    big = orc.kernel_case(40, 14, 128, 4, n_vox=nb)  # 40 + 3 * 14 + 1 = 83 free columns
    refusals = [
        ("group index out of range", c, dict(group=[0, 2, 1])),
        ("negative group index", c, dict(group=[0, -1, 1])),
        ("empty group", c, dict(group=[0, 0, 0])),
        ("no metabolite", c, dict(n_metab=0)),
        ("fitted points fewer than the free columns", c, dict(skip=n - 9)),
        ("NaN bound", c, bounds(M, lo=np.nan)),
        ("NaN upper bound of an amplitude", c, bounds(0, hi=np.nan)),
        ("infinite bound of a shift", c, bounds(M, hi=np.inf)),
        ("infinite bound of a damping", c, bounds(M + G, lo=-np.inf)),
        ("more than 80 free columns", big, {}),
    ]
    for what, case, over in refusals:
        o = sentinel()
        if case is big:
            o["params"] = torch.full((nb, 83), -3.5, dtype=torch.float64, device="cuda")
            o["amp_sd"] = torch.full((nb, 40), -3.5, dtype=torch.float64, device="cuda")
            o["fit"] = torch.full((nb, 128), -3.5, dtype=torch.complex128, device="cuda")
            wk = torch.full((64 + 80,), 7, dtype=torch.int32, device="cuda")
            x_, b_, n_ = torch.from_numpy(big["x"]).to("cuda"), torch.from_numpy(big["B"]).to("cuda"), 128
        else:
            wk, x_, b_, n_ = work, xd, bd, n
        with pytest.raises(_lib.XmrisHipError) as e:
            _raw_fit(x_.data_ptr(), n_, nb, n_, case, _lib.XM_C128, wk, b_, want_fit=True, out=o, **over)
        assert e.value.code == _lib.XM_ERR_INVALID_ARG, what
        for k, v in o.items():
            assert torch.all(v == (-9 if v.dtype == torch.int32 else -3.5)), (what, k)
        assert torch.all(wk == 7), what
    # and the same arguments without the fault run
    work.zero_()
    ok = _raw_fit(xd.data_ptr(), n, nb, n, c, _lib.XM_C128, work, bd, want_fit=True)
    assert np.all(ok["status"] != 2) and not work.cpu().numpy()[:64].any()


@pytest.mark.gpu
@pytest.mark.parametrize("dims,shape", [(("x", "y", "time"), (2, 3, 256)), (("time", "voxel"), (256, 6))])
def test_accessor_and_basis_model(dims, shape):
    import xmris_amd as xm

    c = orc.kernel_case(5, 2, 256, 12, n_vox=6, skip=3)
    axis = dims.index("time")
    lead = tuple(s for i, s in enumerate(shape) if i != axis)
    x = np.moveaxis(c["x"].reshape(lead + (256,)), -1, axis).copy()
    time = np.arange(256) * c["dt"]
    coords = {d: (time if d == "time" else np.arange(shape[i])) for i, d in enumerate(dims)}
    da = xm.LabeledArray(x, dims, coords)
    names = ["NAA", "Cr", "Cho", "Glu", "Lac"]
    B = xm.LabeledArray(c["B"], ("metabolite", "time"), {"time": time, "metabolite": np.array(names)})
    groups = [f"g{k}" for k in c["group"]]
    before = x.copy()
    ds = da.xmr.fit_basis(B, groups=groups, skip=3)
    assert np.array_equal(da.values, before)
    raw = _fit(c["x"], c)
    other = tuple(d for d in dims if d != "time")
    assert ds["amplitude"].dims == other + ("metabolite",) and ds["shift"].dims == other + ("group",)
    assert ds["fit_data"].dims == dims and ds["phase"].dims == other
    assert list(ds.coords["metabolite"].values) == names and list(ds.coords["group"].values) == ["g0", "g1"]
    assert ds.attrs == {"n_free_parameters": 12, "lineshape": "voigt", "skip": 3}
    np.testing.assert_array_equal(ds["amplitude"].values.reshape(6, 5), raw["params"][:, :5])
    np.testing.assert_array_equal(np.moveaxis(ds["fit_data"].values, axis, -1).reshape(6, 256), raw["fit"])
    np.testing.assert_array_equal(ds["rss"].values.reshape(6), raw["rss"])
    assert np.all(ds["status"].values == 0)
    # basis_model of the result is fit_data (the units go there and back: a few ulp)
    fid = xm.basis_model(ds["amplitude"], ds["shift"], ds["linewidth"], ds["gaussian"], ds["phase"], B, groups=groups)
    assert fid.dims == other + ("time",)
    fit = np.moveaxis(ds["fit_data"].values, axis, -1)
    assert np.abs(fid.values - fit).max() <= 1e-12 * np.abs(fit).max()
    # ... and basis_model against the oracle's model, parameters of its own
    p = c["truth"]
    got = xm.basis_model(p[:5], p[5:7], p[7:9] / np.pi, 2.0 * np.sqrt(orc.LN2 * p[9:11]) / np.pi, np.rad2deg(p[11]),
                         c["B"], groups=groups, dwell=c["dt"])
    ref = orc.model(p, c["B"], c["group"], c["dt"])
    assert got.shape == (256,) and np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
