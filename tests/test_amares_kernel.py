"""k_amares_fit (csrc/xm_amares.h) away from the one configuration tests/test_amares.py runs: 1 ... 16 peaks over the
three staging tiers, ragged and tiny records, every bound type, the first trial steps one by one, the status codes,
degenerate voxels and the ticket counter.

Most assertions here do not depend on where the iteration ends: either they recompute an output from the returned
parameters (section "invariants"), or they compare the first m trial steps with the iteration of DESIGN.md section 8
restated in numpy (tests/_amares_oracle.py: lm_steps).  CPU tests first pin those oracle pieces."""
import functools

import numpy as np
import pytest

import _amares_oracle as orc
from test_amares import _check_against_oracle

EPS = np.finfo(np.float64).eps

# Largest disagreement between lm_steps solved by the fp64 normal equations and lm_steps solved by least squares on the
# augmented Jacobian, per parameter in units of that parameter's path length, over orc.step_cases() x m in STEP_M:
# 1.32e-8 (K = 6, n = 1000, m = 1; tests/tool_amares_tolerance.py, CPU only, the kernel is not involved).  The kernel is
# a third summation order and a Cholesky solve of the same equations: 16 x that.
STEP_TOL_MEASURED = 1.32e-8
STEP_TOL = 16 * STEP_TOL_MEASURED
# The same two runs disagree in rss by at most 3.4e-10 relative (same tool); on top of 16 x that, the kernel's own
# summation order of the cost: the bound tests/test_amares.py already uses for rss at equal parameters.
STEP_RSS_TOL = 16 * 3.4e-10 + 1e-9
STEP_M = (1, 2, 3, 5)
TIE = 1e-9  # accept / reject margins below this are too close to call


def tier(P):
    """Points per staging round as lm_q_pts (xm_lm.h) states it: 2 q (P + 1) doubles within 64 KiB."""
    return 128 if P <= 31 else 64 if P <= 63 else 32


# name -> (K, kernel_case options, free parameters)
CONFIGS = {"K1": (1, {}, 5), "K2": (2, {}, 10), "K6": (6, {}, 30), "K7": (7, {}, 35), "K12": (12, {}, 60),
           "K13": (13, {}, 65), "K16": (16, {}, 80), "K16_fixed_g": (16, {"fix_g": True}, 64),
           "K7_fixed_phase": (7, {"fix_phase": True}, 28)}
N_LIST = (80, 127, 128, 129, 255, 256, 257, 1000, 3001)


def _sweep():
    out = []
    for name, (K, _, P) in CONFIGS.items():
        n_min = 0 if K <= 2 else 127 if P <= 31 else 255
        for n in sorted(set((P, P + 1) + N_LIST if K <= 2 else N_LIST)):
            if n >= max(P, n_min):
                out.append((name, n))
    return out


SWEEP = _sweep()
TIMING = ((0.0, 1e-4), (5e-4, 1e-4), (0.0, 1.25e-4), (3e-4, 1.25e-4))  # (t0, dt)


# ---- CPU: the oracle pieces, before they judge the kernel ---------------------------------------------------------------
def test_sweep_contains_every_tier_ragged_and_whole():
    seen = {(tier(CONFIGS[name][2]), n % tier(CONFIGS[name][2]) == 0) for name, n in SWEEP}
    assert seen == {(q, whole) for q in (128, 64, 32) for whole in (True, False)}
    P = sorted({CONFIGS[name][2] for name, _ in SWEEP})
    assert {5, 10, 28, 30, 35, 60, 64, 65, 80} == set(P)  # both sides of 31 | 32 and 63 | 64, holes in col[], the ends
    for name, (K, kw, p) in CONFIGS.items():
        c = orc.kernel_case(K, 300, 0, **kw)
        assert np.count_nonzero(~(c["fixed"] | (c["lo"] == c["hi"]))) == p, name
    # entries per thread of the (P+1)(P+2)/2 - 1 triangle: 1 ... 13
    assert {-(-((p + 1) * (p + 2) // 2 - 1) // 256) for p in P} >= {1, 2, 3, 8, 9, 13}
    assert any(n < 256 for _, n in SWEEP) and any(n == CONFIGS[name][2] for name, n in SWEEP)


def test_kernel_case_mixes_all_bound_types():
    c = orc.kernel_case(4, 512, 3)
    lo, hi = c["lo"], c["hi"]
    kinds = {(bool(np.isfinite(a)), bool(np.isfinite(b))) for a, b in zip(lo.ravel(), hi.ravel())}
    assert kinds == {(True, True), (True, False), (False, True), (False, False)}
    assert np.all((c["truth"][:, 4] > 0) & (c["truth"][:, 4] < 1)) and c["t"][0] > 0
    assert np.all((c["init"] >= lo) & (c["init"] <= hi)) and not np.array_equal(c["init"], c["truth"])
    again = orc.kernel_case(4, 512, 3)
    assert all(np.array_equal(c[k], again[k]) for k in ("x", "init", "lo", "hi", "fixed"))


@pytest.mark.parametrize("which", ["notebook", "K8"])
def test_lm_steps_converges_to_minpack(which):
    if which == "notebook":
        data, t, mhz = orc.notebook_dataset()
        init, lo, hi = orc.notebook_pk(mhz)
        fixed = None
    else:
        c = orc.kernel_case(8, 1537, 11, n_vox=1)
        data, t, init, lo, hi, fixed = c["x"], c["t"], c["init"], c["lo"], c["hi"], c["fixed"]
    for x in data:
        o = orc.fit(x, t, init, lo, hi, fixed)
        assert o["ier"] in (1, 2, 3)
        for solver in ("normal", "qr"):
            r = orc.lm_steps(x, t, init, lo, hi, fixed, solver=solver)
            assert r["status"] == 0 and r["iters"] < 200 and len(r["trials"]) == r["iters"]
            free = o["sd"] > 0
            assert np.all(np.abs(r["params"] - o["params"])[free] <= 1e-3 * o["sd"][free]), solver
            assert np.array_equal(r["params"][~free], o["params"][~free])
            assert abs(r["rss"] - o["rss"]) <= 1e-9 * o["rss"]


@pytest.mark.parametrize("kind", ["free", "lo", "hi", "two"])
def test_normal_equations_internal_against_finite_differences(kind):
    """J^T r and J^T J in the internal variables against a central difference of the residual in u, with every
    parameter of a 2-peak case given the bound type under test."""
    c = orc.kernel_case(2, 200, 5)
    p = c["init"].copy()
    lo, hi = np.full((2, 5), -np.inf), np.full((2, 5), np.inf)
    if kind in ("lo", "two"):
        lo = p - np.array([3.0, 40.0, 20.0, 1.0, 0.4])
    if kind in ("hi", "two"):
        hi = p + np.array([4.0, 70.0, 30.0, 2.0, 0.3])
    x, t = c["x"][0], c["t"]
    H, g, F = orc.normal_equations(x, t, p, lo, hi, None, internal=True)
    v0, u = orc.start_values(p, lo, hi)
    np.testing.assert_allclose(orc.physical(u, v0, lo, hi)[0], p.ravel(), rtol=1e-12)

    def res(uu):
        return orc.real_rows(x - orc.model(orc.physical(uu, v0, lo, hi)[0], t))

    jfd = np.zeros((2 * len(t), u.size))
    for j in range(u.size):
        h = 1e-6 * max(1.0, abs(u[j]))
        e = np.zeros(u.size)
        e[j] = h
        jfd[:, j] = -(res(u + e) - res(u - e)) / (2 * h)  # d model / du = -d r / du
    r = res(u)
    assert abs(F - r @ r) <= 1e-12 * F
    scale = np.sqrt(np.diag(H))
    np.testing.assert_allclose(jfd.T @ jfd / np.outer(scale, scale), H / np.outer(scale, scale), atol=1e-7)
    np.testing.assert_allclose(jfd.T @ r / scale, g / scale, atol=1e-7 * np.linalg.norm(r))
    Hp, gp, _ = orc.normal_equations(x, t, p, lo, hi, None, internal=False)
    if kind == "free":
        assert np.array_equal(H, Hp) and np.array_equal(g, gp)
    else:
        assert not np.allclose(H, Hp)


@functools.lru_cache(maxsize=None)
def _step_case(name):
    return orc.kernel_case(**dict(orc.step_cases())[name])


@functools.lru_cache(maxsize=None)
def _step_ref(name, v, m, ftol=1e-10, xtol=1e-10):
    c = _step_case(name)
    return orc.lm_steps(c["x"][v], c["t"], c["init"], c["lo"], c["hi"], c["fixed"], max_iter=m, ftol=ftol, xtol=xtol)


def _too_close(ref):
    return any(abs(margin) < TIE for _, margin in ref["trials"])


def test_step_cases_leave_few_ties():
    """At most 1 in 20 (case, m) pairs may hinge on an accept / reject decision too close to call (reference only)."""
    pairs = [(name, m) for name, _ in orc.step_cases() for m in STEP_M]
    excluded = [(name, m) for name, m in pairs
                if any(_too_close(_step_ref(name, v, m)) for v in range(_step_case(name)["x"].shape[0]))]
    assert 20 * len(excluded) <= len(pairs), excluded
    kinds = set()
    for name, kw in orc.step_cases():
        c = _step_case(name)
        for k, col, side in kw.get("on_bound", ()):
            kinds.add((bool(np.isfinite(c["lo"][k, col])), bool(np.isfinite(c["hi"][k, col])), side))
    assert kinds >= {(True, False, "lo"), (False, True, "hi"), (True, True, "lo"), (True, True, "hi")}
    assert {kw["K"] for _, kw in orc.step_cases()} >= {1, 6, 7, 13, 16}


# ---- GPU helpers --------------------------------------------------------------------------------------------------------
def _fit(x, c, max_iter=200, ftol=1e-10, xtol=1e-10, want_fit=True):
    import torch
    from xmris_amd import device as dev

    r = dev.amares_fit(torch.from_numpy(np.ascontiguousarray(x)).to("cuda"), 1, c["init"], c["lo"], c["hi"], c["fixed"],
                       dt=c["dt"], t0=c["t0"], max_iter=max_iter, ftol=ftol, xtol=xtol, want_fit=want_fit)
    assert "k_amares_fit" in dev.last_kernel()
    out = {k: getattr(r, k).cpu().numpy() for k in ("params", "amp_sd", "rss", "status", "iters")}
    out["fit"] = r.fit.cpu().numpy() if want_fit else None
    return out


def _same(a, b):
    return all((a[k] is None and b[k] is None) or np.array_equal(a[k], b[k], equal_nan=True) for k in a)


def _check_invariants(out, x, c, rows=None):
    """Every output of a voxel with status 0 / 1 recomputed from its returned parameters.  Returns the voxels checked."""
    t, lo, hi = c["t"], c["lo"], c["hi"]
    fixed = c["fixed"] | (lo == hi)
    v0 = np.clip(c["init"], lo, hi)
    checked = 0
    for v in (range(x.shape[0]) if rows is None else rows):
        st = int(out["status"][v])
        assert st in (0, 1, 2), (v, st)
        if st == 2:
            continue
        checked += 1
        p = out["params"][v]
        assert np.all(np.isfinite(p)), (v, p)
        assert np.array_equal(p[fixed], v0[fixed]), (v, "a fixed parameter moved")
        assert np.all((p >= lo) & (p <= hi)), (v, "outside the bounds", p)
        ref = orc.model(p, t)
        if out["fit"] is not None:
            assert np.abs(out["fit"][v] - ref).max() <= 1e-12 * np.abs(ref).max(), (v, "fit")
        rss = float(np.sum(np.abs(x[v].astype(np.complex128) - ref) ** 2))
        assert abs(out["rss"][v] - rss) <= 1e-9 * rss, (v, "rss", out["rss"][v], rss)
        sd, cond = orc.amplitude_sd(t, p, lo, hi, fixed)
        bound = 64 * EPS * cond
        got = out["amp_sd"][v]
        assert np.all(got[fixed[:, 0]] == 0.0), (v, "a fixed amplitude reports a deviation")
        if bound < 1.0:  # otherwise eps cond(J^T J) promises no digit (tiny records) and the factorisation may fail
            free = ~fixed[:, 0]
            err = np.abs(got[free] - sd[free]) / sd[free]
            assert np.all(err <= bound), (v, "amp_sd", err.max(), bound, cond)
        assert 0 < out["iters"][v] <= 200
    return checked


# ---- GPU: invariants of every returned voxel ----------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,n", SWEEP, ids=[f"{a}-n{b}" for a, b in SWEEP])
def test_outputs_follow_from_returned_parameters(name, n):
    K, kw, P = CONFIGS[name]
    checked = 0
    for ti, (t0, dt) in enumerate(TIMING):
        c = orc.kernel_case(K, n, 100 + ti, dt=dt, t0=t0, n_vox=2, **kw)
        for max_iter in (1, 3, 200):
            out = _fit(c["x"], c, max_iter=max_iter)
            checked += _check_invariants(out, c["x"], c)
            assert np.all(out["iters"] <= max_iter)
            if max_iter == 1:
                assert np.all(out["iters"] == 1) and np.all(out["status"] != 2)
            if n * dt >= 0.025:
                assert np.all(out["status"] != 2)
            if max_iter == 200 and n >= 1000:
                assert np.all(out["status"] == 0), out["status"]
            if ti == 1 and max_iter != 1:
                # complex64 samples are widened on load: bitwise what the host-widened samples give
                x32 = c["x"].astype(np.complex64)
                a, b = _fit(x32, c, max_iter=max_iter), _fit(x32.astype(np.complex128), c, max_iter=max_iter)
                assert _same(a, b)
                checked += _check_invariants(a, x32, c)
                assert not _same(a, out)
    assert checked >= 2 * len(TIMING)  # the max_iter = 1 launches at least


def _raw_fit(first_ptr, stride, nb, c, code, work, max_iter=200, want_fit=False):
    import torch
    from xmris_amd import _lib

    K = c["init"].shape[0]
    n = len(c["t"])
    o = {"params": torch.empty((nb, K, 5), dtype=torch.float64, device="cuda"),
         "amp_sd": torch.empty((nb, K), dtype=torch.float64, device="cuda"),
         "rss": torch.empty(nb, dtype=torch.float64, device="cuda"),
         "status": torch.empty(nb, dtype=torch.int32, device="cuda"),
         "iters": torch.empty(nb, dtype=torch.int32, device="cuda"),
         "fit": torch.empty((nb, n), dtype=torch.complex128, device="cuda") if want_fit else None}
    host = [np.ascontiguousarray(c[k], dtype=np.float64) for k in ("init", "lo", "hi")]
    fixed = np.ascontiguousarray(c["fixed"], dtype=np.int32)
    _lib.call("xm_amares_fit", first_ptr, stride, nb, n, float(c["dt"]), float(c["t0"]), K,
              *[a.ctypes.data for a in host], fixed.ctypes.data, max_iter, 1e-10, 1e-10, o["params"].data_ptr(),
              o["amp_sd"].data_ptr(), o["rss"].data_ptr(), o["status"].data_ptr(), o["iters"].data_ptr(),
              o["fit"].data_ptr() if want_fit else None, work.data_ptr(), work.numel() * work.element_size(), code,
              torch.cuda.current_stream().cuda_stream)
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in o.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["complex64", "complex128"])
@pytest.mark.parametrize("name,n", [("K2", 257), ("K7", 1000), ("K13", 1000), ("K1", 96)])
def test_strided_rows_through_the_c_abi(name, n, dtype):
    """in_row_stride = n + 24, the first row 5 elements into the buffer, fit_data null."""
    import torch
    from xmris_amd import _lib
    from xmris_amd import device as dev

    K, kw, _ = CONFIGS[name]
    nb, stride = 5, n + 24
    c = orc.kernel_case(K, n, 42, n_vox=nb, **kw)
    rng = np.random.default_rng(n)
    wide = (1e3 * (rng.standard_normal((nb, stride)) + 1j * rng.standard_normal((nb, stride)))).astype(dtype)
    wide[:, 5:5 + n] = c["x"].astype(dtype)
    x = np.ascontiguousarray(wide[:, 5:5 + n])
    wd = torch.from_numpy(wide).to("cuda")
    work = torch.zeros(256, dtype=torch.uint8, device="cuda")
    code = _lib.XM_C64 if dtype == "complex64" else _lib.XM_C128
    for max_iter in (2, 200):
        got = _raw_fit(wd.data_ptr() + 5 * wd.element_size(), stride, nb, c, code, work, max_iter=max_iter)
        assert "k_amares_fit" in dev.last_kernel()
        ref = _fit(x, c, max_iter=max_iter, want_fit=False)
        assert _same(got, ref)
        assert _check_invariants(got, x, c) == nb


# ---- GPU: the first trial steps against the restated iteration --------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", [name for name, _ in orc.step_cases()])
def test_first_steps_match_the_restated_iteration(name):
    """params, rss, iters and status after m = 1, 2, 3, 5 trials against orc.lm_steps with the same cap.  Per parameter
    the disagreement is bounded in units of the parameter's path length (sum of |change| over the accepted steps);
    a parameter that starts on a bound has slope 0 and must not move at all."""
    c = _step_case(name)
    lo, hi = c["lo"], c["hi"]
    v0, _ = orc.start_values(c["init"], lo, hi, c["fixed"])
    on_bound = dict(orc.step_cases())[name].get("on_bound", ())
    excluded = 0
    for m in STEP_M:
        out = _fit(c["x"], c, max_iter=m)
        for v in range(c["x"].shape[0]):
            ref = _step_ref(name, v, m)
            for k, col, side in on_bound:
                u = orc.to_internal(v0[5 * k + col], lo[k, col], hi[k, col])
                assert out["params"][v, k, col] == orc.from_internal(u, lo[k, col], hi[k, col])[0], (m, v, k, col)
                assert ref["path"][5 * k + col] == 0.0
            if _too_close(ref):
                excluded += 1
                continue
            assert out["iters"][v] == ref["iters"] == m and out["status"][v] == ref["status"] == 1, (m, v)
            d = np.abs(out["params"][v].ravel() - ref["params"].ravel())
            worst = np.max(np.where(ref["path"] > 0, d / np.where(ref["path"] > 0, ref["path"], 1.0), 0.0))
            print(f"{name} m={m} voxel {v}: worst |dp| / path {worst:.3e} (bound {STEP_TOL:.3e}), rss rel "
                  f"{abs(out['rss'][v] - ref['rss']) / ref['rss']:.3e}")
            assert np.all(d <= STEP_TOL * ref["path"]), (m, v, worst, np.argmax(d - STEP_TOL * ref["path"]))
            assert abs(out["rss"][v] - ref["rss"]) <= STEP_RSS_TOL * ref["rss"], (m, v)
    assert 20 * excluded <= len(STEP_M) * c["x"].shape[0]


# ---- GPU: convergence parity at the sizes test_amares.py does not reach -------------------------------------------------
def _pk_csv(c, mhz):
    """The case's prior knowledge in the notebook's CSV layout (file units: ppm, Hz linewidth, degrees)."""
    K = c["init"].shape[0]
    unit = np.array([1.0, 1.0 / mhz, 1.0 / np.pi, 180.0 / np.pi, 1.0])
    init, lo, hi = c["init"] * unit, c["lo"] * unit, c["hi"] * unit
    num = lambda v: "" if np.isinf(v) else repr(float(v))  # noqa: E731
    lines = ["Index," + ",".join(f"p{k}" for k in range(K)), "Initial Values" + "," * K]
    lines += [row + "," + ",".join(repr(float(init[k, col])) for k in range(K)) for col, row in
              enumerate(("amplitude", "chemicalshift", "linewidth", "phase", "g"))]
    lines += ["Bounds" + "," * K]
    lines += [row + "," + ",".join(f'"({num(lo[k, col])}, {num(hi[k, col])})"' for k in range(K)) for col, row in
              enumerate(("amplitude", "chemicalshift", "linewidth", "phase", "g"))]
    return "\n".join(lines) + "\n"


@pytest.mark.gpu
@pytest.mark.parametrize("K,n,dtype", [(7, 1000, "complex128"), (7, 1000, "complex64"), (12, 1537, "complex128"),
                                       (13, 1000, "complex128"), (16, 3001, "complex128")])
def test_converged_fit_matches_minpack(tmp_path, K, n, dtype):
    import xmris_amd as xm
    from xmris_amd.fitting.prior_knowledge import read_prior_knowledge

    mhz = 120.0
    c = orc.kernel_case(K, n, 21, n_vox=2)
    pk_file = tmp_path / "pk.csv"
    pk_file.write_text(_pk_csv(c, mhz))
    pk = read_prior_knowledge(pk_file)
    init, lo, hi = pk.fitting_units(mhz)  # what the file says, conversions included
    assert not pk.fixed.any() and np.allclose(init, c["init"], rtol=1e-12, atol=1e-12)
    data = c["x"].astype(dtype)
    ds = xm.fit_amares(xm.LabeledArray(data, ("v", "time"), {"time": c["t"]}, {"MHz": mhz}), pk_file,
                       sw=1.0 / c["dt"], deadtime=c["t0"])
    x = data.astype(np.complex128)
    _check_against_oracle({k: np.asarray(a.values) for k, a in ds.data_vars.items()}, x, c["t"], mhz, init, lo, hi)
    raw = _fit(data, dict(c, init=init, lo=lo, hi=hi))
    assert np.all(raw["status"] == 0) and np.all(raw["iters"] < 200), (raw["status"], raw["iters"])
    np.testing.assert_array_equal(raw["params"][..., 0], ds["amplitude"].values)


# ---- GPU: status, cap, degenerate voxels ----------------------------------------------------------------------------------
@pytest.mark.gpu
def test_iteration_cap_and_tolerances():
    name = "K6_n1000"
    c = _step_case(name)
    full = _fit(c["x"], c)
    assert np.all(full["status"] == 0) and np.all(full["iters"] > 5) and np.all(full["iters"] < 100)
    for m in (1, 4):  # a start that needs more trials than that
        out = _fit(c["x"], c, max_iter=m)
        assert np.all(out["status"] == 1) and np.all(out["iters"] == m)
        assert _check_invariants(out, c["x"], c) == c["x"].shape[0]
        assert np.all(out["rss"] > full["rss"])
    # ftol = xtol = 0: no stopping rule can fire while steps are accepted, so the cap just past the default run's end
    m = int(full["iters"].max()) + 1
    out = _fit(c["x"], c, max_iter=m, ftol=0.0, xtol=0.0)
    assert np.all(out["status"] == 1) and np.all(out["iters"] == m), (out["status"], out["iters"])
    assert _check_invariants(out, c["x"], c) == c["x"].shape[0]
    # at the full cap the iteration ends only by a zero step or an overflowing lambda, both far past the default run
    out = _fit(c["x"], c, ftol=0.0, xtol=0.0)
    assert np.all(out["iters"] > full["iters"] + 20) and np.all(np.isin(out["status"], (0, 1)))
    assert np.all(out["rss"] <= full["rss"]) and np.all(out["rss"] >= full["rss"] * (1 - 1e-6))
    assert _check_invariants(out, c["x"], c) == c["x"].shape[0]
    # ftol = 1: the first accepted step ends the fit
    out = _fit(c["x"], c, ftol=1.0)
    for v in range(c["x"].shape[0]):
        ref = _step_ref(name, v, 200, ftol=1.0)
        assert [a for a, _ in ref["trials"]].count(True) == 1 and ref["trials"][-1][0] and ref["status"] == 0
        assert not _too_close(ref)
        assert out["status"][v] == 0 and out["iters"][v] == ref["iters"]
        assert np.all(np.abs(out["params"][v].ravel() - ref["params"].ravel()) <= STEP_TOL * ref["path"])
    assert _check_invariants(out, c["x"], c) == c["x"].shape[0]


@pytest.mark.gpu
def test_degenerate_voxels(tmp_path):
    """Zeros, a peak whose amplitude sits on its bound 0, infinities: the kernel terminates with a status and finite
    parameters; an undefined CRLB is NaN; neighbours do not notice."""
    import xmris_amd as xm

    mhz = 120.0
    c = orc.kernel_case(2, 300, 8, n_vox=4)
    good = c["x"]
    zero = np.zeros((1, 300), complex)
    inf = good[:1].copy()
    inf[0, 17] = complex(np.inf, 0.0)
    big = np.concatenate([good[:1], zero, good[1:3], inf, good[3:]])
    keep = [0, 2, 3, 5]
    base, out = _fit(good, c), _fit(big, c)
    for k in base:
        assert np.array_equal(out[k][keep], base[k], equal_nan=True), k  # bitwise
    assert np.all(base["status"] == 0)
    assert out["status"][1] in (0, 1) and 0 < out["iters"][1] <= 200 and np.all(np.isfinite(out["params"][1]))
    assert np.isfinite(out["rss"][1]) and out["rss"][1] <= 1e-12 and np.all(out["params"][1, :, 0] >= 0)
    assert np.all(np.isnan(out["amp_sd"][1]) | (out["amp_sd"][1] > 0))
    assert _check_invariants(out, big, c, rows=[0, 2, 3, 5]) == 4
    assert out["status"][4] == 2 and np.isnan(out["rss"][4])
    assert not out["params"][4].any() and not out["amp_sd"][4].any() and not out["fit"][4].any()

    def through_fit_amares(case, data):
        f = tmp_path / "pk.csv"
        f.write_text(_pk_csv(case, mhz))
        return xm.fit_amares(xm.LabeledArray(data, ("v", "time"), {"time": case["t"]}, {"MHz": mhz}), f,
                             sw=1.0 / case["dt"], deadtime=case["t0"])

    ds = through_fit_amares(c, big)
    crlb, snr = ds["crlb"].values, ds["snr"].values
    assert np.all(np.isfinite(crlb[keep])) and np.all(crlb[keep] > 0)
    assert np.all(crlb[4] == 0) and np.all(snr[4] == 0)  # failed voxel: zeros
    # the all-zero voxel: NaN exactly where the kernel could not factor J^T J, else a finite figure; never an exception
    undefined = np.isnan(out["amp_sd"][1])
    assert np.array_equal(np.isnan(crlb[1]), undefined) and np.all(np.isfinite(snr[1]))
    assert np.all(crlb[1][~undefined] >= 0)

    # peak 0 starts on its amplitude bound 0 and stays: its f, d, phi, g columns of the physical Jacobian vanish
    c0 = orc.kernel_case(2, 300, 8, n_vox=4, on_bound=((0, 0, "lo"),))
    out0 = _fit(c0["x"], c0)
    assert np.all(out0["params"][:, 0, 0] == 0.0) and np.all(np.isin(out0["status"], (0, 1)))
    assert np.all(np.isfinite(out0["params"])) and np.all(np.isfinite(out0["rss"]))
    assert np.all(np.isnan(out0["amp_sd"]))  # singular J^T J: no deviation for any amplitude of the voxel
    for v in range(4):  # everything else still follows from the returned parameters
        ref = orc.model(out0["params"][v], c0["t"])
        assert np.abs(out0["fit"][v] - ref).max() <= 1e-12 * np.abs(ref).max()
        rss = float(np.sum(np.abs(c0["x"][v] - ref) ** 2))
        assert abs(out0["rss"][v] - rss) <= 1e-9 * rss
    ds0 = through_fit_amares(c0, c0["x"])
    assert np.all(np.isnan(ds0["crlb"].values)) and np.all(np.isfinite(ds0["snr"].values))
    assert np.all(ds0["amplitude"].values[:, 0] == 0.0) and np.all(ds0["snr"].values[:, 0] == 0.0)


# ---- GPU: persistent grid ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_ticket_counter_over_many_rounds():
    """5003 voxels of the smallest footprint (K = 1, n = 96): many tickets per resident workgroup; every row bitwise the
    7-voxel launch's row i % 7; twice through the C ABI on one workspace, which the kernel leaves at zero."""
    import torch
    from xmris_amd import _lib

    c = orc.kernel_case(1, 96, 6, n_vox=7)
    small = _fit(c["x"], c)
    assert np.all(small["status"] != 2) and len({float(r) for r in small["rss"]}) == 7
    idx = np.arange(5003) % 7
    tiled = np.ascontiguousarray(c["x"][idx])
    out = _fit(tiled, c)
    for k in small:
        assert np.array_equal(out[k], small[k][idx], equal_nan=True), k
    xd = torch.from_numpy(tiled).to("cuda")
    work = torch.full((64,), 0, dtype=torch.int32, device="cuda")
    for _ in range(2):
        got = _raw_fit(xd.data_ptr(), 96, 5003, c, _lib.XM_C128, work, want_fit=True)
        for k in small:
            assert np.array_equal(got[k], small[k][idx], equal_nan=True), k
        assert not work.cpu().numpy().any()
