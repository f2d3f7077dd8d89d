"""k_kinetics_fit (csrc/xm_kinetics.h) on the GPU against tests/_kinetics_oracle.py: the first trial steps against the
restated iteration, converged parity with scipy, invariants of every returned row, batch independence, degenerate rows,
the refusals of the C ABI with real buffers, and the public call.  tests/test_kinetics.py pins the oracle and the
selection of the cases on the CPU."""
import numpy as np
import pytest

import _kinetics_oracle as orc
from test_kinetics import PARITY, STEP_M, TIE, _parity_case, _parity_ref, _step_case, _step_ref

EPS = np.finfo(np.float64).eps

# tests/tool_kinetics_tolerance.py -> profiles/kinetics/tolerance.txt (CPU only, the kernel is not involved):
# (a) the model and its columns in scan order against the sequential recurrence: 8.179e-16 of the column's largest value.
# The kernel is a further order (FMAs, its own exp): 16 x that.
SCAN_TOL_MEASURED = 8.179e-16
SCAN_TOL = 16 * SCAN_TOL_MEASURED
# (b) lm_steps_kinetics by the normal equations against least squares on the augmented Jacobian, per parameter in units
# of its path length: 2.660e-11; the kernel is a third summation order and a Cholesky solve: 16 x that.
STEP_TOL_MEASURED = 2.660e-11
STEP_TOL = 16 * STEP_TOL_MEASURED
# The same two runs disagree in rss by 2.672e-12 relative; 16 x that, plus the cost's own sensitivity to the model's
# order: d rss <= 2 sqrt(rss) ||w|| max|model| SCAN_TOL (Cauchy-Schwarz), added per row by _rss_slack.
STEP_RSS_TOL = 16 * 2.672e-12


def _fit(c, rows=None, max_iter=200, want_fit=True, **over):
    """The case `c` (or its voxels `rows`) through device.kinetics_fit; every output as numpy."""
    import torch
    from xmris_amd import device as dev

    rows = np.arange(c["S"].shape[0]) if rows is None else np.asarray(rows)
    a = dict(init=c["init"], lo=c["lo"], hi=c["hi"], fixed=c["fixed"])
    a.update(over)
    to = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to("cuda")  # noqa: E731
    r = dev.kinetics_fit(to(c["S"][rows]), to(c["Y"][rows]), c["t"], c["ths"], c["thp"], a["init"], a["lo"], a["hi"],
                         a["fixed"], weights=to(c["w"][rows]) if c["w"] is not None else None, max_iter=max_iter,
                         want_fit=want_fit)
    assert "k_kinetics_fit" in dev.last_kernel()
    out = {k: getattr(r, k).cpu().numpy() for k in ("params", "param_sd", "rss", "status", "iters", "auc_ratio")}
    out["fit"] = r.fit.cpu().numpy() if want_fit else None
    return out


def _same(a, b, rows_a=slice(None), rows_b=slice(None)):
    return all((a[k] is None and b[k] is None) or np.array_equal(a[k][rows_a], b[k][rows_b], equal_nan=True) for k in a)


def _rss_slack(it, ref_model):
    w = np.where(it["w"] > 0, it["w"], 0.0)
    return lambda rss: 2.0 * np.sqrt(rss) * np.linalg.norm(w) * np.abs(ref_model).max() * SCAN_TOL + 4 * len(w) * EPS * rss


def _check_invariants(out, c, max_iter, over=None):
    """Every output of a row with status 0 / 1 recomputed from its returned parameters.  Returns (rows checked, the
    largest share of a bound that any figure reached)."""
    checked, share = 0, 0.0
    cc = dict(c, **(over or {}))
    for v in range(out["status"].shape[0]):
        for m in range(c["M"]):
            st = int(out["status"][v, m])
            assert st in (0, 1, 2, 3), (v, m, st)
            if st >= 2:
                continue
            checked += 1
            it = orc.item(cc, v, m)
            p = out["params"][v, m]
            lo, hi, fixed, free = orc._split(it["lo"], it["hi"], it["fixed"])
            assert np.all(np.isfinite(p)) and np.all((p >= lo) & (p <= hi)), (v, m, p)
            v0 = orc.start_values(it["Y"], it["w"], it["thp"], it["init"], lo, hi, fixed)[0]
            assert np.array_equal(p[fixed], v0[fixed]), (v, m, "a fixed parameter moved")
            ref = orc.model(p, it["S"], it["t"], it["ths"], it["thp"])
            if out["fit"] is not None:
                err = np.abs(out["fit"][v, m] - ref).max() / np.abs(ref).max() if np.abs(ref).max() > 0 else 0.0
                share = max(share, err / SCAN_TOL)
                assert err <= SCAN_TOL, (v, m, "fit", err)
            rss = orc.cost(p, it)
            slack = _rss_slack(it, ref)(rss)
            share = max(share, abs(out["rss"][v, m] - rss) / slack if slack > 0 else 0.0)
            assert abs(out["rss"][v, m] - rss) <= slack, (v, m, "rss", out["rss"][v, m], rss)
            # the trapezoid sums: T terms each, summed in another order
            on = it["w"] > 0
            want = orc.auc_ratio(it["S"], it["Y"], it["w"], it["t"])
            if np.isfinite(want):
                tt = it["t"][on]
                spread = sum(np.sum(np.abs(0.5 * np.diff(tt) * (x[on][1:] + x[on][:-1]))) /
                             abs(np.sum(0.5 * np.diff(tt) * (x[on][1:] + x[on][:-1]))) for x in (it["S"], it["Y"]))
                tol = 2 * len(tt) * EPS * spread * abs(want)
                share = max(share, abs(out["auc_ratio"][v, m] - want) / tol)
                assert abs(out["auc_ratio"][v, m] - want) <= tol, (v, m, "auc", out["auc_ratio"][v, m], want)
            # the covariance: Cholesky of J^T W J is as good as eps cond; the columns carry the scan's own error; and the
            # factor sqrt(rss / (T_w - P)) carries half the relative error that rss is allowed above
            sd, cond = orc.covariance_sd(p, it)
            got = out["param_sd"][v, m]
            assert np.all(got[fixed] == 0.0), (v, m, "a fixed parameter reports a deviation")
            bound = cond * (64 * EPS + 4 * SCAN_TOL) + (0.5 * slack / rss if rss > 0 else 0.0)
            if np.all(np.isnan(sd[free])):
                assert np.all(np.isnan(got[free])), (v, m, got)
            elif bound < 1.0:
                err = np.max(np.abs(got[free] - sd[free]) / sd[free])
                share = max(share, err / bound)
                assert err <= bound, (v, m, "param_sd", err, bound, cond)
            assert 0 < out["iters"][v, m] <= max_iter
    return checked, share


# ---- (a) the first trial steps against the restated iteration ----------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n, _ in orc.step_cases()])
def test_first_steps_match_the_restated_iteration(name):
    """params, rss, iters and status after m = 1, 2, 3 trials against orc.lm_steps_kinetics with the same cap.  Per
    parameter the disagreement is bounded in units of the parameter's path length.  tests/test_kinetics.py shows that no
    trial of these cases is too close to call: none is excluded."""
    c = _step_case(name)
    for steps in STEP_M:
        out = _fit(c, max_iter=steps)
        worst, worst_rss = 0.0, 0.0
        for v in range(c["S"].shape[0]):
            for m in range(c["M"]):
                ref = _step_ref(name, v, m, steps)
                assert not any(abs(margin) < TIE for _, margin in ref["trials"])
                assert out["iters"][v, m] == ref["iters"] == steps and out["status"][v, m] == ref["status"] == 1, (steps, v, m)
                d = np.abs(out["params"][v, m] - ref["params"])
                on = ref["path"] > 0
                assert np.array_equal(out["params"][v, m][~on], ref["params"][~on])
                worst = max(worst, float(np.max(d[on] / ref["path"][on])) if on.any() else 0.0)
                it = orc.item(c, v, m)
                slack = STEP_RSS_TOL * ref["rss"] + _rss_slack(it, it["Y"][it["w"] > 0])(ref["rss"])
                worst_rss = max(worst_rss, abs(out["rss"][v, m] - ref["rss"]) / slack)
                assert np.all(d <= STEP_TOL * ref["path"]), (steps, v, m, d, ref["path"])
                assert abs(out["rss"][v, m] - ref["rss"]) <= slack, (steps, v, m)
        print(f"{name} m={steps}: worst |dp| / path {worst:.3e} (bound {STEP_TOL:.3e}, share {worst / STEP_TOL:.3f}), "
              f"rss share {worst_rss:.3f}")


# ---- (b) parity with scipy ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PARITY))
def test_converged_fit_matches_scipy(name):
    c = _parity_case(name)
    out = _fit(c)
    worst, skipped, total = 0.0, 0, 0
    for v, m, o in _parity_ref(name):
        total += 1
        if not o["success"]:  # scipy itself reports non-convergence
            skipped += 1
            continue
        assert out["status"][v, m] == 0 and out["iters"][v, m] < 200, (v, m, out["status"][v, m], out["iters"][v, m])
        free = o["sd"] > 0
        dev_sd = np.abs(out["params"][v, m] - o["params"])[free] / o["sd"][free]
        worst = max(worst, float(dev_sd.max()))
        assert np.all(dev_sd <= 1e-3), (v, m, dev_sd)
        assert np.array_equal(out["params"][v, m][~free], o["params"][~free])
        assert abs(out["rss"][v, m] - o["rss"]) <= 1e-9 * o["rss"], (v, m)
        np.testing.assert_allclose(out["param_sd"][v, m][free], o["sd"][free], rtol=1e-3)
    assert skipped <= 0.02 * total
    checked, share = _check_invariants(out, c, 200)
    assert checked == total
    print(f"{name}: worst |dp| / sd {worst:.3e} (bound 1e-3), {skipped} of {total} skipped, invariants at {share:.3f} of "
          f"their bounds")


# ---- (c) invariants at every shape and iteration cap -------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("T", orc.T_LIST)
@pytest.mark.parametrize("M", [1, 4])
def test_outputs_follow_from_returned_parameters(T, M):
    rf, zf = orc.free_for(T)
    checked, share = 0, 0.0
    for vi, kw in enumerate((dict(), dict(uniform=False, flip_per_rep=True, missing=0.2 if T >= 63 else 0.0))):
        c = orc.kinetic_case(T, M, 200 + vi, rho_free=rf, z_free=zf, **kw)
        for max_iter in (1, 3, 200):
            out = _fit(c, max_iter=max_iter)
            n, s = _check_invariants(out, c, max_iter)
            checked, share = checked + n, max(share, s)
            if max_iter == 1:
                assert np.all(out["iters"] == 1) and np.all(out["status"] == 1)
            assert _same(_fit(c, max_iter=max_iter, want_fit=False), dict(out, fit=None))
    assert checked == 2 * 3 * 2 * M
    print(f"T={T} M={M}: invariants at {share:.3f} of their bounds")


# ---- (d) batch independence ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("T,M", [(30, 1), (65, 4), (256, 1)])
def test_a_row_does_not_depend_on_its_batch(T, M):
    """A row's result is bitwise the same alone, in a batch of 5 and in a batch of 1031 (not a multiple of the four waves
    of a workgroup), where with M = 1 row r = voxel r % 5 also sits in every wave position of a workgroup."""
    c = orc.kinetic_case(T, M, 300, n_vox=5, z_free=True, missing=0.2)
    five = _fit(c)
    many = _fit(c, rows=np.arange(1031) % 5)
    for v in range(5):
        assert _same(_fit(c, rows=[v]), five, slice(None), slice(v, v + 1)), v
    for r in range(1031):
        assert _same(many, five, slice(r, r + 1), slice(r % 5, r % 5 + 1)), r
    assert np.all(five["status"] == 0)


# ---- (e) degenerate rows ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_degenerate_rows_leave_their_neighbours_alone():
    T = 65
    c = orc.kinetic_case(T, 1, 400, n_vox=8, z_free=True, sigma_weights=True)
    clean = _fit(c)
    d = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in c.items()}
    d["S"][1] = 0.0  # no substrate: the k and rho columns vanish
    d["w"][2, 0, :] = 0.0
    d["w"][2, 0, [3, 40]] = 1.0  # two weighted points, three free parameters
    d["Y"][3, 0, 17] = np.nan  # a NaN sample of positive weight
    d["w"][5, 0, 20] = 0.0
    d["Y"][5, 0, 20] = np.nan  # a NaN sample of weight 0 is not read
    out = _fit(d)
    for v in (0, 4, 6, 7):  # rows 0 ... 3 share a workgroup, 4 ... 7 the next
        assert _same(out, clean, slice(v, v + 1), slice(v, v + 1)), v
    assert out["status"][1, 0] in (0, 1) and np.all(np.isfinite(out["params"][1, 0]))
    assert np.all(np.isnan(out["param_sd"][1, 0])) and not np.isfinite(out["auc_ratio"][1, 0])
    assert out["status"][2, 0] == 3 and out["iters"][2, 0] == 0 and np.isnan(out["rss"][2, 0])
    assert out["status"][3, 0] == 2 and np.isnan(out["rss"][3, 0])
    for v in (2, 3):
        assert not out["params"][v].any() and not out["param_sd"][v].any() and not out["fit"][v].any()
        assert out["auc_ratio"][v, 0] == 0.0
    assert out["status"][5, 0] == 0 and np.all(np.isfinite(out["fit"][5]))
    n, share = _check_invariants(out, d, 200)
    assert n == 6
    # all weights zero, and exactly as many weighted points as free parameters (no degrees of freedom: NaN deviations)
    d["w"][0, 0, :] = 0.0
    d["w"][4, 0, :] = 0.0
    d["w"][4, 0, [0, 10, 50]] = 1.0
    out = _fit(d)
    assert out["status"][0, 0] == 3 and out["status"][4, 0] in (0, 1) and np.all(np.isnan(out["param_sd"][4, 0]))
    # a parameter starting on a bound stays there (slope 0 of the transform); the others are fitted
    init = c["init"].copy()
    init[:, 0] = 0.0
    out = _fit(c, init=init)
    assert np.all(out["params"][:, 0, 0] == 0.0) and np.all(out["param_sd"][:, 0, 0] != 0.0)
    assert np.all(out["status"] <= 1) and np.all(out["params"][:, 0, 2] > 0.0)
    n, _ = _check_invariants(out, c, 200, over={"init": init})
    assert n == 8
    print(f"degenerate rows: invariants at {share:.3f} of their bounds")


@pytest.mark.gpu
def test_refusals_leave_the_outputs_untouched():
    import torch
    from xmris_amd import _lib

    lib = _lib.load()
    M, T, nb = 2, 5, 3
    f64 = dict(dtype=torch.float64, device="cuda")
    bufs = {"substrate": torch.ones((nb, T), **f64), "products": torch.ones((nb, M, T), **f64),
            "weights": torch.ones((nb, M, T), **f64), "params": torch.full((nb, M, 3), -3.5, **f64),
            "param_sd": torch.full((nb, M, 3), -3.5, **f64), "rss": torch.full((nb, M), -3.5, **f64),
            "status": torch.full((nb, M), -7, dtype=torch.int32, device="cuda"),
            "iters": torch.full((nb, M), -7, dtype=torch.int32, device="cuda"), "fit": torch.full((nb, M, T), -3.5, **f64),
            "auc_ratio": torch.full((nb, M), -3.5, **f64)}
    torch.cuda.synchronize()
    for label, change in orc.REFUSALS:
        a = orc.abi_ok(M, T)
        a.update({k: v.data_ptr() for k, v in bufs.items()})
        change(a)
        args, keep = orc.abi_arguments(a, torch.cuda.current_stream().cuda_stream)
        assert lib.xm_kinetics_fit(*args) == _lib.XM_ERR_INVALID_ARG, label
    torch.cuda.synchronize()
    for k in ("params", "param_sd", "rss", "fit", "auc_ratio"):
        assert torch.all(bufs[k] == -3.5), k
    assert torch.all(bufs["status"] == -7) and torch.all(bufs["iters"] == -7)
    # and the valid call on the same buffers runs
    a = orc.abi_ok(M, T)
    a.update({k: v.data_ptr() for k, v in bufs.items()})
    args, keep = orc.abi_arguments(a, torch.cuda.current_stream().cuda_stream)
    assert lib.xm_kinetics_fit(*args) == 0
    torch.cuda.synchronize()
    assert torch.all(bufs["status"] >= 0) and torch.all(bufs["status"] <= 3)


# ---- (f) the public call ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_public_call_end_to_end():
    import xmris_amd as xm
    from xmris_amd import device as dev
    from xmris_amd.fitting import LabeledDataset

    T = 30
    c = orc.kinetic_case(T, 2, 500, n_vox=15)
    amp = np.zeros((5, 3, T, 3))
    amp[..., 0] = c["S"].reshape(5, 3, T)
    amp[..., 1:] = np.moveaxis(c["Y"], 1, 2).reshape(5, 3, T, 2)
    crlb = np.full(amp.shape, 2.0)
    crlb[2, 1, 9, 1] = np.nan  # a failed repetition
    dims = ("x", "y", "repetition", "Metabolite")
    coords = {"repetition": c["t"], "Metabolite": np.array(["pyruvate", "lactate", "alanine"])}
    ds = LabeledDataset({"amplitude": xm.LabeledArray(amp, dims, coords), "crlb": xm.LabeledArray(crlb, dims, coords)})
    flips = {"pyruvate": np.rad2deg(c["ths"]), "lactate": np.rad2deg(c["thp"][0]), "alanine": np.rad2deg(c["thp"][1])}
    kin = xm.fit_kinetics(ds, "pyruvate", ["lactate", "alanine"], flip_angle=flips, r1=(1 / 60, 1 / 10))
    assert "k_kinetics_fit" in dev.last_kernel()
    assert kin["rate"].dims == ("x", "y", "Metabolite") and kin["rate"].shape == (5, 3, 2)
    assert kin["fit"].shape == amp.shape and np.all(kin["status"].values == 0)
    z = np.abs(kin["rate"].values - c["truth"][:, 0]) / kin["rate_sd"].values
    print(f"public call: worst |k - truth| / rate_sd {z.max():.2f}")
    assert z.max() < 6.0
    assert np.all(np.abs(kin["decay"].values - c["truth"][:, 1]) < 6.0 * kin["decay_sd"].values)
    # the same numbers as the raw call with the weights the layer derives
    w = 1.0 / (0.02 * np.abs(c["Y"]))
    w[2 * 3 + 1, 0, 9] = 0.0
    init, lo, hi, fixed = c["init"].copy(), c["lo"], c["hi"], c["fixed"]
    init[:, 0] = 0.1
    raw = _fit(dict(c, w=w), init=init)
    assert np.array_equal(kin["rate"].values.reshape(15, 2), raw["params"][..., 0])
    assert np.array_equal(kin["auc_ratio"].values.reshape(15, 2), raw["auc_ratio"])
