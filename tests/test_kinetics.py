"""CPU tests of fit_kinetics / simulate_kinetics: pins of the oracle (tests/_kinetics_oracle.py:
closed forms as x -> 0, a two-repetition case by hand, the Jacobian against central differences, the scan order, recovery
of k), the selection of the GPU tests' cases (no trial too close to call, scipy converges, the restated iteration agrees
with scipy), the Python layer on an oracle-backed stand-in for the launch (Dataset and array input, crlb -> weights, a
failed repetition -> weight 0, every ValueError before the device is reached), xm_kinetics_fit's refusals through the
built library without a GPU, and the signatures.

The tests of the oracle alone import nothing from the package and pass without the feature; all others fail without it."""
import functools
import os
import re

import numpy as np
import pytest

import _kinetics_oracle as orc

PROFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "kinetics", "tolerance.txt")
# tests/tool_kinetics_tolerance.py, recorded in profiles/kinetics/tolerance.txt
SCAN_GAP = 8.179e-16
STEP_GAP = 2.660e-11
STEP_RSS_GAP = 2.672e-12

STEP_M = (1, 2, 3)
# A trial whose relative gain (F - Ft) / F is nearer to 0 than this could be judged either way by another rounding: two
# summation orders disagree in rss by 16 x STEP_RSS_GAP = 4.3e-11 at the most, so 1e-9 leaves a factor of 20.
TIE = 1e-9

# converged parity with scipy: rho free and fixed, z free and fixed, stretched times, per-repetition flip angles, a fifth
# of the points missing, weights 1 / sigma; T = 2 and 3 carry k alone
PARITY = {
    "T2_k": dict(T=2, M=1, seed=11, rho_free=False, n_vox=5),
    "T3_k_M4": dict(T=3, M=4, seed=12, rho_free=False, n_vox=5),
    "T63_k_rho": dict(T=63, M=4, seed=13, n_vox=5),
    "T64_all": dict(T=64, M=1, seed=14, z_free=True, n_vox=5, uniform=False),
    "T65_k_z_flips": dict(T=65, M=4, seed=15, rho_free=False, z_free=True, flip_per_rep=True, n_vox=5),
    "T129_all_missing": dict(T=129, M=1, seed=16, z_free=True, missing=0.2, n_vox=5, uniform=False, flip_per_rep=True),
    "T256_k_rho_sigma": dict(T=256, M=4, seed=17, sigma_weights=True, missing=0.2, n_vox=5),
    "T30_k_rho": dict(T=30, M=3, seed=18, n_vox=5),
}


@functools.lru_cache(maxsize=None)
def _step_case(name):
    return orc.kinetic_case(**dict(orc.step_cases())[name])


@functools.lru_cache(maxsize=None)
def _step_ref(name, v, m, steps):
    return orc.lm_steps_kinetics(orc.item(_step_case(name), v, m), max_iter=steps)


@functools.lru_cache(maxsize=None)
def _parity_case(name):
    return orc.kinetic_case(**PARITY[name])


@functools.lru_cache(maxsize=None)
def _parity_ref(name):
    """[(voxel, product, scipy's result)] of a parity case."""
    c = _parity_case(name)
    return [(v, m, orc.fit_scipy(orc.item(c, v, m))) for v in range(c["S"].shape[0]) for m in range(c["M"])]


# ---- the oracle -----------------------------------------------------------------------------------------------------------
def test_recorded_figures_match_their_tool():
    text = open(PROFILE).read()
    assert float(re.search(r"disagreement of the scan order: ([0-9.e+-]+)", text).group(1)) == SCAN_GAP
    assert float(re.search(r"largest \|dp\| / path: ([0-9.e+-]+)", text).group(1)) == STEP_GAP
    assert float(re.search(r"relative rss disagreement: ([0-9.e+-]+)", text).group(1)) == STEP_RSS_GAP


def test_weights_reach_their_limits_without_cancellation():
    """x -> 0: w0, w1 -> D / 2, dw0 -> -D^2 / 3, dw1 -> -D^2 / 6; both branches agree where they meet."""
    D = np.array([2.0])
    for rho in (1e-300, 1e-12, 1e-6):
        E, w0, w1, dE, dw0, dw1 = orc.weights(rho, D)
        x = rho * 2.0
        assert abs(w0[0] - (1.0 - 2.0 * x / 3.0)) <= 4 * orc.EPS + x * x and abs(w1[0] - (1.0 - x / 3.0)) <= 4 * orc.EPS + x * x
        assert abs(dw0[0] + 4.0 / 3.0) <= 4 * x + 4 * orc.EPS and abs(dw1[0] + 4.0 / 6.0) <= 4 * x + 4 * orc.EPS
        assert dE[0] == -2.0 * E[0]
    x = orc.SERIES_X
    for a, b in zip(orc.weights_series(x, np.array([1.0])), orc.weights_closed(x, np.array([1.0]))):
        assert abs(a[0] - b[0]) <= 8 * orc.EPS * abs(b[0])
    # w0 + w1 is the integral of e^{-rho (D - s)} over the interval
    for rho in (0.01, 0.2, 0.3, 2.0):
        _, w0, w1, *_ = orc.weights(rho, D)
        assert abs(w0[0] + w1[0] + np.expm1(-rho * 2.0) / rho) <= 8 * orc.EPS


def test_two_repetitions_by_hand():
    t, ths, thp = np.array([0.0, 3.0]), np.array([0.2, 0.3]), np.array([0.4, 0.5])
    S = np.array([7.0, 5.0])
    k, rho, z = 0.05, 0.1, 2.0
    x = rho * 3.0
    e = np.exp(-x)
    w1 = 3.0 * (x - 1 + e) / x ** 2
    w0 = 3.0 * (1 - e) / x - w1
    z1 = e * np.cos(0.4) * z + k * (w0 * 7.0 / np.sin(0.2) * np.cos(0.2) + w1 * 5.0 / np.sin(0.3))
    got = orc.model((k, rho, z), S, t, ths, thp)
    assert np.allclose(got, [z * np.sin(0.4), z1 * np.sin(0.5)], rtol=1e-14, atol=0)


@pytest.mark.parametrize("name", [n for n, _ in orc.step_cases()])
def test_jacobian_and_scan_order(name):
    c = _step_case(name)
    it = orc.item(c, 0, c["M"] - 1)
    p = np.array([0.03, 0.05, 3.0])
    args = (it["S"], it["t"], it["ths"], it["thp"])
    J, Jc = orc.model_jacobian(p, *args), orc.jacobian_central(p, *args)
    assert np.abs(J - Jc).max() <= 1e-8 * np.abs(J).max()
    (z1, d1), (z2, d2) = orc.forward(p, *args), orc.forward_scan(p, *args)
    assert np.abs(z1 - z2).max() <= 2 * SCAN_GAP * np.abs(z1).max()
    assert np.abs(d1 - d2).max() <= 2 * SCAN_GAP * np.abs(d1).max()


def test_no_step_is_too_close_to_call():
    for name, _ in orc.step_cases():
        c = _step_case(name)
        for v in range(c["S"].shape[0]):
            for m in range(c["M"]):
                ref = _step_ref(name, v, m, max(STEP_M))
                assert ref["status"] == 1 and ref["iters"] == max(STEP_M), (name, v, m)
                assert not any(abs(margin) < TIE for _, margin in ref["trials"]), (name, v, m, ref["trials"])


@pytest.mark.parametrize("name", list(PARITY))
def test_restated_iteration_matches_scipy(name):
    """What the GPU test asks of the kernel holds for the restated iteration, and scipy converges on every item (the
    GPU test may skip 2 % of them; this selection needs none)."""
    c = _parity_case(name)
    worst = 0.0
    for v, m, o in _parity_ref(name):
        assert o["success"], (name, v, m)
        r = orc.lm_steps_kinetics(orc.item(c, v, m))
        assert r["status"] == 0 and r["iters"] < 200
        free = o["sd"] > 0
        assert free.any()
        worst = max(worst, float(np.max(np.abs(r["params"] - o["params"])[free] / o["sd"][free])))
        assert abs(r["rss"] - o["rss"]) <= 1e-9 * o["rss"]
    print(f"{name}: worst |dp| / sd {worst:.3e} (bound 1e-3)")
    assert worst <= 1e-3


def test_rate_is_recovered_from_simulated_data():
    from xmris_amd import simulate_kinetics

    t = 2.0 * np.arange(30)
    mag = 100.0 * ((t + 2) / 8) ** 2 * np.exp(2 * (1 - (t + 2) / 8))
    S = mag * np.sin(np.deg2rad(10.0))
    Y = simulate_kinetics(S, t, 0.03, 0.04, flip_angle=(10.0, 25.0))
    ths, thp = np.full(30, np.deg2rad(10.0)), np.full(30, np.deg2rad(25.0))
    assert np.allclose(Y, orc.model((0.03, 0.04, 0.0), S, t, ths, thp), rtol=1e-13, atol=0)
    init, lo, hi, fixed = orc.parameters(1)
    it = {"S": S, "Y": Y, "w": np.ones(30), "t": t, "ths": ths, "thp": thp, "init": init[0], "lo": lo[0], "hi": hi[0],
          "fixed": fixed[0]}
    r = orc.lm_steps_kinetics(it)
    assert r["status"] == 0 and abs(r["params"][0] - 0.03) <= 1e-8 and abs(r["params"][1] - 0.04) <= 1e-7
    # leading axes broadcast; per-repetition flip angles
    both = simulate_kinetics(np.stack([S, 2 * S]), t, [0.03, 0.01], 0.04, initial=[0.0, 4.0],
                             flip_angle=(10.0, np.linspace(20, 30, 30)))
    assert both.shape == (2, 30) and both[1, 0] == 4.0 * np.sin(np.deg2rad(20.0))
    for bad in (dict(times=t[::-1]), dict(flip_angle=(10.0, 90.0)), dict(flip_angle=10.0), dict(decay=-0.1),
                dict(times=t[:5])):
        kw = dict(substrate=S, times=t, rate=0.03, decay=0.04, flip_angle=(10.0, 25.0))
        kw.update(bad)
        with pytest.raises(ValueError):
            simulate_kinetics(**kw)


# ---- the Python layer on a stand-in for the launch -----------------------------------------------------------------------
def _stand_in(calls):
    def run(sub, prod, weights, times, ths, thp, init, lo, hi, fixed, max_iter):
        calls.append(dict(sub=sub, prod=prod, weights=weights, times=times, ths=ths, thp=thp, init=init, lo=lo, hi=hi,
                          fixed=fixed, max_iter=max_iter))
        nb, M, T = prod.shape
        out = {"params": np.zeros((nb, M, 3)), "param_sd": np.zeros((nb, M, 3)), "rss": np.zeros((nb, M)),
               "status": np.zeros((nb, M), np.int32), "iters": np.zeros((nb, M), np.int32), "fit": np.zeros((nb, M, T)),
               "auc_ratio": np.zeros((nb, M))}
        for v in range(nb):
            for m in range(M):
                it = {"S": sub[v], "Y": prod[v, m], "w": np.ones(T) if weights is None else weights[v, m], "t": times,
                      "ths": ths, "thp": thp[m], "init": init[m], "lo": lo[m], "hi": hi[m], "fixed": fixed[m]}
                r = orc.lm_steps_kinetics(it, max_iter=max_iter)
                out["params"][v, m], out["rss"][v, m] = r["params"], r["rss"]
                out["status"][v, m], out["iters"][v, m] = r["status"], r["iters"]
                if r["status"] < 2:
                    out["param_sd"][v, m] = orc.covariance_sd(r["params"], it)[0]
                    out["fit"][v, m] = orc.model(r["params"], sub[v], times, ths, thp[m])
                    out["auc_ratio"][v, m] = orc.auc_ratio(sub[v], prod[v, m], it["w"], times)
        return out
    return run


def _dataset(T=30, crlb=True, seed=3):
    """A fit Dataset [x 2, repetition T, Metabolite (lactate, pyruvate, alanine, urea)] from the oracle's case."""
    import xmris_amd as xm
    from xmris_amd.fitting import LabeledDataset

    c = orc.kinetic_case(T, 2, seed)
    amp = np.zeros((2, T, 4))
    amp[:, :, 1] = c["S"]
    amp[:, :, 0], amp[:, :, 2] = c["Y"][:, 0], c["Y"][:, 1]
    amp[:, :, 3] = 50.0
    coords = {"repetition": c["t"], "Metabolite": np.array(["lactate", "pyruvate", "alanine", "urea"])}
    dv = {"amplitude": xm.LabeledArray(amp, ("x", "repetition", "Metabolite"), coords)}
    if crlb:
        dv["crlb"] = xm.LabeledArray(np.full(amp.shape, 2.0), ("x", "repetition", "Metabolite"), coords)
    return LabeledDataset(dv, {"note": "kept"}), c


FLIPS = {"pyruvate": 10.0, "lactate": 25.0, "alanine": 15.0}


def test_dataset_input_weights_and_outputs(monkeypatch):
    import xmris_amd as xm
    from xmris_amd import ATTRS
    from xmris_amd.fitting import kinetics

    calls = []
    monkeypatch.setattr(kinetics, "_run_fit", _stand_in(calls))
    ds, c = _dataset()
    amp, crlb = ds["amplitude"].values, ds["crlb"].values
    crlb[0, 4, 0] = np.nan  # a failed repetition of lactate in voxel 0 ...
    amp[1, 7, 2], crlb[1, 7, 2] = 0.0, 0.0  # ... and of alanine in voxel 1
    out = xm.fit_kinetics(ds, "pyruvate", ["lactate", "alanine"], flip_angle=FLIPS, r1=(1 / 60, 1 / 10))
    (call,) = calls
    assert call["sub"].shape == (2, 30) and call["prod"].shape == (2, 2, 30) and call["max_iter"] == 200
    assert np.array_equal(call["sub"], amp[:, :, 1]) and np.array_equal(call["prod"][:, 1], amp[:, :, 2])
    w = call["weights"]
    assert w[0, 0, 4] == 0.0 and w[1, 1, 7] == 0.0 and np.count_nonzero(w == 0) == 2
    assert w[0, 0, 5] == 1.0 / (0.02 * abs(amp[0, 5, 0]))
    assert np.array_equal(call["times"], c["t"])
    assert np.allclose(call["ths"], np.deg2rad(10.0)) and np.allclose(call["thp"][1], np.deg2rad(15.0))
    assert np.array_equal(call["fixed"], [[False, False, True]] * 2) and np.array_equal(call["lo"][:, 1], [1 / 60] * 2)
    assert np.all(call["init"][:, 0] == 0.1) and np.all(call["hi"][:, 0] == 1.0) and np.all(np.isinf(call["hi"][:, 2]))
    assert set(out.data_vars) == set(kinetics.PRODUCT_VARS) | {"fit"}
    assert out["rate"].dims == ("x", "Metabolite") and list(out["rate"].coords["Metabolite"].values) == ["lactate", "alanine"]
    assert out["fit"].dims == ("x", "repetition", "Metabolite") and out["fit"].shape == amp.shape
    assert np.all(np.isnan(out["fit"].values[:, :, [1, 3]])) and np.all(np.isfinite(out["fit"].values[:, :, [0, 2]]))
    assert np.all(out["status"].values == 0)
    assert np.all(np.abs(out["rate"].values - c["truth"][:, 0]) <= 5 * out["rate_sd"].values)
    assert out.attrs["note"] == "kept" and out.attrs[ATTRS.kinetics_substrate] == "pyruvate"
    assert out.attrs[ATTRS.kinetics_dim] == "repetition" and out.attrs[ATTRS.kinetics_fit_initial] is False
    assert out.attrs[ATTRS.kinetics_rate_bounds] == (0.0, 1.0)
    assert out.attrs[ATTRS.kinetics_decay_bounds] == {"lactate": (1 / 60, 1 / 10), "alanine": (1 / 60, 1 / 10)}
    assert out.attrs[ATTRS.kinetics_flip_angle]["alanine"] == pytest.approx([15.0] * 30)


def test_array_input_sigma_r1_forms_and_accessor(monkeypatch):
    import xmris_amd as xm
    from xmris_amd.fitting import kinetics

    calls = []
    monkeypatch.setattr(kinetics, "_run_fit", _stand_in(calls))
    ds, c = _dataset(crlb=False)
    amp = ds["amplitude"]
    xm.fit_kinetics(amp, "pyruvate", "lactate", flip_angle=12.0, r1=0.04, fit_initial=True, max_iter=7)
    assert calls[-1]["weights"] is None and calls[-1]["prod"].shape == (2, 1, 30) and calls[-1]["max_iter"] == 7
    assert np.array_equal(calls[-1]["fixed"], [[False, True, False]]) and calls[-1]["init"][0, 1] == 0.04
    assert np.isnan(calls[-1]["init"][0, 2]) and np.allclose(calls[-1]["thp"], np.deg2rad(12.0))
    # the Dataset without crlb: unit weights too; sigma given: 1 / sigma, 0 where sigma is 0
    xm.fit_kinetics(ds, "pyruvate", ["alanine"], flip_angle=FLIPS, r1={"alanine": (0.01, 0.2)})
    assert calls[-1]["weights"] is None and tuple(calls[-1]["lo"][0, 1:2]) == (0.01,) and calls[-1]["hi"][0, 1] == 0.2
    sg = np.full(amp.shape, 0.5)
    sg[0, 3, 0] = 0.0
    xm.fit_kinetics(amp, "pyruvate", ["lactate"], flip_angle=FLIPS, sigma=sg)
    assert calls[-1]["weights"][0, 0, 3] == 0.0 and calls[-1]["weights"][1, 0, 3] == 2.0
    # explicit times, per-repetition flip angles, the accessor, another order of the dims
    moved = xm.LabeledArray(np.moveaxis(amp.values, 2, 0), ("Metabolite", "x", "repetition"),
                            {"Metabolite": amp.coords["Metabolite"].values})
    ramp = np.linspace(20, 30, 30)
    out = moved.xmr.fit_kinetics("pyruvate", ["lactate", "alanine"], times=c["t"] + 5.0,
                                 flip_angle={"pyruvate": 10.0, "lactate": ramp, "alanine": 15.0})
    assert np.array_equal(calls[-1]["times"], c["t"] + 5.0) and np.allclose(calls[-1]["thp"][0], np.deg2rad(ramp))
    assert out["rate"].dims == ("x", "Metabolite") and out["fit"].dims == ("Metabolite", "x", "repetition")
    assert np.array_equal(calls[-1]["prod"][:, 0], amp.values[:, :, 0])


def test_every_validation_error_comes_before_the_device(monkeypatch):
    import xmris_amd as xm
    from xmris_amd.fitting import kinetics

    def never(*a, **k):
        raise AssertionError("the launch was reached")

    monkeypatch.setattr(kinetics, "_run_fit", never)
    ds, c = _dataset()
    amp = ds["amplitude"]
    ok = dict(substrate="pyruvate", products=["lactate", "alanine"], flip_angle=FLIPS)
    nocoord = xm.LabeledArray(amp.values, amp.dims, {"Metabolite": amp.coords["Metabolite"].values})
    nonames = xm.LabeledArray(amp.values, amp.dims, {"repetition": c["t"]})
    long = xm.LabeledArray(np.ones((257, 2)), ("repetition", "Metabolite"), {"Metabolite": np.array(["a", "b"])})
    bad = [
        (ds, dict(dim="time")), (ds, dict(metabolite_dim="metabolite")), (ds, dict(dim="Metabolite")),
        (nonames, {}), (ds, dict(substrate="pyr")), (ds, dict(products=["lactate", "citrate"])),
        (ds, dict(products=["lactate", "pyruvate"])), (ds, dict(products=["lactate", "lactate"])), (ds, dict(products=[])),
        (nocoord, {}), (ds, dict(times=c["t"][:-1])), (ds, dict(times=c["t"][::-1])), (ds, dict(times=np.full(30, np.nan))),
        (ds, dict(flip_angle=None)), (ds, dict(flip_angle={"pyruvate": 10.0, "lactate": 25.0})),
        (ds, dict(flip_angle=0.0)), (ds, dict(flip_angle=90.0)), (ds, dict(flip_angle={**FLIPS, "lactate": np.ones(29)})),
        (ds, dict(r1=-0.1)), (ds, dict(r1=(0.1, 0.05))), (ds, dict(r1=(0.0, np.inf))), (ds, dict(r1=(0.1, 0.2, 0.3))),
        (ds, dict(r1={"lactate": 0.04})), (ds, dict(rate_bounds=(0.0, np.inf))), (ds, dict(rate_bounds=(1.0, 0.0))),
        (ds, dict(max_iter=0)), (amp, dict(sigma=np.ones(7))), (amp, dict(sigma=-1.0)),
        (long, dict(substrate="a", products=["b"], flip_angle=10.0, times=np.arange(257.0))),
        (xm.fitting.LabeledDataset({"crlb": ds["crlb"]}), {}),
    ]
    for data, change in bad:
        with pytest.raises(ValueError):
            xm.fit_kinetics(data, **{**ok, **change})
    with pytest.raises(TypeError):
        xm.fit_kinetics(amp.values, **ok)


# ---- the C ABI without a GPU ---------------------------------------------------------------------------------------------
def test_abi_refusals_come_before_any_hip_call():
    from xmris_amd import _lib

    lib = _lib.load()
    args, keep = orc.abi_arguments(orc.abi_ok())
    for label, change in orc.REFUSALS:
        a = orc.abi_ok()
        change(a)
        args, keep = orc.abi_arguments(a)
        rc = lib.xm_kinetics_fit(*args)
        assert rc == _lib.XM_ERR_INVALID_ARG, label
        assert b"kinetics" in lib.xm_last_error_string(), label
    # no voxels: nothing is launched, whatever the pointers hold; weights and fit may be null
    a = orc.abi_ok()
    a.update(n_batch=0, substrate=0, products=0, params=0)
    assert lib.xm_kinetics_fit(*orc.abi_arguments(a)[0]) == 0
    assert len(orc.REFUSALS) >= 35


def test_signature_vocabulary_and_exports():
    import ctypes

    import xmris_amd
    from xmris_amd import ATTRS, _lib

    res, args = _lib.SIGNATURES["xm_kinetics_fit"]
    assert res is ctypes.c_int and len(args) == len(orc.ABI_ORDER) + 1
    assert [a is ctypes.c_double for a in args].count(True) == 2 and args[3] is ctypes.c_int64
    for name in ("fit_kinetics", "simulate_kinetics"):
        assert name in xmris_amd.__all__ and name in xmris_amd.fitting.__all__
        assert getattr(xmris_amd, name) is getattr(xmris_amd.fitting, name)
    assert hasattr(xmris_amd.XmrisAccessor, "fit_kinetics") and hasattr(xmris_amd.device, "kinetics_fit")
    assert (ATTRS.kinetics_model, ATTRS.kinetics_substrate, ATTRS.kinetics_flip_angle) == \
        ("kinetics_model", "kinetics_substrate", "kinetics_flip_angle")
