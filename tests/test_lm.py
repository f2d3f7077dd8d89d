"""tests/_lm_oracle.py pinned on the CPU: the restated Levenberg-Marquardt driver converges where the standard problems
are known to end, its two routes agree, and the case list of tests/test_gpu_lm.py reaches every branch of lm_fit_item
without a trial that is too close to call.  The kernel is not involved."""
import functools
import os
import re

import numpy as np
import pytest
from scipy.optimize import least_squares

import _lm_oracle as orc

EPS = orc.EPS
TIE = 1e-9  # accept / reject margins below this are too close to call (tests/test_basis.py)

# Largest disagreement of lm_fit's two routes over orc.cases() x caps (tests/tool_lm_tolerance.py ->
# profiles/lm/tolerance.txt, CPU only): per parameter in units of its path length, in rss, in a deviation.  The kernel is
# a third summation order and a Cholesky solve of the same equations: 16 x those.  (The deviations are recorded only: the
# GPU test holds them to 64 eps cond(J^T J) at the returned parameters, which the measured figure is far inside.)
PATH_MEASURED, RSS_MEASURED, SD_MEASURED = 3.21e-12, 1.27e-09, 9.75e-11
PATH_TOL, RSS_TOL = 16 * PATH_MEASURED, 16 * RSS_MEASURED


@functools.lru_cache(maxsize=None)
def case_list():
    return {c.name: c for c in orc.cases()}


@functools.lru_cache(maxsize=None)
def reference(name, max_iter, route="normal"):
    """lm_fit of a listed case, computed once and shared (read only)."""
    return orc.lm_fit(case_list()[name], max_iter, route)


@functools.lru_cache(maxsize=None)
def stop_trial(name):
    return reference(name, 100000)["iters"]


def _tight(c):
    return orc.Case(c.name, c.kind, c.start, c.lo, c.hi, c.fixed, c.tab, ftol=1e-15, xtol=1e-15, n_amp=c.NA)


# ---- the oracle's own parts ---------------------------------------------------------------------------------------------------
# (nan_jacobian and infinite_start are other cases' problems with a Jacobian or a start that is not finite)
@pytest.mark.parametrize("name", [n for n in case_list() if n not in ("nan_jacobian", "infinite_start")])
def test_jacobians_against_central_differences(name):
    c = case_list()[name]
    rng = np.random.default_rng(3)
    p = np.clip(c.start, c.lo, c.hi) + 0.1 * rng.standard_normal(c.Q)
    if c.kind == "wall":
        p[0] = min(p[0], c.tab[0] - 0.1)
    _, _, j = orc.evaluate(c.kind, p, c.tab)
    for q in range(c.Q):
        h = 1e-6 * max(1.0, abs(p[q]))
        e = np.zeros(c.Q)
        e[q] = h
        num = (orc.evaluate(c.kind, p + e, c.tab)[0] - orc.evaluate(c.kind, p - e, c.tab)[0]) / (2 * h)
        assert np.abs(num - j[:, q]).max() <= 1e-7 * max(1.0, np.abs(j[:, q]).max()), (name, q)


def test_transforms_invert_and_slopes_are_derivatives():
    for bt, lo, hi in ((orc.FREE, -np.inf, np.inf), (orc.LO, -2.0, np.inf), (orc.HI, -np.inf, 5.0), (orc.TWO, -1.0, 3.0)):
        assert orc.bound_type(lo, hi) == bt
        for v in (-0.5, 0.25, 2.5):
            u = orc.to_internal(bt, v, lo, hi)
            p, s = orc.from_internal(bt, u, lo, hi)
            assert abs(p - v) <= 16 * EPS * 8
            num = (orc.from_internal(bt, u + 1e-6, lo, hi)[0] - orc.from_internal(bt, u - 1e-6, lo, hi)[0]) / 2e-6
            assert abs(num - s) <= 1e-8 * max(1.0, abs(s))
    # on a bound: the value is the bound and the slope exactly 0
    assert orc.from_internal(orc.TWO, orc.to_internal(orc.TWO, 3.0, -1.0, 3.0), -1.0, 3.0) == (3.0, 0.0)
    assert orc.from_internal(orc.HI, orc.to_internal(orc.HI, 5.0, -np.inf, 5.0), -np.inf, 5.0) == (5.0, 0.0)
    assert orc.bound_type(0.0, 1.0, fixed=True) == orc.FIXED


def test_solvers_against_lapack():
    rng = np.random.default_rng(5)
    a, b = rng.standard_normal((30, 7)), rng.standard_normal(30)
    x = orc.lstsq_longdouble(a, b)
    assert np.abs(x - np.linalg.lstsq(a, b, rcond=None)[0]).max() <= 1e-13
    h = a.T @ a
    assert np.abs(orc.cholesky(h) - np.linalg.cholesky(h)).max() <= 1e-13 * np.abs(h).max()
    h[3, 3] = -1.0
    assert orc.cholesky(h) is None
    h[3, 3] = np.nan
    assert orc.cholesky(h) is None and orc.lstsq_longdouble(np.full((3, 2), np.nan), np.zeros(3)) is None


def test_caps_run_past_the_stopping_trial():
    assert orc.caps(1) == [1, 2] and orc.caps(8) == [1, 2, 3, 5, 8, 13] and orc.caps(9)[-1] == 13 and orc.caps(0) == [1]


# ---- converged answers --------------------------------------------------------------------------------------------------------
MINIMA = {  # More, Garbow, Hillstrom (1981): parameters (None: not unique to this accuracy) and the cost at the minimum
    "rosenbrock": ([1.0, 1.0], 0.0), "rosenbrock_lo_hi": ([1.0, 1.0], 0.0), "helical": ([1.0, 0.0, 0.0], 0.0),
    "box3d_two": ([1.0, 10.0, 1.0], 0.0), "freudenstein": ([11.41277899, -0.89680525], 48.98425368),
    "brown_dennis": (None, 85822.20163), "powell_lo": ([0.0, 0.0, 0.0, 0.0], 0.0),
}


@pytest.mark.parametrize("name", list(MINIMA))
@pytest.mark.parametrize("route", ["normal", "lstsq"])
def test_closed_form_problems_end_in_their_known_minima(name, route):
    """With tolerances that do not stop the fit early.  Freudenstein-Roth ends in its local minimum, after rejections."""
    p_min, f_min = MINIMA[name]
    r = orc.lm_fit(_tight(case_list()[name]), 2000, route)
    assert r["status"] in (0, 1)
    if f_min == 0.0:
        assert r["rss"] <= 1e-20, r["rss"]
    else:
        assert abs(r["rss"] - f_min) <= 1e-9 * f_min, r["rss"]
    if p_min is not None:
        # Powell's singular function has a singular Jacobian at its minimum: the parameters converge as rss^(1/4)
        assert np.abs(r["params"] - p_min).max() <= (1e-4 if name == "powell_lo" else 1e-7), r["params"]
    if name == "freudenstein":
        assert any(not t[0] for t in r["trials"])


@pytest.mark.parametrize("name", ["exp2_lo", "exp2_fixed", "brown_dennis", "freudenstein"])
def test_converged_fit_matches_scipy(name):
    c = _tight(case_list()[name])
    r = orc.lm_fit(c, 2000)
    u0 = c.start_vector()[c.free]

    def fun(u):
        m, x, _ = orc.evaluate(c.kind, c.physical(u)[0], c.tab)
        return x - m

    def jac(u):
        p, s = c.physical(u)
        return -orc.evaluate(c.kind, p, c.tab)[2][:, c.free] * s[c.free]

    sol = least_squares(fun, u0, jac=jac, method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=4000)
    p = c.physical(sol.x)[0]
    assert abs(r["rss"] - 2.0 * sol.cost) <= 1e-10 * r["rss"]
    assert np.abs(r["params"] - p).max() <= 1e-6 * np.abs(p).max()


@pytest.mark.parametrize("name", ["table5", "table6_on_bound", "table_zero_column"])
def test_table_matches_lstsq(name):
    """The parameters that can move end where numpy.linalg.lstsq puts them; one that starts on its bound (slope 0) or owns
    a zero column stays at its start."""
    c = _tight(case_list()[name])
    r = orc.lm_fit(c, 2000)
    rows = c.tab[1:].reshape(-1, c.Q + 1)
    a, y = rows[:, :c.Q], rows[:, c.Q]
    held = {"table5": [], "table6_on_bound": [1, 4], "table_zero_column": [2]}[name]
    move = np.setdiff1d(np.arange(c.Q), held)
    want = c.start.copy()
    want[move] = np.linalg.lstsq(a[:, move], y - a[:, held] @ c.start[held], rcond=None)[0]
    assert np.array_equal(r["params"][held], c.start[held])
    assert np.abs(r["params"] - want).max() <= 1e-9 * np.abs(want).max()
    assert r["branches"]["zero_column_scale"] > 0 or not held


# ---- the case list: branches, ties, conditioning ------------------------------------------------------------------------------
def test_case_list_reaches_every_branch():
    total = dict.fromkeys(orc.BRANCHES, 0)
    for name, c in case_list().items():
        r = reference(name, 100000)
        for k, v in r["branches"].items():
            total[k] += v
        e = c.expect
        if "status" in e:
            assert r["status"] == e["status"], name
        if "iters" in e:
            assert r["iters"] == e["iters"], name
        if e.get("asd_nan"):
            assert r["status"] != 2 and np.all(np.isnan(r["asd"][~c.fixed[:c.NA]])) and r["branches"]["crlb_failed"] == 1, name
        elif r["status"] != 2:
            assert np.all(np.isfinite(r["asd"])) and r["branches"]["crlb_failed"] == 0, name
        if e.get("all_no_solve"):
            assert r["trials"] and all(t[2] == "no_solve" for t in r["trials"]) and r["branches"]["lambda_overflow"] == 1, name
    assert all(v > 0 for v in total.values()), total
    # each branch-only case ends as described
    wall = reference("wall", 100000)
    assert wall["branches"]["nonfinite_cost_rejected"] > 0 and wall["branches"]["xconv_on_rejection"] == 1
    assert not wall["trials"][-1][0] and wall["status"] == 0 and any(t[0] for t in wall["trials"])
    nanj = reference("nan_jacobian", 100000)
    assert nanj["iters"] == 45 and np.array_equal(nanj["params"], case_list()["nan_jacobian"].start)
    inf = reference("infinite_start", 100000)
    assert inf["status"] == 2 and inf["iters"] == 0 and np.isnan(inf["rss"])
    assert not inf["params"].any() and not inf["asd"].any() and not inf["fit"].any()
    zero = reference("table_zero_column", 100000)
    assert zero["params"][2] == case_list()["table_zero_column"].start[2] and zero["path"][2] == 0.0
    # every bound type, a fixed parameter, and a start on a bound with slope exactly 0
    types = set(int(b) for c in case_list().values() for b in c.bt)
    assert types == {orc.FIXED, orc.FREE, orc.LO, orc.HI, orc.TWO}
    c = case_list()["table6_on_bound"]
    s = c.physical(c.start_vector()[c.free])[1]
    assert s[1] == 0.0 and s[4] == 0.0 and np.all(s[[0, 2, 3, 5]] == 1.0)
    assert all(f != 1.0 for c in case_list().values() for f in c.factor)


@pytest.mark.parametrize("name", list(case_list()))
def test_no_trial_is_too_close_to_call_and_the_routes_agree(name):
    """At every cap of the GPU test: no margin below TIE (a trial that cannot be solved, whose cost is not finite or whose
    step is exactly zero has no margin), the same decisions, iterations and status by both routes."""
    stop = stop_trial(name)
    for m in orc.caps(stop):
        a, b = reference(name, m), reference(name, m, "lstsq")
        assert (a["iters"], a["status"]) == (b["iters"], b["status"]) and a["iters"] == min(m, stop)
        assert a["status"] == (reference(name, 100000)["status"] if m >= stop else 1)
        assert [t[0] for t in a["trials"]] == [t[0] for t in b["trials"]]
        for r in (a, b):
            assert not any(abs(t[1]) < TIE for t in r["trials"]), (name, m, [t for t in r["trials"] if abs(t[1]) < TIE])
    assert stop <= 60  # a few seconds on the GPU, caps included


def _cond_bound(c):
    p = c.physical(c.start_vector()[c.free])[0]
    return 64 * EPS * orc.crlb(c, p)[1]


def test_table_cases_are_conditioned_for_the_deviation_check():
    """64 eps cond(J^T J) < 1 for every `table` problem whose deviations are compared (the Jacobian of a linear problem
    does not depend on p).  The staging shapes with fewer residuals than columns, 2 n_points < P, are rank deficient by
    shape: their deviations are not compared, and they are exactly those below."""
    for name in ("table5", "table6_on_bound"):
        assert _cond_bound(case_list()[name]) < 1e-6
    deficient = []
    for P in orc.STAGING_P:
        assert len(set(orc.staging_points(P))) >= 4
        for n in orc.staging_points(P):
            c = orc.staging_case(P, n)
            assert (c.P, c.n_points, c.NA) == (P, n, P)
            if 2 * n < P:
                deficient.append((P, n))
            else:
                assert _cond_bound(c) < 1e-3, (P, n)
    assert deficient == [(64, 31), (65, 31), (65, 32), (80, 31), (80, 32), (80, 33)]
    assert [orc.q_pts(P) for P in orc.STAGING_P] == [128, 64, 32, 32, 32]
    assert [2 * orc.q_pts(P) * (P + 1) // P for P in (63, 64, 65, 80)] == [130, 65, 64, 64]  # amplitudes per CRLB round
    rounds = orc.crlb_round_cases()
    assert [(c.P, c.NA, int(c.fixed.sum())) for c in rounds] == [(80, 64, 0), (80, 65, 0), (80, 80, 0), (80, 120, 40)]
    for c in rounds:
        assert _cond_bound(c) < 1e-6
    last = rounds[-1]
    assert last.fixed[:64].any() and last.fixed[64:].any()  # fixed amplitudes in both rounds


def test_bounds_are_sixteen_times_the_measured_figures():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "lm", "tolerance.txt")
    with open(path) as f:
        text = f.read()
    last = text.strip().splitlines()[-1]
    dp, du, rss, sd = (float(v) for v in re.findall(r"(\d\.\d\de[-+]\d\d)", last))
    assert max(dp, du) == PATH_MEASURED and rss == RSS_MEASURED and sd == SD_MEASURED
    assert "84 of 84" in text  # every cap: both routes take the same decisions
