"""lm_fit_item (xmris_amd/csrc/xm_lm.h), the Levenberg-Marquardt driver of k_amares_fit and k_basis_fit, on the GPU by
itself: xm_wgp_lm_fit of the probe library (csrc/xm_wg_probe.hip) runs it on standard least-squares problems inside the
persistent loop of the product kernels, and every trial is held to the generic restatement tests/_lm_oracle.py.
tests/test_lm.py pins the oracle, the case list (every branch reached, no trial too close to call) and the bounds on the
CPU; the bounds come from the reference side alone (tests/tool_lm_tolerance.py, profiles/lm/tolerance.txt)."""
import numpy as np
import pytest

import _lm_oracle as orc
from test_gpu_wg import INVALID, _probe, _up
from test_lm import PATH_TOL, RSS_TOL, TIE, case_list, reference, stop_trial
from test_wg import TRANSFORM_TOL

pytestmark = pytest.mark.gpu

EPS = orc.EPS
FILL = -7.0  # what every output holds before a launch


def _run(cases, max_iter, grid=None, want_fit=True):
    """One launch over `cases` (rows of one problem: the same kind, bounds, sizes and tolerances).  Returns numpy arrays:
    params [nb, Q], asd [nb, NA], rss, status, iters [nb], fit [nb, 2 n], u [nb, P]."""
    import torch

    c0, nb = cases[0], len(cases)
    for c in cases:
        assert (c.kind, c.Q, c.P, c.NA, c.n_points, c.ftol, c.xtol, c.tab.size) == \
            (c0.kind, c0.Q, c0.P, c0.NA, c0.n_points, c0.ftol, c0.xtol, c0.tab.size)
        assert np.array_equal(c.bt, c0.bt) and np.array_equal(c.lo, c0.lo) and np.array_equal(c.hi, c0.hi)
        assert np.array_equal(c.factor, c0.factor)
    f64 = dict(dtype=torch.float64, device="cuda")
    i32 = dict(dtype=torch.int32, device="cuda")
    o = {"params": torch.full((nb, c0.Q), FILL, **f64), "asd": torch.full((nb, c0.NA), FILL, **f64),
         "rss": torch.full((nb,), FILL, **f64), "status": torch.full((nb,), -7, **i32), "iters": torch.full((nb,), -7, **i32),
         "fit": torch.full((nb, 2 * c0.n_points), FILL, **f64) if want_fit else None, "u": torch.full((nb, c0.P), FILL, **f64)}
    start, tab, factor = _up(np.stack([c.start_vector() for c in cases])), _up(np.stack([c.tab for c in cases])), _up(c0.factor)
    counter = torch.zeros(2, **i32)
    bt, lo, hi = np.ascontiguousarray(c0.bt, dtype=np.int32), np.ascontiguousarray(c0.lo), np.ascontiguousarray(c0.hi)
    rc = _probe().xm_wgp_lm_fit(orc.KINDS.index(c0.kind), start.data_ptr(), tab.data_ptr(), c0.tab.size, factor.data_ptr(),
                                bt.ctypes.data, lo.ctypes.data, hi.ctypes.data, nb, c0.n_points, c0.Q, c0.NA, c0.P, max_iter,
                                c0.ftol, c0.xtol, o["params"].data_ptr(), o["asd"].data_ptr(), o["rss"].data_ptr(),
                                o["status"].data_ptr(), o["iters"].data_ptr(), o["fit"].data_ptr() if want_fit else None,
                                o["u"].data_ptr(), counter.data_ptr(), grid or min(nb, 1024), None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert not counter.cpu().numpy().any()  # the last workgroup out leaves the counters at zero
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in o.items()}


def _row(out, v):
    return {k: (a[v] if a is not None else None) for k, a in out.items()}


def _transform_slack(c):
    """Rounding of a physical value formed from its internal one (tests/test_wg.py: TRANSFORM_TOL roundings of the
    largest quantity that enters: the value, a finite bound, the 1 of the one-sided transforms)."""
    scale = np.maximum(1.0, np.abs(c.start))
    for b in (c.lo, c.hi):
        scale = np.maximum(scale, np.where(np.isfinite(b), np.abs(b), 0.0))
    return TRANSFORM_TOL * EPS * scale


def _model_tolerance(c, p):
    """Per residual: what two fp64 evaluations of the model at the same p may differ by.  1e-12 (the bound of `fit` in
    tests/test_gpu_basis.py) of the magnitude of what is added up: |x^| + |d x^ / d p| |p| + |x|."""
    m, x, j = orc.evaluate(c.kind, p, c.tab)
    with np.errstate(all="ignore"):
        return 1e-12 * (np.abs(m) + np.nan_to_num(np.abs(j), nan=0.0) @ np.abs(p) + np.abs(x)), m, x, j


def _check_status_2(r, c):
    assert not r["params"].any() and not r["asd"].any() and np.isnan(r["rss"]), "a status-2 row is all zeros, NaN rss"
    assert r["fit"] is None or not r["fit"].any()


def _check_outputs(r, c, deviations=True):
    """Every output of a row with status 0 / 1 recomputed from its returned u and parameters."""
    assert r["status"] in (0, 1)
    p, u = r["params"], r["u"]
    assert np.all(np.isfinite(p)) and np.all(np.isfinite(u))
    want_p = c.physical(u)[0]
    assert np.array_equal(p[c.fixed], c.start[c.fixed]), "a fixed parameter moved"
    assert np.all(np.abs(p - want_p) <= _transform_slack(c) + TRANSFORM_TOL * EPS * np.abs(want_p)), "params are not u's"
    assert np.all((p >= c.lo) & (p <= c.hi))
    tol, m, x, _ = _model_tolerance(c, p)
    if r["fit"] is not None:
        assert np.all(np.abs(r["fit"] - m) <= tol), ("fit", np.abs(r["fit"] - m).max())
    res = x - m
    rss = float(np.sum(res * res))
    rss_tol = float(np.sum(2.0 * np.abs(res) * tol + tol * tol)) + 256 * EPS * rss
    assert abs(r["rss"] - rss) <= rss_tol, ("rss", r["rss"], rss, rss_tol)
    sd, cond, failed = orc.crlb(c, p)
    fixed_amp = c.fixed[:c.NA]
    assert np.all(r["asd"][fixed_amp] == 0.0), "a fixed amplitude reports a deviation"
    if not deviations:  # fewer residuals than columns: J^T J is singular, whatever the factorisation makes of it
        assert np.all(np.isnan(r["asd"][~fixed_amp]) | (r["asd"][~fixed_amp] >= 0.0))
        return 0.0
    if failed:  # NaN exactly where the CRLB factorisation fails
        assert np.all(np.isnan(r["asd"][~fixed_amp])), r["asd"]
        return 0.0
    bound = 64 * EPS * cond
    assert bound < 1.0, (c.name, bound)  # test_lm.py: the listed cases are conditioned; none is skipped
    err = np.abs(r["asd"] - sd)[~fixed_amp] / sd[~fixed_amp]
    assert np.all(err <= bound), ("asd", err.max(), bound)
    return float(err.max() / bound)


# ---- 1. the trajectory, trial by trial until the fit stops -----------------------------------------------------------------
@pytest.mark.parametrize("name", list(case_list()))
def test_trajectory_matches_the_restated_driver(name):
    """max_iter = 1, 2, 3, 5, 8, 13, ... up to and past the stopping trial: iterations and status equal the reference's;
    u and the parameters agree per parameter in units of its path length (a parameter that never moved: u bit for bit),
    rss within RSS_TOL and what the allowed parameter disagreement d makes of it, 2 sqrt(rss) e + e^2 with
    e = || |J| d ||.  tests/test_lm.py: no trial of these cases is too close to call, at every cap both routes of the
    reference take the same decisions."""
    c = case_list()[name]
    for m in orc.caps(stop_trial(name)):
        ref = reference(name, m)
        assert not any(abs(t[1]) < TIE for t in ref["trials"])
        r = _row(_run([c], m), 0)
        assert (r["iters"], r["status"]) == (ref["iters"], ref["status"]), (name, m, r["iters"], r["status"], ref["iters"])
        if ref["status"] == 2:
            _check_status_2(r, c)
            print(f"{name} m={m}: status 2, iters {r['iters']}")
            continue
        du, dp = np.abs(r["u"] - ref["u"]), np.abs(r["params"] - ref["params"])
        still = ref["path_u"] == 0
        assert np.array_equal(r["u"][still], ref["u"][still]), (name, m, "a variable that never moved")
        u_allow = PATH_TOL * ref["path_u"]
        p_allow = PATH_TOL * ref["path"] + _transform_slack(c)
        j = np.nan_to_num(np.abs(orc.evaluate(c.kind, ref["params"], c.tab)[2]), nan=0.0)
        e = float(np.linalg.norm(j @ p_allow))
        f_allow = RSS_TOL * ref["rss"] + 2.0 * np.sqrt(ref["rss"]) * e + e * e
        df = abs(r["rss"] - ref["rss"])
        shares = (float(np.max(du[~still] / u_allow[~still])) if (~still).any() else 0.0, float(np.max(dp / p_allow)),
                  df / f_allow)
        print(f"{name} m={m}: iters {r['iters']} status {r['status']}  share of the bound reached: u {shares[0]:.1e}  "
              f"p {shares[1]:.1e}  rss {shares[2]:.1e}")
        assert np.all(du <= u_allow), (name, m, "u", shares)
        assert np.all(dp <= p_allow), (name, m, "params", shares)
        assert df <= f_allow, (name, m, "rss", shares)


# ---- 2. outputs follow from the returned parameters ------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(case_list()))
def test_outputs_follow_from_returned_parameters(name):
    c = case_list()[name]
    stop = stop_trial(name)
    for m in sorted({1, 3, stop, stop + 5}):
        for want_fit in (True, False):
            r = _row(_run([c], m, want_fit=want_fit), 0)
            if c.expect.get("status") == 2:
                _check_status_2(r, c)
                assert r["status"] == 2 and r["iters"] == 0
                continue
            share = _check_outputs(r, c)
            assert 0 < r["iters"] <= m
            if want_fit:
                print(f"{name} m={m}: iters {r['iters']} status {r['status']}  deviations at {share:.1e} of 64 eps cond")
            if c.expect.get("asd_nan"):
                assert np.all(np.isnan(r["asd"][~c.fixed[:c.NA]]))
            else:
                assert np.all(np.isfinite(r["asd"]))


# ---- 3. staging rounds and CRLB rounds -------------------------------------------------------------------------------------
def _check_table_row(r, c):
    two_n = 2 * c.n_points
    share = _check_outputs(r, c, deviations=two_n >= c.P)
    if r["status"] == 0 and two_n > c.P:
        # The stopping step lowered the cost by at most ftol F, and on a linear problem with lambda D below J^T J a step
        # leaves less excess over the minimum than it removed.
        rows = c.tab[1:].reshape(-1, c.Q + 1)
        a, y = rows[:, :c.Q], rows[:, c.Q]
        best = np.linalg.lstsq(a[:, c.free], y - a[:, c.fixed] @ c.start[c.fixed], rcond=None)
        res = y - a[:, c.fixed] @ c.start[c.fixed] - a[:, c.free] @ best[0]
        assert r["rss"] <= float(res @ res) * (1.0 + 10.0 * c.ftol), (c.name, r["rss"], float(res @ res))
    return share


@pytest.mark.parametrize("P", orc.STAGING_P)
def test_staging_rounds_at_every_size(P):
    """P either side of q_pts = 64 / 32 and of one CRLB round (cap = 64 amplitudes); points either side of a staging
    round, one round short, and three rounds and a rest.  Every parameter is an amplitude: every deviation is checked."""
    for n in orc.staging_points(P):
        c = orc.staging_case(P, n)
        for m in (2, 200):
            r = _row(_run([c], m), 0)
            share = _check_table_row(r, c)
            print(f"P={P} n_points={n} m={m}: iters {r['iters']} status {r['status']}  deviations at {share:.1e} of 64 eps cond")
        if 2 * n > P:
            assert r["status"] == 0


@pytest.mark.parametrize("c", orc.crlb_round_cases(), ids=lambda c: c.name)
def test_second_crlb_round(c):
    """P = 80, where a round hands out 64 amplitudes: 64 (one round), 65, 80, and 120 of which 40 are fixed."""
    r = _row(_run([c], 200), 0)
    assert r["status"] == 0 and np.all(np.isfinite(r["asd"]))
    share = _check_table_row(r, c)
    assert np.count_nonzero(r["asd"] == 0.0) == int(c.fixed[:c.NA].sum())
    print(f"{c.name}: deviations at {share:.1e} of 64 eps cond, amplitudes {c.NA}, fixed {int(c.fixed.sum())}")


# ---- 4. what a voxel leaves behind in the LDS ------------------------------------------------------------------------------
def _mixed_rows():
    """40 rows of one `table` shape (Q = 6, one fixed, 9 points): a status-2 row, a zero-column row and a row whose
    Jacobian is NaN, each directly before an ordinary row."""
    rows = []
    for v in range(40):
        a, y, truth = orc.table_data(5, 9, 100 + v, Q=6, zero_cols=(3,) if v == 10 else ())
        start = truth + np.cos(v + np.arange(6.0))
        if v == 3:
            start[0] = 1e200  # the cost overflows: status 2
        rows.append(orc.Case(f"row{v}", "table", start, fixed=[False, False, False, False, False, True],
                             tab=orc.table_of(a, y, jadd=np.nan if v == 20 else 0.0), ftol=1e-6, n_amp=5))
    return rows


def _same_rows(a, b):
    for k in a:
        if a[k] is None:
            continue
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        if x.dtype == np.float64:
            nan = np.isnan(x)
            if not (np.array_equal(nan, np.isnan(y)) and np.array_equal(x[~nan].view(np.uint64), y[~nan].view(np.uint64))):
                return False
        elif not np.array_equal(x, y):
            return False
    return True


def test_rows_do_not_depend_on_their_predecessors():
    rows = _mixed_rows()
    alone = [_row(_run([c], 200), 0) for c in rows]
    assert alone[3]["status"] == 2 and alone[20]["status"] == 1 and np.all(np.isnan(alone[20]["asd"]))
    assert np.all(np.isnan(alone[10]["asd"])) and alone[10]["status"] == 0
    for v in (4, 11, 21):
        assert alone[v]["status"] == 0 and np.all(np.isfinite(alone[v]["asd"]))
        _check_outputs(alone[v], rows[v])
    _check_status_2(alone[3], rows[3])
    for grid in (1, 40, 1024):  # grid = 1: one workgroup fits them all in order
        out = _run(rows, 200, grid=grid)
        for v in range(40):
            assert _same_rows(_row(out, v), alone[v]), (grid, v)
    out = _run(rows[::-1], 200, grid=1)
    for v in range(40):
        assert _same_rows(_row(out, 39 - v), alone[v]), ("reversed", v)


# ---- 5. the host side refuses what would overrun ----------------------------------------------------------------------------
def test_refusals_leave_outputs_untouched():
    import torch

    lib = _probe()
    buf = torch.full((4096,), 7.0, dtype=torch.float64, device="cuda")
    b = buf.data_ptr()
    bt, lo, hi = np.full(4, orc.FREE, dtype=np.int32), np.full(4, -np.inf), np.full(4, np.inf)
    good = dict(kind=orc.KINDS.index("table"), start=b, tab=b, stride=1 + 2 * 3 * 5, factor=b, bt=bt.ctypes.data,
                lo=lo.ctypes.data, hi=hi.ctypes.data, nb=1, n=3, Q=4, NA=4, P=4, max_iter=5, ftol=1e-10, xtol=1e-10, params=b,
                asd=b, rss=b, status=b, iters=b, fit=b, u=b, counter=b, grid=1)
    two = np.array([orc.TWO, orc.FREE, orc.FREE, orc.FREE], dtype=np.int32)
    one_fixed = np.array([orc.FIXED, orc.FREE, orc.FREE, orc.FREE], dtype=np.int32)
    bad_type = np.array([5, orc.FREE, orc.FREE, orc.FREE], dtype=np.int32)
    bad = [dict(kind=-1), dict(kind=len(orc.KINDS)), dict(start=None), dict(tab=None), dict(factor=None), dict(bt=None),
           dict(lo=None), dict(hi=None), dict(params=None), dict(asd=None), dict(rss=None), dict(status=None),
           dict(iters=None), dict(u=None), dict(counter=None), dict(nb=-1), dict(nb=(1 << 20) + 1), dict(n=0), dict(n=4097),
           dict(Q=0), dict(Q=129), dict(NA=0), dict(NA=5), dict(P=0), dict(P=3), dict(P=5), dict(max_iter=-1),
           dict(ftol=-1.0), dict(xtol=float("nan")), dict(ftol=float("inf")), dict(stride=30), dict(grid=0), dict(grid=1025),
           dict(bt=two.ctypes.data), dict(bt=one_fixed.ctypes.data), dict(bt=bad_type.ctypes.data),
           dict(kind=orc.KINDS.index("rosenbrock")), dict(kind=orc.KINDS.index("exp2"), stride=12),
           dict(kind=orc.KINDS.index("powell"), n=3)]
    assert lib.xm_wgp_lm_fit(*dict(good, nb=0).values(), None) == 0  # the arguments the refusals depart from are valid
    for over in bad:
        a = dict(good, **over)
        assert lib.xm_wgp_lm_fit(*a.values(), None) == INVALID, over
    q81 = 81
    bt81, lo81, hi81 = np.full(q81, orc.FREE, dtype=np.int32), np.full(q81, -np.inf), np.full(q81, np.inf)
    a = dict(good, Q=q81, NA=q81, P=q81, n=1, stride=4096, bt=bt81.ctypes.data, lo=lo81.ctypes.data, hi=hi81.ctypes.data)
    assert lib.xm_wgp_lm_fit(*a.values(), None) == INVALID  # more free columns than the driver's LDS layout holds
    torch.cuda.synchronize()
    assert bool((buf == 7.0).all())
