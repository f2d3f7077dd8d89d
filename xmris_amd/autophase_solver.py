"""Host side of ``autophase``: the O(1)-per-dataset search for (p0, p1) on the ONE 1-D slice
that holds the global |X| maximum (reference ``processing/phasing.py:100-157, 257-287``).

The reference drives ``scipy.optimize.differential_evolution`` (best1bin, tol=0.01, seed=42)
with objectives that go through ``phase()`` -> xarray on every evaluation.  Here the same
optimiser is driven with the same arithmetic on plain ndarrays (no xarray object per
evaluation).  The data-parallel parts of autophase -- the global arg-max and the broadcast
phase multiply over the whole dataset -- run on the GPU (``xm_pipeline_fused``).
"""
from __future__ import annotations

import ctypes
import os
import time

import numpy as np

from .cpu_budget import burst_threads, default_threads, scarce_cpus, stream_threads  # noqa: F401 -- callers find them here
from .polish_workers import PolishWorkers, polish_workers  # noqa: F401 -- likewise

METHODS = ("acme", "peak_minima", "positivity")
MSG_METHOD = "Method must be 'acme', 'peak_minima', or 'positivity'"  # phasing.py:268 (kept in dims.py too)


def phase_angles(coords: np.ndarray, p0: float, p1: float, pivot: float):
    """phasing.py:56-69: phi = rad(p0) + rad(p1) * (c - pivot) / (max c - min c); scalar if range 0."""
    x_min = float(coords.min())
    x_max = float(coords.max())
    x_range = x_max - x_min
    p0_rad = np.radians(p0)
    p1_rad = np.radians(p1)
    if x_range == 0:
        return p0_rad
    return p0_rad + p1_rad * ((coords - pivot) / x_range)


def phase_table(coords: np.ndarray, p0: float, p1: float, pivot: float) -> np.ndarray:
    """e^{i phi} over the axis in fp64 (phasing.py:73); always an array of len(coords)."""
    ph = phase_angles(np.asarray(coords, dtype=np.float64), p0, p1, pivot)
    f = np.exp(1.0j * ph)
    if np.ndim(f) == 0:
        f = np.full(len(coords), f, dtype=np.complex128)
    return f


def search_bounds(p0_only: bool):
    """phasing.py:270-274: p0 in degrees and, unless `p0_only`, p1 in degrees over the axis."""
    return [(-180.0, 180.0)] if p0_only else [(-180.0, 180.0), (-4000.0, 4000.0)]


def default_polish() -> str:
    """The polish route of a call that names none (`XMRIS_AMD_POLISH`; see `solve`)."""
    return os.environ.get("XMRIS_AMD_POLISH", "exact")


# The three objectives on `real`, the real part of the phased slice.  These statements are the ONLY copy: every promise
# that (p0, p1) equal the reference's exactly rests on their operation order (numpy ufuncs, numpy's summation order) --
# the order is the reference's, statement by statement; the names are this project's.

def _acme(real):
    """phasing.py:100-122 -- entropy of the first derivative + negativity penalty."""
    slope = np.abs((real[1:] - real[:-1]) / 2)
    weight = slope / np.sum(slope)
    weight[weight == 0] = 1
    entropy = np.sum(-weight * np.log(weight))
    negative = real - np.abs(real)
    penalty = 0.0
    if np.sum(negative) < 0:
        penalty = np.sum((negative / 2) ** 2)
    return (entropy + 1000 * penalty) / real.shape[-1] / np.max(real)


def _window(n, target_idx, index_width):
    """[first, stop) of the bins within `index_width` of the target peak (phasing.py:133-134, 150-151)."""
    return max(0, target_idx - index_width), min(n, target_idx + index_width)


def _peak_minima(real, target_idx, index_width):
    """phasing.py:125-139 -- the lowest points left and right of the peak at the same height."""
    first, stop = _window(len(real), target_idx, index_width)
    left = np.min(real[first:target_idx]) if first < target_idx else real[target_idx]
    right = np.min(real[target_idx:stop]) if stop > target_idx else real[target_idx]
    return np.abs(left - right)


def _roi_positivity(real, target_idx, index_width):
    """phasing.py:142-157 -- negative area around the peak, weighted five-fold, against the positive area."""
    first, stop = _window(len(real), target_idx, index_width)
    roi = real[first:stop]
    return np.sum(np.abs(roi[roi < 0])) * 5.0 - np.sum(roi[roi > 0])


def _phased_real(ph, sl, coords, pivot):
    p0 = ph[0]
    p1 = ph[1] if len(ph) > 1 else 0.0
    return np.real(sl * np.exp(1.0j * phase_angles(coords, p0, p1, pivot)))


def acme_score(ph, sl, coords, pivot):
    """phasing.py:100-122 at ph = (p0[, p1]) on the slice `sl` over `coords`."""
    return _acme(_phased_real(ph, sl, coords, pivot))


def peak_minima_score(ph, sl, coords, pivot, target_idx, index_width):
    """phasing.py:125-139."""
    return _peak_minima(_phased_real(ph, sl, coords, pivot), target_idx, index_width)


def roi_positivity_score(ph, sl, coords, pivot, target_idx, index_width):
    """phasing.py:142-157."""
    return _roi_positivity(_phased_real(ph, sl, coords, pivot), target_idx, index_width)


class NumpyObjective:
    """The objective as the reference evaluates it (numpy ufuncs, numpy's summation order, the platform's libm / SVML)
    for one slice, with what does not depend on (p0, p1) computed
    ONCE: `phase_angles` evaluates (coords - pivot) / (max - min) -- the same two numpy statements on the same
    operands, hence the same bits -- on every call (a min, a max, a subtraction and a division over the axis: 25 us
    of a 390 us evaluation at 8192 bins).  `obj(ph)` equals `acme_score(ph, ...)` etc. to the bit
    (tests/test_abi_and_host.py); `nfev` counts the calls, `score_batch` is the interface `polish_lbfgsb`'s forward
    differences use."""

    def __init__(self, sl, coords, pivot, target_idx, index_width, method):
        self.sl, self.roi = sl, () if method == "acme" else (target_idx, index_width)
        self.score = {"acme": _acme, "peak_minima": _peak_minima, "positivity": _roi_positivity}[method]
        x_range = float(coords.max()) - float(coords.min())
        self.u = None if x_range == 0 else (coords - pivot) / x_range
        self.nfev = 0

    def __call__(self, ph):
        self.nfev += 1
        p0_rad = np.radians(ph[0])
        p1_rad = np.radians(ph[1] if len(ph) > 1 else 0.0)
        ang = p0_rad if self.u is None else p0_rad + p1_rad * self.u
        return self.score(np.real(self.sl * np.exp(1.0j * ang)), *self.roi)

    def score_batch(self, pts):
        return np.array([self(p) for p in np.asarray(pts, dtype=np.float64)])


def index_width_of(coords: np.ndarray, peak_width: float) -> int:
    """phasing.py:245-247."""
    step = np.abs(coords[1] - coords[0])
    return max(1, int(round((peak_width / 2.0) / step)))


class NativeObjective:
    """The three objectives evaluated by libxmris_hip.so's host solver (vectorised C++, fp64)."""

    def __init__(self, sl, coords, pivot, target_idx, index_width, method):
        from . import _lib

        self._lib = _lib.load()
        self._sl = np.ascontiguousarray(sl, dtype=np.complex128)
        self._c = np.ascontiguousarray(coords, dtype=np.float64)
        self._h = self._lib.xm_solver_create(self._sl.ctypes.data, self._c.ctypes.data, len(self._sl), float(pivot),
                                             METHODS.index(method), int(target_idx), int(index_width))
        if not self._h:
            raise ValueError("xm_solver_create rejected the slice (needs n >= 2 and a valid target index)")
        self.set_threads(default_threads())

    def __call__(self, x):
        xx = np.ascontiguousarray(x, dtype=np.float64)
        return self._lib.xm_solver_score(self._h, xx.ctypes.data, len(xx))

    def set_threads(self, n):
        return self._lib.xm_solver_set_threads(self._h, int(n))

    def evaluations(self):
        """Objective evaluations performed so far (>= the sequential algorithm's nfev: xm_solver_de
        evaluates trials speculatively in batches)."""
        return int(self._lib.xm_solver_nfev(self._h))

    def score_batch(self, xs):
        xs = np.asarray(xs, dtype=np.float64)
        buf = np.zeros((xs.shape[0], 2))
        buf[:, :xs.shape[1]] = xs
        out = np.empty(xs.shape[0])
        self._lib.xm_solver_score_batch(self._h, buf.ctypes.data, int(xs.shape[1]), int(xs.shape[0]), out.ctypes.data)
        return out

    def fg(self, x, lb, ub):
        """(f, forward-difference gradient) at x inside the box [lb, ub] in ONE native call (`xm_solver_fg`): what
        `polish_lbfgsb` otherwise spells out in ~20 numpy operations per request, under the interpreter lock that the
        other searches in flight and the launch thread are waiting for."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        g = np.empty(len(x))
        f = np.empty(1)
        rc = self._lib.xm_solver_fg(self._h, x.ctypes.data, len(x), lb.ctypes.data, ub.ctypes.data, f.ctypes.data,
                                    g.ctypes.data)
        if rc:
            raise ValueError("xm_solver_fg rejected its arguments")
        return float(f[0]), g

    def de(self, p0_only, seed=42, tol=0.01, maxiter=1000):
        x = (ctypes.c_double * 2)()
        fun, nfev, nit = ctypes.c_double(), ctypes.c_int(), ctypes.c_int()
        rc = self._lib.xm_solver_de(self._h, int(bool(p0_only)), seed, tol, maxiter, x, ctypes.byref(fun),
                                    ctypes.byref(nfev), ctypes.byref(nit))
        return rc, np.array(x[:1 if p0_only else 2]), fun.value, nfev.value, nit.value

    def __del__(self):
        try:
            self._lib.xm_solver_destroy(self._h)
        except Exception:
            pass


def polish_lbfgsb(obj, x0, bounds, force_scipy: bool = False):
    """`scipy.optimize.minimize(obj, x0, method="L-BFGS-B", bounds=bounds)` -- the polish step of
    `differential_evolution` (phasing.py:276-284 runs it with scipy's defaults) -- without the per-call Python
    machinery around it (`ScalarFunction`, bounds standardisation, `approx_derivative`'s generic front end: 0.3-0.5 ms
    of interpreter time per search, held under the GIL while other searches and the launch thread wait).  Same
    compiled core (`scipy.optimize._lbfgsb.setulb`), same defaults (maxcor 10, ftol 2.22e-9, gtol 1e-5, eps 1e-8,
    maxls 20), same forward-difference gradient as `approx_derivative(method="2-point", abs_step=1e-8, bounds=...)`
    with its exactly-representable step and its flip at the upper bound, same evaluation count (the gradient's
    evaluations included, the repeated request for f at x0 answered from the cache like `ScalarFunction` does):
    x, fun, nfev, nit, success are scipy's to the bit (tests/test_abi_and_host.py).  The three points of one
    f-and-gradient request go to the native objective in ONE call.  Any surprise in scipy's private interface
    (this follows 1.15.3, the version SURVEY pins) -> the public `minimize`."""
    import scipy
    import scipy.optimize

    try:
        # the private entry point is followed as scipy 1.15 has it (SURVEY 8c pins 1.15.3); any other release takes
        # the public route
        if force_scipy or not scipy.__version__.startswith("1.15."):
            raise ImportError
        from scipy.optimize import _lbfgsb
        from scipy.optimize._lbfgsb_py import _minimize_lbfgsb  # noqa: F401 -- same module layout as the code followed
    except ImportError:
        return scipy.optimize.minimize(obj, np.copy(x0), method="L-BFGS-B", bounds=bounds)
    lb = np.array([b[0] for b in bounds], dtype=np.float64)
    ub = np.array([b[1] for b in bounds], dtype=np.float64)
    n = len(lb)
    m, maxls, maxfun, maxiter = 10, 20, 15000, 15000
    factr = 2.2204460492503131e-09 / np.finfo(float).eps
    pgtol, abs_step = 1e-5, 1e-8
    x0 = np.clip(np.asarray(x0, dtype=np.float64).ravel(), lb, ub)
    state = {"nfev": 0, "x": None, "f": None, "g": None}
    native_fg = hasattr(obj, "fg") and n <= 2 and not os.environ.get("XM_POLISH_NUMPY_FG")  # (switch: cross-checks)

    def func_and_grad(x):
        if state["x"] is not None and np.array_equal(x, state["x"]):
            return state["f"], state["g"]
        xc = np.array(x, dtype=np.float64)
        if native_fg:  # the same arithmetic in one native call (bit-equal: tests/test_abi_and_host.py)
            f, g = obj.fg(xc, lb, ub)
            state["nfev"] += n + 1
            state.update(x=xc, f=f, g=g)
            return f, g
        # approx_derivative: absolute step, relative fallback when it vanishes, flipped where it leaves the bounds
        sign = (xc >= 0).astype(float) * 2 - 1
        h = np.full(n, abs_step)
        h = np.where(((xc + h) - xc) == 0, np.finfo(np.float64).eps ** 0.5 * sign * np.maximum(1.0, np.abs(xc)), h)
        lower, upper = xc - lb, ub - xc
        xt = xc + h
        violated = (xt < lb) | (xt > ub)
        fitting = np.abs(h) <= np.maximum(lower, upper)
        h[violated & fitting] *= -1
        forward = (upper >= lower) & ~fitting
        h[forward] = upper[forward]
        backward = (upper < lower) & ~fitting
        h[backward] = -lower[backward]
        pts = np.tile(xc, (n + 1, 1))
        dx = np.empty(n)
        for i in range(n):
            pts[1 + i, i] += h[i]
            dx[i] = pts[1 + i, i] - xc[i]  # the step as an exactly representable number
        vals = obj.score_batch(pts)
        state["nfev"] += n + 1
        f = float(vals[0])
        g = (vals[1:] - f) / dx
        state.update(x=xc, f=f, g=g)
        return f, g

    func_and_grad(x0)  # ScalarFunction evaluates f and the gradient at x0 when it is built
    nbd = np.full(n, 2, dtype=np.int32)
    x = np.array(x0, dtype=np.float64)
    f = np.array(0.0, dtype=np.int32)
    g = np.zeros((n,), dtype=np.int32)
    wa = np.zeros(2 * m * n + 5 * n + 11 * m * m + 8 * m, np.float64)
    iwa = np.zeros(3 * n, dtype=np.int32)
    task = np.zeros(2, dtype=np.int32)
    ln_task = np.zeros(2, dtype=np.int32)
    lsave = np.zeros(4, dtype=np.int32)
    isave = np.zeros(44, dtype=np.int32)
    dsave = np.zeros(29, dtype=np.float64)
    nit = 0
    try:
        while True:
            g = g.astype(np.float64)
            _lbfgsb.setulb(m, x, lb, ub, nbd, f, g, factr, pgtol, wa, iwa, task, lsave, isave, dsave, maxls, ln_task)
            if task[0] == 3:
                f, g = func_and_grad(x)
            elif task[0] == 1:
                nit += 1
                if nit >= maxiter:
                    task[0], task[1] = 5, 504
                elif state["nfev"] > maxfun:
                    task[0], task[1] = 5, 502
            else:
                break
    except (TypeError, ValueError):  # another scipy: its private entry point takes other arguments
        return scipy.optimize.minimize(obj, np.copy(x0), method="L-BFGS-B", bounds=bounds)
    return scipy.optimize.OptimizeResult(x=x, fun=f, jac=g, nfev=state["nfev"], nit=nit, success=bool(task[0] == 4),
                                         status=0 if task[0] == 4 else (1 if (state["nfev"] > maxfun or nit >= maxiter) else 2))


def _accepted(res, fun, bounds) -> bool:
    """`differential_evolution`'s rule for its polish: taken when it succeeded, lowered the objective below the
    generations' best `fun` and stayed inside the bounds."""
    lo = np.array([b[0] for b in bounds])
    hi = np.array([b[1] for b in bounds])
    return bool(res.fun < fun and res.success and np.all(res.x <= hi) and np.all(lo <= res.x))


def polish_reference(sl, coords, pivot, target_idx, index_width, method, p0_only, x):
    """The polish of `differential_evolution` on the reference's own route (phasing.py:276-284 with scipy's defaults):
    scipy's L-BFGS-B minimiser on the NUMPY objective from the generations' best member `x`; accepted when it lowers
    that objective.  Returns (x, fun, nfev, polished).  The one polish of every engine whose generations ended with a
    member that does not pass scipy's projected-gradient test (`polish="exact"`; the device search's `needs_polish`).

    The polish walks a finite-difference gradient (steps of 1e-8 degrees): on a flat landscape (pure noise, the README
    quick start) the LAST BITS of the objective decide where it ends, and the native objective's differ from numpy's
    (vectorised log / sincos recurrence, its own summation order).  Driving scipy's minimiser with the numpy objective
    reproduces the reference's polish bit for bit whenever the generations took the same decisions -- at ~0.15 ms per
    evaluation instead of 6 us."""
    bounds = search_bounds(p0_only)
    x = np.asarray(x, dtype=np.float64)[:len(bounds)]
    fn = NumpyObjective(np.asarray(sl, dtype=np.complex128), np.asarray(coords, dtype=np.float64), pivot, target_idx,
                        index_width, method)
    fun = float(fn(x))
    # scipy's minimiser itself, driven without its per-call Python front end (`polish_lbfgsb`: the same compiled
    # L-BFGS-B core, the same forward differences, bit for bit -- tests/test_abi_and_host.py); 4.9 -> 2.6 ms per polish
    res = polish_lbfgsb(fn, np.copy(x), bounds)
    if _accepted(res, fun, bounds):
        return np.asarray(res.x, dtype=np.float64), float(res.fun), int(res.nfev), True
    return x, fun, int(res.nfev), False


def _gradient_test(obj, x, bounds) -> bool:
    """Would scipy's polish keep the generations' best member `x`?  What that polish does in the usual case is
    NOTHING: L-BFGS-B evaluates f and the forward-difference
    gradient at the member, finds the projected gradient below pgtol = 1e-5 (the scores are
    ~1e-3 and the parameters are degrees: gradients of 1e-8 ... 1e-6 at a converged population) and returns that
    member -- `result.fun < fun` fails and differential_evolution keeps it (measured: 19 of 20 ACME searches,
    nit = 0, nfev = 3).  That test is made here with the native objective (three evaluations, one native call;
    the noise of a difference quotient over steps of 1e-8 is ~1e-11, five orders below pgtol), and it holds only
    with a factor of two to spare."""
    lo = np.array([b[0] for b in bounds])
    hi = np.array([b[1] for b in bounds])
    xc = np.clip(np.asarray(x, dtype=np.float64), lo, hi)
    _, g0 = obj.fg(xc, lo, hi)
    pg = np.where(g0 < 0, np.maximum(xc - hi, g0), np.minimum(xc - lo, g0))  # L-BFGS-B's projgr, both bounds set
    return float(np.max(np.abs(pg))) <= 0.5 * 1e-5


def _solve_native(sl, coords, pivot, target_idx, index_width, method, p0_only, threads=None, polish="exact"):
    """scipy's differential_evolution(best1bin, tol=0.01, seed=42) restated natively: the generations
    run in libxmris_hip.so (same RandomState stream, same trial vectors as scipy given equal objective
    values, objectives vectorised over host cores), the final L-BFGS-B polish is scipy's, exactly as
    `DifferentialEvolutionSolver.solve` does it.  polish="exact": a member that passes `_gradient_test` is kept, any
    other is polished on the reference's route -- either way the result is the reference's whenever the generations
    took the same decisions."""
    import scipy.optimize

    t0 = time.perf_counter()
    obj = NativeObjective(sl, coords, pivot, target_idx, index_width, method)
    if threads is not None:  # several searches in flight share the host's cores
        obj.set_threads(max(1, int(threads)))
    rc, x, fun, nfev, nit = obj.de(p0_only)  # worker pool spins for the duration of the generations
    t1 = time.perf_counter()
    # the polish's isolated evaluations below run serially (the pool is parked outside xm_solver_de)
    bounds = search_bounds(p0_only)
    if polish == "exact" and _gradient_test(obj, x, bounds):
        route, polished = "none", False
        nfev += len(bounds) + 1  # (f and the forward differences, as scipy counts them)
    elif polish in ("exact", "numpy"):  # a single accessor call can afford its milliseconds; a stream hands them to helpers
        route = "numpy"
        x, fun, nfev_polish, polished = polish_reference(sl, coords, pivot, target_idx, index_width, method, p0_only, x)
        nfev += nfev_polish
    else:
        route = polish
        res = polish_lbfgsb(obj, np.copy(x), bounds)
        nfev += res.nfev
        polished = _accepted(res, fun, bounds)
        if polished:
            x, fun = res.x, float(res.fun)
    return scipy.optimize.OptimizeResult(x=x, fun=fun, nfev=nfev, nit=nit, success=(rc == 0), polished=polished,
                                         polish_route=route, t_generations=t1 - t0, t_polish=time.perf_counter() - t1)


def solve(sl: np.ndarray, coords: np.ndarray, pivot: float, target_idx: int, index_width: int,
          method: str = "acme", p0_only: bool = False, disp: bool = False, engine: str = "native", threads=None,
          polish: str = "exact"):
    """phasing.py:257-287.  Returns (p0, p1, OptimizeResult).  engine="native" (default) runs the
    optimiser's generations in libxmris_hip.so; engine="scipy" calls scipy's driver with the numpy
    objectives above (the reference's own route, ~15x slower; kept for cross-checks).  `polish` (native engine):
    "exact" (default) -- the projected-gradient test scipy's polish starts with is made natively, and only a search
    that does not pass it is polished, on the reference's route (numpy objective); "numpy" -- always that route;
    "native" -- scipy's compiled L-BFGS-B core on the native objective (round 3's streaming default: its end point
    can differ from the reference's by ~1e-3 degrees when a polish iterates).  See `_solve_native`."""
    import scipy.optimize

    sl = np.asarray(sl, dtype=np.complex128)
    coords = np.asarray(coords, dtype=np.float64)
    if method not in METHODS:
        raise ValueError(MSG_METHOD)
    if engine == "native" and len(sl) >= 2:
        opt = _solve_native(sl, coords, pivot, target_idx, index_width, method, p0_only, threads, polish)
    else:
        fn = {"acme": acme_score, "peak_minima": peak_minima_score, "positivity": roi_positivity_score}[method]
        roi = () if method == "acme" else (target_idx, index_width)
        opt = scipy.optimize.differential_evolution(fn, bounds=search_bounds(p0_only), args=(sl, coords, pivot) + roi,
                                                    strategy="best1bin", tol=0.01, seed=42, disp=disp)
    return float(opt.x[0]), (float(opt.x[1]) if not p0_only else 0.0), opt
