"""``fit_kinetics``: the apparent conversion rate of every voxel of a dynamic series in one GPU launch.

The model is this backend's own, stated in DESIGN.md section 19: along `dim` (T repetitions at times t_n, flip angles
th_S[n] and th_m[n]) the substrate's magnetisation is taken from its measured amplitudes S_n and is piecewise linear
between excitations, and each product m follows Z' = -rho Z + k Zs(t) exactly::

    Zs_n = S_n / sin th_S[n],   Zs+_n = Zs_n cos th_S[n],   D_n = t_{n+1} - t_n,   x = rho D_n
    Z_0 = z,   Z_{n+1} = e^{-x} cos th_m[n] Z_n + k (w0_n Zs+_n + w1_n Zs_{n+1}),   P^_n = Z_n sin th_m[n]
    w1_n = D_n (x - 1 + e^{-x}) / x^2,   w0_n = D_n (1 - e^{-x}) / x - w1_n

Each (voxel, product) pair is one weighted least-squares fit of k (and, where asked, rho and z) by Levenberg-Marquardt
in lmfit's bound variables, one wave per fit (``xm_kinetics_fit``).  ``simulate_kinetics`` is the same model on the
host, for test and demonstration data.
"""
from __future__ import annotations

import copy as _copy
import math

import numpy as np

from .. import device as dev
from ..config import ATTRS
from ..labeled import Coordinate, LabeledArray, as_labeled, is_xarray
from .dataset import LabeledDataset

MAX_T, MAX_M = 256, 8
PRODUCT_VARS = ("rate", "rate_sd", "decay", "decay_sd", "initial", "auc_ratio", "rss", "status", "iterations")
_SERIES_X, _TERMS = 0.5, 16


def _series(x, den, num):
    acc = np.zeros_like(x)
    for i in range(_TERMS - 1, -1, -1):
        acc = acc * (-x) + num(i) / math.factorial(i + den)
    return acc


def interval_weights(decay, delta):
    """(E, w0, w1) of the intervals `delta` at the decay rate `decay` (broadcast): below x = decay delta = 0.5 the
    power series of DESIGN.md section 19, from there on the closed forms on expm1."""
    decay, delta = np.broadcast_arrays(np.asarray(decay, dtype=np.float64), np.asarray(delta, dtype=np.float64))
    x = decay * delta
    with np.errstate(all="ignore"):
        em = np.expm1(-x)
        f2 = (x + em) / (x * x)
        w1 = np.where(x < _SERIES_X, _series(x, 2, lambda i: 1.0), f2)
        w0 = np.where(x < _SERIES_X, _series(x, 2, lambda i: i + 1.0), -em / x - f2)
    return np.exp(-x), delta * w0, delta * w1


def _angles(v, t, what):
    a = np.deg2rad(np.asarray(v, dtype=np.float64))
    if a.ndim > 1 or (a.ndim == 1 and a.size != t):
        raise ValueError(f"flip_angle of {what}: a number or {t} values, got shape {a.shape}")
    a = np.ascontiguousarray(np.broadcast_to(a, (t,)))
    if not np.all((a > 0) & (a < np.pi / 2)):
        raise ValueError(f"flip_angle of {what} must lie strictly between 0 and 90 degrees")
    return a


def _check_times(times, t):
    tv = np.asarray(times, dtype=np.float64).reshape(-1)
    if tv.size != t:
        raise ValueError(f"times must hold one value per repetition ({t}), got {tv.size}")
    if not np.all(np.isfinite(tv)) or np.any(np.diff(tv) <= 0):
        raise ValueError("times must be finite and increase")
    return np.ascontiguousarray(tv)


def simulate_kinetics(substrate, times, rate, decay, initial=0.0, flip_angle=(10.0, 10.0)):
    """The forward model in host numpy fp64: the product's signal P^ [..., T] that the substrate signal `substrate`
    [..., T] drives at `times` [T] with the rate k = `rate`, the decay rho = `decay` and the magnetisation `initial`
    before the first excitation (numbers, or arrays over the leading axes).  `flip_angle`: (substrate, product) in
    degrees, each a number or T values."""
    s = np.asarray(substrate, dtype=np.float64)
    if s.ndim < 1 or s.shape[-1] < 2:
        raise ValueError("substrate must hold at least 2 repetitions along its last axis")
    t = s.shape[-1]
    tv = _check_times(times, t)
    if not isinstance(flip_angle, (tuple, list)) or len(flip_angle) != 2:
        raise ValueError("flip_angle must be a (substrate, product) pair in degrees")
    ths, thp = _angles(flip_angle[0], t, "the substrate"), _angles(flip_angle[1], t, "the product")
    lead = s.shape[:-1]
    k, rho, z = (np.broadcast_to(np.asarray(v, dtype=np.float64), lead) for v in (rate, decay, initial))
    if np.any(rho < 0):
        raise ValueError("decay must not be negative")
    zs = s / np.sin(ths)
    zsp = zs * np.cos(ths)
    out = np.empty(s.shape)
    zc = np.array(z, dtype=np.float64)
    out[..., 0] = zc * np.sin(thp[0])
    for n in range(t - 1):
        e, w0, w1 = interval_weights(rho, tv[n + 1] - tv[n])
        zc = e * np.cos(thp[n]) * zc + k * (w0 * zsp[..., n] + w1 * zs[..., n + 1])
        out[..., n + 1] = zc * np.sin(thp[n + 1])
    return out


def _variables(data, sigma):
    """(amplitude LabeledArray, crlb LabeledArray or None) of a fit Dataset or an amplitude array."""
    if isinstance(data, LabeledDataset):
        if "amplitude" not in data:
            raise ValueError("the Dataset has no variable 'amplitude'")
        return data["amplitude"], (data["crlb"] if sigma is None and "crlb" in data else None)
    if is_xarray(data) and hasattr(data, "data_vars"):
        if "amplitude" not in data.data_vars:
            raise ValueError("the Dataset has no variable 'amplitude'")
        crlb = as_labeled(data["crlb"]) if sigma is None and "crlb" in data.data_vars else None
        return as_labeled(data["amplitude"]), crlb
    return as_labeled(data), None


def _per_name(value, names, what):
    """value -> one entry per name: a mapping must name every one."""
    if isinstance(value, dict):
        missing = [n for n in names if n not in value]
        if missing:
            raise ValueError(f"{what} names no value for {missing}")
        return [value[n] for n in names]
    return [value for _ in names]


def _run_fit(sub, prod, weights, times, ths, thp, init, lo, hi, fixed, max_iter):
    """The launch: substrate [nb, T], products and weights [nb, M, T] (numpy) to the device, ``device.kinetics_fit``,
    every output back as numpy."""
    import torch

    to_dev = lambda a: torch.from_numpy(a).to("cuda")  # noqa: E731
    res = dev.kinetics_fit(to_dev(sub), to_dev(prod), times, ths, thp, init, lo, hi, fixed,
                           weights=to_dev(weights) if weights is not None else None, max_iter=max_iter)
    return {k: getattr(res, k).cpu().numpy() for k in ("params", "param_sd", "rss", "status", "iters", "fit", "auc_ratio")}


def fit_kinetics(data, substrate, products, dim: str = "repetition", times=None, flip_angle=None,
                 r1=(1.0 / 60.0, 1.0 / 10.0), rate_bounds=(0.0, 1.0), fit_initial: bool = False, sigma=None,
                 metabolite_dim: str = "Metabolite", max_iter: int = 200):
    """Fit the conversion rate from `substrate` to each of `products` (names on `metabolite_dim`) along `dim`, for
    every voxel at once.

    `data`: the Dataset of ``fit_amares`` / ``fit_basis`` (its ``amplitude``; with ``sigma=None`` the weights are 1 / sigma
    from sigma = crlb / 100 |amplitude|, and a point whose crlb is NaN, or whose amplitude and crlb are both 0 -- a
    failed fit -- gets weight 0), or an amplitude array with `metabolite_dim` (weights 1, or 1 / `sigma`).  `sigma`: a
    number or an array that broadcasts against the amplitudes.  `times` [s]: default the coordinate of `dim`.
    `flip_angle` [deg]: a number, a mapping name -> number or T values.  `r1` [1/s]: a number (fixed), a (lo, hi) pair
    (fitted, started in the middle), or a mapping product -> either.  `rate_bounds`: of k [1/s], started at a tenth of
    the way up.  `fit_initial`: fit the product's magnetisation before the first excitation (z >= 0, started at
    |P_j| / sin th_j of the first weighted repetition j), otherwise 0.  The substrate must be present at every repetition: it enters as data, unweighted.

    Returns a LabeledDataset (an ``xarray.Dataset`` for xarray input): rate, rate_sd, decay, decay_sd, initial,
    auc_ratio, rss, status (0 converged, 1 iteration cap, 2 non-finite data, 3 fewer weighted points than free
    parameters: zeros), iterations over (other dims..., "Metabolite" over the products), and fit in the dims of the
    amplitudes (NaN for the metabolites that are neither substrate nor product)."""
    amp, crlb = _variables(data, sigma)
    if dim not in amp.dims:
        raise ValueError(f"Dimension '{dim}' missing in the amplitudes (dims {tuple(amp.dims)}).")
    if metabolite_dim not in amp.dims:
        raise ValueError(f"Dimension '{metabolite_dim}' missing in the amplitudes (dims {tuple(amp.dims)}).")
    if dim == metabolite_dim:
        raise ValueError("dim and metabolite_dim must differ")
    mc = amp.coords.get(metabolite_dim)
    if mc is None:
        raise ValueError(f"the amplitudes carry no coordinate '{metabolite_dim}' to find the names on")
    names = [str(v) for v in np.asarray(mc.values)]
    products = [products] if isinstance(products, str) else [str(p) for p in products]
    substrate = str(substrate)
    for n in [substrate] + products:
        if n not in names:
            raise ValueError(f"'{n}' is not on '{metabolite_dim}' ({names})")
    if substrate in products or len(set(products)) != len(products):
        raise ValueError("the products must be distinct and must not include the substrate")
    m = len(products)
    if not 1 <= m <= MAX_M:
        raise ValueError(f"between 1 and {MAX_M} products, got {m}")
    t_axis, m_axis = amp.get_axis_num(dim), amp.get_axis_num(metabolite_dim)
    t = amp.shape[t_axis]
    if not 2 <= t <= MAX_T:
        raise ValueError(f"between 2 and {MAX_T} repetitions along '{dim}', got {t}")
    if times is None:
        tc = amp.coords.get(dim)
        if tc is None:
            raise ValueError(f"times is required: the amplitudes carry no coordinate '{dim}'")
        times = tc.values
    tv = _check_times(times, t)
    if flip_angle is None:
        raise ValueError("flip_angle is required (degrees): a number, or a mapping from each name to a number or T values")
    fl = _per_name(flip_angle, [substrate] + products, "flip_angle")
    ths = _angles(fl[0], t, substrate)
    thp = np.stack([_angles(v, t, p) for v, p in zip(fl[1:], products)])
    if max_iter < 1:
        raise ValueError(f"max_iter must be at least 1, got {max_iter}")

    k_lo, k_hi = (float(v) for v in rate_bounds)
    if not (np.isfinite(k_lo) and np.isfinite(k_hi) and k_lo < k_hi):
        raise ValueError(f"rate_bounds must be two finite increasing values, got {rate_bounds}")
    init, lo, hi = np.zeros((m, 3)), np.zeros((m, 3)), np.zeros((m, 3))
    fixed = np.zeros((m, 3), dtype=bool)
    init[:, 0], lo[:, 0], hi[:, 0] = k_lo + 0.1 * (k_hi - k_lo), k_lo, k_hi
    for j, (v, p) in enumerate(zip(_per_name(r1, products, "r1"), products)):
        v = np.asarray(v, dtype=np.float64)
        if v.shape == ():
            if not (np.isfinite(v) and v >= 0):
                raise ValueError(f"r1 of {p} must be finite and not negative, got {v}")
            init[j, 1] = lo[j, 1] = hi[j, 1] = float(v)
            fixed[j, 1] = True
        elif v.shape == (2,):
            if not (np.all(np.isfinite(v)) and 0 <= v[0] < v[1]):
                raise ValueError(f"r1 of {p}: a (lo, hi) pair needs 0 <= lo < hi, both finite, got {tuple(v)}")
            lo[j, 1], hi[j, 1], init[j, 1] = v[0], v[1], 0.5 * (v[0] + v[1])
        else:
            raise ValueError(f"r1 of {p} must be a number or a (lo, hi) pair, got shape {v.shape}")
    hi[:, 2] = np.inf
    init[:, 2] = np.nan if fit_initial else 0.0
    fixed[:, 2] = not fit_initial

    # (other..., metabolite, repetition)
    vals = np.moveaxis(np.asarray(amp.values, dtype=np.float64), (m_axis, t_axis), (-2, -1))
    lead = vals.shape[:-2]
    idx = [names.index(p) for p in products]
    sub = np.ascontiguousarray(vals[..., names.index(substrate), :]).reshape(-1, t)
    prod = np.ascontiguousarray(vals[..., idx, :]).reshape(-1, m, t)
    weights = None
    if sigma is not None:
        sg = np.asarray(sigma.values if isinstance(sigma, LabeledArray) or is_xarray(sigma) else sigma, dtype=np.float64)
        try:
            sg = np.broadcast_to(sg, amp.shape)
        except ValueError:
            raise ValueError(f"sigma of shape {sg.shape} does not broadcast against the amplitudes {amp.shape}") from None
        if np.any(sg < 0) or np.any(np.isnan(sg)):
            raise ValueError("sigma must not be negative or NaN")
        sg = np.moveaxis(sg, (m_axis, t_axis), (-2, -1))[..., idx, :]
        with np.errstate(divide="ignore"):
            weights = np.where(sg > 0, 1.0 / sg, 0.0)
    elif crlb is not None:
        if tuple(crlb.dims) != tuple(amp.dims):
            raise ValueError("crlb and amplitude must share their dims")
        cv = np.moveaxis(np.asarray(crlb.values, dtype=np.float64), (m_axis, t_axis), (-2, -1))[..., idx, :]
        av = vals[..., idx, :]
        sg = cv / 100.0 * np.abs(av)
        with np.errstate(divide="ignore", invalid="ignore"):
            weights = np.where(np.isfinite(sg) & (sg > 0), 1.0 / sg, 0.0)
    if weights is not None:
        weights = np.ascontiguousarray(weights).reshape(-1, m, t)

    res = _run_fit(sub, prod, weights, tv, ths, thp, init, lo, hi, fixed, int(max_iter))
    params, psd = res["params"], res["param_sd"]
    out = {"rate": params[..., 0], "rate_sd": psd[..., 0], "decay": params[..., 1], "decay_sd": psd[..., 1],
           "initial": params[..., 2], "auc_ratio": res["auc_ratio"], "rss": res["rss"], "status": res["status"],
           "iterations": res["iters"]}

    other = tuple(d for d in amp.dims if d not in (dim, metabolite_dim))
    vcoords = {k: c.copy() for k, c in amp.coords.items() if c.dim in other}
    pcoords = dict(vcoords)
    pcoords["Metabolite"] = Coordinate("Metabolite", np.array(products))
    data_vars = {k: LabeledArray(out[k].reshape(lead + (m,)), other + ("Metabolite",), pcoords) for k in PRODUCT_VARS}
    fit = np.full(vals.shape, np.nan)
    fit[..., idx, :] = res["fit"].reshape(lead + (m, t))
    fit = np.moveaxis(fit, (-2, -1), (m_axis, t_axis))
    data_vars["fit"] = LabeledArray(fit, amp.dims, {k: c.copy() for k, c in amp.coords.items()})
    attrs = _copy.copy(data.attrs) if hasattr(data, "attrs") else {}
    attrs.update({ATTRS.kinetics_model: "two-site, inputless, substrate from data", ATTRS.kinetics_substrate: substrate,
                  ATTRS.kinetics_dim: dim,
                  ATTRS.kinetics_flip_angle: {n: np.rad2deg(a).tolist() for n, a in zip([substrate] + products, [ths, *thp])},
                  ATTRS.kinetics_rate_bounds: (k_lo, k_hi),
                  ATTRS.kinetics_decay_bounds: {p: (float(lo[j, 1]), float(hi[j, 1])) for j, p in enumerate(products)},
                  ATTRS.kinetics_fit_initial: bool(fit_initial)})
    ds = LabeledDataset(data_vars, attrs)
    return ds.to_xarray() if is_xarray(data) else ds
