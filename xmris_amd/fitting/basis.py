"""``fit_basis``: linear-combination (basis-set) quantification of every FID of an N-dimensional array in one GPU launch.

The estimator is this backend's own, stated in DESIGN.md section 15: each metabolite is one simulated or measured FID
``B_m``; per voxel the fit adjusts the amplitudes ``a_m >= 0`` and, per group of metabolites, a shift, a Lorentzian and
(``lineshape="voigt"``) a Gaussian broadening, plus one zero-order phase::

    x^_n = e^{i phi} sum_m a_m B_m[n] exp(-d_g t_n - s_g t_n^2 + i 2 pi f_g t_n),   g = group(m),  t_n = n dt

by Levenberg-Marquardt in lmfit's bound variables with the analytic Jacobian, one workgroup per voxel
(``xm_basis_fit``), the iteration of ``fit_amares``.
"""
from __future__ import annotations

import copy as _copy

import numpy as np

from .. import device as dev
from ..labeled import Coordinate, LabeledArray, as_labeled, is_xarray
from .dataset import LabeledDataset

LINESHAPES = ("voigt", "lorentzian")
MAX_FREE = 80  # free columns of one fit (the kernel's limit, as for fit_amares)
METAB_VARS = ("amplitude", "crlb", "snr")
GROUP_VARS = ("shift", "linewidth", "gaussian")
VOXEL_VARS = ("phase", "rss", "status", "iters")
_LN2 = float(np.log(2.0))


def gaussian_damping(fwhm_hz):
    """s [1/s^2] of exp(-s t^2) whose line has the FWHM `fwhm_hz`: w = 2 sqrt(ln 2 s) / pi."""
    return (np.pi * np.asarray(fwhm_hz, dtype=np.float64)) ** 2 / (4.0 * _LN2)


def gaussian_fwhm(s):
    """FWHM [Hz] of the line of exp(-s t^2): the inverse of ``gaussian_damping``."""
    return 2.0 * np.sqrt(_LN2 * np.asarray(s, dtype=np.float64)) / np.pi


def parse_groups(groups, names):
    """`groups` -> (index [M] int32, labels): None: one common group "all"; "each": every metabolite its own group,
    labelled by its name; a list of M labels: metabolites with equal labels share a group, groups numbered in order of
    first appearance."""
    m = len(names)
    if groups is None:
        return np.zeros(m, dtype=np.int32), ["all"]
    if isinstance(groups, str):
        if groups != "each":
            raise ValueError(f"groups must be None, 'each' or a list of {m} labels, got {groups!r}")
        return np.arange(m, dtype=np.int32), [str(v) for v in names]
    labels = list(groups)
    if len(labels) != m:
        raise ValueError(f"groups must hold one label per metabolite ({m}), got {len(labels)}")
    order = []
    for v in labels:
        if v not in order:
            order.append(v)
    return np.array([order.index(v) for v in labels], dtype=np.int32), order


def basis_parameters(n_metab, n_groups, lineshape="voigt", max_shift=10.0, max_broadening=20.0, broadening_start=2.0,
                     max_gaussian=20.0, gaussian_start=2.0, fit_phase=True, amplitude_start=None):
    """(init, lo, hi, fixed), each [Q = M + 3 G + 1] in fitting units and in the layout of ``xm_basis_fit``: amplitudes
    (lower bound 0 only; NaN start: automatic), shifts [Hz] (+-max_shift, start 0), Lorentzian dampings [1/s]
    ([0, pi max_broadening], start pi broadening_start), Gaussian dampings [1/s^2] (two-sided up to max_gaussian's,
    start gaussian_start's; fixed at 0 for ``lineshape="lorentzian"``), phase [rad] (unbounded, start 0)."""
    if lineshape not in LINESHAPES:
        raise ValueError(f"lineshape must be one of {LINESHAPES}, got {lineshape!r}")
    m, g = int(n_metab), int(n_groups)
    if not (max_shift > 0 and np.isfinite(max_shift)):
        raise ValueError(f"max_shift must be positive and finite, got {max_shift}")
    if not (0 < broadening_start < max_broadening and np.isfinite(max_broadening)):
        raise ValueError(f"broadening_start must lie strictly inside (0, max_broadening), got {broadening_start} and "
                         f"{max_broadening}")
    if lineshape == "voigt" and not (0 < gaussian_start < max_gaussian and np.isfinite(max_gaussian)):
        raise ValueError(f"gaussian_start must lie strictly inside (0, max_gaussian), got {gaussian_start} and "
                         f"{max_gaussian}")
    q = m + 3 * g + 1
    init, lo, hi, fixed = np.zeros(q), np.zeros(q), np.zeros(q), np.zeros(q, dtype=bool)
    if amplitude_start is None:
        init[:m] = np.nan
    else:
        a0 = np.asarray(amplitude_start, dtype=np.float64).reshape(-1)
        if a0.size != m or not np.all(np.isfinite(a0)) or np.any(a0 < 0):
            raise ValueError(f"amplitude_start must hold {m} finite values >= 0")
        init[:m] = a0
    hi[:m] = np.inf
    lo[m:m + g], hi[m:m + g] = -float(max_shift), float(max_shift)
    init[m + g:m + 2 * g], hi[m + g:m + 2 * g] = np.pi * broadening_start, np.pi * max_broadening
    if lineshape == "voigt":
        init[m + 2 * g:m + 3 * g] = gaussian_damping(gaussian_start)
        hi[m + 2 * g:m + 3 * g] = gaussian_damping(max_gaussian)
    else:
        fixed[m + 2 * g:m + 3 * g] = True
    lo[-1], hi[-1] = -np.inf, np.inf
    fixed[-1] = not fit_phase
    return init, lo, hi, fixed


def _dwell(coord, what, dim):
    if coord is None or len(coord.values) < 2:
        raise ValueError(f"{what} needs a coordinate '{dim}' of at least 2 points: its dwell time is read from it")
    tv = np.asarray(coord.values, dtype=np.float64)
    return float(tv[1] - tv[0])


def _basis_array(basis, dim, names):
    """basis -> (values [M, n_basis] complex128, dwell or None, names).  A labelled basis must carry the coordinate
    `dim`; a plain array is [metabolite, time] and is taken to be on the data's grid."""
    labelled = isinstance(basis, LabeledArray) or is_xarray(basis)
    if labelled:
        b = as_labeled(basis)
        if dim not in b.dims:
            raise ValueError(f"Dimension '{dim}' missing in the basis.")
        if b.ndim not in (1, 2):
            raise ValueError(f"the basis must be [metabolite, {dim}], got dims {tuple(b.dims)}")
        dwell = _dwell(b.coords.get(dim), "the basis", dim)
        vals = np.asarray(b.values)
        if b.ndim == 1:
            vals = vals[None, :]
        elif b.get_axis_num(dim) == 0:
            vals = vals.T
        if names is None and b.ndim == 2:
            mdim = [d for d in b.dims if d != dim][0]
            c = b.coords.get(mdim)
            if c is not None:
                names = [str(v) for v in np.asarray(c.values)]
    else:
        vals = np.asarray(basis)
        if vals.ndim == 1:
            vals = vals[None, :]
        if vals.ndim != 2:
            raise ValueError(f"the basis must be [metabolite, {dim}], got shape {vals.shape}")
        dwell = None
    vals = np.ascontiguousarray(vals, dtype=np.complex128)
    if names is None:
        names = [f"m{k}" for k in range(vals.shape[0])]
    names = [str(v) for v in names]
    if len(names) != vals.shape[0]:
        raise ValueError(f"names must hold one name per metabolite ({vals.shape[0]}), got {len(names)}")
    return vals, dwell, names


def _same_dwell(a, b):
    return abs(a - b) <= 1e-9 * abs(a)


def _run_fit(src, axis, basis, group, init, lo, hi, fixed, dt, skip, max_iter, want_fit):
    """The launch: data and basis to the device, ``device.basis_fit``, every output back as numpy."""
    import torch

    x = src.data if src.is_device_resident else torch.from_numpy(np.ascontiguousarray(src.data))
    if not x.is_complex():
        x = x.to(torch.complex128 if x.dtype == torch.float64 else torch.complex64)
    x = x.to("cuda")
    res = dev.basis_fit(x, axis, torch.from_numpy(basis).to(x.device), group, init, lo, hi, fixed, dt=dt, skip=skip,
                        max_iter=max_iter, want_fit=want_fit)
    out = {k: getattr(res, k).cpu().numpy() for k in ("params", "amp_sd", "rss", "status", "iters")}
    out["fit"] = res.fit.cpu().numpy() if want_fit else None
    out["n_free"] = res.n_free
    return out


def fit_basis(da, basis, dim: str = "time", names=None, groups=None, lineshape: str = "voigt", max_shift: float = 10.0,
              max_broadening: float = 20.0, broadening_start: float = 2.0, max_gaussian: float = 20.0,
              gaussian_start: float = 2.0, fit_phase: bool = True, skip: int = 0, amplitude_start=None,
              max_iter: int = 200, return_fit: bool = True):
    """Fit every FID along `dim` as a combination of the FIDs of `basis` ([metabolite, `dim`]; a labelled basis must
    carry the coordinate `dim` with the data's dwell time, a plain array is taken to be on the data's grid; points past
    the data's length are cut).  `groups`: None (one shift / broadening for all), "each", or M labels.  Widths are in Hz:
    `max_shift`, the Lorentzian FWHM `max_broadening` / `broadening_start`, the Gaussian FWHM `max_gaussian` /
    `gaussian_start` (``lineshape="voigt"`` only).  `skip`: leading points left out of the cost.  `amplitude_start`:
    M values for every voxel instead of the automatic start ||x|| / (M ||B_m||).

    Returns a LabeledDataset (an ``xarray.Dataset`` for DataArray input): amplitude, crlb [%], snr over (voxel dims...,
    "metabolite"); shift [Hz], linewidth [Hz], gaussian [Hz] over (voxel dims..., "group"); phase [deg, wrapped into
    (-180, 180]], rss, status (0 converged, 1 iteration cap, 2 non-finite data: zeros), iters per voxel; with
    `return_fit` also fit_data, residuals and raw_data in the input's dims.  attrs: n_free_parameters, lineshape, skip."""
    src = as_labeled(da)
    if dim not in src.dims:
        raise ValueError(f"Dimension '{dim}' missing in DataArray.")
    axis = src.get_axis_num(dim)
    n = src.shape[axis]
    dt = _dwell(src.coords.get(dim), "fit_basis", dim)
    if not (dt > 0 and np.isfinite(dt)):
        raise ValueError(f"the coordinate '{dim}' must increase, got a dwell time of {dt}")
    bvals, bdt, names = _basis_array(basis, dim, names)
    if bdt is not None and not _same_dwell(dt, bdt):
        raise ValueError(f"the basis' dwell time ({bdt!r} s) differs from the data's ({dt!r} s): resample the basis")
    if bvals.shape[1] < n:
        raise ValueError(f"the basis has {bvals.shape[1]} points along '{dim}', fewer than the data's {n}")
    bvals = np.ascontiguousarray(bvals[:, :n])
    if not np.all(np.isfinite(bvals.real) & np.isfinite(bvals.imag)):
        raise ValueError("the basis has a non-finite sample")
    m = bvals.shape[0]
    group, glabels = parse_groups(groups, names)
    g = len(glabels)
    init, lo, hi, fixed = basis_parameters(m, g, lineshape, max_shift, max_broadening, broadening_start, max_gaussian,
                                           gaussian_start, fit_phase, amplitude_start)
    n_free = int(np.count_nonzero(~fixed))
    skip = int(skip)
    if n_free > MAX_FREE:
        raise ValueError(f"{n_free} free parameters ({m} metabolites, {g} groups, {lineshape}): at most {MAX_FREE}")
    if skip < 0 or n - skip < n_free:
        raise ValueError(f"skip={skip} leaves {n - skip} of {n} points for {n_free} free parameters")
    if max_iter < 1:
        raise ValueError(f"max_iter must be at least 1, got {max_iter}")

    res = _run_fit(src, axis, bvals, group, init, lo, hi, fixed, dt, skip, int(max_iter), bool(return_fit))

    params = res["params"]
    failed = res["status"] == 2
    rss = np.where(failed, 0.0, res["rss"])
    sigma = np.sqrt(rss / (2 * (n - skip) - res["n_free"]))[..., None]
    amp = params[..., :m]
    with np.errstate(divide="ignore", invalid="ignore"):
        asd = res["amp_sd"]
        crlb = np.where(amp != 0, 100.0 * asd * sigma / np.abs(amp), 0.0)
        crlb = np.where(np.isnan(asd), np.nan, crlb)  # singular J^T J: the bound is undefined, whatever the amplitude
        snr = np.where(sigma > 0, amp / sigma, 0.0)
    phase = np.rad2deg(params[..., -1])
    phase = -((-phase + 180.0) % 360.0 - 180.0)  # into (-180, 180]
    metab = {"amplitude": amp, "crlb": crlb, "snr": snr}
    grp = {"shift": params[..., m:m + g], "linewidth": params[..., m + g:m + 2 * g] / np.pi,
           "gaussian": gaussian_fwhm(params[..., m + 2 * g:m + 3 * g])}
    for d in (metab, grp):
        for k in d:
            d[k] = np.where(failed[..., None], 0.0, d[k])
    voxel = {"phase": np.where(failed, 0.0, phase), "rss": res["rss"], "status": res["status"], "iters": res["iters"]}

    other = tuple(d for d in src.dims if d != dim)
    vcoords = {k: c.copy() for k, c in src.coords.items() if c.dim in other}
    mcoords = dict(vcoords, metabolite=Coordinate("metabolite", np.array(names)))
    gcoords = dict(vcoords, group=Coordinate("group", np.array([str(v) for v in glabels])))
    data_vars = {}
    if return_fit:
        order = [other.index(d) if d != dim else len(other) for d in src.dims]  # (other..., dim) -> the input's order
        fit = np.transpose(res["fit"], order)
        raw = np.array(src.values)
        coords = {k: c.copy() for k, c in src.coords.items()}
        data_vars["raw_data"] = LabeledArray(raw, src.dims, coords)
        data_vars["fit_data"] = LabeledArray(fit, src.dims, coords)
        data_vars["residuals"] = LabeledArray(raw - fit, src.dims, coords)
    for k in METAB_VARS:
        data_vars[k] = LabeledArray(metab[k], other + ("metabolite",), mcoords)
    for k in GROUP_VARS:
        data_vars[k] = LabeledArray(grp[k], other + ("group",), gcoords)
    for k in VOXEL_VARS:
        data_vars[k] = LabeledArray(np.asarray(voxel[k]), other, vcoords)
    attrs = _copy.copy(src.attrs)
    attrs.update({"n_free_parameters": res["n_free"], "lineshape": lineshape, "skip": skip})
    ds = LabeledDataset(data_vars, attrs)
    return ds.to_xarray() if is_xarray(da) else ds


def _plain(v):
    if isinstance(v, LabeledArray):
        return np.asarray(v.values)
    return np.asarray(v.values if is_xarray(v) else v)


def basis_model(amplitude, shift, linewidth, gaussian, phase, basis, groups=None, names=None, dim: str = "time",
                dwell: float | None = None):
    """The forward model of ``fit_basis`` on the GPU (``xm_basis_model``), in the units ``fit_basis`` reports:
    `amplitude` [..., M], `shift` [Hz], `linewidth` [Hz] and `gaussian` [Hz] each [..., G], `phase` [deg] [...];
    `basis` and `groups` as in ``fit_basis``.  The dwell time comes from the basis' coordinate `dim`, or from `dwell`.
    Returns complex128 FIDs [..., n_basis]: a LabeledArray over (the dims of `amplitude` but its last, `dim`) when
    `amplitude` is labelled, else an ndarray."""
    import torch

    bvals, bdt, names = _basis_array(basis, dim, names)
    if dwell is None:
        if bdt is None:
            raise ValueError("basis_model needs `dwell` when the basis carries no time coordinate")
        dwell = bdt
    m, n = bvals.shape
    group, glabels = parse_groups(groups, names)
    g = len(glabels)
    a, f, w, gw, ph = (np.asarray(_plain(v), dtype=np.float64) for v in (amplitude, shift, linewidth, gaussian, phase))
    lead = a.shape[:-1]
    if a.shape[-1:] != (m,) or any(v.shape != lead + (g,) for v in (f, w, gw)) or ph.shape != lead:
        raise ValueError(f"basis_model needs amplitude [..., {m}], shift / linewidth / gaussian [..., {g}] and phase "
                         f"[...] with equal leading shapes")
    params = np.concatenate([a, f, w * np.pi, gaussian_damping(gw), np.deg2rad(ph)[..., None]], axis=-1)
    out = dev.basis_model(torch.from_numpy(np.ascontiguousarray(params)).to("cuda"),
                          torch.from_numpy(bvals).to("cuda"), group, float(dwell)).cpu().numpy()
    src = as_labeled(amplitude) if isinstance(amplitude, LabeledArray) or is_xarray(amplitude) else None
    if src is None:
        return out
    other = tuple(src.dims[:-1])
    coords = {k: c.copy() for k, c in src.coords.items() if c.dim in other}
    coords[dim] = Coordinate(dim, np.arange(n) * float(dwell), {"units": "s", "long_name": "Time"})
    res = LabeledArray(out, other + (dim,), coords)
    return res.to_xarray() if is_xarray(amplitude) else res
