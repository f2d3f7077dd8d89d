"""``fit_amares``: AMARES quantification of every FID of an N-dimensional array in one GPU launch.

Host-side mirror of the reference's ``src/xmris/fitting/amares.py:207-488`` (signature, defaults, error texts, result
variables, dims and attrs).  The estimator is this backend's own, stated in DESIGN.md ("Quantification: AMARES"):
Levenberg-Marquardt in lmfit's bound variables with the analytic Jacobian, one workgroup per voxel (``xm_amares_fit``).
"""
from __future__ import annotations

import copy as _copy

import numpy as np

from .. import device as dev
from ..labeled import Coordinate, LabeledArray, as_labeled, is_xarray
from .dataset import LabeledDataset
from .prior_knowledge import read_prior_knowledge

METHODS = ("leastsq", "least_squares")
PARAM_VARS = ("amplitude", "chem_shift", "linewidth", "phase", "crlb", "snr")


def fit_amares(da, prior_knowledge_file, dim: str = "time", mhz: float | None = None, sw: float | None = None,
               deadtime: float | None = None, method: str = "leastsq", initialize_with_lm: bool = True,
               num_workers: int = 4, init_fid=None, verbose: bool = False):
    """Fit every FID along `dim` with the prior knowledge of `prior_knowledge_file` (CSV).  Returns a LabeledDataset
    (an ``xarray.Dataset`` for DataArray input) with raw_data, fit_data, residuals (the input's dims) and amplitude,
    chem_shift [ppm], linewidth [Hz], phase [deg], crlb [%], snr (other dims..., "Metabolite").  Linked prior knowledge
    (fitting/prior_knowledge.py) needs no keyword: every CSV column stays one "Metabolite" entry, and attrs
    ["n_free_parameters"] counts the free columns of the fit (a group of linked parameters is one).
    `initialize_with_lm`, `num_workers` and `init_fid` are accepted for compatibility and do not change the result:
    every voxel starts from the prior knowledge's initial values."""
    src = as_labeled(da)
    if dim not in src.dims:
        raise ValueError(f"Dimension '{dim}' missing in DataArray.")
    if mhz is None:
        mhz = src.attrs.get("MHz")
        if mhz is None:
            raise ValueError("mhz must be provided or present in da.attrs['MHz']")
    if method not in METHODS:
        raise ValueError(f"method must be one of {METHODS}, got {method!r}")
    axis = src.get_axis_num(dim)
    n = src.shape[axis]
    coord = src.coords.get(dim)
    if sw is None or deadtime is None:
        if coord is None or len(coord.values) < 2:
            raise ValueError(f"sw and deadtime default to the coordinate '{dim}', which is missing or too short")
        tv = np.asarray(coord.values, dtype=np.float64)
        if sw is None:
            sw = 1.0 / float(tv[1] - tv[0])
        if deadtime is None:
            deadtime = float(tv[0])
    if init_fid is not None and np.asarray(init_fid).shape != (n,):
        raise ValueError(f"init_fid must be one FID of {n} points, got shape {np.asarray(init_fid).shape}")
    pk = read_prior_knowledge(prior_knowledge_file)
    init, lo, hi = pk.fitting_units(mhz)

    import torch

    x = src.data if src.is_device_resident else torch.from_numpy(np.ascontiguousarray(src.data))
    if not x.is_complex():
        x = x.to(torch.complex128 if x.dtype == torch.float64 else torch.complex64)
    x = x.to("cuda")
    res = dev.amares_fit(x, axis, init, lo, hi, pk.fixed, dt=1.0 / float(sw), t0=float(deadtime),
                         links=pk.fitting_links(mhz))

    params = res.params.cpu().numpy()
    failed = res.status.cpu().numpy() == 2
    rss = np.where(failed, 0.0, res.rss.cpu().numpy())
    sigma = np.sqrt(rss / (2 * n - res.n_free))[..., None]
    amp = params[..., 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        asd = res.amp_sd.cpu().numpy()
        crlb = np.where(amp != 0, 100.0 * asd * sigma / np.abs(amp), 0.0)
        crlb = np.where(np.isnan(asd), np.nan, crlb)  # singular J^T J: the bound is undefined, whatever the amplitude
        snr = np.where(sigma > 0, amp / sigma, 0.0)
    values = {"amplitude": amp, "chem_shift": params[..., 1] / mhz, "linewidth": params[..., 2] / np.pi,
              "phase": np.rad2deg(params[..., 3]), "crlb": crlb, "snr": snr}
    for k in values:
        values[k] = np.where(failed[..., None], 0.0, values[k])

    other = tuple(d for d in src.dims if d != dim)
    order = [other.index(d) if d != dim else len(other) for d in src.dims]  # (other..., dim) -> the input's order
    fit = np.transpose(res.fit.cpu().numpy(), order)
    raw = np.asarray(src.values)
    residuals = raw - fit

    coords = {k: c.copy() for k, c in src.coords.items()}
    pcoords = {k: c.copy() for k, c in src.coords.items() if c.dim in other}
    pcoords["Metabolite"] = Coordinate("Metabolite", np.array(pk.names))
    data_vars = {
        "raw_data": LabeledArray(raw, src.dims, coords),
        "fit_data": LabeledArray(fit, src.dims, coords),
        "residuals": LabeledArray(residuals, src.dims, coords),
    }
    for k in PARAM_VARS:
        data_vars[k] = LabeledArray(values[k], other + ("Metabolite",), pcoords)
    from .. import __version__

    attrs = _copy.copy(src.attrs)
    attrs.update({"fit_method": method, "prior_knowledge_file": str(prior_knowledge_file),
                  "amares_version": f"xmris_amd {__version__}", "n_free_parameters": res.n_free})
    ds = LabeledDataset(data_vars, attrs)
    return ds.to_xarray() if is_xarray(da) else ds
