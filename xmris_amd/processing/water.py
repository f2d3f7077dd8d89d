"""``remove_water``: per-voxel removal of the residual water signal from 1H FIDs on the GPU by HSVD (Hankel SVD;
Barkhuijsen 1987, Pijnappel 1992; "HLSVD" in jMRUI), the step between ``align_averages`` and the fit.

The definition is this backend's own (the reference has no such function).  For every FID x[t],
t < N: H[l, j] = x[l + j] with M = `n_cols` columns, G = H^H H; W = conj(U), U the eigenvectors of G's K = `rank` largest
eigenvalues; Q the least-squares solution of W[:-1] Q = W[1:]; z_k = eig(Q), f_k = arg z_k / (2 pi dt),
d_k = -ln|z_k| / dt; a the least-squares amplitudes of sum_k a_k z_k^t over all N points; y = x minus the components with
band[0] <= f_k <= band[1].  One launch of ``xm_hsvd_rows`` does all voxels.
"""
from __future__ import annotations

import copy as _copy

import numpy as np

from .. import device as dev
from ..config import ATTRS, DIMS
from ..labeled import LabeledArray, as_labeled, is_xarray, like_input
from ._common import device_data

COMPONENT_DIM = "component"


def _time_step(src, dim: str) -> float:
    """dt of a uniform time coordinate; ValueError when it is missing or not uniform (to 1e-9 of dt)."""
    if dim not in src.coords:
        raise ValueError(f"dt: {dim!r} has no coordinate; give dt (seconds) or a time coordinate")
    t = np.asarray(src.coords[dim].values, dtype=np.float64)
    if t.size < 2:
        raise ValueError(f"dt: the coordinate of {dim!r} has fewer than two points")
    dt = float(t[-1] - t[0]) / (t.size - 1)
    if not (np.all(np.isfinite(t)) and dt > 0 and np.all(np.abs(t - (t[0] + np.arange(t.size) * dt)) <= 1e-9 * dt * t.size)):
        raise ValueError(f"dt: the coordinate of {dim!r} must be uniform and increasing (or give dt)")
    return dt


def remove_water(da, dim: str = DIMS.time, band=(-50.0, 50.0), rank: int = 20, n_cols: int = 64, dt: float = None,
                 return_components: bool = False):
    """Remove from every FID along `dim` the HSVD components whose frequency lies in `band` = (f_lo, f_hi) Hz (the
    frequency coordinate of ``to_spectrum``: e^{+2 pi i f t} shows up at +f).  `rank`: the number K of damped
    exponentials of the model, 1 ... min(n_cols - 1, 32); `n_cols`: the columns M of the Hankel matrix, 2 ... 64; the
    FID needs 2 M ... 16384 points.  `dt`: the sample spacing in seconds, else taken from the coordinate of `dim`, which
    must then be uniform.  Returns the input without those components (dims, coords and attrs kept, plus attrs
    ``water_band``, ``water_rank``, ``water_n_cols``), device-resident; with `return_components` a dataset of
    ``cleaned``, and along a new ``component`` dim (sorted by frequency) ``frequency`` (Hz), ``damping`` (1/s),
    ``amplitude``, ``phase`` (rad) and ``removed`` (0 / 1), plus per voxel ``n_removed`` and ``status`` (0 done, 1 nothing
    in the band or an all-zero FID: unchanged, 2 non-finite sample: zeros, 3 iteration cap: unchanged, 4 degenerate
    poles or amplitudes: unchanged).  A `dim` that is not last costs one contiguous copy."""
    src = as_labeled(da)
    if dim not in src.dims:
        raise ValueError(f"dim: dimension {dim!r} missing in the array (dims {src.dims})")
    if not np.issubdtype(src.dtype, np.complexfloating):
        raise ValueError(f"remove_water needs complex FIDs, got dtype {src.dtype}")
    try:
        f_lo, f_hi = (float(b) for b in band)
    except (TypeError, ValueError):
        raise ValueError(f"band must be a pair (f_lo, f_hi) in Hz, got {band!r}") from None
    if not (np.isfinite(f_lo) and np.isfinite(f_hi) and f_lo <= f_hi):
        raise ValueError(f"band must be finite with f_lo <= f_hi, got {band!r}")
    if int(n_cols) != n_cols or not 2 <= n_cols <= dev.HSVD_MAX_COLS:
        raise ValueError(f"n_cols must be an integer in 2 ... {dev.HSVD_MAX_COLS}, got {n_cols!r}")
    top = min(int(n_cols) - 1, dev.HSVD_MAX_RANK)
    if int(rank) != rank or not 1 <= rank <= top:
        raise ValueError(f"rank must be an integer in 1 ... {top} (min(n_cols - 1, {dev.HSVD_MAX_RANK})), got {rank!r}")
    ta = src.get_axis_num(dim)
    n = src.shape[ta]
    if not 2 * int(n_cols) <= n <= dev.HSVD_MAX_POINTS:
        raise ValueError(f"dim / n_cols: {dim!r} has {n} points; needs 2 * n_cols = {2 * int(n_cols)} ... "
                         f"{dev.HSVD_MAX_POINTS}")
    if dt is None:
        dt = _time_step(src, dim)
    elif not (np.isfinite(dt) and dt > 0):
        raise ValueError(f"dt must be finite and positive, got {dt!r}")

    x, _ = device_data(src)
    res = dev.hsvd_rows(x, ta, int(n_cols), int(rank), float(dt), (f_lo, f_hi))
    y = res.y
    if ta != src.ndim - 1:
        import torch

        y = torch.movedim(y, -1, ta).contiguous()
    attrs = _copy.copy(src.attrs)
    attrs[ATTRS.water_band] = (f_lo, f_hi)
    attrs[ATTRS.water_rank] = int(rank)
    attrs[ATTRS.water_n_cols] = int(n_cols)
    out = LabeledArray(y, tuple(src.dims), dict(src.coords), attrs, src.name)
    if not return_components:
        return like_input(out, da)
    from ..fitting.dataset import LabeledDataset

    vox = tuple(d for d in src.dims if d != dim)
    vcoords = {k: c_ for k, c_ in src.coords.items() if c_.dim in vox}
    ds = {"cleaned": out}
    for name in ("frequency", "damping", "amplitude", "phase", "removed"):
        ds[name] = LabeledArray(getattr(res, name), vox + (COMPONENT_DIM,), vcoords)
    ds["n_removed"] = LabeledArray(res.n_removed, vox, vcoords)
    ds["status"] = LabeledArray(res.status, vox, vcoords)
    ds = LabeledDataset(ds, attrs)
    return ds.to_xarray() if is_xarray(da) else ds
