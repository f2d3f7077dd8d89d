"""``align_averages``: per-transient frequency and phase correction of repeated acquisitions on the GPU (time-domain
spectral registration, Near et al. 2015), the step between ``combine_coils`` and the single-channel chain.

The definition is this backend's own (the reference has no such function).  For a transient x
and its voxel's reference r over the L leading points, tau_t = t0 + t dt: z = r conj(x), C(f) = sum_t z_t
e^{-2 pi i f tau_t}; f* maximises |C|^2 within +-max_shift (a coarse grid of spacing 1 / (4 L dt), then a safeguarded
Newton iteration), phi* = arg C(f*), y_t = x_t e^{i (2 pi f* tau_t + phi*)} -- the least-squares registration with unit
amplitude.  One launch of ``xm_align_rows`` does all transients.
"""
from __future__ import annotations

import copy as _copy

import numpy as np

from .. import device as dev
from ..config import ATTRS, DIMS
from ..dims import _check_dims
from ..labeled import LabeledArray, as_labeled, is_xarray, like_input
from ._common import device_data


def _uniform_time(src, time_dim: str):
    """(t0, dt) of a uniform time coordinate; ValueError when it is missing or not uniform (to 1e-9 of dt)."""
    if time_dim not in src.coords:
        raise ValueError(f"time_dim: {time_dim!r} has no coordinate; the alignment needs the sample times in seconds")
    t = np.asarray(src.coords[time_dim].values, dtype=np.float64)
    if t.size < 2:
        return (float(t[0]) if t.size else 0.0), 1.0
    dt = float(t[-1] - t[0]) / (t.size - 1)
    if not (np.all(np.isfinite(t)) and dt > 0 and np.all(np.abs(t - (t[0] + np.arange(t.size) * dt)) <= 1e-9 * dt * t.size)):
        raise ValueError(f"time_dim: the coordinate of {time_dim!r} must be uniform and increasing")
    return float(t[0]), dt


def align_averages(da, dim: str = DIMS.average, time_dim: str = DIMS.time, reference="mean", max_shift: float = 20.0,
                   t_max: float = None, n_points: int = None, passes: int = 1, average: bool = False,
                   min_quality: float = 0.0, return_shifts: bool = False):
    """Align every transient along `dim` to its voxel's reference by a frequency shift (|shift| <= `max_shift` Hz) and
    a phase.  `reference`: ``"mean"`` (the per-voxel mean over `dim` of the unaligned data), ``"first"`` or an index
    along `dim`, or an array with the data's dims without `dim` (or 1-D along `time_dim`), which may be shorter than
    the data.  The fit uses the leading `n_points` points, else those with time <= `t_max`, else all.  `passes` > 1
    (``"mean"`` only): every further pass aligns the original data to the mean of the previous pass's result.
    Returns the input aligned (`dim` kept), or with `average` the per-voxel mean of the aligned transients whose
    quality is at least `min_quality` (`dim` dropped); other dims, coords and attrs kept, plus attrs ``align_dim``,
    ``align_reference``, ``align_max_shift``; device-resident.  With `return_shifts` a dataset of ``aligned`` (or
    ``averaged``), ``shift`` (Hz, what was applied: a transient lying +d Hz from the reference gets -d), ``phase``
    (degrees), ``quality``, ``status`` (0 aligned, 1 window edge, 2 non-finite sample, 3 nothing to go by, 4 step cap)
    and with `average` ``n_averaged``."""
    src = as_labeled(da)
    _check_dims(src, (dim, time_dim), "align_averages")
    if dim == time_dim:
        raise ValueError("dim and time_dim must differ")
    if not np.issubdtype(src.dtype, np.complexfloating):
        raise ValueError(f"align_averages needs complex FIDs, got dtype {src.dtype}")
    t0, dt = _uniform_time(src, time_dim)
    aa, ta = src.get_axis_num(dim), src.get_axis_num(time_dim)
    n = src.shape[ta]
    if n < 1 or src.shape[aa] < 1:
        raise ValueError(f"dim / time_dim: {dim!r} and {time_dim!r} must have at least one point")
    if not (np.isfinite(max_shift) and max_shift >= 0):
        raise ValueError(f"max_shift must be finite and not negative, got {max_shift!r}")
    if int(passes) != passes or passes < 1:
        raise ValueError(f"passes must be a positive integer, got {passes!r}")
    other = tuple(d for d in src.dims if d != dim)
    vox = tuple(d for d in other if d != time_dim)

    ref_arr, ref_name, n_ref = None, reference, n
    if isinstance(reference, str):
        if reference not in ("mean", "first"):
            raise ValueError(f"reference must be 'mean', 'first', an index along {dim!r} or an array, got {reference!r}")
    elif isinstance(reference, (int, np.integer)):
        if not -src.shape[aa] <= reference < src.shape[aa]:
            raise ValueError(f"reference: index {reference} out of range for {dim!r} of size {src.shape[aa]}")
        ref_name = int(reference)
    else:
        ref_arr, ref_name = as_labeled(reference), "array"
        ok = time_dim in ref_arr.dims and dim not in ref_arr.dims and (
            ref_arr.dims == (time_dim,) or
            (set(ref_arr.dims) == set(other) and all(ref_arr.sizes[d] == src.sizes[d] for d in vox)))
        if not ok:
            raise ValueError(f"reference: dims / sizes {ref_arr.sizes} must be the data's {src.sizes} without {dim!r} "
                             f"(any length along {time_dim!r}), or 1-D along {time_dim!r}")
        n_ref = ref_arr.sizes[time_dim]
    if passes > 1 and ref_name != "mean":
        raise ValueError("passes > 1 needs reference='mean'")

    if n_points is not None:
        if int(n_points) != n_points or not 1 <= n_points <= min(n, n_ref):
            raise ValueError(f"n_points must be in 1 ... {min(n, n_ref)}, got {n_points!r}")
        length = int(n_points)
    elif t_max is not None:
        length = int(np.count_nonzero(t0 + np.arange(n) * dt <= t_max))
        if not 1 <= length <= n_ref:
            raise ValueError(f"t_max: {length} points have time <= {t_max!r}; needs 1 ... {n_ref}")
    else:
        length = min(n, n_ref)
    _, g = dev.align_grid(length, dt, float(max_shift))
    if length > dev.ALIGN_MAX_POINTS:
        raise ValueError(f"t_max / n_points: the fit would use {length} points, at most {dev.ALIGN_MAX_POINTS} are "
                         "supported; give t_max or n_points")
    if 2 * g + 1 > dev.ALIGN_MAX_GRID:
        raise ValueError(f"max_shift / t_max: the coarse grid of {2 * g + 1} points (spacing 1 / (4 L dt)) exceeds "
                         f"{dev.ALIGN_MAX_GRID}; lower max_shift or shorten the fit with t_max / n_points")

    x, _ = device_data(src)
    if ref_arr is not None:
        r, _ = device_data(ref_arr)
        r = r.to(x.dtype)
        if ref_arr.ndim > 1:  # the data's order of dims
            r = r.permute(*[ref_arr.dims.index(d) for d in other])
    elif reference == "mean":
        r = x.mean(dim=aa)
    else:
        r = x.select(aa, 0 if reference == "first" else int(reference))

    def launch(ref, last):  # `ref`: 1-D, or the data's axes without `dim` in the data's order
        return dev.align_rows(x, aa, ta, ref, n_points=length, dt=dt, t0=t0, max_shift=float(max_shift),
                              average=average and last, min_quality=float(min_quality), want_y=not (average and last))

    res = launch(r, passes == 1)
    for k in range(1, int(passes)):
        nxt = res.y.mean(dim=aa if aa < ta else aa - 1)  # res.y has time last
        if ta != src.ndim - 1:
            import torch

            nxt = torch.movedim(nxt, -1, other.index(time_dim))
        res = launch(nxt, k == passes - 1)

    attrs = _copy.copy(src.attrs)
    attrs[ATTRS.align_dim] = str(dim)
    attrs[ATTRS.align_reference] = ref_name
    attrs[ATTRS.align_max_shift] = float(max_shift)

    def back(t, dims_now):  # time from last to where the input has it
        want = dims_now.index(time_dim)
        if want == len(dims_now) - 1:
            return t
        import torch

        return torch.movedim(t, -1, want).contiguous()

    if average:
        coords = {k: c_ for k, c_ in src.coords.items() if c_.dim != dim}
        out = LabeledArray(back(res.mean, other), other, coords, attrs, src.name)
    else:
        out = LabeledArray(back(res.y, tuple(src.dims)), tuple(src.dims), dict(src.coords), attrs, src.name)
    if not return_shifts:
        return like_input(out, da)
    from ..fitting.dataset import LabeledDataset

    per = tuple(d for d in src.dims if d != time_dim)
    pcoords = {k: c_ for k, c_ in src.coords.items() if c_.dim in per}
    ds = {"averaged" if average else "aligned": out,
          "shift": LabeledArray(res.shift, per, pcoords),
          "phase": LabeledArray(res.phase * (180.0 / np.pi), per, pcoords),
          "quality": LabeledArray(res.quality, per, pcoords),
          "status": LabeledArray(res.status, per, pcoords)}
    if average:
        ds["n_averaged"] = LabeledArray(res.n_averaged, vox, {k: c_ for k, c_ in src.coords.items() if c_.dim in vox})
    ds = LabeledDataset(ds, attrs)
    return ds.to_xarray() if is_xarray(da) else ds
