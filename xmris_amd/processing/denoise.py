"""``denoise_mppca``: Marchenko-Pastur patch PCA denoising of MRSI FIDs on the GPU (Veraart et al. 2016), the step
between ``align_averages`` / ``remove_water`` and the fit.

The definition is this backend's own (the reference has no such function).  Every voxel gets the
full window of `patch` voxels around it along `dims` (shifted inward at an edge); X is the P x N matrix of the window's
FIDs, G = X X^H, lambda_k = max(eig_k, 0) / N descending with eigenvectors U.  The rank r is given, or the first p with
(lambda_p - lambda_{P-1}) / (4 sqrt((P - p) / N)) < mean(lambda_p ... lambda_{P-1}).  The voxel's own row of the projection
onto the top-r subspace is its output; sigma = sqrt(mean(lambda_r ... lambda_{P-1})) is its noise level.  One launch of
``xm_denoise_patches`` does all voxels.
"""
from __future__ import annotations

import copy as _copy

import numpy as np

from .. import device as dev
from ..config import ATTRS, DIMS
from ..labeled import LabeledArray, as_labeled, is_xarray, like_input
from ._common import device_data


def denoise_mppca(da, dims, patch, time_dim: str = DIMS.time, rank=None, return_noise: bool = False):
    """Denoise every FID along `time_dim` by the PCA of its spatial neighbourhood.  `dims`: one name or 1 ... 3 names
    of the dimensions the patch extends over (spatial dims, or e.g. ``"repetition"``); every other dim is batch.
    `patch`: the patch size along each, an int for all or one per dim, 1 ... the dim's size; the patch holds
    P = 2 ... 64 voxels and the FID needs P ... 16384 points.  `rank`: the number of components kept, 0 ... P, or None
    for the Marchenko-Pastur rule (no tuning parameter).  Returns the denoised array (dims, coords and attrs kept, plus
    attrs ``denoise_dims``, ``denoise_patch``, ``denoise_rank``), device-resident; with `return_noise` a dataset of
    ``denoised`` and per voxel ``sigma`` (the standard deviation of the complex noise; real and imaginary parts
    sqrt(1/2) of it each), ``rank`` and ``status`` (0 done, 1 all-zero window: zeros, 2 non-finite sample in the
    window: zeros, 3 iteration cap: unchanged).  Patch dims that are not adjacent and right in front of a last time dim
    cost one contiguous copy."""
    src = as_labeled(da)
    names = (dims,) if isinstance(dims, str) else tuple(dims)
    if time_dim not in src.dims:
        raise ValueError(f"time_dim: dimension {time_dim!r} missing in the array (dims {src.dims})")
    if not 1 <= len(names) <= 3:
        raise ValueError(f"dims: needs 1 ... 3 dimensions, got {len(names)}")
    for d in names:
        if d not in src.dims:
            raise ValueError(f"dims: dimension {d!r} missing in the array (dims {src.dims})")
        if d == time_dim:
            raise ValueError(f"dims: {d!r} is the time dimension")
    if len(set(names)) != len(names):
        raise ValueError(f"dims: a dimension is repeated in {names}")
    if not np.issubdtype(src.dtype, np.complexfloating):
        raise ValueError(f"da: denoise_mppca needs complex FIDs, got dtype {src.dtype}")
    try:
        raw = (patch,) * len(names) if np.ndim(patch) == 0 else tuple(patch)
        sizes = tuple(int(p) for p in raw)
        if any(s_ != p for s_, p in zip(sizes, raw)):
            raise ValueError
    except (TypeError, ValueError):
        raise ValueError(f"patch must be an integer or one integer per dim, got {patch!r}") from None
    if len(sizes) != len(names):
        raise ValueError(f"patch: {len(sizes)} sizes for {len(names)} dims")
    axes = [src.get_axis_num(d) for d in names]
    for d, a, p in zip(names, axes, sizes):
        if not 1 <= p <= src.shape[a]:
            raise ValueError(f"patch: size {p} along {d!r}, which has {src.shape[a]} points; needs 1 ... {src.shape[a]}")
    big_p = int(np.prod(sizes))
    if not 2 <= big_p <= dev.DENOISE_MAX_PATCH:
        raise ValueError(f"patch: {sizes} holds {big_p} voxels, supported are 2 ... {dev.DENOISE_MAX_PATCH}")
    ta = src.get_axis_num(time_dim)
    n = src.shape[ta]
    if not big_p <= n <= dev.DENOISE_MAX_POINTS:
        raise ValueError(f"time_dim / patch: {time_dim!r} has {n} points; needs the patch's {big_p} ... "
                         f"{dev.DENOISE_MAX_POINTS}")
    if rank is not None and (isinstance(rank, bool) or int(rank) != rank or not 0 <= rank <= big_p):
        raise ValueError(f"rank must be None or an integer in 0 ... {big_p} (the patch's voxels), got {rank!r}")

    x, _ = device_data(src)
    res = dev.denoise_patches(x, axes, ta, sizes, rank=None if rank is None else int(rank))
    attrs = _copy.copy(src.attrs)
    attrs[ATTRS.denoise_dims] = tuple(str(d) for d in names)
    attrs[ATTRS.denoise_patch] = sizes
    attrs[ATTRS.denoise_rank] = "mp" if rank is None else int(rank)
    y = res.y if res.y.is_contiguous() else res.y.contiguous()
    out = LabeledArray(y, tuple(src.dims), dict(src.coords), attrs, src.name)
    if not return_noise:
        return like_input(out, da)
    from ..fitting.dataset import LabeledDataset

    vox = tuple(d for d in src.dims if d != time_dim)
    vcoords = {k: c_ for k, c_ in src.coords.items() if c_.dim in vox}
    ds = {"denoised": out}
    for name in ("sigma", "rank", "status"):
        ds[name] = LabeledArray(getattr(res, name).contiguous(), vox, vcoords)
    ds = LabeledDataset(ds, attrs)
    return ds.to_xarray() if is_xarray(da) else ds
