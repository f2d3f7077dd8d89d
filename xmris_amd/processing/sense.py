"""``unfold_sense``: SENSE unfolding of regularly undersampled phased-array MRSI on the GPU (Pruessmann et al. 1999;
SENSE-MRSI, Dydak et al. 2001), the step between ``to_image`` and the single-channel chain (``align_averages``,
``remove_water``, ``denoise_mppca``, the fits).  ``sense_maps``: relative coil sensitivities from a fully sampled
reference image.

The definition is this backend's own (the reference has no such function).  Per undersampled dim
with n acquired lines and acceleration R, N = R n: the acquisition keeps the lines N // 2 + R (l - n // 2), l = 0 ... n - 1,
of the full centred k-space, and ``to_image`` of them (no filter, zero fill or shift) is the aliased image

    a_c[p] = (1 / sqrt(R)) sum_k s_c[q_k(p)] rho[q_k(p)],   q_k(p) = (p - n // 2 + N // 2 + k n) mod N.

For every group of R = prod R_a voxels, with Psi = L L^H the noise covariance (or I) and W = L^-1: S the C x Ra matrix of
the members whose sensitivity is not zero in every coil, Sw = W S, A = Sw^H Sw, lambda' = regularization trace(A) / Ra,
B = (A + lambda' I)^-1 Sw^H by Cholesky, U = sqrt(R) B W; rho[q_k, t] = sum_c U[k, c] a_c[p, t] and
g[q_k] = sqrt((B B^H)_kk A_kk).  One launch of ``xm_sense_unfold`` does all groups.
"""
from __future__ import annotations

import copy as _copy

import numpy as np

from .. import device as dev
from ..config import ATTRS, DIMS
from ..dims import _check_dims
from ..labeled import Coordinate, LabeledArray, as_labeled, is_xarray, like_input
from ._common import device_data, to_host
from .coils import MAX_COILS, _linv, _tail_cov
from .mrsi import _int, _per_dim

MAX_ACCEL = 16


def _noise(noise_cov, c: int):
    """(L^-1 or None, whether the covariance is to be estimated from the tail of the data)."""
    tail = isinstance(noise_cov, str)
    if tail and noise_cov != "tail":
        raise ValueError(f"noise_cov must be a {c} x {c} matrix or 'tail', got {noise_cov!r}")
    return (None if noise_cov is None or tail else _linv(noise_cov, c)), tail


def _sens_values(sensitivities, coil_dim, names, c, full):
    """The sensitivities as an array or tensor of shape (C, *N) in the order (coil_dim, *names)."""
    want = (c, *full)
    if isinstance(sensitivities, LabeledArray) or is_xarray(sensitivities):
        s = as_labeled(sensitivities)
        order = (coil_dim, *names)
        if set(s.dims) != set(order) or len(s.dims) != len(order):
            raise ValueError(f"sensitivities: dims {s.dims} must be {order} in any order")
        vals = s.data
        perm = [s.get_axis_num(d) for d in order]
        vals = vals.permute(perm) if hasattr(vals, "detach") else np.transpose(np.asarray(vals), perm)
    else:
        vals = sensitivities if hasattr(sensitivities, "detach") else np.asarray(sensitivities)
    if tuple(vals.shape) != want:
        raise ValueError(f"sensitivities: shape {tuple(vals.shape)} in the order {(coil_dim, *names)} must be {want}: the "
                         f"coils, then accel x the data's size along each of {names}")
    return vals


def _over_batch(g, status, nb: int):
    """g and status over the spatial dims alone: the highest status over the batch axes, g NaN where any is."""
    if nb == 0:
        return g, status
    lead = tuple(range(nb))
    if hasattr(g, "detach"):
        import torch

        first = g[(0,) * nb]
        return torch.where(torch.isnan(g).any(dim=lead), torch.full_like(first, float("nan")), first), status.amax(dim=lead)
    first = g[(0,) * nb]
    return np.where(np.isnan(g).any(axis=lead), np.nan, first), status.max(axis=lead)


def unfold_sense(da, sensitivities, accel, dims=(DIMS.x, DIMS.y), coil_dim: str = DIMS.coil, time_dim: str = DIMS.time,
                 noise_cov=None, regularization: float = 0.0, return_maps: bool = False):
    """Unfold the aliased images `da` (``to_image`` of a regularly undersampled k-space, without filter, zero fill or
    shift: a spatial filter applied before the unfolding changes the aliasing model) along `dims` (one name or 1 ... 3).
    `accel`: the acceleration, an int for all dims or one per dim, their product at most 16.  `sensitivities`: an array
    with the dims ``(coil_dim, *dims)`` in any order, or array-like in that order, of sizes C and accel x the data's; a
    voxel whose sensitivity is zero in every coil is masked out of the unfolding.  `noise_cov`: a C x C Hermitian
    positive-definite matrix, or ``"tail"`` to estimate it from the end of the FIDs of `da`.  `regularization`: Tikhonov
    weight relative to the mean diagonal of S^H Psi^-1 S.  Returns the input without `coil_dim` and with every dim of
    `dims` grown to accel x its size (coordinate ``(arange(N) - N // 2) dx``, other coordinates along a grown dim
    dropped), attrs kept plus ``sense_dims``, ``sense_accel`` and ``sense_regularization``; device-resident for
    LabeledArray input.  With `return_maps` a dataset of ``unfolded``, ``g_factor`` and ``status`` (over `dims`: 0
    unfolded, 1 masked, 2 non-finite sample in the group, 3 not positive definite; the highest over the other axes)."""
    src = as_labeled(da)
    names = (dims,) if isinstance(dims, str) else tuple(dims)
    _check_dims(src, names, "unfold_sense")
    if not 1 <= len(names) <= 3:
        raise ValueError(f"dims: needs 1 ... 3 dimensions, got {len(names)}")
    if len(set(names)) != len(names):
        raise ValueError(f"dims: a dimension is repeated in {names}")
    for arg, d in (("coil_dim", coil_dim), ("time_dim", time_dim)):
        if d in names:
            raise ValueError(f"{arg}: {d!r} is one of the undersampled dims {names}")
        if d not in src.dims:
            raise ValueError(f"{arg}: dimension {d!r} missing in the array (dims {src.dims})")
    if coil_dim == time_dim:
        raise ValueError("coil_dim and time_dim must differ")
    acc = _per_dim(accel, len(names), "accel", _int)
    if acc is None or any(r < 1 for r in acc):
        raise ValueError(f"accel must be an integer >= 1 or one per dim, got {accel!r}")
    if int(np.prod(acc)) > MAX_ACCEL:
        raise ValueError(f"accel: the total acceleration {int(np.prod(acc))} exceeds {MAX_ACCEL}")
    ca, ta = src.get_axis_num(coil_dim), src.get_axis_num(time_dim)
    axes = [src.get_axis_num(d) for d in names]
    c = src.shape[ca]
    if c < 1 or c > MAX_COILS:
        raise ValueError(f"coil_dim: {c} coils along {coil_dim!r}, supported are 1 ... {MAX_COILS}")
    small = [src.shape[a] for a in axes]
    if src.shape[ta] < 1 or min(small) < 1:
        raise ValueError(f"dims: {names} or time_dim {time_dim!r} holds an empty dimension")
    full = [r * n for r, n in zip(acc, small)]
    try:
        reg = float(regularization)
    except (TypeError, ValueError):
        reg = float("nan")
    if not np.isfinite(reg) or reg < 0.0:
        raise ValueError(f"regularization must be a finite number >= 0, got {regularization!r}")
    sens = _sens_values(sensitivities, coil_dim, names, c, full)
    linv, tail = _noise(noise_cov, c)

    x, _ = device_data(src)
    if tail:
        linv = _linv(_tail_cov(x, ca, ta), c)
    res = dev.unfold_sense(x, sens, ca, axes, ta, acc, linv=linv, regularization=reg)

    other = tuple(d for d in src.dims if d != coil_dim)
    y = res.y
    if other.index(time_dim) != len(other) - 1:
        if hasattr(y, "detach"):
            import torch

            y = torch.movedim(y, -1, other.index(time_dim)).contiguous()
        else:
            y = np.ascontiguousarray(np.moveaxis(y, -1, other.index(time_dim)))
    coords, grid = {}, {}
    for k, co in src.coords.items():
        if co.dim == coil_dim:
            continue
        if co.dim not in names or full[names.index(co.dim)] == len(co.values):
            coords[k] = co
        elif k == co.dim:
            old = np.asarray(co.values)
            dx = (old[1] - old[0]) if len(old) > 1 else 1.0
            m = full[names.index(co.dim)]
            coords[k] = Coordinate(k, (np.arange(m) - m // 2) * dx, co.attrs)
    for k, co in coords.items():
        if co.dim in names:
            grid[k] = co
    attrs = _copy.copy(src.attrs)
    attrs[ATTRS.sense_dims] = tuple(str(d) for d in names)
    attrs[ATTRS.sense_accel] = tuple(acc)
    attrs[ATTRS.sense_regularization] = reg
    out = LabeledArray(y, other, coords, attrs, src.name)
    if not return_maps:
        return like_input(out, da)
    from ..fitting.dataset import LabeledDataset

    g, status = _over_batch(res.g, res.status, len(src.dims) - 2 - len(names))
    ds = LabeledDataset({"unfolded": out, "g_factor": LabeledArray(g, names, grid),
                         "status": LabeledArray(status, names, grid)}, attrs)
    return ds.to_xarray() if is_xarray(da) else ds


def sense_maps(reference, dim: str = DIMS.coil, time_dim: str = DIMS.time, noise_cov=None, threshold: float = 0.05):
    """Relative coil sensitivities from the fully sampled image `reference` (dims: `dim`, `time_dim` and the voxels):
    s = Psi w per voxel, w the weights of ``combine_coils(method="svd")`` (w itself without `noise_cov`), so that
    ``unfold_sense`` at accel 1 gives what ``combine_coils`` gives.  A voxel whose energy, summed over coils and time, is
    below `threshold` x the largest is set to zero in every coil: ``unfold_sense`` masks it.  Returns a host
    LabeledArray (complex128) with the dims ``(dim, *voxel dims)``."""
    src = as_labeled(reference)
    for name, d in (("dim", dim), ("time_dim", time_dim)):
        if d not in src.dims:
            raise ValueError(f"{name}: dimension {d!r} missing in the array (dims {src.dims})")
    if dim == time_dim:
        raise ValueError("dim and time_dim must differ")
    ca, ta = src.get_axis_num(dim), src.get_axis_num(time_dim)
    c = src.shape[ca]
    if c < 1 or c > MAX_COILS:
        raise ValueError(f"dim: {c} coils along {dim!r}, supported are 1 ... {MAX_COILS}")
    if src.shape[ta] < 1:
        raise ValueError(f"time_dim: {time_dim!r} must have at least one point")
    try:
        thr = float(threshold)
    except (TypeError, ValueError):
        thr = float("nan")
    if not 0.0 <= thr <= 1.0:
        raise ValueError(f"threshold must be in 0 ... 1, got {threshold!r}")
    linv, tail = _noise(noise_cov, c)

    x, _ = device_data(src)
    if tail:
        linv = _linv(_tail_cov(x, ca, ta), c)
    res = dev.coil_combine(x, ca, ta, method="svd", linv=linv)
    w = to_host(res.weights)  # [voxels..., C]
    if hasattr(x, "detach"):
        energy = to_host((x.real ** 2 + x.imag ** 2).sum(dim=(ca, ta)).double())
    else:
        energy = (np.abs(x) ** 2).sum(axis=(ca, ta))
    if linv is not None:
        chol = np.linalg.inv(linv)
        w = w @ (chol @ chol.conj().T).T  # s_c = sum_d Psi[c, d] w_d
    s = np.where((energy >= thr * energy.max())[..., None], w, 0.0)
    vox = tuple(d for d in src.dims if d not in (dim, time_dim))
    coords = {k: co for k, co in src.coords.items() if co.dim in vox or co.dim == dim}
    return LabeledArray(np.ascontiguousarray(np.moveaxis(s, -1, 0)), (str(dim),) + vox, coords, _copy.copy(src.attrs), src.name)
