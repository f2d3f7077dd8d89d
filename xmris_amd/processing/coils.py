"""``combine_coils``: per-voxel coil combination of phased-array data on the GPU, the step in front of the single-channel
chain (zero_fill ... autophase, baseline_als, fit_amares).

The definition is this backend's own (the reference has no such function).  For every voxel, with
X its C x N matrix of FIDs, R the same voxel of `reference` (or X) and Psi = L L^H the noise covariance (or I):
G = L^-1 (R R^H) L^-H; u = the unit eigenvector of G's largest eigenvalue (``"svd"``, Rodgers & Robson's WSVD) or
L^-1 mean(R[:, :n_points]) normalised (``"first_point"``); w = L^-H u turned so that w^H R[:, 0] >= 0; y = w^H X;
quality = u^H G u / trace(G).  One launch of ``xm_coil_combine`` does all voxels.
"""
from __future__ import annotations

import copy as _copy

import numpy as np

from .. import device as dev
from ..config import ATTRS, DIMS
from ..labeled import LabeledArray, as_labeled, is_xarray, like_input
from ._common import device_data

METHODS = ("svd", "first_point")
MAX_COILS = 64


def tail_points(n: int) -> int:
    """Points at the end of an FID that ``noise_cov="tail"`` takes for noise: the window of the reference's SNR estimate
    (fitting/amares.py:301)."""
    return min(n, max(10, n // 5))


def _linv(noise_cov, c: int) -> np.ndarray:
    """L^-1 of the Cholesky factor of a C x C Hermitian positive-definite matrix (host, complex128)."""
    psi = np.asarray(noise_cov)
    if psi.shape != (c, c):
        raise ValueError(f"noise_cov must be a {c} x {c} matrix (one row per coil), got shape {psi.shape}")
    psi = psi.astype(np.complex128)
    # Hermitian to rounding on the scale of its diagonal: |psi_ij - conj(psi_ji)| <= 1e-12 sqrt(|psi_ii psi_jj|)
    d = np.sqrt(np.abs(np.diag(psi).real))
    herm = np.all(np.isfinite(psi)) and np.all(np.abs(psi - psi.conj().T) <= 1e-12 * np.outer(d, d))
    try:
        if not herm:
            raise np.linalg.LinAlgError
        chol = np.linalg.cholesky(psi)
    except np.linalg.LinAlgError:
        raise ValueError("noise_cov must be Hermitian and positive definite") from None
    return np.ascontiguousarray(np.linalg.solve(chol, np.eye(c, dtype=np.complex128)))


def _tail_cov(x, coil_axis: int, time_axis: int):
    """Pooled noise covariance of the last tail_points(N) samples of every voxel: (1 / S) sum_s n_s n_s^H over the S
    pooled samples n_s (one C-vector each), computed on the device; one C x C matrix comes back."""
    import torch

    k = tail_points(x.shape[time_axis])
    tail = torch.movedim(x.narrow(time_axis, x.shape[time_axis] - k, k), coil_axis, 0)
    t2 = tail.reshape(tail.shape[0], -1).to(torch.complex128)
    psi = (t2 @ t2.conj().T / t2.shape[1]).cpu().numpy()
    return 0.5 * (psi + psi.conj().T)  # Hermitian exactly, whatever order the product was summed in


def combine_coils(da, dim: str = DIMS.coil, time_dim: str = DIMS.time, method: str = "svd", reference=None,
                  noise_cov=None, n_points: int = 1, return_weights: bool = False):
    """Combine the `dim` (coil) axis of `da` away, one weight vector per voxel.  `reference`: an array with the same
    dims and sizes except along `time_dim` (e.g. an unsuppressed water scan) that the weights are computed from.
    `noise_cov`: a C x C Hermitian positive-definite matrix, or ``"tail"`` to estimate it from the end of the FIDs of
    `da`.  Returns the input without `dim` (other dims, coords and attrs kept, plus attrs ``coil_combine_method`` /
    ``coil_combine_dim``), device-resident; with `return_weights` a dataset of ``combined``, ``weights`` (other dims...,
    coil), ``quality`` and ``status`` (0 combined, 1 nothing to go by, 2 non-finite sample, 3 iteration cap).  The coil
    axis may sit anywhere in front of a trailing `time_dim`; a `time_dim` that is not last costs one contiguous copy."""
    src = as_labeled(da)
    for name, d in (("dim", dim), ("time_dim", time_dim)):
        if d not in src.dims:
            raise ValueError(f"{name}: dimension {d!r} missing in the array (dims {src.dims})")
    if dim == time_dim:
        raise ValueError("dim and time_dim must differ")
    ca, ta = src.get_axis_num(dim), src.get_axis_num(time_dim)
    c, n = src.shape[ca], src.shape[ta]
    if c < 1 or c > MAX_COILS:
        raise ValueError(f"dim: {c} coils along {dim!r}, supported are 1 ... {MAX_COILS}")
    if method not in METHODS:
        raise ValueError(f"method must be one of {METHODS}, got {method!r}")
    n_ref, ref = n, None
    if reference is not None:
        ref = as_labeled(reference)
        same = ref.dims == src.dims and all(ref.sizes[d] == src.sizes[d] for d in src.dims if d != time_dim)
        if not same:
            raise ValueError(f"reference: dims / sizes {ref.sizes} must equal the data's {src.sizes} except along "
                             f"{time_dim!r}")
        n_ref = ref.sizes[time_dim]
    if n < 1 or n_ref < 1:
        raise ValueError(f"time_dim: {time_dim!r} must have at least one point")
    if int(n_points) != n_points or not 1 <= n_points <= n_ref:
        raise ValueError(f"n_points must be in 1 ... {n_ref}, got {n_points!r}")
    tail = isinstance(noise_cov, str)
    if tail and noise_cov != "tail":
        raise ValueError(f"noise_cov must be a {c} x {c} matrix or 'tail', got {noise_cov!r}")
    linv = None if noise_cov is None or tail else _linv(noise_cov, c)

    x, _ = device_data(src)
    if tail:
        linv = _linv(_tail_cov(x, ca, ta), c)
    r = None
    if ref is not None:
        r, _ = device_data(ref)
        r = r.to(x.dtype)
    res = dev.coil_combine(x, ca, ta, method=method, reference=r, linv=linv, n_points=int(n_points))

    other = tuple(d for d in src.dims if d != dim)
    vox = tuple(d for d in other if d != time_dim)
    y = res.y
    if other.index(time_dim) != len(other) - 1:
        import torch

        y = torch.movedim(y, -1, other.index(time_dim)).contiguous()
    attrs = _copy.copy(src.attrs)
    attrs[ATTRS.coil_combine_method] = method
    attrs[ATTRS.coil_combine_dim] = str(dim)
    coords = {k: c_ for k, c_ in src.coords.items() if c_.dim != dim}
    out = LabeledArray(y, other, coords, attrs, src.name)
    if not return_weights:
        return like_input(out, da)
    from ..fitting.dataset import LabeledDataset

    vcoords = {k: c_ for k, c_ in src.coords.items() if c_.dim in vox}
    wcoords = {k: c_ for k, c_ in src.coords.items() if c_.dim in vox or c_.dim == dim}
    ds = LabeledDataset({"combined": out,
                         "weights": LabeledArray(res.weights, vox + (str(dim),), wcoords),
                         "quality": LabeledArray(res.quality, vox, vcoords),
                         "status": LabeledArray(res.status, vox, vcoords)}, attrs)
    return ds.to_xarray() if is_xarray(da) else ds
