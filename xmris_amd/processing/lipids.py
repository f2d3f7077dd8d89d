"""``remove_lipids`` / ``lipid_basis``: lipid-subspace (L2) suppression of 1H MRSI on the GPU (Bilgic 2014; the
subspace variants of Ma 2016), the step between ``remove_water`` and ``denoise_mppca`` / the fits.

The definition is this backend's own (the reference has no such function).  Data are
``[..., time]``; a row is one FID.  The FIDs of the voxels inside a scalp mask (or the rows given as ``basis=``) are the
columns of M (T x N_l) = U S V^H.  Every row y is replaced by

    x = argmin ||x - y||^2 + beta ||M^H x||^2 = (I + beta M M^H)^-1 y = y - sum_k u_k w_k (u_k^H y),

    beta = 1 / (level sigma_1)^2,    w_k = beta sigma_k^2 / (1 + beta sigma_k^2):

`level` is the singular value, relative to the largest, at which a component is halved, so the call does not depend on
the data's scale.  The operator is linear along time and the same for every row: it is the same on FIDs and on spectra.
"""
from __future__ import annotations

import copy as _copy
from dataclasses import dataclass, field

import numpy as np

from .. import device as dev
from ..config import ATTRS, DIMS
from ..labeled import LabeledArray, as_labeled, like_input
from ._common import device_data

MIN_WEIGHT = 2.0 ** -20  # rank=None keeps every component with at least this weight


@dataclass
class LipidBasis:
    """The result of ``lipid_basis``.  `vectors`: [time, rank] complex128, the orthonormal u_k; `sigma`: every singular
    value of the lipid rows, descending; `weights`: w_k of the `rank` components kept; `beta`, `level`; `n_rows`: the
    lipid rows N_l the basis was made from; `dropped_weight`: the w of the first component left out, or 0.  The record
    keeps the device copy of its table that its first use on a device made, so one basis serves the frames of a dynamic
    series; `vectors` and `weights` are not to be changed in place."""

    vectors: np.ndarray
    sigma: np.ndarray
    weights: np.ndarray
    beta: float
    level: float
    n_rows: int
    dropped_weight: float = 0.0
    _resident: dict = field(default_factory=dict, repr=False, compare=False)  # device -> the uploaded table

    @property
    def rank(self) -> int:
        return int(self.vectors.shape[1])

    @property
    def n_time(self) -> int:
        return int(self.vectors.shape[0])

    def table_on(self, device):
        """U[T][r] (re, im), then w[r] as an fp64 tensor on `device`: uploaded at the first call, the same afterwards."""
        key = str(device)
        if key not in self._resident:
            self._resident[key] = dev.lipid_tables(self.vectors, self.weights, device)
        return self._resident[key]


def _check_level(level) -> float:
    try:
        lv = float(level)
    except (TypeError, ValueError):
        raise ValueError(f"level must be a positive number, got {level!r}") from None
    if not (np.isfinite(lv) and lv > 0):
        raise ValueError(f"level must be finite and positive, got {level!r}")
    return lv


def _check_rank(rank):
    if rank is None:
        return None
    if isinstance(rank, bool) or int(rank) != rank or not 1 <= rank <= dev.LIPID_MAX_RANK:
        raise ValueError(f"rank must be None or an integer in 1 ... {dev.LIPID_MAX_RANK}, got {rank!r}")
    return int(rank)


def lipid_weights(sigma, level: float):
    """(beta, w) of the singular values `sigma` (descending): beta = 1 / (level sigma_1)^2, w = beta s^2 / (1 + beta s^2),
    formed as q / (1 + q) with q = (s / (level sigma_1))^2."""
    sigma = np.asarray(sigma, dtype=np.float64)
    s1 = float(sigma[0])
    if not (np.isfinite(s1) and s1 > 0):
        raise ValueError("the lipid basis is all zero (or not finite): there is no subspace to remove")
    q = (sigma / (level * s1)) ** 2
    return 1.0 / (level * s1) ** 2, q / (1.0 + q)


def basis_from_subspace(sigma, vectors, level: float = 0.01, rank=None, n_rows: int = 0) -> LipidBasis:
    """The record from the singular values (all, descending) and the leading left vectors [time, >= rank] of the lipid
    rows: the weights, the rank rule (`rank` = None: every k with w_k >= 2^-20, at least 1 and at most 64) and
    `dropped_weight`."""
    level, rank = _check_level(level), _check_rank(rank)
    sigma = np.asarray(sigma, dtype=np.float64).reshape(-1)
    vectors = np.asarray(vectors, dtype=np.complex128)
    beta, w = lipid_weights(sigma, level)
    avail = min(len(sigma), vectors.shape[1], dev.LIPID_MAX_RANK)
    if rank is None:
        r = max(1, min(int(np.count_nonzero(w >= MIN_WEIGHT)), avail))
    else:
        if rank > avail:
            raise ValueError(f"rank: {rank} components asked for, the lipid rows have {avail} (min of their count, the "
                             f"points along time and {dev.LIPID_MAX_RANK})")
        r = rank
    dropped = float(w[r]) if r < len(w) else 0.0
    return LipidBasis(vectors=np.ascontiguousarray(vectors[:, :r]), sigma=sigma, weights=np.ascontiguousarray(w[:r]),
                      beta=float(beta), level=level, n_rows=int(n_rows), dropped_weight=dropped)


def _names(dims):
    return (dims,) if isinstance(dims, str) else tuple(str(d) for d in dims)


def _mask(src, mask, dims, dim: str, what: str):
    """(dim names, boolean array over them) of a mask argument, checked against the data."""
    if dims is None and hasattr(mask, "dims"):
        dims = tuple(mask.dims)
    if dims is None:
        raise ValueError(f"dims: name the dimensions that {what} extends over")
    names = _names(dims)
    if len(set(names)) != len(names) or not names:
        raise ValueError(f"dims must be distinct dimension names, got {dims!r}")
    for d in names:
        if d not in src.dims:
            raise ValueError(f"dims: dimension {d!r} missing in the array (dims {src.dims})")
        if d == dim:
            raise ValueError(f"dims: {d!r} is the time dim of the rows")
    m = np.asarray(getattr(mask, "values", mask))
    if m.dtype != np.bool_:
        raise TypeError(f"{what} must be boolean, got dtype {m.dtype}")
    want = tuple(src.sizes[d] for d in names)
    if m.shape != want:
        raise ValueError(f"{what}: shape {m.shape} does not match the dims {names} of sizes {want}")
    return names, m


def _time_last(src, x, dim: str):
    """x with `dim` last (a view) and the names of the leading dims."""
    ta = src.get_axis_num(dim)
    lead = tuple(d for d in src.dims if d != dim)
    if ta != src.ndim - 1:
        x = x.movedim(ta, -1) if hasattr(x, "movedim") else np.moveaxis(x, ta, -1)
    return x, lead


def _check_data(src, dim: str, who: str):
    if dim not in src.dims:
        raise ValueError(f"dim: dimension {dim!r} missing in the array (dims {src.dims})")
    if src.dtype not in (np.dtype(np.complex64), np.dtype(np.complex128)):
        raise ValueError(f"{who} needs complex64 or complex128 rows, got dtype {src.dtype}")
    T = src.sizes[dim]
    if not dev.LIPID_MIN_POINTS <= T <= dev.LIPID_MAX_POINTS:
        raise ValueError(f"dim: {dim!r} has {T} points; needs {dev.LIPID_MIN_POINTS} ... {dev.LIPID_MAX_POINTS}")
    return T


def _build(src, x, lipid_mask, basis, dims, level, rank, dim: str, who: str) -> LipidBasis:
    """The checks of both public functions and the basis; `x`: a callable that gives the device data (not called before
    every check of the metadata has passed)."""
    level, rank = _check_level(level), _check_rank(rank)
    if (lipid_mask is None) == (basis is None):
        raise ValueError(f"{who} needs exactly one of lipid_mask and basis=")
    T = _check_data(src, dim, who) if src is not None else None
    if isinstance(basis, LipidBasis):
        if T is not None and basis.n_time != T:
            raise ValueError(f"basis: made for {basis.n_time} points along time, {dim!r} has {T}")
        return basis
    if basis is not None:
        shape = tuple(getattr(basis, "shape", np.shape(basis)))
        if len(shape) != 2 or shape[0] < 1:
            raise ValueError(f"basis must be [n, time] with n >= 1, got shape {shape}")
        if T is not None and shape[1] != T:
            raise ValueError(f"basis: {shape[1]} points along time, {dim!r} has {T}")
        if not dev.LIPID_MIN_POINTS <= shape[1] <= dev.LIPID_MAX_POINTS:
            raise ValueError(f"basis: {shape[1]} points along time; needs {dev.LIPID_MIN_POINTS} ... {dev.LIPID_MAX_POINTS}")
        L = basis if hasattr(basis, "detach") else dev.to_device(np.asarray(basis))
    else:
        if src is None:
            raise ValueError(f"{who}: a lipid_mask needs the data it selects rows of")
        names, m = _mask(src, lipid_mask, dims, dim, "lipid_mask")
        if not m.any():
            raise ValueError("lipid_mask has no true entry: there are no lipid rows")
        xt, lead = _time_last(src, x(), dim)
        L = dev.lipid_rows(xt, [lead.index(d) for d in names], m)
    sigma, vec = dev.lipid_subspace(L)
    return basis_from_subspace(sigma, vec, level, rank, n_rows=int(L.shape[0]))


def lipid_basis(x, lipid_mask=None, *, basis=None, dims=None, level: float = 0.01, rank=None,
                dim: str = DIMS.time) -> LipidBasis:
    """The lipid subspace of the rows of `x` inside `lipid_mask` (boolean over the dims named by `dims`; every other
    dim but `dim` contributes rows), or of the rows ``basis=[n, time]`` (`x` may then be None).  `level`: the singular
    value, relative to the largest, at which a component is halved; `rank`: the components kept, 1 ... 64, or None for
    every one with a weight of at least 2^-20 (at most 64).  The Gram matrix is one complex128 matmul on the device, its
    eigen-decomposition host numpy.  Returns a ``LipidBasis``; pass it as ``basis=`` to ``remove_lipids``."""
    src = as_labeled(x) if x is not None else None
    if isinstance(basis, LipidBasis):
        raise ValueError("lipid_basis: basis= is already a LipidBasis")
    return _build(src, (lambda: device_data(src)[0]), lipid_mask, basis, dims, level, rank, dim, "lipid_basis")


def remove_lipids(x, lipid_mask=None, *, basis=None, dims=None, level: float = 0.01, rank=None, apply_mask=None,
                  return_basis: bool = False, dim: str = DIMS.time):
    """Remove the lipid subspace from every row of `x` along `dim` (module docstring), one launch of
    ``xm_lipid_project``.  The subspace comes from the rows inside `lipid_mask` (boolean over `dims`), from rows
    ``basis=[n, time]``, or from a ``LipidBasis`` (`level` and `rank` are then the record's).  `apply_mask` (boolean over
    `dims`; default: every row): rows outside it are copied bit for bit.  A row with a non-finite sample becomes NaN and
    touches no other row.  Returns the input's kind with dims, coords, dtype and attrs kept, plus the attrs
    ``lipid_level``, ``lipid_rank``, ``lipid_beta`` and ``lipid_rows``, device-resident for LabeledArray input; with
    `return_basis` the tuple (result, the ``LipidBasis``, status per row: 0 done, 1 copied, 2 non-finite).  A `dim` that is
    not last costs one contiguous copy."""
    src = as_labeled(x)
    cache = []

    def data():
        if not cache:
            cache.append(device_data(src)[0])
        return cache[0]

    ap_names = ap = None
    if apply_mask is not None:
        _check_data(src, dim, "remove_lipids")
        ap_names, ap = _mask(src, apply_mask, dims, dim, "apply_mask")
    rec = _build(src, data, lipid_mask, basis, dims, level, rank, dim, "remove_lipids")

    xt, lead = _time_last(src, data(), dim)
    apply = None
    if ap is not None:
        order = sorted(range(len(ap_names)), key=lambda i: lead.index(ap_names[i]))
        shape = [src.sizes[d] if d in ap_names else 1 for d in lead]
        apply = np.broadcast_to(np.transpose(ap, order).reshape(shape), tuple(src.sizes[d] for d in lead))
    res = dev.lipid_project(xt, rec, apply)
    y = res.out
    ta = src.get_axis_num(dim)
    if ta != src.ndim - 1:
        y = y.movedim(-1, ta).contiguous() if hasattr(y, "movedim") else np.ascontiguousarray(np.moveaxis(y, -1, ta))
    attrs = _copy.copy(src.attrs)
    attrs[ATTRS.lipid_level] = rec.level
    attrs[ATTRS.lipid_rank] = rec.rank
    attrs[ATTRS.lipid_beta] = rec.beta
    attrs[ATTRS.lipid_rows] = rec.n_rows
    out = like_input(LabeledArray(y, tuple(src.dims), dict(src.coords), attrs, src.name), x)
    if not return_basis:
        return out
    vcoords = {k: c_ for k, c_ in src.coords.items() if c_.dim in lead}
    return out, rec, LabeledArray(res.status, lead, vcoords)
