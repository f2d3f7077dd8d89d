"""``to_image`` / ``to_kspace``: MRSI spatial reconstruction on the GPU, the step in front of ``combine_coils``.

The definition is this backend's own (the reference has nothing beyond ``zero_fill`` + ``ifftc``).
Per transformed axis with n points in and m >= n out, c_n = n // 2, c_m = m // 2:

    T[p][j] = w[j] exp(-sigma 2 pi i (j - c_n) s / m) exp(sigma 2 pi i (j - c_n) (p - c_m) / m) / sqrt(m)

sigma = +1 for ``to_image`` and -1 for ``to_kspace``, w the filter, s the shift in output points.  Filter, zero fill,
shift, both centring rolls and the ortho scale are all in that matrix: the padded zeros are never stored or multiplied.
With m <= 64 a dim is one launch of ``xm_axis_dft`` on the tensor where it lies (no transpose); a larger m runs the
same factors as ``phase_apply`` -> ``zero_fill`` -> ``fft``.  The zero fill puts the k-space centre n // 2 on m // 2
(pad_left = m // 2 - n // 2), which differs from the reference's symmetric pad (m - n) // 2 for odd n and even m only.
"""
from __future__ import annotations

import copy as _copy

import numpy as np

from .. import device as dev
from ..config import ATTRS, DIMS
from ..dims import _check_dims
from ..labeled import Coordinate, LabeledArray, as_labeled, like_input
from ._common import device_data

FILTERS = {"hamming": 0.54, "hann": 0.5}
_TO_IMAGE = {DIMS.kx: DIMS.x, DIMS.ky: DIMS.y, DIMS.kz: DIMS.z}
_TO_KSPACE = {v: k for k, v in _TO_IMAGE.items()}


def filter_weights(name: str, n: int) -> np.ndarray:
    """alpha + (1 - alpha) cos(2 pi (j - n // 2) / n): centred on the DC sample n // 2, periodic."""
    alpha = FILTERS[name]
    return alpha + (1.0 - alpha) * np.cos(2.0 * np.pi * (np.arange(n) - n // 2) / n)


def _unit(num, den: int, sign: float) -> np.ndarray:
    """exp(sign 2 pi i num / den) for integer `num`: the fraction is reduced on the integers."""
    a = 2.0 * np.pi * (np.asarray(num, dtype=np.int64) % den) / den
    return np.cos(a) + 1j * sign * np.sin(a)


def ramp(n: int, m: int, weights, shift: float, sign: float) -> np.ndarray:
    """w[j] exp(-sign 2 pi i (j - n // 2) s / m): the factors of T that depend on j alone (complex128, n values)."""
    k = np.arange(n) - n // 2
    w = np.ones(n) if weights is None else np.asarray(weights, dtype=np.float64)
    return w * np.exp(-sign * 2j * np.pi * k * (float(shift) / m))


def axis_table(n: int, m: int, weights=None, shift: float = 0.0, sign: float = 1.0) -> np.ndarray:
    """T of the module docstring, [m, n] complex128, from fp64 host arithmetic."""
    k = np.arange(n) - n // 2
    p = np.arange(m) - m // 2
    return ramp(n, m, weights, shift, sign)[None, :] * _unit(np.outer(p, k), m, sign) / np.sqrt(m)


def _per_dim(value, count: int, what: str, cast):
    """None -> None; a scalar -> that for every dim; a sequence -> one entry per dim."""
    if value is None:
        return None
    if np.ndim(value) == 0:
        raw = (value,) * count
    else:
        raw = tuple(value)
        if len(raw) != count:
            raise ValueError(f"{what}: {len(raw)} values for {count} dims")
    try:
        return tuple(cast(v) for v in raw)
    except (TypeError, ValueError):
        raise ValueError(f"{what} must be {cast.__doc__}, got {value!r}") from None


def _int(v):
    """an integer or one integer per dim"""
    if isinstance(v, bool) or int(v) != v:
        raise ValueError
    return int(v)


def _float(v):
    """a finite number or one per dim"""
    f = float(v)
    if not np.isfinite(f):
        raise ValueError
    return f


def _filters(filter, names, sizes):
    """(weights per dim: None or n fp64 values, the label for the attrs)."""
    if filter is None:
        return [None] * len(names), "none"
    if isinstance(filter, str):
        if filter not in FILTERS:
            raise ValueError(f"filter: unknown name {filter!r}; known are {tuple(FILTERS)}, or give one array per dim")
        return [filter_weights(filter, n) for n in sizes], filter
    try:
        entries = list(filter)
    except TypeError:
        raise ValueError(f"filter must be None, a name or a sequence with one entry per dim, got {filter!r}") from None
    if len(entries) != len(names):
        raise ValueError(f"filter: {len(entries)} entries for {len(names)} dims (a sequence holds one entry per dim)")
    out = []
    for d, n, e in zip(names, sizes, entries):
        if e is None:
            out.append(None)
        elif isinstance(e, str):
            if e not in FILTERS:
                raise ValueError(f"filter: unknown name {e!r} for {d!r}; known are {tuple(FILTERS)}")
            out.append(filter_weights(e, n))
        else:
            w = np.asarray(e)
            if w.ndim != 1 or w.dtype.kind not in "fiu" or len(w) != n or not np.all(np.isfinite(w)):
                raise ValueError(f"filter: the entry for {d!r} must be {n} finite real weights, got shape {w.shape} "
                                 f"of {w.dtype}")
            out.append(w.astype(np.float64))
    return out, "custom"


def _reconstruct(da, dim, out_dim, matrix, filter, shift, sign: float, default_names, name: str, _staged: bool):
    src = as_labeled(da)
    names = (dim,) if isinstance(dim, str) else tuple(dim)
    _check_dims(src, names, name)
    if not 1 <= len(names) <= 3:
        raise ValueError(f"dim: needs 1 ... 3 dimensions, got {len(names)}")
    if len(set(names)) != len(names):
        raise ValueError(f"dim: a dimension is repeated in {names}")
    if out_dim is None:
        unknown = [d for d in names if d not in default_names]
        if unknown:
            raise ValueError(f"out_dim: no default name for {unknown}; {name} renames {dict(default_names)} on its own, "
                             "any other dim needs an explicit out_dim")
        outs = tuple(default_names[d] for d in names)
    else:
        outs = (out_dim,) if isinstance(out_dim, str) else tuple(out_dim)
        if len(outs) != len(names):
            raise ValueError(f"out_dim: {len(outs)} names for {len(names)} dims")
    others = [d for d in src.dims if d not in names]
    if len(set(outs)) != len(outs) or any(o in others for o in outs):
        raise ValueError(f"out_dim: {outs} repeats a name or takes the name of another dim of the array ({src.dims})")
    for d in names:  # as in fft: KeyError without a coordinate
        src.coords[d]
    sizes = [src.sizes[d] for d in names]
    mat = _per_dim(matrix, len(names), "matrix", _int)
    mat = tuple(sizes) if mat is None else mat
    for d, n, m in zip(names, sizes, mat):
        if m < n:
            raise ValueError(f"matrix: {m} points along {d!r}, which has {n}; the matrix must be at least the dim's size")
    if any(n < 1 for n in sizes):
        raise ValueError(f"dim: {names} holds an empty dimension")
    sh = _per_dim(shift, len(names), "shift", _float)
    sh = (0.0,) * len(names) if sh is None else sh
    weights, label = _filters(filter, names, sizes)

    x, _ = device_data(src)
    for d, n, m, w, s in zip(names, sizes, mat, weights, sh):
        axis = src.get_axis_num(d)
        if m <= dev.AXIS_DFT_MAX and not _staged:
            x = dev.axis_dft(x, axis, axis_table(n, m, w, s, sign))
        else:  # the same factors from the calls that were there before the kernel
            if w is not None or s != 0.0:
                x = dev.phase_apply(x, axis, ramp(n, m, w, s, sign))
            if m != n:
                x = dev.zero_fill(x, axis, m, pad_left=m // 2 - n // 2)
            x = dev.fft(x, axis, inverse=sign > 0, ortho=True, shift_in=True, shift_out=True)

    new_dims = [outs[names.index(d)] if d in names else d for d in src.dims]
    coords = {}
    for k, c in src.coords.items():
        if c.dim not in names:
            coords[k] = c
            continue
        i = names.index(c.dim)
        if k == c.dim:
            old = np.asarray(c.values)
            delta = (old[1] - old[0]) if len(old) > 1 else 1.0
            coords[outs[i]] = Coordinate(outs[i], np.roll(np.fft.fftfreq(mat[i], d=delta), mat[i] // 2), {})
        elif mat[i] == sizes[i] and k not in outs:  # (ifftc's two rolls add up to a full turn: kept as they are)
            coords[k] = Coordinate(outs[i], c.values, c.attrs)
    attrs = _copy.copy(src.attrs)
    attrs[ATTRS.mrsi_dims] = tuple(str(d) for d in names)
    attrs[ATTRS.mrsi_matrix] = tuple(mat)
    attrs[ATTRS.mrsi_filter] = label
    attrs[ATTRS.mrsi_shift] = tuple(sh)
    return like_input(LabeledArray(x, new_dims, coords, attrs, src.name), da)


def to_image(da, dim=(DIMS.kx, DIMS.ky), out_dim=None, matrix=None, filter=None, shift=None, _staged: bool = False):
    """k-space -> voxels along `dim` (one name or 1 ... 3): the k-space is weighted by `filter`, zero filled to
    `matrix`, shifted by `shift` output voxels and inverse transformed (centred, ortho), one launch per dim.
    `out_dim`: the new names; ``kx -> x, ky -> y, kz -> z`` by default, any other dim needs it.  `matrix`: None (the
    dims' sizes), an int for all or one per dim, at least the dim's size.  `filter`: None, ``"hamming"`` or ``"hann"``
    (centred on the DC sample n // 2, periodic), or a sequence with one entry per dim of None, a name or n real
    weights.  `shift`: None, a number for all or one per dim; positive moves the image towards higher index, an integer
    equals a roll.  Constant k-space gives a peak at matrix // 2.  Returns the array with the dims renamed, the
    reciprocal coordinates ``roll(fftfreq(m, d=c[1] - c[0]), m // 2)``, attrs kept plus ``mrsi_dims``, ``mrsi_matrix``,
    ``mrsi_filter`` and ``mrsi_shift``; device-resident for LabeledArray input."""
    return _reconstruct(da, dim, out_dim, matrix, filter, shift, 1.0, _TO_IMAGE, "to_image", _staged)


def to_kspace(da, dim=(DIMS.x, DIMS.y), out_dim=None, matrix=None, filter=None, shift=None, _staged: bool = False):
    """Voxels -> k-space along `dim`: ``to_image`` with the forward transform (``x -> kx, y -> ky, z -> kz`` by
    default).  Without filter, zero fill and shift it undoes ``to_image``."""
    return _reconstruct(da, dim, out_dim, matrix, filter, shift, -1.0, _TO_KSPACE, "to_kspace", _staged)
