"""``grappa_calibrate`` / ``grappa_fill``: GRAPPA for regularly undersampled Cartesian phased-array MRSI (Griswold et al.
2002) on the GPU, the route from accelerated k-space to the full grid when no coil sensitivity maps exist: the weights
come from a small fully sampled centre of k-space, the auto-calibration signal (ACS).  ``grappa_fill`` -> ``to_image`` ->
``combine_coils`` -> the single-channel chain.

The definition is this backend's own (the reference has no such function).  Per undersampled dim
with n kept lines and acceleration R, N = R n: the kept lines of the full centred k-space are j = j0 + R l,
j0 = N // 2 - R (n // 2), the sampling of ``unfold_sense`` (section 16).  A full-grid position has per dim
l = floor((j - j0) / R) and o = (j - j0) mod R; o = 0 everywhere: acquired, copied bit for bit.  Any other offset tuple is
a type (R - 1 of them, row-major over the offsets), and with the block sizes b per dim

    y[c, j, t] = sum_s sum_c' W[type][c][s][c'] a[c', l + s, t],   s = -((b - 1) // 2) ... b // 2 per dim,

s row-major, a neighbour outside the kept lines skipped.  One launch of ``xm_grappa_fill`` writes the whole grid.

Calibration (host numpy, complex128): for a type with offsets o, every position p of the ACS block whose S sources
p - o + R s lie inside the block gives one equation per calibration time point; Sm [K, n_eq] (K = C S, rows ordered
s then coil) and Tm [C, n_eq]; G = Sm Sm^H, lambda' = regularization trace(G) / K, W = ((G + lambda' I)^-1 Sm Tm^H)^H.
"""
from __future__ import annotations

import copy as _copy
import itertools
from dataclasses import dataclass, field

import numpy as np

from .. import device as dev
from ..config import ATTRS, DIMS
from ..dims import _check_dims
from ..labeled import Coordinate, LabeledArray, as_labeled, is_xarray, like_input
from ._common import device_data, to_host
from .mrsi import _int, _per_dim

MAX_COILS = dev.GRAPPA_MAX_COILS
MAX_ACCEL = dev.GRAPPA_MAX_ACCEL
MAX_SOURCES = dev.GRAPPA_MAX_SOURCES  # S = the product of the kernel sizes
MAX_TERMS = dev.GRAPPA_MAX_TERMS  # C S
MAX_SYSTEM = 1 << 26  # entries of the calibration's source matrix Sm


@dataclass(frozen=True)
class GrappaWeights:
    """The result of ``grappa_calibrate``.  `weights`: [R - 1, C, S, C] complex128, per type the C x (S C) matrix that
    makes a missing sample of coil c from the sources (neighbour s, coil c'); `accel`, `kernel`: per dim of `dims`;
    per type `n_equations`, `kappa` (of G + lambda' I) and `residual` (||W Sm - Tm|| / ||Tm||).  The record keeps the
    device copy of `weights` that its first ``grappa_fill`` on a device made, so `weights` is not to be changed in place."""

    weights: np.ndarray
    accel: tuple
    kernel: tuple
    dims: tuple
    n_equations: tuple
    kappa: tuple
    residual: tuple
    regularization: float = 0.0
    _resident: dict = field(default_factory=dict, repr=False, compare=False)  # device -> the uploaded weights

    @property
    def coils(self) -> int:
        return int(self.weights.shape[1])

    def on_device(self, device):
        """`weights` as a complex128 tensor on `device`: uploaded at the first call, the same tensor afterwards."""
        key = str(device)
        if key not in self._resident:
            self._resident[key] = dev.grappa_weights(self.weights, device)
        return self._resident[key]


def type_offsets(accel):
    """The offset tuples of the R - 1 types, row-major, the all-zero tuple skipped."""
    return [o for o in itertools.product(*[range(r) for r in accel]) if any(o)]


def neighbour_range(b: int):
    """The neighbour lines s of a block of b lines."""
    return range(-((b - 1) // 2), b // 2 + 1)


def _names(dims):
    return (dims,) if isinstance(dims, str) else tuple(str(d) for d in dims)


def _geometry(accel, kernel, count: int):
    """(accel, kernel) per dim, checked."""
    acc = _per_dim(accel, count, "accel", _int)
    if acc is None or any(r < 1 for r in acc):
        raise ValueError(f"accel must be an integer >= 1 or one per dim, got {accel!r}")
    if int(np.prod(acc)) > MAX_ACCEL:
        raise ValueError(f"accel: the total acceleration {int(np.prod(acc))} exceeds {MAX_ACCEL}")
    ker = tuple(2 if r > 1 else 3 for r in acc) if kernel is None else _per_dim(kernel, count, "kernel", _int)
    if any(b < 1 for b in ker):
        raise ValueError(f"kernel must be an integer >= 1 or one per dim, got {kernel!r}")
    if int(np.prod(ker)) > MAX_SOURCES:
        raise ValueError(f"kernel: {int(np.prod(ker))} neighbours per sample exceed {MAX_SOURCES}")
    return acc, ker


def _check_names(names, coil_dim, time_dim):
    if not 1 <= len(names) <= 3:
        raise ValueError(f"dims: needs 1 ... 3 dimensions, got {len(names)}")
    if len(set(names)) != len(names):
        raise ValueError(f"dims: a dimension is repeated in {names}")
    for arg, d in (("coil_dim", coil_dim), ("time_dim", time_dim)):
        if d in names:
            raise ValueError(f"{arg}: {d!r} is one of the undersampled dims {names}")
    if coil_dim == time_dim:
        raise ValueError("coil_dim and time_dim must differ")


def _number(value, what: str) -> float:
    try:
        v = float(value)
    except (TypeError, ValueError):
        v = float("nan")
    if not np.isfinite(v) or v < 0.0:
        raise ValueError(f"{what} must be a finite number >= 0, got {value!r}")
    return v


def _acs_values(acs, names, coil_dim, time_dim):
    """The ACS block as a host complex128 array (coil, *names, time)."""
    if isinstance(acs, LabeledArray) or is_xarray(acs):
        s = as_labeled(acs)
        order = (coil_dim, *names) + ((time_dim,) if time_dim in s.dims else ())
        if set(s.dims) != set(order) or len(s.dims) != len(order):
            raise ValueError(f"acs: dims {s.dims} must be {(coil_dim, *names)}, with or without {time_dim!r}, in any order")
        vals = np.transpose(to_host(s.data), [s.get_axis_num(d) for d in order])
    else:
        vals = to_host(acs) if hasattr(acs, "detach") else np.asarray(acs)
        if vals.ndim not in (len(names) + 1, len(names) + 2):
            raise ValueError(f"acs: an array must have the axes {(coil_dim, *names)}, with or without {time_dim!r}, "
                             f"got {vals.ndim} axes")
    if vals.ndim == len(names) + 1:
        vals = vals[..., None]
    if min(vals.shape) < 1:
        raise ValueError(f"acs: an empty axis in shape {vals.shape}")
    return np.asarray(vals, dtype=np.complex128)


def _calibrate(block, acc, ker, points: int, reg: float):
    """The weights of every type from block [C, A..., T] (complex128): (W [R - 1, C, S, C], n_eq, kappa, residual)."""
    c, shape = block.shape[0], block.shape[1:-1]
    t = min(points, block.shape[-1])
    s_tot, types = int(np.prod(ker)), type_offsets(acc)
    k = c * s_tot
    w = np.zeros((len(types), c, s_tot, c), dtype=np.complex128)
    n_eq, kappa, residual = [], [], []
    for ti, o in enumerate(types):
        # positions whose every source lies inside the block, per dim: lo ... hi
        lo = [oa + r * ((b - 1) // 2) for oa, r, b in zip(o, acc, ker)]
        hi = [a - 1 + min(0, oa - r * (b // 2)) for a, oa, r, b in zip(shape, o, acc, ker)]  # (the target inside as well)
        count = [max(h - l + 1, 0) for l, h in zip(lo, hi)]
        ne = int(np.prod(count)) * t
        if ne < k:
            raise ValueError(f"acs: type {o} has {ne} equations for {k} unknowns per coil ({c} coils x {s_tot} neighbours): "
                             f"a larger block, more acs_points or a smaller kernel is needed")
        if k * ne > MAX_SYSTEM:
            raise ValueError(f"acs: the calibration system of type {o} has {k} x {ne} entries, more than 2^26: lower "
                             f"acs_points or shrink the block")
        tm = block[(slice(None), *[slice(l, h + 1) for l, h in zip(lo, hi)], slice(0, t))].reshape(c, ne)
        sm = np.empty((s_tot, c, ne), dtype=np.complex128)
        for si, s in enumerate(itertools.product(*[neighbour_range(b) for b in ker])):
            sl = [slice(l - oa + r * sa, h - oa + r * sa + 1) for l, h, oa, r, sa in zip(lo, hi, o, acc, s)]
            sm[si] = block[(slice(None), *sl, slice(0, t))].reshape(c, ne)
        sm = sm.reshape(k, ne)
        g = sm @ sm.conj().T
        lam = reg * float(np.trace(g).real) / k
        gl = g + lam * np.eye(k)
        with np.errstate(all="ignore"):
            try:
                chol = np.linalg.cholesky(gl)
                ok = bool(np.all(np.isfinite(chol)))
            except np.linalg.LinAlgError:
                ok = False
            if ok:
                x = np.linalg.solve(chol.conj().T, np.linalg.solve(chol, sm @ tm.conj().T))  # [K, C]
                ok = bool(np.all(np.isfinite(x)))
        if not ok:
            raise ValueError(f"acs: the calibration system of type {o} is not positive definite or not finite; raise "
                             f"regularization (now {reg!r}) or check the block")
        wt = x.conj().T  # [C, K]
        w[ti] = wt.reshape(c, s_tot, c)
        ev = np.linalg.eigvalsh(gl)
        n_eq.append(ne)
        kappa.append(float(ev[-1] / ev[0]) if ev[0] > 0 else float("inf"))
        tn = float(np.linalg.norm(tm))
        residual.append(float(np.linalg.norm(wt @ sm - tm)) / tn if tn > 0 else 0.0)
    return w, tuple(n_eq), tuple(kappa), tuple(residual)


def grappa_calibrate(acs, accel, kernel=None, dims=(DIMS.kx, DIMS.ky), coil_dim: str = DIMS.coil,
                     time_dim: str = DIMS.time, acs_points: int = 8, regularization: float = 1e-4) -> GrappaWeights:
    """GRAPPA weights from the auto-calibration block `acs`, a fully sampled piece of the full k-space grid: an array
    with the dims ``(coil_dim, *dims)`` and optionally `time_dim` in any order, or array-like in that order.  `accel`:
    the acceleration, an int for all dims or one per dim, their product at most 16.  `kernel`: neighbour lines per dim
    (default 2 along an accelerated dim, 3 along one with accel 1), their product at most 64 and coils x product at
    most 1024.  Each of the first `acs_points` time points gives its own equations.  `regularization`: Tikhonov weight
    relative to the mean diagonal of the source Gram matrix.  Host work in complex128; raises ValueError when a type has
    fewer equations than unknowns, when the system would exceed 2^26 entries, or when it cannot be solved."""
    names = _names(dims)
    _check_names(names, coil_dim, time_dim)
    acc, ker = _geometry(accel, kernel, len(names))
    try:
        points = _int(acs_points)
    except (TypeError, ValueError):
        points = 0
    if points < 1:
        raise ValueError(f"acs_points must be an integer >= 1, got {acs_points!r}")
    reg = _number(regularization, "regularization")
    block = _acs_values(acs, names, coil_dim, time_dim)
    c = block.shape[0]
    if c > MAX_COILS:
        raise ValueError(f"acs: {c} coils along {coil_dim!r}, supported are 1 ... {MAX_COILS}")
    if c * int(np.prod(ker)) > MAX_TERMS:
        raise ValueError(f"kernel: {c} coils x {int(np.prod(ker))} neighbours exceed {MAX_TERMS} terms per sample")
    w, n_eq, kappa, residual = _calibrate(block, acc, ker, points, reg)
    return GrappaWeights(w, tuple(acc), tuple(ker), names, n_eq, kappa, residual, reg)


def grappa_fill(da, weights=None, *, acs=None, accel=None, kernel=None, dims=None, coil_dim: str = DIMS.coil,
                time_dim: str = DIMS.time, acs_points: int = 8, regularization: float = 1e-4, return_weights: bool = False):
    """Fill the regularly undersampled k-space `da` (the kept lines along `dims`, one name or 1 ... 3) to the full grid.
    Give exactly one of `weights` (a ``GrappaWeights``; `accel`, `kernel` and `dims` then default to its own and must
    agree with it when given) and `acs` (the calibration block; `accel` is required, the other arguments as in
    ``grappa_calibrate``; `dims` defaults to (kx, ky)).  Returns the input with every dim of `dims` grown to accel x its
    size (coordinate ``(arange(N) - N // 2) dk`` with dk the input's spacing over accel, other coordinates along a grown
    dim dropped), the acquired lines bit for bit, attrs kept plus ``grappa_dims``, ``grappa_accel``, ``grappa_kernel``
    and ``grappa_regularization``; device-resident for LabeledArray input.  With `return_weights` the pair (filled,
    ``GrappaWeights``)."""
    src = as_labeled(da)
    if (weights is None) == (acs is None):
        raise ValueError("weights: give exactly one of weights and acs")
    if weights is not None:
        if not isinstance(weights, GrappaWeights):
            raise ValueError(f"weights must be a GrappaWeights (grappa_calibrate), got {type(weights).__name__}")
        names = weights.dims if dims is None else _names(dims)
    else:
        names = (DIMS.kx, DIMS.ky) if dims is None else _names(dims)
    _check_dims(src, names, "grappa_fill")
    _check_names(names, coil_dim, time_dim)
    for arg, d in (("coil_dim", coil_dim), ("time_dim", time_dim)):
        if d not in src.dims:
            raise ValueError(f"{arg}: dimension {d!r} missing in the array (dims {src.dims})")
    ca, ta = src.get_axis_num(coil_dim), src.get_axis_num(time_dim)
    axes = [src.get_axis_num(d) for d in names]
    c = src.shape[ca]
    if c < 1 or c > MAX_COILS:
        raise ValueError(f"coil_dim: {c} coils along {coil_dim!r}, supported are 1 ... {MAX_COILS}")
    small = [src.shape[a] for a in axes]
    if src.shape[ta] < 1 or min(small) < 1:
        raise ValueError(f"dims: {names} or time_dim {time_dim!r} holds an empty dimension")
    if weights is not None:
        if tuple(names) != tuple(weights.dims):
            raise ValueError(f"weights: calibrated for the dims {weights.dims}, asked to fill {names}")
        acc, ker = _geometry(weights.accel if accel is None else accel, weights.kernel if kernel is None else kernel, len(names))
        if tuple(acc) != tuple(weights.accel):
            raise ValueError(f"weights: calibrated for accel {weights.accel}, asked for {tuple(acc)}")
        if tuple(ker) != tuple(weights.kernel):
            raise ValueError(f"weights: calibrated for kernel {weights.kernel}, asked for {tuple(ker)}")
        if weights.coils != c or tuple(weights.weights.shape) != (int(np.prod(acc)) - 1, c, int(np.prod(ker)), c):
            raise ValueError(f"weights: shape {tuple(weights.weights.shape)} does not fit {c} coils, accel {tuple(acc)} and "
                             f"kernel {tuple(ker)}")
        rec = weights
    else:
        if accel is None:
            raise ValueError("accel is required with acs")
        rec = grappa_calibrate(acs, accel, kernel, names, coil_dim, time_dim, acs_points, regularization)
        acc, ker = rec.accel, rec.kernel
        if rec.coils != c:
            raise ValueError(f"acs: {rec.coils} coils, the data has {c}")
    if c * int(np.prod(ker)) > MAX_TERMS:
        raise ValueError(f"kernel: {c} coils x {int(np.prod(ker))} neighbours exceed {MAX_TERMS} terms per sample")
    full = [r * n for r, n in zip(acc, small)]

    x, _ = device_data(src)
    w = None
    if len(rec.weights):
        w = rec.on_device(x.device) if hasattr(x, "detach") else rec.weights
    y = dev.grappa_fill(x, w, ca, axes, ta, list(acc), list(ker))
    if ta != len(src.dims) - 1:
        if hasattr(y, "detach"):
            import torch

            y = torch.movedim(y, -1, ta).contiguous()
        else:
            y = np.ascontiguousarray(np.moveaxis(y, -1, ta))
    coords = {}
    for k, co in src.coords.items():
        if co.dim not in names or full[names.index(co.dim)] == len(co.values):
            coords[k] = co
        elif k == co.dim:
            old = np.asarray(co.values)
            r = acc[names.index(co.dim)]
            dk = ((old[1] - old[0]) if len(old) > 1 else 1.0) / r
            m = full[names.index(co.dim)]
            coords[k] = Coordinate(k, (np.arange(m) - m // 2) * dk, co.attrs)
    attrs = _copy.copy(src.attrs)
    attrs[ATTRS.grappa_dims] = tuple(str(d) for d in names)
    attrs[ATTRS.grappa_accel] = tuple(acc)
    attrs[ATTRS.grappa_kernel] = tuple(ker)
    attrs[ATTRS.grappa_regularization] = float(rec.regularization)
    out = like_input(LabeledArray(y, src.dims, coords, attrs, src.name), da)
    return (out, rec) if return_weights else out
