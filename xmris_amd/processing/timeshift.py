"""``shift_time`` / ``correct_readout_time`` / ``readout_offsets``: per-row time shifts of FIDs on the GPU, the step in
front of ``grid_kspace`` for spiral, ring, rosette and EPSI readouts, whose sample s is acquired tau_s after the nominal
time of its spectral point.

The definition is this backend's own (the reference has nothing here).  Along `dim`, N points of
dwell dt, transform length L = `pad_to` >= N (default N), phi = tau / dt:

    X[k] = sum_{n<N} x[n] exp(-2 pi i k n / L)                                  k = 0 ... L - 1
    kappa_k = numpy.fft.fftfreq(L)[k] L
    y[n] = (1 / L) sum_k X[k] exp(-2 pi i kappa_k phi / L) exp(+2 pi i k n / L)     n = 0 ... N - 1

-- the periodic band-limited interpolant of the zero-padded row, evaluated tau earlier: a row acquired tau late,
x[n] = s(t_n + tau), comes back as s(t_n).  A delay of whole dwells is a circular roll over L; at L = N the operator is
unitary and ``shift_time(., -tau)`` is its inverse and its Hermitian transpose.  An FID jumps at t = 0, so the
interpolant rings there: the first few output points, y[0] above all, are not the unshifted FID (in the spectrum a flat
offset of about dt / T2* of the peak height) -- judge the correction on the spectrum, and give ``fit_basis`` a `skip`.
"""
from __future__ import annotations

import copy as _copy

import numpy as np

from .. import device as dev
from ..config import ATTRS, DIMS
from ..dims import _check_dims
from ..labeled import LabeledArray, as_labeled, like_input
from ._common import device_data


def readout_offsets(n_samples: int, readout_dwell: float, interleaves: int = 1, start: float = 0.0) -> np.ndarray:
    """``tau_s = start + (s mod (S / interleaves)) readout_dwell``: the acquisition delay of each of the S samples of
    `interleaves` equal interleaves played out one after the other from the same nominal time."""
    if isinstance(n_samples, bool) or not isinstance(n_samples, (int, np.integer)) or n_samples < 1:
        raise ValueError(f"n_samples must be a positive integer, got {n_samples!r}")
    if isinstance(interleaves, bool) or not isinstance(interleaves, (int, np.integer)) or interleaves < 1 \
            or n_samples % interleaves:
        raise ValueError(f"interleaves must be a positive integer that divides n_samples = {n_samples}, got {interleaves!r}")
    if not np.isfinite(readout_dwell) or not np.isfinite(start):
        raise ValueError(f"readout_dwell and start must be finite, got {readout_dwell!r} and {start!r}")
    return float(start) + (np.arange(int(n_samples)) % (int(n_samples) // int(interleaves))) * float(readout_dwell)


def _dwell(src, dim: str, dwell):
    if dwell is not None:
        try:
            dt = float(dwell)
        except (TypeError, ValueError):
            raise ValueError(f"dwell must be a positive number, got {dwell!r}") from None
        if not np.isfinite(dt) or dt <= 0:
            raise ValueError(f"dwell must be a finite positive number, got {dwell!r}")
        return dt
    c = src.coords.get(dim)
    axis = dev.uniform_axis(c.values) if c is not None and c.values.dtype.kind in "fiu" else None
    if axis is None or axis[1] <= 0:
        raise ValueError(f"dwell: the {dim!r} dim has no uniform ascending coordinate of at least two points to take the "
                         f"dwell from; pass dwell=")
    return axis[1]


def _length(pad_to, n: int) -> int:
    if pad_to is None:
        return n
    if isinstance(pad_to, bool) or not isinstance(pad_to, (int, np.integer)) or pad_to < n:
        raise ValueError(f"pad_to must be an integer >= the {n} points of the dim, got {pad_to!r}")
    return int(pad_to)


def _compact(phi: np.ndarray):
    """Delays shaped like the array without `dim` (broadcast, size-1 axes kept) -> (frac, n_delay, delay_div) of
    `device.shift_time`'s row rule ``frac[(r // delay_div) % n_delay]``: delays that vary along one axis only are
    passed as that axis' values, anything else as one delay per row."""
    lead = phi.shape
    varying = [a for a, s in enumerate(phi.strides) if s != 0 and lead[a] > 1]
    if not varying:
        return phi.reshape(-1)[:1].copy(), 1, 1
    if len(varying) == 1:
        a = varying[0]
        idx = [0] * len(lead)
        idx[a] = slice(None)
        return phi[tuple(idx)].copy(), lead[a], int(np.prod(lead[a + 1:], dtype=np.int64))
    return phi.reshape(-1).copy(), phi.size, 1


def _shift(src, tau, what: str, dim: str, pad_to, dwell, extra_attrs):
    """`tau`: delays shaped like `src` without `dim` (broadcastable).  Validation, then one device call."""
    n = src.sizes[dim]
    L = _length(pad_to, n)
    dt = _dwell(src, dim, dwell)
    lead = tuple(s for d, s in zip(src.dims, src.shape) if d != dim)
    if tau.dtype.kind not in "fiu" or not np.all(np.isfinite(tau)):
        raise ValueError(f"{what} must be finite real numbers")
    try:
        phi = np.broadcast_to(tau.astype(np.float64) / dt, lead)
    except ValueError:
        raise ValueError(f"{what}: shape {tau.shape} does not broadcast against the dims other than {dim!r}, {lead}") from None
    x, _ = device_data(src)  # complex; a real FID becomes complex as in remove_digital_filter
    if not np.any(phi):  # every delay exactly zero: a copy, no launch
        y = x.clone() if hasattr(x, "clone") else np.array(x)
    else:
        frac, n_delay, delay_div = _compact(phi)
        y = dev.shift_time(x, src.get_axis_num(dim), frac, n_delay, delay_div, L)
    attrs = _copy.copy(src.attrs)
    attrs[ATTRS.time_shift_pad_to] = L
    attrs.update(extra_attrs)
    return LabeledArray(y, src.dims, src.coords, attrs, src.name)


def shift_time(da, delay, dim: str = DIMS.time, pad_to=None, dwell=None):
    """Each row along `dim` evaluated `delay` earlier (module docstring), one fused launch where the transform length has
    an in-LDS plan.  `delay`: a scalar or an array that broadcasts against the other dims, in the unit of `dim`'s
    coordinate; the dwell comes from that coordinate, which must be uniform, or from `dwell`.  `pad_to`: the transform
    length L >= N (default N).  Real input becomes complex; dims, coordinates, name and attrs are kept and
    ``time_shift_pad_to`` is added; the result is device-resident for LabeledArray input."""
    src = as_labeled(da)
    _check_dims(src, (dim,), "shift_time")
    try:
        tau = np.asarray(delay)
        if tau.dtype.kind not in "fiu":
            raise TypeError
    except TypeError:
        raise ValueError(f"delay must be a real number or an array of them, got {delay!r}") from None
    return like_input(_shift(src, tau, "delay", dim, pad_to, dwell, {}), da)


def correct_readout_time(da, offsets, dim: str = DIMS.time, sample_dim: str = DIMS.sample, pad_to=None, dwell=None,
                         inverse: bool = False):
    """Undo the acquisition delay of each k-space sample of a non-Cartesian readout: ``shift_time`` with the delay
    ``offsets[s]`` (S values in the unit of `dim`'s coordinate, e.g. from `readout_offsets`) for sample s of
    `sample_dim`, whatever the order of the dims.  ``inverse=True`` applies ``-offsets``: the forward-model direction,
    and at ``pad_to=None`` the adjoint.  Adds the attrs ``time_shift_pad_to`` and ``readout_time_corrected``."""
    src = as_labeled(da)
    _check_dims(src, (dim, sample_dim), "correct_readout_time")
    if dim == sample_dim:
        raise ValueError(f"sample_dim: {sample_dim!r} is the dim that is shifted")
    off = np.asarray(offsets)
    S = src.sizes[sample_dim]
    if off.dtype.kind not in "fiu" or off.ndim != 1 or len(off) != S:
        raise ValueError(f"offsets must be {S} real numbers, one per point of {sample_dim!r}, got shape {off.shape} of {off.dtype}")
    others = [d for d in src.dims if d != dim]
    shape = [1] * len(others)
    shape[others.index(sample_dim)] = S
    tau = (-off if inverse else off).astype(np.float64).reshape(shape)
    out = _shift(src, tau, "offsets", dim, pad_to, dwell, {ATTRS.readout_time_corrected: not inverse})
    return like_input(out, da)
