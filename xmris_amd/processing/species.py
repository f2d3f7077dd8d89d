"""``separate_species`` / ``simulate_echoes`` / ``species_matrix``: least-squares separation of chemical species from a
few echoes on the GPU (IDEAL-type spiral CSI, multi-echo EPI / bSSFP, Dixon-type X-nuclei imaging; Reeder 2004,
Wiesinger 2012), the route from multi-echo acquisitions to the amplitudes that ``fit_kinetics`` takes.

The definition is this backend's own (the reference has nothing here).  E echoes at TE_e, M
species of frequency f_m (Hz) and decay R_m (1/s).  A row r -- every index of the dims that are neither `dim` nor in
`share` -- has a readout delay tau_r and a field offset psi_r, and each of its columns c (the `share` dims) follows

    y[e, c] = sum_m rho[m, c] exp((2 pi i f_m - R_m) t_e) exp(2 pi i psi_r t_e),    t_e = TE_e + tau_r

With A0[e, m] = exp((2 pi i f_m - R_m) TE_e) and P0 = pinv(A0), shared by all rows,

    rho[m, c] = exp(-(2 pi i f_m - R_m) tau_r) sum_e P0[m, e] exp(-2 pi i psi_r t_e) y[e, c]

``fit_field=True`` finds psi_r per row by variable projection from all columns of the row, within +-`max_field` Hz: the
maximum of G(psi) = || Q^H D(psi)^H y ||^2 (Q: an orthonormal basis of range(A0)), a coarse grid of spacing
1 / (4 (max TE - min TE)) and a safeguarded Newton iteration.  G repeats every 1 / dTE for uniform echoes and has side
lobes where psi moves one species onto another: `max_field` is the caller's statement of how far the field can be off;
neither is detected.
"""
from __future__ import annotations

import copy as _copy

import numpy as np

from .. import device as dev
from ..config import ATTRS, DIMS
from ..dims import _check_dims
from ..labeled import Coordinate, LabeledArray, as_labeled, is_xarray, like_input
from ._common import device_data

RANK_TOL = 1e-8  # smallest / largest singular value of A0 below which the species cannot be told apart


def _species_args(frequencies, decay):
    """(names, f, R) of a mapping name -> Hz or a sequence of Hz (names "s0", "s1", ...)."""
    if hasattr(frequencies, "items"):
        names = [str(k) for k in frequencies]
        vals = list(frequencies.values())
    else:
        vals = list(np.atleast_1d(np.asarray(frequencies)).reshape(-1))
        names = [f"s{i}" for i in range(len(vals))]
    try:
        f = np.array([float(v) for v in vals], dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"frequencies must be real numbers in Hz, got {frequencies!r}") from None
    if f.size < 1 or not np.all(np.isfinite(f)):
        raise ValueError(f"frequencies must be at least one finite number in Hz, got {frequencies!r}")
    if decay is None:
        r = np.zeros_like(f)
    else:
        if hasattr(decay, "items"):
            if set(map(str, decay)) - set(names):
                raise ValueError(f"decay names {sorted(set(map(str, decay)) - set(names))} that are not in frequencies {names}")
            decay = [dict((str(k), v) for k, v in decay.items()).get(n, 0.0) for n in names]
        r = np.broadcast_to(np.asarray(decay, dtype=np.float64), f.shape).copy() if np.ndim(decay) == 0 \
            else np.asarray(decay, dtype=np.float64).reshape(-1)
        if r.shape != f.shape or not np.all(np.isfinite(r)) or np.any(r < 0):
            raise ValueError(f"decay must be one finite rate >= 0 (1/s) per species ({f.size}), got {decay!r}")
    return names, f, r


def _echo_times(echo_times):
    te = np.asarray(echo_times, dtype=np.float64).reshape(-1)
    if not np.all(np.isfinite(te)):
        raise ValueError("echo_times must be finite (seconds)")
    if len(np.unique(te)) != len(te):
        raise ValueError(f"echo_times must be distinct, got {te.tolist()}")
    return te


def species_matrix(frequencies, echo_times, decay=None) -> np.ndarray:
    """A0[e, m] = exp((2 pi i f_m - R_m) TE_e), complex128 [E, M]."""
    _, f, r = _species_args(frequencies, decay)
    te = _echo_times(echo_times)
    return np.exp((2j * np.pi * f - r)[None, :] * te[:, None])


def species_nsa(a0: np.ndarray) -> np.ndarray:
    """nsa[m] = 1 / [(A0^H A0)^-1]_mm: the effective number of averages of each species' estimate."""
    return 1.0 / np.real(np.diagonal(np.linalg.inv(a0.conj().T @ a0)))


def _check_model(names, f, te, a0, fit_field: bool):
    E, M = a0.shape
    if E < 2:
        raise ValueError(f"separate_species needs at least 2 echoes, got {E}")
    if E > dev.SPECIES_MAX_ECHOES:
        raise ValueError(f"at most {dev.SPECIES_MAX_ECHOES} echoes are supported, got {E}")
    if M > dev.SPECIES_MAX_SPECIES:
        raise ValueError(f"at most {dev.SPECIES_MAX_SPECIES} species are supported, got {M}")
    if M > E:
        raise ValueError(f"{M} species cannot be separated from {E} echoes (needs M <= E)")
    sv = np.linalg.svd(a0, compute_uv=False)
    if not sv[-1] > RANK_TOL * sv[0]:
        i, j = 0, 0
        if M > 1:
            d = np.abs(f[:, None] - f[None, :]) + np.diag(np.full(M, np.inf))
            i, j = np.unravel_index(np.argmin(d), d.shape)
        raise ValueError(f"frequencies: the species cannot be told apart from these echoes (smallest / largest singular "
                         f"value of A0 = {sv[-1] / sv[0]:.2e} <= {RANK_TOL:g}); the closest are {names[i]!r} ({f[i]:g} Hz) "
                         f"and {names[j]!r} ({f[j]:g} Hz), the echoes span {te.max() - te.min():g} s")
    if fit_field:
        if M >= E:
            raise ValueError(f"fit_field needs fewer species than echoes, got {M} species and {E} echoes")
        if E > dev.SPECIES_MAX_ECHOES_FIT:
            raise ValueError(f"fit_field takes at most {dev.SPECIES_MAX_ECHOES_FIT} echoes, got {E}")


def _per_row(value, what: str, row_dims, row_shape, forbidden):
    """An array or LabeledArray over a subset of the row dims -> fp64 host array that broadcasts against the row dims."""
    if isinstance(value, LabeledArray) or is_xarray(value):
        la = as_labeled(value)
        bad = [d for d in la.dims if d in forbidden]
        if bad:
            raise ValueError(f"{what}: dim {bad[0]!r} is the echo dim or one of the shared (column) dims; the field is per row")
        extra = [d for d in la.dims if d not in row_dims]
        if extra:
            raise ValueError(f"{what}: dim {extra[0]!r} is not a dim of the data; the row dims are {list(row_dims)}")
        v = np.asarray(la.values, dtype=np.float64)
        have = [d for d in row_dims if d in la.dims]
        v = np.transpose(v, [la.dims.index(d) for d in have])
        v = v.reshape([la.sizes[d] if d in la.dims else 1 for d in row_dims])
    else:
        v = np.asarray(value)
        if v.dtype.kind not in "fiu":
            raise ValueError(f"{what} must be real numbers, got dtype {v.dtype}")
        v = v.astype(np.float64)
    try:
        np.broadcast_to(v, row_shape)
    except ValueError:
        raise ValueError(f"{what}: shape {v.shape} does not broadcast against the row dims {dict(zip(row_dims, row_shape))}") from None
    if v.ndim < len(row_shape):
        v = v.reshape((1,) * (len(row_shape) - v.ndim) + v.shape)
    return v


def separate_species(da, frequencies, echo_times=None, dim: str = DIMS.echo, out_dim: str = DIMS.species, decay=None,
                     readout_time=None, sample_dim: str = DIMS.sample, field_map=None, fit_field: bool = False,
                     max_field=None, share=(DIMS.coil,), return_field: bool = False):
    """Species amplitudes from the echoes along `dim` (module docstring), one launch of ``xm_species_separate``.
    `frequencies`: a mapping name -> Hz, or a sequence (names "s0", "s1", ...); the names label the `out_dim`
    coordinate.  `echo_times` (s): default the coordinate of `dim`.  `decay`: R_m in 1/s per species (default 0).
    `readout_time`: one delay tau (s) per entry of `sample_dim`, the convention of ``grid_kspace`` -- the k-space form,
    in front of ``nufft_adjoint`` / ``recon_cg_sense``.  `field_map`: psi in Hz, an array that broadcasts against the row
    dims or a LabeledArray over a subset of them; or ``fit_field=True`` with `max_field` (Hz) to fit it per row from all
    columns of the row.  `share`: the dims that are columns of a row (those the data does not have are ignored); every
    other dim but `dim` is a row dim.  The data are addressed where they lie when the row dims collapse into two strided
    levels and the column dims into two, which ``[repetition, echo, coil, sample]`` and ``[echo, coil, x, y]`` do; any
    other layout costs one contiguous copy.
    Returns the input with `dim` replaced by `out_dim`, in the input's dtype (real input becomes complex), other dims,
    coords and attrs kept, plus the attrs ``species_frequencies``, ``species_echo_times``, ``species_decay``,
    ``species_nsa``, ``species_field`` ('none', 'given' or 'fitted') and ``species_max_field``; device-resident for
    LabeledArray input.  With `return_field` a dataset of ``species``, ``field`` (Hz), ``status`` (0 done, 1 the window's
    end, 2 non-finite sample, delay or field, 3 all-zero row, 4 step cap) and, with `fit_field`, ``residual`` (the share
    of the row's energy that the model leaves)."""
    src = as_labeled(da)
    _check_dims(src, (dim,), "separate_species")
    names, f, r = _species_args(frequencies, decay)
    if echo_times is None:
        c = src.coords.get(dim)
        if c is None or c.dim != dim or np.asarray(c.values).dtype.kind not in "fiu":
            raise ValueError(f"echo_times: the {dim!r} dim has no numeric coordinate to take the echo times from; pass echo_times=")
        echo_times = c.values
    te = _echo_times(echo_times)
    E = src.sizes[dim]
    if len(te) != E:
        raise ValueError(f"echo_times: {len(te)} values for the {E} points of {dim!r}")
    a0 = np.exp((2j * np.pi * f - r)[None, :] * te[:, None])
    if fit_field and field_map is not None:
        raise ValueError("field_map and fit_field exclude each other (a fit around a given map is not supported)")
    _check_model(names, f, te, a0, bool(fit_field))
    share = (share,) if isinstance(share, str) else tuple(share)
    if dim in share:
        raise ValueError(f"share: {dim!r} is the echo dim")
    if out_dim != dim and out_dim in src.dims:
        raise ValueError(f"out_dim: the data already has a dim {out_dim!r}")
    col_dims = tuple(d for d in src.dims if d in share)
    row_dims = tuple(d for d in src.dims if d != dim and d not in col_dims)
    row_shape = tuple(src.sizes[d] for d in row_dims)

    tau = None
    if readout_time is not None:
        _check_dims(src, (sample_dim,), "separate_species")
        if sample_dim not in row_dims:
            raise ValueError(f"sample_dim: {sample_dim!r} is the echo dim or one of the shared (column) dims {list(share)}")
        rt = np.asarray(readout_time)
        S = src.sizes[sample_dim]
        if rt.dtype.kind not in "fiu" or rt.ndim != 1 or len(rt) != S:
            raise ValueError(f"readout_time must be {S} real numbers, one per point of {sample_dim!r}, got shape {rt.shape} of {rt.dtype}")
        shape = [1] * len(row_dims)
        shape[row_dims.index(sample_dim)] = S
        tau = rt.astype(np.float64).reshape(shape)
    psi = None
    if field_map is not None:
        psi = _per_row(field_map, "field_map", row_dims, row_shape, (dim,) + col_dims)
    if fit_field:
        if max_field is None:
            raise ValueError("fit_field needs max_field, the largest field offset in Hz that the fit may find")
        try:
            max_field = float(max_field)
        except (TypeError, ValueError):
            raise ValueError(f"max_field must be a positive number (Hz), got {max_field!r}") from None
        if not (np.isfinite(max_field) and max_field > 0):
            raise ValueError(f"max_field must be finite and positive (Hz), got {max_field!r}")
        delta, g = dev.species_grid(te, max_field)
        if 2 * g + 1 > dev.SPECIES_MAX_GRID:
            raise ValueError(f"max_field: the coarse grid of {2 * g + 1} points (spacing {delta:g} Hz = 1 / (4 x the echo span)) "
                             f"exceeds {dev.SPECIES_MAX_GRID}; lower max_field")

    x, _ = device_data(src)
    res = dev.species_separate(x, src.get_axis_num(dim), [src.get_axis_num(d) for d in col_dims], te, f, r, tau=tau,
                               psi=psi, fit_field=bool(fit_field), max_field=max_field if fit_field else None)

    attrs = _copy.copy(src.attrs)
    attrs[ATTRS.species_frequencies] = dict(zip(names, f.tolist()))
    attrs[ATTRS.species_echo_times] = te.tolist()
    attrs[ATTRS.species_decay] = r.tolist()
    attrs[ATTRS.species_nsa] = species_nsa(a0).tolist()
    attrs[ATTRS.species_field] = "fitted" if fit_field else "given" if field_map is not None else "none"
    if fit_field:
        attrs[ATTRS.species_max_field] = max_field
    dims = tuple(out_dim if d == dim else d for d in src.dims)
    coords = {k: c_ for k, c_ in src.coords.items() if c_.dim != dim}
    coords[out_dim] = Coordinate(out_dim, np.array(names), {"long_name": DIMS.species.long_name})
    out = LabeledArray(res.species, dims, coords, attrs, src.name)
    if not return_field:
        return like_input(out, da)
    from ..fitting.dataset import LabeledDataset

    pcoords = {k: c_ for k, c_ in src.coords.items() if c_.dim in row_dims}
    ds = {"species": out, "field": LabeledArray(res.field, row_dims, pcoords),
          "status": LabeledArray(res.status, row_dims, pcoords)}
    if fit_field:
        ds["residual"] = LabeledArray(res.residual, row_dims, pcoords)
    ds = LabeledDataset(ds, attrs)
    return ds.to_xarray() if is_xarray(da) else ds


def _forward(rho, axis: int, f, r, te, tau, psi):
    """y with the echoes at `axis`: rho [.., M, ..] complex128, tau and psi broadcast against rho without `axis`."""
    rho = np.moveaxis(np.asarray(rho, dtype=np.complex128), axis, 0)  # [M, rest...]
    rest = rho.shape[1:]
    tau = np.broadcast_to(np.zeros(()) if tau is None else tau, rest)
    psi = np.broadcast_to(np.zeros(()) if psi is None else psi, rest)
    y = np.zeros((len(te),) + rest, dtype=np.complex128)
    for e, t0 in enumerate(te):
        t = t0 + tau
        for m in range(len(f)):
            y[e] += rho[m] * np.exp((2j * np.pi * f[m] - r[m]) * t)
        y[e] *= np.exp(2j * np.pi * psi * t)
    return np.moveaxis(y, 0, axis)


def simulate_echoes(species, frequencies, echo_times, decay=None, readout_time=None, field_map=None,
                    dim: str = DIMS.species, out_dim: str = DIMS.echo, sample_dim: str = DIMS.sample, axis: int = 0):
    """The forward model of ``separate_species`` in host numpy fp64, for tests and the quick start.  `species`: a
    LabeledArray / DataArray with the species along `dim` (replaced by `out_dim` with the echo times as its coordinate;
    `readout_time` runs along `sample_dim`, `field_map` broadcasts against the other dims or is a LabeledArray over a
    subset of them), or a plain array with the species along `axis` (`readout_time` and `field_map` then broadcast
    against the array without that axis).  Returns complex128 host data in the input's container type."""
    names, f, r = _species_args(frequencies, decay)
    te = _echo_times(echo_times)
    if not (isinstance(species, LabeledArray) or is_xarray(species)):
        rho = np.asarray(species)
        if rho.shape[axis] != len(f):
            raise ValueError(f"species has {rho.shape[axis]} entries along axis {axis}, frequencies names {len(f)}")
        tau = None if readout_time is None else np.asarray(readout_time, dtype=np.float64)
        psi = None if field_map is None else np.asarray(field_map, dtype=np.float64)
        return _forward(rho, axis, f, r, te, tau, psi)
    src = as_labeled(species)
    _check_dims(src, (dim,), "simulate_echoes")
    if src.sizes[dim] != len(f):
        raise ValueError(f"{dim!r} has {src.sizes[dim]} entries, frequencies names {len(f)}")
    rest = tuple(d for d in src.dims if d != dim)
    rest_shape = tuple(src.sizes[d] for d in rest)
    tau = None
    if readout_time is not None:
        _check_dims(src, (sample_dim,), "simulate_echoes")
        rt = np.asarray(readout_time, dtype=np.float64)
        if rt.ndim != 1 or len(rt) != src.sizes[sample_dim] or sample_dim == dim:
            raise ValueError(f"readout_time must be {src.sizes.get(sample_dim)} real numbers, one per point of {sample_dim!r}")
        shape = [1] * len(rest)
        shape[rest.index(sample_dim)] = len(rt)
        tau = rt.reshape(shape)
    psi = None if field_map is None else _per_row(field_map, "field_map", rest, rest_shape, (dim,))
    y = _forward(src.values, src.get_axis_num(dim), f, r, te, tau, psi)
    dims = tuple(out_dim if d == dim else d for d in src.dims)
    coords = {k: c_ for k, c_ in src.coords.items() if c_.dim != dim}
    coords[out_dim] = Coordinate(out_dim, te, {"long_name": DIMS.echo.long_name, "units": "s"})
    return like_input(LabeledArray(y, dims, coords, _copy.copy(src.attrs), src.name), species)
