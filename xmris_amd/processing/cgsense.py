"""``recon_cg_sense``: iterative SENSE (Pruessmann et al. 2001) for multi-coil, undersampled, non-Cartesian MRSI on the
GPU -- spirals, rings and radial readouts whose ``nufft_adjoint`` + ``combine_coils`` image would alias.

The definition is this backend's own (the reference has nothing here).  With the trajectory, matrix,
oversampling and width of ``nufft_adjoint`` (section 17), sensitivities s_c, density weights w (D = diag(w) per coil):

    (E x)_c = nufft_forward(s_c x),     E^H D y = sum_c conj(s_c) nufft_adjoint(y_c, density=w)
    solve (E^H D E + lambda I) x = E^H D y,   lambda = regularization (sum_j w_j / V) mean_p sum_c |s_c[p]|^2

the mean over the voxels whose sensitivity is not zero in every coil, V the number of voxels: the mean diagonal of the
normal matrix in closed form.  Plain conjugate gradients from x = 0, every column (time point, repetition ...) on its
own with its own scalars:

    b = E^H D y;  r = p = b;  rho = rho0 = |b|^2
    repeat `iterations` times, for a column whose status is still 0:
        if rho <= max(tol, 1e-14)^2 rho0:   status 1 (converged), freeze
        q = (E^H D E) p + lambda p;  delta = Re<p, q>
        if not (delta > 0 and finite):      status 2 (breakdown), freeze
        alpha = rho / delta;  x += alpha p;  r -= alpha q;  rho' = |r|^2;  p = r + (rho' / rho) p;  rho = rho'

and the first test once more at the end.  A column whose rho0 is not finite gets status 3 and a NaN image.  x, r, p, q,
the sensitivities and every scalar are complex128 / fp64; what is coil-sized is in the data's dtype.
"""
from __future__ import annotations

import copy as _copy

import numpy as np

from .. import device as dev
from ..config import ATTRS, DIMS
from ..dims import _check_dims
from ..labeled import Coordinate, LabeledArray, as_labeled, is_xarray, like_input
from ._common import device_data
from .coils import MAX_COILS, _linv
from .grid import (X_DIMS, _attrs, _fov, _image_tables, _label, _names, _readout, _to_samples, _to_voxels, _trajectory,
                   grid_table)
from .mrsi import _int, _per_dim

SCRATCH_BYTES = 1 << 30  # the default `chunk` keeps the oversampled grid of one pass at or below this


def _number(value, name: str) -> float:
    try:
        v = float(value)
    except (TypeError, ValueError):
        v = float("nan")
    if isinstance(value, bool) or not np.isfinite(v) or v < 0.0:
        raise ValueError(f"{name} must be a finite number >= 0, got {value!r}")
    return v


def _sens(sensitivities, coil_dim: str, d: int, c: int):
    """The maps as an array or tensor (C, m_0[, m_1[, m_2]]) in the order (coil_dim, x[, y[, z]]), as ``unfold_sense``
    takes them: a labelled array with those dims in any order, or array-like in that order."""
    names = X_DIMS[:d]
    if isinstance(sensitivities, LabeledArray) or is_xarray(sensitivities):
        s = as_labeled(sensitivities)
        order = (coil_dim, *names)
        if set(s.dims) != set(order) or len(s.dims) != len(order):
            raise ValueError(f"sensitivities: dims {s.dims} must be {order} in any order")
        vals = s.data
        perm = [s.get_axis_num(n) for n in order]
        vals = vals.permute(perm) if hasattr(vals, "detach") else np.transpose(np.asarray(vals), perm)
    else:
        vals = sensitivities if hasattr(sensitivities, "detach") else np.asarray(sensitivities)
    shape = tuple(int(n) for n in vals.shape)
    if len(shape) != d + 1 or shape[0] != c or min(shape) < 1:
        raise ValueError(f"sensitivities: shape {shape} in the order {(coil_dim, *names)} must be ({c}, m per trajectory "
                         f"dim): the data's {c} coils, then the matrix")
    return vals, shape[1:]


def default_chunk(n_coils: int, oversampled, itemsize: int, n_cols: int) -> int:
    """Columns per pass such that the oversampled grid, n_coils prod(G) chunk elements, stays within SCRATCH_BYTES
    (1 GiB); even where it is more than one, so that complex64 columns keep their 16-byte words."""
    per_col = int(n_coils) * int(np.prod(oversampled, dtype=np.int64)) * int(itemsize)
    chunk = max(1, min(int(n_cols), SCRATCH_BYTES // per_col))
    return chunk - chunk % 2 if 2 < chunk < n_cols else chunk


def normal_scale(sens_abs2_sum, weights, n_vox: int) -> float:
    """lambda / regularization: (sum_j w_j / V) x the mean of sum_c |s_c|^2 over the voxels where it is not zero."""
    live = sens_abs2_sum[sens_abs2_sum > 0]
    if len(live) == 0:
        return 0.0
    return float(np.sum(weights) / n_vox) * float(live.mean())


class _Problem:
    """What ``recon_cg_sense`` and ``recon_l1_sense`` share: the data as [C, S, T] in its dtype, the (whitened) maps [C, V]
    complex128 and their energy per voxel, the gridding table, the two chains on raw tensors, and what the result's
    dims, coordinates and attrs are made from."""


def _columns(chunk):
    if chunk is not None and (isinstance(chunk, bool) or not isinstance(chunk, (int, np.integer)) or chunk < 1):
        raise ValueError(f"chunk must be an integer >= 1, got {chunk!r}")


def _problem(who: str, da, trajectory, sensitivities, matrix, density, noise_cov, oversampling, width, dim, coil_dim, out_dim,
             fov, readout_time) -> _Problem:
    """Validates everything that describes the acquisition (before the library is reached) and uploads maps and tables
    once."""
    pb = _Problem()
    src0 = as_labeled(da)
    _check_dims(src0, (dim, coil_dim), who)
    if dim == coil_dim:
        raise ValueError(f"coil_dim: {coil_dim!r} is the sample dim")
    c = src0.sizes[coil_dim]
    if not 1 <= c <= MAX_COILS:
        raise ValueError(f"coil_dim: {c} coils along {coil_dim!r}, supported are 1 ... {MAX_COILS}")
    k = _trajectory(trajectory)
    d = k.shape[1]
    if k.shape[0] != src0.sizes[dim]:
        raise ValueError(f"trajectory: {k.shape[0]} samples for a {dim!r} dim of {src0.sizes[dim]} points")
    sens, spatial = _sens(sensitivities, coil_dim, d, c)
    if matrix is not None:
        mat = _per_dim(matrix, d, "matrix", _int)
        if mat is None or tuple(mat) != tuple(spatial):
            raise ValueError(f"matrix: {matrix!r} disagrees with the sensitivities' spatial shape {tuple(spatial)}")
    rest = [n for n in src0.dims if n not in (dim, coil_dim)]
    names = _names(out_dim, d, X_DIMS, "out_dim", rest)
    f = _fov(fov, d)
    linv = None if noise_cov is None else _linv(noise_cov, c)
    t = grid_table(k, spatial, oversampling, width, density)
    pb.da, pb.dim, pb.coil_dim, pb.density = da, dim, coil_dim, density
    pb.c, pb.spatial, pb.rest, pb.names, pb.fov, pb.table = c, tuple(spatial), rest, names, f, t
    pb.sens, pb.linv = sens, linv
    return pb


def _upload(pb: _Problem, readout_time, arrange=None) -> _Problem:
    """The second half of the set-up, which reaches the library: the data in the order (coil, sample, columns), the maps
    and the tables on the device, the whitening.  `arrange` (``recon_subspace``): takes the data as (coil, sample, *rest)
    and returns it as the caller's kernels want it, with the column count and the sizes `_result` reshapes to, in place
    of the contiguous [C, S, columns]."""
    da, dim, coil_dim, c, spatial, rest, t, sens, linv = (pb.da, pb.dim, pb.coil_dim, pb.c, pb.spatial, pb.rest, pb.table,
                                                          pb.sens, pb.linv)
    da_t = _readout(da, readout_time, dim, False)
    src = as_labeled(da_t)
    y, _ = device_data(src)
    on_device = hasattr(y, "detach")
    perm = [src.get_axis_num(coil_dim), src.get_axis_num(dim)] + [src.get_axis_num(n) for n in rest]
    if perm != list(range(src.ndim)):
        y = y.permute(perm) if on_device else np.transpose(y, perm)
    cols = tuple(int(n) for n in y.shape[2:])
    n_samples, n_cols, n_vox = int(len(t.density)), int(np.prod(cols, dtype=np.int64)), int(np.prod(spatial))
    if n_cols < 1:
        raise ValueError(f"da: an empty dimension among {tuple(rest)}")
    if arrange is None:
        y = y.reshape(c, n_samples, n_cols)
        y = y.contiguous() if on_device else np.ascontiguousarray(y)
    else:
        y, n_cols = arrange(y, on_device)

    # the maps: complex128 on the device, [C, V]; whitening is one axis_dft along the coil axis of maps and data
    if on_device:
        import torch

        s = (sens if hasattr(sens, "detach") else torch.from_numpy(np.array(sens, dtype=np.complex128, order="C")))
        s = s.to(device=y.device, dtype=torch.complex128).reshape(c, n_vox).contiguous()
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.complex128)).to(y.device)  # noqa: E731
    else:
        s = np.array(sens, dtype=np.complex128, order="C").reshape(c, n_vox)
        up = lambda a: np.ascontiguousarray(a, dtype=np.complex128)  # noqa: E731
    if linv is not None:
        white = up(linv)
        s = dev.axis_dft(s, 0, white)
        y = dev.axis_dft(y, 0, white)
    energy = s.real ** 2 + s.imag ** 2
    energy = energy.sum(dim=0).cpu().numpy() if on_device else energy.sum(axis=0)

    # the tables of both chains go up once; SparseTable keeps its own device copy
    to_voxels, to_samples = [up(a) for a in _image_tables(t, 1.0)], [up(a) for a in _image_tables(t, -1.0)]

    def adjoint(v):  # [C, S, T] -> [C, V, T]
        g = dev.axis_sparse(v, 1, t.grid)
        return _to_voxels(g, 1, t, to_voxels).reshape(c, n_vox, v.shape[2])

    def forward(u):  # [C, V, T] -> [C, S, T]
        return _to_samples(u.reshape((c,) + tuple(spatial) + (u.shape[2],)), 1, t, to_samples)

    pb.src, pb.y, pb.s, pb.energy, pb.on_device, pb.cols = src, y, s, energy, on_device, cols
    pb.n_cols, pb.n_vox, pb.adjoint, pb.forward = n_cols, n_vox, adjoint, forward
    return pb


def _passes(pb: _Problem, chunk, run):
    """``run(columns of y)`` per pass of `chunk` columns (default: `default_chunk`)."""
    y, n_cols, on_device = pb.y, pb.n_cols, pb.on_device
    step = default_chunk(pb.c, pb.table.oversampled, y.dtype.itemsize if not on_device else y.element_size(), n_cols) \
        if chunk is None else int(chunk)
    parts = []
    for t0 in range(0, n_cols, step):
        yk = y if step >= n_cols else y[:, :, t0:t0 + step]
        if step < n_cols:
            yk = yk.contiguous() if on_device else np.ascontiguousarray(yk)
        parts.append(run(yk))
    return parts


def _result(pb: _Problem, parts, own_attrs: dict, info_names, return_info: bool, info_dims=None, extra=None):
    """The image (and with `return_info` the dataset) from the raw outputs of the passes.  `info_dims`: the dims of the
    per-column outputs where they are not all of `rest`; `extra(joined, coords)`: further variables of the dataset."""
    da, src, dim, coil_dim, spatial, cols, rest, names, on_device = (pb.da, pb.src, pb.dim, pb.coil_dim, pb.spatial, pb.cols,
                                                                     pb.rest, pb.names, pb.on_device)

    def joined(name, axis):
        vals = [getattr(p, name) for p in parts]
        if len(vals) == 1:
            return vals[0]
        if on_device:
            import torch

            return torch.cat(vals, dim=axis)
        return np.concatenate(vals, axis=axis)

    # the image: (x, y, z, columns) -> the input's order without the coil dim, the image dims in place of `dim`
    img = joined("x", 1).reshape(tuple(spatial) + cols)
    out_dims = []
    for n in src.dims:
        if n != coil_dim:
            out_dims.extend(names if n == dim else (n,))
    have = list(names) + rest
    order = [have.index(n) for n in out_dims]
    if order != list(range(len(have))):
        img = img.permute(order).contiguous() if on_device else np.ascontiguousarray(np.transpose(img, order))
    coords = {key: co for key, co in src.coords.items() if co.dim not in (dim, coil_dim)}
    for a, n in enumerate(names):
        coords[n] = Coordinate(n, (np.arange(spatial[a]) - spatial[a] // 2) * pb.fov[a] / spatial[a], {})
    attrs = _attrs(src, names, pb.table, _label(pb.density))
    attrs.update(own_attrs)
    image = LabeledArray(img, out_dims, coords, attrs, src.name)
    if not return_info:
        return like_input(image, da)
    from ..fitting.dataset import LabeledDataset

    if info_dims is not None:
        rest, cols = list(info_dims), tuple(src.sizes[n] for n in info_dims)
    col_coords = {key: co for key, co in coords.items() if co.dim in rest}
    info = {name: LabeledArray(joined(name, 0).reshape(cols), rest, col_coords) for name in info_names}
    if extra is not None:
        info.update(extra(joined, coords))
    ds = LabeledDataset(dict(image=image, **info), _copy.copy(attrs))
    return ds.to_xarray() if is_xarray(da) else ds


def recon_cg_sense(da, trajectory, sensitivities, matrix=None, iterations: int = 20, tol: float = 1e-6,
                   regularization: float = 0.0, density=None, noise_cov=None, oversampling: float = 2.0, width: int = 4,
                   dim: str = DIMS.sample, coil_dim: str = DIMS.coil, out_dim=None, fov=1.0, readout_time=None,
                   chunk=None, return_info: bool = False):
    """CG-SENSE reconstruction of the non-Cartesian multi-coil samples `da` (module docstring).
    `trajectory`, `oversampling`, `width`, `density` (None, S weights or ``"pipe"``), `fov`, `out_dim` and `readout_time`
    as in ``nufft_adjoint``; `sensitivities`: the dims ``(coil_dim, x[, y[, z]])`` in any order, or array-like in that
    order, C <= 64 coils; a voxel whose sensitivity is zero in every coil stays exactly 0.  `matrix` defaults to the
    sensitivities' spatial shape.  `noise_cov`: a C x C Hermitian positive-definite matrix; data and maps are whitened
    once in front.  `regularization`: Tikhonov weight relative to the mean diagonal of the normal matrix.  `iterations`:
    the cap; `tol`: a column stops at ``|r| <= max(tol, 1e-14) |b|``.  Every dim but `dim` and `coil_dim` is a column;
    data that is not in the order (coil, sample, columns) costs one permuting copy.  `chunk`: columns per pass; the
    default keeps the oversampled grid of a pass, C prod(G) chunk elements, within 1 GiB.  Results do not depend on it.

    Returns the image (complex128) without `coil_dim` and with `dim` replaced in place by ``x[, y[, z]]`` (or
    `out_dim`), coordinates as in ``nufft_adjoint``, other coords and attrs kept, plus the ``grid_*`` attrs and
    ``cgsense_iterations``, ``cgsense_tol``, ``cgsense_regularization``; device-resident for LabeledArray input.  With
    `return_info` a dataset of ``image``, ``residual`` (sqrt(rho / rho0)), ``iterations`` and ``status`` (0 iteration
    cap, 1 converged, 2 breakdown, 3 not finite) over the column dims."""
    if isinstance(iterations, bool) or not isinstance(iterations, (int, np.integer)) or iterations < 0:
        raise ValueError(f"iterations must be an integer >= 0, got {iterations!r}")
    tol = _number(tol, "tol")
    reg = _number(regularization, "regularization")
    _columns(chunk)
    pb = _problem("recon_cg_sense", da, trajectory, sensitivities, matrix, density, noise_cov, oversampling, width, dim,
                  coil_dim, out_dim, fov, readout_time)
    _upload(pb, readout_time)
    lam = reg * normal_scale(pb.energy, pb.table.density, pb.n_vox)
    parts = _passes(pb, chunk, lambda yk: dev.cg_sense(yk, pb.s, pb.adjoint, pb.forward, lam, int(iterations), tol))
    own = {ATTRS.cgsense_iterations: int(iterations), ATTRS.cgsense_tol: tol, ATTRS.cgsense_regularization: reg}
    return _result(pb, parts, own, ("residual", "iterations", "status"), return_info)
