"""``grid_kspace`` / ``degrid_kspace`` / ``nufft_adjoint`` / ``nufft_forward``: non-Cartesian MRSI on the GPU, the step in
front of ``to_image`` for spiral, radial, concentric-ring, rosette and ramp-sampled readouts.

The definition is this backend's own (the reference has nothing here).  `trajectory` is [S, d]
real, d = 1 ... 3, in cycles per field of view, k in [-m/2, m/2] per dim for the target matrix m; it is the same for
every time point and every other dim (per-sample time offsets within a readout: the keyword `readout_time`,
``processing/timeshift.py``).  Per dim:

    G = the smallest even integer >= oversampling m,  alpha = G / m,  W = width <= G
    beta = pi sqrt((W / alpha)^2 (alpha - 1/2)^2 - 0.8)                                   (Beatty et al. 2005)
    KB(u) = I0(beta sqrt(1 - (2 u / W)^2)) / I0(beta)
    u_j = k_j G / m + G // 2,   cells g = ceil(u_j - W / 2) + 0 ... W - 1, each mod G     (-W/2 <= g - u < W/2)

Gridding is the sparse matrix A[cell, j] = dens_j prod_a KB(g_a - u_ja), cell the C-order flat index over (kx, ky, kz),
each row's entries in ascending j; degridding is A^T with unit density, each row's entries in ascending cell.  Both are
one launch of ``xm_axis_sparse`` on the tensor where it lies.  ``nufft_adjoint`` is gridding, then per dim the [m, G]
table

    F[p][g] = c[p] exp(2 pi i (g - G // 2) (p - m // 2) / G) / sqrt(G)
    c[p] = sqrt(G / m) I0(beta) z / (W sinh z),   z = sqrt(beta^2 - (pi W (p - m // 2) / G)^2)  (complex square root)

-- the centred transform, the crop to m and the de-apodisation in one ``xm_axis_dft`` launch (G <= 64; a larger G runs
the centred transform of ``to_image`` on G, the crop and the product with c).  It approximates
(1 / sqrt(m^d)) sum_j dens_j x_j exp(2 pi i k_j (p - m // 2) / m); ``nufft_forward`` is the transposed chain.
"""
from __future__ import annotations

import copy as _copy
from collections import namedtuple

import numpy as np

from .. import device as dev
from ..config import ATTRS, DIMS
from ..dims import _check_dims
from ..labeled import Coordinate, LabeledArray, as_labeled, like_input
from ._common import device_data
from .mrsi import _float, _int, _per_dim, _unit

K_DIMS = (DIMS.kx, DIMS.ky, DIMS.kz)
X_DIMS = (DIMS.x, DIMS.y, DIMS.z)
PIPE_ITERATIONS = 10

GridTable = namedtuple("GridTable", "grid degrid oversampled beta deapodization matrix width density")
GridTable.__doc__ = """What `grid_table` returns: `grid` ([cells, S]) and `degrid` ([S, cells]) as `SparseTable`s, and per
dim `oversampled` (G), `beta`, `deapodization` (c, m values), `matrix` (m); `width`; `density`: the S weights in `grid`."""


def oversampled(m: int, oversampling: float) -> int:
    """The smallest even integer >= oversampling m."""
    return 2 * int(np.ceil(oversampling * m / 2.0))


def kb_beta(width: int, alpha: float) -> float:
    return float(np.pi * np.sqrt((width / alpha) ** 2 * (alpha - 0.5) ** 2 - 0.8))


def kb(t, width: int, beta: float):
    """KB(t) on |t| <= W / 2."""
    return np.i0(beta * np.sqrt(np.maximum(1.0 - (2.0 * t / width) ** 2, 0.0))) / np.i0(beta)


def deapodization(m: int, G: int, width: int, beta: float) -> np.ndarray:
    """c of the module docstring, m fp64 values."""
    t = np.pi * width * (np.arange(m) - m // 2) / G
    z = np.sqrt((beta * beta - t * t).astype(np.complex128))
    small = np.abs(z) < 1e-8  # z / sinh z -> 1
    ratio = np.where(small, 1.0, z / np.where(small, 1.0, np.sinh(z)))
    return np.sqrt(G / m) * np.i0(beta) * ratio.real / width


def _geometry(matrix, oversampling, width, d: int):
    mat = _per_dim(matrix, d, "matrix", _int)
    if mat is None or any(m < 1 for m in mat):
        raise ValueError(f"matrix must be a positive integer or one per dim, got {matrix!r}")
    try:
        a0 = float(oversampling)
    except (TypeError, ValueError):
        raise ValueError(f"oversampling must be a number >= 1, got {oversampling!r}") from None
    if not np.isfinite(a0) or a0 < 1.0:
        raise ValueError(f"oversampling must be a finite number >= 1, got {oversampling!r}")
    if isinstance(width, bool) or not isinstance(width, (int, np.integer)) or not 2 <= int(width) <= 8:
        raise ValueError(f"width must be an integer 2 ... 8, got {width!r}")
    W = int(width)
    Gs = tuple(oversampled(m, a0) for m in mat)
    for m, G in zip(mat, Gs):
        if W > G:
            raise ValueError(f"width: {W} cells do not fit the oversampled grid of {G} (matrix {m}, oversampling {a0})")
    return mat, Gs, W


def _trajectory(trajectory):
    k = np.asarray(trajectory)
    if k.dtype.kind not in "fiu" or k.ndim != 2 or not 1 <= k.shape[1] <= 3 or k.shape[0] < 1:
        raise ValueError(f"trajectory must be [S, d] real with S >= 1 and d = 1 ... 3, got shape {k.shape} of {k.dtype}")
    k = k.astype(np.float64)
    if not np.all(np.isfinite(k)):
        raise ValueError(f"trajectory: sample {int(np.flatnonzero(~np.isfinite(k).all(axis=1))[0])} is not finite")
    return k


def _footprint(k, mat, Gs, W):
    """(cells [S, W^d] int64 C-order flat indices, kb [S, W^d] products of KB, betas) from fp64 host arithmetic."""
    S, d = k.shape
    cells = np.zeros((S, 1), dtype=np.int64)
    prod = np.ones((S, 1))
    betas = []
    for a, (m, G) in enumerate(zip(mat, Gs)):
        far = np.abs(k[:, a]) > m / 2.0
        if far.any():
            j = int(np.flatnonzero(far)[0])
            raise ValueError(f"trajectory: sample {j} has k = {k[j, a]!r} along dim {a}, outside [-{m / 2}, {m / 2}]")
        beta = kb_beta(W, G / m)
        betas.append(beta)
        u = k[:, a] * G / m + G // 2
        g = np.ceil(u - W / 2.0)[:, None] + np.arange(W)[None, :]  # [S, W]
        w = kb(g - u[:, None], W, beta)
        g = np.mod(g.astype(np.int64), G)
        cells = (cells[:, :, None] * G + g[:, None, :]).reshape(S, -1)
        prod = (prod[:, :, None] * w[:, None, :]).reshape(S, -1)
    return cells, prod, tuple(betas)


def _pipe(cells, prod, n_cells: int, iterations: int) -> np.ndarray:
    """Pipe-Menon: w <- w / (A1^T A1 w) from w = 1, A1 the unit-density gridding matrix."""
    w = np.ones(cells.shape[0])
    for _ in range(iterations):
        g = np.bincount(cells.ravel(), weights=(prod * w[:, None]).ravel(), minlength=n_cells)
        w = w / (prod * g[cells]).sum(axis=1)
    return w


def _density(density, cells, prod, n_cells: int, iterations: int):
    S = cells.shape[0]
    if density is None:
        return np.ones(S), "none"
    if isinstance(density, str):
        if density != "pipe":
            raise ValueError(f"density: unknown name {density!r}; give None, 'pipe' or {S} real weights")
        if isinstance(iterations, bool) or not isinstance(iterations, (int, np.integer)) or iterations < 0:
            raise ValueError(f"iterations must be an integer >= 0, got {iterations!r}")
        return _pipe(cells, prod, n_cells, int(iterations)), "pipe"
    w = np.asarray(density)
    if w.ndim != 1 or w.dtype.kind not in "fiu" or len(w) != S or not np.all(np.isfinite(w)):
        raise ValueError(f"density must be None, 'pipe' or {S} finite real weights (one per sample), got shape {w.shape} "
                         f"of {w.dtype}")
    return w.astype(np.float64), "custom"


def grid_table(trajectory, matrix, oversampling: float = 2.0, width: int = 4, density=None,
               iterations: int = PIPE_ITERATIONS) -> GridTable:
    """The two sparse tables of a trajectory (module docstring), from vectorised fp64 host arithmetic: O(S W^d)."""
    k = _trajectory(trajectory)
    mat, Gs, W = _geometry(matrix, oversampling, width, k.shape[1])
    cells, prod, betas = _footprint(k, mat, Gs, W)
    S, per = cells.shape
    n_cells = int(np.prod(Gs))
    dens, _ = _density(density, cells, prod, n_cells, iterations)
    # gridding: rows are cells, entries in ascending j (the flat order is j-major: a stable sort by cell keeps it)
    flat = cells.ravel()
    order = np.argsort(flat, kind="stable")
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(flat, minlength=n_cells))])
    grid = dev.SparseTable(rowptr, (order // per).astype(np.int32), (prod * dens[:, None]).ravel()[order], n=S)
    # degridding: rows are samples, entries in ascending cell
    inner = np.argsort(cells, axis=1, kind="stable")
    degrid = dev.SparseTable(np.arange(S + 1, dtype=np.int64) * per, np.take_along_axis(cells, inner, 1).ravel(),
                             np.take_along_axis(prod, inner, 1).ravel(), n=n_cells)
    c = tuple(deapodization(m, G, W, b) for m, G, b in zip(mat, Gs, betas))
    return GridTable(grid, degrid, Gs, betas, c, mat, W, dens)


def density_weights(trajectory, matrix, oversampling: float = 2.0, width: int = 4,
                    iterations: int = PIPE_ITERATIONS) -> np.ndarray:
    """Pipe-Menon density compensation of a trajectory: S weights, ``w <- w / (A1^T A1 w)`` for `iterations` rounds
    from w = 1 with A1 the unit-density gridding matrix of `grid_table` (host arithmetic, O(S W^d) per round)."""
    k = _trajectory(trajectory)
    mat, Gs, W = _geometry(matrix, oversampling, width, k.shape[1])
    cells, prod, _ = _footprint(k, mat, Gs, W)
    return _density("pipe", cells, prod, int(np.prod(Gs)), iterations)[0]


def _label(density) -> str:
    return "none" if density is None else density if isinstance(density, str) else "custom"


def _names(value, d: int, default, what: str, taken):
    names = default[:d] if value is None else ((value,) if isinstance(value, str) else tuple(value))
    names = tuple(str(n) for n in names)
    if len(names) != d:
        raise ValueError(f"{what}: {len(names)} names for {d} trajectory dims")
    if len(set(names)) != d or any(n in taken for n in names):
        raise ValueError(f"{what}: {names} repeats a name or takes the name of another dim of the array ({tuple(taken)})")
    return names


def _fov(fov, d: int):
    f = _per_dim(fov, d, "fov", _float)
    if f is None or any(v <= 0 for v in f):
        raise ValueError(f"fov must be a positive number or one per dim, got {fov!r}")
    return f


def _attrs(src, names, t: GridTable, label: str):
    attrs = _copy.copy(src.attrs)
    attrs[ATTRS.grid_dims] = tuple(names)
    attrs[ATTRS.grid_matrix] = tuple(t.matrix)
    attrs[ATTRS.grid_oversampled] = tuple(t.oversampled)
    attrs[ATTRS.grid_width] = t.width
    attrs[ATTRS.grid_beta] = tuple(t.beta)
    attrs[ATTRS.grid_density] = label
    return attrs


def _readout(da, readout_time, sample_dim: str, inverse: bool):
    """`da` itself for ``readout_time=None``; otherwise ``correct_readout_time`` along the ``time`` dim."""
    if readout_time is None:
        return da
    from .timeshift import correct_readout_time

    return correct_readout_time(da, readout_time, sample_dim=sample_dim, inverse=inverse)


def _grid(da, trajectory, matrix, oversampling, width, density, iterations, dim, out_dim, fov, name):
    """Validation, table and the gridding launch: (source, tensor with the flat cell axis, axis, names, table, fov)."""
    src = as_labeled(da)
    _check_dims(src, (dim,), name)
    k = _trajectory(trajectory)
    d = k.shape[1]
    if k.shape[0] != src.sizes[dim]:
        raise ValueError(f"trajectory: {k.shape[0]} samples for a {dim!r} dim of {src.sizes[dim]} points")
    names = _names(out_dim, d, K_DIMS if name == "grid_kspace" else X_DIMS, "out_dim", [n for n in src.dims if n != dim])
    f = _fov(fov, d)
    t = grid_table(k, matrix, oversampling, width, density, iterations)
    x, _ = device_data(src)
    axis = src.get_axis_num(dim)
    return src, dev.axis_sparse(x, axis, t.grid), axis, names, t, f


def _expand(src, dim, names, coords_of):
    """Dims and coords with `dim` replaced in place by `names`; coordinates along `dim` are dropped."""
    dims = []
    for n in src.dims:
        dims.extend(names if n == dim else (n,))
    coords = {k: c for k, c in src.coords.items() if c.dim != dim}
    for a, n in enumerate(names):
        coords[n] = Coordinate(n, coords_of(a), {})
    return dims, coords


def grid_kspace(da, trajectory, matrix, oversampling: float = 2.0, width: int = 4, density=None, dim: str = DIMS.sample,
                out_dim=None, fov=1.0, iterations: int = PIPE_ITERATIONS, readout_time=None):
    """Non-Cartesian samples -> the oversampled Cartesian k-space: one launch of the gather kernel for all coils and time
    points (module docstring).  `trajectory`: [S, d] in cycles per field of view; `matrix`: the target matrix m (an int
    or one per dim); `density`: None, S real weights or ``"pipe"`` (`iterations` rounds of Pipe-Menon).  The `dim` dim
    is replaced in place by ``kx[, ky[, kz]]`` (or `out_dim`) of G points each with the coordinate
    ``(arange(G) - G // 2) (m / G) / fov``; other coords and attrs are kept, ``grid_*`` attrs are added; the result is
    device-resident for LabeledArray input.  A cell that no sample touches is zero.  `readout_time`: None, or the S
    acquisition delays of the samples in the unit of the ``time`` coordinate: ``correct_readout_time`` runs first."""
    da = _readout(da, readout_time, dim, False)
    src, y, axis, names, t, f = _grid(da, trajectory, matrix, oversampling, width, density, iterations, dim, out_dim, fov,
                                      "grid_kspace")
    shape = tuple(y.shape)
    y = y.reshape(shape[:axis] + tuple(t.oversampled) + shape[axis + 1:])
    dims, coords = _expand(src, dim, names,
                           lambda a: (np.arange(t.oversampled[a]) - t.oversampled[a] // 2) * (t.matrix[a] / t.oversampled[a]) / f[a])
    return like_input(LabeledArray(y, dims, coords, _attrs(src, names, t, _label(density)), src.name), da)


def _image_table(m: int, G: int, c: np.ndarray, sign: float) -> np.ndarray:
    """F of the module docstring ([m, G], sign = +1) or its Hermitian transpose ([G, m], sign = -1)."""
    f = c[:, None] * _unit(np.outer(np.arange(m) - m // 2, np.arange(G) - G // 2), G, 1.0) / np.sqrt(G)
    return f if sign > 0 else np.ascontiguousarray(f.conj().T)


def _narrow(x, axis: int, start: int, length: int):
    idx = [slice(None)] * len(x.shape)
    idx[axis] = slice(start, start + length)
    y = x[tuple(idx)]
    return y.contiguous() if hasattr(y, "contiguous") else np.ascontiguousarray(y)


def _image_tables(t: GridTable, sign: float):
    """Per dim what the transform between the oversampled grid and the voxels needs: the [m, G] table F (sign = +1) or
    F^H (sign = -1) where G fits ``axis_dft``, else the complex vector c of the staged transform."""
    return [_image_table(m, G, c, sign) if G <= dev.AXIS_DFT_MAX else c + 0j
            for m, G, c in zip(t.matrix, t.oversampled, t.deapodization)]


def _to_voxels(y, axis: int, t: GridTable, tables):
    """The gridded samples `y` (flat cell axis at `axis`) -> voxels: per dim one ``axis_dft`` launch, or for G > 64 the
    centred transform of ``to_image`` on G, the crop and the product with c.  `tables`: ``_image_tables(t, 1.0)``, host
    values or already on the device."""
    shape = tuple(y.shape)
    y = y.reshape(shape[:axis] + tuple(t.oversampled) + shape[axis + 1:])
    for a, (m, G) in enumerate(zip(t.matrix, t.oversampled)):
        if G <= dev.AXIS_DFT_MAX:
            y = dev.axis_dft(y, axis + a, tables[a])
        else:
            y = dev.fft(y, axis + a, inverse=True, ortho=True, shift_in=True, shift_out=True)
            y = dev.phase_apply(_narrow(y, axis + a, G // 2 - m // 2, m), axis + a, tables[a])
    return y


def _to_samples(x, axis: int, t: GridTable, tables):
    """Voxels (the image dims from `axis` on) -> samples: the transposed chain of `_to_voxels` and degridding.
    `tables`: ``_image_tables(t, -1.0)``."""
    for a, (m, G) in enumerate(zip(t.matrix, t.oversampled)):
        if G <= dev.AXIS_DFT_MAX:
            x = dev.axis_dft(x, axis + a, tables[a])
        else:
            x = dev.phase_apply(x, axis + a, tables[a])
            x = dev.zero_fill(x, axis + a, G, pad_left=G // 2 - m // 2)
            x = dev.fft(x, axis + a, inverse=False, ortho=True, shift_in=True, shift_out=True)
    return _apply_degrid(x, axis, t)


def nufft_adjoint(da, trajectory, matrix, oversampling: float = 2.0, width: int = 4, density=None,
                  dim: str = DIMS.sample, out_dim=None, fov=1.0, iterations: int = PIPE_ITERATIONS, readout_time=None):
    """Non-Cartesian samples -> voxels: ``grid_kspace``, then per dim the centred inverse transform, the crop to
    `matrix` and the de-apodisation in one launch (module docstring).  Approximates
    ``(1 / sqrt(m^d)) sum_j dens_j x_j exp(2 pi i k_j (p - m // 2) / m)``; for a full Cartesian trajectory with unit
    density that is ``to_image``.  The `dim` dim is replaced in place by ``x[, y[, z]]`` (or `out_dim`) of m points each
    with the coordinate ``(arange(m) - m // 2) fov / m``.  `readout_time`: as in ``grid_kspace``."""
    da = _readout(da, readout_time, dim, False)
    src, y, axis, names, t, f = _grid(da, trajectory, matrix, oversampling, width, density, iterations, dim, out_dim, fov,
                                      "nufft_adjoint")
    y = _to_voxels(y, axis, t, _image_tables(t, 1.0))
    dims, coords = _expand(src, dim, names, lambda a: (np.arange(t.matrix[a]) - t.matrix[a] // 2) * f[a] / t.matrix[a])
    return like_input(LabeledArray(y, dims, coords, _attrs(src, names, t, _label(density)), src.name), da)


def _gather_dims(src, names, name: str):
    """The tensor with the dims `names` adjacent and in order at the place of the first (one copy when they are not
    already), that axis, and the array's other dims in their order."""
    _check_dims(src, names, name)
    if len(set(names)) != len(names):
        raise ValueError(f"dim: a dimension is repeated in {names}")
    x, _ = device_data(src)
    axes = [src.get_axis_num(n) for n in names]
    first = min(axes)
    rest = [i for i in range(src.ndim) if i not in axes]
    lead = [i for i in rest if i < first]
    perm = lead + axes + [i for i in rest if i > first]
    if perm != list(range(src.ndim)):
        x = x.permute(perm) if hasattr(x, "permute") else np.transpose(x, perm)
    return x, len(lead)


def _degrid(da, trajectory, matrix, oversampling, width, dim, out_dim, default, name, image: bool):
    src = as_labeled(da)
    k = _trajectory(trajectory)
    d = k.shape[1]
    names = default[:d] if dim is None else ((dim,) if isinstance(dim, str) else tuple(dim))
    if len(names) != d:
        raise ValueError(f"dim: {len(names)} names for {d} trajectory dims")
    others = [n for n in src.dims if n not in names]
    if out_dim in others:
        raise ValueError(f"out_dim: {out_dim!r} is the name of another dim of the array ({src.dims})")
    _check_dims(src, names, name)
    t = grid_table(k, matrix, oversampling, width, None)
    want = t.matrix if image else t.oversampled
    for n, w in zip(names, want):
        if src.sizes[n] != w:
            raise ValueError(f"matrix: dim {n!r} has {src.sizes[n]} points, the trajectory's "
                             f"{'matrix' if image else 'oversampled grid'} has {w}")
    x, axis = _gather_dims(src, names, name)
    return src, x, axis, names, t


def _collapse(src, names, out_dim, S: int):
    first = min(src.get_axis_num(n) for n in names)
    dims = [n for n in src.dims if n not in names]
    dims.insert(sum(1 for n in src.dims[:first] if n not in names), out_dim)
    coords = {k: c for k, c in src.coords.items() if c.dim not in names}
    coords[out_dim] = Coordinate(out_dim, np.arange(S), {})
    return dims, coords


def _apply_degrid(x, axis: int, t: GridTable):
    shape = tuple(x.shape)
    d = len(t.oversampled)
    flat = x.reshape(shape[:axis] + (int(np.prod(t.oversampled)),) + shape[axis + d:])
    return dev.axis_sparse(flat, axis, t.degrid)


def degrid_kspace(da, trajectory, matrix, oversampling: float = 2.0, width: int = 4, dim=None, out_dim: str = DIMS.sample,
                  readout_time=None):
    """The oversampled Cartesian k-space -> its values at the trajectory's samples: the transpose of ``grid_kspace``
    with unit density, one launch.  `dim`: the k-space dims in the trajectory's order (``kx[, ky[, kz]]`` by default),
    of G points each; they are replaced by `out_dim` (S points, coordinate ``arange(S)``) at the place of the first.
    `readout_time`: None, or the S acquisition delays of the samples: ``correct_readout_time(inverse=True)`` runs last,
    the transpose of what ``grid_kspace`` does with them."""
    src, x, axis, names, t = _degrid(da, trajectory, matrix, oversampling, width, dim, out_dim, K_DIMS, "degrid_kspace", False)
    y = _apply_degrid(x, axis, t)
    dims, coords = _collapse(src, names, out_dim, t.grid.n)
    return _readout(like_input(LabeledArray(y, dims, coords, _attrs(src, names, t, "none"), src.name), da), readout_time,
                    out_dim, True)


def nufft_forward(da, trajectory, matrix=None, oversampling: float = 2.0, width: int = 4, dim=None,
                  out_dim: str = DIMS.sample, readout_time=None):
    """Voxels -> non-Cartesian samples: the transpose chain of ``nufft_adjoint`` with unit density (the product with c,
    the centred forward transform zero filled to G, degridding); with ``nufft_adjoint`` the building blocks of an
    iterative reconstruction.  `dim`: the image dims in the trajectory's order (``x[, y[, z]]`` by default); `matrix`
    defaults to their sizes.  `readout_time`: as in ``degrid_kspace``."""
    src0 = as_labeled(da)
    k = _trajectory(trajectory)
    names = X_DIMS[:k.shape[1]] if dim is None else ((dim,) if isinstance(dim, str) else tuple(dim))
    if matrix is None:
        _check_dims(src0, names, "nufft_forward")
        matrix = tuple(src0.sizes[n] for n in names)
    src, x, axis, names, t = _degrid(da, k, matrix, oversampling, width, names, out_dim, X_DIMS, "nufft_forward", True)
    if hasattr(x, "contiguous"):
        x = x.contiguous()
    y = _to_samples(x, axis, t, _image_tables(t, -1.0))
    dims, coords = _collapse(src, names, out_dim, t.grid.n)
    return _readout(like_input(LabeledArray(y, dims, coords, _attrs(src, names, t, "none"), src.name), da), readout_time,
                    out_dim, True)
