"""``espirit_maps``: ESPIRiT coil sensitivities (Uecker et al. 2014) from the auto-calibration block of k-space, the map
maker for protocols without a fully sampled reference image: the same ACS block ``grappa_calibrate`` takes feeds
``unfold_sense`` and ``recon_cg_sense``.

The definition is this backend's own (the reference has no such function).  Calibration (host numpy,
complex128): every position of a window of b_a points per dim inside the block, at each of the first `acs_points` time
points, is one row of the calibration matrix A, columns ordered (s_1, ..., s_d, coil) with the coil fastest; v_j are the
right singular vectors of A with sigma_j > threshold sigma_1 (from the eigen-decomposition of A^H A), S = prod b_a.  Per
voxel p of the image, q_a = p_a - N_a // 2:

    g_j(q)[c] = sum_s conj(v_j[s, c]) exp(+2 pi i sum_a q_a s_a / N_a),   H(q) = (1 / S) sum_j g_j(q) g_j(q)^H.

H is Hermitian with eigenvalues in [0, 1]; where the calibration holds, the largest is 1 and its eigenvector is the coil
sensitivity up to a common phase.  H is computed through its autocorrelation coefficients

    Hc[u][c, d] = (1 / S) sum_j sum_{s - s' = u} conj(v_j[s, c]) v_j[s', d],   H(q) = sum_u Hc[u] exp(2 pi i q u / N),

u_a = -(b_a - 1) ... b_a - 1: host FFTs of length 2 b_a - 1, then one launch of ``xm_axis_dft`` per dim on the array
[u_1 .. u_d, E] that holds the E = C (C + 1) / 2 entries of the upper triangle where the time axis normally lies (the
staged transform above 64 points), then one launch of ``xm_espirit_eig`` for the eigenpairs of every voxel.
"""
from __future__ import annotations

import numpy as np

from .. import device as dev
from ..config import DIMS
from ..labeled import Coordinate, LabeledArray, as_labeled, is_xarray, like_input
from ._common import to_host
from .coils import _linv
from .grappa import _acs_values, _check_names, _names
from .mrsi import _TO_IMAGE, _int, _per_dim, _unit

MAX_COILS = dev.ESPIRIT_MAX_COILS
MAX_TERMS = 4096  # K = C S, the order of A^H A
MAX_SYSTEM = 1 << 26  # entries of the calibration matrix A
MAP_DIM = "map"


def _fraction(value, what: str) -> float:
    try:
        v = float(value)
    except (TypeError, ValueError):
        v = float("nan")
    if isinstance(value, bool) or not 0.0 <= v <= 1.0:
        raise ValueError(f"{what} must be a number in 0 ... 1, got {value!r}")
    return v


def calibration_matrix(block, ker, points: int) -> np.ndarray:
    """A of the module docstring from block [C, A_1 .. A_d, T] (complex128): [positions x time points, S C]."""
    d = len(ker)
    t = min(points, block.shape[-1])
    win = np.lib.stride_tricks.sliding_window_view(block[..., :t], tuple(ker), axis=tuple(range(1, d + 1)))
    # [C, P_1 .. P_d, T, b_1 .. b_d] -> [P_1 .. P_d, T, b_1 .. b_d, C]
    win = np.moveaxis(win, 0, -1)
    return np.ascontiguousarray(win).reshape(-1, int(np.prod(ker)) * block.shape[0])


def calibrate(block, ker, points: int, threshold: float):
    """(v [Nk, b_1 .. b_d, C], singular values of A, all K of them, descending)."""
    c, shape = block.shape[0], block.shape[1:-1]
    k = c * int(np.prod(ker))
    rows = int(np.prod([a - b + 1 for a, b in zip(shape, ker)])) * min(points, block.shape[-1])
    if rows * k > MAX_SYSTEM:
        raise ValueError(f"acs: the calibration matrix has {rows} x {k} entries, more than 2^26: lower acs_points or "
                         f"shrink the kernel")
    if not np.all(np.isfinite(block)):
        raise ValueError("acs: the block holds a non-finite value")
    a = calibration_matrix(block, ker, points)
    if not np.any(a):
        raise ValueError("acs: the block is zero at every calibration point")
    w, vec = np.linalg.eigh(a.conj().T @ a)
    sigma = np.sqrt(np.maximum(w[::-1], 0.0))
    keep = int(np.count_nonzero(sigma > threshold * sigma[0]))
    v = vec[:, ::-1][:, :keep].T
    return v.reshape((keep, *ker, c)), sigma


def autocorrelation(v) -> np.ndarray:
    """Hc of the module docstring from v [Nk, b_1 .. b_d, C]: [2 b_1 - 1 .. 2 b_d - 1, C, C], u = 0 at index b_a - 1."""
    ker, c = v.shape[1:-1], v.shape[-1]
    span = tuple(2 * b - 1 for b in ker)
    axes = tuple(range(1, 1 + len(ker)))
    f = np.fft.fftn(np.conj(v), s=span, axes=axes).reshape(v.shape[0], -1, c)
    p = np.einsum("jkc,jkd->kcd", f, np.conj(f)).reshape(span + (c, c))
    hc = np.fft.ifftn(p, axes=tuple(range(len(ker)))) / float(np.prod(ker))
    return np.fft.fftshift(hc, axes=tuple(range(len(ker))))


def image_table(n: int, b: int) -> np.ndarray:
    """exp(2 pi i (p - n // 2) (k - (b - 1)) / n), [n, 2 b - 1]: the zero-filled centred inverse transform of a dim's
    2 b - 1 coefficients without the ortho scale."""
    return _unit(np.outer(np.arange(n) - n // 2, np.arange(2 * b - 1) - (b - 1)), n, 1.0)


def voxel_matrices(hc, mat, device="cuda"):
    """The upper triangles of H at every voxel, [N_1 .. N_d, E] (on `device`): one ``axis_dft`` per dim."""
    ker = tuple((n + 1) // 2 for n in hc.shape[:-2])
    iu, ju = np.triu_indices(hc.shape[-1])
    coef = np.ascontiguousarray(hc[..., iu, ju])
    staged = [n > dev.AXIS_DFT_MAX for n in mat]
    coef = coef * float(np.prod([np.sqrt(n) for n, s in zip(mat, staged) if s]))  # the staged transform is ortho
    x = dev.to_device(coef, device)
    for axis, (n, b) in enumerate(zip(mat, ker)):
        if not staged[axis]:
            x = dev.axis_dft(x, axis, image_table(n, b))
        else:
            x = dev.zero_fill(x, axis, n, pad_left=n // 2 - (b - 1))
            x = dev.fft(x, axis, inverse=True, ortho=True, shift_in=True, shift_out=True)
    return x


def espirit_maps(acs, matrix, kernel=None, dims=(DIMS.kx, DIMS.ky), coil_dim: str = DIMS.coil, time_dim: str = DIMS.time,
                 acs_points: int = 8, threshold: float = 0.02, crop: float = 0.8, n_maps: int = 1, noise_cov=None,
                 phase_ref: int = 0, return_eigenvalues: bool = False):
    """ESPIRiT coil sensitivities on the image grid `matrix` (an int for all dims or one per dim) from the
    auto-calibration block `acs`, a fully sampled piece of centred k-space: an array with the dims ``(coil_dim, *dims)``
    and optionally `time_dim` in any order, or array-like in that order, on the host or the device.  `kernel`: window
    points per dim, default min(6, the block's size); each of the first `acs_points` time points gives its own rows.
    `threshold`: singular vectors of the calibration matrix above threshold x the largest singular value span the
    signal space.  `n_maps`: 1 or 2 maps per voxel, by descending eigenvalue.  A map is exact zeros where its
    eigenvalue is below `crop`: the mask of ``unfold_sense`` and ``recon_cg_sense``.  Each map has unit norm over the
    coils and coil `phase_ref` real and >= 0.  `noise_cov`: a C x C Hermitian positive-definite matrix Psi = L L^H; the
    block is whitened by L^-1 and the maps are returned as L m, the frame ``sense_maps`` returns.

    Returns a host LabeledArray (complex128; a DataArray for DataArray input) with the dims ``(coil_dim, x[, y[, z]])``
    (named as ``to_image`` names them for `dims`), with a leading ``map`` dim when `n_maps` is 2.  With
    `return_eigenvalues` a dataset of ``maps``, ``eigenvalues`` ([map,] voxels) and ``status`` (voxels: 0 ok, 1 the
    Jacobi sweep cap was reached, 2 not finite), attrs ``n_kernels`` (singular vectors kept), ``singular_values``,
    ``threshold``, ``crop`` and ``kernel``."""
    names = _names(dims)
    _check_names(names, coil_dim, time_dim)
    unknown = [d for d in names if d not in _TO_IMAGE]
    if unknown:
        raise ValueError(f"dims: no image name for {unknown}; known are {tuple(_TO_IMAGE)}")
    outs = tuple(_TO_IMAGE[d] for d in names)
    mat = _per_dim(matrix, len(names), "matrix", _int)
    if mat is None or any(n < 1 for n in mat):
        raise ValueError(f"matrix must be an integer >= 1 or one per dim, got {matrix!r}")
    try:
        points = _int(acs_points)
    except (TypeError, ValueError):
        points = 0
    if points < 1:
        raise ValueError(f"acs_points must be an integer >= 1, got {acs_points!r}")
    thr, crp = _fraction(threshold, "threshold"), _fraction(crop, "crop")
    if isinstance(n_maps, bool) or n_maps not in (1, 2):
        raise ValueError(f"n_maps must be 1 or 2, got {n_maps!r}")
    block = _acs_values(acs, names, coil_dim, time_dim)
    c, shape = block.shape[0], block.shape[1:-1]
    if c > MAX_COILS:
        raise ValueError(f"acs: {c} coils along {coil_dim!r}, supported are 1 ... {MAX_COILS}")
    if n_maps > c:
        raise ValueError(f"n_maps: {n_maps} maps need at least as many coils, the block has {c}")
    if isinstance(phase_ref, bool) or not isinstance(phase_ref, (int, np.integer)) or not 0 <= phase_ref < c:
        raise ValueError(f"phase_ref must be a coil index in 0 ... {c - 1}, got {phase_ref!r}")
    ker = tuple(min(6, a) for a in shape) if kernel is None else _per_dim(kernel, len(names), "kernel", _int)
    if any(b < 1 for b in ker):
        raise ValueError(f"kernel must be an integer >= 1 or one per dim, got {kernel!r}")
    for d, b, a, n in zip(names, ker, shape, mat):
        if b > a:
            raise ValueError(f"kernel: {b} points along {d!r}, the block has {a}")
        if 2 * b - 1 > n:
            raise ValueError(f"matrix: {n} points along {d!r} cannot hold the {2 * b - 1} coefficients of a kernel of {b}")
    if c * int(np.prod(ker)) > MAX_TERMS:
        raise ValueError(f"kernel: {c} coils x {int(np.prod(ker))} window points exceed {MAX_TERMS} columns")
    if isinstance(noise_cov, str):
        raise ValueError(f"noise_cov must be a {c} x {c} matrix, got {noise_cov!r}")
    linv = None if noise_cov is None else _linv(noise_cov, c)
    if linv is not None:
        block = np.einsum("cd,d...->c...", linv, block)

    v, sigma = calibrate(block, ker, points, thr)
    data = acs.data if isinstance(acs, LabeledArray) else acs
    device = data.device if hasattr(data, "detach") and data.is_cuda else "cuda"
    h = voxel_matrices(autocorrelation(v), mat, device)
    n_vox = int(np.prod(mat))
    res = dev.espirit_eig(h.reshape(n_vox, dev.espirit_entries(c)), c, int(n_maps), int(phase_ref), crp)
    maps = to_host(res.maps)  # [M, C, V]
    if linv is not None:
        maps = np.einsum("cd,mdv->mcv", np.linalg.inv(linv), maps)
    maps = np.ascontiguousarray(maps).reshape((int(n_maps), c) + tuple(mat))
    values = to_host(res.values).reshape((int(n_maps),) + tuple(mat))
    status = to_host(res.status).reshape(tuple(mat))

    coords, attrs, name = {}, {}, None
    if isinstance(acs, LabeledArray) or is_xarray(acs):
        src = as_labeled(acs)
        name = src.name
        for k, co in src.coords.items():
            if co.dim == coil_dim:
                coords[k] = co
            elif k == co.dim and co.dim in names:
                i = names.index(co.dim)
                old = np.asarray(co.values)
                delta = (old[1] - old[0]) if len(old) > 1 else 1.0
                coords[outs[i]] = Coordinate(outs[i], np.roll(np.fft.fftfreq(mat[i], d=delta), mat[i] // 2), {})
    lead = (MAP_DIM,) if n_maps == 2 else ()
    cut = (slice(None),) if n_maps == 2 else (0,)
    out = LabeledArray(np.ascontiguousarray(maps[cut]), lead + (str(coil_dim),) + outs, coords, attrs, name)
    if not return_eigenvalues:
        return like_input(out, acs) if is_xarray(acs) else out
    from ..fitting.dataset import LabeledDataset

    grid = {k: co for k, co in coords.items() if co.dim in outs}
    info = dict(n_kernels=int(v.shape[0]), singular_values=sigma, threshold=thr, crop=crp, kernel=tuple(ker))
    ds = LabeledDataset({"maps": out, "eigenvalues": LabeledArray(np.ascontiguousarray(values[cut]), lead + outs, grid),
                         "status": LabeledArray(status, outs, grid)}, info)
    return ds.to_xarray() if is_xarray(acs) else ds
