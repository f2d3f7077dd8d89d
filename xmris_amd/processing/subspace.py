"""``recon_subspace``: temporal-subspace iterative SENSE for multi-coil non-Cartesian MRSI on the GPU, and
``temporal_basis``, which makes the subspace from training data (SPICE, Lam & Liang 2014; the "subspace kernel" of
T2-shuffling, Tamir et al. 2017).

The definition is this backend's own (the reference has nothing here).  With E, D = diag(w) and
the sensitivities of ``recon_cg_sense`` (section 21), a basis V [R, T] (R <= 32, rows need not be orthonormal) and the
sampling flags m[s, t] in {0, 1}, per frame (every dim that is not sample, coil or time):

    minimise over U [V, R]:   sum_{c,s,t} w_s m[s,t] | sum_r (E U)_{c,s,r} V[r,t] - y[c,s,t] |^2  +  lambda |U|^2
    K_s[r, r'] = sum_t m[s,t] conj(V[r,t]) V[r',t]          b[c,s,r] = sum_t m[s,t] conj(V[r,t]) y[c,s,t]
    E^H D (K o E U) + lambda U = E^H D b,                    x[v, t] = sum_r U[v, r] V[r, t]
    lambda = regularization x normal_scale (section 21) x kappa,   kappa = sum_s w_s tr(K_s) / (R sum_s w_s)

The time axis leaves the iteration: only the R coefficient columns of a frame go through the two NUFFT chains, and the
sampling pattern -- which may differ from time point to time point -- enters as one R x R matrix per sample.  The R
columns of a frame are one coupled system and share every conjugate-gradient scalar: ``device.cg_sense`` runs unchanged
on the state folded to [V R, frames]."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from .. import device as dev
from ..config import ATTRS, DIMS
from ..dims import _check_dims
from ..labeled import LabeledArray, as_labeled, is_xarray
from .cgsense import _columns, _number, _passes, _problem, _result, _upload, default_chunk, normal_scale

MAX_RANK = dev.SUB_MAX_RANK


@dataclass
class TemporalBasis:
    """The result of ``temporal_basis``.  `vectors`: V [rank, time] complex128, the leading right singular vectors of
    the training data's Casorati matrix (rows orthonormal); `singular_values`: all of them, descending; `energy`: the
    share of sum sigma^2 the kept vectors hold.  The record keeps the device copy that its first use on a device made;
    `vectors` is not to be changed in place."""

    vectors: np.ndarray
    singular_values: np.ndarray = None
    energy: float = None
    _resident: dict = field(default_factory=dict, repr=False, compare=False)  # device -> the uploaded basis

    @property
    def rank(self) -> int:
        return int(self.vectors.shape[0])

    @property
    def n_time(self) -> int:
        return int(self.vectors.shape[1])

    def on(self, device):
        """V as a complex128 tensor on `device`: uploaded at the first call, the same afterwards."""
        key = str(device)
        if key not in self._resident:
            import torch

            self._resident[key] = torch.from_numpy(self.vectors).to(device)
        return self._resident[key]


def _rank(rank, n_time: int, limit=None) -> int:
    if isinstance(rank, bool) or not isinstance(rank, (int, np.integer)) or not 1 <= rank <= MAX_RANK:
        raise ValueError(f"rank must be an integer in 1 ... {MAX_RANK}, got {rank!r}")
    if rank > n_time or (limit is not None and rank > limit):
        raise ValueError(f"rank: {rank} vectors asked for, the training data has {n_time} points along time"
                         + ("" if limit is None else f" and {limit} rows"))
    return int(rank)


def temporal_basis(training, rank: int, dim: str = DIMS.time) -> TemporalBasis:
    """The first `rank` right singular vectors of the Casorati matrix of `training` (every dim but `dim` is a row): a
    labelled array with `dim`, or array-like with time last -- a low-resolution fully sampled navigator, say, or an
    earlier reconstruction.  The SVD is host numpy; rank <= 32, the time points and the rows."""
    if isinstance(training, LabeledArray) or is_xarray(training):
        src = as_labeled(training)
        _check_dims(src, (dim,), "temporal_basis")
        vals = src.data
        vals = vals.detach().cpu().numpy() if hasattr(vals, "detach") else np.asarray(vals)
        vals = np.moveaxis(vals, src.get_axis_num(dim), -1)
    else:
        vals = np.asarray(training)
    if vals.ndim < 1 or vals.size == 0:
        raise ValueError("training: needs at least the time axis and one row")
    rows = np.ascontiguousarray(vals.reshape(-1, vals.shape[-1]), dtype=np.complex128)
    r = _rank(rank, rows.shape[1], rows.shape[0])
    if not np.all(np.isfinite(rows.view(np.float64))):
        raise ValueError("training: a sample is not finite")
    _, sigma, vh = np.linalg.svd(rows, full_matrices=False)
    total = float(np.sum(sigma ** 2))
    energy = float(np.sum(sigma[:r] ** 2) / total) if total > 0 else 0.0
    return TemporalBasis(vectors=np.ascontiguousarray(vh[:r]), singular_values=sigma, energy=energy)


def _basis(basis, n_time: int) -> TemporalBasis:
    if not isinstance(basis, TemporalBasis):
        try:
            v = np.array(basis.detach().cpu().numpy() if hasattr(basis, "detach") else basis, dtype=np.complex128, order="C")
        except (TypeError, ValueError):
            raise ValueError(f"basis must be a TemporalBasis or array-like [R, T], got {type(basis).__name__}") from None
        basis = TemporalBasis(vectors=v)
    v = basis.vectors
    if v.ndim != 2 or v.dtype != np.complex128:
        raise ValueError(f"basis must be complex [R, T], got shape {v.shape}")
    if v.shape[1] != n_time:
        raise ValueError(f"basis: {v.shape[1]} points along time, the data has {n_time}")
    if not 1 <= v.shape[0] <= MAX_RANK or v.shape[0] > n_time:
        raise ValueError(f"basis: rank {v.shape[0]} must be in 1 ... {MAX_RANK} and at most the {n_time} time points")
    if not np.all(np.isfinite(v.view(np.float64))):
        raise ValueError("basis: an entry is not finite")
    return basis


def _sampling(sampling, dim: str, time_dim: str, n_samples: int, n_time: int):
    """None, or the flags as a host bool array [S, T]."""
    if sampling is None:
        return None
    if isinstance(sampling, LabeledArray) or is_xarray(sampling):
        s = as_labeled(sampling)
        if set(s.dims) != {dim, time_dim} or len(s.dims) != 2:
            raise ValueError(f"sampling: dims {s.dims} must be {(dim, time_dim)} in any order")
        m = s.data
        m = m.detach().cpu().numpy() if hasattr(m, "detach") else np.asarray(m)
        if s.dims[0] != dim:
            m = m.T
    else:
        m = sampling.detach().cpu().numpy() if hasattr(sampling, "detach") else np.asarray(sampling)
    if m.dtype != np.bool_:
        raise ValueError(f"sampling must be boolean, got dtype {m.dtype}")
    if m.shape != (n_samples, n_time):
        raise ValueError(f"sampling: shape {m.shape} must be ({n_samples}, {n_time}): ({dim}, {time_dim})")
    return np.ascontiguousarray(m)


def recon_subspace(da, trajectory, sensitivities, basis, sampling=None, matrix=None, iterations: int = 30, tol: float = 1e-6,
                   regularization: float = 0.0, density=None, noise_cov=None, oversampling: float = 2.0, width: int = 4,
                   dim: str = DIMS.sample, coil_dim: str = DIMS.coil, time_dim: str = DIMS.time, out_dim=None, fov=1.0,
                   chunk=None, return_info: bool = False, return_coefficients: bool = False):
    """Temporal-subspace SENSE reconstruction of the non-Cartesian multi-coil samples `da` (module docstring; DESIGN.md
    section 26).  `trajectory`, `sensitivities`, `matrix`, `density`, `noise_cov`, `oversampling`, `width`, `out_dim`, `fov`
    as in ``recon_cg_sense``.  `basis`: a ``TemporalBasis`` or array-like [R, T], R <= 32 and R <= T, finite; its rows need
    not be orthonormal.  `sampling`: None (everything was acquired), or booleans with the dims (`dim`, `time_dim`) in any
    order, or array-like [S, T]: which (sample, time) positions were acquired.  What the data holds at the others -- zeros,
    garbage, NaN -- reaches no output.  Every dim but `dim`, `coil_dim` and `time_dim` is a frame with its own conjugate-
    gradient scalars, status, residual and iterations (those of section 21); frames do not depend on the batch or on
    `chunk`, which counts frames (a pass carries R x chunk columns through the chains).  Data in the order
    ([frames,] coil, sample, time) is read where it lies; any other order costs one permuting copy.  `regularization` is
    relative to the mean diagonal of the normal matrix (kappa, the mean sampled energy of the basis, included).

    `readout_time` is deliberately not a parameter: the per-sample delay correction needs each sample's full FID, which
    (k, t)-undersampled data does not have.  A delay term inside K_s is the follow-up.

    Returns the image (complex128) without `coil_dim`, with `dim` replaced in place by ``x[, y[, z]]`` and `time_dim`
    kept, with the ``grid_*`` attrs, ``subspace_rank``, ``subspace_sampled_fraction`` and the three ``cgsense_*``.  A voxel
    whose sensitivity is zero in every coil has exactly zero coefficients and FID; a frame with a non-finite sampled
    value gets status 3 and NaN; all-false `sampling` gives a zero image with status 1.  With `return_coefficients` a
    dataset that also holds ``coefficients`` over (x..., ``coefficient``, frames), with `return_info` ``residual``,
    ``iterations`` and ``status`` per frame."""
    who = "recon_subspace"
    if isinstance(iterations, bool) or not isinstance(iterations, (int, np.integer)) or iterations < 0:
        raise ValueError(f"iterations must be an integer >= 0, got {iterations!r}")
    tol = _number(tol, "tol")
    reg = _number(regularization, "regularization")
    _columns(chunk)
    src0 = as_labeled(da)
    if time_dim == dim or time_dim == coil_dim:
        raise ValueError(f"time_dim: {time_dim!r} is the {'sample' if time_dim == dim else 'coil'} dim")
    _check_dims(src0, (dim, coil_dim, time_dim), who)
    n_time = src0.sizes[time_dim]
    tb = _basis(basis, n_time)
    m = _sampling(sampling, dim, time_dim, src0.sizes[dim], n_time)
    pb = _problem(who, da, trajectory, sensitivities, matrix, density, noise_cov, oversampling, width, dim, coil_dim, out_dim,
                  fov, None)
    frames = [n for n in pb.rest if n != time_dim]
    pb.rest = frames + [time_dim]
    r = tb.rank

    def arrange(y, on_device):  # (coil, sample, *frames, time) -> [C, S, F, T], where it lies if its layout allows
        shape = (y.shape[0], y.shape[1], int(np.prod(y.shape[2:-1], dtype=np.int64)), y.shape[-1])
        if not on_device:
            return np.ascontiguousarray(y.reshape(shape)), shape[2]
        try:
            y4 = y.view(shape) if y.stride(-1) == 1 or n_time == 1 else y.contiguous().view(shape)
        except RuntimeError:  # the frame dims do not collapse into one stride
            y4 = y.contiguous().view(shape)
        return y4, shape[2]

    _upload(pb, None, arrange)
    device = pb.y.device if pb.on_device else None
    setup = dev.subspace_setup(tb.on(device) if pb.on_device else tb.vectors, m, pb.table.density, len(pb.table.density), device)
    lam = reg * normal_scale(pb.energy, pb.table.density, pb.n_vox) * setup.kappa
    itemsize = pb.y.element_size() if pb.on_device else pb.y.dtype.itemsize
    step = max(1, default_chunk(pb.c, pb.table.oversampled, itemsize, r * pb.n_cols) // r) if chunk is None else int(chunk)
    parts = _passes(pb, step, lambda yk: dev.subspace_sense(yk, pb.s, pb.adjoint, pb.forward, setup, lam, int(iterations), tol))
    own = {ATTRS.subspace_rank: r, ATTRS.subspace_sampled_fraction: setup.fraction, ATTRS.cgsense_iterations: int(iterations),
           ATTRS.cgsense_tol: tol, ATTRS.cgsense_regularization: reg}
    if not (return_info or return_coefficients):
        return _result(pb, parts, own, (), False)

    def extra(joined, coords):
        if not return_coefficients:
            return {}
        sizes = tuple(pb.src.sizes[n] for n in frames)
        dims = list(pb.names) + [DIMS.coefficient] + frames
        keep = {key: co for key, co in coords.items() if co.dim in dims}
        return {"coefficients": LabeledArray(joined("coefficients", 2).reshape(tuple(pb.spatial) + (r,) + sizes), dims, keep)}

    names = ("residual", "iterations", "status") if return_info else ()
    return _result(pb, parts, own, names, True, info_dims=frames, extra=extra)
