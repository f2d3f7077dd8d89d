"""``recon_l1_sense``: wavelet-sparse iterative SENSE (compressed-sensing MRSI) for multi-coil, undersampled,
non-Cartesian MRSI on the GPU -- few spokes or interleaves per frame, pseudo-random blips: acquisitions that alias under
``recon_cg_sense``'s Tikhonov term alone.

The definition is this backend's own (the reference has nothing here).  With E, D and the maps of
``recon_cg_sense`` (section 21), per column:

    minimise  1/2 |D^(1/2) (E x - y)|^2 + lambda2 / 2 |x|^2 + lambda_t |Psi x|_1,   x = 0 where every coil's map is 0

Psi: the image is cut into blocks of 2^l_d voxels per dim (`levels`), each transformed by the orthonormal decimated Haar
transform to that depth; the approximation coefficient of a block is not penalised (all levels 0: Psi = I, everything
is).  lambda_t = sparsity max_v |b[v]| with b = E^H D y, lambda2 = tikhonov x the scale of section 21.  FISTA from x = 0
with the step tau = 1 / L, L = step_safety x (Rayleigh quotient of E^H D E after `power_iterations` power steps) + lambda2:

    g = (E^H D E) v_k + lambda2 v_k - b;  x_{k+1} = mask . S_k^H Psi^H soft(Psi S_k (v_k - tau g), tau lambda_t)
    t_{k+1} = (1 + sqrt(1 + 4 t_k^2)) / 2;  v_{k+1} = x_{k+1} + (t_k - 1) / t_{k+1} (x_{k+1} - x_k)

a column stops when |x_{k+1} - x_k| <= tol |x_{k+1}|.  S_k is the identity, or with `cycle_spin` the circular shift of
the block lattice by k mod 2^l_d voxels per dim.  x, v, b and every scalar are complex128 / fp64; what is coil-sized is
in the data's dtype.
"""
from __future__ import annotations

import numpy as np

from .. import device as dev
from ..config import ATTRS, DIMS
from .cgsense import _columns, _number, _passes, _problem, _result, _upload, normal_scale

MAX_BLOCK = 16  # voxels per Haar block
# 1 + 2 x the largest shortfall lambda_max / estimate - 1 of 20 power steps over the oracle's cases, rounded up to two
# digits (tests/tool_l1sense_tolerance.py, profiles/l1sense/tolerance.txt)
STEP_SAFETY = 1.2


def default_levels(matrix) -> tuple:
    """min(2, the largest l with 2^l | m_d) per dim, then lowered from the last dim backwards until the block has at most
    16 voxels."""
    levels = []
    for m in matrix:
        l = 0
        while l < 2 and int(m) % (2 << l) == 0:
            l += 1
        levels.append(l)
    d = len(levels) - 1
    while sum(levels) > 4:
        if levels[d] == 0:
            d -= 1
        else:
            levels[d] -= 1
    return tuple(levels)


def _levels(levels, matrix) -> tuple:
    if levels is None:
        return default_levels(matrix)
    vals = [levels] * len(matrix) if isinstance(levels, (int, np.integer)) and not isinstance(levels, bool) else levels
    try:
        vals = list(vals)
    except TypeError:
        vals = [None]
    if len(vals) != len(matrix) or any(isinstance(l, bool) or not isinstance(l, (int, np.integer)) or l < 0 for l in vals):
        raise ValueError(f"levels must be an integer >= 0 per image dim ({len(matrix)}), got {levels!r}")
    vals = tuple(int(l) for l in vals)
    if sum(vals) > 4:
        raise ValueError(f"levels: {vals} makes blocks of {1 << sum(vals)} voxels, supported are at most {MAX_BLOCK}")
    for m, l in zip(matrix, vals):
        if int(m) % (1 << l):
            raise ValueError(f"levels: the matrix size {int(m)} is not divisible by 2^{l}")
    return vals


def _count(value, name: str) -> int:
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or value < 0:
        raise ValueError(f"{name} must be an integer >= 0, got {value!r}")
    return int(value)


def recon_l1_sense(da, trajectory, sensitivities, matrix=None, sparsity: float = 0.02, levels=None, iterations: int = 50,
                   tol: float = 1e-4, tikhonov: float = 0.0, cycle_spin: bool = False, step=None,
                   power_iterations: int = 20, step_safety: float = STEP_SAFETY, density=None, noise_cov=None,
                   oversampling: float = 2.0, width: int = 4, dim: str = DIMS.sample, coil_dim: str = DIMS.coil,
                   out_dim=None, fov=1.0, readout_time=None, chunk=None, return_info: bool = False):
    """Wavelet-sparse SENSE reconstruction of the non-Cartesian multi-coil samples `da` (module docstring; DESIGN.md
    section 24).  Data, `trajectory`, `sensitivities`, `matrix`, `density`, `noise_cov`, `oversampling`, `width`, `fov`,
    `out_dim`, `readout_time` and `chunk` exactly as in ``recon_cg_sense``.  `sparsity`: weight of the l1 penalty relative
    to the largest ``|E^H D y|`` of the column.  `levels`: Haar levels per image dim (an integer for all), each matrix size
    divisible by ``2^level`` and at most 16 voxels per block; default min(2, what divides) per dim, lowered from the last
    dim until the block fits.  `tikhonov`: weight of ``1/2 |x|^2`` relative to the mean diagonal of the normal matrix.
    `iterations`: the cap; `tol`: a column stops at ``|x_new - x| <= tol |x_new|``.  `cycle_spin`: move the block lattice
    by one voxel per step (then no longer one convex problem).  `step`: the step size tau; by default 1 / L with L =
    `step_safety` x the power estimate of `power_iterations` steps + the Tikhonov weight (the estimate is a lower bound of
    the largest eigenvalue: keep `step_safety` above 1).

    Returns the image (complex128) laid out as by ``recon_cg_sense``, plus the attrs ``l1sense_sparsity``,
    ``l1sense_levels``, ``l1sense_iterations``, ``l1sense_tol``, ``l1sense_step`` (the tau used) and ``l1sense_lipschitz``
    (1 / tau).  With `return_info` a dataset of ``image``, ``change`` (|x_new - x| / |x_new| at the column's last test),
    ``iterations`` and ``status`` (0 iteration cap, 1 converged, 3 not finite) over the column dims."""
    iterations = _count(iterations, "iterations")
    power_iterations = _count(power_iterations, "power_iterations")
    tol = _number(tol, "tol")
    sparsity = _number(sparsity, "sparsity")
    tikhonov = _number(tikhonov, "tikhonov")
    step_safety = _number(step_safety, "step_safety")
    if step is not None:
        step = _number(step, "step")
    if (step is not None and step == 0.0) or step_safety == 0.0:
        raise ValueError(f"step and step_safety must be > 0, got step={step!r}, step_safety={step_safety!r}")
    if not isinstance(cycle_spin, (bool, np.bool_)):
        raise ValueError(f"cycle_spin must be True or False, got {cycle_spin!r}")
    _columns(chunk)
    pb = _problem("recon_l1_sense", da, trajectory, sensitivities, matrix, density, noise_cov, oversampling, width, dim,
                  coil_dim, out_dim, fov, readout_time)
    lv = _levels(levels, pb.spatial)
    _upload(pb, readout_time)
    lam2 = tikhonov * normal_scale(pb.energy, pb.table.density, pb.n_vox)
    mask = np.ascontiguousarray(pb.energy > 0, dtype=np.uint8)
    if pb.on_device:
        import torch

        mask = torch.from_numpy(mask).to(pb.y.device)
    if step is None:
        lipschitz = step_safety * dev.l1_lipschitz(pb.s, pb.adjoint, pb.forward, mask, power_iterations, pb.y.dtype) + lam2
        if not (np.isfinite(lipschitz) and lipschitz > 0.0):
            raise ValueError(f"step: the estimate of the Lipschitz bound is {lipschitz!r}; sensitivities, density and data "
                             f"dtype must give a finite, non-zero operator, or pass `step`")
        step = 1.0 / lipschitz
    parts = _passes(pb, chunk, lambda yk: dev.l1_sense(yk, pb.s, pb.adjoint, pb.forward, mask, pb.spatial, lv, lam2, sparsity,
                                                       step, iterations, tol, bool(cycle_spin)))
    own = {ATTRS.l1sense_sparsity: sparsity, ATTRS.l1sense_levels: lv, ATTRS.l1sense_iterations: iterations,
           ATTRS.l1sense_tol: tol, ATTRS.l1sense_step: step, ATTRS.l1sense_lipschitz: 1.0 / step}
    return _result(pb, parts, own, ("change", "iterations", "status"), return_info)
