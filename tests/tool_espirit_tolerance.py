#!/usr/bin/env python3
"""Where the ESP_TOL_* constants and the ORACLE figures of tests/test_espirit.py come from.  CPU only; the kernels are
not involved.  Every case of tests/_espirit_oracle.py.

(a) H by two routes.  The package's host route (eigen-decomposition of A^H A, autocorrelation coefficients, one table per
dim applied as a matrix product) against the oracle's dense route (SVD of A, g_j(q) at every voxel).  The largest
|difference| of an entry of H; the entries are at most 1.  "route": both from the oracle's singular vectors; "whole": each
from its own decomposition.  ESP_TOL_H is 16 x the largest "whole" figure: the project's margin for two routes through
the same arithmetic.

(b) Eigenpairs by two routes.  ``_wg_oracle.jacobi``, the numpy restatement of wg_jacobi, against ``numpy.linalg.eigh``,
both followed by the selection, norm and phase rules, on the H of every case and on the matrices of the kernel's own GPU
test (U diag(1, 0.6, 0.3, 0.15 ...) U^H, 37 of them, 1 ... 64 coils: the rounding of a Jacobi sweep grows with the order,
and the cases stop at 8 coils).  Recorded: the eigenvalue difference, the residual ||H m - lambda m|| / ||H||_F of the
Jacobi pairs, and the difference of the first map (on the cases: on the voxels of the object, where lambda_1 - lambda_2
>= 0.5) and of the second.  ESP_TOL_VALUE, ESP_TOL_RESIDUAL and ESP_TOL_MAP are 16 x the largest of each; the second map
of a case is printed and left out, because lambda_2 and lambda_3 of a case may all but coincide: such a map is held to
its residual alone.  A whole call differs from the oracle by (a) as well: by Weyl's bound and the sin-theta bound its
eigenvalues are held to ESP_TOL_VALUE + C ESP_TOL_H and its first map to ESP_TOL_MAP + C ESP_TOL_H / 0.5, 0.5 being the
gap the conditions of (c) demand.

(c) The oracle against the truth, per case, maps cropped at 0.9: the smallest lambda_1, the largest lambda_2 and the
smallest gap inside the object, the share of object voxels left out, the largest map error inside the object and the
error of a SENSE unfolding at accel 2 along the first dim relative to max |object|.  The tests allow the package 2 x the
last two.

    python tests/tool_espirit_tolerance.py > profiles/espirit/tolerance.txt
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _espirit_oracle as orc  # noqa: E402
import _mrsi_oracle as mrsi_orc  # noqa: E402
import _wg_oracle as wg  # noqa: E402
from xmris_amd.processing import espirit as esp  # noqa: E402

KERNEL_TEST_COILS = (1, 2, 3, 8, 17, 64)


def host_route(v, mat):
    """H [N..., C, C] from the package's coefficients and tables, the tables applied as matrix products."""
    hc = esp.autocorrelation(v)
    for axis, (n, b) in enumerate(zip(mat, v.shape[1:-1])):
        hc = mrsi_orc.apply_table(hc, axis, esp.image_table(n, b))
    return hc


def eig_gaps(h, n_maps, where=None):
    """(value gap, residual of the Jacobi pairs, gap of map 0, gap of map 1 or 0) of jacobi against eigh on h [V, C, C]."""
    lam_j, vec_j, _ = wg.jacobi(h)
    order = np.argsort(lam_j, axis=-1, kind="stable")
    lam_j = np.take_along_axis(lam_j, order, axis=-1)
    vec_j = np.take_along_axis(vec_j, order[:, None, :], axis=-1)
    lam_e, vec_e = np.linalg.eigh(h)
    mj, vj = orc.select(lam_j, vec_j, n_maps, 0, 0.0)
    me, ve = orc.select(lam_e, vec_e, n_maps, 0, 0.0)
    fro = np.sqrt((np.abs(h) ** 2).sum(axis=(1, 2)))
    res = 0.0
    for m in range(n_maps):
        x = np.moveaxis(mj[m], 0, -1)
        r = np.linalg.norm(np.einsum("vcd,vd->vc", h, x) - vj[m][:, None] * x, axis=-1)
        res = max(res, float((r / np.where(fro > 0, fro, 1.0)).max()))
    keep = slice(None) if where is None else where
    gaps = [float(np.abs(mj[m] - me[m])[:, keep].max()) for m in range(n_maps)]
    return float(np.abs(vj - ve).max()), res, gaps[0], gaps[1] if n_maps > 1 else 0.0


worst_h = worst = 0.0
worst_b = np.zeros(3)
for name in orc.CASES:
    c = orc.case(name)
    ref = orc.reference(name, crop=0.0)
    v_orc, _ = orc.singular_vectors(c.acs, c.kernel, 8, c.threshold)
    v_pkg, sigma = esp.calibrate(np.asarray(c.acs), c.kernel, 8, c.threshold)
    route = float(np.abs(host_route(v_orc, c.mat) - ref["H"]).max())
    whole = float(np.abs(host_route(v_pkg, c.mat) - ref["H"]).max())
    assert v_pkg.shape == v_orc.shape
    print(f"{name:7s} matrix {c.mat} C {c.C} ACS {c.block} kernel {c.kernel} kept {v_orc.shape[0]} of {sigma.size}  "
          f"H route {route:.3e} whole {whole:.3e}")
    worst_h = max(worst_h, whole)
    h = ref["H"].reshape(-1, c.C, c.C)
    dv, res, g0, g1 = eig_gaps(h, 2, c.mask.reshape(-1))
    print(f"eigenpairs {name:7s} value {dv:.3e} residual {res:.3e} map 1 {g0:.3e} map 2 {g1:.3e}")
    worst_b = np.maximum(worst_b, [dv, res, g0])  # (lambda_2 and lambda_3 of a case may coincide: map 2 by its residual)
    f = orc.figures(c, ref["maps"], ref["values"])
    print(f"truth {name:7s} lambda_1 min {f['lam1_min']:.4f} lambda_2 max {f['lam2_max']:.4f} gap min {f['gap_min']:.4f} "
          f"left out {f['left_out']:.3f} map error {f['map_error']:.3e} unfolding error {f['unfold_error']:.3e}")
for coils in KERNEL_TEST_COILS:
    h, _ = orc.random_hermitian(coils, 37, coils)
    dv, res, g0, g1 = eig_gaps(h, min(2, coils))
    print(f"eigenpairs kernel test C {coils:2d} value {dv:.3e} residual {res:.3e} map 1 {g0:.3e} map 2 {g1:.3e}")
    worst_b = np.maximum(worst_b, [dv, res, max(g0, g1)])
print(f"largest H disagreement: {worst_h:.3e}")
print(f"ESP_TOL_H = {16 * worst_h:.3e}")
print(f"largest eigenvalue disagreement: {worst_b[0]:.3e}")
print(f"ESP_TOL_VALUE = {16 * worst_b[0]:.3e}")
print(f"largest residual: {worst_b[1]:.3e}")
print(f"ESP_TOL_RESIDUAL = {16 * worst_b[1]:.3e}")
print(f"largest map disagreement: {worst_b[2]:.3e}")
print(f"ESP_TOL_MAP = {16 * worst_b[2]:.3e}")
