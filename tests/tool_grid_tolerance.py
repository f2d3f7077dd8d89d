#!/usr/bin/env python3
"""Where GRID_TOL and the approximation bounds of tests/test_grid.py come from.  CPU only; the kernel is not involved.

(a) Kernel tolerance.  Every parity case of tests/_grid_oracle.py is gridded twice by the oracle, by the CSR sum in its
stated order and by one dense matrix product, and the gridded data is degridded both ways too.  Printed per case: the
largest disagreement in units of the output's U = eps64 sum_e |val_e| |x_e|.  GRID_TOL is 16 x the worst figure.

(b) Approximation error.  For the named accuracy cases (oversampling 2, unit density): the largest error of the oracle's
nufft_adjoint against the exact sum, relative to the exact sum's largest magnitude.  The error is a property of (W,
alpha) and the fixed trajectory, not of rounding; the tests bound the package's nufft_adjoint by 2 x these figures.

    python tests/tool_grid_tolerance.py > profiles/grid/tolerance.txt
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _grid_oracle as orc  # noqa: E402

worst = 0.0
for name in orc.PARITY_CASES:
    x, traj, matrix, a0, W, axis, A, y, u = orc.parity_case(name)
    g = orc.gap(y, orc.apply_dense(A, x, axis), u)
    gd = orc.gap(orc.apply_csr(A.T, y, axis), orc.apply_dense(A.T, y, axis), orc.unit(A.T, y, axis))
    print(f"{name:12s} {str(x.shape):14s} -> {str(y.shape):14s} W {W}  entries {int((A != 0).sum()):6d}  "
          f"routes differ by {g:6.3f} units (gridding) {gd:6.3f} units (degridding)")
    worst = max(worst, g, gd)
print(f"largest disagreement: {worst:.3f} units")
print(f"GRID_TOL = {16 * worst:.1f}")
for name in orc.ACCURACY_CASES:
    x, traj, matrix, W, exact = orc.accuracy_case(name)
    err = orc.accuracy(orc.nufft_adjoint(x, traj, matrix, 2.0, W), exact)
    print(f"accuracy {name:18s} S {len(traj):5d}  W {W}  alpha 2  relative error {err:.3e}")
