#!/usr/bin/env python3
"""Where CGS_TOL128, CGS_TOL64 and the convergence figures of tests/test_cgsense.py come from.  CPU only; the kernels are
not involved.  Every case of tests/_cgsense_oracle.py, 3 columns, all figures relative to the largest |x| of the plain
oracle's result.

(a) complex128.  6 iterations at tol 0 by the oracle with one dense normal matrix, and by the oracle that applies the two
chains stage by stage with every sparse stage as the CSR sum, one term at a time.  CGS_TOL128 is 16 x the largest
disagreement: the project's margin for two routes through the same arithmetic.

(b) complex64.  The data rounded to complex64; 6 iterations by the stage-by-stage oracle, and by the one that rounds every
coil-sized intermediate to complex64 where the GPU has a launch boundary (after the expansion, every per-dim transform,
degridding, gridding).  CGS_TOL64 is 16 x the largest disagreement.  The same gap is printed at 30 iterations: on these
conditioned cases (density weights or regularization) it stays flat; conjugate gradients amplify rounding with the
condition number, and on unweighted, unregularised radial data the gap grows with the iteration count (last line).

(c) Convergence.  The plain oracle's distance to the direct solve of the normal equations after 30 iterations, and its
relative residual.  The GPU test allows 4 x the recorded distance.

    python tests/tool_cgsense_tolerance.py > profiles/cgsense/tolerance.txt
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _cgsense_oracle as orc  # noqa: E402

worst128 = worst64 = 0.0
for name in orc.CASES:
    c = orc.case(name)
    b = c.rhs()
    plain = orc.cg(c.dense(), b, 6)[0]
    routes = orc.rel(orc.cg(c.staged(csr=True), c.rhs(csr=True), 6)[0], plain)
    y64 = orc.c64(c.y)
    b64, b64r = c.rhs(y64), c.rhs(y64, rnd=orc.c64)
    gaps = []
    for n in (6, 30):
        ref = orc.cg(c.staged(), b64, n)[0]
        gaps.append(orc.rel(orc.cg(c.staged(rnd=orc.c64), b64r, n)[0], ref))
    x30, res30, _, _ = orc.cg(c.dense(), b, 30)
    ev = np.linalg.eigvalsh(c.normal_matrix())
    live = ev[ev > 1.5 * c.lam] if name == "masked2d" else ev  # (a masked voxel is an eigenvector of value lambda)
    print(f"{name:9s} V {c.V:3d} S {c.S:3d} C {c.C}  condition {live.max() / live.min():6.2f}  routes differ by {routes:.3e}  "
          f"complex64 rounding {gaps[0]:.3e} (6 iterations) {gaps[1]:.3e} (30)")
    print(f"convergence {name:9s} distance to the direct solve at 30 iterations {orc.rel(x30, c.solve(b)):.3e}  "
          f"residual {res30.max():.3e}")
    worst128, worst64 = max(worst128, routes), max(worst64, gaps[0])
print(f"largest route disagreement: {worst128:.3e}")
print(f"CGS_TOL128 = {16 * worst128:.3e}")
print(f"largest complex64 rounding gap: {worst64:.3e}")
print(f"CGS_TOL64 = {16 * worst64:.3e}")

# unweighted, unregularised radial data: not a parity case, and why
c = orc.Case("radial2d")
c.w, c.lam = np.ones(c.S), 0.0
y64 = orc.c64(c.y)
for n in (6, 12, 30):
    gap = orc.rel(orc.cg(c.staged(rnd=orc.c64), c.rhs(y64, rnd=orc.c64), n)[0], orc.cg(c.staged(), c.rhs(y64), n)[0])
    print(f"unconditioned radial2d (no density, regularization 0): complex64 rounding {gap:.3e} at {n} iterations")
