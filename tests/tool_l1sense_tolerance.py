#!/usr/bin/env python3
"""Where L1_TOL128, L1_TOL64, the default of `step_safety` and the figures of the benefit case in tests/test_l1sense.py
come from.  CPU only; the kernels are not involved.  The parity cases of tests/_l1sense_oracle.py, 3 columns, their own
levels, sparsity 0.02, the Tikhonov weight of the case, tau = 1 / (step_safety x power estimate + lambda2).

(a) complex128.  10 steps at tol 0 by the oracle with one dense normal matrix, and by the one that applies the two chains
stage by stage with every sparse stage as the CSR sum.  L1_TOL128 is 16 x the largest disagreement relative to max |x|.

(b) complex64.  The data rounded to complex64; 10 steps by the stage-by-stage oracle, and by the one that rounds every
coil-sized intermediate to complex64 where the GPU has a launch boundary.  L1_TOL64 is 16 x the largest disagreement.  The
shrink is non-expansive and the gradient step a contraction, so rounding is not amplified: the same gap at 40 steps.

(c) The power estimate: lambda_max (eigvalsh of the dense normal matrix) over the Rayleigh quotient after 20 power steps
from the mask indicator, per case.  STEP_SAFETY = 1 + 2 x the largest shortfall, rounded up to two digits.

(d) The benefit case (16 x 16, 4 coils, radial(16, 6, 32), pipe density, 2 % noise, a 4 x 4 plateau and two point sources
per column): |x - truth| / |truth| of 30 conjugate-gradient iterations at regularization 0.05 and of 100 FISTA steps at
several sparsities; and sparsity 0 with a Tikhonov weight against the direct solve after 200 steps.

    python tests/tool_l1sense_tolerance.py > profiles/l1sense/tolerance.txt
"""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _cgsense_oracle as cgs  # noqa: E402
import _l1sense_oracle as orc  # noqa: E402

PARITY = ("radial2d", "masked2d", "random3d", "odd2d", "line1d")
SPARSITY = 0.02

shortfall = {}
for name in list(PARITY) + ["benefit"]:
    c = orc.case(name)
    M0 = c.normal_matrix(0.0)
    top = float(np.linalg.eigvalsh(M0)[-1])
    est = orc.power(lambda v: M0 @ v, c.mask, 20)
    shortfall[name] = top / est - 1.0
    print(f"power {name:9s} lambda_max {top:.6e}  estimate after 20 steps {est:.6e}  shortfall {shortfall[name]:.3e}")
worst = max(shortfall.values())
safety = math.ceil((1.0 + 2.0 * worst) * 10.0) / 10.0
print(f"largest shortfall: {worst:.3e}")
print(f"STEP_SAFETY = {safety:.1f}")

worst128 = worst64 = 0.0
for name in PARITY:
    c = orc.case(name)
    M0 = c.normal_matrix(0.0)
    tau = 1.0 / (safety * orc.power(lambda v: M0 @ v, c.mask, 20) + c.lam)
    args = (c.ms, c.levels, SPARSITY, tau)
    plain = orc.fista(c.dense(), c.rhs(), *args, 10, mask=c.mask).x
    routes = orc.rel(orc.fista(c.staged(csr=True), c.rhs(csr=True), *args, 10, mask=c.mask).x, plain)
    y64 = orc.c64(c.y)
    b64, b64r = c.rhs(y64), c.rhs(y64, rnd=orc.c64)
    gaps = []
    for n in (10, 40):
        ref = orc.fista(c.staged(), b64, *args, n, mask=c.mask).x
        gaps.append(orc.rel(orc.fista(c.staged(rnd=orc.c64), b64r, *args, n, mask=c.mask).x, ref))
    print(f"{name:9s} V {c.V:3d} S {c.S:3d} C {c.C} levels {c.levels}  routes differ by {routes:.3e}  "
          f"complex64 rounding {gaps[0]:.3e} (10 steps) {gaps[1]:.3e} (40)")
    worst128, worst64 = max(worst128, routes), max(worst64, gaps[0])
print(f"largest route disagreement: {worst128:.3e}")
print(f"L1_TOL128 = {16 * worst128:.3e}")
print(f"largest complex64 rounding gap: {worst64:.3e}")
print(f"L1_TOL64 = {16 * worst64:.3e}")

# sparsity 0 with a Tikhonov weight is the linear problem of section 21
c = orc.case("radial2d")
M0 = c.normal_matrix(0.0)
tau = 1.0 / (safety * orc.power(lambda v: M0 @ v, c.mask, 20) + c.lam)
x200 = orc.fista(c.dense(), c.rhs(), c.ms, c.levels, 0.0, tau, 200, mask=c.mask).x
print(f"linear radial2d sparsity 0, tikhonov {c.reg}: distance to the direct solve at 200 steps {orc.rel(x200, c.solve()):.3e}")

c = orc.case("benefit")
M0 = c.normal_matrix(0.0)
tau = 1.0 / (safety * orc.power(lambda v: M0 @ v, c.mask, 20))
lam = 0.05 * c.scale()
Mreg = c.normal_matrix(lam)
xcg = cgs.cg(lambda p: Mreg @ p, c.rhs(), 30)[0]
print(f"benefit V {c.V} S {c.S} (S/V = {c.S / c.V:.2f}): 30 CG iterations, regularization 0.05: error {orc.error(xcg, c.obj):.3f}")
for sp in (0.02, 0.0, 0.05, 0.1):
    x = orc.fista(lambda v: M0 @ v, c.rhs(), c.ms, c.levels, sp, tau, 100, mask=c.mask).x
    print(f"benefit 100 FISTA steps, levels {c.levels}, sparsity {sp}: error {orc.error(x, c.obj):.3f}")
