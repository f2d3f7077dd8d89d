#!/usr/bin/env python3
"""Where the bounds of tests/test_gpu_wg.py come from (JACOBI_TOL, CHOL_TOL of tests/test_wg.py).  CPU only; no kernel is
involved.  The output is kept as profiles/wg_toolbox/tolerance.txt.

Jacobi, every C in 1 ... 64, the four matrices of tests/_wg_oracle.py's families: the residual max |G V - V Lambda| in
units of eps64 ||G||_F and the departure from orthonormality max |V^H V - I| in units of eps64 (it has no scale: V is
unitary whatever the size of G), evaluated in longdouble, for np.linalg.eigh and for the oracle's plain row-cyclic fp64
Jacobi; per size the larger of the two, and the oracle's sweep count.  JACOBI_TOL is 16 x the worst figure of each
quantity over all sizes: the margin for a third summation order of the same algorithm.  (The oracle's Jacobi applies
plain products with c and s, so its V drifts from orthonormality about five times as far as eigh's; the kernel's
Rutishauser form stays below both.)

Cholesky, every P in 1 ... 80, two problems x lam in {0, 1e-3, 1e3}: max |L L^T - (H + lam D)| in units of
eps64 ||H + lam D||_F for np.linalg.cholesky, max |x - x_longdouble| in units of eps64 cond max |x| for that factor with
fp64 substitution and for np.linalg.solve (the larger), and the largest cond(H + lam D), which must stay <= 1e12.
CHOL_TOL is 16 x the worst figure of each quantity over all sizes.

The third Jacobi figure (off(G) <= 2 eps ||G||_F, the kernel's own stopping rule with a factor 2 for the rounding of the
two norms) and the transforms' 16 units (at most 8 roundings in the longest formula, doubled) are derivations, not
measurements: tests/test_wg.py states them."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _wg_oracle as orc  # noqa: E402

jw = [0.0, 0.0, 0]
for c in range(1, orc.MAXC + 1):
    res, orth, sweeps = orc.jacobi_reference(c)
    print(f"jacobi C={c:2d}  residual {res:6.3f}  orthonormality {orth:7.3f}  oracle sweeps {sweeps}")
    jw = [max(jw[0], res), max(jw[1], orth), max(jw[2], sweeps)]
print(f"jacobi worst: residual {jw[0]:.3f}  orthonormality {jw[1]:.3f}  oracle sweeps {jw[2]}")
print(f'JACOBI_TOL = {{"residual": {16 * jw[0]:.1f}, "orthonormality": {16 * jw[1]:.1f}}}')
# a record, not a bound (the bound is XM_WG_SWEEPS = 30): what tests/test_gpu_wg.py printed on an MI355X
print("wg_jacobi on the same matrices, MI355X: at most 9 sweeps")
cw = [0.0, 0.0, 0.0]
for p in range(1, orc.MAXP + 1):
    fac, sol, cond = orc.cholesky_reference(p)
    print(f"cholesky P={p:2d}  factor {fac:6.3f}  solution {sol:.3e}  cond {cond:.2e}")
    cw = [max(cw[0], fac), max(cw[1], sol), max(cw[2], cond)]
print(f"cholesky worst: factor {cw[0]:.3f}  solution {cw[1]:.3f}  cond {cw[2]:.2e}")
print(f'CHOL_TOL = {{"factor": {16 * cw[0]:.1f}, "solution": {16 * cw[1]:.2f}}}')
