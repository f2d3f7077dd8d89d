#!/usr/bin/env python3
"""Where GRAPPA_TOL and GRAPPA_CAL_TOL of tests/test_grappa.py come from, and what the oracle reconstructs.  CPU only;
the kernel is not involved.  Writes profiles/grappa/tolerance.txt.

(a) Apply.  Every parity case of tests/_grappa_oracle.py (seeded samples and weights) is filled twice by the oracle: the
sum of the definition in ascending order in float64, every product and addition rounded on its own, and the same terms in
numpy.longdouble.  The unit of an output is eps64 sum |W| |a| over its terms.  GRAPPA_TOL is 16 x the largest gap: the
kernel's fused multiply-adds round differently from numpy's separate products.  complex64 output adds the one rounding
the definition makes, eps32 |y|.
(b) Calibration.  Every end-to-end case is calibrated by two routes in complex128: the normal equations, and lstsq on the
system augmented by sqrt(lambda') I, which never forms them.  The unit of a weight is eps64 kappa(G + lambda' I)
max |W_type|.  GRAPPA_CAL_TOL is 16 x the largest gap.
(c) Reconstruction.  Per end-to-end case ||filled - true|| / ||true|| over the missing lines (zeros score 1.0).
(d) The condition number of the first case's calibration system at regularization 0, 1e-8, 1e-6 and 1e-4."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

import _grappa_oracle as orc  # noqa: E402

lines = ["(a) apply: case                 terms   gap to the long-double sum"]
worst_a = 0.0
for name, (ns, accel, kernel, c, t) in orc.APPLY_CASES.items():
    r = orc.apply_case(name)[4]
    g = orc.gap(r["y"], r["alt"], r["unit"])
    lines.append(f"{name:30s} {c * int(np.prod(kernel)):5d}   {g:6.3f}")
    worst_a = max(worst_a, g)
lines.append(f"largest gap: {worst_a:.3f} units")
lines.append(f"GRAPPA_TOL = {16 * worst_a:.1f}")
lines.append("")
lines.append("(b) calibration: case            lambda    K   n_eq   largest kappa   residual   routes' gap   (c) score")
worst_b = 0.0
for name in orc.E2E_CASES:
    cal, _, sc = orc.e2e_oracle(name)
    g = orc.calibration_gap(cal, orc.e2e_oracle(name, "lstsq")[0])
    k = cal["w"].shape[1] * cal["w"].shape[2]
    lines.append(f"{name:30s} {orc.E2E_CASES[name][5]:7.0e} {k:4d}  {min(cal['n_eq']):5d}   {max(cal['kappa']):12.3e}   "
                 f"{max(cal['residual']):8.2e}   {g:8.3f}      {sc:8.4f}")
    worst_b = max(worst_b, g)
lines.append(f"largest gap of the two routes: {worst_b:.3f} units")
lines.append(f"GRAPPA_CAL_TOL = {16 * worst_b:.1f}")
lines.append("")
lines.append("(d) why the default regularization is 1e-4: kappa(G + lambda' I) of the first case's system (8 coils, 2 x 3, 12 x 12 ACS)")
_, sm, _ = next(orc.systems(orc.e2e_case("16x32_r2x1_b2x3_c8")["acs"], (2, 1), (2, 3), 8))
g = sm @ sm.conj().T
for lam in (0.0, 1e-8, 1e-6, 1e-4):
    ev = np.linalg.eigvalsh(g + lam * np.trace(g).real / len(g) * np.eye(len(g)))
    lines.append(f"lambda {lam:7.0e}: {ev[-1] / ev[0]:10.3e}")
text = "\n".join(lines) + "\n"
print(text, end="")
out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "grappa")
os.makedirs(out, exist_ok=True)
with open(os.path.join(out, "tolerance.txt"), "w") as f:
    f.write(text)
