#!/usr/bin/env python3
"""Where SENSE_TOL of tests/test_sense.py comes from.  CPU only; the kernel is not involved.  Writes
profiles/sense/tolerance.txt.

Every parity case of tests/_sense_oracle.py is unfolded twice by the oracle in complex128: through the normal equations
and numpy's Cholesky factor, and through the pseudo-inverse (SVD) of the stacked whitened system, which never forms the
normal equations.  The unit of an output sample is eps64 kappa(A + lambda' I) sum_c |U[k, c]| |a_c[p, t]|, that of a
g-factor eps64 kappa(A + lambda' I) g.  Per case: the largest disagreement of rho and of g in these units, the largest
kappa(A) and the smallest relative Cholesky pivot.  SENSE_TOL is 16 x the largest disagreement (the project's usual margin
for the other summation order on the device); complex64 output adds the one rounding the definition makes,
eps32 |rho|."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

import _sense_oracle as orc  # noqa: E402

lines = ["case                  rho      g   largest kappa(A)   smallest pivot"]
worst = 0.0
for name in orc.PARITY_CASES:
    gr, gg = orc.route_gaps(name)
    a = orc.parity_routes(name)[0]
    lines.append(f"{name:18s} {gr:6.3f} {gg:6.3f}   {np.nanmax(a['kappa']):12.3e}   {np.nanmin(a['pivot']):12.3e}")
    worst = max(worst, gr, gg)
lines.append(f"largest disagreement of the two routes: {worst:.3f} units")
lines.append(f"SENSE_TOL = {16 * worst:.1f}")
text = "\n".join(lines) + "\n"
print(text, end="")
out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "sense")
os.makedirs(out, exist_ok=True)
with open(os.path.join(out, "tolerance.txt"), "w") as f:
    f.write(text)
