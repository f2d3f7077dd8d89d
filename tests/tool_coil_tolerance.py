#!/usr/bin/env python3
"""Where COIL_TOL of tests/test_coils.py comes from.  CPU only; the kernel is not involved.

Every parity case of tests/_coils_oracle.py is combined twice by the oracle: u from numpy.linalg.eigh of the whitened
Gram matrix, and u from numpy.linalg.svd of the whitened reference (G never formed).  Printed per case: the largest
disagreement of y, w and quality in units of eps lam1 / (lam1 - lam2) (y relative to max |y|, w to max |w|), and the
smallest relative gap (lam1 - lam2) / lam1.  COIL_TOL is 16 x the largest figure of y, the last line."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _coils_oracle as orc  # noqa: E402

worst = 0.0
for name in orc.PARITY_CASES:
    x = orc.parity_case(name)
    a, b = (orc.combine_batch(x, coil_axis=1, route=r) for r in ("eigh", "svd"))
    uy, uw, uq = orc.route_gap_units(a, b)
    gap = float(np.min((a["lam1"] - a["lam2"]) / a["lam1"]))
    print(f"{name:18s} y {uy:6.2f}  w {uw:6.2f}  quality {uq:6.2f}   smallest gap {gap:.3f}")
    worst = max(worst, uy)
print(f"largest disagreement of y {worst:.2f} units of eps lam1 / (lam1 - lam2)   ->  COIL_TOL = {16 * worst:.0f}")
