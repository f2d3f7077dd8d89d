#!/usr/bin/env python3
"""Where ALIGN_TOL of tests/test_align.py comes from.  CPU only; the kernel is not involved.

Every parity case of tests/_align_oracle.py is aligned twice by the oracle: f* from the safeguarded Newton iteration of
the definition in fp64, and f* from scipy's brentq on P' over the same bracket with every sum in long double.  Printed
per case: the largest disagreement of f* in units of u_f = eps (sum |z|) (4 pi sum |z| |tau|) / |P''(f*)| and of phi* in
units of u_phi = eps sum |z| / |C(f*)| + 2 pi taubar u_f, and the smallest margin.  ALIGN_TOL is 16 x the larger of the
two figures, the last line."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _align_oracle as orc  # noqa: E402

worst_f = worst_p = 0.0
for name in orc.PARITY_CASES:
    x, r, dt, ms, L = orc.parity_case(name)
    a, b = (orc.align_batch(x, r, dt, 0.0, ms, L, route=rt) for rt in ("newton", "brentq"))
    uf, up = orc.route_gap_units(a, b)
    print(f"{name:18s} f* {uf:6.2f}  phi* {up:6.2f}   smallest margin {np.min(a['margin']):.3f}")
    worst_f, worst_p = max(worst_f, uf), max(worst_p, up)
print(f"largest disagreement: f* {worst_f:.2f} units of u_f, phi* {worst_p:.2f} units of u_phi   ->  "
      f"ALIGN_TOL = {16 * max(worst_f, worst_p):.0f}")
