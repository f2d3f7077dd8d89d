#!/usr/bin/env python3
"""Where MRSI_TOL of tests/test_mrsi.py comes from.  CPU only; the kernel is not involved.

Every parity case of tests/_mrsi_oracle.py is reconstructed twice by the oracle: by the table product per axis, and by
numpy's pad / ifftshift / (i)fftn / fftshift of the weighted, ramp-multiplied array.  Printed per case: the largest
disagreement in units of the pencil's U = eps64 prod(1 / sqrt(m_a)) sum_j prod(w_a[j_a]) |K_j|.  MRSI_TOL is 16 x the
worst figure, the last line.

    python tests/tool_mrsi_tolerance.py > profiles/mrsi/tolerance.txt
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _mrsi_oracle as orc  # noqa: E402

worst = 0.0
for name in orc.PARITY_CASES:
    x, axes, matrix, filters, shifts, sign, a, b, u = orc.parity_case(name)
    g = orc.gap(a, b, u)
    print(f"{name:30s} {str(x.shape):18s} -> {str(a.shape):18s} sign {sign:+d}  routes differ by {g:6.3f} units")
    worst = max(worst, g)
print(f"largest disagreement: {worst:.3f} units")
print(f"MRSI_TOL = {16 * worst:.1f}")
