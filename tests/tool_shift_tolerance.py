#!/usr/bin/env python3
"""What tests/test_shift.py records about its oracle (tests/_shift_oracle.py).  CPU only; the kernel is not involved.

(a) The two routes of the oracle, numpy.fft and the explicit O(N L) sums, on every case of ROUTE_CASES with the delays
PHIS: the largest disagreement per case, relative to each row's largest magnitude.  The GPU tests do not take their bound
from this figure (theirs is 4 x TIGHT of tests/test_gpu_kernels.py); it shows how far below that bound the oracle's own
error lies.

(b) The physical case: three damped lines, 50 rows acquired tau in [0, dt) late.  The largest spectral error against
the tau = 0 data, relative to the spectrum's largest magnitude, uncorrected and after the oracle's shift.

    python tests/tool_shift_tolerance.py > profiles/shift/tolerance.txt
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _shift_oracle as orc  # noqa: E402

worst = 0.0
for L, N in orc.ROUTE_CASES:
    x = orc.make((len(orc.PHIS), N), seed=L + N)
    g = float(orc.row_gap(orc.shift_fft(x, orc.PHIS, L), orc.shift_sums(x, orc.PHIS, L)).max())
    print(f"L {L:5d} N {N:5d} delays {orc.PHIS}: routes differ by {g:.3e} of the row's largest magnitude")
    worst = max(worst, g)
print(f"largest disagreement: {worst:.3e}")
x, tau, truth, dt = orc.physical_case()
print(f"physical case: lines {orc.LINES_HZ} Hz, T2* {orc.T2_STAR} s, dt {orc.DT} s, N = L = {orc.N_PHYS}, {orc.ROWS_PHYS} rows, "
      f"tau = r dt / {orc.ROWS_PHYS}")
print(f"spectral error uncorrected: {orc.spectral_error(x, truth):.4e}")
print(f"spectral error corrected: {orc.spectral_error(orc.shift_fft(x, tau / dt), truth):.4e}")
