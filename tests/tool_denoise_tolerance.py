#!/usr/bin/env python3
"""Where DENOISE_TOL of tests/test_denoise.py comes from.  CPU only; the kernel is not involved.

Every parity case of tests/_denoise_oracle.py is denoised twice by the oracle: the eigenpairs of G = X X^H from
numpy.linalg.eigh of G, and from numpy's SVD of the window matrix X itself.  Printed per case: the seed, the ranks, the
smallest margin of the rank scan, and the largest disagreement of y in units of eps max(1, lam_0 / (lam_{r-1} - lam_r))
max |x| (eps max |x| where r = 0 or r = P) and of sigma relative to itself.  DENOISE_TOL is 16 x the worst figure of
each quantity, the last line.  Also the improvement at 8 x 8 / 5 x 5 / 256 and 5 x 5 x 4 / 3 x 3 x 3 / 128: the rms
distance to the noise-free FIDs before and after, and the mean sigma."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _denoise_oracle as orc  # noqa: E402

worst = dict(y=0.0, sigma=0.0)
for name in orc.PARITY_CASES:
    clean, x, a, b, seed = orc.parity_case(name)
    gy, gs = orc.route_gap(a, b, x)
    print(f"{name:20s} seed {seed}  ranks {a['rank'].min()}-{a['rank'].max()}  margin {min(a['margin'].min(), b['margin'].min()):.1e}  "
          f"y {gy:6.2f} units  sigma {gs:.2e}")
    worst["y"], worst["sigma"] = max(worst["y"], gy), max(worst["sigma"], gs)
print(f"largest disagreement: y {worst['y']:.2f} units  sigma {worst['sigma']:.2e}")
print(f'DENOISE_TOL = {{"y": {16 * worst["y"]:.1f}, "sigma": {16 * worst["sigma"]:.1e}}}')
rms = lambda z: float(np.sqrt(np.mean(np.abs(z) ** 2)))  # noqa: E731
for name in ("g8x8_p5x5_n256", "g5x5x4_p3x3x3_n128"):
    clean, x, a, _, _ = orc.parity_case(name)
    print(f"{name}: rms |x - clean| {rms(x - clean):.4f} -> rms |y - clean| {rms(a['y'] - clean):.4f}, "
          f"mean sigma {a['sigma'].mean():.4f}")
