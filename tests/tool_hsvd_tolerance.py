#!/usr/bin/env python3
"""Where HSVD_TOL of tests/test_hsvd.py comes from.  CPU only; the kernel is not involved.

Every parity case of tests/_hsvd_oracle.py is decomposed twice by the oracle: the signal subspace from eigh of G = H^H H,
and from numpy's SVD of the Hankel matrix H itself; Q by lstsq, the poles by eigvals and the amplitudes by lstsq in
both.  Printed per case: the largest disagreement of y in units of max |x|, and over the in-band components of arg z_k
(radians per sample, f_k in units of 1 / (2 pi dt)), ln |z_k| (d_k in units of 1 / dt) and a_k in units of |a_k|.
HSVD_TOL is 16 x the worst figure of each quantity, the last lines.  Also the noise-free recovery at N = 512, M = 32,
K = 6: the rms distance of y from the metabolite-only FID.

Then the sparse and two-level combs (orc.VALUE_CASES), whose poles and amplitudes are known in closed form: per case and
route the oracle's distance from that truth, "pole" as max |dz|, "amp" the amplitudes relative, "sig" y in units of max |x|.
COMB_TOL is 16 x the worst of each: the kernel's Jacobi and QR against LAPACK are two roundings of the same answer.
Last the model cases (orc.MODEL_CASES), where parity with the oracle is not defined: per case and route
max |x - B a| / max |x| of the full model, cond(B) and the status; MODEL_RESIDUAL holds the larger route's figure."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _hsvd_oracle as orc  # noqa: E402

worst = dict(y=0.0, f=0.0, d=0.0, a=0.0)
for name in orc.PARITY_CASES:
    g, a, _ = orc.route_gap(name)
    print(f"{name:18s} y {g['y']:.2e}  f {g['f']:.2e}  d {g['d']:.2e}  a {g['a']:.2e}   cond(B) {a['cond'].max():7.0f}  "
          f"removed {a['n_removed'].tolist()}")
    for key in worst:
        worst[key] = max(worst[key], g[key])
print("largest disagreement: " + "  ".join(f"{k} {v:.2e}" for k, v in worst.items()))
print("HSVD_TOL = {" + ", ".join(f'"{k}": {16 * v:.1e}' for k, v in worst.items()) + "}")
x, met, _ = orc.make_fid(512, 11, 1, noise=0.0)
for rt in ("eigh", "svd"):
    r = orc.hsvd(x[0], 32, 6, route=rt)
    print(f"noise-free N 512, M 32, K 6, route {rt}: rms |y - metabolites| = {np.sqrt(np.mean(np.abs(r['y'] - met[0]) ** 2)):.1e}, "
          f"status {r['status']}, removed {r['n_removed']}")
comb = dict(pole=0.0, amp=0.0, sig=0.0)
for name in orc.VALUE_CASES:
    g, r, tg = orc.comb_routes(name)
    for rt in ("eigh", "svd"):
        print(f"{name:22s} {rt:4s} pole {tg[rt]['pole']:.2e}  amp {tg[rt]['amp']:.2e}  sig {tg[rt]['sig']:.2e}   cond(B) {r[rt]['cond']:5.2f}  "
              f"status {r[rt]['status']}  removed {r[rt]['n_removed']}")
        for key in comb:
            comb[key] = max(comb[key], tg[rt][key])
    print(f"{name:22s} routes: y {g['y']:.2e}  f {g['f']:.2e}  d {g['d']:.2e}  a {g['a']:.2e}")
print("largest distance from the truth: " + "  ".join(f"{k} {v:.2e}" for k, v in comb.items()))
print("COMB_TOL = {" + ", ".join(f'"{k}": {16 * v:.1e}' for k, v in comb.items()) + "}")
res = {}
for name in orc.MODEL_CASES:
    r, mr = orc.model_routes(name)
    for rt in ("eigh", "svd"):
        print(f"{name:12s} {rt:4s} max |x - B a| / max |x| {mr[rt]:.2e}   cond(B) {r[rt]['cond']:.1e}  status {r[rt]['status']}  "
              f"removed {r[rt]['removed'].tolist()}")
    res[name] = max(mr.values())
print("MODEL_RESIDUAL = {" + ", ".join(f'"{k}": {v:.1e}' for k, v in res.items()) + "}")
