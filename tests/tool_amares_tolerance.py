#!/usr/bin/env python3
"""Where STEP_TOL of tests/test_amares_kernel.py comes from.  CPU only; the kernel is not involved.

The first m trial steps of the AMARES iteration are computed twice by tests/_amares_oracle.py:
lm_steps -- once solving the fp64 normal equations (numpy.linalg.solve), once by least squares on the augmented Jacobian
[J; sqrt(lambda D)] (LAPACK, orthogonal factorisation; J^T J is never formed).  Printed per case and m: the largest
disagreement of a parameter in units of that parameter's path length (the sum of |change| over the accepted steps), the
relative disagreement in rss, and whether a trial's accept / reject margin was below the tie threshold.  The test's
bound is 16 x the largest figure of the last line."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _amares_oracle as orc  # noqa: E402

STEP_M = (1, 2, 3, 5)
TIE = 1e-9

worst_p, worst_f, pairs, ties = 0.0, 0.0, 0, 0
for name, kw in orc.step_cases():
    c = orc.kernel_case(**kw)
    for m in STEP_M:
        pairs += 1
        tie = False
        for v in range(c["x"].shape[0]):
            a, b = (orc.lm_steps(c["x"][v], c["t"], c["init"], c["lo"], c["hi"], c["fixed"], max_iter=m, solver=s)
                    for s in ("normal", "qr"))
            assert [t[0] for t in a["trials"]] == [t[0] for t in b["trials"]], (name, m, v)
            tie = tie or any(abs(g) < TIE for _, g in a["trials"])
            d = np.abs(a["params"].ravel() - b["params"].ravel())
            still = a["path"] == 0
            assert np.all(d[still] == 0), (name, m, v)
            dp = float(np.max(d[~still] / a["path"][~still])) if (~still).any() else 0.0
            df = abs(a["rss"] - b["rss"]) / a["rss"]
            cond = np.linalg.cond(orc.normal_equations(c["x"][v], c["t"], a["params"], c["lo"], c["hi"], c["fixed"],
                                                       internal=True)[0])
            print(f"{name:20s} m={m} voxel {v}: accepted {sum(t[0] for t in a['trials'])}/{m}  |dp|/path {dp:.2e}  "
                  f"rss rel {df:.2e}  cond(J^T J) {cond:.1e}")
            worst_p, worst_f = max(worst_p, dp), max(worst_f, df)
        ties += tie
print(f"largest |dp| / path {worst_p:.2e}   largest rss rel {worst_f:.2e}   (case, m) pairs with a tie: {ties} of {pairs}")
