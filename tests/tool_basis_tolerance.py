#!/usr/bin/env python3
"""Where STEP_TOL of tests/test_gpu_basis.py comes from.  CPU only; the kernel's own figures play no part in it.

The first m trial steps of the basis-set iteration (DESIGN.md sections 8 and 15) are computed twice by
tests/_basis_oracle.py: lm_steps_basis -- once solving the fp64 normal equations (numpy.linalg.solve), once by least
squares on the augmented Jacobian [J; sqrt(lambda D)] (LAPACK, orthogonal factorisation; J^T J is never formed).
Printed per case and m: the largest disagreement of a parameter in units of that parameter's path length (the sum of
|change| over the accepted steps), the relative disagreement in rss, and whether a trial's accept / reject margin was
below the tie threshold.  The test's bound is 16 x the largest figure of the last line, which this tool also writes to
profiles/basis/tolerance.txt."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _basis_oracle as orc  # noqa: E402

STEP_M = (1, 2, 3, 5)
TIE = 1e-9

lines = []


def say(s):
    print(s)
    lines.append(s)


worst_p, worst_f, pairs, ties = 0.0, 0.0, 0, 0
for name, kw in orc.step_cases():
    c = orc.kernel_case(**kw)
    args = (c["B"], c["group"], c["dt"], c["init"], c["lo"], c["hi"], c["fixed"], c["skip"])
    for m in STEP_M:
        pairs += 1
        tie = False
        for v in range(c["x"].shape[0]):
            a, b = (orc.lm_steps_basis(c["x"][v], *args, max_iter=m, solver=s) for s in ("normal", "qr"))
            assert [t[0] for t in a["trials"]] == [t[0] for t in b["trials"]], (name, m, v)
            tie = tie or any(abs(g) < TIE for _, g in a["trials"])
            d = np.abs(a["params"] - b["params"])
            still = a["path"] == 0
            assert np.all(d[still] == 0), (name, m, v)
            dp = float(np.max(d[~still] / a["path"][~still])) if (~still).any() else 0.0
            df = abs(a["rss"] - b["rss"]) / a["rss"]
            say(f"{name:22s} m={m} voxel {v}: accepted {sum(t[0] for t in a['trials'])}/{m}  |dp|/path {dp:.2e}  "
                f"rss rel {df:.2e}")
            worst_p, worst_f = max(worst_p, dp), max(worst_f, df)
        ties += tie
say(f"largest |dp| / path {worst_p:.2e}   largest rss rel {worst_f:.2e}   (case, m) pairs with a tie: {ties} of {pairs}")
out = os.path.join(os.path.dirname(HERE), "profiles", "basis")
os.makedirs(out, exist_ok=True)
with open(os.path.join(out, "tolerance.txt"), "w") as f:
    f.write("python tests/tool_basis_tolerance.py  (CPU only: two solves of the same steps, normal equations against least\n"
            "squares on the augmented Jacobian; STEP_TOL of tests/test_gpu_basis.py is 16 x the largest |dp| / path)\n")
    f.write("\n".join(lines) + "\n")
