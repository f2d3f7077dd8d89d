#!/usr/bin/env python3
"""Where PATH_TOL and RSS_TOL of tests/test_lm.py (the bounds of tests/test_gpu_lm.py) come from.  CPU only; the kernel's
own figures play no part in it.

Every case of tests/_lm_oracle.py: cases() is run by lm_fit twice at every trial cap of the GPU test (1, 2, 3, 5, 8, 13,
... up to and past the case's stopping trial): once solving the fp64 normal equations by a Cholesky factorisation, as the
kernel forms them, once by least squares on the augmented Jacobian [J; sqrt(lambda D)] in longdouble (Householder
reflections; J^T J is never formed).  Printed per case and cap: whether the two routes take the same decision at every
trial, the largest disagreement of a physical parameter and of an internal variable in units of its path length (the
sum of |change| over the accepted steps), the relative disagreement in rss, and the largest relative disagreement of a
deviation (recorded; the GPU test holds deviations to 64 eps cond).  The test's bounds are 16 x the largest figures of
the last line, which this tool also writes to profiles/lm/tolerance.txt."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _lm_oracle as orc  # noqa: E402

lines = []


def say(s):
    print(s)
    lines.append(s)


def in_path_units(a, b, path):
    d, moved = np.abs(a - b), path > 0
    assert np.all(d[~moved] == 0), "a parameter that never moved differs"
    return float(np.max(d[moved] / path[moved])) if moved.any() else 0.0


worst = {"p": 0.0, "u": 0.0, "rss": 0.0, "sd": 0.0}
agreeing, differing = [], []
for c in orc.cases():
    stop = orc.lm_fit(c, 100000)["iters"]
    for m in orc.caps(stop):
        a, b = (orc.lm_fit(c, m, route) for route in ("normal", "lstsq"))
        assert (a["iters"], a["status"]) == (b["iters"], b["status"]), (c.name, m)
        same = [t[0] for t in a["trials"]] == [t[0] for t in b["trials"]]
        (agreeing if same else differing).append((c.name, m))
        if a["status"] == 2 or not same:
            say(f"{c.name:18s} m={m:3d}: iters {a['iters']} status {a['status']}  same decisions: {same}")
            continue
        dp, du = in_path_units(a["params"], b["params"], a["path"]), in_path_units(a["u"], b["u"], a["path_u"])
        df = abs(a["rss"] - b["rss"]) / a["rss"] if a["rss"] > 0 else 0.0
        ok = np.isfinite(a["asd"]) & (a["asd"] > 0)
        assert np.array_equal(ok, np.isfinite(b["asd"]) & (b["asd"] > 0)), (c.name, m)
        ds = float(np.max(np.abs(a["asd"] - b["asd"])[ok] / a["asd"][ok])) if ok.any() else 0.0
        say(f"{c.name:18s} m={m:3d}: iters {a['iters']} status {a['status']}  same decisions: {same}  |dp|/path {dp:.2e}  "
            f"|du|/path {du:.2e}  rss rel {df:.2e} (rss {a['rss']:.2e})  sd rel {ds:.2e}")
        for k, v in (("p", dp), ("u", du), ("rss", df), ("sd", ds)):
            worst[k] = max(worst[k], v)
say(f"caps at which both routes take the same decisions (trajectories are compared there): {len(agreeing)} of "
    f"{len(agreeing) + len(differing)}" + ("" if not differing else f"; not at {differing}"))
say(f"largest |dp| / path {worst['p']:.2e}   largest |du| / path {worst['u']:.2e}   largest rss rel {worst['rss']:.2e}   "
    f"largest sd rel {worst['sd']:.2e}")
out = os.path.join(os.path.dirname(HERE), "profiles", "lm")
os.makedirs(out, exist_ok=True)
with open(os.path.join(out, "tolerance.txt"), "w") as f:
    f.write("python tests/tool_lm_tolerance.py  (CPU only: the same trials solved twice, fp64 normal equations against least\n"
            "squares on the augmented Jacobian in longdouble; PATH_TOL and RSS_TOL of tests/test_lm.py are 16 x the largest\n"
            "|dp| / path or |du| / path and the largest rss rel of the last line; sd rel is recorded)\n")
    f.write("\n".join(lines) + "\n")
