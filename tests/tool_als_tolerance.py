#!/usr/bin/env python3
"""Where the AsLS bounds of tests/_als_oracle.py come from.  CPU only; the kernel is not involved.

For every case of _als_oracle.CASES, with the spectra as float64 and rounded to float32, relative to each row's scale
max |y| and taken over the rows of the case:

  e64     the float64 run of the band-LDL' recurrence against its long-double run (the largest row);
  scipy   the oracle (`als_core` of oracle/xmris_oracle.py, scipy's spsolve) against the long-double run (the largest row);
  margin  the smallest |y - z| at any point after any iteration of the long-double run (the smallest row).

The GPU bound of a (lam, p) is 16 x the largest e64 among its cases; a case is usable when its margin is at least 64 x
that bound.  With `--seeds K` the tool also reports, for every case, the first seed of 1 ... K that is usable.

    python tests/tool_als_tolerance.py > profiles/als/tolerance.txt
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
import _als_oracle as orc  # noqa: E402
import xmris_oracle  # noqa: E402


def figures(case, single):
    return orc.figures(case, single, xmris_oracle.als_core)


def main():
    n_seeds = int(sys.argv[sys.argv.index("--seeds") + 1]) if "--seeds" in sys.argv else 0
    print(f"np.longdouble eps {float(np.finfo(np.longdouble).eps):.3e}; figures relative to max |y| of the row")
    rows, worst = [], {}
    for case in orc.CASES:
        for single in (False, True):
            e64, esp, margin = figures(case, single)
            rows.append((case, single, e64, esp, margin))
            key = case[2][:2]
            worst[key] = max(worst.get(key, 0.0), e64)
    for case, single, e64, esp, margin in rows:
        need = 64 * 16 * worst[case[2][:2]]
        print(f"{orc.case_id(case):38s} {'float32' if single else 'float64'} rows: e64 {e64:.3e}  scipy {esp:.3e} "
              f"({esp / e64 if e64 else float('inf'):6.2f} e64)  margin {margin:.3e} ({margin / need:9.2f} x the {need:.3e} needed)")
    print()
    for (lam, p), e in worst.items():
        print(f"lam {lam:g} p {p:g}: largest e64 {e:.3e}, bound 16 x = {16 * e:.3e}, margin needed 64 x = {64 * 16 * e:.3e}")
    if n_seeds:
        print()
        for case in orc.CASES:
            need = 64 * 16 * worst[case[2][:2]]
            good = next((s for s in range(1, n_seeds + 1)
                         if min(figures(case[:3] + (s,), single)[2] for single in (False, True)) >= need), None)
            print(f"{orc.case_id(case):38s} first usable seed: {good}")


if __name__ == "__main__":
    main()
