"""Measures what the tolerances of tests/test_lipids.py and tests/test_gpu_lipids.py are derived from (CPU only, the
kernel is not involved).  The output is committed as profiles/lipids/tolerance.txt:

    python tests/tool_lipids_tolerance.py > profiles/lipids/tolerance.txt

Over all parity cases of tests/_lipids_oracle.py, relative to the largest magnitude of the *input* row (the output is the
small remainder of a cancellation):
(a) the factorised route against the dense solve of (I + beta M M^H) x = y at full rank;
(b) the factorised route against itself with both sums in reversed order;
(c) the two routes to the basis (eigen-decomposition of the smaller Gram matrix, SVD of M), compared through the
    projector U diag(w) U^H, which depends on no phase choice (absolute: the projector's norm is at most 1).
Then the phantom's error against the truth before and after removal at the default level and two ranks."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _lipids_oracle as orc  # noqa: E402


def main():
    worst = {"a": 0.0, "b": 0.0, "c": 0.0}
    print("(a) factorised vs dense solve, (b) vs reversed sums (of max |y| of the row); (c) projector, eig vs svd route")
    for n, T, r in orc.CASES + orc.CLASS_CASES:
        c = orc.make_case(n, T, r)
        be = orc.basis(c["L"], c["level"], r, route="eig")
        bs = orc.basis(c["L"], c["level"], r, route="svd")
        out = orc.apply(c["y"], be["U"], be["w"])
        a = orc.rel_err(out, orc.dense(c["y"], c["L"], c["level"]), c["y"])
        b = orc.rel_err(out, orc.apply(c["y"], be["U"], be["w"], reverse=True), c["y"])
        cc = float(np.abs(orc.projector(be["U"], be["w"]) - orc.projector(bs["U"], bs["w"])).max())
        print(f"  rows={n:3d} T={T:5d} rank={r:3d}  dense {a:.3e}  reversed {b:.3e}  projector {cc:.3e}")
        worst = {"a": max(worst["a"], a), "b": max(worst["b"], b), "c": max(worst["c"], cc)}
    print("measured, the largest over all cases:")
    for k in "abc":
        print(f"  ({k}) {worst[k]:.3e}")
    ph = orc.phantom()
    print(f"phantom {ph['data'].shape[0]} x {ph['data'].shape[1]}, {int(ph['scalp'].sum())} scalp and "
          f"{int(ph['brain'].sum())} brain voxels, T = {ph['data'].shape[2]}: error of the brain voxels against the truth")
    print(f"  untreated {orc.phantom_error(ph['data'], ph):.4f}")
    for rank in (None, 16, 32):
        out, b = orc.remove(ph["data"], ph["scalp"], 0.01, rank)
        print(f"  level 0.01 rank {str(rank):>4s} (kept {b['rank']:2d}, dropped weight {b['dropped_weight']:.3e})  "
              f"error {orc.phantom_error(out, ph):.4f}")


if __name__ == "__main__":
    main()
