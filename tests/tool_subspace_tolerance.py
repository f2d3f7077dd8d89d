"""TOOL (not a test): measures on the CPU what the tolerances of tests/test_subspace.py and tests/test_gpu_subspace.py are
made from, and writes profiles/subspace/tolerance.txt.  Run from the repository root: python tests/tool_subspace_tolerance.py

* the disagreement of two routes of the oracle after ITERATIONS iterations, relative to max |x|: the dense normal matrix
  against the staged operator (complex128), and the staged operator with every coil-sized intermediate rounded to
  complex64 against the same without rounding (on the complex64-rounded data).  The GPU tests allow 16 x the largest.
* the benefit on radial2d with a quarter of the (sample, time) positions kept: the error against the truth of the subspace
  solve, of the per-column solve of the fully sampled data and of the zero-filled per-column solve."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _cgsense_oracle as cg  # noqa: E402
import _subspace_oracle as orc  # noqa: E402

ITERATIONS = 6
CASES = ("radial2d", "masked2d", "odd2d", "line1d", "random3d")


def main():
    lines, gap128, gap64 = [], 0.0, 0.0
    for name in CASES:
        for keep in (1.0, 0.5):
            for frames in (1, 4):
                p = orc.problem(name, keep, frames)
                dense = p.image(p.folded(p.dense(), p.rhs(), ITERATIONS)[0])
                staged = p.image(p.folded(p.staged(), p.staged_rhs(), ITERATIONS)[0])
                y64 = cg.c64(p.y)
                plain = p.image(p.folded(p.staged(), p.staged_rhs(y=y64), ITERATIONS)[0])
                rounded = p.image(p.folded(p.staged(cg.c64), p.staged_rhs(cg.c64, y64), ITERATIONS)[0])
                g128, g64 = cg.rel(staged, dense), cg.rel(rounded, plain)
                gap128, gap64 = max(gap128, g128), max(gap64, g64)
                lines.append(f"routes {name} keep {keep} frames {frames}: complex128 {g128:.3e} complex64 {g64:.3e}")
    lines.append(f"largest route disagreement: {gap128:.3e}")
    lines.append(f"largest complex64 rounding gap: {gap64:.3e}")
    lines.append(f"SUB_TOL128 = {16 * gap128:.3e}")
    lines.append(f"SUB_TOL64 = {16 * gap64:.3e}")
    p = orc.problem("radial2d", 0.25)
    sub, full, zf = (orc.err(x, p.truth) for x in (p.image(p.solve()), p.per_column(p.full), p.per_column(p.y)))
    lines.append(f"benefit radial2d keep 0.25: subspace {sub:.3f} fully sampled {full:.3f} zero-filled {zf:.3f}")
    text = "\n".join(lines) + "\n"
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "subspace", "tolerance.txt")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        fh.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
