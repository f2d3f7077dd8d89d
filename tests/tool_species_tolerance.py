"""Measures what the GPU tests of k_species may allow, on the CPU alone (the kernel is not involved); its output is
committed as profiles/species/tolerance.txt:

    python tests/tool_species_tolerance.py > profiles/species/tolerance.txt

(a) the factorised known-field estimate against per-row numpy.linalg.lstsq on A_r, and against the same sum in reversed
    echo order, relative to the largest magnitude of the case;
(b) psi* of the restated iteration against scipy.optimize.brentq on G' in the same bracket, W summed over the columns in
    reversed order, in units of the grid spacing delta;
(c) `residual` between the two routes of (b)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _species_oracle as orc  # noqa: E402

TOOL_ROWS, TOOL_COLS = 65, 3


def measure(out=None):
    say = (lambda *a: None) if out is None else (lambda *a: print(*a, file=out))
    a_lstsq = a_rev = b = c = 0.0
    say("(a) known field: factorised estimate vs per-row lstsq, and vs the reversed echo order (relative to max |rho|)")
    for k, (E, M) in enumerate(orc.KNOWN_EM):
        cs = orc.make_case(E, M, TOOL_ROWS, TOOL_COLS, 10 + k)
        est = orc.known(cs["y"], cs["te"], cs["f"], cs["r"], cs["tau"], cs["psi"])
        scale = np.abs(est).max()
        e1 = np.abs(est - orc.lstsq_rows(cs["y"], cs["te"], cs["f"], cs["r"], cs["tau"], cs["psi"])).max() / scale
        e2 = np.abs(est - orc.known(cs["y"], cs["te"], cs["f"], cs["r"], cs["tau"], cs["psi"], reverse=True)).max() / scale
        cond = np.linalg.cond(orc.a0(cs["te"], cs["f"], cs["r"]))
        say(f"  E={E:2d} M={M} rows={TOOL_ROWS} cols={TOOL_COLS} cond(A0)={cond:9.3e}  lstsq {e1:.3e}  reversed {e2:.3e}")
        a_lstsq, a_rev = max(a_lstsq, e1), max(a_rev, e2)
    say("(b), (c) field fit: restated iteration vs brentq with W in reversed column order")
    for name, E, M, rows, cols, n_grid, seed in orc.fit_cases():
        cs = orc.make_fit_case(E, M, rows, cols, n_grid, seed)
        delta, Gn = orc.grid(cs["te"], cs["max_field"])
        Pi = orc.projector(orc.a0(cs["te"], cs["f"], cs["r"]))
        eb = ec = 0.0
        for i in range(rows):
            o = orc.fit_row(cs["y"][i], cs["te"], cs["f"], cs["r"], cs["tau"][i], cs["max_field"], Pi)
            alt = orc.brent_row(cs["y"][i], cs["te"], cs["f"], cs["r"], cs["max_field"], o["g"], Pi)
            assert o["status"] == 0 and alt is not None, (name, i, o["status"])
            eb, ec = max(eb, abs(alt[0] - o["field"]) / delta), max(ec, abs(alt[1] - o["residual"]))
        say(f"  {name:18s} grid {2 * Gn + 1:4d}  psi* {eb:.3e} delta  residual {ec:.3e}")
        b, c = max(b, eb), max(c, ec)
    res = dict(a=max(a_lstsq, a_rev), a_lstsq=a_lstsq, a_reversed=a_rev, b=b, c=c)
    say("measured, the largest over all cases:")
    say(f"  (a) {res['a']:.3e}   (lstsq {a_lstsq:.3e}, reversed {a_rev:.3e})")
    say(f"  (b) {b:.3e}")
    say(f"  (c) {c:.3e}")
    return res


if __name__ == "__main__":
    measure(sys.stdout)
