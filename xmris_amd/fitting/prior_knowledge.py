"""Reader of AMARES prior knowledge in the CSV layout of the reference's fitting notebook
(docs/notebooks/fitting/pyamares.md:85-98):

    Index,PCr,ATP                       <- one column per peak, named
    Initial Values,,
    amplitude,10.0,5.0                  <- rows amplitude, chemicalshift [ppm], linewidth [Hz], phase [deg], g
    ...
    Bounds,,
    amplitude,"(0, ","(0, "             <- "(lo, hi)"; an empty side is unbounded, an empty cell unbounded on both
    ...

Initial values are clipped into their bounds; lo == hi fixes a parameter.  Anything else -- spreadsheets, expression or
link cells, unknown rows, non-numeric values -- is refused with a ValueError that names the row and the column.
"""
from __future__ import annotations

import csv
import math
from dataclasses import dataclass
from pathlib import Path

import numpy as np

ROWS = ("amplitude", "chemicalshift", "linewidth", "phase", "g")
_REQUIRED_INITIAL = ("amplitude", "chemicalshift", "linewidth")
_DEFAULT_INITIAL = {"phase": 0.0, "g": 0.0}


@dataclass
class PriorKnowledge:
    """names [K]; init / lo / hi [K, 5] in the file's units (columns in ROWS order); fixed [K, 5] bool."""

    names: list
    init: np.ndarray
    lo: np.ndarray
    hi: np.ndarray
    fixed: np.ndarray

    def fitting_units(self, mhz: float):
        """(init, lo, hi) in the units of the fit: a, f = ppm * mhz [Hz], d = pi * linewidth [1/s], phi [rad], g."""
        scale = np.array([1.0, float(mhz), math.pi, math.pi / 180.0, 1.0])
        return self.init * scale, self.lo * scale, self.hi * scale


def _number(text: str, where: str) -> float:
    try:
        v = float(text)
    except ValueError:
        raise ValueError(f"prior knowledge {where}: {text!r} is not a number (expressions and links are not "
                         f"supported)") from None
    if math.isnan(v):
        raise ValueError(f"prior knowledge {where}: NaN is not allowed")
    return v


def _bound(text: str, where: str):
    s = text.strip()
    if not s:
        return -math.inf, math.inf
    if not s.startswith("("):
        raise ValueError(f"prior knowledge {where}: bound {text!r} must be written '(lo, hi)'")
    s = s[1:]
    if s.endswith(")"):
        s = s[:-1]
    parts = s.split(",")
    if len(parts) != 2:
        raise ValueError(f"prior knowledge {where}: bound {text!r} must be written '(lo, hi)'")
    lo = -math.inf if not parts[0].strip() else _number(parts[0].strip(), where)
    hi = math.inf if not parts[1].strip() else _number(parts[1].strip(), where)
    if lo > hi:
        raise ValueError(f"prior knowledge {where}: lower bound {lo} above upper bound {hi}")
    return lo, hi


def read_prior_knowledge(path) -> PriorKnowledge:
    path = Path(path)
    if path.suffix.lower() != ".csv":
        raise ValueError(f"prior knowledge {path.name!r}: only the CSV format is supported")
    with open(path, newline="", encoding="utf-8") as fh:
        rows = [r for r in csv.reader(fh) if any(c.strip() for c in r)]
    if not rows or rows[0][0].strip() != "Index":
        raise ValueError(f"prior knowledge {path.name!r}: the first row must be 'Index,<peak name>,...'")
    names = [c.strip() for c in rows[0][1:]]
    while names and not names[-1]:
        names.pop()
    if not names or any(not n for n in names) or len(set(names)) != len(names):
        raise ValueError(f"prior knowledge {path.name!r}: peak names in the header must be present and distinct")
    k = len(names)
    cells = {"Initial Values": {}, "Bounds": {}}
    section = None
    for ln, r in enumerate(rows[1:], start=2):
        head = r[0].strip()
        body = [c for c in r[1:]] + [""] * max(0, k - len(r) + 1)
        if any(c.strip() for c in body[k:]):
            raise ValueError(f"prior knowledge row {ln} ({head!r}): more cells than peaks")
        if head in cells:
            if any(c.strip() for c in body[:k]):
                raise ValueError(f"prior knowledge row {ln}: section header {head!r} must have empty cells")
            section = head
            continue
        if head not in ROWS:
            raise ValueError(f"prior knowledge row {ln}: unknown row {head!r} (expected one of {', '.join(ROWS)})")
        if section is None:
            raise ValueError(f"prior knowledge row {ln} ({head!r}): outside the 'Initial Values' / 'Bounds' sections")
        if head in cells[section]:
            raise ValueError(f"prior knowledge row {ln}: {head!r} appears twice in {section!r}")
        cells[section][head] = (ln, body[:k])

    init = np.zeros((k, 5))
    lo = np.full((k, 5), -math.inf)
    hi = np.full((k, 5), math.inf)
    for c, row in enumerate(ROWS):
        if row in cells["Initial Values"]:
            ln, vals = cells["Initial Values"][row]
            for j, v in enumerate(vals):
                init[j, c] = _number(v.strip(), f"row {ln} ({row!r}), column {names[j]!r}")
        elif row in _REQUIRED_INITIAL:
            raise ValueError(f"prior knowledge {path.name!r}: the 'Initial Values' section has no {row!r} row")
        else:
            init[:, c] = _DEFAULT_INITIAL[row]
        if row in cells["Bounds"]:
            ln, vals = cells["Bounds"][row]
            for j, v in enumerate(vals):
                lo[j, c], hi[j, c] = _bound(v, f"row {ln} ({row!r}), column {names[j]!r}")
    init = np.clip(init, lo, hi)
    return PriorKnowledge(names=names, init=init, lo=lo, hi=hi, fixed=lo == hi)
