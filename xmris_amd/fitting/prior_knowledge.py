"""Reader of AMARES prior knowledge in the CSV layout of the reference's fitting notebook
(docs/notebooks/fitting/pyamares.md:85-98):

    Index,PCr,ATP                       <- one column per peak, named
    Initial Values,,
    amplitude,10.0,5.0                  <- rows amplitude, chemicalshift [ppm], linewidth [Hz], phase [deg], g
    ...
    Bounds,,
    amplitude,"(0, ","(0, "             <- "(lo, hi)"; an empty side is unbounded, an empty cell unbounded on both
    ...

Initial values are clipped into their bounds; lo == hi fixes a parameter.

Links.  A cell of the Initial Values section may name another peak instead of a number: the parameter then follows
that peak's parameter of the same row as ``p = scale * p_root + offset``.  Grammar of such a cell:

    [num *] NAME [/ num] [(+ | -) num [Hz | ppm]]        BATP   BATP/2   2*BATP   BATP-15Hz   PCr+0.1   3*BATP/2-1

A factor stands in front of the name and a divisor behind it; a factor behind the name (``PCr*0.5``) stays refused, as
it always was -- write ``0.5*PCr`` or ``PCr/2``.

NAME is one of the header's peak names (the longest name that fits is taken).  A unit may follow the offset in the
chemicalshift row only: ``ppm`` is that row's own unit, ``Hz`` is divided by the spectrometer frequency once it is known
(``fitting_units`` / ``fitting_links``).  pyAMARES is not available to this project: the grammar is this project's
own, written to read like pyAMARES's prior-knowledge spreadsheets, and is not a port of their expression language.
Rules: chains are composed (C = B/2, B = 2*A+1 gives C = A + 0.5), so every link ends at an unlinked root; a cell that
names its own column, a cycle, an unknown name, a zero factor, a division by zero or a unit in another row are
refused.  THE BOUNDS CELL OF A LINKED PARAMETER IS NOT APPLIED (it is still checked for syntax): the root's bounds
carry through the affine map, so the follower ranges over scale * [lo, hi] + offset of its root.  A follower of a
fixed root is fixed at the mapped value.  The initial value of a follower is the mapped, clipped value of its root.

Anything else -- spreadsheets, other expressions, unknown rows, non-numeric values -- is refused with a ValueError that
names the row and the column.
"""
from __future__ import annotations

import csv
import math
import re
from dataclasses import dataclass
from pathlib import Path

import numpy as np

ROWS = ("amplitude", "chemicalshift", "linewidth", "phase", "g")
_REQUIRED_INITIAL = ("amplitude", "chemicalshift", "linewidth")
_DEFAULT_INITIAL = {"phase": 0.0, "g": 0.0}


@dataclass
class PriorKnowledge:
    """names [K]; init / lo / hi [K, 5] in the file's units (columns in ROWS order); fixed [K, 5] bool (followers of a
    fixed root included).  Links, all [K, 5]: link_to -- the root's parameter index 5 k' + c, or -1; link_scale;
    link_offset in the file's units, except where link_offset_hz is set (chemicalshift offsets written in Hz): those are
    in Hz.  A follower's lo / hi are unbounded (its Bounds cell is not applied); its init is the mapped root value, NaN
    while an offset in Hz awaits the spectrometer frequency (fitting_units gives it)."""

    names: list
    init: np.ndarray
    lo: np.ndarray
    hi: np.ndarray
    fixed: np.ndarray
    link_to: np.ndarray = None
    link_scale: np.ndarray = None
    link_offset: np.ndarray = None
    link_offset_hz: np.ndarray = None

    def __post_init__(self):
        shape = np.shape(self.init)
        if self.link_to is None:
            self.link_to = np.full(shape, -1, dtype=np.int32)
        if self.link_scale is None:
            self.link_scale = np.ones(shape)
        if self.link_offset is None:
            self.link_offset = np.zeros(shape)
        if self.link_offset_hz is None:
            self.link_offset_hz = np.zeros(shape, dtype=bool)

    @staticmethod
    def _scale(mhz: float):
        return np.array([1.0, float(mhz), math.pi, math.pi / 180.0, 1.0])

    def fitting_links(self, mhz: float):
        """(link_to, link_scale, link_offset) with the offsets in the units of the fit: x mhz for an offset in ppm (one
        written in Hz is taken as it is), x pi for a linewidth, x pi / 180 for a phase."""
        off = np.where(self.link_offset_hz, self.link_offset, self.link_offset * self._scale(mhz))
        return self.link_to.copy(), self.link_scale.copy(), off

    def fitting_units(self, mhz: float):
        """(init, lo, hi) in the units of the fit: a, f = ppm * mhz [Hz], d = pi * linewidth [1/s], phi [rad], g.
        The init of a follower is its link applied to the root's init, in these units."""
        scale = self._scale(mhz)
        init = self.init * scale
        to, sc, off = self.fitting_links(mhz)
        q = np.flatnonzero(to.ravel() >= 0)
        init.ravel()[q] = sc.ravel()[q] * init.ravel()[to.ravel()[q]] + off.ravel()[q]
        return init, self.lo * scale, self.hi * scale


def _number(text: str, where: str) -> float:
    try:
        v = float(text)
    except ValueError:
        raise ValueError(f"prior knowledge {where}: {text!r} is not a number") from None
    if math.isnan(v):
        raise ValueError(f"prior knowledge {where}: NaN is not allowed")
    return v


_NUM = r"(?:\d+\.?\d*|\.\d+)(?:[eE][+-]?\d+)?"
_LINK_HEAD = re.compile(rf"\s*(?:([+-]?{_NUM})\s*\*)?\s*")
_LINK_TAIL = re.compile(rf"\s*(?:/\s*([+-]?{_NUM}))?\s*(?:([+-])\s*({_NUM})\s*(Hz|ppm)?)?\s*")


def _link(text: str, names: list, row: str, where: str):
    """A link cell -> (root column, scale, offset, offset is in Hz).  ValueError when `text` is not one."""
    for name in sorted(names, key=len, reverse=True):
        at = text.find(name)
        while at >= 0:
            head = _LINK_HEAD.fullmatch(text[:at])
            tail = _LINK_TAIL.fullmatch(text[at + len(name):])
            if head and tail:
                scale = float(head.group(1)) if head.group(1) else 1.0
                if tail.group(1):
                    f = float(tail.group(1))
                    if f == 0.0:
                        raise ValueError(f"prior knowledge {where}: {text!r} divides by zero")
                    scale /= f
                if scale == 0.0 or not math.isfinite(scale):
                    raise ValueError(f"prior knowledge {where}: {text!r} has a zero factor: a link needs a finite, "
                                     f"nonzero scale")
                offset = float(tail.group(3)) * (-1.0 if tail.group(2) == "-" else 1.0) if tail.group(2) else 0.0
                unit = tail.group(4)
                if unit and row != "chemicalshift":
                    raise ValueError(f"prior knowledge {where}: {text!r}: the unit {unit!r} is allowed in the "
                                     f"'chemicalshift' row only")
                return names.index(name), scale, offset, unit == "Hz"
            at = text.find(name, at + 1)
    if any(name in text for name in names):
        raise ValueError(f"prior knowledge {where}: {text!r} is not a link of the form "
                         f"'[num *] NAME [/ num] [(+ | -) num [Hz | ppm]]' (a factor goes in front of the name)")
    raise ValueError(f"prior knowledge {where}: {text!r} is neither a number nor a link to one of the peaks "
                     f"{', '.join(names)} (unknown name)")


def _is_number(text: str) -> bool:
    try:
        float(text)
    except ValueError:
        return False
    return True


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
    link_to = np.full((k, 5), -1, dtype=np.int32)
    link_scale, link_offset = np.ones((k, 5)), np.zeros((k, 5))
    link_hz = np.zeros((k, 5), dtype=bool)
    where_of = {}
    for c, row in enumerate(ROWS):
        if row in cells["Initial Values"]:
            ln, vals = cells["Initial Values"][row]
            for j, v in enumerate(vals):
                where = f"row {ln} ({row!r}), column {names[j]!r}"
                if _is_number(v.strip()) or not v.strip():
                    init[j, c] = _number(v.strip(), where)
                    continue
                root, link_scale[j, c], link_offset[j, c], link_hz[j, c] = _link(v.strip(), names, row, where)
                if root == j:
                    raise ValueError(f"prior knowledge {where}: {v.strip()!r} links the parameter to itself")
                link_to[j, c] = 5 * root + c
                where_of[(j, c)] = where
        elif row in _REQUIRED_INITIAL:
            raise ValueError(f"prior knowledge {path.name!r}: the 'Initial Values' section has no {row!r} row")
        else:
            init[:, c] = _DEFAULT_INITIAL[row]
        if row in cells["Bounds"]:
            ln, vals = cells["Bounds"][row]
            for j, v in enumerate(vals):
                lo[j, c], hi[j, c] = _bound(v, f"row {ln} ({row!r}), column {names[j]!r}")
    # compose chains down to an unlinked root: p = s1 (s2 r + o2) + o1
    done = set()

    def compose(j, c, stack):
        if link_to[j, c] < 0 or (j, c) in done:
            return
        if j in stack:
            raise ValueError(f"prior knowledge {where_of[(j, c)]}: the links of this row form a cycle ("
                             f"{' -> '.join(names[i] for i in stack + [j])})")
        m = link_to[j, c] // 5
        compose(m, c, stack + [j])
        if link_to[m, c] >= 0:
            if link_offset[j, c] != 0.0 and link_offset[m, c] != 0.0 and link_hz[j, c] != link_hz[m, c]:
                raise ValueError(f"prior knowledge {where_of[(j, c)]}: the chain through {names[m]!r} mixes offsets "
                                 f"in Hz and in ppm")
            if link_offset[j, c] == 0.0:
                link_hz[j, c] = link_hz[m, c]
            link_offset[j, c] += link_scale[j, c] * link_offset[m, c]
            link_scale[j, c] *= link_scale[m, c]
            link_to[j, c] = link_to[m, c]
        done.add((j, c))

    for j, c in where_of:
        compose(j, c, [])
    linked = link_to >= 0
    lo[linked], hi[linked] = -math.inf, math.inf  # a follower's Bounds cell is not applied
    init = np.clip(init, lo, hi)
    fixed = lo == hi
    roots = link_to.ravel()[linked.ravel()]
    init[linked] = link_scale[linked] * init.ravel()[roots] + link_offset[linked]
    init[linked & link_hz] = math.nan  # needs the spectrometer frequency: fitting_units(mhz)
    fixed[linked] = fixed.ravel()[roots]
    return PriorKnowledge(names=names, init=init, lo=lo, hi=hi, fixed=fixed, link_to=link_to, link_scale=link_scale,
                          link_offset=link_offset, link_offset_hz=link_hz)
