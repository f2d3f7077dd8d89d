"""Shared inputs of the `autophase_each` tests (CPU and GPU files): rows from the generator of
``scripts/check_device_search.py::make_slice`` and the oracle's answer for one row alone, computed once per row."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_gen = None
_oracle_rows = {}


def make_slice(n, seed):
    global _gen
    if _gen is None:
        spec = importlib.util.spec_from_file_location("_check_device_search",
                                                      os.path.join(ROOT, "scripts", "check_device_search.py"))
        _gen = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(_gen)
    return _gen.make_slice(n, seed)


def make_rows(n, seeds):
    """([len(seeds), n] complex128 spectra, their common frequency axis)."""
    rows, freq = [], None
    for s in seeds:
        spec, freq, _ = make_slice(n, s)
        rows.append(spec)
    return np.stack(rows), freq


def oracle_row(oracle, row, freq, key=None, **kw):
    """``oracle.autophase`` of the 1-D spectrum `row` alone (mode="single"); cached under `key` when one is given."""
    k = None if key is None else (key, tuple(sorted(kw.items())))
    if k is not None and k in _oracle_rows:
        return _oracle_rows[k]
    o = oracle.Labeled(np.array(row), ("frequency",), {"frequency": oracle.Coord("frequency", np.asarray(freq))}, {}, None)
    res = oracle.autophase(o, **kw)
    if k is not None:
        _oracle_rows[k] = res
    return res


def oracle_search(oracle, row, freq, p0_only=False):
    """The oracle's differential evolution on `row` alone: (OptimizeResult, target_idx, pivot)."""
    row = np.asarray(row)
    k = int(np.argmax(np.abs(row)))
    _, _, opt = oracle.autophase_solve(row.astype(np.complex128), np.asarray(freq), float(freq[k]), k, 1, "acme", p0_only)
    return opt, k, float(freq[k])
