"""Shared by `test_gpu_search_kernel.py`, `scripts/check_device_search.py` and `scripts/dump_search_records.py`: the
pinned cases of the device search (csrc/xm_search.hip), one search into a pinned record under a Python deadline, the
host engine's answer for the same slice, and the record layouts as numpy dtypes."""
import time

import numpy as np

import _each_rows

# (n, points per worker P, seeds of `_each_rows.make_slice`).  n = 448 P is the kernels' FULL instantiation.  At every
# seed the device search and the host engine agree for p0_only = 0 and 1 (profiles/r04/device_search.txt for n >= 1000;
# the flat-landscape slices n = 8192 seed 819206 and n = 1000 seed 100002, where they part, are left out; the seeds at
# n = 448 and 300 are the first two at which the host engine's landscape is an ordinary one -- 30000 is not: 67
# generations with p0_only).
CASES = (
    (16384, 37, (1638400, 1638401)),
    (8192, 19, (819200, 819201, 819202, 819203)),
    (4096, 10, (409600, 409601)),
    (2048, 5, (204800, 204801)),
    (1000, 3, (100000, 100001)),
    (896, 2, (7000, 7001, 7002)),          # FULL; FULL_SEEDS[:3] of test_gpu_autophase_each.py
    (512, 2, (7000, 7001, 7002, 7003)),    # SEEDS[:4] of the same file
    (448, 1, (44800, 44801)),              # FULL
    (300, 1, (30001, 30002)),
)
CASE_LIST = tuple((n, s) for n, _, seeds in CASES for s in seeds)

# xm_search_result (128 bytes) and the nine fields it shares with xm_search_row (`device.SEARCH_ROW_DTYPE`)
RESULT_DTYPE = np.dtype([("x", "<f8", (2,)), ("fun", "<f8"), ("pg_norm", "<f8"), ("nfev", "<i4"), ("nit", "<i4"),
                         ("status", "<i4"), ("needs_polish", "<i4"), ("target_idx", "<i4"), ("pad_", "<i4"),
                         ("seq", "<u8"), ("t_us", "<f8", (8,))])
SHARED = ("x", "fun", "pg_norm", "nfev", "nit", "status", "needs_polish", "target_idx", "pad_")
PGTOL_RULE = 0.5e-5  # needs_polish = pg_norm > 0.5e-5 (both engines)
DEADLINE_S = 20.0

_seq = [0]


def next_seq():
    _seq[0] += 1
    return _seq[0]


def wait_done(dev, records, seq, deadline=DEADLINE_S):
    """Polls until every record carries `seq`; raises after `deadline` seconds."""
    t0 = time.perf_counter()
    while not all(dev.search_done(r, seq) for r in records):
        if time.perf_counter() - t0 > deadline:
            raise TimeoutError("search did not finish")


def run_search(dev, sl_pinned, axis, rec, seq, p0_only, stream=None):
    """`search_launch` into `rec`, then its fields as `device.read_search_record` gives them."""
    dev.search_launch(sl_pinned, axis, rec, seq, p0_only=p0_only, stream=stream)
    wait_done(dev, [rec], seq)
    return dev.read_search_record(rec)


def shared_fields(rec):
    """The nine shared fields of an `xm_search_result` (a pinned int64[16] tensor) or of one `SEARCH_ROW_DTYPE` element,
    each as bytes."""
    a = rec if isinstance(rec, np.void) else rec.numpy().view(RESULT_DTYPE)[0]
    return {f: np.asarray(a[f]).tobytes() for f in SHARED}


def host_answer(spec, freq, k, p0_only):
    """The host engine on the same slice: (status, x, fun, nfev, nit) of `NativeObjective.de` and the host's
    needs_polish rule from `obj.fg` (scripts/check_device_search.py)."""
    from xmris_amd import autophase_solver as aps

    obj = aps.NativeObjective(spec, freq, float(freq[k]), k, 1, "acme")
    rc, x, fun, nfev, nit = obj.de(p0_only)
    lo, hi = np.array([-180.0, -4000.0])[:len(x)], np.array([180.0, 4000.0])[:len(x)]
    _, g0 = obj.fg(np.clip(x, lo, hi), lo, hi)
    pg = np.where(g0 < 0, np.maximum(x - hi, g0), np.minimum(x - lo, g0))
    pgn = float(np.abs(pg).max())
    return dict(status=rc, x=np.array(x), fun=fun, nfev=nfev, nit=nit, pg_norm=pgn, needs_polish=pgn > PGTOL_RULE)


def equals_host(r, host, k):
    """(x, nfev, nit, status, target_idx equal exactly; needs_polish equal) of a `read_search_record` dict."""
    xd = np.array(r["x"][:len(host["x"])])
    same = (np.array_equal(xd, host["x"]) and r["nfev"] == host["nfev"] and r["nit"] == host["nit"] and
            r["target_idx"] == k and r["status"] == host["status"])
    return same, r["needs_polish"] == host["needs_polish"]


def rows_record(dev, spec, axis, k, p0_only):
    """`search_rows` on `spec` as a one-row complex128 tensor.  With p0_only the pivot and the target bin are GIVEN (the
    arg-max's, in the kernel's own expression c0 + k cstep), so the pivot override runs and the search is still the
    single one's."""
    row = dev.to_device(np.ascontiguousarray(spec[None, :], dtype=np.complex128))
    if p0_only:
        return dev.search_rows(row, axis, p0_only=True, pivot=axis[0] + axis[1] * float(k), target_idx=k)[0]
    return dev.search_rows(row, axis)[0]


def eval_points(seed):
    """16 points of the (p0, p1) box, drawn as scripts/check_device_search.py draws them."""
    rng = np.random.default_rng(seed % 100)
    return np.stack([rng.uniform(-180, 180, 16), rng.uniform(-4000, 4000, 16)], 1)


def eval_reference(xs, spec, freq, k):
    from xmris_amd import autophase_solver as aps

    return np.array([aps.acme_score(x, spec, freq, float(freq[k])) for x in xs])


make_slice = _each_rows.make_slice
