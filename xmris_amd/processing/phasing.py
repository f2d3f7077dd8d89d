"""Manual and automatic phase correction on the GPU.

Host-side mirror of the reference's ``src/xmris/processing/phasing.py``: ``phase`` applies one
(p0, p1, pivot) ramp to the whole N-D array (one broadcast-multiply launch); ``autophase``
(mode="single") finds the global |X| maximum on the device, optimises (p0, p1) on that ONE 1-D
slice on the host (same scipy differential evolution as the reference) and applies the result to
everything.
"""
from __future__ import annotations

import copy as _copy
import warnings

import numpy as np

from .. import autophase_solver as aps
from .. import device as dev
from ..config import ATTRS, DIMS
from ..dims import MSG_METHOD, MSG_MODE, MSG_MODE_ALL, _check_dims, msg_phase_units
from ._common import (Coordinate, LabeledArray, as_labeled, binary_op_name, device_data, like_input,
                      promote_for_float64_operand, to_host)


def _global_argmax(src: LabeledArray, x):
    """phasing.py:229-231 / 50-52: flat arg-max of |values| in C order, unravelled."""
    _, flat = dev.absmax_argmax(x)
    return flat, np.unravel_index(flat, src.shape)


def _phase_labeled(src: LabeledArray, x, dim, p0, p1, pivot) -> LabeledArray:
    coords = src.coords[dim].values
    table = aps.phase_table(coords, p0, p1, pivot)  # fp64 on the host (phasing.py:56-73)
    y = dev.phase_apply(promote_for_float64_operand(x), src.get_axis_num(dim), table)  # * complex128 (phasing.py:73)
    out = src.copy(data=y)
    out.name = binary_op_name(src, dim)
    out.attrs = _copy.copy(src.attrs)  # phasing.py:76
    if pivot is not None and ATTRS.phase_pivot_coord in out.attrs:  # phasing.py:79-88
        old = out.attrs[ATTRS.phase_pivot_coord]
        if old != dim:
            warnings.warn(msg_phase_units(dim, old, pivot))  # phasing.py:84-88
    out.attrs[ATTRS.phase_p0] = p0  # phasing.py:91-94
    out.attrs[ATTRS.phase_p1] = p1
    out.attrs[ATTRS.phase_pivot] = pivot
    out.attrs[ATTRS.phase_pivot_coord] = dim
    return out


def phase(da, dim: str = DIMS.frequency, p0: float = 0.0, p1: float = 0.0, pivot: float = None):
    """Zero- and first-order phase correction, phi = rad(p0) + rad(p1)*(c - pivot)/(max c - min c)
    (reference ``phasing.py:10-96``).  Default pivot: coordinate of the global |X| maximum."""
    src = as_labeled(da)
    _check_dims(src, dim, "phase")
    x, _ = device_data(src)
    if pivot is None:  # phasing.py:49-53
        _, idx = _global_argmax(src, x)
        pivot = float(src.coords[dim].values[idx[src.get_axis_num(dim)]])
    return like_input(_phase_labeled(src, x, dim, p0, p1, pivot), da)


def _fused_chain(src: LabeledArray, dim, method, peak_width, target_coord, p0_only, lb):
    """`autophase` on a spectrum that is still a RECORDED chain to_spectrum(apodize_exp([zero_fill](fid))) along one
    dim: run the fused kernels (`fused.spectral_pipeline`: two passes over the data instead of six, no intermediate
    is ever materialised) on the chain's root.  Returns None when the pattern does not apply (anything else was
    recorded, an intermediate was looked at, the FID axis is not the last one, autophase's own `lb` is set)."""
    if not src.is_deferred or lb > 0:
        return None
    steps, root = src.pending_chain()
    names = ["apodize" if s_[0] in ("apodize_exp", "apodize_lg") else s_[0] for s_ in steps]
    if names not in (["to_spectrum", "apodize", "zero_fill"], ["to_spectrum", "apodize"]):
        return None
    sp, ap = steps[0][1], steps[1][1]
    lg = steps[1][0] == "apodize_lg"
    zf = steps[2][1] if len(steps) == 3 else None
    d0 = sp["dim"]
    if sp["out_dim"] != dim or ap["dim"] != d0 or (zf is not None and zf["dim"] != d0):
        return None
    if d0 not in root.dims or root.get_axis_num(d0) != root.ndim - 1:
        return None
    if not np.issubdtype(root.dtype, np.complexfloating):
        return None
    from ..fused import spectral_pipeline

    # The fused path regenerates coordinates and attrs from the ROOT.  A caller may have edited an intermediate of the
    # recorded chain without looking at its data (`zf.coords["time"] = ...`, `zf.attrs[...] = ...`): the staged chain
    # honours such edits, so the fused path only runs when every intermediate still carries what the recording call
    # produced (the coordinate of the FID axis and the attrs are compared with a regenerated chain of metadata).
    if not _chain_metadata_untouched(src, root, steps):
        return None
    # the staged chain is complex128 from apodize_exp on (`_promote`); host-resident roots stay on the host here: the
    # fused front end uploads them chunk by chunk, overlapped with the passes
    base = root
    n = root.sizes[d0]
    # the weights as recorded (both windows), and for Lorentz-to-Gauss the lineage attrs that call stamps (fid.py:190-196)
    extra = dict(_window=ap["_weight"])
    if lg:
        from ..config import ATTRS

        extra["_apodization_attrs"] = {ATTRS.apodization_lb: ap["lb"], ATTRS.apodization_gb: ap["gb"]}
    return spectral_pipeline(base, target_points=zf["target_points"] if zf is not None else n, lb=ap["lb"], dim=d0,
                             out_dim=dim, position=zf["position"] if zf is not None else "end", method=method,
                             peak_width=peak_width, target_coord=target_coord, p0_only=p0_only, _promote=True, **extra)


def _chain_metadata_untouched(src: LabeledArray, root: LabeledArray, steps) -> bool:
    """Replay the recorded steps' METADATA (host arithmetic only, nothing is computed on the device) from the root and
    compare coordinates, attrs and names with what the chain's arrays carry now."""
    from . import fid as _fid

    nodes = []
    node = src
    while node.is_deferred:
        nodes.append(node)
        node = node._lazy.parent
    if node is not root or len(nodes) != len(steps):
        return False
    replay = root
    for (name, kw), have in zip(reversed(steps), reversed(nodes)):
        if name == "zero_fill":
            replay = _fid.zero_fill(replay, dim=kw["dim"], target_points=kw["target_points"], position=kw["position"])
        elif name == "apodize_exp":
            replay = _fid.apodize_exp(replay, dim=kw["dim"], lb=kw["lb"])
        elif name == "apodize_lg":
            replay = _fid.apodize_lg(replay, dim=kw["dim"], lb=kw["lb"], gb=kw["gb"])
        elif name == "to_spectrum":
            replay = _fid.to_spectrum(replay, dim=kw["dim"], out_dim=kw["out_dim"])
        else:
            return False
        if have.dims != replay.dims or have.attrs != replay.attrs or have.name != replay.name:
            return False
        if set(have.coords) != set(replay.coords):
            return False
        for k, c in replay.coords.items():
            hc = have.coords[k]
            if hc.dim != c.dim or hc.attrs != c.attrs or not np.array_equal(hc.values, c.values, equal_nan=True):
                return False
    return True


def autophase(da, dim: str = DIMS.frequency, method: str = "acme", mode: str = "single",
              peak_width: float = 0.5, target_coord: float | None = None, p0_only: bool = False,
              lb: float = 0.0, temp_time_dim: str = DIMS.time, **kwargs):
    """Automatic phase correction (reference ``phasing.py:161-290``).  ``mode="all"`` raises as the reference's does;
    one phase pair per spectrum is `autophase_each`."""
    src = as_labeled(da)
    _check_dims(src, dim, "autophase")
    kwargs.setdefault("disp", False)
    if mode == "all":
        raise NotImplementedError(MSG_MODE_ALL)
    elif mode != "single":
        raise ValueError(MSG_MODE)
    if method not in aps.METHODS:
        raise ValueError(MSG_METHOD)
    fused = _fused_chain(src, dim, method, peak_width, target_coord, p0_only, lb)
    if fused is not None:
        return like_input(fused, da)

    coords = src.coords[dim].values
    x, _ = device_data(src)
    ax = src.get_axis_num(dim)
    _, idx = _global_argmax(src, x)  # device reduction, 16 bytes to the host
    if target_coord is not None:  # phasing.py:233-235
        target_idx = int(np.argmin(np.abs(coords - target_coord)))
        pivot = float(target_coord)
    else:  # phasing.py:237-238
        target_idx = int(idx[ax])
        pivot = float(coords[target_idx])

    # the ONE 1-D slice through the global maximum (phasing.py:241-242), upcast to complex128
    sel = tuple(slice(None) if i == ax else int(j) for i, j in enumerate(idx))
    sl = np.asarray(to_host(x[sel]), dtype=np.complex128)
    index_width = aps.index_width_of(coords, peak_width)  # phasing.py:245-247

    work, work_coords = sl, coords
    if lb > 0:  # phasing.py:250-253, on the 1-D slice only (three tiny launches)
        from .fid import apodize_exp, to_fid, to_spectrum

        one = LabeledArray(sl, (dim,), {dim: Coordinate(dim, coords)})
        tmp = to_spectrum(apodize_exp(to_fid(one, dim=dim, out_dim=temp_time_dim), dim=temp_time_dim, lb=lb),
                          dim=temp_time_dim, out_dim=dim)
        work, work_coords = tmp.values, tmp.coords[dim].values

    if method not in aps.METHODS:
        raise ValueError(MSG_METHOD)
    # the search's final polish follows the reference's route wherever it does anything (pipeline.run, polish="exact")
    p0_opt, p1_opt, _ = aps.solve(work, work_coords, pivot, target_idx, index_width, method=method,
                                  p0_only=p0_only, disp=kwargs.get("disp"), threads=aps.burst_threads(),
                                  polish=aps.default_polish())
    return like_input(_phase_labeled(src, x, dim, p0_opt, p1_opt, pivot), da)  # phasing.py:290


MSG_ENGINE = "engine must be 'auto', 'device' or 'host'"
MSG_ENGINE_DEVICE = ("engine='device' needs method='acme', lb == 0, a uniform coordinate axis and 2 <= n <= 16576 "
                     "points along the dimension")


def _solve_rows_host(rows, work, coords, work_coords, target_coord, index_width, method, p0_only, disp):
    """The host route of `autophase_each`: the native search (`aps.solve`) for every row of `rows` ([n_rows, n], host)
    on `work` (the same rows, or their line-broadened copies), as many at a time as the CPU budget has threads, one
    thread each.  Returns (p0, p1, pivot, skip)."""
    from concurrent.futures import ThreadPoolExecutor

    nb = rows.shape[0]
    p0, p1, pivot = (np.full(nb, np.nan) for _ in range(3))
    skip = np.zeros(nb, dtype=bool)

    def one(r):
        row = rows[r]
        if not np.all(np.isfinite(row)) or not np.any(row):  # the ACME score is 0/0: no search
            return r, None
        if target_coord is not None:  # phasing.py:233-235
            tidx, pv = int(np.argmin(np.abs(coords - target_coord))), float(target_coord)
        else:  # phasing.py:229, 237-238 on this row alone
            tidx = int(np.argmax(np.abs(row)))
            pv = float(coords[tidx])
        a, b, _ = aps.solve(np.asarray(work[r], dtype=np.complex128), work_coords, pv, tidx, index_width, method=method,
                            p0_only=p0_only, disp=disp, threads=1, polish=aps.default_polish())
        return r, (a, b, pv)

    workers = max(1, min(aps.burst_threads(), nb))
    with ThreadPoolExecutor(max_workers=workers) as pool:
        for r, res in pool.map(one, range(nb)):
            if res is None:
                skip[r] = True
            else:
                p0[r], p1[r], pivot[r] = res
    return p0, p1, pivot, skip


def _solve_rows_device(x2, coords, axis, target_coord, index_width, p0_only):
    """The device route: `xm_search_rows` on the rows where they are; the few rows whose best member does not pass
    scipy's projected-gradient test come to the host and are polished on the reference's route."""
    if target_coord is not None:
        recs = dev.search_rows(x2, axis, p0_only=p0_only, pivot=float(target_coord),
                               target_idx=int(np.argmin(np.abs(coords - target_coord))))
    else:
        recs = dev.search_rows(x2, axis, p0_only=p0_only)
    skip = recs["status"] >= dev.SEARCH_ALL_ZERO
    p0, p1 = recs["x"][:, 0].copy(), recs["x"][:, 1].copy()
    if target_coord is not None:
        pivot = np.where(skip, np.nan, float(target_coord))
    else:
        pivot = np.where(skip, np.nan, coords[np.clip(recs["target_idx"], 0, len(coords) - 1)])
    for r in np.nonzero(recs["needs_polish"] != 0)[0]:
        row = np.asarray(to_host(x2[int(r)]), dtype=np.complex128)
        xr, _, _, _ = aps.polish_reference(row, coords, float(pivot[r]), int(recs["target_idx"][r]), index_width, "acme",
                                           p0_only, recs["x"][r])
        p0[r] = xr[0]
        p1[r] = xr[1] if not p0_only else 0.0
    return p0, p1, pivot, skip


def autophase_each(da, dim: str = DIMS.frequency, method: str = "acme", peak_width: float = 0.5,
                   target_coord: float | None = None, p0_only: bool = False, lb: float = 0.0,
                   temp_time_dim: str = DIMS.time, engine: str = "auto", **kwargs):
    """One (p0, p1) per spectrum: every 1-D spectrum along `dim` is phased as the reference's
    ``autophase(spectrum, mode="single", ...)`` phases that spectrum alone (its own pivot -- the coordinate of its
    own |X| maximum, or `target_coord` --, the same bounds, seed, tolerance and polish).  What the reference names
    ``mode="all"`` and does not implement.

    engine="device": the searches run on the GPU, one workgroup per spectrum (ACME, ``lb == 0``, a uniform axis of at
    most 16576 points); engine="host": the native host search per spectrum on this process's CPUs (every method,
    any axis, ``lb > 0``); "auto" takes the device where it applies.  The phase is applied on the GPU either way.

    The result has the input's dims, coords and name like `phase`; attrs gain ``phase_p0`` / ``phase_p1`` /
    ``phase_pivot`` as float64 arrays shaped like the data without `dim` (0-d for a single spectrum) and
    ``phase_pivot_coord``.  A spectrum that is all zero or holds a value that is not finite has no search: it passes
    through unchanged with NaN in the three arrays."""
    src = as_labeled(da)
    _check_dims(src, dim, "autophase_each")
    kwargs.setdefault("disp", False)
    if method not in aps.METHODS:
        raise ValueError(MSG_METHOD)
    if engine not in ("auto", "device", "host"):
        raise ValueError(MSG_ENGINE)
    coords = np.asarray(src.coords[dim].values, dtype=np.float64)
    ax = src.get_axis_num(dim)
    n = src.shape[ax]
    lead = tuple(s_ for i, s_ in enumerate(src.shape) if i != ax)
    axis = dev.uniform_axis(coords)
    x, _ = device_data(src)
    on_device = (method == "acme" and not lb > 0 and axis is not None
                 and dev.search_rows_supported(n, method, axis[2], str(x.dtype).endswith("complex128")))
    if engine == "device" and not on_device:
        raise ValueError(MSG_ENGINE_DEVICE)
    index_width = aps.index_width_of(coords, peak_width)  # phasing.py:245-247

    if on_device and engine != "host":
        x2, _ = dev._rows(x, ax)
        p0, p1, pivot, skip = _solve_rows_device(x2, coords, axis, target_coord, index_width, p0_only)
    else:
        xm = x.movedim(ax, -1) if hasattr(x, "movedim") else np.moveaxis(x, ax, -1)
        x2 = xm.reshape(-1, n)
        rows = to_host(x2)
        work, work_coords = rows, coords
        if lb > 0:  # phasing.py:250-253 for every row at once: three launches over [n_rows, n]
            from .fid import apodize_exp, to_fid, to_spectrum

            each = LabeledArray(promote_for_float64_operand(x2), ("__spectrum__", dim), {dim: Coordinate(dim, coords)})
            tmp = to_spectrum(apodize_exp(to_fid(each, dim=dim, out_dim=temp_time_dim), dim=temp_time_dim, lb=lb),
                              dim=temp_time_dim, out_dim=dim)
            work, work_coords = tmp.values, tmp.coords[dim].values
        p0, p1, pivot, skip = _solve_rows_host(rows, work, coords, work_coords, target_coord, index_width, method,
                                               p0_only, kwargs.get("disp"))

    p0, p1, pivot, skip = (v.reshape(lead) for v in (p0, p1, pivot, skip))
    y = dev.phase_apply_rows(promote_for_float64_operand(x), ax, coords, np.where(skip, 0.0, p0), np.where(skip, 0.0, p1),
                             np.where(skip, 0.0, pivot), skip=skip)
    out = src.copy(data=y)
    out.name = binary_op_name(src, dim)
    out.attrs = _copy.copy(src.attrs)
    old = out.attrs.get(ATTRS.phase_pivot_coord)
    if old is not None and old != dim:  # phasing.py:79-88
        warnings.warn(msg_phase_units(dim, old, "one per spectrum" if target_coord is None else target_coord))
    out.attrs[ATTRS.phase_p0] = p0
    out.attrs[ATTRS.phase_p1] = p1
    out.attrs[ATTRS.phase_pivot] = pivot
    out.attrs[ATTRS.phase_pivot_coord] = dim
    return like_input(out, da)
