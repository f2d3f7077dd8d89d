"""Array-level fused hot path:  zero_fill -> apodize_exp -> to_spectrum -> autophase.

This is what the four chained accessor calls of the reference's quick start
(``README.md:66-73``) amount to on the data, done in two data-parallel launches instead of six
full-size numpy passes:

  pre-pass   read the FIDs, FFT in LDS, emit only (max |X|^2, arg-max) per spectrum
  exchange   device reduce -> 16 bytes to the host (over ranks: caller-provided gather)
  solve      the one arg-max spectrum (64 KiB D2H) -> differential evolution on the host
  main pass  read the FIDs again, FFT, multiply by e^{i phi}, write the phased spectra

All coordinate arithmetic stays on the host in fp64, restating ``processing/fid.py:254-263``
(zero-fill coords), ``:136`` (window), ``processing/fourier.py:95-98, 31`` (frequency coords,
roll) and ``processing/phasing.py:226-247, 56-73`` (selection, phase ramp).
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from . import autophase_solver as aps
from . import device as dev
from .cpu_budget import search_team as _search_team, search_workers as _search_workers  # noqa: F401 -- the policy's home
from .dims import MSG_POSITION


@dataclass
class PipelinePlan:
    """Host-side metadata of one pipeline configuration (depends on coords, not on the data)."""

    n_in: int
    n_out: int
    pad_left: int
    time: np.ndarray          # zero-fill-extrapolated time coordinate (fid.py:257-263)
    freq: np.ndarray          # fftshifted frequency coordinate (fourier.py:98, 31-32)
    window_host: np.ndarray   # exp(-pi*lb*t) in fp64 (fid.py:136) or ones
    window: object = None     # device tensor, storage precision
    window64: object = None   # device tensor, float64 (for the complex128 recomputation of the arg-max slice)
    extra: dict = field(default_factory=dict)


def zero_fill_coords(t: np.ndarray, target_points: int, pad_left: int) -> np.ndarray:
    """fid.py:257-263."""
    delta = t[1] - t[0]
    if pad_left == 0:
        return t[0] + np.arange(target_points) * delta
    return (t[0] - (pad_left * delta)) + np.arange(target_points) * delta


def make_plan(x2, t: np.ndarray, target_points: int, lb, position: str = "end", window_host=None) -> PipelinePlan:
    """`window_host`: the apodisation weights over the zero-filled axis when they are not exp(-pi lb t) (`apodize_lg`)."""
    import torch

    n_in = x2.shape[-1]
    t = np.asarray(t, dtype=np.float64)
    if target_points <= n_in:  # fid.py:235-236: no-op zero fill
        n_out, pad_left, tt = n_in, 0, t
    else:
        n_out = int(target_points)
        if position == "end":
            pad_left = 0
        elif position == "symmetric":
            pad_left = (n_out - n_in) // 2
        else:
            raise ValueError(MSG_POSITION)
        tt = zero_fill_coords(t, n_out, pad_left) if len(t) > 1 else t
    win = np.exp(-np.pi * lb * tt) if lb is not None else np.ones(n_out)
    if window_host is not None:
        win = np.asarray(window_host, dtype=np.float64)
        if win.shape != (n_out,):
            raise ValueError("window_host must cover the zero-filled axis")
    delta = (tt[1] - tt[0]) if len(tt) > 1 else 1.0
    freq = np.roll(np.fft.fftfreq(n_out, d=delta), n_out // 2)
    rd = torch.float32 if x2.dtype == torch.complex64 else torch.float64
    wdev = torch.from_numpy(np.ascontiguousarray(win)).to(device=x2.device, dtype=rd)
    return PipelinePlan(n_in, n_out, pad_left, tt, freq, win, wdev)


@dataclass
class AutophaseResult:
    p0: float
    p1: float
    pivot: float
    flat_index: int
    target_idx: int
    max_abs: float
    nfev: int = 0
    fun: float = float("nan")
    timing: dict = field(default_factory=dict)
    owner: int = 0      # rank that owns the winning spectrum (run_stream)
    mine: bool = True   # ... and whether that is this rank
    speculation: str = ""  # run_stream(speculate=True): "hit" or "repaired"
    hedged: bool = False   # run_stream(speculate=True): the search ran late and was started a second time (see there)


def slice_on_host() -> bool:
    """Where the winning row's spectrum -- the slice the (p0, p1) search runs on (phasing.py:241-247) -- is computed.
    On the HOST (default): the row comes back as complex128 (64 KiB) and `winner_spectrum` restates the reference's own
    numpy statements on it, so the search sees the reference's slice BIT FOR BIT (numpy's pocketfft transforms a row of
    a batch exactly as it transforms the row alone) and, with generations and polish that replicate scipy's, returns
    the reference's (p0, p1).  `XMRIS_AMD_SLICE=device` keeps rounds 1-3's fp64 kernel (one workgroup, 17 us of the
    step; its spectrum differs from pocketfft's in the last bit, which the flat landscape of a noise-only dataset
    amplified to 3e-6 of the spectrum's maximum, profiles/r03/c1_tolerance.txt)."""
    import os

    return os.environ.get("XMRIS_AMD_SLICE", "host") != "device"


def winner_spectrum(plan: "PipelinePlan", row) -> np.ndarray:
    """zero_fill -> apodize -> ortho FFT -> fftshift of ONE row in numpy, statement for statement what the reference does
    to every row (fid.py:251 `da.pad(..., constant_values=0)`, fid.py:136-139 `da * weight` with float64 weights --
    numpy promotes a complex64 FID to complex128 there --, fourier.py:153 `np.fft.fftn(..., norm="ortho")`,
    fourier.py:31-32 `roll(n // 2)`)."""
    n_out, n_in, pl = plan.n_out, plan.n_in, plan.pad_left
    row = np.asarray(row).reshape(-1)[:n_in]
    buf = np.zeros(n_out, dtype=np.complex128)
    buf[pl:pl + n_in] = row
    if plan.window_host is not None:
        buf = buf * np.asarray(plan.window_host, dtype=np.float64)
    return np.roll(np.fft.fft(buf, norm="ortho"), n_out // 2)


class Selection:
    """Device-side selection stage of autophase, queued without any host synchronisation right behind a
    pre-pass: global arg-max reduction -> gather of the winning FID (row index read from device memory)
    -> its spectrum recomputed in complex128, with (max, flat index, slice) written by the kernels straight
    into pinned host memory, closed by an event.  `wait()` blocks on that event only, so kernels queued
    later on the same stream (another dataset's main pass) do not delay the host solver."""

    @staticmethod
    def new_slot(x2, plan: "PipelinePlan", real_dtype):
        """Pinned host buffers (max, flat index, fp64 spectrum) + the device staging row of one selection in flight."""
        import torch

        return (torch.empty(1, dtype=real_dtype, pin_memory=True), torch.empty(1, dtype=torch.int64, pin_memory=True),
                torch.empty((1, plan.n_out), dtype=torch.complex128, pin_memory=True),
                torch.empty((1, x2.shape[1]), dtype=torch.complex128, device=x2.device),
                torch.empty((1, x2.shape[1]), dtype=torch.complex128, pin_memory=True))  # (the winning FID, host-slice mode)

    def __init__(self, x2, plan: "PipelinePlan", absmax2, argidx, index_from_slice: bool = False, key=None, slot=None,
                 refine=None, blocking=None):
        import torch

        n = plan.n_out
        self.index_from_slice = index_from_slice  # pre-pass ran with argmax_value_only: only the ROW is known
        if plan.window64 is None:
            plan.window64 = torch.from_numpy(np.ascontiguousarray(plan.window_host)).to(x2.device, torch.float64)
        self.n = n
        # Results go straight into pinned host memory (device-accessible at the same address on ROCm): the
        # reduction writes (max, flat index) there, the gather reads the index back from there, and the
        # complex128 spectrum kernel stores its 128 KiB row there -- no memcpy nodes on the stream.  The
        # buffers are reused across datasets (two sets: a streaming caller keeps at most two selections
        # in flight); allocating pinned memory per call costs more than the transfers.
        rdt = absmax2.dtype if (key is None and refine is None) else torch.float32
        if slot is None:
            pool = plan.extra.setdefault("pinned", [])
            turn = plan.extra["turn"] = (plan.extra.get("turn", -1) + 1) % 2
            if len(pool) <= turn:
                pool.append(Selection.new_slot(x2, plan, rdt))
            slot = pool[turn]
        self.h_max, self.h_flat, self.h_slice, x1 = slot[:4]
        self.plan = plan
        self.h_row = slot[4] if (len(slot) > 4 and slice_on_host()) else None
        if self.h_row is not None:
            x1 = self.h_row  # (the kernels below write the winning FID straight into pinned host memory)
        if refine is not None:  # coarse estimates -> exact check of the candidates -> winner decoded + gathered
            window32, est, gkey, wkey, band = refine
            dev.guess_refine(x2, n, window32, est, gkey, wkey, self.h_max, self.h_flat, x1, band=band)
        elif key is not None:  # the producer left the winner in a 64-bit key: decode + gather in one small launch
            dev.argmax_key_take(key, n, self.h_max, self.h_flat, x2, out_row=x1)
        else:
            dev.argmax_reduce_async(absmax2, argidx, n, gmax=self.h_max, gflat=self.h_flat)
            dev.gather_row_c128(x2, self.h_flat, n, out=x1)
        if self.h_row is None:
            dev.pipeline_fused(x1, n, plan.pad_left, window=plan.window64, out=self.h_slice)
        self.event = torch.cuda.Event(blocking=aps.scarce_cpus() if blocking is None else blocking)
        self.event.record()
        self._done = False

    def wait(self):
        self.event.synchronize()
        if self.h_row is not None and not self._done:
            # (into the pinned slice buffer: the search service, the device search and the polish read it from there)
            self.h_slice[0].numpy()[:] = winner_spectrum(self.plan, self.h_row[0].numpy())
            self._done = True
        sl = self.h_slice[0].numpy().copy()
        flat = int(self.h_flat.item())
        if self.index_from_slice:  # index along the axis = first arg-max of the (fp64) winning spectrum
            flat = (flat // self.n) * self.n + int(np.argmax(np.abs(sl)))
        return float(self.h_max.item()) ** 0.5, flat, sl


def select_and_solve(x2, plan: PipelinePlan, absmax2, argidx, method="acme", peak_width=100, target_coord=None,
                     p0_only=False, exchange=None, rank_offset_rows=0, disp=False, on_host_phase=None,
                     selection: "Selection | None" = None, threads=None, polish="exact"):
    """phasing.py:226-287 on the outputs of the pre-pass.  `exchange(max_abs, flat)` may merge the
    per-rank winners (returns (owner_is_me, global_flat)); default = single device.
    `on_host_phase()` is called once the device has nothing left to do for this dataset until the
    solver returns (a streaming caller queues the next dataset's pre-pass there)."""
    n = plan.n_out
    sl_ready = None
    if selection is not None:  # everything was queued behind the pre-pass already
        amax, flat, sl_ready = selection.wait()
    else:
        amax, flat = dev.argmax_reduce(absmax2, argidx, n)
    gflat = rank_offset_rows * n + flat
    mine = True
    if exchange is not None:
        mine, gflat = exchange(amax, gflat)
    k = gflat % n
    if target_coord is not None:  # phasing.py:233-235
        target_idx = int(np.argmin(np.abs(plan.freq - target_coord)))
        pivot = float(target_coord)
    else:  # phasing.py:237-238
        target_idx = int(k)
        pivot = float(plan.freq[k])
    res = AutophaseResult(0.0, 0.0, pivot, int(gflat), target_idx, amax)
    if mine:
        # The optimiser is chaotic in its input (a 1e-7 perturbation of the slice can steer the search
        # into another local minimum of the ACME landscape), so the ONE spectrum it works on is
        # recomputed in complex128 from the stored samples, as the reference's float64 path would.
        import torch

        if sl_ready is not None:
            sl = sl_ready
        else:
            row = gflat // n - rank_offset_rows
            x1 = x2[row:row + 1].to(torch.complex128)
            if plan.window64 is None:
                plan.window64 = torch.from_numpy(np.ascontiguousarray(plan.window_host)).to(x2.device, torch.float64)
            w64 = plan.window64
            sl = dev.pipeline_fused(x1, n, plan.pad_left, window=w64).out[0].cpu().numpy()
        if on_host_phase is not None:
            on_host_phase()
        iw = aps.index_width_of(plan.freq, peak_width)
        p0, p1, opt = aps.solve(sl, plan.freq, pivot, target_idx, iw, method=method, p0_only=p0_only, disp=disp,
                                threads=threads, polish=polish)
        res.p0, res.p1, res.nfev, res.fun = p0, p1, int(opt.nfev), float(opt.fun)
        res.timing = {"generations_ms": 1e3 * opt.get("t_generations", 0.0), "polish_ms": 1e3 * opt.get("t_polish", 0.0)}
    elif on_host_phase is not None:
        on_host_phase()
    return res, mine


def run(x2, t, target_points: int, lb: float, method: str = "acme", peak_width=100, target_coord=None,
        p0_only: bool = False, out=None, plan: PipelinePlan | None = None, params=None, polish: str | None = None):
    """Fused hot path on ``x2`` = [n_batch, n_time] complex rows resident in HBM.

    Returns (phased [n_batch, n_out] tensor, AutophaseResult, plan).  `params=(p0, p1)` skips the
    solver (used by parity tests that inject the oracle's parameters).  `polish` (`XMRIS_AMD_POLISH` overrides the
    default): "exact" -- the projected-gradient test that scipy's polish starts (and usually ends) with is made
    natively, a search that does not pass it is polished on the reference's own route, scipy's minimiser on the numpy
    objective: (p0, p1) equal the reference's to the last bit also on flat landscapes; "numpy" -- always that route
    (~5-10 ms); "native" -- scipy's L-BFGS-B core on the native objective (~0.1 ms; its end point differs from the
    reference's by ~1e-3 degrees when the polish iterates).  `run_stream` has the same default."""
    import os

    import torch

    if polish is None:
        polish = aps.default_polish()

    if plan is None:
        plan = make_plan(x2, t, target_points, lb)
    n = plan.n_out
    # One dataset, own solve: where the guess stage and the arg-max key apply, the speculative schedule replaces the
    # FFT pre-pass (0.89 ms on the roofline shape) by coarse spectra + an exact check of the candidates (0.14 ms); the
    # main pass verifies the guess and a wrong one is repaired -- same result as the classic order below
    # (XMRIS_AMD_RUN_CLASSIC=1 keeps that order).
    if (params is None and target_coord is None and os.environ.get("XMRIS_AMD_RUN_CLASSIC") is None
            and x2.dim() == 2 and x2.is_contiguous() and plan.window is not None
            and dev.guess_supported(x2, n, plan.pad_left) and dev.key_native(x2, n, plan.pad_left)):
        if out is None:
            out = torch.empty((x2.shape[0], n), dtype=x2.dtype, device=x2.device)
        res = run_stream([x2], [out], plan, method=method, peak_width=peak_width, p0_only=p0_only, speculate=True,
                         polish=polish)[0]
        return out, res, plan
    # with a solve, only the winning ROW is needed from the pre-pass (its index along the axis comes from
    # the winning spectrum itself, recomputed in fp64); injected parameters need the full arg-max
    pre = dev.pipeline_fused(x2, n, plan.pad_left, window=plan.window, want_out=False, want_argmax=True,
                             argmax_value_only=params is None)
    if params is None:  # arg-max reduction, row gather, fp64 slice and D2H all queued without host syncs
        sel = Selection(x2, plan, pre.absmax2, pre.argidx, index_from_slice=True)
        res, _ = select_and_solve(x2, plan, pre.absmax2, pre.argidx, method, peak_width, target_coord, p0_only,
                                  selection=sel, threads=aps.burst_threads(), polish=polish)  # one search, nothing beside it
    else:
        res = _selection_only(pre, plan, target_coord)
    if params is not None:
        res.p0, res.p1 = float(params[0]), float(params[1])
    main = main_pass(plan, x2, out, res.p0, res.p1, res.pivot)
    return main.out, res, plan


def run_stream(inputs, outputs, plan: PipelinePlan, *, exchange=None, broadcast=None, rank_offset_rows: int = 0,
               overlap: bool = True, method: str = "acme", peak_width=100, target_coord=None, p0_only: bool = False,
               trace: list | None = None, speculate: bool = False, polish: str | None = None):
    """The fused hot path over a SEQUENCE of independent datasets of one shape, software-pipelined.

    ``inputs[i]`` ([n_batch, n_in] complex rows in HBM) is transformed into ``outputs[i]`` ([n_batch, n_out]);
    the lists may repeat tensors.  Per dataset the device does a pre-pass (per-spectrum max |X|^2), the
    selection stage (`Selection`) and the main pass; the host does the O(1) exchange, the (p0, p1) search on
    the winning spectrum and the phase table.  With `overlap` the pre-pass + selection of dataset i+1 is queued
    before the host starts searching for dataset i, so the device works on dataset i+1 (and on the main pass
    of dataset i-1) while the host searches -- every dataset still gets all of its own work, nothing is
    reused across datasets.

    Multi-device: `exchange(max_abs, global_flat) -> (owner_rank_is_me, winning_global_flat, owner)` merges
    the per-rank winners and `broadcast(values, owner) -> values` hands the owner's (p0, p1) to every rank
    (`xmris_amd.sharding`); `rank_offset_rows` = first global row of this rank's shard.

    `speculate=True` replaces the arg-max pre-pass (an FFT of every row, instruction bound) by a GUESS of the
    winning row (`xmris_amd.stream`): coarse spectra of the first 512 windowed samples of every row (`xm_guess_rows`),
    then an exact transform of the candidate rows whose estimate lies within a band of the largest (`xm_guess_refine`);
    where that guess stage does not apply (`XM_GUESS_L1`, no window, an unsupported layout) the windowed L1 norm of the
    FIDs stands in (`xm_row_l1`: sum|z|/sqrt(N) bounds every |X[k]| of a row).  (p0, p1) is searched on the guessed
    row's spectrum, the main pass applies it AND returns the true global maximum, and the true arg-max row is compared
    with the guess before the dataset's output buffer is reused.  A wrong guess is repaired exactly: the true row's
    spectrum is fetched, (p0, p1) searched again and the dataset's main pass run again with them; the result equals
    the non-speculative schedule's.  How often the guess is right depends on the data; correctness never does.

    `trace`, if given, receives one dict per dataset: host timestamps (`t_start`, `t_exchanged`, `t_solved`,
    `t_table`; speculative schedule: also `t_search_begin`, `t_search_end` on the search's thread and `t_collect`) and torch events around the two kernels (`pre0`, `pre1`, `main0`, `main1`).
    Returns the list of AutophaseResult (p0, p1 filled on every rank; `.speculation` = "hit" / "repaired" with
    `speculate`)."""
    import time

    import torch

    n_sets = len(inputs)
    if polish is None:
        polish = aps.default_polish()
    if n_sets != len(outputs):
        raise ValueError("inputs and outputs must have the same length")
    if n_sets == 0:
        return []
    # The loop is latency sensitive (one dataset every ~2 ms) and creates a little cyclic garbage per dataset; a
    # generation-2 collection over an interpreter that has torch and numpy loaded costs 10+ ms.  The cyclic
    # collector is paused for the duration of the call (reference counting still frees almost everything).
    import gc

    gc_was_enabled = gc.isenabled()
    gc.disable()
    try:
        return _run_stream(inputs, outputs, plan, exchange, broadcast, rank_offset_rows, overlap, method, peak_width,
                           target_coord, p0_only, trace, speculate, polish)
    finally:
        if gc_was_enabled:
            gc.enable()


def _run_stream(inputs, outputs, plan, exchange, broadcast, rank_offset_rows, overlap, method, peak_width,
                target_coord, p0_only, trace, speculate, polish="exact"):
    import time

    import torch

    n_sets = len(inputs)
    if speculate:
        if target_coord is not None:
            raise ValueError("speculate=True needs the arg-max pivot (target_coord=None)")
        from . import stream

        return stream.run_speculative(inputs, outputs, plan, exchange, broadcast, rank_offset_rows, overlap, method,
                                      peak_width, p0_only, trace, polish)
    n = plan.n_out
    x0 = inputs[0]
    rd = torch.float32 if x0.dtype == torch.complex64 else torch.float64
    bufs = plan.extra.get(("stream_bufs", x0.shape[0], str(rd)))
    if bufs is None:  # two sets of pre-pass outputs: dataset i+1's pre-pass runs while dataset i is being solved
        bufs = plan.extra[("stream_bufs", x0.shape[0], str(rd))] = (
            [torch.empty(x0.shape[0], dtype=rd, device=x0.device) for _ in range(2)],
            [torch.empty(x0.shape[0], dtype=torch.int32, device=x0.device) for _ in range(2)])
    absmax2, argidx = bufs
    sel = [None, None]
    events = [dict() for _ in range(n_sets)]

    def prepass(i):
        b = i & 1
        ev = events[i]
        if trace is not None:
            ev["pre0"], ev["pre1"] = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev["pre0"].record()
        dev.pipeline_fused(inputs[i], n, plan.pad_left, window=plan.window, want_out=False, want_argmax=True,
                           absmax2=absmax2[b], argidx=argidx[b], argmax_value_only=True)
        if trace is not None:
            ev["pre1"].record()
        # selection stage queued right behind it (device-side arg-max -> fp64 slice -> pinned host memory)
        sel[b] = Selection(inputs[i], plan, absmax2[b], argidx[b], index_from_slice=True)

    results = []
    prepass(0)
    for i in range(n_sets):
        b = i & 1
        ev = events[i]
        ev["t_start"] = time.perf_counter()
        owner_box = [0]

        def merged(amax, gflat):
            if exchange is None:
                ev["t_exchanged"] = time.perf_counter()
                return True, gflat
            mine, gwin, owner = exchange(amax, gflat)
            owner_box[0] = owner
            ev["t_exchanged"] = time.perf_counter()
            return mine, gwin

        def queue_next():
            if overlap and i + 1 < n_sets:
                prepass(i + 1)

        res, mine = select_and_solve(inputs[i], plan, absmax2[b], argidx[b], method, peak_width, target_coord,
                                     p0_only, exchange=merged, rank_offset_rows=rank_offset_rows,
                                     on_host_phase=queue_next, selection=sel[b], polish=polish)
        if broadcast is not None:
            res.p0, res.p1 = broadcast([res.p0, res.p1], owner_box[0])
        res.owner, res.mine = owner_box[0], mine
        ev["t_solved"] = ev["t_table"] = time.perf_counter()
        if trace is not None:
            ev["main0"], ev["main1"] = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev["main0"].record()
        main_pass(plan, inputs[i], outputs[i], res.p0, res.p1, res.pivot)
        if trace is not None:
            ev["main1"].record()
        if not overlap and i + 1 < n_sets:
            prepass(i + 1)
        results.append(res)
        if trace is not None:
            trace.append(ev)
    return results


def phase_ramp_of(plan: PipelinePlan, p0: float, p1: float, pivot: float):
    """phasing.py:56-69 on the plan's (uniform) frequency axis in closed form: phi[k] = phase0 + dphase * k.
    Returns (phase0, dphase) in radians, or None when the axis is not uniform (a table is needed then)."""
    lin = plan.extra.get("freq_linear")
    if lin is None:
        f = np.asarray(plan.freq, dtype=np.float64)
        ok = f.size >= 2
        if ok:
            step = (f[-1] - f[0]) / (f.size - 1)
            ok = step != 0 and bool(np.all(np.abs(f - (f[0] + step * np.arange(f.size))) <= 1e-12 * np.abs(f).max()))
        lin = plan.extra["freq_linear"] = (float(f[0]), float(step), float(f.max() - f.min())) if ok else False
    if lin is False:
        return None
    c0, step, rng = lin
    if rng == 0:
        return float(np.deg2rad(p0)), 0.0
    return (float(np.deg2rad(p0) + np.deg2rad(p1) * (c0 - pivot) / rng), float(np.deg2rad(p1) * step / rng))


def main_pass(plan: PipelinePlan, x2, out, p0: float, p1: float, pivot: float, **kw):
    """The fused main pass with the autophase ramp: in closed form where the kernel applies it natively (no table
    is built, nothing is uploaded), through a phase table otherwise."""
    native = plan.extra.get(("ramp_native", x2.data_ptr() & 15, x2.shape[1], str(x2.dtype)))
    if native is None:
        native = plan.extra[("ramp_native", x2.data_ptr() & 15, x2.shape[1], str(x2.dtype))] = dev.ramp_native(
            x2, plan.n_out, plan.pad_left)
    ramp = phase_ramp_of(plan, p0, p1, pivot) if native else None
    if ramp is not None:
        return dev.pipeline_fused(x2, plan.n_out, plan.pad_left, window=plan.window, phase_ramp=ramp, out=out, **kw)
    ph = upload_phase_table(plan, x2, p0, p1, pivot)
    return dev.pipeline_fused(x2, plan.n_out, plan.pad_left, window=plan.window, phase_table=ph, out=out, **kw)


def upload_phase_table(plan: PipelinePlan, like, p0: float, p1: float, pivot: float):
    """e^{i phi} over the frequency axis (fp64 on the host, phasing.py:56-73), rounded once to the storage
    precision into a reused pinned staging buffer and copied to the device asynchronously."""
    import torch

    n = plan.n_out
    key = ("phase_stage", str(like.dtype))
    stage = plan.extra.get(key)
    if stage is None:
        stage = plan.extra[key] = [torch.empty(n, dtype=like.dtype, pin_memory=True) for _ in range(2)] + [0]
    stage[2] ^= 1
    host = stage[stage[2]]
    # fp64 cos / sin of the ramp, rounded once, written straight into the pinned staging buffer by the host library
    from . import _lib

    freq = plan.extra.get("freq_c")
    if freq is None:
        freq = plan.extra["freq_c"] = np.ascontiguousarray(plan.freq, dtype=np.float64)
    rc = _lib.load().xm_phase_table(freq.ctypes.data, n, float(p0), float(p1), float(pivot), host.data_ptr(),
                                    1 if like.dtype == torch.complex64 else 0)
    if rc:
        raise ValueError("xm_phase_table rejected its arguments")
    dev_t = plan.extra.setdefault(("phase_dev", str(like.dtype)),
                                  [torch.empty(n, dtype=like.dtype, device=like.device) for _ in range(2)])
    out = dev_t[stage[2]]
    out.copy_(host, non_blocking=True)
    return out


def _selection_only(pre, plan, target_coord):
    amax, flat = dev.argmax_reduce(pre.absmax2, pre.argidx, plan.n_out)
    k = flat % plan.n_out
    if target_coord is not None:
        return AutophaseResult(0.0, 0.0, float(target_coord), flat,
                               int(np.argmin(np.abs(plan.freq - target_coord))), amax)
    return AutophaseResult(0.0, 0.0, float(plan.freq[k]), flat, int(k), amax)
