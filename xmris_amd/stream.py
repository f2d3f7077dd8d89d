"""The speculative stream executor: `pipeline.run_stream(speculate=True)`.

Guess pass -> search -> main pass with true maxima -> verify (-> repair), software-pipelined over the datasets (with
`overlap`): while the main pass of dataset i is queued, the guess kernels + selection stages of the next datasets are
already on the stream and the (p0, p1) searches of datasets i+1 ... run on a search engine, so a search has several
device periods to finish instead of racing one.  Every dataset still gets all of its own work; the collective-like
calls (`exchange`, `broadcast`) are made by the launch thread in dataset order, identically on every rank.

The parts: `Schedule` (every quantity that fixes the order of launches and collective calls, fixed once per call),
`Ring` (the buffers of the datasets in flight), three search engines with one interface (`ServiceEngine`,
`ThreadEngine`, `DeviceEngine`), the `Hedger` and the `PolishHandoff` they share, and the `Executor` that runs the
pipeline.  Device entry points are looked up through `device` at call time (tests replace them)."""
from __future__ import annotations

import os
import threading
import time
from concurrent.futures import FIRST_COMPLETED, ThreadPoolExecutor
from concurrent.futures import TimeoutError as FutureTimeout
from concurrent.futures import wait as wait_first
from dataclasses import dataclass
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from . import autophase_solver as aps
from . import cpu_budget
from . import device as dev
from .pipeline import AutophaseResult, Selection, main_pass, slice_on_host, winner_spectrum

_SUB_STEP = 8  # the L1 guess reads every 8th 1-KiB block of the samples it uses (see `Schedule`)


def _look_ahead(workers: int, n_sets: int, overlap: bool, polish: str) -> int:
    """Datasets whose searches are SUBMITTED ahead of the main pass being queued.  `workers` of them run side by side;
    with the native search service (polish="exact") three more wait in its queue: a search then ends five or six device
    periods before its result is needed instead of two, which is what hides the rare search whose polish has to run on
    the reference's route (scipy's minimiser on the numpy objective: 3-8 ms) -- on the heterogeneous dataset family
    one search in seven needs it, and with the polish done by the launch thread when the result was collected the rate
    fell from 46 to 33 M spectra/s (profiles/r04/hetero_steps.txt)."""
    if not overlap:
        return 0
    if n_sets <= 2:
        return 1
    extra = 3 if polish == "exact" else 0
    return min(workers + extra, n_sets - 1)


_ABANDONED_RECORDS = []  # result records of searches nobody waits for any more (a hedged search's loser, a test hook's
                          # late submission): their searches still write them when they end, so they must not be freed


def _abandon(rec):
    _ABANDONED_RECORDS.append(rec)
    del _ABANDONED_RECORDS[:-256]


# ---- schedule ----------------------------------------------------------------------------------------------------

@dataclass(frozen=True)
class Schedule:
    """Everything that fixes the order of the kernel launches and of the exchange / broadcast calls of one call.  With
    several ranks the order of the exchange calls must be the same on every rank: the order-fixing fields are then
    derived from rank 0's broadcast values and from nothing a rank measures or owns."""

    workers: int      # searches in flight (`cpu_budget.search_workers`)
    team: int         # threads per search in flight
    fill_team: int    # threads of the pipeline-filling search
    n_workers: int    # searches RUNNING side by side (more may be queued)
    s_ahead: int      # searches submitted ahead of the main pass being queued
    s_look: int       # ... counting the device engine's
    g_ahead: int      # guess kernels queued ahead of it
    ring: int         # slots of the buffers in flight
    cpu_fill: int     # device engine: the first datasets, searched by the host engine
    use_dev: bool     # device engine behind the fill
    dev_ahead: int    # device engine: datasets its search starts ahead of the main pass
    est_ms: float     # device engine: a search's expected time
    fast_fill: bool   # one rank: event-driven pipeline fill
    ramped: bool      # look-ahead built up over the first datasets (2 + 3 i searches)
    use_service: bool  # host searches on the library's native service (else Python threads)
    use_keys: bool    # the main pass leaves its global arg-max in a key
    use_guess: bool   # guess stage = coarse spectra + exact check of the candidates (else the L1 norm)
    l1_keys: bool     # the L1 guess leaves its winner in a key
    band: float       # candidate band of the guess stage
    n_used: int       # leading samples the L1 guess reads
    sub_step: int     # ... every `sub_step`-th 1-KiB block of them
    blocking: bool    # few cores per rank: waits sleep instead of spinning


def _uniform_axis(plan):
    axis = plan.extra.get("uniform_axis")
    if axis is None:
        axis = plan.extra["uniform_axis"] = dev.uniform_axis(plan.freq) or False
    return axis


def _device_engine_wanted(plan, method, polish, overlap) -> bool:
    """`XMRIS_AMD_SEARCH`.  The device engine (a search is ONE workgroup of `xm_search_launch` on a reserved CU, scipy's
    generations bit for bit, then the projected-gradient test scipy's polish starts with): no host core computes
    anything, and what a shared host does to its threads no longer reaches the device's schedule.  Measured on one
    rank with 16 CPUs (profiles/r04/search_engines.txt): the host engine is FASTER -- a search kernel needs a whole
    CU's registers for 2.5-4 ms, so the chip is split (`xm_stream_create`), and the streaming kernels lose more than
    the CUs' share (65,536 x 4096 -> 8192: 52.3 vs 48.0 M spectra/s; 16,384 x 2048 -> 4096: 0.35 vs 0.49 ms per
    dataset).  "auto" therefore takes it only where the host cannot carry the searches: fewer than TWO CPUs per rank
    of this node (searches are per dataset, not per rank: eight ranks on 16 CPUs still carry them,
    profiles/r03/rehearsal_6ranks.txt), and only where every rank has a GPU of its own (see below)."""
    want = os.environ.get("XMRIS_AMD_SEARCH", "auto")
    if want == "auto":
        local_world = cpu_budget.local_world()
        # (a GPU of its own: the partition is made of CU-masked queues, and those of several processes on ONE card
        # reserve the same CUs and oversubscribe its hardware queues -- six ranks sharing a GPU fell into the
        # scheduler's 10.7 ms process time slices, 124 instead of 1.4 ms per step, profiles/r04/rehearsal_6ranks.txt;
        # four ranks still ran at full speed)
        own_gpu = torch.cuda.device_count() >= local_world
        want = "device" if (cpu_budget.cpu_share() < 2 * local_world and own_gpu) else "host"
    axis = _uniform_axis(plan)
    return (want == "device" and polish == "exact" and method == "acme" and overlap and axis is not False
            and dev.search_supported(plan.n_out, method, axis[2]))


def _geometry(plan, x):
    """(key_native, guess_supported) of a dataset: they depend on its alignment, shape and dtype only."""
    k = ("geometry", x.data_ptr() & 15, tuple(x.shape), str(x.dtype), x.is_contiguous())
    g = plan.extra.get(k)
    if g is None:
        g = plan.extra[k] = (dev.key_native(x, plan.n_out, plan.pad_left), dev.guess_supported(x, plan.n_out, plan.pad_left))
    return g


def _window_weights(plan):
    return np.abs(np.asarray(plan.window_host, dtype=np.float64)[plan.pad_left:plan.pad_left + plan.n_in])


def _guess_band(plan) -> float:
    """Candidate band of the guess stage.  A coarse spectrum (first 512 samples, 1024 bins) underestimates a line's
    height by the part of its windowed FID beyond sample 512 -- at most the window's own weight out there, for a line
    that does not decay by itself -- and by the grid's scalloping (>= 0.9 for a 2x zero-filled truncated line): rows
    whose estimate reaches 0.9 x (window weight inside the first 512 samples) of the largest estimate are checked
    exactly (lb = 5 Hz at 5 kHz: 0.72; measured on the heterogeneous family: estimates within [0.83, 0.97] of the true
    peaks, scripts/study_guess_statistics.py).  A wider band only costs exact transforms (<= 16 per workgroup)."""
    band = plan.extra.get("guess_band")
    if band is None:
        wabs = _window_weights(plan)
        inside = float(wabs[:512].sum()) / max(float(wabs.sum()), 1e-300)
        # ... floored at 0.4: the window bound assumes a line that does not decay by itself; measured on the
        # heterogeneous family WITHOUT apodisation (lb = 0, inside = 0.125): 12/12 hits with 0.25 and with 0.4 (device
        # period 1.43 / 1.31 ms: a wide band costs exact transforms), 11/12 with 0.5 (scripts/time_hetero_lb.py)
        band = plan.extra["guess_band"] = float(min(0.95, max(0.4, 0.9 * inside)))
    return band


def _guess_n_used(plan) -> int:
    """The L1 guess needs a ranking, not the norm itself: samples whose window weight is negligible are not read --
    the leading samples that carry all but 1e-3 of the window's total weight (rounded up to 256).  Of those, every
    `_SUB_STEP`-th 1-KiB block is read (whole cache lines at the start, middle and end of the window's support): the
    guess is verified by the main pass anyway, and a regular subset ranks rows like the full sum does."""
    n_used = plan.extra.get("guess_n_used")
    if n_used is None:
        wabs = _window_weights(plan)
        total = float(wabs.sum())
        n_used = plan.n_in
        if total > 0:
            n_used = int(np.searchsorted(np.cumsum(wabs), (1.0 - 1e-3) * total)) + 1
            n_used = min(plan.n_in, max(256, -(-n_used // 256) * 256))
        plan.extra["guess_n_used"] = n_used
    return n_used


def make_schedule(inputs, plan, exchange, broadcast, overlap, method, polish) -> Schedule:
    n_sets, n, x0 = len(inputs), plan.n_out, inputs[0]
    workers, _ = cpu_budget.search_workers(plan, x0.shape[0], x0.element_size())
    use_dev = _device_engine_wanted(plan, method, polish, overlap)
    # ~600 objective evaluations; measured per evaluation: 2.3 us + 0.4 us per 1000 bins (profiles/r04/device_search.txt)
    est_ms = 600 * (2.3 + 0.4 * n / 1000.0) * 1e-3
    dev_ahead = 0
    if use_dev:  # a search takes milliseconds on its one CU: it starts `dev_ahead` datasets in front of its main pass
        device_ms = x0.shape[0] * (plan.n_in + plan.n_out) * x0.element_size() / 5.5e9 + 0.12
        dev_ahead = int(min(24, max(3, -(-est_ms // device_ms) + 2)))
    if exchange is not None:
        # several ranks: the look-ahead fixes the ORDER of the exchange calls, which every rank must make alike -- it
        # may not depend on anything a rank measures or owns (its shard size, its share of the host's cores, its
        # environment).  Rank 0's choice goes to everyone (one more broadcast at the start of the call); without a
        # broadcast callable: two searches in flight on the host engine.
        if broadcast is not None:
            got = broadcast([float(workers), float(dev_ahead)], 0)
            workers, dev_ahead = int(round(got[0])), int(round(got[1]))
        else:
            workers, dev_ahead = 2, 0
        use_dev = dev_ahead > 0
    s_ahead = _look_ahead(workers, n_sets, overlap, polish)
    # device engine: the first `cpu_fill` datasets of the call (the pipeline is still filling: nothing hides a search
    # there) are searched by the host engine, s_ahead at a time
    cpu_fill = min(n_sets, min(workers, s_ahead) + 1) if use_dev else n_sets
    use_dev = use_dev and cpu_fill < n_sets
    # (the selection stage of dataset j on a stream of its own beside the coarse spectra of dataset j + 1, gated so that
    # it never shares the chip with a main pass, hides nothing -- the coarse-spectra kernel fills the chip, 1.20 vs
    # 1.20 ms per step; let loose beside the main kernel it costs 6 %.  Everything stays on one stream.)
    g_ahead = s_ahead + 1 if overlap else 0
    if use_dev:
        g_ahead = max(g_ahead, min(dev_ahead, n_sets - 1))
    # (device engine: a search is started as soon as its selection stage is queued -- one rank -- or has ended --
    # several ranks, whose exchange needs the stage's result: one dataset behind the newest guess)
    s_look = s_ahead if not use_dev else (g_ahead if exchange is None else max(s_ahead, g_ahead - 1))
    n_workers = min(workers, s_ahead) if s_ahead >= 2 else 0
    fast_fill = exchange is None and not use_dev and overlap and n_sets > 2 and s_ahead >= 2
    c128 = x0.dtype == torch.complex128
    distinct = list({id(x): x for x in inputs}.values())
    # the main pass leaves its true global arg-max in a key (no per-row arrays): every dataset must take that kernel
    use_keys = all(_geometry(plan, x)[0] for x in distinct)
    # guess stage: coarse spectra + exact check of the candidates (both precisions); else the windowed L1 norm's winner
    use_guess = (os.environ.get("XM_GUESS_L1") is None and plan.window is not None
                 and all(_geometry(plan, x)[1] for x in distinct))
    return Schedule(
        workers=workers, team=cpu_budget.search_team(n_workers) if n_workers else cpu_budget.stream_threads(),
        # the pipeline-filling search (the first main pass waits for it) takes the whole CPU share for its
        # millisecond: four A/B pairs at the driver's K = 20: 53.1 -> 53.8 M spectra/s
        fill_team=cpu_budget.burst_threads(), n_workers=n_workers, s_ahead=s_ahead, s_look=s_look, g_ahead=g_ahead,
        ring=g_ahead + 2, cpu_fill=cpu_fill, use_dev=use_dev, dev_ahead=dev_ahead, est_ms=est_ms, fast_fill=fast_fill,
        # (the ramp, measured through the multi-rank code path on a GPU of its own, profiles/r04/fill.txt: 1.302 ->
        # 1.244 ms per step against the whole look-ahead in front of the first main pass)
        ramped=overlap and not use_dev and not fast_fill,
        use_service=polish == "exact", use_keys=use_keys, use_guess=use_guess,
        l1_keys=use_keys and not c128 and not use_guess,  # the L1 guess stage leaves its winner in a key (complex64)
        band=_guess_band(plan), n_used=_guess_n_used(plan), sub_step=_SUB_STEP, blocking=cpu_budget.scarce_cpus())


# ---- buffers -----------------------------------------------------------------------------------------------------

@dataclass
class Ring:
    """Device and pinned buffers of the `ring` datasets in flight (slot = dataset % ring), cached with the plan.
    complex64: the guess kernel and the main kernel leave their winners in arg-max key buffers (no per-row arrays, no
    separate reductions); every key is cleared by the launch that decodes it."""

    norm: list
    est: list
    wkey: object
    zero_idx: object
    tmax: list
    tidx: list
    vmax: list
    vflat: list
    gkey: list
    vkey: list
    vres: list
    sel_slots: list

    @staticmethod
    def of(plan, x0, s: Schedule) -> "Ring":
        rd = torch.float32 if x0.dtype == torch.complex64 else torch.float64
        nb, d = x0.shape[0], x0.device
        # (use_keys / l1_keys depend on the alignment of every input: buffers cached for one combination hold None
        # where another needs arrays)
        key = ("spec_bufs", nb, str(rd), s.ring, s.use_guess, s.use_keys, s.l1_keys)
        ring = plan.extra.get(key)
        if ring is None:
            slots = range(s.ring)
            sel_rd = torch.float32 if s.use_guess else rd
            ring = plan.extra[key] = Ring(
                norm=[None if (s.l1_keys or s.use_guess) else torch.empty(nb, dtype=rd, device=d) for _ in slots],
                est=[torch.empty(nb, dtype=torch.float32, device=d) if s.use_guess else None for _ in slots],
                wkey=dev.new_argmax_key(d) if s.use_guess else None,
                zero_idx=torch.zeros(nb, dtype=torch.int32, device=d),
                tmax=[None if s.use_keys else torch.empty(nb, dtype=rd, device=d) for _ in slots],
                tidx=[None if s.use_keys else torch.empty(nb, dtype=torch.int32, device=d) for _ in slots],
                vmax=[torch.empty(1, dtype=rd, pin_memory=True) for _ in slots],
                vflat=[torch.empty(1, dtype=torch.int64, pin_memory=True) for _ in slots],
                gkey=[dev.new_argmax_key(d) if (s.use_keys or s.use_guess) else None for _ in slots],
                vkey=[dev.new_argmax_key(d) if s.use_keys else None for _ in slots],
                vres=[dev.new_key_result() if s.use_keys else None for _ in slots],
                sel_slots=[Selection.new_slot(x0, plan, sel_rd) for _ in slots])
        return ring


class Records:
    """Result records of the searches in flight (slot = dataset % ring), cached with the plan, and the sequence number
    of the latest submission: a record is complete when its word 7 carries its submission's number."""

    def __init__(self, recs):
        self.recs, self.seq = recs, 0

    @staticmethod
    def of(plan, name, ring, new):
        r = plan.extra.get((name, ring))
        if r is None:
            r = plan.extra[(name, ring)] = Records([new() for _ in range(ring)])
        return r

    def next_seq(self) -> int:
        self.seq += 1
        return self.seq


# ---- searches ----------------------------------------------------------------------------------------------------

@dataclass
class SearchOutcome:
    p0: float
    p1: float
    nfev: int
    fun: float
    timing: dict
    hedged: bool
    k: int


class Ticket(NamedTuple):
    """A submitted search: `handle` (record sequence number, future, or an inline search's result) + its arguments."""

    handle: object
    sl: object
    k: int
    pivot: float


class Pending(NamedTuple):
    """A dataset whose search is under way: its partial result (None: one rank, device engine -- the search record is
    the first the host hears of the winner), the engine (None: another rank owns the search) and the ticket."""

    res: AutophaseResult | None
    engine: object
    ticket: Ticket | None


class Hedger:
    """Hedged host searches.  A search is O(1) work on ONE thread plus its team; when that thread loses its CPU (or is
    dispatched late) on a contended host the search ends milliseconds late and the device waits (seen: 3-10 ms searches
    with next to no team shares taken over, `profiles/r03/box_spread.txt`).  The result is a pure function of the
    slice, so when the launch thread needs a result that is later than twice the typical run time it has the SAME
    search started again with the whole team and takes whichever of the two ends first.  At most one dataset in
    `XM_HEDGE_SPACING` (default 8: a uniformly slow host gains nothing from doing everything twice)."""

    def __init__(self, plan, s: Schedule):
        self.enabled = os.environ.get("XMRIS_AMD_HEDGE", "1") != "0"
        self.gap = max(1, int(os.environ.get("XM_HEDGE_SPACING", "8")))  # (test switch: datasets between two hedges)
        # typical run times, kept with the plan from call to call: the pipeline-filling search of a call (whole team,
        # the device idle behind it) has a history of its own
        self.run_hist = plan.extra.setdefault("search_run_hist", [])
        self.fill_hist = plan.extra.setdefault("fill_run_hist", [])
        self.last = -100
        self.n_out, self.team, self.fill_team = plan.n_out, s.team, s.fill_team

    def allowed(self, i: int) -> bool:
        return self.enabled and i - self.last >= self.gap

    def deadline(self, i: int, t_exchanged: float, scale: float, offset: float = 0.0) -> float:
        """When dataset i's search counts as late.  Without a history of three searches -- with several ranks a rank
        only searches the datasets it owns, so it may never have one (found by the eight-rank executor test) -- the
        cost model stands in, generously: `scale` x `cpu_budget.search_ms` + `offset` (seconds)."""
        recent = (self.fill_hist if i == 0 else self.run_hist)[-9:]
        if len(recent) < 3:
            recent = [scale * cpu_budget.search_ms(self.n_out, self.fill_team if i == 0 else self.team) + offset]
        typical = sorted(recent)[len(recent) // 2]
        return t_exchanged + 2.0 * typical + 0.5e-3

    def record(self, i: int, seconds: float):
        hist = self.fill_hist if i == 0 else self.run_hist
        hist.append(seconds)
        del hist[:-16]


class PolishHandoff:
    """Searches that do not pass scipy's projected-gradient test are polished on the reference's route (numpy
    objective, milliseconds of interpreter): a helper starts on that as soon as the search's record says so -- the
    launch thread looks at the records of the searches in flight once per dataset -- instead of the launch thread
    doing it when it needs the result.  The helper is a worker PROCESS (`polish_workers.PolishWorkers`): a polish is
    milliseconds of small numpy operations, and on helper THREADS they were taken out of this thread's share of the
    interpreter lock -- on the heterogeneous family, where 13 searches of 16 need the polish, the launch thread fell
    from 1.4 to 2.3 ms per dataset (profiles/r04/hetero_polish.txt).  XM_POLISH_THREADS=n keeps them on threads."""

    def __init__(self, x: "Executor"):
        self.x, self.futs = x, {}
        pool = x.plan.extra.get("polish_pool")
        if pool is None:
            if os.environ.get("XM_POLISH_THREADS"):
                pool = ThreadPoolExecutor(max_workers=max(1, int(os.environ["XM_POLISH_THREADS"])),
                                          thread_name_prefix="xm-polish")
            elif x.n_sets > 4:  # (a stream: the workers start now, in the background -- a process start + scipy's import is ~1 s)
                pool = aps.polish_workers()
            if pool is not None:
                x.plan.extra["polish_pool"] = pool
        self.pool = pool

    def _args(self, j, k, x0):
        x = self.x
        sl = x.sel[j % x.s.ring].h_slice[0].numpy().copy()
        return (sl, x.plan.freq, float(x.plan.freq[k]), k, x.iw, x.method, x.p0_only, x0)

    def advance(self, pending):
        """Start the polish of every finished search in flight that needs one."""
        for j, p in pending.items():
            if j in self.futs or p.engine is None:
                continue
            rec = p.engine.record(j)
            if rec is None or not dev.search_done(rec, p.ticket.handle):
                continue
            r = dev.read_search_record(rec)
            if not r["needs_polish"] or self.pool is None:  # (a short call: the launch thread polishes when it collects)
                self.futs[j] = None
                continue
            args = self._args(j, r["target_idx"], r["x"])
            self.futs[j] = (self.pool.submit(aps.polish_reference, *args) if isinstance(self.pool, ThreadPoolExecutor)
                            else self.pool.submit(*args))

    def settle(self, i, r, k, out: SearchOutcome) -> SearchOutcome:
        """`out` of dataset i's finished search record `r`, polished where the record says so."""
        if r["needs_polish"]:
            t0 = time.perf_counter()
            fut = self.futs.pop(i, None)
            x, fun, nfev_p, _ = fut.result() if fut is not None else aps.polish_reference(*self._args(i, k, r["x"]))
            out.p0, out.p1, out.fun, out.nfev = float(x[0]), (float(x[1]) if not self.x.p0_only else 0.0), fun, r["nfev"] + nfev_p
            out.timing["polish_ms"] = 1e3 * (time.perf_counter() - t0)  # (what the launch thread still waited for)
            out.timing["polish_route"] = "numpy"
        else:
            self.futs.pop(i, None)
        if self.x.p0_only:
            out.p1 = 0.0
        return out


def _record_outcome(r, p0_only, k, timing) -> SearchOutcome:
    """A finished search record (+ the gradient test's evaluations in nfev, like scipy's count)."""
    p0, p1 = r["x"]
    return SearchOutcome(p0, p1, r["nfev"] + (1 if p0_only else 2) + 1, r["fun"], timing, False, k)


def _opt_outcome(p0, p1, opt, hedged, k) -> SearchOutcome:
    timing = {"generations_ms": 1e3 * opt.get("t_generations", 0.0), "polish_ms": 1e3 * opt.get("t_polish", 0.0)}
    return SearchOutcome(p0, p1, int(opt.nfev), float(opt.fun), timing, hedged, k)


class ServiceEngine:
    """Host searches on NATIVE threads of the library (`xm_hostsearch_submit`: generations + the projected-gradient
    test, the result in a record this thread polls) -- a search on a Python thread costs 60-100 us of interpreter under
    the lock this thread needs to queue kernels, which is what paced the small configurations.  polish="exact" only."""

    def __init__(self, x: "Executor"):
        self.x = x
        self.records = Records.of(x.plan, "host_search", x.s.ring, lambda: torch.zeros(dev.SEARCH_RECORD_WORDS, dtype=torch.int64))
        if x.plan.extra.get("freq_c") is None:
            x.plan.extra["freq_c"] = np.ascontiguousarray(x.plan.freq, dtype=np.float64)
        # (as many as run side by side: with spinning teams, one search more than the thread budget was cut for
        # oversubscribes the cores; a hedged second start raises the cap for itself)
        self.workers = max(1, x.s.n_workers)
        _lib.load().xm_hostsearch_set_workers(self.workers)

    def record(self, j):
        return self.records.recs[j % self.x.s.ring]

    def done(self, j, t: Ticket) -> bool:
        return dev.search_done(self.record(j), t.handle)

    def _submit(self, j, k, threads, rec, delay=0.0) -> int:
        """`xm_hostsearch_submit` of dataset j's slice (pinned, in its selection slot) after `delay` seconds."""
        x = self.x
        seq = self.records.next_seq()
        rec[7] = 0
        args = ("xm_hostsearch_submit", x.sel[j % x.s.ring].h_slice.data_ptr(), x.plan.n_out,
                x.plan.extra["freq_c"].ctypes.data, aps.METHODS.index(x.method), int(k), int(x.iw), int(bool(x.p0_only)),
                42, 0.01, 1000, int(threads), seq, rec.data_ptr())
        if delay:
            _abandon(rec)  # (the late search writes it whenever it ends, maybe after this call has returned)
            tm = threading.Timer(delay, _lib.call, args)
            tm.daemon = True
            tm.start()
        else:
            _lib.call(*args)
        return seq

    def submit(self, j, sl, k, pivot, threads) -> Ticket:
        return Ticket(self._submit(j, k, threads, self.record(j), self.x.slow_delay(j)), sl, k, pivot)

    def collect(self, i, t: Ticket, ev) -> SearchOutcome:
        """A search later than twice the typical time is submitted a second time with the whole team and the first to
        finish is taken (`Hedger`)."""
        x, h, b = self.x, self.x.hedger, i % self.x.s.ring
        rec = self.records.recs[b]
        deadline = h.deadline(i, ev["t_exchanged"], 3e-3, 1e-3)  # (x 3: a process's first searches also start the service's threads)
        can_hedge, second, hedged, nap = h.allowed(i), None, False, 0.0
        give_up = time.perf_counter() + 120.0
        while not dev.search_done(rec, t.handle):
            if second is not None and dev.search_done(*second):
                # the first submission is still on its way: it will write its record whenever it ends, so that record
                # leaves the ring (a later dataset's result in the same slot must not be overwritten by it)
                _abandon(rec)
                self.records.recs[b] = torch.zeros(dev.SEARCH_RECORD_WORDS, dtype=torch.int64)
                rec = second[0]
                break
            now = time.perf_counter()
            if can_hedge and second is None and now > deadline:
                h.last, hedged = i, True
                spare = torch.zeros(dev.SEARCH_RECORD_WORDS, dtype=torch.int64)  # (its own record: see above)
                _abandon(spare)
                _lib.load().xm_hostsearch_set_workers(self.workers + 1)  # (it must not wait in the queue)
                second = (spare, self._submit(i, t.k, x.s.fill_team, spare))
                _lib.load().xm_hostsearch_set_workers(self.workers)
            if now > give_up:
                raise RuntimeError("the search service did not answer within two minutes")
            nap = x.nap(nap)
            # (no time.sleep(0) here to hand over the interpreter lock: with the search teams spinning on every core of
            # the quota a yielding launch thread lost its CPU for 2-3 ms at a time, K = 20 went from 1.22 to 1.39-1.51
            # ms per step in two collections)
        r = dev.read_search_record(rec)
        h.record(i, 1e-6 * r["t_us"][5])
        timing = {"generations_ms": 1e-3 * r["t_us"][0], "polish_ms": 1e-3 * (r["t_us"][5] - r["t_us"][0])}
        out = _record_outcome(r, x.p0_only, t.k, timing)
        out.hedged = hedged
        return x.polish.settle(i, r, t.k, out)


class ThreadEngine:
    """Host searches on Python worker threads (`autophase_solver.solve`, one native call that releases the interpreter
    lock and brings its own team): the engine of the polish modes other than "exact".  With no search beside it
    (`n_workers` = 0) a search runs inline, on the launch thread."""

    def __init__(self, x: "Executor"):
        self.x, self.pool = x, None
        n_workers = x.s.n_workers
        if n_workers:
            self.pool = x.plan.extra.get(("search_pool", n_workers))
            if self.pool is None:
                # (one thread more than searches in flight: a search that was hedged keeps its thread until it ends)
                self.pool = x.plan.extra[("search_pool", n_workers)] = ThreadPoolExecutor(
                    max_workers=n_workers + 1, thread_name_prefix="xm-search")

    def record(self, j):
        return None

    def done(self, j, t: Ticket) -> bool:
        return not hasattr(t.handle, "done") or t.handle.done()

    def submit(self, j, sl, k, pivot, threads) -> Ticket:
        x = self.x
        if self.pool is None:
            return Ticket(x.search(sl, k, pivot, threads, x.events[j]), sl, k, pivot)
        return Ticket(self.pool.submit(x.search, sl, k, pivot, threads, x.events[j], x.slow_delay(j)), sl, k, pivot)

    def collect(self, i, t: Ticket, ev) -> SearchOutcome:
        if self.pool is None:
            return _opt_outcome(*t.handle, False, t.k)
        (p0, p1, opt), hedged = self._wait(i, t, ev)
        if "t_search_end" in ev and "t_search_begin" in ev:
            self.x.hedger.record(i, ev["t_search_end"] - ev["t_search_begin"])
        return _opt_outcome(p0, p1, opt, hedged, t.k)

    def _wait(self, i, t: Ticket, ev):
        x, h, fut = self.x, self.x.hedger, t.handle
        if not h.allowed(i):
            return fut.result(), False
        try:
            return fut.result(timeout=max(h.deadline(i, ev["t_exchanged"], 1.5e-3) - time.perf_counter(), 0.0)), False
        except FutureTimeout:
            h.last = i
            hedge_pool = x.plan.extra.get("hedge_pool")
            if hedge_pool is None:
                hedge_pool = x.plan.extra["hedge_pool"] = ThreadPoolExecutor(max_workers=1, thread_name_prefix="xm-hedge")
            again = hedge_pool.submit(x.search, t.sl, t.k, t.pivot, x.s.fill_team, {})
            done, _ = wait_first([fut, again], return_when=FIRST_COMPLETED)
            return (fut.result() if fut in done else again.result()), True


class DeviceEngine:
    """Searches as ONE workgroup each on the search partition of the chip (`xm_search_launch`, csrc/xm_search.hip:
    scipy's generations bit for bit, then the projected-gradient test scipy's polish starts with).  A search that does
    not pass the test is polished on the reference's route (`PolishHandoff`); one that runs far beyond the usual time
    (a landscape that keeps the generations going for tens of thousands of evaluations) is overtaken by a host search
    -- the search is a pure function of the slice."""

    def __init__(self, x: "Executor", partition_streams):
        self.x, self.partition_streams = x, partition_streams
        self.records = Records.of(x.plan, "dev_search", x.s.ring, dev.new_search_record)
        self.streams = list(partition_streams)

    def record(self, j):
        return self.records.recs[j % self.x.s.ring]

    def done(self, j, t: Ticket) -> bool:
        return dev.search_done(self.record(j), t.handle)

    def submit(self, j, sl, k, pivot, threads, after=None) -> Ticket:
        """`xm_search_launch` for dataset j on a search stream, behind the event `after` if given."""
        x = self.x
        st = self.streams[j % len(self.streams)]
        if after is not None:
            st.wait_event(after)
        seq = self.records.next_seq()
        dev.search_launch(x.sel[j % x.s.ring].h_slice[0], _uniform_axis(x.plan), self.record(j), seq, p0_only=x.p0_only,
                          stream=st)
        x.events[j]["t_search_begin"] = time.perf_counter()
        return Ticket(seq, sl, k, pivot)

    def collect(self, i, t: Ticket, ev) -> SearchOutcome:
        x = self.x
        rec = self.record(i)
        deadline = time.perf_counter() + max(4.0 * x.s.est_ms * 1e-3, 8e-3)
        nap = 0.0
        while not dev.search_done(rec, t.handle):  # (bounded: past the deadline a host search takes over)
            if time.perf_counter() > deadline:
                return self._overtake(i, rec)
            nap = x.nap(nap)
        ev["t_search_end"] = time.perf_counter()
        r = dev.read_search_record(rec)
        out = _record_outcome(r, x.p0_only, r["target_idx"], {"generations_ms": 1e-3 * r["t_us"][5], "polish_ms": 0.0,
                                                                "device": True})
        return x.polish.settle(i, r, out.k, out)

    def _overtake(self, i, rec) -> SearchOutcome:
        x = self.x
        sl = x.sel[i % x.s.ring].h_slice[0].numpy().copy()
        k = int(np.argmax(np.abs(sl)))
        p0, p1, opt = x.search(sl, k, float(x.plan.freq[k]), x.s.fill_team, {})
        # the kernel is still running: its record and its stream are retired (it will write the record when it ends;
        # the stream's later searches would queue behind it)
        s = i % len(self.streams)
        _abandon((rec, self.streams[s]))
        self.records.recs[i % x.s.ring] = dev.new_search_record()
        self.streams[s] = dev.replacement_search_stream(x.inputs[0].device, self.partition_streams)
        return _opt_outcome(p0, p1, opt, True, k)


# ---- the pipeline ------------------------------------------------------------------------------------------------

class Executor:
    """One call's software pipeline (`run`).  `guessed` / `started`: the newest dataset whose guess kernels are queued /
    whose search is started; `unverified`: datasets whose main pass is queued and whose guess is not settled yet."""

    def __init__(self, inputs, outputs, plan, s: Schedule, exchange, broadcast, rank_offset_rows, method, peak_width,
                 p0_only, trace, polish, search_streams=None):
        self.t_call = time.perf_counter()
        self.inputs, self.outputs, self.plan, self.s = inputs, outputs, plan, s
        self.exchange, self.broadcast, self.rank_offset_rows = exchange, broadcast, rank_offset_rows
        self.method, self.p0_only, self.trace, self.polish_mode = method, p0_only, trace, polish
        self.n_sets, self.n = len(inputs), plan.n_out
        self.c128 = inputs[0].dtype == torch.complex128
        self.bufs = Ring.of(plan, inputs[0], s)
        if s.use_guess and plan.extra.get("window32") is None:
            plan.extra["window32"] = plan.window.to(torch.float32).contiguous()
        self.sel = [None] * s.ring
        self.events = [dict() for _ in range(self.n_sets)]
        self.results = [None] * self.n_sets
        self.iw = aps.index_width_of(plan.freq, peak_width)
        self.pending, self.dev_tickets, self.unverified = {}, {}, []
        self.guessed = self.started = -1
        slow = os.environ.get("XM_TEST_SLOW_SEARCH")  # test hook "<dataset>,<ms>": that dataset's search starts late
        self.slow_j, self.slow_s = (int(slow.split(",")[0]), 1e-3 * float(slow.split(",")[1])) if slow else (-1, 0.0)
        self.host = ServiceEngine(self) if s.use_service else ThreadEngine(self)
        self.polish = PolishHandoff(self)
        self.device = DeviceEngine(self, search_streams) if s.use_dev else None
        self.hedger = Hedger(plan, s)

    def slow_delay(self, j) -> float:
        return self.slow_s if j == self.slow_j and j >= 0 else 0.0

    def nap(self, nap: float) -> float:
        """One turn of a polling wait: few cores per rank -- do not spin beside another rank's launch thread."""
        if self.s.blocking:
            nap = min(1e-4, nap + 1e-5)
            time.sleep(nap)
        return nap

    def search(self, sl, k, pivot, threads, ev, delay=0.0):
        """One host search on the calling thread (`ev`: its trace; dispatch latency = t_search_begin - t_exchanged)."""
        ev["t_search_begin"] = time.perf_counter()
        if delay:
            time.sleep(delay)
        out = aps.solve(sl, self.plan.freq, pivot, k, self.iw, method=self.method, p0_only=self.p0_only, threads=threads,
                        polish=self.polish_mode)
        ev["t_search_end"] = time.perf_counter()
        return out

    def guess_next(self):
        """Coarse spectra (or streaming L1 norms) + the selection stage on the winning row of the next dataset."""
        self.guessed += 1
        j, s, bufs, plan = self.guessed, self.s, self.bufs, self.plan
        b, ev, x2 = j % s.ring, self.events[j], self.inputs[j]
        if self.trace is not None:
            ev["pre0"], ev["pre1"] = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev["pre0"].record()
        if s.use_guess:
            dev.guess_rows(x2, self.n, plan.extra["window32"], bufs.est[b], bufs.gkey[b])
        else:
            dev.row_l1(x2, plan.window, plan.pad_left, out=bufs.norm[b], n_used=s.n_used, sub_step=s.sub_step,
                       key=bufs.gkey[b] if s.l1_keys else None)
        if self.trace is not None:
            ev["pre1"].record()
            ev["guess_kernel"] = dev.last_kernel()
        self.sel[b] = Selection(x2, plan, bufs.norm[b], bufs.zero_idx, index_from_slice=True,
                                key=bufs.gkey[b] if s.l1_keys else None, slot=bufs.sel_slots[b],
                                refine=(plan.extra["window32"], bufs.est[b], bufs.gkey[b], bufs.wkey, s.band)
                                if s.use_guess else None, blocking=s.blocking)
        if self.trace is not None:  # (the selection stage: exact check of the candidates + the winner's fp64 spectrum)
            ev["sel1"] = torch.cuda.Event(enable_timing=True)
            ev["sel1"].record()
        if s.use_dev and self.exchange is None and j >= s.cpu_fill and not slice_on_host():
            # one rank, slice computed by the device: the winner needs no exchange -- the search kernel is queued at
            # once, gated on the selection stage by an event; this thread does not wait for either
            self.dev_tickets[j] = self.device.submit(j, None, -1, 0.0, 0, after=self.sel[b].event)

    def start_search(self, j):
        """Selection of dataset j -> (exchange) -> its search on its engine."""
        s, ev, n = self.s, self.events[j], self.n
        ev["t_start"] = time.perf_counter()
        on_dev = s.use_dev and j >= s.cpu_fill
        if on_dev and self.exchange is None and not slice_on_host():  # queued behind its selection stage already
            ev["t_exchanged"] = ev["t_start"]
            self.pending[j] = Pending(None, self.device, self.dev_tickets.pop(j))
            return
        amax, flat, sl = self.sel[j % s.ring].wait()  # (guessed row's max, its row * n + arg-max of its fp64 spectrum, spectrum)
        ev["t_selected"] = time.perf_counter()
        gflat, mine, owner = self.rank_offset_rows * n + flat, True, 0
        if self.exchange is not None:  # the guess is global too: the rank with the largest estimate owns it
            mine, gflat, owner = self.exchange(amax, gflat)
        ev["t_exchanged"] = time.perf_counter()
        k = gflat % n
        res = AutophaseResult(0.0, 0.0, float(self.plan.freq[k]), int(gflat), int(k), amax)
        res.owner, res.mine = owner, mine
        if not mine:
            self.pending[j] = Pending(res, None, None)
            return
        # the first search fills the pipeline (the first main pass waits for it): whole team; the others have device
        # periods of slack (smaller teams for the searches right behind the first: slower, -1...3 %)
        engine = self.device if on_dev else self.host  # (several ranks: the owner of the winning row queues the kernel)
        ticket = engine.submit(j, sl, int(k), res.pivot, s.fill_team if j == 0 else s.team)
        self.pending[j] = Pending(res, engine, ticket)

    def fill_one_rank(self):
        """Filling the pipeline, one rank: every guess of the look-ahead is queued at once (the device works through
        them while the first search runs), searches start as their selection stages END -- this thread polls the events
        instead of blocking on each in turn -- and the moment the FIRST search is there its main pass is queued.
        Starting all the look-ahead's searches first, each behind a blocking wait for its selection (8 x (0.13 ms of
        kernels + the host's turnaround)), had the first main pass queued at 1.5-1.7 ms with the first search done at
        1.0 and the device idle in between (profiles/r04/fill.txt).  One search starts beside the first (it has the
        whole team for its millisecond; the others have device periods of slack and start right behind it)."""
        s, last = self.s, self.n_sets - 1
        while self.guessed < min(last, 1):  # (two guesses, then the first search: nothing else delays its start)
            self.guess_next()
        self.started = 0
        self.start_search(0)
        first = self.pending[0]
        while first.engine is not None and not first.engine.done(0, first.ticket):
            more_guesses = self.guessed < min(last, s.g_ahead)
            if more_guesses:  # one per turn: a launch takes this thread half the time the device needs for it
                self.guess_next()
            nxt = self.started + 1
            if nxt > min(last, s.s_look, 1):
                if more_guesses:
                    continue
                break  # (`collect` waits for the first search -- and hedges it if it is late)
            if nxt <= self.guessed and self.sel[nxt % s.ring].event.query():
                self.started = nxt
                self.start_search(nxt)
            elif s.blocking and not more_guesses:
                time.sleep(2e-5)

    def look_ahead(self, i):
        """Keep the guess kernels g_ahead and the searches s_look datasets in front of dataset i, every search right
        behind its own guess.  Where the fill is not event driven (`ramped`: several ranks, where the order of the
        exchange calls may not depend on anything a rank observes) the look-ahead is built up over the first datasets,
        three searches before the first main pass and three more with every dataset."""
        s, last = self.s, self.n_sets - 1
        if i == 0 and s.fast_fill:
            self.fill_one_rank()
        ramp = 2 + 3 * i if s.ramped else self.n_sets
        while self.started < min(last, i + s.s_look, ramp):
            while self.guessed < min(last, self.started + 1):
                self.guess_next()
            self.started += 1
            self.start_search(self.started)
        while self.guessed < min(last, i + s.g_ahead):
            self.guess_next()

    def collect(self, i) -> AutophaseResult:
        """Dataset i's (p0, p1): its search's outcome, from the owner to every rank."""
        ev, s, n = self.events[i], self.s, self.n
        if s.use_service or s.use_dev:
            self.polish.advance(self.pending)
        p = self.pending.pop(i)
        ev["t_collect"] = time.perf_counter()
        res = p.res
        if p.engine is not None:
            out = p.engine.collect(i, p.ticket, ev)
            if res is None:  # one rank, device engine: the record is the first the host hears of this dataset's winner
                slot = self.bufs.sel_slots[i % s.ring]
                gflat = (self.rank_offset_rows + int(slot[1].item()) // n) * n + out.k
                res = AutophaseResult(0.0, 0.0, float(self.plan.freq[out.k]), int(gflat), int(out.k),
                                      float(slot[0].item()) ** 0.5)
            res.p0, res.p1, res.nfev, res.fun, res.timing, res.hedged = (out.p0, out.p1, out.nfev, out.fun, out.timing,
                                                                         out.hedged)
        if self.broadcast is not None:
            res.p0, res.p1 = self.broadcast([res.p0, res.p1], res.owner)
        ev["t_solved"] = ev["t_table"] = time.perf_counter()
        return res

    def queue_main(self, i, res):
        """Dataset i's main pass with (p0, p1), leaving the true global arg-max for `verify`."""
        s, bufs, ev, b = self.s, self.bufs, self.events[i], i % self.s.ring
        if self.trace is not None:
            ev["main0"], ev["main1"] = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev["main0"].record()
        if s.use_keys:
            main_pass(self.plan, self.inputs[i], self.outputs[i], res.p0, res.p1, res.pivot, global_key=bufs.vkey[b],
                      key_result=bufs.vres[b])  # the kernel's last workgroup decodes + clears the key
        else:
            main_pass(self.plan, self.inputs[i], self.outputs[i], res.p0, res.p1, res.pivot, want_argmax=True,
                      absmax2=bufs.tmax[b], argidx=bufs.tidx[b], argmax_value_only=True)
        if self.trace is not None:
            ev["main1"].record()
            ev["main_kernel"] = dev.last_kernel()
        if not s.use_keys:
            dev.argmax_reduce_async(bufs.tmax[b], bufs.tidx[b], self.n, gmax=bufs.vmax[b], gflat=bufs.vflat[b])
        ev["verify_event"] = torch.cuda.Event(blocking=s.blocking)
        ev["verify_event"].record()

    def verify(self, i):
        """True global arg-max row of dataset i (its main pass has been queued) against the guess; repair."""
        b, n, plan, off = i % self.s.ring, self.n, self.plan, self.rank_offset_rows
        res, ev = self.results[i], self.events[i]
        ev["verify_event"].synchronize()
        if self.s.use_keys:
            m2, fl = dev.read_key_result(self.bufs.vres[b], self.c128)
            tmax, trow = m2 ** 0.5, fl // n
        else:
            tmax, trow = float(self.bufs.vmax[b].item()) ** 0.5, int(self.bufs.vflat[b].item()) // n
        g_row, owner, mine = off + trow, 0, True
        if self.exchange is not None:
            mine, gflat, owner = self.exchange(tmax, (off + trow) * n)
            g_row = gflat // n
        if g_row == res.flat_index // n:
            res.speculation = "hit"
            if mine:
                res.max_abs = tmax  # the guess stage only knew an estimate
            return
        # wrong guess: the owner of the true row fetches its spectrum (fp64), searches again, everyone rotates
        vals = [0.0, 0.0, 0.0, 0.0]
        if mine:
            x1 = self.inputs[i][g_row - off:g_row - off + 1].to(torch.complex128)
            if plan.window64 is None:
                plan.window64 = torch.from_numpy(np.ascontiguousarray(plan.window_host)).to(x1.device, torch.float64)
            if slice_on_host():
                sl = winner_spectrum(plan, x1[0].cpu().numpy())
            else:
                sl = dev.pipeline_fused(x1, n, plan.pad_left, window=plan.window64).out[0].cpu().numpy()
            k = int(np.argmax(np.abs(sl)))
            p0, p1, opt = aps.solve(sl, plan.freq, float(plan.freq[k]), k, self.iw, method=self.method,
                                    p0_only=self.p0_only, polish=self.polish_mode)
            vals = [p0, p1, float(k), float(opt.nfev)]
        if self.broadcast is not None:
            vals = self.broadcast(vals, owner)
        p0, p1, k = float(vals[0]), float(vals[1]), int(vals[2])
        pivot = float(plan.freq[k])
        # the dataset's FIDs are still there: run its main pass again with the right parameters (one read + one write of
        # the dataset, and the result is the classic schedule's to the bit; rotating the wrong output in place by the
        # phase ratio reads AND writes the spectra and adds two roundings)
        main_pass(plan, self.inputs[i], self.outputs[i], p0, p1, pivot)
        res.p0, res.p1, res.pivot, res.target_idx = p0, p1, pivot, k
        res.flat_index, res.max_abs, res.owner, res.mine = g_row * n + k, tmax, owner, mine
        res.nfev = int(vals[3]) if mine else 0
        res.speculation = "repaired"

    def run(self):
        self.events[0]["t_call"] = self.t_call
        for i in range(self.n_sets):
            self.look_ahead(i)
            res = self.results[i] = self.collect(i)
            # Settle earlier guesses: always those two or more datasets back (their main pass finished a device period
            # ago, so this never waits -- neither for this GPU nor, through the exchange, for another rank's), and at
            # once any whose output buffer is about to be overwritten (a repair must still find its spectra there).
            out_i = self.outputs[i].data_ptr()
            while self.unverified and (self.unverified[0] <= i - 2
                                       or any(self.outputs[j].data_ptr() == out_i for j in self.unverified)):
                self.verify(self.unverified.pop(0))
            self.queue_main(i, res)
            self.unverified.append(i)
            if self.trace is not None:
                self.trace.append(self.events[i])
        self.events[-1]["t_last_queued"] = time.perf_counter()
        while self.unverified:
            self.verify(self.unverified.pop(0))
        self.events[-1]["t_return"] = time.perf_counter()
        return self.results


def run_speculative(inputs, outputs, plan, exchange, broadcast, rank_offset_rows, overlap, method, peak_width, p0_only,
                    trace, polish="exact"):
    """`run_stream(speculate=True)`."""
    s = make_schedule(inputs, plan, exchange, broadcast, overlap, method, polish)
    args = (inputs, outputs, plan, s, exchange, broadcast, rank_offset_rows, method, peak_width, p0_only, trace, polish)
    if not s.use_dev:
        return Executor(*args).run()
    # Search kernels need a whole CU's registers for milliseconds, the streaming kernels are persistent grids sized to
    # fill every CU: sharing one pool, a search waits for a kernel boundary to start and the main pass then finds CUs
    # taken (measured: main pass +7 %, stalls of milliseconds).  So the chip is split for the duration of the call --
    # `reserved` CUs, spread over the eight XCDs, for the searches; the streaming kernels run on a stream that owns
    # the rest and size their grids by it (`xm_stream_create`).
    x0 = inputs[0]
    reserved = int(min(32, 8 * -(-max(s.dev_ahead, 1) // 8)))
    part = dev.chip_partition(x0.device, reserved, n_search=min(16, max(s.dev_ahead, 1) + 2))
    caller = torch.cuda.current_stream(x0.device)
    part.compute.wait_stream(caller)
    try:
        with torch.cuda.stream(part.compute):
            return Executor(*args, search_streams=part.search).run()
    finally:
        caller.wait_stream(part.compute)
