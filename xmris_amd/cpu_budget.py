"""The host CPU policy in one place: how many CPUs this process may use, how many threads a (p0, p1) search gets --
alone, beside the other searches of a streaming call, beside the other ranks of its node -- and how many searches a
streaming call keeps in flight.  Pure Python on `os` alone: the polish worker processes import it too."""
from __future__ import annotations

import os

_CPU_SHARE = None


def cpu_share() -> int:
    """CPUs this process may use: scheduler affinity, capped by the cgroup v2 quota.  Read once per process (the
    executor asks on every dataset: a sched_getaffinity call and a file read on the launch thread; advisor, round 3)."""
    global _CPU_SHARE
    if _CPU_SHARE is None:
        _CPU_SHARE = _read_cpu_share()
    return _CPU_SHARE


def _read_cpu_share() -> int:
    try:
        cpus = len(os.sched_getaffinity(0))
    except AttributeError:
        cpus = os.cpu_count() or 1
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            quota, period = f.read().split()[:2]
        if quota != "max":
            cpus = min(cpus, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    return cpus


def local_world() -> int:
    """Ranks on this node, as the launcher's environment says; one without a launcher."""
    return max(1, int(os.environ.get("LOCAL_WORLD_SIZE", "1")))


def scarce_cpus() -> bool:
    """Several ranks on few cores (fewer than four per rank): host waits on device events should BLOCK (interrupt)
    instead of spinning -- a spinning wait of one rank takes the core another rank's search team is running on."""
    if os.environ.get("XM_BLOCKING_SYNC"):  # tuning switch
        return os.environ["XM_BLOCKING_SYNC"] != "0"
    ranks = local_world()
    return ranks > 1 and cpu_share() < 4 * ranks


def default_threads() -> int:
    """Team size for the native objective: at most 16 and at most HALF of this process's share of the CPUs it may use
    (scheduler affinity and the cgroup v2 quota), as a power of two; several ranks on one node: see below."""
    if os.environ.get("XM_SOLVER_THREADS"):  # tuning switch
        return max(1, min(32, int(os.environ["XM_SOLVER_THREADS"])))
    cpus = cpu_share()
    ranks = local_world()
    if ranks > 1:
        # Several ranks on one node share its cores.  Searches are per DATASET, not per rank: only the rank that owns
        # a dataset's winning spectrum searches, the streaming executor keeps its look-ahead's worth of searches (two to four)
        # in flight on the whole node (`stream.make_schedule`), and the other ranks wait for the
        # broadcast sleep-polling.  So the node-wide budget is what the ranks' launch threads leave: one core per rank
        # is reserved for launching and polling (a launch thread is busy for ~0.2 ms of a 1.2 ms step), the searches
        # in flight share the rest -- 16 CPUs and 8 ranks: 8 cores, 4 per search (1.1 ms of generations; round 2's
        # (cpus - 2 ranks) / 2 left ONE thread there: 3.2 ms against a 1.2 ms device period).  Any team size works (a
        # batch of evaluations is cut into 16+ work units).
        return max(1, min(16, cpus - ranks))
    # Half of the share, as a power of two (the work units of a batch are 4 evaluations x 4 parts): a team that
    # fills the whole CPU quota while it spins leaves no headroom for the HIP runtime's threads, and a cgroup that
    # overdraws its quota is frozen until the next 100 ms period.
    share = max(1, cpus // 2)
    team = 1
    while team * 2 <= min(16, share):
        team *= 2
    return team


def burst_threads() -> int:
    """Team size for ONE search with nothing beside it (a single accessor call, or the search that fills a streaming
    call's pipeline: the device waits for it): the whole share of the CPUs this process may use, up to 16 --
    `default_threads` keeps half of it free because a streaming executor's teams spin for as long as it runs; a
    millisecond does not reach the quota."""
    if os.environ.get("XM_SOLVER_THREADS") or local_world() > 1:
        return default_threads()
    cpus = cpu_share()
    team = 1
    while team * 2 <= min(16, cpus):
        team *= 2
    return max(team, default_threads())


def stream_threads(host_paced: bool = False) -> int:
    """Thread budget of ALL the searches a streaming executor keeps in flight (`search_workers` divides it).
    One rank on its node, two or three searches in flight (the device paces the steps; each search is busy for
    about half of the device periods it has): THREE QUARTERS of the share, up to 12 -- with two in flight, six threads
    apiece ran the generations in 1.25 instead of 1.45 ms at the same throughput (round 3, six interleaved pairs at the
    driver's K = 20: 51.5 vs 51.6 M spectra/s, 6.5 vs 5.3 cores busy); the executor now keeps THREE in flight with four
    threads each (`search_workers`: the same throughput again, a third device period of slack for a search
    that runs late).  The WHOLE share (two teams of eight, 1.05 ms) is 2 % faster when nothing goes wrong and stalled
    for 2-5 ms in three of seven runs: sixteen spinning threads plus the launch thread oversubscribe a 16-CPU quota.
    `host_paced` (more than three searches in flight: every team spins all the time): the whole share (see below; round
    3, with the searches on Python threads: half).  Several ranks on one node, or XM_SOLVER_THREADS: `default_threads`."""
    if os.environ.get("XM_SOLVER_THREADS") or local_world() > 1:
        return default_threads()
    cpus = min(16, cpu_share())
    if host_paced:
        # Round 4: the searches run on native threads of the library now (`xm_hostsearch_submit`), no interpreter lock
        # is fought over, and where the searches pace the steps the WHOLE share is theirs -- 16,384 x 2048 -> 4096 with
        # four searches in flight: 0.38 ms per dataset with teams of two (round 3's half share), 0.31 with three,
        # 0.26 with four (profiles/r04/search_workers.txt).
        return max(default_threads(), cpus)
    return max(default_threads(), cpus - cpus // 4)


# measured speed-up of one host search with a team of 1 / 2 / 4 / 8 / 16 threads
_SPEEDUP = {1: 1.0, 2: 1.73, 4: 3.05, 8: 4.25, 16: 5.7}


def search_ms(n_out: int, threads: int) -> float:
    """Host search time (ms) with a team of `threads` (n_out = 8192, ACME: 3.2 / 1.9 / 1.1 / 0.76 ms of generations with
    1 / 2 / 4 / 8 threads + 0.3 ms of polish; generations scale with n_out)."""
    gain = _SPEEDUP[max(k for k in _SPEEDUP if k <= max(1, threads))]
    return 0.3 + 3.2 * (n_out / 8192.0) / gain


def search_workers(plan, n_rows: int, elem_bytes: int, threads: int | None = None):
    """(searches in flight, threads per search) for the streaming executor; of `plan` (a `pipeline.PipelinePlan`) only
    `n_in` / `n_out` are read.  A search is O(1) per dataset on the host
    (`search_ms`); the device period is the dataset's compulsory traffic at ~5.5 TB/s plus ~0.12 ms of small launches.
    Three searches at a time with a third of the team each where that keeps up with the device; otherwise four with a
    quarter each (a smaller team spends fewer core-milliseconds per search).  Measured (16-CPU share; ms per step with
    2 / 4 / 8 in flight): 16,384 x 2048 -> 4096: 0.73 / 0.60 / 0.79, 32,768 x 1536: 0.49 / 0.47 / 0.66, 65,536 x 4096
    -> 8192: 1.17 / 1.19 / 1.23 -- eight single-thread searches lose to the interpreter lock (every search ends in
    scipy's polish, ~0.3 ms of Python)."""
    def team_of(w):  # an explicit budget (tests, tuning) is divided evenly
        return max(1, threads // w) if given else search_team(w)

    given = threads is not None
    if not given:
        threads = stream_threads()
    device_ms = n_rows * (plan.n_in + plan.n_out) * elem_bytes / 5.5e9 + 0.12
    # THREE in flight where the device paces the steps (teams of four out of twelve threads): a search then has three
    # device periods, ~2 ms of slack instead of ~1 for a search that runs late (a contended host), at the same
    # throughput on a quiet one -- six A/B pairs at K = 20: 51.7 vs 51.4 M spectra/s, three at K = 100: 55.35 vs
    # 55.20, 5.7 instead of 6.8 cores busy.
    w = 3
    if search_ms(plan.n_out, max(1, threads // w)) / w > 0.8 * device_ms and threads >= 4:
        w = 4
    return w, team_of(w)


def search_team(workers: int) -> int:
    """Threads per search with `workers` searches in flight (`stream_threads`: more than three in flight means the host
    paces the steps)."""
    return max(1, stream_threads(host_paced=workers > 3) // max(1, workers))
