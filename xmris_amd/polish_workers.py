"""Worker processes for the polish on the reference's route: `PolishWorkers` (the parent's side), `polish_workers()`
(the process-wide instance) and `main()` (the child's loop).

A search whose best member does not pass scipy's projected-gradient test is polished on the reference's own route --
scipy's L-BFGS-B on the NUMPY objective (processing/phasing.py:276-284 with scipy's defaults): a few milliseconds of
small numpy operations, i.e. of interpreter.  Run on threads of the process that queues the kernels, those milliseconds
are fought for under its interpreter lock (heterogeneous datasets: 13 searches of 16 need the polish, and the launch
thread fell from 1.4 to 2.3 ms per dataset); run in a child, they cost that process nothing.  The child never touches
the GPU or the HIP library: it imports numpy, scipy and the objective statements only (`autophase_solver` is imported
where it is used, and loads the library only for a native objective), and talks length-prefixed pickles over its
stdin / stdout."""
from __future__ import annotations

import atexit
import os
import pickle
import queue
import struct
import subprocess
import sys
import threading
from concurrent.futures import ThreadPoolExecutor

from . import cpu_budget

_CHILD = "from xmris_amd import polish_workers as w; w.main()"


def _polish(args):
    from .autophase_solver import polish_reference  # (not at the top: that module imports this one)

    return polish_reference(*args)


def _send(stream, obj):
    blob = pickle.dumps(obj, protocol=pickle.HIGHEST_PROTOCOL)
    stream.write(struct.pack("<q", len(blob)))
    stream.write(blob)
    stream.flush()


def _receive(stream):
    """The next message, or None at the end of the stream."""
    head = stream.read(8)
    if len(head) < 8:
        return None
    return pickle.loads(stream.read(struct.unpack("<q", head)[0]))


class PolishWorkers:
    """A few worker PROCESSES (`main` below, started as plain children: `python -c ...`, no fork of
    this process, no re-import of its main module) that run `polish_reference` away from this process's interpreter
    lock.  `submit(...)` takes `polish_reference`'s arguments and returns a future.  Nobody ever waits for a worker to
    come up: a worker joins the free list when it has reported ready (its imports take ~1 s of CPU), and a request that
    finds no free worker -- none started yet, all busy, one died -- is polished by the future's own thread.
    `start()` launches the children (idempotent); with `lazy` the first request does (several ranks on one node: 6 x 4
    interpreters importing scipy at the start of a stream ate a 16-CPU quota and the cgroup was throttled for
    40-60 ms inside the timed region, profiles/r04/rehearsal_6ranks.txt)."""

    def __init__(self, n: int = 4, lazy: bool = False):
        self._n = max(1, int(n))
        self._alive = 0  # workers that have reported ready and have not been found dead
        self._free = queue.Queue()
        self._procs = []
        self._started = False
        self._lock = threading.Lock()
        # (threads that mostly wait on a pipe: they hold the interpreter lock for microseconds per request)
        self._pool = ThreadPoolExecutor(max_workers=self._n, thread_name_prefix="xm-polish")
        atexit.register(self.close)
        if not lazy:
            self.start()

    def start(self):
        with self._lock:
            if self._started:
                return
            self._started = True
            root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
            env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""), OMP_NUM_THREADS="1",
                       OPENBLAS_NUM_THREADS="1", MKL_NUM_THREADS="1")
            for _ in range(self._n):
                try:
                    pr = subprocess.Popen([sys.executable, "-c", _CHILD], stdin=subprocess.PIPE, stdout=subprocess.PIPE,
                                          env=env, cwd=root)
                except OSError:
                    break
                self._procs.append(pr)
                threading.Thread(target=self._await_ready, args=(pr,), daemon=True, name="xm-polish-ready").start()

    def _await_ready(self, pr):
        try:
            if pr.stdout.read(8) == b"XMREADY\n":  # (written by the worker once numpy, scipy and the objective are imported)
                with self._lock:
                    self._alive += 1
                self._free.put(pr)
        except Exception:  # noqa: BLE001 -- a worker that never reports is never used
            pass

    def submit(self, *args):
        if not self._started:
            self.start()
        return self._pool.submit(self._call, args)

    def _call(self, args):
        # no worker is up (yet, or any more): this thread does it; otherwise wait for one to come free -- a polish in
        # this process costs the launch thread its share of the interpreter lock, which is what the workers are for
        pr = None
        while pr is None:
            if self._alive <= 0:
                return _polish(args)
            try:
                pr = self._free.get(timeout=0.02)
            except queue.Empty:
                pass
        try:
            if pr.poll() is None:
                _send(pr.stdin, args)
                reply = _receive(pr.stdout)
                if reply is not None and reply[0] == "ok":
                    return reply[1]
        except Exception:  # noqa: BLE001 -- any trouble with a worker: this thread does the polish
            pass
        finally:
            if pr.poll() is None:
                self._free.put(pr)
            else:  # (found dead, before or during the request: it leaves the count, nobody waits for it again)
                with self._lock:
                    self._alive -= 1
        return _polish(args)

    def close(self):
        for pr in self._procs:
            try:
                pr.stdin.close()
            except Exception:  # noqa: BLE001
                pass
        for pr in self._procs:
            try:
                pr.wait(timeout=2.0)
            except Exception:  # noqa: BLE001
                pr.kill()
            try:
                pr.stdout.close()
            except Exception:  # noqa: BLE001
                pass
        self._procs = []


_POLISH_WORKERS = None


def polish_workers():
    """The process-wide `PolishWorkers`, created on first use.  How many (`XM_POLISH_WORKERS`): up to four, and at most
    one per two CPUs of this rank's share; one rank alone starts them at once, several ranks on a node start theirs
    with the first search that needs a polish."""
    global _POLISH_WORKERS
    if _POLISH_WORKERS is None:
        ranks = cpu_budget.local_world()
        n = int(os.environ.get("XM_POLISH_WORKERS", "0")) or max(1, min(4, cpu_budget.cpu_share() // (2 * ranks)))
        _POLISH_WORKERS = PolishWorkers(n, lazy=ranks > 1)
    return _POLISH_WORKERS


def main():
    """The child: answers `polish_reference` requests from its stdin until that closes."""
    from . import autophase_solver  # noqa: F401 -- now, while nobody waits, like scipy:

    try:  # (the first request must not pay for scipy's import)
        import scipy.optimize  # noqa: F401
        from scipy.optimize import _lbfgsb  # noqa: F401
    except ImportError:
        pass
    inp, out = sys.stdin.buffer, sys.stdout.buffer
    sys.stdout = sys.stderr  # (anything a library prints must not end up in the reply stream)
    out.write(b"XMREADY\n")  # (eight bytes: the parent hands requests only to workers that have said this)
    out.flush()
    while True:
        args = _receive(inp)
        if args is None:
            return
        try:
            reply = ("ok", _polish(args))
        except Exception as e:  # noqa: BLE001 -- reported to the caller, which polishes itself
            reply = ("error", repr(e))
        _send(out, reply)
