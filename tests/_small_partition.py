"""The smallest CU partition run_speculative creates (8 CUs: one per XCD), as a stream for tests.

A persistent kernel caps its grid at the CUs of its stream times the resident workgroups per CU (xm_resident_blocks,
csrc/xm_host.h).  On the whole chip that cap is 256 ... 2048 workgroups and the suite's shapes run every item loop once;
on this stream it is at most `grid_bound(nt)` and `items_for(nt)` items make every workgroup come round three times,
with a partial last round, whatever the kernel's real occupancy is."""
import numpy as np

CUS = 8
_STREAM = []


def stream():
    """The one 8-CU stream of the process: dev.chip_partition(cuda, 8, 1).search[0]."""
    import torch

    from xmris_amd import _lib
    from xmris_amd import device as dev

    if not _STREAM:
        st = dev.chip_partition(torch.device("cuda"), CUS, 1).search[0]
        # (xm_stream_cus returns the count itself, so it is called past _lib.call, which reads a result as a status)
        cus = _lib.load().xm_stream_cus(st.cuda_stream)
        assert cus == CUS, f"the search stream of an {CUS}-CU partition owns {cus} CUs"
        _STREAM.append(st)
    return _STREAM[0]


def grid_bound(nt, factor=1):
    """No `nt`-thread kernel has more workgroups than this on stream(): CUs x (threads a CU holds // nt), times the
    `factor` of a launcher that asks for several grids' worth (k_axis_dft: 8)."""
    import torch

    props = torch.cuda.get_device_properties(torch.cuda.current_device())
    return int(factor) * CUS * (props.max_threads_per_multi_processor // int(nt))


def items_for(nt, factor=1):
    """Three full rounds of the largest possible grid and a partial fourth."""
    return 3 * grid_bound(nt, factor) + 5


def rows_for(nt, per_item=1):
    """The odd row count of the row kernels: three rounds of `per_item`-row items, and one row more."""
    return 3 * grid_bound(nt) * int(per_item) + 1


def _host(v):
    if v is None:
        return None
    if isinstance(v, np.ndarray):
        return v.copy()
    return v.detach().cpu().numpy()


def both(fn):
    """fn() -> dict of device tensors (None, or host arrays, allowed), launched on the current stream and then, on the
    same inputs, inside stream().  The device is idle before, between and after, so no tensor crosses streams
    unsynchronised.  Returns (default, small): dicts of numpy arrays, each with dev.last_kernel() under "kernel"."""
    import torch

    from xmris_amd import device as dev

    out = []
    side = stream()
    torch.cuda.synchronize()
    for st in (None, side):
        if st is None:
            r = fn()
            name = dev.last_kernel()
        else:
            with torch.cuda.stream(st):
                r = fn()
                name = dev.last_kernel()
        torch.cuda.synchronize()
        host = {k: _host(v) for k, v in r.items()}
        host["kernel"] = name
        out.append(host)
    return out[0], out[1]


def sample(n_items, bound, extra=()):
    """At most 16 items for the oracle: the first, the last, and items of the second and third rounds (a round is at most
    `bound` items long, so items bound ... 2 bound - 1 are past every workgroup's first trip, 2 bound ... past its
    second)."""
    picks = [0, n_items - 1, bound, bound + 1, bound + bound // 2, 2 * bound - 1, 2 * bound, 2 * bound + 1,
             2 * bound + bound // 2, 3 * bound - 1, 3 * bound, *extra]
    seen = []
    for i in picks:
        if 0 <= i < n_items and i not in seen:
            seen.append(int(i))
    return seen[:16]
