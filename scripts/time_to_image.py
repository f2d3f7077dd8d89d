"""GPU timing of to_image (xm_axis_dft) against the staged route (phase_apply, zero_fill, fft: the calls that were there
before the kernel), Hamming filter, seeded complex noise made on the GPU, time last:

  A     16 coils x 32 x 32 x 2048, no zero fill, complex64        B  as A with matrix=64
  C     8 coils x 16 x 16 x 8 x 2048 (three dims)                  D  4 coils x 64 x 64 x 2048
  A128  as A in complex128

Per workload and route: seconds (HIP events around the call; warm-up, median of the repeats), the algorithmic bytes
(every pass reads its input once and writes its output once) over that time as GB/s and as a fraction of the device
copy rate measured in the same run (a 1:1 copy of the workload's input, read + write bytes), and the seconds of every
pass on its own (the same call on one dim, on the tensor the passes before it left) and, for the kernel route, of the
launch alone (``device.axis_dft`` with the table already on the device: what the call adds is host work, the table's
fp64 arithmetic and its upload).

    python scripts/time_to_image.py --out profiles/mrsi/time_to_image.json
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name -> (shape, dims, transformed dims, matrix, dtype)
WORKLOADS = {
    "A": ((16, 32, 32, 2048), ("coil", "kx", "ky", "time"), ("kx", "ky"), None, "complex64"),
    "B": ((16, 32, 32, 2048), ("coil", "kx", "ky", "time"), ("kx", "ky"), 64, "complex64"),
    "C": ((8, 16, 16, 8, 2048), ("coil", "kx", "ky", "kz", "time"), ("kx", "ky", "kz"), None, "complex64"),
    "D": ((4, 64, 64, 2048), ("coil", "kx", "ky", "time"), ("kx", "ky"), None, "complex64"),
    "A128": ((16, 32, 32, 2048), ("coil", "kx", "ky", "time"), ("kx", "ky"), None, "complex128"),
}


def timed(run, warmup, repeats):
    import torch

    for _ in range(warmup):
        run()
    torch.cuda.synchronize()
    times, res = [], None
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        res = run()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) / 1e3)
    return times, float(np.median(times)), res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.repeats < 3:
        ap.error("--repeats must be at least 3")

    import torch

    from xmris_amd import LabeledArray, to_image
    from xmris_amd import device as dev
    from xmris_amd.processing.mrsi import axis_table, filter_weights

    rec = {"device": torch.cuda.get_device_name(0), "filter": "hamming", "repeats": a.repeats, "workloads": []}
    for name in a.workloads.split(","):
        shape, dims, tdims, matrix, dtype = WORKLOADS[name]
        tdt = getattr(torch, dtype)
        g = torch.Generator(device="cuda").manual_seed(2024)
        x = torch.view_as_complex(torch.randn(shape + (2,), generator=g, device="cuda", dtype=torch.float32)).to(tdt)
        item = x.element_size()
        coords = {d: np.arange(float(n)) - n // 2 for d, n in zip(dims, shape) if d in tdims}
        la = LabeledArray(x, dims, coords)
        dst = torch.empty_like(x)
        _, t_copy, _ = timed(lambda: dst.copy_(x), a.warmup, a.repeats)
        copy_gbs = 2.0 * x.numel() * item / t_copy / 1e9
        del dst
        w = {"name": name, "shape": list(shape), "dims": list(tdims), "matrix": matrix, "dtype": dtype,
             "copy_seconds": t_copy, "copy_gbs": copy_gbs, "routes": {}}
        for route, staged in (("kernel", False), ("staged", True)):
            run = lambda: to_image(la, dim=tdims, matrix=matrix, filter="hamming", _staged=staged)  # noqa: E731
            times, t_med, res = timed(run, a.warmup, a.repeats)
            passes, cur, nbytes = [], la, 0
            for d in tdims:
                one = lambda: to_image(cur, dim=d, matrix=matrix, filter="hamming", _staged=staged)  # noqa: E731
                _, t_pass, nxt = timed(one, a.warmup, a.repeats)
                moved = (int(np.prod(cur.shape)) + int(np.prod(nxt.shape))) * item
                launch = None
                if not staged:  # the launch alone: the table already on the device, no Python around it
                    n_d, ax = cur.sizes[d], cur.get_axis_num(d)
                    tab = torch.from_numpy(axis_table(n_d, nxt.shape[ax], filter_weights("hamming", n_d))).to("cuda")
                    _, launch, _ = timed(lambda: dev.axis_dft(cur.data, ax, tab), a.warmup, a.repeats)
                passes.append({"dim": d, "n": cur.sizes[d], "m": nxt.shape[cur.get_axis_num(d)], "seconds": t_pass,
                               "algorithmic_bytes": moved, "algorithmic_gbs": moved / t_pass / 1e9,
                               "fraction_of_copy_rate": moved / t_pass / 1e9 / copy_gbs, "kernel": dev.last_kernel(),
                               "launch_alone_seconds": launch,
                               "launch_alone_fraction_of_copy_rate": moved / launch / 1e9 / copy_gbs if launch else None})
                nbytes += moved
                cur = nxt
            w["routes"][route] = {"seconds": times, "seconds_median": t_med, "algorithmic_bytes": nbytes,
                                  "algorithmic_gbs": nbytes / t_med / 1e9,
                                  "fraction_of_copy_rate": nbytes / t_med / 1e9 / copy_gbs, "passes": passes}
            del res, cur, nxt
        w["staged_over_kernel"] = w["routes"]["staged"]["seconds_median"] / w["routes"]["kernel"]["seconds_median"]
        rec["workloads"].append(w)
        del x, la
        torch.cuda.empty_cache()
    text = json.dumps(rec, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
