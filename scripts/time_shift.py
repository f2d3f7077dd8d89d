"""GPU timing of the per-row time shift (xm_shift_time): seeded random data [coils, samples, time],
one delay per sample (tau_s = s / S dwells), time last:

  A       16 coils x 3200 samples x 2048 points, complex64 (workload A of section 17)
  A128    the same in complex128
  Apad    A with pad_to = 4096
  A1536   N = L = 1536, complex64

Per workload: seconds of the fused launch and of the staged route on the same build (``device.shift_time(staged=True)``:
zero fill, transform, ramp product, inverse transform, crop) -- HIP events around a few calls each, divided by their
number; warm-up, median of the repeats, the two routes alternating; input + output bytes over the fused time as GB/s and
as a fraction of the copy11 rate of tools/stream_ceiling measured in the same run (a child process of its own, before the
first workload; the tool is built when it is missing); and the largest difference of the two routes' results relative to
the largest magnitude.

    python scripts/time_shift.py --out profiles/shift/time_shift.json
"""
import argparse
import json
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name -> (coils, samples, N, L, dtype)
WORKLOADS = {
    "A": (16, 3200, 2048, 2048, "complex64"),
    "A128": (16, 3200, 2048, 2048, "complex128"),
    "Apad": (16, 3200, 2048, 4096, "complex64"),
    "A1536": (16, 3200, 1536, 1536, "complex64"),
}
INNER = 20  # calls between two events: the host queues ahead, so the figure is the device's time per call


def tools_copy_gbs():
    """The copy11 line of tools/stream_ceiling (a child process of its own); the tool is built first when it is missing."""
    exe = os.path.join(ROOT, "tools", "stream_ceiling")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.join(ROOT, "tools"), "stream_ceiling"], check=True)
    out = subprocess.run([exe, "16384", "10"], capture_output=True, text=True, timeout=120, check=True).stdout
    for line in out.splitlines():
        m = re.search(r"([0-9]+(?:\.[0-9]+)?)\s*GB/s", line)
        if line.startswith("copy11") and m:
            return float(m.group(1))
    raise RuntimeError("tools/stream_ceiling printed no copy11 line:\n" + out)


def once(run, inner=INNER):
    import torch

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        res = run()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / 1e3 / inner, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    from xmris_amd import device as dev

    copy11 = tools_copy_gbs()
    rec = {"device": torch.cuda.get_device_name(0), "repeats": a.repeats, "calls_per_timing": INNER,
           "tools_stream_ceiling_copy11_gbs": copy11, "workloads": []}
    for name in a.workloads.split(","):
        coils, S, N, L, dtype = WORKLOADS[name]
        tdt = getattr(torch, dtype)
        g = torch.Generator(device="cuda").manual_seed(2024)
        x = torch.view_as_complex(torch.randn((coils, S, N, 2), generator=g, device="cuda", dtype=torch.float32)).to(tdt)
        frac = torch.arange(S, dtype=torch.float64, device="cuda") / S
        routes = {"fused": lambda: dev.shift_time(x, 2, frac, S, 1, L), "staged": lambda: dev.shift_time(x, 2, frac, S, 1, L, staged=True)}
        assert dev.shift_time_fused(L, dtype == "complex128")
        times, kernels, results = {k: [] for k in routes}, {}, {}
        for _ in range(a.warmup):
            for k, run in routes.items():
                run()
        torch.cuda.synchronize()
        for _ in range(a.repeats):  # the two routes alternate
            for k, run in routes.items():
                t, results[k] = once(run)
                times[k].append(t)
                kernels[k] = dev.last_kernel()
        item = x.element_size()
        moved = 2 * x.numel() * item
        t_f, t_s = float(np.median(times["fused"])), float(np.median(times["staged"]))
        scale = float(results["staged"].abs().max().item())
        rec["workloads"].append({
            "name": name, "coils": coils, "samples": S, "points": N, "transform_length": L, "dtype": dtype,
            "bytes_in_plus_out": moved, "fused_kernel": kernels["fused"], "staged_last_kernel": kernels["staged"],
            "fused_seconds": times["fused"], "fused_seconds_median": t_f, "staged_seconds": times["staged"],
            "staged_seconds_median": t_s, "speedup_vs_staged": t_s / t_f, "fused_in_plus_out_gbs": moved / t_f / 1e9,
            "fused_fraction_of_tools_copy11": moved / t_f / 1e9 / copy11,
            "staged_in_plus_out_gbs": moved / t_s / 1e9,
            "routes_differ_relative_to_max": float((results["fused"] - results["staged"]).abs().max().item()) / scale})
        del x, results
        torch.cuda.empty_cache()
    text = json.dumps(rec, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")
    tol = {"complex64": 1e-5, "complex128": 1e-12}
    worst = {w["name"]: w["routes_differ_relative_to_max"] for w in rec["workloads"]}
    assert all(worst[w["name"]] <= tol[w["dtype"]] for w in rec["workloads"]), f"the two routes disagree: {worst}"


if __name__ == "__main__":
    main()
