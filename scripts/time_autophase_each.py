"""GPU timing of `autophase_each`: 65,536 spectra x 8192 bins, complex64, ACME -- one (p0, p1) search per spectrum.

Spectra: three to five Lorentzian lines per row with seeded positions, widths and amplitudes plus noise, each row
mis-phased by its own seeded (p0, p1) around its own maximum (made on the GPU from seeded FIDs).

Reports spectra/s of the device route (`search_rows` alone, and `autophase_each(engine="device")` end to end with
the polish of the flagged rows and the phase pass), of the host route (`engine="host"`: the native host search on
this process's CPUs) on the first --host-rows rows, and of the CPU oracle (scipy, one core) on the first
--oracle-rows rows; and the achieved GB/s (one read + one write) of `phase_apply_rows` beside `phase_apply` on the
same shape.  The kernel times of a separate `rocprofv3 --kernel-trace --stats` run (`--kernels-only`: one launch of
each kernel, nothing else) are merged in with --kernel-stats.

    python scripts/time_autophase_each.py --out profiles/autophase_each/time_autophase_each.json
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/time_autophase_each.py --kernels-only --rows 8192
    python scripts/time_autophase_each.py --out <json> --kernel-stats <..._kernel_stats.csv> --stats-csv <summary.csv>
"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

KERNELS = ("k_search_rows", "k_phase_rows", "k_phase<")


def make_spectra(rows, n, sw=5000.0, chunk=4096):
    """[rows, n] complex64 spectra on the GPU and their frequency axis (host)."""
    import torch

    g = torch.Generator(device="cuda").manual_seed(2025)
    freq = np.roll(np.fft.fftfreq(n, d=1 / sw), n // 2)
    t = torch.arange(n // 2, device="cuda", dtype=torch.float64) / sw
    fq = torch.from_numpy(freq).to("cuda")
    out = torch.empty((rows, n), dtype=torch.complex64, device="cuda")
    u = lambda lo, hi, *s: lo + (hi - lo) * torch.rand(s, generator=g, device="cuda", dtype=torch.float64)  # noqa: E731
    for lo in range(0, rows, chunk):
        m = min(chunk, rows - lo)
        fid = torch.zeros((m, n // 2), dtype=torch.complex128, device="cuda")
        for k in range(5):
            amp = u(0.3, 1.0, m, 1) * (1.0 if k < 3 else (u(0, 1, m, 1) < 0.5).double())
            fid += amp * torch.exp(-u(15.0, 60.0, m, 1) * t) * torch.exp(2j * np.pi * u(-2000, 2000, m, 1) * t)
        fid += 0.01 * torch.complex(torch.randn(fid.shape, generator=g, device="cuda", dtype=torch.float64),
                                    torch.randn(fid.shape, generator=g, device="cuda", dtype=torch.float64))
        spec = torch.fft.fftshift(torch.fft.fft(torch.nn.functional.pad(fid, (0, n - n // 2)), norm="ortho"), dim=-1)
        k = spec.abs().argmax(dim=1, keepdim=True)
        ang = torch.deg2rad(u(-150, 150, m, 1)) + torch.deg2rad(u(-600, 600, m, 1)) * (fq[None, :] - fq[k]) / (freq.max() - freq.min())
        out[lo:lo + m] = (spec * torch.exp(1j * ang)).to(torch.complex64)
    return out, freq


def merge_kernel_stats(a):
    rec = json.load(open(a.out)) if a.out and os.path.exists(a.out) else {}
    with open(a.kernel_stats) as fh:
        rows = [r for r in csv.DictReader(fh) if any(k in r.get("Name", "") for k in KERNELS)]
    rec["rocprofv3_kernel_stats"] = rows
    if a.stats_csv and rows:
        os.makedirs(os.path.dirname(os.path.abspath(a.stats_csv)), exist_ok=True)
        with open(a.stats_csv, "w", newline="") as fh:
            w = csv.DictWriter(fh, fieldnames=list(rows[0]))
            w.writeheader()
            w.writerows(rows)
    text = json.dumps(rec, indent=1)
    print(text)
    if a.out:
        open(a.out, "w").write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--bins", type=int, default=8192)
    ap.add_argument("--host-rows", type=int, default=None, help="rows of the host-route run (default: all)")
    ap.add_argument("--oracle-rows", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernels-only", action="store_true", help="one launch of each kernel (for a profiler run)")
    ap.add_argument("--kernel-stats", default=None, help="merge a rocprofv3 kernel_stats.csv into --out and exit")
    ap.add_argument("--stats-csv", default=None, help="with --kernel-stats: write the two kernels' rows here")
    a = ap.parse_args()
    if a.kernel_stats:
        return merge_kernel_stats(a)

    import torch

    import xmris_amd
    from xmris_amd import autophase_solver as aps
    from xmris_amd import device as dev

    x, freq = make_spectra(a.rows, a.bins)
    axis = dev.uniform_axis(freq)
    torch.cuda.synchronize()

    def timed(fn, repeats):
        out, times = None, []
        for _ in range(repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        return out, times

    recs, t_search = timed(lambda: dev.search_rows(x, axis), 1 if a.kernels_only else a.repeats)
    p0, p1 = recs["x"][:, 0], recs["x"][:, 1]
    pivot = freq[np.clip(recs["target_idx"], 0, a.bins - 1)]
    phase = {}
    for name, xt in (("complex64", x), ("complex128", x.to(torch.complex128))):
        table = aps.phase_table(freq, float(p0[0]), float(p1[0]), float(pivot[0]))
        nbytes = 2.0 * xt.numel() * xt.element_size()
        for _ in range(1 if a.kernels_only else 2):  # (the first pass also warms the caches of both)
            _, t_rows = timed(lambda: dev.phase_apply_rows(xt, 1, freq, p0, p1, pivot), 1)
            _, t_one = timed(lambda: dev.phase_apply(xt, 1, table), 1)
        phase[name] = {"phase_apply_rows_gbs": nbytes / t_rows[0] / 1e9, "phase_apply_gbs": nbytes / t_one[0] / 1e9,
                       "phase_apply_rows_ms": 1e3 * t_rows[0], "phase_apply_ms": 1e3 * t_one[0]}
        del xt
    if a.kernels_only:
        print(json.dumps({"search_rows_s": t_search, "phase": phase}))
        return

    la = xmris_amd.LabeledArray(x, ("voxel", "frequency"), {"frequency": freq})
    res, t_each = timed(lambda: la.xmr.autophase_each(engine="device"), 1)
    hr = a.rows if a.host_rows is None else min(a.host_rows, a.rows)
    lh = xmris_amd.LabeledArray(x[:hr], ("voxel", "frequency"), {"frequency": freq})
    res_h, t_host = timed(lambda: lh.xmr.autophase_each(engine="host"), 1)
    same = (np.array_equal(res.attrs["phase_p0"][:hr], res_h.attrs["phase_p0"]) and
            np.array_equal(res.attrs["phase_p1"][:hr], res_h.attrs["phase_p1"]))
    differ = int(np.count_nonzero((res.attrs["phase_p0"][:hr] != res_h.attrs["phase_p0"]) |
                                  (res.attrs["phase_p1"][:hr] != res_h.attrs["phase_p1"])))
    rec = {
        "workload": {"rows": a.rows, "bins": a.bins, "dtype": "complex64", "method": "acme"},
        "device": torch.cuda.get_device_name(0), "cpus": aps.burst_threads(),
        "search_rows_seconds": t_search, "search_rows_spectra_per_s": a.rows / float(np.median(t_search)),
        "nfev_mean": float(recs["nfev"].mean()), "nfev_max": int(recs["nfev"].max()),
        "needs_polish_rows": int(recs["needs_polish"].sum()),
        "status_counts": {str(s): int((recs["status"] == s).sum()) for s in range(4)},
        "device_route_seconds": t_each[0], "device_route_spectra_per_s": a.rows / t_each[0],
        "host_route_rows": hr, "host_route_seconds": t_host[0], "host_route_spectra_per_s": hr / t_host[0],
        "host_and_device_routes_equal": bool(same), "rows_that_differ": differ,
        "phase_pass": phase,
    }
    if a.oracle_rows > 0:
        import xmris_oracle as orc

        xh = x[:a.oracle_rows].cpu().numpy()
        t0 = time.perf_counter()
        worst = 0.0
        for r in range(a.oracle_rows):
            o = orc.autophase(orc.Labeled(xh[r], ("frequency",), {"frequency": orc.Coord("frequency", freq)}, {}, None))
            worst = max(worst, abs(o.attrs["phase_p0"] - res.attrs["phase_p0"][r]), abs(o.attrs["phase_p1"] - res.attrs["phase_p1"][r]))
        dt = time.perf_counter() - t0
        rec.update(oracle_rows=a.oracle_rows, oracle_one_core_spectra_per_s=a.oracle_rows / dt,
                   oracle_max_abs_dp_degrees=worst)
    text = json.dumps(rec, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
