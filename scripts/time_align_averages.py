"""GPU timing of the alignment of repeated transients (xm_align_rows): complex64, 2048 points, the fit on the leading
1024, max_shift 20 Hz at dt = 2e-4 s; 4096 voxels x 64 averages and 1 voxel x 256 averages, each in the per-transient
and in the averaging form.  Seeded data made on the GPU (a two-peak damped FID per voxel, every transient shifted, turned
and with noise).

Per workload and form: transients/s (HIP events around the launch; one warm-up, median of 3), the algorithmic traffic --
8 N bytes in and 8 N out per transient plus the reference once per voxel; in the averaging form the output once per
voxel -- as GB/s and as a fraction of the device-copy ceiling of profiles/r02/stream_ceiling.txt, and the split between
the stages from runs with stages left out (the test-only `_skip` of device.align_rows): refine and apply as what
leaving them out saves, the coarse stage as what it adds to staging alone -- leaving only the coarse stage out would send
the refine stage looking from the wrong bracket, which takes longer than the coarse stage itself.  The one-core
transients/s of the numpy oracle (tests/_align_oracle.py) over 64 transients stands next to it.

    timeout 600 python scripts/time_align_averages.py --out profiles/align/time_align_averages.json
"""
import os

os.environ.setdefault("OMP_NUM_THREADS", "1")  # the oracle's one-core figure: no BLAS threads
os.environ.setdefault("OPENBLAS_NUM_THREADS", "1")
os.environ.setdefault("MKL_NUM_THREADS", "1")

import argparse  # noqa: E402
import json  # noqa: E402
import re  # noqa: E402
import sys  # noqa: E402
import time  # noqa: E402

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _align_oracle as orc  # noqa: E402

DT, MAX_SHIFT = 2e-4, 20.0


def copy_ceiling_gbs():
    """The 1:1 device copy (median, read + write bytes per second) recorded in profiles/r02/stream_ceiling.txt."""
    path = os.path.join(ROOT, "profiles", "r02", "stream_ceiling.txt")
    for line in open(path):
        m = re.search(r"([0-9]+(?:\.[0-9]+)?)\s*GB/s", line)
        if line.startswith("copy11") and m:
            return float(m.group(1))
    return 0.0


def make(nv, a, n, seed):
    import torch

    g = torch.Generator(device="cuda").manual_seed(seed)
    rn = lambda *s: torch.randn(s, generator=g, device="cuda", dtype=torch.float32)  # noqa: E731
    un = lambda *s: torch.rand(s, generator=g, device="cuda", dtype=torch.float32)  # noqa: E731
    t = torch.arange(n, device="cuda", dtype=torch.float32) * DT
    fid = torch.exp(torch.complex(-8.0 * t, 2 * np.pi * 31.0 * t)) + 0.6 * torch.exp(torch.complex(-12.0 * t, -2 * np.pi * 57.0 * t))
    f = (un(nv, a, 1) - 0.5) * 1.2 * MAX_SHIFT
    p = (un(nv, a, 1) - 0.5) * 2 * np.pi
    x = fid * torch.exp(torch.complex(torch.zeros_like(f * t), 2 * np.pi * f * t + p)) + 0.2 * torch.complex(rn(nv, a, n), rn(nv, a, n))
    return x.to(torch.complex64).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--fit-points", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--oracle-transients", type=int, default=64)
    ap.add_argument("--workloads", default="4096x64,1x256", help="voxels x averages, comma separated")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    from xmris_amd import device as dev

    ceiling = copy_ceiling_gbs()
    n, L = a.points, a.fit_points
    rec = {"device": torch.cuda.get_device_name(0), "points": n, "fit_points": L, "dt": DT, "max_shift": MAX_SHIFT,
           "grid": dev.align_grid(L, DT, MAX_SHIFT), "dtype": "complex64", "copy_ceiling_gbs": ceiling, "workloads": []}
    for spec in a.workloads.split(","):
        nv, na = (int(v) for v in spec.split("x"))
        x = make(nv, na, n, seed=2024)
        ref = x.mean(dim=1)
        work = torch.zeros(256, dtype=torch.uint8, device="cuda")
        w = {"voxels": nv, "averages": na, "forms": {}}
        for form in ("each", "average"):
            avg = form == "average"
            nbytes = 8 * n * nv * na + 8 * n * nv + (8 * n * nv if avg else 8 * n * nv * na)
            runs = {}
            for label, skip in (("all", ()), ("no_refine", ("refine",)), ("no_apply", ("apply",)),
                                ("staging_and_coarse", ("refine", "apply")), ("staging_only", ("coarse", "refine", "apply"))):
                run = lambda: dev.align_rows(x, 1, 2, ref, n_points=L, dt=DT, max_shift=MAX_SHIFT, average=avg,  # noqa: E731
                                             want_y=not avg, workspace=work, _skip=skip)
                for _ in range(a.warmup):
                    run()
                torch.cuda.synchronize()
                times, res = [], None
                for _ in range(a.repeats):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    res = run()
                    e1.record()
                    e1.synchronize()
                    times.append(e0.elapsed_time(e1) / 1e3)
                runs[label] = {"seconds": times, "seconds_median": float(np.median(times))}
                if label == "all":
                    status = res.status.cpu().numpy()
                    t_med = runs[label]["seconds_median"]
                    runs[label].update({
                        "transients_per_s": nv * na / t_med, "algorithmic_bytes": nbytes, "algorithmic_gbs": nbytes / t_med / 1e9,
                        "fraction_of_copy_ceiling": nbytes / t_med / 1e9 / ceiling if ceiling else None,
                        "kernel": dev.last_kernel(), "status_counts": {str(s): int((status == s).sum()) for s in range(5)},
                        "quality_mean": float(res.quality.mean().item())})
            t_all = runs["all"]["seconds_median"]
            runs["split_seconds"] = {k: t_all - runs["no_" + k]["seconds_median"] for k in ("refine", "apply")}
            runs["split_seconds"]["coarse"] = runs["staging_and_coarse"]["seconds_median"] - runs["staging_only"]["seconds_median"]
            runs["split_seconds"]["staging_and_rest"] = runs["staging_only"]["seconds_median"]
            w["forms"][form] = runs
        if a.oracle_transients > 0:
            k = min(a.oracle_transients, na)
            xh = x[0, :k].cpu().numpy().astype(np.complex128)
            rh = ref[0].cpu().numpy().astype(np.complex128)
            t0 = time.perf_counter()
            for v in range(k):
                orc.align(xh[v], rh, DT, 0.0, MAX_SHIFT, L)
            w["oracle_one_core_transients_per_s"] = k / (time.perf_counter() - t0)
            w["speedup_vs_one_core_oracle"] = w["forms"]["each"]["all"]["transients_per_s"] / w["oracle_one_core_transients_per_s"]
        rec["workloads"].append(w)
        del x, ref
    text = json.dumps(rec, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
