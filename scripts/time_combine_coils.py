"""GPU timing of coil combination (xm_coil_combine): 65,536 voxels x 16 coils x 2048 points, complex64, and 16,384
voxels x 32 coils; seeded data made on the GPU (per-voxel random sensitivities times a two-peak damped FID plus noise).

Per workload and method (svd, svd_fma, first_point, and svd / first_point with a noise covariance): voxels/s (HIP events around the launch; warm-up, median of
repeats), the algorithmic traffic 8 (C + 1) N bytes per voxel as GB/s and as a fraction of the device-copy ceiling of
profiles/r02/stream_ceiling.txt, and the kernel's own split: first_point runs neither the Gram matrix nor the Jacobi
iteration, so svd - first_point is what those two cost and svd - svd_fma what the matrix cores change.  The one-core
voxels/s of the numpy oracle (tests/_coils_oracle.py) over 64 voxels stands next to it.

    python scripts/time_combine_coils.py --out profiles/coils/time_combine_coils.json
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

import _coils_oracle as orc  # noqa: E402


def copy_ceiling_gbs():
    """The 1:1 device copy (median, read + write bytes per second) recorded in profiles/r02/stream_ceiling.txt."""
    path = os.path.join(ROOT, "profiles", "r02", "stream_ceiling.txt")
    for line in open(path):
        m = re.search(r"([0-9]+(?:\.[0-9]+)?)\s*GB/s", line)
        if line.startswith("copy11") and m:
            return float(m.group(1))
    return 0.0


def make(nv, c, n, seed):
    import torch

    g = torch.Generator(device="cuda").manual_seed(seed)
    rn = lambda *s: torch.randn(s, generator=g, device="cuda", dtype=torch.float32)  # noqa: E731
    t = torch.arange(n, device="cuda", dtype=torch.float32) / n
    fid = torch.exp(torch.complex(-2.0 * t, 2 * np.pi * 4.0 * t)) + 0.6 * torch.exp(torch.complex(-3.0 * t, -2 * np.pi * 7.0 * t))
    sens = torch.complex(rn(nv, c, 1), rn(nv, c, 1))
    x = sens * fid + 0.3 * torch.complex(rn(nv, c, n), rn(nv, c, n))
    return x.to(torch.complex64).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--oracle-voxels", type=int, default=64)
    ap.add_argument("--workloads", default="65536x16,16384x32", help="voxels x coils, comma separated")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    from xmris_amd import device as dev

    ceiling = copy_ceiling_gbs()
    n = a.points
    rec = {"device": torch.cuda.get_device_name(0), "points": n, "dtype": "complex64",
           "copy_ceiling_gbs": ceiling, "workloads": []}
    for spec in a.workloads.split(","):
        nv, c = (int(v) for v in spec.split("x"))
        x = make(nv, c, n, seed=2024)
        work = torch.zeros(256, dtype=torch.uint8, device="cuda")
        w = {"voxels": nv, "coils": c, "algorithmic_bytes_per_voxel": 8 * (c + 1) * n, "methods": {}}
        linv = orc.linv_of(orc.random_psd(c, 7))
        # "svd+reference_copy": the weights from a copy of x in other memory, so that pass 2 reads X for the first
        # time -- against plain "svd", where pass 2 reads what pass 1 has just read, it shows what the caches give
        xcopy = x.clone()
        for label in ("svd", "svd_fma", "first_point", "svd+noise_cov", "first_point+noise_cov", "svd+reference_copy"):
            method, white = label.split("+")[0], label.endswith("noise_cov")
            ref = xcopy if label.endswith("reference_copy") else None
            run = lambda: dev.coil_combine(x, 1, 2, method=method, workspace=work, linv=linv if white else None,  # noqa: E731
                                           reference=ref)
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
            t_med = float(np.median(times))
            status = res.status.cpu().numpy()
            gbs = 8.0 * (c + 1) * n * nv / t_med / 1e9
            w["methods"][label] = {
                "seconds": times, "seconds_median": t_med, "voxels_per_s": nv / t_med, "algorithmic_gbs": gbs,
                "fraction_of_copy_ceiling": gbs / ceiling if ceiling else None, "kernel": dev.last_kernel(),
                "status_counts": {str(s): int((status == s).sum()) for s in (0, 1, 2, 3)},
                "quality_mean": float(res.quality.mean().item())}
        m = w["methods"]
        w["split_seconds"] = {"apply_and_reductions (first_point)": m["first_point"]["seconds_median"],
                              "gram_and_jacobi (svd - first_point)": m["svd"]["seconds_median"] - m["first_point"]["seconds_median"],
                              "matrix_cores_against_fma (svd_fma - svd)": m["svd_fma"]["seconds_median"] - m["svd"]["seconds_median"]}
        if a.oracle_voxels > 0:
            xh = x[: a.oracle_voxels].cpu().numpy().astype(np.complex128)
            t0 = time.perf_counter()
            for v in range(a.oracle_voxels):
                orc.combine(xh[v])
            w["oracle_one_core_voxels_per_s"] = a.oracle_voxels / (time.perf_counter() - t0)
            w["speedup_vs_one_core_oracle"] = m["svd"]["voxels_per_s"] / w["oracle_one_core_voxels_per_s"]
        rec["workloads"].append(w)
        del x, xcopy
    text = json.dumps(rec, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
