"""GPU timing of HSVD water removal (xm_hsvd_rows): complex64, 2048 points, n_cols = 64, rank = 20, band +-50 Hz at
dt = 2e-4 s; 65,536 and 4,096 voxels.  Seeded data made on the GPU (three metabolite peaks, three water-band components
at 6 ... 40 times the largest peak, complex noise -- the generator of tests/_hsvd_oracle.py, per voxel).

Per workload: voxels/s (HIP events around the launch; one warm-up, median of 3) with the Gram matrix on the fp64 matrix
cores and on plain FMAs, and the split between the stages from runs that end every voxel after the Gram matrix, the
Jacobi iteration, the poles and the amplitudes (the timing-only `_stop` of device.hsvd_rows): every stage as what it
adds to the run that ends before it.  The one-core voxels/s of the numpy oracle (route eigh) over 16 rows stands next to it.

    timeout 600 python scripts/time_remove_water.py --out profiles/hsvd/time_remove_water.json
"""
import os

os.environ.setdefault("OMP_NUM_THREADS", "1")  # the oracle's one-core figure: no BLAS threads
os.environ.setdefault("OPENBLAS_NUM_THREADS", "1")
os.environ.setdefault("MKL_NUM_THREADS", "1")

import argparse  # noqa: E402
import json  # noqa: E402
import sys  # noqa: E402
import time  # noqa: E402

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _hsvd_oracle as orc  # noqa: E402

DT, BAND = orc.DT, orc.BAND


def make(nv, n, seed):
    import torch

    g = torch.Generator(device="cuda").manual_seed(seed)
    un = lambda lo, hi: lo + (hi - lo) * torch.rand((nv, 1), generator=g, device="cuda", dtype=torch.float32)  # noqa: E731
    t = torch.arange(n, device="cuda", dtype=torch.float32) * DT
    x = 0.02 * torch.complex(torch.randn((nv, n), generator=g, device="cuda"), torch.randn((nv, n), generator=g, device="cuda"))
    for f0, a_lo, a_hi, d_lo, d_hi, jit in ((260.0, 1.0, 1.0, 15.0, 40.0, 20.0), (430.0, 0.4, 0.9, 15.0, 40.0, 20.0),
                                            (640.0, 0.4, 0.9, 15.0, 40.0, 20.0), (-11.0, 6.0, 40.0, 20.0, 60.0, 3.0),
                                            (1.0, 6.0, 40.0, 20.0, 60.0, 3.0), (12.0, 6.0, 40.0, 20.0, 60.0, 3.0)):
        f, a, d, p = f0 + un(-jit, jit), un(a_lo, a_hi), un(d_lo, d_hi), un(-np.pi, np.pi)
        x = x + a * torch.exp(torch.complex(-d * t, 2 * np.pi * f * t + p))
    return x.to(torch.complex64).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--n-cols", type=int, default=64)
    ap.add_argument("--rank", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--oracle-rows", type=int, default=16)
    ap.add_argument("--workloads", default="65536,4096", help="voxels, comma separated")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    from xmris_amd import device as dev

    n, m, k = a.points, a.n_cols, a.rank
    rec = {"device": torch.cuda.get_device_name(0), "points": n, "n_cols": m, "rank": k, "dt": DT, "band": BAND,
           "dtype": "complex64", "gram_mflop_per_voxel": 8 * (n - m + 1) * (m * (m + 1) // 2) / 1e6, "workloads": []}
    for spec in a.workloads.split(","):
        nv = int(spec)
        x = make(nv, n, seed=2024)
        work = torch.zeros(256, dtype=torch.uint8, device="cuda")
        runs = {}
        for label, kw in (("all", {}), ("all_fma_gram", dict(_gram_fma=True)), ("to_gram", dict(_stop="gram")),
                          ("to_gram_fma", dict(_stop="gram", _gram_fma=True)), ("to_eig", dict(_stop="eig")),
                          ("to_poles", dict(_stop="poles")), ("to_ampl", dict(_stop="ampl"))):
            run = lambda: dev.hsvd_rows(x, 1, m, k, DT, BAND, workspace=work, **kw)  # noqa: E731
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
            if label.startswith("all"):
                status = res.status.cpu().numpy()
                runs[label].update({"voxels_per_s": nv / runs[label]["seconds_median"], "kernel": dev.last_kernel(),
                                    "status_counts": {str(s): int((status == s).sum()) for s in range(5)},
                                    "n_removed_mean": float(res.n_removed.double().mean().item())})
        med = lambda key: runs[key]["seconds_median"]  # noqa: E731
        runs["split_seconds"] = {"gram_with_launch_and_hand_out": med("to_gram"), "jacobi": med("to_eig") - med("to_gram"),
                                 "shift_matrix_and_poles": med("to_poles") - med("to_eig"),
                                 "amplitudes": med("to_ampl") - med("to_poles"), "subtract": med("all") - med("to_ampl")}
        runs["gram_seconds"] = {"mfma": med("to_gram"), "fma": med("to_gram_fma")}
        w = {"voxels": nv, "runs": runs}
        if a.oracle_rows > 0:
            xh = x[:a.oracle_rows].cpu().numpy().astype(np.complex128)
            t0 = time.perf_counter()
            for row in xh:
                orc.hsvd(row, m, k, DT, BAND)
            w["oracle_one_core_voxels_per_s"] = len(xh) / (time.perf_counter() - t0)
            w["speedup_vs_one_core_oracle"] = runs["all"]["voxels_per_s"] / w["oracle_one_core_voxels_per_s"]
        rec["workloads"].append(w)
        del x
    text = json.dumps(rec, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
