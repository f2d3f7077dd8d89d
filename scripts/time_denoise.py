"""GPU timing of Marchenko-Pastur patch PCA denoising (xm_denoise_patches): 65,536 voxels x 2048 points, complex64, as
256 x 256 with 3 x 3 and 5 x 5 patches and as 32 x 32 x 64 with 3 x 3 x 3; seeded data made on the GPU (three
Gaussian-shaped amplitude maps times damped exponentials plus noise of sd 0.05).

Per workload: voxels/s of the matrix-core and the plain-FMA form (HIP events around the launch; one warm-up, median of
three), the stages from runs that end after the Gram matrix and after the eigen stage (gram, eig - gram, full - eig =
weights and apply pass), the algorithmic traffic 8 (P + 1) N bytes per voxel (every window row read once, y written)
as GB/s, and `combine_coils` "svd" with C = the nearest coil count on the same tensor viewed as (voxels / C, C, N): the
same Gram and eigen stages without the gather.  The one-core voxels/s of the numpy oracle (tests/_denoise_oracle.py)
over 64 voxels stands next to it.

    python scripts/time_denoise.py --out profiles/denoise/time_denoise.json
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

import _denoise_oracle as orc  # noqa: E402

WORKLOADS = {"256x256_p3x3": ((256, 256), (3, 3), 8), "256x256_p5x5": ((256, 256), (5, 5), 32),
             "32x32x64_p3x3x3": ((32, 32, 64), (3, 3, 3), 32)}  # grid, patch, coils of the coil-combination baseline


def make(grid, n, seed):
    import torch

    g = torch.Generator(device="cuda").manual_seed(seed)
    rn = lambda *s: torch.randn(s, generator=g, device="cuda", dtype=torch.float32)  # noqa: E731
    t = torch.arange(n, device="cuda", dtype=torch.float32) / n
    axes = torch.meshgrid(*(torch.arange(s, device="cuda", dtype=torch.float32) / s for s in grid), indexing="ij")
    x = torch.zeros(tuple(grid) + (n,), dtype=torch.complex64, device="cuda")
    for k, (f, d) in enumerate(((4.0, 2.0), (-7.0, 3.0), (11.0, 5.0))):
        m = torch.exp(-sum((a - 0.25 * (k + 1)) ** 2 for a in axes) / 0.1)
        x += m[..., None] * torch.exp(torch.complex(-d * t, 2 * np.pi * f * t))
    x += orc.NOISE_SD / np.sqrt(2.0) * torch.complex(rn(*x.shape), rn(*x.shape))
    return x.contiguous()


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
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--oracle-voxels", type=int, default=64)
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    from xmris_amd import device as dev

    n = a.points
    rec = {"device": torch.cuda.get_device_name(0), "points": n, "dtype": "complex64", "workloads": []}
    for name in a.workloads.split(","):
        grid, patch, coils = WORKLOADS[name]
        nv, p, d = int(np.prod(grid)), int(np.prod(patch)), len(grid)
        x = make(grid, n, seed=2024)
        work = torch.zeros(256, dtype=torch.uint8, device="cuda")
        w = {"name": name, "voxels": nv, "patch_voxels": p, "algorithmic_bytes_per_voxel": 8 * (p + 1) * n, "forms": {}}
        for label, kw in (("mfma", {}), ("fma", dict(_gram_fma=True)), ("mfma_stop_gram", dict(_stop="gram")),
                          ("mfma_stop_eig", dict(_stop="eig")), ("fma_stop_gram", dict(_gram_fma=True, _stop="gram"))):
            run = lambda: dev.denoise_patches(x, tuple(range(d)), d, patch, workspace=work, **kw)  # noqa: E731
            times, t_med, res = timed(run, a.warmup, a.repeats)
            f = {"seconds": times, "seconds_median": t_med, "voxels_per_s": nv / t_med, "kernel": dev.last_kernel()}
            if "stop" not in label:
                status, rank = res.status.cpu().numpy(), res.rank.cpu().numpy()
                f.update(algorithmic_gbs=8.0 * (p + 1) * n * nv / t_med / 1e9,
                         status_counts={str(s): int((status == s).sum()) for s in (0, 1, 2, 3)},
                         rank_counts={str(r): int((rank == r).sum()) for r in np.unique(rank)},
                         sigma_mean=float(res.sigma.mean().item()))
            w["forms"][label] = f
        m = {k: v["seconds_median"] for k, v in w["forms"].items()}
        w["split_seconds"] = {"gram (stop after it)": m["mfma_stop_gram"], "eigen stage and rank (eig - gram)": m["mfma_stop_eig"] - m["mfma_stop_gram"],
                              "weights and apply pass (full - eig)": m["mfma"] - m["mfma_stop_eig"],
                              "gram on plain FMAs (stop after it)": m["fma_stop_gram"]}
        xc = x.reshape(nv // coils, coils, n)
        times, t_med, _ = timed(lambda: dev.coil_combine(xc, 1, 2, method="svd", workspace=work), a.warmup, a.repeats)
        w["coil_combine_svd"] = {"coils": coils, "voxels": nv // coils, "seconds": times, "seconds_median": t_med,
                                 "seconds_per_window_at_this_rate": t_med / (nv // coils), "kernel": dev.last_kernel()}
        w["seconds_per_voxel"] = m["mfma"] / nv
        if a.oracle_voxels > 0:
            sub = tuple(min(s, 8) for s in grid)  # a corner of the grid holding at least 64 voxels
            xh = x[tuple(slice(0, s) for s in sub)].cpu().numpy().astype(np.complex128)
            win = list(orc.windows(sub, patch))[: a.oracle_voxels]
            t0 = time.perf_counter()
            for _, rows, c in win:
                orc.denoise_window(np.stack([xh[j] for j in rows]), c)
            w["oracle_one_core_voxels_per_s"] = len(win) / (time.perf_counter() - t0)
            w["speedup_vs_one_core_oracle"] = w["forms"]["mfma"]["voxels_per_s"] / w["oracle_one_core_voxels_per_s"]
        rec["workloads"].append(w)
        del x, xc
    text = json.dumps(rec, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
