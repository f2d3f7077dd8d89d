"""GPU timing of AMARES quantification (xm_amares_fit): 65,536 voxels x 2048 points, five 31P-like peaks (PCr, Pi,
gamma-, alpha-, beta-ATP), complex64 input, seeded per-voxel truth (tests/_amares_oracle.py::p31_workload's prior
knowledge and truth ranges; the FIDs are made on the GPU by xm_amares_model plus seeded noise).

Reports voxels/s (HIP events around the fit launch; warm-up, median of repeats), mean / max iterations, the achieved
fp64 rate from the FLOP count below, and the one-core voxels/s of the CPU oracle (scipy MINPACK) over 64 voxels.
The kernel time of a separate `rocprofv3 --kernel-trace --stats` run is merged in with --kernel-stats.

    python scripts/time_amares.py --out profiles/amares/time_amares.json [--kernel-stats <..._kernel_stats.csv>]

--linked / --nine-unlinked: the 9-line model instead (PCr, Pi, gamma-ATP x 2, alpha-ATP x 2, beta-ATP x 3; multiplet
amplitudes, shifts (-J, -2J in Hz), linewidths and phases linked to the first line of each multiplet, g fixed: 45
parameters, 20 free columns), respectively the same nine peaks with only g fixed (36 free columns), on the same seeded
linked truth (tests/_amares_links.py::multiplet_pk).
"""
import os

os.environ.setdefault("OMP_NUM_THREADS", "1")  # the oracle's one-core figure: no BLAS threads
os.environ.setdefault("OPENBLAS_NUM_THREADS", "1")
os.environ.setdefault("MKL_NUM_THREADS", "1")

import argparse  # noqa: E402
import csv  # noqa: E402
import json  # noqa: E402
import sys  # noqa: E402
import time  # noqa: E402

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _amares_links as lk  # noqa: E402
import _amares_oracle as orc  # noqa: E402


def flops_per_voxel(n: int, k: int, p: int, iters: int) -> float:
    """fp64 FLOPs of one voxel's fit, counted from the shapes (an upper estimate: every trial is charged one Jacobian,
    while a rejected trial reuses the last one).  Per trial:
      normal equations  2n residual rows x ((p+1)(p+2)/2 - 1) entries of [J | r]^T [J | r], one FMA (2 FLOPs) each;
      model terms       3 passes (Jacobian rows, trial cost) x n points x k peaks x 40 FLOPs -- exp and sincos counted
                        as 10 each, the term, its five derivative columns and the residual as the rest;
      Cholesky          p^3 / 3 FLOPs, two triangular solves 2 p^2.
    Plus the CRLB pass (one more normal-equation pass and factorisation) and the fit_data pass."""
    entries = (p + 1) * (p + 2) // 2 - 1
    normal = 2.0 * (2 * n) * entries
    terms = 3.0 * n * k * 40.0
    solve = p ** 3 / 3.0 + 2.0 * p * p
    return iters * (normal + terms + solve) + normal + p ** 3 / 3.0 + n * k * 40.0


def kernel_stats(path):
    """Rows of a rocprofv3 kernel_stats.csv whose name mentions k_amares."""
    out = []
    with open(path) as fh:
        for r in csv.DictReader(fh):
            if "k_amares" in r.get("Name", ""):
                out.append({k: r[k] for k in r})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxels", type=int, default=65536)
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--oracle-voxels", type=int, default=64)
    ap.add_argument("--out", default=None)
    ap.add_argument("--linked", action="store_true", help="the 9-line multiplet workload with its links")
    ap.add_argument("--nine-unlinked", action="store_true", help="the same nine peaks, every line on its own")
    ap.add_argument("--kernel-stats", default=None, help="merge a rocprofv3 kernel_stats.csv into --out and exit")
    a = ap.parse_args()

    if a.kernel_stats:
        rec = json.load(open(a.out)) if a.out and os.path.exists(a.out) else {}
        rows = kernel_stats(a.kernel_stats)
        rec["rocprofv3_kernel_stats"] = rows
        fit = [r for r in rows if "k_amares_fit" in r.get("Name", "")]
        if fit and "flop_per_fit" in rec:
            avg_ns = float(fit[0]["AverageNs"])
            rec["kernel_avg_ms"] = avg_ns / 1e6
            rec["kernel_fp64_tflops"] = rec["flop_per_fit"] / (avg_ns * 1e-9) / 1e12
        text = json.dumps(rec, indent=1)
        print(text)
        if a.out:
            open(a.out, "w").write(text + "\n")
        return

    import torch

    from xmris_amd import device as dev

    mhz, sw, n, nv = 120.0, 10000.0, a.points, a.voxels
    rng = np.random.default_rng(2024)
    nine = a.linked or a.nine_unlinked
    links = None
    if nine:
        init, lo, hi, fixed, links = lk.multiplet_pk(mhz)
        E, b, roots = lk.expansion(links, 9)
        truth = np.broadcast_to(init, (nv, 9, 5)).copy()
        truth[:, :, 0] *= rng.uniform(0.6, 1.4, (nv, 9))
        truth[:, :, 1] += rng.uniform(-0.15, 0.15, (nv, 9)) * mhz
        truth[:, :, 2] *= rng.uniform(0.8, 1.2, (nv, 9))
        truth[:, :, 3] = rng.uniform(-0.3, 0.3, (nv, 1))
        truth = (truth.reshape(nv, 45)[:, roots] @ E.T + b).reshape(nv, 9, 5)  # the followers obey their links
        if a.nine_unlinked:  # every line free within +-0.4 ppm, 4 ... 60 Hz, +-180 deg of its own; g still fixed
            to = links[0] >= 0
            lo[to[:, 0], 0], hi[to[:, 0], 0] = 0.0, np.inf
            lo[to[:, 1], 1], hi[to[:, 1], 1] = init[to[:, 1], 1] - 0.4 * mhz, init[to[:, 1], 1] + 0.4 * mhz
            lo[to[:, 2], 2], hi[to[:, 2], 2] = 4 * np.pi, 60 * np.pi
            lo[to[:, 3], 3], hi[to[:, 3], 3] = -np.pi, np.pi
            links = None
    else:
        truth = np.zeros((nv, 5, 5))
        truth[:, :, 0] = np.array(orc.P31_AMP) * rng.uniform(0.6, 1.4, (nv, 5))
        truth[:, :, 1] = (np.array(orc.P31_PPM) + rng.uniform(-0.15, 0.15, (nv, 5))) * mhz
        truth[:, :, 2] = np.array(orc.P31_LW) * rng.uniform(0.8, 1.2, (nv, 5)) * np.pi
        truth[:, :, 3] = rng.uniform(-0.3, 0.3, (nv, 1))
    x = dev.amares_model(torch.from_numpy(truth).to("cuda"), n, 1.0 / sw, 0.0)
    g = torch.Generator(device="cuda").manual_seed(2024)
    x = (x + 0.5 * torch.complex(torch.randn(x.shape, generator=g, device="cuda", dtype=torch.float64),
                                 torch.randn(x.shape, generator=g, device="cuda", dtype=torch.float64)))
    x = x.to(torch.complex64).contiguous()
    if not nine:
        init, lo, hi = orc.p31_pk(mhz)
        fixed = np.zeros((5, 5), bool)
    n_peaks = init.shape[0]

    def run():
        if links is None:
            return dev.amares_fit(x, 1, init, lo, hi, fixed, dt=1.0 / sw, want_fit=False)
        return dev.amares_fit(x, 1, init, lo, hi, fixed, dt=1.0 / sw, want_fit=False, links=links)

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
    iters = res.iters.cpu().numpy()
    status = res.status.cpu().numpy()
    amp = res.params.cpu().numpy()[:, :, 0]
    # five peaks x (a, f, d, phi, g): g starts on its bound and is held there by its zero slope; nine peaks: g is fixed
    p_free = res.n_free if nine else 25
    flop = float(sum(flops_per_voxel(n, n_peaks, p_free, int(i)) for i in iters))
    rec = {
        "workload": {"voxels": nv, "points": n, "peaks": n_peaks, "free_parameters": p_free, "dtype": "complex64",
                     "sw_hz": sw, "mhz": mhz,
                     "model": "linked multiplets" if a.linked else "nine unlinked" if nine else "five singlets"},
        "fit_seconds": times, "fit_seconds_median": t_med, "voxels_per_s": nv / t_med,
        "iterations_mean": float(iters.mean()), "iterations_max": int(iters.max()),
        "status_counts": {str(s): int((status == s).sum()) for s in (0, 1, 2)},
        "amplitude_rel_err_median": float(np.median(np.abs(amp / truth[:, :, 0] - 1))),
        "flop_per_fit": flop, "fp64_tflops_achieved": flop / t_med / 1e12,
        "device": torch.cuda.get_device_name(0), "kernel": dev.last_kernel(),
    }
    if a.oracle_voxels > 0 and not nine:
        xh = x[: a.oracle_voxels].cpu().numpy().astype(np.complex128)
        t = np.arange(n) / sw
        t0 = time.perf_counter()
        for v in range(a.oracle_voxels):
            orc.fit(xh[v], t, init, lo, hi, xtol=1e-10, ftol=1e-10)
        dt = time.perf_counter() - t0
        rec["oracle_one_core_voxels_per_s"] = a.oracle_voxels / dt
        rec["speedup_vs_one_core_oracle"] = rec["voxels_per_s"] / rec["oracle_one_core_voxels_per_s"]
    text = json.dumps(rec, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
