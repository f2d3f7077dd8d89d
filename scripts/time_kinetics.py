"""GPU timing of the per-voxel rate fit (xm_kinetics_fit) on seeded synthetic series: a
gamma-variate substrate, products from ``simulate_kinetics`` at k in 0.01 ... 0.06 and rho in 1/40 ... 1/15, 1 % noise,
10 / 25 degree flip angles, unit weights:

  T30       65,536 voxels x 3 products x 30 repetitions (TR 2 s), k and rho fitted
  T30fixed  the same with rho fixed at its truth (the recurrence's coefficients are then constants of the fit)
  T64       16,384 voxels x 3 products x 64 repetitions, k and rho fitted: one repetition per lane
  T256      16,384 voxels x 3 products x 256 repetitions, k and rho fitted: four repetitions per lane

Per workload: seconds of ``device.kinetics_fit`` (HIP events around a few queued calls, divided by their number; warm-up,
median of the repeats), fits per second, the mean number of trial steps, seconds per wave and trial step, and the
status counts.  T64 against T256 separates the two candidate bounds: per trial step a wave runs the same two 64-lane
scans in both, but four times the exp / weight-series work in T256.

The scipy oracle (tests/_kinetics_oracle.fit_scipy, one core) is timed in the same run on the first `--oracle-items`
(voxel, product) pairs of T30 and T30fixed, and its parameters are compared with the kernel's on those pairs.

    python scripts/time_kinetics.py --out profiles/kinetics/time_kinetics.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# name -> (voxels, T, TR seconds, rho free)
WORKLOADS = {"T30": (65536, 30, 2.0, True), "T30fixed": (65536, 30, 2.0, False), "T64": (16384, 64, 1.0, True),
             "T256": (16384, 256, 0.25, True)}
M = 3
INNER = 5


def make(nv, T, tr, seed=2024):
    from xmris_amd import simulate_kinetics

    rng = np.random.default_rng(seed)
    t = tr * np.arange(T)
    tt = (t + 2.0) / 8.0
    mag = 100.0 * tt ** 2 * np.exp(2.0 * (1.0 - tt))
    S = rng.uniform(0.5, 2.0, (nv, 1)) * mag * np.sin(np.deg2rad(10.0))
    k, rho = rng.uniform(0.01, 0.06, (nv, M)), rng.uniform(1 / 40, 1 / 15, (nv, M))
    Y = simulate_kinetics(np.broadcast_to(S[:, None, :], (nv, M, T)), t, k, rho, flip_angle=(10.0, 25.0))
    Y = Y + 0.01 * np.abs(Y).max(axis=-1, keepdims=True) * rng.standard_normal(Y.shape)
    S = S + 0.01 * np.abs(S).max(axis=-1, keepdims=True) * rng.standard_normal(S.shape)
    return t, S, Y, k, rho


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--oracle-items", type=int, default=48)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    import _kinetics_oracle as orc
    from xmris_amd import device as dev

    rec = {"device": torch.cuda.get_device_name(0), "repeats": a.repeats, "calls_per_timing": INNER, "products": M,
           "workloads": []}
    for name in a.workloads.split(","):
        nv, T, tr, rho_free = WORKLOADS[name]
        t, S, Y, k, rho = make(nv, T, tr)
        ths, thp = np.full(T, np.deg2rad(10.0)), np.full((M, T), np.deg2rad(25.0))
        # every voxel shares the bounds, so a fixed rho is one value per product: the truth's mean
        init, lo, hi, fixed = orc.parameters(M, rho_free=rho_free, rho_fixed=rho.mean(axis=0))
        Sd, Yd = torch.from_numpy(S).to("cuda"), torch.from_numpy(Y).to("cuda")
        run = lambda: dev.kinetics_fit(Sd, Yd, t, ths, thp, init, lo, hi, fixed)  # noqa: E731
        for _ in range(a.warmup):
            res = run()
        torch.cuda.synchronize()
        times = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(INNER):
                res = run()
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1) / 1e3 / INNER)
        kernel = dev.last_kernel()
        sec = float(np.median(times))
        status, iters = res.status.cpu().numpy(), res.iters.cpu().numpy()
        params = res.params.cpu().numpy()
        w = {"name": name, "voxels": nv, "repetitions": T, "rho_free": rho_free, "kernel": kernel, "seconds": times,
             "seconds_median": sec, "fits_per_second": nv * M / sec, "mean_trial_steps": float(iters.mean()),
             "max_trial_steps": int(iters.max()),
             "seconds_per_wave_and_trial_step": sec / float(iters.sum()),
             "status_counts": {str(s): int(np.count_nonzero(status == s)) for s in range(4)},
             "median_abs_rate_error": float(np.median(np.abs(params[..., 0] - k)))}
        if name in ("T30", "T30fixed") and a.oracle_items > 0:
            c = {"S": S, "Y": Y, "w": None, "t": t, "ths": ths, "thp": thp, "init": init, "lo": lo, "hi": hi, "fixed": fixed}
            pairs = [(i // M, i % M) for i in range(a.oracle_items)]
            t0 = time.perf_counter()
            refs = [orc.fit_scipy(orc.item(c, v, m)) for v, m in pairs]
            dt = (time.perf_counter() - t0) / len(pairs)
            dev_sd = [float(np.max(np.abs(params[v, m] - o["params"])[o["sd"] > 0] / o["sd"][o["sd"] > 0]))
                      for (v, m), o in zip(pairs, refs) if o["success"]]
            w.update({"oracle_items": len(pairs), "oracle_seconds_per_fit_one_core": dt,
                      "oracle_seconds_for_all_fits_extrapolated": dt * nv * M,
                      "speedup_over_oracle_one_core": dt * nv * M / sec,
                      "largest_parameter_difference_in_sd": max(dev_sd), "oracle_converged": len(dev_sd)})
        rec["workloads"].append(w)
        del Sd, Yd, res
        torch.cuda.empty_cache()
    by = {w["name"]: w for w in rec["workloads"]}
    if "T64" in by and "T256" in by:
        rec["trial_step_time_T256_over_T64"] = (by["T256"]["seconds_per_wave_and_trial_step"] /
                                                by["T64"]["seconds_per_wave_and_trial_step"])
    text = json.dumps(rec, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
