"""GPU timing of basis-set quantification (xm_basis_fit): 65,536 voxels x 2048 points, complex64 input, a basis of 16
metabolites in 2 groups made from multiplets by simulate_fid, Voigt lineshape (16 amplitudes + 2 x (shift, Lorentzian,
Gaussian) + phase = 23 free columns), seeded per-voxel truth (the FIDs are made on the GPU by xm_basis_model plus
seeded noise).

Reports seconds and voxels/s (HIP events around the fit launch; warm-up, median of repeats), mean / max trials, the
converged share, the achieved fp64 rate from the FLOP count below, and the one-core voxels/s of the CPU oracle
(tests/_basis_oracle.py: scipy MINPACK with the analytic Jacobian) over 64 of the voxels.

    python scripts/time_basis.py --out profiles/basis/time_fit_basis.json
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

import _basis_oracle as orc  # noqa: E402

FLOP_FORMULA = ("per trial: normal equations 2 * (2 nf) * ((P+1)(P+2)/2 - 1) [one FMA per entry and residual row]"
                " + model terms 3 * nf * (G * 30 + M * 14) [Jacobian rows and the trial cost; exp and sincos 10 each per"
                " group, 14 per metabolite for E B, its column and the sums] + Cholesky P^3/3 + 2 P^2;"
                " plus once: the start (nf * 4 + cost), the CRLB pass (normal equations + P^3/3) and nothing for"
                " fit_data (not requested); nf = points - skip")


def flops_per_voxel(nf: int, m: int, g: int, p: int, iters: int) -> float:
    """fp64 FLOPs of one voxel's fit, counted from the shapes as FLOP_FORMULA states (an upper estimate: every trial is
    charged one Jacobian, while a rejected trial reuses the last one)."""
    entries = (p + 1) * (p + 2) // 2 - 1
    normal = 2.0 * (2 * nf) * entries
    terms = nf * (g * 30.0 + m * 14.0)
    solve = p ** 3 / 3.0 + 2.0 * p * p
    return iters * (normal + 3.0 * terms + solve) + (4.0 * nf + terms) + normal + p ** 3 / 3.0


def make_basis(n, sw, rng):
    """16 multiplet FIDs by simulate_fid: 1 ... 4 lines each around centres spread over +-35 % of the spectral width."""
    import xmris_amd as xm

    names, rows = [], []
    for m in range(16):
        k = 1 + m % 4
        centre = (-0.35 + 0.7 * m / 15.0) * sw
        w = rng.uniform(0.5, 1.5, k)
        fid = xm.simulate_fid(w / w.sum(), frequencies=centre + 7.0 * (np.arange(k) - (k - 1) / 2.0),
                              spectral_width=sw, n_points=n, dampings=rng.uniform(6.0, 14.0, k))
        rows.append(np.asarray(fid.values))
        names.append(f"met{m:02d}")
    return np.stack(rows), names


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxels", type=int, default=65536)
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--oracle-voxels", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    from xmris_amd import device as dev
    from xmris_amd.fitting.basis import basis_parameters, gaussian_damping

    sw, n, nv, M, G = 4000.0, a.points, a.voxels, 16, 2
    dt = 1.0 / sw
    rng = np.random.default_rng(2025)
    B, names = make_basis(n, sw, rng)
    group = (np.arange(M) % G).astype(np.int32)
    truth = np.zeros((nv, M + 3 * G + 1))
    truth[:, :M] = rng.uniform(0.5, 2.0, (nv, M))
    truth[:, M:M + G] = rng.uniform(-4.0, 4.0, (nv, G))
    truth[:, M + G:M + 2 * G] = np.pi * rng.uniform(1.0, 5.0, (nv, G))
    truth[:, M + 2 * G:M + 3 * G] = gaussian_damping(rng.uniform(1.0, 5.0, (nv, G)))
    truth[:, -1] = rng.uniform(-0.4, 0.4, nv)
    bd = torch.from_numpy(B).to("cuda")
    x = dev.basis_model(torch.from_numpy(truth).to("cuda"), bd, group, dt)
    g = torch.Generator(device="cuda").manual_seed(2025)
    x = (x + 0.02 * torch.complex(torch.randn(x.shape, generator=g, device="cuda", dtype=torch.float64),
                                  torch.randn(x.shape, generator=g, device="cuda", dtype=torch.float64)))
    x = x.to(torch.complex64).contiguous()
    init, lo, hi, fixed = basis_parameters(M, G, "voigt")

    def run():
        return dev.basis_fit(x, 1, bd, group, init, lo, hi, fixed, dt=dt, want_fit=False)

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
    amp = res.params.cpu().numpy()[:, :M]
    p_free = res.n_free
    flop = float(sum(flops_per_voxel(n, M, G, p_free, int(i)) for i in iters))
    rec = {
        "workload": {"voxels": nv, "points": n, "metabolites": M, "groups": G, "lineshape": "voigt",
                     "free_parameters": p_free, "dtype": "complex64", "sw_hz": sw, "skip": 0, "noise_sd": 0.02},
        "fit_seconds": times, "fit_seconds_median": t_med, "voxels_per_s": nv / t_med,
        "trials_mean": float(iters.mean()), "trials_max": int(iters.max()),
        "converged_share": float((status == 0).mean()),
        "status_counts": {str(s): int((status == s).sum()) for s in (0, 1, 2)},
        "amplitude_rel_err_median": float(np.median(np.abs(amp / truth[:, :M] - 1))),
        "flop_formula": FLOP_FORMULA, "flop_per_fit": flop, "fp64_tflops_achieved": flop / t_med / 1e12,
        "jtj_form": "per-thread FMA", "device": torch.cuda.get_device_name(0), "kernel": dev.last_kernel(),
    }
    if a.oracle_voxels > 0:
        xh = x[: a.oracle_voxels].cpu().numpy().astype(np.complex128)
        t0 = time.perf_counter()
        for v in range(a.oracle_voxels):
            orc.fit(xh[v], B, group, dt, init, lo, hi, fixed, tol=1e-10)
        el = time.perf_counter() - t0
        rec["oracle_one_core_voxels_per_s"] = a.oracle_voxels / el
        rec["speedup_vs_one_core_oracle"] = rec["voxels_per_s"] / rec["oracle_one_core_voxels_per_s"]
    text = json.dumps(rec, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
