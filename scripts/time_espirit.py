"""GPU timing of espirit_maps on synthetic calibrations made like the cases of
tests/_espirit_oracle.py (ring coils, an ellipse, the central block of the centred k-space, 2 time points).

Per workload: the host calibration (window matrix, eigen-decomposition of A^H A, autocorrelation coefficients; wall
clock), the transform launches (``xm_axis_dft`` per dim on the coefficients already in device memory) and
``k_espirit_eig`` (HIP events around the queued calls: warm-up, median of the repeats), and the whole call from the host
block to the host maps (wall clock).  The yardstick, in the same process on the same matrices: ``torch.linalg.eigh`` on the
batch of full complex128 matrices, which returns every eigenpair and applies none of the selection, phase and crop rules.

    python scripts/time_espirit.py --out profiles/espirit/time_espirit.json
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

import _espirit_oracle as orc  # noqa: E402

# (matrix, coils, kernel, ACS block)
WORKLOADS = [((64, 64), 32, (6, 6), (24, 24)), ((32, 32, 32), 16, (4, 4, 4), (12, 12, 12)), ((64, 64), 8, (6, 6), (24, 24))]


def block(mat, c, acs, seed=0):
    """[C, A..., 2] complex128: the central block of the centred ortho k-space of the coil images, plus 1e-3 noise."""
    s = orc.true_maps(mat, c)
    rho, _ = orc.true_object(mat, 2)
    axes = tuple(range(1, len(mat) + 1))
    img = s[..., None] * rho[None]
    k = np.fft.fftshift(np.fft.fftn(np.fft.ifftshift(img, axes=axes), axes=axes, norm="ortho"), axes=axes)
    rng = np.random.default_rng(seed)
    k = k + orc.NOISE * (rng.standard_normal(k.shape) + 1j * rng.standard_normal(k.shape))
    return np.ascontiguousarray(orc.centre_block(k, acs))


def timed(torch, run, warmup, repeats):
    """(seconds of every repeat, the last result) with HIP events around the queued calls of run()."""
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
    return times, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--workloads", default="0,1,2", help="indices into WORKLOADS, comma separated")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    from xmris_amd import device as dev
    from xmris_amd import espirit_maps
    from xmris_amd.processing import espirit as esp

    rec = {"device": torch.cuda.get_device_name(0), "repeats": a.repeats, "workloads": []}
    for i in (int(v) for v in a.workloads.split(",")):
        mat, c, ker, acs = WORKLOADS[i]
        blk = block(mat, c, acs)
        n_vox, e = int(np.prod(mat)), dev.espirit_entries(c)
        host = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            v, sigma = esp.calibrate(blk, ker, 8, 0.02)
            hc = esp.autocorrelation(v)
            host.append(time.perf_counter() - t0)
        iu, ju = np.triu_indices(c)
        coef = dev.to_device(np.ascontiguousarray(hc[..., iu, ju]))
        tables = [dev.to_device(esp.image_table(n, b)) for n, b in zip(mat, ker)]

        def transform():
            x = coef
            for axis, t in enumerate(tables):
                x = dev.axis_dft(x, axis, t)
            return x

        t_dft, h = timed(torch, transform, a.warmup, a.repeats)
        h = h.reshape(n_vox, e)
        t_eig, res = timed(torch, lambda: dev.espirit_eig(h, c, 1, 0, 0.8), a.warmup, a.repeats)
        kernel = dev.last_kernel()
        t_eig2, _ = timed(torch, lambda: dev.espirit_eig(h, c, 2, 0, 0.8), a.warmup, a.repeats)
        status = res.status.cpu().numpy()
        lam = res.values.cpu().numpy()[0]
        # the yardstick: every eigenpair of the full matrices
        full = torch.zeros((n_vox, c, c), dtype=torch.complex128, device="cuda")
        full[:, torch.from_numpy(iu).cuda(), torch.from_numpy(ju).cuda()] = h
        full = full + torch.triu(full, 1).mH
        t_torch, ref = timed(torch, lambda: torch.linalg.eigh(full), a.warmup, a.repeats)
        gap = float((ref[0][:, -1] - res.values[0]).abs().max().item())
        whole = []
        for _ in range(a.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            espirit_maps(blk, mat, kernel=ker, dims=("kx", "ky", "kz")[:len(mat)])
            whole.append(time.perf_counter() - t0)
        med = lambda t: float(np.median(t))  # noqa: E731
        rec["workloads"].append({
            "matrix": list(mat), "coils": c, "kernel": list(ker), "acs": list(acs), "voxels": n_vox, "entries_per_voxel": e,
            "singular_vectors_kept": int(v.shape[0]), "of": int(sigma.size),
            "host_calibration_seconds": host, "host_calibration_seconds_median": med(host),
            "transform_launches_seconds": t_dft, "transform_launches_seconds_median": med(t_dft),
            "k_espirit_eig_seconds": t_eig, "k_espirit_eig_seconds_median": med(t_eig),
            "k_espirit_eig_microseconds_per_voxel": 1e6 * med(t_eig) / n_vox,
            "k_espirit_eig_two_maps_seconds_median": med(t_eig2), "kernel": kernel,
            "torch_linalg_eigh_seconds": t_torch, "torch_linalg_eigh_seconds_median": med(t_torch),
            "torch_eigh_over_k_espirit_eig": med(t_torch) / med(t_eig),
            "largest_eigenvalue_gap_to_torch": gap,
            "whole_call_seconds": whole, "whole_call_seconds_median": med(whole),
            "status_counts": {str(s): int((status == s).sum()) for s in (0, 1, 2)},
            "voxels_kept_at_crop_0.8": int((lam >= 0.8).sum())})
        print(json.dumps(rec["workloads"][-1]), flush=True)
        del full, ref, h, coef
    text = json.dumps(rec, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
