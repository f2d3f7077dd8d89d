"""GPU timing of CG-SENSE (recon_cg_sense's device loop), seeded trajectories (tests/_grid_oracle),
seeded random data and smooth sensitivities, 2048 columns, 10 iterations at tol 0, pipe density, regularization 0.05:

  R64    16 coils, radial m = 32 (50 spokes x 64 samples = 3200), G = 64, W = 4, complex64
  R128   R64 in complex128
  V64    8 coils, 3-D m = 16, G = 32, W = 4, 16,384 random samples, complex64

Per workload, HIP events around queued calls, median of the repeats:
  * seconds per iteration: (a call of 10 iterations - a call of 2) / 8, so the set-up (b = E^H D y) drops out;
  * the three new launches alone (k_cgs_expand, k_cgs_reduce, k_cgs_step on the shapes of one pass, five queued calls each)
    and their share of an iteration;
  * the bytes every launch of an iteration reads and writes once (counted from the shapes), over the time, against the
    copy11 rate of tools/stream_ceiling measured in the same run (a child process of its own, before the first workload);
  * the yardstick, same run and build: the same recurrences written with what the package had before -- ``nufft_forward`` /
    ``nufft_adjoint`` on device-resident arrays plus torch element-wise ops, ``sum`` and products for the per-column
    scalars -- and the largest difference of the two results relative to max |x|.

    python scripts/time_cgsense.py --out profiles/cgsense/time_cgsense.json
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import _cgsense_oracle as cgs_orc  # noqa: E402
import _grid_oracle as orc  # noqa: E402
from time_grid import tools_copy_gbs  # noqa: E402

# name -> (coils, trajectory, matrix per dim, dtype)
WORKLOADS = {
    "R64": (16, lambda: orc.radial(32, 50, 64), (32, 32), "complex64"),
    "R128": (16, lambda: orc.radial(32, 50, 64), (32, 32), "complex128"),
    "V64": (8, lambda: orc.random(16, 16384, 3, 19), (16, 16, 16), "complex64"),
}
ITERATIONS = 10


def timed(run, warmup, repeats, inner=1):
    import torch

    for _ in range(warmup):
        run()
    torch.cuda.synchronize()
    times, res = [], None
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            res = run()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) / 1e3 / inner)
    return times, float(np.median(times)), res


def iteration_bytes(C, S, ms, Gs, T, item):
    """Bytes each launch of one iteration reads + writes once: name -> bytes."""
    V = int(np.prod(ms))
    out = {"k_cgs_expand": 3 * V * T * 16 + C * V * T * item}
    shape = list(ms)
    for a, G in enumerate(Gs):  # forward: F^H per dim
        before = C * int(np.prod(shape)) * T * item
        shape[a] = G
        out[f"forward axis_dft {a}"] = before + C * int(np.prod(shape)) * T * item
    cells = C * int(np.prod(Gs)) * T * item
    out["degrid axis_sparse"] = cells + C * S * T * item
    out["grid axis_sparse"] = cells + C * S * T * item
    for a, m in enumerate(ms):
        before = C * int(np.prod(shape)) * T * item
        shape[a] = m
        out[f"adjoint axis_dft {a}"] = before + C * int(np.prod(shape)) * T * item
    out["k_cgs_reduce"] = C * V * T * item + 2 * V * T * 16
    out["k_cgs_step"] = 6 * V * T * 16
    return out


def torch_cg(y, s_img, traj, ms, w, lam, n):
    """The recurrences on what the package had before this module: nufft_forward / nufft_adjoint on labelled device
    arrays, torch for the rest.  y [C, S, T]; s_img [C, *ms]; tol 0, no freeze rules.  Returns x [*ms, T] complex128."""
    import torch

    from xmris_amd import LabeledArray, nufft_adjoint, nufft_forward

    d = len(ms)
    names = ("x", "y", "z")[:d]
    vox = tuple(range(d))
    sc = s_img.conj().unsqueeze(-1)
    se = s_img.unsqueeze(-1)

    def adjoint(v):
        img = nufft_adjoint(LabeledArray(v, ("coil", "sample", "time"), {}, {}, None), traj, ms, density=w).data
        return (sc * img.to(torch.complex128)).sum(dim=0)

    def normal(p):
        u = (se * p.unsqueeze(0)).to(y.dtype)
        k = nufft_forward(LabeledArray(u, ("coil",) + names + ("time",), {}, {}, None), traj).data
        return adjoint(k) + lam * p

    b = adjoint(y)
    x = torch.zeros_like(b)
    r, p = b.clone(), b.clone()
    rho = (r.real ** 2 + r.imag ** 2).sum(dim=vox)
    for _ in range(n):
        q = normal(p)
        delta = (p.real * q.real + p.imag * q.imag).sum(dim=vox)
        alpha = rho / delta
        x = x + alpha * p
        r = r - alpha * q
        new = (r.real ** 2 + r.imag ** 2).sum(dim=vox)
        p = r + (new / rho) * p
        rho = new
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    from xmris_amd import LabeledArray, recon_cg_sense
    from xmris_amd import device as dev
    from xmris_amd.processing.cgsense import default_chunk
    from xmris_amd.processing.grid import density_weights, oversampled

    T = a.points
    copy11 = tools_copy_gbs()
    rec = {"device": torch.cuda.get_device_name(0), "columns": T, "iterations": ITERATIONS, "repeats": a.repeats,
           "tools_stream_ceiling_copy11_gbs": copy11, "workloads": []}
    for name in a.workloads.split(","):
        C, tr, ms, dtype = WORKLOADS[name]
        tdt = getattr(torch, dtype)
        traj = tr()
        S, V = len(traj), int(np.prod(ms))
        Gs = tuple(oversampled(m, 2.0) for m in ms)
        w = density_weights(traj, ms)
        s_host = cgs_orc.maps(ms, C)
        g = torch.Generator(device="cuda").manual_seed(2024)
        y = torch.view_as_complex(torch.randn((C, S, T, 2), generator=g, device="cuda", dtype=torch.float32)).to(tdt)
        item = y.element_size()
        la = LabeledArray(y, ("coil", "sample", "time"), {}, {}, None)
        chunk = default_chunk(C, Gs, item, T)

        def run(n):
            return recon_cg_sense(la, traj, s_host, iterations=n, tol=0.0, regularization=0.05, density=w).data

        run(1)  # (the tables' upload)
        _, t_few, _ = timed(lambda: run(2), 0, a.repeats)
        times, t_full, x = timed(lambda: run(ITERATIONS), 0, a.repeats)
        per_iter = (t_full - t_few) / (ITERATIONS - 2)
        by_launch = iteration_bytes(C, S, ms, Gs, T, item)
        total = sum(by_launch.values())
        rowd = {"name": name, "coils": C, "samples": S, "matrix": list(ms), "oversampled": list(Gs), "dtype": dtype,
                "columns_per_pass": chunk, "seconds_10_iterations": times, "seconds_10_iterations_median": t_full,
                "seconds_2_iterations_median": t_few, "seconds_per_iteration": per_iter, "bytes_per_iteration": total,
                "bytes_per_iteration_by_launch": by_launch, "iteration_gbs": total / per_iter / 1e9,
                "fraction_of_tools_copy11": total / per_iter / 1e9 / copy11}
        # the three new launches alone, on the shapes of one pass
        Tc = chunk
        passes = -(-T // Tc)
        r, p, q, xx = (torch.view_as_complex(torch.randn((V, Tc, 2), generator=g, device="cuda", dtype=torch.float64)) for _ in range(4))
        s = torch.from_numpy(s_host.reshape(C, V)).to("cuda")
        nb = dev.cgs_blocks(V)
        part = [torch.rand((nb, Tc), generator=g, device="cuda", dtype=torch.float64) + 0.5 for _ in range(4)]
        st = [torch.zeros(Tc, dtype=torch.int32, device="cuda") for _ in range(2)]
        n_it, res = torch.zeros(Tc, dtype=torch.int32, device="cuda"), torch.zeros(Tc, dtype=torch.float64, device="cuda")
        u = torch.empty((C, V, Tc), dtype=tdt, device="cuda")
        new = {}
        _, new["k_cgs_expand"], _ = timed(lambda: dev.cgs_expand(r, p, s, part[0], part[1], st[0], False, tdt, out=u), 1, a.repeats, 5)
        _, new["k_cgs_reduce"], _ = timed(lambda: dev.cgs_reduce(u, s, p, q, part[2], 0.01), 1, a.repeats, 5)
        part[2].fill_(1e30)  # (a large delta: tiny steps, so that the repeated updates stay finite)
        _, new["k_cgs_step"], _ = timed(lambda: dev.cgs_step(xx, r, p, q, part[0], part[1], part[2], part[3], st[0], st[1], n_it, res,
                                                            0.0, 1), 1, a.repeats, 5)
        rowd["new_launch_seconds_per_pass"] = new
        rowd["new_launch_gbs"] = {k: by_launch[k] / passes / v / 1e9 for k, v in new.items()}
        rowd["new_launches_seconds_per_iteration"] = passes * sum(new.values())
        rowd["new_launches_share_of_iteration"] = passes * sum(new.values()) / per_iter
        del r, p, q, xx, u, part
        # the yardstick
        s_img = torch.from_numpy(s_host).to("cuda")
        lam = 0.05 * float(w.sum() / V) * float((np.abs(s_host.reshape(C, V)) ** 2).sum(axis=0).mean())
        _, y_few, _ = timed(lambda: torch_cg(y, s_img, traj, ms, w, lam, 2), 1, a.repeats)
        y_times, y_full, x_ref = timed(lambda: torch_cg(y, s_img, traj, ms, w, lam, ITERATIONS), 0, a.repeats)
        rowd.update(yardstick_seconds_10_iterations=y_times, yardstick_seconds_per_iteration=(y_full - y_few) / (ITERATIONS - 2),
                    speedup_per_iteration=(y_full - y_few) / (ITERATIONS - 2) / per_iter,
                    speedup_10_iterations=y_full / t_full,
                    differs_from_yardstick_relative_to_max=float((x - x_ref).abs().max().item() / x_ref.abs().max().item()))
        rec["workloads"].append(rowd)
        del y, la, x, x_ref
        torch.cuda.empty_cache()
    text = json.dumps(rec, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")
    tol = {"complex64": 1e-4, "complex128": 1e-10}
    worst = {r_["name"]: r_["differs_from_yardstick_relative_to_max"] for r_ in rec["workloads"]}
    assert all(worst[r_["name"]] <= tol[r_["dtype"]] for r_ in rec["workloads"]), f"kernels and yardstick disagree: {worst}"


if __name__ == "__main__":
    main()
