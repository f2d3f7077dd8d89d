"""GPU timing of temporal-subspace SENSE (recon_subspace): seeded trajectories (tests/_grid_oracle),
seeded random data, smooth sensitivities, a random orthonormal basis of rank 16 over 2048 time points, half of the
(sample, time) positions kept, one frame, pipe density, regularization 0.05:

  R64    16 coils, radial m = 32 (50 spokes x 64 samples = 3200), G = 64, W = 4, complex64
  R128   R64 in complex128
  V64    8 coils, 3-D m = 16, G = 32, W = 4, 16,384 random samples, complex64

Per workload, HIP events around queued calls, median of the repeats:
  * k_sub_project alone, the bytes it reads and writes once over the time against the copy11 rate of tools/stream_ceiling
    measured in the same run (a child process of its own, before the first workload), and torch's masked einsum of the
    same product in complex128 and in complex64 with the largest difference relative to max |b|;
  * seconds per iteration: (a call of 10 iterations - a call of 2) / 8, and its split: the two chains on R columns,
    k_sub_mix, and the three cgs launches on the folded state, each timed alone (five queued calls);
  * one iteration of recon_cg_sense over all 2048 columns of the same data, same run;
  * the set-up (K, kappa), k_sub_expand, and the whole call of 10 iterations.

    python scripts/time_subspace.py --out profiles/subspace/time_subspace.json
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
from time_cgsense import timed  # noqa: E402
from time_grid import tools_copy_gbs  # noqa: E402

# name -> (coils, trajectory, matrix per dim, dtype)
WORKLOADS = {
    "R64": (16, lambda: orc.radial(32, 50, 64), (32, 32), "complex64"),
    "R128": (16, lambda: orc.radial(32, 50, 64), (32, 32), "complex128"),
    "V64": (8, lambda: orc.random(16, 16384, 3, 19), (16, 16, 16), "complex64"),
}
ITERATIONS = 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--rank", type=int, default=16)
    ap.add_argument("--keep", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    from xmris_amd import LabeledArray, TemporalBasis, recon_cg_sense, recon_subspace
    from xmris_amd import device as dev
    from xmris_amd.processing.cgsense import _problem, _upload
    from xmris_amd.processing.grid import density_weights

    T, R = a.points, a.rank
    copy11 = tools_copy_gbs()
    rec = {"device": torch.cuda.get_device_name(0), "time_points": T, "rank": R, "keep": a.keep, "frames": 1,
           "iterations": ITERATIONS, "repeats": a.repeats, "tools_stream_ceiling_copy11_gbs": copy11, "workloads": []}
    rng = np.random.default_rng(2026)
    basis = TemporalBasis(vectors=np.ascontiguousarray(np.linalg.qr((rng.standard_normal((T, R)) + 1j * rng.standard_normal((T, R))))[0].T))
    for name in a.workloads.split(","):
        C, tr, ms, dtype = WORKLOADS[name]
        tdt = getattr(torch, dtype)
        traj = tr()
        S, V = len(traj), int(np.prod(ms))
        w = density_weights(traj, ms)
        s_host = cgs_orc.maps(ms, C)
        m_host = rng.uniform(size=(S, T)) < a.keep
        g = torch.Generator(device="cuda").manual_seed(2024)
        y = torch.view_as_complex(torch.randn((C, S, T, 2), generator=g, device="cuda", dtype=torch.float32)).to(tdt)
        item = y.element_size()
        la = LabeledArray(y, ("coil", "sample", "time"), {}, {}, None)
        Vd, md = basis.on(y.device), torch.from_numpy(m_host).to("cuda")
        row = {"name": name, "coils": C, "samples": S, "matrix": list(ms), "dtype": dtype}

        # ---- k_sub_project alone, and torch's masked einsum ---------------------------------------------------------
        y4 = y.reshape(C, S, 1, T)
        _, t_proj, b = timed(lambda: dev.sub_project(y4, Vd, md), 1, a.repeats, 5)
        kernel = dev.last_kernel()
        moved = C * S * T * item + S * T + C * S * R * item + R * T * 16
        mask = md.reshape(1, S, T)

        def einsum(cdt):
            return torch.einsum("rt,cst->csr", Vd.conj().to(cdt), torch.where(mask, y, torch.zeros((), dtype=tdt, device="cuda")).to(cdt))

        _, t_e128, b128 = timed(lambda: einsum(torch.complex128), 1, a.repeats)
        _, t_e64, b64 = timed(lambda: einsum(torch.complex64), 1, a.repeats)
        top = b128.abs().max().item()
        row["project"] = {"kernel": kernel, "seconds": t_proj, "bytes": moved,
                          "gbs": moved / t_proj / 1e9, "fraction_of_tools_copy11": moved / t_proj / 1e9 / copy11,
                          "fp64_fma_tflops": 8 * C * S * T * R / t_proj / 1e12,
                          "torch_einsum_complex128_seconds": t_e128, "torch_einsum_complex64_seconds": t_e64,
                          "differs_from_einsum_complex128": float((b[..., 0].to(torch.complex128) - b128).abs().max().item() / top),
                          "einsum_complex64_differs_from_complex128": float((b64.to(torch.complex128) - b128).abs().max().item() / top)}
        del b128, b64, b

        # ---- the whole call and the iteration -------------------------------------------------------------------------
        def run(n):
            return recon_subspace(la, traj, s_host, basis, sampling=m_host, iterations=n, tol=0.0, regularization=0.05, density=w).data

        run(1)  # (the tables' upload)
        _, t_few, _ = timed(lambda: run(2), 0, a.repeats)
        times, t_full, _ = timed(lambda: run(ITERATIONS), 0, a.repeats)
        per_iter = (t_full - t_few) / (ITERATIONS - 2)
        row.update(seconds_10_iterations=times, seconds_10_iterations_median=t_full, seconds_2_iterations_median=t_few,
                   seconds_per_iteration=per_iter)

        # ---- the parts of an iteration, alone, on R columns ---------------------------------------------------------------
        small = LabeledArray(y[:, :, :R].contiguous(), ("coil", "sample", "time"), {}, {}, None)
        pb = _upload(_problem("time_subspace", small, traj, s_host, None, w, None, 2.0, 4, "sample", "coil", None, 1.0, None), None)
        u = torch.view_as_complex(torch.randn((C, V, R, 2), generator=g, device="cuda", dtype=torch.float32)).to(tdt)
        _, t_chains, _ = timed(lambda: pb.adjoint(pb.forward(u)), 1, a.repeats, 5)
        setup = dev.subspace_setup(Vd, m_host, w, S, y.device)
        z = torch.view_as_complex(torch.randn((C, S, R, 1, 2), generator=g, device="cuda", dtype=torch.float32)).to(tdt)
        _, t_mix, _ = timed(lambda: dev.sub_mix(z, setup.kernel, out=z), 1, a.repeats, 5)
        n = V * R
        r, p, q, xx = (torch.view_as_complex(torch.randn((n, 1, 2), generator=g, device="cuda", dtype=torch.float64)) for _ in range(4))
        s_rep = torch.from_numpy(s_host.reshape(C, V)).to("cuda").repeat_interleave(R, dim=1)
        nb = dev.cgs_blocks(n)
        part = [torch.rand((nb, 1), generator=g, device="cuda", dtype=torch.float64) + 0.5 for _ in range(4)]
        st = [torch.zeros(1, dtype=torch.int32, device="cuda") for _ in range(2)]
        n_it, res = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.float64, device="cuda")
        uu = torch.empty((C, n, 1), dtype=tdt, device="cuda")
        cgs = {}
        _, cgs["k_cgs_expand"], _ = timed(lambda: dev.cgs_expand(r, p, s_rep, part[0], part[1], st[0], False, tdt, out=uu), 1, a.repeats, 5)
        _, cgs["k_cgs_reduce"], _ = timed(lambda: dev.cgs_reduce(uu, s_rep, p, q, part[2], 0.01), 1, a.repeats, 5)
        part[2].fill_(1e30)  # (a large delta: tiny steps, so that the repeated updates stay finite)
        _, cgs["k_cgs_step"], _ = timed(lambda: dev.cgs_step(xx, r, p, q, part[0], part[1], part[2], part[3], st[0], st[1], n_it, res,
                                                            0.0, 1), 1, a.repeats, 5)
        row["iteration_parts_seconds"] = {"chains": t_chains, "k_sub_mix": t_mix, **cgs}
        row["iteration_parts_sum_seconds"] = t_chains + t_mix + sum(cgs.values())

        # ---- set-up and expansion ----------------------------------------------------------------------------------------
        _, t_setup, _ = timed(lambda: dev.subspace_setup(Vd, m_host, w, S, y.device), 1, a.repeats)
        coef = torch.view_as_complex(torch.randn((V, R, 1, 2), generator=g, device="cuda", dtype=torch.float64))
        _, t_expand, _ = timed(lambda: dev.sub_expand(coef, Vd), 1, a.repeats, 5)
        row.update(setup_seconds=t_setup, expand_seconds=t_expand)
        del u, z, uu, pb, small

        # ---- recon_cg_sense over all the columns, same data -------------------------------------------------------------------
        def cg(n):
            return recon_cg_sense(la, traj, s_host, iterations=n, tol=0.0, regularization=0.05, density=w).data

        cg(1)
        _, c_few, _ = timed(lambda: cg(2), 0, a.repeats)
        _, c_full, _ = timed(lambda: cg(ITERATIONS), 0, a.repeats)
        cg_iter = (c_full - c_few) / (ITERATIONS - 2)
        row.update(cg_sense_seconds_per_iteration=cg_iter, cg_sense_seconds_10_iterations=c_full,
                   iteration_speedup_over_cg_sense=cg_iter / per_iter, call_speedup_over_cg_sense=c_full / t_full)
        rec["workloads"].append(row)
        del y, y4, la
        torch.cuda.empty_cache()
    text = json.dumps(rec, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")
    worst = {r_["name"]: r_["project"]["differs_from_einsum_complex128"] for r_ in rec["workloads"]}
    assert all(v <= (1e-6 if rec_["dtype"] == "complex64" else 1e-13) for v, rec_ in zip(worst.values(), rec["workloads"])), worst


if __name__ == "__main__":
    main()
