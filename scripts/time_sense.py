"""GPU timing of SENSE unfolding (xm_sense_unfold), smooth seeded sensitivities (tests/_sense_oracle.make_sens), a seeded
random object pushed through the aliasing model on the GPU, time last:

  main    32 coils x 32 x 32 reduced voxels x 2048, accel (2, 2), complex64 (537 MB in, 67 MB out)
  three   16 coils x 16 x 16 x 8 x 2048, accel (2, 2, 2), complex64
  main128 as main in complex128

Per workload: seconds of the launch (HIP events around five calls of ``device.unfold_sense`` with the sensitivities
already on the device, divided by five; warm-up, median of the repeats); its algorithmic bytes (C + R rows of N_t
samples per group) over that time as GB/s and as a fraction of two device copy rates measured in the same run: the
copy11 kernel of tools/stream_ceiling (built here when it is missing; a child process of its own, before the first
workload) and a 1:1 torch copy of the workload's input (read + write bytes); the prologue's share, from the same launch
on one time point (an upper bound: that launch is too short to hide the host's part of a call); for complex64 the same
launch in the one-point form (rows that start 8 bytes off a 16-byte boundary: a view one sample into a wider tensor);
the same job without the kernel (torch: gather the groups, batched ``linalg.solve`` for U, ``einsum`` in complex128,
scatter); and the numpy oracle on one core over a few groups.  After the timed steps the
kernel's and the torch route's outputs are compared within SENSE_TOL of tests/test_sense.py.

    python scripts/time_sense.py --out profiles/sense/time_unfold_sense.json
"""
import os

os.environ.setdefault("OMP_NUM_THREADS", "1")  # the oracle's one-core figure: no BLAS threads
os.environ.setdefault("OPENBLAS_NUM_THREADS", "1")
os.environ.setdefault("MKL_NUM_THREADS", "1")

import argparse  # noqa: E402
import json  # noqa: E402
import re  # noqa: E402
import subprocess  # noqa: E402
import sys  # noqa: E402
import time  # noqa: E402

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _sense_oracle as orc  # noqa: E402
from test_sense import SENSE_TOL  # noqa: E402

# name -> (coils, reduced sizes, accel, dtype)
WORKLOADS = {
    "main": (32, (32, 32), (2, 2), "complex64"),
    "three": (16, (16, 16, 8), (2, 2, 2), "complex64"),
    "main128": (32, (32, 32), (2, 2), "complex128"),
}


INNER = 5  # calls between two events: the host queues ahead, so the figure is the device's time per call


def timed(run, warmup, repeats):
    import torch

    for _ in range(warmup):
        run()
    torch.cuda.synchronize()
    times, res = [], None
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(INNER):
            res = run()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) / 1e3 / INNER)
    return times, float(np.median(times)), res


def tools_copy_gbs():
    """The copy11 line of tools/stream_ceiling (a child process of its own); the tool is built first when it is missing."""
    exe = os.path.join(ROOT, "tools", "stream_ceiling")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.join(ROOT, "tools"), "stream_ceiling"], check=True)
    out = subprocess.run([exe, "16384", "10"], capture_output=True, text=True, timeout=120, check=True).stdout
    for line in out.splitlines():
        m = re.search(r"([0-9]+(?:\.[0-9]+)?)\s*GB/s", line)
        if line.startswith("copy11") and m:
            return float(m.group(1))
    raise RuntimeError("tools/stream_ceiling printed no copy11 line:\n" + out)


def group_index(ns, rs):
    """q [G, R]: flat full-grid index of every member of every group, groups in row-major order of the reduced grid."""
    full = [n * r for n, r in zip(ns, rs)]
    return np.array([[np.ravel_multi_index(q, full) for q in qq] for _, qq in orc.groups(ns, rs)], dtype=np.int64)


def torch_route(a, sens, q, rtot):
    """The job without the kernel: S gathered per group, U = sqrt(R) (S^H S)^-1 S^H by a batched solve, the unfolding an
    einsum in complex128, the rows scattered to the full grid.  a [C, G, T], sens [C, Nfull]; returns (y [Nfull, T], U)."""
    import torch

    s = sens[:, q].permute(1, 0, 2)  # [G, C, R]
    sh = s.conj().transpose(1, 2)
    u = np.sqrt(rtot) * torch.linalg.solve(sh @ s, sh)  # [G, R, C]
    out = torch.einsum("grc,cgt->grt", u, a.to(torch.complex128))
    y = torch.empty((sens.shape[1], a.shape[-1]), dtype=a.dtype, device=a.device)
    y[q.reshape(-1)] = out.reshape(-1, a.shape[-1]).to(a.dtype)
    return y, u


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--oracle-groups", type=int, default=16)
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    from xmris_amd import device as dev

    nt = a.points
    copy11 = tools_copy_gbs()
    rec = {"device": torch.cuda.get_device_name(0), "points": nt, "repeats": a.repeats, "sense_tol": SENSE_TOL,
           "tools_stream_ceiling_copy11_gbs": copy11, "workloads": []}
    for name in a.workloads.split(","):
        c, ns, rs, dtype = WORKLOADS[name]
        tdt = getattr(torch, dtype)
        full = tuple(n * r for n, r in zip(ns, rs))
        rtot, ng = int(np.prod(rs)), int(np.prod(ns))
        sens_h = orc.make_sens(c, full, seed=11)
        sens = torch.from_numpy(sens_h).to("cuda")
        q_h = group_index(ns, rs)
        q = torch.from_numpy(q_h).to("cuda")
        g = torch.Generator(device="cuda").manual_seed(2024)
        rho = torch.view_as_complex(torch.randn((int(np.prod(full)), nt, 2), generator=g, device="cuda", dtype=torch.float32))
        sflat = sens.reshape(c, -1).to(torch.complex64)
        x = torch.zeros((c, ng, nt), dtype=torch.complex64, device="cuda")
        for k in range(rtot):  # the aliasing model
            x += sflat[:, q[:, k], None] * rho[q[:, k]][None]
        x = (x / np.sqrt(rtot)).to(tdt).reshape(c, *ns, nt).contiguous()
        del rho
        item = x.element_size()
        axes = list(range(1, 1 + len(ns)))
        work = torch.zeros(256, dtype=torch.uint8, device="cuda")
        run = lambda v=x: dev.unfold_sense(v, sens, 0, axes, -1, rs, workspace=work)  # noqa: E731

        dst = torch.empty_like(x)
        _, t_copy, _ = timed(lambda: dst.copy_(x), a.warmup, a.repeats)
        del dst
        copy_gbs = 2.0 * x.numel() * item / t_copy / 1e9
        times, t_med, res = timed(run, a.warmup, a.repeats)
        kernel = dev.last_kernel()
        x1 = x[..., :1].contiguous()
        _, t_one, _ = timed(lambda: run(x1), a.warmup, a.repeats)
        moved = float((c + rtot) * ng * nt * item)
        t_single = None
        if dtype == "complex64":  # the one-point form on the same samples
            wide = torch.empty((*x.shape[:-1], nt + 1), dtype=tdt, device="cuda")
            wide[..., 1:] = x
            off = wide[..., 1:]
            assert off.data_ptr() % 16 == 8 and off.stride(-1) == 1
            _, t_single, _ = timed(lambda: run(off), a.warmup, a.repeats)
            del wide, off
        xg = x.reshape(c, ng, nt)
        sf = sens.reshape(c, -1)
        t_times, t_torch, (y_t, u_t) = timed(lambda: torch_route(xg, sf, q, rtot), a.warmup, a.repeats)
        status = res.status.cpu().numpy()
        w = {"name": name, "coils": c, "reduced": list(ns), "accel": list(rs), "dtype": dtype, "groups": ng,
             "bytes_in": x.numel() * item, "bytes_out": rtot * ng * nt * item, "copy_seconds": t_copy, "copy_gbs": copy_gbs,
             "kernel": kernel, "seconds": times, "seconds_median": t_med, "algorithmic_gbs": moved / t_med / 1e9,
             "fraction_of_copy_rate": moved / t_med / 1e9 / copy_gbs,
             "fraction_of_tools_copy11": moved / t_med / 1e9 / copy11, "one_point_form_seconds": t_single,
             "one_point_seconds": t_one,
             "prologue_share": t_one / t_med, "torch_route_seconds": t_times, "torch_route_seconds_median": t_torch,
             "speedup_vs_torch_route": t_torch / t_med,
             "status_counts": {str(s): int((status == s).sum()) for s in (0, 1, 2, 3)},
             "g_factor_max": float(res.g.max().item())}
        # agreement of the two routes, after the timed steps: |difference| against SENSE_TOL eps kappa sum |U| |a|
        # (complex64: plus the one rounding of each route)
        s_g = sf[:, q].permute(1, 0, 2)
        kappa = torch.linalg.cond(s_g.conj().transpose(1, 2) @ s_g)  # [G]
        unit = orc.EPS * kappa[:, None, None] * torch.einsum("grc,cgt->grt", u_t.abs(), xg.abs().to(torch.float64))
        y_k = res.y.reshape(-1, nt)[q.reshape(-1)].reshape(ng, rtot, nt)
        y_r = y_t[q.reshape(-1)].reshape(ng, rtot, nt)
        bound = SENSE_TOL * unit + (2 * orc.EPS32 * y_r.abs().to(torch.float64) if dtype == "complex64" else 0.0)
        frac = float(((y_k - y_r).abs().to(torch.float64) / bound).max().item())
        w["routes_agree_fraction_of_bound"] = frac
        w["kappa_max"] = float(kappa.max().item())
        if a.oracle_groups > 0:
            xh = xg[:, :a.oracle_groups].cpu().numpy().astype(np.complex128)
            t0 = time.perf_counter()
            for i in range(a.oracle_groups):
                sol = orc.solve_group(sens_h.reshape(c, -1)[:, q_h[i]])
                sol["U"] @ xh[:, i]
            per = (time.perf_counter() - t0) / a.oracle_groups
            w["oracle_one_core_seconds_extrapolated"] = per * ng
            w["speedup_vs_one_core_oracle"] = per * ng / t_med
        rec["workloads"].append(w)
        del x, xg, y_t, u_t, res, unit, y_k, y_r, bound
        torch.cuda.empty_cache()
    text = json.dumps(rec, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")
    worst = {w["name"]: w["routes_agree_fraction_of_bound"] for w in rec["workloads"]}
    assert all(f <= 1.0 for f in worst.values()), f"kernel and torch route disagree beyond SENSE_TOL: {worst}"


if __name__ == "__main__":
    main()
