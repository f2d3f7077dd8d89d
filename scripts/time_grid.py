"""GPU timing of non-Cartesian gridding (xm_axis_sparse), seeded trajectories (tests/_grid_oracle), seeded random data, time
last, 2048 points:

  A        16 coils, radial m = 32 (50 spokes x 64 samples), G = 64, W = 4, complex64
  B        the same number of samples placed uniformly at random
  C        8 coils, 3-D m = 16, G = 32, W = 4, 16,384 random samples, complex64
  A128     A in complex128
  Adegrid  the degridding direction of A (the gridded data back to the samples)

Per workload: seconds of the launch (HIP events around five calls of ``device.axis_sparse`` with the table already on
the device, divided by five; warm-up, median of the repeats); input + output bytes over that time as GB/s and as a
fraction of two device copy rates measured in the same run: the copy11 kernel of tools/stream_ceiling (built here when it
is missing; a child process of its own, before the first workload) and a 1:1 torch copy of the workload's input; the
bytes the gather asks of L2 (entries x row bytes); the entries per row (median, maximum); and what a user can do without
the kernel, in the same run: torch's dense [rows x columns] complex matmul, and ``torch.sparse`` CSR with complex values
(its refusal is recorded when it does not take them).  After the timed steps the kernel's and the dense route's outputs
are compared.  The last figure is the radial / uniform ratio, A over B: equal entry counts, different skew.

    python scripts/time_grid.py --out profiles/grid/time_grid.json
"""
import argparse
import json
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _grid_oracle as orc  # noqa: E402

# name -> (coils, trajectory, matrix, dtype, direction)
WORKLOADS = {
    "A": (16, lambda: orc.radial(32, 50, 64), 32, "complex64", "grid"),
    "B": (16, lambda: orc.random(32, 3200, 2, 17), 32, "complex64", "grid"),
    "C": (8, lambda: orc.random(16, 16384, 3, 19), 16, "complex64", "grid"),
    "A128": (16, lambda: orc.radial(32, 50, 64), 32, "complex128", "grid"),
    "Adegrid": (16, lambda: orc.radial(32, 50, 64), 32, "complex64", "degrid"),
}
INNER = 5  # calls between two events: the host queues ahead, so the figure is the device's time per call


def timed(run, warmup, repeats, inner=INNER):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    from xmris_amd import device as dev
    from xmris_amd import grid_table

    nt = a.points
    copy11 = tools_copy_gbs()
    rec = {"device": torch.cuda.get_device_name(0), "points": nt, "repeats": a.repeats,
           "tools_stream_ceiling_copy11_gbs": copy11, "workloads": []}
    for name in a.workloads.split(","):
        coils, tr, m, dtype, direction = WORKLOADS[name]
        tdt = getattr(torch, dtype)
        t = grid_table(tr(), m)
        table = t.grid if direction == "grid" else t.degrid
        per_row = np.diff(table.rowptr)
        g = torch.Generator(device="cuda").manual_seed(2024)
        x = torch.view_as_complex(torch.randn((coils, table.n, nt, 2), generator=g, device="cuda", dtype=torch.float32)).to(tdt)
        item = x.element_size()
        run = lambda: dev.axis_sparse(x, 1, table)  # noqa: E731
        run()  # (the table's upload)
        dst = torch.empty_like(x)
        _, t_copy, _ = timed(lambda: dst.copy_(x), a.warmup, a.repeats)
        del dst
        copy_gbs = 2.0 * x.numel() * item / t_copy / 1e9
        times, t_med, y = timed(run, a.warmup, a.repeats)
        kernel = dev.last_kernel()
        b_in, b_out = x.numel() * item, y.numel() * item
        w = {"name": name, "coils": coils, "direction": direction, "dtype": dtype, "matrix": list(t.matrix),
             "oversampled": list(t.oversampled), "width": t.width, "columns": table.n, "rows": table.n_rows,
             "entries": table.nnz, "entries_per_row_median": float(np.median(per_row)), "entries_per_row_max": int(per_row.max()),
             "bytes_in": b_in, "bytes_out": b_out, "bytes_gathered": table.nnz * coils * nt * item, "copy_seconds": t_copy,
             "copy_gbs": copy_gbs, "kernel": kernel, "seconds": times, "seconds_median": t_med,
             "in_plus_out_gbs": (b_in + b_out) / t_med / 1e9, "fraction_of_copy_rate": (b_in + b_out) / t_med / 1e9 / copy_gbs,
             "fraction_of_tools_copy11": (b_in + b_out) / t_med / 1e9 / copy11,
             "gathered_tbs": table.nnz * coils * nt * item / t_med / 1e12}
        # the dense route: one complex matrix of the data's dtype, batched over the coils
        rows = torch.from_numpy(np.repeat(np.arange(table.n_rows), per_row)).to("cuda")
        cols = torch.from_numpy(table.col.astype(np.int64)).to("cuda")
        vals = torch.from_numpy(table.val).to("cuda")
        dense = torch.zeros((table.n_rows, table.n), dtype=tdt, device="cuda")
        dense[rows, cols] = vals.to(tdt)
        d_times, t_dense, y_d = timed(lambda: torch.matmul(dense, x), 1, 2, inner=1)
        w.update(dense_matmul_seconds=d_times, dense_matmul_seconds_median=t_dense, speedup_vs_dense_matmul=t_dense / t_med,
                 dense_matrix_bytes=dense.numel() * item)
        scale = float(y_d.abs().max().item())
        w["routes_differ_relative_to_max"] = float((y - y_d).abs().max().item()) / scale
        del dense, y_d
        # torch.sparse CSR with complex values: [rows, columns] @ [columns, T] per coil
        try:
            sp = torch.sparse_csr_tensor(torch.from_numpy(table.rowptr.astype(np.int64)).to("cuda"), cols, vals.to(tdt),
                                         size=(table.n_rows, table.n))
            s_times, t_sp, y_s = timed(lambda: torch.stack([sp @ x[c] for c in range(coils)]), 1, 2, inner=1)
            w.update(torch_sparse_csr_seconds=s_times, torch_sparse_csr_seconds_median=t_sp, speedup_vs_torch_sparse_csr=t_sp / t_med,
                     torch_sparse_differs_relative_to_max=float((y - y_s).abs().max().item()) / scale)
            del sp, y_s
        except Exception as e:  # noqa: BLE001 (recorded: whether this build takes complex CSR is a finding)
            w["torch_sparse_csr_refused"] = f"{type(e).__name__}: {e}"[:300]
        rec["workloads"].append(w)
        del x, y
        torch.cuda.empty_cache()
    by = {w["name"]: w for w in rec["workloads"]}
    if "A" in by and "B" in by:
        rec["radial_over_uniform"] = by["A"]["seconds_median"] / by["B"]["seconds_median"]
    text = json.dumps(rec, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")
    tol = {"complex64": 1e-4, "complex128": 1e-12}
    worst = {w["name"]: w["routes_differ_relative_to_max"] for w in rec["workloads"]}
    assert all(worst[w["name"]] <= tol[w["dtype"]] for w in rec["workloads"]), f"kernel and dense matmul disagree: {worst}"


if __name__ == "__main__":
    main()
