"""GPU timing of the GRAPPA fill (xm_grappa_fill), seeded random kept lines and seeded weights of an interpolation's size
(tests/_grappa_oracle.random_weights), time last:

  main    32 coils x 16 x 32 kept lines x 2048, accel (2, 1), kernel (2, 3), complex64
  main128 as main in complex128
  two     32 coils x 16 x 16 x 2048, accel (2, 2), kernel (2, 2), complex64
  three   16 coils x 8 x 8 x 8 x 2048, accel (2, 2, 2), kernel (2, 2, 2), complex64

Per workload: seconds of the launch (HIP events around five queued calls of ``device.grappa_fill`` with the weights
already on the device, divided by five; warm-up, median of the repeats); its fused multiply-adds (4 per weight, source
sample and time point, neighbours outside the kept lines not counted) as TFLOP/s and as a fraction of the chip's vector
fp64 peak (half the 157.3 TFLOP/s vector fp32 rate of the MI355X: 78.6); its algorithmic bytes (the kept lines once,
the full grid once) as GB/s and as a fraction of the copy11 rate of tools/stream_ceiling measured in the same run (built
here when it is missing; a child process of its own, before the first workload); for complex64 the same launch in the
one-point form (rows 8 bytes off a 16-byte boundary); and the same job without the kernel (torch: per type an index
gather of the S source lines of every position, then ``einsum`` with the weights, in complex128 and in the data's dtype)
with the peak bytes that route allocates on top of input and output.  After the timed steps the kernel's and the
complex128 torch route's outputs are compared within GRAPPA_TOL of tests/test_grappa.py.

    python scripts/time_grappa.py --out profiles/grappa/time_grappa.json
"""
import argparse
import itertools
import json
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _grappa_oracle as orc  # noqa: E402
from test_grappa import GRAPPA_TOL  # noqa: E402

# name -> (coils, kept lines per dim, accel, kernel, dtype)
WORKLOADS = {
    "main": (32, (16, 32), (2, 1), (2, 3), "complex64"),
    "main128": (32, (16, 32), (2, 1), (2, 3), "complex128"),
    "two": (32, (16, 16), (2, 2), (2, 2), "complex64"),
    "three": (16, (8, 8, 8), (2, 2, 2), (2, 2, 2), "complex64"),
}
FP64_VECTOR_PEAK_TFLOPS = 157.3 / 2  # fp64 vector FMAs issue at half the fp32 vector rate
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


def type_tables(ns, accel, kernel):
    """Per type: (flat full-grid index of its positions [P], flat kept-line index of their sources [P, S], a neighbour
    outside the kept lines pointing at the extra all-zero line prod(ns)); and the number of in-range sources in all."""
    full = tuple(r * n for r, n in zip(accel, ns))
    s_tot, zero = int(np.prod(kernel)), int(np.prod(ns))
    pos = {t: [] for t in range(int(np.prod(accel)) - 1)}
    src = {t: [] for t in pos}
    terms = 0
    for j in itertools.product(*[range(m) for m in full]):
        ty, inside = orc.sources(j, ns, accel, kernel)
        if ty < 0:
            continue
        row = [zero] * s_tot
        for si, q in inside:
            row[si] = int(np.ravel_multi_index(q, ns))
        terms += len(inside)
        pos[ty].append(int(np.ravel_multi_index(j, full)))
        src[ty].append(row)
    return [(np.array(pos[t], dtype=np.int64), np.array(src[t], dtype=np.int64)) for t in sorted(pos)], terms


def torch_route(x0, w, tables, kept_idx, n_full, dtype):
    """The job without the kernel.  x0 [C, kept + 1, T] (the last line zero), w [R - 1, C, S, C]; per type the gathered
    sources [C', P, S, T] and an einsum with the weights in `dtype`; the kept lines copied.  Returns y [C, n_full, T]."""
    import torch

    y = torch.empty((x0.shape[0], n_full, x0.shape[-1]), dtype=x0.dtype, device=x0.device)
    y[:, kept_idx] = x0[:, :-1]
    xs = x0.to(dtype)
    for t, (pos, src) in enumerate(tables):
        g = xs[:, src]  # [C', P, S, T]
        y[:, pos] = torch.einsum("csd,dpst->cpt", w[t].to(dtype), g).to(x0.dtype)
    return y


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

    nt = a.points
    copy11 = tools_copy_gbs()
    rec = {"device": torch.cuda.get_device_name(0), "points": nt, "repeats": a.repeats, "grappa_tol": GRAPPA_TOL,
           "tools_stream_ceiling_copy11_gbs": copy11, "fp64_vector_peak_tflops": FP64_VECTOR_PEAK_TFLOPS, "workloads": []}
    for name in a.workloads.split(","):
        c, ns, accel, kernel, dtype = WORKLOADS[name]
        tdt = getattr(torch, dtype)
        rdt = torch.float32 if dtype == "complex64" else torch.float64
        full = tuple(r * n for r, n in zip(accel, ns))
        n_kept, n_full = int(np.prod(ns)), int(np.prod(full))
        g = torch.Generator(device="cuda").manual_seed(2024)
        x = torch.view_as_complex(torch.randn((c, *ns, nt, 2), generator=g, device="cuda", dtype=rdt))
        w_h = orc.random_weights(accel, kernel, c, 11)
        w = torch.from_numpy(w_h).to("cuda")
        axes = list(range(1, 1 + len(ns)))
        item = x.element_size()
        run = lambda v=x: dev.grappa_fill(v, w, 0, axes, -1, list(accel), list(kernel))  # noqa: E731

        times, t_med, y_k = timed(run, a.warmup, a.repeats)
        kern = dev.last_kernel()
        t_single = None
        if dtype == "complex64":  # the one-point form on the same samples
            wide = torch.empty((*x.shape[:-1], nt + 1), dtype=tdt, device="cuda")
            wide[..., 1:] = x
            off = wide[..., 1:]
            assert off.data_ptr() % 16 == 8 and off.stride(-1) == 1
            _, t_single, y_s = timed(lambda: run(off), a.warmup, a.repeats)
            assert torch.equal(y_s.view(rdt), y_k.view(rdt)), "the paired and the one-point form disagree"
            del wide, off, y_s
        tables_h, terms = type_tables(ns, accel, kernel)
        tables = [(torch.from_numpy(p).to("cuda"), torch.from_numpy(s).to("cuda")) for p, s in tables_h]
        kept_h = np.ravel_multi_index(np.meshgrid(*[orc.kept_lines(n, r) for n, r in zip(ns, accel)], indexing="ij"), full).reshape(-1)
        kept_idx = torch.from_numpy(kept_h.astype(np.int64)).to("cuda")
        x0 = torch.cat([x.reshape(c, n_kept, nt), torch.zeros((c, 1, nt), dtype=tdt, device="cuda")], dim=1)
        route = {}
        for label, dt in (("complex128", torch.complex128), ("data_dtype", tdt)):
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            tt, tm, y_t = timed(lambda d=dt: torch_route(x0, w, tables, kept_idx, n_full, d), a.warmup, a.repeats, inner=1)
            route[label] = {"seconds": tt, "seconds_median": tm,
                            "peak_intermediate_bytes": int(torch.cuda.max_memory_allocated() - base - y_t.numel() * item),
                            "speedup_of_the_kernel": tm / t_med}
            if label == "complex128":
                y_ref = y_t
            del y_t
        flops = 8.0 * terms * c * c * nt  # 4 fused multiply-adds per weight, source sample and time point
        moved = float((n_kept + n_full) * c * nt * item)
        wl = {"name": name, "coils": c, "kept": list(ns), "accel": list(accel), "kernel": list(kernel), "dtype": dtype,
              "bytes_in": n_kept * c * nt * item, "bytes_out": n_full * c * nt * item, "kernel_name": kern, "seconds": times,
              "seconds_median": t_med, "fp64_flop": flops, "fp64_tflops": flops / t_med / 1e12,
              "fraction_of_fp64_vector_peak": flops / t_med / 1e12 / FP64_VECTOR_PEAK_TFLOPS,
              "algorithmic_gbs": moved / t_med / 1e9, "fraction_of_tools_copy11": moved / t_med / 1e9 / copy11,
              "one_point_form_seconds": t_single, "torch_route": route}
        # agreement of the two routes, after the timed steps: |difference| against GRAPPA_TOL eps sum |W| |a| (complex64: plus
        # the one rounding of each route); the acquired lines equal
        yk = y_k.reshape(c, n_full, nt)
        assert torch.equal(yk[:, kept_idx].view(rdt), x.reshape(c, n_kept, nt).view(rdt)), "an acquired line was changed"
        a1 = (x0.real.abs() + x0.imag.abs()).to(torch.float64)
        frac = 0.0
        for t, (pos, src) in enumerate(tables):
            w1 = (w[t].real.abs() + w[t].imag.abs())
            unit = orc.EPS * torch.einsum("csd,dpst->cpt", w1, a1[:, src])
            bound = GRAPPA_TOL * unit + (2 * orc.EPS32 * y_ref[:, pos].abs().to(torch.float64) if dtype == "complex64" else 0.0)
            frac = max(frac, float(((yk[:, pos] - y_ref[:, pos]).abs().to(torch.float64) / bound).max().item()))
            del unit, bound
        wl["routes_agree_fraction_of_bound"] = frac
        rec["workloads"].append(wl)
        del x, x0, y_k, yk, y_ref, a1, tables
        torch.cuda.empty_cache()
    text = json.dumps(rec, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")
    worst = {w["name"]: w["routes_agree_fraction_of_bound"] for w in rec["workloads"]}
    assert all(f <= 1.0 for f in worst.values()), f"kernel and torch route disagree beyond GRAPPA_TOL: {worst}"


if __name__ == "__main__":
    main()
