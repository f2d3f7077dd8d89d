"""GPU timing of the lipid-subspace projection (xm_lipid_project) on 65,536 rows x 2048 points of
seeded random data made on the GPU, the basis from 512 random lipid rows with singular values over three decades:

  r16, r32, r64   complex64 at rank 16, 32 and 64
  r32_c128        rank 32 in complex128
  r32_inplace     rank 32 in complex64, x == y

Per workload: seconds per call (HIP events around 5 queued calls; one warm-up, median of 3) of device.lipid_project in
the MFMA and the plain-FMA form; for r32 also the two forms with a stage left out (the test-only skip bits) and the
torch route ``y - ((y @ conj(U)) * w) @ U.T`` in complex128 and in complex64.  Reported against them: the input plus
output bytes as GB/s and as a fraction of the copy11 rate of tools/stream_ceiling measured in the same run, and the
fp64 work, 8 flops per complex multiply-add in two stages = 16 V T r, as a fraction of the vector fp64 rate the GRAPPA
figures assume (half of 157.3 TFLOP/s).  The set-up (Gram matrix on the device, eigen-decomposition on the host:
device.lipid_subspace) is timed apart by the wall clock for 512 and 4096 lipid rows.

Every GPU step -- the copy tool and each workload -- is a child process of its own under ``timeout -k 10``; the first
step that fails ends the run and nothing is started after it.

    python scripts/time_lipids.py --out profiles/lipids/time_lipids.json
"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROWS, POINTS, LIPID_ROWS = 65536, 2048, 512
ASSUMED_FP64_FLOPS = 0.5 * 157.3e12
WORKLOADS = {  # name -> rank, dtype, in place, extras (skip forms and the torch route), step time limit in s
    "r16": dict(rank=16, dtype="complex64", inplace=False, extras=False, limit=240),
    "r32": dict(rank=32, dtype="complex64", inplace=False, extras=True, limit=300),
    "r64": dict(rank=64, dtype="complex64", inplace=False, extras=False, limit=240),
    "r32_c128": dict(rank=32, dtype="complex128", inplace=False, extras=False, limit=240),
    "r32_inplace": dict(rank=32, dtype="complex64", inplace=True, extras=False, limit=240),
    "setup": dict(limit=300),
}
INNER = 5  # queued calls between a pair of events


def lipid_rows(n, seed=7):
    """[n, POINTS] complex128 on the GPU: random rows, singular values over three decades."""
    import torch

    g = torch.Generator(device="cuda").manual_seed(seed)
    rn = lambda *s: torch.randn(s, generator=g, device="cuda", dtype=torch.float64)  # noqa: E731
    k = min(n, 128)
    a = torch.complex(rn(n, k), rn(n, k))
    b = torch.complex(rn(k, POINTS), rn(k, POINTS))
    sv = 10.0 ** (-3.0 * torch.arange(k, device="cuda", dtype=torch.float64) / (k - 1))
    return (a * sv) @ b


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
    return {"seconds": times, "seconds_median": float(np.median(times))}, res


def setup_step():
    import torch

    from xmris_amd import device as dev

    rec = {"workload": "setup", "device": torch.cuda.get_device_name(0), "points": POINTS, "lipid_rows": {}}
    for n in (512, 4096):
        L = lipid_rows(n)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sigma, u = dev.lipid_subspace(L)
        torch.cuda.synchronize()
        rec["lipid_rows"][str(n)] = {"seconds_wall": time.perf_counter() - t0, "gram": [min(n, POINTS)] * 2,
                                     "vectors": list(u.shape)}
    return rec


def step(name, warmup, repeats):
    """One workload in this process -> its record."""
    import torch

    from xmris_amd import device as dev
    from xmris_amd.processing.lipids import basis_from_subspace

    if name == "setup":
        return setup_step()
    w = WORKLOADS[name]
    sigma, u = dev.lipid_subspace(lipid_rows(LIPID_ROWS))
    rec_b = basis_from_subspace(sigma, u, 0.01, w["rank"], n_rows=LIPID_ROWS)
    g = torch.Generator(device="cuda").manual_seed(11)
    rdt = torch.float32 if w["dtype"] == "complex64" else torch.float64
    x = torch.view_as_complex(torch.randn((ROWS, POINTS, 2), generator=g, device="cuda", dtype=rdt))
    elem = 8 if w["dtype"] == "complex64" else 16
    nbytes = 2 * elem * ROWS * POINTS
    flops = 16.0 * ROWS * POINTS * w["rank"]
    rec = {"workload": name, "device": torch.cuda.get_device_name(0), "rows": ROWS, "points": POINTS, "rank": w["rank"],
           "dtype": w["dtype"], "in_place": w["inplace"], "bytes_in_plus_out": nbytes, "fp64_flops": flops,
           "table_bytes": 16 * POINTS * w["rank"], "forms": {}}
    out = x if w["inplace"] else torch.empty_like(x)
    runs = [("mfma", "mfma", ()), ("fma", "fma", ())]
    if w["extras"]:
        runs += [("mfma_skip_coef", "mfma", ("coef",)), ("mfma_skip_apply", "mfma", ("apply",)),
                 ("fma_skip_coef", "fma", ("coef",)), ("fma_skip_apply", "fma", ("apply",))]
    first = None
    for label, form, skip in runs:
        r, res = timed(lambda: dev.lipid_project(x, rec_b, out=out, form=form, _skip=skip), warmup, repeats)
        s = r["seconds_median"]
        r.update({"kernel": dev.last_kernel(), "copied": res.copied, "rows_per_s": ROWS / s, "gbs": nbytes / s / 1e9,
                  "fp64_tflops": flops / s / 1e12, "fraction_of_assumed_fp64": flops / s / ASSUMED_FP64_FLOPS})
        if not skip and not w["inplace"]:
            if first is None:
                first = res.out.clone()
            else:
                r["max_abs_difference_to_mfma"] = float((res.out - first).abs().max().item())
        rec["forms"][label] = r
    if w["extras"]:
        for prec in ("complex128", "complex64"):
            dt = getattr(torch, prec)
            U = torch.from_numpy(rec_b.vectors).to("cuda", dt)
            wv = torch.from_numpy(rec_b.weights).to("cuda", dt)
            Uc, Ut = U.conj().resolve_conj(), U.T.contiguous()

            def torch_route():
                y = x.to(dt)
                return (y - ((y @ Uc) * wv) @ Ut).to(x.dtype)

            tr, o = timed(torch_route, warmup, repeats)
            tr["max_abs_difference_to_kernel"] = float((o - first).abs().max().item())
            tr["kernel_speedup"] = tr["seconds_median"] / rec["forms"]["mfma"]["seconds_median"]
            rec["torch_" + prec] = tr
            del o, U
    return rec


def child(args, limit):
    """A GPU step as a child process under its own time limit -> its stdout; raises when it fails."""
    out = subprocess.run(["timeout", "-k", "10", str(limit)] + args, capture_output=True, text=True)
    if out.returncode != 0:
        sys.stderr.write(out.stdout[-4000:] + out.stderr[-4000:])
        raise SystemExit(f"step {' '.join(args[-3:])} ended with status {out.returncode}: nothing more is started")
    return out.stdout


def tools_copy_gbs():
    """The copy11 line of tools/stream_ceiling (a child process of its own); the tool is built first when it is missing."""
    exe = os.path.join(ROOT, "tools", "stream_ceiling")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.join(ROOT, "tools"), "stream_ceiling"], check=True)
    out = child([exe, "16384", "10"], 120)
    for line in out.splitlines():
        m = re.search(r"([0-9]+(?:\.[0-9]+)?)\s*GB/s", line)
        if line.startswith("copy11") and m:
            return float(m.group(1))
    raise RuntimeError("tools/stream_ceiling printed no copy11 line:\n" + out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--step", default=None, help="run this one workload in this process and print its record")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.step:
        print("RECORD " + json.dumps(step(a.step, a.warmup, a.repeats)))
        return

    copy11 = tools_copy_gbs()
    rec = {"rows": ROWS, "points": POINTS, "basis_lipid_rows": LIPID_ROWS, "repeats": a.repeats, "calls_per_timing": INNER,
           "warmup": a.warmup, "tools_stream_ceiling_copy11_gbs": copy11, "assumed_fp64_flops": ASSUMED_FP64_FLOPS,
           "workloads": []}
    for name in a.workloads.split(","):
        out = child([sys.executable, os.path.abspath(__file__), "--step", name, "--repeats", str(a.repeats), "--warmup",
                     str(a.warmup)], WORKLOADS[name]["limit"])
        w = json.loads(next(line for line in out.splitlines() if line.startswith("RECORD "))[7:])
        for r in w.get("forms", {}).values():
            r["fraction_of_copy11"] = r["gbs"] / copy11
        rec["workloads"].append(w)
    text = json.dumps(rec, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
