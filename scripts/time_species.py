"""GPU timing of the multi-echo species separation (xm_species_separate), 3 species
(0, 390, -320 Hz) from 8 uniform echoes 1.1 ms apart, seeded model data made on the GPU (exact model plus 1e-3 noise):

  i    [30 repetitions, 8 echoes, 16 coils, 3200 samples] complex64, readout_time given, no field
  ii   [8, 16, 64, 64] complex64 with fit_field, max_field 100 Hz
  iii  [8, 16, 256, 256] complex64 in both forms
  iv   workload i in complex128
  v    workload i laid out echo-last, [30, 16, 3200, 8]

Per workload: seconds per call (HIP events around 20 calls in a row; one warm-up, median of 3) of
device.species_separate as a whole and of the launch alone -- the arguments of one xm_species_separate call replayed, so
the host's share is the ctypes call -- and the algorithmic traffic, every echo read once and every species written once,
as GB/s and as a fraction of the copy11 rate of tools/stream_ceiling measured in the same run.  Known-field workloads
also time the torch route on the same build: broadcast phase tables and ``torch.einsum`` in complex128 (the kernel's
arithmetic) and in complex64.  Fit workloads time the stages from runs with stages left out (the test-only skip bits, on
the replayed launch): apply and refine as what leaving them out saves, coarse as what it adds to the Gram stage alone,
Gram as the run with nothing else.

Every GPU step -- the copy tool and each workload -- is a child process of its own under ``timeout -k 10``; the first
step that fails ends the run and nothing is started after it.

    python scripts/time_species.py --out profiles/species/time_species.json
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

F = [0.0, 390.0, -320.0]
TE = (1e-3 + 1.1e-3 * np.arange(8)).tolist()
MAX_FIELD = 100.0
WORKLOADS = {  # name -> (R0, R1 as a shape, dtype, form(s), layout, step time limit in s)
    "i": dict(r0=30, r1=(3200,), dtype="complex64", forms=("known",), layout="natural", limit=240),
    "ii": dict(r0=1, r1=(64, 64), dtype="complex64", forms=("fit",), layout="image", limit=240),
    "iii": dict(r0=1, r1=(256, 256), dtype="complex64", forms=("known", "fit"), layout="image", limit=300),
    "iv": dict(r0=30, r1=(3200,), dtype="complex128", forms=("known",), layout="natural", limit=240),
    "v": dict(r0=30, r1=(3200,), dtype="complex64", forms=("known",), layout="echo_last", limit=240),
}
COILS = 16


def make(w, seed=2024):
    """([R0, E, C, R1] model data in the workload's dtype, tau [R1] or None)."""
    import torch

    g = torch.Generator(device="cuda").manual_seed(seed)
    n1 = int(np.prod(w["r1"]))
    rn = lambda *s: torch.randn(s, generator=g, device="cuda", dtype=torch.float64)  # noqa: E731
    rho = torch.complex(rn(w["r0"], len(F), COILS, n1), rn(w["r0"], len(F), COILS, n1))
    psi = (torch.rand((w["r0"], 1, 1, n1), generator=g, device="cuda", dtype=torch.float64) - 0.5) * 1.6 * MAX_FIELD
    if "fit" not in w["forms"]:
        psi = psi * 0.0
    tau = torch.arange(n1, device="cuda", dtype=torch.float64) % 800 * 4e-6 if w["layout"] != "image" else None
    te = torch.tensor(TE, device="cuda", dtype=torch.float64).reshape(1, -1, 1, 1)
    t = te + (tau.reshape(1, 1, 1, -1) if tau is not None else 0.0)
    y = torch.zeros((w["r0"], len(TE), COILS, n1), dtype=torch.complex128, device="cuda")
    for m, f in enumerate(F):
        ang = 2 * np.pi * (f + psi) * t
        y += rho[:, m:m + 1] * torch.complex(torch.cos(ang), torch.sin(ang))
    y += 1e-3 * torch.complex(rn(*y.shape), rn(*y.shape))
    return y.to(getattr(torch, w["dtype"])), tau


INNER = 20  # calls between a pair of events: a call is tens of microseconds of GPU work, the host must not be the figure


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


def step(name, warmup, repeats):
    """One workload in this process -> its record."""
    import torch

    from xmris_amd import _lib
    from xmris_amd import device as dev

    w = WORKLOADS[name]
    y, tau = make(w)
    n1 = int(np.prod(w["r1"]))
    if w["layout"] == "natural":  # [repetition, echo, coil, sample]
        x, ea, ca, tau_b = y, 1, [2], tau.reshape(1, -1)
    elif w["layout"] == "echo_last":  # [repetition, coil, sample, echo]
        x, ea, ca, tau_b = y.permute(0, 2, 3, 1).contiguous(), 3, [1], tau.reshape(1, -1)
    else:  # [echo, coil, x, y]
        x, ea, ca, tau_b = y[0].reshape((len(TE), COILS) + w["r1"]).contiguous(), 0, [1], None
    del y
    elem = 8 if w["dtype"] == "complex64" else 16
    rows = w["r0"] * n1
    nbytes = elem * COILS * rows * (len(TE) + len(F))
    rec = {"workload": name, "device": torch.cuda.get_device_name(0), "shape": list(x.shape), "layout": w["layout"],
           "dtype": w["dtype"], "rows": rows, "algorithmic_bytes": nbytes, "forms": {}}
    for form in w["forms"]:
        fit = form == "fit"
        call = lambda skip=(): dev.species_separate(x, ea, ca, TE, F, tau=tau_b, fit_field=fit,  # noqa: E731
                                                    max_field=MAX_FIELD if fit else None, _skip=skip)
        r, res = timed(call, warmup, repeats)
        status = res.status.cpu().numpy()
        r.update({"kernel": dev.last_kernel(), "copied": res.copied, "levels": list(res.levels),
                  "rows_per_s": rows / r["seconds_median"], "algorithmic_gbs": nbytes / r["seconds_median"] / 1e9,
                  "status_counts": {str(s): int((status == s).sum()) for s in range(5)}})
        # the launch alone: the arguments of one xm_species_separate call, replayed (same buffers, no host work but ctypes)
        seen = {}
        plain = _lib.call
        _lib.call = lambda func, *args: (seen.update({func: args}), plain(func, *args))[1]
        try:
            keep = call()  # (holds the buffers the arguments point to)
        finally:
            _lib.call = plain
        args = list(seen["xm_species_separate"])

        def replay(bits=0):
            a_ = list(args)
            a_[20] |= bits  # the dtype argument carries the test-only skip bits
            plain("xm_species_separate", *a_)
            return keep

        launch = timed(replay, warmup, repeats)[0]
        launch.update({"algorithmic_gbs": nbytes / launch["seconds_median"] / 1e9})
        r["launch_alone"] = launch
        if fit:
            r["grid_points"] = 2 * dev.species_grid(TE, MAX_FIELD)[1] + 1
            runs = {}
            for label, skip in (("no_apply", ("apply",)), ("no_refine", ("refine",)), ("gram_and_coarse", ("refine", "apply")),
                                ("gram_only", ("coarse", "refine", "apply"))):
                bits = 0
                for k in skip:
                    bits |= dev.SPECIES_SKIP[k]
                runs[label] = timed(lambda: replay(bits), warmup, repeats)[0]
            t_all = launch["seconds_median"]
            r["stage_runs"] = runs
            r["split_seconds"] = {"apply": t_all - runs["no_apply"]["seconds_median"],
                                  "refine": t_all - runs["no_refine"]["seconds_median"],
                                  "coarse": runs["gram_and_coarse"]["seconds_median"] - runs["gram_only"]["seconds_median"],
                                  "gram_and_launch": runs["gram_only"]["seconds_median"]}
        else:  # the torch route: broadcast phase tables and einsum
            te = np.asarray(TE)
            p0 = np.linalg.pinv(np.exp(2j * np.pi * np.asarray(F)[None, :] * te[:, None]))
            sub = {"natural": "me,recs->rmcs", "echo_last": "me,rcse->rcsm", "image": "me,ecxy->mcxy"}[w["layout"]]
            for prec in ("complex128", "complex64"):
                dt = getattr(torch, prec)
                P = torch.from_numpy(p0).to("cuda", dt)
                cm = None
                if tau_b is not None:
                    ang = -2 * np.pi * torch.tensor(F, device="cuda", dtype=torch.float64).reshape(-1, 1) * tau_b.reshape(1, -1)
                    cm = torch.complex(torch.cos(ang), torch.sin(ang)).to(dt)  # [M, S]
                    cm = {"natural": cm.reshape(1, len(F), 1, -1), "echo_last": cm.T.reshape(1, 1, -1, len(F))}[w["layout"]]

                def torch_route():
                    out = torch.einsum(sub, P, x.to(dt))
                    if cm is not None:
                        out = out * cm
                    return out.to(x.dtype)

                tr, out = timed(torch_route, warmup, repeats)
                tr["max_abs_difference_to_kernel"] = float((out - res.species).abs().max().item())
                tr["kernel_speedup"] = tr["seconds_median"] / r["seconds_median"]  # (whole call against whole call)
                r["torch_einsum_" + prec] = tr
                del out, P
        rec["forms"][form] = r
        del res
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
    rec = {"frequencies_hz": F, "echo_times_s": TE, "coils": COILS, "max_field_hz": MAX_FIELD, "repeats": a.repeats, "calls_per_timing": INNER,
           "warmup": a.warmup, "tools_stream_ceiling_copy11_gbs": copy11, "workloads": []}
    for name in a.workloads.split(","):
        out = child([sys.executable, os.path.abspath(__file__), "--step", name, "--repeats", str(a.repeats), "--warmup",
                     str(a.warmup)], WORKLOADS[name]["limit"])
        w = json.loads(next(line for line in out.splitlines() if line.startswith("RECORD "))[7:])
        for r in w["forms"].values():
            r["fraction_of_copy11"] = r["algorithmic_gbs"] / copy11
            r["launch_alone"]["fraction_of_copy11"] = r["launch_alone"]["algorithmic_gbs"] / copy11
        rec["workloads"].append(w)
    text = json.dumps(rec, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
