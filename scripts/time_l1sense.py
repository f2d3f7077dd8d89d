"""GPU timing of wavelet-sparse SENSE (recon_l1_sense's device loop) on the workloads of
scripts/time_cgsense.py (seeded trajectories, seeded random data, smooth sensitivities, 2048 columns, pipe density):

  R64    16 coils, radial m = 32 (50 spokes x 64 samples = 3200), G = 64, W = 4, complex64, levels (2, 2)
  R128   R64 in complex128
  V64    8 coils, 3-D m = 16, G = 32, W = 4, 16,384 random samples, complex64, levels (2, 2, 0)

10 steps at tol 0, sparsity 0.02, tikhonov 0.05, the step given (so that the power estimate is timed on its own).  Per
workload, HIP events around queued calls, median of the repeats:
  * seconds per step: (a call of 10 steps - a call of 2) / 8, so the set-up (b = E^H D y, the start launches) drops out;
  * k_l1_prox alone on the shapes of one pass (five queued calls) and its share of a step; the bytes it reads and writes
    once (counted from the shapes) over its time, against the copy11 rate of tools/stream_ceiling measured in the same run;
  * the set-up power estimate (20 steps, one column, a host read per step): a call of 2 steps with the default step minus
    the same call with the step given;
  * the yardstick, same run and build: the same recurrence on the package's two chains with torch element-wise ops, sums
    over the coils and a reshape-based Haar transform (einsum with the Haar matrices), and the largest difference of the
    two results relative to max |x|.

    python scripts/time_l1sense.py --out profiles/l1sense/time_l1sense.json
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
import _l1sense_oracle as l1_orc  # noqa: E402
from time_cgsense import WORKLOADS, iteration_bytes, timed  # noqa: E402
from time_grid import tools_copy_gbs  # noqa: E402

STEPS = 10
SPARSITY, TIKHONOV = 0.02, 0.05


def torch_fista(pb, mask, ms, levels, lam2, tau, n):
    """The recurrence with torch ops around the package's chains; tol 0, no freeze rules.  Returns x [V, T] complex128."""
    import torch

    from xmris_amd import device as dev

    s, y = pb.s, pb.y
    c, v = s.shape
    t = y.shape[2]
    sc, se = s.conj().unsqueeze(-1), s.unsqueeze(-1)
    mats = [torch.from_numpy(l1_orc.haar_matrix(l)).to(device=y.device, dtype=torch.complex128) for l in levels]
    keep = torch.from_numpy(~l1_orc.penalised(ms, levels)).to(y.device).reshape(ms).unsqueeze(-1)
    live = mask.to(torch.bool).reshape(v, 1)

    def transform(a, inverse):
        for d, (m, l, H) in enumerate(zip(ms, levels, mats)):
            pre = int(np.prod(ms[:d], dtype=np.int64))
            a = a.reshape(pre, m >> l, 1 << l, -1)
            a = torch.einsum("ij,pnjq->pniq", H.T if inverse else H, a)
        return a.reshape(tuple(ms) + (t,))

    def reduce(u):
        return (sc * u.reshape(c, v, t).to(torch.complex128)).sum(dim=0)

    b = reduce(pb.adjoint(y))
    theta = (tau * SPARSITY * b.abs().amax(dim=0)).reshape((1,) * len(ms) + (t,))
    x = torch.zeros_like(b)
    vk = torch.zeros_like(b)
    for k, beta in enumerate(dev.fista_momentum(n)):
        if k:
            g = reduce(pb.adjoint(pb.forward((se * vk.unsqueeze(0)).to(y.dtype)))) + lam2 * vk - b
        else:
            g = -b
        coeff = transform((vk - tau * g).reshape(tuple(ms) + (t,)), False)
        mag = coeff.abs()
        shrunk = coeff * torch.where(mag <= theta, torch.zeros_like(mag), 1.0 - theta / mag.clamp_min(1e-300))
        xn = transform(torch.where(keep, coeff, shrunk), True).reshape(v, t) * live
        vk = xn + beta * (xn - x)
        x = xn
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    from xmris_amd import LabeledArray, recon_l1_sense
    from xmris_amd import device as dev
    from xmris_amd.processing import cgsense as host
    from xmris_amd.processing.cgsense import default_chunk, normal_scale
    from xmris_amd.processing.grid import density_weights, oversampled
    from xmris_amd.processing.l1sense import STEP_SAFETY, default_levels

    T = a.points
    copy11 = tools_copy_gbs()
    rec = {"device": torch.cuda.get_device_name(0), "columns": T, "steps": STEPS, "repeats": a.repeats, "sparsity": SPARSITY,
           "tikhonov": TIKHONOV, "tools_stream_ceiling_copy11_gbs": copy11, "workloads": []}
    for name in a.workloads.split(","):
        C, tr, ms, dtype = WORKLOADS[name]
        tdt = getattr(torch, dtype)
        traj = tr()
        S, V = len(traj), int(np.prod(ms))
        Gs = tuple(oversampled(m, 2.0) for m in ms)
        levels = default_levels(ms)
        w = density_weights(traj, ms)
        s_host = cgs_orc.maps(ms, C)
        g = torch.Generator(device="cuda").manual_seed(2024)
        y = torch.view_as_complex(torch.randn((C, S, T, 2), generator=g, device="cuda", dtype=torch.float32)).to(tdt)
        item = y.element_size()
        la = LabeledArray(y, ("coil", "sample", "time"), {}, {}, None)
        chunk = default_chunk(C, Gs, item, T)

        def run(n, step):
            return recon_l1_sense(la, traj, s_host, iterations=n, tol=0.0, sparsity=SPARSITY, tikhonov=TIKHONOV, density=w,
                                  step=step)

        first = run(1, None)  # (the tables' upload; the step of the default path)
        tau = float(first.attrs["l1sense_step"])
        _, t_few, _ = timed(lambda: run(2, tau).data, 0, a.repeats)
        times, t_full, x = timed(lambda: run(STEPS, tau).data, 0, a.repeats)
        _, t_few_default, _ = timed(lambda: run(2, None).data, 0, a.repeats)
        per_step = (t_full - t_few) / (STEPS - 2)
        nbl = dev.l1_blocks(ms, levels)
        by_launch = iteration_bytes(C, S, ms, Gs, T, item)
        del by_launch["k_cgs_step"]
        by_launch["k_l1_prox"] = 6 * V * T * 16 + 4 * nbl * T * 8
        total = sum(by_launch.values())
        rowd = {"name": name, "coils": C, "samples": S, "matrix": list(ms), "oversampled": list(Gs), "levels": list(levels),
                "dtype": dtype, "columns_per_pass": chunk, "step_size": tau, "step_safety": STEP_SAFETY,
                "seconds_10_steps": times, "seconds_10_steps_median": t_full, "seconds_2_steps_median": t_few,
                "seconds_per_step": per_step, "bytes_per_step": total, "bytes_per_step_by_launch": by_launch,
                "step_gbs": total / per_step / 1e9, "fraction_of_tools_copy11": total / per_step / 1e9 / copy11,
                "seconds_power_estimate_20_steps": t_few_default - t_few,
                "power_estimate_in_steps": (t_few_default - t_few) / per_step}
        # the new launch alone, on the shapes of one pass
        Tc = chunk
        passes = -(-T // Tc)
        xx, vv, q, b = (torch.view_as_complex(torch.randn((V, Tc, 2), generator=g, device="cuda", dtype=torch.float64)) for _ in range(4))
        part = [torch.rand((nbl, Tc), generator=g, device="cuda", dtype=torch.float64) + 0.5 for _ in range(4)]
        st = [torch.zeros(Tc, dtype=torch.int32, device="cuda") for _ in range(2)]
        n_it, change = torch.zeros(Tc, dtype=torch.int32, device="cuda"), torch.zeros(Tc, dtype=torch.float64, device="cuda")
        bmax = torch.ones(Tc, dtype=torch.float64, device="cuda")
        mask = torch.ones(V, dtype=torch.uint8, device="cuda")
        zero = [0] * len(ms)
        _, t_prox, _ = timed(lambda: dev.l1_prox(xx, vv, q, b, mask, bmax, part[0], part[1], part[2], part[3], st[0], st[1], n_it,
                                                 change, ms, levels, zero, 1e-3, 1e-3 * SPARSITY, 0.5, 0.0, 1, 0), 1, a.repeats, 5)
        rowd["k_l1_prox_seconds_per_pass"] = t_prox
        rowd["k_l1_prox_gbs"] = by_launch["k_l1_prox"] / passes / t_prox / 1e9
        rowd["k_l1_prox_fraction_of_tools_copy11"] = rowd["k_l1_prox_gbs"] / copy11
        rowd["k_l1_prox_share_of_step"] = passes * t_prox / per_step
        del xx, vv, q, b, part
        # the yardstick: the same set-up, torch for the image-sized half
        pb = host._problem("time_l1sense", la, traj, s_host, None, w, None, 2.0, 4, "sample", "coil", None, 1.0, None)
        host._upload(pb, None)
        lam2 = TIKHONOV * normal_scale(pb.energy, pb.table.density, V)
        live = torch.from_numpy((pb.energy > 0).astype(np.uint8)).to("cuda")

        def yard(n):
            outs = []
            for t0 in range(0, T, chunk):
                pb.y = y[:, :, t0:t0 + chunk].contiguous()
                outs.append(torch_fista(pb, live, ms, levels, lam2, tau, n))
            return torch.cat(outs, dim=1)

        _, y_few, _ = timed(lambda: yard(2), 1, a.repeats)
        y_times, y_full, x_ref = timed(lambda: yard(STEPS), 0, a.repeats)
        y_step = (y_full - y_few) / (STEPS - 2)
        rowd.update(yardstick_seconds_10_steps=y_times, yardstick_seconds_per_step=y_step, speedup_per_step=y_step / per_step,
                    speedup_10_steps=y_full / t_full,
                    differs_from_yardstick_relative_to_max=float((x.reshape(V, T) - x_ref).abs().max().item() / x_ref.abs().max().item()))
        rec["workloads"].append(rowd)
        del y, la, x, x_ref, pb
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
