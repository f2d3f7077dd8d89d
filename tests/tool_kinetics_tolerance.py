#!/usr/bin/env python3
"""What tests/test_gpu_kinetics.py takes its bounds from (oracle: tests/_kinetics_oracle.py).  CPU only; the kernel is
not involved.

(a) The model and its three parameter columns evaluated sequentially against the same numbers in the order of the
affine prefix scan (lane-local composition, Hillis-Steele over 64 lanes, local application), on every item of
orc.step_cases() at its starting parameters and at its truth: the largest disagreement relative to the column's largest
magnitude.

(b) The first m = 1, 2, 3 trial steps of lm_steps_kinetics solved by the normal equations against least squares on the
augmented Jacobian, on the same items: per parameter the disagreement in units of its path length, and the relative
disagreement of the cost.

(c) The weights w0, w1 and their rho derivatives: the power series (x < SERIES_X) and the closed forms on expm1
(x >= SERIES_X) against 100-digit arithmetic, each over its own range and at the crossover, relative.

The GPU bounds are 16 x (a) and 16 x (b).

    python tests/tool_kinetics_tolerance.py > profiles/kinetics/tolerance.txt
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _kinetics_oracle as orc  # noqa: E402

STEP_M = (1, 2, 3)


def items():
    for name, kw in orc.step_cases():
        c = orc.kinetic_case(**kw)
        for v in range(c["S"].shape[0]):
            for m in range(c["M"]):
                yield f"{name} voxel {v} product {m}", c, orc.item(c, v, m)


def scan_gap(it, p):
    args = (it["S"], it["t"], it["ths"], it["thp"])
    z1, d1 = orc.forward(p, *args)
    z2, d2 = orc.forward_scan(p, *args)
    gaps = [np.abs(z1 - z2).max() / np.abs(z1).max()]
    for q in range(3):
        top = np.abs(d1[:, q]).max()
        if top > 0:
            gaps.append(np.abs(d1[:, q] - d2[:, q]).max() / top)
    return max(gaps)


def main():
    worst_a, worst_b, worst_f = 0.0, 0.0, 0.0
    for name, c, it in items():
        v0 = orc.start_values(it["Y"], it["w"], it["thp"], it["init"], it["lo"], it["hi"], it["fixed"])[0]
        truth = c["truth"][int(name.rsplit(" ", 1)[1])]
        a = max(scan_gap(it, v0), scan_gap(it, truth))
        worst_a = max(worst_a, a)
        b, f = 0.0, 0.0
        for m in STEP_M:
            r1 = orc.lm_steps_kinetics(it, max_iter=m)
            r2 = orc.lm_steps_kinetics(it, max_iter=m, solver="qr")
            assert [t[0] for t in r1["trials"]] == [t[0] for t in r2["trials"]], (name, m)
            on = r1["path"] > 0
            if on.any():
                b = max(b, float(np.max(np.abs(r1["params"] - r2["params"])[on] / r1["path"][on])))
            f = max(f, abs(r1["rss"] - r2["rss"]) / r1["rss"])
        worst_b, worst_f = max(worst_b, b), max(worst_f, f)
        print(f"{name}: (a) scan against sequential {a:.3e}; (b) normal against qr, |dp| / path {b:.3e}, rss rel {f:.3e}")
    print(f"(a) largest disagreement of the scan order: {worst_a:.3e}")
    print(f"(b) largest |dp| / path: {worst_b:.3e}; largest relative rss disagreement: {worst_f:.3e}")

    import mpmath as mp

    mp.mp.dps = 100

    def exact(x):
        x = mp.mpf(float(x))
        e = mp.exp(-x)
        f1, f2 = (1 - e) / x, (x - 1 + e) / x ** 2
        df1, df2 = (e * (x + 1) - 1) / x ** 2, (2 - x - (x + 2) * e) / x ** 3
        return [f1 - f2, f2, df1 - df2, df2]  # w0, w1, dw0, dw1 at D = 1 (rho = x)

    def worst(fn, xs):
        out = np.zeros(4)
        for x in xs:
            got = [float(v) for v in fn(float(x), np.float64(1.0))]
            for q, (g, e) in enumerate(zip(got, exact(x))):
                out[q] = max(out[q], float(abs((mp.mpf(g) - e) / e)))
        return out

    X = orc.SERIES_X
    below = np.concatenate([np.geomspace(1e-12, X, 400, endpoint=False), [np.nextafter(X, 0)]])
    above = np.concatenate([[X], np.geomspace(X, 40.0, 400)])
    names = "w0 w1 dw0/drho dw1/drho".split()
    fmt = lambda v: ", ".join(f"{n} {e:.2e}" for n, e in zip(names, v))  # noqa: E731
    print(f"(c) series of {orc.TERMS} terms, x in [1e-12, {X}): {fmt(worst(orc.weights_series, below))}")
    print(f"(c) closed forms, x in [{X}, 40]: {fmt(worst(orc.weights_closed, above))}")
    print(f"(c) at the crossover x = {X}: series {fmt(worst(orc.weights_series, [np.nextafter(X, 0)]))}; "
          f"closed forms {fmt(worst(orc.weights_closed, [X]))}")
    print(f"(c) closed forms where the series is used instead, x = 1e-3: {fmt(worst(orc.weights_closed, [1e-3]))}")


if __name__ == "__main__":
    main()
