"""`autophase_each` on the GPU: `search_rows` (csrc/xm_search.hip, k_search_rows) against the oracle's differential
evolution row by row, the row hand-out, `phase_apply_rows` (k_phase_rows) against the oracle's `phase`, and the accessor
end to end.  The oracle's answers are computed once per module."""
import numpy as np
import pytest

import _each_rows

pytestmark = pytest.mark.gpu

SEEDS = tuple(range(7000, 7012))
# n = 448 P (the kernel's FULL instantiation, P = 2): seeds at which the oracle and the host engine agree bit for bit on the
# CPU (checked when this test was written; see DESIGN.md "autophase_each")
FULL_N, FULL_SEEDS = 896, (7000, 7001, 7002, 7003, 7004, 7005)
# the generator's seed 7003 at n = 512 (complex128 and its complex64 cast): the generations' best member fails scipy's
# projected-gradient test (norm 3.9e-4 against pgtol 1e-5, found on the CPU with autophase_solver), the search reports
# `needs_polish`, and the oracle's polish moves the member (27 evaluations)
POLISH_SEED = 7003
DP_POLISH = 1e-9  # degrees: what test_gpu_pipeline.py allows between a polished (p0, p1) and the oracle's


@pytest.fixture(scope="module")
def dev():
    import torch

    from xmris_amd import device

    assert torch.cuda.is_available(), "GPU tests need a HIP device (no CPU fallback exists)"
    return device


def _relerr(got, ref):
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300))


_searches = {}


def _oracle_searches(oracle, n, seeds, dtype):
    """Per row: the oracle's OptimizeResult, target index and pivot, and the host engine's generations."""
    from xmris_amd import autophase_solver as aps

    key = (n, tuple(seeds), dtype)
    if key not in _searches:
        rows, freq = _each_rows.make_rows(n, seeds)
        rows = rows.astype(dtype)
        out = []
        for row in rows:
            opt, k, pv = _each_rows.oracle_search(oracle, row, freq)
            obj = aps.NativeObjective(row.astype(np.complex128), freq, pv, k, 1, "acme")
            out.append((opt, k, pv, obj.de(False)))
        _searches[key] = (rows, freq, out)
    return _searches[key]


def _check_records(dev, oracle, n, seeds, dtype, expect_all):
    from xmris_amd import autophase_solver as aps

    rows, freq, refs = _oracle_searches(oracle, n, seeds, dtype)
    recs = dev.search_rows(dev.to_device(rows), dev.uniform_axis(freq))
    checked = 0
    for i, (rec, (opt, k, pv, (rc, hx, hfun, hnfev, hnit))) in enumerate(zip(recs, refs)):
        print(f"n={n} {dtype} seed {seeds[i]}: device x=({rec['x'][0]!r}, {rec['x'][1]!r}) nfev {rec['nfev']} nit {rec['nit']} "
              f"polish {rec['needs_polish']} | oracle x=({opt.x[0]!r}, {opt.x[1]!r}) nfev {opt.nfev} nit {opt.nit} | host nfev {hnfev}")
        if opt.nfev >= 2000:  # where the engines may part (degenerate landscapes)
            continue
        checked += 1
        assert rec["status"] == rc == 0 and rec["target_idx"] == k
        assert (rec["x"][0], rec["x"][1], rec["nfev"], rec["nit"]) == (hx[0], hx[1], hnfev, hnit)  # host engine, bit for bit
        assert rec["nit"] == opt.nit
        if rec["needs_polish"]:
            x, _, _, _ = aps.polish_reference(rows[i], freq, pv, k, 1, "acme", False, rec["x"])
            assert abs(x[0] - opt.x[0]) < DP_POLISH and abs(x[1] - opt.x[1]) < DP_POLISH
        else:  # scipy's polish evaluates f and two forward differences, and keeps the member
            assert (rec["x"][0], rec["x"][1]) == (float(opt.x[0]), float(opt.x[1])) and rec["nfev"] + 3 == opt.nfev
    if expect_all:
        assert checked == len(seeds)
    assert checked >= len(seeds) - 2
    return recs


@pytest.mark.parametrize("dtype", ["complex128", "complex64"])
@pytest.mark.parametrize("n", [512, 1000])
def test_search_rows_equals_the_oracle(dev, oracle, n, dtype):
    """n = 512: P = 2, n = 1000: P = 3, neither FULL.  Every oracle search here ends below 2000 evaluations (450-670
    for the complex128 rows), so no row is left out."""
    _check_records(dev, oracle, n, SEEDS, dtype, expect_all=dtype == "complex128")


def test_search_rows_full_length(dev, oracle):
    _check_records(dev, oracle, FULL_N, FULL_SEEDS, "complex128", expect_all=True)


def test_row_hand_out_more_rows_than_workgroups(dev):
    rows, freq = _each_rows.make_rows(512, SEEDS)
    recs = dev.search_rows(dev.to_device(np.tile(rows, (50, 1))), dev.uniform_axis(freq))
    assert recs.shape == (600,)
    first = recs[:12].tobytes()
    for c in range(1, 50):
        assert recs[12 * c:12 * (c + 1)].tobytes() == first, c


def test_search_rows_pivot_override_p0_only_and_degenerate_rows(dev, oracle):
    from xmris_amd import autophase_solver as aps

    rows, freq = _each_rows.make_rows(512, SEEDS[:4])
    rows = rows.copy()
    rows[1] = 0.0
    rows[3, 300] = complex(1.0, np.inf)
    tc = float(freq[200]) + 0.3 * float(freq[1] - freq[0])
    tidx = int(np.argmin(np.abs(freq - tc)))
    recs = dev.search_rows(dev.to_device(rows), dev.uniform_axis(freq), p0_only=True, pivot=tc, target_idx=tidx)
    assert recs["status"].tolist() == [0, dev.SEARCH_ALL_ZERO, 0, dev.SEARCH_NOT_FINITE]
    assert recs["nfev"][1] == recs["nfev"][3] == 0 and np.isnan(recs["x"][1]).all() and np.isnan(recs["x"][3]).all()
    for i in (0, 2):
        obj = aps.NativeObjective(rows[i], freq, tc, tidx, 1, "acme")
        rc, hx, _, hnfev, hnit = obj.de(True)
        assert (recs["x"][i, 0], recs["x"][i, 1], recs["nfev"][i], recs["nit"][i], recs["target_idx"][i]) == \
            (hx[0], 0.0, hnfev, hnit, tidx)


def _ramps(nb, seed):
    rng = np.random.default_rng(seed)
    p0, p1 = rng.uniform(-180, 180, nb), rng.uniform(-4000, 4000, nb)
    p1[0], p1[-1] = 4000.0, -4000.0
    return p0, p1, rng.uniform(-2000, 2000, nb)


@pytest.mark.parametrize("dtype,tol", [("complex128", 1e-15), ("complex64", 3e-7)])
@pytest.mark.parametrize("shape", [(37, 1531), (5, 8192)])
def test_phase_apply_rows(dev, oracle, shape, dtype, tol):
    """Tolerances: those of the `phase_apply` tests in test_gpu_kernels.py (complex128 1e-15, complex64 3e-7, relative
    to the largest reference value)."""
    nb, n = shape
    rng = np.random.default_rng(n)
    x = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(dtype)
    coords = np.linspace(-2500, 2500, n)
    p0, p1, pv = _ramps(nb, nb)
    ref = np.stack([oracle.phase_values(x[r].astype(np.complex128), coords, 0, p0[r], p1[r], pv[r]) for r in range(nb)])
    xd = dev.to_device(x)
    got = dev.phase_apply_rows(xd, 1, coords, p0, p1, pv).cpu().numpy()
    assert got.dtype == np.dtype(dtype)
    err = _relerr(got, ref)
    print(f"phase_apply_rows {shape} {dtype}: rel err {err:.3e} (tolerance {tol:.0e})")
    assert err < tol
    # the skip mask: those rows are copied through, whatever their parameters hold
    skip = np.zeros(nb, dtype=bool)
    skip[[1, nb - 2]] = True
    bad = np.where(skip, np.nan, p0)
    got = dev.phase_apply_rows(xd, 1, coords, bad, p1, pv, skip=skip).cpu().numpy()
    np.testing.assert_array_equal(got[skip], x[skip])
    assert _relerr(got[~skip], ref[~skip]) < tol
    # in place
    same = dev.phase_apply_rows(xd, 1, coords, p0, p1, pv, out=xd)
    assert same is xd and _relerr(xd.cpu().numpy(), ref) < tol


def test_phase_apply_rows_other_axes(dev, oracle):
    """A non-uniform axis (with a gap that takes the kernel's own-sincos path), the axis in the middle, a zero range."""
    rng = np.random.default_rng(5)
    n = 301
    coords = np.sort(rng.uniform(-10.0, 10.0, n))
    coords[200:] += 40.0
    x = rng.standard_normal((3, n, 2)) + 1j * rng.standard_normal((3, n, 2))
    p0, p1, pv = rng.uniform(-180, 180, (3, 2)), rng.uniform(-4000, 4000, (3, 2)), rng.uniform(-10, 10, (3, 2))
    got = dev.phase_apply_rows(dev.to_device(x), 1, coords, p0, p1, pv).cpu().numpy()
    ref = np.empty_like(x)
    for a, b in np.ndindex(3, 2):
        ref[a, :, b] = oracle.phase_values(x[a, :, b], coords, 0, p0[a, b], p1[a, b], pv[a, b])
    err = _relerr(got, ref)
    print(f"non-uniform axis: rel err {err:.3e}")
    assert err < 1e-15
    flat = np.full(6, 3.5)  # max c - min c = 0: phi = rad(p0) (phasing.py:62-69)
    y = x[:, :6, 0].copy()
    got = dev.phase_apply_rows(dev.to_device(y), 1, flat, p0[:, 0], p1[:, 0], pv[:, 0]).cpu().numpy()
    ref = np.stack([oracle.phase_values(y[r], flat, 0, p0[r, 0], p1[r, 0], pv[r, 0]) for r in range(3)])
    assert _relerr(got, ref) < 1e-15


def test_accessor_end_to_end(dev, oracle):
    """[3, 4, 512] complex64 through `.xmr.autophase_each()`: eleven generator rows (one of them needs the host's
    polish) and one all-zero row, against `oracle.autophase` of every row alone."""
    import xmris_amd

    seeds = list(SEEDS[:11])
    rows, freq = _each_rows.make_rows(512, seeds)
    rows = np.concatenate([rows[:5], np.zeros((1, 512)), rows[5:]]).astype(np.complex64)
    polish_at = seeds.index(POLISH_SEED)
    assert polish_at < 5
    x = rows.reshape(3, 4, 512)
    a = xmris_amd.LabeledArray(x, ("y", "x", "frequency"), {"frequency": freq}, {"te": 30.0})
    from xmris_amd import device

    raw = device.search_rows(device.to_device(rows), device.uniform_axis(freq))
    assert raw["needs_polish"][polish_at] == 1 and raw["status"][5] == device.SEARCH_ALL_ZERO
    r = a.xmr.autophase_each()
    assert r.dims == a.dims and r.attrs["te"] == 30.0 and r.attrs["phase_pivot_coord"] == "frequency"
    got = r.values
    assert got.shape == x.shape and got.dtype == np.complex128  # numpy's promotion against the complex128 phase factor
    p0, p1, pv = (r.attrs[k].reshape(12) for k in ("phase_p0", "phase_p1", "phase_pivot"))
    assert r.attrs["phase_p0"].shape == (3, 4)
    for i in range(12):
        if i == 5:
            assert np.isnan(p0[i]) and np.isnan(p1[i]) and np.isnan(pv[i])
            np.testing.assert_array_equal(got.reshape(12, 512)[i], 0)
            continue
        o = _each_rows.oracle_row(oracle, rows[i], freq, peak_width=100)
        d0, d1 = p0[i] - o.attrs["phase_p0"], p1[i] - o.attrs["phase_p1"]
        err = _relerr(got.reshape(12, 512)[i], o.values)
        print(f"row {i}: dp0 {d0:.3e} dp1 {d1:.3e} degrees, values rel err {err:.3e}, needs_polish {raw['needs_polish'][i]}")
        assert pv[i] == o.attrs["phase_pivot"]
        if raw["needs_polish"][i]:
            assert abs(d0) < DP_POLISH and abs(d1) < DP_POLISH
        else:
            assert d0 == 0.0 and d1 == 0.0
        assert err < 1e-12  # complex128 tolerance of the phased spectra in test_gpu_kernels.py / test_gpu_pipeline.py
    np.testing.assert_array_equal(a.values, x)  # the input is never mutated


def test_host_route_on_the_gpu(dev, oracle):
    """engine="host" (here: positivity) ends in the same `phase_apply_rows` kernel."""
    import xmris_amd

    rows, freq = _each_rows.make_rows(512, SEEDS[:2])
    a = xmris_amd.LabeledArray(rows, ("v", "frequency"), {"frequency": freq})
    r = a.xmr.autophase_each(method="positivity", peak_width=50)
    for i in range(2):
        o = _each_rows.oracle_row(oracle, rows[i], freq, method="positivity", peak_width=50)
        assert abs(r.attrs["phase_p0"][i] - o.attrs["phase_p0"]) < 1e-2 and abs(r.attrs["phase_p1"][i] - o.attrs["phase_p1"]) < 1e-2
        np.testing.assert_allclose(r.values[i], o.values, rtol=0, atol=1e-2 * np.abs(o.values).max())
