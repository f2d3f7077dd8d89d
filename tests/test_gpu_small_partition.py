"""Every persistent-grid kernel on the 8-CU stream of tests/_small_partition.py, against the same launch on the default
stream and against the kernel's own CPU oracle ("Testing persistent kernels on a small partition").

A kernel whose grid follows xm_resident_blocks has at most grid_bound(nt) workgroups on that stream, so items_for(nt)
distinct items take every workgroup through its item loop three times and leave a partial fourth round: the LDS reuse
between consecutive items, the prefetch guards of the last trip, the ticket counters' return to zero and the duplicated
odd row of the pair kernels all run at the smallest per-item sizes of the kernels' own test files.  On the whole chip the
same launch is a one-trip run, which those files cover; where the kernel's header promises that an item's bits depend on
its own inputs only, the two runs are compared bit for bit.  The oracle (imported with its tolerance from the kernel's own
test file, no new number) is consulted on a fixed sample: the first and the last item and items of the second and third
rounds.  One non-finite item lies in the second round where the kernel has a status for it.

No kernel here waits for another workgroup; each atomic load is read once and acted on, none is polled.  Those of k_zf2d
(xm_zf2d.h:299), k_zf2p (xm_zf2p.h:466) and k_fft2 (xm_kernels.h:874) are made by the workgroup that drew the last
`done` ticket, after every other one has finished.  xm_zf2p.h:113 reads the key that the earlier guess launch left, and
xm_zf2p.h:220 (next_live) is every workgroup's one look at the running best estimate, whatever it is by then.  k_zf2p's
nap (xm_zf2p.h:247, three s_sleep) has a fixed length.  So none is left out.

The guess stage (k_coarse_mfma, k_zf2p) chooses the candidate rows it transforms from what the other workgroups have
published by then, which may depend on timing: it is held to the assertions of test_gpu_kernels.test_guess_rows_and_refine
only, not compared across the streams."""
import re

import numpy as np
import pytest

import _small_partition as sp

pytestmark = pytest.mark.gpu

# kernel -> threads per workgroup (None: the plan's, read from last_kernel()), how the grid is sized, the factor on the
# resident workgroups, rows per item, and the tests that run it.  tests/test_small_partition_table.py holds this table
# against the launchers in xmris_amd/csrc.
CASES = {
    "k_align": dict(nt=256, grid="ticket", factor=1, tests=("test_align_each", "test_align_average")),
    "k_sense_unfold": dict(nt=256, grid="ticket", factor=1, tests=("test_sense_unfold",)),
    "k_coil_combine": dict(nt=256, grid="ticket", factor=1, tests=("test_coil_combine",)),
    "k_denoise": dict(nt=256, grid="ticket", factor=1, tests=("test_denoise",)),
    "k_hsvd": dict(nt=256, grid="ticket", factor=1, tests=("test_hsvd",)),
    "k_basis_fit": dict(nt=256, grid="ticket", factor=1, tests=("test_basis_fit",)),
    "k_amares_fit": dict(nt=256, grid="ticket", factor=1, tests=("test_amares_fit", "test_amares_fit_linked")),
    "k_axis_dft": dict(nt=256, grid="stride", factor=8, tests=("test_axis_dft",)),
    "k_espirit_eig": dict(nt=256, grid="stride", factor=1, tests=("test_espirit_eig",)),
    "k_search_rows": dict(nt=512, grid="stride", factor=1, tests=("test_search_rows",)),
    "k_zf2": dict(nt=None, grid="stride", factor=1, tests=("test_fused_rows",)),
    "k_zf2d": dict(nt=None, grid="stride", factor=1, tests=("test_fused_rows",)),
    "k_zf2p": dict(nt=None, grid="stride", factor=1, tests=("test_fused_rows", "test_guess_stage")),
    "k_fft2": dict(nt=None, grid="stride", factor=1, tests=("test_fused_rows", "test_fft_rows")),
    "k_fft1": dict(nt=None, grid="stride", factor=1, tests=("test_fused_rows", "test_fft_rows")),
    "k_blue": dict(nt=None, grid="stride", factor=1, tests=("test_fused_rows", "test_fft_rows")),
    "k_zf_apod": dict(nt=256, grid="stride", factor=1, tests=("test_zf_apod",)),
    "k_coarse_mfma": dict(nt=256, grid="stride", factor=1, tests=("test_guess_stage",)),
}


def _up(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _work():
    import torch

    return torch.zeros(256, dtype=torch.uint8, device="cuda")


def _items(kernel):
    """(items, grid bound) of a kernel of the table; the count is checked against the bound here, at run time."""
    c = CASES[kernel]
    bound = sp.grid_bound(c["nt"], c["factor"])
    n = sp.items_for(c["nt"], c["factor"])
    assert n >= 3 * bound + 5 and n % bound != 0
    return n, bound


def _bitwise(a, b, keys, what):
    """Both launches name the same instantiation and give the same bits on every output."""
    assert a["kernel"] == b["kernel"], (what, a["kernel"], b["kernel"])
    for k in keys:
        if a[k] is None and b[k] is None:
            continue
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (what, k)


def _figure(what, n, bound, kernel):
    print(f"{what}: {n} items, grid_bound {bound}, {kernel}")


def _first_seed(make, ok, what):
    """The first seed below 64 whose sample meets the conditions the oracle's tolerance is stated for (the rule of the
    oracles' own parity cases)."""
    for seed in range(64):
        data = make(seed)
        if ok(data):
            return data
    raise AssertionError(f"{what}: no seed below 64 meets the oracle's conditions on the sample")


def _take(d, idx, keys, axis=0):
    return {k: (None if d[k] is None else np.take(d[k], idx, axis=axis)) for k in keys}


# ---- ticket kernels ---------------------------------------------------------------------------------------------------------
def _align_ok(want):
    return bool(np.all(want["margin"] >= 0.2) and np.all(want["one_sign_change"]) and np.all(want["status"] == 0))


@pytest.mark.parametrize("dtype", ["complex128", "complex64"])
def test_align_each(dtype):
    """k_align<each>: one transient per ticket, N = L = 65 (test_a_transient_does_not_depend_on_its_batch's size)."""
    import _align_oracle as orc
    import test_gpu_align as ga
    from xmris_amd import device as dev

    n, bound = _items("k_align")
    pick = sp.sample(n, bound)
    bad = bound + 3

    def make(seed):
        x, r, _, _ = orc.make_data(1, n, 1, 65, seed=400 + seed, max_shift=30.0)
        x, r = x.astype(dtype), r.astype(dtype)  # (the oracle sees what the kernel sees)
        want = orc.align_batch(x[:, pick].astype(np.complex128), r.astype(np.complex128), orc.DT, 0.0, 30.0, 65)
        return x, r, want

    x, r, want = _first_seed(make, lambda d: _align_ok(d[2]), "k_align<each>")
    x[0, bad, 0, 7] = np.nan
    xd, rd, work = _up(x), _up(r), _work()

    def run():
        o = dev.align_rows(xd, 1, -1, rd, n_points=65, dt=orc.DT, max_shift=30.0, workspace=work)
        return dict(y=o.y, shift=o.shift, phase=o.phase, quality=o.quality, status=o.status, work=work)

    a, b = sp.both(run)
    _bitwise(a, b, ga.OUT, "k_align<each>")
    assert "k_align<each" in b["kernel"] and not a["work"].any() and not b["work"].any()
    assert b["status"][0, bad, 0] == 2 and not b["y"][0, bad].any()
    got = _take(b, pick, ga.OUT, axis=1)
    got["kernel"] = b["kernel"]
    ga._check(got, want, x[:, pick].astype(np.complex128), c64=dtype == "complex64", what=f"small partition k_align<each> {dtype}")
    _figure(f"k_align<each> {dtype}", n, bound, b["kernel"])


def test_align_average():
    """k_align<average>: one voxel per ticket, N = 2300 > R 256 = 2048, so every voxel's mean takes two passes before the
    workgroup moves on; two transients a voxel."""
    import _align_oracle as orc
    import test_gpu_align as ga
    from xmris_amd import device as dev

    n, bound = _items("k_align")
    pick = sp.sample(n, bound)
    N, L, A = 2300, 128, 2

    def make(seed):
        x, r, _, _ = orc.make_data(n, A, 1, N, seed=430 + seed, max_shift=30.0, snr=(0.3, 10.0))
        want = orc.align_batch(x[pick], r[pick], orc.DT, 0.0, 30.0, L)
        return x, r, want

    x, r, want = _first_seed(make, lambda d: _align_ok(d[2]), "k_align<average>")
    bad = bound + 3
    x[bad, 1, 0, 7] = np.inf  # (inside the L points the fit reads)
    xd, rd, work = _up(x), _up(r), _work()

    def run():
        o = dev.align_rows(xd, 1, -1, rd, n_points=L, dt=orc.DT, max_shift=30.0, average=True, workspace=work)
        return dict(y=o.y, shift=o.shift, phase=o.phase, quality=o.quality, status=o.status, mean=o.mean,
                    n_averaged=o.n_averaged, work=work)

    a, b = sp.both(run)
    keys = ga.OUT + ("mean", "n_averaged")
    _bitwise(a, b, keys, "k_align<average>")
    assert "k_align<average" in b["kernel"] and not a["work"].any() and not b["work"].any()
    assert list(b["status"][bad, :, 0]) == [0, 2] and b["n_averaged"][bad, 0] == 1
    got = _take(b, pick, keys)
    got["kernel"] = b["kernel"]
    ga._check(got, want, x[pick], what="small partition k_align<average>")
    mean, cnt = orc.average(got["y"], got["status"], got["quality"])  # the ordered sum of the aligned transients, exactly
    assert np.array_equal(got["n_averaged"], cnt) and np.array_equal(got["mean"], mean)
    _figure("k_align<average>", n, bound, b["kernel"])


@pytest.mark.parametrize("dtype", ["complex128", "complex64"])
def test_sense_unfold(dtype):
    """k_sense_unfold: one group of aliased voxels per ticket; the geometry of the parity case 4x5_r2x1_c4 (20 groups, 4
    coils, 9 time points) under a repetition axis of different objects.  The oracle's unit is a repetition: the first,
    the last, one of the second round and one of the third."""
    import _sense_oracle as orc
    from test_sense import check
    from xmris_amd import device as dev

    n, bound = _items("k_sense_unfold")
    ns, rs, c, t = orc.PARITY_CASES["4x5_r2x1_c4"]
    per = int(np.prod(ns))
    reps = -(-n // per)
    assert reps * per >= n
    full = tuple(m * r for m, r in zip(ns, rs))
    sens = orc.make_sens(c, full, 207)
    a_all = np.stack([orc.forward(orc.make((*full, t), 500 + i), sens, rs) for i in range(reps)]).astype(dtype)
    pick = sorted({0, reps - 1, (bound + per) // per, (2 * bound + per) // per})
    bad = (bound + bound // 2) // per + 1
    assert bad not in pick and bound <= bad * per < 2 * bound
    a_all[bad, 1, 0, 2, 5] = np.nan
    xd, work = _up(a_all), _work()

    def run():
        o = dev.unfold_sense(xd, sens, 1, [2, 3], -1, rs, workspace=work)
        return dict(y=o.y, g=o.g, status=o.status, work=work)

    a, b = sp.both(run)
    _bitwise(a, b, ("y", "g", "status"), "k_sense_unfold")
    assert "k_sense_unfold" in b["kernel"] and not a["work"].any() and not b["work"].any()
    assert (b["status"][bad] == 2).sum() == int(np.prod(rs)) and (np.delete(b["status"], bad, axis=0) == 0).all()
    for i in pick:
        want = orc.unfold(a_all[i].astype(np.complex128), sens, rs)
        check(b["y"][i], b["g"][i], b["status"][i], want, dtype, what=f"small partition k_sense_unfold {dtype} repetition {i}")
    _figure(f"k_sense_unfold {dtype}", reps * per, bound, b["kernel"])


@pytest.mark.parametrize("c", [8, 3])
def test_coil_combine(c):
    """k_coil_combine: one voxel per ticket, 33 time points; 8 coils take the matrix-core Gram form, 3 the plain one."""
    import _coils_oracle as orc
    import test_gpu_coils as gc
    from xmris_amd import device as dev

    n, bound = _items("k_coil_combine")
    pick = sp.sample(n, bound)
    bad = bound + 3
    x = orc.make_data(n, c, 1, 33, seed=21 + c)
    want = orc.combine_batch(x[pick], coil_axis=1)
    x[bad, c - 1, 0, 30] = np.nan
    xd, work = _up(x), _work()

    def run():
        o = dev.coil_combine(xd, 1, -1, workspace=work)
        return dict(y=o.y, w=o.weights, quality=o.quality, status=o.status, work=work)

    a, b = sp.both(run)
    _bitwise(a, b, gc.OUT, "k_coil_combine")
    assert ("k_coil_combine<mfma" if c >= 8 else "k_coil_combine<fma") in b["kernel"]
    assert not a["work"].any() and not b["work"].any()
    assert list(np.flatnonzero(b["status"].ravel())) == [bad]
    got = _take(b, pick, gc.OUT)
    got["kernel"] = b["kernel"]
    gc._check(got, want, what=f"small partition k_coil_combine C={c}")
    _figure(f"k_coil_combine C={c}", n, bound, b["kernel"])


@pytest.mark.parametrize("dtype", ["complex128", "complex64"])
def test_denoise(dtype):
    """k_denoise: one voxel per ticket, a 1-D patch of 5 over 40 time points (the parity case g9_p5_n40 on a longer
    grid).  The sample's windows meet the conditions of the oracle's parity cases."""
    import _denoise_oracle as orc
    import test_gpu_denoise as gd
    from xmris_amd import device as dev

    n, bound = _items("k_denoise")
    pick = sp.sample(n, bound)
    bad = bound + 9
    assert all(abs(i - bad) > 5 for i in pick)
    patch = (5,)

    def oracle(x, route):
        win = list(orc.windows((n,), patch))
        rows = [orc.denoise_window(np.stack([x[j] for j in win[i][1]]), win[i][2], None, route) for i in pick]
        return {k: np.array([r[k] for r in rows]) for k in rows[0]}

    def make(seed):
        _, x = orc.make_data((n,), 40, 2, 600 + seed)
        x = x.astype(dtype)
        a, b2 = (oracle(x.astype(np.complex128), rt) for rt in ("eigh", "svd"))
        return x, a, b2

    x, want, _ = _first_seed(make, lambda d: orc.conditions(d[1], d[2]), "k_denoise")
    clean = x.astype(np.complex128)
    x[bad, 17] = np.nan
    xd, work = _up(x), _work()

    def run():
        o = dev.denoise_patches(xd, (0,), -1, patch, workspace=work)
        return dict(y=o.y, rank=o.rank, sigma=o.sigma, status=o.status, work=work)

    a, b = sp.both(run)
    _bitwise(a, b, gd.OUT, "k_denoise")
    assert "k_denoise<fma, 5>" in b["kernel"] and not a["work"].any() and not b["work"].any()
    hit = np.flatnonzero(b["status"])
    assert bad in hit and hit.min() >= bad - 4 and hit.max() <= bad + 4  # the windows that hold the voxel, no other
    got = _take(b, pick, gd.OUT)
    got["kernel"] = b["kernel"]
    gd._check(got, want, clean, dtype, what=f"small partition k_denoise {dtype}")
    _figure(f"k_denoise {dtype}", n, bound, b["kernel"])


@pytest.mark.parametrize("dtype", ["complex128", "complex64"])
def test_hsvd(dtype):
    """k_hsvd: one row per ticket; N = 33, M = 16, K = 2 (the parity case N33-M16-K2).  The sample's rows meet the
    conditions of tests/test_hsvd.py on both of the oracle's routes."""
    import _hsvd_oracle as orc
    import test_gpu_hsvd as gh
    from test_hsvd import EDGE_HZ, HSVD_TOL, MAX_COND
    from xmris_amd import device as dev

    n, bound = _items("k_hsvd")
    pick = sp.sample(n, bound)
    bad = bound + 3
    N, M, K = 33, 16, 2

    def make(seed):
        x = orc.make_fid(N, 700 + seed, n)[0].astype(dtype)
        xs = x[pick].astype(np.complex128)
        return x, orc.hsvd_rows(xs, M, K), orc.hsvd_rows(xs, M, K, route="svd")

    def ok(d):
        x, p, q = d
        g = orc.gap(p, q, x[pick].astype(np.complex128))
        if not all(g[k] <= HSVD_TOL[k] / 16 * 1.01 for k in HSVD_TOL):
            return False
        for r in (p, q):
            f = r["frequency"]
            if not (np.all(r["status"] == 0) and np.all(r["n_removed"] >= 1) and np.all(r["cond"] <= MAX_COND)
                    and np.min(np.minimum(np.abs(f - orc.BAND[0]), np.abs(f - orc.BAND[1]))) >= EDGE_HZ):
                return False
        return True

    x, want, _ = _first_seed(make, ok, "k_hsvd")
    x[bad, 20] = np.inf
    xd, work = _up(x), _work()

    def run():
        o = dev.hsvd_rows(xd, -1, M, K, orc.DT, orc.BAND, workspace=work)
        d = {k: getattr(o, k) for k in gh.OUT}
        d["work"] = work
        return d

    a, b = sp.both(run)
    _bitwise(a, b, gh.OUT, "k_hsvd")
    assert f"k_hsvd<mfma, {M}, {K}>" in b["kernel"] and not a["work"].any() and not b["work"].any()
    assert b["status"][bad] != 0  # (a row of the batch that the method itself gives up on has a status too)
    got = _take(b, pick, gh.OUT)
    got["kernel"] = b["kernel"]
    gh._check(got, want, x[pick].astype(np.complex128), c64=dtype == "complex64", what=f"small partition k_hsvd {dtype}")
    _figure(f"k_hsvd {dtype}", n, bound, b["kernel"])


FIT_OUT = ("params", "amp_sd", "rss", "status", "iters", "fit")


def _fit_result(o):
    return {k: getattr(o, k) for k in FIT_OUT}


def _fit_shares(what, out, x, rows, model, skip=0):
    """The shares that the sampled voxels reach of the two bounds _check_invariants states in numbers: the model within
    1e-12 of its largest magnitude, the cost within 1e-9 of itself (both recomputed from the returned parameters)."""
    fit = rss = 0.0
    for v in rows:
        ref = model(out["params"][v])
        fit = max(fit, float(np.abs(out["fit"][v] - ref).max() / (1e-12 * np.abs(ref).max())))
        want = float(np.sum(np.abs((x[v].astype(np.complex128) - ref)[skip:]) ** 2))
        rss = max(rss, abs(float(out["rss"][v]) - want) / (1e-9 * want))
    print(f"small partition {what}: fit {fit:.3f} of its bound, rss {rss:.3f} of its bound, {len(rows)} voxels")


def test_basis_fit():
    """k_basis_fit: one voxel per ticket; 3 metabolites in 3 groups, 129 points (SHAPES["M3G3"], N_LIST[1])."""
    import _basis_oracle as orc
    import test_gpu_basis as gb
    from xmris_amd import device as dev

    n, bound = _items("k_basis_fit")
    pick = sp.sample(n, bound)
    bad = bound + 3
    c = orc.kernel_case(3, 3, 129, 100, n_vox=n)
    x = np.array(c["x"])
    x[bad, 40] = np.inf
    xd, bd = _up(x), _up(c["B"])

    def run():
        o = dev.basis_fit(xd, 1, bd, c["group"], c["init"], c["lo"], c["hi"], c["fixed"], dt=c["dt"], skip=c["skip"])
        return _fit_result(o)

    a, b = sp.both(run)
    _bitwise(a, b, FIT_OUT, "k_basis_fit")
    assert "k_basis_fit" in b["kernel"] and b["status"][bad] == 2 and len({float(v) for v in b["rss"][pick]}) == len(pick)
    assert gb._check_invariants(b, x, c, 200, rows=pick) == len(pick)
    _fit_shares("k_basis_fit", b, x, pick, lambda p: orc.model(p, c["B"], c["group"], c["dt"]), c["skip"])
    _figure("k_basis_fit", n, bound, b["kernel"])


def test_amares_fit():
    """k_amares_fit<false>: one voxel per ticket; K = 1, n = 96, the smallest footprint (test_ticket_counter_over_many_rounds)."""
    import _amares_oracle as orc
    import test_amares_kernel as gk
    from xmris_amd import device as dev

    n, bound = _items("k_amares_fit")
    pick = sp.sample(n, bound)
    bad = bound + 3
    c = orc.kernel_case(1, 96, 6, n_vox=n)
    x = np.array(c["x"])
    x[bad, 17] = complex(np.inf, 0.0)
    xd = _up(x)

    def run():
        return _fit_result(dev.amares_fit(xd, 1, c["init"], c["lo"], c["hi"], c["fixed"], dt=c["dt"], t0=c["t0"]))

    a, b = sp.both(run)
    _bitwise(a, b, FIT_OUT, "k_amares_fit<false>")
    assert "k_amares_fit<false" in b["kernel"] and b["status"][bad] == 2 and np.isnan(b["rss"][bad])
    assert np.all(np.delete(b["status"], bad) != 2) and len({float(v) for v in b["rss"][pick]}) == len(pick)
    assert gk._check_invariants(b, x, c, rows=pick) == len(pick)
    _fit_shares("k_amares_fit<false>", b, x, pick, lambda p: orc.model(p, c["t"]))
    _figure("k_amares_fit<false>", n, bound, b["kernel"])


def test_amares_fit_linked():
    """k_amares_fit<true>: the linked doublet of lk.gpu_cases() (K = 3, n = 64), one voxel per ticket."""
    import _amares_links as lk
    import test_gpu_amares_links as gl
    from xmris_amd import device as dev

    n, bound = _items("k_amares_fit")
    pick = sp.sample(n, bound)
    bad = bound + 3
    c = lk.doublet_case(n_vox=n)
    x = np.array(c["x"])
    x[bad, 17] = complex(np.inf, 0.0)
    xd = _up(x)
    n_free = []

    def run():
        o = dev.amares_fit(xd, 1, c["init"], c["lo"], c["hi"], c["fixed"], dt=c["dt"], t0=c["t0"], links=c["links"])
        n_free.append(o.n_free)
        return _fit_result(o)

    a, b = sp.both(run)
    _bitwise(a, b, FIT_OUT, "k_amares_fit<true>")
    assert b["status"][bad] == 2 and np.all(np.delete(b["status"], bad) != 2)
    got = _take(b, pick, FIT_OUT)
    got["n_free"], got["kernel"] = n_free[1], b["kernel"]
    gl._check_invariants(got, x[pick], c)
    _fit_shares("k_amares_fit<true>", b, x, pick, lambda p: gl.orc.model(p.ravel(), c["t"]))
    _figure("k_amares_fit<true>", n, bound, b["kernel"])


# ---- stride kernels, per voxel and MRSI ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["complex64", "complex128"])
@pytest.mark.parametrize("n, m", [(7, 16), (3, 32), (5, 64)])  # PT = 4, 8, 16; n no multiple of JB = 4, 2 (1 divides all)
def test_axis_dft(n, m, dtype):
    """k_axis_dft: a tile of 64 pencils per trip, at most 8 x resident workgroups; three outer blocks whose inner length
    is no multiple of 64, so tiles straddle the blocks and the last one is part dead.  The whole result is held to the
    bound (the oracle is one einsum); one NaN pencil lies in a second-round tile."""
    import _mrsi_oracle as orc
    from test_mrsi import bound as mrsi_bound
    from xmris_amd import device as dev

    tiles, bound = _items("k_axis_dft")
    n_inner = (tiles * 64 - 20) // 3
    n_inner -= (n_inner % 64 == 0)
    assert n_inner % 64 and -(-3 * n_inner // 64) >= 3 * bound + 5 and (3 * n_inner) % 64
    x = orc.make((3, n, n_inner), seed=n + m).astype(dtype)
    t = orc.make((m, n), seed=n + m + 1)
    bo, bi = divmod(64 * (bound + 2) + 11, n_inner)  # a pencil of a second-round tile
    x[bo, n - 1, bi] = np.nan
    xd, td = _up(x), _up(t)
    a, b = sp.both(lambda: dict(y=dev.axis_dft(xd, 1, td)))
    _bitwise(a, b, ("y",), "k_axis_dft")
    assert f"k_axis_dft<{'c64' if dtype == 'complex64' else 'c128'}, {4 if m <= 16 else 8 if m <= 32 else 16}" in b["kernel"], b["kernel"]
    assert np.isnan(b["y"][bo, :, bi]).all()
    x128 = np.nan_to_num(x.astype(np.complex128))
    want = np.einsum("pj,oji->opi", t, x128)
    u = orc.EPS * np.einsum("pj,oji->opi", np.abs(t), np.abs(x128))
    d, lim = np.abs(b["y"] - want), mrsi_bound(u, dtype)
    d[bo, :, bi] = 0.0
    share = float((d / np.where(lim > 0, lim, 1.0)).max())
    print(f"small partition k_axis_dft n {n} m {m} {dtype}: {share:.3f} of its bound")
    assert np.all(d <= lim), share
    _figure(f"k_axis_dft n {n} m {m} {dtype}", -(-3 * n_inner // 64), bound, b["kernel"])


@pytest.mark.parametrize("c", [3, 8])
def test_espirit_eig(c):
    """k_espirit_eig: one voxel per trip; 3 coils have a bye in the round-robin pairing, 8 fill their pairs.  A
    non-finite voxel of the second round takes the early `continue`."""
    import _espirit_oracle as orc
    import test_gpu_espirit as ge
    from test_espirit import ESP_TOL_MAP, ESP_TOL_RESIDUAL, ESP_TOL_VALUE
    from xmris_amd import device as dev

    n, bound = _items("k_espirit_eig")
    pick = sp.sample(n, bound)
    bad = bound + 3
    h, _ = orc.random_hermitian(c, n, 900 + c)
    h[bad, 0, c - 1] = np.nan
    hd = _up(orc.upper(h))

    def run():
        o = dev.espirit_eig(hd, c, n_maps=2, crop=0.0)
        return dict(maps=o.maps, values=o.values, status=o.status)

    a, b = sp.both(run)
    _bitwise(a, b, ("maps", "values", "status"), "k_espirit_eig")
    assert list(np.flatnonzero(b["status"])) == [bad] and b["status"][bad] == 2
    assert np.all(b["maps"][:, :, bad] == 0) and np.all(np.isnan(b["values"][:, bad]))
    lam, vec = np.linalg.eigh(h[pick])
    want_maps, want_values = orc.select(lam, vec, 2, 0, 0.0)
    maps, values = b["maps"][:, :, pick], b["values"][:, pick]
    dv, dm = float(np.abs(values - want_values).max()), float(np.abs(maps - want_maps).max())
    res = max(float(ge.residual(h[pick], maps[k], values[k]).max()) for k in range(2))
    print(f"small partition k_espirit_eig C {c}: values {dv:.3e} of {ESP_TOL_VALUE:.3e}, maps {dm:.3e} of {ESP_TOL_MAP:.3e}, "
          f"residual {res:.3e} of {ESP_TOL_RESIDUAL:.3e}")
    assert dv <= ESP_TOL_VALUE and dm <= ESP_TOL_MAP and res <= ESP_TOL_RESIDUAL
    _figure(f"k_espirit_eig C {c}", n, bound, b["kernel"])


def test_search_rows(oracle):
    """k_search_rows: one row per trip, 512 threads; n = 512 (P = 2).  The sample is held to what
    test_gpu_autophase_each._check_records holds every row to: the host engine bit for bit, the oracle's search by its
    iteration count and its member, a member that needs the polish within DP_POLISH of the oracle's once polished.
    xm_search_rows notes no kernel name, so there is none to compare between the streams."""
    import _each_rows
    from test_gpu_autophase_each import DP_POLISH
    from xmris_amd import autophase_solver as aps
    from xmris_amd import device as dev

    n, bound = _items("k_search_rows")
    pick = sp.sample(n, bound)[:12]
    bad = bound + 3
    rows, freq = _each_rows.make_rows(512, range(7000, 7000 + n))
    rows = np.array(rows)
    rows[bad, 300] = complex(1.0, np.inf)
    xd = dev.to_device(rows)
    a, b = sp.both(lambda: dict(rec=dev.search_rows(xd, dev.uniform_axis(freq))))
    assert a["rec"].dtype == b["rec"].dtype and a["rec"].tobytes() == b["rec"].tobytes()
    recs = b["rec"]
    assert recs["status"][bad] == dev.SEARCH_NOT_FINITE and recs["nfev"][bad] == 0
    checked = polished = 0
    for i in pick:
        opt, k, pv = _each_rows.oracle_search(oracle, rows[i], freq)
        rc, hx, _, hnfev, hnit = aps.NativeObjective(rows[i], freq, pv, k, 1, "acme").de(False)
        rec = recs[i]
        if opt.nfev >= 2000:  # where the engines may part (degenerate landscapes)
            continue
        checked += 1
        assert rec["status"] == rc == 0 and rec["target_idx"] == k
        assert (rec["x"][0], rec["x"][1], rec["nfev"], rec["nit"]) == (hx[0], hx[1], hnfev, hnit)
        assert rec["nit"] == opt.nit
        if rec["needs_polish"]:
            x, _, _, _ = aps.polish_reference(rows[i], freq, pv, k, 1, "acme", False, rec["x"])
            assert abs(x[0] - opt.x[0]) < DP_POLISH and abs(x[1] - opt.x[1]) < DP_POLISH
            polished += 1
        else:  # scipy's polish evaluates f and two forward differences, and keeps the member
            assert (rec["x"][0], rec["x"][1]) == (float(opt.x[0]), float(opt.x[1])) and rec["nfev"] + 3 == opt.nfev
    assert checked >= len(pick) - 2
    print(f"small partition k_search_rows: {checked} of {len(pick)} sampled rows equal the host engine bit for bit and the "
          f"oracle in nit and member ({polished} after the polish, bound {DP_POLISH} degrees)")
    _figure("k_search_rows", n, bound, "k_search_rows (no name noted)")


# ---- stride kernels, FFT family -----------------------------------------------------------------------------------------------
def _rand(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(dtype)


def _plan_threads(kernel):
    m = re.search(r"FftPlan<(\d+),(\d+)", kernel)
    assert m, kernel
    return int(m.group(2))


def _rows_checked(kernel, rows, base, per_item=1):
    """The launch ran `base`, and `rows` is odd and at least three rounds of this plan's grid bound plus one."""
    assert kernel.startswith(base + "<"), kernel
    nt = CASES[base]["nt"] or _plan_threads(kernel)
    bound = sp.grid_bound(nt)
    assert rows % 2 == 1 and rows >= 3 * bound * per_item + 1, (kernel, rows, bound)
    return bound


# (dtype, n_in, n_out, pad_left, want_argmax, kernel, threads of its plan, rows per item): one power-of-two zero fill, one
# mixed and one Bluestein length in both dtypes, plus the forms only one geometry reaches -- the complex128 write-only
# ">= 2x" kernel (k_zf2d) and the complex64 rows off the 16-byte grid (k_zf2<float>).  Rows per item: k_fft2 takes a pair of
# rows per trip and so does k_blue on complex64 rows (complex128: one); the two kernels that write through a row queue
# hand out QUEUE rows per ticket, see _queue_rows.  The threads are what the row count is sized by; _rows_checked holds
# them to the plan that ran.
QUEUE = "queue"
FUSED = [
    ("complex64", 1024, 2048, 0, True, "k_zf2p", 128, QUEUE), ("complex128", 1024, 2048, 0, True, "k_zf2", 128, QUEUE),
    ("complex64", 1023, 2048, 1, True, "k_zf2", 128, 1), ("complex128", 4096, 8192, 0, False, "k_zf2d", 256, 1),
    ("complex64", 2048, 2048, 0, True, "k_fft2", 256, 2), ("complex128", 2048, 2048, 0, True, "k_fft1", 128, 1),
    ("complex64", 1536, 1536, 0, True, "k_fft2", 128, 2), ("complex128", 1536, 1536, 0, True, "k_fft1", 128, 1),
    ("complex64", 1000, 1000, 0, True, "k_blue", 256, 2), ("complex128", 1000, 1000, 0, True, "k_blue", 256, 1),
]


def _queue_rows(dtype, n_in, n_out):
    """Rows per ticket of the writing row queues of k_zf2p (xm_launch_zf2p.hip, `chunk`) and of k_zf2<double>
    (xm_launch.inc, launch_zf2_mode): about 96 KiB of traffic, a row being n_in samples read and n_out written."""
    row_bytes = (8 if dtype == "complex64" else 16) * (n_in + n_out)
    return min(max(-(-98304 // row_bytes), 1), 64)


@pytest.mark.parametrize("dtype, n_in, n_out, pad_left, amax, kernel, nt, per_item", FUSED)
def test_fused_rows(oracle, dtype, n_in, n_out, pad_left, amax, kernel, nt, per_item):
    """pipeline_fused as test_gpu_kernels.test_persistent_grid_boundaries runs it, on an odd row count three rounds of the
    small grid long: spectra within TIGHT of the oracle, the arg-max numpy's, and the same bits on both streams."""
    from test_gpu_kernels import TIGHT, _relerr
    from xmris_amd import device as dev

    if per_item == QUEUE:
        per_item = _queue_rows(dtype, n_in, n_out)
        assert per_item == (4 if dtype == "complex64" else 2)  # (1024 -> 2048: 24 KiB and 48 KiB a row)
    rows = sp.rows_for(nt, per_item)
    x = _rand((rows, n_in), dtype, seed=rows + n_in)
    pads = [(0, 0), (pad_left, n_out - n_in - pad_left)]
    spec = oracle.to_spectrum_values(np.pad(x.astype(np.complex128), pads), 1)
    xd = dev.to_device(x)

    def run():
        r = dev.pipeline_fused(xd, n_out, pad_left, want_argmax=amax)
        return dict(out=r.out, argidx=r.argidx if amax else None)

    a, b = sp.both(run)
    _bitwise(a, b, ("out", "argidx"), kernel)
    bound = _rows_checked(b["kernel"], rows, kernel, per_item)
    err, tol = _relerr(b["out"], spec), TIGHT[dtype] * (4 if n_out == 1000 else 1)
    print(f"small partition {b['kernel']} {dtype} {n_in} -> {n_out}: {err / tol:.3f} of its bound")
    assert err < tol
    if amax:
        np.testing.assert_array_equal(b["argidx"], np.argmax(np.abs(spec), axis=1))
    _figure(f"{kernel} {dtype} {n_in} -> {n_out}", rows, bound, b["kernel"])


@pytest.mark.parametrize("dtype, n, kernel, per_item, nt", [
    ("complex64", 1024, "k_fft2", 2, 128), ("complex128", 1024, "k_fft1", 1, 64),
    ("complex64", 768, "k_fft2", 2, 64), ("complex128", 768, "k_fft1", 1, 64),
    ("complex64", 1000, "k_blue", 2, 256), ("complex128", 1000, "k_blue", 1, 256)])
def test_fft_rows(oracle, dtype, n, kernel, per_item, nt):
    """dev.fft as test_gpu_kernels.test_fft_matches_numpy runs it, on the same kind of row count."""
    from test_gpu_kernels import TIGHT, _relerr
    from xmris_amd import device as dev

    rows = sp.rows_for(nt, per_item)
    x = _rand((rows, n), dtype, seed=rows + n)
    ref = oracle.fft_values(x.astype(np.complex128), 1)
    xd = dev.to_device(x)
    a, b = sp.both(lambda: dict(out=dev.fft(xd, 1)))
    _bitwise(a, b, ("out",), kernel)
    bound = _rows_checked(b["kernel"], rows, kernel, per_item)
    err, tol = _relerr(b["out"], ref), TIGHT[dtype] * (4 if n == 1000 else 1)
    print(f"small partition fft {b['kernel']} {dtype} {n}: {err / tol:.3f} of its bound")
    assert b["out"].dtype == np.dtype(dtype) and err < tol
    _figure(f"fft {kernel} {dtype} {n}", rows, bound, b["kernel"])


@pytest.mark.parametrize("dtype, promote", [("complex64", False), ("complex64", True), ("complex128", False)])
def test_zf_apod(dtype, promote):
    """k_zf_apod as test_gpu_kernels.test_zero_fill_apodize_one_launch runs it (1024 -> 2048): numpy's products and +0
    padding bit for bit, on both streams, and a second launch on the counters the first one left."""
    import torch

    from xmris_amd import device as dev

    rows, n_in, n_out = sp.rows_for(256), 1024, 2048
    x = _rand((rows, n_in), dtype, seed=rows)
    w = np.exp(-np.pi * 5.0 * np.arange(n_out) / 5000.0)
    out_c128 = promote or dtype == "complex128"
    xd = dev.to_device(x)
    wd = torch.from_numpy(w).to("cuda", torch.float64 if out_c128 else torch.float32)
    a, b = sp.both(lambda: dict(out=dev.zf_apod(xd, n_out, 0, wd, promote=promote), again=dev.zf_apod(xd, n_out, 0, wd, promote=promote)))
    _bitwise(a, b, ("out", "again"), "k_zf_apod")
    bound = _rows_checked(b["kernel"], rows, "k_zf_apod")
    ref = np.zeros((rows, n_out), dtype=np.complex128 if out_c128 else np.complex64)
    ref[:, :n_in] = x.astype(ref.dtype) * (w if out_c128 else w.astype(np.float32))[:n_in][None, :]
    assert np.array_equal(b["out"].view(np.uint8), ref.view(np.uint8)) and np.array_equal(b["again"].view(np.uint8), ref.view(np.uint8))
    print(f"small partition k_zf_apod {dtype}{' promoted' if promote else ''}: numpy's products and padding bit for bit (no bound)")
    _figure(f"k_zf_apod {dtype}{' promoted' if promote else ''}", rows, bound, b["kernel"])


@pytest.mark.parametrize("dtype", ["complex64", "complex128"])
@pytest.mark.parametrize("n_in, n_out, kernel, nt, per_item", [(1024, 2048, "k_coarse_mfma", 256, 4), (400, 1024, "k_zf2p", 64, 1)])
def test_guess_stage(dtype, n_in, n_out, kernel, nt, per_item):
    """xm_guess_rows and xm_guess_refine inside the small stream, held to the assertions of
    test_gpu_kernels.test_guess_rows_and_refine and to nothing else (see the module's docstring): the estimates of every
    row, the exact arg-max row, its value and its FID, and both keys left zero."""
    import torch

    from xmris_amd import device as dev

    nb = sp.rows_for(nt, per_item)
    rng = np.random.default_rng(n_in + nb)
    t = np.arange(n_in) * 2e-4
    x = 0.02 * (rng.standard_normal((nb, n_in)) + 1j * rng.standard_normal((nb, n_in)))
    x[3] += 1.00 * np.exp((-np.pi * 40.0 + 2j * np.pi * 500.0) * t)
    x[nb - 2] += 0.15 * np.exp((-np.pi * 0.5 + 2j * np.pi * -729.98) * t)
    x = x.astype(dtype)
    w = np.exp(-np.pi * 5.0 * np.arange(n_out) * 2e-4)
    xd = dev.to_device(x)
    w32 = torch.from_numpy(w).to("cuda", torch.float32)
    est = torch.full((nb,), -7.0, dtype=torch.float32, device="cuda")
    gkey, wkey = dev.new_argmax_key("cuda"), dev.new_argmax_key("cuda")
    gmax = torch.zeros(1, dtype=torch.float32, pin_memory=True)
    gflat = torch.zeros(1, dtype=torch.int64, pin_memory=True)
    row = torch.zeros((1, n_in), dtype=torch.complex128, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(sp.stream()):
        assert dev.guess_supported(xd, n_out)
        dev.guess_rows(xd, n_out, w32, est, gkey)
        first = dev.last_kernel()
        dev.guess_refine(xd, n_out, w32, est, gkey, wkey, gmax, gflat, row, band=0.5)
        second = dev.last_kernel()
    torch.cuda.synchronize()
    bound = _rows_checked(first, nb, kernel, per_item)
    if second.startswith("k_zf2p<"):
        _rows_checked(second, nb, "k_zf2p")
    m = min(512, n_in)
    xc = x[:, :m].astype(np.complex128) * w[:m]
    ref_est = (np.abs(np.fft.fft(xc, n=1024, axis=1)) ** 2).max(axis=1) / n_out
    rtol = 2e-3 if n_in >= 512 else 2e-5
    np.testing.assert_allclose(est.cpu().numpy(), ref_est, rtol=rtol)
    full = np.abs(np.fft.fft(x.astype(np.complex128) * w[:n_in], n=n_out, axis=1)) ** 2 / n_out
    true_row = int(np.argmax(full.max(axis=1)))
    if n_in > 512:
        assert true_row == nb - 2 and int(np.argmax(ref_est)) == 3, "the construction must fool the coarse estimate"
    assert int(gflat.item()) == true_row * n_out
    np.testing.assert_allclose(float(gmax.item()), full[true_row].max(), rtol=2e-5)
    assert np.array_equal(row.cpu().numpy()[0], x[true_row].astype(np.complex128))
    assert int(gkey.abs().sum().item()) == 0 and int(wkey.abs().sum().item()) == 0
    print(f"small partition guess stage {dtype} {n_in} -> {n_out}: estimates {float(np.abs(est.cpu().numpy() / ref_est - 1).max()) / rtol:.3f} "
          f"of their bound, the maximum {abs(float(gmax.item()) / full[true_row].max() - 1) / 2e-5:.3f} of its bound")
    _figure(f"guess stage {dtype} {n_in} -> {n_out}", nb, bound, f"{first} | {second}")


# ---- whole calls on the side stream -------------------------------------------------------------------------------------------
# Each builder returns (call, check): call() makes the whole public call -- uploads, tables, temporaries, every launch --
# the way its own GPU file makes it and returns its outputs on the host (names with a leading underscore are carried along
# and not compared); check(outputs) holds them to that file's oracle with that file's tolerance.  The case is the file's
# smallest parity case of the public call (for fit_kinetics, remove_lipids, separate_species, shift_time and grappa_fill
# the file's one public end-to-end case: the layers above the device wrapper are what mixes uploads, downloads and
# launches).  Every kernel involved promises bits that depend on the inputs alone, so the two streams agree bit for bit; a
# piece of the call that ran on another stream than the one it was made on would break either.  The library's cached
# tables are dropped before the second call, so the side stream builds and uploads its own.
def _call_cg_sense():
    import test_gpu_cgsense as g

    c, y, want = g._reference("line1d", "complex128", 6)

    def call():
        ds = g._recon(c, g._up(y), 6)
        return {k: g._down(ds[k].data) for k in ("image", "iterations", "status", "residual")}

    def check(o):
        err = g.orc.rel(o["image"].reshape(c.V, c.T), want)
        print(f"small partition recon_cg_sense line1d: {err / g.CGS_TOL128:.3f} of its bound")
        assert err <= g.CGS_TOL128 and np.all(o["iterations"] == 6) and np.all(o["status"] == 0)

    return call, check


def _call_l1_sense():
    import test_gpu_l1sense as g

    c, y, ref = g._reference("line1d", "complex128")

    def call():
        ds = g._recon(c, g._up(y))
        return {k: g._down(ds[k].data) for k in ("image", "iterations", "status", "change")}

    def check(o):
        err = g.orc.rel(o["image"].reshape(c.V, c.T), ref.x)
        print(f"small partition recon_l1_sense line1d: {err / g.L1_TOL128:.3f} of its bound")
        assert err <= g.L1_TOL128 and np.all(o["iterations"] == 10) and np.all(o["status"] == 0)

    return call, check


def _call_subspace():
    import test_gpu_subspace as g

    p, y, want = g._reference("line1d", 1.0, 1, "complex128")

    def call():
        ds = g._recon(p, g._up(y), sampling=None)
        return {k: g._down(ds[k].data) for k in ("image", "iterations", "status")}

    def check(o):
        err = g.cg.rel(o["image"].reshape(p.c.V, 1, p.T), want)
        print(f"small partition recon_subspace line1d: {err / g.SUB_TOL128:.3f} of its bound")
        assert err <= g.SUB_TOL128 and np.all(o["iterations"] == 6) and np.all(o["status"] == 0)

    return call, check


def _call_espirit_maps():
    import test_gpu_espirit as g

    c = g.orc.case("line1d")
    ref = g.orc.reference("line1d", crop=0.0)

    def call():
        ds = g.labeled_acs(c).xmr.espirit_maps(c.mat, kernel=c.kernel, dims=g.K_DIMS[:c.d], threshold=c.threshold, crop=0.0,
                                               n_maps=2, return_eigenvalues=True)
        return dict(maps=np.asarray(ds["maps"].values), eigenvalues=np.asarray(ds["eigenvalues"].values),
                    status=np.asarray(ds["status"].values), _ds=ds)

    def check(o):
        assert not o["status"].any() and o["_ds"].attrs["n_kernels"] == ref["n_kernels"]
        dv, dm = g.compare_with_oracle(c, o["_ds"], ref)
        print(f"small partition espirit_maps line1d: values {dv / g.value_tol(c.C):.3f} of their bound, first map {dm / g.map_tol(c.C):.3f} of its bound")

    return call, check


def _call_grappa_fill():
    import test_gpu_grappa as g

    from xmris_amd import LabeledArray
    from xmris_amd import device as dev

    name = "16x16_r2x2_b2x2_c12"  # .xmr.grappa_fill from an ACS block: calibration, the weights' upload and the fill
    cs = g.orc.e2e_case(name)
    coords = {"kx": (g.orc.kept_lines(16, 2) - 16) * 0.5, "ky": (g.orc.kept_lines(16, 2) - 16) * 0.25}
    kept = cs["kept"].astype(np.complex64)

    def call():
        la = LabeledArray(kept, ("coil", "kx", "ky", "time"), coords, {"MHz": 120.0})
        out, rec = la.xmr.grappa_fill(acs=LabeledArray(cs["acs"], ("coil", "kx", "ky", "time")), accel=(2, 2),
                                      regularization=cs["lam"], return_weights=True)
        assert "k_grappa_fill" in dev.last_kernel()
        return dict(y=out.values, weights=np.array(rec.weights))

    def check(o):
        want = g.orc.fill(kept.astype(np.complex128), o["weights"], (2, 2), (2, 2))
        g.check(o["y"], want, np.complex64, what=f"small partition grappa_fill {name}")

    return call, check


def _call_to_image():
    import test_gpu_mrsi as g
    import xmris_amd

    dla, host, kw, fn, want, u, d = g._device_case("odd_7_to_16", "complex128")
    return (lambda: dict(y=getattr(xmris_amd, fn)(dla, **kw).values),
            lambda o: g._report("small partition to_image odd_7_to_16", o["y"], want, g.bound(u, "complex128", d)))


def _call_remove_water():
    import test_gpu_hsvd as g

    x, _, _ = g.orc.make_fid(256, 1, 6)
    want = g.orc.hsvd_rows(x, 32, 8)

    def call():
        ds = g._labeled(x.reshape(2, 3, 256), ("x", "y", "time"), MHz=300.0).xmr.remove_water(rank=8, n_cols=32, return_components=True)
        got = {k: ds[k].values.reshape((6,) + ds[k].shape[2:]) for k in g.OUT[1:]}
        got["y"] = ds["cleaned"].values.reshape(6, 256)
        return got

    return call, lambda o: g._check(dict(o, kernel="remove_water"), want, x, what="small partition remove_water")


def _call_fit_kinetics():
    import test_gpu_kinetics as g

    import xmris_amd as xm
    from xmris_amd import device as dev
    from xmris_amd.fitting import LabeledDataset

    # xm.fit_kinetics on a fitted dataset, the case of test_gpu_kinetics.test_public_call_end_to_end: the layer derives the
    # weights from the CRLBs, the starts and the flip-angle tables, uploads them and reshapes the results
    T = 30
    c = g.orc.kinetic_case(T, 2, 500, n_vox=15)
    amp = np.zeros((5, 3, T, 3))
    amp[..., 0] = c["S"].reshape(5, 3, T)
    amp[..., 1:] = np.moveaxis(c["Y"], 1, 2).reshape(5, 3, T, 2)
    crlb = np.full(amp.shape, 2.0)
    crlb[2, 1, 9, 1] = np.nan  # a failed repetition
    dims = ("x", "y", "repetition", "Metabolite")
    coords = {"repetition": c["t"], "Metabolite": np.array(["pyruvate", "lactate", "alanine"])}
    flips = {"pyruvate": np.rad2deg(c["ths"]), "lactate": np.rad2deg(c["thp"][0]), "alanine": np.rad2deg(c["thp"][1])}
    keys = ("rate", "rate_sd", "decay", "decay_sd", "auc_ratio", "status", "fit")

    def call():
        ds = LabeledDataset({"amplitude": xm.LabeledArray(amp.copy(), dims, coords), "crlb": xm.LabeledArray(crlb.copy(), dims, coords)})
        kin = xm.fit_kinetics(ds, "pyruvate", ["lactate", "alanine"], flip_angle=flips, r1=(1 / 60, 1 / 10))
        assert "k_kinetics_fit" in dev.last_kernel()
        return {k: np.array(kin[k].values) for k in keys}

    def check(o):
        assert np.all(o["status"] == 0)
        z = np.abs(o["rate"] - c["truth"][:, 0]) / o["rate_sd"]
        zd = np.abs(o["decay"] - c["truth"][:, 1]) / o["decay_sd"]
        print(f"small partition fit_kinetics: worst |k - truth| / rate_sd {z.max() / 6.0:.3f} of its bound, decay {zd.max() / 6.0:.3f}")
        assert z.max() < 6.0 and zd.max() < 6.0
        # the numbers of the raw call with the weights the layer derives, and that call's outputs from its parameters
        w = 1.0 / (0.02 * np.abs(c["Y"]))
        w[2 * 3 + 1, 0, 9] = 0.0
        init = c["init"].copy()
        init[:, 0] = 0.1
        raw = g._fit(dict(c, w=w), init=init)
        assert np.array_equal(o["rate"].reshape(15, 2), raw["params"][..., 0])
        assert np.array_equal(o["auc_ratio"].reshape(15, 2), raw["auc_ratio"])
        n, share = g._check_invariants(raw, dict(c, w=w), 200, over=dict(init=init))
        print(f"small partition fit_kinetics: {n} rows, invariants at {share:.3f} of their bounds")

    return call, check


def _call_remove_lipids():
    import test_gpu_lipids as g

    from xmris_amd import Coordinate, LabeledArray
    from xmris_amd import device as dev

    # .xmr.remove_lipids with a mask on the phantom of test_public_call_and_accessor_on_the_phantom: the lipid rows are
    # gathered, their Gram matrix is formed on the device and downloaded, the basis is built and uploaded, then projected
    ph = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in g.orc.phantom().items()}  # (the phantom is read-only)
    data = ph["data"].astype(np.complex128)
    coords = {d: Coordinate(d, np.arange(n, dtype=np.float64)) for d, n in zip(("y", "x", "time"), data.shape)}
    ref, b = g.orc.remove(data, ph["scalp"], 0.01, None, apply_mask=ph["brain"])

    def call():
        fid = LabeledArray(data.copy(), ("y", "x", "time"), coords, {}, "fid")
        out, rec, status = fid.xmr.remove_lipids(ph["scalp"], dims=("y", "x"), apply_mask=ph["brain"], return_basis=True)
        assert "k_lipid_project" in dev.last_kernel()
        return dict(out=dev.to_host(out.data), status=dev.to_host(status.data), vectors=np.array(rec.vectors),
                    weights=np.array(rec.weights), _rank=rec.rank)

    def check(o):
        assert o["_rank"] == b["rank"] and np.array_equal(o["status"], np.where(ph["brain"], 0, 1))
        span = np.abs(g.orc.projector(o["vectors"], o["weights"]) - g.orc.projector(b["U"], b["w"])).max()
        bound = (g.TOL + 16 * 1.202e-12) * np.abs(data).max(axis=-1, keepdims=True)
        share = float((np.abs(o["out"] - ref) / bound).max())
        print(f"small partition remove_lipids phantom: {share:.3f} of its bound, the basis' projector {span / (16 * 1.202e-12):.3f} of its bound")
        assert share <= 1.0 and span <= 16 * 1.202e-12
        assert np.array_equal(g._bits(o["out"][~ph["brain"]]), g._bits(data[~ph["brain"]]))

    return call, check


def _call_separate_species():
    import test_gpu_species as g

    from xmris_amd import LabeledArray
    from xmris_amd import device as dev

    # .xmr.separate_species, the case of test_accessor_on_a_device_resident_array: with a given field (tables, the field
    # and the delays uploaded per call) and with the field fitted
    F, te, rho, tau, psi, raw = g._public_case()
    delta, _ = g.orc.grid(te, 45.0)

    def call():
        da = LabeledArray(dev.to_device(np.array(raw.values)), raw.dims, raw.coords, raw.attrs)
        out = da.xmr.separate_species(F, decay=[3.0, 9.0], readout_time=tau, field_map=psi)
        assert "k_species" in dev.last_kernel()
        ds = da.xmr.separate_species(F, decay=[3.0, 9.0], readout_time=tau, fit_field=True, max_field=45.0, return_field=True)
        return dict(species=np.array(out.values), fitted=np.array(ds["species"].values), field=np.array(ds["field"].values),
                    residual=np.array(ds["residual"].values), status=np.array(ds["status"].values))

    def check(o):
        err = np.abs(o["species"] - rho).max() / (g.A_TOL * np.abs(rho).max())
        gap = np.abs(o["field"] - psi).max() / (g.B_TOL * delta)
        print(f"small partition separate_species: given field {err:.3f} of its bound, fitted field {gap:.3f} of its bound")
        assert err <= 1.0 and gap <= 1.0 and np.all(o["status"] == 0)

    return call, check


def _call_shift_time():
    import test_gpu_shift as g

    from xmris_amd import LabeledArray, readout_offsets
    from xmris_amd import device as dev
    from xmris_amd.processing.timeshift import shift_time

    # processing.timeshift.shift_time with one delay per sample, the data of test_gpu_shift.test_correct_readout_time
    dt = 0.5e-3
    x = g.orc.make((2, 5, 256), seed=3, dtype="complex128")
    t = np.arange(256) * dt
    off = readout_offsets(5, 0.2 * dt, start=0.05 * dt)
    want = g.orc.shift_fft(x, off[None, :] / dt)

    def call():
        y = shift_time(LabeledArray(x.copy(), ("coil", "sample", "time"), {"time": t}, {}, "fid"), off[None, :])
        assert dev.last_kernel().startswith("k_shift_time<")
        return dict(y=np.array(y.values))

    def check(o):
        share = g.orc.row_gap(o["y"], want).max() / g.bound("complex128")
        print(f"small partition shift_time: {share:.3f} of its bound")
        assert share <= 1.0

    return call, check


WHOLE_CALLS = {"recon_cg_sense": _call_cg_sense, "recon_l1_sense": _call_l1_sense, "recon_subspace": _call_subspace,
               "espirit_maps": _call_espirit_maps, "grappa_fill": _call_grappa_fill, "to_image": _call_to_image,
               "remove_water": _call_remove_water, "fit_kinetics": _call_fit_kinetics, "remove_lipids": _call_remove_lipids,
               "separate_species": _call_separate_species, "shift_time": _call_shift_time}


@pytest.mark.parametrize("name", list(WHOLE_CALLS))
def test_whole_call(name):
    import torch

    from xmris_amd import _lib

    call, check = WHOLE_CALLS[name]()
    side = sp.stream()
    torch.cuda.synchronize()
    a = call()
    torch.cuda.synchronize()
    _lib.call("xm_clear_cache")  # (nothing is queued: the tables the first call built are freed, the next builds them anew)
    with torch.cuda.stream(side):
        b = call()
    torch.cuda.synchronize()
    for k in a:
        if not k.startswith("_") and a[k] is not None:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (name, k)
    check(b)
