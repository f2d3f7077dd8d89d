"""k_amares_fit<true> / xm_amares_fit_linked on the GPU against tests/_amares_links.py: invariants of every returned
voxel, the first trial steps, MINPACK parity, a degenerate doublet, the no-link equivalence, the ABI's refusals and
.xmr.fit_amares with a linked CSV.  The cases are lk.gpu_cases(), selected on the CPU in tests/test_amares_links.py."""
import functools
import os

import numpy as np
import pytest

import _amares_links as lk
import _amares_oracle as orc
from test_amares_kernel import STEP_RSS_TOL, STEP_TOL  # 16 x the 1.32e-8 of tests/tool_amares_tolerance.py

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
HERE = os.path.dirname(os.path.abspath(__file__))
PK_MULTI = os.path.join(HERE, "golden", "amares_pk_p31_multiplets.csv")
STEP_M = (1, 2, 3, 5)
OUT = ("params", "amp_sd", "rss", "status", "iters")


@functools.lru_cache(maxsize=None)
def _cases():
    return lk.gpu_cases()


def _fit(x, c, max_iter=200, want_fit=True, links="case"):
    import torch
    from xmris_amd import device as dev

    r = dev.amares_fit(torch.from_numpy(np.ascontiguousarray(x)).to("cuda"), 1, c["init"], c["lo"], c["hi"], c["fixed"],
                       dt=c["dt"], t0=c["t0"], max_iter=max_iter, want_fit=want_fit,
                       links=c["links"] if links == "case" else links)
    out = {k: getattr(r, k).cpu().numpy() for k in OUT}
    out["fit"] = r.fit.cpu().numpy() if want_fit else None
    out["n_free"], out["kernel"] = r.n_free, dev.last_kernel()
    return out


def _same(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in OUT + ("fit",) if a[k] is not None)


def _check_invariants(out, x, c):
    """Every output of a voxel recomputed from its returned parameters; the links hold to one rounding."""
    t, lo, hi, links = c["t"], c["lo"], c["hi"], c["links"]
    L = lk._Layout(c["init"], lo, hi, c["fixed"], links)
    to, sc, off = L.to, L.sc, L.off
    follower = np.flatnonzero(L.linked & (L.col >= 0))
    root_free = L.free
    assert out["n_free"] == root_free.size and "k_amares_fit<true" in out["kernel"]
    for v in range(x.shape[0]):
        assert out["status"][v] in (0, 1), (v, out["status"][v])
        p = out["params"][v].ravel()
        assert np.all(np.isfinite(p))
        # fused against unfused multiply-add
        want = sc[follower] * p[to[follower]] + off[follower]
        gap = np.abs(p[follower] - want)
        assert np.all(gap <= EPS * (np.abs(sc[follower] * p[to[follower]]) + np.abs(off[follower]))), (v, gap.max())
        assert np.array_equal(p[L.fixed_all], L.v0[L.fixed_all]), (v, "a fixed parameter or fixed follower moved")
        assert np.all((p[root_free] >= L.lo[root_free]) & (p[root_free] <= L.hi[root_free])), (v, "root out of bounds")
        ref = orc.model(p, t)
        assert np.abs(out["fit"][v] - ref).max() <= 1e-12 * np.abs(ref).max(), (v, "fit")
        rss = float(np.sum(np.abs(x[v].astype(np.complex128) - ref) ** 2))
        assert abs(out["rss"][v] - rss) <= 1e-9 * rss, (v, "rss", out["rss"][v], rss)
        sd, cond = lk.amplitude_sd_linked(t, p, lo, hi, c["fixed"], links)
        bound = 64 * EPS * cond
        assert bound < 1.0, (v, cond)
        got = out["amp_sd"][v]
        has = L.col[0::5] >= 0
        assert np.all(got[~has] == 0.0)
        err = np.abs(got[has] - sd[has]) / sd[has]
        assert np.all(err <= bound), (v, "amp_sd", err.max(), bound)
        assert 0 < out["iters"][v] <= 200


# ---- 1. invariants ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(lk.gpu_cases()))
def test_outputs_follow_from_returned_parameters(name):
    c = _cases()[name]
    for max_iter in (1, 3, 200):
        out = _fit(c["x"], c, max_iter=max_iter)
        _check_invariants(out, c["x"], c)
        assert np.all(out["iters"] <= max_iter)
        if max_iter == 200 and name != "doublet_root_on_bound":
            assert np.all(out["status"] == 0), out["status"]
    # complex64 samples are widened on load: bitwise what the host-widened samples give
    x32 = c["x"].astype(np.complex64)
    a, b = _fit(x32, c), _fit(x32.astype(np.complex128), c)
    assert _same(a, b) and not _same(a, out)
    _check_invariants(a, x32, c)


def test_fixed_root_makes_fixed_followers_bitwise():
    """Peak 1's damping fixed through lo == hi: peak 0's follows at scale * value + offset exactly and has no column."""
    c = dict(_cases()["doublet_K3_n64"])
    lo, hi, init = c["lo"].copy(), c["hi"].copy(), c["init"].copy()
    lo[1, 2] = hi[1, 2] = init[1, 2] = 27.5
    links = tuple(a.copy() for a in c["links"])
    links[1][0, 2], links[2][0, 2] = 1.3, 0.7
    c.update(lo=lo, hi=hi, init=init, links=links)
    out = _fit(c["x"], c)
    assert out["n_free"] == 7
    assert np.all(out["params"][:, 1, 2] == 27.5) and np.all(out["params"][:, 0, 2] == 1.3 * 27.5 + 0.7)
    _check_invariants(out, c["x"], c)


@pytest.mark.parametrize("dtype", ["complex64", "complex128"])
def test_strided_rows_through_the_c_abi(dtype):
    """in_row_stride = n + 24, the first row 5 elements into the buffer, fit_data null; K = 9, n = 300."""
    import torch
    from xmris_amd import _lib

    c = _cases()["multiplets_K9_n300"]
    nb, n = c["x"].shape
    stride = n + 24
    rng = np.random.default_rng(n)
    wide = (1e3 * (rng.standard_normal((nb, stride)) + 1j * rng.standard_normal((nb, stride)))).astype(dtype)
    wide[:, 5:5 + n] = c["x"].astype(dtype)
    x = np.ascontiguousarray(wide[:, 5:5 + n])
    wd = torch.from_numpy(wide).to("cuda")
    code = _lib.XM_C64 if dtype == "complex64" else _lib.XM_C128
    got = _raw(wd.data_ptr() + 5 * wd.element_size(), stride, nb, c, code, c["links"])[1]
    ref = _fit(x, c, want_fit=False)
    assert all(np.array_equal(got[k], ref[k], equal_nan=True) for k in OUT)


# ---- 2. the first trial steps ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", lk.STEP_CASES)
def test_first_steps_match_the_restated_iteration(name):
    """params, rss, iters and status after m = 1, 2, 3, 5 trials against lk.lm_steps_linked with the same cap; per
    parameter the disagreement is bounded in units of its path length.  A group whose root starts on a two-sided bound
    does not move, bit for bit."""
    c = _cases()[name]
    L = lk._Layout(c["init"], c["lo"], c["hi"], c["fixed"], c["links"])
    for m in STEP_M:
        out = _fit(c["x"], c, max_iter=m, want_fit=False)
        for v in range(c["x"].shape[0]):
            ref = lk.lm_steps_linked(c["x"][v], c["t"], c["init"], c["lo"], c["hi"], c["fixed"], c["links"], max_iter=m)
            assert not any(abs(margin) < 1e-9 for _, margin in ref["trials"])  # (asserted on the CPU for every case)
            assert out["iters"][v] == ref["iters"] == m and out["status"][v] == ref["status"] == 1, (m, v)
            d = np.abs(out["params"][v].ravel() - ref["params"].ravel())
            worst = np.max(np.where(ref["path"] > 0, d / np.where(ref["path"] > 0, ref["path"], 1.0), 0.0))
            print(f"{name} m={m} voxel {v}: worst |dp| / path {worst:.3e} (bound {STEP_TOL:.3e}), rss rel "
                  f"{abs(out['rss'][v] - ref['rss']) / ref['rss']:.3e}")
            assert np.all(d <= STEP_TOL * ref["path"]), (m, v, worst)
            assert abs(out["rss"][v] - ref["rss"]) <= STEP_RSS_TOL * ref["rss"], (m, v)
            if name == "doublet_root_on_bound":
                f_root = c["hi"][1, 1]
                assert ref["path"][6] == 0.0 and ref["path"][1] == 0.0
                assert out["params"][v, 1, 1] == ref["params"][1, 1] == L.physical(L.u0)[0][6]
                assert abs(out["params"][v, 1, 1] - f_root) <= EPS * abs(f_root)
                assert out["params"][v, 0, 1] == out["params"][v, 1, 1] - 17.0  # exact: scale 1, one rounding


# ---- 3. MINPACK parity ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", lk.PARITY_CASES)
def test_converged_fit_matches_minpack(name):
    c = _cases()[name]
    out = _fit(c["x"], c)
    assert out["n_free"] == lk.n_columns(c) and np.all(out["status"] == 0)
    for v in range(c["x"].shape[0]):
        o = lk.fit_linked(c["x"][v], c["t"], c["init"], c["lo"], c["hi"], c["fixed"], c["links"])
        assert o["ier"] in (1, 2, 3, 4) and o["n_free"] == out["n_free"]
        free = o["sd"] > 0
        dev_ = np.abs(out["params"][v] - o["params"])
        assert np.all(dev_[free] <= 1e-3 * o["sd"][free]), (v, (dev_[free] / o["sd"][free]).max())
        assert abs(out["rss"][v] - o["rss"]) <= 1e-9 * o["rss"], (v, out["rss"][v], o["rss"])


# ---- 4. a doublet without signal ------------------------------------------------------------------------------------------
def test_doublet_root_amplitude_at_zero():
    """The doublet's amplitude root starts on its bound 0 and stays (slope 0): root and follower are exactly 0, J^T J is
    singular and amp_sd is NaN for both lines (and every amplitude with a column); an empty voxel in the batch changes
    nothing for its neighbours."""
    c = dict(_cases()["doublet_K3_n64"])
    init = c["init"].copy()
    init[1, 0] = 0.0
    c["init"] = init
    good = c["x"][:4]
    big = np.concatenate([good[:1], np.zeros((1, good.shape[1]), complex), good[1:]])
    base, out = _fit(good, c), _fit(big, c)
    keep = [0, 2, 3, 4]
    for k in OUT + ("fit",):
        assert np.array_equal(out[k][keep], base[k], equal_nan=True), k  # bitwise
    assert np.all(np.isin(out["status"], (0, 1))) and np.all(np.isfinite(out["params"])) and np.all(np.isfinite(out["rss"]))
    assert np.all(out["params"][:, 1, 0] == 0.0) and np.all(out["params"][:, 0, 0] == 0.0)
    assert np.all(np.isnan(out["amp_sd"]))
    for v in range(big.shape[0]):
        ref = orc.model(out["params"][v], c["t"])
        assert np.abs(out["fit"][v] - ref).max() <= 1e-12 * max(np.abs(ref).max(), 1e-300)
    # the empty voxel from a start inside the bounds: it ends with a status and finite parameters, and the two lines of
    # the doublet are judged alike -- both undefined, or the follower's deviation |scale| times the root's
    c2 = _cases()["doublet_K3_n64"]
    e = _fit(big, c2)
    assert e["status"][1] in (0, 1) and np.all(np.isfinite(e["params"][1])) and np.isfinite(e["rss"][1])
    a0, a1 = e["amp_sd"][1, 0], e["amp_sd"][1, 1]
    assert (np.isnan(a0) and np.isnan(a1)) or a0 == 0.5 * a1
    base2 = _fit(good, c2)
    assert all(np.array_equal(e[k][keep], base2[k], equal_nan=True) for k in OUT)


# ---- 5. / 6. the C ABI ------------------------------------------------------------------------------------------------------
def _raw(first_ptr, stride, nb, c, code, links, func="xm_amares_fit_linked", work=None, outs=None):
    import torch
    from xmris_amd import _lib

    K, n = c["init"].shape[0], len(c["t"])
    o = outs or {"params": torch.empty((nb, K, 5), dtype=torch.float64, device="cuda"),
                 "amp_sd": torch.empty((nb, K), dtype=torch.float64, device="cuda"),
                 "rss": torch.empty(nb, dtype=torch.float64, device="cuda"),
                 "status": torch.empty(nb, dtype=torch.int32, device="cuda"),
                 "iters": torch.empty(nb, dtype=torch.int32, device="cuda")}
    work = torch.zeros(64, dtype=torch.int32, device="cuda") if work is None else work
    host = [np.ascontiguousarray(c[k], dtype=np.float64) for k in ("init", "lo", "hi")]
    fixed = np.ascontiguousarray(c["fixed"], dtype=np.int32)
    extra = []
    if func == "xm_amares_fit_linked":
        extra = [np.ascontiguousarray(links[0], dtype=np.int32), np.ascontiguousarray(links[1], dtype=np.float64),
                 np.ascontiguousarray(links[2], dtype=np.float64)]
    rc = getattr(_lib.load(), func)(first_ptr, stride, nb, n, float(c["dt"]), float(c["t0"]), K,
                                    *[a.ctypes.data for a in host], fixed.ctypes.data, *[a.ctypes.data for a in extra],
                                    200, 1e-10, 1e-10, o["params"].data_ptr(), o["amp_sd"].data_ptr(),
                                    o["rss"].data_ptr(), o["status"].data_ptr(), o["iters"].data_ptr(), None,
                                    work.data_ptr(), work.numel() * work.element_size(), code,
                                    torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in o.items()}, work.cpu().numpy()


def test_no_links_is_xm_amares_fit_bitwise():
    import torch
    from xmris_amd import _lib
    from xmris_amd import device as dev

    c = orc.kernel_case(7, 1000, 42, n_vox=5)
    xd = torch.from_numpy(c["x"]).to("cuda")
    rc0, plain, _ = _raw(xd.data_ptr(), 1000, 5, c, _lib.XM_C128, None, func="xm_amares_fit")
    assert "k_amares_fit<false" in dev.last_kernel()
    rc1, linked, work = _raw(xd.data_ptr(), 1000, 5, c, _lib.XM_C128, lk.no_links(7))
    assert rc0 == rc1 == 0 and "k_amares_fit<false" in dev.last_kernel() and not work.any()
    for k in OUT:
        assert np.array_equal(plain[k], linked[k], equal_nan=True), k
    assert np.all(plain["status"] == 0)


def test_abi_refusals_launch_nothing():
    import torch
    from xmris_amd import _lib

    lib = _lib.load()
    c = _cases()["doublet_K3_n64"]
    nb, n = c["x"].shape
    xd = torch.from_numpy(c["x"]).to("cuda")
    outs = {"params": torch.full((nb, 3, 5), -7.0, dtype=torch.float64, device="cuda"),
            "amp_sd": torch.full((nb, 3), -7.0, dtype=torch.float64, device="cuda"),
            "rss": torch.full((nb,), -7.0, dtype=torch.float64, device="cuda"),
            "status": torch.full((nb,), -7, dtype=torch.int32, device="cuda"),
            "iters": torch.full((nb,), -7, dtype=torch.int32, device="cuda")}
    work = torch.zeros(64, dtype=torch.int32, device="cuda")

    def bad(i, k, col, value, text):
        links = tuple(a.copy() for a in c["links"])
        links[i][k, col] = value
        rc, got, w = _raw(xd.data_ptr(), n, nb, c, _lib.XM_C128, links, work=work, outs=outs)
        assert rc == _lib.XM_ERR_INVALID_ARG and text.encode() in lib.xm_last_error_string(), (text, rc)
        assert all(np.all(a == -7) for a in got.values()) and not w.any(), text

    bad(0, 2, 0, 15, "out of range")
    bad(0, 2, 0, 6, "another kind")
    bad(0, 2, 0, 10, "itself")
    bad(0, 2, 0, 0, "itself linked")
    bad(1, 0, 0, 0.0, "link_scale")
    bad(1, 0, 0, np.nan, "link_scale")
    bad(2, 0, 1, np.inf, "link_offset")
    short = dict(c, t=c["t"][:7])  # n = 7 < P = 8
    rc, got, w = _raw(xd.data_ptr(), n, nb, short, _lib.XM_C128, c["links"], work=work, outs=outs)
    assert rc == _lib.XM_ERR_INVALID_ARG and b"smaller than the free parameters (8)" in lib.xm_last_error_string()
    assert all(np.all(a == -7) for a in got.values()) and not w.any()
    rc, got, w = _raw(xd.data_ptr(), n, nb, c, _lib.XM_C128, c["links"], work=work, outs=outs)  # and the valid table runs
    assert rc == 0 and np.all(got["status"] == 0) and not w.any()


# ---- 7. end to end ------------------------------------------------------------------------------------------------------------
def test_fit_amares_with_the_multiplet_csv():
    import xmris_amd as xm

    mhz, sw, n, nv = 120.0, 10000.0, 512, 8
    init, lo, hi, fixed, links = lk.multiplet_pk(mhz)
    E, b, roots = lk.expansion(links, 9)
    rng = np.random.default_rng(11)
    data = np.zeros((nv, n), complex)
    for v in range(nv):
        p = init.copy()
        p[:, 0] *= rng.uniform(0.7, 1.3, 9)
        p[:, 1] += rng.uniform(-0.1, 0.1, 9) * mhz
        p[:, 2] *= rng.uniform(0.85, 1.15, 9)
        p[:, 3] = rng.uniform(-0.3, 0.3)
        p = (E @ p.ravel()[roots] + b).reshape(9, 5)  # linked truth
        fid = xm.simulate_fid(amplitudes=p[:, 0], frequencies=p[:, 1], spectral_width=sw, n_points=n,
                              dampings=p[:, 2], phases=p[:, 3], lineshape_g=0.0)
        data[v] = np.asarray(fid.values) + 0.2 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    t = np.arange(n) / sw
    da = xm.LabeledArray(data, ("voxel", "time"), {"time": t}, {"MHz": mhz})
    ds = da.xmr.fit_amares(PK_MULTI)
    assert ds.attrs["n_free_parameters"] == 20
    assert list(ds.coords["Metabolite"].values) == list(lk.MULTIPLET_NAMES)  # one entry per CSV column
    amp, ppm, lw, ph = (np.asarray(ds[k].values) for k in ("amplitude", "chem_shift", "linewidth", "phase"))
    crlb = np.asarray(ds["crlb"].values)
    assert np.all(np.isfinite(crlb)) and np.all(crlb > 0)
    for follower, root, ratio, hz in ((3, 2, 1.0, -16.0), (5, 4, 1.0, -16.0), (7, 6, 2.0, -16.0), (8, 6, 1.0, -32.0)):
        assert np.array_equal(amp[:, follower], ratio * amp[:, root])  # scale 1 or 2, no offset: exact
        f_root, f_fol = ppm[:, root] * mhz, ppm[:, follower] * mhz  # through / mhz and back: a few roundings
        assert np.all(np.abs(f_fol - (f_root + hz)) <= 4 * EPS * (np.abs(f_root) + abs(hz)))
        assert np.array_equal(lw[:, follower], lw[:, root]) and np.array_equal(ph[:, follower], ph[:, root])
        np.testing.assert_allclose(crlb[:, follower], crlb[:, root], rtol=4 * EPS, atol=0)
    # and it is the fit the oracle finds
    for v in (0, 7):
        o = lk.fit_linked(data[v], t, init, lo, hi, fixed, links)
        free = o["sd"][:, 0] > 0
        assert np.all(np.abs(amp[v] - o["params"][:, 0])[free] <= 1e-3 * o["sd"][:, 0][free])
        np.testing.assert_allclose(crlb[v], o["crlb"], rtol=1e-3)
