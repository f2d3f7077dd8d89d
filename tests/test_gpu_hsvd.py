"""k_hsvd / xm_hsvd_rows / .xmr.remove_water on the GPU against tests/_hsvd_oracle.py.  The shapes are
orc.PARITY_CASES, whose conditions (the same in-band set on both routes, no pole near a band edge, status 0,
cond(B) <= 1e4) and route agreement are checked on the CPU in tests/test_hsvd.py."""
import functools

import numpy as np
import pytest

import _hsvd_oracle as orc
from test_hsvd import COMB_TOL, HSVD_TOL, MODEL_RESIDUAL  # 16 x the routes' disagreement and 16 x the oracle's distance
# from the closed form; the oracle's model residuals -- tests/tool_hsvd_tolerance.py

pytestmark = pytest.mark.gpu

HALF32 = 2.0 ** -24  # one rounding of an fp32 value, relative
OUT = ("y", "frequency", "damping", "amplitude", "phase", "removed", "n_removed", "status")


def _up(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _run(x, m, k, band=orc.BAND, dt=orc.DT, **kw):
    from xmris_amd import device as dev

    r = dev.hsvd_rows(x if hasattr(x, "is_cuda") else _up(x), -1, m, k, dt, band, **kw)
    host = lambda t: None if t is None else t.cpu().numpy()  # noqa: E731
    out = {key: host(getattr(r, key)) for key in OUT}
    out["kernel"] = dev.last_kernel()
    return out


def _same(a, b, keys=OUT):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in keys)


def _check(got, want, x, c64=False, what=""):
    """y within HSVD_TOL["y"] max |x| (complex64: plus one fp32 rounding of y), the in-band poles and amplitudes within
    HSVD_TOL in their units, removed / n_removed / status equal."""
    g = orc.gap(want, orc.with_poles(got), x)
    tol_y = HSVD_TOL["y"] + (np.sqrt(2.0) * HALF32 * float((np.abs(want["y"]).max(axis=-1) / np.abs(x).max(axis=-1)).max()) if c64 else 0.0)
    print(f"{what}: y {g['y']:.2e} of max|x| (bound {tol_y:.1e}), f {g['f']:.2e} ({HSVD_TOL['f']:.1e}), d {g['d']:.2e} "
          f"({HSVD_TOL['d']:.1e}), a {g['a']:.2e} ({HSVD_TOL['a']:.1e}); {got['kernel']}")
    assert np.array_equal(got["status"], want["status"]), got["status"]
    assert np.array_equal(got["removed"], want["removed"]) and np.array_equal(got["n_removed"], want["n_removed"])
    assert g["y"] <= tol_y and g["f"] <= HSVD_TOL["f"] and g["d"] <= HSVD_TOL["d"] and g["a"] <= HSVD_TOL["a"], (what, g)
    return g


@functools.lru_cache(maxsize=None)
def _case(name, dtype):
    x, _, m, k = orc.parity_case(name)
    x = x.astype(dtype)
    return x, m, k, orc.hsvd_rows(x.astype(np.complex128), m, k)


# ---- 1. parity ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["complex128", "complex64"])
@pytest.mark.parametrize("name", list(orc.PARITY_CASES))
def test_parity_with_the_oracle(name, dtype):
    x, m, k, want = _case(name, dtype)
    got = _run(x, m, k)
    assert got["y"].dtype == np.dtype(dtype) and f"k_hsvd<mfma, {m}, {k}>" in got["kernel"]
    _check(got, want, x.astype(np.complex128), c64=dtype == "complex64", what=f"{name} {dtype}")


@pytest.mark.parametrize("name", ["N7-M3-K2", "N33-M16-K2", "N257-M17-K16", "N255-M63-K20", "N2048-M64-K20"])
def test_matrix_core_and_fma_gram_agree(name):
    x, m, k, want = _case(name, "complex128")
    a, b = _run(x, m, k), _run(x, m, k, _gram_fma=True)
    assert "k_hsvd<fma" in b["kernel"]
    _check(b, want, x, what=f"{name} fma")
    g = orc.gap(orc.with_poles(a), orc.with_poles(b), x)
    print(f"{name}: mfma against fma: {g}")
    assert all(g[key] <= HSVD_TOL[key] for key in HSVD_TOL), g


# ---- 1b. the pole solver on matrices with exact zeros: against the oracle and against the closed form -------------------
@functools.lru_cache(maxsize=None)
def _comb(name, dtype):
    x, m, k, band, z, a, k0, y = orc.comb_case(name)
    xs = x.astype(dtype)[None]
    return xs, m, k, band, orc.hsvd_rows(xs.astype(np.complex128), m, k, band=band), (z, a, k0, y)


_FMA_COMBS = ("P2-M4-N16-rho0.9", "P16-M17-N67-rho0.8", "P32-M64-N320-rho0.8", "P32-M64-N320-rho1.0",
              "P5-M16-N64-rho0.9-real")
_COMB_RUNS = [(n, d, False) for n in orc.VALUE_CASES for d in ("complex128", "complex64")] + \
             [(n, d, True) for n in _FMA_COMBS for d in ("complex128", "complex64")]


@pytest.mark.parametrize("name, dtype, fma", _COMB_RUNS)
def test_sparse_combs_against_the_oracle_and_the_closed_form(name, dtype, fma):
    """orc.VALUE_CASES: Q is a weighted cyclic permutation with exact zeros (hs_hessenberg's sigma == 0, hs_qr's
    tst == 0 and exceptional shift; tests/test_hsvd.py shows which case enters which, and that the real-valued combs do
    not converge without the exceptional shift), or, for the one GRID_CASES entry, unitary with degenerate groups, where
    the restated iteration deflates mid-matrix (l > 0).  The kernel's basis inside a degenerate eigenvalue group of G may
    differ from the restatement's, so l > 0 on the GPU is likely, not proven."""
    xs, m, k, band, want, (z, a, k0, y) = _comb(name, dtype)
    got = _run(xs, m, k, band=band, _gram_fma=fma)
    assert got["y"].dtype == np.dtype(dtype) and f"k_hsvd<{'fma' if fma else 'mfma'}, {m}, {k}>" in got["kernel"]
    assert got["status"][0] == 0 and got["n_removed"][0] == 1 and got["removed"][0][k0] == 1
    what = f"{name} {dtype}{' fma' if fma else ''}"
    _check(got, want, xs.astype(np.complex128), c64=dtype == "complex64", what=what)
    if dtype == "complex128":
        r = orc.with_poles({key: got[key][0] for key in OUT})
        tg = orc.truth_gap(r, xs[0], z, a, k0, y)
        print(f"{what}: against the closed form: pole {tg['pole']:.2e} ({COMB_TOL['pole']:.1e}), amp {tg['amp']:.2e} "
              f"({COMB_TOL['amp']:.1e}), sig {tg['sig']:.2e} ({COMB_TOL['sig']:.1e})")
        assert all(tg[key] <= COMB_TOL[key] for key in COMB_TOL), (what, tg)


# ---- 1c. where parity is undefined: the outputs follow from the components returned -------------------------------------
@pytest.mark.parametrize("name", list(orc.MODEL_CASES))
def test_outputs_follow_from_the_returned_components(name):
    """Noise-free, K the true number of components: clustered poles, a dynamic range of 1e6, a real-valued FID, a
    growing pole.  y = x - sum over the removed components, rebuilt in numpy from the arrays the kernel returned; the angle
    t arg z rounded costs eps pi t, the rest a few eps: 16 eps (1 + pi N) max_t sum_k |a_k| |z_k|^t.  The full model's
    residual within 16 x the larger of the oracle's two routes' (tests/test_hsvd.py MODEL_RESIDUAL)."""
    x, m, k, band, f, d, a = orc.model_case(name)
    want = orc.hsvd(x, m, k, band=band)
    got = _run(x[None], m, k, band=band)
    row = {key: got[key][0] for key in OUT}
    assert row["status"] == want["status"] == 0 and row["n_removed"] == want["n_removed"]
    assert np.array_equal(row["removed"], want["removed"])
    sel = row["removed"].astype(bool)
    t = np.arange(x.size)[:, None]
    amp = (row["amplitude"] * np.exp(1j * row["phase"]))[sel]
    parts = amp * np.exp((2j * np.pi * row["frequency"][sel] - row["damping"][sel]) * (t * orc.DT))
    bound = 16 * orc.EPS * (1 + np.pi * x.size) * float(np.abs(parts).sum(axis=1).max())
    dy = float(np.abs(row["y"] - (x - parts.sum(axis=1))).max())
    res = orc.model_residual(x, row)
    print(f"{name}: |y - (x - removed components)| {dy:.2e} (bound {bound:.1e}); max |x - B a| / max |x| {res:.2e} "
          f"(bound {16 * MODEL_RESIDUAL[name]:.1e}); f {row['frequency']}, d {row['damping']}, a {row['amplitude']}")
    assert dy <= bound
    assert res <= 16 * MODEL_RESIDUAL[name]


# ---- 1d. scale ----------------------------------------------------------------------------------------------------------------
_SCALE_FREE = ("frequency", "damping", "phase", "removed", "n_removed", "status")


@pytest.mark.parametrize("dtype", ["complex128", "complex64"])
def test_a_power_of_two_scale_changes_no_bit(dtype):
    """Every operation is homogeneous, every threshold relative, and a power of two commutes with rounding: f(2^k x) has
    the bits of f(x) in frequency, damping, phase, removed and status, and exactly 2^k times its amplitude and y."""
    x, m, k, _ = _case("N257-M17-K16", dtype)
    base = _run(x, m, k)
    assert np.all(base["status"] == 0)
    for e in (40, -40):
        got = _run(np.ldexp(x.real, e) + 1j * np.ldexp(x.imag, e), m, k) if dtype == "complex128" else \
            _run((x * np.float32(2.0 ** e)).astype(dtype), m, k)
        for key in _SCALE_FREE:
            assert np.array_equal(got[key], base[key]), (e, key)
        assert np.array_equal(got["amplitude"], np.ldexp(base["amplitude"], e)), e
        assert np.array_equal(got["y"], base["y"] * base["y"].real.dtype.type(2.0 ** e)), e


def _scaled(x, e):
    return np.ldexp(x.real, e) + 1j * np.ldexp(x.imag, e)


def test_samples_at_the_ends_of_the_exponent_range():
    """complex128.  x 2^-300: G = H^H H is 2^-600 times what it was, its square underflows to zero; the Jacobi stopping
    test takes its norms on a scaled G, so the rows are decomposed as their unscaled selves (status 0, the scale-free
    outputs within HSVD_TOL of the unscaled run, amplitude and y scaled).  x 2^300: the squared norm of G overflows, the
    documented status 2 with y zero and the components NaN."""
    x, m, k, _ = _case("N257-M17-K16", "complex128")
    base, got = _run(x, m, k), _run(_scaled(x, -300), m, k)
    back = dict(got, amplitude=np.ldexp(got["amplitude"], 300), y=_scaled(got["y"], 300))
    print(f"2^-300: status {got['status']}, bits equal {_same(back, base)}")
    assert np.all(base["status"] == 0)
    _check(back, orc.with_poles(base), x, what="x 2^-300 against x")
    big = _run(_scaled(x, 300), m, k)
    assert np.all(big["status"] == 2) and not big["y"].any() and not big["n_removed"].any() and not big["removed"].any()
    assert all(np.isnan(big[key]).all() for key in ("frequency", "damping", "amplitude", "phase"))


# ---- 2. bitwise properties ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["complex64", "complex128"])
def test_a_row_does_not_depend_on_its_batch(dtype):
    import torch

    x7, _, _ = orc.make_fid(70, 21, 7)
    x7 = x7.astype(dtype)
    big = np.tile(x7, (715, 1))[:5003]
    work = torch.zeros(256, dtype=torch.uint8, device="cuda")
    a, b = _run(x7, 17, 6, workspace=work), _run(big, 17, 6, workspace=work)
    assert int(work.sum().item()) == 0
    idx = np.arange(5003) % 7
    for key in OUT:
        assert np.array_equal(b[key], a[key][idx], equal_nan=True), key


def test_row_stride_and_components_only():
    x, _, _ = orc.make_fid(96, 22, 5)
    wide = np.full((5, 131), 7.0 + 7.0j)
    wide[:, :96] = x
    dense = _run(x, 16, 5)
    strided = _run(_up(wide)[:, :96], 16, 5)  # a view: rows 131 elements apart, read where they lie
    assert _same(dense, strided)
    only = _run(x, 16, 5, want_y=False)  # y = NULL
    assert only["y"] is None and _same(dense, only, OUT[1:])


# ---- 3. status ------------------------------------------------------------------------------------------------------------
def test_status_cases_leave_their_neighbours_alone():
    x, _, _ = orc.make_fid(64, 23, 8)
    bad = x.copy()
    bad[1, 9] = np.nan
    bad[3] = 0.0
    bad[5, 63] = np.inf
    got = _run(bad, 16, 4)
    want = orc.hsvd_rows(bad, 16, 4)
    assert list(got["status"]) == list(want["status"]) == [0, 2, 0, 1, 0, 2, 0, 0]
    keep = [0, 2, 4, 6, 7]
    clean = _run(x[keep], 16, 4)
    for key in OUT:
        assert np.array_equal(got[key][keep], clean[key]), key
    assert not got["y"][[1, 5]].any() and np.array_equal(got["y"][3], bad[3])
    for r in (1, 3, 5):
        assert got["n_removed"][r] == 0 and not got["removed"][r].any()
        assert all(np.isnan(got[key][r]).all() for key in ("frequency", "damping", "amplitude", "phase"))
    # a single nonzero sample: G = e_0 e_0^T, the pole is zero and z^t is not finite -- status 4, y = x
    one = x[:3].copy()
    one[1] = 0.0
    one[1, 0] = 1.0
    got1, want1 = _run(one, 16, 1), orc.hsvd_rows(one, 16, 1)
    assert list(got1["status"]) == list(want1["status"]) == [0, 4, 0]
    assert np.array_equal(got1["y"][1], one[1]) and np.isnan(got1["frequency"][1]).all() and got1["n_removed"][1] == 0
    alone = _run(one[[0, 2]], 16, 1)
    for key in OUT:
        assert np.array_equal(got1[key][[0, 2]], alone[key]), key
    # a band away from every pole: y = x bitwise, the components are what they are with any band
    for dtype in (np.complex128, np.complex64):
        xs = x.astype(dtype)
        far, near = _run(xs, 16, 4, band=(1000.0, 1100.0)), _run(xs, 16, 4)
        assert np.all(far["status"] == 1) and not far["n_removed"].any() and not far["removed"].any()
        assert np.array_equal(far["y"], xs) and _same(far, near, ("frequency", "damping", "amplitude", "phase"))


def test_c_abi_refusals_leave_outputs_and_workspace_alone():
    import torch
    from xmris_amd import _lib

    lib = _lib.load()
    n = 8
    x = torch.ones((2, n), dtype=torch.complex64, device="cuda")
    y = torch.full((2, n), 7.0, dtype=torch.complex64, device="cuda")
    f = [torch.full((2, 2), 7.0, dtype=torch.float64, device="cuda") for _ in range(4)]
    s = [torch.full((2, 2), 7, dtype=torch.int32, device="cuda") for _ in range(3)]
    ws = torch.full((256,), 171, dtype=torch.uint8, device="cuda")
    ok = dict(x=x.data_ptr(), rs=n, N=n, M=3, K=2, dt=1e-3, lo=-1.0, hi=1.0, dtype=0, ws=ws.data_ptr())
    for change in (dict(x=None), dict(ws=None), dict(M=1), dict(M=5), dict(K=0), dict(K=3), dict(rs=n - 1), dict(dt=0.0),
                   dict(lo=2.0), dict(dtype=5), dict(dtype=0x1000), dict(N=5)):
        a = dict(ok, **change)
        rc = lib.xm_hsvd_rows(a["x"], a["rs"], y.data_ptr(), f[0].data_ptr(), f[1].data_ptr(), f[2].data_ptr(),
                              f[3].data_ptr(), s[0].data_ptr(), s[1].data_ptr(), s[2].data_ptr(), 2, a["N"], a["M"], a["K"],
                              a["dt"], a["lo"], a["hi"], a["dtype"], a["ws"], None)
        assert rc == _lib.XM_ERR_INVALID_ARG, change
    torch.cuda.synchronize()
    assert bool((y == 7).all()) and all(bool((v == 7).all()) for v in f + s) and bool((ws == 171).all())


# ---- 4. through the accessor ----------------------------------------------------------------------------------------------
def _labeled(x, dims, **attrs):
    from xmris_amd import LabeledArray

    coords = {d: np.arange(x.shape[i], dtype=float) for i, d in enumerate(dims) if d != "time"}
    coords["time"] = ("time", np.arange(x.shape[dims.index("time")]) * orc.DT, {"units": "s", "long_name": "Time"})
    return LabeledArray(x, dims, coords, dict(attrs))


def test_accessor_layouts_metadata_and_components():
    from xmris_amd import LabeledArray
    from xmris_amd.fitting.dataset import LabeledDataset

    x, _, _ = orc.make_fid(256, 1, 6)
    want = orc.hsvd_rows(x, 32, 8)
    assert np.all(want["status"] == 0)
    da = _labeled(x.reshape(2, 3, 256), ("x", "y", "time"), MHz=300.0)
    before = da.values.copy()
    out = da.xmr.remove_water(rank=8, n_cols=32)
    ds = da.xmr.remove_water(rank=8, n_cols=32, return_components=True)
    assert isinstance(out, LabeledArray) and isinstance(ds, LabeledDataset)
    assert out.dims == da.dims and out.is_device_resident and set(out.coords) == set(da.coords)
    assert out.attrs == {"MHz": 300.0, "water_band": (-50.0, 50.0), "water_rank": 8, "water_n_cols": 32}
    assert da.attrs == {"MHz": 300.0} and np.array_equal(da.values, before)
    assert set(ds.data_vars) == {"cleaned", "frequency", "damping", "amplitude", "phase", "removed", "n_removed", "status"}
    assert ds.attrs == out.attrs and np.array_equal(ds["cleaned"].values, out.values)
    assert ds["frequency"].dims == ("x", "y", "component") == ds["removed"].dims and ds["status"].dims == ("x", "y")
    assert ds["frequency"].shape == (2, 3, 8) and np.all(ds["status"].values == 0)
    got = {k: ds[k].values.reshape((6,) + ds[k].shape[2:]) for k in OUT[1:]}
    got.update(y=out.values.reshape(6, 256), kernel="accessor")
    _check(got, want, x, what="accessor (x, y, time)")
    # dt given instead of a coordinate: the same bits
    from xmris_amd import remove_water

    bare = LabeledArray(x.reshape(2, 3, 256), ("x", "y", "time"))
    assert np.array_equal(remove_water(bare, rank=8, n_cols=32, dt=orc.DT).values, out.values)
    # (time, voxel): one copy, the same numbers, time where it was
    d2 = _labeled(np.ascontiguousarray(x.T), ("time", "voxel")).xmr.remove_water(rank=8, n_cols=32, return_components=True)
    assert d2["cleaned"].dims == ("time", "voxel") and np.array_equal(d2["cleaned"].values.T, out.values.reshape(6, 256))
    assert d2["amplitude"].dims == ("voxel", "component")
    assert np.array_equal(d2["amplitude"].values, ds["amplitude"].values.reshape(6, 8))


class _FakeDataset:
    """What tests/_fake_xarray.py lacks: the container LabeledDataset.to_xarray() builds."""

    def __init__(self, data_vars, attrs=None):
        self.data_vars, self.attrs = dict(data_vars), dict(attrs or {})

    def __getitem__(self, k):
        return self.data_vars[k]


def test_fake_xarray_in_gives_xarray_out(monkeypatch):
    import _fake_xarray

    from xmris_amd import accessor, labeled

    xr = _fake_xarray.install(monkeypatch)
    monkeypatch.setattr(xr, "Dataset", _FakeDataset, raising=False)
    accessor.register_xarray_accessor(force=True)
    x, _, _ = orc.make_fid(128, 2, 3)
    t = np.arange(128) * orc.DT
    coords = {"x": [10, 11, 12], "time": xr.Variable("time", t, {"units": "s"})}
    da = xr.DataArray(x, dims=("x", "time"), coords=coords, attrs={"MHz": 300.0}, name="fid")
    la = _labeled(x, ("x", "time"), MHz=300.0)
    assert labeled.is_xarray(da) and isinstance(da.xmr, accessor.XmrisAccessor)
    attrs = {"MHz": 300.0, "water_band": (-50.0, 50.0), "water_rank": 6, "water_n_cols": 24}
    got, want = da.xmr.remove_water(rank=6, n_cols=24), la.xmr.remove_water(rank=6, n_cols=24)
    assert isinstance(got, xr.DataArray) and isinstance(got.data, np.ndarray)
    assert got.dims == ("x", "time") and got.attrs == attrs and got.name == "fid"
    assert np.array_equal(got.coords["time"].values, t) and got.coords["time"].attrs == {"units": "s"}
    assert np.array_equal(got.values, want.values)
    ds = da.xmr.remove_water(rank=6, n_cols=24, return_components=True)
    wds = la.xmr.remove_water(rank=6, n_cols=24, return_components=True)
    assert isinstance(ds, _FakeDataset) and set(ds.data_vars) == set(wds.data_vars) and ds.attrs == attrs
    for k in ds.data_vars:
        assert isinstance(ds[k], xr.DataArray) and ds[k].dims == wds[k].dims, k
        assert np.array_equal(ds[k].values, wds[k].values, equal_nan=True), k
    assert np.array_equal(ds["status"].coords["x"].values, [10, 11, 12])
