"""k_denoise / xm_denoise_patches / .xmr.denoise_mppca on the GPU against tests/_denoise_oracle.py.  The shapes are
orc.PARITY_CASES, whose conditions (the same rank on both routes, every comparison of the rank scan decided by a margin,
status 0) and route agreement are checked on the CPU in tests/test_denoise.py."""
import functools

import numpy as np
import pytest

import _denoise_oracle as orc
from test_denoise import DENOISE_TOL, y_bound  # 16 x the routes' disagreement, tests/tool_denoise_tolerance.py

pytestmark = pytest.mark.gpu

OUT = ("y", "rank", "sigma", "status")


def _up(a):
    import torch

    return torch.from_numpy(np.array(a)).to("cuda")  # (a copy: the shared cases are read-only)


def _run(x, patch, **kw):
    """x [..., grid..., N] with len(patch) patch axes in front of time."""
    from xmris_amd import device as dev

    xd = x if hasattr(x, "is_cuda") else _up(x)
    nd = xd.dim()
    r = dev.denoise_patches(xd, tuple(range(nd - 1 - len(patch), nd - 1)), -1, patch, **kw)
    out = {key: getattr(r, key).cpu().numpy() for key in OUT}
    out["kernel"] = dev.last_kernel()
    return out


def _check(got, want, x, dtype="complex128", what=""):
    """rank and status equal; y within DENOISE_TOL["y"] of the oracle's units per voxel (complex64: plus the one fp32
    rounding of y); sigma within DENOISE_TOL["sigma"] of itself."""
    assert np.array_equal(got["status"], want["status"]), (what, got["status"])
    assert np.array_equal(got["rank"], want["rank"]), (what, got["rank"], want["rank"])
    dy = np.abs(got["y"] - want["y"]).max(axis=-1)
    bound = y_bound(want, x, dtype)
    sg = np.where(want["sigma"] > 0, want["sigma"], 1.0)
    ds = np.abs(got["sigma"] - want["sigma"]) / sg
    print(f"{what}: y {float((dy / orc.units(want, x)).max()):.2f} units, {float((dy / bound).max()):.3f} of its bound; "
          f"sigma {float(ds.max()):.2e} (bound {DENOISE_TOL['sigma']:.1e}); ranks {want['rank'].min()}-{want['rank'].max()}; "
          f"{got.get('kernel', '')}")
    assert np.all(dy <= bound), (what, float((dy / bound).max()))
    assert np.all(ds <= DENOISE_TOL["sigma"]), (what, float(ds.max()))


@functools.lru_cache(maxsize=None)
def _case(name, dtype):
    """(x in `dtype`, patch, the oracle's result on x widened): complex128 is the case's own data and result."""
    _, x, a, _, _ = orc.parity_case(name)
    patch = orc.PARITY_CASES[name][1]
    if dtype == "complex128":
        return x, patch, a
    x = x.astype(dtype)
    return x, patch, orc.denoise(x.astype(np.complex128), patch)


# ---- 1. parity ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["complex128", "complex64"])
@pytest.mark.parametrize("name", list(orc.PARITY_CASES))
def test_parity_with_the_oracle(name, dtype):
    x, patch, want = _case(name, dtype)
    got = _run(x, patch)
    p = int(np.prod(patch))
    assert got["y"].dtype == np.dtype(dtype) and got["y"].shape == x.shape
    assert f"k_denoise<{'mfma' if p >= 8 else 'fma'}, {p}>" in got["kernel"]
    _check(got, want, x.astype(np.complex128), dtype, what=f"{name} {dtype}")


@pytest.mark.parametrize("name, k", [("g6x7_p3x3_n65", 2), ("g5x5x4_p3x3x3_n128", 3)])
def test_a_given_rank(name, k):
    x, patch, _ = _case(name, "complex128")
    p = int(np.prod(patch))
    for r in (0, 1, k, p):
        got, want = _run(x, patch, rank=r), orc.denoise(x, patch, rank=r)
        assert np.all(got["rank"] == r) and f"{p}, {r}>" in got["kernel"]
        _check(got, want, x, what=f"{name} rank {r}")
        if r == 0:
            assert not got["y"].any()
        if r == p:  # (y = x to rounding: the oracle's y is, and _check has held y to it in units of eps max |x|)
            assert not got["sigma"].any()


@pytest.mark.parametrize("name", ["g6x5_p2x4_n40", "g5x5x4_p3x3x3_n128", "g8x8_p8x8_n2048"])
def test_matrix_core_and_fma_gram_agree(name):
    x, patch, want = _case(name, "complex128")
    a, b = _run(x, patch), _run(x, patch, _gram_fma=True)
    assert "k_denoise<mfma" in a["kernel"] and "k_denoise<fma" in b["kernel"]
    _check(b, want, x, what=f"{name} fma")
    _check(a, dict(b, lam=want["lam"]), x, what=f"{name} mfma against fma")


@pytest.mark.parametrize("p", list(orc.SWEEP_CASES))
def test_every_patch_size_on_both_gram_forms(p):
    """Every P the kernel accepts (orc.SWEEP_CASES, whose conditions are checked in tests/test_denoise.py): every block-row
    count and padded row of the matrix-core Gram map, every entries-per-thread count of the plain-FMA one, and every
    round-robin schedule of the Jacobi with all its eigenvectors in use."""
    _, x, want, _, _ = orc.sweep_case(p)
    a, b = _run(x, (p,)), _run(x, (p,), _gram_fma=True)
    assert f"k_denoise<{'mfma' if p >= 8 else 'fma'}, {p}>" in a["kernel"] and "k_denoise<fma" in b["kernel"]
    _check(a, want, x, what=f"P={p}")
    _check(b, want, x, what=f"P={p} fma")


# ---- 1b. scale ------------------------------------------------------------------------------------------------------------
def _scaled(x, e):
    if x.dtype == np.complex64:
        return (x * np.float32(2.0 ** e)).astype(np.complex64)
    if x.dtype == np.float64:
        return np.ldexp(x, e)
    return np.ldexp(x.real, e) + 1j * np.ldexp(x.imag, e)


@pytest.mark.parametrize("dtype", ["complex128", "complex64"])
def test_a_power_of_two_scale_changes_no_bit(dtype):
    """Every operation is homogeneous, every threshold relative, and a power of two commutes with rounding: the rank and
    the status of 2^k x have the bits of x's, y and sigma are exactly 2^k times x's."""
    x, patch, _ = _case("g6x7_p3x3_n65", dtype)
    base = _run(x, patch)
    assert np.all(base["status"] == 0)
    for e in (40, -40):
        got = _run(_scaled(x, e), patch)
        assert np.array_equal(got["rank"], base["rank"]) and np.array_equal(got["status"], base["status"]), e
        assert np.array_equal(got["y"], _scaled(base["y"], e)), e
        assert np.array_equal(got["sigma"], _scaled(base["sigma"], e)), e


def test_samples_at_the_ends_of_the_exponent_range():
    """complex128.  x 2^-300: G is 2^-600 times what it was, its square underflows to zero; the Jacobi stopping test
    takes its norms on a scaled G, so the voxels are denoised as their unscaled selves (status 0, the rank equal, y and
    sigma scaled and within the file's bounds of the unscaled run).  x 2^300: the squared norm of G overflows, the
    documented status 2 with y zero, rank 0 and sigma NaN, as the oracle has it."""
    x, patch, want = _case("g6x7_p3x3_n65", "complex128")
    base, got = _run(x, patch), _run(_scaled(x, -300), patch)
    back = dict(got, y=_scaled(got["y"], 300), sigma=_scaled(got["sigma"], 300))
    print(f"2^-300: status {np.unique(got['status'])}, bits equal {all(np.array_equal(back[k], base[k]) for k in OUT)}")
    _check(back, dict(want, y=base["y"], sigma=base["sigma"]), x, what="x 2^-300 against x")
    big = _run(_scaled(x, 300), patch)
    assert np.all(orc.denoise(_scaled(x, 300), patch)["status"] == 2)
    assert np.all(big["status"] == 2) and not big["y"].any() and not big["rank"].any() and np.isnan(big["sigma"]).all()


# ---- 2. bitwise properties ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["complex64", "complex128"])
def test_a_voxel_does_not_depend_on_its_batch(dtype):
    import torch

    _, x7 = orc.make_data((7,), 70, 2, seed=21)
    x7 = x7.astype(dtype)
    big = np.tile(x7, (715, 1, 1))
    work = torch.zeros(256, dtype=torch.uint8, device="cuda")
    a, b = _run(x7, (3,), workspace=work), _run(big, (3,), workspace=work)
    assert int(work.sum().item()) == 0
    assert np.all(a["status"] == 0) and b["y"].shape == (715, 7, 70)
    for key in OUT:
        assert np.array_equal(b[key], np.broadcast_to(a[key], b[key].shape), equal_nan=True), key


# ---- 3. status ------------------------------------------------------------------------------------------------------------
def test_status_cases_leave_their_neighbours_alone():
    grid, patch = (8, 9), (3, 3)
    _, x = orc.make_data(grid, 64, 2, seed=23)
    bad = x.copy()
    bad[:3, :3] = 0.0
    bad[7, 8, 5] = np.nan
    bad[4, 8, 60] = np.inf
    changed = np.zeros(grid, bool)
    changed[:3, :3] = changed[7, 8] = changed[4, 8] = True
    got, want, clean = _run(bad, patch), orc.denoise(bad, patch), _run(x, patch)
    zero, nonfinite, touched = (np.zeros(grid, bool) for _ in range(3))
    for idx, rows, _ in orc.windows(grid, patch):
        zero[idx] = all(r[0] < 3 and r[1] < 3 for r in rows)
        nonfinite[idx] = (7, 8) in rows or (4, 8) in rows
        touched[idx] = any(changed[r] for r in rows)
    assert zero.sum() == 4 and nonfinite.sum() == 2 * 2 + 3 * 2
    assert np.array_equal(got["status"], want["status"])
    assert np.array_equal(got["status"], np.where(nonfinite, 2, np.where(zero, 1, 0)))
    assert not got["y"][zero | nonfinite].any() and not got["rank"][zero | nonfinite].any()
    assert not got["sigma"][zero].any() and np.isnan(got["sigma"][nonfinite]).all()
    assert touched.sum() < touched.size
    for key in OUT:
        assert np.array_equal(got[key][~touched], clean[key][~touched]), key


def test_c_abi_refusals_leave_outputs_and_workspace_alone():
    import torch
    from xmris_amd import _lib

    lib = _lib.load()
    n = 16
    x = torch.ones((2, 3, 3, n), dtype=torch.complex64, device="cuda")
    y = torch.full((2, 3, 3, n), 7.0, dtype=torch.complex64, device="cuda")
    rk = torch.full((2, 3, 3), 7, dtype=torch.int32, device="cuda")
    sg = torch.full((2, 3, 3), 7.0, dtype=torch.float64, device="cuda")
    st = torch.full((2, 3, 3), 7, dtype=torch.int32, device="cuda")
    ws = torch.full((256,), 171, dtype=torch.uint8, device="cuda")
    ok = dict(x=x.data_ptr(), y=y.data_ptr(), s2=3, s3=3, p2=3, p3=3, N=n, rank=-1, dtype=0, ws=ws.data_ptr())
    for change in (dict(x=None), dict(ws=None), dict(y=x.data_ptr()), dict(p2=4), dict(p3=0), dict(p2=1, p3=1), dict(N=8),
                   dict(N=16385), dict(rank=10), dict(rank=-2), dict(dtype=5), dict(dtype=0x800)):
        a = dict(ok, **change)
        rc = lib.xm_denoise_patches(a["x"], a["y"], rk.data_ptr(), sg.data_ptr(), st.data_ptr(), 2, 1, a["s2"], a["s3"], 1,
                                    a["p2"], a["p3"], a["N"], a["rank"], a["dtype"], a["ws"], None)
        assert rc == _lib.XM_ERR_INVALID_ARG, change
    torch.cuda.synchronize()
    assert bool((y == 7).all()) and all(bool((v == 7).all()) for v in (rk, sg, st)) and bool((ws == 171).all())


# ---- 4. through the accessor ----------------------------------------------------------------------------------------------
def _labeled(x, dims, **attrs):
    from xmris_amd import LabeledArray

    coords = {d: np.arange(x.shape[i], dtype=float) for i, d in enumerate(dims) if d != "time"}
    coords["time"] = ("time", np.arange(x.shape[dims.index("time")]) * 1e-3, {"units": "s", "long_name": "Time"})
    return LabeledArray(x, dims, coords, dict(attrs))


def test_accessor_layouts_metadata_and_noise():
    from xmris_amd import LabeledArray
    from xmris_amd.fitting.dataset import LabeledDataset

    x, patch, want = _case("g6x7_p3x3_n65", "complex128")
    da = _labeled(x, ("x", "y", "time"), MHz=120.0)
    before = da.values.copy()
    out = da.xmr.denoise_mppca(("x", "y"), 3)
    ds = da.xmr.denoise_mppca(("x", "y"), (3, 3), return_noise=True)
    assert isinstance(out, LabeledArray) and isinstance(ds, LabeledDataset)
    assert out.dims == da.dims and out.is_device_resident and set(out.coords) == set(da.coords)
    assert out.attrs == {"MHz": 120.0, "denoise_dims": ("x", "y"), "denoise_patch": (3, 3), "denoise_rank": "mp"}
    assert da.attrs == {"MHz": 120.0} and np.array_equal(da.values, before)
    assert set(ds.data_vars) == {"denoised", "sigma", "rank", "status"}
    assert ds.attrs == out.attrs and np.array_equal(ds["denoised"].values, out.values)
    assert ds["sigma"].dims == ds["rank"].dims == ds["status"].dims == ("x", "y") and ds["sigma"].shape == (6, 7)
    got = {k: ds[k].values for k in OUT[1:]}
    got.update(y=out.values, kernel="accessor")
    _check(got, want, x, what="accessor (x, y, time)")
    fixed = da.xmr.denoise_mppca(("x", "y"), 3, rank=2)
    assert fixed.attrs["denoise_rank"] == 2 and np.array_equal(fixed.values, _run(x, patch, rank=2)["y"])
    # (time, x, y): one copy, the same numbers, time where it was
    d2 = _labeled(np.ascontiguousarray(np.moveaxis(x, -1, 0)), ("time", "x", "y")).xmr.denoise_mppca(("x", "y"), 3, return_noise=True)
    assert d2["denoised"].dims == ("time", "x", "y") and d2["sigma"].dims == ("x", "y")
    assert np.array_equal(np.moveaxis(d2["denoised"].values, 0, -1), out.values)
    assert np.array_equal(d2["sigma"].values, ds["sigma"].values)
    # the patch dims named in the other order: the transposed problem
    d3 = da.xmr.denoise_mppca(("y", "x"), 3, return_noise=True)
    tr = _run(np.ascontiguousarray(x.transpose(1, 0, 2)), (3, 3))
    assert d3["denoised"].dims == ("x", "y", "time") and np.array_equal(d3["denoised"].values, tr["y"].transpose(1, 0, 2))
    assert np.array_equal(d3["rank"].values, tr["rank"].T)


def test_accessor_with_batch_dims_and_a_repetition_patch():
    x, patch, _ = _case("g5x5x4_p3x3x3_n128", "complex128")
    two = np.stack([x, 1j * x[::-1]])  # (coil, x, y, z, time), coil is batch
    ds = _labeled(two, ("coil", "x", "y", "z", "time")).xmr.denoise_mppca(("x", "y", "z"), 3, return_noise=True)
    assert ds["denoised"].shape == two.shape and ds["sigma"].dims == ("coil", "x", "y", "z")
    for c in range(2):
        alone = _run(two[c], patch)
        assert np.array_equal(ds["denoised"].values[c], alone["y"]) and np.array_equal(ds["sigma"].values[c], alone["sigma"])
        assert np.array_equal(ds["rank"].values[c], alone["rank"]) and np.all(ds["status"].values[c] == 0)
    # a patch along a dim that is not spatial, voxels as batch on either side of it
    _, r = orc.make_data((9,), 40, 2, seed=0, n_outer=3)  # (voxel, repetition, time)
    want = orc.denoise(r, (5,))
    o1 = _labeled(r, ("voxel", "repetition", "time")).xmr.denoise_mppca(("repetition",), 5, return_noise=True)
    got = {k: o1[k].values for k in OUT[1:]}
    got.update(y=o1["denoised"].values, kernel="accessor")
    _check(got, want, r, what="accessor dims=(repetition,)")
    o2 = _labeled(np.ascontiguousarray(r.transpose(1, 0, 2)), ("repetition", "voxel", "time")).xmr.denoise_mppca("repetition", 5, return_noise=True)
    assert o2["denoised"].dims == ("repetition", "voxel", "time") and o2["rank"].dims == ("repetition", "voxel")
    assert np.array_equal(o2["denoised"].values.transpose(1, 0, 2), got["y"])
    assert np.array_equal(o2["sigma"].values.T, got["sigma"])


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
    x, _, _ = _case("g4x3_p2x3_n7", "complex128")
    t = np.arange(7) * 1e-3
    coords = {"x": [10, 11, 12, 13], "time": xr.Variable("time", t, {"units": "s"})}
    da = xr.DataArray(x, dims=("x", "y", "time"), coords=coords, attrs={"MHz": 120.0}, name="fid")
    la = _labeled(x, ("x", "y", "time"), MHz=120.0)
    assert labeled.is_xarray(da) and isinstance(da.xmr, accessor.XmrisAccessor)
    attrs = {"MHz": 120.0, "denoise_dims": ("x", "y"), "denoise_patch": (2, 3), "denoise_rank": "mp"}
    got, want = da.xmr.denoise_mppca(("x", "y"), (2, 3)), la.xmr.denoise_mppca(("x", "y"), (2, 3))
    assert isinstance(got, xr.DataArray) and isinstance(got.data, np.ndarray)
    assert got.dims == ("x", "y", "time") and got.attrs == attrs and got.name == "fid"
    assert np.array_equal(got.coords["time"].values, t) and got.coords["time"].attrs == {"units": "s"}
    assert np.array_equal(got.values, want.values)
    ds = da.xmr.denoise_mppca(("x", "y"), (2, 3), return_noise=True)
    wds = la.xmr.denoise_mppca(("x", "y"), (2, 3), return_noise=True)
    assert isinstance(ds, _FakeDataset) and set(ds.data_vars) == set(wds.data_vars) and ds.attrs == attrs
    for k in ds.data_vars:
        assert isinstance(ds[k], xr.DataArray) and ds[k].dims == wds[k].dims, k
        assert np.array_equal(ds[k].values, wds[k].values, equal_nan=True), k
    assert np.array_equal(ds["status"].coords["x"].values, [10, 11, 12, 13])


def test_chain_to_the_spectrum():
    """denoise_mppca -> zero_fill -> apodize_exp -> to_spectrum against the same chain on the oracle's y.  The chain is
    linear and, with a window <= 1 and an orthonormal FFT, does not increase the 2-norm: a bin differs by at most
    ||dy||_2 <= sqrt(N) max |dy| per voxel, plus the two chains' own fp64 rounding, a few eps log2(n_fft) ||y||_2 each
    (taken as 16 eps log2(n_fft) sqrt(N) max |y| together)."""
    x, patch, want = _case("g8x8_p5x5_n256", "complex128")
    n, nfft = x.shape[-1], 512
    chain = lambda a: a.xmr.zero_fill(target_points=nfft).xmr.apodize_exp(lb=3.0).xmr.to_spectrum()  # noqa: E731
    got = chain(_labeled(x, ("x", "y", "time")).xmr.denoise_mppca(("x", "y"), 5)).values
    ref = chain(_labeled(want["y"], ("x", "y", "time"))).values
    assert got.shape == (8, 8, nfft)
    d = np.abs(got - ref).max(axis=-1)
    bound = np.sqrt(n) * (y_bound(want, x) + 16 * orc.EPS * np.log2(nfft) * np.abs(want["y"]).max(axis=-1))
    print(f"chain: spectrum differs by {float((d / bound).max()):.3f} of its bound, {float(d.max()):.2e} absolute")
    assert np.all(d <= bound)
