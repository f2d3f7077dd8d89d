"""k_coil_combine / xm_coil_combine / .xmr.combine_coils on the GPU against tests/_coils_oracle.py.  The shapes are
orc.PARITY_CASES, whose spectral gaps and route agreement are checked on the CPU in tests/test_coils.py."""
import functools

import numpy as np
import pytest

import _coils_oracle as orc
from test_coils import COIL_TOL  # 16 x the 5.48 of tests/tool_coil_tolerance.py

pytestmark = pytest.mark.gpu

EPS = orc.EPS
HALF32 = 2.0 ** -24  # one rounding of an fp32 value, relative
OUT = ("y", "w", "quality", "status")


def _run(x, coil_axis=1, reference=None, work=None, **kw):
    import torch
    from xmris_amd import device as dev

    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda")  # noqa: E731
    r = dev.coil_combine(up(x), coil_axis, -1, reference=None if reference is None else up(reference), workspace=work, **kw)
    return dict(y=r.y.cpu().numpy(), w=r.weights.cpu().numpy(), quality=r.quality.cpu().numpy(),
                status=r.status.cpu().numpy(), kernel=dev.last_kernel())


def _same(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in OUT)


def _check(got, want, c64=False, tol=COIL_TOL, what=""):
    """y (relative to max |y|), w (to max |w|) and quality within tol eps lam1 / (lam1 - lam2); complex64 output: plus
    one fp32 rounding of the oracle's y (sqrt 2: both components)."""
    gain = EPS * want["lam1"] / (want["lam1"] - want["lam2"])
    dy = np.abs(got["y"] - want["y"]).max(axis=-1) / np.abs(want["y"]).max(axis=-1)
    dw = np.abs(got["w"] - want["w"]).max(axis=-1) / np.abs(want["w"]).max(axis=-1)
    dq = np.abs(got["quality"] - want["quality"])
    extra = np.sqrt(2.0) * HALF32 if c64 else 0.0
    print(f"{what}: y {np.max(dy / gain):.2f} (fp32 rounding {np.max(extra / gain):.0f})  w {np.max(dw / gain):.2f}  quality {np.max(dq / gain):.2f} "
          f"units of eps lam1 / (lam1 - lam2); bound {tol}; {got['kernel']}")
    assert np.all(got["status"] == 0), got["status"]
    assert np.all(dy <= tol * gain + extra), (what, "y", np.max(dy / gain))
    assert np.all(dw <= tol * gain), (what, "w", np.max(dw / gain))
    assert np.all(dq <= tol * gain), (what, "quality", np.max(dq / gain))


@functools.lru_cache(maxsize=None)
def _case(name, dtype):
    x = orc.parity_case(name).astype(dtype)
    return x, orc.combine_batch(x.astype(np.complex128), coil_axis=1)


# ---- 1. parity ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["complex128", "complex64"])
@pytest.mark.parametrize("name", list(orc.PARITY_CASES))
def test_parity_with_the_oracle(name, dtype):
    x, want = _case(name, dtype)
    got = _run(x)
    c = x.shape[1]
    assert got["y"].dtype == np.dtype(dtype) and got["w"].dtype == np.complex128
    assert ("k_coil_combine<mfma" if c >= 8 else "k_coil_combine<fma") in got["kernel"]
    _check(got, want, c64=dtype == "complex64", what=f"{name} {dtype}")


@pytest.mark.parametrize("name", ["c8_n63_v37", "c33_n65_inner3", "c64_n63_v37"])
def test_plain_fma_gram_agrees_with_the_oracle_too(name):
    x, want = _case(name, "complex128")
    got = _run(x, method="svd_fma")
    assert "k_coil_combine<fma" in got["kernel"]
    _check(got, want, what=f"{name} fma")


# ---- 1b. every coil count ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", list(orc.SWEEP_COILS))
def test_every_coil_count_on_both_gram_forms(c):
    """Every C the kernel accepts, so every block-row count of the matrix-core Gram map, every padded row inside a block
    and every entries-per-thread count of the plain-FMA map; the gaps are checked in tests/test_coils.py."""
    x = orc.sweep_case(c)
    want = orc.combine_batch(x, coil_axis=1)
    got = _run(x)
    assert ("k_coil_combine<mfma" if c >= 8 else "k_coil_combine<fma") in got["kernel"]
    _check(got, want, what=f"C={c} svd")
    fma = _run(x, method="svd_fma")
    assert "k_coil_combine<fma" in fma["kernel"]
    _check(fma, want, what=f"C={c} svd_fma")


# ---- 2. reference -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_ref", [7, 100])
def test_reference_of_another_length(n_ref):
    x = orc.make_data(3, 8, 2, 33, seed=11)
    ref = orc.make_data(3, 8, 2, n_ref, seed=12)
    want = orc.combine_batch(x, ref, coil_axis=1)
    got = _run(x, reference=ref)
    _check(got, want, what=f"reference N_R={n_ref}")
    other = _run(orc.make_data(3, 8, 2, 33, seed=13), reference=ref)
    assert np.array_equal(other["w"], got["w"]) and np.array_equal(other["quality"], got["quality"])
    assert not np.array_equal(other["y"], got["y"])


# ---- 3. noise covariance ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [3, 16])
def test_noise_covariance(c):
    x = orc.make_data(5, c, 1, 65, seed=21)
    psi = orc.random_psd(c, 22)
    want = orc.combine_batch(x, coil_axis=1, psi=psi)
    alt = orc.combine_batch(x, coil_axis=1, psi=psi, route="svd")
    assert np.all((want["lam1"] - want["lam2"]) / want["lam1"] >= 0.5)
    print("oracle routes under whitening:", orc.route_gap_units(want, alt))
    _check(_run(x, linv=orc.linv_of(psi)), want, what=f"noise_cov C={c}")
    assert _same(_run(x, linv=orc.linv_of(np.eye(c))), _run(x))


# ---- 4. first_point ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_points", [1, 5])
@pytest.mark.parametrize("whiten", [False, True])
def test_first_point_against_the_closed_form(n_points, whiten):
    c = 8
    x = orc.make_data(9, c, 1, 70, seed=31 + n_points)
    psi = orc.random_psd(c, 32) if whiten else None
    want = orc.combine_batch(x, coil_axis=1, psi=psi, method="first_point", n_points=n_points)
    got = _run(x, method="first_point", n_points=n_points, linv=None if psi is None else orc.linv_of(psi))
    assert "first_point" in got["kernel"] and np.all(got["status"] == 0)
    rel = lambda a, b: np.abs(a - b).max() / np.abs(b).max()  # noqa: E731
    print("first_point rel err / eps:", rel(got["y"], want["y"]) / EPS, rel(got["w"], want["w"]) / EPS,
          rel(got["quality"], want["quality"]) / EPS)
    assert rel(got["y"], want["y"]) <= 64 * EPS and rel(got["w"], want["w"]) <= 64 * EPS
    assert rel(got["quality"], want["quality"]) <= 64 * EPS


# ---- 5. batch independence --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c, dtype", [(8, "complex64"), (3, "complex128")])
def test_a_voxel_does_not_depend_on_its_batch(c, dtype):
    import torch

    x7 = orc.make_data(7, c, 1, 33, seed=41).astype(dtype)
    big = np.tile(x7, (715, 1, 1, 1))[:5003]
    work = torch.zeros(256, dtype=torch.uint8, device="cuda")
    a, b = _run(x7, work=work), _run(big, work=work)
    assert int(work.sum().item()) == 0
    idx = np.arange(5003) % 7
    for k in OUT:
        assert np.array_equal(b[k], a[k][idx]), k


# ---- 6. degenerate voxels ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c, method", [(8, "svd"), (3, "svd"), (8, "first_point")])
def test_degenerate_voxels_inside_a_batch(c, method):
    x = orc.make_data(9, c, 1, 70, seed=51)
    bad = x.copy()
    bad[2] = 0.0
    bad[4, c - 1, 0, 69] = np.nan
    bad[6, 0, 0, 3] = np.inf
    got = _run(bad, method=method)
    keep = [0, 1, 3, 5, 7, 8]
    clean = _run(x[keep], method=method)
    for k in OUT:
        assert np.array_equal(got[k][keep], clean[k]), k
    assert list(got["status"][[2, 4, 6]]) == [1, 2, 2]
    assert not got["y"][[2, 4, 6]].any() and not got["w"][[2, 4, 6]].any()
    assert got["quality"][2] == 0.0 and np.isnan(got["quality"][4]) and np.isnan(got["quality"][6])
    # a non-finite sample in X alone, the reference clean: status 2 as well
    ref = orc.make_data(9, c, 1, 20, seed=52)
    r = _run(bad, reference=ref, method=method)
    assert list(r["status"]) == [0, 0, 0, 0, 2, 0, 2, 0, 0] and not r["y"][[2, 4, 6]].any()
    assert np.array_equal(r["w"][keep], _run(x, reference=ref, method=method)["w"][keep])


# ---- 7. refusals of the C ABI -----------------------------------------------------------------------------------------
def test_c_abi_refusals_leave_outputs_and_workspace_alone():
    import torch
    from xmris_amd import _lib

    lib = _lib.load()
    c, n = 4, 8
    x = torch.ones((2, c, n), dtype=torch.complex64, device="cuda")
    y = torch.full((2, n), 7.0, dtype=torch.complex64, device="cuda")
    w = torch.full((2, c), 7.0, dtype=torch.complex128, device="cuda")
    q = torch.full((2,), 7.0, dtype=torch.float64, device="cuda")
    s = torch.full((2,), 7, dtype=torch.int32, device="cuda")
    ws = torch.full((256,), 171, dtype=torch.uint8, device="cuda")
    ok = dict(x=x.data_ptr(), ref=None, y=y.data_ptr(), w=w.data_ptr(), q=q.data_ptr(), s=s.data_ptr(), no=2, C=c, ni=1,
              N=n, NR=n, linv=None, method=0, npts=1, c128=0, ws=ws.data_ptr())
    for change in (dict(C=0), dict(C=65), dict(N=0), dict(NR=0), dict(npts=0), dict(npts=n + 1), dict(method=7),
                   dict(x=None), dict(y=None), dict(w=None), dict(q=None), dict(s=None), dict(ws=None)):
        a = dict(ok, **change)
        rc = lib.xm_coil_combine(a["x"], a["ref"], a["y"], a["w"], a["q"], a["s"], a["no"], a["C"], a["ni"], a["N"], a["NR"],
                                 a["linv"], a["method"], a["npts"], a["c128"], a["ws"], None)
        assert rc == _lib.XM_ERR_INVALID_ARG, change
    torch.cuda.synchronize()
    assert bool((y == 7).all()) and bool((w == 7).all()) and bool((q == 7).all()) and bool((s == 7).all())
    assert bool((ws == 171).all())


# ---- 8. through the accessor ------------------------------------------------------------------------------------------
def _labeled(x, dims, **attrs):
    from xmris_amd import LabeledArray

    coords = {d: np.arange(x.shape[i], dtype=float) for i, d in enumerate(dims) if d != "time"}
    coords["time"] = ("time", np.arange(x.shape[dims.index("time")]) / 2000.0, {"units": "s", "long_name": "Time"})
    return LabeledArray(x, dims, coords, dict(attrs))


def test_accessor_keeps_metadata_and_layouts():
    x = orc.make_data(6, 8, 1, 40, seed=61).reshape(2, 3, 8, 40)  # (x, y, coil, time)
    da = _labeled(x, ("x", "y", "coil", "time"), MHz=120.0)
    before = da.values.copy()
    want = orc.combine_batch(x, coil_axis=2)
    out = da.xmr.combine_coils()
    assert out.dims == ("x", "y", "time") and out.is_device_resident and set(out.coords) == {"x", "y", "time"}
    assert out.coords["time"].attrs == {"units": "s", "long_name": "Time"}
    assert np.array_equal(out.coords["time"].values, da.coords["time"].values)
    assert out.attrs == {"MHz": 120.0, "coil_combine_method": "svd", "coil_combine_dim": "coil"}
    assert da.attrs == {"MHz": 120.0} and np.array_equal(da.values, before)
    ds = da.xmr.combine_coils(return_weights=True)
    assert set(ds.data_vars) == {"combined", "weights", "quality", "status"}
    assert ds["weights"].dims == ("x", "y", "coil") and ds["quality"].dims == ("x", "y") == ds["status"].dims
    assert np.array_equal(ds["combined"].values, out.values) and ds.attrs == out.attrs
    got = dict(y=out.values, w=ds["weights"].values, quality=ds["quality"].values, status=ds["status"].values, kernel="")
    _check(got, want, what="(x, y, coil, time)")
    # coil in front: addressed where it is
    xt = np.ascontiguousarray(np.moveaxis(x.reshape(6, 8, 40), 1, 0))  # (coil, x, time)
    d2 = _labeled(xt, ("coil", "x", "time"))
    o2 = d2.xmr.combine_coils(return_weights=True)
    assert o2["combined"].dims == ("x", "time") and o2["weights"].dims == ("x", "coil")
    assert np.array_equal(o2["combined"].values, out.values.reshape(6, 40))
    assert np.array_equal(o2["weights"].values, ds["weights"].values.reshape(6, 8))
    # time not last: one copy, the same numbers, time where it was
    d3 = _labeled(np.ascontiguousarray(np.moveaxis(xt, 2, 1)), ("coil", "time", "x"))
    o3 = d3.xmr.combine_coils()
    assert o3.dims == ("time", "x") and np.array_equal(o3.values, o2["combined"].values.T)


def test_tail_noise_covariance_equals_the_matrix_passed():
    from xmris_amd.processing.coils import tail_points

    x = orc.make_data(6, 8, 1, 60, seed=71)[:, :, 0, :]
    da = _labeled(x, ("x", "coil", "time"))
    k = tail_points(60)
    assert k == 12
    t = np.moveaxis(x[:, :, -k:], 1, 0).reshape(8, -1)
    psi = t @ t.conj().T / t.shape[1]
    # the estimate itself: window, pooling and normalisation.  A sum of S products is off by at most ~S eps of
    # sum |a_i| |a_j| / S <= sqrt(psi_ii psi_jj) (Cauchy-Schwarz); 4 S eps leaves room for the complex products
    from xmris_amd.processing.coils import _tail_cov
    import torch

    est = _tail_cov(torch.from_numpy(x).to("cuda"), 1, 2)
    d = np.sqrt(np.diag(psi).real)
    assert np.all(np.abs(est - psi) <= 4 * t.shape[1] * EPS * np.outer(d, d)), np.abs(est - psi).max()
    assert np.array_equal(est, est.conj().T)
    a = da.xmr.combine_coils(noise_cov="tail", return_weights=True)
    b = da.xmr.combine_coils(noise_cov=psi, return_weights=True)
    want = orc.combine_batch(x, coil_axis=1, psi=psi)
    for r in (a, b):  # the two matrices agree to rounding, so the results do within the oracle's bound
        _check(dict(y=r["combined"].values, w=r["weights"].values, quality=r["quality"].values,
                    status=r["status"].values, kernel=""), want, what="tail")


def test_samples_whose_gram_matrix_overflows_are_reported():
    """Finite samples around 1e160: R R^H is inf.  Status 2 like a non-finite sample, the neighbours untouched."""
    x = orc.make_data(4, 8, 1, 40, seed=91)
    big = x.copy()
    big[1] *= 1e160
    big[2] *= 1e80  # G is finite, its squared norm is not
    for method in ("svd", "svd_fma", "first_point"):
        got = _run(big, method=method)
        bad = [1] if method == "first_point" else [1, 2]  # first_point forms no matrix: 1e80 is an ordinary voxel to it
        good = [v for v in range(4) if v not in bad]
        clean = _run(big[good], method=method)
        assert [int(s) for s in got["status"].ravel()] == [2 if v in bad else 0 for v in range(4)], (method, got["status"])
        assert not got["y"][bad].any() and not got["w"][bad].any() and np.all(np.isnan(got["quality"][bad]))
        for k in OUT:
            assert np.array_equal(got[k][good], clean[k]), (method, k)


# ---- 8b. scale --------------------------------------------------------------------------------------------------------
def _scaled(x, e):
    if x.dtype == np.complex64:
        return (x * np.float32(2.0 ** e)).astype(np.complex64)
    return np.ldexp(x.real, e) + 1j * np.ldexp(x.imag, e)


@pytest.mark.parametrize("dtype", ["complex128", "complex64"])
def test_a_power_of_two_scale_changes_no_bit(dtype):
    """Every operation is homogeneous, every threshold relative, and a power of two commutes with rounding: the weights,
    the quality and the status of 2^k x have the bits of x's, y is exactly 2^k times x's."""
    x, _ = _case("c8_n63_v37", dtype)
    base = _run(x)
    assert np.all(base["status"] == 0)
    for e in (40, -40):
        got = _run(_scaled(x, e))
        for k in ("w", "quality", "status"):
            assert np.array_equal(got[k], base[k]), (e, k)
        assert np.array_equal(got["y"], _scaled(base["y"], e)), e


def test_samples_at_the_ends_of_the_exponent_range():
    """complex128.  x 2^-300: R R^H is 2^-600 times what it was, its square underflows to zero; the Jacobi stopping test
    takes its norms on a scaled G, so the voxels are combined as their unscaled selves (status 0, weights and quality
    within COIL_TOL of the unscaled run, y scaled).  x 2^300: the squared norm of R R^H overflows, the documented
    status 2 with y and w zero and the quality NaN."""
    x, want = _case("c8_n63_v37", "complex128")
    base, got = _run(x), _run(_scaled(x, -300))
    back = dict(got, y=_scaled(got["y"], 300))
    print(f"2^-300: status {np.unique(got['status'])}, bits equal {_same(back, base)}")
    _check(back, dict(want, y=base["y"], w=base["w"], quality=base["quality"]), what="x 2^-300 against x")
    big = _run(_scaled(x, 300))
    assert np.all(big["status"] == 2) and not big["y"].any() and not big["w"].any() and np.all(np.isnan(big["quality"]))


# ---- 9. chaining ------------------------------------------------------------------------------------------------------
def test_result_feeds_the_single_channel_chain():
    x = orc.make_data(5, 8, 1, 64, seed=81, snr=(20.0, 30.0))[:, :, 0, :]
    da = _labeled(x, ("x", "coil", "time"))
    want = orc.combine_batch(x, coil_axis=1)
    chain = lambda a: a.xmr.zero_fill(target_points=128).xmr.apodize_exp(lb=2.0).xmr.to_spectrum().xmr.autophase()  # noqa: E731
    got = chain(da.xmr.combine_coils())
    ref = chain(_labeled(want["y"], ("x", "time")))
    assert got.dims == ref.dims and set(got.coords) == set(ref.coords)
    # the bounds of the existing chain-against-oracle tests (tests/test_gpu_accessor.py)
    assert abs(got.attrs["phase_p0"] - ref.attrs["phase_p0"]) < 1e-6 and abs(got.attrs["phase_p1"] - ref.attrs["phase_p1"]) < 1e-6
    np.testing.assert_allclose(got.values, ref.values, rtol=0, atol=1e-9 * np.abs(ref.values).max())
