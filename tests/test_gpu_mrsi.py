"""k_axis_dft / xm_axis_dft / to_image / to_kspace on the GPU against tests/_mrsi_oracle.py.  The bound is the one of
tests/test_mrsi.py: MRSI_TOL (16 x the disagreement of the oracle's two routes, measured on the CPU) in units of the
pencil's U, plus for complex64 the roundings the definition itself makes, eps32 U / eps64 per pass.  The staged route is
held to this project's own FFT tolerances (tests/test_gpu_kernels.py: 1e-5 of the largest magnitude for complex64,
1e-12 for complex128), once per pass."""
import functools

import numpy as np
import pytest

import _mrsi_oracle as orc
from test_mrsi import MRSI_TOL, bound, labeled_case

pytestmark = pytest.mark.gpu

DTYPES = ["complex64", "complex128"]
FFT_TOL = {"complex64": 1e-5, "complex128": 1e-12}


def _up(a):
    import torch

    return torch.from_numpy(np.array(a)).to("cuda")  # (a copy: the shared cases are read-only)


def _report(what, got, want, b):
    d = np.abs(got - want)
    print(f"{what}: {float((d / np.where(b > 0, b, 1.0)).max()):.3f} of its bound")
    assert np.all(d <= b), (what, float((d / np.where(b > 0, b, 1.0)).max()))


# ---- 1. the kernel applies a general matrix ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _matrix_case(shape):
    n_outer, n, m, n_inner = shape
    x = orc.make((n_outer, n, n_inner), seed=sum(shape))
    t = orc.make((m, n), seed=sum(shape) + 1)
    return x, t


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (2, 2, 3, 1), (3, 7, 16, 3), (1, 12, 12, 65), (1, 5, 64, 64),
                                   (2, 64, 64, 130), (4, 16, 16, 257), (2, 20, 24, 100), (1, 3, 32, 64)])
def test_matrix_parity(shape, dtype):
    from xmris_amd import device as dev

    x, t = _matrix_case(shape)
    x = x.astype(dtype)
    xd = _up(x)
    got = dev.axis_dft(xd, 1, t)
    assert "k_axis_dft" in dev.last_kernel(), dev.last_kernel()
    assert got.dtype == xd.dtype and tuple(got.shape) == (shape[0], shape[2], shape[3]) and got.is_contiguous()
    assert np.array_equal(xd.cpu().numpy(), x)  # the input is untouched
    x128 = x.astype(np.complex128)
    want = np.einsum("pj,oji->opi", t, x128)
    u = orc.EPS * np.einsum("pj,oji->opi", np.abs(t), np.abs(x128))  # |T| in place of the DFT weights
    _report(f"{shape} {dtype} {dev.last_kernel()}", got.cpu().numpy(), want, bound(u, dtype))


def test_any_axis_and_a_device_table():
    import torch

    from xmris_amd import device as dev

    x = orc.make((3, 5, 4, 6), seed=31)
    xd = _up(x)
    for axis in (0, 1, 2, 3, -1):
        n = x.shape[axis]
        t = orc.make((n + 2, n), seed=32 + axis)
        got = dev.axis_dft(xd, axis, torch.from_numpy(t).to("cuda"))
        u = orc.EPS * orc.apply_table(np.abs(x), axis, np.abs(t)).real
        _report(f"axis {axis}", got.cpu().numpy(), orc.apply_table(x, axis, t), bound(u))
    with pytest.raises(ValueError, match="table"):
        dev.axis_dft(xd, 1, np.ones((4, 4), complex))
    with pytest.raises(Exception, match="64"):
        dev.axis_dft(xd, 1, np.ones((65, 5), complex))
    empty = dev.axis_dft(xd[:0], 1, np.ones((7, 5), complex))
    assert tuple(empty.shape) == (0, 7, 4, 6)


# ---- 2. to_image / to_kspace against the oracle -------------------------------------------------------------------------
def _device_case(name, dtype):
    from xmris_amd import LabeledArray

    la, kw, fn, want, u, d = labeled_case(name, np.dtype(dtype).type)
    dla = LabeledArray(_up(la.values), la.dims, la.coords, la.attrs, la.name)
    return dla, la.values, kw, fn, want, u, d


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(orc.PARITY_CASES))
def test_parity_with_the_oracle(name, dtype):
    import xmris_amd
    from xmris_amd import device as dev

    dla, host, kw, fn, want, u, d = _device_case(name, dtype)
    got = getattr(xmris_amd, fn)(dla, **kw)
    assert "k_axis_dft" in dev.last_kernel()
    assert got.is_device_resident and got.dtype == np.dtype(dtype) and got.shape == want.shape
    assert np.array_equal(dla.values, host)
    _report(f"{name} {dtype}", got.values, want, bound(u, dtype, d))


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_permuted_input_gives_the_same_result(dtype):
    from xmris_amd import LabeledArray, to_image

    dla, host, kw, fn, want, u, d = _device_case("coil3_7x12_to_16x12_hamming", dtype)
    ref = to_image(dla, **kw).values
    xt = dla.data.permute(3, 2, 0, 1).contiguous().permute(2, 3, 1, 0)  # the same values, time-major in memory
    assert not xt.is_contiguous() and tuple(xt.shape) == host.shape
    got = to_image(LabeledArray(xt, dla.dims, dla.coords), **kw)
    assert np.array_equal(got.values, ref)
    assert not xt.is_contiguous() and np.array_equal(xt.cpu().numpy(), host)  # unmodified
    _report(f"permuted {dtype}", got.values, want, bound(u, dtype, d))


# ---- 3. routes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["coil3_7x12_to_16x12_hamming", "4x6x5_to_8x6x5_custom", "kspace_6x5_to_9x9", "time_first_grid_last"])
def test_kernel_and_staged_routes_agree(name, dtype):
    import xmris_amd
    from xmris_amd import device as dev

    dla, host, kw, fn, want, u, d = _device_case(name, dtype)
    a = getattr(xmris_amd, fn)(dla, **kw).values
    assert "k_axis_dft" in dev.last_kernel()
    b = getattr(xmris_amd, fn)(dla, _staged=True, **kw).values
    assert "k_axis_dft" not in dev.last_kernel(), dev.last_kernel()
    staged_bound = np.full(want.shape, d * FFT_TOL[dtype] * np.abs(want).max())
    _report(f"{name} {dtype} kernel", a, want, bound(u, dtype, d))
    _report(f"{name} {dtype} staged", b, want, staged_bound)
    _report(f"{name} {dtype} kernel against staged", a, b, bound(u, dtype, d) + staged_bound)


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_matrix_of_96_takes_the_staged_route(dtype):
    from xmris_amd import LabeledArray, to_image
    from xmris_amd import device as dev

    x = orc.make((6, 40), seed=41).astype(dtype)
    la = LabeledArray(_up(x), ("kx", "time"), {"kx": np.arange(6.0) - 3})
    got = to_image(la, dim="kx", matrix=96, filter="hamming", shift=0.5)
    assert "k_axis_dft" not in dev.last_kernel() and got.shape == (96, 40), dev.last_kernel()
    want = orc.reconstruct(x.astype(np.complex128), [0], 96, "hamming", 0.5)
    _report(f"6 -> 96 {dtype}", got.values, want, np.full(want.shape, FFT_TOL[dtype] * np.abs(want).max()))


# ---- 4. locality ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_nan_stays_in_its_pencil(dtype):
    from xmris_amd import device as dev

    x = orc.make((3, 7, 70), seed=51).astype(dtype)
    t = orc.make((16, 7), seed=52)
    clean = dev.axis_dft(_up(x), 1, t).cpu().numpy()
    bad = x.copy()
    bad[1, 4, 66] = np.nan
    got = dev.axis_dft(_up(bad), 1, t).cpu().numpy()
    hit = np.zeros(clean.shape, bool)
    hit[1, :, 66] = True
    assert np.isfinite(clean).all() and not np.isfinite(got[hit]).any()
    assert np.array_equal(got[~hit], clean[~hit])
