"""k_shift_time / xm_shift_time / shift_time / correct_readout_time on the GPU against tests/_shift_oracle.py (complex128).

The bound is 4 x TIGHT[dtype] of tests/test_gpu_kernels.py -- this project's figure for its other kernel of two
transforms -- per row, relative to the oracle row's largest magnitude.  Lengths without a fused kernel take the staged
route and the factor 4 that test_gpu_kernels.py gives its chirp-z and four-step lengths, on top.  Every case prints its
share of the bound (profiles/shift/gpu_test_figures.txt).  Shapes are the smallest that reach every path: one stage
without an exchange (16), two stages (32, 256), the odd factor last (384, 640) and first (768), the widest workgroups
(8192, 16384) and the largest exchange buffer; N = L and the odd N = L/2 + 3, whose complex64 rows start 8 bytes off a
16-byte boundary."""
import numpy as np
import pytest

import _grid_oracle as grid_orc
import _shift_oracle as orc

pytestmark = pytest.mark.gpu

TIGHT = {"complex64": 2e-6, "complex128": 1e-13}  # tests/test_gpu_kernels.py
DTYPES = ["complex64", "complex128"]
FUSED_L = [16, 32, 256, 384, 640, 768, 2048, 8192]
STAGED_FACTOR = 4  # test_gpu_kernels.py: TIGHT x 4 for its chirp-z (1000, 1972) and four-step (32768) lengths


@pytest.fixture(autouse=True)
def torch_first():
    """torch brings its HIP runtime before the library is loaded (`shift_time_fused` alone would load the library first,
    and the process would hold two runtimes)."""
    import torch  # noqa: F401


def bound(dtype, staged=False):
    return 4 * TIGHT[dtype] * (STAGED_FACTOR if staged else 1)


def _up(x):
    from xmris_amd import device as dev

    return dev.to_device(np.ascontiguousarray(x))


def _run(x, phi, L, n_delay=None, delay_div=1, staged=False):
    from xmris_amd import device as dev

    y = dev.shift_time(_up(x), 1, phi, n_delay, delay_div, L, staged=staged)
    return y.cpu().numpy(), dev.last_kernel()


def _lengths(dtype):
    return FUSED_L + ([16384] if dtype == "complex64" else [])


# ---- 1. parity ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_parity_on_every_fused_path(dtype):
    from xmris_amd import device as dev

    for L in _lengths(dtype):
        assert dev.shift_time_fused(L, dtype == "complex128")
        for N in (L, L // 2 + 3):
            x = orc.make((len(orc.PHIS), N), seed=L + N, dtype=dtype)
            got, kernel = _run(x, orc.PHIS, L)
            share = orc.row_gap(got, orc.shift_fft(x, orc.PHIS, L)) / bound(dtype)
            print(f"parity {dtype} L {L} N {N} {kernel}: {share.max():.3f} of its bound (rows {np.round(share, 3).tolist()})")
            assert got.dtype == np.dtype(dtype) and got.shape == x.shape
            assert kernel.startswith("k_shift_time<") and f"{L}" in kernel
            assert share.max() <= 1.0


# ---- 2. which row takes which delay ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_delay_indexing(dtype):
    L, N = 256, 200
    x = orc.make((12, N), seed=12, dtype=dtype)  # (2 outer x S = 3 x 2 inner)
    per_sample = np.array([0.41, -1.3, 2.75])
    got, _ = _run(x, per_sample, L, n_delay=3, delay_div=2)
    want = orc.shift_fft(x.reshape(2, 3, 2, N), per_sample[None, :, None], L).reshape(12, N)
    share = orc.row_gap(got, want).max() / bound(dtype)
    print(f"delay indexing {dtype} per sample: {share:.3f} of its bound")
    assert share <= 1.0
    per_row = np.linspace(-3.0, 3.0, 12) + 0.013
    got, _ = _run(x, per_row, L, n_delay=12, delay_div=1)
    share = orc.row_gap(got, orc.shift_fft(x, per_row, L)).max() / bound(dtype)
    print(f"delay indexing {dtype} per row: {share:.3f} of its bound")
    assert share <= 1.0


# ---- 3. the two routes -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_fused_and_staged_agree(dtype):
    for L, N in ((256, 256), (640, 323), (2048, 2048)):
        x = orc.make((len(orc.PHIS), N), seed=7 * L + N, dtype=dtype)
        fused, k1 = _run(x, orc.PHIS, L)
        staged, k2 = _run(x, orc.PHIS, L, staged=True)
        assert k1.startswith("k_shift_time<") and not k2.startswith("k_shift_time<")
        share = orc.row_gap(fused, staged).max() / (2 * bound(dtype))
        print(f"fused / staged {dtype} L {L} N {N}: {share:.3f} of twice the bound")
        assert share <= 1.0


# ---- 4. a row does not depend on its batch ------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_batch_independence(dtype):
    for L in (32, 256, 2048):  # 64, 16 and 2 rows per workgroup
        x = orc.make((67, L), seed=L, dtype=dtype)
        phi = np.linspace(-2.0, 2.0, 67) + 0.1
        batch, _ = _run(x, phi, L)
        alone, _ = _run(x[41:42], phi[41:42], L)
        assert np.array_equal(alone[0].view(np.uint8), batch[41].view(np.uint8))


# ---- 5. exact properties ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_roll_round_trip_and_untouched_input(dtype):
    from xmris_amd import device as dev

    L = 768
    x = orc.make((4, L), seed=5, dtype=dtype)
    shifts = np.array([1.0, -3.0, 773.0, 0.0])
    xd = _up(x)
    got = dev.shift_time(xd, 1, shifts, 4, 1, L).cpu().numpy()
    want = np.stack([np.roll(x[i], int(s)) for i, s in enumerate(shifts)])
    share = orc.row_gap(got, want).max() / bound(dtype)
    print(f"integer roll {dtype}: {share:.3f} of its bound")
    assert share <= 1.0
    assert np.array_equal(xd.cpu().numpy().view(np.uint8), x.view(np.uint8))  # the input is untouched
    phi = np.array([0.37, -12.81, 1000.25, 0.5])
    there = dev.shift_time(xd, 1, phi, 4, 1, L)
    back = dev.shift_time(there, 1, -phi, 4, 1, L).cpu().numpy()
    share = orc.row_gap(back, x).max() / (2 * bound(dtype))
    print(f"round trip {dtype}: {share:.3f} of twice the bound")
    assert share <= 1.0


# ---- 6. lengths without a fused kernel -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_staged_lengths(dtype):
    from xmris_amd import device as dev

    for L in [1000, 1972, 32768] + ([16384] if dtype == "complex128" else []):
        assert not dev.shift_time_fused(L, dtype == "complex128")
        x = orc.make((len(orc.PHIS), L), seed=L, dtype=dtype)
        got, kernel = _run(x, orc.PHIS, L)
        assert not kernel.startswith("k_shift_time<")
        share = orc.row_gap(got, orc.shift_fft(x, orc.PHIS, L)) / bound(dtype, staged=True)
        print(f"staged {dtype} L {L} (last launch {kernel}): {share.max():.3f} of its bound")
        assert share.max() <= 1.0


# ---- 7. the public layer, end to end ------------------------------------------------------------------------------------------
def _device_array(x, dims, **coords):
    from xmris_amd import LabeledArray

    return LabeledArray(_up(x), dims, coords, {"note": "kept"}, "fid")


@pytest.mark.parametrize("dtype", DTYPES)
def test_correct_readout_time(dtype):
    from xmris_amd import ATTRS, device as dev, readout_offsets

    dt = 0.5e-3
    x = orc.make((2, 5, 256), seed=3, dtype=dtype)
    t = np.arange(256) * dt
    off = readout_offsets(5, 0.2 * dt, start=0.05 * dt)
    want = orc.shift_fft(x, off[None, :] / dt)
    y = _device_array(x, ("coil", "sample", "time"), time=t).xmr.correct_readout_time(off)
    assert dev.last_kernel().startswith("k_shift_time<")
    assert y.is_device_resident and y.dims == ("coil", "sample", "time") and y.dtype == np.dtype(dtype)
    assert y.attrs == {"note": "kept", ATTRS.time_shift_pad_to: 256, ATTRS.readout_time_corrected: True}
    share = orc.row_gap(y.values, want).max() / bound(dtype)
    first = _device_array(np.ascontiguousarray(np.moveaxis(x, -1, 0)), ("time", "coil", "sample"), time=t)
    z = first.xmr.correct_readout_time(off)
    assert z.dims == ("time", "coil", "sample")
    share2 = orc.row_gap(np.moveaxis(z.values, 0, -1), want).max() / bound(dtype)
    print(f"correct_readout_time {dtype}: {share:.3f} of its bound, time first {share2:.3f}")
    assert share <= 1.0 and share2 <= 1.0
    assert np.array_equal(np.moveaxis(z.values, 0, -1), y.values)


def test_nufft_adjoint_with_readout_time():
    """The 2d_random case of _grid_oracle, (3, 37 samples, 5 time points): the shift of a 5-point row takes the staged
    route, within 16 TIGHT = 1.6e-12 of the row's largest magnitude; the gridding chain is held to 2e-12 of the largest
    magnitude as tests/test_gpu_grid.py holds it.  The bound is their sum."""
    x, traj, matrix, a0, W, axis, *_ = grid_orc.parity_case("2d_random")
    dt = 1e-3
    off = np.linspace(0.0, 0.9, x.shape[axis]) * dt
    la = _device_array(x, ("coil", "sample", "time"), time=np.arange(x.shape[-1]) * dt)
    got = la.xmr.nufft_adjoint(traj, matrix, a0, W, readout_time=off)
    want = grid_orc.nufft_adjoint(orc.shift_fft(x, off[None, :] / dt), traj, matrix, a0, W, axis=axis)
    err = np.abs(got.values - want).max() / np.abs(want).max()
    print(f"nufft_adjoint(readout_time): {err:.3e} of the largest magnitude (bound 3.6e-12)")
    assert got.dims == ("coil", "x", "y", "time") and err <= 3.6e-12
    plain = la.xmr.nufft_adjoint(traj, matrix, a0, W)
    assert np.abs(got.values - plain.values).max() > 1e-3 * np.abs(want).max()  # the keyword does something


def test_refusals_write_nothing():
    """Bad arguments return XM_ERR_INVALID_ARG before any launch: the output keeps its bits."""
    import torch

    from xmris_amd import _lib

    lib = _lib.load()
    xd = _up(orc.make((5, 200), seed=1, dtype=np.complex64))
    out = torch.full((5, 200), 7.0, dtype=torch.complex64, device="cuda")
    frac = torch.zeros(5, dtype=torch.float64, device="cuda")
    ok = dict(orc.ABI_OK, **{"in": xd.data_ptr(), "out": out.data_ptr(), "frac": frac.data_ptr()})
    for change in ({"L": 128}, {"L": 1000}, {"n": 0}, {"n_delay": 0}, {"delay_div": 0}, {"dtype": 2}, {"out": xd.data_ptr()},
                   {"frac": 0}, {"in": xd.data_ptr() + 4}):
        a = dict(ok, **change)
        assert lib.xm_shift_time(*[a[k] for k in orc.ABI_ORDER], None) == _lib.XM_ERR_INVALID_ARG, change
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
