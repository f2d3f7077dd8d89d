"""The long-transform path (`pipeline_big` of csrc/xm_bigfft.inc: the four-step algorithm over global memory, and chirp-z
on top of it) against numpy.fft in fp64: the flags that `big_load` / `big_store` fold in, the lengths that
`xm_fft_supported` promises up to 2^22, the second turn of the row-chunk loop, and strided input rows.

Bounds, relative to the largest magnitude of the reference: 4 x TIGHT of tests/test_gpu_kernels.py (the project's figure for
its four-step and chirp-z lengths, set at lengths up to 2^16) for lengths up to 65536, and that times log2(n) / 16 beyond
them (the rounding error of an FFT grows with log n).  Every case prints its share of the bound
(profiles/bigfft/gpu_test_figures.txt)."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TIGHT = {"complex64": 2e-6, "complex128": 1e-13}  # tests/test_gpu_kernels.py
DTYPES = ["complex64", "complex128"]
ODD_LONG = 300007  # a prime: chirp-z with M = 2^20
# 12288 = 32 x 384: a direct split whose first factor is a single tile wide; 32768 = 128 x 256; the last two: odd,
# chirp-z with M = 32768 and 65536
FLAG_LENGTHS = [12288, 32768, 9001, 20011]


@pytest.fixture(scope="module")
def dev():
    import torch

    from xmris_amd import device

    assert torch.cuda.is_available(), "GPU tests need a HIP device (no CPU fallback exists)"
    return device


def _rand(shape, dtype, seed=0):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(dtype)


def _relerr(got, ref):
    return float(np.abs(got - ref).max() / np.abs(ref).max())


def bound(dtype, n):
    return 4 * TIGHT[dtype] * max(1.0, math.log2(n) / 16)


# ---- 1. the folded-in rolls, conjugates and scales ---------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", FLAG_LENGTHS)
def test_flags_on_long_lengths(dev, n, dtype):
    """Every case of test_gpu_kernels.test_fft_flags.  On the odd lengths the input roll (n + 1) // 2 and the output roll
    n // 2 differ."""
    x = _rand((3, n), dtype, seed=3 + n)
    xd = dev.to_device(x)
    x128 = x.astype(np.complex128)
    rolled = np.roll(x128, (n + 1) // 2, axis=1)
    want = {
        "shift-out": (dict(shift_out=True), np.roll(np.fft.fft(x128, axis=1, norm="ortho"), n // 2, axis=1)),
        "inverse shift-in": (dict(inverse=True, shift_in=True), np.fft.ifft(rolled, axis=1, norm="ortho")),
        "both rolls": (dict(shift_in=True, shift_out=True), np.roll(np.fft.fft(rolled, axis=1, norm="ortho"), n // 2, axis=1)),
        "inverse both rolls": (dict(inverse=True, shift_in=True, shift_out=True),
                               np.roll(np.fft.ifft(rolled, axis=1, norm="ortho"), n // 2, axis=1)),
        "un-normalised": (dict(ortho=False), np.fft.fft(x128, axis=1)),
        "1/N inverse": (dict(inverse=True, ortho=False), np.fft.ifft(x128, axis=1)),
    }
    shares = {}
    for name, (flags, ref) in want.items():
        got = dev.fft(xd, 1, **flags).cpu().numpy()
        assert got.dtype == np.dtype(dtype)
        shares[name] = _relerr(got, ref) / bound(dtype, n)
    print(f"flags n {n} {dtype}: " + ", ".join(f"{k} {v:.3f}" for k, v in shares.items()) + " of the bound")
    assert max(shares.values()) <= 1.0, shares


# ---- 2. the promised range ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1 << 20, 1 << 22, ODD_LONG])
def test_the_promised_range(dev, n, dtype):
    assert dev.fft_supported(n, complex128=dtype == "complex128")
    x = _rand((2, n), dtype, seed=n % 1000)
    xd = dev.to_device(x)
    ref = np.fft.fft(x.astype(np.complex128), axis=1, norm="ortho")
    plain = _relerr(dev.fft(xd, 1).cpu().numpy(), ref) / bound(dtype, n)
    shifted = _relerr(dev.fft(xd, 1, shift_out=True).cpu().numpy(), np.roll(ref, n // 2, axis=1)) / bound(dtype, n)
    print(f"range n {n} {dtype}: plain {plain:.3f}, shift-out {shifted:.3f} of the bound {bound(dtype, n):.2e}")
    assert plain <= 1.0 and shifted <= 1.0


# ---- 3. the second turn of the row-chunk loop --------------------------------------------------------------------------
@pytest.mark.parametrize("n,n_rows,rows_per", [(ODD_LONG, 67, 64), (1 << 22, 17, 16)], ids=["chirp-z", "direct"])
def test_second_row_chunk(dev, n, n_rows, rows_per):
    """complex128 rows beyond one chunk of the scratch (2^30 bytes / (M x 16 bytes) rows): the later chunks take their
    input, output and arg-max slots at an offset.  Rows are three base rows times distinct constants c_k, built and
    compared on the device; the reference is three CPU transforms."""
    import torch

    dtype = "complex128"
    m = n if n == 1 << 22 else 1 << 20
    assert (1 << 30) // (m * 16) == rows_per < n_rows
    n_in = n - 12345
    base = _rand((3, n_in), dtype, seed=n_rows)
    w = np.exp(-3.0 * np.arange(n) / n)
    ph = np.exp(1j * (0.3 + 2.0 * np.arange(n) / n))
    spec = np.roll(np.fft.fft(np.pad(base, [(0, 0), (0, n - n_in)]) * w, axis=1, norm="ortho"), n // 2, axis=1)
    top = np.sort(np.abs(spec), axis=1)[:, -2:]
    assert ((top[:, 1] - top[:, 0]) / top[:, 1]).min() > 1e-6  # the arg-max of every base row is not a near tie
    amax_ref = np.argmax(np.abs(spec), axis=1)
    k = torch.arange(n_rows, device="cuda", dtype=torch.float64)
    c = torch.polar(1.0 + 0.01 * k, 0.7 * k)
    x = torch.from_numpy(base).cuda()[torch.arange(n_rows, device="cuda") % 3] * c[:, None]
    ref = torch.from_numpy(spec * ph).cuda()
    wd, phd = torch.from_numpy(w).cuda(), torch.from_numpy(ph).cuda()
    r = dev.pipeline_fused(x, n, 0, window=wd, phase_table=phd, want_argmax=True)
    scale = float(ref.abs().max())
    err = max(float((r.out[i] - c[i] * ref[i % 3]).abs().max() / (abs(complex(c[i])) * scale)) for i in range(n_rows))
    share = err / bound(dtype, n)
    print(f"row chunks n {n} rows {n_rows}: {share:.3f} of the bound {bound(dtype, n):.2e}")
    assert share <= 1.0
    want_idx = amax_ref[np.arange(n_rows) % 3]
    want_max = np.abs(spec).max(axis=1)[np.arange(n_rows) % 3] * np.abs(c.cpu().numpy())
    np.testing.assert_array_equal(r.argidx.cpu().numpy(), want_idx)
    np.testing.assert_allclose(np.sqrt(r.absmax2.cpu().numpy()), want_max, rtol=20 * bound(dtype, n))
    del r
    only = dev.pipeline_fused(x, n, 0, window=wd, phase_table=None, want_out=False, want_argmax=True)
    np.testing.assert_array_equal(only.argidx.cpu().numpy(), want_idx)
    np.testing.assert_allclose(np.sqrt(only.absmax2.cpu().numpy()), want_max, rtol=20 * bound(dtype, n))


# ---- 4. strided rows ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [32768, 20011])
def test_strided_rows_as_shift_fractional_reads_them(dev, n, dtype):
    """device.shift_fractional on rows that start 5 samples into a wider buffer (pointer offset + row stride):
    ifft(fft(x[:, 5:]) * table).  Two transforms with a unit-modulus table between them: twice the bound of one."""
    wide = _rand((3, n + 5), dtype, seed=n)
    table = np.exp(2j * np.pi * np.fft.fftfreq(n) * 0.37)
    ref = np.fft.ifft(np.fft.fft(wide[:, 5:].astype(np.complex128), axis=1) * table, axis=1)
    got = dev.shift_fractional(dev.to_device(wide), 1, 5, table).cpu().numpy()
    assert got.shape == (3, n) and got.dtype == np.dtype(dtype)
    share = _relerr(got, ref) / (2 * bound(dtype, n))
    print(f"strided n {n} {dtype}: {share:.3f} of twice the bound")
    assert share <= 1.0
