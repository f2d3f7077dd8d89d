"""CPU tests of shift_time / correct_readout_time / readout_offsets: the oracle's own properties
(integer delays are rolls, on-grid exponentials are exact, round trip and adjoint at L = N, a delay of 1000.25 dwells is
as exact as one of 0.25), the physical case of three damped lines, the Python layer on a numpy stand-in for
``device.shift_time`` (dims, coordinates, attrs, names, the row rule of the delays, the ``readout_time`` keyword of the
gridding calls), every validation error before the device is reached, and xm_shift_time's refusals without a GPU.

The physical case follows the issue's statement (tau = r dt / 50, r < 50): the oracle gives 1.494 uncorrected and 0.0439
corrected.  (With tau centred on zero, [-dt/2, dt/2), the same code gives 0.855 and 0.0353.)

The tests of the oracle alone import nothing from the package and pass without the feature; all others fail without it."""
import os
import re

import numpy as np
import pytest

import _grid_oracle as grid_orc
import _shift_oracle as orc

# tests/tool_shift_tolerance.py, recorded in profiles/shift/tolerance.txt
ROUTE_GAP = 9.991e-16
UNCORRECTED = 1.4945
CORRECTED = 4.3868e-02
PROFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "shift", "tolerance.txt")
EXACT = 64 * orc.EPS  # "exact" for the oracle: a few roundings of two length-L transforms


# ---- the oracle -----------------------------------------------------------------------------------------------------------
def test_recorded_figures_match_their_tool():
    text = open(PROFILE).read()
    assert float(re.search(r"largest disagreement: ([0-9.e+-]+)", text).group(1)) == ROUTE_GAP
    assert float(re.search(r"uncorrected: ([0-9.e+-]+)", text).group(1)) == UNCORRECTED
    assert float(re.search(r" corrected: ([0-9.e+-]+)", text).group(1)) == CORRECTED
    gap = orc.worst_route_gap()
    print("route gap", gap)
    assert gap <= 2 * ROUTE_GAP


@pytest.mark.parametrize("L, N", [(16, 16), (64, 37), (384, 384), (1000, 1000)])
def test_integer_delays_are_rolls(L, N):
    x = orc.make((4, N), seed=L)
    shifts = (1, -3, L + 5, 0)
    want = np.stack([np.roll(np.pad(x[i], (0, L - N)), s)[:N] for i, s in enumerate(shifts)])
    for route in (orc.shift_fft, orc.shift_sums):
        gap = orc.row_gap(route(x, shifts, L), want).max()
        print(route.__name__, L, N, gap)
        assert gap <= EXACT


def test_on_grid_exponentials_are_exact():
    N = 96
    n = np.arange(N)

    def tone(k, late):  # exp(2 pi i k (n + late) / N), the integer part of the angle reduced on the integers
        return np.exp(2j * np.pi * (((k * n) % N) / N + k * late / N))

    for k, phi in ((5, 0.3), (-17, -2.6), (47, 0.5), (0, 11.2)):
        assert orc.row_gap(orc.shift_fft(tone(k, 0.0), phi), tone(k, -phi)) <= EXACT  # s(t_n - tau)
    # a row acquired tau late comes back on the grid
    assert orc.row_gap(orc.shift_fft(tone(7, 0.41), 0.41), tone(7, 0.0)) <= EXACT


@pytest.mark.parametrize("N", [32, 45, 640])
def test_round_trip_and_adjoint_at_full_length(N):
    x, y = orc.make((3, N), seed=N), orc.make((3, N), seed=N + 1)
    phi = np.array([0.37, -12.81, 1000.25])
    assert orc.row_gap(orc.shift_fft(orc.shift_fft(x, phi), -phi), x).max() <= EXACT
    lhs = np.sum(orc.shift_fft(x, phi) * y.conj(), axis=-1)
    rhs = np.sum(x * orc.shift_fft(y, -phi).conj(), axis=-1)
    scale = np.sqrt(np.sum(np.abs(x) ** 2, -1) * np.sum(np.abs(y) ** 2, -1))
    assert np.all(np.abs(lhs - rhs) <= EXACT * scale)
    # unitary: norms are kept (an odd N has no Nyquist bin; an even N's has the unit factor exp(i pi phi) too)
    assert np.allclose(np.sum(np.abs(orc.shift_fft(x, phi)) ** 2, -1), np.sum(np.abs(x) ** 2, -1), rtol=1e-13)


@pytest.mark.parametrize("L", [256, 384, 1000])
def test_a_large_delay_is_as_exact_as_its_fraction(L):
    x = orc.make((2, L), seed=L)
    for route in (orc.shift_fft, orc.shift_sums):
        gap = orc.row_gap(route(x, 1000.25), np.roll(route(x, 0.25), 1000, axis=-1)).max()
        print(route.__name__, L, gap)
        assert gap <= EXACT


def test_physical_case():
    x, tau, truth, dt = orc.physical_case()
    assert x.shape == (50, 256) and tau[0] == 0 and tau[-1] < dt
    before = orc.spectral_error(x, truth)
    after = orc.spectral_error(orc.shift_fft(x, tau / dt), truth)
    print("uncorrected", before, "corrected", after)
    assert after <= before / 10
    assert before == pytest.approx(UNCORRECTED, rel=0.01) and after == pytest.approx(CORRECTED, rel=0.01)


# ---- the Python layer on a numpy stand-in for the device -------------------------------------------------------------------
def np_shift_time(x, axis, frac, n_delay=None, delay_div=1, L=None, staged=False):
    """``device.shift_time`` in numpy: the row rule applied to the oracle."""
    xm = np.moveaxis(np.asarray(x), axis, -1)
    rows = xm.reshape(-1, xm.shape[-1])
    frac = np.asarray(frac, dtype=np.float64).reshape(-1)
    n_delay = len(frac) if n_delay is None else n_delay
    assert len(frac) == n_delay and delay_div >= 1
    phi = frac[(np.arange(len(rows)) // delay_div) % n_delay]
    y = orc.shift_fft(rows, phi, L).astype(rows.dtype)
    return np.ascontiguousarray(np.moveaxis(y.reshape(xm.shape), -1, axis))


@pytest.fixture
def numpy_device(monkeypatch):
    import _mrsi_oracle as mrsi_orc
    import _numpy_device
    from xmris_amd import device as dev

    _numpy_device.install(monkeypatch)
    calls = []

    def shift_time(x, axis, frac, n_delay=None, delay_div=1, L=None, staged=False):
        calls.append(("shift_time", len(np.atleast_1d(frac)), n_delay, delay_div, L))
        return np_shift_time(x, axis, frac, n_delay, delay_div, L)

    def axis_sparse(x, axis, table):
        calls.append(("axis_sparse",))
        A = np.zeros((table.n_rows, table.n))
        for r in range(table.n_rows):
            sl = slice(table.rowptr[r], table.rowptr[r + 1])
            np.add.at(A[r], table.col[sl], table.val[sl])
        return np.moveaxis(np.tensordot(A, x, axes=([1], [axis])), 0, axis).astype(x.dtype)

    def axis_dft(x, axis, table):
        calls.append(("axis_dft",))
        return mrsi_orc.apply_table(x, axis, np.asarray(table)).astype(x.dtype)

    monkeypatch.setattr(dev, "shift_time", shift_time)
    monkeypatch.setattr(dev, "axis_sparse", axis_sparse)
    monkeypatch.setattr(dev, "axis_dft", axis_dft)
    return calls


def labeled(x, dims, **coords):
    from xmris_amd import LabeledArray

    return LabeledArray(x, dims, coords, {"note": "kept"}, "fid")


DT = 2e-3


def test_shift_time_keeps_metadata_and_applies_the_row_rule(numpy_device):
    from xmris_amd import ATTRS, shift_time

    x = orc.make((3, 4, 20), seed=3)
    t = np.arange(20) * DT
    la = labeled(x, ("coil", "sample", "time"), time=t, coil=np.arange(3), label=("sample", np.arange(4) * 10.0, {"units": "us"}))
    # a scalar delay
    y = shift_time(la, 0.3 * DT)
    assert y.dims == la.dims and y.name == "fid" and y.attrs == {"note": "kept", ATTRS.time_shift_pad_to: 20}
    assert np.array_equal(y.coords["time"].values, t) and y.coords["label"].attrs == {"units": "us"}
    assert la.attrs == {"note": "kept"}
    assert orc.row_gap(y.values, orc.shift_fft(x, 0.3)).max() <= EXACT
    assert numpy_device[-1] == ("shift_time", 1, 1, 1, 20)
    # one delay per coil, per sample, per (coil, sample); pad_to
    per_coil = np.array([0.1, -0.2, 1.5])[:, None] * DT
    y = shift_time(la, per_coil, pad_to=32)
    assert numpy_device[-1] == ("shift_time", 3, 3, 4, 32) and y.attrs[ATTRS.time_shift_pad_to] == 32
    assert orc.row_gap(y.values, orc.shift_fft(x, per_coil / DT, 32)).max() <= EXACT
    per_sample = np.array([0.0, 0.25, 0.5, 0.75]) * DT
    y = la.xmr.shift_time(per_sample)
    assert numpy_device[-1] == ("shift_time", 4, 4, 1, 20)
    assert orc.row_gap(y.values, orc.shift_fft(x, per_sample[None, :] / DT)).max() <= EXACT
    both = orc.make((3, 4), seed=5).real * DT
    y = shift_time(la, both)
    assert numpy_device[-1] == ("shift_time", 12, 12, 1, 20)
    assert orc.row_gap(y.values, orc.shift_fft(x, both / DT)).max() <= EXACT
    # `dim` not last; the dwell from the keyword, the coordinate absent
    moved = labeled(np.ascontiguousarray(np.moveaxis(x, -1, 0)), ("time", "coil", "sample"))
    y = shift_time(moved, per_sample, dwell=DT)
    assert y.dims == ("time", "coil", "sample") and numpy_device[-1] == ("shift_time", 4, 4, 1, 20)
    assert orc.row_gap(np.moveaxis(y.values, 0, -1), orc.shift_fft(x, per_sample[None, :] / DT)).max() <= EXACT
    # real input becomes complex; an all-zero delay is a copy without a device call
    n_calls = len(numpy_device)
    r = shift_time(labeled(x.real.copy(), ("coil", "sample", "time"), time=t), 0.0)
    assert np.iscomplexobj(r.values) and np.array_equal(r.values, x.real) and len(numpy_device) == n_calls
    assert r.attrs[ATTRS.time_shift_pad_to] == 20
    assert np.iscomplexobj(shift_time(labeled(x.real.copy(), ("coil", "sample", "time"), time=t), DT).values)


def test_correct_readout_time_whatever_the_order_of_the_dims(numpy_device):
    from xmris_amd import ATTRS, correct_readout_time, readout_offsets

    S = 5
    off = readout_offsets(S, 0.2 * DT, start=0.1 * DT)
    x = orc.make((2, S, 3, 24), seed=9)
    t = np.arange(24) * DT
    want = orc.shift_fft(x, off[None, :, None] / DT)
    la = labeled(x, ("coil", "sample", "x", "time"), time=t)  # sample_dim not adjacent to dim
    y = correct_readout_time(la, off)
    assert y.dims == la.dims and y.name == "fid"
    assert y.attrs == {"note": "kept", ATTRS.time_shift_pad_to: 24, ATTRS.readout_time_corrected: True}
    assert numpy_device[-1] == ("shift_time", S, S, 3, 24)
    assert orc.row_gap(y.values, want).max() <= EXACT
    # time first, sample last
    perm = labeled(np.ascontiguousarray(np.transpose(x, (3, 2, 0, 1))), ("time", "x", "coil", "sample"), time=t)
    y = perm.xmr.correct_readout_time(off)
    assert y.dims == perm.dims and numpy_device[-1] == ("shift_time", S, S, 1, 24)
    assert orc.row_gap(np.transpose(y.values, (2, 3, 1, 0)), want).max() <= EXACT
    # the inverse is the forward-model direction: -offsets, and undoes the correction at L = N
    back = correct_readout_time(correct_readout_time(la, off), off, inverse=True)
    assert back.attrs[ATTRS.readout_time_corrected] is False
    assert orc.row_gap(back.values, x).max() <= EXACT
    assert orc.row_gap(correct_readout_time(la, off, inverse=True).values, orc.shift_fft(x, -off[None, :, None] / DT)).max() <= EXACT
    # other names
    named = labeled(x, ("coil", "shot", "x", "t"), t=t)
    assert np.array_equal(correct_readout_time(named, off, dim="t", sample_dim="shot").values, correct_readout_time(la, off).values)


def test_readout_offsets():
    from xmris_amd import readout_offsets

    assert np.array_equal(readout_offsets(6, 2.0), np.arange(6) * 2.0)
    assert np.array_equal(readout_offsets(6, 2.0, interleaves=2, start=1.0), 1.0 + np.array([0, 1, 2, 0, 1, 2]) * 2.0)
    assert np.array_equal(readout_offsets(6, 2.0, interleaves=6), np.zeros(6))
    for bad in (dict(interleaves=4), dict(interleaves=0), dict(interleaves=1.5)):
        with pytest.raises(ValueError, match="interleaves"):
            readout_offsets(6, 2.0, **bad)
    with pytest.raises(ValueError, match="n_samples"):
        readout_offsets(0, 2.0)
    with pytest.raises(ValueError, match="readout_dwell"):
        readout_offsets(6, np.nan)


def _grid_input():
    x, traj, matrix, a0, W, axis, A, want, u = grid_orc.parity_case("2d_random")
    dims = ["a", "b", "c"][:x.ndim]
    dims[axis] = "sample"
    dims[-1 if axis != x.ndim - 1 else 0] = "time"
    n_t = x.shape[dims.index("time")]
    return labeled(x, dims, time=np.arange(n_t) * DT), traj, matrix, a0, W


def test_readout_time_keyword_of_the_gridding_calls(numpy_device):
    from xmris_amd import correct_readout_time, degrid_kspace, grid_kspace, nufft_adjoint, nufft_forward

    la, traj, matrix, a0, W = _grid_input()
    off = np.linspace(0.0, 0.9, la.sizes["sample"]) * DT
    for fn in (grid_kspace, nufft_adjoint):
        plain = fn(la, traj, matrix, a0, W)
        none = fn(la, traj, matrix, a0, W, readout_time=None)
        assert np.array_equal(none.values, plain.values) and none.attrs == plain.attrs and none.dims == plain.dims
        del numpy_device[:]
        got = fn(la, traj, matrix, a0, W, readout_time=off)
        assert numpy_device[0][0] == "shift_time"  # before gridding
        want = fn(correct_readout_time(la, off), traj, matrix, a0, W)
        assert np.array_equal(got.values, want.values) and got.attrs == want.attrs and got.dims == want.dims
        assert not np.array_equal(got.values, plain.values)
        assert np.array_equal(getattr(la.xmr, fn.__name__)(traj, matrix, a0, W, readout_time=off).values, got.values)
    g = grid_kspace(la, traj, matrix, a0, W)
    img = nufft_adjoint(la, traj, matrix, a0, W)
    for fn, src in ((degrid_kspace, g), (nufft_forward, img)):
        plain = fn(src, traj, matrix, a0, W)
        none = fn(src, traj, matrix, a0, W, readout_time=None)
        assert np.array_equal(none.values, plain.values) and none.attrs == plain.attrs
        del numpy_device[:]
        got = fn(src, traj, matrix, a0, W, readout_time=off)
        assert numpy_device[-1][0] == "shift_time"  # after degridding
        want = correct_readout_time(plain, off, inverse=True)
        assert np.array_equal(got.values, want.values) and got.attrs == want.attrs and got.dims == plain.dims
        assert np.array_equal(getattr(src.xmr, fn.__name__)(traj, matrix, a0, W, readout_time=off).values, got.values)


# ---- validation: every error fires before the device is reached ----------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    from xmris_amd import _lib
    from xmris_amd import device as dev

    def boom(*a, **k):
        raise AssertionError("the device was reached")

    monkeypatch.setattr(_lib, "call", boom)
    for name in ("to_device", "shift_time", "zero_fill", "fft"):
        monkeypatch.setattr(dev, name, boom)


def _la(**coords):
    coords = coords or dict(time=np.arange(20) * DT)
    return labeled(orc.make((3, 4, 20), seed=1), ("coil", "sample", "time"), **coords)


def test_validation_errors_name_their_argument(no_library):
    from xmris_amd import correct_readout_time, shift_time

    off = np.arange(4) * 1e-4
    with pytest.raises(ValueError, match=r"Method 'shift_time' attempted to operate on missing dimension\(s\): \['t'\]"):
        shift_time(_la(), 1e-3, dim="t")
    with pytest.raises(ValueError, match=r"Method 'correct_readout_time' .* missing dimension\(s\): \['shot'\]"):
        correct_readout_time(_la(), off, sample_dim="shot")
    with pytest.raises(ValueError, match="sample_dim"):
        correct_readout_time(_la(), np.zeros(20), sample_dim="time")
    uneven = np.arange(20) * DT
    uneven[7] += 1e-5
    for coords in (dict(time=uneven), dict(coil=np.arange(3)), dict(time=np.arange(20)[::-1] * DT)):
        with pytest.raises(ValueError, match="dwell"):
            shift_time(_la(**coords), 1e-3)
        with pytest.raises(ValueError, match="dwell"):
            correct_readout_time(_la(**coords), off)
    for bad in (0.0, -1e-3, np.nan, "fast"):
        with pytest.raises(ValueError, match="dwell"):
            shift_time(_la(), 1e-3, dwell=bad)
    for bad in (np.nan, np.inf, np.array([0.0, 1.0, np.nan, 0.0]), 1j, "late"):
        with pytest.raises(ValueError, match="delay"):
            shift_time(_la(), bad)
    with pytest.raises(ValueError, match="delay"):
        shift_time(_la(), np.zeros(5))  # does not broadcast against (coil 3, sample 4)
    for bad in (off[:3], np.zeros((4, 1)), off * 1j, np.array([0.0, np.inf, 0.0, 0.0])):
        with pytest.raises(ValueError, match="offsets"):
            correct_readout_time(_la(), bad)
        with pytest.raises(ValueError, match="offsets"):
            _la().xmr.correct_readout_time(bad)
    for bad in (19, 0, 20.5, True):
        with pytest.raises(ValueError, match="pad_to"):
            shift_time(_la(), 1e-3, pad_to=bad)
        with pytest.raises(ValueError, match="pad_to"):
            correct_readout_time(_la(), off, pad_to=bad)
    with pytest.raises(TypeError):
        shift_time(np.zeros((4, 20), complex), 1e-3)


def test_c_abi_refusals_without_gpu():
    from xmris_amd import _lib

    lib = _lib.load()
    ok = orc.ABI_OK
    for change in orc.REFUSALS:
        a = dict(ok, **change)
        rc = lib.xm_shift_time(*[a[k] for k in orc.ABI_ORDER], None)
        assert rc == _lib.XM_ERR_INVALID_ARG, change
        assert b"shift_time" in lib.xm_last_error_string()
    # no rows: nothing is launched, whatever the pointers hold
    assert lib.xm_shift_time(*[dict(ok, n_rows=0)[k] for k in orc.ABI_ORDER], None) == 0
    # the fused set: the direct in-LDS plans, 16384 in complex64 only
    fused = [L for L in range(1, 20000) if lib.xm_shift_time_fused(L, 0)]
    assert fused == sorted([2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 384, 768, 1536, 3072, 6144,
                            640, 1280, 2560, 5120])
    assert [L for L in range(1, 20000) if lib.xm_shift_time_fused(L, 1)] == fused[:-1]
    assert lib.xm_shift_time_fused(256, 2) == 0


def test_vocabulary_and_exports():
    import xmris_amd
    from xmris_amd import ATTRS, processing

    assert (ATTRS.time_shift_pad_to, ATTRS.readout_time_corrected) == ("time_shift_pad_to", "readout_time_corrected")
    for name in ("shift_time", "correct_readout_time", "readout_offsets"):
        assert getattr(xmris_amd, name) is getattr(processing, name) and name in xmris_amd.__all__ and name in processing.__all__
    for name in ("shift_time", "correct_readout_time"):
        assert hasattr(xmris_amd.XmrisAccessor, name)
    assert "xm_shift_time" in xmris_amd._lib.SIGNATURES and "xm_shift_time_fused" in xmris_amd._lib.SIGNATURES
