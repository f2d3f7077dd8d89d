"""k_grappa_fill / xm_grappa_fill / .xmr.grappa_fill on the GPU against tests/_grappa_oracle.py.  The shapes are
orc.APPLY_CASES with seeded weights, whose own summation error is measured on the CPU in tests/test_grappa.py.  A time
tile of the kernel is 256 points (XM_GR_NT); complex64 with an even N_t and 16-byte aligned rows runs the paired form,
whose tile is 512.  Coil counts above 2 run in blocks of 4, 8 or 16 output coils, chunks of 8 (paired: 4) source coils."""
import functools

import numpy as np
import pytest

import _grappa_oracle as orc
from test_grappa import ABI_BAD, ABI_OK, GRAPPA_TOL, SCORE_PACKAGE, _abi_call, check  # 16 x the 0.958 of tests/tool_grappa_tolerance.py

pytestmark = pytest.mark.gpu


def _up(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _run(a, w, accel, kernel, coil_axis=0, axes=None, tensor=None, time_axis=-1):
    """a: (coil, dims..., time) unless `coil_axis` / `axes` say otherwise; `tensor`: a device tensor in place of a.
    Returns (y on the host: the input's axis order, time last; the kernel's name)."""
    from xmris_amd import device as dev

    x = _up(a) if tensor is None else tensor
    axes = list(range(1, 1 + len(accel))) if axes is None else axes
    y = dev.grappa_fill(x, w, coil_axis, axes, time_axis, list(accel), list(kernel))
    return y.cpu().numpy(), dev.last_kernel()


@functools.lru_cache(maxsize=None)
def _case(name, dtype, nt=None):
    """(a in `dtype`, W, accel, kernel, the oracle on the rounded input)."""
    a, w, accel, kernel, want = orc.apply_case(name, nt)
    a = a.astype(dtype)
    if np.dtype(dtype) != np.complex128:
        want = orc.fill(a.astype(np.complex128), w, accel, kernel)
    return a, w, accel, kernel, want


# ---- 1. parity: every shape where the index arithmetic can go wrong, coil counts 1 ... 64 -------------------------------
@pytest.mark.parametrize("dtype", ["complex128", "complex64"])
@pytest.mark.parametrize("name", list(orc.APPLY_CASES))
def test_parity_with_the_oracle(name, dtype):
    a, w, accel, kernel, want = _case(name, dtype)
    y, kern = _run(a, w, accel, kernel)
    assert y.dtype == np.dtype(dtype) and y.shape == want["y"].shape and "k_grappa_fill" in kern
    check(y, want, dtype, what=f"{name} {dtype} {kern}")


# ---- 2. time lengths: one and two points, and below, at and above the tile boundaries of both forms ---------------------
@pytest.mark.parametrize("nt, dtype", [(1, "complex128"), (2, "complex128"), (255, "complex128"), (256, "complex128"),
                                       (257, "complex128"), (1, "complex64"), (255, "complex64"), (257, "complex64"),
                                       (2, "complex64"), (256, "complex64"), (510, "complex64"), (512, "complex64"),
                                       (514, "complex64")])
def test_time_lengths_around_the_tile(nt, dtype):
    """complex128 and odd complex64 lengths: tiles of 256; even complex64 lengths: the paired form, tiles of 512."""
    a, w, accel, kernel, want = _case("5x4_r2x3_b2x3_c6", dtype, nt)
    y, kern = _run(a, w, accel, kernel)
    assert y.shape == (6, 10, 12, nt) and kern.endswith(", 2>") == (dtype == "complex64" and nt % 2 == 0)
    check(y, want, dtype, what=f"N_t={nt} {dtype} {kern}")


def test_paired_and_single_point_forms_give_the_same_bits():
    """Rows that start off a 16-byte boundary (a view one sample into a wider tensor) take the one-point form."""
    a, w, accel, kernel, _ = _case("3x2_r2x2_b2x2_c17", "complex64", 514)
    paired, k2 = _run(a, w, accel, kernel)
    wide = _up(np.concatenate([a[..., :1], a], axis=-1))
    single, k1 = _run(None, w, accel, kernel, tensor=wide[..., 1:])
    assert wide[..., 1:].stride(-1) == 1 and wide[..., 1:].data_ptr() % 16 == 8
    assert k2.endswith(", 2>") and k1.endswith(", 1>") and np.array_equal(paired, single)


# ---- 3. layouts ---------------------------------------------------------------------------------------------------------
def test_coil_axis_anywhere_repetitions_and_strided_input():
    a, w, accel, kernel, want = _case("5x4_r2x3_b2x3_c6", "complex128")  # (coil, x, y, time)
    first, _ = _run(a, w, accel, kernel)
    check(first, want, what="coil first")
    between, _ = _run(np.moveaxis(a, 0, 1), w, accel, kernel, coil_axis=1, axes=[0, 2])  # (x, coil, y, time)
    last, _ = _run(np.moveaxis(a, 0, 2), w, accel, kernel, coil_axis=2, axes=[0, 1])  # (x, y, coil, time)
    assert np.array_equal(np.moveaxis(between, 1, 0), first) and np.array_equal(np.moveaxis(last, 2, 0), first)
    rep = np.stack([a, 2 * a, a])  # (rep, coil, x, y, time)
    r3, _ = _run(rep, w, accel, kernel, coil_axis=1, axes=[2, 3])
    assert r3.shape == (3, 6, 10, 12, 4) and np.array_equal(r3[0], first) and np.array_equal(r3[2], first)
    assert np.array_equal(r3[1], 2 * first)  # (a power of two)
    # two repetition axes around the coil axis do not fold into one stride: one copy, the same numbers
    r22, _ = _run(np.stack([rep[:2], rep[1:]]).transpose(0, 2, 1, 3, 4, 5), w, accel, kernel, coil_axis=1, axes=[3, 4])
    assert np.array_equal(r22[1, :, 0], r3[1]) and np.array_equal(r22[0, :, 0], first)
    # a non-contiguous input (time strided, a transposed view of the dims, time in front): the same result
    wide = _up(np.repeat(a, 2, axis=-1))
    assert np.array_equal(_run(None, w, accel, kernel, tensor=wide[..., ::2])[0], first)
    assert np.array_equal(_run(None, w, accel, kernel, tensor=_up(np.swapaxes(a, 1, 2)).transpose(1, 2))[0], first)
    front, _ = _run(np.moveaxis(a, -1, 0), w, accel, kernel, coil_axis=1, axes=[2, 3], time_axis=0)
    assert np.array_equal(front, first)
    # a view that skips every other kept line along y: strides, no copy
    skip = _up(np.repeat(a, 2, axis=2))[:, :, ::2]
    assert not skip.is_contiguous() and np.array_equal(_run(None, w, accel, kernel, tensor=skip)[0], first)


@pytest.mark.parametrize("name, dtype", [("3_r2_b2_c4", "complex64"), ("3x2_r2x2_b2x2_c17", "complex128")])
def test_a_sample_does_not_depend_on_its_batch(name, dtype):
    a, w, accel, kernel, _ = _case(name, dtype)
    axes = list(range(2, 2 + len(accel)))
    one, _ = _run(a[None], w, accel, kernel, coil_axis=1, axes=axes)
    many, _ = _run(np.broadcast_to(a, (700, *a.shape)), w, accel, kernel, coil_axis=1, axes=axes)
    assert np.array_equal(many, np.broadcast_to(one, many.shape))


# ---- 4. acquired lines, accel 1, non-finite samples ---------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["complex128", "complex64"])
def test_acquired_lines_and_accel_one_are_bit_exact(dtype):
    a, w, accel, kernel, want = _case("5x4_r2x3_b2x3_c6", dtype)
    odd = a.copy()
    odd[0, 0, 0, 0] = complex(-0.0, np.nan)
    odd[1, 2, 1, 1] = complex(np.inf, 5e-324 if dtype == "complex128" else 1e-45)  # a denormal beside an infinity
    y, _ = _run(odd, w, accel, kernel)
    assert np.array_equal(y[:, want["acquired"]].view(np.uint8), odd.reshape(6, 20, 4).view(np.uint8))
    same, kern = _run(odd, None, (1, 1), (3, 3))
    assert np.array_equal(same.view(np.uint8), odd.view(np.uint8)) and "k_grappa_fill" in kern


@pytest.mark.parametrize("dtype", ["complex128", "complex64"])
def test_a_nan_reaches_exactly_the_outputs_that_read_it(dtype):
    a, w, accel, kernel, _ = _case("5x4_r2x3_b2x3_c6", dtype, 300)
    clean, _ = _run(a, w, accel, kernel)
    bad = a.copy()
    bad[4, 2, 1, 299] = np.nan
    got, _ = _run(bad, w, accel, kernel)
    want = orc.fill(bad.astype(np.complex128), w, accel, kernel)["y"]
    hit = ~np.isfinite(want)
    # the line itself in its coil, and in every coil the 30 missing positions among the 2 x 2 by 3 x 3 that have it as a source
    acquired = orc.apply_case("5x4_r2x3_b2x3_c6")[4]["acquired"]
    assert hit[..., 299].any(axis=0).sum() == 31 and not hit[..., :299].any() and hit[:, acquired].sum() == 1
    assert hit[:, ~acquired][..., 299].all(axis=0).sum() == 30
    assert np.array_equal(~np.isfinite(got), hit)
    assert np.array_equal(got[~hit].view(np.uint8), clean[~hit].view(np.uint8))


# ---- 5. refusals of the C ABI -----------------------------------------------------------------------------------------
def test_c_abi_refusals_leave_the_output_alone():
    import torch
    from xmris_amd import _lib

    lib = _lib.load()
    a = torch.ones((2, 4, 3, 4, 8), dtype=torch.complex64, device="cuda")
    y = torch.full((2, 4, 6, 8, 8), 7.0, dtype=torch.complex64, device="cuda")
    w = _up(orc.random_weights((2, 2), (2, 2), 4, 3))
    big = _up(np.zeros((3, 64, 64, 64), dtype=np.complex128))  # weights large enough for every refused shape
    ok = dict(ABI_OK, a=a.data_ptr(), y=y.data_ptr(), w=w.data_ptr())
    for change in ABI_BAD:
        if change.get("y") == 16:
            change = dict(y=a.data_ptr())
        rc = _abi_call(lib, dict(ok, **dict(dict(w=big.data_ptr()), **change)))
        assert rc == _lib.XM_ERR_INVALID_ARG, change
    torch.cuda.synchronize()
    assert bool((y == 7).all())
    # the same arguments unchanged are a valid call: every element is written
    assert _abi_call(lib, ok) == 0
    torch.cuda.synchronize()
    assert not bool((y == 7).any())
    want = orc.fill(np.ones((4, 3, 4, 8), dtype=complex), w.cpu().numpy(), (2, 2), (2, 2))
    check(y[1].cpu().numpy(), want, np.complex64, what="ABI call")


# ---- 6. through the accessor ------------------------------------------------------------------------------------------
def test_accessor_end_to_end_from_an_acs_block():
    from xmris_amd import ATTRS, LabeledArray

    name = "16x16_r2x2_b2x2_c12"
    cs = orc.e2e_case(name)
    kept = LabeledArray(cs["kept"].astype(np.complex64), ("coil", "kx", "ky", "time"),
                        {"kx": (orc.kept_lines(16, 2) - 16) * 0.5, "ky": (orc.kept_lines(16, 2) - 16) * 0.25}, {"MHz": 120.0})
    centre = LabeledArray(cs["acs"], ("coil", "kx", "ky", "time"))
    out, rec = kept.xmr.grappa_fill(acs=centre, accel=(2, 2), regularization=cs["lam"], return_weights=True)
    assert out.dims == kept.dims and out.shape == cs["full"].shape and out.is_device_resident and out.values.dtype == np.complex64
    assert out.attrs[ATTRS.grappa_dims] == ("kx", "ky") and out.attrs[ATTRS.grappa_accel] == (2, 2) and out.attrs["MHz"] == 120.0
    assert np.allclose(out.coords["kx"].values, (np.arange(32) - 16) * 0.5) and np.allclose(out.coords["ky"].values, (np.arange(32) - 16) * 0.25)
    # against the oracle on the very samples and weights that went in, and against the truth
    want = orc.fill(kept.values.astype(np.complex128), rec.weights, (2, 2), (2, 2))
    check(out.values, want, np.complex64, what="accessor complex64")
    sc = orc.score(out.values, cs["full"], want["acquired"])
    print(f"accessor end to end: score {sc:.4f}")
    assert sc <= SCORE_PACKAGE
    img = out.xmr.to_image().xmr.combine_coils()
    assert img.dims == ("x", "y", "time") and img.shape == (32, 32, 3)
    # the record keeps the device copy of its weights: one upload, whatever the number of fills
    wd = rec.on_device(out.data.device)
    assert np.array_equal(kept.xmr.grappa_fill(rec).values, out.values)
    assert rec.on_device(out.data.device) is wd and len(rec._resident) == 1 and np.array_equal(wd.cpu().numpy(), rec.weights)
