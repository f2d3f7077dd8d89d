"""k_axis_sparse / xm_axis_sparse / grid_kspace / degrid_kspace / nufft_adjoint / nufft_forward on the GPU against
tests/_grid_oracle.py.  The bound is the one of tests/test_grid.py: GRID_TOL (16 x the disagreement of the oracle's two
product routes, measured on the CPU) in units of the output's U = eps64 sum_e |val_e| |x_e|, plus for complex64 the final
rounding eps32 |y|.  Shapes are the smallest that reach every path: the kernel's inner tiles are 64 elements (complex128
and the 8-byte complex64 form) and 128 (the 16-byte complex64 form), its row loop takes 4 entries per step."""
import functools

import numpy as np
import pytest

import _grid_oracle as orc
from test_grid import ACCURACY, GRID_TOL, bound, np_axis_sparse

pytestmark = pytest.mark.gpu

DTYPES = ["complex64", "complex128"]


def _up(a):
    import torch

    return torch.from_numpy(np.array(a)).to("cuda")  # (a copy: the shared cases are read-only)


def _report(what, got, want, b):
    d = np.abs(got - want)
    worst = float((d / np.where(b > 0, b, 1.0)).max())
    print(f"{what}: {worst:.3f} of its bound")
    assert np.all(d <= b), (what, worst)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@functools.lru_cache(maxsize=None)
def _parity(name):
    """The oracle's side of a parity case, computed once: both dtypes round the same complex128 x."""
    from xmris_amd import grid_table

    x, traj, matrix, a0, W, axis, A, _, _ = orc.parity_case(name)
    out = {"table": grid_table(traj, matrix, a0, W), "axis": axis, "A": A}
    for dtype in DTYPES:
        xr = x.astype(dtype)
        y = orc.apply_csr(A, xr, axis)
        yr = y.astype(dtype)  # what degridding starts from
        out[dtype] = (xr, y, orc.unit(A, xr, axis), yr, orc.apply_csr(A.T, yr, axis), orc.unit(A.T, yr, axis))
    return out


# ---- 1. parity with the oracle, both directions -----------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(orc.PARITY_CASES))
def test_parity(name, dtype):
    from xmris_amd import device as dev

    case = _parity(name)
    t, axis = case["table"], case["axis"]
    x, want, u, yr, back_want, back_u = case[dtype]
    xd = _up(x)
    got = dev.axis_sparse(xd, axis, t.grid)
    assert "k_axis_sparse" in dev.last_kernel(), dev.last_kernel()
    assert got.dtype == xd.dtype and tuple(got.shape) == want.shape and got.is_contiguous()
    assert np.array_equal(xd.cpu().numpy(), x)  # the input is untouched
    _report(f"grid {name} {dtype} {dev.last_kernel()}", got.cpu().numpy(), want, bound(u, want, dtype))
    back = dev.axis_sparse(_up(yr), axis, t.degrid)
    assert tuple(back.shape) == x.shape
    _report(f"degrid {name} {dtype} {dev.last_kernel()}", back.cpu().numpy(), back_want, bound(back_u, back_want, dtype))


def test_dot_test():
    """<A1 x, y> = <x, A1^T y> with both products from the kernel (complex128)."""
    from xmris_amd import device as dev

    case = _parity("2d_random")
    t, A = case["table"], case["A"]
    x = orc.make((37, 3), seed=21)
    y = orc.make((A.shape[0], 3), seed=22)
    ax = dev.axis_sparse(_up(x), 0, t.grid).cpu().numpy()
    aty = dev.axis_sparse(_up(y), 0, t.degrid).cpu().numpy()
    lhs, rhs = np.vdot(y, ax), np.vdot(aty, x)
    u = orc.EPS * float(np.einsum("ci,cj,ji->", np.abs(y), np.abs(A), np.abs(x)))
    print(f"dot test: |<A x, y> - <x, A^T y>| = {abs(lhs - rhs) / u:.3f} units of eps64 sum |y| |A| |x|")
    assert abs(lhs - rhs) <= GRID_TOL * u


# ---- 2. inner lengths: below, at and above every inner tile; the two complex64 forms ------------------------------------
@functools.lru_cache(maxsize=None)
def _inner_case():
    from xmris_amd import grid_table

    traj = orc.random(4, 11, 1, 5)
    t = grid_table(traj, 4, 2.0, 4, density=1.0 + np.arange(11) / 11.0)
    x = orc.make((2, 11, 131), seed=23)
    return t, x


@pytest.mark.parametrize("dtype", DTYPES)
def test_inner_lengths(dtype):
    from xmris_amd import device as dev

    t, x = _inner_case()
    x = x.astype(dtype)
    want = np_axis_sparse(x.astype(np.complex128), 1, t.grid)
    dense = np.zeros((t.grid.n_rows, 11))
    dense[np.repeat(np.arange(t.grid.n_rows), np.diff(t.grid.rowptr)), t.grid.col] = t.grid.val
    u = orc.unit(dense, x, 1)
    seen = set()
    for L in (1, 2, 3, 63, 64, 65, 66, 126, 127, 128, 129, 130, 131):
        got = dev.axis_sparse(_up(x[:, :, :L]), 1, t.grid)
        seen.add(dev.last_kernel())
        d = np.abs(got.cpu().numpy() - want[:, :, :L])
        assert np.all(d <= bound(u[:, :, :L], want[:, :, :L], dtype)), (L, dev.last_kernel())
    print(dtype, sorted(seen))
    assert seen == ({"k_axis_sparse<c128, 1>"} if dtype == "complex128" else {"k_axis_sparse<c64, 1>", "k_axis_sparse<c64, 2>"})


def test_complex64_forms_give_the_same_bits():
    """An even inner length on a 16-byte boundary takes two elements per lane, the same data 8 bytes off one per lane."""
    import torch

    from xmris_amd import device as dev

    t, x = _inner_case()
    x = x[:, :, :130].astype(np.complex64)
    wide = dev.axis_sparse(_up(x), 1, t.grid)
    assert dev.last_kernel() == "k_axis_sparse<c64, 2>"
    store = torch.empty(x.size + 1, dtype=torch.complex64, device="cuda")
    off = store[1:].view(x.shape)
    off.copy_(_up(x))
    assert off.data_ptr() % 16 == 8 and off.is_contiguous()
    narrow = dev.axis_sparse(off, 1, t.grid)
    assert dev.last_kernel() == "k_axis_sparse<c64, 1>"
    assert _same_bits(wide.cpu().numpy(), narrow.cpu().numpy())
    odd = dev.axis_sparse(_up(x[:, :, :129]), 1, t.grid)  # an odd length: one per lane as well
    assert dev.last_kernel() == "k_axis_sparse<c64, 1>" and _same_bits(odd.cpu().numpy(), wide.cpu().numpy()[:, :, :129].copy())


# ---- 3. the sample axis anywhere -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_sample_axis_position(dtype):
    from xmris_amd import device as dev

    case = _parity("2d_random")
    t, A = case["table"], case["A"]
    base = orc.make((2, 37, 3, 4), seed=24).astype(dtype)  # (repetition, sample, a, b)
    want = orc.apply_csr(A, base, 1)
    u = orc.unit(A, base, 1)
    for pos in (1, 2, 3):  # first after the repetition axis, middle, last (n_inner = 1)
        x = np.ascontiguousarray(np.moveaxis(base, 1, pos))
        got = dev.axis_sparse(_up(x), pos, t.grid).cpu().numpy()
        _report(f"sample axis {pos} {dtype}", np.moveaxis(got, pos, 1), want, bound(u, want, dtype))
    # a tensor that is not contiguous costs one copy and gives the same bits
    xd = _up(base)
    view = xd.permute(0, 2, 1, 3)
    assert not view.is_contiguous()
    a = dev.axis_sparse(view, 2, t.grid).cpu().numpy()
    b = dev.axis_sparse(view.contiguous(), 2, t.grid).cpu().numpy()
    assert _same_bits(a, b)


# ---- 4. row shapes ----------------------------------------------------------------------------------------------------------
def test_empty_rows_are_written_as_zero():
    import torch

    from xmris_amd import _lib
    from xmris_amd import device as dev

    t = dev.SparseTable([0, 0, 2, 2, 2, 3, 3], [1, 0, 2], [2.0, -1.0, 0.5], n=3)
    x = orc.make((2, 3, 5), seed=25)
    xd = _up(x)
    out = torch.full((2, 6, 5), 7.0, dtype=torch.complex128, device="cuda")
    rowptr, col, val = t._on(xd.device)
    _lib.call("xm_axis_sparse", xd.data_ptr(), out.data_ptr(), rowptr.data_ptr(), col.data_ptr(), val.data_ptr(), 2, 3, 6, 5,
              _lib.XM_C128, torch.cuda.current_stream().cuda_stream)
    got = out.cpu().numpy()
    assert np.all(got[:, [0, 2, 3, 5]] == 0)
    assert np.array_equal(got[:, 4], 0.5 * x[:, 2]) and np.allclose(got[:, 1], 2.0 * x[:, 1] - x[:, 0], rtol=1e-15)
    assert np.array_equal(dev.axis_sparse(xd, 1, t).cpu().numpy(), got)
    none = dev.SparseTable([0, 0, 0], np.zeros(0, np.int32), np.zeros(0), n=3)  # no entry at all
    assert np.all(dev.axis_sparse(xd, 1, none).cpu().numpy() == 0)


@pytest.mark.parametrize("S", [5, 1003])
def test_all_samples_on_one_point(S):
    """Every row that has entries has S of them: S = 1003 is 250 steps of the row loop and a remainder of 3."""
    from xmris_amd import device as dev, grid_table

    t = grid_table(np.full((S, 2), 0.3), 4)
    assert int(np.diff(t.grid.rowptr).max()) == S and t.grid.nnz == 16 * S
    x = orc.make((S, 3), seed=26)
    want = np_axis_sparse(x, 0, t.grid)
    dense = np.zeros((t.grid.n_rows, S))
    dense[np.repeat(np.arange(t.grid.n_rows), np.diff(t.grid.rowptr)), t.grid.col] = t.grid.val
    got = dev.axis_sparse(_up(x), 0, t.grid).cpu().numpy()
    _report(f"{S} samples on one point", got, want, bound(orc.unit(dense, x, 0)))


# ---- 5. an output depends on its own entries only ------------------------------------------------------------------------
def test_nan_containment():
    from xmris_amd import device as dev

    case = _parity("2d_random")
    t, A = case["table"], case["A"]
    x = orc.make((3, 37, 5), seed=27)
    clean = dev.axis_sparse(_up(x), 1, t.grid).cpu().numpy()
    bad = x.copy()
    bad[1, 9, 2] = np.nan
    got = dev.axis_sparse(_up(bad), 1, t.grid).cpu().numpy()
    hit = np.zeros(clean.shape, dtype=bool)
    hit[1, :, 2] = A[:, 9] != 0
    assert hit.sum() == 16 and np.all(~np.isfinite(got[hit])) and np.all(np.isfinite(got[~hit]))
    assert _same_bits(got[~hit], clean[~hit])


@pytest.mark.parametrize("dtype", DTYPES)
def test_batch_independence(dtype):
    from xmris_amd import device as dev

    case = _parity("radial")
    t = case["table"]
    x = case[dtype][0][:1]  # (1, 112, 5)
    one = dev.axis_sparse(_up(x), 1, t.grid).cpu().numpy()
    many = dev.axis_sparse(_up(x).expand(700, -1, -1).contiguous(), 1, t.grid).cpu().numpy()
    assert many.shape == (700,) + one.shape[1:] and _same_bits(many, np.broadcast_to(one, many.shape).copy())


# ---- 6. the C ABI refuses before any HIP call ---------------------------------------------------------------------------
def test_c_abi_refusals_leave_y_untouched():
    import torch

    from xmris_amd import _lib
    from xmris_amd import device as dev

    lib = _lib.load()
    t = dev.SparseTable(np.minimum(np.arange(17), 7), np.arange(7), np.ones(7), n=7)
    x = _up(orc.make((2, 7, 4), seed=28).astype(np.complex64))
    y = torch.full((2, 16, 4), 7.0, dtype=torch.complex64, device="cuda")
    rowptr, col, val = t._on(x.device)
    ok = dict(x=x.data_ptr(), y=y.data_ptr(), rowptr=rowptr.data_ptr(), col=col.data_ptr(), val=val.data_ptr(), n_outer=2, n=7,
              n_rows=16, n_inner=4, dtype=0)
    order = ("x", "y", "rowptr", "col", "val", "n_outer", "n", "n_rows", "n_inner", "dtype")
    for change in orc.REFUSALS:
        a = dict(ok)
        for k, v in change.items():
            a[k] = ok["x"] if v == "x" else (ok[k] + v if k in ("x", "y") and isinstance(v, int) else v)
        assert lib.xm_axis_sparse(*[a[k] for k in order], None) == _lib.XM_ERR_INVALID_ARG, change
    torch.cuda.synchronize()
    assert torch.all(y == 7.0).item()
    assert lib.xm_axis_sparse(*[ok[k] for k in order], None) == 0  # (the valid call itself runs)
    torch.cuda.synchronize()
    assert torch.all(y[:, 7:] == 0).item() and torch.equal(y[:, :7], x)


# ---- 7. the accessor, end to end ------------------------------------------------------------------------------------------
def _device_array(x, dims, **coords):
    from xmris_amd import LabeledArray

    return LabeledArray(_up(x), dims, coords, {"note": "kept"}, "fid")


def test_radial_point_source_peaks_where_it_is():
    traj = orc.radial(16, 26, 32)
    p0 = np.array([3, -2])
    x = np.exp(-2j * np.pi * (traj @ p0) / 16)
    data = np.stack([x, 2j * x])[:, :, None] * np.array([1.0, 0.5, -1.0])  # (coil, sample, time)
    img = _device_array(data.astype(np.complex64), ("coil", "sample", "time")).xmr.nufft_adjoint(traj, 16, density="pipe")
    assert img.is_device_resident and img.dims == ("coil", "x", "y", "time") and img.shape == (2, 16, 16, 3)
    mag = np.abs(img.values)
    for c in range(2):
        for t in range(3):
            assert np.unravel_index(np.argmax(mag[c, :, :, t]), (16, 16)) == (8 + 3, 8 - 2)
    side = np.sort(mag[0, :, :, 0].ravel())
    print(f"point source: peak / next voxel = {side[-1] / side[-2]:.2f}")
    assert side[-1] > 2 * side[-2]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("W", [4, 6])
def test_cartesian_trajectory_matches_to_image(W, dtype):
    x, traj, matrix, _, _ = orc.accuracy_case(f"cartesian_m8_w{W}")
    x = x.astype(dtype)
    k = _device_array(x.reshape(8, 8, 3), ("kx", "ky", "time"), kx=np.arange(8.0) - 4, ky=np.arange(8.0) - 4)
    want = k.xmr.to_image().values
    got = _device_array(x, ("sample", "time")).xmr.nufft_adjoint(traj, 8, width=W).values
    err = orc.accuracy(got, want)
    print(f"cartesian m 8 W {W} {dtype}: {err:.3e} against to_image (recorded {ACCURACY[f'cartesian_m8_w{W}']:.3e})")
    assert got.dtype == np.dtype(dtype) and err <= 2 * ACCURACY[f"cartesian_m8_w{W}"]


def test_forward_and_adjoint_are_a_hermitian_pair():
    """<nufft_adjoint x, v> = <x, nufft_forward v>: every stage of either chain is within its own tolerance in units of
    eps64 sum |.| |.|, so the two inner products agree within (GRID_TOL + 2 MRSI_TOL) units per chain."""
    from test_mrsi import MRSI_TOL

    traj = orc.random((6, 5), 37, 2, 1)
    x, v = orc.make((2, 37, 3), seed=29), orc.make((2, 6, 5, 3), seed=30)
    ax = _device_array(x, ("coil", "sample", "time")).xmr.nufft_adjoint(traj, (6, 5))
    fv = _device_array(v, ("coil", "x", "y", "time")).xmr.nufft_forward(traj)
    assert fv.dims == ("coil", "sample", "time") and fv.is_device_resident
    lhs, rhs = np.vdot(v, ax.values), np.vdot(fv.values, x)
    A, Gs = orc.dense_matrix(traj, (6, 5))
    M = np.einsum("pg,qh,ghj->pqj", np.abs(orc.image_table(6, 12, 4)), np.abs(orc.image_table(5, 10, 4)), A.reshape(12, 10, 37))
    u = orc.EPS * float(np.einsum("cpqt,pqj,cjt->", np.abs(v), M, np.abs(x)))
    print(f"forward / adjoint: |<A^H x, v> - <x, A v>| = {abs(lhs - rhs) / u:.3f} units")
    assert abs(lhs - rhs) <= 2 * (GRID_TOL + 2 * MRSI_TOL) * u
    ref = orc.nufft_forward(v, traj, (6, 5), axis=1)
    assert np.abs(fv.values - ref).max() <= 1e-12 * np.abs(ref).max()


def test_a_grid_above_64_takes_the_staged_transform():
    """G = 80 along the first dim: the centred transform, the crop and c run as `fft` and `phase_apply` (held to this
    project's FFT tolerance for complex128, 1e-12 of the largest magnitude per pass); the second dim is the table."""
    traj = orc.random((40, 6), 90, 2, 9)
    x = orc.make((2, 90, 3), seed=31)
    img = _device_array(x, ("coil", "sample", "time")).xmr.nufft_adjoint(traj, (40, 6))
    want = orc.nufft_adjoint(x, traj, (40, 6), axis=1)
    assert img.shape == (2, 40, 6, 3) and np.abs(img.values - want).max() <= 2e-12 * np.abs(want).max()
    back = img.xmr.nufft_forward(traj)
    ref = orc.nufft_forward(img.values, traj, (40, 6), axis=1)
    assert back.dims == ("coil", "sample", "time") and np.abs(back.values - ref).max() <= 2e-12 * np.abs(ref).max()
    # k dims that are neither adjacent nor in order are gathered with one copy: the same bits
    g = _device_array(x, ("coil", "sample", "time")).xmr.grid_kspace(traj, (40, 6))
    moved = _device_array(np.ascontiguousarray(np.transpose(g.values, (2, 0, 3, 1))), ("ky", "coil", "time", "kx"))
    a = g.xmr.degrid_kspace(traj, (40, 6)).values
    b = moved.xmr.degrid_kspace(traj, (40, 6), dim=("kx", "ky")).values  # (sample, coil, time)
    assert _same_bits(a, np.ascontiguousarray(np.transpose(b, (1, 0, 2))))
