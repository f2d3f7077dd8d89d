"""k_lipid_project (csrc/xm_lipids.h) on the GPU against tests/_lipids_oracle.py: parity on every parity case in both
dtypes and both forms, bitwise independence of a row from batch, tile offset, strides and in-place use, status and
isolation, a lipid-like dynamic range, the refusals of the C ABI with real buffers, and the public call on the phantom.
tests/test_lipids.py pins the oracle on the CPU."""
import numpy as np
import pytest

import _lipids_oracle as orc
from test_lipids import A_MEASURED, B_MEASURED

# tests/tool_lipids_tolerance.py -> profiles/lipids/tolerance.txt (CPU only, the kernel is not involved): the largest of
# (a) factorised vs dense solve and (b) factorised vs reversed sums over all parity cases, of the input row's largest
# magnitude.  The kernel is a third summation order: 16 x.  complex64 output adds 2^-23 of that magnitude for the one
# rounding.
TOL = 16 * max(A_MEASURED, B_MEASURED)
TOL_B = 16 * B_MEASURED  # (reported only: the share of the order-of-summation figure alone)
C64 = 2.0 ** -23
DTYPES = (np.complex64, np.complex128)
FORMS = ("mfma", "fma")


def _up(a):
    import torch

    return torch.from_numpy(np.array(a)).to("cuda")  # (a copy: the cases are read-only)


def _record(b, level=0.01, n_rows=0):
    """The oracle's basis as the product's record: kernel and oracle then use the same table."""
    from xmris_amd.processing.lipids import LipidBasis

    return LipidBasis(vectors=b["U"], sigma=b["s"], weights=b["w"], beta=b["beta"], level=level, n_rows=n_rows,
                      dropped_weight=b["dropped_weight"])


def _run(x, rec, form=None, **kw):
    """device.lipid_project on a device tensor: (out, status) as numpy, and the result."""
    from xmris_amd import device as dev

    res = dev.lipid_project(x, rec, form=form, **kw)
    name = dev.last_kernel()
    assert name.startswith(f"k_lipid_project<{form or 'mfma'}, {x.shape[-1]}, {rec.rank}>"), name
    return res.out.cpu().numpy(), res.status.cpu().numpy(), res


def _bound(dtype, x):
    """Per row, of the input row's largest magnitude."""
    return (TOL + (C64 if np.dtype(dtype) == np.complex64 else 0.0)) * np.abs(x).max(axis=-1, keepdims=True)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.complex64 else np.uint64)


# ---- 1. parity -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_parity_with_the_oracle(dtype, form):
    """Every (rows, T, rank) of the lists: rows around the 16-row tile, T around the 32-point chunk and the 16-byte
    loads (odd T: 8-byte loads), ranks around the 8-coefficient blocks and the rank classes 16 | 17 and 32 | 33.  The reference is the oracle on the kernel's own
    input (the case rounded to `dtype`) with the same table."""
    worst = worst_b = 0.0
    for n, T, r in orc.CASES + orc.CLASS_CASES:
        x, b, ref = orc.case_reference(n, T, r, np.dtype(dtype).name)
        out, status, res = _run(_up(x), _record(b, n_rows=r), form)
        assert out.dtype == dtype and out.shape == (n, T) and not res.copied and np.all(status == 0)
        err = np.abs(out - ref)
        share = float((err / _bound(dtype, x)).max())
        worst = max(worst, share)
        worst_b = max(worst_b, float((err / ((TOL_B + (C64 if dtype == np.complex64 else 0.0)) * np.abs(x).max(axis=-1, keepdims=True))).max()))
        assert share <= 1.0, (n, T, r, share)
    print(f"parity {np.dtype(dtype)} {form}: largest share of the bound {worst:.3e} (of 16 x (b) alone: {worst_b:.3f})")


# ---- 2. bitwise independence ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T", [250, 257])
def test_a_row_depends_on_nothing_but_itself(T, dtype, form):
    import torch

    n, r = 17, 9
    x, b, _ = orc.case_reference(n, T, r, np.dtype(dtype).name)
    rec = _record(b)
    alone, _, _ = _run(_up(x), rec, form)
    # inside a larger batch, at another place in the tile
    other = orc.case_reference(33, T, r, np.dtype(dtype).name)[0]
    big = np.concatenate([other[:5], x, other[5:]])
    inside, _, _ = _run(_up(big), rec, form)
    assert np.array_equal(_bits(inside[5:5 + n]), _bits(alone))
    # single rows
    for i in (0, 16):
        one, _, _ = _run(_up(x[i:i + 1]), rec, form)
        assert np.array_equal(_bits(one[0]), _bits(alone[i]))
    # a strided row level, addressed where it lies
    for pad in (6, 7):
        wide = torch.zeros((n, T + pad), dtype=_up(x).dtype, device="cuda")
        wide[:, :T] = _up(x)
        strided, _, res = _run(wide[:, :T], rec, form)
        assert not res.copied and np.array_equal(_bits(strided), _bits(alone))
    # two leading axes that do not merge: the one copy
    cube = torch.zeros((n, 2, T), dtype=_up(x).dtype, device="cuda")
    cube[:, 0] = _up(x)
    sliced, _, res = _run(cube.permute(1, 0, 2)[:, ::2], rec, form)
    assert res.copied and np.array_equal(_bits(sliced[0]), _bits(alone[::2]))
    # in place
    xd = _up(x).clone()
    same, _, res = _run(xd, rec, form, out=xd)
    assert res.out.data_ptr() == xd.data_ptr() and np.array_equal(_bits(same), _bits(alone))
    wide2 = torch.zeros((n, T + 6), dtype=xd.dtype, device="cuda")
    wide2[:, :T] = _up(x)
    view = wide2[:, :T]
    _run(view, rec, form, out=view)
    assert np.array_equal(_bits(view.cpu().numpy()), _bits(alone)) and float(wide2[:, T:].abs().max()) == 0.0


# ---- 3. status and isolation ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_status_and_isolation(dtype, form):
    n, T, r = 33, 257, 9
    x, b, _ = orc.case_reference(n, T, r, np.dtype(dtype).name)
    rec = _record(b)
    clean, status, _ = _run(_up(x), rec, form)
    assert np.all(status == 0)
    for where, value in ((0, np.nan), (T - 1, np.inf), (100, -np.inf)):
        bad = x.copy()
        bad[5, where] = value
        out, status, _ = _run(_up(bad), rec, form)
        others = np.arange(n) != 5
        assert np.all(np.isnan(out[5].real)) and np.all(np.isnan(out[5].imag))
        assert status[5] == 2 and np.all(status[others] == 0)
        assert np.array_equal(_bits(out[others]), _bits(clean[others]))
    # rows outside apply: bit-for-bit copies, status 1, also of a non-finite row; a tile with no row to project
    bad = x.copy()
    bad[20, 3] = np.nan
    apply = np.ones(n, dtype=bool)
    apply[[0, 7, 20, 32]] = False
    apply[16:32] = False
    out, status, _ = _run(_up(bad), rec, form, apply=apply)
    assert np.array_equal(status, np.where(apply, 0, 1))
    assert np.array_equal(_bits(out[~apply]), _bits(bad[~apply]))
    assert np.array_equal(_bits(out[apply]), _bits(clean[apply]))
    none, status, _ = _run(_up(x), rec, form, apply=np.zeros(n, dtype=bool))
    assert np.array_equal(_bits(none), _bits(x)) and np.all(status == 1)
    # no rows at all
    from xmris_amd import device as dev

    res = dev.lipid_project(_up(x)[:0], rec, form=form)
    assert tuple(res.out.shape) == (0, T) and tuple(res.status.shape) == (0,)


# ---- 4. a lipid-like dynamic range ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_lipid_a_thousand_times_the_rest_in_complex64(form):
    """Rows whose part inside the subspace is 10^3 times the rest: the result is the small remainder of a cancellation,
    and stays within the bound stated against the input's magnitude."""
    n, T, r = 33, 257, 9
    x, b, ref = orc.case_reference(n, T, r, "complex64", 1e3)
    assert np.abs(x).max() > 100 * np.abs(ref).max()  # the cancellation is there
    out, status, _ = _run(_up(x), _record(b), form)
    share = float((np.abs(out - ref) / _bound(np.complex64, x)).max())
    print(f"dynamic range 1e3 complex64 {form}: largest share of the bound {share:.3f}")
    assert np.all(status == 0) and share <= 1.0


# ---- 5. the C ABI with real buffers --------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals_write_nothing():
    import torch

    from xmris_amd import _lib

    lib = _lib.load()
    n, T, r = 4, 64, 8
    x, b, _ = orc.case_reference(16, T, r, "complex64")
    buf = torch.full((2 * n * T + 8,), 7.0 + 3.0j, dtype=torch.complex64, device="cuda")
    buf[:n * T] = _up(x[:n]).reshape(-1)
    status = torch.full((n,), -5, dtype=torch.int32, device="cuda")
    tab = torch.zeros(2 * T * r + r + 2, dtype=torch.float64, device="cuda")
    tab[:2 * T * r + r] = _record(b).table_on("cuda")
    before = buf.clone()
    es = 8
    ok = dict(x=buf.data_ptr(), y=buf.data_ptr() + n * T * es, n_rows=n, xs=T, ys=T, T=T, rank=r, tables=tab.data_ptr(),
              apply=None, status=status.data_ptr(), dtype=0)
    changes = [dict(T=1), dict(T=65537), dict(rank=0), dict(rank=65), dict(n_rows=-1), dict(x=None), dict(y=None),
               dict(tables=None), dict(status=None), dict(dtype=2), dict(dtype=0x800), dict(xs=T - 1), dict(ys=T - 1),
               dict(tables=tab.data_ptr() + 8), dict(x=buf.data_ptr() + 4), dict(y=buf.data_ptr() + es),
               dict(y=buf.data_ptr(), ys=2 * T), dict(y=buf.data_ptr() + (n - 1) * T * es)]
    stream = torch.cuda.current_stream().cuda_stream
    for change in changes:
        a = dict(ok, **change)
        rc = lib.xm_lipid_project(*[a[k] for k in orc.ABI_ORDER], stream)
        assert rc == _lib.XM_ERR_INVALID_ARG, change
        assert b"lipid_project" in lib.xm_last_error_string()
    torch.cuda.synchronize()
    assert torch.equal(buf, before) and bool((status == -5).all())
    assert lib.xm_lipid_project(*[dict(ok, n_rows=0)[k] for k in orc.ABI_ORDER], stream) == 0
    torch.cuda.synchronize()
    assert torch.equal(buf, before) and bool((status == -5).all())
    # the valid call writes the rows of y, the status, and nothing else
    assert lib.xm_lipid_project(*[ok[k] for k in orc.ABI_ORDER], stream) == 0
    torch.cuda.synchronize()
    assert torch.equal(buf[:n * T], before[:n * T]) and torch.equal(buf[2 * n * T:], before[2 * n * T:])
    assert bool((status == 0).all()) and not torch.equal(buf[n * T:2 * n * T], before[n * T:2 * n * T])


# ---- 6. the public call ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_public_call_and_accessor_on_the_phantom(dtype):
    import xmris_amd as xa
    from xmris_amd import ATTRS, Coordinate, LabeledArray
    from xmris_amd import device as dev

    ph = orc.phantom()
    data = ph["data"].astype(dtype)
    coords = {d: Coordinate(d, np.arange(n, dtype=np.float64)) for d, n in zip(("y", "x", "time"), data.shape)}
    fid = LabeledArray(data, ("y", "x", "time"), coords, {}, "fid")
    out, rec, status = fid.xmr.remove_lipids(ph["scalp"], dims=("y", "x"), apply_mask=ph["brain"], return_basis=True)
    assert "k_lipid_project" in dev.last_kernel()
    got = dev.to_host(out.data)
    ref, b = orc.remove(data.astype(np.complex128), ph["scalp"], 0.01, None, apply_mask=ph["brain"])
    assert got.dtype == dtype and rec.rank == b["rank"] and rec.n_rows == 44
    # the product's own basis (Gram matrix on the device) spans the oracle's subspace: (c) of the tolerance file
    assert np.abs(orc.projector(rec.vectors, rec.weights) - orc.projector(b["U"], b["w"])).max() <= 16 * 1.202e-12
    bound = (TOL + 16 * 1.202e-12 + (C64 if dtype == np.complex64 else 0.0)) * np.abs(data).max(axis=-1, keepdims=True)
    assert np.all(np.abs(got - ref) <= bound)
    assert np.array_equal(_bits(got[~ph["brain"]]), _bits(data[~ph["brain"]]))
    st = dev.to_host(status.data)
    assert np.array_equal(st, np.where(ph["brain"], 0, 1))
    e_got, e_ref = orc.phantom_error(got.astype(np.complex128), ph), orc.phantom_error(ref, ph)
    print(f"phantom {np.dtype(dtype)}: error {e_got:.6f} (oracle {e_ref:.6f})")
    assert abs(e_got - e_ref) <= 1e-6 * e_ref
    assert out.attrs[ATTRS.lipid_rank] == rec.rank and out.attrs[ATTRS.lipid_rows] == 44
    # the function, and a basis reused on a second frame: the same bits as a fresh one
    frame2 = LabeledArray((data * (0.5 + 0.25j)).astype(dtype), ("y", "x", "time"), coords, {}, "fid")
    reused = xa.remove_lipids(frame2, basis=rec)
    table = rec.table_on(reused.data.device)
    fresh = xa.remove_lipids(frame2, basis=xa.processing.lipids.basis_from_subspace(rec.sigma, rec.vectors, rec.level, rec.rank))
    assert rec.table_on(reused.data.device) is table  # uploaded once
    assert np.array_equal(_bits(dev.to_host(reused.data)), _bits(dev.to_host(fresh.data)))
    whole = xa.remove_lipids(fid, basis=rec)
    assert np.array_equal(_bits(dev.to_host(whole.data)[ph["brain"]]), _bits(got[ph["brain"]]))
