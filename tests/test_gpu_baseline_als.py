"""k_als_transpose_in / k_als_solve / k_als_transpose_out (`xm_baseline_als`, `device.baseline_als`) on the GPU against the
long-double reference of tests/_als_oracle.py.

The bound of a case is _als_oracle.BOUND of its (lam, p): 16 x the float64 rounding error of the same recurrence on the
CPU (profiles/als/tolerance.txt), per row and relative to the row's max |y|.  The cases are the table of _als_oracle:
lengths around the 32-wide transpose tile and the smallest legal ones, batches around the 32-row tile and the 64-thread
block of the solver.  Every case prints its share of the bound (profiles/als/gpu_test_figures.txt)."""
import numpy as np
import pytest

import _als_oracle as als

pytestmark = pytest.mark.gpu

DTYPES = ["complex128", "complex64", "float64", "float32"]
DEGENERATE = (1e5, 0.001, 10)  # the defaults of baseline_als


def _single(dtype):
    return dtype in ("complex64", "float32")


def _input(case, dtype):
    """The case's spectra as `dtype`; the real part is `als.case_rows(case, _single(dtype))` exactly."""
    n, nb, _, seed = case
    x = als.make(n, nb, seed)
    return (x if dtype.startswith("complex") else x.real).astype(dtype)


def _run(x, prm, axis=-1):
    import torch

    from xmris_amd import device as dev

    out = dev.baseline_als(torch.from_numpy(np.ascontiguousarray(x)).cuda(), axis, *prm)
    assert out.dtype == torch.float64 and tuple(out.shape) == x.shape
    return out.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ---- 1. parity --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", als.CASES, ids=als.case_id)
def test_parity(case, dtype):
    y, z, _ = als.case_reference(case, _single(dtype))
    x = _input(case, dtype)
    assert np.array_equal(x.real.astype(np.float64), y)
    got = _run(x, case[2])
    share = als.row_gap(got, y.astype(np.longdouble) - z, y) / als.bound(case)
    print(f"parity {als.case_id(case)} {dtype}: {share.max():.3f} of its bound {als.bound(case):.1e} (row {int(share.argmax())})")
    assert np.isfinite(got).all() and share.max() <= 1.0


# ---- 2. what is read, and along which axis -----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,huge", [("complex128", 1e300), ("complex64", 3e38)])
def test_only_the_real_part_is_read(dtype, huge):
    case = als.CASES[8]  # n 37, 65 rows: ragged tiles both ways, a second solver block
    assert case[:2] == (37, 65)
    x = _input(case, dtype)
    rng = np.random.default_rng(5)
    loud = (x.real + 1j * huge * rng.choice([-1.0, 1.0], x.shape)).astype(dtype)
    assert np.isfinite(loud.imag).all() and np.abs(loud.imag).min() >= 0.99 * huge
    alone = _run(x.real.copy(), case[2])
    assert np.array_equal(_bits(_run(loud, case[2])), _bits(alone))
    assert np.array_equal(_bits(_run(x, case[2])), _bits(alone))


def test_along_a_non_last_axis():
    case = als.CASES[7]  # n 33, 33 rows
    assert case[:2] == (33, 33)
    y, z, _ = als.case_reference(case)
    x = _input(case, "complex128")
    got = _run(np.ascontiguousarray(x.T), case[2], axis=0)
    share = als.row_gap(got.T, y.astype(np.longdouble) - z, y).max() / als.bound(case)
    print(f"axis 0 {als.case_id(case)}: {share:.3f} of its bound")
    assert share <= 1.0
    assert np.array_equal(_bits(got.T), _bits(_run(x, case[2])))
    cube = np.ascontiguousarray(x.reshape(3, 11, 33).transpose(0, 2, 1))  # [3, n, 11]: the axis in the middle
    assert np.array_equal(_bits(_run(cube, case[2], axis=1).transpose(0, 2, 1).reshape(33, 33)), _bits(got.T))


# ---- 3. one thread owns one spectrum -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["complex128", "float32"])
def test_batch_invariance(dtype):
    """7 spectra tiled to 5003 rows (157 row tiles, 79 solver blocks, both ragged): every copy has the bits of the 7-row run."""
    prm = als.PARAMS[0]
    x7 = (als.make(37, 7, seed=11) if dtype == "complex128" else als.make(37, 7, seed=11).real).astype(dtype)
    few = _run(x7, prm)
    many = _run(np.tile(x7, (715, 1))[:5003], prm)
    assert np.isfinite(few).all()
    assert np.array_equal(_bits(many), _bits(np.tile(few, (715, 1))[:5003]))


def test_bad_rows_stay_alone():
    """An all-NaN, an all-Inf and an all-zero row among good ones: the good rows keep the bits of a run without them."""
    case = als.CASES[7]
    good = _input(case, "float64")[:6]
    n = good.shape[1]
    mixed = np.stack([good[0], np.full(n, np.nan), good[1], good[2], np.full(n, np.inf), good[3], np.zeros(n), good[4], good[5]])
    got = _run(mixed, case[2])
    clean = _run(good, case[2])
    assert np.isfinite(clean).all()
    assert np.array_equal(_bits(got[[0, 2, 3, 5, 7, 8]]), _bits(clean))
    assert not got[6].any() and not np.signbit(got[6]).any()  # the masked voxel stays exactly 0


# ---- 4. degenerate spectra ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4, 5, 64, 1000])
def test_degenerate_rows(n):
    """All-zero rows give exactly 0 (n = 4 too: the rule of DESIGN.md, where the oracle's spsolve gives NaN).  Constant and
    exactly linear rows lie in the null space of D: their weights are decided by rounding, no reference value exists, and
    the output is only required to be finite and within 1e-6 of max |y| of zero (tests/test_baseline_als.py's bound;
    a float64 emulation and scipy both reach 5e-8)."""
    j = np.arange(n, dtype=np.float64)
    rows = np.stack([np.zeros(n), np.full(n, 3.75), np.full(n, -2.0 ** -10), -0.25 + j / 64, 5.0 - j / 8])  # exact in float32
    for dtype in ("float64", "complex64"):
        x = rows.astype(dtype)
        for prm in (DEGENERATE, als.PARAMS[4]):
            got = _run(x, prm)
            assert np.array_equal(_bits(got[0]), np.zeros(n, np.uint64)), (dtype, prm)
            share = np.abs(got[1:]).max(axis=1) / np.abs(x.real[1:]).max(axis=1)
            print(f"degenerate n {n} {dtype} {prm}: |y - z| / max|y| = {share.tolist()}")
            assert np.isfinite(got).all() and share.max() <= 1e-6, (dtype, prm)


# ---- 5. the C ABI ------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing():
    import torch

    from xmris_amd import _lib

    lib = _lib.load()
    nb, n = 5, 37
    x = torch.ones((nb, n), dtype=torch.float64, device="cuda")
    out = torch.full((nb, n), 7.0, dtype=torch.float64, device="cuda")
    need = int(lib.xm_baseline_als_workspace_bytes(nb, n))
    assert need == 5 * nb * n * 8
    work = torch.full((need // 8,), 7.0, dtype=torch.float64, device="cuda")
    order = ("in", "is_complex", "n_batch", "n", "lam", "p", "n_iter", "out", "work", "work_bytes", "dtype")
    ok = {"in": x.data_ptr(), "is_complex": 0, "n_batch": nb, "n": n, "lam": 1e5, "p": 0.01, "n_iter": 3,
          "out": out.data_ptr(), "work": work.data_ptr(), "work_bytes": need, "dtype": _lib.XM_C128}
    for change in ({"n": 3}, {"n_iter": 0}, {"dtype": 2}, {"dtype": -1}, {"work_bytes": need - 1}, {"in": None},
                   {"out": None}, {"work": None}, {"n_batch": -1}):
        a = dict(ok, **change)
        assert lib.xm_baseline_als(*[a[k] for k in order], None) == _lib.XM_ERR_INVALID_ARG, change
    empty = dict(ok, n_batch=0)
    assert lib.xm_baseline_als(*[empty[k] for k in order], None) == 0
    nothing = dict(ok, n_batch=0, out=None, work=None, work_bytes=0, **{"in": None})
    assert lib.xm_baseline_als(*[nothing[k] for k in order], None) == 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((work == 7.0).all())
    assert lib.xm_baseline_als(*[ok[k] for k in order], None) == 0  # and the unchanged call does run
    torch.cuda.synchronize()
    assert bool((out != 7.0).all())
