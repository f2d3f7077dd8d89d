"""The workgroup toolbox (xmris_amd/csrc/xm_wg.h) and lm_normal (xm_lm.h) part by part on the GPU, through the probe library
xmris_amd/libxmris_wgprobe.so (csrc/xm_wg_probe.hip), against tests/_wg_oracle.py.  The oracle's pieces, the matrix
families and the bounds are pinned on the CPU in tests/test_wg.py; the bounds come from the reference side alone
(tests/tool_wg_tolerance.py, profiles/wg_toolbox/tolerance.txt)."""
import ctypes
import functools
import os

import numpy as np
import pytest

import _wg_oracle as orc
from test_wg import CHOL_TOL, JACOBI_TOL, OFF_TOL, TRANSFORM_TOL

pytestmark = pytest.mark.gpu

EPS = orc.EPS
_p, _i, _l, _d = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_double
SIGNATURES = {  # the extern "C" entries of xm_wg_probe.hip, every one returning an int status
    "xm_wgp_sum": [_p, _p, _l, _p],
    "xm_wgp_mirror": [_p, _p, _l, _i, _p],
    "xm_wgp_gram_entries": [_p, _p, _i, _p],
    "xm_wgp_gram_items": [_p, _p, _p, _i, _p],
    "xm_wgp_jacobi": [_p, _p, _p, _p, _l, _i, _p],
    "xm_wgp_cholesky": [_p, _p, _p, _p, _p, _p, _p, _p, _p, _l, _i, _p],
    "xm_wgp_from_internal": [_p, _p, _p, _p, _p, _p, _l, _p],
    "xm_wgp_to_internal": [_p, _p, _p, _p, _p, _l, _p],
    "xm_wgp_ticket": [_p, _p, _p, _l, _i, _p],
    "xm_wgp_lm_normal": [_p, _p, _p, _l, _i, _i, _p],
    "xm_wgp_lm_fit": [_i, _p, _p, _l, _p, _p, _p, _p, _l, _i, _i, _i, _i, _i, _d, _d] + [_p] * 8 + [_i, _p],  # tests/test_gpu_lm.py
}
INVALID = -1  # XM_ERR_INVALID_ARG


@functools.lru_cache(maxsize=None)
def _probe():
    import xmris_amd

    # (XMRIS_AMD_WGPROBE: another build of the probes, as XMRIS_AMD_LIB is for the product library)
    path = os.environ.get("XMRIS_AMD_WGPROBE") or os.path.join(os.path.dirname(os.path.abspath(xmris_amd.__file__)),
                                                              "libxmris_wgprobe.so")
    if not os.path.exists(path):
        raise RuntimeError(f"{path} is missing: build it with `make -C xmris_amd/csrc`")
    lib = ctypes.CDLL(path)
    for name, args in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _i, args
    return lib


def _up(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _out(shape, dtype, fill=None):
    import torch

    dt = {np.float64: torch.float64, np.int32: torch.int32}[dtype]
    return torch.empty(shape, dtype=dt, device="cuda") if fill is None else torch.full(shape, fill, dtype=dt, device="cuda")


def _call(name, *args):
    """Launches on the null stream, waits, and returns nothing; tensors go in as pointers."""
    import torch

    rc = getattr(_probe(), name)(*[a.data_ptr() if hasattr(a, "data_ptr") else a for a in args], None)
    assert rc == 0, (name, rc)
    torch.cuda.synchronize()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _cx(a):
    """complex128 [..., C] <-> interleaved float64 [..., 2 C], whichever way."""
    a = np.ascontiguousarray(a)
    return a.view(np.float64) if a.dtype == np.complex128 else a.view(np.complex128)


# ---- the host side refuses what would overrun the LDS ---------------------------------------------------------------------
def test_refusals_launch_nothing():
    import torch

    lib = _probe()
    buf = torch.full((4096,), 7.0, dtype=torch.float64, device="cuda")
    b = buf.data_ptr()
    bad = [
        ("xm_wgp_sum", (None, b, 1)), ("xm_wgp_sum", (b, None, 1)), ("xm_wgp_sum", (b, b, -1)),
        ("xm_wgp_mirror", (b, b, 1, 0)), ("xm_wgp_mirror", (b, b, 1, 65)), ("xm_wgp_mirror", (b, None, 1, 4)),
        ("xm_wgp_mirror", (b, b, -1, 4)),
        ("xm_wgp_gram_entries", (b, b, 0)), ("xm_wgp_gram_entries", (b, b, 65)), ("xm_wgp_gram_entries", (None, b, 4)),
        ("xm_wgp_gram_items", (b, b, b, 0)), ("xm_wgp_gram_items", (b, b, b, 9)), ("xm_wgp_gram_items", (b, b, None, 2)),
        ("xm_wgp_jacobi", (b, b, b, b, 1, 0)), ("xm_wgp_jacobi", (b, b, b, b, 1, 65)), ("xm_wgp_jacobi", (b, b, b, b, -1, 4)),
        ("xm_wgp_jacobi", (b, b, b, None, 1, 4)),
        ("xm_wgp_cholesky", (b,) * 9 + (1, 0)), ("xm_wgp_cholesky", (b,) * 9 + (1, 81)), ("xm_wgp_cholesky", (b,) * 9 + (-1, 4)),
        ("xm_wgp_cholesky", (b,) * 8 + (None, 1, 4)),
        ("xm_wgp_from_internal", (b, b, b, b, b, b, -1)), ("xm_wgp_from_internal", (b, b, b, b, b, None, 4)),
        ("xm_wgp_to_internal", (b, b, b, b, b, -1)), ("xm_wgp_to_internal", (None, b, b, b, b, 4)),
        ("xm_wgp_ticket", (b, b, b, -1, 4)), ("xm_wgp_ticket", (b, b, b, 4, 0)), ("xm_wgp_ticket", (b, b, b, 4, 1025)),
        ("xm_wgp_ticket", (None, b, b, 4, 4)),
        ("xm_wgp_lm_normal", (b, b, b, 1, 1, 0)), ("xm_wgp_lm_normal", (b, b, b, 1, 1, 81)), ("xm_wgp_lm_normal", (b, b, b, 1, 0, 4)),
        ("xm_wgp_lm_normal", (b, b, b, 1, -1, 4)), ("xm_wgp_lm_normal", (b, b, b, -1, 1, 4)),
        ("xm_wgp_lm_normal", (b, b, b, (1 << 20) + 1, 1, 4)), ("xm_wgp_lm_normal", (None, b, b, 1, 1, 4)),
        ("xm_wgp_lm_normal", (b, None, b, 1, 1, 4)), ("xm_wgp_lm_normal", (b, b, None, 1, 1, 4)),
    ]
    for name, args in bad:
        assert getattr(lib, name)(*args, None) == INVALID, (name, args)
    torch.cuda.synchronize()
    assert bool((buf == 7.0).all())


# ---- wg_sum ---------------------------------------------------------------------------------------------------------------
def test_block_sum_is_the_fixed_tree_in_every_thread():
    rng = np.random.default_rng(1)
    cancel = np.tile([1e16, 1.0, -1e16, 3.0], orc.NT // 4)
    sub = rng.integers(-1000, 1000, orc.NT) * 5e-324
    one_inf, one_nan, both = rng.standard_normal(orc.NT), rng.standard_normal(orc.NT), rng.standard_normal(orc.NT)
    one_inf[77], one_nan[200] = np.inf, np.nan
    both[[3, 131]] = np.inf, -np.inf  # partners of the first level: inf - inf
    rows = np.stack([rng.standard_normal(orc.NT), rng.standard_normal(orc.NT) * 10.0 ** rng.uniform(-200, 200, orc.NT), cancel,
                     rng.permutation(cancel), sub, np.full(orc.NT, 5e-324), np.zeros(orc.NT), -np.zeros(orc.NT), one_inf,
                     one_nan, both])
    out = _out(rows.shape, np.float64)
    _call("xm_wgp_sum", _up(rows), out, len(rows))
    got, want = out.cpu().numpy(), orc.tree_sum(rows)
    assert np.array_equal(_bits(got), np.broadcast_to(_bits(got[:, :1]), got.shape))  # the same bits in all 256 threads
    finite = ~np.isnan(want)
    assert list(finite) == [True] * 9 + [False, False] and want[8] == np.inf and want[4] != 0 and want[5] == 256 * 5e-324
    assert np.array_equal(_bits(got[finite, 0]), _bits(want[finite]))  # bit for bit, signed zeros and subnormals included
    assert np.isnan(got[~finite]).all()  # (a NaN's payload is the hardware's own)


# ---- wg_mirror ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lo", [1, 33])
def test_mirror_at_every_size(lo):
    rng = np.random.default_rng(2)
    for c in range(lo, lo + 32):
        a = rng.standard_normal((3, c, c)) + 1j * rng.standard_normal((3, c, c))
        a[1] = np.where(rng.random((c, c)) < 0.3, a[1].real, a[1])  # some entries with imaginary part +0
        below = np.tril(np.ones((c, c), bool), -1)
        a[:, below] = np.nan + 1j * np.nan  # garbage below the diagonal ...
        a[2][below] = 1e300
        idx = np.arange(c)
        a[:, idx, idx] += 1j * rng.standard_normal((3, c))  # ... and in the diagonal's imaginary parts
        a[0, idx, idx] = a[0, idx, idx].real + 1j * np.nan
        out = _out((3, c, 2 * c), np.float64)
        _call("xm_wgp_mirror", _up(_cx(a)), out, 3, c)
        got = _cx(out.cpu().numpy())
        up = np.triu(np.ones((c, c), bool), 1)
        assert np.array_equal(_bits(got.real)[:, up], _bits(a.real)[:, up]), c  # the upper triangle: unchanged
        assert np.array_equal(_bits(got.imag)[:, up], _bits(a.imag)[:, up]), c
        assert np.array_equal(_bits(got.real)[:, idx, idx], _bits(a.real)[:, idx, idx]), c
        assert not _bits(got.imag)[:, idx, idx].any(), c  # the diagonal's imaginary parts: +0.0
        want = np.swapaxes(a, 1, 2)  # the lower triangle: the conjugate, bit for bit (-0.0 where the upper one has +0.0)
        assert np.array_equal(_bits(got.real)[:, below], _bits(want.real)[:, below]), c
        assert np.array_equal(_bits(got.imag)[:, below], _bits(-want.imag)[:, below]), c


# ---- the two Gram maps ------------------------------------------------------------------------------------------------------
def test_entry_map_at_every_size():
    for c in range(1, orc.MAXC + 1):
        ci, cj = _out((orc.NT, orc.MAXE), np.int32, -1), _out((orc.NT, orc.MAXE), np.int32, -1)
        _call("xm_wgp_gram_entries", ci, cj, c)
        wi, wj = orc.gram_entries(c)
        assert np.array_equal(ci.cpu().numpy(), wi) and np.array_equal(cj.cpu().numpy(), wj), c


def test_item_map_at_every_block_count():
    for nb in range(1, orc.MAXC // 8 + 1):
        outs = [_out((orc.NT, orc.MAXB), np.int32, -1) for _ in range(3)]
        _call("xm_wgp_gram_items", *outs, nb)
        for got, want in zip(outs, orc.gram_items(nb)):
            got = got.cpu().numpy().reshape(4, 64, orc.MAXB)
            assert np.array_equal(got, np.broadcast_to(want[:, None, :], got.shape)), nb  # every lane of a wave alike


# ---- row ticket -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_items, grid", [(1000, 8), (3, 3), (0, 4)])
def test_ticket_hands_out_every_item_once(n_items, grid):
    import torch

    counter = torch.zeros(2, dtype=torch.int32, device="cuda")
    for launch in range(2):  # the second launch finds the pair as the first left it
        who, drawn = _out((max(n_items, 1),), np.int32, -1), _out((max(n_items, 1),), np.int32, 0)
        _call("xm_wgp_ticket", counter, who, drawn, n_items, grid)
        who, drawn = who.cpu().numpy()[:n_items], drawn.cpu().numpy()[:n_items]
        assert np.all(drawn == 1), (launch, np.flatnonzero(drawn != 1)[:8])
        assert np.all((who >= 0) & (who < grid)), launch
        if n_items > grid:
            assert np.bincount(who, minlength=grid).max() > 1  # a workgroup comes back for more
        assert counter.cpu().tolist() == [0, 0], launch


# ---- wg_jacobi --------------------------------------------------------------------------------------------------------------
def _jacobi(gs):
    n, c, _ = gs.shape
    g_out, v_out, ret = _out((n, c, 2 * c), np.float64), _out((n, c, 2 * c), np.float64), _out((n, orc.NT), np.int32, -99)
    _call("xm_wgp_jacobi", _up(_cx(gs)), g_out, v_out, ret, n, c)
    ret = ret.cpu().numpy()
    assert np.array_equal(ret, np.broadcast_to(ret[:, :1], ret.shape)), ret  # the same value in all 256 threads, always
    return _cx(g_out.cpu().numpy()), _cx(v_out.cpu().numpy()), ret[:, 0]


@pytest.mark.parametrize("c", [1, 2, 7, 64])
def test_jacobi_leaves_a_diagonal_matrix_alone(c):
    rng = np.random.default_rng(3)
    d = rng.standard_normal((3, c)) * 10.0 ** rng.uniform(-3, 3, (3, c))
    d[1, 0] = 0.0
    d[2] = np.abs(d[2])
    gs = np.zeros((3, c, c), np.complex128)
    gs[:, np.arange(c), np.arange(c)] = d
    g, v, ret = _jacobi(gs)
    assert list(ret) == [0, 0, 0]
    assert np.array_equal(_bits(_cx(g)), _bits(_cx(gs)))  # bit-identical
    assert np.array_equal(_bits(_cx(v)), _bits(_cx(np.broadcast_to(np.eye(c, dtype=np.complex128), v.shape))))


def test_jacobi_reports_a_norm_that_overflows():
    gs = orc.jacobi_cases(8)
    big = np.stack([gs[0] * 1e160, gs[0], gs[2] * 1e200, orc.hermitian(gs[0] * np.where(np.eye(8), 1.0, 1e-300))])
    big[3, 0, 0] = 1e160  # one entry is enough
    assert np.isfinite(big.view(np.float64)).all()
    _, _, ret = _jacobi(big)
    assert ret[0] == -1 and ret[2] == -1 and ret[3] == -1 and 1 <= ret[1] <= orc.SWEEPS


@pytest.mark.parametrize("lo", [1, 17, 33, 49])
def test_jacobi_at_every_size(lo):
    worst = dict(residual=0.0, orthonormality=0.0, off=0.0, sweeps=0)
    for c in range(lo, lo + 16):
        gs = orc.jacobi_cases(c)
        g, v, ret = _jacobi(gs)
        # (a 1 x 1 matrix has no off-diagonal entry: no sweep, as the fixed points above)
        assert np.all(ret == 0) if c == 1 else np.all((ret >= 1) & (ret <= orc.SWEEPS)), (c, ret)
        for k, name in enumerate(orc.FAMILIES):
            lam = np.diagonal(g[k]).real
            res, orth = orc.eig_quality(gs[k], lam, v[k])
            off = orc.off_units(gs[k], g[k])
            worst = dict(residual=max(worst["residual"], res), orthonormality=max(worst["orthonormality"], orth),
                         off=max(worst["off"], off), sweeps=max(worst["sweeps"], int(ret[k])))
            assert res <= JACOBI_TOL["residual"], (c, name, "residual", res)
            assert orth <= JACOBI_TOL["orthonormality"], (c, name, "orthonormality", orth)
            assert off <= OFF_TOL, (c, name, "off", off)
    print(f"jacobi C={lo}..{lo + 15}: residual {worst['residual']:.2f} units of eps ||G||_F, "
          f"{worst['residual'] / JACOBI_TOL['residual']:.3f} of its bound; orthonormality {worst['orthonormality']:.2f} eps, "
          f"{worst['orthonormality'] / JACOBI_TOL['orthonormality']:.3f} of its bound; off {worst['off']:.3f} units, "
          f"{worst['off'] / OFF_TOL:.3f} of its bound; most sweeps {worst['sweeps']}")


# ---- wg_cholesky, wg_solve ------------------------------------------------------------------------------------------------
def _cholesky(h, hd, dsc, g, lam):
    n, p, _ = h.shape
    h_out, ld, dl = _out((n, p, p), np.float64), _out((n, p), np.float64), _out((n, p), np.float64)
    ok = _out((n, 2, orc.NT), np.int32, -99)
    _call("xm_wgp_cholesky", _up(h), _up(hd), _up(dsc), _up(g), _up(lam), h_out, ld, dl, ok, n, p)
    ok = ok.cpu().numpy()
    assert np.array_equal(ok, np.broadcast_to(ok[:, :, :1], ok.shape))  # every thread alike
    return h_out.cpu().numpy(), ld.cpu().numpy(), dl.cpu().numpy(), ok[:, 0, 0], ok[:, 1, 0]


@pytest.mark.parametrize("p", [1, 6, 80])
def test_cholesky_flags(p):
    rng = np.random.default_rng(4)
    spd, g = orc.cholesky_case(p, 0)
    last = p - 1
    names = ["indefinite", "zero matrix, lam 0", "nan on the diagonal", "inf on the diagonal", "zero column, lam > 0", "fine"]
    h = np.stack([spd] * 6)
    hd = np.stack([np.diagonal(spd).copy()] * 6)
    lam = np.array([0.0, 0.0, 1e-3, 1e-3, 1e-3, 0.0])
    hd[0, last] = -hd[0, last]  # (a negative pivot in the last column: every earlier column is factored first)
    h[1], hd[1] = 0.0, 0.0
    hd[2, last // 2], hd[3, last] = np.nan, np.inf
    h[4, last // 2, :], h[4, :, last // 2], hd[4, last // 2] = 0.0, 0.0, 0.0
    dsc = hd.copy()
    dsc[2:4] = np.diagonal(spd)
    gs = np.stack([g] * 6)
    h_out, ld, dl, c_ok, s_ok = _cholesky(h, hd, dsc, gs, lam)
    print(dict(zip(names, zip(c_ok, s_ok))))
    assert list(c_ok) == [0, 0, 0, 0, 1, 1] and list(s_ok) == [-1, -1, -1, -1, 1, 1]
    assert _bits(ld[4, last // 2]) == _bits(np.sqrt(np.float64(1e-3)))  # dsc = 0 scales by 1 (MINPACK): the pivot is lam
    assert np.all(dl[:4] == -7.0)  # wg_solve was not called
    assert np.array_equal(h_out[:, np.triu(np.ones((p, p), bool))], h[:, np.triu(np.ones((p, p), bool))])


@pytest.mark.parametrize("lo", [1, 21, 41, 61])
def test_cholesky_and_solve_at_every_size(lo):
    worst = dict(factor=0.0, solution=0.0, cond=0.0)
    for p in range(lo, lo + 20):
        up, hd, dsc, g, lam = orc.cholesky_cases(p)
        h_out, ld, dl, c_ok, s_ok = _cholesky(up, hd, dsc, g, lam)
        assert np.all(c_ok == 1) and np.all(s_ok == 1), (p, c_ok, s_ok)
        above = np.triu(np.ones((p, p), bool), 1)
        assert np.array_equal(_bits(h_out)[:, above], _bits(up)[:, above]), p  # the upper triangle is left alone
        assert np.isnan(h_out[:, np.arange(p), np.arange(p)]).all(), p  # ... and the diagonal, which hd stands for
        for k in range(len(lam)):
            low = np.tril(h_out[k], -1) + np.diag(ld[k])
            fac, sol, cond = orc.cholesky_quality(orc.damped(up[k], hd[k], dsc[k], lam[k]), g[k], low, dl[k])
            worst = dict(factor=max(worst["factor"], fac), solution=max(worst["solution"], sol), cond=max(worst["cond"], cond))
            assert fac <= CHOL_TOL["factor"], (p, lam[k], "factor", fac)
            assert sol <= CHOL_TOL["solution"], (p, lam[k], "solution", sol)
    print(f"cholesky P={lo}..{lo + 19}: L L^T {worst['factor']:.2f} units of eps ||H + lam D||_F, "
          f"{worst['factor'] / CHOL_TOL['factor']:.3f} of its bound; dl {worst['solution']:.2e} units of eps cond max |x|, "
          f"{worst['solution'] / CHOL_TOL['solution']:.3f} of its bound; largest cond {worst['cond']:.1e}")


# ---- lm_normal (xm_lm.h) ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", orc.LM_NORMAL_P)
def test_lm_normal_is_the_row_after_row_sum_bit_for_bit(p):
    """The probes are built without contraction: every product is rounded, then added, as the oracle does."""
    q = orc.lm_q_pts(p)
    upper, diag = np.triu(np.ones((p, p), bool), 1), np.eye(p, dtype=bool)
    for n_points in (1, q, q + 1):  # one ragged round; one full round; a full round, then a ragged one
        cases = orc.lm_normal_cases(p, n_points)
        n = len(cases)
        h_out, vec_out = _out((n, p, p), np.float64), _out((n, 7, p), np.float64)
        _call("xm_wgp_lm_normal", _up(cases), h_out, vec_out, n, n_points, p)
        h, vec = h_out.cpu().numpy(), vec_out.cpu().numpy()
        for k in range(n):
            want = orc.lm_normal(cases[k].reshape(2 * n_points, p + 1))
            assert np.array_equal(_bits(h[k][upper]), _bits(want[:p, :p][upper])), (p, n_points, k, "H")
            assert np.array_equal(_bits(vec[k, 0]), _bits(want[:p, :p][diag])), (p, n_points, k, "hd")
            assert np.array_equal(_bits(vec[k, 2]), _bits(want[:p, p])), (p, n_points, k, "g")
        # nothing else is written: H on and below the diagonal, and dsc, u, ut, dl, ld
        assert np.all(h[:, ~upper] == -7.0) and np.all(vec[:, [1, 3, 4, 5, 6]] == -7.0), (p, n_points)


# ---- wg_from_internal, wg_to_internal -------------------------------------------------------------------------------------
def _from_internal(bt, u, lo, hi):
    n = len(bt)
    p, s = _out((n,), np.float64, -7.0), _out((n,), np.float64, -7.0)
    _call("xm_wgp_from_internal", _up(np.asarray(bt, np.int32)), _up(np.asarray(u, np.float64)), _up(np.asarray(lo, np.float64)),
          _up(np.asarray(hi, np.float64)), p, s, n)
    return p.cpu().numpy(), s.cpu().numpy()


def _to_internal(bt, v, lo, hi):
    n = len(bt)
    u = _out((n,), np.float64, -7.0)
    _call("xm_wgp_to_internal", _up(np.asarray(bt, np.int32)), _up(np.asarray(v, np.float64)), _up(np.asarray(lo, np.float64)),
          _up(np.asarray(hi, np.float64)), u, n)
    return u.cpu().numpy()


# bounds at which lo + (hi - lo) does not round to hi among them
BOUNDS = [(-1e6, 1e-6), (0.1, 0.7), (-3.0, 5.0), (1e-6, 1e6), (-1e6, -1e-6), (-0.3, 1e3), (2.0, 2.0 + 1e-6)]


def test_transforms_exact_cases():
    # FREE and FIXED: p has the bits of u, the slope is 1
    u = np.array([0.0, -0.0, 1.5, -1e8, 5e-324, 1e300])
    for bt in (orc.FREE, orc.FIXED):
        p, s = _from_internal([bt] * len(u), u, [-np.inf] * len(u), [np.inf] * len(u))
        assert np.array_equal(_bits(p), _bits(u)) and np.all(s == 1.0)
    # TWO on a bound: the slope exactly 0, the value the bound itself
    half_pi = np.pi / 2
    on = [half_pi * k for k in range(-9, 10, 2)]
    for step in range(1, 5):
        on += [half_pi + step * np.spacing(half_pi), half_pi - step * np.spacing(half_pi),
               -half_pi - step * np.spacing(half_pi), -half_pi + step * np.spacing(half_pi)]
    on = np.array(on)
    sine = np.sin(on.astype(orc.LD))
    assert np.all(1 - np.abs(sine) < 1e-28)  # far closer to +-1 than half an ulp, 1.1e-16: any sincos rounds them to +-1
    for lo, hi in BOUNDS:
        p, s = _from_internal([orc.TWO] * len(on), on, [lo] * len(on), [hi] * len(on))
        assert np.all(s == 0.0), (lo, hi, s)
        assert np.array_equal(p, np.where(sine > 0, hi, lo)), (lo, hi, p)
    # a v outside its bounds: the bits of u(lo) or u(hi)
    for bt in (orc.LO, orc.HI, orc.TWO):
        for lo, hi in BOUNDS:
            w = hi - lo
            v = [lo, hi, lo - 1e-9 * w, lo - w, lo - 1e9, -1e300, hi + 1e-9 * w, hi + w, hi + 1e9, 1e300]
            got = _to_internal([bt] * len(v), v, [lo] * len(v), [hi] * len(v))
            assert np.isfinite(got).all()
            assert np.array_equal(_bits(got[2:6]), np.broadcast_to(_bits(got[0]), (4,))), (bt, lo, hi)
            assert np.array_equal(_bits(got[6:]), np.broadcast_to(_bits(got[1]), (4,))), (bt, lo, hi)


def test_transforms_against_lmfit_in_longdouble():
    bt, u, lo, hi, v = orc.transform_grid()
    two = bt == orc.TWO
    p, s = _from_internal(bt, u, lo, hi)
    want_p, want_s = orc.from_internal(bt, u, lo, hi)
    ep = np.abs(p - want_p) / orc.transform_scale(lo, hi, want_p)
    es = np.abs(s - want_s) / orc.transform_scale(lo, hi, want_s)
    # within four ulps of sin u = +-1 a sincos may or may not return +-1: there the forced slope 0 is as good
    edge = two & (1 - np.abs(np.sin(u.astype(orc.LD))) <= 4 * EPS)
    es = np.where(edge & (s == 0.0), 0.0, es)
    got_u = _to_internal(bt, v, lo, hi)
    want_u = orc.to_internal(bt, v, lo, hi)
    vc = np.clip(v, lo, hi)
    dist = np.where(bt == orc.LO, vc - lo, np.where(bt == orc.HI, hi - vc, np.minimum(vc - lo, hi - vc)))
    far = ~np.isfinite(lo) | (dist >= 1.0)  # next to a bound the rounding of u is legitimately amplified
    eu = np.abs(got_u - want_u) / orc.transform_scale(lo, hi, want_u)
    back, _ = _from_internal(bt, got_u, lo, hi)
    er = np.abs(back - vc.astype(orc.LD)) / orc.transform_scale(lo, hi, vc)
    figures = dict(p=ep, s=es, u=np.where(far, eu, 0.0), round_trip=er)
    print("transforms: " + "; ".join(f"{k} {float(e.max()):.2f} units, {float(e.max()) / TRANSFORM_TOL:.3f} of its bound"
                                     for k, e in figures.items()) + f"; {int(far.sum())} of {len(bt)} u judged")
    assert far.sum() > 5000 and edge.sum() > 100
    for k, e in figures.items():
        i = int(np.argmax(e))
        assert e[i] <= TRANSFORM_TOL, (k, float(e[i]), int(bt[i]), u[i], lo[i], hi[i], v[i])
