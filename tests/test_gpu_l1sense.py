"""k_l1_start / k_l1_prox and recon_l1_sense on the GPU against tests/_l1sense_oracle.py.  End to
end the bound is the one of tests/test_l1sense.py: L1_TOL128 / L1_TOL64 (16 x the disagreement of two routes of the oracle,
measured on the CPU) x the largest |x| of the oracle.  The prox kernel alone is bounded by its own rounding: with at most
4 butterfly levels, each two roundings in either direction, and under 16 roundings in the gradient step, the shrink and
the momentum, x and v are within 32 eps max |w| of the numpy restatement in the same butterfly order; a partial is a sum
of 2 B <= 32 squares.

Shapes are the smallest that reach every path: every block size B = 1, 2, 4, 8, 16 (one instantiation each), 1, 2 and 3
dims, a matrix size that is not a power of two (6), more than four blocks (more than one workgroup), a cycle-spin shift
that wraps; T = 1, 3 (odd) and 70 (one tile of 64 columns and a partial one)."""
import functools

import numpy as np
import pytest

import _cgsense_oracle as cgs_orc
import _grid_oracle as grid_orc
import _l1sense_oracle as orc
from test_l1sense import BENEFIT, L1_TOL64, L1_TOL128, PARITY, tau_of

pytestmark = pytest.mark.gpu

EPS = grid_orc.EPS
DTYPES = ["complex64", "complex128"]
# (matrix, levels, shift)
SHAPES = [((8,), (3,), (0,)), ((8, 6), (2, 1), (0, 0)), ((4, 4, 4), (1, 1, 1), (0, 0, 0)), ((8, 8), (2, 2), (0, 0)),
          ((8, 8), (0, 0), (0, 0)), ((16, 16), (2, 2), (3, 1))]
TAU, THETA_SCALE, BETA, TOL = 0.7, 0.21, 0.3, 1e-3


def _up(a):
    import torch

    return torch.from_numpy(np.array(a)).to("cuda")  # (a copy: the shared inputs are read-only)


def _down(t):
    return t.cpu().numpy()


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _block_of(ms, levels, shift):
    """[V] int: the Haar block (C order over the block lattice) of every voxel."""
    flat = np.zeros((), dtype=np.int64)
    for m, l, s in zip(ms, levels, shift):
        flat = np.add.outer(flat * (m >> l), ((np.arange(m) - s) % m) >> l)
    return flat.reshape(-1)


def _block_sums(terms, ms, levels, shift):
    nb = int(np.prod([m >> l for m, l in zip(ms, levels)]))
    out = np.zeros((nb, terms.shape[1]))
    np.add.at(out, _block_of(ms, levels, shift), terms)
    return out


def _total(part):
    a = np.zeros(part.shape[1])
    for b in range(part.shape[0]):
        a = a + part[b]
    return a


@functools.lru_cache(maxsize=None)
def _inputs(ms, levels, T):
    """Seeded state of one step.  Of the columns whose status is 0: column 0 runs; with T >= 3 column 2 has converged
    (d2 tiny); with T = 70 column 5 has a d2 that is not finite and column 6 an n2 that is NaN.  Columns 1, 4, 7 ... come
    in frozen."""
    V = int(np.prod(ms))
    nb = V >> sum(levels)
    rng = np.random.default_rng(V + 7 * T + sum(levels))
    mk = lambda *shape: rng.standard_normal(shape) + 1j * rng.standard_normal(shape)  # noqa: E731
    status = np.zeros(T, dtype=np.int32)
    status[1::3] = rng.integers(1, 4, len(status[1::3]))
    d2, n2 = rng.uniform(0.5, 1.5, (nb, T)), rng.uniform(0.5, 1.5, (nb, T))
    if T >= 3:
        d2[:, 2] *= 1e-8
    if T == 70:
        d2[nb // 2, 5] = np.inf
        n2[0, 6] = np.nan
    mask = (rng.uniform(size=V) > 0.2).astype(np.uint8)
    out = dict(x=mk(V, T), v=mk(V, T), q=mk(V, T), b=mk(V, T), mask=mask, bmax=rng.uniform(0.5, 3.0, T), status=status,
               d2=d2, n2=n2)
    for a in out.values():
        a.setflags(write=False)
    return out


def _launch(a, ms, levels, shift, mode, iteration=4, tol=TOL):
    import torch

    from xmris_amd import device as dev

    T = a["x"].shape[1]
    nb = a["d2"].shape[0]
    x, v = _up(a["x"]), _up(a["v"])
    d2_out = torch.full((nb, T), -1.0, dtype=torch.float64, device="cuda")
    n2_out = torch.full((nb, T), -1.0, dtype=torch.float64, device="cuda")
    status_out = torch.full((T,), -1, dtype=torch.int32, device="cuda")
    n_iter = torch.full((T,), 2, dtype=torch.int32, device="cuda")
    change = torch.full((T,), -1.0, dtype=torch.float64, device="cuda")
    first = mode == 1
    dev.l1_prox(x, v, None if first else _up(a["q"]), _up(a["b"]), _up(a["mask"]), _up(a["bmax"]),
                None if first else _up(a["d2"]), None if first else _up(a["n2"]), d2_out, n2_out, _up(a["status"]), status_out,
                n_iter, change, ms, levels, shift, TAU, THETA_SCALE, BETA, tol, iteration, mode)
    B = 1 << sum(levels)
    assert dev.last_kernel() == f"k_l1_prox<c128, {B}, {mode}>", dev.last_kernel()
    return dict(x=_down(x), v=_down(v), d2=_down(d2_out), n2=_down(n2_out), status=_down(status_out), n_iter=_down(n_iter),
                change=_down(change))


def _expected(a, ms, levels, shift, mode, tol=TOL):
    """The numpy restatement of one launch: (status, run, x', v', w)."""
    status = a["status"].copy()
    active = status == 0
    t_d2, t_n2 = _total(a["d2"]), _total(a["n2"])
    if mode == 1:
        run = active.copy()
    else:
        bad = active & ~(np.isfinite(t_d2) & np.isfinite(t_n2))
        with np.errstate(invalid="ignore"):
            conv = active & ~bad & (t_d2 <= tol * tol * t_n2)
        status[bad], status[conv] = 3, 1
        run = active & ~bad & ~conv & (mode == 0)
    g = (0 if mode == 1 else a["q"]) - a["b"]
    w = a["v"] - TAU * g
    xn = orc.prox(w, ms, levels, THETA_SCALE * a["bmax"], a["mask"] != 0, shift)
    vn = xn + BETA * (xn - a["x"])
    return status, run, xn, vn, w


@pytest.mark.parametrize("T", [1, 3, 70])
@pytest.mark.parametrize("ms, levels, shift", SHAPES)
def test_prox_kernel(ms, levels, shift, T):
    a = _inputs(ms, levels, T)
    got = _launch(a, ms, levels, shift, 0)
    status, run, xn, vn, w = _expected(a, ms, levels, shift, 0)
    assert run[0] and (T < 3 or status[2] == 1) and (T < 70 or (status[5] == 3 and status[6] == 3))
    assert np.array_equal(got["status"], status) and np.array_equal(got["n_iter"], np.where(run, 4, 2))
    bound = 32 * EPS * np.abs(w).max(axis=0)
    for name, want in (("x", xn), ("v", vn)):
        d = np.abs(got[name] - want)[:, run]
        print(f"prox {name} {ms} {levels} shift {shift} T {T}: {float((d / bound[run]).max()):.3f} of its bound")
        assert np.all(d <= bound[run])
    # a frozen column, and one that freezes here, is bit for bit what it was; a masked voxel is exactly 0
    newly_bad = (a["status"] == 0) & (status == 3)
    assert _same_bits(got["x"][:, ~run & ~newly_bad], a["x"][:, ~run & ~newly_bad]) and _same_bits(got["v"][:, ~run], a["v"][:, ~run])
    assert np.all(np.isnan(got["x"][:, newly_bad])) and np.all(got["x"][a["mask"] == 0][:, run] == 0)
    if any(levels):  # (with B = 1 every coefficient is shrunk, and a small one becomes 0)
        assert np.all(got["x"][a["mask"] != 0][:, run] != 0)
    # the partials are the fp64 sums of what was written
    dx = got["x"] - a["x"]
    for name, terms in (("d2", dx.real ** 2 + dx.imag ** 2), ("n2", got["x"].real ** 2 + got["x"].imag ** 2)):
        want = _block_sums(terms, ms, levels, shift)[:, run]
        d = np.abs(got[name][:, run] - want)
        print(f"prox partials {name} {ms} T {T}: {float((d / np.maximum(34 * EPS * want, 1e-300)).max()):.3f} of its bound")
        assert np.all(d <= 34 * EPS * want) and np.all(got[name][:, ~run] == -1.0)
    # change: written for a column that freezes here only
    t_d2, t_n2 = _total(a["d2"]), _total(a["n2"])
    told = (a["status"] == 0) & (status != 0)
    assert np.all(got["change"][~told] == -1.0) and np.all(np.isnan(got["change"][newly_bad]))
    conv = told & ~newly_bad
    assert np.allclose(got["change"][conv], np.sqrt(t_d2[conv] / t_n2[conv]), rtol=4 * EPS, atol=0)


@pytest.mark.parametrize("ms, levels, shift", [SHAPES[1], SHAPES[5]])
def test_first_step_and_final_test(ms, levels, shift):
    """Mode 1 takes q as 0 and tests nothing; mode 2 writes status, iterations and change and nothing else (but the NaN
    column of a status 3)."""
    T = 70
    a = _inputs(ms, levels, T)
    got = _launch(a, ms, levels, shift, 1)
    status, run, xn, vn, w = _expected(a, ms, levels, shift, 1)
    assert np.array_equal(got["status"], a["status"]) and np.array_equal(run, a["status"] == 0)
    bound = 32 * EPS * np.abs(w).max(axis=0)
    assert np.all(np.abs(got["x"] - xn)[:, run] <= bound[run]) and np.all(np.abs(got["v"] - vn)[:, run] <= bound[run])
    assert _same_bits(got["x"][:, ~run], a["x"][:, ~run]) and np.all(got["change"] == -1.0)
    assert np.array_equal(got["n_iter"], np.where(run, 4, 2))

    got = _launch(a, ms, levels, shift, 2)
    status, run, _, _, _ = _expected(a, ms, levels, shift, 2)
    assert not run.any() and np.array_equal(got["status"], status)
    newly_bad = (a["status"] == 0) & (status == 3)
    assert newly_bad.sum() == 2 and np.all(np.isnan(got["x"][:, newly_bad]))
    assert _same_bits(got["x"][:, ~newly_bad], a["x"][:, ~newly_bad]) and _same_bits(got["v"], a["v"])
    assert np.all(got["d2"] == -1.0) and np.all(got["n2"] == -1.0) and np.all(got["n_iter"] == 2)
    active = a["status"] == 0
    t_d2, t_n2 = _total(a["d2"]), _total(a["n2"])
    ok = active & ~newly_bad
    assert np.all(got["change"][~active] == -1.0) and np.all(np.isnan(got["change"][newly_bad]))
    assert np.allclose(got["change"][ok], np.sqrt(t_d2[ok] / t_n2[ok]), rtol=4 * EPS, atol=0)


def test_a_column_alone_equals_itself_in_a_batch():
    ms, levels, shift = SHAPES[5]
    a = _inputs(ms, levels, 70)
    whole = _launch(a, ms, levels, shift, 0)
    for t in (0, 66):
        one = {k: np.ascontiguousarray(v[..., t:t + 1]) if k != "mask" else v for k, v in a.items()}
        assert a["status"][t] == 0
        got = _launch(one, ms, levels, shift, 0)
        for name in ("x", "v", "d2", "n2"):
            assert _same_bits(got[name][..., 0], np.ascontiguousarray(whole[name][..., t])), (name, t)


@pytest.mark.parametrize("V, T", [(8, 3), (37, 70)])
def test_start_kernel(V, T):
    """bmax is the largest |b| of the column exactly as numpy forms it from the same squares; a NaN or an infinity
    anywhere in the column gives status 3, a NaN bmax and change and a NaN column of x."""
    import torch

    from xmris_amd import device as dev

    rng = np.random.default_rng(V)
    b = rng.standard_normal((V, T)) + 1j * rng.standard_normal((V, T))
    b[:, 1] = 0
    b[V - 1, 2] = np.nan
    if T > 3:
        b[17, 65] = np.inf
    x = torch.zeros((V, T), dtype=torch.complex128, device="cuda")
    bmax, change = (torch.full((T,), -1.0, dtype=torch.float64, device="cuda") for _ in range(2))
    status = torch.full((T,), -1, dtype=torch.int32, device="cuda")
    dev.l1_start(_up(b), x, bmax, status, change)
    assert dev.last_kernel() == "k_l1_start<c128, 1>", dev.last_kernel()
    bad = ~np.isfinite(b).all(axis=0)
    assert bad.sum() == (2 if T > 3 else 1)
    assert np.array_equal(_down(status), np.where(bad, 3, 0))
    want = np.abs(b).max(axis=0)
    got = _down(bmax)
    assert np.all(np.isnan(got[bad])) and np.allclose(got[~bad], want[~bad], rtol=4 * EPS, atol=0) and got[1] == 0
    gx = _down(x)
    assert np.all(np.isnan(gx[:, bad])) and np.all(gx[:, ~bad] == 0)
    assert np.all(np.isnan(_down(change)[bad])) and np.all(_down(change)[~bad] == -1.0)


# ---- recon_l1_sense against the oracle ------------------------------------------------------------------------------------
# columns per case: 5 (odd: the 8-byte complex64 form of the chain), 4, 70 (a tile edge plus remainder), 3
COLUMNS = {"radial2d": 5, "masked2d": 4, "random3d": 70, "odd2d": 70, "line1d": 3}


def _labeled(x, dims):
    from xmris_amd import LabeledArray

    return LabeledArray(x, dims, {}, {}, None)


def _recon(c, y, iterations=10, tol=0.0, **kw):
    from xmris_amd import recon_l1_sense

    kw = dict(dict(tikhonov=c.reg, density=c.density, width=c.W, levels=c.levels, return_info=True), **kw)
    return recon_l1_sense(_labeled(y, ("coil", "sample", "time")), c.traj, c.s, iterations=iterations, tol=tol, **kw)


@functools.lru_cache(maxsize=None)
def _reference(name, dtype, iterations=10):
    """(case, data in `dtype`, the oracle's result from that data); computed once and shared."""
    c = orc.case(name, COLUMNS[name])
    y = c.y.astype(dtype)
    r = orc.fista(c.dense(), c.rhs(y.astype(np.complex128)), c.ms, c.levels, 0.02, tau_of(c), iterations, mask=c.mask)
    r.x.setflags(write=False)
    return c, y, r


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", PARITY)
def test_recon_matches_the_oracle(name, dtype):
    """10 steps at tol 0 with the step from the package's own power estimate, within L1_TOL max |x|."""
    from xmris_amd import device as dev

    c, y, ref = _reference(name, dtype)
    yd = _up(y)
    ds = _recon(c, yd)
    assert "k_l1_prox" in dev.last_kernel()
    got = _down(ds["image"].data).reshape(c.V, c.T)
    tol = L1_TOL64 if dtype == "complex64" else L1_TOL128
    err = orc.rel(got, ref.x)
    step = ds["image"].attrs["l1sense_step"]
    print(f"recon {name} {dtype} T {c.T}: {err / tol:.3f} of its bound; step differs from the oracle's by {abs(step / tau_of(c) - 1):.1e}")
    assert got.dtype == np.complex128 and ds["image"].dims == ("x", "y", "z")[:len(c.ms)] + ("time",)
    assert np.all(_down(ds["iterations"].data) == 10) and np.all(_down(ds["status"].data) == 0)
    assert np.allclose(_down(ds["change"].data), [col[-1] for col in ref.ratios], rtol=1e-4)
    assert err <= tol
    assert _same_bits(_down(yd), y)  # the data is untouched
    if name == "masked2d":
        assert (~c.mask).sum() > 8 and np.all(got[~c.mask] == 0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_columns_chunks_zero_and_nan(dtype):
    """radial2d, 5 columns: `chunk=2` and a column alone give the bits of the one pass; a zero column converges after one
    step at x = 0; a NaN sample gives status 3 and a NaN column; neither touches its neighbours."""
    c, y, _ = _reference("radial2d", dtype)
    step = tau_of(c)
    whole = _recon(c, _up(y), step=step)
    img = _down(whole["image"].data)
    parts = _recon(c, _up(y), step=step, chunk=2)
    assert _same_bits(_down(parts["image"].data), img) and _same_bits(_down(parts["change"].data), _down(whole["change"].data))
    one = _recon(c, _up(np.ascontiguousarray(y[:, :, 3:4])), step=step)
    assert _same_bits(_down(one["image"].data)[..., 0], img[..., 3])
    z = y.copy()
    z[:, :, 1] = 0
    ds = _recon(c, _up(z), step=step)
    got = _down(ds["image"].data)
    keep = [0, 2, 3, 4]
    assert np.all(got[..., 1] == 0) and _down(ds["status"].data)[1] == 1 and _down(ds["iterations"].data)[1] == 1
    assert _down(ds["change"].data)[1] == 0 and _same_bits(got[..., keep], img[..., keep])
    z[1, 3, 1] = np.nan
    ds = _recon(c, _up(z), step=step)
    got = _down(ds["image"].data)
    assert _down(ds["status"].data)[1] == 3 and np.all(np.isnan(got[..., 1])) and _down(ds["iterations"].data)[1] == 0
    assert np.all(_down(ds["status"].data)[keep] == 0) and _same_bits(got[..., keep], img[..., keep])


def test_stopping_rule_and_cycle_spinning():
    """A tol that no step's change comes within 1e-6 of (the oracle checks): every column stops at the oracle's step.
    Cycle spinning: the lattice moves by k mod 4 voxels per dim, within L1_TOL128 of the oracle doing the same."""
    c, y, _ = _reference("radial2d", "complex128")
    ref = orc.fista(c.dense(), c.rhs(), c.ms, c.levels, 0.02, tau_of(c), 40, mask=c.mask)
    tol = 3e-3
    assert orc.clear_of(ref.ratios, tol)
    ds = _recon(c, _up(y), iterations=40, tol=tol, step=tau_of(c))
    want = [next(k + 1 for k, r in enumerate(col) if r <= tol) for col in ref.ratios]
    assert _down(ds["iterations"].data).tolist() == want and np.all(_down(ds["status"].data) == 1) and max(want) < 40
    stopped = orc.fista(c.dense(), c.rhs(), c.ms, c.levels, 0.02, tau_of(c), 40, tol, mask=c.mask)
    assert orc.rel(_down(ds["image"].data).reshape(c.V, c.T), stopped.x) <= L1_TOL128
    spun = _recon(c, _up(y), cycle_spin=True, step=tau_of(c))
    want = orc.fista(c.dense(), c.rhs(), c.ms, c.levels, 0.02, tau_of(c), 10, mask=c.mask, cycle_spin=True).x
    err = orc.rel(_down(spun["image"].data).reshape(c.V, c.T), want)
    print(f"cycle spinning radial2d: {err / L1_TOL128:.3f} of its bound")
    assert err <= L1_TOL128


def test_benefit_of_the_penalty():
    """The undersampled 16 x 16 radial case: the errors recorded from the oracle (tests/test_l1sense.py), on the GPU."""
    from xmris_amd import recon_cg_sense

    c = orc.case("benefit")
    yd = _up(c.y)
    la = _labeled(yd, ("coil", "sample", "time"))
    x_cg = _down(recon_cg_sense(la, c.traj, c.s, iterations=30, tol=0.0, regularization=0.05, density="pipe").data)
    e_cg = orc.error(x_cg.reshape(c.V, c.T), c.obj)
    e_l1 = orc.error(_down(_recon(c, yd, iterations=100)["image"].data).reshape(c.V, c.T), c.obj)
    e_off = orc.error(_down(_recon(c, yd, iterations=100, sparsity=0.0)["image"].data).reshape(c.V, c.T), c.obj)
    print(f"benefit: cg {e_cg:.3f}  l1 {e_l1:.3f}  sparsity 0 {e_off:.3f}")
    assert e_l1 < 0.5 * e_cg and e_off >= e_cg
    assert e_cg == pytest.approx(BENEFIT["cg"], rel=0.05) and e_l1 == pytest.approx(BENEFIT["l1"], rel=0.05)
    assert e_off == pytest.approx(BENEFIT["l1_off"], rel=0.05)
