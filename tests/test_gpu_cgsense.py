"""k_cgs_expand / k_cgs_reduce / k_cgs_step and recon_cg_sense on the GPU against tests/_cgsense_oracle.py (DESIGN.md
section 21).  End to end the bound is the one of tests/test_cgsense.py: CGS_TOL128 / CGS_TOL64 (16 x the disagreement of two
routes of the oracle, measured on the CPU) x the largest |x| of the oracle.  The kernels alone are bounded by the rounding
of their own sums: an n-term fp64 sum of products differs between two orders or two contractions by at most
n eps64 sum |terms|, and a value stored as complex64 adds eps32 of its magnitude.

Shapes are the smallest that reach every path.  The voxel block is 16: V = 37 is two blocks and a remainder, V = 8 less
than one.  A column tile is 64 columns (complex128 and the 8-byte complex64 form) or 128 (the 16-byte complex64 form):
T = 5 is odd and takes the 8-byte form, T = 130 is one tile of either form plus a remainder, and an even T on a base that
is not 16-byte aligned takes the 8-byte form again."""
import functools

import numpy as np
import pytest

import _cgsense_oracle as orc
import _grid_oracle as grid_orc
from test_cgsense import CGS_TOL64, CGS_TOL128, DISTANCE30, FULL_SAMPLING, full_sampling_case

pytestmark = pytest.mark.gpu

DTYPES = ["complex64", "complex128"]
EPS, EPS32 = grid_orc.EPS, grid_orc.EPS32
C, V = 3, 37
NB = 3


def _up(a):
    import torch

    return torch.from_numpy(np.array(a)).to("cuda")  # (a copy: the shared cases are read-only)


def _down(t):
    return t.cpu().numpy()


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _report(what, got, want, b):
    d = np.abs(got - want)
    worst = float((d / np.where(b > 0, b, 1.0)).max())
    print(f"{what}: {worst:.3f} of its bound")
    assert np.all(d <= b), (what, worst)


def _total(part):
    """A column's partials added in ascending block order, as the kernels add them."""
    a = np.zeros(part.shape[1])
    for b in range(part.shape[0]):
        a = a + part[b]
    return a


def _block_sums(terms):
    """[V, T] -> [NB, T], ascending v within a block."""
    out = np.zeros((NB, terms.shape[1]))
    for v in range(terms.shape[0]):
        out[v // 16] += terms[v]
    return out


@functools.lru_cache(maxsize=None)
def _kernel_inputs(T):
    rng = np.random.default_rng(T)
    mk = lambda *shape: rng.standard_normal(shape) + 1j * rng.standard_normal(shape)  # noqa: E731
    status = np.zeros(T, dtype=np.int32)
    status[1::3] = [1, 2, 3][:len(status[1::3])] if T < 10 else rng.integers(1, 4, len(status[1::3]))
    return dict(r=mk(V, T), p=mk(V, T), s=mk(C, V), rho_new=rng.uniform(0.5, 1.5, (NB, T)), rho_old=rng.uniform(0.5, 1.5, (NB, T)),
                status=status, u=mk(C, V, T), q=mk(V, T), x=mk(V, T))


def _u_buffer(dtype, T, misaligned):
    """A [C, V, T] tensor of `dtype`; `misaligned`: its base 8 bytes past a 16-byte boundary (complex64 only)."""
    import torch

    flat = torch.zeros(C * V * T + 1, dtype=getattr(torch, dtype), device="cuda")
    return flat[1:].view(C, V, T) if misaligned else flat[:-1].view(C, V, T)


FORMS = [("complex64", 5, False, "k_cgs_{}<c64, 1>"), ("complex64", 130, False, "k_cgs_{}<c64, 2>"),
         ("complex64", 130, True, "k_cgs_{}<c64, 1>"), ("complex128", 5, False, "k_cgs_{}<c128, 1>"),
         ("complex128", 130, False, "k_cgs_{}<c128, 1>")]


# ---- 1. the three kernels alone -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", [True, False])
@pytest.mark.parametrize("dtype, T, misaligned, kernel", FORMS)
def test_expand_kernel(dtype, T, misaligned, kernel, first):
    """V = 37: two voxel blocks and a remainder.  T = 5: the odd, 8-byte form; T = 130: a tile edge plus remainder in the
    16-byte form, and on a misaligned base the 8-byte form, whose bits must be the same."""
    import torch

    from xmris_amd import device as dev

    a = _kernel_inputs(T)
    r, p, s = _up(a["r"]), _up(a["p"]), _up(a["s"])
    u = dev.cgs_expand(r, p, s, _up(a["rho_new"]), _up(a["rho_old"]), _up(a["status"]), first, getattr(torch, dtype),
                       out=_u_buffer(dtype, T, misaligned))
    assert dev.last_kernel() == kernel.format("expand"), dev.last_kernel()
    live = a["status"] == 0
    beta = _total(a["rho_new"]) / _total(a["rho_old"])
    want_p = np.where(live, a["r"] if first else a["r"] + beta * a["p"], a["p"])
    got_p = _down(p)
    assert _same_bits(got_p[:, ~live], a["p"][:, ~live])  # a frozen column keeps its p
    if first:
        assert _same_bits(got_p[:, live], a["r"][:, live])
    _report(f"expand p {dtype} T {T} first {first}", got_p, want_p, 4 * EPS * (np.abs(a["r"]) + np.abs(beta * a["p"])))
    want_u = a["s"][:, :, None] * got_p[None]
    b = 4 * EPS * np.abs(want_u) + (EPS32 * np.abs(want_u) if dtype == "complex64" else 0)
    _report(f"expand u {dtype} T {T} {dev.last_kernel()}", _down(u).astype(np.complex128), want_u, b)
    assert _same_bits(_down(r), a["r"]) and _same_bits(_down(s), a["s"])  # inputs untouched
    if misaligned:  # the same bits as the 16-byte form
        p2 = _up(a["p"])
        u2 = dev.cgs_expand(r, p2, s, _up(a["rho_new"]), _up(a["rho_old"]), _up(a["status"]), first, getattr(torch, dtype))
        assert dev.last_kernel() == "k_cgs_expand<c64, 2>" and _same_bits(_down(u2), _down(u)) and _same_bits(_down(p2), got_p)


@pytest.mark.parametrize("initial", [True, False])
@pytest.mark.parametrize("dtype, T, misaligned, kernel", FORMS)
def test_reduce_kernel(dtype, T, misaligned, kernel, initial):
    """The shapes of test_expand_kernel.  q is a sum of 2 C + 1 complex products, a partial one of 16 voxels' two."""
    import torch

    from xmris_amd import device as dev

    a = _kernel_inputs(T)
    lam = 0.37
    u = _u_buffer(dtype, T, misaligned)
    u.copy_(_up(a["u"]).to(u.dtype))
    un = _down(u).astype(np.complex128)
    s, p = _up(a["s"]), _up(a["p"])
    q = torch.full((V, T), float("nan"), dtype=torch.complex128, device="cuda")
    part = torch.full((NB, T), float("nan"), dtype=torch.float64, device="cuda")
    dev.cgs_reduce(u, s, None if initial else p, q, part, lam, initial)
    assert dev.last_kernel() == kernel.format("reduce"), dev.last_kernel()
    want = (np.conj(a["s"])[:, :, None] * un).sum(axis=0) + (0 if initial else lam * a["p"])
    mag = (np.abs(a["s"])[:, :, None] * np.abs(un)).sum(axis=0) + (0 if initial else lam * np.abs(a["p"]))
    got = _down(q)
    _report(f"reduce q {dtype} T {T} initial {initial} {dev.last_kernel()}", got, want, (2 * C + 4) * EPS * mag)
    other = got if initial else a["p"]
    terms = other.real * got.real + other.imag * got.imag
    _report(f"reduce partials {dtype} T {T} initial {initial}", _down(part), _block_sums(terms),
            34 * EPS * _block_sums(np.abs(other.real * got.real) + np.abs(other.imag * got.imag)))
    assert _same_bits(_down(u).astype(np.complex128), un) and _same_bits(_down(p), a["p"])
    if misaligned:
        q2, part2 = torch.empty_like(q), torch.empty_like(part)
        dev.cgs_reduce(_up(a["u"]).to(u.dtype), s, None if initial else p, q2, part2, lam, initial)
        assert dev.last_kernel() == "k_cgs_reduce<c64, 2>" and _same_bits(_down(q2), got) and _same_bits(_down(part2), _down(part))


@pytest.mark.parametrize("final", [False, True])
@pytest.mark.parametrize("T", [5, 130])
def test_step_kernel(T, final):
    """One column per lane whatever the data's dtype: T = 5 less than a tile, T = 130 two tiles and a remainder; V = 37.
    Column 0 runs, 2 has converged, 3 breaks down (delta < 0), 4 has a rho0 that is not finite; columns 1, 4, 7 ... come in
    frozen."""
    import torch

    from xmris_amd import device as dev

    a = _kernel_inputs(T)
    rng = np.random.default_rng(7)
    rho0, rho, delta = (rng.uniform(0.5, 1.5, (NB, T)) for _ in range(3))
    status_in = a["status"].copy()
    status_in[[0, 2, 3]] = 0
    status_in[4] = 0
    rho[:, 2] = 1e-14 * rho0[:, 2]  # rho <= tol^2 rho0 at tol 1e-6
    delta[1, 3] = -5.0
    rho0[2, 4] = np.inf
    x, r, p, q = _up(a["x"]), _up(a["r"]), _up(a["p"]), _up(a["q"])
    rho_out = torch.full((NB, T), -1.0, dtype=torch.float64, device="cuda")
    status_out = torch.full((T,), -1, dtype=torch.int32, device="cuda")
    n_iter = torch.full((T,), 2, dtype=torch.int32, device="cuda")
    residual = torch.full((T,), -1.0, dtype=torch.float64, device="cuda")
    dev.cgs_step(x, r, p, q, _up(rho), _up(rho0), None if final else _up(delta), rho_out, _up(status_in), status_out, n_iter,
                 residual, 1e-6, 3, final)
    assert dev.last_kernel() == "k_cgs_step<c128, 1>", dev.last_kernel()
    t_rho, t_rho0, t_delta = _total(rho), _total(rho0), _total(delta)
    want_status = status_in.copy()
    active = status_in == 0
    want_status[active & ~np.isfinite(t_rho0)] = 3
    conv = active & np.isfinite(t_rho0) & (t_rho <= 1e-12 * t_rho0)
    want_status[conv] = 1
    running = active & np.isfinite(t_rho0) & ~conv
    if not final:
        want_status[running & ~(t_delta > 0)] = 2
    upd = running & (t_delta > 0) & (not final)
    assert want_status[0] == 0 and want_status[2] == 1 and want_status[3] == (0 if final else 2) and want_status[4] == 3
    assert np.array_equal(_down(status_out), want_status)
    assert np.array_equal(_down(n_iter), np.where(upd, 3, 2))
    alpha = np.where(upd, t_rho / np.where(upd, t_delta, 1.0), 0.0)
    gx, gr = _down(x), _down(r)
    assert np.all(np.isnan(gx[:, 4])) and _same_bits(gx[:, ~upd & (want_status != 3) | ~active], a["x"][:, ~upd & (want_status != 3) | ~active])
    assert _same_bits(gr[:, ~upd], a["r"][:, ~upd])
    if final:  # nothing moves (x and r are bit for bit the inputs, above)
        assert not upd.any() and np.all(_down(rho_out) == -1.0)
    else:
        bx = 2 * EPS * (np.abs(a["x"]) + np.abs(alpha * a["p"]))
        br = 2 * EPS * (np.abs(a["r"]) + np.abs(alpha * a["q"]))
        _report(f"step x T {T}", gx[:, upd], (a["x"] + alpha * a["p"])[:, upd], bx[:, upd])
        _report(f"step r T {T}", gr[:, upd], (a["r"] - alpha * a["q"])[:, upd], br[:, upd])
        terms = gr.real ** 2 + gr.imag ** 2
        _report(f"step partials T {T}", _down(rho_out)[:, upd], _block_sums(terms)[:, upd], 34 * EPS * _block_sums(terms)[:, upd])
        assert upd.sum() >= 1 and np.all(_down(rho_out)[:, ~upd] == -1.0)
    res = _down(residual)
    told = (active & (want_status != 0)) | (active & final)
    assert np.all(res[~told] == -1.0)
    ok = told & np.isfinite(t_rho0)
    assert np.allclose(res[ok], np.sqrt(t_rho / t_rho0)[ok], rtol=4 * EPS, atol=0) and np.isnan(res[4])
    assert _same_bits(_down(p), a["p"]) and _same_bits(_down(q), a["q"])


# ---- 2. recon_cg_sense against the oracle ---------------------------------------------------------------------------------
# columns per case: radial2d 5 (odd: the 8-byte form), masked2d 4 (one 16-byte word per two columns), random3d and odd2d
# 130 (a tile edge plus remainder; odd2d has V = 48, three voxel blocks), line1d 3 (V = 8: less than one block), long1d 6
# (G = 80: the staged transform)
COLUMNS = {"radial2d": 5, "masked2d": 4, "random3d": 130, "line1d": 3, "long1d": 6, "odd2d": 130}


def _labeled(x, dims):
    from xmris_amd import LabeledArray

    return LabeledArray(x, dims, {}, {}, None)


def _recon(c, y, iterations, tol=0.0, **kw):
    from xmris_amd import recon_cg_sense

    kw = dict(dict(regularization=c.reg, density=c.density, width=c.W, return_info=True), **kw)
    return recon_cg_sense(_labeled(y, ("coil", "sample", "time")), c.traj, c.s, iterations=iterations, tol=tol, **kw)


@functools.lru_cache(maxsize=None)
def _reference(name, dtype, iterations):
    """(data in `dtype` on the device, the oracle's x from that data); computed once and shared."""
    c = orc.case(name, COLUMNS[name])
    y = c.y.astype(dtype)
    x = orc.cg(c.dense(), c.rhs(y.astype(np.complex128)), iterations)[0]
    x.setflags(write=False)
    return c, y, x


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(orc.CASES))
def test_recon_matches_the_oracle(name, dtype):
    """6 iterations at tol 0 within CGS_TOL max |x|; see COLUMNS for the path each case's shape is there for."""
    from xmris_amd import device as dev

    c, y, want = _reference(name, dtype, 6)
    yd = _up(y)
    ds = _recon(c, yd, 6)
    assert "k_cgs_step" in dev.last_kernel()
    got = _down(ds["image"].data).reshape(c.V, c.T)
    tol = CGS_TOL64 if dtype == "complex64" else CGS_TOL128
    err = orc.rel(got, want)
    print(f"recon {name} {dtype} T {c.T}: {err / tol:.3f} of its bound")
    assert got.dtype == np.complex128 and ds["image"].dims == ("x", "y", "z")[:len(c.ms)] + ("time",)
    assert np.all(_down(ds["iterations"].data) == 6) and np.all(_down(ds["status"].data) == 0)
    assert np.all(np.isfinite(_down(ds["residual"].data)))
    assert err <= tol
    assert _same_bits(_down(yd), y)  # the data is untouched
    if name == "masked2d":
        dead = (np.abs(c.sv) ** 2).sum(axis=0) == 0
        assert dead.sum() > 8 and np.all(got[dead] == 0) and np.all(got[~dead] != 0)


@pytest.mark.parametrize("name, dtype", [("radial2d", "complex128"), ("masked2d", "complex128"), ("random3d", "complex128"),
                                         ("radial2d", "complex64")])
def test_convergence(name, dtype):
    """30 iterations reach the direct solve of the normal equations within 4 x the oracle's own distance.  Only where
    that distance is a convergence figure: at complex64 it must stand above the rounding of the chains (CGS_TOL64),
    which of these cases holds for radial2d alone."""
    c, y, _ = _reference(name, dtype, 6)
    ds = _recon(c, _up(y), 30)
    got = _down(ds["image"].data).reshape(c.V, c.T)
    d = orc.rel(got, c.solve(c.rhs(y.astype(np.complex128))))
    print(f"convergence {name} {dtype}: distance {d:.3e}, {d / (4 * DISTANCE30[name]):.3f} of its bound")
    assert d <= 4 * DISTANCE30[name]
    assert np.all(_down(ds["iterations"].data) == 30) and np.all(_down(ds["residual"].data) < 1e-5)


@pytest.mark.parametrize("dtype, tol", [("complex128", 0.0), ("complex64", 1e-6), ("complex64", 0.0)])
def test_exact_convergence_freezes_the_column(dtype, tol):
    """line1d has 8 unknowns, V = 8 is less than one voxel block.  In complex128 at tol 0 the residual is at rounding by
    step 8, the floor of 1e-14 stops the column, and the 11 launches that follow leave it alone.  In complex64 the chains
    round at 6e-8, so step 8 lands at 7e-8 (the oracle with complex64 rounding: tests/_cgsense_oracle.py), which stops
    the column at the default tol of 1e-6; at tol 0 the recurrence needs about 17 steps to the floor, and the check is
    that nothing turns NaN on the way."""
    c, y, _ = _reference("line1d", dtype, 6)
    ds = _recon(c, _up(y), 20, tol=tol)
    img, n, status = _down(ds["image"].data), _down(ds["iterations"].data), _down(ds["status"].data)
    res = _down(ds["residual"].data)
    print(f"line1d {dtype} tol {tol}: iterations {n.tolist()} status {status.tolist()} residual {res.tolist()}")
    assert np.all(np.isfinite(img)) and np.all(np.isfinite(res)) and np.all(n >= 6)
    if dtype == "complex64" and tol == 0.0:
        assert np.all(status <= 1) and np.all(res <= 1e-6)
    else:
        assert np.all(status == 1) and np.all(n <= 9) and np.all(res <= max(tol, 1e-14))
    want = c.solve(c.rhs(y.astype(np.complex128)))
    assert orc.rel(img.reshape(c.V, c.T), want) <= (CGS_TOL64 if dtype == "complex64" else CGS_TOL128)


@pytest.mark.parametrize("name, dtype", [("line1d", "complex64"), ("masked2d", "complex64"), ("masked2d", "complex128")])
def test_zero_and_nan_columns(name, dtype):
    """Column 1 zero: x = 0, converged at 0 iterations.  Column 1 with one NaN sample: status 3, a NaN image, and its
    neighbours bit for bit what they are without it -- in masked2d (T = 4, complex64) column 0 shares its 16-byte words
    with the NaN column."""
    c, y, _ = _reference(name, dtype, 6)
    clean = _recon(c, _up(y), 6)
    img = _down(clean["image"].data).reshape(c.V, c.T)
    z = y.copy()
    z[:, :, 1] = 0
    ds = _recon(c, _up(z), 6)
    got = _down(ds["image"].data).reshape(c.V, c.T)
    assert np.all(got[:, 1] == 0) and _down(ds["status"].data)[1] == 1 and _down(ds["iterations"].data)[1] == 0
    assert _down(ds["residual"].data)[1] == 0
    keep = [t for t in range(c.T) if t != 1]
    assert _same_bits(got[:, keep], img[:, keep])
    z[1, 3, 1] = np.nan
    ds = _recon(c, _up(z), 6)
    got = _down(ds["image"].data).reshape(c.V, c.T)
    status = _down(ds["status"].data)
    assert status[1] == 3 and np.all(np.isnan(got[:, 1])) and _down(ds["iterations"].data)[1] == 0
    assert np.all(status[keep] == 0) and _same_bits(got[:, keep], img[:, keep])
    assert _same_bits(_down(ds["residual"].data)[keep], _down(clean["residual"].data)[keep])


@pytest.mark.parametrize("dtype", DTYPES)
def test_columns_do_not_interact(dtype):
    """radial2d, 5 columns: `chunk=2` (the 16-byte form twice, then one column alone) and the columns one at a time (the
    8-byte form) give the bits of the one pass of 5."""
    c, y, _ = _reference("radial2d", dtype, 6)
    whole = _recon(c, _up(y), 6)
    img = _down(whole["image"].data)
    parts = _recon(c, _up(y), 6, chunk=2)
    assert _same_bits(_down(parts["image"].data), img)
    assert _same_bits(_down(parts["residual"].data), _down(whole["residual"].data))
    for t in range(c.T):
        one = _recon(c, _up(np.ascontiguousarray(y[:, :, t:t + 1])), 6)
        assert _same_bits(_down(one["image"].data)[..., 0], img[..., t]), t


@pytest.mark.parametrize("W", [4, 6])
def test_full_sampling_approaches_nufft_adjoint(W):
    """One coil, s = 1, regularization 0, a fully sampled Cartesian trajectory with pipe density: mu x is nufft_adjoint of
    the data within 2 x the figure recorded from the dense oracle (tests/test_cgsense.py)."""
    from xmris_amd import nufft_adjoint, recon_cg_sense

    y, traj, sens, mu = full_sampling_case(W)
    la = _labeled(_up(y), ("coil", "sample", "time"))
    x = _down(recon_cg_sense(la, traj, sens, iterations=10, tol=0.0, density="pipe", width=W).data)
    adj = _down(nufft_adjoint(la, traj, 8, width=W, density="pipe").data)[0]
    print(f"full sampling W {W}: {orc.rel(mu * x, adj):.3e} (recorded {FULL_SAMPLING[W]:.3e})")
    assert orc.rel(mu * x, adj) <= 2 * FULL_SAMPLING[W]


def test_layouts_whitening_and_host_input():
    """Coil and sample dims anywhere (one permuting copy) give the bits of the plain order; host input comes back as a
    host array; whitening by Psi = 4 I leaves the solution where it is."""
    from xmris_amd import recon_cg_sense

    c, y, want = _reference("radial2d", "complex128", 6)
    img = _down(_recon(c, _up(y), 6)["image"].data)
    moved = _labeled(_up(np.ascontiguousarray(np.transpose(y, (2, 1, 0)))), ("time", "sample", "coil"))
    got = recon_cg_sense(moved, c.traj, c.s, iterations=6, tol=0.0, regularization=c.reg, density="pipe")
    assert got.dims == ("time", "x", "y") and got.is_device_resident
    assert _same_bits(np.ascontiguousarray(np.moveaxis(_down(got.data), 0, -1)), img)
    host = recon_cg_sense(_labeled(y, ("coil", "sample", "time")), c.traj, c.s, iterations=6, tol=0.0, regularization=c.reg,
                          density="pipe")
    assert _same_bits(np.asarray(host.values), img)
    white = _recon(c, _up(y), 6, noise_cov=4.0 * np.eye(c.C))
    assert orc.rel(_down(white["image"].data).reshape(c.V, c.T), want) <= CGS_TOL128
