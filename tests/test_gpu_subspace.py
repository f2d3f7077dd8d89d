"""GPU tests of temporal-subspace SENSE: k_sub_project, k_sub_mix and k_sub_expand alone against
their sums in extended precision within the derived bound -- a sum of n products carries at most (n + 4) 2^-53 sum |terms|,
plus half an ulp of the output dtype -- and bit for bit against themselves (layout, batch, sampling=None, in place, NaN
where nothing was sampled); then whole calls of recon_subspace against the oracle within 16 x the oracle's own route
disagreement (tests/tool_subspace_tolerance.py), and their bitwise properties.

Shapes (R, T, C, S, F): the tile of k_sub_project is 16 rows (s, c, f) x 64 time points, one or two coefficients per thread
(R <= 16, R <= 32); of k_sub_mix one sample x 8 columns (c, f); of k_sub_expand 4 rows (v, f) x 256 time points.  The
list holds every value the issue names, one row, a partial tile, several workgroups, T below, at and above a chunk, and
R = 16 / 17 on either side of the two-coefficient form."""
import functools

import numpy as np
import pytest

import _cgsense_oracle as cg
import _subspace_oracle as orc
from test_subspace import SUB_TOL64, SUB_TOL128

pytestmark = pytest.mark.gpu

DTYPES = ["complex64", "complex128"]
SHAPES = [(1, 1, 1, 1, 1), (3, 5, 3, 7, 2), (16, 64, 3, 7, 3), (32, 70, 1, 7, 70), (32, 257, 3, 1, 1), (16, 257, 3, 7, 2),
          (3, 70, 1, 1, 70), (17, 64, 3, 7, 1), (1, 5, 1, 7, 3)]


def _up(a):
    import torch

    return torch.from_numpy(np.array(a)).to("cuda")  # (a copy: the shared cases are read-only)


def _down(t):
    return t.cpu().numpy()


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _rand(rng, shape, dtype=np.complex128):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(dtype)


@functools.lru_cache(maxsize=None)
def _inputs(shape, dtype):
    R, T, C, S, F = shape
    rng = np.random.default_rng(sum(shape))
    y, V, m = _rand(rng, (C, S, F, T), dtype), _rand(rng, (R, T)), rng.uniform(size=(S, T)) < 0.6
    a, K, U = _rand(rng, (C, S, R, F), dtype), _rand(rng, (S, R, R)), _rand(rng, (5, R, F))
    for x in (y, V, m, a, K, U):
        x.setflags(write=False)
    return y, V, m, a, K, U


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_project_kernel(shape, dtype):
    from xmris_amd import device as dev

    R, T, C, S, F = shape
    y, V, m, _, _, _ = _inputs(shape, dtype)
    yd, Vd, md = _up(y), _up(V), _up(m)
    got = _down(dev.sub_project(yd, Vd, md))
    assert "k_sub_project" in dev.last_kernel() and got.shape == (C, S, R, F) and got.dtype == y.dtype
    value, mag = orc.contract("rt,csft->csrf", V, np.where(m[None, :, None, :], y, 0).astype(np.complex128), conj_a=True)
    worst = orc.within(got, value, mag, 2 * T, dtype)
    print(f"project {shape} {dtype}: {worst:.3f} of its bound")
    assert worst <= 1.0
    assert _same_bits(_down(yd), y)
    # the layout: the frames outermost, addressed where they lie
    strided = _up(np.ascontiguousarray(np.moveaxis(y, 2, 0))).permute(1, 2, 0, 3)
    assert F == 1 or C * S == 1 or not strided.is_contiguous()
    assert _same_bits(_down(dev.sub_project(strided, Vd, md)), got)
    # a frame alone
    f = F - 1
    assert _same_bits(_down(dev.sub_project(yd[:, :, f:f + 1], Vd, md))[..., 0], got[..., f])
    # sampling=None is all ones
    ones = _down(dev.sub_project(yd, Vd, _up(np.ones((S, T), bool))))
    assert _same_bits(_down(dev.sub_project(yd, Vd, None)), ones)
    # NaN where nothing was sampled changes no bit; NaN at a sampled position reaches its own row only
    off, on = np.argwhere(~m), np.argwhere(m)
    if len(off):
        z = y.copy()
        z[:, off[:, 0], :, off[:, 1]] = np.nan
        assert _same_bits(_down(dev.sub_project(_up(z), Vd, md)), got)
    if len(on):
        s, t = on[len(on) // 2]
        z = y.copy()
        z[C - 1, s, F - 1, t] = np.nan
        bad = _down(dev.sub_project(_up(z), Vd, md))
        assert np.all(np.isnan(bad[C - 1, s, :, F - 1]))
        bad[C - 1, s, :, F - 1] = got[C - 1, s, :, F - 1]
        assert _same_bits(bad, got)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_mix_kernel(shape, dtype):
    from xmris_amd import device as dev

    R, T, C, S, F = shape
    _, _, _, a, K, _ = _inputs(shape, dtype)
    ad, Kd = _up(a), _up(K)
    got = _down(dev.sub_mix(ad, Kd))
    assert "k_sub_mix" in dev.last_kernel() and got.shape == a.shape and got.dtype == a.dtype and _same_bits(_down(ad), a)
    value, mag = orc.contract("srp,cspf->csrf", K, a.astype(np.complex128))
    worst = orc.within(got, value, mag, 2 * R, dtype)
    print(f"mix {shape} {dtype}: {worst:.3f} of its bound")
    assert worst <= 1.0
    assert dev.sub_mix(ad, Kd, out=ad) is ad and _same_bits(_down(ad), got)  # in place
    f = F - 1
    assert _same_bits(_down(dev.sub_mix(_up(a[..., f:f + 1]), Kd))[..., 0], got[..., f])


@pytest.mark.parametrize("shape", SHAPES)
def test_expand_kernel(shape):
    from xmris_amd import device as dev

    R, T, C, S, F = shape
    _, V, _, _, _, U = _inputs(shape, "complex128")
    Ud, Vd = _up(U), _up(V)
    got = _down(dev.sub_expand(Ud, Vd))
    assert "k_sub_expand" in dev.last_kernel() and got.shape == (5, F, T) and got.dtype == np.complex128
    value, mag = orc.contract("vrf,rt->vft", U, V)
    worst = orc.within(got, value, mag, 2 * R, "complex128")
    print(f"expand {shape}: {worst:.3f} of its bound")
    assert worst <= 1.0
    f = F - 1
    assert _same_bits(_down(dev.sub_expand(_up(U[..., f:f + 1]), Vd))[:, 0], got[:, f])
    assert _same_bits(_down(dev.sub_expand(_up(U[3:4]), Vd))[0], got[3])


# ---- whole calls ---------------------------------------------------------------------------------------------------------
def _labeled(x, dims):
    from xmris_amd import LabeledArray

    return LabeledArray(x, dims, {}, {}, None)


def _recon(p, y, iterations=6, tol=0.0, dims=("coil", "sample", "rep", "time"), **kw):
    from xmris_amd import recon_subspace

    c = p.c
    kw = dict(dict(regularization=c.reg, density=c.density, width=c.W, return_info=True, sampling=p.m), **kw)
    return recon_subspace(_labeled(y, dims), c.traj, c.s, p.V, iterations=iterations, tol=tol, **kw)


@functools.lru_cache(maxsize=None)
def _reference(name, keep, frames, dtype):
    """(the problem, its data in `dtype`, the oracle's image after 6 iterations from that data); computed once, shared."""
    p = orc.problem(name, keep, frames)
    y = p.y.astype(dtype)
    b = p.rhs(orc.project(y.astype(np.complex128), p.V, p.m))
    x = p.image(p.folded(p.dense(), b, 6)[0])
    x.setflags(write=False)
    return p, y, x


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("frames", [1, 4])
@pytest.mark.parametrize("keep", [1.0, 0.5])
@pytest.mark.parametrize("name", ["radial2d", "masked2d", "odd2d", "line1d", "random3d"])
def test_recon_matches_the_oracle(name, keep, frames, dtype):
    """6 iterations at tol 0 within SUB_TOL max |x|.  frames = 1: R F = 3 columns, the 8-byte form of the chains; odd2d:
    V R = 144, several voxel blocks."""
    p, y, want = _reference(name, keep, frames, dtype)
    yd = _up(y)
    ds = _recon(p, yd, sampling=None if keep == 1.0 else p.m)
    got = _down(ds["image"].data).reshape(p.c.V, frames, p.T)
    tol = SUB_TOL64 if dtype == "complex64" else SUB_TOL128
    err = cg.rel(got, want)
    print(f"recon {name} keep {keep} frames {frames} {dtype}: {err / tol:.3f} of its bound")
    assert got.dtype == np.complex128 and ds["image"].dims == ("x", "y", "z")[:len(p.c.ms)] + ("rep", "time")
    assert np.all(_down(ds["iterations"].data) == 6) and np.all(_down(ds["status"].data) == 0)
    assert err <= tol
    assert _same_bits(_down(yd), y)  # the data is untouched
    if name == "masked2d":
        dead = (np.abs(p.c.sv) ** 2).sum(axis=0) == 0
        assert dead.sum() > 8 and np.all(got[dead] == 0) and np.all(got[~dead] != 0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_frames_chunks_layouts_and_coefficients(dtype):
    from xmris_amd import device as dev

    p, y, _ = _reference("radial2d", 0.5, 4, dtype)
    ds = _recon(p, _up(y), return_coefficients=True)
    img = _down(ds["image"].data)
    # the coefficients expand to the image through k_sub_expand, bit for bit
    co = ds["coefficients"].data
    assert tuple(co.shape) == (8, 8, 3, 4) and ds["coefficients"].dims == ("x", "y", "coefficient", "rep")
    again = _down(dev.sub_expand(co.reshape(64, 3, 4).contiguous(), _up(p.V))).reshape(8, 8, 4, p.T)
    assert _same_bits(again, img)
    # chunk = 1 and a frame alone give the bits of the one pass; the frames outermost are read where they lie
    one = _recon(p, _up(y), chunk=1)
    assert _same_bits(_down(one["image"].data), img) and _same_bits(_down(one["residual"].data), _down(ds["residual"].data))
    alone = _recon(p, _up(y[:, :, 2:3]))
    assert _same_bits(_down(alone["image"].data)[:, :, 0], img[:, :, 2])
    outer = _recon(p, _up(np.ascontiguousarray(np.moveaxis(y, 2, 0))), dims=("rep", "coil", "sample", "time"))
    assert outer["image"].dims == ("rep", "x", "y", "time") and _same_bits(_down(outer["image"].data), np.ascontiguousarray(np.moveaxis(img, 2, 0)))
    # garbage where nothing was sampled reaches nothing
    junk = np.where(p.m[None, :, None, :], y, np.nan).astype(dtype)
    assert _same_bits(_down(_recon(p, _up(junk))["image"].data), img)


@pytest.mark.parametrize("name, dtype", [("line1d", "complex64"), ("masked2d", "complex128")])
def test_zero_and_nan_frames(name, dtype):
    """Frame 1 zero: zero coefficients, converged at 0 iterations.  Frame 1 with one NaN at a sampled position: status 3,
    a NaN image, and its neighbours bit for bit what they are without it."""
    p, y, _ = _reference(name, 0.5, 4, dtype)
    clean = _recon(p, _up(y))
    img = _down(clean["image"].data).reshape(p.c.V, 4, p.T)
    keep = [0, 2, 3]
    z = y.copy()
    z[:, :, 1] = 0
    ds = _recon(p, _up(z))
    got = _down(ds["image"].data).reshape(p.c.V, 4, p.T)
    assert np.all(got[:, 1] == 0) and _down(ds["status"].data)[1] == 1 and _down(ds["iterations"].data)[1] == 0
    assert _same_bits(got[:, keep], img[:, keep])
    s, t = np.argwhere(p.m)[7]
    z[1, s, 1, t] = np.nan
    ds = _recon(p, _up(z))
    got, status = _down(ds["image"].data).reshape(p.c.V, 4, p.T), _down(ds["status"].data)
    assert status[1] == 3 and np.all(np.isnan(got[:, 1])) and np.all(status[keep] == 0)
    assert _same_bits(got[:, keep], img[:, keep])
    # all-false sampling: a zero image with status 1
    ds = _recon(p, _up(y), sampling=np.zeros_like(p.m))
    assert np.all(_down(ds["image"].data) == 0) and np.all(_down(ds["status"].data) == 1)


def test_convergence_to_the_direct_solve():
    """odd2d with half the positions kept, complex128, tol 1e-10: the oracle's folded recurrence converges in 40
    iterations; the GPU's stops converged too and lies within cond(M) x its residual of the direct solve."""
    p, y, _ = _reference("odd2d", 0.5, 1, "complex128")
    ds = _recon(p, _up(y), iterations=60, tol=1e-10)
    ev = np.linalg.eigvalsh(p.normal_matrix())
    got = _down(ds["image"].data).reshape(p.c.V, 1, p.T)
    d = orc.err(got, p.image(p.solve()))
    res, n = float(_down(ds["residual"].data)[0]), int(_down(ds["iterations"].data)[0])
    print(f"convergence odd2d: distance {d:.3e} residual {res:.3e} iterations {n}")
    assert _down(ds["status"].data)[0] == 1 and res <= 1e-10 and n <= 60
    assert d <= (ev.max() / ev.min()) * res
