"""k_espirit_eig and espirit_maps on the GPU against tests/_espirit_oracle.py.  The bounds are those
of tests/test_espirit.py: ESP_TOL_VALUE, ESP_TOL_RESIDUAL and ESP_TOL_MAP for the kernel against ``numpy.linalg.eigh`` on the
same matrices (16 x what ``_wg_oracle.jacobi`` and eigh disagree by on them, measured on the CPU), widened for a whole call
by what two routes to H may differ by (``value_tol``, ``map_tol``), and the conditions every calibration has to meet.

Shapes: V = 37 voxels is more than one pass of a small grid and no multiple of anything; C = 1 and 2 have no or one
rotation, 3 and 17 a bye in the round-robin pairing, 8 fills its pairs, 64 is the limit and fills the LDS."""
import functools

import numpy as np
import pytest

import _espirit_oracle as orc
import _sense_oracle as sense_orc
from test_espirit import (ESP_TOL_MAP, ESP_TOL_RESIDUAL, ESP_TOL_VALUE, K_DIMS, MAP_ERROR, UNFOLD_ERROR, check_conditions,
                          compare_with_oracle, map_tol, value_tol)

pytestmark = pytest.mark.gpu

V = 37
COILS = [1, 2, 3, 8, 17, 64]


def _up(a):
    import torch

    return torch.from_numpy(np.array(a)).to("cuda")  # (a copy: the shared cases are read-only)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def eig(h, c, **kw):
    """``device.espirit_eig`` on the host array h [V, C, C]: (maps [M, C, V], values [M, V], status [V]) on the host."""
    from xmris_amd import device as dev

    r = dev.espirit_eig(_up(orc.upper(h)), c, **kw)
    return r.maps.cpu().numpy(), r.values.cpu().numpy(), r.status.cpu().numpy()


@functools.lru_cache(maxsize=None)
def matrices(c):
    h, lam = orc.random_hermitian(c, V, c)
    h.setflags(write=False)
    return h, lam


def residual(h, maps_m, values_m):
    """||H m - lambda m|| / ||H||_F per voxel; maps_m [C, V]."""
    x = np.moveaxis(maps_m, 0, -1)
    r = np.linalg.norm(np.einsum("vcd,vd->vc", h, x) - values_m[:, None] * x, axis=-1)
    fro = np.sqrt((np.abs(h) ** 2).sum(axis=(1, 2)))
    return r / np.where(fro > 0, fro, 1.0)


# ---- the kernel alone ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_maps", [1, 2])
@pytest.mark.parametrize("c", COILS)
def test_kernel_against_eigh(c, n_maps):
    if n_maps > c:
        from xmris_amd._lib import XmrisHipError

        with pytest.raises(XmrisHipError, match="n_maps"):
            eig(matrices(c)[0], c, n_maps=n_maps)
        return
    h, spectrum = matrices(c)
    maps, values, status = eig(h, c, n_maps=n_maps, crop=0.0)
    lam, vec = np.linalg.eigh(h)
    want_maps, want_values = orc.select(lam, vec, n_maps, 0, 0.0)
    dv = float(np.abs(values - want_values).max())
    dm = float(np.abs(maps - want_maps).max())
    res = max(float(residual(h, maps[m], values[m]).max()) for m in range(n_maps))
    norm = float(np.abs((np.abs(maps) ** 2).sum(axis=1) - 1.0).max())
    print(f"kernel C {c:2d} M {n_maps}: values {dv:.3e} of {ESP_TOL_VALUE:.3e}, maps {dm:.3e} of {ESP_TOL_MAP:.3e}, "
          f"residual {res:.3e} of {ESP_TOL_RESIDUAL:.3e}, |norm - 1| {norm:.3e}")
    assert maps.shape == (n_maps, c, V) and values.shape == (n_maps, V) and not status.any()
    assert float(np.abs(values - spectrum[:n_maps, None]).max()) <= ESP_TOL_VALUE + 16 * c * orc_eps()
    assert dv <= ESP_TOL_VALUE and dm <= ESP_TOL_MAP and res <= ESP_TOL_RESIDUAL
    assert norm <= (2 * c + 8) * orc_eps()  # a C-term sum of squares, formed twice (kernel, test), and the division
    assert np.all(maps[:, 0].imag == 0) and np.all(maps[:, 0].real >= 0)  # the phase rule: coil 0 real and >= 0


def orc_eps():
    return float(np.finfo(np.float64).eps)


def test_phase_ref_crop_and_degenerate_voxels():
    c = 8
    h = np.array(matrices(c)[0])
    # voxel 5: lambda_1 = lambda_2 (any vector of the plane is an eigenvector: held to its residual alone)
    u = np.linalg.eigh(h[5])[1]
    spectrum = np.array(matrices(c)[1][::-1])
    spectrum[-2] = spectrum[-1]
    h[5] = (u * spectrum) @ u.conj().T
    # voxel 9: eigenvalues scaled below the crop; voxel 11: zero; voxel 13: coil 3 is not part of the first eigenvector
    h[9] *= 0.5
    h[11] = 0
    w = np.linalg.eigh(h[13])[1]
    w[3, -1] = 0
    q = np.linalg.qr(w[:, ::-1])[0][:, ::-1]  # orthonormal again, the first eigenvector a multiple of what it was
    assert abs(q[3, -1]) <= 4 * orc_eps()
    h[13] = (q * matrices(c)[1][::-1]) @ q.conj().T
    maps, values, status = eig(h, c, n_maps=2, crop=0.55, phase_ref=3)
    plain = eig(h, c, n_maps=2, crop=0.0, phase_ref=3)
    assert not status.any()
    assert np.all(maps[0, 3].imag == 0) and np.all(maps[0, 3].real >= 0) and np.all(maps[1, 3].imag == 0)
    # crop: exact zeros below, the very bits of the uncropped run at and above; values are never cropped
    assert _same_bits(values, plain[1])
    low = values < 0.55
    assert low[0, 9] and low[0, 11] and not low[0, 0] and low[1, 9] and not low[1, 0]  # 1 and 0.6 kept, 0.5 and 0.3 cropped
    assert np.all(maps[np.broadcast_to(low[:, None, :], maps.shape)] == 0)
    keep = np.broadcast_to(~low[:, None, :], maps.shape)
    assert _same_bits(maps[keep], plain[0][keep])
    # the zero voxel: eigenvalue 0 and, with any positive crop, a zero map
    assert np.all(values[:, 11] == 0) and np.all(maps[:, :, 11] == 0)
    # the degenerate voxel: both pairs are eigenpairs of lambda = 1
    for m in range(2):
        r = residual(h[5:6], plain[0][m][:, 5:6], plain[1][m][5:6])
        assert abs(plain[1][m, 5] - 1.0) <= ESP_TOL_VALUE and float(r.max()) <= ESP_TOL_RESIDUAL
    # a reference component that is (all but) zero: the vector is still an eigenvector of unit norm
    r = residual(h[13:14], plain[0][0][:, 13:14], plain[1][0][13:14])
    assert float(r.max()) <= ESP_TOL_RESIDUAL and abs(np.linalg.norm(plain[0][0][:, 13]) - 1) <= (2 * c + 8) * orc_eps()
    assert abs(plain[0][0][3, 13]) <= ESP_TOL_MAP
    # an exactly zero reference component leaves the vector as it is: C = 1 ... a diagonal matrix rotates nothing
    d = np.zeros((2, 3, 3), dtype=np.complex128)
    d[:, 0, 0], d[:, 1, 1], d[:, 2, 2] = 0.2, 1.0, 0.6
    dm, dv, ds = eig(d, 3, n_maps=2, crop=0.0, phase_ref=0)
    assert np.array_equal(dv[:, 0], [1.0, 0.6]) and np.array_equal(dm[0, :, 0], [0, 1, 0]) and np.array_equal(dm[1, :, 0], [0, 0, 1])
    # ties go to the lower column
    d[:, 2, 2] = 1.0
    dm, dv, ds = eig(d, 3, n_maps=2, crop=0.0)
    assert np.array_equal(dm[0, :, 1], [0, 1, 0]) and np.array_equal(dm[1, :, 1], [0, 0, 1]) and np.array_equal(dv[:, 1], [1.0, 1.0])


@pytest.mark.parametrize("c", [3, 64])
def test_voxels_are_independent_of_the_batch(c):
    h = np.array(matrices(c)[0])
    maps, values, status = eig(h, c, n_maps=2, crop=0.0)
    # a non-finite voxel: status 2, maps 0, values NaN; its neighbours keep their bits
    bad = h.copy()
    bad[7, 0, c - 1] = np.nan
    bad[20, 1, 1] = np.inf
    bm, bv, bs = eig(bad, c, n_maps=2, crop=0.0)
    assert list(np.flatnonzero(bs)) == [7, 20] and np.all(bs[[7, 20]] == 2)
    assert np.all(bm[:, :, [7, 20]] == 0) and np.all(np.isnan(bv[:, [7, 20]]))
    ok = np.ones(V, bool)
    ok[[7, 20]] = False
    assert _same_bits(bm[:, :, ok], maps[:, :, ok]) and _same_bits(bv[:, ok], values[:, ok])
    # a subset in another order gives the same bits as the full batch
    pick = np.array([30, 2, 17, 36, 0])
    sm, sv, ss = eig(h[pick], c, n_maps=2, crop=0.0)
    assert _same_bits(sm, np.ascontiguousarray(maps[:, :, pick])) and _same_bits(sv, np.ascontiguousarray(values[:, pick]))
    # more voxels than resident workgroups: every workgroup takes several, the bits stay
    many = np.concatenate([h] * 60)
    mm, mv, ms = eig(many, c, n_maps=2, crop=0.0)
    assert not ms.any() and _same_bits(mm.reshape(2, c, 60, V), np.ascontiguousarray(np.broadcast_to(maps[:, :, None, :], (2, c, 60, V))))
    assert _same_bits(mv.reshape(2, 60, V), np.ascontiguousarray(np.broadcast_to(values[:, None, :], (2, 60, V))))


def test_device_wrapper_refuses_what_the_kernel_cannot_take():
    import torch

    from xmris_amd import device as dev

    h = _up(orc.upper(matrices(3)[0]))
    with pytest.raises(ValueError, match="h must be"):
        dev.espirit_eig(h, 4)
    with pytest.raises(ValueError, match="h must be"):
        dev.espirit_eig(h.to(torch.complex64), 3)
    with pytest.raises(ValueError, match="n_coils"):
        dev.espirit_eig(h, 65)
    with pytest.raises(RuntimeError):
        dev.espirit_eig(h.cpu(), 3)


# ---- the whole call ------------------------------------------------------------------------------------------------------
def labeled_acs(c, device=True):
    from xmris_amd import LabeledArray

    data = _up(c.acs) if device else np.array(c.acs)
    return LabeledArray(data, ("coil",) + K_DIMS[:c.d] + ("time",), {}, {}, "acs")


@pytest.mark.parametrize("name", list(orc.CASES))
def test_whole_call_against_the_oracle(name):
    c = orc.case(name)
    ds = labeled_acs(c).xmr.espirit_maps(c.mat, kernel=c.kernel, dims=K_DIMS[:c.d], threshold=c.threshold, crop=0.0, n_maps=2,
                                         return_eigenvalues=True)
    ref = orc.reference(name, crop=0.0)
    assert not np.asarray(ds["status"].values).any() and ds.attrs["n_kernels"] == ref["n_kernels"]
    compare_with_oracle(c, ds, ref)
    check_conditions(name, orc.figures(c, np.asarray(ds["maps"].values), np.asarray(ds["eigenvalues"].values)))
    # one map at crop 0.9 from host input: the first map of the two-map run, cropped, bit for bit
    one = labeled_acs(c, device=False).xmr.espirit_maps(c.mat, kernel=c.kernel, dims=K_DIMS[:c.d], threshold=c.threshold, crop=0.9)
    lam = np.asarray(ds["eigenvalues"].values)[0]
    want = np.where((lam < 0.9)[None], 0.0, np.asarray(ds["maps"].values)[0])
    assert one.dims == ("coil",) + ("x", "y", "z")[:c.d] and isinstance(one.values, np.ndarray) and _same_bits(one.values, want)


def test_whole_call_layouts_and_the_staged_route():
    from xmris_amd import LabeledArray, espirit_maps

    c = orc.case("rect2d")
    kw = dict(kernel=c.kernel, threshold=c.threshold, crop=0.9, n_maps=2)
    base = labeled_acs(c).xmr.espirit_maps(c.mat, **kw)
    moved = LabeledArray(_up(np.ascontiguousarray(np.transpose(c.acs, (3, 2, 0, 1)))), ("time", "ky", "coil", "kx"), {}, {}, None)
    assert base.dims == ("map", "coil", "x", "y") and _same_bits(moved.xmr.espirit_maps(c.mat, **kw).values, base.values)
    assert _same_bits(espirit_maps(np.array(c.acs), c.mat, **kw).values, base.values)  # a plain host array
    assert _same_bits(espirit_maps(_up(c.acs), c.mat, **kw).values, base.values)  # a plain device tensor
    # 72 points along the only dim: zero_fill and fft in place of the table
    c = orc.case("line1d")
    ds = labeled_acs(c).xmr.espirit_maps(72, kernel=c.kernel, dims="kx", threshold=c.threshold, crop=0.0, n_maps=2,
                                         return_eigenvalues=True)
    want = orc.espirit(c.acs, (72,), c.kernel, threshold=c.threshold, crop=0.0, n_maps=2)
    dv = float(np.abs(np.asarray(ds["eigenvalues"].values) - want["values"]).max())
    big = want["values"][0] - want["values"][1] >= 0.5
    dm = float(np.abs(np.asarray(ds["maps"].values)[0] - want["maps"][0])[:, big].max())
    print(f"staged 72: values {dv:.3e} of {value_tol(c.C):.3e}, maps {dm:.3e} of {map_tol(c.C):.3e}")
    assert big.sum() > 36 and dv <= value_tol(c.C) and dm <= map_tol(c.C)


# ---- end to end ----------------------------------------------------------------------------------------------------------
def test_maps_feed_unfold_sense():
    from xmris_amd import LabeledArray

    c = orc.case("disc2d")
    maps = labeled_acs(c).xmr.espirit_maps(c.mat, kernel=c.kernel, threshold=c.threshold, crop=0.9)
    kept = sense_orc.undersample(c.k, [1, 2], (2, 1))
    img = LabeledArray(_up(kept), ("coil", "kx", "ky", "time"), {"kx": np.arange(16.0), "ky": np.arange(32.0)}, {}, None).xmr.to_image()
    full = img.xmr.unfold_sense(maps, accel=(2, 1))
    err = float(np.abs(full.values - c.rho).max() / np.abs(c.rho).max())
    print(f"disc2d: espirit_maps -> unfold_sense at accel (2, 1): {err:.3e} of max |object| (the oracle {UNFOLD_ERROR['disc2d']:.3e})")
    assert full.dims == ("x", "y", "time") and err <= 2 * UNFOLD_ERROR["disc2d"] and err < 0.1
    assert orc.map_error(c, maps.values) <= 2 * MAP_ERROR["disc2d"]


def test_maps_feed_recon_cg_sense_on_radial_data():
    """24 spokes of 64 samples over a 32 x 32 matrix (a third of what full sampling takes), the data made by the
    package's own nufft_forward from the true coil images.  Iterative SENSE with the ESPIRiT maps of the Cartesian centre
    against gridding + combine_coils; both measured by || a x - rho || / || rho || over all voxels with the best complex
    scalar a, so neither is charged for its scale."""
    import _grid_oracle as grid_orc
    from xmris_amd import LabeledArray

    c = orc.case("disc2d")
    traj = grid_orc.radial(32, 24, 64)
    truth = LabeledArray(_up(c.s[..., None] * c.rho[None]), ("coil", "x", "y", "time"), {}, {}, None)
    y = truth.xmr.nufft_forward(traj)
    maps = labeled_acs(c).xmr.espirit_maps(c.mat, kernel=c.kernel, threshold=c.threshold, crop=0.9)
    cg = y.xmr.recon_cg_sense(traj, maps, iterations=15, tol=0.0, density="pipe", regularization=0.01).values
    adj = y.xmr.nufft_adjoint(traj, 32, density="pipe").xmr.combine_coils().values

    def err(x):
        a = np.vdot(x, c.rho) / np.vdot(x, x)
        return float(np.linalg.norm(a * x - c.rho) / np.linalg.norm(c.rho))

    print(f"radial disc2d: recon_cg_sense with ESPIRiT maps {err(cg):.3e}, nufft_adjoint + combine_coils {err(adj):.3e}")
    assert cg.shape == adj.shape == (32, 32, 2) and err(cg) < err(adj)
