"""k_species (csrc/xm_species.h) on the GPU against tests/_species_oracle.py: known-field parity, the layouts the kernel
addresses in place, field-fit parity, round trips, status codes, batch independence, invariants of every returned row,
the refusals of the C ABI with real buffers, and the public call.  tests/test_species.py pins the oracle and the
selection of the cases on the CPU."""
import ctypes

import numpy as np
import pytest

import _species_oracle as orc
from test_species import FIT_NAMES, _fit_case, _known_case

EPS = np.finfo(np.float64).eps

# tests/tool_species_tolerance.py -> profiles/species/tolerance.txt (CPU only, the kernel is not involved), the largest
# figure over all parity cases; the kernel is a third summation order with the device's own sincospi: 16 x each.
# (a) the factorised estimate against per-row lstsq on A_r and against the reversed echo order: 4.257e-15 of the case's
# largest magnitude.  complex64 output adds 2^-23 of that magnitude for the one rounding.
A_MEASURED = 4.257e-15
A_TOL = 16 * A_MEASURED
# (b) psi* of the restated iteration against brentq on G' with W summed in reversed column order: 5.615e-14 delta.
B_MEASURED = 5.615e-14
B_TOL = 16 * B_MEASURED
# (c) residual between the two routes of (b): 1.443e-15.
C_MEASURED = 1.443e-15
C_TOL = 16 * C_MEASURED
C64 = 2.0 ** -23
DTYPES = (np.complex64, np.complex128)


def _up(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _np(res):
    """A SpeciesResult as host arrays."""
    g = lambda t: None if t is None else t.cpu().numpy()  # noqa: E731
    return dict(species=g(res.species), field=g(res.field), residual=g(res.residual), status=g(res.status),
                copied=res.copied, levels=res.levels)


def _run(y, c, tau="case", psi=None, fit=False, max_field=None):
    """y [R, E, C] (host, any complex dtype) through device.species_separate; every output as numpy."""
    from xmris_amd import device as dev

    res = dev.species_separate(_up(y), 1, [2], c["te"], c["f"], c["r"], tau=c["tau"] if isinstance(tau, str) else tau,
                               psi=psi, fit_field=fit, max_field=max_field)
    assert "k_species" in dev.last_kernel() and ("fit" if fit else "known") in dev.last_kernel()
    return _np(res)


def _same(a, b, ra=slice(None), rb=slice(None)):
    return all((a[k] is None and b[k] is None) or np.array_equal(a[k][ra], b[k][rb], equal_nan=True)
               for k in ("species", "field", "residual", "status"))


def _bound(dtype, scale):
    return (A_TOL + (C64 if dtype == np.complex64 else 0.0)) * scale


# ---- 1. known field --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("E,M", orc.KNOWN_EM)
def test_known_field_matches_the_oracle(E, M, dtype):
    """Every row count around the 64-row tile and every column count around the four waves: non-uniform unsorted echo
    times, decay, delays up to 5 ms, fields up to +-300 Hz.  The reference is the oracle on the kernel's input (the case
    rounded to `dtype`)."""
    worst = 0.0
    for rows in orc.KNOWN_ROWS:
        for cols in orc.KNOWN_COLS:
            c = _known_case(E, M, rows, cols)
            y = c["y"].astype(dtype)
            ref = c["ref"] if dtype == np.complex128 else orc.known(y.astype(np.complex128), c["te"], c["f"], c["r"], c["tau"], c["psi"])
            out = _run(y, c, psi=c["psi"])
            assert out["species"].dtype == dtype and out["species"].shape == (rows, M, cols)
            assert not out["copied"] and out["residual"] is None
            assert np.all(out["status"] == 0) and np.array_equal(out["field"], c["psi"])
            err = np.abs(out["species"] - ref).max() / np.abs(ref).max()
            worst = max(worst, err / _bound(dtype, 1.0))
            assert err <= _bound(dtype, 1.0), (rows, cols, err)
    print(f"known field E {E} M {M} {np.dtype(dtype)}: largest share of the bound {worst:.3f}")


# ---- 2. layouts --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("fit", [False, True])
def test_layouts_agree_bit_for_bit_and_say_whether_they_copied(fit):
    import torch

    from xmris_amd import device as dev

    REP, E, C, S = 3, 8, 4, 70
    c = orc.make_case(E, 3, REP * S, C, seed=77, max_field=40.0 if fit else None, psi_max=40.0)
    base = np.transpose(c["y"].reshape(REP, S, E, C), (0, 2, 3, 1)).astype(np.complex64)  # [repetition, echo, coil, sample]
    tau = c["tau"][:S]
    psi = None if fit else c["psi"].reshape(REP, S)
    kw = dict(echo_times=c["te"], frequencies=c["f"], decay=c["r"], fit_field=fit, max_field=40.0 if fit else None)
    x = _up(base)

    nat = dev.species_separate(x, 1, [2], tau=tau[None, :], psi=None if fit else _up(psi), **kw)
    assert not nat.copied and nat.levels == (2, 1) and nat.species.shape == (REP, 3, C, S) and nat.species.is_contiguous()
    a = _np(nat)
    assert np.all(a["status"] == 0)

    img = x.permute(1, 2, 0, 3).contiguous()  # [echo, coil, x, y]: the rows (x, y) merge into one level
    r = dev.species_separate(img, 0, [1], tau=np.broadcast_to(tau, (REP, S)).copy(), psi=None if fit else _up(psi), **kw)
    assert not r.copied and r.levels == (1, 1)
    b = _np(r)
    assert np.array_equal(b["species"], np.transpose(a["species"], (1, 2, 0, 3)))
    assert all(np.array_equal(b[k], a[k], equal_nan=True) for k in ("field", "status")) and (not fit or np.array_equal(b["residual"], a["residual"]))
    r = dev.species_separate(img, 0, [1], tau=tau[None, :], psi=None if fit else _up(psi), **kw)  # tau along y only: two levels
    assert not r.copied and r.levels == (2, 1) and np.array_equal(_np(r)["species"], b["species"])

    last = x[0].permute(1, 2, 0).contiguous()  # [coil, sample, echo]: the echoes are read with a stride
    r = dev.species_separate(last, 2, [0], tau=tau, psi=None if fit else _up(psi[0]), **kw)
    assert not r.copied and r.levels == (1, 1) and r.species.shape == (C, S, 3)
    d = _np(r)
    assert np.array_equal(d["species"], np.transpose(a["species"][0], (1, 2, 0))) and np.array_equal(d["field"], a["field"][0])

    view = x.permute(0, 3, 1, 2)  # a view, [repetition, sample, echo, coil] by strides: still no copy
    r = dev.species_separate(view, 2, [3], tau=tau[None, :], psi=None if fit else _up(psi), **kw)
    assert not r.copied and np.array_equal(_np(r)["species"], np.transpose(a["species"], (0, 3, 1, 2)))

    five = x.reshape(REP, E, C, 7, 10).permute(0, 1, 3, 2, 4).contiguous()  # [a, echo, b, coil, c]: three row levels
    r = dev.species_separate(five, 1, [3], tau=tau.reshape(1, 7, 10), psi=None if fit else _up(psi.reshape(REP, 7, 10)), **kw)
    assert r.copied and r.species.shape == (REP, 3, 7, C, 10)
    e = _np(r)
    assert np.array_equal(np.transpose(e["species"], (0, 1, 3, 2, 4)).reshape(REP, 3, C, S), a["species"])
    assert np.array_equal(e["field"].reshape(REP, S), a["field"]) and np.array_equal(e["status"].reshape(REP, S), a["status"])
    assert torch.equal(x, _up(base))  # the input is left as it was


# ---- 3. field fit ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", FIT_NAMES)
def test_field_fit_matches_the_oracle(name):
    """psi*, the species and the residual of every row within (b), (a), (c) of the restated iteration.  The cases are
    those tests/test_species.py shows to be decided on every row; iteration counts are not compared."""
    c = _fit_case(name)
    out = _run(c["y"], c, fit=True, max_field=c["max_field"])
    assert np.array_equal(out["status"], c["status"]) and not out["copied"]
    e_b = np.abs(out["field"] - c["field"]).max() / c["delta"]
    e_a = np.abs(out["species"] - c["species"]).max() / np.abs(c["species"]).max()
    e_c = np.abs(out["residual"] - c["residual"]).max()
    print(f"field fit {name}: psi* {e_b:.3e} delta ({e_b / B_TOL:.3f} of the bound), species {e_a:.3e} ({e_a / A_TOL:.3f}), "
          f"residual {e_c:.3e} ({e_c / C_TOL:.3f})")
    assert e_b <= B_TOL and e_a <= A_TOL and e_c <= C_TOL


def test_grid_sizes_around_the_cap():
    """512.5 grid spacings give the 1025-point grid that still runs, 513.2 the 1027 points that are refused (test 8)."""
    from xmris_amd import device as dev

    te = np.array([1e-3, 2e-3, 3.5e-3])
    delta, _ = dev.species_grid(te, 1.0)
    assert dev.species_grid(te, 512.5 * delta)[1] == 512 and dev.species_grid(te, 513.2 * delta)[1] == 513


# ---- 4. round trip ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_round_trip_of_the_forward_model():
    from xmris_amd import simulate_echoes

    rng = np.random.default_rng(41)
    E, M, C, R = 8, 3, 4, 65
    te, f, r = orc.echo_times(E, rng), np.array(orc.FREQS[:M]), np.array(orc.DECAYS[:M])
    rho = rng.standard_normal((R, M, C)) + 1j * rng.standard_normal((R, M, C))
    tau, psi = rng.uniform(0, 5e-3, R), rng.uniform(-48.0, 48.0, R)
    y = simulate_echoes(rho, f, te, decay=r, readout_time=tau[:, None], field_map=psi[:, None], axis=1)
    c = dict(te=te, f=f, r=r, tau=tau)
    delta, _ = orc.grid(te, 60.0)
    out = _run(y, c, fit=True, max_field=60.0)
    assert np.all(out["status"] == 0)
    e_b, e_c = np.abs(out["field"] - psi).max() / delta, out["residual"].max()
    known = _run(y, c, psi=psi)
    e_a = np.abs(known["species"] - rho).max() / np.abs(rho).max()
    print(f"round trip: psi* {e_b:.3e} delta ({e_b / B_TOL:.3f} of the bound), residual {e_c / EPS:.1f} eps, species {e_a:.3e} ({e_a / A_TOL:.3f})")
    assert e_b <= B_TOL and e_c <= 64 * EPS and e_a <= A_TOL


# ---- 5. status ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_field_outside_the_window_ends_at_the_window_end_with_status_1():
    c = orc.make_case(8, 3, 1, 2, seed=3, max_field=40.0)
    delta, _ = orc.grid(c["te"], 40.0)
    mf = 2.5 * delta
    rho = np.ones((3, 3, 2), dtype=np.complex128)
    y = orc.forward(rho, c["te"], c["f"], c["r"], np.zeros(3), np.array([mf + 0.4 * delta, -mf - 0.4 * delta, 0.3 * delta]))
    out = _run(y, c, tau=None, fit=True, max_field=mf)
    assert out["status"].tolist() == [1, 1, 0] and out["field"][0] == mf and out["field"][1] == -mf
    for i in range(2):  # the row is still separated, at the end of the window
        ref = orc.known(y[i:i + 1], c["te"], c["f"], c["r"], np.zeros(1), out["field"][i:i + 1])
        assert np.abs(out["species"][i] - ref[0]).max() <= A_TOL * np.abs(ref).max()
    assert abs(out["field"][2] - 0.3 * delta) <= B_TOL * delta


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fit", [False, True])
def test_non_finite_and_all_zero_rows(fit, dtype):
    c = orc.make_case(8, 3, 70, 5, seed=51, max_field=40.0 if fit else None, psi_max=40.0)
    y = c["y"].astype(dtype)
    kw = dict(fit=True, max_field=40.0) if fit else dict(psi=c["psi"])
    clean = _run(y, c, **kw)
    assert np.all(clean["status"] == 0)
    bad = y.copy()
    bad[10, 3, 4] = np.nan
    bad[66, 0, 0] = complex(0.0, np.inf)
    bad[20] = 0.0
    out = _run(bad, c, **kw)
    want = np.zeros(70, dtype=np.int32)
    want[[10, 66]], want[20] = 2, 3
    assert np.array_equal(out["status"], want)
    for i in (10, 66):
        assert not out["species"][i].any() and np.isnan(out["field"][i]) and (not fit or np.isnan(out["residual"][i]))
    assert not out["species"][20].any() and (not fit or (out["field"][20] == 0.0 and out["residual"][20] == 0.0))
    rest = np.flatnonzero(want == 0)  # the neighbours in both tiles are untouched, bit for bit
    assert _same(out, clean, rest, rest)
    # a non-finite delay, and in the known-field form a non-finite field
    tau = c["tau"].copy()
    tau[7] = np.nan
    t = _run(y, c, tau=tau, **kw)
    assert t["status"][7] == 2 and not t["species"][7].any() and np.isnan(t["field"][7]) and _same(t, clean, rest[rest != 7], rest[rest != 7])
    if not fit:
        psi = c["psi"].copy()
        psi[69] = np.inf
        p = _run(y, c, psi=psi)
        assert p["status"][69] == 2 and not p["species"][69].any() and np.isnan(p["field"][69]) and np.all(p["status"][:69] == 0)


# ---- 6. batch independence -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fit", [False, True])
def test_a_row_does_not_depend_on_its_batch(fit, dtype):
    c = orc.make_case(8, 3, 257, 5, seed=61, max_field=40.0 if fit else None, psi_max=40.0)
    y = c["y"].astype(dtype)
    kw = (lambda s: dict(fit=True, max_field=40.0)) if fit else (lambda s: dict(psi=c["psi"][s]))
    whole = _run(y, c, **kw(slice(None)))
    part = _run(y[5:70], c, tau=c["tau"][5:70], **kw(slice(5, 70)))
    assert np.all(whole["status"] == 0) and _same(part, whole, slice(None), slice(5, 70))


# ---- 7. invariants ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_outputs_follow_from_the_returned_field(dtype):
    """residual and species recomputed on the host from the returned psi* (the kernel's own input, widened)."""
    c = orc.make_case(8, 3, 65, 5, seed=71, max_field=100.0)
    y = c["y"].astype(dtype)
    out = _run(y, c, fit=True, max_field=100.0)
    assert np.all((out["status"] >= 0) & (out["status"] <= 4)) and np.all(out["status"] == 0)
    yw = y.astype(np.complex128)
    Pi = orc.projector(orc.a0(c["te"], c["f"], c["r"]))
    pe, pf = orc.pairs(8)
    dl = c["te"][pf] - c["te"][pe]
    e_c = 0.0
    for i in range(65):
        w0, W, syy = orc.gram_w(yw[i], Pi)
        e_c = max(e_c, abs(out["residual"][i] - max(0.0, 1.0 - orc.G(out["field"][i], w0, W, dl) / syy)))
    ref = orc.known(yw, c["te"], c["f"], c["r"], c["tau"], out["field"])
    e_a = np.abs(out["species"] - ref).max() / np.abs(ref).max()
    print(f"invariants {np.dtype(dtype)}: residual {e_c:.3e} ({e_c / C_TOL:.3f} of the bound), species {e_a:.3e} ({e_a / _bound(dtype, 1.0):.3f})")
    assert e_c <= C_TOL and e_a <= _bound(dtype, 1.0)
    assert np.abs(out["field"]).max() <= 100.0


# ---- 8. the C ABI refuses -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_abi_refusals_with_real_buffers():
    import torch

    from xmris_amd import _lib
    from xmris_amd import device as dev

    lib = _lib.load()
    x = torch.zeros(4 * 33 * 2, dtype=torch.complex64, device="cuda")
    y = torch.full((4 * 9 * 2,), 7.0, dtype=torch.complex64, device="cuda")
    tab = torch.zeros(4096, dtype=torch.float64, device="cuda")
    field = torch.full((4,), 7.0, dtype=torch.float64, device="cuda")
    resid = torch.zeros(4, dtype=torch.float64, device="cuda")
    status = torch.full((4,), 7, dtype=torch.int32, device="cuda")
    i64 = lambda *v: (ctypes.c_int64 * len(v))(*v)  # noqa: E731

    def call(E=8, M=3, fit=0, max_field=50.0, span=7e-3, dtype=_lib.XM_C64, x_=x, y_=y, tab_=tab, field_=field, resid_=resid,
             status_=status, dims=(1, 4, 1, 2), null_dims=False):
        d = None if null_dims else i64(*dims)
        return lib.xm_species_separate(x_.data_ptr() if x_ is not None else None, y_.data_ptr() if y_ is not None else None,
                                       d, i64(0, E * 2, 0, 1, 2), i64(0, M * 2, 0, 1, 2), E, M,
                                       tab_.data_ptr() if tab_ is not None else None, None, 0, 0, None, 0, 0,
                                       field_.data_ptr() if field_ is not None else None,
                                       resid_.data_ptr() if resid_ is not None else None,
                                       status_.data_ptr() if status_ is not None else None, fit, max_field, span, dtype, None)

    bad = [dict(E=33), dict(E=1), dict(E=17, fit=1), dict(M=9, E=16), dict(M=0), dict(E=2, M=3), dict(E=3, M=3, fit=1),
           dict(x_=None), dict(y_=None), dict(tab_=None), dict(field_=None), dict(status_=None), dict(resid_=None, fit=1),
           dict(null_dims=True), dict(dims=(1, 4, 0, 2)), dict(dims=(1, -1, 1, 2)), dict(dtype=5),
           dict(fit=1, max_field=0.0), dict(fit=1, max_field=float("nan")), dict(fit=1, span=0.0),
           dict(fit=1, max_field=513.2 / (4 * 7e-3))]  # 1027 grid points
    for kw in bad:
        assert call(**kw) == _lib.XM_ERR_INVALID_ARG, kw
        assert "species_separate" in lib.xm_last_error_string().decode()
    torch.cuda.synchronize()
    assert torch.all(y.real == 7.0) and torch.all(field == 7.0) and torch.all(status == 7)  # nothing was written
    assert call(dims=(1, 0, 1, 2)) == 0 and call(dims=(0, 4, 1, 2)) == 0  # no rows: nothing is launched
    assert call(fit=1, max_field=512.5 / (4 * 7e-3), E=3, M=2) == 0  # 1025 grid points: the cap itself runs
    assert call(resid_=None) == 0
    torch.cuda.synchronize()
    assert torch.all(status == 3)  # (all-zero rows)
    with pytest.raises(_lib.XmrisHipError, match="1025"):
        dev.species_separate(torch.zeros((4, 3, 2), dtype=torch.complex64, device="cuda"), 1, [2], [0.0, 3e-3, 7e-3], [0.0, 100.0],
                             fit_field=True, max_field=513.2 / (4 * 7e-3))


# ---- 9. the public call ----------------------------------------------------------------------------------------------------------
def _public_case():
    from xmris_amd import LabeledArray, simulate_echoes

    rng = np.random.default_rng(91)
    F = {"pyruvate": 0.0, "lactate": 390.0}
    te = np.array([1e-3, 3.4e-3, 2.2e-3, 4.5e-3, 5.9e-3])
    rho = rng.standard_normal((2, 2, 3, 40)) + 1j * rng.standard_normal((2, 2, 3, 40))
    tau, psi = rng.uniform(0, 2e-3, 40), rng.uniform(-30, 30, (2, 40))
    truth = LabeledArray(rho, ("repetition", "species", "coil", "sample"), {"repetition": [0.0, 3.0], "coil": [0, 1, 2]}, {"MHz": 32.1})
    raw = simulate_echoes(truth, F, te, decay=[3.0, 9.0], readout_time=tau, field_map=LabeledArray(psi, ("repetition", "sample")))
    return F, te, rho, tau, psi, raw


@pytest.mark.gpu
def test_accessor_on_a_device_resident_array():
    from xmris_amd import LabeledArray, device as dev, species_matrix
    from xmris_amd.fitting.dataset import LabeledDataset
    from xmris_amd.processing.species import species_nsa

    F, te, rho, tau, psi, raw = _public_case()
    da = LabeledArray(dev.to_device(raw.values), raw.dims, raw.coords, raw.attrs)
    out = da.xmr.separate_species(F, decay=[3.0, 9.0], readout_time=tau, field_map=psi)
    assert "k_species" in dev.last_kernel()
    assert isinstance(out, LabeledArray) and out.is_device_resident and out.dims == ("repetition", "species", "coil", "sample")
    assert list(out.coords["species"].values) == ["pyruvate", "lactate"] and set(out.coords) == {"repetition", "coil", "species"}
    assert out.dtype == np.complex128 and np.abs(out.values - rho).max() <= A_TOL * np.abs(rho).max()
    assert out.attrs["MHz"] == 32.1 and out.attrs["species_field"] == "given" and out.attrs["species_echo_times"] == te.tolist()
    assert np.allclose(out.attrs["species_nsa"], species_nsa(species_matrix(F, te, [3.0, 9.0])), rtol=1e-14)
    ds = da.xmr.separate_species(F, decay=[3.0, 9.0], readout_time=tau, fit_field=True, max_field=45.0, return_field=True)
    assert isinstance(ds, LabeledDataset) and set(ds.data_vars) == {"species", "field", "residual", "status"}
    assert ds["field"].dims == ("repetition", "sample") and ds["field"].is_device_resident
    delta, _ = orc.grid(te, 45.0)
    assert np.all(ds["status"].values == 0) and np.abs(ds["field"].values - psi).max() <= B_TOL * delta
    assert ds.attrs["species_field"] == "fitted" and ds.attrs["species_max_field"] == 45.0


class _FakeDataset:
    """What tests/_fake_xarray.py lacks: the container LabeledDataset.to_xarray() builds."""

    def __init__(self, data_vars, attrs=None):
        self.data_vars, self.attrs = dict(data_vars), dict(attrs or {})

    def __getitem__(self, k):
        return self.data_vars[k]


@pytest.mark.gpu
def test_fake_xarray_in_gives_xarray_out(monkeypatch):
    import _fake_xarray

    from xmris_amd import accessor

    xr = _fake_xarray.install(monkeypatch)
    monkeypatch.setattr(xr, "Dataset", _FakeDataset, raising=False)
    accessor.register_xarray_accessor(force=True)
    F, te, rho, tau, psi, raw = _public_case()
    da = xr.DataArray(raw.values.astype(np.complex64), dims=raw.dims,
                      coords={"echo": xr.Variable("echo", te, {"units": "s"}), "repetition": [0.0, 3.0]}, attrs={"MHz": 32.1}, name="echoes")
    ds = da.xmr.separate_species(F, decay=[3.0, 9.0], readout_time=tau, fit_field=True, max_field=45.0, return_field=True)
    assert isinstance(ds, _FakeDataset) and set(ds.data_vars) == {"species", "field", "residual", "status"}
    sp = ds["species"]
    assert isinstance(sp, xr.DataArray) and isinstance(sp.data, np.ndarray) and sp.dtype == np.complex64 and sp.name == "echoes"
    assert sp.dims == ("repetition", "species", "coil", "sample") and list(sp.coords["species"].values) == ["pyruvate", "lactate"]
    assert set(sp.coords) == {"repetition", "species"} and ds.attrs["species_field"] == "fitted" and ds.attrs["MHz"] == 32.1
    assert len(ds.attrs["species_nsa"]) == 2 and ds["field"].dims == ("repetition", "sample")
    assert np.abs(sp.values - rho).max() <= 1e-5 * np.abs(rho).max() and np.abs(ds["field"].values - psi).max() <= 1e-3
    one = da.xmr.separate_species(F, decay=[3.0, 9.0], readout_time=tau, field_map=psi)
    assert isinstance(one, xr.DataArray) and one.dims == sp.dims and one.attrs["species_field"] == "given"


@pytest.mark.gpu
def test_species_then_nufft_adjoint():
    """2 species x 4 coils x 200 radial samples: each species' point source comes out where it is."""
    import _grid_oracle as grid

    from xmris_amd import LabeledArray, device as dev, simulate_echoes

    traj = grid.radial(16, 10, 20)
    spots = np.array([[3, -2], [-4, 5]])
    k = np.stack([np.exp(-2j * np.pi * (traj @ p) / 16) for p in spots])  # [species, sample]
    rho = k[:, None, :] * np.array([1.0, 0.5, -1.0, 2j])[None, :, None]
    te = np.array([1e-3, 2.2e-3, 3.1e-3, 4.5e-3])
    tau = (np.arange(200) % 20) * 4e-5
    F = {"pyruvate": 0.0, "lactate": 390.0}
    raw = simulate_echoes(LabeledArray(rho, ("species", "coil", "sample")), F, te, readout_time=tau)
    da = LabeledArray(dev.to_device(raw.values.astype(np.complex64)), raw.dims, raw.coords)
    sp = da.xmr.separate_species(F, readout_time=tau)
    assert sp.dims == ("species", "coil", "sample") and np.abs(sp.values - rho).max() <= 4 * C64 * np.abs(rho).max()
    img = sp.xmr.nufft_adjoint(traj, 16, density="pipe")
    assert img.is_device_resident and img.dims == ("species", "coil", "x", "y") and img.shape == (2, 4, 16, 16)
    mag = np.abs(img.values)
    for m in range(2):
        for c in range(4):
            assert np.unravel_index(np.argmax(mag[m, c]), (16, 16)) == (8 + spots[m, 0], 8 + spots[m, 1])
