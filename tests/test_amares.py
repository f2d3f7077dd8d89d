"""AMARES quantification: fit_amares / simulate_fid (reference src/xmris/fitting, notebook fitting/pyamares.md:350-415).

CPU: the prior-knowledge reader, the oracle (tests/_amares_oracle.py) against the notebook's known answers, argument
checks of the C ABI.  GPU: the model kernel and the batched Levenberg-Marquardt kernel against the oracle."""
import os

import numpy as np
import pytest

import _amares_oracle as orc

HERE = os.path.dirname(os.path.abspath(__file__))
PK = os.path.join(HERE, "golden", "amares_pk_pcr_atp.csv")
PARAM_SCALE = lambda mhz: np.array([1.0, 1.0 / mhz, 1.0 / np.pi, 180.0 / np.pi, 1.0])  # noqa: E731  fit -> output units


# ---- CPU ------------------------------------------------------------------------------------------------------------
def test_prior_knowledge_reader(tmp_path):
    from xmris_amd.fitting.prior_knowledge import read_prior_knowledge

    pk = read_prior_knowledge(PK)
    assert pk.names == ["PCr", "ATP"]
    np.testing.assert_array_equal(pk.init, [[10.0, 0.0, 15.0, 0.0, 0.0], [5.0, -7.5, 20.0, 0.0, 0.0]])
    np.testing.assert_array_equal(pk.lo, [[0.0, -0.5, 5.0, -180, 0], [0.0, -8.0, 10.0, -180, 0]])
    np.testing.assert_array_equal(pk.hi, [[np.inf, 0.5, 30.0, 180, 1], [np.inf, -7.0, 40.0, 180, 1]])
    assert not pk.fixed.any()
    init, lo, hi = pk.fitting_units(120.0)
    o_init, o_lo, o_hi = orc.notebook_pk(120.0)
    np.testing.assert_allclose(init, o_init, rtol=1e-15)
    np.testing.assert_allclose(lo, o_lo, rtol=1e-15)
    np.testing.assert_allclose(hi, o_hi, rtol=1e-15)

    text = open(PK).read()
    # fixed (lo == hi), clipping into the bounds, an empty cell = unbounded
    p = tmp_path / "fixed.csv"
    p.write_text(text.replace('phase,"(-180, 180)","(-180, 180)"', 'phase,"(30, 30)",')
                 .replace("linewidth,15.0,20.0", "linewidth,50.0,20.0"))
    pk = read_prior_knowledge(p)
    assert pk.fixed[0, 3] and not pk.fixed[1, 3] and pk.init[0, 3] == 30.0
    assert pk.lo[1, 3] == -np.inf and pk.hi[1, 3] == np.inf and pk.init[0, 2] == 30.0

    bad = {
        "expr": (text.replace("amplitude,10.0,5.0", "amplitude,10.0,PCr*0.5"), "row 3.*'ATP'"),
        "unknown_row": (text.replace("g,0,0\nBounds", "width,0,0\nBounds"), "unknown row 'width'"),
        "non_numeric": (text.replace('linewidth,"(5.0, 30.0)"', 'linewidth,"(5.0, abc)"'), "row 11.*'PCr'"),
        "bound_syntax": (text.replace('"(-8.0, -7.0)"', '"-8.0 to -7.0"'), "row 10.*'ATP'"),
        "inverted": (text.replace('"(-8.0, -7.0)"', '"(-7.0, -8.0)"'), "row 10.*'ATP'"),
        "header": (text.replace("Index,", "Name,"), "first row"),
        "missing_amp": (text.replace("amplitude,10.0,5.0\n", ""), "no 'amplitude' row"),
    }
    for name, (content, match) in bad.items():
        p = tmp_path / f"{name}.csv"
        p.write_text(content)
        with pytest.raises(ValueError, match=match):
            read_prior_knowledge(p)
    xl = tmp_path / "pk.xlsx"
    xl.write_bytes(b"PK\x03\x04")
    with pytest.raises(ValueError, match="CSV"):
        read_prior_knowledge(xl)


def test_oracle_notebook_kat():
    """pyamares.md:380-415 on the oracle alone (the notebook's regenerated 5-voxel dataset)."""
    data, t, mhz = orc.notebook_dataset()
    init, lo, hi = orc.notebook_pk(mhz)
    fits = [orc.fit(x, t, init, lo, hi) for x in data]
    amp = np.array([f["params"][:, 0] for f in fits])
    np.testing.assert_allclose(amp[:, 0], [10, 20, 30, 40, 50], rtol=0.05)
    np.testing.assert_allclose(amp[:, 1], 5.0, rtol=0.1)
    lw = np.array([f["params"][:, 2] / np.pi for f in fits])
    assert np.all((lw >= 5.0) & (lw <= 40.0))
    assert fits[4]["snr"][0] > fits[0]["snr"][0]
    crlb = np.array([f["crlb"] for f in fits])
    assert not np.isnan(crlb).any() and np.all(crlb <= 20.0)
    assert all(f["params"][k, 4] == 0.0 for f in fits for k in range(2))  # g starts on its bound and stays


def test_abi_rejects_bad_arguments():
    """Invalid arguments return XM_ERR_INVALID_ARG before any HIP call (no GPU needed)."""
    from xmris_amd import _lib

    lib = _lib.load()
    init, lo, hi = (np.ascontiguousarray(a) for a in orc.notebook_pk(120.0))
    fixed = np.zeros((2, 5), np.int32)
    buf = np.zeros(1 << 16)  # stands in for every output (never written: the calls fail first)
    pp = lambda a: a.ctypes.data  # noqa: E731

    def fit(n_peaks=2, n=1024, ptr=pp(buf), lo_=lo, fixed_=fixed, max_iter=200):
        return lib.xm_amares_fit(ptr, n, 4, n, 1e-4, 0.0, n_peaks, pp(init), pp(lo_), pp(hi), pp(fixed_), max_iter,
                                 1e-10, 1e-10, ptr, ptr, ptr, ptr, ptr, None, ptr, 256, _lib.XM_C128, None)

    bad_lo = lo.copy()
    bad_lo[0, 2] = 1e9  # above its upper bound
    all_fixed = np.ones((2, 5), np.int32)
    for kw in [dict(n_peaks=0), dict(n_peaks=17), dict(n=5), dict(ptr=None), dict(lo_=bad_lo),
               dict(fixed_=all_fixed), dict(max_iter=0)]:
        assert fit(**kw) == _lib.XM_ERR_INVALID_ARG, kw
    assert lib.xm_amares_fit(pp(buf), 8, 1, 8, 1e-4, 0.0, 2, None, pp(lo), pp(hi), pp(fixed), 200, 1e-10, 1e-10,
                             *([pp(buf)] * 5), None, pp(buf), 256, _lib.XM_C128, None) == _lib.XM_ERR_INVALID_ARG
    assert lib.xm_amares_fit(pp(buf), 8, 1, 8, 1e-4, 0.0, 2, pp(init), pp(lo), pp(hi), pp(fixed), 200, 1e-10, 1e-10,
                             *([pp(buf)] * 5), None, pp(buf), 4, _lib.XM_C128, None) == _lib.XM_ERR_INVALID_ARG
    assert lib.xm_amares_fit(pp(buf), 8, 1, 8, 1e-4, 0.0, 2, pp(init), pp(lo), pp(hi), pp(fixed), 200, 1e-10, 1e-10,
                             *([pp(buf)] * 5), None, pp(buf), 256, 7, None) == _lib.XM_ERR_INVALID_ARG
    for args in [(pp(buf), 1, 0, 16, 1e-4, 0.0, pp(buf)), (pp(buf), 1, 17, 16, 1e-4, 0.0, pp(buf)),
                 (pp(buf), 1, 2, 0, 1e-4, 0.0, pp(buf)), (None, 1, 2, 16, 1e-4, 0.0, pp(buf)),
                 (pp(buf), 1, 2, 16, 1e-4, 0.0, None)]:
        assert lib.xm_amares_model(*args, None) == _lib.XM_ERR_INVALID_ARG, args
    assert b"amares" in lib.xm_last_error_string()


def test_package_exports():
    import xmris_amd as xm

    assert "fit_amares" in xm.__all__ and "simulate_fid" in xm.__all__
    assert callable(xm.fit_amares) and callable(xm.simulate_fid)
    assert hasattr(xm.XmrisAccessor, "fit_amares")


# ---- GPU ------------------------------------------------------------------------------------------------------------
def _check_against_oracle(vals, data2, t, mhz, init, lo, hi, fixed=None):
    """vals: output name -> [n_vox, K].  Every parameter of every voxel within 1e-3 of the oracle's sd for it; CRLB and
    SNR as the oracle defines them."""
    scale = PARAM_SCALE(mhz)
    for v in range(data2.shape[0]):
        o = orc.fit(data2[v], t, init, lo, hi, fixed)
        for c, name in enumerate(("amplitude", "chem_shift", "linewidth", "phase")):
            ref, sd = o["params"][:, c] * scale[c], o["sd"][:, c] * scale[c]
            assert np.all(np.abs(vals[name][v] - ref) <= 1e-3 * sd), (v, name, vals[name][v], ref, sd)
        np.testing.assert_allclose(vals["crlb"][v], o["crlb"], rtol=1e-3, err_msg=f"voxel {v}")
        np.testing.assert_allclose(vals["snr"][v], o["snr"], rtol=1e-6, err_msg=f"voxel {v}")


@pytest.mark.gpu
@pytest.mark.parametrize("method", ["leastsq", "least_squares"])
def test_notebook_kat_through_accessor(method):
    import xmris_amd as xm

    data, t, mhz = orc.notebook_dataset()
    da = xm.LabeledArray(data, ("voxel", "time"), {"voxel": np.arange(5), "time": (
        "time", t, {"units": "s", "long_name": "Time"})}, {"MHz": mhz, "sw": 10000.0})
    ds = da.xmr.fit_amares(prior_knowledge_file=PK, method=method, num_workers=1)
    for v in ["raw_data", "fit_data", "residuals", "amplitude", "chem_shift", "linewidth", "phase", "crlb", "snr"]:
        assert v in ds.data_vars
    assert ds["amplitude"].dims == ("voxel", "Metabolite") and ds["fit_data"].dims == ("voxel", "time")
    assert list(ds.coords["Metabolite"].values) == ["PCr", "ATP"]
    assert ds.coords["time"].attrs == {"units": "s", "long_name": "Time"}
    amp = ds["amplitude"].values
    np.testing.assert_allclose(amp[:, 0], [10, 20, 30, 40, 50], rtol=0.05)
    np.testing.assert_allclose(amp[:, 1], 5.0, rtol=0.1)
    lw = ds["linewidth"].values
    assert np.all((lw >= 5.0) & (lw <= 40.0))
    assert ds["snr"].values[4, 0] > ds["snr"].values[0, 0]
    crlb = ds["crlb"].values
    assert not np.isnan(crlb).any() and np.all(crlb <= 20.0)
    np.testing.assert_array_equal(ds["residuals"].values, ds["raw_data"].values - ds["fit_data"].values)
    assert abs(np.mean(ds["residuals"].values[-1])) < 1.0
    assert ds.attrs["fit_method"] == method and ds.attrs["prior_knowledge_file"] == PK
    assert ds.attrs["MHz"] == mhz and ds.attrs["amares_version"].startswith("xmris_amd")
    init, lo, hi = orc.notebook_pk(mhz)
    _check_against_oracle({v: ds[v].values for v in ds.data_vars}, data, t, mhz, init, lo, hi)
    # RSS of the kernel itself
    from xmris_amd import device as dev
    import torch

    raw = dev.amares_fit(torch.from_numpy(data).to("cuda"), 1, init, lo, hi, np.zeros((2, 5), bool), dt=1e-4)
    rss = raw.rss.cpu().numpy()
    for v in range(5):
        o = orc.fit(data[v], t, init, lo, hi)
        assert abs(rss[v] - o["rss"]) <= 1e-9 * o["rss"]
    assert (raw.status.cpu().numpy() == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["complex64", "complex128"])
def test_oracle_parity_at_scale(tmp_path, dtype):
    import xmris_amd as xm

    mhz, sw = 120.0, 10000.0
    data, _, t = orc.p31_workload(512, n=2048, sw=sw, mhz=mhz, seed=7)
    data = data.astype(dtype)
    cube = np.ascontiguousarray(data.reshape(16, 32, 2048).transpose(2, 0, 1))  # dims (time, x, y): time not last
    pk_file = tmp_path / "p31.csv"
    pk_file.write_text(orc.p31_pk_csv())
    da = xm.LabeledArray(cube, ("time", "x", "y"), {"time": t, "x": np.arange(16), "y": np.arange(32)}, {"MHz": mhz})
    ds = xm.fit_amares(da, pk_file)
    assert ds["amplitude"].dims == ("x", "y", "Metabolite") and ds["fit_data"].dims == ("time", "x", "y")
    assert ds["raw_data"].values.dtype == np.dtype(dtype) and ds["fit_data"].values.dtype == np.complex128
    np.testing.assert_array_equal(ds["residuals"].values, ds["raw_data"].values - ds["fit_data"].values)
    init, lo, hi = orc.p31_pk(mhz)
    x64 = data.astype(np.complex128)  # complex64 input is widened on load
    flat = {v: (np.asarray(a.values).reshape(512, -1) if a.dims[-1] == "Metabolite"
                else np.asarray(a.values).reshape(2048, 512).T) for v, a in ds.data_vars.items()}
    _check_against_oracle(flat, x64, t, mhz, init, lo, hi)
    # fit_data = the oracle's model at the returned parameters
    scale = PARAM_SCALE(mhz)
    got = np.stack([np.stack([flat[v][:, k] / scale[c] for c, v in
                              enumerate(("amplitude", "chem_shift", "linewidth", "phase"))] + [np.zeros(512)], axis=1)
                    for k in range(5)], axis=1)
    fit = flat["fit_data"]
    for v in range(0, 512, 37):
        ref = orc.model(got[v], t)
        assert np.abs(fit[v] - ref).max() <= 1e-12 * np.abs(ref).max()


@pytest.mark.gpu
def test_voigt_and_dead_time():
    import torch
    from xmris_amd import device as dev

    mhz, sw, dead = 120.0, 10000.0, 5e-4
    t = np.arange(2048) / sw + dead
    truth = np.array([[20.0, 30.0, 40.0, 0.2, 0.3], [8.0, -900.0, 70.0, -0.4, 0.3]])
    x = orc.model(truth, t)[None]
    init = truth.copy()
    init[:, 0] *= 0.8
    init[:, 1] += 5.0
    init[:, 2] *= 1.2
    init[:, 3] = 0.0
    init[:, 4] = 0.5
    lo = np.array([[0, -200, 10, -np.pi, 0], [0, -1100, 10, -np.pi, 0]], float)
    hi = np.array([[np.inf, 200, 300, np.pi, 1], [np.inf, -700, 300, np.pi, 1]], float)
    r = dev.amares_fit(torch.from_numpy(x).to("cuda"), 1, init, lo, hi, np.zeros((2, 5), bool), dt=1.0 / sw, t0=dead)
    got = r.params.cpu().numpy()[0]
    np.testing.assert_allclose(got, truth, rtol=1e-7, atol=1e-9)
    assert int(r.status.cpu()[0]) == 0
    ref = orc.model(got, t)
    assert np.abs(r.fit.cpu().numpy()[0] - ref).max() <= 1e-12 * np.abs(ref).max() * 10


@pytest.mark.gpu
def test_batch_independence_nan_voxel_and_fixed_phase(tmp_path):
    import xmris_amd as xm

    mhz = 120.0
    data, _, t = orc.p31_workload(24, n=1024, mhz=mhz, seed=3)
    pk_file = tmp_path / "p31.csv"
    pk_file.write_text(orc.p31_pk_csv())
    base = xm.fit_amares(xm.LabeledArray(data, ("v", "time"), {"time": t}, {"MHz": mhz}), pk_file)
    nan_row = data[0].copy()
    nan_row[100] = np.nan
    big = np.concatenate([data[:10], nan_row[None], data[10:]])
    ds = xm.fit_amares(xm.LabeledArray(big, ("v", "time"), {"time": t}, {"MHz": mhz}), pk_file)
    keep = np.r_[0:10, 11:25]
    for v in ds.data_vars:
        a = np.asarray(ds[v].values)
        assert np.array_equal(a[keep], np.asarray(base[v].values), equal_nan=True), v  # bitwise
        if v in ("raw_data", "residuals"):
            np.testing.assert_array_equal(a[10], big[10])
        else:
            assert np.all(a[10] == 0), v
    # a fixed phase (lo == hi) equals its bound exactly; the other voxels do not move when it is in the batch
    text = orc.p31_pk_csv().replace('phase,"(-180, 180)"', 'phase,"(12.5, 12.5)"', 1)
    fixed_file = tmp_path / "p31_fixed.csv"
    fixed_file.write_text(text)
    ds = xm.fit_amares(xm.LabeledArray(data, ("v", "time"), {"time": t}, {"MHz": mhz}), fixed_file)
    assert np.all(ds["phase"].values[:, 0] == np.rad2deg(12.5 * (np.pi / 180.0)))
    init, lo, hi = orc.p31_pk(mhz)
    lo[0, 3] = hi[0, 3] = np.deg2rad(12.5)
    init[0, 3] = lo[0, 3]
    o = orc.fit(data[5], t, init, lo, hi)
    np.testing.assert_allclose(ds["amplitude"].values[5], o["params"][:, 0], rtol=0, atol=1e-3 * o["sd"][:, 0].max())


@pytest.mark.gpu
def test_simulate_fid_matches_model_and_reference_contract():
    import xmris_amd as xm

    # 1H set (simufid.md:66-90)
    kw = dict(amplitudes=[1000.0, 150.0, 50.0], chemical_shifts=[4.7, 1.3, 0.9], reference_frequency=127.7,
              spectral_width=2000.0, n_points=2048, dampings=[15.0, 30.0, 30.0], phases=[0.0, 0.0, 0.0],
              lineshape_g=[0.0, 0.2, 0.2])
    fid = xm.simulate_fid(**kw)
    t = np.arange(2048) / 2000.0
    p = np.stack([kw["amplitudes"], np.array(kw["chemical_shifts"]) * 127.7, kw["dampings"], kw["phases"],
                  kw["lineshape_g"]], axis=1)
    ref = orc.model(p, t)
    assert np.abs(fid.values - ref).max() <= 1e-12 * np.abs(ref).max()
    assert fid.dims == ("time",) and fid.name == "FID Signal" and fid.values.dtype == np.complex128
    assert fid.coords["time"].attrs == {"units": "s", "long_name": "Time"}
    np.testing.assert_array_equal(fid.coords["time"].values, np.arange(2048) * (1 / 2000.0))
    assert fid.attrs == {"spectral_width": 2000.0, "dead_time": 0.0, "sim_amplitudes": [1000.0, 150.0, 50.0],
                         "sim_dampings": [15.0, 30.0, 30.0], "carrier_ppm": 0.0, "units": "a.u.",
                         "reference_frequency": 127.7, "sim_chemical_shifts_ppm": [4.7, 1.3, 0.9]}
    # 13C set with a carrier (simufid.md:136-159), dead time
    kw13 = dict(amplitudes=[200.0, 50.0, 1000.0, 80.0], chemical_shifts=[183.3, 176.6, 171.1, 161.0],
                reference_frequency=32.1, carrier_ppm=171.0, spectral_width=5000.0, n_points=2048,
                dampings=[10.0, 10.0, 12.0, 10.0], phases=[0.0, 0.0, 0.0, 0.0], lineshape_g=0.0, dead_time=2e-4)
    fid = xm.simulate_fid(**kw13)
    t = np.arange(2048) / 5000.0 + 2e-4
    p = np.stack([kw13["amplitudes"], (np.array(kw13["chemical_shifts"]) - 171.0) * 32.1, kw13["dampings"],
                  kw13["phases"], np.zeros(4)], axis=1)
    ref = orc.model(p, t)
    assert np.abs(fid.values - ref).max() <= 1e-12 * np.abs(ref).max()
    assert fid.attrs["carrier_ppm"] == 171.0 and fid.attrs["dead_time"] == 2e-4
    fid = xm.simulate_fid([1.0, 2.0], frequencies=[10.0, -20.0])
    assert fid.attrs["sim_frequencies_hz"] == [10.0, -20.0] and "reference_frequency" not in fid.attrs
    # errors
    with pytest.raises(ValueError, match="not both"):
        xm.simulate_fid([1.0], frequencies=[1.0], chemical_shifts=[1.0], reference_frequency=1.0)
    with pytest.raises(ValueError, match="reference_frequency"):
        xm.simulate_fid([1.0], chemical_shifts=[1.0])
    with pytest.raises(ValueError, match="must be provided"):
        xm.simulate_fid([1.0])
    with pytest.raises(ValueError, match="must match amplitudes"):
        xm.simulate_fid([1.0, 2.0], frequencies=[1.0])
    # noise: std = mean(|fid[:10]|) / target_snr in total, 1/sqrt(2) per channel
    kwn = dict(kw, n_points=1 << 16, target_snr=40.0)
    noisy, ideal = xm.simulate_fid(**kwn), xm.simulate_fid(**dict(kwn, target_snr=None))
    assert noisy.attrs["target_snr"] == 40.0
    noise = noisy.values - ideal.values
    want = np.mean(np.abs(ideal.values[:10])) / 40.0 / np.sqrt(2)
    for ch in (noise.real, noise.imag):
        assert abs(np.std(ch) / want - 1) < 0.03


def test_fit_amares_errors():
    """Validation happens before any device work (no GPU needed)."""
    import xmris_amd as xm

    data, t, mhz = orc.notebook_dataset()
    da = xm.LabeledArray(data, ("voxel", "time"), {"time": t}, {"MHz": mhz})
    with pytest.raises(ValueError, match=r"Dimension 'spectrum' missing in DataArray\."):
        da.xmr.fit_amares(PK, dim="spectrum")
    with pytest.raises(ValueError, match=r"mhz must be provided or present in da.attrs\['MHz'\]"):
        xm.LabeledArray(data, ("voxel", "time"), {"time": t}).xmr.fit_amares(PK)
    with pytest.raises(ValueError, match="method"):
        da.xmr.fit_amares(PK, method="nelder")
    with pytest.raises(ValueError, match="init_fid"):
        da.xmr.fit_amares(PK, init_fid=np.zeros(3))
