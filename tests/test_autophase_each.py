"""`autophase_each` on the CPU: metadata, errors and the host route against ``oracle.autophase`` of every row alone.
The device kernels are replaced by the numpy test double, `phase_apply_rows` by a numpy stand-in of this file's."""
import numpy as np
import pytest

import _each_rows

SEEDS = range(7000, 7006)
N = 512


def _phase_apply_rows(x, axis, coords, p0, p1, pivot, skip=None, out=None):
    """phasing.py:56-73 row by row (numpy; the product's kernel is tested in test_gpu_autophase_each.py)."""
    import xmris_oracle as orc

    xm = np.moveaxis(np.asarray(x), axis, -1)
    res = np.array(xm)
    p0, p1, pivot = (np.broadcast_to(np.asarray(v, dtype=np.float64), xm.shape[:-1]) for v in (p0, p1, pivot))
    for idx in np.ndindex(xm.shape[:-1]):
        if skip is not None and np.asarray(skip)[idx]:
            continue
        res[idx] = xm[idx] * np.exp(1j * orc.phase_array(np.asarray(coords), p0[idx], p1[idx], pivot[idx]))
    return np.moveaxis(res, -1, axis)


@pytest.fixture
def host(monkeypatch, oracle):
    import _numpy_device

    import xmris_amd
    from xmris_amd import device

    _numpy_device.install(monkeypatch)
    monkeypatch.setattr(device, "phase_apply_rows", _phase_apply_rows)
    return xmris_amd


@pytest.fixture(scope="module")
def rows():
    return _each_rows.make_rows(N, SEEDS)


def _labeled(host, values, freq, dims=("voxel", "frequency"), attrs=None, name=None):
    return host.LabeledArray(values, dims, {"frequency": np.asarray(freq)}, attrs or {}, name)


def test_errors_match_autophase(host):
    a = host.LabeledArray(np.zeros(4, complex), ("x",), {"x": np.arange(4)})
    with pytest.raises(ValueError) as e:
        a.xmr.autophase_each()
    msg = str(e.value)
    assert "Method 'autophase_each'" in msg and "missing dimension" in msg and "['x']" in msg
    s = host.LabeledArray(np.ones((2, 8), complex), ("v", "frequency"), {"frequency": np.arange(8.0)})
    with pytest.raises(ValueError, match="Method must be 'acme', 'peak_minima', or 'positivity'"):
        s.xmr.autophase_each(method="nope")
    with pytest.raises(ValueError, match="engine='device' needs method='acme'"):
        s.xmr.autophase_each(method="positivity", engine="device")
    with pytest.raises(ValueError, match="engine='device' needs"):
        s.xmr.autophase_each(lb=2.0, engine="device")
    with pytest.raises(ValueError, match="engine must be"):
        s.xmr.autophase_each(engine="gpu")
    with pytest.raises(NotImplementedError, match="is not yet implemented"):
        s.xmr.autophase(mode="all")
    b = host.LabeledArray(np.ones((2, 8), complex), ("v", "frequency"))  # no coordinate, as autophase
    with pytest.raises(KeyError):
        b.xmr.autophase_each(engine="host")


def test_public_surface(host):
    import inspect

    import xmris_amd.processing as proc

    assert host.autophase_each is proc.autophase_each and "autophase_each" in host.__all__ and "autophase_each" in proc.__all__
    acc = {k: v.default for k, v in inspect.signature(host.XmrisAccessor.autophase_each).parameters.items() if k != "self"}
    assert (acc["dim"], acc["method"], acc["peak_width"], acc["lb"], acc["temp_time_dim"]) == \
        ("frequency", "acme", 100, 0.0, "time")
    fn = {k: v.default for k, v in inspect.signature(host.autophase_each).parameters.items()}
    assert fn["peak_width"] == 0.5 and fn["engine"] == "auto" and fn["target_coord"] is None and fn["p0_only"] is False
    assert "autophase_each" in (host.autophase.__doc__ or "")


def test_host_route_acme_equals_the_oracle_row_by_row(host, oracle, rows):
    x, freq = rows
    a = _labeled(host, x, freq, attrs={"seq": "press"}, name="spec")
    before = x.copy()
    r = a.xmr.autophase_each(engine="host")
    np.testing.assert_array_equal(a.values, before)  # the input is never mutated
    assert r.dims == a.dims and r.name is None and r.attrs["seq"] == "press" and r.attrs["phase_pivot_coord"] == "frequency"
    np.testing.assert_array_equal(r.coords["frequency"].values, freq)
    assert set(r.attrs) == {"seq", "phase_p0", "phase_p1", "phase_pivot", "phase_pivot_coord"}
    for k in ("phase_p0", "phase_p1", "phase_pivot"):
        assert r.attrs[k].shape == (len(SEEDS),) and r.attrs[k].dtype == np.float64
    for i, seed in enumerate(SEEDS):
        o = _each_rows.oracle_row(oracle, x[i], freq, key=(N, seed), peak_width=100)
        got = (r.attrs["phase_p0"][i], r.attrs["phase_p1"][i], r.attrs["phase_pivot"][i])
        want = (o.attrs["phase_p0"], o.attrs["phase_p1"], o.attrs["phase_pivot"])
        print(f"seed {seed}: got {got} oracle {want}")
        assert got == want, (seed, got, want)  # bit for bit
        np.testing.assert_allclose(r.values[i], o.values, rtol=1e-12, atol=1e-12)


def test_host_route_positivity(host, oracle, rows):
    x, freq = rows
    r = _labeled(host, x, freq).xmr.autophase_each(method="positivity", peak_width=50, engine="auto")
    for i, seed in enumerate(SEEDS):
        o = _each_rows.oracle_row(oracle, x[i], freq, key=(N, seed), method="positivity", peak_width=50)
        d0, d1 = r.attrs["phase_p0"][i] - o.attrs["phase_p0"], r.attrs["phase_p1"][i] - o.attrs["phase_p1"]
        print(f"seed {seed}: dp0 {d0:.3e} dp1 {d1:.3e} degrees")
        assert abs(d0) < 1e-2 and abs(d1) < 1e-2
        assert r.attrs["phase_pivot"][i] == o.attrs["phase_pivot"]
        np.testing.assert_allclose(r.values[i], o.values, rtol=0, atol=1e-2 * np.abs(o.values).max())


def test_shapes_and_attrs(host, oracle, rows):
    x, freq = rows
    cube = np.ascontiguousarray(np.moveaxis(x.reshape(2, 3, N), -1, 1))  # [2, N, 3]: `dim` in the middle
    a = host.LabeledArray(cube, ("y", "frequency", "x"), {"frequency": freq, "x": np.arange(3)})
    r = a.xmr.autophase_each(engine="host")
    assert r.dims == a.dims and r.shape == cube.shape
    for k in ("phase_p0", "phase_p1", "phase_pivot"):
        assert r.attrs[k].shape == (2, 3)
    for (iy, ix), seed in zip(np.ndindex(2, 3), SEEDS):
        o = _each_rows.oracle_row(oracle, x[3 * iy + ix], freq, key=(N, seed), peak_width=100)
        assert (r.attrs["phase_p0"][iy, ix], r.attrs["phase_p1"][iy, ix], r.attrs["phase_pivot"][iy, ix]) == \
            (o.attrs["phase_p0"], o.attrs["phase_p1"], o.attrs["phase_pivot"])
        np.testing.assert_allclose(r.values[iy, :, ix], o.values, rtol=1e-12, atol=1e-12)
    # one spectrum: 0-d arrays
    one = host.LabeledArray(x[0], ("frequency",), {"frequency": freq}).xmr.autophase_each(engine="host")
    o = _each_rows.oracle_row(oracle, x[0], freq, key=(N, SEEDS[0]), peak_width=100)
    assert one.attrs["phase_p0"].shape == () and float(one.attrs["phase_p0"]) == o.attrs["phase_p0"]
    assert float(one.attrs["phase_p1"]) == o.attrs["phase_p1"] and float(one.attrs["phase_pivot"]) == o.attrs["phase_pivot"]
    np.testing.assert_allclose(one.values, o.values, rtol=1e-12, atol=1e-12)


def test_p0_only_and_target_coord(host, oracle, rows):
    x, freq = rows
    a = _labeled(host, x[:3], freq)
    r = a.xmr.autophase_each(p0_only=True, engine="host")
    assert np.all(r.attrs["phase_p1"] == 0.0)
    tc = float(freq[200]) + 0.3 * float(freq[1] - freq[0])
    r = a.xmr.autophase_each(target_coord=tc, engine="host")
    assert np.all(r.attrs["phase_pivot"] == tc)
    # row by row this is the product's own `autophase` of that spectrum alone (an off-peak pivot is outside the cases
    # in which the host engine is recorded bit-equal to scipy, so the oracle is not the yardstick here)
    for i in range(3):
        one = host.LabeledArray(x[i], ("frequency",), {"frequency": freq}).xmr.autophase(target_coord=tc)
        assert (r.attrs["phase_p0"][i], r.attrs["phase_p1"][i]) == (one.attrs["phase_p0"], one.attrs["phase_p1"])
        np.testing.assert_allclose(r.values[i], one.values, rtol=1e-12, atol=1e-12)


def test_line_broadened_search(host, oracle, rows):
    """lb > 0: the to_fid -> apodize_exp -> to_spectrum detour for all rows at once (phasing.py:250-253)."""
    x, freq = rows
    r = _labeled(host, x[:2], freq).xmr.autophase_each(lb=2.0, engine="auto")
    for i in range(2):
        o = _each_rows.oracle_row(oracle, x[i], freq, key=(N, SEEDS[i]), peak_width=100, lb=2.0)
        # the tolerance test_abi_and_host.py uses for autophase's own lb detour
        assert abs(r.attrs["phase_p0"][i] - o.attrs["phase_p0"]) < 1e-6 and abs(r.attrs["phase_p1"][i] - o.attrs["phase_p1"]) < 1e-6
        assert r.attrs["phase_pivot"][i] == o.attrs["phase_pivot"]
        np.testing.assert_allclose(r.values[i], o.values, rtol=0, atol=1e-6 * np.abs(o.values).max())


def test_degenerate_rows_pass_through(host, rows):
    x, freq = rows
    y = x[:4].copy()
    y[1] = 0.0
    y[3, 17] = complex(np.nan, 1.0)
    r = _labeled(host, y, freq).xmr.autophase_each(engine="host")
    for i in (1, 3):
        assert np.isnan(r.attrs["phase_p0"][i]) and np.isnan(r.attrs["phase_p1"][i]) and np.isnan(r.attrs["phase_pivot"][i])
        assert np.array_equal(r.values[i], y[i], equal_nan=True)
    for i in (0, 2):
        assert np.isfinite(r.attrs["phase_p0"][i]) and np.isfinite(r.attrs["phase_pivot"][i])
        assert not np.array_equal(r.values[i], y[i])


def test_pivot_coord_warning(host, rows):
    x, freq = rows
    a = host.LabeledArray(x[:1], ("v", "chemical_shift"), {"chemical_shift": freq / 100.0}, {"phase_pivot_coord": "frequency"})
    with pytest.warns(UserWarning, match="previous phase operations"):
        a.xmr.autophase_each(dim="chemical_shift", engine="host")
