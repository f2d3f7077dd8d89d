"""k_align / xm_align_rows / .xmr.align_averages on the GPU against tests/_align_oracle.py.  The shapes are
orc.PARITY_CASES, whose margins, sign changes and route agreement are checked on the CPU in tests/test_align.py."""
import functools

import numpy as np
import pytest

import _align_oracle as orc
from test_align import ALIGN_TOL  # 16 x the 2.51 of tests/tool_align_tolerance.py

pytestmark = pytest.mark.gpu

EPS = orc.EPS
HALF32 = 2.0 ** -24  # one rounding of an fp32 value, relative
OUT = ("y", "shift", "phase", "quality", "status")


def _up(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _run(x, ref, dt, ms, L, t0=0.0, average_axis=1, **kw):
    from xmris_amd import device as dev

    r = dev.align_rows(_up(x), average_axis, -1, _up(ref.astype(x.dtype)), n_points=L, dt=dt, t0=t0, max_shift=ms, **kw)
    host = lambda t: None if t is None else t.cpu().numpy()  # noqa: E731
    return dict(y=host(r.y), mean=host(r.mean), shift=host(r.shift), phase=host(r.phase), quality=host(r.quality),
                status=host(r.status), n_averaged=host(r.n_averaged), kernel=dev.last_kernel())


def _same(a, b, keys=OUT):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in keys)


def _check(got, want, x, c64=False, what=""):
    """shift within ALIGN_TOL u_f, phase within ALIGN_TOL u_phi, quality within ALIGN_TOL u_q,
    |y - y_oracle| <= |x_t| (2 pi |tau_t| ALIGN_TOL u_f + ALIGN_TOL u_phi + 4 eps), complex64 plus one fp32 rounding."""
    uf = np.where(want["u_f"] > 0, want["u_f"], 1.0)
    df = np.abs(got["shift"] - want["shift"]) / uf
    dp = orc.phase_gap(got["phase"], want["phase"]) / want["u_phi"]
    dq = np.abs(got["quality"] - want["quality"]) / want["u_q"]
    tau = np.abs(np.arange(x.shape[-1]) * orc.DT)
    bound = np.abs(x) * (2 * np.pi * tau * ALIGN_TOL * want["u_f"][..., None] + ALIGN_TOL * want["u_phi"][..., None]
                         + 4 * EPS + (np.sqrt(2.0) * HALF32 if c64 else 0.0))
    dy = np.abs(got["y"] - want["y"])
    with np.errstate(invalid="ignore", divide="ignore"):
        worst_y = np.nanmax(np.where(bound > 0, dy / bound, 0.0))
    print(f"{what}: shift {df.max():.2f} units of u_f, phase {dp.max():.2f} of u_phi, quality {dq.max():.2f} of u_q "
          f"(bound {ALIGN_TOL}); y {worst_y:.3f} of its bound; {got['kernel']}")
    assert np.array_equal(got["status"], want["status"]), got["status"]
    assert np.all(df <= ALIGN_TOL) and np.all(dp <= ALIGN_TOL) and np.all(dq <= ALIGN_TOL), (what, df.max(), dp.max(), dq.max())
    assert np.all(dy <= bound), (what, worst_y)


@functools.lru_cache(maxsize=None)
def _case(name, dtype):
    x, r, dt, ms, L = orc.parity_case(name)
    x, r = x.astype(dtype), r.astype(dtype)
    return x, r, dt, ms, L, orc.align_batch(x.astype(np.complex128), r.astype(np.complex128), dt, 0.0, ms, L)


# ---- 1. parity ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["complex128", "complex64"])
@pytest.mark.parametrize("name", list(orc.PARITY_CASES))
def test_parity_with_the_oracle(name, dtype):
    x, r, dt, ms, L, want = _case(name, dtype)
    got = _run(x, r, dt, ms, L)
    assert got["y"].dtype == np.dtype(dtype) and "k_align<each" in got["kernel"]
    _check(got, want, x.astype(np.complex128), c64=dtype == "complex64", what=f"{name} {dtype}")


def test_parity_with_a_time_offset():
    x, r, _, _ = orc.make_data(2, 3, 1, 100, seed=3, max_shift=15.0)
    t0 = 0.0123
    want = orc.align_batch(x, r, orc.DT, t0, 15.0)
    got = _run(x, r, orc.DT, 15.0, 100, t0=t0)
    uf = np.abs(got["shift"] - want["shift"]) / want["u_f"]
    print("t0 = 0.0123: shift", uf.max(), "units")
    assert np.all(uf <= ALIGN_TOL) and np.all(orc.phase_gap(got["phase"], want["phase"]) <= ALIGN_TOL * want["u_phi"])


# ---- 2. bitwise properties ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["complex64", "complex128"])
def test_a_transient_does_not_depend_on_its_batch(dtype):
    import torch

    x7, r, _, _ = orc.make_data(1, 7, 1, 65, seed=41, max_shift=30.0)
    x7 = x7.astype(dtype)
    big = np.tile(x7, (1, 715, 1, 1))[:, :5003]
    work = torch.zeros(256, dtype=torch.uint8, device="cuda")
    a, b = _run(x7, r, orc.DT, 30.0, 65, workspace=work), _run(big, r, orc.DT, 30.0, 65, workspace=work)
    assert int(work.sum().item()) == 0
    idx = np.arange(5003) % 7
    for k in OUT:
        assert np.array_equal(b[k], a[k][:, idx]), k


def test_reference_forms_give_the_same_bits():
    x, r, _, _ = orc.make_data(1, 5, 3, 40, seed=42, max_shift=30.0)
    x[:, :, 1:] = x[:, :, :1]  # the same samples in every voxel
    r[:, 1:] = r[:, :1]
    per = _run(x, r, orc.DT, 30.0, 32)
    shared = _run(x, r[0, 0], orc.DT, 30.0, 32)
    longer = np.concatenate([r, 7.0 + 0 * r], axis=-1)  # N_r > N, and other samples beyond L
    other = r.copy()
    other[..., 32:] = -3.0
    assert _same(per, shared) and _same(per, _run(x, longer, orc.DT, 30.0, 32)) and _same(per, _run(x, other, orc.DT, 30.0, 32))
    assert np.array_equal(per["shift"][:, :, 0], per["shift"][:, :, 2])


# ---- 3. averaging form --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [65, 2300])  # one pass, and two passes of 2048 points
def test_average_is_the_ordered_sum_of_the_aligned_transients(n):
    x, r, _, _ = orc.make_data(2, 6, 3, n, seed=43, max_shift=30.0, snr=(0.3, 10.0))
    L = min(n, 128)
    each = _run(x, r, orc.DT, 30.0, L)
    q = float(np.sort(each["quality"].ravel())[9])
    for mq in (0.0, q, 2.0):
        avg = _run(x, r, orc.DT, 30.0, L, average=True, min_quality=mq)
        assert "k_align<average" in avg["kernel"] and _same(avg, each)
        mean, cnt = orc.average(each["y"], each["status"], each["quality"], mq)
        assert np.array_equal(avg["n_averaged"], cnt) and np.array_equal(avg["mean"], mean)
        only = _run(x, r, orc.DT, 30.0, L, average=True, min_quality=mq, want_y=False)  # y = NULL
        assert only["y"] is None and np.array_equal(only["mean"], mean)
    assert not avg["mean"].any() and not avg["n_averaged"].any()  # min_quality 2: nobody
    want = orc.align_batch(x, r, orc.DT, 0.0, 30.0, L)
    assert np.array_equal(want["quality"] >= q, each["quality"] >= q)  # the oracle leaves the same transients out
    a32 = _run(x.astype(np.complex64), r, orc.DT, 30.0, L, average=True)
    m32, _ = orc.average(a32["y"].astype(np.complex128), a32["status"], a32["quality"])
    assert np.abs(a32["mean"] - m32).max() <= 2 * HALF32 * np.abs(m32).max()


# ---- 4. status ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("average", [False, True])
def test_status_cases_leave_their_neighbours_alone(average):
    n = 64
    x, r, _, _ = orc.make_data(1, 9, 1, n, seed=44, max_shift=10.0)
    delta, _ = orc.grid(n, orc.DT, 1.0)
    ms = 3.3 * delta
    bad = x.copy()
    bad[0, 2] = x[0, 2] * np.exp(2j * np.pi * 9 * delta * np.arange(n) * orc.DT)  # the maximum lies outside the window
    bad[0, 4, 0, 7] = np.nan
    bad[0, 6, 0, 0] = np.inf
    bad[0, 7] = 0.0
    got = _run(bad, r, orc.DT, ms, n, average=average)
    want = orc.align_batch(bad, r, orc.DT, 0.0, ms)
    assert list(got["status"].ravel()) == list(want["status"].ravel())
    assert got["status"].ravel()[2] == 1 and list(got["status"].ravel()[[4, 6, 7]]) == [2, 2, 3]
    keep = [0, 1, 3, 5, 8]
    clean = _run(x[:, keep], r, orc.DT, ms, n)
    for k in OUT:
        assert np.array_equal(got[k][:, keep], clean[k]), k
    assert abs(got["shift"][0, 2, 0]) == ms
    assert not got["y"][0, [4, 6]].any() and np.isnan(got["shift"][0, [4, 6]]).all() and np.isnan(got["quality"][0, [4, 6]]).all()
    assert np.array_equal(got["y"][0, 7], bad[0, 7]) and got["quality"][0, 7, 0] == 0.0 and got["phase"][0, 7, 0] == 0.0
    if average:
        mean, cnt = orc.average(got["y"], got["status"], got["quality"])
        assert cnt[0, 0] == 7 and np.array_equal(got["n_averaged"], cnt) and np.array_equal(got["mean"], mean)


def test_c_abi_refusals_leave_outputs_and_workspace_alone():
    import torch
    from xmris_amd import _lib

    lib = _lib.load()
    n = 8
    x = torch.ones((2, n), dtype=torch.complex64, device="cuda")
    y = torch.full((2, n), 7.0, dtype=torch.complex64, device="cuda")
    f = [torch.full((2,), 7.0, dtype=torch.float64, device="cuda") for _ in range(3)]
    s = torch.full((2,), 7, dtype=torch.int32, device="cuda")
    ws = torch.full((256,), 171, dtype=torch.uint8, device="cuda")
    ok = dict(x=x.data_ptr(), r=x.data_ptr(), rs=0, y=y.data_ptr(), L=n, dt=1e-3, ms=20.0, dtype=0, ws=ws.data_ptr())
    for change in (dict(x=None), dict(r=None), dict(y=None), dict(ws=None), dict(L=0), dict(L=n + 1), dict(dt=0.0),
                   dict(ms=-1.0), dict(ms=1e6), dict(dtype=5), dict(rs=3)):
        a = dict(ok, **change)
        rc = lib.xm_align_rows(a["x"], a["r"], a["rs"], a["y"], None, f[0].data_ptr(), f[1].data_ptr(), f[2].data_ptr(),
                               s.data_ptr(), None, 1, 2, 1, n, n, a["L"], a["dt"], 0.0, a["ms"], 0.0, a["dtype"], a["ws"], None)
        assert rc == _lib.XM_ERR_INVALID_ARG, change
    torch.cuda.synchronize()
    assert bool((y == 7).all()) and all(bool((v == 7).all()) for v in f) and bool((s == 7).all()) and bool((ws == 171).all())


# ---- 5. through the accessor ----------------------------------------------------------------------------------------------
def _labeled(x, dims, **attrs):
    from xmris_amd import LabeledArray

    coords = {d: np.arange(x.shape[i], dtype=float) for i, d in enumerate(dims) if d != "time"}
    coords["time"] = ("time", np.arange(x.shape[dims.index("time")]) * orc.DT, {"units": "s", "long_name": "Time"})
    return LabeledArray(x, dims, coords, dict(attrs))


def test_accessor_layouts_metadata_and_passes():
    x, r, _, _ = orc.make_data(6, 5, 1, 48, seed=61, max_shift=25.0)
    x4 = x.reshape(2, 3, 5, 48)  # (x, y, average, time)
    da = _labeled(x4, ("x", "y", "average", "time"), MHz=120.0)
    before = da.values.copy()
    ds = da.xmr.align_averages(max_shift=25.0, return_shifts=True)
    out = da.xmr.align_averages(max_shift=25.0)
    assert out.dims == da.dims and out.is_device_resident and set(out.coords) == set(da.coords)
    assert out.attrs == {"MHz": 120.0, "align_dim": "average", "align_reference": "mean", "align_max_shift": 25.0}
    assert da.attrs == {"MHz": 120.0} and np.array_equal(da.values, before)
    assert set(ds.data_vars) == {"aligned", "shift", "phase", "quality", "status"} and ds.attrs == out.attrs
    assert ds["shift"].dims == ("x", "y", "average") == ds["status"].dims
    assert np.array_equal(ds["aligned"].values, out.values)
    want = orc.align_batch(x, x.mean(axis=1), orc.DT, 0.0, 25.0)
    assert np.all(np.abs(ds["shift"].values.reshape(6, 5, 1) - want["shift"]) <= ALIGN_TOL * want["u_f"] + 64 * EPS * 25.0)
    assert np.all(orc.phase_gap(np.deg2rad(ds["phase"].values.reshape(6, 5, 1)), want["phase"]) <= ALIGN_TOL * want["u_phi"] + 64 * EPS)
    # (average, voxel, time): addressed where it lies, the same numbers
    xt = np.ascontiguousarray(np.moveaxis(x[:, :, 0], 1, 0))
    d2 = _labeled(xt, ("average", "x", "time")).xmr.align_averages(max_shift=25.0, return_shifts=True)
    assert np.array_equal(np.moveaxis(d2["aligned"].values, 0, 1), out.values.reshape(6, 5, 48))
    assert np.array_equal(d2["shift"].values.T, ds["shift"].values.reshape(6, 5))
    # time not last: one copy, the same numbers, time where it was
    d3 = _labeled(np.ascontiguousarray(np.moveaxis(xt, 2, 1)), ("average", "time", "x")).xmr.align_averages(max_shift=25.0)
    assert d3.dims == ("average", "time", "x") and np.array_equal(np.moveaxis(d3.values, 1, 2), d2["aligned"].values)
    # passes = 2 is two explicit calls; average drops the dim
    two = da.xmr.align_averages(max_shift=25.0, passes=2, return_shifts=True)
    # (the mean taken on the device, as passes=2 takes it: numpy's mean sums in another order, and the test is bitwise)
    ref2 = _labeled(np.asarray(out.data.mean(dim=2).cpu().numpy()), ("x", "y", "time"))
    again = da.xmr.align_averages(max_shift=25.0, reference=ref2, return_shifts=True)
    for k in ("aligned", "shift", "phase", "quality", "status"):
        assert np.array_equal(two[k].values, again[k].values), k
    assert again.attrs["align_reference"] == "array"
    av = da.xmr.align_averages(max_shift=25.0, average=True, return_shifts=True)
    assert av["averaged"].dims == ("x", "y", "time") and av["n_averaged"].dims == ("x", "y") and np.all(av["n_averaged"].values == 5)
    mean, _ = orc.average(out.values.reshape(6, 5, 1, 48), ds["status"].values.reshape(6, 5, 1), ds["quality"].values.reshape(6, 5, 1))
    assert np.array_equal(av["averaged"].values.reshape(6, 1, 48), mean)
    first = da.xmr.align_averages(max_shift=25.0, reference="first", return_shifts=True)
    assert np.all(np.abs(first["shift"].values[:, :, 0]) <= 1e-9) and np.all(first["quality"].values[:, :, 0] > 1 - 1e-12)


def test_plain_input_gives_what_combine_coils_gives():
    x, _, _, _ = orc.make_data(2, 4, 1, 32, seed=62, max_shift=25.0)
    da = _labeled(x[:, :, 0], ("x", "average", "time"))
    from xmris_amd import LabeledArray
    from xmris_amd.fitting.dataset import LabeledDataset

    assert isinstance(da.xmr.align_averages(max_shift=25.0), LabeledArray)
    assert isinstance(da.xmr.align_averages(max_shift=25.0, return_shifts=True), LabeledDataset)


class _FakeDataset:
    """What tests/_fake_xarray.py lacks: the container LabeledDataset.to_xarray() builds."""

    def __init__(self, data_vars, attrs=None):
        self.data_vars, self.attrs = dict(data_vars), dict(attrs or {})

    def __getitem__(self, k):
        return self.data_vars[k]


def test_fake_xarray_in_gives_xarray_out(monkeypatch):
    import _fake_xarray

    from xmris_amd import accessor, labeled

    xr = _fake_xarray.install(monkeypatch)
    monkeypatch.setattr(xr, "Dataset", _FakeDataset, raising=False)
    accessor.register_xarray_accessor(force=True)
    x, _, _, _ = orc.make_data(3, 4, 1, 40, seed=63, max_shift=25.0)
    x = x[:, :, 0]
    t = np.arange(40) * orc.DT
    coords = {"x": [10, 11, 12], "time": xr.Variable("time", t, {"units": "s"})}
    da = xr.DataArray(x, dims=("x", "average", "time"), coords=coords, attrs={"MHz": 120.0}, name="fid")
    la = _labeled(x, ("x", "average", "time"), MHz=120.0)
    assert labeled.is_xarray(da) and isinstance(da.xmr, accessor.XmrisAccessor)
    attrs = {"MHz": 120.0, "align_dim": "average", "align_reference": "mean", "align_max_shift": 25.0}

    got, want = da.xmr.align_averages(max_shift=25.0), la.xmr.align_averages(max_shift=25.0)
    assert isinstance(got, xr.DataArray) and isinstance(got.data, np.ndarray)
    assert got.dims == ("x", "average", "time") and got.attrs == attrs and got.name == "fid"
    assert set(got.coords) == {"x", "time"} and got.coords["time"].attrs == {"units": "s"}
    assert np.array_equal(got.coords["time"].values, t) and np.array_equal(got.coords["x"].values, [10, 11, 12])
    assert np.array_equal(got.values, want.values)

    ds, wds = da.xmr.align_averages(max_shift=25.0, return_shifts=True), la.xmr.align_averages(max_shift=25.0, return_shifts=True)
    assert isinstance(ds, _FakeDataset) and set(ds.data_vars) == {"aligned", "shift", "phase", "quality", "status"}
    assert ds.attrs == attrs
    for k in ds.data_vars:
        assert isinstance(ds[k], xr.DataArray) and ds[k].dims == wds[k].dims, k
        assert np.array_equal(ds[k].values, wds[k].values), k
    assert np.array_equal(ds["shift"].coords["x"].values, [10, 11, 12])

    av, wav = (o.xmr.align_averages(max_shift=25.0, average=True, return_shifts=True) for o in (da, la))
    assert isinstance(av, _FakeDataset) and set(av.data_vars) == {"averaged", "shift", "phase", "quality", "status", "n_averaged"}
    assert av["averaged"].dims == ("x", "time") and av["n_averaged"].dims == ("x",) and av["averaged"].attrs == attrs
    for k in av.data_vars:
        assert np.array_equal(av[k].values, wav[k].values), k
    one = da.xmr.align_averages(max_shift=25.0, average=True)
    assert isinstance(one, xr.DataArray) and one.dims == ("x", "time") and np.array_equal(one.values, wav["averaged"].values)


# ---- 6. the caps: 128 KiB of z in the LDS, the opt-in beyond 64 KiB, fewer running sums per pass -------------------------
def test_the_largest_fit_in_both_forms():
    n, L, G = 8192 + 300, 8192, 512
    ms = orc.shift_for(G, L)
    x, r, _, _ = orc.make_data(1, 3, 2, n, seed=64, max_shift=ms)
    want = orc.align_batch(x, r, orc.DT, 0.0, ms, L)
    assert np.all(want["margin"] >= 0.2) and np.all(want["one_sign_change"]) and np.all(want["status"] == 0)
    each = _run(x, r, orc.DT, ms, L)
    assert "k_align<each, 8192, 512>" in each["kernel"]
    _check(each, want, x, what="L 8192, G 512")
    avg = _run(x, r, orc.DT, ms, L, average=True)
    mean, cnt = orc.average(each["y"], each["status"], each["quality"])
    assert _same(avg, each) and np.array_equal(avg["n_averaged"], cnt) and np.array_equal(avg["mean"], mean)
