"""remove_lipids / lipid_basis without a GPU: the oracle pinned against itself (two routes to the basis, a dense route
to the result), the definition's properties, the host layer's metadata logic on the numpy double, and the C ABI's
refusals.  GPU parity of k_lipid_project: tests/test_gpu_lipids.py."""
import os
import re

import numpy as np
import pytest

import _lipids_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# profiles/lipids/tolerance.txt (tests/tool_lipids_tolerance.py), the largest over all parity cases, of the input row's
# largest magnitude
A_MEASURED = 1.685e-12  # (a) factorised route vs the dense solve at full rank (cond(I + beta M M^H) = 1 + 1 / level^2 = 1e4)
B_MEASURED = 2.872e-15  # (b) factorised route vs itself with both sums reversed
C_MEASURED = 1.202e-12  # (c) projector of the eigen route vs the SVD route
PHANTOM_UNTREATED = 9.0001
PHANTOM_ERROR = 0.4020  # level 0.01, rank None / 16 / 32 alike


def test_quoted_figures_are_the_tools():
    txt = open(os.path.join(ROOT, "profiles", "lipids", "tolerance.txt")).read()
    got = {k: float(v) for k, v in re.findall(r"^\s+\((a|b|c)\) ([0-9.e+-]+)", txt, flags=re.M)}
    assert got == {"a": A_MEASURED, "b": B_MEASURED, "c": C_MEASURED}
    assert float(re.search(r"untreated ([0-9.]+)", txt).group(1)) == PHANTOM_UNTREATED
    assert [float(v) for v in re.findall(r"error ([0-9.]+)$", txt, flags=re.M)] == [PHANTOM_ERROR] * 3


def test_case_lists_are_the_issues():
    assert orc.ROWS == (1, 15, 16, 17, 33) and orc.POINTS == (2, 6, 64, 250, 257, 1026)
    assert orc.RANKS == (1, 2, 7, 8, 9, 33, 64)
    assert all(r <= T for _, T, r in orc.CASES) and len(orc.CASES) == 5 * (2 + 2 + 7 + 7 + 7 + 7)


@pytest.mark.parametrize("T", orc.POINTS)
def test_oracle_routes_agree(T):
    """(a) - (c) on the cases of 33 rows (every T and rank) within 4 x the recorded figures."""
    for n, T_, r in orc.CASES:
        if n != 33 or T_ != T:
            continue
        c = orc.make_case(n, T, r)
        be, bs = orc.basis(c["L"], c["level"], r, "eig"), orc.basis(c["L"], c["level"], r, "svd")
        out = orc.apply(c["y"], be["U"], be["w"])
        assert orc.rel_err(out, orc.dense(c["y"], c["L"], c["level"]), c["y"]) <= 4 * A_MEASURED, (T, r)
        assert orc.rel_err(out, orc.apply(c["y"], be["U"], be["w"], reverse=True), c["y"]) <= 4 * B_MEASURED, (T, r)
        assert np.abs(orc.projector(be["U"], be["w"]) - orc.projector(bs["U"], bs["w"])).max() <= 4 * C_MEASURED, (T, r)
        np.testing.assert_allclose(be["s"], bs["s"], rtol=0, atol=1e-12 * be["s"][0])


@pytest.mark.parametrize("rank", [None, 16, 32])
def test_phantom_error(rank):
    ph = orc.phantom()
    before = orc.phantom_error(ph["data"], ph)
    out, _ = orc.remove(ph["data"], ph["scalp"], 0.01, rank)
    after = orc.phantom_error(out, ph)
    assert abs(before - PHANTOM_UNTREATED) < 1e-3
    assert after <= 1.5 * PHANTOM_ERROR and after < before


def test_scale_invariance():
    ph = orc.phantom()
    a, ba = orc.remove(ph["data"], ph["scalp"], 0.01, 16)
    b, bb = orc.remove(1024.0 * ph["data"], ph["scalp"], 0.01, 16)
    np.testing.assert_allclose(bb["w"], ba["w"], rtol=1e-9)
    assert np.abs(b / 1024.0 - a).max() <= 1e-11 * np.abs(ph["data"]).max()
    assert bb["beta"] == pytest.approx(ba["beta"] / 1024.0 ** 2, rel=1e-12)


def test_a_large_level_removes_nothing_and_a_small_one_projects():
    """w_k <= 1 / (1 + level^2): level -> infinity removes nothing beyond rounding.  level -> 0 is the w = 1 limit, the
    orthogonal projection off the subspace, which is idempotent."""
    c = orc.make_case(17, 64, 8)
    big = orc.basis(c["L"], 1e9, 8)
    assert big["w"].max() <= 1e-18
    assert orc.rel_err(orc.apply(c["y"], big["U"], big["w"]), c["y"], c["y"]) <= 1e-15
    small = orc.basis(c["L"], 1e-9, 8)
    assert small["w"].min() >= 1.0 - 1e-11
    once = orc.apply(c["y"], small["U"], small["w"])
    twice = orc.apply(once, small["U"], small["w"])
    assert orc.rel_err(once, twice, c["y"]) <= 1e-10
    assert np.abs(small["U"].conj().T @ once.T).max() <= 1e-10 * np.abs(c["y"]).max() * 8


def test_rank_rule_and_dropped_weight():
    from xmris_amd.processing import lipids

    s = np.array([3.0, 1.0, 0.5, 3e-2, 3e-5, 2e-5, 1e-6, 0.0])
    vec = np.eye(16, 8, dtype=np.complex128)
    beta, w = lipids.lipid_weights(s, 0.01)
    assert beta == pytest.approx(1.0 / 0.03 ** 2) and w[3] == pytest.approx(0.5)
    np.testing.assert_allclose(w, orc.weights(s, 0.01)[1], rtol=1e-15)
    b = lipids.basis_from_subspace(s, vec, 0.01, None, n_rows=8)
    keep = int(np.count_nonzero(w >= 2.0 ** -20))
    assert keep == 5 and b.rank == keep == orc.pick_rank(w)[0]
    assert b.dropped_weight == w[5] and b.weights.tolist() == w[:5].tolist() and b.n_rows == 8 and b.n_time == 16
    b3 = lipids.basis_from_subspace(s, vec, 0.01, 3)
    assert b3.rank == 3 and b3.dropped_weight == w[3] and b3.vectors.shape == (16, 3)
    b8 = lipids.basis_from_subspace(s, vec, 0.01, 8)
    assert b8.rank == 8 and b8.dropped_weight == 0.0
    many = lipids.basis_from_subspace(np.ones(100), np.eye(128, 100, dtype=np.complex128), 0.01, None)
    assert many.rank == 64 and many.dropped_weight == pytest.approx(1.0 / (1.0 + 1e-4))
    tiny = lipids.basis_from_subspace(s, vec, 1e6, None)  # no weight reaches 2^-20: the first component stays
    assert tiny.rank == 1
    with pytest.raises(ValueError, match="rank"):
        lipids.basis_from_subspace(s, vec, 0.01, 9)
    with pytest.raises(ValueError, match="all zero"):
        lipids.basis_from_subspace(np.zeros(4), vec[:, :4], 0.01, None)


def test_table_layout():
    from xmris_amd import device

    U = (np.arange(12) + 1j * np.arange(12, 24)).reshape(4, 3)
    tab = device.lipid_tables(U, [0.5, 0.25, 0.125])
    assert tab.dtype == np.float64 and tab.shape == (2 * 12 + 3,)
    assert tab[2 * (2 * 3 + 1)] == U[2, 1].real and tab[2 * (2 * 3 + 1) + 1] == U[2, 1].imag
    assert tab[24:].tolist() == [0.5, 0.25, 0.125]


# ---- the public call on host arrays: the numpy double of the device layer --------------------------------------------
class _Result:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _install(monkeypatch):
    import _numpy_device
    from xmris_amd import device

    _numpy_device.install(monkeypatch)
    calls = []

    def lipid_rows(x, axes, mask):
        lead = list(range(x.ndim - 1))
        perm = list(axes) + [a for a in lead if a not in axes] + [x.ndim - 1]
        return np.transpose(x, perm)[mask].reshape(-1, x.shape[-1]).astype(np.complex128)

    def lipid_subspace(L, kmax=64):
        s, u = orc.subspace_eig(np.asarray(L))
        return s, u[:, :kmax]

    def lipid_project(x, rec, apply=None, out=None, form=None, _skip=()):
        calls.append(dict(shape=x.shape, rank=rec.rank, apply=None if apply is None else np.array(apply)))
        flat = np.ascontiguousarray(x).reshape(-1, x.shape[-1])
        y = orc.apply(flat, rec.vectors, rec.weights).astype(x.dtype)
        status = np.zeros(flat.shape[0], dtype=np.int32)
        if apply is not None:
            off = ~np.asarray(apply).reshape(-1)
            y[off] = flat[off]
            status[off] = 1
        return _Result(out=y.reshape(x.shape), status=status.reshape(x.shape[:-1]), copied=not x.flags.c_contiguous)

    monkeypatch.setattr(device, "lipid_rows", lipid_rows)
    monkeypatch.setattr(device, "lipid_subspace", lipid_subspace)
    monkeypatch.setattr(device, "lipid_project", lipid_project)
    return calls


def _labeled(data, dims, attrs=None):
    from xmris_amd import Coordinate, LabeledArray

    coords = {d: Coordinate(d, np.arange(n, dtype=np.float64)) for d, n in zip(dims, data.shape)}
    return LabeledArray(data, dims, coords, dict(attrs or {}), "fid")


def test_public_call_on_the_phantom(monkeypatch):
    import xmris_amd as xa
    from xmris_amd import ATTRS

    calls = _install(monkeypatch)
    ph = orc.phantom()
    data = ph["data"].astype(np.complex64)
    fid = _labeled(data, ("y", "x", "time"), {"b0_field": 3.0})
    out, rec, status = xa.remove_lipids(fid, ph["scalp"], dims=("y", "x"), apply_mask=ph["brain"], return_basis=True)
    ref, b = orc.remove(data.astype(np.complex128), ph["scalp"], 0.01, None, apply_mask=ph["brain"])
    got = np.asarray(out.data)
    assert out.dims == ("y", "x", "time") and got.dtype == np.complex64 and out.name == "fid"
    assert np.abs(got - ref).max() <= 2.0 ** -23 * np.abs(data).max()
    assert np.array_equal(got[~ph["brain"]].view(np.float32), data[~ph["brain"]].view(np.float32))  # bit for bit
    assert np.array_equal(np.asarray(status.data) == 1, ~ph["brain"]) and status.dims == ("y", "x")
    assert rec.rank == b["rank"] and rec.n_rows == int(ph["scalp"].sum()) and rec.dropped_weight == b["dropped_weight"]
    assert out.attrs[ATTRS.lipid_level] == 0.01 and out.attrs[ATTRS.lipid_rank] == rec.rank
    assert out.attrs[ATTRS.lipid_beta] == rec.beta == pytest.approx(b["beta"]) and out.attrs[ATTRS.lipid_rows] == 44
    assert out.attrs["b0_field"] == 3.0 and set(out.coords) == {"y", "x", "time"}
    assert len(calls) == 1 and calls[0]["shape"] == (12, 12, 256)
    # the accessor is the same call; a LipidBasis is taken as it is
    again = fid.xmr.remove_lipids(basis=rec, dims=("y", "x"), apply_mask=ph["brain"])
    assert np.array_equal(np.asarray(again.data).view(np.float32), got.view(np.float32))
    # basis= rows give the subspace of the mask's rows
    rows = xa.remove_lipids(fid, basis=data[ph["scalp"]])
    full = xa.remove_lipids(fid, ph["scalp"], dims=("y", "x"))
    assert np.abs(np.asarray(rows.data) - np.asarray(full.data)).max() <= 1e-5 * np.abs(data).max()


def test_mask_over_some_dims_and_time_not_last(monkeypatch):
    """Every dim but the mask's and time contributes lipid rows; a mask given in another order of dims; time in front."""
    import xmris_amd as xa

    calls = _install(monkeypatch)
    rng = np.random.default_rng(5)
    data = rng.standard_normal((3, 32, 4, 5)) + 1j * rng.standard_normal((3, 32, 4, 5))  # coil, time, y, x
    fid = _labeled(data, ("coil", "time", "y", "x"))
    scalp = np.zeros((4, 5), dtype=bool)
    scalp[0, :] = scalp[3, 1] = True
    brain = np.zeros((5, 4), dtype=bool)  # over (x, y)
    brain[1:4, 1:3] = True
    out, rec, status = xa.remove_lipids(fid, scalp, dims=("y", "x"), rank=4, return_basis=True)
    assert rec.n_rows == 3 * 6 and rec.rank == 4 and out.dims == fid.dims and status.dims == ("coil", "y", "x")
    moved = np.moveaxis(data, 1, -1)  # coil, y, x, time
    L = np.transpose(moved, (1, 2, 0, 3))[scalp].reshape(-1, 32)
    b = orc.basis(L, 0.01, 4)
    ref = np.moveaxis(orc.apply(moved.reshape(-1, 32), b["U"], b["w"]).reshape(moved.shape), -1, 1)
    np.testing.assert_allclose(np.asarray(out.data), ref, rtol=0, atol=1e-12 * np.abs(data).max())
    masked = xa.remove_lipids(fid, scalp, dims=("y", "x"), rank=4, apply_mask=brain.T)
    ap = calls[-1]["apply"]
    assert ap.shape == (3, 4, 5) and np.array_equal(ap, np.broadcast_to(brain.T, (3, 4, 5)))
    keep = ~np.broadcast_to(brain.T[None, None], (3, 32, 4, 5))
    assert np.array_equal(np.asarray(masked.data)[keep], data[keep])
    with pytest.raises(ValueError, match="shape"):  # the mask in the order (x, y) under the names (y, x)
        xa.remove_lipids(fid, scalp, dims=("y", "x"), apply_mask=brain)


def test_value_errors(monkeypatch):
    import xmris_amd as xa
    from xmris_amd.processing import lipids

    calls = _install(monkeypatch)
    rng = np.random.default_rng(6)
    data = (rng.standard_normal((4, 5, 16)) + 1j * rng.standard_normal((4, 5, 16))).astype(np.complex64)
    fid = _labeled(data, ("y", "x", "time"))
    mask = np.zeros((4, 5), dtype=bool)
    mask[0] = True
    ok = dict(dims=("y", "x"))
    rec = xa.lipid_basis(fid, mask, **ok)
    bad = [
        (dict(lipid_mask=None), "exactly one"),
        (dict(lipid_mask=mask, basis=data[0]), "exactly one"),
        (dict(lipid_mask=mask[:3]), "shape"),
        (dict(lipid_mask=np.zeros((4, 5), dtype=bool)), "no true entry"),
        (dict(lipid_mask=mask, dims=None), "dims"),
        (dict(lipid_mask=mask, dims=("y", "z")), "missing"),
        (dict(lipid_mask=mask, dims=("y", "y")), "distinct"),
        (dict(lipid_mask=mask[0], dims=("time",)), "time dim"),
        (dict(lipid_mask=mask, level=0.0), "level"),
        (dict(lipid_mask=mask, level=-1.0), "level"),
        (dict(lipid_mask=mask, level=float("nan")), "level"),
        (dict(lipid_mask=mask, rank=0), "rank"),
        (dict(lipid_mask=mask, rank=65), "rank"),
        (dict(lipid_mask=mask, rank=2.5), "rank"),
        (dict(lipid_mask=mask, rank=6), "rank"),  # five lipid rows
        (dict(lipid_mask=None, basis=np.ones((3, 15), dtype=complex)), "along time"),
        (dict(lipid_mask=None, basis=np.ones(16, dtype=complex)), r"\[n, time\]"),
        (dict(lipid_mask=None, basis=lipids.basis_from_subspace([1.0], np.ones((8, 1)))), "points along time"),
        (dict(lipid_mask=mask, apply_mask=np.ones((5, 4), dtype=bool)), "shape"),
        (dict(lipid_mask=mask, dim="frequency"), "missing"),
    ]
    for change, match in bad:
        kw = dict(ok, lipid_mask=mask)
        kw.update(change)
        m = kw.pop("lipid_mask")
        with pytest.raises(ValueError, match=match):
            xa.remove_lipids(fid, m, **kw)
    with pytest.raises(TypeError, match="boolean"):
        xa.remove_lipids(fid, mask.astype(np.int32), **ok)
    with pytest.raises(ValueError, match="complex"):
        xa.remove_lipids(_labeled(data.real.copy(), ("y", "x", "time")), mask, **ok)
    with pytest.raises(ValueError, match="points"):
        xa.remove_lipids(_labeled(data[:, :, :1], ("y", "x", "time")), mask, **ok)
    with pytest.raises(ValueError, match="non-finite|all zero"):
        xa.remove_lipids(fid, basis=np.zeros((2, 16), dtype=complex))
    with pytest.raises(ValueError, match="already"):
        xa.lipid_basis(fid, basis=rec)
    assert not calls  # no refusal reached the projection


def test_vocabulary():
    from xmris_amd import ATTRS

    for name in ("lipid_level", "lipid_rank", "lipid_beta", "lipid_rows"):
        assert getattr(ATTRS, name) == name and ATTRS.get_description(name) != "No description available."


def test_c_abi_refusals_without_gpu():
    from xmris_amd import _lib

    lib = _lib.load()
    args = lambda a: [a[k] for k in orc.ABI_ORDER] + [None]  # noqa: E731
    for change in orc.REFUSALS:
        rc = lib.xm_lipid_project(*args(dict(orc.ABI_OK, **change)))
        assert rc == _lib.XM_ERR_INVALID_ARG, change
        assert b"lipid_project" in lib.xm_last_error_string(), change
    # no rows: nothing is launched, whatever the pointers hold
    assert lib.xm_lipid_project(*args(dict(orc.ABI_OK, n_rows=0, x=None, y=None))) == 0
    # every flag on top of both dtypes is a known dtype word (refused here for another reason: T)
    for flag in (_lib.XM_LIPID_FMA, _lib.XM_LIPID_SKIP_COEF, _lib.XM_LIPID_SKIP_APPLY):
        for dt in (_lib.XM_C64, _lib.XM_C128):
            assert lib.xm_lipid_project(*args(dict(orc.ABI_OK, dtype=dt | flag, T=1))) == _lib.XM_ERR_INVALID_ARG
            assert b"time points" in lib.xm_last_error_string()
