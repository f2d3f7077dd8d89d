"""The device search's two kernels directly (csrc/xm_search.hip): `k_search` through `search_launch` / `search_eval`
against the host engine and the numpy objective, and `k_search_rows` against `k_search` on the same slice -- both
instantiate one body, so their records must agree byte for byte.  One case per points-per-worker count P of the launch
table, FULL (n = 448 P) and not; `_search_cases.CASES` lists them.  Slices and host answers are made once per module."""
import numpy as np
import pytest

import _search_cases as sc

pytestmark = pytest.mark.gpu

_ids = [f"n{n}-seed{s}" for n, s in sc.CASE_LIST]
_slices, _hosts, _singles = {}, {}, {}


@pytest.fixture(scope="module")
def dev():
    import torch

    from xmris_amd import device

    assert torch.cuda.is_available(), "GPU tests need a HIP device (no CPU fallback exists)"
    return device


def _slice(dev, n, seed):
    """(spectrum, frequency axis, arg-max bin, uniform axis, the spectrum in pinned memory)"""
    import torch

    if (n, seed) not in _slices:
        spec, freq, k = sc.make_slice(n, seed)
        _slices[n, seed] = (spec, freq, k, dev.uniform_axis(freq), torch.from_numpy(spec.copy()).pin_memory())
    return _slices[n, seed]


def _host(dev, n, seed, p0_only):
    if (n, seed, p0_only) not in _hosts:
        spec, freq, k, _, _ = _slice(dev, n, seed)
        _hosts[n, seed, p0_only] = sc.host_answer(spec, freq, k, p0_only)
    return _hosts[n, seed, p0_only]


def _single(dev, n, seed, p0_only):
    """One `search_launch` of the case: (its fields, the nine shared ones as bytes)"""
    if (n, seed, p0_only) not in _singles:
        _, _, _, axis, pinned = _slice(dev, n, seed)
        rec = dev.new_search_record()
        r = sc.run_search(dev, pinned, axis, rec, sc.next_seq(), p0_only)
        _singles[n, seed, p0_only] = (r, sc.shared_fields(rec))
    return _singles[n, seed, p0_only]


@pytest.mark.parametrize("p0_only", [False, True])
@pytest.mark.parametrize("n,seed", sc.CASE_LIST, ids=_ids)
def test_search_launch_equals_the_host_engine(dev, n, seed, p0_only):
    """x, nfev, nit, status, target_idx are `NativeObjective.de`'s exactly; needs_polish is the host's rule
    pg_norm > 0.5e-5 on `obj.fg`'s gradient."""
    k = _slice(dev, n, seed)[2]
    host = _host(dev, n, seed, p0_only)
    r, _ = _single(dev, n, seed, p0_only)
    print(f"n={n} seed={seed} p0_only={int(p0_only)}: device x={r['x']!r} nfev {r['nfev']} nit {r['nit']} status {r['status']} "
          f"target {r['target_idx']} pg {r['pg_norm']:.3e} | host x={host['x']!r} nfev {host['nfev']} nit {host['nit']} "
          f"status {host['status']} target {k} pg {host['pg_norm']:.3e}")
    assert np.array_equal(np.array(r["x"][:len(host["x"])]), host["x"])
    assert (r["nfev"], r["nit"], r["status"], r["target_idx"]) == (host["nfev"], host["nit"], host["status"], k)
    assert r["needs_polish"] == host["needs_polish"]


@pytest.mark.parametrize("p0_only", [False, True])
@pytest.mark.parametrize("n,seed", sc.CASE_LIST, ids=_ids)
def test_search_rows_record_equals_search_launch(dev, n, seed, p0_only):
    """The same slice as a one-row complex128 tensor (p0_only: with the pivot and target bin given): the nine fields
    the two records share are equal as bytes."""
    spec, _, k, axis, _ = _slice(dev, n, seed)
    _, single = _single(dev, n, seed, p0_only)
    row = sc.shared_fields(sc.rows_record(dev, spec, axis, k, p0_only))
    for f in sc.SHARED:
        assert row[f] == single[f], f


@pytest.mark.parametrize("n,seed", sc.CASE_LIST, ids=_ids)
def test_search_eval_equals_the_numpy_objective(dev, n, seed):
    """16 points against `acme_score`: relative error <= 1e-11 (scripts/check_device_search.py's bound); the kernel's
    own arg-max (target_idx = -1) and the index given are the same pivot, so the same scores."""
    spec, freq, k, axis, pinned = _slice(dev, n, seed)
    xs = sc.eval_points(seed)
    ref = sc.eval_reference(xs, spec, freq, k)
    got = dev.search_eval(pinned, axis, xs)
    given = dev.search_eval(pinned, axis, xs, target_idx=k)
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print(f"n={n} seed={seed}: objective rel err {err:.2e}")
    assert err <= 1e-11
    assert np.array_equal(got, given)


def test_four_searches_at_once(dev):
    """Four `search_launch` on four streams into four records, in flight together: each equals the lone run."""
    import torch

    n, seed = 512, 7000
    _, _, _, axis, pinned = _slice(dev, n, seed)
    _, single = _single(dev, n, seed, False)
    streams = [torch.cuda.Stream() for _ in range(4)]
    recs = [dev.new_search_record() for _ in range(4)]
    seq = sc.next_seq()
    torch.cuda.synchronize()
    for st, rec in zip(streams, recs):
        dev.search_launch(pinned, axis, rec, seq, stream=st)
    sc.wait_done(dev, recs, seq)
    for rec in recs:
        assert sc.shared_fields(rec) == single
