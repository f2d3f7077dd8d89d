"""Linked AMARES prior knowledge without a GPU: the reader's link grammar (fitting/prior_knowledge.py), the linked oracle
(tests/_amares_links.py) pinned to the unlinked one and to finite differences, the ABI's refusals, and the selection of
the cases tests/test_gpu_amares_links.py runs on the kernel."""
import functools
import os

import numpy as np
import pytest

import _amares_links as lk
import _amares_oracle as orc

HERE = os.path.dirname(os.path.abspath(__file__))
PK_PLAIN = os.path.join(HERE, "golden", "amares_pk_pcr_atp.csv")
PK_MULTI = os.path.join(HERE, "golden", "amares_pk_p31_multiplets.csv")
STEP_M = (1, 2, 3, 5)
TIE = 1e-9  # accept / reject margins below this are too close to call (tests/test_amares_kernel.py)

HEAD = "Index,A,B,C,AB\nInitial Values,,,,\n"
BOUNDS = ('Bounds,,,,\namplitude,"(0, ","(0, 3)","(0, 1)","(0, "\nchemicalshift,"(-1, 1)","(0, 0.5)",,\n'
          'linewidth,"(4, 60)","(4, 60)","(7, 7)","(4, 60)"\nphase,"(-180, 180)","(30, 30)",,\n')


def _read(tmp_path, rows, bounds=BOUNDS, name="pk.csv"):
    from xmris_amd.fitting.prior_knowledge import read_prior_knowledge

    f = tmp_path / name
    body = {"amplitude": "10,5,2,1", "chemicalshift": "0.2,0.1,0,3", "linewidth": "15,20,7,9", "phase": "0,30,0,0",
            "g": "0,0,0,0"}
    body.update(rows)
    f.write_text(HEAD + "".join(f"{k},{v}\n" for k, v in body.items()) + bounds)
    return read_prior_knowledge(f)


# ---- the reader -----------------------------------------------------------------------------------------------------
def test_every_grammar_form(tmp_path):
    q = lambda k, c: 5 * k + c  # noqa: E731
    pk = _read(tmp_path, {"amplitude": "10,A,A/2,2*A", "chemicalshift": "0.2,A-15Hz,A+0.1,A + 0.25 ppm",
                          "linewidth": "15,1.5*A,3 * A / 2 - 1,9", "phase": "0,30,B, A -  10"})
    assert pk.names == ["A", "B", "C", "AB"]
    to, sc, off, hz = pk.link_to, pk.link_scale, pk.link_offset, pk.link_offset_hz
    np.testing.assert_array_equal(to[:, 0], [-1, q(0, 0), q(0, 0), q(0, 0)])
    np.testing.assert_array_equal(sc[:, 0], [1, 1, 0.5, 2])
    np.testing.assert_array_equal(to[:, 1], [-1, q(0, 1), q(0, 1), q(0, 1)])
    np.testing.assert_array_equal(off[:, 1], [0, -15.0, 0.1, 0.25])
    np.testing.assert_array_equal(hz[:, 1], [False, True, False, False])
    assert not hz[:, [0, 2, 3, 4]].any()
    # "AB" is a name of its own: the longest name that fits wins over "A" (and "B")
    np.testing.assert_array_equal(to[:, 2], [-1, q(0, 2), q(0, 2), -1])
    np.testing.assert_array_equal(to[2, 2], q(0, 2))
    np.testing.assert_array_equal(sc[:, 2], [1, 1.5, 1.5, 1])
    np.testing.assert_array_equal(off[:, 2], [0, 0, -1.0, 0])
    np.testing.assert_array_equal(to[:, 3], [-1, -1, q(1, 3), q(0, 3)])
    np.testing.assert_array_equal(off[:, 3], [0, 0, 0, -10.0])
    pk2 = _read(tmp_path, {"linewidth": "AB,20,7,9"})
    assert pk2.link_to[0, 2] == q(3, 2) and pk2.link_to[3, 2] == -1

    # units: Hz offsets as they are, ppm x mhz, linewidth x pi, phase x pi / 180
    mhz = 120.0
    fto, fsc, foff = pk.fitting_links(mhz)
    np.testing.assert_array_equal(fto, to)
    np.testing.assert_array_equal(fsc, sc)
    np.testing.assert_allclose(foff[:, 1], [0, -15.0, 0.1 * mhz, 0.25 * mhz], rtol=1e-15)
    np.testing.assert_allclose(foff[2, 2], -np.pi, rtol=1e-15)
    np.testing.assert_allclose(foff[3, 3], -10.0 * np.pi / 180.0, rtol=1e-15)
    init, lo, hi = pk.fitting_units(mhz)
    np.testing.assert_allclose(init[:, 1], [0.2 * mhz, 0.2 * mhz - 15.0, 0.3 * mhz, 0.45 * mhz], rtol=1e-14)
    # file units: an Hz offset is offset / mhz ppm, known only once mhz is; every other follower is mapped at once
    assert np.isnan(pk.init[1, 1]) and pk.init[2, 1] == 0.2 + 0.1
    np.testing.assert_allclose(init[1, 1] / mhz, 0.2 - 15.0 / mhz, rtol=1e-14)


def test_chains_fixed_roots_ignored_bounds_and_clipped_start(tmp_path):
    # chains are composed: C = B/2, B = 2*A+1  ->  C = A + 0.5, both rooted in A
    pk = _read(tmp_path, {"amplitude": "10,2*A+1,B/2,1"})
    assert pk.link_to[1, 0] == pk.link_to[2, 0] == 0
    assert (pk.link_scale[1, 0], pk.link_offset[1, 0]) == (2.0, 1.0)
    assert (pk.link_scale[2, 0], pk.link_offset[2, 0]) == (1.0, 0.5)
    np.testing.assert_array_equal(pk.init[:, 0], [10.0, 21.0, 10.5, 1.0])
    # ... in the other column order too, and with Hz offsets along the chain
    pk = _read(tmp_path, {"chemicalshift": "B-8Hz,C-8Hz,0.3,3"}, bounds=BOUNDS.replace('"(0, 0.5)"', ""))
    assert pk.link_to[0, 1] == pk.link_to[1, 1] == 11 and pk.link_offset_hz[0, 1] and pk.link_offset_hz[1, 1]
    assert (pk.link_offset[0, 1], pk.link_offset[1, 1]) == (-16.0, -8.0)
    # a follower's Bounds cell is not applied: B's amplitude bounds (0, 3) do not clip 2 * 10 + 1, B's chemical shift
    # bounds (0, 0.5) do not fix or clip it; the follower is unbounded in the arrays
    pk = _read(tmp_path, {"amplitude": "10,2*A+1,2,1", "chemicalshift": "0.2,A+1,0,3"})
    assert pk.init[1, 0] == 21.0 and pk.lo[1, 0] == -np.inf and pk.hi[1, 0] == np.inf
    assert pk.init[1, 1] == 1.2 and not pk.fixed[1, 1]
    # the initial value is mapped from the CLIPPED root: A's chemical shift 5 is clipped to its bound 1
    pk = _read(tmp_path, {"chemicalshift": "5,2*A+0.5,0,3"})
    assert pk.init[0, 1] == 1.0 and pk.init[1, 1] == 2.5
    # a fixed root (C's linewidth, lo == hi == 7) makes fixed followers, at the mapped value
    pk = _read(tmp_path, {"linewidth": "2*C,C+1,7,9"})
    assert pk.fixed[:, 2].tolist() == [True, True, True, False]
    np.testing.assert_array_equal(pk.init[:, 2], [14.0, 8.0, 7.0, 9.0])
    # ... also when the follower's own Bounds cell would have fixed it: A follows the free AB
    pk = _read(tmp_path, {"linewidth": "15,20,AB,9"})
    assert not pk.fixed[2, 2] and pk.init[2, 2] == 9.0


@pytest.mark.parametrize("rows,match", [
    ({"amplitude": "10,5,D*2,1"}, r"row 3 \('amplitude'\), column 'C'.*unknown name"),
    ({"amplitude": "10,B,2,1"}, r"row 3 \('amplitude'\), column 'B'.*itself"),
    ({"linewidth": "B,C,A,9"}, r"row 5 \('linewidth'\), column '[ABC]'.*cycle"),
    ({"linewidth": "B,A,7,9"}, r"row 5 \('linewidth'\), column '[AB]'.*cycle"),
    ({"phase": "0,A/0,0,0"}, r"row 6 \('phase'\), column 'B'.*divides by zero"),
    ({"phase": "0,0*A,0,0"}, r"row 6 \('phase'\), column 'B'.*zero factor"),
    ({"phase": "0,0.0 * A / 3,0,0"}, r"row 6 \('phase'\), column 'B'.*zero factor"),
    ({"amplitude": "10,A*0.5,2,1"}, r"row 3 \('amplitude'\), column 'B'.*not a link.*in front"),
    ({"linewidth": "15,A-2Hz,7,9"}, r"row 5 \('linewidth'\), column 'B'.*unit 'Hz'.*'chemicalshift'"),
    ({"amplitude": "10,A+1ppm,2,1"}, r"row 3 \('amplitude'\), column 'B'.*unit 'ppm'"),
    ({"amplitude": "10,A*B,2,1"}, r"row 3 \('amplitude'\), column 'B'.*not a link"),
    ({"amplitude": "10,sqrt(A),2,1"}, r"row 3 \('amplitude'\), column 'B'.*not a link"),
    ({"amplitude": "10,A+,2,1"}, r"row 3 \('amplitude'\), column 'B'.*not a link"),
    ({"chemicalshift": "0.2,A-8Hz,B+0.1,3"}, r"row 4 \('chemicalshift'\), column 'C'.*mixes"),
])
def test_refusals_name_row_and_column(tmp_path, rows, match):
    with pytest.raises(ValueError, match=match):
        _read(tmp_path, rows)


def test_plain_fixtures_parse_as_before():
    from xmris_amd.fitting.prior_knowledge import read_prior_knowledge

    pk = read_prior_knowledge(PK_PLAIN)
    np.testing.assert_array_equal(pk.init, [[10.0, 0.0, 15.0, 0.0, 0.0], [5.0, -7.5, 20.0, 0.0, 0.0]])
    np.testing.assert_array_equal(pk.lo, [[0.0, -0.5, 5.0, -180, 0], [0.0, -8.0, 10.0, -180, 0]])
    np.testing.assert_array_equal(pk.hi, [[np.inf, 0.5, 30.0, 180, 1], [np.inf, -7.0, 40.0, 180, 1]])
    assert not pk.fixed.any() and np.all(pk.link_to == -1) and pk.link_to.shape == (2, 5)
    assert np.all(pk.link_scale == 1) and not pk.link_offset.any() and not pk.link_offset_hz.any()
    for a, b in zip(pk.fitting_units(120.0), orc.notebook_pk(120.0)):
        np.testing.assert_allclose(a, b, rtol=1e-15)


def test_multiplet_fixture_is_the_helpers_prior_knowledge():
    from xmris_amd.fitting.prior_knowledge import read_prior_knowledge

    mhz = 120.0
    pk = read_prior_knowledge(PK_MULTI)
    assert tuple(pk.names) == lk.MULTIPLET_NAMES
    init, lo, hi, fixed, links = lk.multiplet_pk(mhz)
    got = pk.fitting_units(mhz)
    for a, b in zip(got, (init, lo, hi)):
        np.testing.assert_allclose(a, b, rtol=1e-14, atol=1e-12)
    np.testing.assert_array_equal(pk.fixed, fixed)
    to, sc, off = pk.fitting_links(mhz)
    np.testing.assert_array_equal(to, links[0])
    np.testing.assert_array_equal(sc, links[1])
    np.testing.assert_allclose(off, links[2], rtol=1e-15)
    assert np.count_nonzero(to >= 0) == 16 and pk.link_offset_hz.sum() == 4
    assert np.count_nonzero(~pk.fixed & (to < 0)) == 20  # 45 parameters, 20 free columns
    # the followers' Bounds cells are filled in the file (as typical files have them) and are not applied
    assert np.all(np.isinf(pk.lo[to >= 0][~pk.fixed[to >= 0]]))


# ---- the linked oracle against the unlinked one ---------------------------------------------------------------------
@pytest.mark.parametrize("name", [name for name, _ in orc.step_cases()])
def test_lm_steps_linked_without_links_is_lm_steps_bit_for_bit(name):
    c = orc.kernel_case(**dict(orc.step_cases())[name])
    for m in (1, 5, 200):
        a = orc.lm_steps(c["x"][0], c["t"], c["init"], c["lo"], c["hi"], c["fixed"], max_iter=m)
        b = lk.lm_steps_linked(c["x"][0], c["t"], c["init"], c["lo"], c["hi"], c["fixed"], None, max_iter=m)
        assert a["iters"] == b["iters"] and a["status"] == b["status"] and a["rss"] == b["rss"], (name, m)
        assert np.array_equal(a["params"], b["params"]) and np.array_equal(a["u"], b["u"]), (name, m)
        assert a["trials"] == b["trials"] and np.array_equal(a["path"], b["path"]), (name, m)


@pytest.mark.parametrize("which", ["notebook", "K8"])
def test_fit_linked_without_links_is_fit(which):
    if which == "notebook":
        data, t, mhz = orc.notebook_dataset()
        init, lo, hi = orc.notebook_pk(mhz)
        fixed = None
    else:
        c = orc.kernel_case(8, 1537, 11, n_vox=1)
        data, t, init, lo, hi, fixed = c["x"], c["t"], c["init"], c["lo"], c["hi"], c["fixed"]
    for x in data[:2]:
        a, b = orc.fit(x, t, init, lo, hi, fixed), lk.fit_linked(x, t, init, lo, hi, fixed, None)
        for k in ("params", "sd", "crlb", "snr"):
            np.testing.assert_allclose(b[k], a[k], rtol=1e-12, atol=0, err_msg=k)
        assert abs(a["rss"] - b["rss"]) <= 1e-12 * a["rss"] and a["ier"] == b["ier"]
        sd, cond = orc.amplitude_sd(t, a["params"], lo, hi, fixed)
        sd2, cond2 = lk.amplitude_sd_linked(t, a["params"], lo, hi, fixed, None)
        np.testing.assert_allclose(sd2, sd, rtol=1e-12)
        assert abs(cond - cond2) <= 1e-12 * cond


@functools.lru_cache(maxsize=None)
def _cases():
    return lk.gpu_cases()


@pytest.mark.parametrize("name", ["doublet_K3_n64", "doublet_negative_scale", "doublet_amplitude_offset",
                                  "multiplets_K9_n300", "K16_P20_n257"])
def test_chained_jacobian_against_finite_differences(name):
    """d model / d theta through E (expansion) and through the summed columns (reduce), against central differences of
    the model in the root parameters."""
    c = _cases()[name]
    K = c["init"].shape[0]
    E, b, roots = lk.expansion(c["links"], K)
    assert E.shape == (5 * K, np.count_nonzero(np.asarray(c["links"][0]) < 0))
    p = c["truth"].ravel()
    np.testing.assert_allclose(E @ p[roots] + b, p, rtol=1e-14, atol=1e-12)  # the truth obeys its links
    t = c["t"]
    L = lk._Layout(c["init"], c["lo"], c["hi"], c["fixed"], c["links"])
    cols = [int(np.flatnonzero(roots == q)[0]) for q in L.free]
    jac = orc.model_jacobian(p, t) @ E[:, cols]
    summed = L.reduce(orc.model_jacobian(p, t), L.link_scale())
    np.testing.assert_allclose(summed, jac, rtol=1e-12, atol=1e-12 * np.abs(jac).max())
    theta = p[roots]
    for j, col in enumerate(cols):
        h = 1e-6 * max(1.0, abs(theta[col]))
        e = np.zeros(theta.size)
        e[col] = h
        fd = (orc.model(E @ (theta + e) + b, t) - orc.model(E @ (theta - e) + b, t)) / (2 * h)
        assert np.abs(fd - jac[:, j]).max() <= 1e-6 * np.abs(jac[:, j]).max(), (name, j)


# ---- selection of the GPU cases, without the kernel -------------------------------------------------------------------
def test_gpu_cases_cover_what_they_claim():
    c = _cases()
    cols = {name: lk.n_columns(case) for name, case in c.items()}
    assert cols == {"doublet_K3_n64": 8, "doublet_negative_scale": 8, "doublet_amplitude_offset": 8,
                    "doublet_root_on_bound": 8, "multiplets_K9_n300": 20, "K16_P20_n257": 20,
                    "K16_single_link_n300": 63}
    assert c["doublet_K3_n64"]["links"][0][0, 0] == 5  # the root (peak 1) is listed after its follower (peak 0)
    assert c["doublet_negative_scale"]["links"][1][0, 0] < 0 and c["doublet_amplitude_offset"]["links"][2][0, 0] != 0
    assert 300 % 128 and 257 % 128 and 300 % 64  # ragged last rounds in their staging tiers
    for case in c.values():
        assert 4 <= case["x"].shape[0] <= 7
    b = c["doublet_root_on_bound"]
    assert b["init"][1, 1] == b["hi"][1, 1] and np.isfinite(b["lo"][1, 1])


@pytest.mark.parametrize("name", list(lk.gpu_cases()))
def test_oracle_converges_on_every_gpu_case(name):
    c = _cases()[name]
    for v in range(c["x"].shape[0]):
        o = lk.fit_linked(c["x"][v], c["t"], c["init"], c["lo"], c["hi"], c["fixed"], c["links"])
        assert o["ier"] in (1, 2, 3, 4), (name, v, o["ier"])
        assert o["n_free"] == lk.n_columns(c)


def test_step_cases_have_no_ties():
    """No trial of lm_steps_linked on the committed step cases has an accept / reject margin below 1e-9 relative: the
    share of excluded trials is 0."""
    for name in lk.STEP_CASES:
        c = _cases()[name]
        for v in range(c["x"].shape[0]):
            for m in STEP_M:
                ref = lk.lm_steps_linked(c["x"][v], c["t"], c["init"], c["lo"], c["hi"], c["fixed"], c["links"],
                                         max_iter=m)
                assert ref["iters"] == m and ref["status"] == 1, (name, v, m)
                assert not any(abs(margin) < TIE for _, margin in ref["trials"]), (name, v, m, ref["trials"])


# ---- the C ABI's refusals (no GPU needed: they come before any HIP call) ----------------------------------------------
def test_abi_refuses_bad_link_tables():
    from xmris_amd import _lib

    lib = _lib.load()
    c = _cases()["doublet_K3_n64"]
    init, lo, hi = (np.ascontiguousarray(c[k]) for k in ("init", "lo", "hi"))
    fixed = np.ascontiguousarray(c["fixed"], dtype=np.int32)
    buf = np.zeros(1 << 12)
    pp = lambda a: a.ctypes.data  # noqa: E731

    def call(to, sc, off, n=64):
        to = np.ascontiguousarray(to, dtype=np.int32)
        sc, off = np.ascontiguousarray(sc, dtype=np.float64), np.ascontiguousarray(off, dtype=np.float64)
        return lib.xm_amares_fit_linked(pp(buf), n, 0, n, 1e-3, 0.0, 3, pp(init), pp(lo), pp(hi), pp(fixed), pp(to),
                                        pp(sc), pp(off), 200, 1e-10, 1e-10, pp(buf), pp(buf), pp(buf), pp(buf),
                                        pp(buf), None, pp(buf), 256, _lib.XM_C128, None)

    good = [a.copy() for a in c["links"]]
    assert call(*good) == 0  # n_batch = 0: validated, nothing launched
    assert call(*good, n=8) == 0 and call(*good, n=7) == _lib.XM_ERR_INVALID_ARG  # n against the 8 columns, not 11
    assert b"smaller than the free parameters (8)" in lib.xm_last_error_string()

    def bad(edit, text):
        to, sc, off = (a.copy() for a in good)
        edit(to, sc, off)
        assert call(to, sc, off) == _lib.XM_ERR_INVALID_ARG, text
        assert text.encode() in lib.xm_last_error_string(), (text, lib.xm_last_error_string())

    def set_(i, k, c_, v):
        return lambda to, sc, off: (to, sc, off)[i].__setitem__((k, c_), v)

    bad(set_(0, 2, 0, 15), "out of range")
    bad(set_(0, 2, 0, -2), "out of range")
    bad(set_(0, 2, 0, 6), "another kind")
    bad(set_(0, 2, 0, 10), "itself")
    bad(set_(0, 2, 0, 0), "itself linked")   # peak 0's amplitude follows peak 1's
    bad(set_(1, 0, 0, 0.0), "link_scale")
    bad(set_(1, 0, 1, np.inf), "link_scale")
    bad(set_(1, 0, 2, np.nan), "link_scale")
    bad(set_(2, 0, 1, np.nan), "link_offset")
    bad(set_(2, 0, 0, -np.inf), "link_offset")
    assert lib.xm_amares_fit_linked(pp(buf), 64, 0, 64, 1e-3, 0.0, 3, pp(init), pp(lo), pp(hi), pp(fixed),
                                    pp(np.ascontiguousarray(good[0], dtype=np.int32)), None, None, 200, 1e-10, 1e-10,
                                    *([pp(buf)] * 5), None, pp(buf), 256, _lib.XM_C128, None) == _lib.XM_ERR_INVALID_ARG
