"""Linked prior knowledge on top of tests/_amares_oracle.py, in numpy / scipy alone (no xmris_amd): the yardstick of
k_amares_fit<true> and xm_amares_fit_linked.

A link makes parameter q = 5 k + c follow its root m = 5 k' + c (same kind of parameter, another peak, itself unlinked)
as p_q = scale_q p_m + offset_q.  With theta the unlinked parameters ("roots", fixed ones included), p = E theta + b.
The fit runs over the free roots: column j of the reduced Jacobian is the sum over the members q of group j of
d model / d p_q times scale_q (times the root's dp/du in the internal variables) -- summed in the kernel's order,
peak index ascending (the members of a group share c).

links: None or (link_to, link_scale, link_offset), each [K, 5], link_to holding parameter indices (-1: not linked).
"""
import numpy as np
from scipy.optimize import leastsq

import _amares_oracle as orc


def no_links(K):
    return np.full((K, 5), -1, dtype=np.int32), np.ones((K, 5)), np.zeros((K, 5))


def _flat(links, K):
    to, sc, off = no_links(K) if links is None else links
    return (np.asarray(to, dtype=np.int64).ravel(), np.asarray(sc, dtype=np.float64).ravel(),
            np.asarray(off, dtype=np.float64).ravel())


def expansion(links, K):
    """(E [5K, R], b [5K], roots [R]): p = E theta + b with theta = p[roots], roots ascending."""
    to, sc, off = _flat(links, K)
    roots = np.flatnonzero(to < 0)
    E, b = np.zeros((5 * K, roots.size)), np.zeros(5 * K)
    where = {int(q): j for j, q in enumerate(roots)}
    for q in range(5 * K):
        if to[q] < 0:
            E[q, where[q]] = 1.0
        else:
            assert to[q] % 5 == q % 5 and to[q] != q and to[to[q]] < 0, (q, to[q])
            E[q, where[int(to[q])]] = sc[q]
            b[q] = off[q]
    return E, b, roots


class _Layout:
    """Who is free, who follows whom, and the start: everything lm_steps_linked / fit_linked share."""

    def __init__(self, init, lo, hi, fixed, links):
        init = np.asarray(init, dtype=np.float64)
        K = init.size // 5
        self.K = K
        self.to, self.sc, self.off = _flat(links, K)
        lo, hi, fx, _ = orc._split(lo, hi, fixed)
        self.lo, self.hi = lo, hi
        self.linked = self.to >= 0
        self.free = np.flatnonzero(~fx & ~self.linked)                   # free roots, ascending: the columns
        self.members = [[int(q)] + [int(f) for f in np.flatnonzero(self.to == q)] for q in self.free]
        for m in self.members:
            m.sort()
        self.col = np.full(5 * K, -1)
        for j, m in enumerate(self.members):
            self.col[m] = j
        v0 = np.clip(init.ravel(), lo, hi)
        f = np.flatnonzero(self.linked)
        v0[f] = self.sc[f] * v0[self.to[f]] + self.off[f]                  # followers start at the mapped root
        self.v0 = v0
        self.fixed_all = self.col < 0                                      # fixed roots and their followers
        self.u0 = np.array([orc.to_internal(v0[q], lo[q], hi[q]) for q in self.free])

    def physical(self, u):
        """(p, s) [5K]: physical values and d p / d u_col of every parameter (0 for fixed ones)."""
        p, s = self.v0.copy(), np.zeros(5 * self.K)
        for j, q in enumerate(self.free):
            p[q], s[q] = orc.from_internal(u[j], self.lo[q], self.hi[q])
        for q in np.flatnonzero(self.linked & (self.col >= 0)):
            m = self.to[q]
            p[q] = self.sc[q] * p[m] + self.off[q]
            s[q] = self.sc[q] * s[m]
        return p, s

    def link_scale(self):
        """d p_q / d p_root [5K]: 1 for a free root, scale for a follower, 0 for fixed parameters."""
        w = np.zeros(5 * self.K)
        w[self.free] = 1.0
        f = self.linked & (self.col >= 0)
        w[f] = self.sc[f]
        return w

    def reduce(self, jm, w):
        """complex [n, 5K] physical Jacobian, factors w [5K] -> [n, P]: the members of a column added in ascending
        parameter order (the first one assigned, as a column with one member is in _amares_oracle)."""
        first = np.array([m[0] for m in self.members], dtype=np.int64)
        out = jm[:, first] * w[first]  # the very expression of _amares_oracle._normal when nothing is linked
        for j, m in enumerate(self.members):
            for q in m[1:]:
                out[:, j] += jm[:, q] * w[q]
        return out


def fit_linked(x, t, init, lo, hi, fixed=None, links=None, xtol=1e-12, ftol=1e-12, maxfev=4000):
    """orc.fit over the free roots: MINPACK lmder in their internal variables, Jacobian model_jacobian(p) @ E chained
    through the root's from_internal.  Returns orc.fit's dict (sd of a follower = |scale| sd of its root) + n_free."""
    x = np.asarray(x, dtype=np.complex128)
    t = np.asarray(t, dtype=np.float64)
    L = _Layout(init, lo, hi, fixed, links)
    E, _, roots = expansion(links, L.K)
    cols = np.array([int(np.flatnonzero(roots == q)[0]) for q in L.free])
    Ef = E[:, cols]

    def fun(u):
        r = x - orc.model(L.physical(u)[0], t)
        return np.concatenate([r.real, r.imag])

    def jac(u):
        p, s = L.physical(u)
        jm = (orc.model_jacobian(p, t) @ Ef) * s[L.free]
        return -np.concatenate([jm.real, jm.imag])

    u, _, _, _, ier = leastsq(fun, L.u0, Dfun=jac, full_output=True, xtol=xtol, ftol=ftol, maxfev=maxfev)
    p = L.physical(u)[0]
    r = fun(u)
    rss = float(r @ r)
    sigma = np.sqrt(rss / (2 * len(t) - L.free.size))
    jr = orc.real_rows(orc.model_jacobian(p, t) @ Ef)
    cov = sigma ** 2 * np.linalg.inv(jr.T @ jr)
    sd = np.abs(Ef) @ np.sqrt(np.diag(cov))  # one nonzero per row of Ef
    P, SD = p.reshape(-1, 5), sd.reshape(-1, 5)
    a = P[:, 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        crlb = np.where(a != 0, 100.0 * SD[:, 0] / np.abs(a), 0.0)
    return {"params": P, "sd": SD, "rss": rss, "sigma": sigma, "crlb": crlb, "snr": a / sigma, "ier": ier,
            "n_free": int(L.free.size)}


def amplitude_sd_linked(t, params, lo, hi, fixed=None, links=None):
    """orc.amplitude_sd over the reduced physical Jacobian: (sd [K], cond).  The sd of a linked amplitude is |scale|
    times its column's; 0 for a fixed amplitude (a follower of a fixed root included)."""
    p = np.asarray(params, dtype=np.float64).ravel()
    L = _Layout(p, lo, hi, fixed, links)
    w = L.link_scale()
    jr = orc.real_rows(L.reduce(orc.model_jacobian(p, t), w))
    sv = np.linalg.svd(jr, compute_uv=False)
    with np.errstate(divide="ignore"):
        cond = float((sv[0] / sv[-1]) ** 2) if sv[-1] > 0 else np.inf
    c = np.linalg.norm(jr, axis=0)
    sd_col = np.full(len(L.members), np.nan)
    if np.all(c > 0):
        _, s, vt = np.linalg.svd(jr / c, full_matrices=False)
        with np.errstate(divide="ignore", invalid="ignore"):
            sd_col = np.sqrt(np.sum((vt.T / s) ** 2, axis=1)) / c
    sd = np.zeros(5 * L.K)
    has = L.col >= 0
    sd[has] = np.abs(w[has]) * sd_col[L.col[has]]
    return sd.reshape(-1, 5)[:, 0], cond


def lm_steps_linked(x, t, init, lo, hi, fixed=None, links=None, max_iter=200, ftol=1e-10, xtol=1e-10):
    """orc.lm_steps (solver "normal") over the reduced columns; the same dict.  Without links it performs the same
    floating-point operations as orc.lm_steps."""
    x = np.asarray(x, dtype=np.complex128)
    t = np.asarray(t, dtype=np.float64)
    L = _Layout(init, lo, hi, fixed, links)
    u = L.u0.copy()
    P = L.free.size

    def normal(p, s):
        jr = orc.real_rows(L.reduce(orc.model_jacobian(p, t), s))
        r = orc.real_rows(x - orc.model(p, t))
        return jr.T @ jr, jr.T @ r

    p, s = L.physical(u)
    r = x - orc.model(p, t)
    F = float(np.sum(r.real ** 2 + r.imag ** 2))
    dsc = np.zeros(P)
    lam, nu, it = 1e-3, 2.0, 0
    status = 1 if np.isfinite(F) else 2
    need_jac, trials, path = True, [], np.zeros(5 * L.K)
    while status == 1 and it < max_iter:
        if need_jac:
            p, s = L.physical(u)
            H, g = normal(p, s)
            dsc = np.maximum(dsc, np.diag(H))
            need_jac = False
        it += 1
        D = np.where(dsc > 0, dsc, 1.0)
        try:
            with np.errstate(all="ignore"):
                dl = np.linalg.solve(H + lam * np.diag(D), g)
            ok = bool(np.all(np.isfinite(dl)))
        except np.linalg.LinAlgError:
            ok = False
        if not ok:
            trials.append((False, -np.inf))
            lam *= nu
            nu *= 2.0
            if not np.isfinite(lam):
                break
            continue
        dn = np.sqrt(np.sum(D * dl * dl))
        un = np.sqrt(np.sum(D * u * u))
        pred = float(dl @ (lam * D * dl + g))
        xconv = dn <= xtol * (un + xtol)
        ut = u + dl
        pt, _ = L.physical(ut)
        with np.errstate(all="ignore"):
            rt = x - orc.model(pt, t)
            Ft = float(np.sum(rt.real ** 2 + rt.imag ** 2))
        margin = (F - Ft) / F if F > 0 and np.isfinite(Ft) else -np.inf
        if np.isfinite(Ft) and Ft < F:
            trials.append((True, margin))
            rho = min(max((F - Ft) / pred, 0.0), 1.0)
            fconv = (F - Ft) <= ftol * F
            path += np.abs(pt - p)
            u, F, p = ut, Ft, pt
            q = 2.0 * rho - 1.0
            lam *= max(1.0 / 3.0, 1.0 - q * q * q)
            nu = 2.0
            need_jac = True
            if fconv or xconv:
                status = 0
        else:
            trials.append((False, margin))
            lam *= nu
            nu *= 2.0
            if xconv:
                status = 0
            if not np.isfinite(lam):
                break
    p = L.physical(u)[0]
    if not (np.all(np.isfinite(p)) and np.isfinite(F)):
        status = 2
    return {"params": p.reshape(-1, 5), "u": u, "rss": F, "iters": it, "status": status, "trials": trials,
            "path": path}


# ---- the committed GPU cases (tests/test_gpu_amares_links.py; selected on the CPU in tests/test_amares_links.py) -----
def _link(links, follower, root, c, scale=1.0, offset=0.0):
    links[0][follower, c] = 5 * root + c
    links[1][follower, c] = scale
    links[2][follower, c] = offset


def _data(truth, links, K, n, dt, t0, n_vox, seed, noise):
    """n_vox noisy voxels of the linked truth (the followers of `truth` are overwritten by their links)."""
    E, b, roots = expansion(links, K)
    truth = (E @ truth.ravel()[roots] + b).reshape(K, 5)
    t = np.arange(n) * dt + t0
    rng = np.random.default_rng([seed, K, n])
    z = rng.standard_normal((n_vox, n)) + 1j * rng.standard_normal((n_vox, n))
    return truth, t, orc.model(truth, t)[None] + noise * z


def doublet_case(n=64, n_vox=5, scale=0.5, amp_offset=0.0, seed=1, dt=1e-3, t0=0.0, noise=0.05, root_on_bound=False):
    """K = 3: peak 0 follows peak 1 (the root is listed after its follower) in amplitude (ratio `scale`, plus
    `amp_offset`), frequency (-17 Hz), damping and phase; peak 2 is a free singlet.  g fixed.  Bounds of all types.
    root_on_bound: the root's frequency (two-sided) starts on its upper bound, so the whole group stays there."""
    K = 3
    links = no_links(K)
    _link(links, 0, 1, 0, scale, amp_offset)
    _link(links, 0, 1, 1, 1.0, -17.0)
    _link(links, 0, 1, 2)
    _link(links, 0, 1, 3)
    truth = np.array([[0.0, 0.0, 0.0, 0.0, 0.3], [8.0, 60.0, 25.0, 0.3, 0.3], [5.0, -140.0, 35.0, -0.2, 0.3]])
    truth, t, x = _data(truth, links, K, n, dt, t0, n_vox, seed, noise)
    init = truth * np.array([1.15, 1.0, 0.85, 1.0, 1.0]) + np.array([0.0, 3.0, 0.0, 0.15, 0.0])
    lo = np.array([[0.0, -np.inf, -np.inf, -np.inf, 0.0]] * K)
    hi = np.array([[np.inf, np.inf, 400.0, np.inf, 1.0]] * K)
    lo[:, 1], hi[:, 1] = truth[:, 1] - 40.0, truth[:, 1] + 40.0
    lo[2, 2], hi[2, 2] = 2.0, np.inf
    lo[2, 3], hi[2, 3] = -np.pi, np.pi
    fixed = np.zeros((K, 5), bool)
    fixed[:, 4] = True
    if root_on_bound:  # the doublet's frequency group starts on the root's upper bound
        init[1, 1] = hi[1, 1]
    return {"x": x, "t": t, "dt": dt, "t0": t0, "truth": truth, "init": init, "lo": lo, "hi": hi, "fixed": fixed,
            "links": links}


# the 9-line 31P model of tests/golden/amares_pk_p31_multiplets.csv, restated in fitting units
MULTIPLET_NAMES = ("PCr", "Pi", "gATP1", "gATP2", "aATP1", "aATP2", "bATP1", "bATP2", "bATP3")
MULTIPLET_J_HZ = 16.0


def multiplet_pk(mhz):
    """(init, lo, hi, fixed, links) [9, 5] in fitting units: what the CSV says.  Followers: lo / hi unbounded (their
    Bounds cells are not applied), init mapped from the root."""
    deg = np.pi / 180.0
    root = {0: None, 1: None, 2: None, 3: 2, 4: None, 5: 4, 6: None, 7: 6, 8: 6}
    amp = {3: 1.0, 5: 1.0, 7: 2.0, 8: 1.0}
    hz = {3: -16.0, 5: -16.0, 7: -16.0, 8: -32.0}
    a0 = {0: 20.0, 1: 6.0, 2: 4.0, 4: 4.0, 6: 1.5}
    ppm = {0: 0.0, 1: 4.9, 2: -2.43, 4: -7.45, 6: -16.0}
    ppm_lo = {0: -0.4, 1: 4.5, 2: -2.83, 4: -7.85, 6: -16.4}
    ppm_hi = {0: 0.4, 1: 5.3, 2: -2.03, 4: -7.05, 6: -15.6}
    lw = {0: 12.0, 1: 18.0, 2: 20.0, 4: 20.0, 6: 22.0}
    K = 9
    init, lo, hi = np.zeros((K, 5)), np.full((K, 5), -np.inf), np.full((K, 5), np.inf)
    links = no_links(K)
    for k in range(K):
        if root[k] is None:
            init[k] = [a0[k], ppm[k] * mhz, lw[k] * np.pi, 0.0, 0.0]
            lo[k] = [0.0, ppm_lo[k] * mhz, 4.0 * np.pi, -180 * deg, 0.0]
            hi[k] = [np.inf, ppm_hi[k] * mhz, 60.0 * np.pi, 180 * deg, 0.0]
    for k in range(K):
        if root[k] is not None:
            r = root[k]
            _link(links, k, r, 0, amp[k])
            _link(links, k, r, 1, 1.0, hz[k])
            _link(links, k, r, 2)
            _link(links, k, r, 3)
            init[k] = [amp[k] * init[r, 0], init[r, 1] + hz[k], init[r, 2], init[r, 3], 0.0]
            lo[k, 4] = hi[k, 4] = 0.0
    fixed = lo == hi
    return init, lo, hi, fixed, links


def multiplet_case(n=300, n_vox=4, seed=3, mhz=120.0, sw=10000.0, t0=0.0, noise=0.3):
    """Seeded truth around the multiplet prior knowledge (amplitudes x 0.7 ... 1.3, shifts +-0.1 ppm, widths x 0.85 ...
    1.15, one phase per voxel set -- shared by the n_vox voxels, which differ in their noise)."""
    init, lo, hi, fixed, links = multiplet_pk(mhz)
    rng = np.random.default_rng([seed, n])
    truth = init.copy()
    truth[:, 0] *= rng.uniform(0.7, 1.3, 9)
    truth[:, 1] += rng.uniform(-0.1, 0.1, 9) * mhz
    truth[:, 2] *= rng.uniform(0.85, 1.15, 9)
    truth[:, 3] = rng.uniform(-0.3, 0.3)
    dt = 1.0 / sw
    truth, t, x = _data(truth, links, 9, n, dt, t0, n_vox, seed, noise)
    return {"x": x, "t": t, "dt": dt, "t0": t0, "truth": truth, "init": init, "lo": lo, "hi": hi, "fixed": fixed,
            "links": links, "mhz": mhz}


def k16_case(n=257, n_vox=4, single_link=False, seed=2, dt=2e-4, t0=3e-4, noise=0.1):
    """orc.kernel_case(16, n) with g fixed.  Default, P = 20 (16 peaks in the small-P staging tier): every damping and
    phase follows peak 0's, and the frequencies form two combs -- even peaks follow peak 0, odd peaks peak 1, at the
    truth's spacing -- so the columns are 16 amplitudes + 2 frequencies + 1 damping + 1 phase.  single_link: only
    peak 9's damping follows peak 4's (P = 63)."""
    K = 16
    c = orc.kernel_case(K, n, seed, dt=dt, t0=t0, noise=noise, n_vox=n_vox, fix_g=True)
    links = no_links(K)
    if single_link:
        _link(links, 9, 4, 2, 1.25, -3.0)
    else:
        for k in range(1, K):
            _link(links, k, 0, 2)
            _link(links, k, 0, 3)
        for k in range(2, K):
            _link(links, k, k % 2, 1, 1.0, c["truth"][k, 1] - c["truth"][k % 2, 1])
    truth, t, x = _data(c["truth"], links, K, n, dt, t0, n_vox, seed, noise)
    init = c["init"].copy()
    if not single_link:  # 20 columns settle within 5 trials from kernel_case's start; this one is further out
        init[:, 0] *= 1.6
        init[:2, 1] += 14.0
        init[0, 2] *= 1.5
        init[0, 3] += 0.5
    return dict(c, x=x, t=t, truth=truth, init=init, links=links)


def n_columns(c):
    return int(_Layout(c["init"], c["lo"], c["hi"], c["fixed"], c["links"]).free.size)


def gpu_cases():
    """name -> case of every shape tests/test_gpu_amares_links.py runs (built once; 4 ... 7 voxels each)."""
    return {
        "doublet_K3_n64": doublet_case(),
        "doublet_negative_scale": doublet_case(scale=-0.5, seed=4),
        "doublet_amplitude_offset": doublet_case(amp_offset=1.5, seed=5, n_vox=4),
        "doublet_root_on_bound": doublet_case(root_on_bound=True, seed=6, n_vox=4),
        "multiplets_K9_n300": multiplet_case(),
        "K16_P20_n257": k16_case(),
        "K16_single_link_n300": k16_case(n=300, single_link=True, seed=7),
    }


STEP_CASES = ("doublet_K3_n64", "doublet_root_on_bound", "multiplets_K9_n300", "K16_P20_n257")
PARITY_CASES = ("doublet_K3_n64", "multiplets_K9_n300")
