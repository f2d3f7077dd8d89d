"""numpy oracle of unfold_sense, complex128.  The product never imports this module, and this module
imports nothing from the product.

Sampling: per dim with n acquired lines and acceleration R, N = R n, the kept lines of the full centred k-space are
N // 2 + R (l - n // 2); the aliased image is a_c[p] = (1 / sqrt(R)) sum_k s_c[q_k(p)] rho[q_k(p)] with
q_k(p) = (p - n // 2 + N // 2 + k n) mod N.  Several dims: the group of p is the tuple product of the q's, the member
index runs row-major over (k_1, k_2, k_3).

Unfolding of one group by two routes, S the C x Ra matrix of the active members, Sw = W S (W = L^-1, Psi = L L^H):
  "chol":  A = Sw^H Sw, lambda' = lam trace(A) / Ra, B = (A + lambda' I)^-1 Sw^H through numpy's Cholesky factor;
  "lstsq": B = the first C columns of pinv([Sw; sqrt(lambda') I]) (SVD; the normal equations are never formed).
U = sqrt(R) B W, rho[q_k] = U[k] a[p], g[q_k] = sqrt((B B^H)_kk A_kk).  Status: 0 unfolded; 1 a masked member, or any member
of a group with no active one; 2 a non-finite sensitivity or data sample in the group; 3 a Cholesky pivot <= 0 or
non-finite, and always Ra > C at lam = 0 (rho 0 and g NaN for the whole group in 2 and 3; 2 wins over 3).

The unit of an output sample is eps64 kappa(A + lambda' I) sum_c |U[k, c]| |a_c[p, t]|; of g, eps64 kappa(A + lambda' I) g."""
import functools
import itertools

import numpy as np

EPS = float(np.finfo(np.float64).eps)
EPS32 = float(np.finfo(np.float32).eps)


def kept_lines(n, r):
    """Indices of the full centred k-space (N = r n points) that the undersampled acquisition keeps."""
    big = r * n
    return big // 2 + r * (np.arange(n) - n // 2)


def members(n, r):
    """q[p, k]: the r full-FOV indices that fold onto the reduced index p."""
    big = r * n
    return (np.arange(n)[:, None] - n // 2 + big // 2 + np.arange(r)[None, :] * n) % big


def groups(ns, rs):
    """Yields (p, [q_0, ..., q_{R-1}]): reduced voxel (a tuple) and its members (tuples), member index row-major."""
    qs = [members(n, r) for n, r in zip(ns, rs)]
    for p in itertools.product(*[range(n) for n in ns]):
        yield p, [tuple(int(qs[d][p[d], k[d]]) for d in range(len(ns))) for k in itertools.product(*[range(r) for r in rs])]


def forward(rho, sens, rs):
    """Aliased coil images [C, n..., T] of the object rho [N..., T] seen through sens [C, N...]."""
    d = len(rs)
    ns = [big // r for big, r in zip(rho.shape[:d], rs)]
    a = np.zeros((sens.shape[0], *ns, rho.shape[-1]), dtype=np.complex128)
    for p, qq in groups(ns, rs):
        for q in qq:
            a[(slice(None), *p)] += sens[(slice(None), *q)][:, None] * rho[q][None, :]
    return a / np.sqrt(np.prod(rs))


def undersample(k, axes, rs):
    """The kept lines of the full k-space `k` along `axes`."""
    for ax, r in zip(axes, rs):
        k = np.take(k, kept_lines(k.shape[ax] // r, r), axis=ax)
    return k


def linv_of(psi):
    return np.linalg.inv(np.linalg.cholesky(np.asarray(psi, dtype=np.complex128)))


def random_psd(c, seed):
    rng = np.random.default_rng(seed)
    m = rng.standard_normal((c, 2 * c)) + 1j * rng.standard_normal((c, 2 * c))
    return m @ m.conj().T / (2 * c) + 0.5 * np.eye(c)


def solve_group(s, w=None, lam=0.0, route="chol"):
    """One group: s the C x R sensitivities of all its members.  Returns dict(active, U [Ra, C] or None, g [Ra], status of
    the group (0, 1, 3; non-finite sensitivities: 2), kappa of A + lambda' I, pivots (relative to A's diagonal))."""
    r = s.shape[1]
    if not np.all(np.isfinite(s)):
        return dict(active=np.zeros(r, bool), U=None, g=None, status=2, kappa=np.nan, pivots=None)
    active = np.any(s != 0, axis=0)
    ra = int(active.sum())
    if ra == 0:
        return dict(active=active, U=None, g=None, status=1, kappa=np.nan, pivots=None)
    if ra > s.shape[0] and not lam > 0.0:  # more unknowns than coils: singular whatever the rounding does
        return dict(active=active, U=None, g=None, status=3, kappa=np.inf, pivots=None)
    sw = s[:, active] if w is None else w @ s[:, active]
    a = sw.conj().T @ sw
    lp = lam * np.trace(a).real / ra
    al = a + lp * np.eye(ra)
    with np.errstate(all="ignore"):
        try:
            chol = np.linalg.cholesky(al)
            ok = bool(np.all(np.isfinite(chol)))
        except np.linalg.LinAlgError:
            ok = False
    if not ok:
        return dict(active=active, U=None, g=None, status=3, kappa=np.inf, pivots=None)
    kappa = float(np.linalg.cond(al))
    if route == "chol":
        z = np.linalg.solve(chol, sw.conj().T)
        b = np.linalg.solve(chol.conj().T, z)
        adiag = np.diag(a).real
    else:
        assert route == "lstsq"
        aug = np.vstack([sw, np.sqrt(lp) * np.eye(ra)])
        b = np.linalg.pinv(aug, rcond=1e-15)[:, :sw.shape[0]]
        adiag = np.linalg.norm(sw, axis=0) ** 2
    u = np.sqrt(r) * (b if w is None else b @ w)
    g = np.sqrt(np.sum(np.abs(b) ** 2, axis=1) * adiag)
    pivots = np.diag(chol).real ** 2 / np.diag(al).real
    return dict(active=active, U=u, g=g, status=0, kappa=kappa, pivots=pivots)


def unfold(a, sens, rs, psi=None, lam=0.0, route="chol", w=None, da=None):
    """a [C, n..., T], sens [C, N...] -> dict(rho [N..., T], g [N...], status [N...], unit [N..., T] (eps kappa sum |U| |a|),
    gunit [N...], kappa [n...], pivot [n...] (the smallest relative Cholesky pivot of the group)).  `w`: L^-1 in place of
    `psi`.  `da`: bounds on the error of `a` (a's shape); then also prop [N..., T] = sum_c |U[k, c]| da_c, what they can
    grow to in rho."""
    a = np.asarray(a, dtype=np.complex128)
    sens = np.asarray(sens, dtype=np.complex128)
    d = len(rs)
    ns = a.shape[1:1 + d]
    full = tuple(n * r for n, r in zip(ns, rs))
    assert sens.shape == (a.shape[0], *full), (sens.shape, a.shape, rs)
    w = (None if psi is None else linv_of(psi)) if w is None else np.asarray(w, dtype=np.complex128)
    t = a.shape[-1]
    rho = np.zeros((*full, t), dtype=np.complex128)
    unit, prop = np.zeros((*full, t)), np.zeros((*full, t))
    g, gunit = np.zeros(full), np.zeros(full)
    status = np.zeros(full, dtype=np.int32)
    kappa, pivot = np.full(ns, np.nan), np.full(ns, np.nan)
    for p, qq in groups(ns, rs):
        s = np.stack([sens[(slice(None), *q)] for q in qq], axis=1)
        ap = a[(slice(None), *p)]  # [C, T]
        sol = solve_group(s, w, lam, route)
        st = sol["status"]
        if st in (0, 3) and not np.all(np.isfinite(ap)):
            st = 2
        kappa[p] = sol["kappa"]
        if st != 0:
            for q in qq:
                status[q] = st
                g[q] = 0.0 if st == 1 else np.nan
            continue
        pivot[p] = sol["pivots"].min()
        out = sol["U"] @ ap
        un = EPS * sol["kappa"] * (np.abs(sol["U"]) @ np.abs(ap))
        pr = np.abs(sol["U"]) @ da[(slice(None), *p)] if da is not None else np.zeros_like(un)
        j = 0
        for q, on in zip(qq, sol["active"]):
            if not on:
                status[q] = 1
                continue
            rho[q], unit[q], prop[q], g[q], gunit[q] = out[j], un[j], pr[j], sol["g"][j], EPS * sol["kappa"] * sol["g"][j]
            j += 1
    return dict(rho=rho, g=g, status=status, unit=unit, gunit=gunit, kappa=kappa, pivot=pivot, prop=prop)


def gap(a, b, u):
    """The largest |a - b| in units of u (samples with u = 0 must agree exactly)."""
    dlt = np.abs(np.asarray(a) - np.asarray(b))
    ok = np.broadcast_to(u, dlt.shape) > 0
    assert not dlt[~ok].any()
    return float((dlt / np.where(u > 0, u, 1.0))[ok].max()) if ok.any() else 0.0


def make_sens(c, full, seed, mask=None):
    """Smooth complex sensitivities [C, N...]: a Gaussian magnitude around a coil centre outside or at the edge of the
    grid, times a linear phase; `mask` (bool [N...], True = keep) zeroes the other voxels in every coil."""
    rng = np.random.default_rng(seed)
    axes = np.meshgrid(*[np.linspace(-1.0, 1.0, n) if n > 1 else np.zeros(1) for n in full], indexing="ij")
    out = np.empty((c, *full), dtype=np.complex128)
    for i in range(c):
        ctr = rng.uniform(-1.2, 1.2, len(full))
        slope = rng.uniform(-3.0, 3.0, len(full))
        r2 = sum((x - m) ** 2 for x, m in zip(axes, ctr))
        ph = sum(k * x for x, k in zip(axes, slope)) + rng.uniform(0, 2 * np.pi)
        out[i] = (0.2 + rng.random()) * np.exp(-r2 / 0.8) * np.exp(1j * ph)
    if mask is not None:
        out = out * mask[None]
    return out


def make(shape, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


# name -> (n per dim, accel per dim, coils, time points)
PARITY_CASES = {
    "4x5_r2x1_c4": ((4, 5), (2, 1), 4, 9),
    "5x3_r2x3_c12": ((5, 3), (2, 3), 12, 7),
    "3x4_r3x2_c8": ((3, 4), (3, 2), 8, 7),
    "2x2_r4x4_c32": ((2, 2), (4, 4), 32, 5),
    "2x3x2_r2x2x2_c16": ((2, 3, 2), (2, 2, 2), 16, 5),
    "7x5_r1x1_c64": ((7, 5), (1, 1), 64, 6),
    "3_r1_c1": ((3,), (1,), 1, 6),
}


@functools.lru_cache(maxsize=None)
def parity_case(name):
    """(rho [N..., T], sens [C, N...], a [C, n..., T] from the forward model, accel); read-only."""
    ns, rs, c, t = PARITY_CASES[name]
    seed = sorted(PARITY_CASES).index(name)
    full = tuple(n * r for n, r in zip(ns, rs))
    rho = make((*full, t), 100 + seed)
    sens = make_sens(c, full, 200 + seed)
    a = forward(rho, sens, rs)
    for v in (rho, sens, a):
        v.setflags(write=False)
    return rho, sens, a, rs


@functools.lru_cache(maxsize=None)
def parity_routes(name):
    rho, sens, a, rs = parity_case(name)
    return unfold(a, sens, rs, route="chol"), unfold(a, sens, rs, route="lstsq")


def route_gaps(name):
    """(gap of rho, gap of g) between the two routes, in their units."""
    x, y = parity_routes(name)
    assert np.array_equal(x["status"], y["status"])
    return gap(x["rho"], y["rho"], x["unit"]), gap(x["g"], y["g"], x["gunit"])


def worst_route_gap():
    return max(max(route_gaps(name)) for name in PARITY_CASES)
