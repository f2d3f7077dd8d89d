"""numpy oracle of grappa_calibrate / grappa_fill, complex128.  The product never imports this
module, and this module imports nothing from the product.

Sampling, per dim with n kept lines and acceleration R, N = R n: the kept lines of the full centred k-space are
j = j0 + R l, l = 0 ... n - 1, j0 = N // 2 - R (n // 2) (the rule of section 16).  A full-grid index j has
l = floor((j - j0) / R) (-1 below j0) and o = (j - j0) mod R >= 0.  o = 0 in every dim: acquired, copied.  Any other offset
tuple is a type, indexed row-major over the offsets with the all-zero tuple skipped.

Sources: block sizes b per dim, S = prod b; the neighbours of a position with line indices l are the kept lines l + s,
s = -((b - 1) // 2) ... b // 2 per dim, s row-major; a neighbour outside 0 ... n - 1 is skipped.

Apply: y[c, j, t] = sum_s sum_c' W[type][c][s][c'] a[c', l + s, t], ascending s then ascending c'.  `fill` forms the sum
twice: in float64 with every product and every addition rounded on its own, and in numpy.longdouble.  The unit of an
output is eps64 sum |W| |a| over its terms.

Calibrate: ACS block [C, A..., T]; for a type with offsets o every position p whose S sources p - o + R s lie inside the
block gives one equation per time point; Sm [K, n_eq] (K = C S, rows ordered s then coil), Tm [C, n_eq]; G = Sm Sm^H,
lambda' = lam trace(G) / K; route "normal": W = ((G + lambda' I)^-1 Sm Tm^H)^H by numpy.linalg.solve; route "lstsq":
the least-squares solution of [Sm^H; sqrt(lambda') I] X = [Tm^H; 0] (SVD; G is never formed), W = X^H.  The unit of a
weight is eps64 kappa(G + lambda' I) max |W_type|."""
import functools
import itertools

import numpy as np

EPS = float(np.finfo(np.float64).eps)
EPS32 = float(np.finfo(np.float32).eps)


# ---- the sampling and source rules ---------------------------------------------------------------------------------------
def first_line(n, r):
    return (r * n) // 2 - r * (n // 2)


def kept_lines(n, r):
    """Indices of the full centred k-space (N = r n points) that the undersampled acquisition keeps."""
    return first_line(n, r) + r * np.arange(n)


def split(j, n, r):
    """(l, o) of the full-grid index j: floor division and a non-negative remainder."""
    d = j - first_line(n, r)
    return d // r, d % r  # Python's // and % take the floor


def type_offsets(accel):
    return [o for o in itertools.product(*[range(r) for r in accel]) if any(o)]


def type_index(o, accel):
    """Row-major index of the offset tuple among the types; -1 for the acquired positions."""
    i = 0
    for oa, r in zip(o, accel):
        i = i * r + oa
    return i - 1


def neighbours(kernel):
    """The neighbour tuples s in their defined (row-major) order."""
    return list(itertools.product(*[range(-((b - 1) // 2), b // 2 + 1) for b in kernel]))


def undersample(k, axes, accel):
    """The kept lines of the full k-space `k` along `axes`."""
    for ax, r in zip(axes, accel):
        k = np.take(k, kept_lines(k.shape[ax] // r, r), axis=ax)
    return k


def sources(j, ns, accel, kernel):
    """(type index, [(s index, kept-line tuple)] of the in-range neighbours) of the full-grid position j."""
    lo = [split(ja, n, r) for ja, n, r in zip(j, ns, accel)]
    l, o = [x[0] for x in lo], [x[1] for x in lo]
    if not any(o):
        return -1, [(0, tuple(l))]
    out = []
    for si, s in enumerate(neighbours(kernel)):
        q = tuple(la + sa for la, sa in zip(l, s))
        if all(0 <= qa < n for qa, n in zip(q, ns)):
            out.append((si, q))
    return type_index(o, accel), out


# ---- apply -----------------------------------------------------------------------------------------------------------------
def fill(a, w, accel, kernel):
    """a [C, n..., T] complex128, w [R - 1, C, S, C].  Returns dict(y: the ascending-order float64 sum, alt: the same terms
    summed in longdouble (rounded to complex128 at the end), unit: eps64 sum |W| |a| per output (0 on acquired lines),
    acquired: bool over the full grid)."""
    a = np.asarray(a, dtype=np.complex128)
    c, ns, t = a.shape[0], a.shape[1:-1], a.shape[-1]
    full = tuple(r * n for r, n in zip(accel, ns))
    ld = np.longdouble
    y = np.zeros((c, *full, t), dtype=np.complex128)
    alt = np.zeros((c, *full, t), dtype=np.complex128)
    unit = np.zeros((c, *full, t))
    acquired = np.zeros(full, dtype=bool)
    ar, ai = a.real.copy(), a.imag.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        for j in itertools.product(*[range(m) for m in full]):
            ty, src = sources(j, ns, accel, kernel)
            at = (slice(None), *j)
            if ty < 0:
                y[at] = alt[at] = a[(slice(None), *src[0][1])]
                acquired[j] = True
                continue
            yr, yi = np.zeros((c, t)), np.zeros((c, t))
            lr, li = np.zeros((c, t), dtype=ld), np.zeros((c, t), dtype=ld)
            u = np.zeros((c, t))
            for si, q in src:
                for d in range(c):
                    wr, wi = w[ty, :, si, d].real[:, None], w[ty, :, si, d].imag[:, None]
                    xr, xi = ar[(d, *q)][None, :], ai[(d, *q)][None, :]
                    yr = yr + wr * xr
                    yr = yr - wi * xi
                    yi = yi + wr * xi
                    yi = yi + wi * xr
                    lr = lr + wr.astype(ld) * xr.astype(ld) - wi.astype(ld) * xi.astype(ld)
                    li = li + wr.astype(ld) * xi.astype(ld) + wi.astype(ld) * xr.astype(ld)
                    u = u + (np.abs(wr) + np.abs(wi)) * (np.abs(xr) + np.abs(xi))
            y[at] = yr + 1j * yi
            alt[at] = lr.astype(np.float64) + 1j * li.astype(np.float64)
            unit[at] = EPS * u
    return dict(y=y, alt=alt, unit=unit, acquired=acquired)


def gap(got, want, unit):
    """The largest |got - want| in units; positions whose unit is 0 must agree exactly."""
    d = np.abs(got - want)
    assert not d[unit == 0].any()
    return float((d[unit > 0] / unit[unit > 0]).max()) if (unit > 0).any() else 0.0


def make(shape, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def random_weights(accel, kernel, c, seed):
    """Seeded weights of the size an interpolation has: entries of order 1 / sqrt(K)."""
    r, s = int(np.prod(accel)), int(np.prod(kernel))
    return make((r - 1, c, s, c), seed) / np.sqrt(2.0 * c * s)


# name -> (n per dim, accel, kernel, coils, time points): the shapes where the index arithmetic can go wrong
APPLY_CASES = {
    "1_r2_b4_c3": ((1,), (2,), (4,), 3, 5),          # every neighbour on one side is missing
    "3_r2_b2_c4": ((3,), (2,), (2,), 4, 5),          # j0 = 1: the first full line has l = -1
    "3_r3_b2_c4": ((3,), (3,), (2,), 4, 5),          # an odd N
    "5x4_r2x3_b2x3_c6": ((5, 4), (2, 3), (2, 3), 6, 4),
    "4x3_r1x3_b3x2_c5": ((4, 3), (1, 3), (3, 2), 5, 4),
    "2x3x2_r2x2x2_b2x2x2_c8": ((2, 3, 2), (2, 2, 2), (2, 2, 2), 8, 3),
    "2x2_r4x4_b2x2_c8": ((2, 2), (4, 4), (2, 2), 8, 3),  # R = 16
    "3x3_r2x2_b8x8_c16": ((3, 3), (2, 2), (8, 8), 16, 2),  # S = 64, C S = 1024
    "3x2_r2x2_b2x2_c1": ((3, 2), (2, 2), (2, 2), 1, 4),
    "3x2_r2x2_b2x2_c5": ((3, 2), (2, 2), (2, 2), 5, 4),
    "3x2_r2x2_b2x2_c16": ((3, 2), (2, 2), (2, 2), 16, 3),
    "3x2_r2x2_b2x2_c17": ((3, 2), (2, 2), (2, 2), 17, 3),
    "3x2_r2x1_b2x3_c33": ((3, 2), (2, 1), (2, 3), 33, 2),
    "2x2_r2x1_b2x2_c64": ((2, 2), (2, 1), (2, 2), 64, 2),
}


@functools.lru_cache(maxsize=None)
def apply_case(name, nt=None):
    """(a [C, n..., T], W, accel, kernel, fill(a, W)) of a parity case; `nt`: another number of time points."""
    ns, accel, kernel, c, t = APPLY_CASES[name]
    seed = sum(map(ord, name))
    a = make((c, *ns, nt or t), seed)
    w = random_weights(accel, kernel, c, seed + 1)
    return a, w, accel, kernel, fill(a, w, accel, kernel)


def worst_apply_gap():
    """The largest gap, over the parity cases, between the ascending-order sum and the long-double sum."""
    return max(gap(r["y"], r["alt"], r["unit"]) for r in (apply_case(n)[4] for n in APPLY_CASES))


# ---- calibrate ----------------------------------------------------------------------------------------------------------
def systems(block, accel, kernel, points):
    """Yields (offsets o, Sm [K, n_eq], Tm [C, n_eq]) per type, by explicit loops over the block's positions."""
    block = np.asarray(block, dtype=np.complex128)
    c, shape = block.shape[0], block.shape[1:-1]
    t = min(points, block.shape[-1])
    nb = neighbours(kernel)
    for o in type_offsets(accel):
        cols_s, cols_t = [], []
        for p in itertools.product(*[range(m) for m in shape]):
            src = [tuple(pa - oa + r * sa for pa, oa, r, sa in zip(p, o, accel, s)) for s in nb]
            if not all(0 <= qa < m for q in src for qa, m in zip(q, shape)):
                continue
            for ti in range(t):
                cols_s.append(np.concatenate([block[(slice(None), *q, ti)] for q in src]))
                cols_t.append(block[(slice(None), *p, ti)])
        k = c * len(nb)
        sm = np.array(cols_s).T if cols_s else np.zeros((k, 0), dtype=np.complex128)
        tm = np.array(cols_t).T if cols_t else np.zeros((c, 0), dtype=np.complex128)
        yield o, sm, tm


def calibrate(block, accel, kernel, points=8, lam=1e-4, route="normal"):
    """dict(w [R - 1, C, S, C], n_eq, kappa (of G + lambda' I), residual, unit (per type)) of an ACS block."""
    c, s = np.asarray(block).shape[0], int(np.prod(kernel))
    ws, n_eq, kappa, residual, unit = [], [], [], [], []
    for o, sm, tm in systems(block, accel, kernel, points):
        k = sm.shape[0]
        g = sm @ sm.conj().T
        lp = lam * np.trace(g).real / k
        gl = g + lp * np.eye(k)
        if route == "normal":
            x = np.linalg.solve(gl, sm @ tm.conj().T)
        else:
            lhs = np.concatenate([sm.conj().T, np.sqrt(lp) * np.eye(k)])
            rhs = np.concatenate([tm.conj().T, np.zeros((k, c))])
            x = np.linalg.lstsq(lhs, rhs, rcond=None)[0]
        w = x.conj().T
        ev = np.linalg.eigvalsh(gl)
        ws.append(w.reshape(c, s, c))
        n_eq.append(sm.shape[1])
        kappa.append(float(ev[-1] / ev[0]))
        residual.append(float(np.linalg.norm(w @ sm - tm) / np.linalg.norm(tm)))
        unit.append(EPS * kappa[-1] * float(np.abs(w).max()))
    return dict(w=np.array(ws).reshape(len(ws), c, s, c), n_eq=n_eq, kappa=kappa, residual=residual, unit=unit)


def calibration_gap(a, b):
    """The largest disagreement of two calibrations' weights, per type in the first one's units."""
    return max(float(np.abs(x - y).max()) / u for x, y, u in zip(a["w"], b["w"], a["unit"]))


# ---- seeded end-to-end cases --------------------------------------------------------------------------------------------
def make_sens(c, full, seed):
    import _sense_oracle

    return _sense_oracle.make_sens(c, full, seed)


def make_object(full, t, seed):
    """An ellipse with a smaller ellipse inside, each times its own seeded complex time course: [N..., T]."""
    rng = np.random.default_rng(seed)
    axes = np.meshgrid(*[np.linspace(-1.0, 1.0, n) if n > 1 else np.zeros(1) for n in full], indexing="ij")
    outer = sum((x / 0.8) ** 2 for x in axes) <= 1.0
    inner = sum(((x - 0.15) / 0.35) ** 2 for x in axes) <= 1.0
    co = rng.standard_normal(t) + 1j * rng.standard_normal(t)
    ci = rng.standard_normal(t) + 1j * rng.standard_normal(t)
    return outer[..., None] * co + inner[..., None] * ci


def to_kspace(img, axes):
    return np.fft.fftshift(np.fft.fftn(np.fft.ifftshift(img, axes=axes), axes=axes, norm="ortho"), axes=axes)


# name -> (n kept per dim, accel, kernel, coils, ACS size per dim, lam): the four cases of the issue, three time points each
E2E_CASES = {
    "16x32_r2x1_b2x3_c8": ((16, 32), (2, 1), (2, 3), 8, (12, 12), 1e-6),
    "16x16_r2x2_b2x2_c12": ((16, 16), (2, 2), (2, 2), 12, (14, 14), 1e-6),
    "16x16_r2x2_b4x3_c8": ((16, 16), (2, 2), (4, 3), 8, (16, 16), 1e-4),
    "11x30_r3x1_b2x3_c8": ((11, 30), (3, 1), (2, 3), 8, (14, 14), 1e-6),
}
E2E_POINTS = 3


@functools.lru_cache(maxsize=None)
def e2e_case(name):
    """dict(full [C, N..., T] true k-space, kept, acs (the central block of the full grid), accel, kernel, lam, coils)."""
    ns, accel, kernel, c, acs, lam = E2E_CASES[name]
    full = tuple(r * n for r, n in zip(accel, ns))
    seed = sum(map(ord, name))
    img = make_sens(c, full, seed)[..., None] * make_object(full, E2E_POINTS, seed + 1)[None]
    axes = list(range(1, 1 + len(ns)))
    k = to_kspace(img, axes)
    centre = tuple(slice(m // 2 - s // 2, m // 2 - s // 2 + s) for m, s in zip(full, acs))
    return dict(full=k, kept=undersample(k, axes, accel), acs=np.ascontiguousarray(k[(slice(None), *centre)]), accel=accel,
                kernel=kernel, lam=lam, coils=c)


def score(filled, true, acquired):
    """||filled - true|| / ||true|| over the missing lines."""
    miss = ~acquired
    return float(np.linalg.norm((filled - true)[:, miss]) / np.linalg.norm(true[:, miss]))


@functools.lru_cache(maxsize=None)
def e2e_oracle(name, route="normal"):
    """(calibration, fill result, score) of an end-to-end case in the oracle."""
    cs = e2e_case(name)
    cal = calibrate(cs["acs"], cs["accel"], cs["kernel"], points=8, lam=cs["lam"], route=route)
    res = fill(cs["kept"], cal["w"], cs["accel"], cs["kernel"])
    return cal, res, score(res["y"], cs["full"], res["acquired"])


def worst_calibration_gap():
    """The largest gap between the two routes over the end-to-end cases."""
    return max(calibration_gap(e2e_oracle(n)[0], e2e_oracle(n, "lstsq")[0]) for n in E2E_CASES)
