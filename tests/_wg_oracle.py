"""numpy restatement of the workgroup toolbox (xmris_amd/csrc/xm_wg.h), the oracle of tests/test_wg.py and
tests/test_gpu_wg.py: the fixed tree of wg_sum, the two Gram maps, the round-robin pairing, a plain row-cyclic Jacobi in
fp64, lmfit's transforms and a Cholesky solve in np.longdouble (80-bit, eps 1.08e-19), the row-after-row sums of lm_normal
(xm_lm.h), and the matrix families the GPU tests run.  tests/test_wg.py pins every piece before it judges a kernel."""
import numpy as np

EPS = np.finfo(np.float64).eps
LD = np.longdouble
CLD = np.clongdouble
NT = 256  # XM_WG_NT
MAXE = 9  # XM_WG_MAXE
MAXB = 9  # XM_WG_MAXB
SWEEPS = 30  # XM_WG_SWEEPS
MAXC = 64
MAXP = 80
FIXED, FREE, LO, HI, TWO = range(5)  # XM_WG_FIXED ...


# ---- block sum ----------------------------------------------------------------------------------------------------------
def tree_sum(rows):
    """rows [n, 256] fp64 -> [n]: red[t] += red[t + h] for h = 128, 64, ... 1, every addition rounded to fp64."""
    red = np.array(rows, dtype=np.float64)
    assert red.shape[-1] == NT
    h = NT // 2
    with np.errstate(all="ignore"):
        while h:
            red[..., :h] = red[..., :h] + red[..., h:2 * h]
            h //= 2
    return red[..., 0].copy()


# ---- Gram maps ------------------------------------------------------------------------------------------------------------
def upper_pairs(n):
    """The upper triangle of an n x n matrix in row-major order."""
    return [(i, j) for i in range(n) for j in range(i, n)]


def gram_entries(c):
    """(ci, cj) [256, MAXE]: thread t's m-th entry is number t + 256 m of the row-major upper triangle, (0, 0) past it."""
    pairs = upper_pairs(c)
    ci, cj = np.zeros((NT, MAXE), np.int32), np.zeros((NT, MAXE), np.int32)
    for t in range(NT):
        for m in range(MAXE):
            e = t + NT * m
            if e < len(pairs):
                ci[t, m], cj[t, m] = pairs[e]
    return ci, cj


def gram_slices(nb):
    """(nblk, S): blocks of the upper triangle of nb x nb, and the slices each tile's points are cut into."""
    nblk = nb * (nb + 1) // 2
    return nblk, (4 if nblk < 4 else 1)


def gram_items(nb):
    """(bi, bj, sl) [4 waves, MAXB]: wave v's m-th item is number v + 4 m, item = slice * nblk + block.  Slots at or past
    nblk * S items wrap around (their accumulators are never stored)."""
    nblk, _ = gram_slices(nb)
    pairs = upper_pairs(nb)
    out = np.zeros((3, 4, MAXB), np.int32)
    for v in range(4):
        for m in range(MAXB):
            item = v + 4 * m
            out[0, v, m], out[1, v, m] = pairs[item % nblk]
            out[2, v, m] = item // nblk
    return out[0], out[1], out[2]


# ---- round-robin pairing ------------------------------------------------------------------------------------------------
def pairing(c):
    """The sweep of wg_jacobi: a list of players - 1 steps, each a list of ceil(c / 2) pairs (p, q), p < q.  A pair with
    q >= c holds the bye of an odd c and is not rotated."""
    n_pairs = (c + 1) // 2
    players = 2 * n_pairs
    steps = []
    for step in range(players - 1):
        pairs = []
        for t in range(n_pairs):
            a = players - 1 if t == 0 else (step + t) % (players - 1)
            b = step if t == 0 else (step - t + players - 1) % (players - 1)
            pairs.append((min(a, b), max(a, b)))
        steps.append(pairs)
    return steps


# ---- plain row-cyclic Jacobi, fp64 ---------------------------------------------------------------------------------------
def hermitian(a):
    """The Hermitian matrix the upper triangle of `a` stands for (what wg_mirror leaves): the diagonal real, the lower
    triangle the conjugate of the upper one, bit for bit."""
    u = np.triu(a, 1)
    return u + np.swapaxes(u.conj(), -1, -2) + np.real(np.diagonal(a, axis1=-2, axis2=-1))[..., None] * np.eye(a.shape[-1])


def jacobi(gs, sweeps=SWEEPS):
    """gs [B, C, C] Hermitian complex128 -> (lam [B, C], V [B, C, C], sweeps done [B]).  Pairs in row-cyclic order
    (0, 1), (0, 2) ... (C - 2, C - 1), one at a time, the B matrices side by side.  The rotation of a pair with
    G_pq = h e^{i phi} is J = [[c, s e^{i phi}], [-s e^{-i phi}, c]], tau = (G_qq - G_pp) / (2 h),
    t = sign(tau) / (|tau| + sqrt(1 + tau^2)); columns p, q of G and V times J, then rows p, q of G times J^H, whole rows
    and columns at once (plain products with c and s, not the kernel's Rutishauser form).  A matrix stops when
    off(G) <= eps ||G||_F at the start of a sweep."""
    g = np.array(gs, dtype=np.complex128)
    nb, c, _ = g.shape
    v = np.broadcast_to(np.eye(c, dtype=np.complex128), g.shape).copy()
    fro = np.sqrt(np.sum(np.abs(g) ** 2, axis=(1, 2)))
    done = np.zeros(nb, int)
    idx = np.arange(c)
    rot2 = np.empty((nb, 2, 2), np.complex128)
    for sweep in range(sweeps + 1):
        off = np.sqrt(np.sum(np.abs(np.where(np.eye(c, dtype=bool), 0.0, g)) ** 2, axis=(1, 2)))
        live = off > EPS * fro
        if not live.any() or sweep == sweeps:
            done[live] = sweeps + 1
            break
        done[live] = sweep + 1
        for p in range(c - 1):
            for q in range(p + 1, c):
                gpq = g[:, p, q]
                h = np.abs(gpq)
                rot = live & (h > 0)
                if not rot.any():
                    continue
                hs = np.where(rot, h, 1.0)
                gpp, gqq = g[:, p, p].real.copy(), g[:, q, q].real.copy()
                with np.errstate(over="ignore"):  # (a huge tau: t = 0, as in the kernel)
                    tau = (gqq - gpp) / (2.0 * hs)
                    t = np.where(tau >= 0, 1.0, -1.0) / (np.abs(tau) + np.sqrt(1.0 + tau * tau))
                t = np.where(rot, t, 0.0)
                cs = 1.0 / np.sqrt(1.0 + t * t)
                se = (t * cs) * (gpq.real / hs + 1j * (gpq.imag / hs))  # s e^{i phi}
                rot2[:, 0, 0] = rot2[:, 1, 1] = cs
                rot2[:, 0, 1], rot2[:, 1, 0] = se, -np.conj(se)
                pq = [p, q]
                g[:, :, pq] = g[:, :, pq] @ rot2
                v[:, :, pq] = v[:, :, pq] @ rot2
                g[:, pq, :] = np.conj(rot2.transpose(0, 2, 1)) @ g[:, pq, :]
                z = np.where(rot, 0.0, g[:, p, q])
                g[:, p, q], g[:, q, p] = z, np.conj(z)
                g[:, p, p], g[:, q, q] = gpp - t * h, gqq + t * h
    return g[:, idx, idx].real.copy(), v, done


FAMILIES = ("gram", "rank_one", "imaginary", "graded")


def jacobi_family(name, c, seed):
    """One Hermitian c x c matrix (complex128, exactly Hermitian, real diagonal):
    gram       A A^H of a random c x (c + 3) complex A;
    rank_one   v v^H + 1e-3 I: c - 1 equal eigenvalues, so 2 x 2 blocks with equal diagonal entries (tau = 0);
    imaginary  a real diagonal and purely imaginary off-diagonal entries (phi = +-pi / 2 in every rotation);
    graded     D A D with D = diag(2^-k), A a well-conditioned Gram matrix: entries over 2 (c - 1) binades."""
    rng = np.random.default_rng([seed, c, FAMILIES.index(name)])
    cx = lambda *s: rng.standard_normal(s) + 1j * rng.standard_normal(s)  # noqa: E731
    if name == "gram":
        a = cx(c, c + 3)
        g = a @ a.conj().T
    elif name == "rank_one":
        x = cx(c)
        g = np.outer(x, x.conj()) + 1e-3 * np.eye(c)
    elif name == "imaginary":
        k = rng.standard_normal((c, c))
        g = 1j * (k - k.T) + np.diag(rng.standard_normal(c))
    else:
        a = cx(c, 2 * c + 3)
        d = np.ldexp(1.0, -np.arange(c))
        g = (a @ a.conj().T / (2 * c + 3)) * np.outer(d, d)  # (powers of two: exact)
    return hermitian(g)


def jacobi_cases(c, seed=0):
    """[4, c, c]: one matrix of every family."""
    return np.stack([jacobi_family(f, c, seed) for f in FAMILIES])


def eig_quality(g, lam, v):
    """In longdouble, for one problem: (residual max |G V - V diag(lam)|, max |V^H V - I|), the first in units of
    eps64 ||G||_F, the second in units of eps64 (it has no scale: V is unitary whatever G's size)."""
    gl, vl = g.astype(CLD), v.astype(CLD)
    fro = np.sqrt(np.sum(np.abs(gl) ** 2))
    res = np.abs(gl @ vl - vl * lam.astype(LD)[None, :]).max()
    orth = np.abs(vl.conj().T @ vl - np.eye(g.shape[0])).max()
    return float(res / (EPS * fro)) if fro > 0 else 0.0, float(orth / EPS)


def off_units(g0, g1):
    """Off-diagonal Frobenius norm of the returned g1 in units of eps64 ||g0||_F, in longdouble."""
    off = np.sqrt(np.sum(np.abs(np.where(np.eye(g1.shape[0], dtype=bool), 0, g1.astype(CLD))) ** 2))
    fro = np.sqrt(np.sum(np.abs(g0.astype(CLD)) ** 2))
    return float(off / (EPS * fro)) if fro > 0 else 0.0


def jacobi_reference(c, seed=0):
    """What numpy shows on jacobi_cases(c): the worst (residual, orthonormality) of np.linalg.eigh and of `jacobi`, and the
    oracle's largest sweep count."""
    gs = jacobi_cases(c, seed)
    lam_j, v_j, done = jacobi(gs)
    worst = [0.0, 0.0]
    for k, g in enumerate(gs):
        lam_e, v_e = np.linalg.eigh(g)
        for lam, v in ((lam_e, v_e), (lam_j[k], v_j[k])):
            r, o = eig_quality(g, lam, v)
            worst = [max(worst[0], r), max(worst[1], o)]
    return worst[0], worst[1], int(done.max())


# ---- Levenberg-Marquardt leaves ------------------------------------------------------------------------------------------
def from_internal(bt, u, lo, hi):
    """lmfit's transforms in longdouble: (p, dp/du) of arrays bt, u, lo, hi."""
    u, lo, hi = (np.asarray(a, dtype=np.float64).astype(LD) for a in (u, lo, hi))
    bt = np.asarray(bt)
    r = np.sqrt(u * u + 1)
    half = (hi - lo) / 2
    with np.errstate(invalid="ignore"):  # (the unused branches of rows without bounds)
        p = np.select([bt == TWO, bt == LO, bt == HI], [lo + (np.sin(u) + 1) * half, lo - 1 + r, hi + 1 - r], u)
        s = np.select([bt == TWO, bt == LO, bt == HI], [np.cos(u) * half, u / r, -u / r], LD(1))
    return p, s


def to_internal(bt, v, lo, hi):
    """The inverse, in longdouble; v clipped into its bounds (whatever the type: FREE and FIXED come with -inf, inf)."""
    v, lo, hi = (np.asarray(a, dtype=np.float64).astype(LD) for a in (v, lo, hi))
    bt = np.asarray(bt)
    vc = np.minimum(np.maximum(v, lo), hi)
    with np.errstate(invalid="ignore", divide="ignore"):
        two = np.arcsin(np.clip(2 * (vc - lo) / (hi - lo) - 1, -1, 1))
        one = np.sqrt(np.maximum((vc - lo + 1) ** 2 - 1, 0))
        other = np.sqrt(np.maximum((hi - vc + 1) ** 2 - 1, 0))
    return np.select([bt == TWO, bt == LO, bt == HI], [two, one, other], vc)


def transform_grid():
    """(bt, u, lo, hi, v) fp64 arrays of one length: every bounded type over |u| up to 1e8, lo and hi of either sign and of
    magnitudes 1e-6 ... 1e6, and v on, next to (1, 2 and 1000 ulps, and 1e-9 ... 0.5 of the width or of 1) and far from
    (1 ... 1e6 away) a bound, a few v outside the bounds among them."""
    rng = np.random.default_rng(5)
    mags = (1e-6, 1e-3, 0.3, 1.0, 7.0, 1e3, 1e6)
    bounds = [(-b, a) for a in mags for b in mags] + [(a, a + w) for a in mags for w in mags]
    bounds += [(-a - w, -a) for a in mags for w in mags]
    us = np.concatenate([[0.0], np.ldexp(1.0, np.arange(-30, 27, 3)), 10.0 ** np.arange(-8, 9), rng.uniform(0, 7, 12),
                         np.pi / 2 * np.arange(1, 9), np.nextafter(np.pi / 2, [0.0, 4.0])])
    us = np.concatenate([us, -us])
    rows = []
    for lo, hi in bounds:
        w = hi - lo
        near = [0.0, 1e-9, 1e-6, 1e-3, 0.1, 0.5]
        far = [1.0, 3.0, 1e2, 1e4, 1e6]
        for bt in (LO, HI, TWO):
            edge = lo if bt != HI else hi
            sign = 1.0 if bt != HI else -1.0
            vs = [edge, np.nextafter(edge, sign * np.inf), edge + sign * 2 * np.spacing(abs(edge)),
                  edge + sign * 1000 * np.spacing(abs(edge)), edge - sign * 0.5 * max(abs(edge), 1.0)]
            if bt == TWO:
                vs += [lo + f * w for f in near] + [hi - f * w for f in near] + [hi, np.nextafter(hi, np.inf), hi + w]
                vs += [lo + d for d in far if d < w - 1.0] + [hi - d for d in far if d < w - 1.0]
            else:
                vs += [edge + sign * f for f in near] + [edge + sign * d for d in far]
            k = max(len(vs), len(us))
            for i in range(k):
                rows.append((bt, us[i % len(us)], lo, hi, vs[i % len(vs)]))
    for bt in (FREE, FIXED):
        for i, u in enumerate(us):
            rows.append((bt, u, -np.inf, np.inf, u))
    a = np.array(rows, dtype=np.float64)
    return a[:, 0].astype(np.int32), a[:, 1].copy(), a[:, 2].copy(), a[:, 3].copy(), a[:, 4].copy()


def transform_scale(lo, hi, *vals):
    """The unit of a transform's error: eps64 x the largest magnitude the formula forms."""
    lo, hi = np.asarray(lo, dtype=LD), np.asarray(hi, dtype=LD)
    bounds = [np.where(np.isfinite(x), np.abs(x), 0) for x in (lo, hi, hi - lo)]  # (-inf, inf: no bound, nothing formed)
    m = np.maximum.reduce(bounds + [np.abs(np.asarray(x, dtype=LD)) for x in vals])
    return EPS * np.maximum(m, 1)


def lm_scale(d):
    return np.where(d > 0, d, 1.0)


LM_STAGE_BYTES = 65536  # XM_LM_STAGE_BYTES
# every branch of lm_normal (xm_lm.h): ne = (P + 1)(P + 2) / 2 - 1 entries over 256 threads, and the tiers of q_pts
LM_NORMAL_P = (1,    # ne = 2: almost every lane idle
               21,   # ne = 252: the last size with one entry per thread
               22,   # ne = 275: the first with two
               31,   # the highest P of the tier q_pts = 128
               32,   # the lowest of q_pts = 64
               63,   # the highest of q_pts = 64
               64,   # the lowest of q_pts = 32
               80)   # ne = 3320: all 13 entries per thread in use, the last one partly


def lm_q_pts(p):
    """Points per staging round of lm_normal at P = p: 128, 64 or 32 so that 2 q (p + 1) doubles fit the staging budget."""
    q = 128
    while q > 32 and 2 * q * (p + 1) * 8 > LM_STAGE_BYTES:
        q //= 2
    return q


def lm_normal_cases(p, n_points, n=3, seed=0):
    """[n, n_points, 2, p + 1] fp64, the staged rows [J | r] the probe's model copies: normal values, every column scaled
    by its own power of ten over four decades, so that a swapped (i, j) or a dropped row changes every sum."""
    rng = np.random.default_rng([seed, p, n_points])
    scale = 10.0 ** rng.uniform(-2.0, 2.0, (n, 1, 1, p + 1))
    return rng.standard_normal((n, n_points, 2, p + 1)) * scale


def lm_normal(rows):
    """rows [n_rows, p + 1] fp64, the staged rows of one problem in order -> the (p + 1) x (p + 1) matrix of lm_normal's
    sums: every entry starts at 0 and takes a[r][i] * a[r][j] row after row, the product rounded before it is added.
    Its upper triangle is what the kernel owns: [:p, :p] above the diagonal H, the diagonal hd, [:p, p] g."""
    a = np.asarray(rows, dtype=np.float64)
    acc = np.zeros((a.shape[1], a.shape[1]))
    for r in a:
        acc = acc + np.outer(r, r)
    return acc


CHOL_LAMS = (0.0, 1e-3, 1e3)


def cholesky_case(p, k, seed=0):
    """(H [p, p], g [p]) fp64 of problem k: H = J^T J of a random 3p x p matrix J, g = J^T r of a random r.  J's columns
    are scaled by 10^e, e even over -2 ... 2: the squared column norms, H's diagonal and Marquardt's scales dsc, cover eight
    decades.  (Column norms over eight decades would put sixteen into cond(H), beyond the cond <= 1e12 at which the
    longdouble reference is exact to fp64.)"""
    rng = np.random.default_rng([seed, p, k])
    scale = 10.0 ** rng.permutation(np.linspace(-2.0, 2.0, p) if p > 1 else np.array([2.0 * (-1) ** k]))
    j = rng.standard_normal((3 * p, p)) * scale
    return j.T @ j, j.T @ rng.standard_normal(3 * p)


def cholesky_cases(p, n=2, seed=0):
    """(h, hd, dsc, g, lam) of the n x len(CHOL_LAMS) problems of size p, as the probe takes them: h [m, p, p] with the
    upper triangle filled and NaN on and below the diagonal (never read), hd = dsc = the diagonal."""
    hs, gs, lams = [], [], []
    for k in range(n):
        h, g = cholesky_case(p, k, seed)
        for lam in CHOL_LAMS:
            hs.append(h)
            gs.append(g)
            lams.append(lam)
    h = np.array(hs)
    hd = np.diagonal(h, axis1=1, axis2=2).copy()
    up = np.where(np.triu(np.ones((p, p), bool), 1), h, np.nan)
    return up, hd, hd.copy(), np.array(gs), np.array(lams)


def damped(h_upper, hd, dsc, lam):
    """H + lam diag(scale(dsc)) of one problem in longdouble, from the upper triangle and hd."""
    u = np.triu(np.nan_to_num(h_upper), 1).astype(LD)
    return u + u.T + np.diag(hd.astype(LD) + LD(lam) * lm_scale(dsc).astype(LD))


def cholesky_ld(m):
    """Lower Cholesky factor of a longdouble matrix, column by column."""
    p = m.shape[0]
    low = np.zeros((p, p), LD)
    for j in range(p):
        d = np.sqrt(m[j, j] - np.sum(low[j, :j] ** 2))
        low[j, j] = d
        if j + 1 < p:
            low[j + 1:, j] = (m[j + 1:, j] - low[j + 1:, :j] @ low[j, :j]) / d
    return low


def solve_ld(m, g):
    """m^-1 g in longdouble through cholesky_ld."""
    low, p = cholesky_ld(m), m.shape[0]
    y = np.zeros(p, LD)
    for j in range(p):
        y[j] = (LD(g[j]) - low[j, :j] @ y[:j]) / low[j, j]
    for j in range(p - 1, -1, -1):
        y[j] = (y[j] - low[j + 1:, j] @ y[j + 1:]) / low[j, j]
    return y


def cholesky_quality(m, g, low, x):
    """For one problem, a factor `low` and a solution `x` in fp64 against the longdouble ones: (max |L L^T - M| in units of
    eps64 ||M||_F, max |x - x_ref| in units of eps64 cond(M) max |x_ref|, cond(M))."""
    cond = float(np.linalg.cond(m.astype(np.float64)))
    ll = low.astype(LD)
    fac = np.abs(ll @ ll.T - m).max() / (EPS * np.sqrt(np.sum(m * m)))
    ref = solve_ld(m, g)
    sol = np.abs(x.astype(LD) - ref).max() / (EPS * cond * np.abs(ref).max())
    return float(fac), float(sol), cond


def substitute64(low, g):
    """(L L^T)^-1 g in fp64 by forward and back substitution with numpy's dot products."""
    p = len(g)
    y = np.zeros(p)
    for j in range(p):
        y[j] = (g[j] - low[j, :j] @ y[:j]) / low[j, j]
    for j in range(p - 1, -1, -1):
        y[j] = (y[j] - low[j + 1:, j] @ y[j + 1:]) / low[j, j]
    return y


def cholesky_reference(p, n=2, seed=0):
    """What numpy shows in fp64 on cholesky_cases(p): the worst factor error of np.linalg.cholesky, the worst solution error
    of that factor with `substitute64` and of np.linalg.solve (the larger), and the largest cond(H + lam D)."""
    up, hd, dsc, g, lam = cholesky_cases(p, n, seed)
    worst = [0.0, 0.0, 0.0]
    for k in range(len(lam)):
        m = damped(up[k], hd[k], dsc[k], lam[k])
        m64 = m.astype(np.float64)
        low = np.linalg.cholesky(m64)
        fac, sol, cond = cholesky_quality(m, g[k], low, substitute64(low, g[k]))
        _, sol2, _ = cholesky_quality(m, g[k], low, np.linalg.solve(m64, g[k]))
        worst = [max(worst[0], fac), max(worst[1], sol, sol2), max(worst[2], cond)]
    return tuple(worst)
