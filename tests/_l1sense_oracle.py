"""ORACLE (not product code): wavelet-sparse SENSE restated in numpy complex128 straight from the definition (DESIGN.md
section 24), on the dense matrices of tests/_cgsense_oracle.py and with nothing imported from the package.

* `L1Case`: a `Case` of tests/_cgsense_oracle.py (same trajectory, maps, density, matrices) whose object is sparse -- a
  plateau and two point sources per column -- with 2 % noise; `benefit` is the undersampled 16 x 16 radial case.
* Psi two ways: `psi_matrix` (explicit Kronecker products of the Haar matrices H_{2n} = [H_n (x) [1, 1]; I_n (x) [1, -1]]
  / sqrt 2 and the shift permutation) and `haar` (butterflies in the kernel's order: dims ascending, levels fine to
  coarse, in place, the approximation left at the even positions).  `standard_index` maps one layout to the other.
* `shrink`, `prox`, `power` (the Rayleigh quotient after n power steps from the mask indicator) and `fista`: the
  iteration of the definition verbatim, one column at a time, on any operator of `Case` (dense, staged, staged with
  complex64 rounding at every launch boundary)."""
import collections
import math

import numpy as np

import _cgsense_oracle as cgs
import _grid_oracle as grid
from _cgsense_oracle import c64, rel, same  # noqa: F401  (re-exported)

R = 0.70710678118654752440

# name: (trajectory, matrix, coils, W, density, tikhonov, masked): the five parity cases are those of the CG-SENSE oracle
CASES = {name: cgs.CASES[name] for name in ("radial2d", "masked2d", "random3d", "odd2d", "line1d")}
CASES["benefit"] = (lambda: grid.radial(16, 6, 32), (16, 16), 4, 4, "pipe", 0.0, False)
LEVELS = {"radial2d": (2, 2), "masked2d": (2, 2), "random3d": (2, 2, 0), "odd2d": (2, 1), "line1d": (2,), "benefit": (2, 2)}


def sparse_object(ms, n_cols, rng):
    """[V, T]: per column a plateau of m_d // 4 voxels per dim (at least 1) next to the centre and two point sources inside
    the inscribed disc, complex amplitudes of magnitude about 1."""
    inside = np.argwhere(cgs.disc(ms).reshape(ms) > 0)
    obj = np.zeros(tuple(ms) + (n_cols,), dtype=np.complex128)
    for t in range(n_cols):
        corner = [m // 2 - max(1, m // 4) + int(rng.integers(0, 2)) for m in ms]
        block = tuple(slice(c, c + max(1, m // 4)) for c, m in zip(corner, ms))
        obj[block + (t,)] = np.exp(1j * rng.uniform(0, 2 * math.pi))
        for _ in range(2):
            at = tuple(inside[int(rng.integers(0, len(inside)))])
            obj[at + (t,)] += 1.5 * np.exp(1j * rng.uniform(0, 2 * math.pi))
    return obj.reshape(-1, n_cols) * cgs.disc(ms).reshape(-1, 1)


class L1Case(cgs.Case):
    """The attributes and methods of `Case`; `reg` / `lam` are the Tikhonov weight (relative / absolute)."""

    def __init__(self, name, n_cols=3, seed=0):
        tr, ms, C, W, dens, reg, masked = CASES[name]
        self.name, self.ms, self.C, self.W, self.reg, self.T = name, tuple(ms), C, W, reg, n_cols
        self.levels = LEVELS[name]
        self.traj = tr()
        self.S, self.V = len(self.traj), int(np.prod(ms))
        self.density = dens
        self.w = grid.pipe(self.traj, ms, 2.0, W) if dens == "pipe" else np.ones(self.S)
        self.A, self.Gs = grid.dense_matrix(self.traj, ms, 2.0, W)
        self.F = [grid.image_table(m, G, W) for m, G in zip(ms, self.Gs)]
        K = np.ones((1, 1), dtype=np.complex128)
        for F in self.F:
            K = np.kron(K, F)
        self.K = K
        self.s = cgs.maps(ms, C, masked)
        self.sv = self.s.reshape(C, self.V)
        self.N = self.A.T @ K.conj().T
        self.lam = reg * self.scale()
        self.mask = ((np.abs(self.sv) ** 2).sum(axis=0) > 0)
        rng = np.random.default_rng(2000 + seed + len(name))
        obj = sparse_object(self.ms, n_cols, rng) * self.mask[:, None]
        y = np.einsum("sv,cv,vt->cst", self.N, self.sv, obj)
        noise = rng.standard_normal(y.shape) + 1j * rng.standard_normal(y.shape)
        self.obj, self.y = obj, y + 0.02 * np.abs(y).max() * noise / math.sqrt(2.0)

    def lambda_max(self):
        """The largest eigenvalue of E^H D E + lam I."""
        return float(np.linalg.eigvalsh(self.normal_matrix())[-1])


_CACHE = {}


def case(name, n_cols=3):
    """The shared, read-only instance of a case."""
    key = (name, n_cols)
    if key not in _CACHE:
        _CACHE[key] = L1Case(name, n_cols)
    return _CACHE[key]


def error(x, truth):
    """|x - truth| / |truth| over everything."""
    return float(np.linalg.norm(x - truth) / np.linalg.norm(truth))


# ---- Psi ----------------------------------------------------------------------------------------------------------------
def haar_matrix(l):
    H = np.ones((1, 1))
    for _ in range(l):
        n = len(H)
        H = np.vstack([np.kron(H, [1.0, 1.0]), np.kron(np.eye(n), [1.0, -1.0])]) / math.sqrt(2.0)
    return H


def psi_matrix(ms, levels, shift=None):
    """Psi S as one [V, V] matrix: per dim kron(I, H_{2^l}) after the circular shift (S w)[j] = w[(j + s) mod m]."""
    shift = (0,) * len(ms) if shift is None else shift
    P = np.ones((1, 1))
    for m, l, s in zip(ms, levels, shift):
        S = np.zeros((m, m))
        S[np.arange(m), (np.arange(m) + s) % m] = 1.0
        P = np.kron(P, np.kron(np.eye(m >> l), haar_matrix(l)) @ S)
    return P


def penalised(ms, levels):
    """[V] bool: False for the coefficient at index 0 along every dim of its block (in either layout), True for the rest;
    all True when every level is 0."""
    if not any(levels):
        return np.ones(int(np.prod(ms)), dtype=bool)
    approx = np.ones((), dtype=bool)
    for m, l in zip(ms, levels):
        approx = np.logical_and.outer(approx, np.arange(m) % (1 << l) == 0)
    return ~approx.reshape(-1)


def standard_index(ms, levels):
    """[V] int: where the coefficient that the in-place butterflies leave at a position stands in the layout of
    `psi_matrix`.  In one block of 2^l: position 0 -> 0; position i with j trailing zero bits is detail i >> (j + 1) of
    level j (0 the finest) -> row 2^(l - j - 1) + (i >> (j + 1))."""
    per_dim = []
    for m, l in zip(ms, levels):
        p = np.zeros(1 << l, dtype=np.int64)
        for i in range(1, 1 << l):
            j = (i & -i).bit_length() - 1
            p[i] = (1 << (l - j - 1)) + (i >> (j + 1))
        per_dim.append((np.arange(m) >> l << l) + p[np.arange(m) % (1 << l)])
    flat = np.zeros((), dtype=np.int64)
    for m, idx in zip(ms, per_dim):
        flat = np.add.outer(flat * m, idx)
    return flat.reshape(-1)


def haar(w, ms, levels, shift=None, inverse=False):
    """The blockwise transform of [V, T] by butterflies in the kernel's order, in place: (a + b) r and (a - b) r with r =
    1 / sqrt 2 as one constant, a at the positions whose in-block index is a multiple of 2^(j + 1), b 2^j further."""
    shift = (0,) * len(ms) if shift is None else shift
    a = np.array(w, dtype=np.complex128).reshape(tuple(ms) + (-1,))
    if not inverse:
        a = np.roll(a, [-s for s in shift], axis=tuple(range(len(ms))))
    steps = [(d, j) for d in range(len(ms)) for j in range(levels[d])]
    for d, j in (reversed(steps) if inverse else steps):
        pos = np.arange(ms[d])
        lo = pos[(pos % (1 << levels[d])) % (2 << j) == 0]
        hi = lo + (1 << j)
        a = np.moveaxis(a, d, 0)
        p, q = a[lo].copy(), a[hi].copy()
        a[lo], a[hi] = (p + q) * R, (p - q) * R
        a = np.moveaxis(a, 0, d)
    if inverse:
        a = np.roll(a, list(shift), axis=tuple(range(len(ms))))
    return a.reshape(-1, a.shape[-1])


def shrink(c, theta, pen):
    """c max(0, 1 - theta / |c|) on the penalised coefficients, 0 at c = 0.  theta: [T] or a scalar."""
    mag = np.sqrt(c.real * c.real + c.imag * c.imag)
    theta = np.broadcast_to(theta, c.shape[1:])[None]
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(mag <= theta, 0.0, 1.0 - theta / np.where(mag > 0, mag, 1.0))
    return np.where(pen[:, None], c * f, c)


def prox(w, ms, levels, theta, mask=None, shift=None, kron=False):
    """mask . S^H Psi^H soft(Psi S w, theta) on [V, T]."""
    pen = penalised(ms, levels)
    if kron:
        P = psi_matrix(ms, levels, shift)
        x = P.T @ shrink(P @ w, theta, pen)
    else:
        x = haar(shrink(haar(w, ms, levels, shift), theta, pen), ms, levels, shift, inverse=True)
    return x if mask is None else x * mask[:, None]


# ---- the iteration --------------------------------------------------------------------------------------------------
def power(op, mask, n):
    """Re<v, A v> for the unit vector v after n power steps from the mask indicator (n + 1 applications of `op`)."""
    v = mask.astype(np.complex128)[:, None] / math.sqrt(mask.sum())
    for k in range(n + 1):
        q = op(v)
        quotient = float(np.vdot(v, q).real)
        if k < n:
            v = q / np.linalg.norm(q)
    return quotient


def momentum(n):
    out, tk = [], 1.0
    for _ in range(n):
        nxt = (1.0 + math.sqrt(1.0 + 4.0 * tk * tk)) / 2.0
        out.append((tk - 1.0) / nxt)
        tk = nxt
    return out


Fista = collections.namedtuple("Fista", "x change n_iter status ratios objective")


def fista(op, b, ms, levels, sparsity, tau, iterations, tol=0.0, mask=None, cycle_spin=False, accelerate=True):
    """The iteration of DESIGN.md section 24, every column on its own.  `op`: v [V, 1] -> (E^H D E + lambda2) v.  Returns
    x, change, n_iter, status, per column the list of sqrt(d2 / n2) of every step taken, and per column the list of the
    objective after every step."""
    V, T = b.shape
    mask = np.ones(V, dtype=bool) if mask is None else mask
    pen = penalised(ms, levels)
    x_all = np.zeros((V, T), dtype=np.complex128)
    change, n_iter, status = np.zeros(T), np.zeros(T, dtype=np.int32), np.zeros(T, dtype=np.int32)
    ratios, objective = [], []
    betas = momentum(iterations)
    for t in range(T):
        ratios.append([])
        objective.append([])
        bt = b[:, t:t + 1]
        top = float(np.abs(bt).max()) if np.all(np.isfinite(bt)) else float("nan")
        if not np.isfinite(top):
            status[t], change[t] = 3, np.nan
            x_all[:, t] = np.nan
            continue
        lam_t = sparsity * top
        x = np.zeros((V, 1), dtype=np.complex128)
        v = x.copy()
        d2 = n2 = None

        def test():
            if not (np.isfinite(d2) and np.isfinite(n2)):
                status[t], change[t] = 3, np.nan
                x_all[:, t] = np.nan
                return True
            if d2 <= tol * tol * n2:
                status[t] = 1
            change[t] = 0.0 if d2 == 0 else (math.sqrt(d2 / n2) if n2 > 0 else np.inf)
            return status[t] != 0

        for k in range(iterations):
            if k >= 1 and test():
                break
            g = (op(v) - bt) if k else -bt
            w = v - tau * g
            shift = tuple(k % (1 << l) for l in levels) if cycle_spin else None
            xn = prox(w, ms, levels, tau * lam_t, mask, shift)
            dx = xn - x
            v = xn + (betas[k] if accelerate else 0.0) * dx
            x = xn
            d2, n2 = float(np.vdot(dx, dx).real), float(np.vdot(x, x).real)
            n_iter[t] += 1
            with np.errstate(divide="ignore", invalid="ignore"):
                ratios[t].append(float(np.sqrt(np.float64(d2) / np.float64(n2))))
            coeff = haar(x, ms, levels)
            objective[t].append(float(0.5 * np.vdot(x, op(x)).real - np.vdot(bt, x).real + lam_t * np.abs(coeff[pen]).sum()))
        else:
            if iterations >= 1:
                test()
        if status[t] != 3:
            x_all[:, t] = x[:, 0]
    return Fista(x_all, change, n_iter, status, ratios, objective)


def clear_of(ratios, tol):
    """No step's sqrt(d2 / n2) within a factor 1 +- 1e-6 of `tol`: the stopping test cannot fall either way by rounding."""
    return all(abs(r / tol - 1.0) > 1e-6 for col in ratios for r in col if np.isfinite(r)) if tol > 0 else True


# ---- what the xm_l1_* entry points must refuse before any HIP call (conventions of tests/_cgsense_oracle.py) -------------
START_ORDER = ("b", "bpart", "bmax", "status", "change", "x", "n_vox", "n_cols", "finish")
START_OK = dict(b=1024, bpart=2048, bmax=3072, status=4096, change=5120, x=6144, n_vox=20, n_cols=6, finish=1)
START_REFUSALS = [dict(bpart=None), dict(bmax=None), dict(status=None), dict(change=None), dict(x=None), dict(n_vox=0),
                  dict(n_cols=0), dict(n_vox=1 << 31), dict(n_cols=1 << 31), dict(n_vox=1 << 30, n_cols=1 << 30),
                  dict(bmax="bpart"), dict(change="bmax"), dict(bpart=4), dict(bmax=4), dict(status=2), dict(x=8),
                  dict(finish=0, b=None), dict(finish=0, bpart=None), dict(finish=0, b=8), dict(finish=0, bpart="b")]
PROX_ORDER = ("x", "v", "q", "b", "mask", "bmax", "d2_in", "n2_in", "d2_out", "n2_out", "status_in", "status_out", "n_iter",
              "change", "n_dims", "m0", "m1", "m2", "l0", "l1", "l2", "s0", "s1", "s2", "n_cols", "tau", "theta_scale", "beta",
              "tol", "iteration", "mode")
PROX_OK = dict(x=1024, v=2048, q=3072, b=4096, mask=5120, bmax=6144, d2_in=7168, n2_in=8192, d2_out=9216, n2_out=10240,
               status_in=11264, status_out=12288, n_iter=13312, change=14336, n_dims=2, m0=8, m1=6, m2=1, l0=2, l1=1, l2=0,
               s0=3, s1=1, s2=0, n_cols=6, tau=0.5, theta_scale=0.01, beta=0.3, tol=1e-4, iteration=1, mode=0)
PROX_DOUBLES = ("tau", "theta_scale", "beta", "tol")
PROX_REFUSALS = ([{k: None} for k in PROX_ORDER[:14]] + [
    dict(x="v"), dict(x="q"), dict(v="b"), dict(d2_out="d2_in"), dict(n2_out="d2_out"), dict(status_out="status_in"),
    dict(change="bmax"), dict(x=8), dict(v=8), dict(q=8), dict(b=8), dict(bmax=4), dict(d2_in=4), dict(n2_out=4),
    dict(status_out=2), dict(n_iter=2), dict(change=4),
    dict(n_dims=0), dict(n_dims=4), dict(n_dims=1), dict(m2=2), dict(l2=1), dict(s2=1),
    dict(m0=0), dict(m0=1 << 31), dict(m0=1 << 16, m1=1 << 16, l1=0, s1=0), dict(n_cols=0), dict(n_cols=1 << 31),
    dict(m0=1 << 20, m1=1 << 10, l1=0, s1=0, n_cols=1 << 30),
    dict(m1=7), dict(m0=10), dict(l0=-1), dict(l0=5, m0=32), dict(l0=3, m0=8, l1=2, m1=8), dict(n_dims=3, m2=4, l2=2),
    dict(s0=4), dict(s0=-1), dict(s1=2),
    dict(tau=-1.0), dict(tau=float("nan")), dict(tau=float("inf")), dict(theta_scale=-1e-3), dict(theta_scale=float("nan")),
    dict(beta=-0.1), dict(beta=float("inf")), dict(tol=-1.0), dict(tol=float("nan")), dict(iteration=-1), dict(mode=3),
    dict(mode=-1), dict(mode=2, q=None), dict(mode=0, d2_in=None)])
