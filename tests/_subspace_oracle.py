"""ORACLE (not product code): temporal-subspace SENSE restated in numpy complex128 straight from the definition (DESIGN.md
section 26), on the dense pieces of tests/_cgsense_oracle.Case and with nothing imported from the package.

* `Problem`: the seeded problem -- four damped lines mixed into a rank-3 temporal subspace, T = 48, the object inside the
  disc, 1 % noise, ``sampling = rng.uniform(size=(S, T)) < keep`` -- on one of the CG-SENSE cases.
* three routes: `solve` (the dense normal matrix, a direct solve), `folded` (the oracle's `cg` on the state folded to
  [V R, F], dense or staged operator) and the staged operator with complex64 rounding at every launch boundary.
* `project`, `mix`, `expand`: the three kernels as sums, with the sum of the terms' magnitudes their bounds are made of.
* the tables of what the xm_sub_* entry points must refuse before any HIP call."""
import math

import numpy as np

import _cgsense_oracle as cg

T, R = 48, 3
KEEPS = (1.0, 0.5, 0.25)


def basis_of(G, rank):
    """The first `rank` right singular vectors of G [n, T]: orthonormal rows."""
    return np.ascontiguousarray(np.linalg.svd(G, full_matrices=False)[2][:rank])


class Problem:
    def __init__(self, name, keep=1.0, n_frames=1, n_time=T, rank=R, seed=0):
        c = cg.case(name)
        self.c, self.name, self.keep, self.F, self.T, self.R = c, name, keep, n_frames, n_time, rank
        rng = np.random.default_rng(7000 + seed + len(name))
        t = np.arange(n_time) / n_time
        damp, freq = rng.uniform(1.0, 4.0, 4), rng.uniform(-8.0, 8.0, 4)
        lines = np.exp((-damp[:, None] + 2j * math.pi * freq[:, None]) * t[None, :])  # [4, T]
        mixing = rng.standard_normal((rank, 4)) + 1j * rng.standard_normal((rank, 4))
        shapes = mixing @ lines  # [R, T]: the temporal functions of the object
        self.V = basis_of(shapes, rank)  # [R, T]
        amp = (rng.standard_normal((c.V, rank, n_frames)) + 1j * rng.standard_normal((c.V, rank, n_frames)))
        amp = amp * cg.disc(c.ms).reshape(-1, 1, 1)
        self.truth = np.einsum("vrf,rt->vft", amp, shapes)  # [V, F, T], inside span(V)
        y = np.einsum("sv,cv,vft->csft", c.N, c.sv, self.truth)
        noise = rng.standard_normal(y.shape) + 1j * rng.standard_normal(y.shape)
        self.full = y + 0.01 * np.abs(y).max() * noise / math.sqrt(2.0)  # [C, S, F, T], every position
        self.m = rng.uniform(size=(c.S, n_time)) < keep
        self.y = self.full * self.m[None, :, None, :]
        self.K = kernel(self.V, self.m)
        self.kappa = kappa(self.K, c.w)
        self.lam = c.reg * c.scale() * self.kappa
        self.s_rep = np.repeat(c.sv, rank, axis=1)  # [C, V R]

    # ---- the dense route ---------------------------------------------------------------------------------------------
    def normal_matrix(self, lam=None):
        """[V R, V R], index v R + r."""
        c = self.c
        M = np.zeros((c.V, self.R, c.V, self.R), dtype=np.complex128)
        for k in range(c.C):
            E = c.N * c.sv[k][None, :]
            M += np.einsum("sv,s,srp,su->vrup", E.conj(), c.w, self.K, E)
        n = c.V * self.R
        return M.reshape(n, n) + (self.lam if lam is None else lam) * np.eye(n)

    def rhs(self, b=None):
        """E^H D b as [V R, F]."""
        c = self.c
        b = project(self.y, self.V, self.m) if b is None else b
        out = np.zeros((c.V, self.R, self.F), dtype=np.complex128)
        for k in range(c.C):
            out += np.einsum("sv,s,srf->vrf", (c.N * c.sv[k][None, :]).conj(), c.w, b[k])
        return out.reshape(c.V * self.R, self.F)

    def solve(self):
        return np.linalg.solve(self.normal_matrix(), self.rhs()).reshape(self.c.V, self.R, self.F)

    def dense(self):
        M = self.normal_matrix()
        return lambda p: M @ p

    # ---- the staged route: expand, forward, mix, adjoint, reduce; `rnd` where the GPU has a launch boundary -------------
    def staged(self, rnd=cg.same):
        c, r = self.c, self.R

        def op(p):  # [V R, F]
            f = p.shape[1]
            u = rnd(self.s_rep[:, :, None] * p[None, :, :]).reshape(c.C, c.V, r * f)
            z = rnd(mix(c.forward(u, rnd).reshape(c.C, c.S, r, f), self.K))
            q = c.adjoint(z.reshape(c.C, c.S, r * f), rnd).reshape(c.C, c.V * r, f)
            return cg.reduce_coils(self.s_rep, q) + self.lam * p
        return op

    def staged_rhs(self, rnd=cg.same, y=None):
        c, r = self.c, self.R
        b = rnd(project(rnd(self.y if y is None else y), self.V, self.m))
        return cg.reduce_coils(self.s_rep, c.adjoint(b.reshape(c.C, c.S, r * self.F), rnd).reshape(c.C, c.V * r, self.F))

    def folded(self, op, b, iterations, tol=0.0):
        """(U [V, R, F], residual, n_iter, status): the coupled recurrence, frames as the columns of `cg`."""
        x, residual, n_iter, status = cg.cg(op, b, iterations, tol)
        return x.reshape(self.c.V, self.R, self.F), residual, n_iter, status

    def image(self, U):
        return expand(U, self.V)

    # ---- what the package offers without the feature: CG-SENSE (a direct solve), every time point on its own ------------
    def per_column(self, y):
        c = self.c
        M = c.normal_matrix()
        b = cg.reduce_coils(c.sv, c.adjoint(y.reshape(c.C, c.S, self.F * self.T)))
        return np.linalg.solve(M, b).reshape(c.V, self.F, self.T)


def kernel(V, m):
    """K_s[r, r'] = sum_t m[s, t] conj(V[r, t]) V[r', t]."""
    return np.einsum("st,rt,pt->srp", m.astype(np.float64), V.conj(), V)


def kappa(K, w):
    r = K.shape[1]
    return float((w * np.einsum("srr->s", K).real).sum() / (r * w.sum()))


def project(y, V, m=None):
    """y [C, S, F, T] -> b [C, S, R, F]; an unsampled position is selected out, not multiplied."""
    if m is not None:
        y = np.where(m[None, :, None, :], y, 0.0)
    return np.einsum("rt,csft->csrf", V.conj(), y)


def mix(a, K):
    """a [C, S, R, F] -> z."""
    return np.einsum("srp,cspf->csrf", K, a)


def expand(U, V):
    """U [V, R, F] -> x [V, F, T]."""
    return np.einsum("vrf,rt->vft", U, V)


def err(x, truth):
    """Relative L2 error."""
    return float(np.linalg.norm(x - truth) / np.linalg.norm(truth))


# ---- the kernels' bounds: a sum of n products carries at most (n + 4) 2^-53 sum |terms|, plus the final rounding -------------
def _wide(a):
    return np.asarray(a.real, dtype=np.longdouble), np.asarray(a.imag, dtype=np.longdouble)


def contract(spec, a, b, conj_a=False):
    """(value, sum of |terms|) of einsum(spec, a, b) for complex a, b in extended precision: value complex as a (re, im)
    pair of longdouble arrays, the magnitudes per component likewise."""
    ar, ai = _wide(a)
    br, bi = _wide(b)
    if conj_a:
        ai = -ai
    e = lambda x, y: np.einsum(spec, x, y)  # noqa: E731
    re, im = e(ar, br) - e(ai, bi), e(ar, bi) + e(ai, br)
    mre = e(np.abs(ar), np.abs(br)) + e(np.abs(ai), np.abs(bi))
    mim = e(np.abs(ar), np.abs(bi)) + e(np.abs(ai), np.abs(br))
    return (re, im), (mre, mim)


def bound(n_products, magnitude, value, out_dtype):
    """(n + 4) 2^-53 sum |terms| + half an ulp of the output dtype at the value."""
    half_ulp = 2.0 ** -24 if np.dtype(out_dtype) == np.complex64 else 2.0 ** -53
    tiny = float(np.finfo(np.float32 if np.dtype(out_dtype) == np.complex64 else np.float64).smallest_subnormal)
    return (n_products + 4) * 2.0 ** -53 * magnitude + half_ulp * np.abs(value) + tiny


def within(got, value, magnitude, n_products, out_dtype):
    """The largest error of `got` over its bound, both components (<= 1 passes)."""
    worst = 0.0
    for g, v, mag in ((got.real, value[0], magnitude[0]), (got.imag, value[1], magnitude[1])):
        d = np.abs(np.asarray(g, dtype=np.longdouble) - v)
        worst = max(worst, float(np.max(d / bound(n_products, mag, v, out_dtype))))
    return worst


# ---- what the xm_sub_* entry points must refuse before any HIP call (the conventions of _cgsense_oracle: a pointer entry
# is None, the name of another argument, or an offset in bytes from the valid pointer) ----------------------------------------
BIG = 1 << 20
PROJECT_ORDER = ("y", "b", "basis", "sampling", "n_coils", "n_samples", "n_frames", "n_time", "rank", "coil_stride",
                 "sample_stride", "frame_stride", "dtype")
PROJECT_OK = dict(y=1 << 20, b=2 << 20, basis=3 << 20, sampling=4 << 20, n_coils=4, n_samples=5, n_frames=2, n_time=48, rank=3,
                  coil_stride=5 * 2 * 48, sample_stride=2 * 48, frame_stride=48, dtype=0)  # (sizes and strides < 1024)
PROJECT_REFUSALS = [dict(y=None), dict(b=None), dict(basis=None), dict(b="y"), dict(b="basis"), dict(b="sampling"),
                    dict(b=64 - (1 << 20)), dict(y=4), dict(b=4), dict(dtype=1, y=8), dict(basis=8), dict(rank=0), dict(rank=33),
                    dict(rank=-1), dict(n_time=0), dict(n_time=2, rank=3), dict(n_coils=0), dict(n_samples=0), dict(n_frames=0),
                    dict(n_samples=1 << 31), dict(n_coils=BIG, n_samples=BIG, n_frames=BIG),
                    dict(coil_stride=1 << 49, sample_stride=1 << 49), dict(coil_stride=-1), dict(sample_stride=-48),
                    dict(frame_stride=-1), dict(dtype=2), dict(dtype=-1)]
MIX_ORDER = ("a", "z", "kernel", "n_coils", "n_samples", "n_frames", "rank", "dtype")
MIX_OK = dict(a=1 << 20, z=2 << 20, kernel=3 << 20, n_coils=4, n_samples=20, n_frames=2, rank=3, dtype=0)
MIX_REFUSALS = [dict(a=None), dict(z=None), dict(kernel=None), dict(z="kernel"), dict(z=64 - (1 << 20)), dict(z=-64 - (1 << 20)),
                dict(a=4), dict(z=4), dict(dtype=1, a=8), dict(kernel=8), dict(rank=0), dict(rank=33), dict(n_coils=0),
                dict(n_samples=0), dict(n_frames=0), dict(n_frames=1 << 31), dict(n_coils=BIG, n_samples=BIG, n_frames=BIG),
                dict(dtype=2), dict(dtype=-1)]
EXPAND_ORDER = ("u", "basis", "x", "n_vox", "n_frames", "n_time", "rank")
EXPAND_OK = dict(u=1 << 20, basis=2 << 20, x=3 << 20, n_vox=20, n_frames=2, n_time=48, rank=3)
EXPAND_REFUSALS = [dict(u=None), dict(basis=None), dict(x=None), dict(x="u"), dict(x="basis"), dict(x=64 - (2 << 20)), dict(u=8),
                   dict(basis=8), dict(x=8), dict(rank=0), dict(rank=33), dict(n_time=0), dict(n_time=2, rank=3), dict(n_vox=0),
                   dict(n_frames=0), dict(n_vox=1 << 31), dict(n_vox=BIG, n_frames=BIG, n_time=BIG)]


_CACHE = {}


def problem(name, keep=1.0, n_frames=1):
    """The shared, read-only instance of a problem."""
    key = (name, keep, n_frames)
    if key not in _CACHE:
        _CACHE[key] = Problem(name, keep, n_frames)
    return _CACHE[key]
