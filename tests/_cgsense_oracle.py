"""ORACLE (not product code): CG-SENSE restated in numpy complex128 straight from the definition,
on the dense matrices of tests/_grid_oracle.py and with nothing imported from the package.

* `Case`: a seeded problem -- trajectory, smooth sensitivities, density, an object inside the inscribed disc, data with
  1 % noise -- with the dense operator pieces: A (gridding, unit density), K (the Kronecker product of the per-dim [m, G]
  image tables), so that nufft_forward = A^T K^H and nufft_adjoint(density w) = K A diag(w).
* `cg`: the recurrences of the definition verbatim, one column at a time, every scalar per column.
* three routes for the operator: `dense` (one matrix product per stage), `staged(csr=True)` (every sparse stage as the
  CSR sum, one term at a time), `staged(rnd=c64)` (every coil-sized intermediate rounded to complex64 where the GPU has
  a launch boundary).  Their disagreements are what the tolerances are made from (tests/tool_cgsense_tolerance.py).
* `solve`: the normal equations by a direct solve."""
import math

import numpy as np

import _grid_oracle as grid

FLOOR = 1e-14


def c64(a):
    return np.asarray(a).astype(np.complex64).astype(np.complex128)


def same(a):
    return a


def maps(ms, n_coils, masked=False):
    """Gaussian-profile sensitivities [C, *ms] with coil centres on a circle (a line in 1-D) around the field of view and
    a phase per coil, normalised to sum_c |s_c|^2 = 1; `masked`: zero outside the inscribed disc."""
    d = len(ms)
    axes = [(np.arange(m) - m // 2) / m for m in ms]  # [-1/2, 1/2)
    pos = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1)  # [*ms, d]
    s = np.zeros((n_coils,) + tuple(ms), dtype=np.complex128)
    for c in range(n_coils):
        a = 2 * math.pi * c / n_coils
        centre = np.array([0.6 * math.cos(a), 0.6 * math.sin(a), 0.5 * math.cos(2 * a)][:d])
        s[c] = np.exp(-((pos - centre) ** 2).sum(axis=-1) / (2 * 0.45 ** 2)) * np.exp(1j * (0.7 * c + 1.3 * pos[..., 0]))
    s = s / np.sqrt((np.abs(s) ** 2).sum(axis=0))
    if masked:
        s = s * disc(ms)
    return s


def disc(ms):
    """1 inside the inscribed disc (ball) of the field of view, 0 outside; in 1-D the inner 80 %."""
    axes = [(np.arange(m) - m // 2) / m for m in ms]
    pos = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1)
    if len(ms) == 1:
        return (np.abs(pos[..., 0]) <= 0.4).astype(np.float64)
    return ((pos ** 2).sum(axis=-1) <= 0.25 * (1 - 1e-9)).astype(np.float64)


# name: (trajectory, matrix, coils, W, density, regularization, masked)
CASES = {
    "radial2d": (lambda: grid.radial(8, 7, 16), (8, 8), 4, 4, "pipe", 0.05, False),
    "masked2d": (lambda: grid.radial(8, 7, 16), (8, 8), 4, 4, "pipe", 0.05, True),
    "random3d": (lambda: grid.random((4, 4, 4), 96, 3, 5), (4, 4, 4), 6, 4, "pipe", 0.05, False),
    "line1d": (lambda: grid.random(8, 12, 1, 2), (8,), 3, 6, None, 0.05, False),
    "long1d": (lambda: grid.random(40, 60, 1, 7), (40,), 3, 4, "pipe", 0.05, False),
    "odd2d": (lambda: grid.random((8, 6), 70, 2, 11), (8, 6), 4, 4, "pipe", 0.05, False),  # V = 48: three voxel blocks
}


class Case:
    def __init__(self, name, n_cols=3, seed=0):
        tr, ms, C, W, dens, reg, masked = CASES[name]
        self.name, self.ms, self.C, self.W, self.reg, self.T = name, tuple(ms), C, W, reg, n_cols
        self.traj = tr()
        self.S, self.V = len(self.traj), int(np.prod(ms))
        self.density = dens
        self.w = grid.pipe(self.traj, ms, 2.0, W) if dens == "pipe" else np.ones(self.S)
        self.A, self.Gs = grid.dense_matrix(self.traj, ms, 2.0, W)  # [cells, S], unit density
        self.F = [grid.image_table(m, G, W) for m, G in zip(ms, self.Gs)]
        K = np.ones((1, 1), dtype=np.complex128)
        for F in self.F:
            K = np.kron(K, F)
        self.K = K  # [V, cells]
        self.s = maps(ms, C, masked)
        self.sv = self.s.reshape(C, self.V)
        self.N = self.A.T @ K.conj().T  # nufft_forward [S, V]
        self.lam = reg * self.scale()
        rng = np.random.default_rng(1000 + seed + len(name))
        obj = (rng.standard_normal((self.V, n_cols)) + 1j * rng.standard_normal((self.V, n_cols))) * disc(ms).reshape(-1, 1)
        y = np.einsum("sv,cv,vt->cst", self.N, self.sv, obj)
        noise = rng.standard_normal(y.shape) + 1j * rng.standard_normal(y.shape)
        self.obj, self.y = obj, y + 0.01 * np.abs(y).max() * noise / math.sqrt(2.0)

    # ---- lambda --------------------------------------------------------------------------------------------------------
    def scale(self):
        """(sum_j w_j / V) mean_p sum_c |s_c[p]|^2 over the voxels that are not masked."""
        e = (np.abs(self.sv) ** 2).sum(axis=0)
        return float(self.w.sum() / self.V) * float(e[e > 0].mean())

    def normal_matrix(self, lam=None):
        """sum_c diag(conj s_c) N^H D N diag(s_c) + lam I, [V, V]."""
        G = self.N.conj().T @ (self.w[:, None] * self.N)
        M = sum(np.conj(self.sv[c])[:, None] * G * self.sv[c][None, :] for c in range(self.C))
        return M + (self.lam if lam is None else lam) * np.eye(self.V)

    def mean_diagonal(self):
        """The true mean diagonal of E^H D E over the voxels that are not masked."""
        e = (np.abs(self.sv) ** 2).sum(axis=0)
        return float(np.diag(self.normal_matrix(0.0)).real[e > 0].mean())

    # ---- the two chains, stage by stage -----------------------------------------------------------------------------
    def adjoint(self, y, rnd=same, csr=False):
        """[C, S, T] -> coil images [C, V, T]: gridding with the density, then F per dim; `rnd` after every stage."""
        sparse = grid.apply_csr if csr else grid.apply_dense
        g = rnd(sparse(self.A * self.w[None, :], y, 1))
        g = g.reshape((self.C,) + self.Gs + (y.shape[2],))
        for a, F in enumerate(self.F):
            g = rnd(grid.apply_dense_complex(F, g, 1 + a))
        return g.reshape(self.C, self.V, y.shape[2])

    def forward(self, u, rnd=same, csr=False):
        """coil images [C, V, T] -> [C, S, T]: F^H per dim, then degridding."""
        sparse = grid.apply_csr if csr else grid.apply_dense
        g = u.reshape((self.C,) + self.ms + (u.shape[2],))
        for a, F in enumerate(self.F):
            g = rnd(grid.apply_dense_complex(F.conj().T, g, 1 + a))
        g = g.reshape(self.C, -1, u.shape[2])
        return rnd(sparse(self.A.T, g, 1))

    def rhs(self, y=None, rnd=same, csr=False):
        """b = sum_c conj(s_c) adjoint(y_c), ascending c."""
        u = self.adjoint(rnd(self.y if y is None else y), rnd, csr)
        return reduce_coils(self.sv, u)

    def dense(self):
        M = self.normal_matrix()
        return lambda p: M @ p

    def staged(self, rnd=same, csr=False):
        """p [V, T] -> (E^H D E + lam I) p through expand, forward, adjoint and reduce."""
        def op(p):
            u = rnd(self.sv[:, :, None] * p[None, :, :])
            return reduce_coils(self.sv, self.adjoint(self.forward(u, rnd, csr), rnd, csr)) + self.lam * p
        return op

    def solve(self, b=None):
        return np.linalg.solve(self.normal_matrix(), self.rhs() if b is None else b)


def reduce_coils(sv, u):
    q = np.zeros(u.shape[1:], dtype=np.complex128)
    for c in range(sv.shape[0]):
        q = q + np.conj(sv[c])[:, None] * u[c]
    return q


def cg(op, b, iterations, tol=0.0):
    """The recurrences of DESIGN.md section 21, every column on its own: (x, residual, n_iter, status)."""
    V, T = b.shape
    x = np.zeros((V, T), dtype=np.complex128)
    residual, n_iter, status = np.zeros(T), np.zeros(T, dtype=np.int32), np.zeros(T, dtype=np.int32)
    limit = max(tol, FLOOR) ** 2
    for t in range(T):
        r = b[:, t].copy()
        p = r.copy()
        rho0 = rho = float(np.vdot(r, r).real)
        if not np.isfinite(rho0):
            status[t], residual[t] = 3, np.nan
            x[:, t] = np.nan
            continue
        for _ in range(iterations + 1):
            if rho <= limit * rho0:
                status[t] = 1
                break
            if n_iter[t] == iterations:
                break
            q = op(p[:, None])[:, 0]
            delta = float(np.vdot(p, q).real)
            if not (delta > 0 and np.isfinite(delta)):
                status[t] = 2
                break
            alpha = rho / delta
            x[:, t] += alpha * p
            r = r - alpha * q
            new = float(np.vdot(r, r).real)
            p = r + (new / rho) * p
            rho = new
            n_iter[t] += 1
        residual[t] = math.sqrt(rho / rho0) if rho0 > 0 else 0.0
    return x, residual, n_iter, status


def rel(a, b):
    """max |a - b| / max |b|."""
    return float(np.abs(a - b).max() / np.abs(b).max())


_CACHE = {}


def case(name, n_cols=3):
    """The shared, read-only instance of a case."""
    key = (name, n_cols)
    if key not in _CACHE:
        _CACHE[key] = Case(name, n_cols)
    return _CACHE[key]


# ---- what the xm_cgs_* entry points must refuse before any HIP call ------------------------------------------------------
# changes to a valid call: a pointer entry is None (null), the name of another argument (the same address) or an integer
# offset in bytes from the valid pointer
EXPAND_ORDER = ("r", "p", "s", "u", "rho_new", "rho_old", "status", "n_coils", "n_vox", "n_cols", "first", "dtype")
EXPAND_OK = dict(r=1024, p=2048, s=3072, u=4096, rho_new=5120, rho_old=6144, status=7168, n_coils=4, n_vox=20, n_cols=6,
                 first=0, dtype=0)
EXPAND_REFUSALS = [dict(r=None), dict(p=None), dict(s=None), dict(u=None), dict(rho_new=None), dict(rho_old=None),
                   dict(status=None), dict(n_coils=0), dict(n_vox=0), dict(n_cols=0), dict(n_cols=1 << 31), dict(n_vox=1 << 31),
                   dict(n_coils=1 << 20, n_vox=1 << 20, n_cols=1 << 20), dict(dtype=2), dict(dtype=-1), dict(p="r"), dict(u="s"),
                   dict(u="p"), dict(r=8), dict(p=8), dict(s=8), dict(u=4), dict(dtype=1, u=8), dict(rho_new=4), dict(status=2)]
REDUCE_ORDER = ("u", "s", "p", "q", "part", "n_coils", "n_vox", "n_cols", "lam", "initial", "dtype")
REDUCE_OK = dict(u=1024, s=2048, p=3072, q=4096, part=5120, n_coils=4, n_vox=20, n_cols=6, lam=0.1, initial=0, dtype=0)
REDUCE_REFUSALS = [dict(u=None), dict(s=None), dict(p=None), dict(q=None), dict(part=None), dict(n_coils=0), dict(n_vox=-1),
                   dict(n_cols=0), dict(n_cols=1 << 31), dict(n_coils=1 << 20, n_vox=1 << 20, n_cols=1 << 20), dict(dtype=3),
                   dict(q="p"), dict(q="u"), dict(part="u"), dict(lam=-1.0), dict(lam=float("nan")), dict(lam=float("inf")),
                   dict(u=4), dict(dtype=1, u=8), dict(q=8), dict(part=4)]
STEP_ORDER = ("x", "r", "p", "q", "rho", "rho0", "delta", "rho_out", "status_in", "status_out", "n_iter", "residual", "n_vox",
              "n_cols", "tol", "iteration", "final")
STEP_OK = dict(x=1024, r=2048, p=3072, q=4096, rho=5120, rho0=6144, delta=7168, rho_out=8192, status_in=9216, status_out=10240,
               n_iter=11264, residual=12288, n_vox=20, n_cols=6, tol=1e-6, iteration=1, final=0)
STEP_REFUSALS = [dict(x=None), dict(r=None), dict(p=None), dict(q=None), dict(rho=None), dict(rho0=None), dict(delta=None),
                 dict(rho_out=None), dict(status_in=None), dict(status_out=None), dict(n_iter=None), dict(residual=None),
                 dict(n_vox=0), dict(n_cols=0), dict(n_vox=1 << 31), dict(n_vox=1 << 30, n_cols=1 << 30), dict(tol=-1.0),
                 dict(tol=float("nan")), dict(iteration=-1), dict(x="p"), dict(r="q"), dict(rho_out="rho"), dict(rho_out="rho0"),
                 dict(status_out="status_in"), dict(x="r"), dict(x=8), dict(rho_out=4), dict(status_out=2), dict(residual=4)]
