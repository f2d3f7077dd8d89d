"""TEST ORACLE (not product code) of espirit_maps, by the dense route: the calibration matrix built
row by row, ``numpy.linalg.svd`` of it, g_j(q) evaluated at every voxel from the singular vectors themselves, H(q) =
(1 / S) sum_j g_j g_j^H and ``numpy.linalg.eigh``.  It does not use the package's autocorrelation coefficients.

Cases: C ring coils with a Gaussian magnitude and a linear phase, normalised to sum_c |s_c|^2 = 1 and with coil 0 real
and positive (the convention of the maps: truth and estimate compare without a free phase); the object is an ellipse
plus a small insert whose amplitude changes between time points; the k-space is the centred ortho transform of the coil
images plus complex noise of standard deviation 1e-3; the ACS is its central block."""
import functools
import itertools

import numpy as np

import _mrsi_oracle as mrsi_orc
import _sense_oracle as sense_orc

NOISE = 1e-3
# name -> (matrix, coils, ACS block, kernel, time points, threshold)
CASES = {
    "disc2d": ((32, 32), 8, (16, 16), (5, 5), 2, 0.02),
    "rect2d": ((24, 20), 5, (12, 10), (4, 3), 2, 0.03),
    "line1d": ((30,), 3, (16,), (6,), 2, 0.02),
    "box3d": ((10, 8, 6), 4, (6, 6, 6), (3, 3, 3), 2, 0.02),
}


def grid(mat):
    return np.meshgrid(*[(np.arange(n) - n // 2) / (n / 2.0) for n in mat], indexing="ij")


def coil_centres(d, c):
    """Coil positions outside the field of view: on a line (1 dim), a ring (2 dims), a ring that alternates in z (3)."""
    if d == 1:
        return np.linspace(-1.4, 1.4, c)[:, None]
    ang = 2.0 * np.pi * (np.arange(c) + 0.25) / c
    ring = np.stack([1.4 * np.cos(ang), 1.4 * np.sin(ang)], axis=1)
    if d == 2:
        return ring
    return np.concatenate([ring, (0.7 * (-1.0) ** np.arange(c))[:, None]], axis=1)


def true_maps(mat, c, width=2.2, twist=0.7):
    """[C, N...] complex128: sum_c |s_c|^2 = 1 at every voxel, coil 0 real and positive."""
    r = grid(mat)
    s = np.empty((c, *mat), dtype=np.complex128)
    for i, pos in enumerate(coil_centres(len(mat), c)):
        d2 = sum((ra - pa) ** 2 for ra, pa in zip(r, pos))
        unit = pos / np.linalg.norm(pos) if np.linalg.norm(pos) > 0 else pos
        s[i] = np.exp(-d2 / (2.0 * width ** 2)) * np.exp(1j * twist * sum(ra * ua for ra, ua in zip(r, unit)))
    s /= np.sqrt((np.abs(s) ** 2).sum(axis=0))
    return s * np.exp(-1j * np.angle(s[0]))


def true_object(mat, t):
    """(rho [N..., T] complex128, the ellipse's mask [N...])."""
    r = grid(mat)
    axes, off = (0.75, 0.6, 0.7)[:len(mat)], (0.25, -0.2, 0.1)[:len(mat)]
    body = sum((ra / a) ** 2 for ra, a in zip(r, axes)) <= 1.0
    insert = sum((ra - o) ** 2 for ra, o in zip(r, off)) <= 0.2 ** 2
    rho = np.empty((*mat, t), dtype=np.complex128)
    for k in range(t):
        rho[..., k] = (body * 1.0 + insert * (0.5 - 0.3 * k)) * np.exp(0.4j * k)
    return rho, body


def centre_block(k, block):
    """The central block of the centred k-space k [C, N..., T]: index N // 2 sits at A // 2."""
    sl = [slice(n // 2 - a // 2, n // 2 - a // 2 + a) for n, a in zip(k.shape[1:-1], block)]
    return k[(slice(None), *sl, slice(None))]


class Case:
    def __init__(self, name):
        self.name = name
        self.mat, self.C, self.block, self.kernel, self.T, self.threshold = CASES[name]
        self.d = len(self.mat)
        self.s = true_maps(self.mat, self.C)
        self.rho, self.mask = true_object(self.mat, self.T)
        img = self.s[..., None] * self.rho[None]
        axes = list(range(1, self.d + 1))
        rng = np.random.default_rng(sorted(CASES).index(name))
        k = mrsi_orc.reconstruct(img, axes, sign=-1)
        self.k = k + NOISE * (rng.standard_normal(k.shape) + 1j * rng.standard_normal(k.shape))
        self.acs = np.ascontiguousarray(centre_block(self.k, self.block))
        for a in (self.s, self.rho, self.mask, self.k, self.acs):
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


# ---- the dense route ----------------------------------------------------------------------------------------------------
def calibration_matrix(acs, kernel, points):
    """A, one row per window position and time point, columns (s_1 .. s_d, coil) with the coil fastest."""
    c, shape, t = acs.shape[0], acs.shape[1:-1], min(points, acs.shape[-1])
    rows = []
    for pos in itertools.product(*[range(a - b + 1) for a, b in zip(shape, kernel)]):
        win = acs[(slice(None), *[slice(p, p + b) for p, b in zip(pos, kernel)], slice(0, t))]
        for k in range(t):
            rows.append(np.moveaxis(win[..., k], 0, -1).reshape(-1))
    return np.array(rows)


def singular_vectors(acs, kernel, points, threshold):
    """(v [Nk, b_1 .. b_d, C], sigma): the right singular vectors of A above threshold x sigma_1."""
    a = calibration_matrix(acs, kernel, points)
    _, sigma, vh = np.linalg.svd(a, full_matrices=False)
    keep = int(np.count_nonzero(sigma > threshold * sigma[0]))
    return vh[:keep].conj().reshape((keep, *kernel, acs.shape[0])), sigma


def voxel_matrices(v, mat):
    """H(q) [N..., C, C] from g_j(q)[c] = sum_s conj(v_j[s, c]) exp(+2 pi i q s / N), q = p - N // 2."""
    g = np.conj(v)  # [j, s_1 .. s_d, c]
    for axis, n in enumerate(mat):
        b = g.shape[1 + axis]
        e = np.exp(2j * np.pi * np.outer(np.arange(n) - n // 2, np.arange(b)) / n)  # [q, s]
        g = np.moveaxis(np.tensordot(e, g, axes=([1], [1 + axis])), 0, 1 + axis)
    s_tot = int(np.prod(v.shape[1:-1]))
    return np.einsum("j...c,j...d->...cd", g, np.conj(g)) / s_tot


def select(lam, vec, n_maps, phase_ref, crop):
    """The rules of k_espirit_eig on eigh's output (ascending lam [..., C], vec [..., C, C] columns): (maps [M, C, ...],
    values [M, ...]): descending eigenvalues, unit norm, component phase_ref real and >= 0, zero below crop."""
    maps, values = [], []
    for m in range(n_maps):
        x = vec[..., :, -1 - m]
        ref = x[..., phase_ref]
        turn = np.where(np.abs(ref) > 0, np.conj(ref) / np.where(np.abs(ref) > 0, np.abs(ref), 1.0), 1.0)
        x = x * turn[..., None] / np.linalg.norm(x, axis=-1, keepdims=True)
        x[..., phase_ref] = np.where(np.abs(ref) > 0, x[..., phase_ref].real, x[..., phase_ref])  # real, and stored so
        lm = lam[..., -1 - m]
        x = np.where((lm < crop)[..., None], 0.0, x)
        maps.append(np.moveaxis(x, -1, 0))
        values.append(lm)
    return np.array(maps), np.array(values)


def espirit(acs, mat, kernel, points=8, threshold=0.02, crop=0.8, n_maps=1, phase_ref=0):
    """dict(maps [M, C, N...], values [M, N...], H [N..., C, C], n_kernels, sigma)."""
    v, sigma = singular_vectors(np.asarray(acs, dtype=np.complex128), kernel, points, threshold)
    h = voxel_matrices(v, mat)
    lam, vec = np.linalg.eigh(h)
    maps, values = select(lam, vec, n_maps, phase_ref, crop)
    return dict(maps=maps, values=values, H=h, n_kernels=v.shape[0], sigma=sigma)


@functools.lru_cache(maxsize=None)
def reference(name, crop=0.8, n_maps=2):
    c = case(name)
    out = espirit(c.acs, c.mat, c.kernel, threshold=c.threshold, crop=crop, n_maps=n_maps)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


# ---- figures against the truth -----------------------------------------------------------------------------------------
def map_error(c, maps):
    """The largest |m - s| over coils and the voxels of the object; maps [C, N...]."""
    return float(np.abs(np.asarray(maps) - c.s)[:, c.mask].max())


def left_out(c, maps):
    """Share of the object's voxels whose map is zero in every coil."""
    dead = ~np.any(np.asarray(maps) != 0, axis=0)
    return float(dead[c.mask].sum()) / float(c.mask.sum())


def unfold_error(c, maps, accel=2):
    """SENSE unfolding at `accel` along the first dim with `maps` [C, N...]: the largest |rho' - rho| over all voxels and
    time points, relative to the largest |rho|."""
    rs = (accel,) + (1,) * (c.d - 1)
    axes = list(range(1, c.d + 1))
    alias = mrsi_orc.reconstruct(sense_orc.undersample(c.k, axes, rs), axes, sign=1)
    got = sense_orc.unfold(alias, np.asarray(maps), rs)["rho"]
    return float(np.abs(got - c.rho).max() / np.abs(c.rho).max())


def figures(c, maps2, values2, crop=0.9):
    """dict of the figures the issue's conditions are about; maps2 [2, C, N...] uncropped, values2 [2, N...]."""
    first = np.where((values2[0] < crop)[None], 0.0, maps2[0])
    return dict(lam1_min=float(values2[0][c.mask].min()), lam2_max=float(values2[1][c.mask].max()),
                gap_min=float((values2[0] - values2[1])[c.mask].min()), left_out=left_out(c, first),
                map_error=map_error(c, first), unfold_error=unfold_error(c, first))


def random_hermitian(c, v, seed, spectrum=None):
    """[V, C, C] = U diag(spectrum) U^H with Haar-like U; the default spectrum is 1, 0.6, then 0.3 / 2^k."""
    rng = np.random.default_rng(seed)
    lam = np.array(([1.0, 0.6] + [0.3 / 2 ** k for k in range(c)])[:c]) if spectrum is None else np.asarray(spectrum, float)
    z = rng.standard_normal((v, c, c)) + 1j * rng.standard_normal((v, c, c))
    u = np.linalg.qr(z)[0]
    return (u * lam[None, None, :]) @ np.conj(np.swapaxes(u, -1, -2)), lam


def upper(h):
    """[..., C, C] -> [..., E]: the upper triangle, row-major."""
    iu, ju = np.triu_indices(h.shape[-1])
    return np.ascontiguousarray(h[..., iu, ju])


# ---- the C ABI: a call that passes every check but the one under test (pointers are never dereferenced) -----------------
EIG_ORDER = ("h", "maps", "values", "status", "n_vox", "n_coils", "n_maps", "phase_ref", "crop")
EIG_OK = dict(h=0x10000, maps=0x20000, values=0x30000, status=0x40000, n_vox=37, n_coils=8, n_maps=2, phase_ref=0, crop=0.8)
EIG_REFUSALS = [dict(h=None), dict(maps=None), dict(values=None), dict(status=None), dict(h=0x10008), dict(maps=0x20008),
                dict(values=0x30004), dict(status=0x40002), dict(n_coils=0), dict(n_coils=65), dict(n_maps=0), dict(n_maps=3),
                dict(n_maps=2, n_coils=1), dict(n_vox=0), dict(n_vox=1 << 31), dict(maps=0x10000), dict(values=0x10000),
                dict(status=0x10000), dict(values=0x20000), dict(phase_ref=8), dict(phase_ref=-1), dict(crop=float("nan"))]
