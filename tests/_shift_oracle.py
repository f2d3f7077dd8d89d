"""TEST ORACLE (not product code): the time shift of DESIGN.md section 18 in numpy, complex128, stated two ways --
through numpy.fft and as the explicit O(N L) sums -- plus the physical case the tests and the tolerance tool share.

    X[k] = sum_{n<N} x[n] exp(-2 pi i k n / L),  kappa_k = numpy.fft.fftfreq(L)[k] L
    y[n] = (1 / L) sum_k X[k] exp(-2 pi i kappa_k phi / L) exp(+2 pi i k n / L),   n < N

Both routes take the ramp from `ramp`, which reduces kappa_k phi / L modulo 1 on the integer part of phi (integer
arithmetic, so nothing is rounded before the reduction): the value of r - rint(r), r = kappa_k phi / L, without the
rounding of r itself."""
import numpy as np

EPS = 2.0 ** -52


def kappa(L: int) -> np.ndarray:
    k = np.arange(L, dtype=np.int64)
    return np.where(k < (L + 1) // 2, k, k - L)


def _unit(num, L: int, sign: float) -> np.ndarray:
    """exp(sign 2 pi i num / L) for integer num, reduced on the integers."""
    a = 2.0 * np.pi * (np.mod(num, L).astype(np.float64) / L)
    return np.cos(a) + sign * 1j * np.sin(a)


def ramp(phi, L: int) -> np.ndarray:
    """exp(-2 pi i kappa_k phi / L): [..., L] for phi [...]."""
    phi = np.asarray(phi, dtype=np.float64)[..., None]
    whole = np.rint(phi)
    part = phi - whole
    kap = kappa(L)
    m = np.mod(kap * np.mod(whole, L).astype(np.int64), L)
    a = -2.0 * np.pi * ((m + kap * part) / L)
    return np.cos(a) + 1j * np.sin(a)


def shift_fft(x, phi, L=None) -> np.ndarray:
    """Rows x[..., N] delayed by phi[...] dwells (broadcast against the rows), through numpy.fft."""
    x = np.asarray(x, dtype=np.complex128)
    N = x.shape[-1]
    L = N if L is None else int(L)
    X = np.fft.fft(x, n=L, axis=-1)
    return np.fft.ifft(X * ramp(np.broadcast_to(phi, x.shape[:-1]), L), axis=-1)[..., :N]


def shift_sums(x, phi, L=None) -> np.ndarray:
    """The same as the explicit sums: two dense [L, N] products per row."""
    x = np.asarray(x, dtype=np.complex128)
    N = x.shape[-1]
    L = N if L is None else int(L)
    E = _unit(np.outer(np.arange(L, dtype=np.int64), np.arange(N, dtype=np.int64)), L, -1.0)  # [L, N]
    X = x @ E.T
    return ((X * ramp(np.broadcast_to(phi, x.shape[:-1]), L)) @ E.conj()) / L


def row_gap(got, want) -> np.ndarray:
    """Per row: the largest |got - want| relative to the row's largest |want|."""
    got, want = np.asarray(got), np.asarray(want)
    return np.abs(got - want).max(axis=-1) / np.abs(want).max(axis=-1)


def make(shape, seed: int, dtype=np.complex128) -> np.ndarray:
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(dtype)


PHIS = (0.0, 0.37, -0.37, 1.0, 1000.25)
ROUTE_CASES = ((16, 16), (32, 19), (256, 256), (384, 195), (640, 640), (1000, 1000))  # (L, N)


def worst_route_gap() -> float:
    """The largest disagreement of the two routes over ROUTE_CASES x PHIS, relative to each row's largest magnitude."""
    worst = 0.0
    for L, N in ROUTE_CASES:
        x = make((len(PHIS), N), seed=L + N)
        worst = max(worst, float(row_gap(shift_fft(x, PHIS, L), shift_sums(x, PHIS, L)).max()))
    return worst


# ---- the physical case: three damped lines, 50 rows acquired tau in [0, dt) late ------------------------------------
LINES_HZ = (300.3, -612.7, 41.9)
T2_STAR, DT, N_PHYS, ROWS_PHYS = 50e-3, 0.5e-3, 256, 50


def physical_case():
    """(x [50, 256] acquired tau late, tau [50] seconds, truth [256] the tau = 0 FID, dt)."""
    tau = np.arange(ROWS_PHYS) * (DT / ROWS_PHYS)
    t = np.arange(N_PHYS) * DT

    def fid(tt):
        return sum(np.exp((2j * np.pi * f - 1.0 / T2_STAR) * tt) for f in LINES_HZ)

    return fid(t[None, :] + tau[:, None]), tau, fid(t), DT


def spectral_error(rows, truth) -> float:
    """The largest spectral error of any row against the truth, relative to the truth spectrum's largest magnitude."""
    S = np.fft.fft(truth)
    return float(np.abs(np.fft.fft(rows, axis=-1) - S).max() / np.abs(S).max())


# ---- what xm_shift_time must refuse before any HIP call (CPU and GPU tests share the list) ---------------------------
ABI_ORDER = ("in", "in_row_stride", "out", "n_rows", "n", "L", "frac", "n_delay", "delay_div", "dtype")
ABI_OK = {"in": 4096, "in_row_stride": 200, "out": 65536, "n_rows": 5, "n": 200, "L": 256, "frac": 1024, "n_delay": 5,
          "delay_div": 1, "dtype": 0}
REFUSALS = (
    {"in": 0}, {"out": 0}, {"frac": 0},  # null pointers
    {"in": 4096 + 4}, {"out": 65536 + 4}, {"frac": 1024 + 4},  # misaligned
    {"in": 4096 + 8, "dtype": 1}, {"out": 65536 + 8, "dtype": 1},  # complex128 needs 16 bytes
    {"out": 4096},  # in == out
    {"L": 128}, {"n": 0}, {"n": -3}, {"n_delay": 0}, {"delay_div": 0}, {"delay_div": -1}, {"n_rows": -1},
    {"in_row_stride": 199},
    {"dtype": 2}, {"dtype": -1},
    {"L": 1000}, {"L": 250}, {"L": 32768}, {"L": 16384, "dtype": 1},  # outside the fused set
)
