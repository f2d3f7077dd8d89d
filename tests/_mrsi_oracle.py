"""numpy oracle of to_image / to_kspace, complex128, by two routes:

  "table": per axis the m x n matrix T[p][j] = w[j] e^{-sigma 2 pi i (j - n//2) s / m} e^{sigma 2 pi i (j - n//2)(p - m//2) / m}
           / sqrt(m), applied with a tensor product, one axis after the other;
  "fft":   the array times w and the shift ramp, zero filled with pad_left = m//2 - n//2, then numpy's
           fftshift((i)fftn(ifftshift(.), norm="ortho")) over all the axes at once.

sigma = +1 is to_image (inverse transform), -1 to_kspace.  The unit of a pencil (all the samples that one output of the
transformed axes depends on) is U = eps64 prod_a(1 / sqrt(m_a)) sum_j prod_a(|w_a[j_a]|) |K_j|: it does not depend on
the output index.  The product never imports this module."""
import functools

import numpy as np

EPS = float(np.finfo(np.float64).eps)
EPS32 = float(np.finfo(np.float32).eps)
ALPHA = {"hamming": 0.54, "hann": 0.5}


def weights(filt, n):
    """n real weights: None -> ones, a name -> alpha + (1 - alpha) cos(2 pi (j - n//2) / n), an array -> itself."""
    if filt is None:
        return np.ones(n)
    if isinstance(filt, str):
        a = ALPHA[filt]
        return np.array([a + (1 - a) * np.cos(2 * np.pi * (j - n // 2) / n) for j in range(n)])
    w = np.asarray(filt, dtype=np.float64)
    assert w.shape == (n,)
    return w


def table(n, m, filt=None, shift=0.0, sign=1):
    w = weights(filt, n)
    t = np.empty((m, n), dtype=np.complex128)
    for p in range(m):
        for j in range(n):
            k = j - n // 2
            t[p, j] = w[j] * np.exp(-sign * 2j * np.pi * k * shift / m) * np.exp(sign * 2j * np.pi * (k * (p - m // 2) % m) / m)
    return t / np.sqrt(m)


def _spec(x, axes, matrix, filters, shifts):
    axes = [a % x.ndim for a in axes]
    sizes = [x.shape[a] for a in axes]
    matrix = list(sizes) if matrix is None else ([matrix] * len(axes) if np.ndim(matrix) == 0 else list(matrix))
    filters = [filters] * len(axes) if (filters is None or isinstance(filters, str)) else list(filters)
    shifts = [0.0] * len(axes) if shifts is None else ([shifts] * len(axes) if np.ndim(shifts) == 0 else list(shifts))
    return axes, sizes, matrix, filters, shifts


def apply_table(x, axis, t):
    """y = t @ x along `axis` (complex128)."""
    y = np.tensordot(t, np.asarray(x, dtype=np.complex128), axes=([1], [axis]))  # the new axis comes first
    return np.moveaxis(y, 0, axis)


def reconstruct(x, axes, matrix=None, filters=None, shifts=None, sign=1, route="table"):
    """to_image (sign +1) / to_kspace (sign -1) of the complex array `x` over `axes`, in the order given."""
    x = np.asarray(x, dtype=np.complex128)
    axes, sizes, matrix, filters, shifts = _spec(x, axes, matrix, filters, shifts)
    if route == "table":
        for a, n, m, f, s in zip(axes, sizes, matrix, filters, shifts):
            x = apply_table(x, a, table(n, m, f, s, sign))
        return x
    assert route == "fft"
    pads = [(0, 0)] * x.ndim
    for a, n, m, f, s in zip(axes, sizes, matrix, filters, shifts):
        shape = [1] * x.ndim
        shape[a] = n
        k = np.arange(n) - n // 2
        x = x * (weights(f, n) * np.exp(-sign * 2j * np.pi * k * s / m)).reshape(shape)
        left = m // 2 - n // 2
        pads[a] = (left, m - n - left)
    x = np.fft.ifftshift(np.pad(x, pads), axes=axes)
    x = (np.fft.ifftn if sign > 0 else np.fft.fftn)(x, axes=axes, norm="ortho")
    return np.fft.fftshift(x, axes=axes)


def unit(x, axes, matrix=None, filters=None, tables=None):
    """U per pencil, with the transformed axes kept at size 1 (it broadcasts against the result).  `tables`: for a
    general matrix per axis, max_p |T[p][j]| takes the place of |w[j]| / sqrt(m)."""
    a = np.abs(np.asarray(x, dtype=np.complex128))
    axes, sizes, matrix, filters, _ = _spec(x, axes, matrix, filters, None)
    for i, (ax, n, m) in enumerate(zip(axes, sizes, matrix)):
        shape = [1] * a.ndim
        shape[ax] = n
        col = np.abs(tables[i]).max(axis=0) if tables is not None else np.abs(weights(filters[i], n)) / np.sqrt(m)
        a = a * col.reshape(shape)
    return EPS * a.sum(axis=tuple(axes), keepdims=True)


def gap(a, b, u):
    """The largest |a - b| in units of u (pencils with u = 0 must agree exactly)."""
    d = np.abs(a - b)
    ok = np.broadcast_to(u, d.shape) > 0
    assert not d[~ok].any()
    return float((d / np.where(u > 0, u, 1.0))[ok].max()) if ok.any() else 0.0


def make(shape, seed, dtype=np.complex128):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(dtype)


def custom_filter(n, seed=7):
    return 0.25 + np.random.default_rng(seed).random(n)


# name -> (shape, dims, transformed dims in the order of the call, matrix, filters, shifts, sign)
PARITY_CASES = {
    "coil3_7x12_to_16x12_hamming": ((3, 7, 12, 33), ("coil", "kx", "ky", "time"), ("kx", "ky"), (16, 12), "hamming", (0.25, -1.5), 1),
    "4x6x5_to_8x6x5_custom": ((4, 6, 5, 20), ("kx", "ky", "kz", "time"), ("kx", "ky", "kz"), (8, 6, 5), (None, "custom", "hann"), None, 1),
    "one_dim_9_to_24": ((2, 9, 17), ("coil", "kx", "time"), ("kx",), 24, "hann", 0.5, 1),
    "order_ky_then_kx": ((5, 8, 9), ("kx", "ky", "time"), ("ky", "kx"), (13, 8), "hamming", (1.0, -0.3), 1),
    "time_first_grid_last": ((21, 6, 7), ("time", "kx", "ky"), ("kx", "ky"), (10, 7), None, (0.0, 2.0), 1),
    "odd_7_to_16": ((7, 5), ("kx", "time"), ("kx",), 16, None, None, 1),
    "even_to_odd_8_to_11": ((8, 70), ("kx", "time"), ("kx",), 11, "hamming", -0.75, 1),
    "kspace_6x5_to_9x9": ((2, 6, 5, 19), ("coil", "x", "y", "time"), ("x", "y"), (9, 9), "hann", (0.5, 0.25), -1),
    "kspace_64_plain": ((64, 3), ("x", "time"), ("x",), None, None, None, -1),
    "full_64x64": ((2, 33, 64, 5), ("coil", "kx", "ky", "time"), ("kx", "ky"), 64, "hamming", (0.125, 0.0), 1),
}


def case_filters(name):
    shape, dims, tdims, matrix, filters, shifts, sign = PARITY_CASES[name]
    if isinstance(filters, tuple):
        return tuple(custom_filter(shape[dims.index(d)]) if f == "custom" else f for d, f in zip(tdims, filters))
    return filters


@functools.lru_cache(maxsize=None)
def parity_case(name):
    """(x complex128, axes, matrix, filters, shifts, sign, result by "table", result by "fft", unit); read-only."""
    shape, dims, tdims, matrix, _, shifts, sign = PARITY_CASES[name]
    filters = case_filters(name)
    x = make(shape, seed=sorted(PARITY_CASES).index(name))
    axes = [dims.index(d) for d in tdims]
    a = reconstruct(x, axes, matrix, filters, shifts, sign, "table")
    b = reconstruct(x, axes, matrix, filters, shifts, sign, "fft")
    u = unit(x, axes, matrix, filters)
    for v in (x, a, b, u):
        v.setflags(write=False)
    return x, axes, matrix, filters, shifts, sign, a, b, u


def worst_route_gap():
    return max(gap(c[6], c[7], c[8]) for c in map(parity_case, PARITY_CASES))
