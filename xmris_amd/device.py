"""Array-level device operations of the xmris spectral hot path (MI355X / gfx950).

Thin host wrappers around the C ABI of ``libxmris_hip.so``.  Inputs are complex torch tensors
resident in HBM (``complex64`` or ``complex128``); PyTorch is used only for device memory and
streams.  Each function names the reference statement it replaces.  There is no CPU fallback:
a tensor that is not on a GPU raises.

The FID / frequency axis may be any axis: it is moved last (one transposing copy) so that the
kernels see ``[n_batch, n]`` C-contiguous rows, and moved back afterwards, exactly like
``da.get_axis_num(dim)`` + ``axes=(axis,)`` in ``processing/fourier.py:152-153``.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np

from . import _lib


def _torch():
    import torch

    return torch


def _dtype_code(x) -> int:
    torch = _torch()
    if x.dtype == torch.complex64:
        return _lib.XM_C64
    if x.dtype == torch.complex128:
        return _lib.XM_C128
    raise TypeError(f"xmris_amd kernels need complex64/complex128 data, got {x.dtype}")


def _real_dtype(x):
    torch = _torch()
    return torch.float32 if x.dtype == torch.complex64 else torch.float64


def _require_device(x):
    torch = _torch()
    if not isinstance(x, torch.Tensor):
        raise TypeError("expected a torch.Tensor resident on the GPU")
    if not x.is_cuda:
        raise RuntimeError(
            "xmris_amd has no CPU path: the tensor must live on a HIP device (use xmris_amd.to_device)"
        )


def _stream(x):
    torch = _torch()
    return torch.cuda.current_stream(x.device).cuda_stream


def to_device(a, device="cuda", dtype=None):
    """Host ndarray (or tensor) -> complex tensor in HBM; real input is promoted to complex."""
    torch = _torch()
    if isinstance(a, torch.Tensor):
        t = a
    else:
        a = np.asarray(a)
        if not np.iscomplexobj(a):
            a = a.astype(np.complex128 if a.dtype != np.float32 else np.complex64)
        t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    if not t.is_complex():
        t = t.to(torch.complex128 if t.dtype == torch.float64 else torch.complex64)
    return t.to(device)


_HOST_STAGE = {}  # device index -> (pinned staging tensors, copy stream, worker pool)
_HOST_STAGE_BUFS = 4
_HOST_STAGE_LOCK = __import__("threading").Lock()  # one large download at a time shares the staging buffers


def to_host(x, chunk_bytes: int = 32 << 20):
    """Device tensor -> host ndarray.  Large results go through a few pinned staging buffers on a side stream:
    the DMA of the next chunks overlaps the host memcpys (worker threads; first-touch page faults of the fresh
    result dominate them) of the previous ones, instead of the runtime's own pageable path (measured 6.9 GB/s
    for a 1 GiB result)."""
    torch = _torch()
    x = x.detach()
    nbytes = x.numel() * x.element_size()
    if not x.is_cuda or nbytes < 4 * chunk_bytes:
        return x.cpu().numpy()
    with _HOST_STAGE_LOCK:
        return _to_host_staged(x.contiguous(), chunk_bytes)


def _to_host_staged(x, chunk_bytes: int):
    torch = _torch()
    from concurrent.futures import ThreadPoolExecutor

    nbytes = x.numel() * x.element_size()
    dev_idx = x.device.index or 0
    if dev_idx not in _HOST_STAGE:
        _HOST_STAGE[dev_idx] = ([torch.empty(chunk_bytes, dtype=torch.uint8, pin_memory=True)
                                 for _ in range(_HOST_STAGE_BUFS)],
                                torch.cuda.Stream(device=x.device), ThreadPoolExecutor(max_workers=_HOST_STAGE_BUFS))
    stage, side, pool = _HOST_STAGE[dev_idx]
    np_dtype = {torch.complex64: np.complex64, torch.complex128: np.complex128, torch.float32: np.float32,
                torch.float64: np.float64}.get(x.dtype)
    if np_dtype is None or chunk_bytes != stage[0].numel():
        return x.cpu().numpy()
    out = np.empty(tuple(x.shape), dtype=np_dtype)
    dst = out.reshape(-1).view(np.uint8)
    src = (torch.view_as_real(x) if x.is_complex() else x).reshape(-1).view(torch.uint8)
    stage_np = [b.numpy() for b in stage]
    side.wait_stream(torch.cuda.current_stream(x.device))  # the producer kernels
    pending = [None] * len(stage)

    def drain(ev, lo, n, k):
        ev.synchronize()
        np.copyto(dst[lo:lo + n], stage_np[k][:n])

    for i, lo in enumerate(range(0, nbytes, chunk_bytes)):
        k, n = i % len(stage), min(chunk_bytes, nbytes - lo)
        if pending[k] is not None:
            pending[k].result()  # the staging buffer is free again
        with torch.cuda.stream(side):
            stage[k][:n].copy_(src[lo:lo + n], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(side)
        pending[k] = pool.submit(drain, ev, lo, n, k)
    for f in pending:
        if f is not None:
            f.result()
    x.record_stream(side)
    return out


def _rows(x, axis):
    """Move `axis` last and flatten the rest -> ([n_batch, n] contiguous, restore(y, n_new))."""
    nd = x.dim()
    axis = axis % nd
    xm = x.movedim(axis, -1) if axis != nd - 1 else x
    lead = tuple(xm.shape[:-1])
    n = xm.shape[-1]
    x2 = xm.reshape(-1, n)
    if not x2.is_contiguous():
        x2 = x2.contiguous()

    def restore(y2):
        y = y2.reshape(lead + (y2.shape[-1],))
        if axis != nd - 1:
            y = y.movedim(-1, axis).contiguous()
        return y

    return x2, restore


def _table(values, like, complex_table: bool):
    """fp64 host table -> device tensor of the storage precision (rounded once)."""
    torch = _torch()
    if isinstance(values, torch.Tensor):
        t = values
    else:
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(values)))
    want = like.dtype if complex_table else _real_dtype(like)
    return t.to(device=like.device, dtype=want).contiguous()


# ---------------------------------------------------------------------------------------------
def zero_fill(x, axis: int, target_points: int, pad_left: int = 0):
    """fid.py:251 ``da.pad({dim: (pad_left, pad_right)}, constant_values=0)`` -- bit-exact copy."""
    _require_device(x)
    torch = _torch()
    x2, restore = _rows(x, axis)
    nb, n_in = x2.shape
    out = torch.empty((nb, target_points), dtype=x.dtype, device=x.device)
    _lib.call("xm_zero_fill", x2.data_ptr(), out.data_ptr(), nb, n_in, target_points, pad_left,
              _dtype_code(x), _stream(x))
    return restore(out)


def apodize(x, axis: int, window):
    """fid.py:139 ``da * weight`` with a real window over `axis` (host-computed in fp64)."""
    _require_device(x)
    torch = _torch()
    x2, restore = _rows(x, axis)
    nb, n = x2.shape
    w = _table(window, x, complex_table=False)
    if w.numel() != n:
        raise ValueError(f"window has {w.numel()} points, axis has {n}")
    out = torch.empty_like(x2)
    _lib.call("xm_apodize", x2.data_ptr(), out.data_ptr(), w.data_ptr(), nb, n, _dtype_code(x), _stream(x))
    return restore(out)


def zf_apod_supported(n_out: int, out_complex128: bool) -> bool:
    """True when `zf_apod` takes this output length (its window must fit the LDS)."""
    return int(n_out) * (8 if out_complex128 else 4) <= 96 * 1024


def zf_apod(x2, n_out: int, pad_left: int, window, promote: bool = False):
    """fid.py:251 + fid.py:136-139 in one launch (`xm_zf_apod`): ``x2`` = [n_batch, n_in] contiguous rows -> [n_batch,
    n_out] rows, zero filled and multiplied by `window` (n_out weights, fp64 host values or a device tensor).
    `promote`: complex64 rows give complex128 results (numpy's promotion against the float64 window)."""
    _require_device(x2)
    torch = _torch()
    if x2.dim() != 2 or not x2.is_contiguous():
        raise ValueError("zf_apod expects a contiguous [n_batch, n_in] tensor")
    nb, n_in = x2.shape
    out_dt = torch.complex128 if (promote or x2.dtype == torch.complex128) else torch.complex64
    rd = torch.float64 if out_dt == torch.complex128 else torch.float32
    if isinstance(window, torch.Tensor):
        w = window.to(device=x2.device, dtype=rd).contiguous()
    else:
        w = torch.from_numpy(np.ascontiguousarray(np.asarray(window, dtype=np.float64))).to(device=x2.device, dtype=rd)
    if w.numel() != n_out:
        raise ValueError(f"window has {w.numel()} points, the zero-filled axis has {n_out}")
    out = torch.empty((nb, n_out), dtype=out_dt, device=x2.device)
    _lib.call("xm_zf_apod", x2.data_ptr(), n_in, out.data_ptr(), w.data_ptr(), nb, n_in, int(n_out), int(pad_left),
              _dtype_code(x2), _lib.XM_C128 if out_dt == torch.complex128 else _lib.XM_C64, _stream(x2))
    return out


def phase_apply(x, axis: int, table):
    """phasing.py:73 ``da * np.exp(1j * phase_array)`` with a complex table over `axis`."""
    _require_device(x)
    torch = _torch()
    x2, restore = _rows(x, axis)
    nb, n = x2.shape
    ph = _table(table, x, complex_table=True)
    if ph.numel() != n:
        raise ValueError(f"phase table has {ph.numel()} points, axis has {n}")
    out = torch.empty_like(x2)
    _lib.call("xm_phase_apply", x2.data_ptr(), out.data_ptr(), ph.data_ptr(), nb, n, _dtype_code(x),
              _stream(x))
    return restore(out)


def roll(x, axis: int, shift: int):
    """fourier.py:31-32 / 57-58 ``da.roll({dim: shift})`` on the data -- bit-exact."""
    _require_device(x)
    torch = _torch()
    x2, restore = _rows(x, axis)
    nb, n = x2.shape
    out = torch.empty_like(x2)
    _lib.call("xm_roll", x2.data_ptr(), out.data_ptr(), nb, n, int(shift) % n, _dtype_code(x), _stream(x))
    return restore(out)


def fft(x, axis: int, inverse: bool = False, ortho: bool = True, shift_in: bool = False,
        shift_out: bool = False):
    """fourier.py:153 / 210 ``np.fft.(i)fftn(values, axes=(axis,), norm="ortho")`` with the
    surrounding (i)fftshift rolls optionally folded into the same launch."""
    _require_device(x)
    torch = _torch()
    x2, restore = _rows(x, axis)
    nb, n = x2.shape
    if n == 1:  # length-1 transform is the identity for every norm used on this path
        return restore(x2.clone())
    flags = ((_lib.XM_FFT_INVERSE if inverse else 0) | (_lib.XM_FFT_ORTHO if ortho else 0)
             | (_lib.XM_FFT_SHIFT_IN if shift_in else 0) | (_lib.XM_FFT_SHIFT_OUT if shift_out else 0))
    out = torch.empty_like(x2)
    _lib.call("xm_fft1d_batched", x2.data_ptr(), out.data_ptr(), nb, n, flags, _dtype_code(x), _stream(x))
    return restore(out)


def slice_axis(x, axis: int, start: int):
    """``da.isel({dim: slice(start, None)})`` on the data (bruker.py:66-67): contiguous copy."""
    _require_device(x)
    idx = [slice(None)] * x.dim()
    idx[axis % x.dim()] = slice(int(start), None)
    return x[tuple(idx)].contiguous()


def shift_fractional(x, axis: int, start: int, table):
    """bruker.py:79-84 on rows that start at sample `start`:  ifft(fft(x[start:]) * table).

    Two launches: the forward transform reads the rows in place (pointer offset + row stride, no slicing
    copy) and multiplies by `table` (complex, n - start values, fp64-computed) on the way out; the
    inverse transform carries numpy's 1/n scale."""
    _require_device(x)
    torch = _torch()
    x2, restore = _rows(x, axis)
    nb, n = x2.shape
    m = n - int(start)
    ph = _table(table, x, complex_table=True)
    if ph.numel() != m:
        raise ValueError(f"table has {ph.numel()} points, sliced axis has {m}")
    view = x2[:, int(start):]
    spec = torch.empty((nb, m), dtype=x.dtype, device=x.device)
    code, st = _dtype_code(x), _stream(x)
    _lib.call("xm_pipeline_fused", view.data_ptr(), n, spec.data_ptr(), None, ph.data_ptr(), nb, m, m, 0, 0,
              None, None, code, st)
    out = torch.empty_like(spec)
    _lib.call("xm_fft1d_batched", spec.data_ptr(), out.data_ptr(), nb, m, _lib.XM_FFT_INVERSE, code, st)
    return restore(out)


def baseline_als(x, axis: int, lam: float, p: float, n_iter: int):
    """baseline.py:10-40 along `axis`: returns real(x) - AsLS baseline as float64 (any real or complex
    float32/float64 input).  fp64 band LDL' solves, one thread per spectrum on transposed scratch."""
    torch = _torch()
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise RuntimeError("xmris_amd has no CPU path: the tensor must live on a HIP device")
    is_complex = x.is_complex()
    if x.dtype in (torch.complex64, torch.float32):
        code = _lib.XM_C64
    elif x.dtype in (torch.complex128, torch.float64):
        code = _lib.XM_C128
    else:
        raise TypeError(f"baseline_als needs float32/float64 (complex) data, got {x.dtype}")
    x2, restore = _rows(x, axis)
    nb, n = x2.shape
    need = int(_lib.load().xm_baseline_als_workspace_bytes(nb, n))
    work = torch.empty(max(need // 8, 1), dtype=torch.float64, device=x.device)
    out = torch.empty((nb, n), dtype=torch.float64, device=x.device)
    _lib.call("xm_baseline_als", x2.data_ptr(), int(is_complex), nb, n, float(lam), float(p), int(n_iter),
              out.data_ptr(), work.data_ptr(), need, code, torch.cuda.current_stream(x.device).cuda_stream)
    return restore(out)


def amares_model(params, n: int, dt: float, t0: float):
    """AMARES model (fitting/simulation.py:9-96): params [..., K, 5] fp64 device tensor (a, f [Hz], d [1/s], phi [rad],
    g per peak) -> complex128 FIDs [..., n] at t_j = j dt + t0."""
    torch = _torch()
    _require_device(params)
    p = params.to(torch.float64).contiguous()
    if p.dim() < 2 or p.shape[-1] != 5:
        raise ValueError(f"amares_model needs parameters [..., n_peaks, 5], got {tuple(p.shape)}")
    lead, k = tuple(p.shape[:-2]), p.shape[-2]
    nb = int(np.prod(lead, dtype=np.int64)) if lead else 1
    out = torch.empty(lead + (n,), dtype=torch.complex128, device=p.device)
    _lib.call("xm_amares_model", p.data_ptr(), nb, k, int(n), float(dt), float(t0), out.data_ptr(), _stream(p))
    return out


class AmaresFit:
    """Raw outputs of ``amares_fit`` with the non-time axes of the input in front: params [..., K, 5] (fitting units),
    amp_sd [..., K] (sqrt of the amplitude's diagonal entry of (J^T J)^-1, not yet scaled by sigma), rss [...],
    status [...] (0 converged, 1 iteration cap, 2 non-finite), iters [...], fit [..., n] complex128 (or None)."""

    __slots__ = ("params", "amp_sd", "rss", "status", "iters", "fit", "n_free")

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)


def amares_fit(x, axis: int, init, lo, hi, fixed, dt: float, t0: float = 0.0, max_iter: int = 200,
               ftol: float = 1e-10, xtol: float = 1e-10, want_fit: bool = True, links=None) -> AmaresFit:
    """One Levenberg-Marquardt AMARES fit per FID along `axis` of the complex64 / complex128 device tensor `x`, all
    voxels in one launch (xm_amares_fit_linked).  init / lo / hi / fixed: [K, 5] prior knowledge in fitting units (a,
    f [Hz], d [1/s], phi [rad], g), shared by every voxel.  links: None, or (link_to, link_scale, link_offset), each
    [K, 5]: parameter q = 5 k + c follows its root link_to[k, c] (a parameter index, -1: not linked) as
    scale * p_root + offset, in fitting units.  `n_free` of the result counts the free columns of the Jacobian: a
    group of linked parameters is one."""
    torch = _torch()
    _require_device(x)
    code = _dtype_code(x)
    init, lo, hi = (np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(-1, 5)) for v in (init, lo, hi))
    fixed = np.ascontiguousarray(np.asarray(fixed, dtype=bool).reshape(-1, 5).astype(np.int32))
    k = init.shape[0]
    if not (lo.shape == hi.shape == fixed.shape == init.shape):
        raise ValueError("init, lo, hi and fixed must all be [n_peaks, 5]")
    if links is None:
        link_to = np.full((k, 5), -1, dtype=np.int32)
        link_sc, link_off = np.ones((k, 5)), np.zeros((k, 5))
    else:
        link_to = np.ascontiguousarray(np.asarray(links[0]).reshape(-1, 5).astype(np.int32))
        link_sc, link_off = (np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(-1, 5)) for v in links[1:])
        if not (link_to.shape == link_sc.shape == link_off.shape == init.shape):
            raise ValueError("links must be three [n_peaks, 5] arrays")
    axis = axis % x.dim()
    x2, restore = _rows(x, axis)
    nb, n = x2.shape
    lead = tuple(s for i, s in enumerate(x.shape) if i != axis)
    dev_ = x.device
    params = torch.empty((nb, k, 5), dtype=torch.float64, device=dev_)
    asd = torch.empty((nb, k), dtype=torch.float64, device=dev_)
    rss = torch.empty(nb, dtype=torch.float64, device=dev_)
    status = torch.empty(nb, dtype=torch.int32, device=dev_)
    iters = torch.empty(nb, dtype=torch.int32, device=dev_)
    fit = torch.empty((nb, n), dtype=torch.complex128, device=dev_) if want_fit else None
    need = int(_lib.load().xm_amares_workspace_bytes(nb, n, k))
    work = torch.zeros(max(need, 8), dtype=torch.uint8, device=dev_)
    ptr = lambda a: a.ctypes.data  # noqa: E731  (host prior-knowledge arrays)
    _lib.call("xm_amares_fit_linked", x2.data_ptr(), n, nb, n, float(dt), float(t0), k, ptr(init), ptr(lo), ptr(hi),
              ptr(fixed), ptr(link_to), ptr(link_sc), ptr(link_off), int(max_iter), float(ftol), float(xtol),
              params.data_ptr(), asd.data_ptr(), rss.data_ptr(), status.data_ptr(), iters.data_ptr(),
              fit.data_ptr() if fit is not None else None, work.data_ptr(), need, code, _stream(x))
    n_free = int(np.count_nonzero(~(fixed.astype(bool) | (lo == hi)) & (link_to < 0)))
    return AmaresFit(params=params.reshape(lead + (k, 5)), amp_sd=asd.reshape(lead + (k,)), rss=rss.reshape(lead),
                     status=status.reshape(lead), iters=iters.reshape(lead),
                     fit=fit.reshape(lead + (n,)) if fit is not None else None, n_free=n_free)


def _basis_groups(group, m: int):
    group = np.ascontiguousarray(np.asarray(group, dtype=np.int32).reshape(-1))
    if group.size != m:
        raise ValueError(f"group must name one group per metabolite ({m}), got {group.size}")
    return group, (int(group.max()) + 1 if m else 0)


def basis_model(params, basis, group, dt: float):
    """Basis-set model: params [..., Q] fp64 device tensor (Q = M + 3 G + 1: amplitudes, then
    shifts [Hz], Lorentzian dampings [1/s] and Gaussian dampings [1/s^2] per group, then the phase [rad]), basis [M, n]
    complex device tensor, group [M] host indices -> complex128 FIDs [..., n] at t_j = j dt."""
    torch = _torch()
    _require_device(params)
    _require_device(basis)
    b = basis.to(torch.complex128).contiguous()
    if b.dim() != 2:
        raise ValueError(f"basis_model needs a basis [n_metab, n], got {tuple(b.shape)}")
    m, n = b.shape
    group, g = _basis_groups(group, m)
    p = params.to(torch.float64).contiguous()
    q = m + 3 * g + 1
    if p.dim() < 1 or p.shape[-1] != q:
        raise ValueError(f"basis_model needs parameters [..., {q}], got {tuple(p.shape)}")
    lead = tuple(p.shape[:-1])
    nb = int(np.prod(lead, dtype=np.int64)) if lead else 1
    out = torch.empty(lead + (n,), dtype=torch.complex128, device=p.device)
    _lib.call("xm_basis_model", p.data_ptr(), nb, b.data_ptr(), m, group.ctypes.data, g, n, float(dt), out.data_ptr(),
              _stream(p))
    return out


class BasisFit:
    """Raw outputs of ``basis_fit`` with the non-time axes of the input in front: params [..., Q] (fitting units, the
    layout of ``basis_model``), amp_sd [..., M] (not yet scaled by sigma), rss [...], status [...] (0 converged,
    1 iteration cap, 2 non-finite), iters [...], fit [..., n] complex128 (or None); n_free: the free columns."""

    __slots__ = ("params", "amp_sd", "rss", "status", "iters", "fit", "n_free")

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)


def basis_fit(x, axis: int, basis, group, init, lo, hi, fixed, dt: float, skip: int = 0, max_iter: int = 200,
              ftol: float = 1e-10, xtol: float = 1e-10, want_fit: bool = True) -> BasisFit:
    """One Levenberg-Marquardt basis-set fit per FID along `axis` of the complex64 / complex128 device tensor `x`, all
    voxels in one launch (xm_basis_fit).  basis: [M, n] complex device tensor on the data's time
    grid; group [M]: host group indices; init / lo / hi / fixed: [Q] host arrays in the layout of ``basis_model``,
    shared by every voxel (a NaN amplitude start: the automatic per-voxel start)."""
    torch = _torch()
    _require_device(x)
    _require_device(basis)
    code = _dtype_code(x)
    axis = axis % x.dim()
    x2, restore = _rows(x, axis)
    nb, n = x2.shape
    b = basis.to(torch.complex128).contiguous()
    if b.dim() != 2 or b.shape[1] != n:
        raise ValueError(f"basis_fit needs a basis [n_metab, {n}], got {tuple(b.shape)}")
    m = b.shape[0]
    group, g = _basis_groups(group, m)
    q = m + 3 * g + 1
    init, lo, hi = (np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(-1)) for v in (init, lo, hi))
    fixed = np.ascontiguousarray(np.asarray(fixed, dtype=bool).reshape(-1).astype(np.int32))
    if not (init.size == lo.size == hi.size == fixed.size == q):
        raise ValueError(f"init, lo, hi and fixed must all hold {q} values")
    lead = tuple(s for i, s in enumerate(x.shape) if i != axis)
    dev_ = x.device
    params = torch.empty((nb, q), dtype=torch.float64, device=dev_)
    asd = torch.empty((nb, m), dtype=torch.float64, device=dev_)
    rss = torch.empty(nb, dtype=torch.float64, device=dev_)
    status = torch.empty(nb, dtype=torch.int32, device=dev_)
    iters = torch.empty(nb, dtype=torch.int32, device=dev_)
    fit = torch.empty((nb, n), dtype=torch.complex128, device=dev_) if want_fit else None
    need = int(_lib.load().xm_basis_workspace_bytes(nb, n, m))
    work = torch.zeros(max(need, 8), dtype=torch.uint8, device=dev_)
    ptr = lambda a: a.ctypes.data  # noqa: E731  (host arrays)
    _lib.call("xm_basis_fit", x2.data_ptr(), n, nb, n, float(dt), int(skip), b.data_ptr(), m, ptr(group), g, ptr(init),
              ptr(lo), ptr(hi), ptr(fixed), int(max_iter), float(ftol), float(xtol), params.data_ptr(), asd.data_ptr(),
              rss.data_ptr(), status.data_ptr(), iters.data_ptr(), fit.data_ptr() if fit is not None else None,
              work.data_ptr(), need, code, _stream(x))
    n_free = int(np.count_nonzero(~(fixed.astype(bool) | (lo == hi))))
    return BasisFit(params=params.reshape(lead + (q,)), amp_sd=asd.reshape(lead + (m,)), rss=rss.reshape(lead),
                    status=status.reshape(lead), iters=iters.reshape(lead),
                    fit=fit.reshape(lead + (n,)) if fit is not None else None, n_free=n_free)


class KineticsFit:
    """Raw outputs of ``kinetics_fit``: params and param_sd [n_batch, M, 3] (k, rho, z), rss, status (0 converged,
    1 iteration cap, 2 non-finite, 3 fewer weighted points than free parameters), iters and auc_ratio [n_batch, M],
    fit [n_batch, M, T] (or None); n_free [M]: the free parameters of each product."""

    __slots__ = ("params", "param_sd", "rss", "status", "iters", "fit", "auc_ratio", "n_free")

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)


def kinetics_fit(substrate, products, times, flip_s, flip_p, init, lo, hi, fixed, weights=None, max_iter: int = 200,
                 ftol: float = 1e-10, xtol: float = 1e-10, want_fit: bool = True) -> KineticsFit:
    """One rate fit per (voxel, product) pair, all in one launch of k_kinetics_fit (xm_kinetics_fit, DESIGN.md section
    19).  Device tensors: substrate [n_batch, T], products and weights [n_batch, M, T] (weights None: all 1; a point of
    weight 0 is missing).  Host values: times [T] (seconds), flip_s [T] and flip_p [M, T] (radians), init / lo / hi /
    fixed [M, 3] in the order k, rho, z, shared by every voxel (a NaN start of a free z: the automatic per-fit start)."""
    torch = _torch()
    _require_device(substrate)
    _require_device(products)
    s = substrate.to(torch.float64).contiguous()
    y = products.to(torch.float64).contiguous()
    if s.dim() != 2 or y.dim() != 3 or y.shape[0] != s.shape[0] or y.shape[2] != s.shape[1]:
        raise ValueError(f"kinetics_fit needs substrate [n_batch, T] and products [n_batch, M, T], got {tuple(s.shape)} "
                         f"and {tuple(y.shape)}")
    nb, m, t = y.shape
    w = None
    if weights is not None:
        _require_device(weights)
        w = weights.to(torch.float64).contiguous()
        if tuple(w.shape) != (nb, m, t):
            raise ValueError(f"weights must have the products' shape {(nb, m, t)}, got {tuple(w.shape)}")
    host = lambda v, shape: np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64), shape))  # noqa: E731
    times, flip_s, flip_p = host(np.asarray(times).reshape(-1), (t,)), host(flip_s, (t,)), host(flip_p, (m, t))
    init, lo, hi = (host(v, (m, 3)) for v in (init, lo, hi))
    fixed = np.ascontiguousarray(np.broadcast_to(np.asarray(fixed, dtype=bool), (m, 3)).astype(np.int32))
    dev_ = s.device
    f64 = dict(dtype=torch.float64, device=dev_)
    params, psd = torch.empty((nb, m, 3), **f64), torch.empty((nb, m, 3), **f64)
    rss, auc = torch.empty((nb, m), **f64), torch.empty((nb, m), **f64)
    status = torch.empty((nb, m), dtype=torch.int32, device=dev_)
    iters = torch.empty((nb, m), dtype=torch.int32, device=dev_)
    fit = torch.empty((nb, m, t), **f64) if want_fit else None
    ptr = lambda a: a.ctypes.data  # noqa: E731  (host arrays)
    _lib.call("xm_kinetics_fit", s.data_ptr(), y.data_ptr(), w.data_ptr() if w is not None else None, nb, m, t,
              ptr(times), ptr(flip_s), ptr(flip_p), ptr(init), ptr(lo), ptr(hi), ptr(fixed), int(max_iter), float(ftol),
              float(xtol), params.data_ptr(), psd.data_ptr(), rss.data_ptr(), status.data_ptr(), iters.data_ptr(),
              fit.data_ptr() if fit is not None else None, auc.data_ptr(), _stream(s))
    n_free = np.count_nonzero(~(fixed.astype(bool) | (lo == hi)), axis=1)
    return KineticsFit(params=params, param_sd=psd, rss=rss, status=status, iters=iters, fit=fit, auc_ratio=auc,
                       n_free=n_free)


class CoilCombine:
    """Raw outputs of ``coil_combine`` with the axes of the input other than coil and time in front, in the input's
    order: y [..., N] (the input's dtype), weights [..., C] complex128, quality [...] fp64, status [...] int32
    (0 combined, 1 nothing to go by, 2 non-finite sample, 3 Jacobi sweep cap)."""

    __slots__ = ("y", "weights", "quality", "status")

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)


COIL_METHODS = {"svd": _lib.XM_COIL_SVD, "first_point": _lib.XM_COIL_FIRST_POINT, "svd_fma": _lib.XM_COIL_SVD_FMA}


def coil_combine(x, coil_axis: int, time_axis: int, method: str = "svd", reference=None, linv=None,
                 n_points: int = 1, workspace=None) -> CoilCombine:
    """Per-voxel coil combination of the complex64 / complex128 device tensor `x` in one launch (xm_coil_combine,
    DESIGN.md section 10).  `reference`: a tensor with x's axes and sizes except along `time_axis`; the weights then
    come from it alone.  `linv`: L^{-1} of the noise covariance L L^H, [C, C] (host or device), or None for the
    identity.  With time as the last axis of a contiguous tensor the kernel addresses the coil axis where it is;
    any other layout costs one contiguous copy (time moved last).  "svd_fma" is "svd" with the Gram matrix on plain
    FMAs (verification).  `workspace`: a zeroed uint8 tensor of XM_COIL_WORKSPACE_BYTES to reuse between calls."""
    torch = _torch()
    _require_device(x)
    if method not in COIL_METHODS:
        raise ValueError(f"method must be one of {tuple(COIL_METHODS)}, got {method!r}")
    nd = x.dim()
    coil_axis, time_axis = coil_axis % nd, time_axis % nd
    if coil_axis == time_axis:
        raise ValueError("coil_axis and time_axis must differ")

    def rows(a):  # time last, C-contiguous
        if time_axis != nd - 1:
            a = torch.movedim(a, time_axis, -1)
        return a if a.is_contiguous() else a.contiguous()

    ca = coil_axis if coil_axis < time_axis else coil_axis - 1  # where the coil axis is once time is last
    xr = rows(x)
    code = _dtype_code(xr)
    shape = tuple(xr.shape)
    c, n = shape[ca], shape[-1]
    n_outer = int(np.prod(shape[:ca], dtype=np.int64))
    n_inner = int(np.prod(shape[ca + 1:-1], dtype=np.int64))
    lead = shape[:ca] + shape[ca + 1:-1]
    n_ref, rr = n, None
    if reference is not None:
        _require_device(reference)
        if reference.dim() != nd or reference.dtype != x.dtype:
            raise ValueError("reference must have x's dtype and number of axes")
        rr = rows(reference)
        if tuple(rr.shape[:-1]) != shape[:-1]:
            raise ValueError(f"reference shape {tuple(reference.shape)} does not match x {tuple(x.shape)} off the time axis")
        n_ref = rr.shape[-1]
    li = None
    if linv is not None:
        li = torch.as_tensor(np.ascontiguousarray(linv, dtype=np.complex128) if not hasattr(linv, "detach") else linv)
        li = li.to(x.device, torch.complex128).contiguous()
        if tuple(li.shape) != (c, c):
            raise ValueError(f"linv must be [{c}, {c}], got {tuple(li.shape)}")
    dev_ = x.device
    y = torch.empty(lead + (n,), dtype=x.dtype, device=dev_)
    w = torch.empty(lead + (c,), dtype=torch.complex128, device=dev_)
    quality = torch.empty(lead, dtype=torch.float64, device=dev_)
    status = torch.empty(lead, dtype=torch.int32, device=dev_)
    work = workspace if workspace is not None else torch.zeros(_lib.XM_COIL_WORKSPACE_BYTES, dtype=torch.uint8, device=dev_)
    _lib.call("xm_coil_combine", xr.data_ptr(), rr.data_ptr() if rr is not None else None, y.data_ptr(), w.data_ptr(),
              quality.data_ptr(), status.data_ptr(), n_outer, c, n_inner, n, n_ref,
              li.data_ptr() if li is not None else None, COIL_METHODS[method], int(n_points),
              int(code == _lib.XM_C128), work.data_ptr(), _stream(x))
    return CoilCombine(y=y, weights=w, quality=quality, status=status)


class SenseUnfold:
    """Raw outputs of ``unfold_sense``: y, the input without its coil axis and with the spatial axes grown to
    N = accel n (the input's dtype, its axis order, time last); g fp64 and status int32 per full-FOV voxel, the batch
    axes in front and the spatial axes in the order they were given (0 unfolded, 1 masked, 2 non-finite sample,
    3 not positive definite)."""

    __slots__ = ("y", "g", "status")

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)


SENSE_MAX_COILS = 64
SENSE_MAX_ACCEL = 16


def unfold_sense(x, sens, coil_axis: int, spatial_axes, time_axis: int, accel, linv=None, regularization: float = 0.0,
                 workspace=None) -> SenseUnfold:
    """SENSE unfolding of the aliased complex64 / complex128 device tensor `x` in one launch (xm_sense_unfold, DESIGN.md
    section 16).  `spatial_axes`: 1 ... 3 undersampled axes, `accel`: the acceleration along each; every axis but these,
    `coil_axis` and `time_axis` is batch.  `sens`: [C, N...] complex, the spatial axes in the order of `spatial_axes`
    (host values or a device tensor; uploaded as complex128).  `linv`: L^{-1} of the noise covariance L L^H, [C, C], or
    None for the identity.  With time last the coil and spatial axes are addressed where they lie; a tensor whose time
    axis is not contiguous, or whose batch axes do not fold into one stride, costs one contiguous copy.  `workspace`: a
    zeroed uint8 tensor of XM_SENSE_WORKSPACE_BYTES to reuse between calls."""
    torch = _torch()
    _require_device(x)
    nd = x.dim()
    coil_axis, time_axis = coil_axis % nd, time_axis % nd
    axes = [int(a) % nd for a in spatial_axes]
    acc = [int(r) for r in accel]
    if not 1 <= len(axes) <= 3 or len(acc) != len(axes):
        raise ValueError(f"spatial_axes: needs 1 ... 3 axes and one accel per axis, got {len(axes)} and {len(acc)}")
    if len({coil_axis, time_axis, *axes}) != len(axes) + 2:
        raise ValueError("coil_axis, time_axis and spatial_axes must all differ")
    if any(r < 1 for r in acc) or int(np.prod(acc)) > SENSE_MAX_ACCEL:
        raise ValueError(f"accel: every entry must be >= 1 and their product at most {SENSE_MAX_ACCEL}, got {acc}")
    c, nt = int(x.shape[coil_axis]), int(x.shape[time_axis])
    small = [int(x.shape[a]) for a in axes]
    full = [r * n for r, n in zip(acc, small)]
    if not 1 <= c <= SENSE_MAX_COILS or nt < 1 or min(small) < 1:
        raise ValueError(f"needs 1 ... {SENSE_MAX_COILS} coils and no empty axis, got shape {tuple(x.shape)}")
    batch = [a for a in range(nd) if a not in (coil_axis, time_axis, *axes)]

    def folds(v):  # the batch axes in front of v fold into one stride
        return all(v.stride(i) == v.stride(i + 1) * v.shape[i + 1] for i in range(len(batch) - 1))

    xv = x.permute(batch + [coil_axis] + axes + [time_axis])
    if xv.numel() and (xv.stride(-1) != 1 and nt > 1 or not folds(xv)):
        xv = xv.contiguous()
    code = _dtype_code(xv)
    dev_ = x.device
    if isinstance(sens, torch.Tensor):
        s = sens.to(device=dev_, dtype=torch.complex128).contiguous()
    else:
        s = torch.from_numpy(np.array(sens, dtype=np.complex128, order="C")).to(dev_)  # (a copy: the source may be read-only)
    if tuple(s.shape) != (c, *full):
        raise ValueError(f"sens must be {[c, *full]} (coils, then accel x size per spatial axis), got {list(s.shape)}")
    li = None
    if linv is not None:
        li = torch.as_tensor(np.ascontiguousarray(linv, dtype=np.complex128) if not hasattr(linv, "detach") else linv)
        li = li.to(dev_, torch.complex128).contiguous()
        if tuple(li.shape) != (c, c):
            raise ValueError(f"linv must be [{c}, {c}], got {tuple(li.shape)}")
    # y: batch axes in front, then the spatial axes in the input's own order, then time
    kept = sorted(axes)
    bshape = [int(x.shape[a]) for a in batch]
    yc = torch.empty(bshape + [full[axes.index(a)] for a in kept] + [nt], dtype=x.dtype, device=dev_)
    nb = len(batch)
    yv = yc.permute(list(range(nb)) + [nb + kept.index(a) for a in axes] + [nb + len(axes)])
    g = torch.empty(bshape + full, dtype=torch.float64, device=dev_)
    status = torch.empty(bshape + full, dtype=torch.int32, device=dev_)
    pad = 3 - len(axes)
    n_outer = int(np.prod(bshape, dtype=np.int64))
    if n_outer > 0:
        ostride = lambda v: int(v.stride(nb - 1)) if nb else 0  # noqa: E731
        a_str = [ostride(xv), int(xv.stride(nb))] + [0] * pad + [int(xv.stride(nb + 1 + i)) for i in range(len(axes))]
        y_str = [ostride(yv)] + [0] * pad + [int(yv.stride(nb + i)) for i in range(len(axes))]
        i32, i64 = ctypes.c_int32 * 3, ctypes.c_int64
        work = workspace if workspace is not None else torch.zeros(_lib.XM_SENSE_WORKSPACE_BYTES, dtype=torch.uint8, device=dev_)
        _lib.call("xm_sense_unfold", xv.data_ptr(), yc.data_ptr(), s.data_ptr(), li.data_ptr() if li is not None else None,
                  g.data_ptr(), status.data_ptr(), n_outer, c, i32(*([1] * pad + small)), i32(*([1] * pad + acc)), nt,
                  (i64 * 5)(*a_str), (i64 * 4)(*y_str), float(regularization), code, work.data_ptr(), _stream(x))
    # back to the input's axis order (without the coil axis, time last)
    order = [a for a in range(nd) if a not in (coil_axis, time_axis)]
    have = batch + kept
    y = yc.permute([have.index(a) for a in order] + [len(have)])
    return SenseUnfold(y=y if y.is_contiguous() else y.contiguous(), g=g, status=status)


GRAPPA_MAX_COILS = 64
GRAPPA_MAX_ACCEL = 16
GRAPPA_MAX_SOURCES = 64  # S = the product of the kernel sizes
GRAPPA_MAX_TERMS = 1024  # C S


def grappa_weights(weights, device):
    """GRAPPA weights (host values or a tensor) as a contiguous complex128 tensor on `device`, as xm_grappa_fill reads them."""
    torch = _torch()
    if isinstance(weights, torch.Tensor):
        return weights.to(device=device, dtype=torch.complex128).contiguous()
    return torch.from_numpy(np.array(weights, dtype=np.complex128, order="C")).to(device)


def grappa_fill(x, weights, coil_axis: int, spatial_axes, time_axis: int, accel, kernel):
    """GRAPPA fill of the kept k-space lines in the complex64 / complex128 device tensor `x` in one launch
    (xm_grappa_fill).  `spatial_axes`: 1 ... 3 undersampled axes, `accel` and `kernel`: the
    acceleration and the number of neighbour lines along each; every axis but these, `coil_axis` and `time_axis` is
    batch.  `weights`: [R - 1, C, S, C] complex (host values, uploaded at every call, or a device tensor, used where it lies when
    it is contiguous complex128: ``grappa_weights``), None at R = 1.
    Returns the tensor with every spatial axis grown to accel x its size, in the input's dtype and axis order but time
    last.  With time last the coil and spatial axes are addressed where they lie; a tensor whose time axis is not
    contiguous, or whose batch axes do not fold into one stride, costs one contiguous copy."""
    torch = _torch()
    _require_device(x)
    nd = x.dim()
    coil_axis, time_axis = coil_axis % nd, time_axis % nd
    axes = [int(a) % nd for a in spatial_axes]
    acc, ker = [int(r) for r in accel], [int(b) for b in kernel]
    if not 1 <= len(axes) <= 3 or len(acc) != len(axes) or len(ker) != len(axes):
        raise ValueError(f"spatial_axes: needs 1 ... 3 axes and one accel and one kernel size per axis, got {len(axes)}, "
                         f"{len(acc)} and {len(ker)}")
    if len({coil_axis, time_axis, *axes}) != len(axes) + 2:
        raise ValueError("coil_axis, time_axis and spatial_axes must all differ")
    rtot, stot = int(np.prod(acc)), int(np.prod(ker))
    if any(r < 1 for r in acc) or rtot > GRAPPA_MAX_ACCEL:
        raise ValueError(f"accel: every entry must be >= 1 and their product at most {GRAPPA_MAX_ACCEL}, got {acc}")
    c, nt = int(x.shape[coil_axis]), int(x.shape[time_axis])
    small = [int(x.shape[a]) for a in axes]
    full = [r * n for r, n in zip(acc, small)]
    if not 1 <= c <= GRAPPA_MAX_COILS or nt < 1 or min(small) < 1:
        raise ValueError(f"needs 1 ... {GRAPPA_MAX_COILS} coils and no empty axis, got shape {tuple(x.shape)}")
    if any(b < 1 for b in ker) or stot > GRAPPA_MAX_SOURCES or c * stot > GRAPPA_MAX_TERMS:
        raise ValueError(f"kernel: every entry must be >= 1, their product at most {GRAPPA_MAX_SOURCES} and coils x product "
                         f"at most {GRAPPA_MAX_TERMS}, got {ker} at {c} coils")
    dev_ = x.device
    w = None
    if rtot > 1:
        if weights is None:
            raise ValueError("weights: needed when the product of accel exceeds 1")
        w = grappa_weights(weights, dev_)
        if tuple(w.shape) != (rtot - 1, c, stot, c):
            raise ValueError(f"weights must be {[rtot - 1, c, stot, c]} (types, coils, sources, coils), got {list(w.shape)}")
    batch = [a for a in range(nd) if a not in (coil_axis, time_axis, *axes)]

    def folds(v):  # the batch axes in front of v fold into one stride
        return all(v.stride(i) == v.stride(i + 1) * v.shape[i + 1] for i in range(len(batch) - 1))

    xv = x.permute(batch + [coil_axis] + axes + [time_axis])
    if xv.numel() and (xv.stride(-1) != 1 and nt > 1 or not folds(xv)):
        xv = xv.contiguous()
    code = _dtype_code(xv)
    # y: batch axes in front, then the coil and spatial axes in the input's own order, then time
    kept = sorted([coil_axis] + axes)
    bshape = [int(x.shape[a]) for a in batch]
    size = {coil_axis: c, **{a: f for a, f in zip(axes, full)}}
    yc = torch.empty(bshape + [size[a] for a in kept] + [nt], dtype=x.dtype, device=dev_)
    nb = len(batch)
    yv = yc.permute(list(range(nb)) + [nb + kept.index(a) for a in [coil_axis] + axes] + [nb + len(kept)])
    pad = 3 - len(axes)
    n_outer = int(np.prod(bshape, dtype=np.int64))
    if n_outer > 0:
        def strides(v):
            return ([int(v.stride(nb - 1)) if nb else 0, int(v.stride(nb))] + [0] * pad
                    + [int(v.stride(nb + 1 + i)) for i in range(len(axes))])

        i32, i64 = ctypes.c_int32 * 3, ctypes.c_int64 * 5
        _lib.call("xm_grappa_fill", xv.data_ptr(), yc.data_ptr(), w.data_ptr() if w is not None else None, n_outer, c,
                  i32(*([1] * pad + small)), i32(*([1] * pad + acc)), i32(*([1] * pad + ker)), nt, i64(*strides(xv)),
                  i64(*strides(yv)), code, _stream(x))
    # back to the input's axis order (time last)
    order = [a for a in range(nd) if a != time_axis]
    have = batch + kept
    y = yc.permute([have.index(a) for a in order] + [len(have)])
    return y if y.is_contiguous() else y.contiguous()


class AlignRows:
    """Raw outputs of ``align_rows``, the input's axes other than time in front and in the input's order: y like x
    (time last) or None, shift (Hz), phase (rad), quality fp64 and status int32 per transient (0 aligned, 1 window edge,
    2 non-finite, 3 nothing to go by, 4 step cap); averaging form: mean [voxels..., N] and n_averaged int32 per voxel."""

    __slots__ = ("y", "mean", "shift", "phase", "quality", "status", "n_averaged")

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)


ALIGN_MAX_POINTS = 8192
ALIGN_MAX_GRID = 1025
ALIGN_SKIP = {"coarse": _lib.XM_ALIGN_SKIP_COARSE, "refine": _lib.XM_ALIGN_SKIP_REFINE, "apply": _lib.XM_ALIGN_SKIP_APPLY}


def align_grid(n_points: int, dt: float, max_shift: float):
    """(delta, G) of the coarse grid of xm_align_rows: delta = 1 / (4 L dt), G = floor(max_shift / delta), and G = 0
    for a single point."""
    delta = 1.0 / (4.0 * n_points * dt)
    return delta, (int(np.floor(max_shift / delta)) if n_points >= 2 else 0)


def align_rows(x, average_axis: int, time_axis: int, reference, n_points: int, dt: float, t0: float = 0.0,
               max_shift: float = 20.0, average: bool = False, min_quality: float = 0.0, want_y: bool = True,
               workspace=None, _skip=()) -> AlignRows:
    """Frequency-and-phase alignment of every transient of the complex64 / complex128 device tensor `x` to its voxel's
    reference in one launch (xm_align_rows).  `reference`: a tensor shaped like x without
    `average_axis` (its time axis any length >= n_points), or 1-D along time, shared by all voxels.  `n_points`: the
    leading points L the fit uses.  With time as the last axis of a contiguous tensor the kernel addresses the average
    axis where it is; any other layout costs one contiguous copy (time moved last).  `average`: also the per-voxel mean
    of the aligned transients with status != 2 and quality >= min_quality (`want_y=False`: only that).  `_skip`
    (tests and timing only): stages to leave out, of "coarse", "refine", "apply"."""
    torch = _torch()
    _require_device(x)
    _require_device(reference)
    nd = x.dim()
    average_axis, time_axis = average_axis % nd, time_axis % nd
    if average_axis == time_axis:
        raise ValueError("average_axis and time_axis must differ")
    if reference.dtype != x.dtype:
        raise ValueError("reference must have x's dtype")

    def rows(a, axis):  # time last, C-contiguous
        if axis != a.dim() - 1:
            a = torch.movedim(a, axis, -1)
        return a if a.is_contiguous() else a.contiguous()

    aa = average_axis if average_axis < time_axis else average_axis - 1  # where the average axis is once time is last
    xr = rows(x, time_axis)
    code = _dtype_code(xr)
    shape = tuple(xr.shape)
    a_, n = shape[aa], shape[-1]
    n_outer = int(np.prod(shape[:aa], dtype=np.int64))
    n_inner = int(np.prod(shape[aa + 1:-1], dtype=np.int64))
    vox = shape[:aa] + shape[aa + 1:-1]
    if reference.dim() == 1:
        rr, stride = rows(reference, 0), 0
    else:
        if reference.dim() != nd - 1:
            raise ValueError("reference must be 1-D along time or have x's axes without the average axis")
        rr = rows(reference, time_axis if time_axis < average_axis else time_axis - 1)
        if tuple(rr.shape[:-1]) != vox:
            raise ValueError(f"reference shape {tuple(reference.shape)} does not match x {tuple(x.shape)} off the "
                             "average and time axes")
        stride = rr.shape[-1]
    n_ref = rr.shape[-1]
    if not average and not want_y:
        raise ValueError("want_y=False needs average=True")
    dev_ = x.device
    per = shape[:-1]
    y = torch.empty(shape, dtype=x.dtype, device=dev_) if want_y else None
    mean = torch.empty(vox + (n,), dtype=x.dtype, device=dev_) if average else None
    n_avg = torch.empty(vox, dtype=torch.int32, device=dev_) if average else None
    shift = torch.empty(per, dtype=torch.float64, device=dev_)
    phase = torch.empty(per, dtype=torch.float64, device=dev_)
    quality = torch.empty(per, dtype=torch.float64, device=dev_)
    status = torch.empty(per, dtype=torch.int32, device=dev_)
    work = workspace if workspace is not None else torch.zeros(_lib.XM_ALIGN_WORKSPACE_BYTES, dtype=torch.uint8, device=dev_)
    for k in _skip:
        code |= ALIGN_SKIP[k]
    ptr = lambda t_: t_.data_ptr() if t_ is not None else None  # noqa: E731
    _lib.call("xm_align_rows", xr.data_ptr(), rr.data_ptr(), stride, ptr(y), ptr(mean), shift.data_ptr(),
              phase.data_ptr(), quality.data_ptr(), status.data_ptr(), ptr(n_avg), n_outer, a_, n_inner, n, n_ref,
              int(n_points), float(dt), float(t0), float(max_shift), float(min_quality), code, work.data_ptr(), _stream(x))
    return AlignRows(y=y, mean=mean, shift=shift, phase=phase, quality=quality, status=status, n_averaged=n_avg)


class HsvdRows:
    """Raw outputs of ``hsvd_rows``, the input's axes other than time in front and in the input's order: y like x (time
    last) or None; frequency (Hz), damping (1/s), amplitude, phase (rad) fp64 and removed int32, each [..., K], sorted
    by frequency; n_removed and status int32 per row (0 done, 1 nothing in the band or an all-zero row, 2 non-finite,
    3 iteration cap, 4 degenerate poles or amplitudes)."""

    __slots__ = ("y", "frequency", "damping", "amplitude", "phase", "removed", "n_removed", "status")

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)


HSVD_MAX_COLS = 64
HSVD_MAX_RANK = 32
HSVD_MAX_POINTS = 16384
HSVD_STOP = {"gram": _lib.XM_HSVD_STOP_GRAM, "eig": _lib.XM_HSVD_STOP_EIG, "poles": _lib.XM_HSVD_STOP_POLES,
             "ampl": _lib.XM_HSVD_STOP_AMPL}


def hsvd_rows(x, time_axis: int, n_cols: int, rank: int, dt: float, band, want_y: bool = True, workspace=None,
              _gram_fma: bool = False, _stop=None) -> HsvdRows:
    """HSVD of every row of the complex64 / complex128 device tensor `x` along `time_axis` and removal of the components
    whose frequency lies in `band` = (f_lo, f_hi) Hz, in one launch (xm_hsvd_rows).  With time as
    the last axis the kernel reads the rows where they lie (one row stride; a tensor whose rows are not evenly spaced is
    copied); a time axis that is not last costs one contiguous copy.  `want_y=False`: the components alone.
    `_gram_fma` (tests and timing only): the Gram matrix on plain FMAs; `_stop`: end after "gram", "eig", "poles" or
    "ampl" (timing only)."""
    torch = _torch()
    _require_device(x)
    nd = x.dim()
    time_axis = time_axis % nd
    xr = torch.movedim(x, time_axis, -1) if time_axis != nd - 1 else x
    n = xr.shape[-1]
    lead = tuple(xr.shape[:-1])
    code = _dtype_code(xr)
    if xr.dim() == 2 and xr.stride(1) == 1 and xr.stride(0) >= n:
        stride = xr.stride(0)  # rows of a wider buffer, read in place
    else:
        xr = xr if xr.is_contiguous() else xr.contiguous()
        stride = n
    nb = int(np.prod(lead, dtype=np.int64))
    k = int(rank)
    dev_ = x.device
    y = torch.empty(lead + (n,), dtype=x.dtype, device=dev_) if want_y else None
    f64 = lambda: torch.empty(lead + (k,), dtype=torch.float64, device=dev_)  # noqa: E731
    freq, damp, amp, phase = f64(), f64(), f64(), f64()
    removed = torch.empty(lead + (k,), dtype=torch.int32, device=dev_)
    n_removed = torch.empty(lead, dtype=torch.int32, device=dev_)
    status = torch.empty(lead, dtype=torch.int32, device=dev_)
    work = workspace if workspace is not None else torch.zeros(_lib.XM_HSVD_WORKSPACE_BYTES, dtype=torch.uint8, device=dev_)
    if _gram_fma:
        code |= _lib.XM_HSVD_GRAM_FMA
    if _stop is not None:
        code |= HSVD_STOP[_stop]
    _lib.call("xm_hsvd_rows", xr.data_ptr(), int(stride), y.data_ptr() if y is not None else None, freq.data_ptr(),
              damp.data_ptr(), amp.data_ptr(), phase.data_ptr(), removed.data_ptr(), n_removed.data_ptr(),
              status.data_ptr(), nb, int(n), int(n_cols), k, float(dt), float(band[0]), float(band[1]), code,
              work.data_ptr(), _stream(x))
    return HsvdRows(y=y, frequency=freq, damping=damp, amplitude=amp, phase=phase, removed=removed,
                    n_removed=n_removed, status=status)


class DenoisePatches:
    """Raw outputs of ``denoise_patches`` in the input's axis order: y like x; rank int32, sigma fp64 and status int32
    per voxel, i.e. with x's axes other than time (0 done, 1 all-zero window, 2 non-finite sample, 3 Jacobi sweep cap)."""

    __slots__ = ("y", "rank", "sigma", "status")

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)


DENOISE_MAX_PATCH = 64
DENOISE_MAX_POINTS = 16384
DENOISE_STOP = {"gram": _lib.XM_DENOISE_STOP_GRAM, "eig": _lib.XM_DENOISE_STOP_EIG}


def denoise_patches(x, patch_axes, time_axis: int, patch, rank=None, workspace=None, _gram_fma: bool = False,
                    _stop=None) -> DenoisePatches:
    """Marchenko-Pastur patch PCA denoising of the complex64 / complex128 device tensor `x` in one launch
    (xm_denoise_patches).  `patch_axes`: 1 ... 3 axes the window extends over, `patch`: its size
    along each; every other axis but `time_axis` is batch.  `rank`: the number of components kept, or None for the
    Marchenko-Pastur rule.  With the patch axes adjacent, in the given order and right in front of a last time axis the
    kernel addresses the tensor where it lies; any other layout costs one contiguous copy.  `_gram_fma` (tests and
    timing only): the Gram matrix on plain FMAs at every patch size; `_stop`: end after "gram" or "eig" (timing only)."""
    torch = _torch()
    _require_device(x)
    nd = x.dim()
    time_axis = time_axis % nd
    axes = [int(a) % nd for a in patch_axes]
    patch = [int(p) for p in patch]
    if not 1 <= len(axes) <= 3:
        raise ValueError(f"patch_axes: needs 1 ... 3 axes, got {len(axes)}")
    if len(set(axes)) != len(axes) or time_axis in axes:
        raise ValueError("patch_axes must differ from each other and from time_axis")
    if len(patch) != len(axes):
        raise ValueError(f"patch: needs one size per patch axis ({len(axes)}), got {len(patch)}")
    batch = [a for a in range(nd) if a != time_axis and a not in axes]
    perm = batch + axes + [time_axis]
    xr = x.permute(perm) if perm != list(range(nd)) else x
    xr = xr if xr.is_contiguous() else xr.contiguous()
    shape = tuple(xr.shape)
    n = shape[-1]
    sizes = [1] * (3 - len(axes)) + list(shape[len(batch):-1])
    pp = [1] * (3 - len(axes)) + patch
    n_outer = int(np.prod(shape[:len(batch)], dtype=np.int64))
    code = _dtype_code(xr)
    dev_ = x.device
    y = torch.empty(shape, dtype=x.dtype, device=dev_)
    rk = torch.empty(shape[:-1], dtype=torch.int32, device=dev_)
    sigma = torch.empty(shape[:-1], dtype=torch.float64, device=dev_)
    status = torch.empty(shape[:-1], dtype=torch.int32, device=dev_)
    work = workspace if workspace is not None else torch.zeros(_lib.XM_DENOISE_WORKSPACE_BYTES, dtype=torch.uint8, device=dev_)
    if _gram_fma:
        code |= _lib.XM_DENOISE_GRAM_FMA
    if _stop is not None:
        code |= DENOISE_STOP[_stop]
    _lib.call("xm_denoise_patches", xr.data_ptr(), y.data_ptr(), rk.data_ptr(), sigma.data_ptr(), status.data_ptr(),
              n_outer, sizes[0], sizes[1], sizes[2], pp[0], pp[1], pp[2], int(n), -1 if rank is None else int(rank), code,
              work.data_ptr(), _stream(x))
    if perm != list(range(nd)):  # back to the input's axis order
        inv = [perm.index(a) for a in range(nd)]
        vperm = [a for a in perm if a != time_axis]
        vinv = [vperm.index(a) for a in range(nd) if a != time_axis]
        y = y.permute(inv)
        rk, sigma, status = rk.permute(vinv), sigma.permute(vinv), status.permute(vinv)
    return DenoisePatches(y=y, rank=rk, sigma=sigma, status=status)


AXIS_DFT_MAX = 64


def axis_dft(x, axis: int, table):
    """``y = table @ x`` along `axis` of the complex64 / complex128 device tensor `x` in one launch (xm_axis_dft,
    DESIGN.md section 14): `table` is [m, n] complex (host values or a device tensor; uploaded as complex128), n the
    size of `axis`, 1 <= n, m <= 64; the products and sums are fp64 and round once to x's dtype.  Any axis of a
    contiguous tensor is read where it lies; a tensor that is not contiguous costs one contiguous copy.  Returns a new
    tensor with m points along `axis`; `x` is left untouched."""
    _require_device(x)
    torch = _torch()
    code = _dtype_code(x)
    nd = x.dim()
    if nd == 0:
        raise ValueError("axis_dft needs at least one axis")
    axis = axis % nd
    if isinstance(table, torch.Tensor):
        t = table.to(device=x.device, dtype=torch.complex128).contiguous()
    else:
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(table, dtype=np.complex128))).to(x.device)
    n = x.shape[axis]
    if t.dim() != 2 or t.shape[1] != n:
        raise ValueError(f"table must be [m, {n}] for an axis of {n} points, got {tuple(t.shape)}")
    m = int(t.shape[0])
    xc = x if x.is_contiguous() else x.contiguous()
    shape = tuple(xc.shape)
    n_outer = int(np.prod(shape[:axis], dtype=np.int64))
    n_inner = int(np.prod(shape[axis + 1:], dtype=np.int64))
    out = torch.empty(shape[:axis] + (m,) + shape[axis + 1:], dtype=x.dtype, device=x.device)
    if n == 0:
        raise ValueError("axis_dft needs at least one point along the axis")
    if out.numel() == 0:
        return out
    _lib.call("xm_axis_dft", xc.data_ptr(), out.data_ptr(), t.data_ptr(), n_outer, int(n), m, n_inner, code, _stream(x))
    return out


class SparseTable:
    """A real sparse matrix [n_rows, n] in CSR form, checked on the host: the only form `axis_sparse` takes, because the
    kernel trusts its table and a column out of range would read out of bounds on the GPU.  `rowptr` must ascend from 0
    to ``len(col)``, every `col` must lie in [0, n) and every `val` must be finite (ValueError otherwise).  The arrays
    are copied and frozen; the device copies are made once per device and kept with the object."""

    __slots__ = ("rowptr", "col", "val", "n", "n_rows", "_device")

    def __init__(self, rowptr, col, val, n: int):
        rp, c, v = np.asarray(rowptr), np.asarray(col), np.asarray(val)
        if rp.ndim != 1 or c.ndim != 1 or v.ndim != 1 or rp.dtype.kind not in "iu" or c.dtype.kind not in "iu":
            raise ValueError("SparseTable: rowptr and col must be one-dimensional integer arrays, val one-dimensional")
        if v.dtype.kind not in "fiu":
            raise ValueError(f"SparseTable: val must be real, got {v.dtype}")
        n = int(n)
        if len(rp) < 2 or not 1 <= n < 2 ** 31 or len(rp) - 1 >= 2 ** 31 or len(c) >= 2 ** 31:
            raise ValueError("SparseTable: needs 1 <= n, n_rows < 2^31 and fewer than 2^31 entries")
        if len(v) != len(c):
            raise ValueError(f"SparseTable: {len(c)} col for {len(v)} val")
        rp = rp.astype(np.int64)
        if rp[0] != 0 or rp[-1] != len(c) or np.any(np.diff(rp) < 0):
            raise ValueError("SparseTable: rowptr must ascend from 0 to len(col)")
        if len(c) and (c.min() < 0 or c.max() >= n):
            bad = int(np.flatnonzero((c < 0) | (c >= n))[0])
            raise ValueError(f"SparseTable: col[{bad}] = {int(c[bad])} is outside [0, {n})")
        v = v.astype(np.float64)
        if not np.all(np.isfinite(v)):
            raise ValueError(f"SparseTable: val[{int(np.flatnonzero(~np.isfinite(v))[0])}] is not finite")
        self.rowptr, self.col, self.val = rp.astype(np.int32), c.astype(np.int32), v
        for a in (self.rowptr, self.col, self.val):
            a.setflags(write=False)
        self.n, self.n_rows = n, len(rp) - 1
        self._device = {}

    @property
    def nnz(self) -> int:
        return len(self.col)

    def __setattr__(self, name, value):
        if hasattr(self, "_device"):
            raise AttributeError("SparseTable is immutable")
        object.__setattr__(self, name, value)

    def _on(self, device):
        """(rowptr, col, val) tensors on `device`, uploaded on first use.  A table without entries still gets one
        element per array: the library takes no null pointer."""
        torch = _torch()
        key = str(device)
        if key not in self._device:
            self._device[key] = tuple(torch.from_numpy(a.copy() if len(a) else np.zeros(1, a.dtype)).to(device)
                                      for a in (self.rowptr, self.col, self.val))
        return self._device[key]


def axis_sparse(x, axis: int, table: SparseTable):
    """``y = table @ x`` along `axis` of the complex64 / complex128 device tensor `x` in one launch (xm_axis_sparse,
    DESIGN.md section 17): `table` is a `SparseTable` [n_rows, n] with n the size of `axis` -- nothing else is taken,
    the object is what has checked the indices.  Each output is the fp64 sum of its row's entries in their stored
    order, rounded once to x's dtype; a row without entries gives zero.  Any axis of a contiguous tensor is read where it
    lies; a tensor that is not contiguous costs one contiguous copy.  Returns a new tensor with n_rows points along
    `axis`; `x` is left untouched."""
    if not isinstance(table, SparseTable):
        raise TypeError(f"axis_sparse takes its table as a SparseTable only, got {type(table).__name__}")
    _require_device(x)
    torch = _torch()
    code = _dtype_code(x)
    nd = x.dim()
    if nd == 0:
        raise ValueError("axis_sparse needs at least one axis")
    axis = axis % nd
    n = x.shape[axis]
    if n != table.n:
        raise ValueError(f"table is bound to an axis of {table.n} points, the axis has {n}")
    xc = x if x.is_contiguous() else x.contiguous()
    shape = tuple(xc.shape)
    n_outer = int(np.prod(shape[:axis], dtype=np.int64))
    n_inner = int(np.prod(shape[axis + 1:], dtype=np.int64))
    out = torch.empty(shape[:axis] + (table.n_rows,) + shape[axis + 1:], dtype=x.dtype, device=x.device)
    if out.numel() == 0:
        return out
    rowptr, col, val = table._on(x.device)
    _lib.call("xm_axis_sparse", xc.data_ptr(), out.data_ptr(), rowptr.data_ptr(), col.data_ptr(), val.data_ptr(),
              n_outer, int(n), table.n_rows, n_inner, code, _stream(x))
    return out


CGS_MAX_COILS = 64
CGS_VOXELS = _lib.XM_CGS_VOXELS


def cgs_blocks(n_vox: int) -> int:
    """Voxel blocks, i.e. partials per column, of the CG-SENSE kernels."""
    return (int(n_vox) + CGS_VOXELS - 1) // CGS_VOXELS


def _cgs_c128(x, shape, what: str):
    torch = _torch()
    _require_device(x)
    if x.dtype != torch.complex128 or tuple(x.shape) != tuple(shape) or not x.is_contiguous():
        raise ValueError(f"{what} must be a contiguous complex128 tensor of shape {tuple(shape)}, got {tuple(x.shape)} of {x.dtype}")
    return x


def _cgs_plain(x, dtype, shape, what: str):
    _require_device(x)
    if x.dtype != dtype or tuple(x.shape) != tuple(shape) or not x.is_contiguous():
        raise ValueError(f"{what} must be a contiguous {dtype} tensor of shape {tuple(shape)}, got {tuple(x.shape)} of {x.dtype}")
    return x


def cgs_expand(r, p, s, rho_new, rho_old, status, first: bool, dtype, out=None):
    """One launch of k_cgs_expand (xm_cgs_expand): in place ``p <- r + (rho_new / rho_old) p`` for the
    columns whose `status` is 0 (``p <- r`` when `first`), then returns ``u[c, v, t] = s[c, v] p[v, t]`` rounded to `dtype`
    (torch.complex64 / complex128), [C, V, T].  r, p: [V, T] complex128; s: [C, V] complex128; rho_new, rho_old: the
    [NB, T] fp64 partials of this and the previous step's rho (read only when not `first`); status: [T] int32."""
    torch = _torch()
    c, v = (int(n) for n in s.shape)
    t = int(r.shape[1])
    _cgs_c128(r, (v, t), "r"), _cgs_c128(p, (v, t), "p"), _cgs_c128(s, (c, v), "s")
    nb = cgs_blocks(v)
    _cgs_plain(rho_new, torch.float64, (nb, t), "rho_new"), _cgs_plain(rho_old, torch.float64, (nb, t), "rho_old")
    _cgs_plain(status, torch.int32, (t,), "status")
    u = torch.empty((c, v, t), dtype=dtype, device=r.device) if out is None else _cgs_plain(out, dtype, (c, v, t), "out")
    _lib.call("xm_cgs_expand", r.data_ptr(), p.data_ptr(), s.data_ptr(), u.data_ptr(), rho_new.data_ptr(), rho_old.data_ptr(),
              status.data_ptr(), c, v, t, int(bool(first)), _dtype_code(u), _stream(r))
    return u


def cgs_reduce(u, s, p, q, part, lam: float = 0.0, initial: bool = False):
    """One launch of k_cgs_reduce (xm_cgs_reduce): ``q[v, t] = sum_c conj(s[c, v]) u[c, v, t] + lam p[v, t]`` and the
    [NB, T] partials of ``Re<p, q>`` into `part`; `initial`: no `lam` term, `p` is not read (may be None) and the partials
    are those of ``|q|^2``.  u: [C, V, T] complex64 / complex128; s, p, q as in `cgs_expand`."""
    torch = _torch()
    _require_device(u)
    c, v, t = (int(n) for n in u.shape)
    if not u.is_contiguous():
        raise ValueError("u must be contiguous")
    _cgs_c128(s, (c, v), "s"), _cgs_c128(q, (v, t), "q")
    if not initial:
        _cgs_c128(p, (v, t), "p")
    _cgs_plain(part, torch.float64, (cgs_blocks(v), t), "part")
    _lib.call("xm_cgs_reduce", u.data_ptr(), s.data_ptr(), None if initial else p.data_ptr(), q.data_ptr(), part.data_ptr(),
              c, v, t, float(lam), int(bool(initial)), _dtype_code(u), _stream(u))
    return q, part


def cgs_step(x, r, p, q, rho, rho0, delta, rho_out, status_in, status_out, n_iter, residual, tol: float, iteration: int,
             final: bool = False):
    """One launch of k_cgs_step (xm_cgs_step): per column whose `status_in` is 0 the stopping rules and, where none holds,
    ``alpha = rho / delta, x += alpha p, r -= alpha q``, the partials of ``|r|^2`` into `rho_out` and ``n_iter =
    iteration``; `final`: the rules alone (`delta` may be None).  rho, rho0, delta, rho_out: [NB, T] fp64 partials;
    status_in, status_out, n_iter: [T] int32; residual: [T] fp64."""
    torch = _torch()
    v, t = (int(n) for n in x.shape)
    nb = cgs_blocks(v)
    for a, name in ((x, "x"), (r, "r"), (p, "p"), (q, "q")):
        _cgs_c128(a, (v, t), name)
    for a, name in ((rho, "rho"), (rho0, "rho0"), (rho_out, "rho_out")) + (() if final else ((delta, "delta"),)):
        _cgs_plain(a, torch.float64, (nb, t), name)
    for a, name in ((status_in, "status_in"), (status_out, "status_out"), (n_iter, "n_iter")):
        _cgs_plain(a, torch.int32, (t,), name)
    _cgs_plain(residual, torch.float64, (t,), "residual")
    _lib.call("xm_cgs_step", x.data_ptr(), r.data_ptr(), p.data_ptr(), q.data_ptr(), rho.data_ptr(), rho0.data_ptr(),
              None if final else delta.data_ptr(), rho_out.data_ptr(), status_in.data_ptr(), status_out.data_ptr(),
              n_iter.data_ptr(), residual.data_ptr(), v, t, float(tol), int(iteration), int(bool(final)), _stream(x))


class CgSense:
    """Raw outputs of ``cg_sense``: x [V, T] complex128; residual [T] fp64 (sqrt(rho / rho0) at the last test of the
    column); iterations [T] int32; status [T] int32 (0 iteration cap, 1 converged, 2 breakdown: <p, A p> not positive,
    3 a right-hand side that is not finite: x is NaN)."""

    __slots__ = ("x", "residual", "iterations", "status")

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)


def cg_sense(y, s, adjoint, forward, lam: float, iterations: int, tol: float) -> CgSense:
    """Conjugate gradients on ``(E^H D E + lam I) x = E^H D y`` from x = 0, every column on its own (DESIGN.md section
    21).  y: [C, S, T] complex64 / complex128, contiguous; s: [C, V] complex128; `adjoint`: [C, S, T] -> the coil images
    [C, V, T] (gridding with the density, transform, crop), `forward`: its transpose with unit density -- the two NUFFT
    chains on raw tensors.  Queues a fixed sequence of launches, 3 of this module per iteration around the chains',
    and reads nothing back: the caller synchronises when it looks at the result."""
    torch = _torch()
    _require_device(y)
    c, v = (int(n) for n in s.shape)
    t = int(y.shape[2])
    dev_ = y.device
    nb = cgs_blocks(v)
    c128 = dict(dtype=torch.complex128, device=dev_)
    x = torch.zeros((v, t), **c128)
    r, p, q = (torch.empty((v, t), **c128) for _ in range(3))
    rho0, delta = (torch.empty((nb, t), dtype=torch.float64, device=dev_) for _ in range(2))
    rho = torch.empty((2, nb, t), dtype=torch.float64, device=dev_)
    status = torch.zeros((2, t), dtype=torch.int32, device=dev_)
    n_iter = torch.zeros(t, dtype=torch.int32, device=dev_)
    residual = torch.zeros(t, dtype=torch.float64, device=dev_)

    cgs_reduce(adjoint(y).reshape(c, v, t), s, None, r, rho0, initial=True)
    for k in range(iterations):
        now = rho0 if k == 0 else rho[k % 2]
        before = rho0 if k <= 1 else rho[(k - 1) % 2]
        u = cgs_expand(r, p, s, now, before, status[k % 2], k == 0, y.dtype)
        u = adjoint(forward(u)).reshape(c, v, t)
        cgs_reduce(u, s, p, q, delta, lam)
        cgs_step(x, r, p, q, now, rho0, delta, rho[(k + 1) % 2], status[k % 2], status[(k + 1) % 2], n_iter, residual, tol,
                 k + 1)
    n = iterations
    cgs_step(x, r, p, q, rho0 if n == 0 else rho[n % 2], rho0, None, rho[(n + 1) % 2], status[n % 2], status[(n + 1) % 2],
             n_iter, residual, tol, n, final=True)
    return CgSense(x=x, residual=residual, iterations=n_iter, status=status[(n + 1) % 2])


L1_MAX_BLOCK = _lib.XM_L1_MAX_BLOCK


def l1_blocks(matrix, levels) -> int:
    """Haar blocks, i.e. partials per column, of k_l1_prox."""
    return int(np.prod([int(m) >> int(l) for m, l in zip(matrix, levels)], dtype=np.int64))


def _l1_three(values, fill: int):
    values = [int(a) for a in values]
    return values + [fill] * (3 - len(values))


def l1_start(b, x, bmax, status, change):
    """The two launches of k_l1_start (xm_l1_start): ``bmax[t] = max_v |b[v, t]|`` and ``status[t] =
    0``; a column whose maximum is not finite gets status 3, a NaN `bmax` and `change` and a NaN column of `x`.
    b, x: [V, T] complex128; bmax, change: [T] fp64; status: [T] int32."""
    torch = _torch()
    v, t = (int(n) for n in b.shape)
    _cgs_c128(b, (v, t), "b"), _cgs_c128(x, (v, t), "x")
    _cgs_plain(bmax, torch.float64, (t,), "bmax"), _cgs_plain(change, torch.float64, (t,), "change")
    _cgs_plain(status, torch.int32, (t,), "status")
    part = torch.empty(((v + L1_MAX_BLOCK - 1) // L1_MAX_BLOCK, t), dtype=torch.float64, device=b.device)
    _lib.call("xm_l1_start", b.data_ptr(), part.data_ptr(), None, None, None, None, v, t, 0, _stream(b))
    _lib.call("xm_l1_start", None, part.data_ptr(), bmax.data_ptr(), status.data_ptr(), change.data_ptr(), x.data_ptr(), v, t,
              1, _stream(b))


def l1_prox(x, v, q, b, mask, bmax, d2_in, n2_in, d2_out, n2_out, status_in, status_out, n_iter, change, matrix, levels,
            shift, tau: float, theta_scale: float, beta: float, tol: float, iteration: int, mode: int = 0):
    """One launch of k_l1_prox (xm_l1_prox): per column whose `status_in` is 0 the stopping test on the totals of `d2_in`,
    `n2_in` and, where it does not hold, ``w = v - tau (q - b)``, the blockwise Haar transform of `levels` on the lattice
    moved by `shift`, the shrink of the detail coefficients by ``theta_scale bmax``, the transform back, the mask, ``v <-
    x' + beta (x' - x)``, ``x <- x'`` and the partials of ``|x' - x|^2`` and ``|x'|^2``.  `mode`: 0 a step, 1 the first
    step (no test; q, d2_in and n2_in may be None), 2 the final test alone.  x, v, q, b: [V, T] complex128, V the product of
    `matrix`; mask: [V] uint8; bmax, change: [T] fp64; the partials: [l1_blocks, T] fp64; status_in, status_out, n_iter: [T]
    int32."""
    torch = _torch()
    vox, t = (int(n) for n in x.shape)
    if int(np.prod(matrix, dtype=np.int64)) != vox or not len(matrix) == len(levels) == len(shift) or not 1 <= len(matrix) <= 3:
        raise ValueError(f"matrix {tuple(matrix)}, levels {tuple(levels)} and shift {tuple(shift)} do not describe the {vox} voxels of x")
    nb = l1_blocks(matrix, levels)
    first = mode == 1
    for a, name in ((x, "x"), (v, "v"), (b, "b")) + (() if first else ((q, "q"),)):
        _cgs_c128(a, (vox, t), name)
    for a, name in ((d2_out, "d2_out"), (n2_out, "n2_out")) + (() if first else ((d2_in, "d2_in"), (n2_in, "n2_in"))):
        _cgs_plain(a, torch.float64, (nb, t), name)
    for a, name in ((status_in, "status_in"), (status_out, "status_out"), (n_iter, "n_iter")):
        _cgs_plain(a, torch.int32, (t,), name)
    _cgs_plain(bmax, torch.float64, (t,), "bmax"), _cgs_plain(change, torch.float64, (t,), "change")
    _cgs_plain(mask, torch.uint8, (vox,), "mask")
    ptr = lambda a: None if a is None else a.data_ptr()  # noqa: E731
    _lib.call("xm_l1_prox", x.data_ptr(), v.data_ptr(), None if first else q.data_ptr(), b.data_ptr(), mask.data_ptr(),
              bmax.data_ptr(), None if first else ptr(d2_in), None if first else ptr(n2_in), d2_out.data_ptr(),
              n2_out.data_ptr(), status_in.data_ptr(), status_out.data_ptr(), n_iter.data_ptr(), change.data_ptr(),
              len(matrix), *_l1_three(matrix, 1), *_l1_three(levels, 0), *_l1_three(shift, 0), t, float(tau),
              float(theta_scale), float(beta), float(tol), int(iteration), int(mode), _stream(x))


def fista_momentum(iterations: int):
    """beta_k = (t_k - 1) / t_{k+1} with t_0 = 1, t_{k+1} = (1 + sqrt(1 + 4 t_k^2)) / 2, k = 0 ... iterations - 1."""
    out, tk = [], 1.0
    for _ in range(int(iterations)):
        nxt = (1.0 + math.sqrt(1.0 + 4.0 * tk * tk)) / 2.0
        out.append((tk - 1.0) / nxt)
        tk = nxt
    return out


def l1_lipschitz(s, adjoint, forward, mask, power_iterations: int, dtype) -> float:
    """The Rayleigh quotient of ``E^H D E`` after `power_iterations` power steps from the mask indicator, on one column
    through the launches of the iteration: k_cgs_expand (first) gives u = s v, the two chains, k_cgs_reduce gives q and
    Re<v, q>.  Set-up: the host reads the scalars of every step.  s: [C, V] complex128; mask: [V] uint8; `dtype`: that of
    the coil-sized arrays."""
    torch = _torch()
    _require_device(s)
    c, v = (int(n) for n in s.shape)
    nb = cgs_blocks(v)
    vec = mask.to(torch.complex128).reshape(v, 1).contiguous()
    norm = float(torch.linalg.vector_norm(vec))
    if not norm > 0.0:
        return 0.0
    vec = vec / norm
    p, q = torch.zeros_like(vec), torch.empty_like(vec)
    part = torch.zeros((nb, 1), dtype=torch.float64, device=s.device)
    live = torch.zeros(1, dtype=torch.int32, device=s.device)
    for k in range(int(power_iterations) + 1):
        u = cgs_expand(vec, p, s, part, part, live, True, dtype)
        cgs_reduce(adjoint(forward(u)).reshape(c, v, 1), s, p, q, part, 0.0)
        quotient = float(part.sum())
        norm = float(torch.linalg.vector_norm(q))
        if k == power_iterations or not norm > 0.0 or not math.isfinite(norm):
            break
        vec = q / norm
    return quotient


class L1Sense:
    """Raw outputs of ``l1_sense``: x [V, T] complex128; change [T] fp64 (sqrt(d2 / n2) at the last test of the column);
    iterations [T] int32; status [T] int32 (0 iteration cap, 1 converged, 3 not finite: x is NaN)."""

    __slots__ = ("x", "change", "iterations", "status")

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)


def l1_sense(y, s, adjoint, forward, mask, matrix, levels, lam2: float, sparsity: float, tau: float, iterations: int,
             tol: float, cycle_spin: bool = False) -> L1Sense:
    """FISTA on ``1/2 |D^(1/2) (E x - y)|^2 + lam2 / 2 |x|^2 + sparsity max|b| |Psi x|_1`` from x = 0, every column on its
    own.  y, s, `adjoint`, `forward` as in `cg_sense`; mask: [V] uint8; `tau`: the step 1 / L.
    Queues a fixed sequence of launches -- per step k_cgs_expand (first), the two chains, k_cgs_reduce and k_l1_prox; the
    first step has the prox alone -- and reads nothing back."""
    torch = _torch()
    _require_device(y)
    c, v = (int(n) for n in s.shape)
    t = int(y.shape[2])
    dev_ = y.device
    nb = l1_blocks(matrix, levels)
    c128 = dict(dtype=torch.complex128, device=dev_)
    f64 = dict(dtype=torch.float64, device=dev_)
    x, vk, p = (torch.zeros((v, t), **c128) for _ in range(3))
    b, q = (torch.empty((v, t), **c128) for _ in range(2))
    scratch = torch.empty((cgs_blocks(v), t), **f64)  # the partials of k_cgs_reduce, which nothing here reads
    d2, n2 = (torch.empty((2, nb, t), **f64) for _ in range(2))
    status = torch.zeros((2, t), dtype=torch.int32, device=dev_)
    n_iter = torch.zeros(t, dtype=torch.int32, device=dev_)
    bmax, change = (torch.zeros(t, **f64) for _ in range(2))

    cgs_reduce(adjoint(y).reshape(c, v, t), s, None, b, scratch, initial=True)
    l1_start(b, x, bmax, status[0], change)
    n = int(iterations)
    zero = [0] * len(matrix)
    for k, beta in enumerate(fista_momentum(n)):
        now, nxt = k % 2, (k + 1) % 2
        if k:
            u = cgs_expand(vk, p, s, scratch, scratch, status[now], True, y.dtype)
            cgs_reduce(adjoint(forward(u)).reshape(c, v, t), s, p, q, scratch, lam2)
        shift = [k % (1 << int(l)) for l in levels] if cycle_spin else zero
        l1_prox(x, vk, q, b, mask, bmax, d2[now], n2[now], d2[nxt], n2[nxt], status[now], status[nxt], n_iter, change,
                matrix, levels, shift, tau, tau * sparsity, beta, tol, k + 1, 1 if k == 0 else 0)
    if n == 0:
        return L1Sense(x=x, change=change, iterations=n_iter, status=status[0])
    l1_prox(x, vk, q, b, mask, bmax, d2[n % 2], n2[n % 2], d2[(n + 1) % 2], n2[(n + 1) % 2], status[n % 2],
            status[(n + 1) % 2], n_iter, change, matrix, levels, zero, tau, tau * sparsity, 0.0, tol, n, 2)
    return L1Sense(x=x, change=change, iterations=n_iter, status=status[(n + 1) % 2])


class EspiritEig:
    """Raw outputs of ``espirit_eig``: maps [M, C, V] complex128, values [M, V] fp64 (descending over M), status [V]
    int32 (0 ok, 1 Jacobi sweep cap, 2 non-finite entry: maps 0, values NaN)."""

    __slots__ = ("maps", "values", "status")

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)


ESPIRIT_MAX_COILS = 64


def espirit_entries(c: int) -> int:
    """Entries of the upper triangle of a c x c matrix, the trailing axis of ``espirit_eig``'s input."""
    return int(c) * (int(c) + 1) // 2


def espirit_eig(h, n_coils: int, n_maps: int = 1, phase_ref: int = 0, crop: float = 0.8) -> EspiritEig:
    """The `n_maps` (1 or 2) largest eigenpairs of one Hermitian matrix per voxel in one launch (xm_espirit_eig,
    DESIGN.md section 22).  h: [V, E] complex128 device tensor, per voxel the upper triangle (i <= j, row-major) of its
    `n_coils` x `n_coils` matrix, E = n_coils (n_coils + 1) / 2.  Each eigenvector has unit norm and its component
    `phase_ref` real and >= 0; a map whose eigenvalue is below `crop` is exact zeros."""
    torch = _torch()
    _require_device(h)
    c, m = int(n_coils), int(n_maps)
    if not 1 <= c <= ESPIRIT_MAX_COILS:
        raise ValueError(f"n_coils must be in 1 ... {ESPIRIT_MAX_COILS}, got {n_coils!r}")
    if h.dtype != torch.complex128 or h.dim() != 2 or h.shape[1] != espirit_entries(c) or h.shape[0] < 1:
        raise ValueError(f"h must be a complex128 tensor [V >= 1, {espirit_entries(c)}] for {c} coils, got "
                         f"{tuple(h.shape)} of {h.dtype}")
    hc = h if h.is_contiguous() else h.contiguous()
    v = int(hc.shape[0])
    maps = torch.empty((m, c, v), dtype=torch.complex128, device=h.device)
    values = torch.empty((m, v), dtype=torch.float64, device=h.device)
    status = torch.empty((v,), dtype=torch.int32, device=h.device)
    _lib.call("xm_espirit_eig", hc.data_ptr(), maps.data_ptr(), values.data_ptr(), status.data_ptr(), v, c, m,
              int(phase_ref), float(crop), _stream(h))
    return EspiritEig(maps=maps, values=values, status=status)


def shift_time_fused(L: int, complex128: bool = False) -> bool:
    """True when `shift_time` runs transform length `L` as one launch of k_shift_time (`xm_shift_time_fused`)."""
    return bool(_lib.load().xm_shift_time_fused(int(L), _lib.XM_C128 if complex128 else _lib.XM_C64))


def _shift_ramp(frac, L: int):
    """exp(-2 pi i kappa_k phi / L) for each phi of `frac` (fp64 device tensor) -> [len(frac), L] complex128: the staged
    route's ramp, with kappa phi / L reduced modulo 1 on the integer part of phi as the kernel does (every product below
    is an exact integer in fp64)."""
    torch = _torch()
    k = torch.arange(L, dtype=torch.float64, device=frac.device)
    kappa = torch.where(k < (L + 1) // 2, k, k - L)
    whole = torch.round(frac)
    part = frac - whole
    m = torch.remainder(kappa[None, :] * torch.remainder(whole, L)[:, None], L)
    angle = (-2.0 * np.pi) * ((m + kappa[None, :] * part[:, None]) / L)
    return torch.complex(torch.cos(angle), torch.sin(angle))


def shift_time(x, axis: int, frac, n_delay: int | None = None, delay_div: int = 1, L: int | None = None,
               staged: bool = False):
    """Each row of `x` along `axis` delayed by its own number of dwells (`xm_shift_time`): with
    `axis` moved last and the rest flattened, row r takes ``frac[(r // delay_div) % n_delay]``; `frac` holds `n_delay`
    fp64 values (host values or a device tensor), `L` >= the axis length is the transform length (default: the axis
    length).  One launch of k_shift_time where `shift_time_fused(L)`; any other length -- chirp-z lengths, lengths above
    16384, complex128 16384 -- and `staged=True` take the same definition in stages: zero fill, transform, the ramp
    (built in fp64 on the device), inverse transform, crop.  Returns a new tensor of x's shape; `x` is left untouched."""
    _require_device(x)
    torch = _torch()
    code = _dtype_code(x)
    x2, restore = _rows(x, axis)
    nb, n = x2.shape
    L = n if L is None else int(L)
    if L < n:
        raise ValueError(f"L: the transform length {L} is shorter than the axis ({n} points)")
    if isinstance(frac, torch.Tensor):
        fr = frac.to(device=x.device, dtype=torch.float64).reshape(-1).contiguous()
    else:
        fr = torch.from_numpy(np.array(frac, dtype=np.float64).reshape(-1)).to(x.device)
    n_delay = fr.numel() if n_delay is None else int(n_delay)
    delay_div = int(delay_div)
    if n_delay < 1 or n_delay != fr.numel() or delay_div < 1:
        raise ValueError(f"frac: {fr.numel()} delays for n_delay = {n_delay}, delay_div = {delay_div}")
    if nb == 0 or n == 0:
        return restore(torch.empty_like(x2))
    if not staged and shift_time_fused(L, x.dtype == torch.complex128):
        out = torch.empty_like(x2)
        _lib.call("xm_shift_time", x2.data_ptr(), n, out.data_ptr(), nb, n, L, fr.data_ptr(), n_delay, delay_div, code,
                  _stream(x))
        return restore(out)
    spec = fft(zero_fill(x2, 1, L) if L > n else x2, 1, inverse=False, ortho=False)
    ramp = _shift_ramp(fr, L).to(x.dtype)  # rounded once to the storage precision
    period = n_delay * delay_div
    if nb % period == 0:
        spec.view(nb // period, n_delay, delay_div, L).mul_(ramp[None, :, None, :])
    else:
        spec.mul_(ramp[(torch.arange(nb, device=x.device) // delay_div) % n_delay])
    y = fft(spec, 1, inverse=True, ortho=False)
    return restore(y[:, :n].contiguous() if L > n else y)


class SpeciesResult:
    """Raw outputs of ``species_separate``: species like x with the echo axis replaced by the M species; per row (the
    axes that are neither echo nor columns, in the input's order) field fp64 (Hz), residual fp64 (field fit only, else
    None) and status int32 (0 done, 1 window end, 2 non-finite, 3 all-zero row, 4 step cap).  `copied`: whether the
    layout needed the one contiguous copy; `levels`: the (row, column) index levels the kernel addressed."""

    __slots__ = ("species", "field", "residual", "status", "copied", "levels")

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)


SPECIES_MAX_ECHOES = 32
SPECIES_MAX_ECHOES_FIT = 16
SPECIES_MAX_SPECIES = 8
SPECIES_MAX_GRID = 1025
SPECIES_SKIP = {"gram": _lib.XM_SPECIES_SKIP_GRAM, "coarse": _lib.XM_SPECIES_SKIP_COARSE,
                "refine": _lib.XM_SPECIES_SKIP_REFINE, "apply": _lib.XM_SPECIES_SKIP_APPLY}


def species_grid(echo_times, max_field: float):
    """(delta, G) of the coarse grid of the field fit: delta = 1 / (4 (max TE - min TE)), G = floor(max_field / delta)."""
    te = np.asarray(echo_times, dtype=np.float64)
    delta = 1.0 / (4.0 * float(te.max() - te.min()))
    return delta, int(np.floor(max_field / delta))


def species_tables(echo_times, frequencies, decay=None, fit: bool = False):
    """Host fp64 tables of xm_species_separate as one flat array: TE[E], f[M], R[M], P0 = pinv(A0) as (re, im), and with
    `fit` the diagonal of Pi = Q Q^H (Q from the QR of A0) and Pi[e', e] for the pairs e < e' in ascending order."""
    te = np.asarray(echo_times, dtype=np.float64).reshape(-1)
    f = np.asarray(frequencies, dtype=np.float64).reshape(-1)
    r = np.zeros_like(f) if decay is None else np.asarray(decay, dtype=np.float64).reshape(-1)
    a0 = np.exp((2j * np.pi * f - r)[None, :] * te[:, None])
    p0 = np.linalg.pinv(a0)
    parts = [te, f, r, np.stack([p0.real, p0.imag], axis=-1).reshape(-1)]
    if fit:
        q = np.linalg.qr(a0)[0]
        pi = q @ q.conj().T
        iu = np.triu_indices(len(te), 1)  # (e, e') ascending, e < e'
        low = pi[iu[1], iu[0]]
        parts += [np.diagonal(pi).real, np.stack([low.real, low.imag], axis=-1).reshape(-1)]
    return np.ascontiguousarray(np.concatenate(parts))


_SPECIES_TABLES = {}  # (device, fit, the model's bytes) -> the tables in HBM; a handful of models per session


def _species_tables_on(device, te, f, r, fit: bool):
    """`species_tables` uploaded once per model and device (the upload is a blocking copy: not one per call)."""
    torch = _torch()
    r = np.zeros_like(np.asarray(f, dtype=np.float64).reshape(-1)) if r is None else np.asarray(r, dtype=np.float64).reshape(-1)
    key = (str(device), bool(fit), te.tobytes(), np.asarray(f, dtype=np.float64).tobytes(), r.tobytes())
    t = _SPECIES_TABLES.get(key)
    if t is None:
        if len(_SPECIES_TABLES) >= 32:
            _SPECIES_TABLES.clear()
        t = _SPECIES_TABLES[key] = torch.from_numpy(species_tables(te, f, r, fit)).to(device)
    return t


def _collapse(sizes, strides):
    """Index levels of axes given outermost first: `strides` lists, per axis, its stride in every array that is
    addressed (x, y, tau, psi).  Axes of size 1 drop out; neighbours merge when in every array the outer stride is the
    inner one times the inner size.  Returns [(size, strides), ...]."""
    out = []
    for n, st in zip(sizes, strides):
        if n == 1:
            continue
        if out and all(a == b * n for a, b in zip(out[-1][1], st)):
            out[-1] = (out[-1][0] * n, tuple(st))
        else:
            out.append((n, tuple(st)))
    return out


def species_separate(x, echo_axis: int, col_axes, echo_times, frequencies, decay=None, tau=None, psi=None,
                     fit_field: bool = False, max_field=None, _skip=()) -> SpeciesResult:
    """Least-squares separation of M chemical species from the E echoes of the complex64 / complex128 device tensor `x`
    in one launch of k_species (xm_species_separate).  `col_axes`: the axes that share a row's
    readout delay and field offset (coils); every axis that is neither `echo_axis` nor a column axis is a row axis.
    `tau` (s) and `psi` (Hz): None, or fp64 values that broadcast against the row axes in the input's order.
    `fit_field`: psi is fitted per row within +-`max_field` Hz from all columns of the row.  The tensor is addressed
    where it lies whenever the row axes collapse into at most two strided index levels and the column axes into at
    most two; any other layout costs one contiguous copy with the rows in front (`copied` on the result says which).
    `_skip` (tests and timing only): stages to leave out, of "gram", "coarse", "refine", "apply"."""
    torch = _torch()
    _require_device(x)
    code = _dtype_code(x)
    nd = x.dim()
    ea = echo_axis % nd
    cols = [a % nd for a in col_axes]
    if ea in cols or len(set(cols)) != len(cols):
        raise ValueError("col_axes must be distinct axes other than echo_axis")
    rows = [a for a in range(nd) if a != ea and a not in cols]
    cols = sorted(cols)
    te = np.asarray(echo_times, dtype=np.float64).reshape(-1)
    E, M = x.shape[ea], int(np.size(frequencies))
    if len(te) != E:
        raise ValueError(f"echo_times: {len(te)} values for {E} echoes")
    if fit_field and psi is not None:
        raise ValueError("psi and fit_field exclude each other")
    tables = _species_tables_on(x.device, te, frequencies, decay, bool(fit_field))
    row_shape = tuple(x.shape[a] for a in rows)
    oshape = tuple(M if a == ea else x.shape[a] for a in range(nd))
    y = torch.empty(oshape, dtype=x.dtype, device=x.device)
    field = torch.empty(row_shape, dtype=torch.float64, device=x.device)
    status = torch.empty(row_shape, dtype=torch.int32, device=x.device)
    residual = torch.empty(row_shape, dtype=torch.float64, device=x.device) if fit_field else None

    def per_row(v):
        if v is None:
            return None
        if not isinstance(v, torch.Tensor):
            v = torch.from_numpy(np.asarray(v, dtype=np.float64))
        v = v.to(device=x.device, dtype=torch.float64)
        return torch.broadcast_to(v, row_shape)

    tau_t, psi_t = per_row(tau), per_row(psi)

    def levels(xs, ys, tt, pt):
        per = [t_ for t_ in (tt, pt) if t_ is not None]
        rl = _collapse(row_shape, [[xs.stride(a), ys.stride(a)] + [t_.stride(i) for t_ in per] for i, a in enumerate(rows)])
        cl = _collapse([xs.shape[a] for a in cols], [[xs.stride(a), ys.stride(a)] for a in cols])
        return rl, cl, per

    rl, cl, per = levels(x, y, tau_t, psi_t)
    if len(rl) > 2 and per:  # the per-row values in the rows' own order: they then merge wherever x does
        tau_t = tau_t.contiguous() if tau_t is not None else None
        psi_t = psi_t.contiguous() if psi_t is not None else None
        rl, cl, per = levels(x, y, tau_t, psi_t)
    xs, ys, copied = x, y, False
    if len(rl) > 2 or len(cl) > 2:  # one contiguous copy: rows, echo, columns
        order = rows + [ea] + cols
        xs = x.permute(order).contiguous()
        ys = torch.empty(tuple(oshape[a] for a in order), dtype=x.dtype, device=x.device)
        inv = [order.index(a) for a in range(nd)]
        xs, ys, copied = xs.permute(inv), ys.permute(inv), True  # the input's axis numbering, the copy's strides
        tau_t = tau_t.contiguous() if tau_t is not None else None
        psi_t = psi_t.contiguous() if psi_t is not None else None
        rl, cl, per = levels(xs, ys, tau_t, psi_t)
    rl = [(1, (0,) * (2 + len(per)))] * (2 - len(rl)) + rl
    cl = [(1, (0, 0))] * (2 - len(cl)) + cl
    i64 = lambda *v: (ctypes.c_int64 * len(v))(*[int(q) for q in v])  # noqa: E731
    dims = i64(rl[0][0], rl[1][0], cl[0][0], cl[1][0])
    xst = i64(rl[0][1][0], rl[1][1][0], cl[0][1][0], cl[1][1][0], xs.stride(ea))
    yst = i64(rl[0][1][1], rl[1][1][1], cl[0][1][1], cl[1][1][1], ys.stride(ea))
    k = 2
    ts = ps = (0, 0)
    if tau_t is not None:
        ts, k = (rl[0][1][k], rl[1][1][k]), k + 1
    if psi_t is not None:
        ps = (rl[0][1][k], rl[1][1][k])
    span = float(te.max() - te.min()) if E else 0.0
    for s in _skip:
        code |= SPECIES_SKIP[s]
    ptr = lambda t_: t_.data_ptr() if t_ is not None else None  # noqa: E731
    _lib.call("xm_species_separate", xs.data_ptr(), ys.data_ptr(), dims, xst, yst, E, M, tables.data_ptr(), ptr(tau_t),
              ts[0], ts[1], ptr(psi_t), ps[0], ps[1], field.data_ptr(), ptr(residual), status.data_ptr(),
              1 if fit_field else 0, float(max_field) if fit_field else 0.0, span, code, _stream(x))
    if copied:
        y.copy_(ys)
    return SpeciesResult(species=y, field=field, residual=residual, status=status, copied=copied,
                         levels=(sum(n > 1 for n, _ in rl), sum(n > 1 for n, _ in cl)))


class LipidResult:
    """Raw outputs of ``lipid_project``: `out` like x, `status` int32 per row (0 done, 1 copied, 2 non-finite sample:
    NaN); `copied`: whether the layout needed the one contiguous copy."""

    __slots__ = ("out", "status", "copied")

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)


LIPID_MAX_RANK = 64
LIPID_MIN_POINTS = 2
LIPID_MAX_POINTS = 65536
LIPID_FLAGS = {"fma": _lib.XM_LIPID_FMA, "coef": _lib.XM_LIPID_SKIP_COEF, "apply": _lib.XM_LIPID_SKIP_APPLY}


def lipid_rows(x, axes, mask):
    """The rows of the device tensor `x` ([..., time]) whose position along the leading `axes` lies inside the boolean
    host array `mask` (shape: the sizes of `axes`), as one [n, time] complex128 tensor; every other leading axis
    contributes rows."""
    torch = _torch()
    _require_device(x)
    lead = list(range(x.dim() - 1))
    axes = [a % x.dim() for a in axes]
    perm = axes + [a for a in lead if a not in axes] + [x.dim() - 1]
    m = torch.from_numpy(np.array(mask, dtype=np.bool_)).to(x.device)  # (a copy: the caller's mask may be read-only)
    return x.permute(perm)[m].reshape(-1, x.shape[-1]).to(torch.complex128)


def lipid_subspace(L, kmax: int = LIPID_MAX_RANK):
    """Singular values (all min(n, T), descending, ties to the lower index) and the first `kmax` left vectors u_k (host
    complex128 [T, k]) of M = L^T, L the [n, T] complex device tensor of lipid FIDs.  The Gram matrix, whichever of
    M M^H (T x T) and M^H M (n x n) is smaller, is one complex128 matmul on the device; its Hermitian eigen-decomposition
    is host numpy; with the n x n form u_k = M v_k / sigma_k is a second matmul on the device (a component with
    sigma_k = 0 has u_k = 0).  A non-finite Gram matrix raises ValueError."""
    torch = _torch()
    _require_device(L)
    L = L.to(torch.complex128)
    n, T = L.shape
    small_t = T <= n
    G = (L.transpose(0, 1) @ L.conj()) if small_t else (L.conj() @ L.transpose(0, 1))
    g = G.cpu().numpy()
    if not np.all(np.isfinite(g.view(np.float64))):
        raise ValueError("the lipid basis has a non-finite sample (or its Gram matrix overflows)")
    ev, vec = np.linalg.eigh(0.5 * (g + g.conj().T))
    order = np.argsort(-ev, kind="stable")
    sigma = np.sqrt(np.maximum(ev[order], 0.0))
    k = min(int(kmax), len(sigma))
    v = np.ascontiguousarray(vec[:, order[:k]])
    if small_t:
        return sigma, v
    inv = np.where(sigma[:k] > 0, 1.0 / np.where(sigma[:k] > 0, sigma[:k], 1.0), 0.0)
    u = (L.transpose(0, 1) @ torch.from_numpy(v * inv[None, :]).to(L.device)).cpu().numpy()
    return sigma, np.ascontiguousarray(u)


def lipid_tables(U, w, device=None):
    """The fp64 table of xm_lipid_project, U[T][r] as (re, im) then w[r]: a host array, or with `device` the tensor there."""
    U = np.asarray(U, dtype=np.complex128)
    w = np.asarray(w, dtype=np.float64).reshape(-1)
    if U.ndim != 2 or U.shape[1] != len(w):
        raise ValueError(f"lipid_tables: U must be [T, r] with one weight per column, got {U.shape} and {len(w)} weights")
    tab = np.concatenate([np.stack([U.real, U.imag], axis=-1).reshape(-1), w])
    return tab if device is None else _torch().from_numpy(np.ascontiguousarray(tab)).to(device)


def lipid_project(x, basis_record, apply=None, out=None, form=None, _skip=()) -> LipidResult:
    """out = x - U diag(w) U^H x along the last axis of the complex64 / complex128 device tensor `x` in one launch of
    k_lipid_project (xm_lipid_project).  `basis_record`: anything with ``rank``, ``n_time`` and
    ``table_on(device)`` (a ``LipidBasis``).  `apply`: None, or a boolean array / tensor of x's leading shape; rows
    where it is false are copied bit for bit.  `out`: None (a fresh tensor), or a tensor of x's shape, dtype and layout
    class; ``out is x`` works in place.  The tensor is addressed where it lies when its time stride is 1 and the
    leading axes collapse into one strided row level; any other layout costs one contiguous copy (`copied`).
    `form`: None / "mfma" (the fp64 matrix cores) or "fma"; `_skip` (timing only): of "coef", "apply"."""
    torch = _torch()
    _require_device(x)
    code = _dtype_code(x)
    if x.dim() < 1:
        raise ValueError("lipid_project needs at least the time axis")
    T, r = int(x.shape[-1]), int(basis_record.rank)
    if T != int(basis_record.n_time):
        raise ValueError(f"lipid_project: the data has {T} points along time, the basis {basis_record.n_time}")
    if form not in (None, "mfma", "fma"):
        raise ValueError(f"form must be 'mfma' or 'fma', got {form!r}")
    lead = tuple(x.shape[:-1])
    n_rows = int(np.prod(lead, dtype=np.int64)) if lead else 1
    tables = basis_record.table_on(x.device)

    def row_level(t_):
        if t_.shape[-1] > 1 and t_.stride(-1) != 1:
            return None
        lv = _collapse(lead, [[t_.stride(a)] for a in range(len(lead))])
        if len(lv) > 1 or (lv and lv[0][1][0] < T):
            return None
        return lv[0][1][0] if lv else T

    in_place = out is x
    if out is not None and (tuple(out.shape) != tuple(x.shape) or out.dtype != x.dtype or out.device != x.device):
        raise ValueError("out must have x's shape, dtype and device")
    xs, copied = x, False
    sx = row_level(xs)
    if sx is None:
        xs, copied, in_place = x.contiguous(), True, False
        sx = T
    if in_place:
        ys = xs
    elif out is not None and not copied and row_level(out) is not None:
        ys = out
    else:
        ys = torch.empty(xs.shape, dtype=x.dtype, device=x.device)
    sy = row_level(ys)
    status = torch.empty(lead, dtype=torch.int32, device=x.device)
    ap = None
    if apply is not None:
        ap = apply if isinstance(apply, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(apply))
        if tuple(ap.shape) != lead:
            raise ValueError(f"apply must have the data's leading shape {lead}, got {tuple(ap.shape)}")
        ap = (ap != 0).to(device=x.device, dtype=torch.uint8).contiguous()
    if form == "fma":
        code |= LIPID_FLAGS["fma"]
    for s in _skip:
        code |= LIPID_FLAGS[s]
    _lib.call("xm_lipid_project", xs.data_ptr(), ys.data_ptr(), n_rows, int(sx), int(sy), T, r, tables.data_ptr(),
              ap.data_ptr() if ap is not None else None, status.data_ptr(), code, _stream(x))
    if out is not None and ys is not out:
        out.copy_(ys)
        ys = out
    return LipidResult(out=ys, status=status, copied=copied)


SUB_MAX_RANK = _lib.XM_SUB_MAX_RANK


def _sub_basis(basis, what: str = "basis"):
    torch = _torch()
    _require_device(basis)
    if basis.dtype != torch.complex128 or basis.dim() != 2 or not basis.is_contiguous():
        raise ValueError(f"{what} must be a contiguous complex128 tensor [R, T], got {tuple(basis.shape)} of {basis.dtype}")
    r, t = (int(n) for n in basis.shape)
    if not 1 <= r <= SUB_MAX_RANK or r > t:
        raise ValueError(f"{what}: rank {r} must be in 1 ... {SUB_MAX_RANK} and at most T = {t}")
    return r, t


def sub_project(y, basis, sampling=None):
    """One launch of k_sub_project (xm_sub_project): ``b[c, s, r, f] = sum_t m[s, t] conj(V[r, t])
    y[c, s, f, t]`` in y's dtype, [C, S, R, F].  y: a complex64 / complex128 device tensor [C, S, F, T] whose time
    stride is 1 (any coil, sample and frame strides: it is addressed where it lies; another time stride costs one
    contiguous copy); basis: V [R, T] complex128; sampling: None (all ones) or a contiguous uint8 / bool tensor [S, T] --
    what y holds where it is 0 reaches no output."""
    torch = _torch()
    _require_device(y)
    code = _dtype_code(y)
    if y.dim() != 4:
        raise ValueError(f"y must be [C, S, F, T], got {tuple(y.shape)}")
    c, s, f, t = (int(n) for n in y.shape)
    r, tb = _sub_basis(basis)
    if tb != t:
        raise ValueError(f"sub_project: the data has {t} points along time, the basis {tb}")
    if t > 1 and y.stride(3) != 1:
        y = y.contiguous()
    m = None
    if sampling is not None:
        _require_device(sampling)
        if sampling.dtype not in (torch.uint8, torch.bool) or tuple(sampling.shape) != (s, t) or not sampling.is_contiguous():
            raise ValueError(f"sampling must be a contiguous uint8 / bool tensor of shape {(s, t)}")
        m = sampling
    b = torch.empty((c, s, r, f), dtype=y.dtype, device=y.device)
    if b.numel():
        _lib.call("xm_sub_project", y.data_ptr(), b.data_ptr(), basis.data_ptr(), None if m is None else m.data_ptr(), c, s, f, t,
                  r, int(y.stride(0)), int(y.stride(1)), int(y.stride(2)), code, _stream(y))
    return b


def sub_mix(a, kernel, out=None):
    """One launch of k_sub_mix (xm_sub_mix): ``z[c, s, r, f] = sum_r' K[s, r, r'] a[c, s, r', f]``.  a: contiguous
    complex64 / complex128 [C, S, R, F]; kernel: K [S, R, R] complex128; `out`: None (a fresh tensor), or a tensor like
    a -- ``out is a`` works in place and gives the same bits."""
    torch = _torch()
    _require_device(a)
    code = _dtype_code(a)
    if a.dim() != 4 or not a.is_contiguous():
        raise ValueError(f"a must be a contiguous tensor [C, S, R, F], got {tuple(a.shape)}")
    c, s, r, f = (int(n) for n in a.shape)
    _cgs_c128(kernel, (s, r, r), "kernel")
    z = torch.empty_like(a) if out is None else out
    if z is not a and (tuple(z.shape) != tuple(a.shape) or z.dtype != a.dtype or not z.is_contiguous() or z.device != a.device):
        raise ValueError("out must be contiguous with a's shape, dtype and device")
    if a.numel():
        _lib.call("xm_sub_mix", a.data_ptr(), z.data_ptr(), kernel.data_ptr(), c, s, f, r, code, _stream(a))
    return z


def sub_expand(u, basis):
    """One launch of k_sub_expand (xm_sub_expand): ``x[v, f, t] = sum_r U[v, r, f] V[r, t]``, complex128 [V, F, T].
    u: contiguous complex128 [V, R, F]; basis: V [R, T] complex128."""
    torch = _torch()
    r, t = _sub_basis(basis)
    if u.dim() != 3 or int(u.shape[1]) != r:
        raise ValueError(f"u must be [V, {r}, F], got {tuple(u.shape)}")
    v, _, f = (int(n) for n in u.shape)
    _cgs_c128(u, (v, r, f), "u")
    x = torch.empty((v, f, t), dtype=torch.complex128, device=u.device)
    if x.numel():
        _lib.call("xm_sub_expand", u.data_ptr(), basis.data_ptr(), x.data_ptr(), v, f, t, r, _stream(u))
    return x


class SubspaceSetup:
    """What ``subspace_sense`` needs besides the data, made once per call by ``subspace_setup``: `basis` V [R, T]
    complex128 and `sampling` (uint8 [S, T], or None) on the device, `kernel` K [S, R, R] complex128 there, and the host
    numbers `kappa` (sum_s w_s tr K_s / (R sum_s w_s)) and `fraction` (the mean of the flags)."""

    __slots__ = ("basis", "sampling", "kernel", "kappa", "fraction")

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)


def subspace_setup(basis, sampling, weights, n_samples: int, device) -> SubspaceSetup:
    """K_s[r, r'] = sum_t m[s, t] conj(V[r, t]) V[r', t] as one complex128 matmul on `device` ([S, T] x [T, R^2]) and
    kappa, read back once.  basis: host complex128 [R, T] or a device tensor; sampling: None or a host bool [S, T];
    weights: the S density weights (host)."""
    torch = _torch()
    V = basis if hasattr(basis, "detach") else torch.from_numpy(np.ascontiguousarray(basis, dtype=np.complex128))
    V = V.to(device=device, dtype=torch.complex128).contiguous()
    r, t = (int(n) for n in V.shape)
    if not 1 <= r <= SUB_MAX_RANK or r > t:
        raise ValueError(f"basis: rank {r} must be in 1 ... {SUB_MAX_RANK} and at most T = {t}")
    pairs = (V.conj()[:, None, :] * V[None, :, :]).reshape(r * r, t)  # [(r, r'), t]
    if sampling is None:
        m, fraction = None, 1.0
        K = pairs.sum(dim=1).reshape(1, r, r).expand(int(n_samples), r, r).contiguous()
    else:
        m = torch.from_numpy(np.ascontiguousarray(sampling, dtype=np.uint8)).to(device)
        K = (m.to(torch.complex128) @ pairs.transpose(0, 1)).reshape(int(n_samples), r, r).contiguous()
        fraction = float(m.to(torch.float64).mean().item())
    w = torch.from_numpy(np.ascontiguousarray(weights, dtype=np.float64)).to(device)
    trace = torch.diagonal(K, dim1=1, dim2=2).real.sum(dim=1)
    kappa = float(((w * trace).sum() / (r * w.sum())).item())
    return SubspaceSetup(basis=V, sampling=m, kernel=K, kappa=kappa, fraction=fraction)


class SubspaceSense:
    """Raw outputs of ``subspace_sense``: x [V, F, T] complex128, coefficients [V, R, F] complex128, and per frame
    residual, iterations, status as ``CgSense``."""

    __slots__ = ("x", "coefficients", "residual", "iterations", "status")

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)


def subspace_sense(y, s, adjoint, forward, setup: SubspaceSetup, lam: float, iterations: int, tol: float) -> SubspaceSense:
    """Temporal-subspace SENSE of the frames of y [C, S, F, T]: k_sub_project, then ``cg_sense``
    unchanged on the folded system -- the state is [V R, F], the maps are repeated R times along the voxel axis, the two
    chains run on R F columns and `forward` ends with k_sub_mix in place -- then k_sub_expand.  s, adjoint, forward as in
    ``cg_sense``; `lam` is the final Tikhonov weight (kappa included).  Nothing is read back."""
    c, n_s, f, _ = (int(n) for n in y.shape)
    v = int(s.shape[1])
    V, K = setup.basis, setup.kernel
    r = int(V.shape[0])
    b = sub_project(y, V, setup.sampling)  # [C, S, R, F]
    s_rep = s.repeat_interleave(r, dim=1) if hasattr(s, "repeat_interleave") else np.repeat(s, r, axis=1)  # [C, V R]

    def adj(a):  # [C, S R, F] -> [C, V R, F]
        n = int(a.shape[2])
        return adjoint(a.reshape(c, n_s, r * n)).reshape(c, v * r, n)

    def fwd(u):  # [C, V R, F] -> [C, S R, F], mixed
        n = int(u.shape[2])
        z = forward(u.reshape(c, v, r * n)).reshape(c, n_s, r, n)
        z = z.contiguous() if hasattr(z, "contiguous") else np.ascontiguousarray(z)
        return sub_mix(z, K, out=z).reshape(c, n_s * r, n)

    res = cg_sense(b.reshape(c, n_s * r, f), s_rep, adj, fwd, lam, iterations, tol)
    coef = res.x.reshape(v, r, f)
    return SubspaceSense(x=sub_expand(coef, V), coefficients=coef, residual=res.residual, iterations=res.iterations,
                         status=res.status)


def absmax_argmax(x):
    """phasing.py:229 ``int(np.argmax(np.abs(values)))``: (max |x|, first flat C-order index).

    The flat arg-max does not depend on which axis is the FID axis, so the array is viewed as
    [prod(shape[:-1]), shape[-1]] rows in its own layout.
    """
    _require_device(x)
    torch = _torch()
    xc = x if x.is_contiguous() else x.contiguous()
    n = xc.shape[-1] if xc.dim() else 1
    x2 = xc.reshape(-1, n)
    nb = x2.shape[0]
    rd = _real_dtype(x)
    amax = torch.empty(nb, dtype=rd, device=x.device)
    aidx = torch.empty(nb, dtype=torch.int32, device=x.device)
    gmax = torch.empty(1, dtype=rd, device=x.device)
    gflat = torch.empty(1, dtype=torch.int64, device=x.device)
    code, st = _dtype_code(x), _stream(x)
    _lib.call("xm_absmax_rows", x2.data_ptr(), nb, n, amax.data_ptr(), aidx.data_ptr(), code, st)
    _lib.call("xm_argmax_reduce", amax.data_ptr(), aidx.data_ptr(), nb, n, gmax.data_ptr(), gflat.data_ptr(),
              code, st)
    return float(gmax.item()) ** 0.5, int(gflat.item())


class FusedResult:
    """Outputs of one fused launch: `out` ([n_batch, n_out] or None) and the arg-max pairs."""

    __slots__ = ("out", "absmax2", "argidx")

    def __init__(self, out, absmax2, argidx):
        self.out, self.absmax2, self.argidx = out, absmax2, argidx


def ramp_native(x2, n_out: int, pad_left: int = 0, shift_out: bool = True, ortho: bool = True) -> bool:
    """True when the fused kernel of this geometry applies a linear phase natively (`phase_ramp=` of
    `pipeline_fused` then costs no table and no per-output load); otherwise callers upload a phase table."""
    _require_device(x2)
    flags = (_lib.XM_FFT_ORTHO if ortho else 0) | (_lib.XM_FFT_SHIFT_OUT if shift_out else 0)
    return bool(_lib.load().xm_pipeline_ramp_native(x2.data_ptr(), x2.shape[1], x2.shape[1], int(n_out), int(pad_left),
                                                    flags, _dtype_code(x2)))


def key_native(x2, n_out: int, pad_left: int = 0, shift_out: bool = True, ortho: bool = True) -> bool:
    """True when `pipeline_fused(global_key=, key_result=)` is available for this geometry and dtype (complex64: the
    geometries of `ramp_native` -- without a >= 2x zero fill only in the `phase_ramp=` form; complex128: half lengths
    4096 and 8192)."""
    _require_device(x2)
    flags = (_lib.XM_FFT_ORTHO if ortho else 0) | (_lib.XM_FFT_SHIFT_OUT if shift_out else 0)
    # (the kernels without a >= 2x zero fill pack two rows per lane pair: a single row takes another kernel)
    return x2.shape[0] >= 2 and bool(_lib.load().xm_pipeline_key_native(x2.data_ptr(), x2.shape[1], x2.shape[1], int(n_out),
                                                                       int(pad_left), flags, _dtype_code(x2)))


def pipeline_fused(x2, n_out: int, pad_left: int = 0, window=None, phase_table=None, shift_out: bool = True,
                   ortho: bool = True, want_out: bool = True, want_argmax: bool = False, out=None,
                   absmax2=None, argidx=None, argmax_value_only: bool = False, phase_ramp=None, global_key=None,
                   key_result=None):
    """One launch of zero-fill + window + FFT(+fftshift) [+ |X|^2 arg-max] [+ phase] on
    ``x2`` = [n_batch, n_in] contiguous rows (FID axis last).  `window` / `phase_table` are
    device tensors of the storage precision (real n_out / complex n_out) or None.
    `phase_ramp` = (phase0, dphase) in radians multiplies output k by e^{i (phase0 + dphase k)} instead of a
    table (phasing.py:62-73 on a uniform axis).  `global_key` (`new_argmax_key`, geometries
    with `ramp_native` only) receives the launch's global arg-max (value bits, row) instead of per-row outputs;
    `argmax_key_take` decodes and clears it -- or, with `key_result` (`new_key_result`: 16 bytes of pinned host
    memory), the kernel's last workgroup does that itself and no further launch is needed."""
    _require_device(x2)
    torch = _torch()
    if x2.dim() != 2 or not x2.is_contiguous():
        raise ValueError("pipeline_fused expects a contiguous [n_batch, n_in] tensor")
    nb, n_in = x2.shape
    rd = _real_dtype(x2)
    if want_out and out is None:
        out = torch.empty((nb, n_out), dtype=x2.dtype, device=x2.device)
    if global_key is not None:
        want_argmax, absmax2 = True, global_key  # the key rides in the absmax2 slot, the result record in argidx's
        argidx = key_result
    if want_argmax:
        if absmax2 is None:
            absmax2 = torch.empty(nb, dtype=rd, device=x2.device)
        if argidx is None and global_key is None:
            argidx = torch.empty(nb, dtype=torch.int32, device=x2.device)
    flags = (_lib.XM_FFT_ORTHO if ortho else 0) | (_lib.XM_FFT_SHIFT_OUT if shift_out else 0)
    if global_key is not None:
        flags |= _lib.XM_AMAX_GLOBAL_KEY | _lib.XM_AMAX_VALUE_ONLY
    if argmax_value_only:  # hint: kernels may skip the first-index scan (argidx then holds 0)
        flags |= _lib.XM_AMAX_VALUE_ONLY
    if phase_ramp is not None:
        if phase_table is not None or not want_out:
            raise ValueError("phase_ramp excludes phase_table and needs an output")
        _lib.call(
            "xm_pipeline_fused_ramp", x2.data_ptr(), n_in, out.data_ptr(),
            window.data_ptr() if window is not None else None, float(phase_ramp[0]), float(phase_ramp[1]), nb, n_in,
            n_out, pad_left, flags, absmax2.data_ptr() if want_argmax else None,
            argidx.data_ptr() if (want_argmax and argidx is not None) else None, _dtype_code(x2), _stream(x2))
        return FusedResult(out, absmax2 if want_argmax else None, argidx if want_argmax else None)
    _lib.call(
        "xm_pipeline_fused", x2.data_ptr(), n_in, out.data_ptr() if want_out else None,
        window.data_ptr() if window is not None else None,
        phase_table.data_ptr() if phase_table is not None else None, nb, n_in, n_out, pad_left, flags,
        absmax2.data_ptr() if want_argmax else None,
        argidx.data_ptr() if (want_argmax and argidx is not None) else None, _dtype_code(x2), _stream(x2))
    return FusedResult(out if want_out else None, absmax2 if want_argmax else None,
                       argidx if want_argmax else None)


def row_l1(x2, window=None, pad_left: int = 0, out=None, n_used: int | None = None, sub_step: int = 1, key=None):
    """Windowed L1 norm of every row of ``x2`` = [n_batch, n_in] (`xm_row_l1`): the cheap streaming guess for
    the row that holds the global maximum of the spectra.  `n_used` < n_in sums only the leading samples of
    every row (a caller that knows the window's tail carries no weight skips reading it); `sub_step` > 1 sums
    every sub_step-th 128-sample block of those (a ranking statistic on 1/sub_step of the bytes).  `key` (complex64:
    `new_argmax_key`) receives the row with the largest norm in the same launch
    (`argmax_key_take` decodes and clears it); the per-row norms are then not written unless `out` is given."""
    _require_device(x2)
    torch = _torch()
    if x2.dim() != 2 or not x2.is_contiguous():
        raise ValueError("row_l1 expects a contiguous [n_batch, n_in] tensor")
    nb, n_in = x2.shape
    if out is None and key is None:
        out = torch.empty(nb, dtype=_real_dtype(x2), device=x2.device)
    n_sum = n_in if n_used is None else max(1, min(int(n_used), n_in))
    _lib.call("xm_row_l1", x2.data_ptr(), n_in, window.data_ptr() if window is not None else None, nb, n_sum,
              int(pad_left), max(1, int(sub_step)), out.data_ptr() if out is not None else None,
              key.data_ptr() if key is not None else None, _dtype_code(x2), _stream(x2))
    return out


def guess_supported(x2, n_out: int, pad_left: int = 0, shift_out: bool = True, ortho: bool = True) -> bool:
    """True when the coarse-spectra guess stage (`guess_rows` + `guess_refine`) takes this geometry ("end" zero fill to
    >= 2x with an in-LDS half-length plan; complex64 rows 16-byte aligned)."""
    _require_device(x2)
    if x2.dim() != 2 or not x2.is_contiguous():
        return False
    flags = (_lib.XM_FFT_ORTHO if ortho else 0) | (_lib.XM_FFT_SHIFT_OUT if shift_out else 0)
    return bool(_lib.load().xm_guess_supported(x2.data_ptr(), x2.shape[1], x2.shape[1], int(n_out), int(pad_left), flags,
                                               _dtype_code(x2)))


def guess_rows(x2, n_out: int, window32, est, key, n_guess: int = 0, shift_out: bool = True, ortho: bool = True):
    """`xm_guess_rows`: est[b] = max |X_c|^2 of the coarse spectrum of row b (its first <= 512 windowed samples on a
    1024-bin grid), the largest estimate merged into `key`.  `window32`: float32 weights over the zero-filled axis
    (for complex128 rows too); `est`: float32 [n_batch]."""
    _require_device(x2)
    flags = (_lib.XM_FFT_ORTHO if ortho else 0) | (_lib.XM_FFT_SHIFT_OUT if shift_out else 0)
    nb, n_in = x2.shape
    _lib.call("xm_guess_rows", x2.data_ptr(), n_in, window32.data_ptr() if window32 is not None else None, nb, n_in,
              int(n_out), int(n_guess), flags, est.data_ptr(), key.data_ptr(), _dtype_code(x2), _stream(x2))
    return est


def guess_refine(x2, n_out: int, window32, est, guess_key, work_key, gmax, gflat, out_row, band: float = 0.75,
                 shift_out: bool = True, ortho: bool = True):
    """`xm_guess_refine`: every row whose estimate is within `band` of the largest one is transformed exactly; the
    winner's max |X|^2 -> `gmax` (float32), row * n_out -> `gflat` (int64), its FID as complex128 -> `out_row`
    ([1, n_in]); both keys are left zero."""
    _require_device(x2)
    flags = (_lib.XM_FFT_ORTHO if ortho else 0) | (_lib.XM_FFT_SHIFT_OUT if shift_out else 0)
    nb, n_in = x2.shape
    _lib.call("xm_guess_refine", x2.data_ptr(), n_in, window32.data_ptr() if window32 is not None else None, nb, n_in,
              int(n_out), flags, est.data_ptr(), guess_key.data_ptr(), float(band), work_key.data_ptr(),
              gmax.data_ptr(), gflat.data_ptr(), out_row.data_ptr(), _dtype_code(x2), _stream(x2))
    return out_row


def new_argmax_key(device):
    """A zeroed arg-max key buffer (XM_KEY_BYTES) for `row_l1(key=)` / `pipeline_fused(global_key=)`."""
    return _torch().zeros(131072 // 8, dtype=_torch().int64, device=device)


def new_key_result():
    """Pinned host record (xm_argmax_result: float32 max |X|^2, pad, int64 flat index) a kernel can fill directly."""
    return _torch().zeros(2, dtype=_torch().int64, pin_memory=True)


def read_key_result(rec, complex128: bool = False):
    """(max |X|^2, flat index) of a `new_key_result` record (after the producing launch has completed); a complex128
    launch leaves the maximum as a double."""
    m2 = rec.view(_torch().float64)[0] if complex128 else rec.view(_torch().float32)[0]
    return float(m2.item()), int(rec[1].item())


def argmax_key_take(key, n_per_row: int, gmax, gflat, x2=None, out_row=None):
    """Decode a global arg-max key (`row_l1(key=)` / `pipeline_fused(global_key=)`) into `gmax` (float32, the value)
    and `gflat` (int64, row * n_per_row) -- device-accessible one-element tensors -- and clear it; with `x2` also
    gather the winning row as complex128 into `out_row` ([1, n_in])."""
    torch = _torch()
    if x2 is not None:
        _require_device(x2)
        if out_row is None:
            out_row = torch.empty((1, x2.shape[1]), dtype=torch.complex128, device=x2.device)
    st = torch.cuda.current_stream(key.device).cuda_stream
    _lib.call("xm_argmax_key_take", key.data_ptr(), int(n_per_row), gmax.data_ptr(), gflat.data_ptr(),
              x2.data_ptr() if x2 is not None else None, x2.shape[1] if x2 is not None else 0,
              x2.shape[1] if x2 is not None else 0, out_row.data_ptr() if x2 is not None else None,
              _dtype_code(x2) if x2 is not None else _lib.XM_C64, st)
    return out_row


def argmax_reduce(absmax2, argidx, n: int):
    """Global (max |X|, flat index) from the per-spectrum pairs of a fused launch."""
    torch = _torch()
    nb = absmax2.numel()
    gmax = torch.empty(1, dtype=absmax2.dtype, device=absmax2.device)
    gflat = torch.empty(1, dtype=torch.int64, device=absmax2.device)
    code = _lib.XM_C64 if absmax2.dtype == torch.float32 else _lib.XM_C128
    _lib.call("xm_argmax_reduce", absmax2.data_ptr(), argidx.data_ptr(), nb, n, gmax.data_ptr(),
              gflat.data_ptr(), code, torch.cuda.current_stream(absmax2.device).cuda_stream)
    return float(gmax.item()) ** 0.5, int(gflat.item())


def argmax_reduce_async(absmax2, argidx, n: int, gmax=None, gflat=None):
    """Same reduction, results left on the device (no host synchronisation)."""
    torch = _torch()
    nb = absmax2.numel()
    if gmax is None:
        gmax = torch.empty(1, dtype=absmax2.dtype, device=absmax2.device)
    if gflat is None:
        gflat = torch.empty(1, dtype=torch.int64, device=absmax2.device)
    code = _lib.XM_C64 if absmax2.dtype == torch.float32 else _lib.XM_C128
    _lib.call("xm_argmax_reduce", absmax2.data_ptr(), argidx.data_ptr(), nb, n, gmax.data_ptr(),
              gflat.data_ptr(), code, torch.cuda.current_stream(absmax2.device).cuda_stream)
    return gmax, gflat


def gather_row_c128(x2, gflat, n_per_row: int, out=None):
    """phasing.py:241-242: the spectrum's source row, selected by a flat index that lives on the DEVICE,
    upcast to complex128 ([1, n_in])."""
    _require_device(x2)
    torch = _torch()
    nb, n_in = x2.shape
    if out is None:
        out = torch.empty((1, n_in), dtype=torch.complex128, device=x2.device)
    _lib.call("xm_gather_row_c128", x2.data_ptr(), n_in, n_in, gflat.data_ptr(), int(n_per_row), out.data_ptr(),
              _dtype_code(x2), _stream(x2))
    return out


def last_kernel() -> str:
    """`xm_last_kernel_string`: the kernel the fused dispatcher launched last on this thread, as the profiler names it."""
    v = _lib.load().xm_last_kernel_string()
    return v.decode("utf-8", "replace") if v else ""


def fft_supported(n: int, complex128: bool = False) -> bool:
    if n == 1:
        return True
    return bool(_lib.load().xm_fft_supported(int(n), _lib.XM_C128 if complex128 else _lib.XM_C64))


# ---------------------------------------------------------------------------------------------
# A7 on the device: the (p0, p1) search as one workgroup beside the streaming kernels (csrc/xm_search.hip)
# ---------------------------------------------------------------------------------------------
SEARCH_RECORD_WORDS = 16  # xm_search_result: 128 bytes


def search_supported(n: int, method: str = "acme", x_range: float = 1.0) -> bool:
    """True when `search_launch` takes this slice length / objective (ACME, n <= 16576, a non-degenerate axis)."""
    from .autophase_solver import METHODS

    return method in METHODS and bool(_lib.load().xm_search_supported(int(n), METHODS.index(method), float(x_range)))


def new_search_record():
    """Pinned host record (`xm_search_result`) that a search kernel fills when it ends, `seq` (word 7) last."""
    return _torch().zeros(SEARCH_RECORD_WORDS, dtype=_torch().int64, pin_memory=True)


def uniform_axis(coords):
    """(c0, cstep, x_range) of a coordinate axis when it is uniform to a few ulp (the fftfreq axis of this path), else
    None: phasing.py:56-69's (c - pivot) / (max c - min c) is then linear in the bin index."""
    c = np.asarray(coords, dtype=np.float64)
    if c.size < 2:
        return None
    step = (c[-1] - c[0]) / (c.size - 1)
    rng = float(c.max() - c.min())
    if step == 0 or rng <= 0 or not np.all(np.abs(c - (c[0] + step * np.arange(c.size))) <= 4e-15 * rng):
        return None
    return float(c[0]), float(step), rng


def search_launch(slice_c128, axis, record, seq: int, p0_only: bool = False, seed: int = 42, tol: float = 0.01,
                  maxiter: int = 1000, stream=None):
    """`xm_search_launch`: phasing.py:276-284's differential evolution for the ACME objective on `slice_c128` (n
    complex128 bins, device-accessible: device memory or pinned host memory), asynchronous on `stream` (a
    torch.cuda.Stream; default: the current one).  `axis` = `uniform_axis(coords)`.  `record` (`new_search_record`)
    receives the result; `search_done(record, seq)` tells when."""
    torch = _torch()
    n = slice_c128.numel()
    st = (stream if stream is not None else torch.cuda.current_stream()).cuda_stream
    _lib.call("xm_search_launch", slice_c128.data_ptr(), int(n), float(axis[0]), float(axis[1]), float(axis[2]), 0,
              int(bool(p0_only)), int(seed), float(tol), int(maxiter), int(seq), record.data_ptr(), st)


def search_done(record, seq: int) -> bool:
    return int(_lib.load().xm_atomic_load_acquire_i64(record.data_ptr() + 56)) == int(seq)


def read_search_record(record) -> dict:
    """The fields of a finished `xm_search_result`."""
    f = record.view(_torch().float64)
    i = record.view(_torch().int32)
    return dict(x=(float(f[0]), float(f[1])), fun=float(f[2]), pg_norm=float(f[3]), nfev=int(i[8]), nit=int(i[9]),
                status=int(i[10]), needs_polish=bool(int(i[11])), target_idx=int(i[12]),
                t_us=[float(v) for v in f[8:14]])


def search_eval(slice_c128, axis, xs, target_idx: int = -1, p0_only: bool = False):
    """`xm_search_eval`: the device objective at the rows of `xs` ([count, 2] degrees); synchronous (tests)."""
    torch = _torch()
    xs_t = torch.as_tensor(np.ascontiguousarray(xs, dtype=np.float64)).reshape(-1, 2).to(slice_c128.device if slice_c128.is_cuda else "cuda")
    fs = torch.empty(xs_t.shape[0], dtype=torch.float64, device=xs_t.device)
    _lib.call("xm_search_eval", slice_c128.data_ptr(), int(slice_c128.numel()), float(axis[0]), float(axis[1]),
              float(axis[2]), int(target_idx), int(bool(p0_only)), xs_t.data_ptr(), int(xs_t.shape[0]), fs.data_ptr(),
              torch.cuda.current_stream().cuda_stream)
    return fs.cpu().numpy()


# ---------------------------------------------------------------------------------------------
# autophase_each: the same search for every row, and one phase ramp per row
# ---------------------------------------------------------------------------------------------
SEARCH_ALL_ZERO, SEARCH_NOT_FINITE = 2, 3  # XM_SEARCH_*: rows without a search
SEARCH_ROW_DTYPE = np.dtype([("x", "<f8", (2,)), ("fun", "<f8"), ("pg_norm", "<f8"), ("nfev", "<i4"), ("nit", "<i4"),
                             ("target_idx", "<i4"), ("status", "<i4"), ("needs_polish", "<i4"), ("pad_", "<i4")])


def search_rows_supported(n: int, method: str = "acme", x_range: float = 1.0, complex128: bool = False) -> bool:
    """True when `search_rows` takes rows of this length / objective (ACME, 2 <= n <= 16576, a non-degenerate axis)."""
    from .autophase_solver import METHODS

    return method in METHODS and bool(_lib.load().xm_search_rows_supported(
        int(n), METHODS.index(method), float(x_range), _lib.XM_C128 if complex128 else _lib.XM_C64))


def search_rows(x2d, axis, p0_only: bool = False, seed: int = 42, tol: float = 0.01, maxiter: int = 1000, pivot=None,
                target_idx: int = -1):
    """`xm_search_rows`: phasing.py:276-284's differential evolution (ACME) for EVERY row of ``x2d`` = [n_rows, n]
    contiguous complex64 / complex128 rows, one workgroup per row.  `axis` = `uniform_axis(coords)`.  `pivot` None:
    every row's pivot is the coordinate of its first arg-max of |X|; otherwise that pivot for all rows, with
    `target_idx` the bin nearest to it.  Returns the records as a structured array (`SEARCH_ROW_DTYPE`) on the host."""
    _require_device(x2d)
    torch = _torch()
    if x2d.dim() != 2 or not x2d.is_contiguous():
        raise ValueError("search_rows expects a contiguous [n_rows, n] tensor")
    nb, n = x2d.shape
    rec = torch.empty((nb, SEARCH_ROW_DTYPE.itemsize), dtype=torch.uint8, device=x2d.device)
    _lib.call("xm_search_rows", x2d.data_ptr(), nb, n, _dtype_code(x2d), float(axis[0]), float(axis[1]), float(axis[2]),
              int(bool(p0_only)), int(seed), float(tol), int(maxiter), float("nan") if pivot is None else float(pivot),
              -1 if pivot is None else int(target_idx), rec.data_ptr(), _stream(x2d))
    return rec.cpu().numpy().view(SEARCH_ROW_DTYPE).reshape(nb)


def phase_apply_rows(x, axis: int, coords, p0, p1, pivot, skip=None, out=None):
    """phasing.py:56-73 with one (p0, p1, pivot) per spectrum (`xm_phase_apply_rows`): `p0` / `p1` (degrees) / `pivot`
    are shaped like `x` without `axis`; rows where `skip` is set are copied through unchanged.  `out`: `x` itself
    for an update in place (the axis must then be the last one of a contiguous tensor)."""
    _require_device(x)
    torch = _torch()
    x2, restore = _rows(x, axis)
    nb, n = x2.shape
    lead = tuple(x.shape[:axis % x.dim()]) + tuple(x.shape[axis % x.dim() + 1:])
    c = np.array(coords, dtype=np.float64)
    if c.size != n:
        raise ValueError(f"coordinate axis has {c.size} points, data axis has {n}")

    def per_row(v, dtype):
        v = np.array(np.broadcast_to(np.asarray(v, dtype=dtype), lead))  # (a copy: torch wants writable memory)
        return torch.from_numpy(v.reshape(nb)).to(x.device)

    cd = torch.from_numpy(c).to(x.device)
    p0d, p1d, pvd = (per_row(v, np.float64) for v in (p0, p1, pivot))
    skd = per_row(np.asarray(skip) != 0, np.int32) if skip is not None else None
    if out is not None:
        if out is not x or x2.data_ptr() != x.data_ptr():
            raise ValueError("phase_apply_rows: `out` must be `x` itself, contiguous with `axis` last")
        y2 = x2
    else:
        y2 = torch.empty_like(x2)
    _lib.call("xm_phase_apply_rows", x2.data_ptr(), y2.data_ptr(), cd.data_ptr(), nb, n, p0d.data_ptr(), p1d.data_ptr(),
              pvd.data_ptr(), skd.data_ptr() if skd is not None else None, _dtype_code(x), _stream(x))
    return x if out is not None else restore(y2)


class ChipPartition:
    """`xm_stream_create`: one compute stream that owns all CUs but `reserved`, and `n_search` streams that own the
    reserved ones (spread over the eight XCDs), as torch stream objects.  Kept for the life of the process."""

    def __init__(self, device, reserved: int, n_search: int):
        import ctypes

        torch = _torch()
        self.device, self.reserved = device, int(reserved)
        self._handles = []

        def make(partition):
            h = ctypes.c_void_p()
            with torch.cuda.device(device):
                _lib.call("xm_stream_create", ctypes.byref(h), int(reserved), partition)
            self._handles.append(h.value)
            return torch.cuda.ExternalStream(h.value, device=device)

        self.compute = make(0)
        self.search = [make(1) for _ in range(int(n_search))]

    def another_search_stream(self):
        import ctypes

        h = ctypes.c_void_p()
        with _torch().cuda.device(self.device):
            _lib.call("xm_stream_create", ctypes.byref(h), self.reserved, 1)
        self._handles.append(h.value)
        st = _torch().cuda.ExternalStream(h.value, device=self.device)
        self.search.append(st)
        return st


_PARTITIONS = {}


def chip_partition(device, reserved: int, n_search: int) -> ChipPartition:
    torch = _torch()
    device = torch.device(device)
    key = (device.index if device.index is not None else torch.cuda.current_device(), int(reserved))
    part = _PARTITIONS.get(key)
    if part is None:
        part = _PARTITIONS[key] = ChipPartition(device, reserved, n_search)
    while len(part.search) < n_search:
        part.another_search_stream()
    return part


def replacement_search_stream(device, partition_streams):
    """A fresh stream for searches (one whose kernel is still running was retired): of the search partition when the
    chip is split, an ordinary one otherwise."""
    torch = _torch()
    if partition_streams is None:
        return torch.cuda.Stream(device=device)
    for part in _PARTITIONS.values():
        if partition_streams and partition_streams[0] in part.search:
            return part.another_search_stream()
    return torch.cuda.Stream(device=device)
