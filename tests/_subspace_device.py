"""TEST DOUBLE (not product code): the numpy stand-in of tests/_numpy_device.py plus numpy versions of what
``recon_subspace`` reaches below the Python layer -- ``axis_sparse``, ``axis_dft`` and ``cg_sense`` as tests/test_cgsense.py
states them, and the three new entries ``sub_project``, ``sub_mix``, ``sub_expand`` from tests/_subspace_oracle.py.  The
driver ``device.subspace_sense`` and the set-up ``device.subspace_setup`` (torch on the CPU here) run as they are."""
import numpy as np

import _mrsi_oracle as mrsi_orc
import _numpy_device
import _subspace_oracle as orc


def _np(a):
    return a.numpy() if hasattr(a, "numpy") else np.asarray(a)


def sub_project(y, basis, sampling=None):
    m = None if sampling is None else _np(sampling) != 0
    return orc.project(np.asarray(y, dtype=np.complex128), _np(basis), m).astype(y.dtype)


def sub_mix(a, kernel, out=None):
    z = orc.mix(np.asarray(a, dtype=np.complex128), _np(kernel)).astype(a.dtype)
    if out is None:
        return z
    out[...] = z
    return out


def sub_expand(u, basis):
    return orc.expand(np.asarray(u, dtype=np.complex128), _np(basis))


def install(monkeypatch):
    """Installs everything and returns the list the stand-ins append their names to, one per call."""
    from test_cgsense import np_axis_sparse, np_cg_sense
    from xmris_amd import device as dev

    _numpy_device.install(monkeypatch)
    calls = []

    def noting(name, fn):
        def wrapped(*a, **k):
            calls.append(name)
            return fn(*a, **k)
        return wrapped

    monkeypatch.setattr(dev, "axis_sparse", noting("axis_sparse", np_axis_sparse))
    monkeypatch.setattr(dev, "axis_dft", noting("axis_dft", lambda x, axis, table: mrsi_orc.apply_table(x, axis, np.asarray(table)).astype(x.dtype)))
    monkeypatch.setattr(dev, "cg_sense", noting("cg_sense", np_cg_sense))
    for name, fn in (("sub_project", sub_project), ("sub_mix", sub_mix), ("sub_expand", sub_expand)):
        monkeypatch.setattr(dev, name, noting(name, fn))
    return calls
