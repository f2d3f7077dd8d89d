"""A small stand-in for ``xarray.Dataset``: named ``LabeledArray`` variables that share coordinates and attrs."""
from __future__ import annotations

import copy as _copy

from ..labeled import LabeledArray


class LabeledDataset:
    """``data_vars``: name -> LabeledArray; ``coords``: the union of the variables' coordinates; ``attrs``.  Variables
    are reached as ``ds["amplitude"]`` or ``ds.amplitude``."""

    def __init__(self, data_vars=None, attrs=None):
        self.data_vars = dict(data_vars or {})
        self.attrs = dict(attrs or {})

    @property
    def coords(self):
        out = {}
        for v in self.data_vars.values():
            for k, c in v.coords.items():
                out.setdefault(k, c)
        return out

    @property
    def dims(self):
        out = {}
        for v in self.data_vars.values():
            out.update(v.sizes)
        return out

    def __getitem__(self, name) -> LabeledArray:
        return self.data_vars[name]

    def __getattr__(self, name):
        dv = self.__dict__.get("data_vars")
        if dv is not None and name in dv:
            return dv[name]
        raise AttributeError(name)

    def __contains__(self, name):
        return name in self.data_vars

    def __iter__(self):
        return iter(self.data_vars)

    def copy(self):
        return LabeledDataset({k: v.copy() for k, v in self.data_vars.items()}, _copy.copy(self.attrs))

    def to_xarray(self):
        """An ``xarray.Dataset`` of the variables' ``to_xarray()`` (a thin conversion; xarray is optional here)."""
        import xarray as xr

        return xr.Dataset({k: v.to_xarray() for k, v in self.data_vars.items()}, attrs=dict(self.attrs))

    def __repr__(self):
        return f"<xmris_amd.LabeledDataset dims={self.dims} data_vars={list(self.data_vars)} attrs={list(self.attrs)}>"
