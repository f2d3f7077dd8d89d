"""``simulate_fid``: the AMARES model as a labelled FID (reference ``src/xmris/fitting/simulation.py:99-232``).

The ideal signal comes from the GPU model kernel (``xm_amares_model``, the same arithmetic as the fit's); noise, when
asked for, is drawn on the host from an unseeded generator as in the reference: total standard deviation
mean(|fid[:10]|) / target_snr, spread over the two channels by 1/sqrt(2).
"""
from __future__ import annotations

import numpy as np

from .. import device as dev
from ..config import ATTRS, COORDS, DIMS
from ..labeled import Coordinate, LabeledArray


def _peak_parameters(amplitudes, frequencies, chemical_shifts, reference_frequency, carrier_ppm, dampings, phases,
                     lineshape_g):
    amplitudes = np.atleast_1d(np.asarray(amplitudes, dtype=np.float64))
    k = len(amplitudes)
    if frequencies is not None and chemical_shifts is not None:
        raise ValueError("Provide either 'frequencies' or 'chemical_shifts', not both.")
    if chemical_shifts is not None:
        if reference_frequency is None:
            raise ValueError("reference_frequency (MHz) must be provided when using chemical shifts.")
        freqs = (np.atleast_1d(np.asarray(chemical_shifts, dtype=np.float64)) - carrier_ppm) * reference_frequency
    elif frequencies is not None:
        freqs = np.atleast_1d(np.asarray(frequencies, dtype=np.float64))
    else:
        raise ValueError("Either 'frequencies' or 'chemical_shifts' must be provided.")
    if len(freqs) != k:
        raise ValueError("Length of frequencies/chemical_shifts must match amplitudes.")
    d = np.broadcast_to(np.asarray(dampings, dtype=np.float64), k)
    ph = np.broadcast_to(np.asarray(phases, dtype=np.float64), k)
    g = np.clip(np.broadcast_to(np.asarray(lineshape_g, dtype=np.float64), k), 0.0, 1.0)
    return np.stack([amplitudes, freqs, d, ph, g], axis=1)


def simulate_fid(amplitudes, *, frequencies=None, chemical_shifts=None, reference_frequency=None,
                 carrier_ppm: float = 0.0, spectral_width: float = 10000.0, n_points: int = 1024,
                 dampings=50.0, phases=0.0, lineshape_g=0.0, dead_time: float = 0.0, target_snr=None) -> LabeledArray:
    """A 1-D complex128 FID on `time` (Vanhamme 1997 eq. 6): peaks of `amplitudes`, at `frequencies` [Hz] or
    `chemical_shifts` [ppm] (relative to `carrier_ppm`, times `reference_frequency` MHz), `dampings` [1/s], `phases`
    [rad], `lineshape_g` in [0, 1]; t_j = j / spectral_width + dead_time.  Parameter names, defaults, errors, attrs and
    the name "FID Signal" as in the reference."""
    import torch

    params = _peak_parameters(amplitudes, frequencies, chemical_shifts, reference_frequency, carrier_ppm, dampings,
                              phases, lineshape_g)
    n_points = int(n_points)
    dwell = 1.0 / spectral_width
    pd = torch.from_numpy(params).to("cuda")
    fid = dev.amares_model(pd, n_points, dwell, float(dead_time)).cpu().numpy()
    if target_snr is not None:
        signal = np.mean(np.abs(fid[: min(10, n_points)]))
        std = signal / target_snr / np.sqrt(2.0)
        rng = np.random.default_rng()
        fid = fid + (rng.normal(0, std, fid.shape) + 1j * rng.normal(0, std, fid.shape))
    time = np.arange(n_points) * dwell + dead_time

    attrs = {
        "spectral_width": spectral_width,
        "dead_time": dead_time,
        "sim_amplitudes": np.atleast_1d(amplitudes).tolist(),
        "sim_dampings": np.atleast_1d(dampings).tolist(),
        ATTRS.carrier_ppm: carrier_ppm,
        "units": "a.u.",
    }
    if target_snr is not None:
        attrs["target_snr"] = target_snr
    if reference_frequency is not None:
        attrs[ATTRS.reference_frequency] = reference_frequency
    if frequencies is not None:
        attrs["sim_frequencies_hz"] = np.atleast_1d(frequencies).tolist()
    if chemical_shifts is not None:
        attrs["sim_chemical_shifts_ppm"] = np.atleast_1d(chemical_shifts).tolist()
    coords = {COORDS.time: Coordinate(DIMS.time, time, {"units": "s", "long_name": "Time"})}
    return LabeledArray(fid, (DIMS.time,), coords, attrs, name="FID Signal")
