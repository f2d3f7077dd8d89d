"""xmris_amd -- MI355X (gfx950) backend of the xmris `.xmr` spectral hot path.

zero_fill -> apodize_exp -> to_spectrum (ortho FFT + fftshift) -> autophase, behind the
reference's accessor method names.  Hand-written HIP kernels reached through a C ABI
(`include/xmris_hip.h`, `xmris_amd/libxmris_hip.so`); Python keeps dims / coords / attrs.
"""

__version__ = "0.4.0"

from . import _lib  # noqa: F401
from .accessor import XmrisAccessor, register_xarray_accessor
from .config import ATTRS, COORDS, DIMS
from .fitting import basis_model, fit_amares, fit_basis, fit_kinetics, simulate_fid, simulate_kinetics
from .fused import spectral_pipeline
from .labeled import Coordinate, LabeledArray
from .vendor.bruker import remove_digital_filter
from .processing import (align_averages, baseline_als, combine_coils, degrid_kspace, denoise_mppca, density_weights, grid_kspace, grid_table, nufft_adjoint, nufft_forward, recon_cg_sense, recon_l1_sense, apodize_exp, apodize_lg, autophase, autophase_each, fft, fftc, fftshift, ifft, ifftc, ifftshift, phase,
                         remove_water, sense_maps, to_fid, to_image, to_kspace, to_spectrum, unfold_sense, zero_fill,
                         correct_readout_time, readout_offsets, shift_time, GrappaWeights, grappa_calibrate, grappa_fill, espirit_maps,
                         separate_species, simulate_echoes, species_matrix, LipidBasis, lipid_basis, remove_lipids,
                         TemporalBasis, recon_subspace, temporal_basis)

DataArray = LabeledArray  # convenience alias for code written against xarray's constructor signature
register_xarray_accessor()  # no-op when xarray is absent or the name `xmr` is already owned

__all__ = ["align_averages", "baseline_als", "combine_coils", "denoise_mppca", "ATTRS", "COORDS", "DIMS", "Coordinate", "DataArray", "LabeledArray", "XmrisAccessor",
           "apodize_exp", "apodize_lg", "autophase", "autophase_each", "basis_model", "fft", "fit_amares", "fit_basis", "fftc", "fftshift", "ifft", "ifftc", "ifftshift",
           "phase", "register_xarray_accessor", "remove_digital_filter", "remove_water", "sense_maps", "simulate_fid", "spectral_pipeline", "to_fid", "to_image", "to_kspace", "to_spectrum", "unfold_sense", "zero_fill",
           "grid_kspace", "degrid_kspace", "nufft_adjoint", "nufft_forward", "density_weights", "grid_table", "recon_cg_sense", "recon_l1_sense",
           "shift_time", "correct_readout_time", "readout_offsets", "fit_kinetics", "simulate_kinetics",
           "GrappaWeights", "grappa_calibrate", "grappa_fill", "espirit_maps",
           "separate_species", "simulate_echoes", "species_matrix", "LipidBasis", "lipid_basis", "remove_lipids",
           "TemporalBasis", "recon_subspace", "temporal_basis"]
