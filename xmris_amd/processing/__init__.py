"""GPU implementations of the reference's ``xmris.processing`` functions on the spectral hot path."""
from .align import align_averages
from .baseline import baseline_als
from .coils import combine_coils
from .denoise import denoise_mppca
from .espirit import espirit_maps
from .fid import apodize_exp, apodize_lg, to_fid, to_spectrum, zero_fill
from .grappa import GrappaWeights, grappa_calibrate, grappa_fill
from .cgsense import recon_cg_sense
from .l1sense import recon_l1_sense
from .lipids import LipidBasis, lipid_basis, remove_lipids
from .subspace import TemporalBasis, recon_subspace, temporal_basis
from .grid import degrid_kspace, density_weights, grid_kspace, grid_table, nufft_adjoint, nufft_forward
from .mrsi import to_image, to_kspace
from .fourier import fft, fftc, fftshift, ifft, ifftc, ifftshift
from .phasing import autophase, autophase_each, phase
from .sense import sense_maps, unfold_sense
from .species import separate_species, simulate_echoes, species_matrix
from .timeshift import correct_readout_time, readout_offsets, shift_time
from .water import remove_water

__all__ = ["align_averages", "baseline_als", "combine_coils", "denoise_mppca", "apodize_exp", "apodize_lg", "to_fid", "to_spectrum", "zero_fill", "fft", "fftc", "fftshift", "ifft",
           "ifftc", "ifftshift", "autophase", "autophase_each", "phase", "remove_water", "to_image", "to_kspace", "sense_maps", "unfold_sense",
           "grid_kspace", "degrid_kspace", "nufft_adjoint", "nufft_forward", "density_weights", "grid_table", "recon_cg_sense", "recon_l1_sense",
           "shift_time", "correct_readout_time", "readout_offsets", "GrappaWeights", "grappa_calibrate", "grappa_fill", "espirit_maps",
           "separate_species", "simulate_echoes", "species_matrix", "LipidBasis", "lipid_basis", "remove_lipids",
           "TemporalBasis", "recon_subspace", "temporal_basis"]

# the lazy chain's end computes itself in one fused launch where it can (labeled.LabeledArray.data)
from .. import labeled as _labeled
from ._common import fused_materialise as _fused_materialise

_labeled._materialise_hook = _fused_materialise
