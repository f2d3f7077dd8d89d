"""Vocabulary of dimension / coordinate / attribute names used on the spectral hot path.

Restates the NAMES and units of the reference's singletons (``src/xmris/core/config.py:9-44``
term class, ``:128-200`` attrs, ``:229-283`` dims/coords, ``:331-334`` singletons) so that the
drop-in emits identical dims, coordinate attrs (``long_name``/``units``) and lineage keys.
Descriptions are this project's own wording.
"""
from __future__ import annotations


class XmrisTerm(str):
    """A ``str`` that also carries ``description``, ``unit`` and a display ``long_name``."""

    def __new__(cls, value: str, description: str = "", unit: str = ""):
        obj = str.__new__(cls, value)
        obj.description = description
        obj.unit = unit
        return obj

    @property
    def long_name(self) -> str:
        return self.replace("_", " ").title()


class _Vocabulary:
    def _terms(self) -> dict:
        return {k: v for k, v in vars(type(self)).items() if isinstance(v, XmrisTerm)}

    def get_description(self, value: str) -> str:
        for term in self._terms().values():
            if term == value:
                return f"{term.description} [{term.unit}]" if term.unit else term.description
        return "No description available."

    def __iter__(self):
        return iter(self._terms().values())


class _Attrs(_Vocabulary):
    reference_frequency = XmrisTerm("reference_frequency", "Larmor frequency of the observed nucleus.", "MHz")
    carrier_ppm = XmrisTerm("carrier_ppm", "Chemical shift that sits at 0 Hz of the baseband signal.", "ppm")
    b0_field = XmrisTerm("b0_field", "Static field strength.", "Tesla")
    phase_p0 = XmrisTerm("phase_p0", "Zero-order phase applied to the whole spectrum.", "degrees")
    phase_p1 = XmrisTerm("phase_p1", "First-order phase: total twist over the full axis range.", "degrees")
    phase_pivot = XmrisTerm("phase_pivot", "Coordinate at which the first-order term vanishes.",
                            "dimension-dependent")
    phase_pivot_coord = XmrisTerm("phase_pivot_coord", "Name of the coordinate the pivot is expressed in.")
    apodization_lb = XmrisTerm("apodization_lb", "Exponential line broadening that was applied.", "Hz")
    apodization_gb = XmrisTerm("apodization_gb", "Gaussian broadening that was applied.", "Hz")
    zero_fill_target = XmrisTerm("zero_fill_target", "Number of points after zero filling.")
    zero_fill_position = XmrisTerm("zero_fill_position", "Where zeros were added: 'end' or 'symmetric'.")
    baseline_method = XmrisTerm("baseline_method", "Algorithm that estimated the removed baseline.")
    baseline_lam = XmrisTerm("baseline_lam", "Smoothness penalty of the AsLS baseline.")
    baseline_p = XmrisTerm("baseline_p", "Asymmetry parameter of the AsLS baseline.")
    baseline_iter = XmrisTerm("baseline_iter", "Number of AsLS re-weighting iterations.")
    coil_combine_method = XmrisTerm("coil_combine_method", "How the receive coils were combined: 'svd' or 'first_point'.")
    coil_combine_dim = XmrisTerm("coil_combine_dim", "Name of the coil dimension that was combined away.")
    align_dim = XmrisTerm("align_dim", "Name of the dimension whose transients were frequency- and phase-aligned.")
    align_reference = XmrisTerm("align_reference", "What the transients were aligned to: 'mean', 'first', an index or 'array'.")
    align_max_shift = XmrisTerm("align_max_shift", "Largest frequency shift the alignment searched.", "Hz")
    water_band = XmrisTerm("water_band", "Frequency band whose HSVD components were removed.", "Hz")
    water_rank = XmrisTerm("water_rank", "Number of damped exponentials of the HSVD model.")
    water_n_cols = XmrisTerm("water_n_cols", "Columns of the HSVD Hankel matrix.")
    denoise_dims = XmrisTerm("denoise_dims", "Names of the dimensions the denoising patch extends over.")
    denoise_patch = XmrisTerm("denoise_patch", "Patch size along each of the denoising dimensions.")
    mrsi_dims = XmrisTerm("mrsi_dims", "Names of the dimensions the spatial reconstruction transformed, as they were before it.")
    mrsi_matrix = XmrisTerm("mrsi_matrix", "Points along each transformed dimension after the reconstruction (the interpolated matrix).")
    mrsi_filter = XmrisTerm("mrsi_filter", "Spatial filter of the reconstruction: 'none', 'hamming', 'hann' or 'custom'.")
    mrsi_shift = XmrisTerm("mrsi_shift", "Shift applied along each transformed dimension.", "output points")
    sense_dims = XmrisTerm("sense_dims", "Names of the undersampled dimensions the SENSE unfolding restored to the full field of view.")
    sense_accel = XmrisTerm("sense_accel", "Acceleration along each unfolded dimension.")
    sense_regularization = XmrisTerm("sense_regularization", "Tikhonov weight of the SENSE unfolding, relative to the mean diagonal of S^H Psi^-1 S.")
    grappa_dims = XmrisTerm("grappa_dims", "Names of the undersampled k-space dimensions that GRAPPA filled to the full grid.")
    grappa_accel = XmrisTerm("grappa_accel", "Acceleration along each filled dimension.")
    grappa_kernel = XmrisTerm("grappa_kernel", "Acquired neighbour lines per filled dimension that one GRAPPA weight set combines.")
    grappa_regularization = XmrisTerm("grappa_regularization", "Tikhonov weight of the GRAPPA calibration, relative to the mean diagonal of the source Gram matrix.")
    grid_dims = XmrisTerm("grid_dims", "Names of the dimensions that gridding put in place of the sample dimension.")
    grid_matrix = XmrisTerm("grid_matrix", "Target matrix along each gridded dimension.")
    grid_oversampled = XmrisTerm("grid_oversampled", "Points of the oversampled Cartesian grid along each gridded dimension.")
    grid_width = XmrisTerm("grid_width", "Width of the Kaiser-Bessel gridding kernel.", "grid cells")
    grid_beta = XmrisTerm("grid_beta", "Shape parameter of the Kaiser-Bessel gridding kernel along each gridded dimension.")
    grid_density = XmrisTerm("grid_density", "Density compensation of the gridding: 'none', 'pipe' or 'custom'.")
    cgsense_iterations = XmrisTerm("cgsense_iterations", "Iteration cap of the CG-SENSE reconstruction.")
    cgsense_tol = XmrisTerm("cgsense_tol", "Relative residual at which a column of the CG-SENSE reconstruction stops.")
    cgsense_regularization = XmrisTerm("cgsense_regularization", "Tikhonov weight of the CG-SENSE reconstruction, relative to the mean diagonal of the normal matrix.")
    l1sense_sparsity = XmrisTerm("l1sense_sparsity", "Weight of the wavelet l1 penalty of the sparse SENSE reconstruction, relative to the largest |E^H D y| of the column.")
    l1sense_levels = XmrisTerm("l1sense_levels", "Haar levels per image dimension of the sparse SENSE reconstruction.")
    l1sense_iterations = XmrisTerm("l1sense_iterations", "Iteration cap of the sparse SENSE reconstruction.")
    l1sense_tol = XmrisTerm("l1sense_tol", "Relative change of the image at which a column of the sparse SENSE reconstruction stops.")
    l1sense_step = XmrisTerm("l1sense_step", "Step size of the proximal iteration of the sparse SENSE reconstruction.")
    l1sense_lipschitz = XmrisTerm("l1sense_lipschitz", "Lipschitz bound of the smooth part that the step size of the sparse SENSE reconstruction comes from.")
    time_shift_pad_to = XmrisTerm("time_shift_pad_to", "Transform length of the last time shift along the FID axis.")
    readout_time_corrected = XmrisTerm("readout_time_corrected", "Whether the acquisition delays of the readout's samples have been removed.")
    kinetics_model = XmrisTerm("kinetics_model", "Rate model that fit_kinetics fitted along the repetitions.")
    kinetics_substrate = XmrisTerm("kinetics_substrate", "Name of the metabolite whose measured amplitudes drive the rate model.")
    kinetics_dim = XmrisTerm("kinetics_dim", "Name of the repetition dimension the rates were fitted along.")
    kinetics_flip_angle = XmrisTerm("kinetics_flip_angle", "Flip angle of each metabolite of the rate model at every repetition.", "degrees")
    kinetics_rate_bounds = XmrisTerm("kinetics_rate_bounds", "Bounds of the fitted conversion rate.", "1/s")
    kinetics_decay_bounds = XmrisTerm("kinetics_decay_bounds", "Bounds of each product's effective decay rate (equal: fixed).", "1/s")
    kinetics_fit_initial = XmrisTerm("kinetics_fit_initial", "Whether the products' magnetisation before the first excitation was fitted.")
    species_frequencies = XmrisTerm("species_frequencies", "Name and frequency of each chemical species that was separated from the echoes.", "Hz")
    species_echo_times = XmrisTerm("species_echo_times", "Echo times the species were separated from.", "s")
    species_decay = XmrisTerm("species_decay", "Decay rate of each species in the separation model.", "1/s")
    species_nsa = XmrisTerm("species_nsa", "Effective number of signal averages of each species' estimate.")
    species_field = XmrisTerm("species_field", "Field offset of the separation model: 'none', 'given' or 'fitted'.")
    species_max_field = XmrisTerm("species_max_field", "Largest field offset the fit searched.", "Hz")
    lipid_level = XmrisTerm("lipid_level", "Singular value, relative to the largest, at which the lipid removal halves a component.")
    lipid_rank = XmrisTerm("lipid_rank", "Components of the lipid subspace that were removed.")
    lipid_beta = XmrisTerm("lipid_beta", "Weight of the L2 lipid penalty, 1 / (lipid_level x largest singular value)^2.")
    lipid_rows = XmrisTerm("lipid_rows", "Number of lipid rows (scalp voxels or given basis rows) the subspace was made from.")
    subspace_rank = XmrisTerm("subspace_rank", "Rank of the temporal subspace of the reconstruction.")
    subspace_sampled_fraction = XmrisTerm("subspace_sampled_fraction", "Fraction of the (sample, time) positions that were acquired.")
    denoise_rank = XmrisTerm("denoise_rank", "Components kept by the patch PCA denoising: 'mp' (Marchenko-Pastur rule) or the number.")


class _Dims(_Vocabulary):
    time = XmrisTerm("time", "Time axis of an FID.")
    frequency = XmrisTerm("frequency", "Relative frequency axis in Hz.")
    chemical_shift = XmrisTerm("chemical_shift", "Chemical-shift axis in ppm.")
    component = XmrisTerm("component", "Real / imaginary split axis.")
    average = XmrisTerm("average", "Signal averages.")
    coil = XmrisTerm("coil", "Receive coils.")
    echo = XmrisTerm("echo", "Echoes.")
    species = XmrisTerm("species", "Chemical species separated from the echoes.")
    coefficient = XmrisTerm("coefficient", "Coefficients of a temporal-subspace basis.")
    sample = XmrisTerm("sample", "Samples of a non-Cartesian k-space trajectory.")
    kx = XmrisTerm("kx", "k-space axis x.")
    ky = XmrisTerm("ky", "k-space axis y.")
    kz = XmrisTerm("kz", "k-space axis z.")
    x = XmrisTerm("x", "Image axis x.")
    y = XmrisTerm("y", "Image axis y.")
    z = XmrisTerm("z", "Image axis z.")


class _Coords(_Vocabulary):
    time = XmrisTerm("time", "Time coordinates.", "s")
    frequency = XmrisTerm("frequency", "Frequency coordinates.", "Hz")
    chemical_shift = XmrisTerm("chemical_shift", "Chemical-shift coordinates.", "ppm")
    kx = XmrisTerm("kx", "k-space coordinates along x.", "1/m")
    ky = XmrisTerm("ky", "k-space coordinates along y.", "1/m")
    kz = XmrisTerm("kz", "k-space coordinates along z.", "1/m")
    x = XmrisTerm("x", "Spatial coordinates along x.", "mm")
    y = XmrisTerm("y", "Spatial coordinates along y.", "mm")
    z = XmrisTerm("z", "Spatial coordinates along z.", "mm")


ATTRS = _Attrs()
DIMS = _Dims()
COORDS = _Coords()
