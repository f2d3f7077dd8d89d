"""The ``.xmr`` accessor for the spectral hot path.

Same method names, keyword names and defaults as the reference's ``XmrisAccessor`` mixins
(``src/xmris/core/accessor.py``: Fourier 369-446, Processing 449-593, Phasing 596-683; defaults pinned
by ``tests/test_core.py:497-552``).  Works on ``xmris_amd.LabeledArray`` out of the box and on
``xarray.DataArray`` after ``register_xarray_accessor()`` (called at import when xarray is installed
and no other package owns the name).  Everything outside the hot path (plots, widgets, fitting,
ppm conversion, vendor I/O) is out of scope.
"""
from __future__ import annotations

from .config import DIMS
from .processing.fid import apodize_exp, apodize_lg, to_fid, to_spectrum, zero_fill
from .processing.fourier import fft, fftc, fftshift, ifft, ifftc, ifftshift
from .processing.phasing import autophase, autophase_each, phase
from .dims import _check_dims  # noqa: F401  (the reference re-exports it from its accessor module)


class XmrisFourierMixin:
    def fftshift(self, dim):
        return fftshift(self._obj, dim=dim)

    def ifftshift(self, dim):
        return ifftshift(self._obj, dim=dim)

    def fft(self, dim=DIMS.time, out_dim=None):
        return fft(self._obj, dim=dim, out_dim=out_dim)

    def ifft(self, dim=DIMS.frequency, out_dim=None):
        return ifft(self._obj, dim=dim, out_dim=out_dim)

    def fftc(self, dim=DIMS.time, out_dim=None):
        return fftc(self._obj, dim=dim, out_dim=out_dim)

    def ifftc(self, dim=DIMS.frequency, out_dim=None):
        return ifftc(self._obj, dim=dim, out_dim=out_dim)


class XmrisProcessingMixin:
    def apodize_exp(self, dim: str = DIMS.time, lb: float = 1.0):
        return apodize_exp(self._obj, dim=dim, lb=lb)

    def apodize_lg(self, dim: str = DIMS.time, lb: float = 1.0, gb: float = 1.0):
        return apodize_lg(self._obj, dim=dim, lb=lb, gb=gb)

    def to_spectrum(self, dim: str = DIMS.time, out_dim: str = DIMS.frequency):
        return to_spectrum(self._obj, dim=dim, out_dim=out_dim)

    def to_fid(self, dim: str = DIMS.frequency, out_dim: str = DIMS.time):
        return to_fid(self._obj, dim=dim, out_dim=out_dim)

    def zero_fill(self, dim: str = DIMS.time, target_points: int = 1024, position: str = "end"):
        return zero_fill(self._obj, dim=dim, target_points=target_points, position=position)

    def baseline_als(self, dim: str = DIMS.frequency, lam: float = 1e5, p: float = 0.001, n_iter: int = 10):
        from .processing.baseline import baseline_als

        return baseline_als(self._obj, dim=dim, lam=lam, p=p, n_iter=n_iter)

    def combine_coils(self, dim: str = DIMS.coil, time_dim: str = DIMS.time, method: str = "svd", reference=None,
                      noise_cov=None, n_points: int = 1, return_weights: bool = False):
        """Per-voxel coil combination on the GPU (an addition of this backend)."""
        from .processing.coils import combine_coils

        return combine_coils(self._obj, dim=dim, time_dim=time_dim, method=method, reference=reference,
                             noise_cov=noise_cov, n_points=n_points, return_weights=return_weights)

    def remove_water(self, dim: str = DIMS.time, band=(-50.0, 50.0), rank: int = 20, n_cols: int = 64, dt: float = None,
                     return_components: bool = False):
        """Per-voxel HSVD removal of the residual water signal on the GPU (an addition of this backend)."""
        from .processing.water import remove_water

        return remove_water(self._obj, dim=dim, band=band, rank=rank, n_cols=n_cols, dt=dt,
                            return_components=return_components)

    def denoise_mppca(self, dims, patch, time_dim: str = DIMS.time, rank=None, return_noise: bool = False):
        """Marchenko-Pastur patch PCA denoising on the GPU (an addition of this backend)."""
        from .processing.denoise import denoise_mppca

        return denoise_mppca(self._obj, dims, patch, time_dim=time_dim, rank=rank, return_noise=return_noise)

    def align_averages(self, dim: str = DIMS.average, time_dim: str = DIMS.time, reference="mean", max_shift: float = 20.0,
                       t_max: float = None, n_points: int = None, passes: int = 1, average: bool = False,
                       min_quality: float = 0.0, return_shifts: bool = False):
        """Per-transient frequency and phase correction on the GPU (an addition of this backend)."""
        from .processing.align import align_averages

        return align_averages(self._obj, dim=dim, time_dim=time_dim, reference=reference, max_shift=max_shift,
                              t_max=t_max, n_points=n_points, passes=passes, average=average, min_quality=min_quality,
                              return_shifts=return_shifts)


class XmrisPhasingMixin:
    def phase(self, dim: str = DIMS.frequency, p0: float = 0.0, p1: float = 0.0, pivot: float = None):
        return phase(self._obj, dim=dim, p0=p0, p1=p1, pivot=pivot)

    def autophase(self, dim: str = DIMS.frequency, method: str = "acme", peak_width: int = 100,
                  lb: float = 0.0, temp_time_dim: str = DIMS.time, **kwargs):
        # NB the accessor's peak_width default (100) differs from the function's (0.5), as in the
        # reference (accessor.py:634 vs phasing.py:166)
        return autophase(self._obj, dim=dim, method=method, peak_width=peak_width, lb=lb,
                         temp_time_dim=temp_time_dim, **kwargs)


    def autophase_each(self, dim: str = DIMS.frequency, method: str = "acme", peak_width: int = 100,
                       lb: float = 0.0, temp_time_dim: str = DIMS.time, **kwargs):
        """One (p0, p1) per spectrum along `dim` (an addition of this backend: the reference's ``mode="all"``)."""
        return autophase_each(self._obj, dim=dim, method=method, peak_width=peak_width, lb=lb,
                              temp_time_dim=temp_time_dim, **kwargs)


class XmrisVendorMixin:
    def remove_digital_filter(self, group_delay: float, dim: str = "time", keep_length: bool = True):
        from .vendor.bruker import remove_digital_filter

        return remove_digital_filter(self._obj, group_delay=group_delay, dim=dim, keep_length=keep_length)


class XmrisFusedMixin:
    def spectral_pipeline(self, target_points: int = 1024, lb: float = 1.0, dim: str = DIMS.time,
                          out_dim: str = DIMS.frequency, method: str = "acme", peak_width: int = 100, **kwargs):
        """zero_fill -> apodize_exp -> to_spectrum -> autophase in two fused launches (an addition of
        this backend; result and metadata equal the four chained calls)."""
        from .fused import spectral_pipeline

        return spectral_pipeline(self._obj, target_points=target_points, lb=lb, dim=dim, out_dim=out_dim,
                                 method=method, peak_width=peak_width, **kwargs)


class XmrisMrsiMixin:
    def to_image(self, dim=(DIMS.kx, DIMS.ky), out_dim=None, matrix=None, filter=None, shift=None):
        """k-space to voxels: filter, zero fill, voxel shift and centred inverse transform, one launch per dim (an
        addition of this backend)."""
        from .processing.mrsi import to_image

        return to_image(self._obj, dim=dim, out_dim=out_dim, matrix=matrix, filter=filter, shift=shift)

    def to_kspace(self, dim=(DIMS.x, DIMS.y), out_dim=None, matrix=None, filter=None, shift=None):
        """Voxels to k-space: the forward counterpart of ``to_image``."""
        from .processing.mrsi import to_kspace

        return to_kspace(self._obj, dim=dim, out_dim=out_dim, matrix=matrix, filter=filter, shift=shift)

    def grid_kspace(self, trajectory, matrix, oversampling: float = 2.0, width: int = 4, density=None,
                    dim: str = DIMS.sample, out_dim=None, fov=1.0, iterations: int = 10, readout_time=None):
        """Non-Cartesian samples to the oversampled Cartesian k-space, one launch of the gather kernel (an addition of
        this backend)."""
        from .processing.grid import grid_kspace

        return grid_kspace(self._obj, trajectory, matrix, oversampling=oversampling, width=width, density=density,
                           dim=dim, out_dim=out_dim, fov=fov, iterations=iterations, readout_time=readout_time)

    def degrid_kspace(self, trajectory, matrix, oversampling: float = 2.0, width: int = 4, dim=None,
                      out_dim: str = DIMS.sample, readout_time=None):
        """The oversampled Cartesian k-space at a trajectory's samples: the transpose of ``grid_kspace`` (DESIGN.md
        section 17)."""
        from .processing.grid import degrid_kspace

        return degrid_kspace(self._obj, trajectory, matrix, oversampling=oversampling, width=width, dim=dim, out_dim=out_dim,
                             readout_time=readout_time)

    def nufft_adjoint(self, trajectory, matrix, oversampling: float = 2.0, width: int = 4, density=None,
                      dim: str = DIMS.sample, out_dim=None, fov=1.0, iterations: int = 10, readout_time=None):
        """Non-Cartesian samples to voxels: gridding, centred inverse transform, crop and de-apodisation (DESIGN.md
        section 17)."""
        from .processing.grid import nufft_adjoint

        return nufft_adjoint(self._obj, trajectory, matrix, oversampling=oversampling, width=width, density=density,
                             dim=dim, out_dim=out_dim, fov=fov, iterations=iterations, readout_time=readout_time)

    def nufft_forward(self, trajectory, matrix=None, oversampling: float = 2.0, width: int = 4, dim=None,
                      out_dim: str = DIMS.sample, readout_time=None):
        """Voxels to non-Cartesian samples: the transpose chain of ``nufft_adjoint``."""
        from .processing.grid import nufft_forward

        return nufft_forward(self._obj, trajectory, matrix=matrix, oversampling=oversampling, width=width, dim=dim,
                             out_dim=out_dim, readout_time=readout_time)

    def recon_cg_sense(self, trajectory, sensitivities, matrix=None, iterations: int = 20, tol: float = 1e-6,
                       regularization: float = 0.0, density=None, noise_cov=None, oversampling: float = 2.0,
                       width: int = 4, dim: str = DIMS.sample, coil_dim: str = DIMS.coil, out_dim=None, fov=1.0,
                       readout_time=None, chunk=None, return_info: bool = False):
        """Iterative SENSE of multi-coil, undersampled, non-Cartesian samples: conjugate gradients around the two NUFFT
        chains, every column on its own (an addition of this backend)."""
        from .processing.cgsense import recon_cg_sense

        return recon_cg_sense(self._obj, trajectory, sensitivities, matrix=matrix, iterations=iterations, tol=tol,
                              regularization=regularization, density=density, noise_cov=noise_cov,
                              oversampling=oversampling, width=width, dim=dim, coil_dim=coil_dim, out_dim=out_dim, fov=fov,
                              readout_time=readout_time, chunk=chunk, return_info=return_info)

    def recon_l1_sense(self, trajectory, sensitivities, matrix=None, sparsity: float = 0.02, levels=None, iterations: int = 50,
                       tol: float = 1e-4, tikhonov: float = 0.0, cycle_spin: bool = False, step=None,
                       power_iterations: int = 20, step_safety=None, density=None, noise_cov=None, oversampling: float = 2.0,
                       width: int = 4, dim: str = DIMS.sample, coil_dim: str = DIMS.coil, out_dim=None, fov=1.0,
                       readout_time=None, chunk=None, return_info: bool = False):
        """Wavelet-sparse iterative SENSE of multi-coil, undersampled, non-Cartesian samples: FISTA with a blockwise
        Haar l1 penalty around the two NUFFT chains, every column on its own (an addition of this backend; DESIGN.md
        section 24)."""
        from .processing.l1sense import STEP_SAFETY, recon_l1_sense

        return recon_l1_sense(self._obj, trajectory, sensitivities, matrix=matrix, sparsity=sparsity, levels=levels,
                              iterations=iterations, tol=tol, tikhonov=tikhonov, cycle_spin=cycle_spin, step=step,
                              power_iterations=power_iterations, step_safety=STEP_SAFETY if step_safety is None else step_safety,
                              density=density, noise_cov=noise_cov, oversampling=oversampling, width=width, dim=dim,
                              coil_dim=coil_dim, out_dim=out_dim, fov=fov, readout_time=readout_time, chunk=chunk,
                              return_info=return_info)

    def recon_subspace(self, trajectory, sensitivities, basis, sampling=None, matrix=None, iterations: int = 30,
                       tol: float = 1e-6, regularization: float = 0.0, density=None, noise_cov=None, oversampling: float = 2.0,
                       width: int = 4, dim: str = DIMS.sample, coil_dim: str = DIMS.coil, time_dim: str = DIMS.time,
                       out_dim=None, fov=1.0, chunk=None, return_info: bool = False, return_coefficients: bool = False):
        """Temporal-subspace iterative SENSE of (k, t)-undersampled non-Cartesian samples: only the coefficient columns
        of a basis from ``temporal_basis`` go through the NUFFT chains (an addition of this backend; DESIGN.md section
        26)."""
        from .processing.subspace import recon_subspace

        return recon_subspace(self._obj, trajectory, sensitivities, basis, sampling=sampling, matrix=matrix,
                              iterations=iterations, tol=tol, regularization=regularization, density=density,
                              noise_cov=noise_cov, oversampling=oversampling, width=width, dim=dim, coil_dim=coil_dim,
                              time_dim=time_dim, out_dim=out_dim, fov=fov, chunk=chunk, return_info=return_info,
                              return_coefficients=return_coefficients)

    def espirit_maps(self, matrix, kernel=None, dims=(DIMS.kx, DIMS.ky), coil_dim: str = DIMS.coil,
                     time_dim: str = DIMS.time, acs_points: int = 8, threshold: float = 0.02, crop: float = 0.8,
                     n_maps: int = 1, noise_cov=None, phase_ref: int = 0, return_eigenvalues: bool = False):
        """ESPIRiT coil sensitivities from this auto-calibration block of k-space, for ``unfold_sense`` and
        ``recon_cg_sense`` (an addition of this backend)."""
        from .processing.espirit import espirit_maps

        return espirit_maps(self._obj, matrix, kernel=kernel, dims=dims, coil_dim=coil_dim, time_dim=time_dim,
                            acs_points=acs_points, threshold=threshold, crop=crop, n_maps=n_maps, noise_cov=noise_cov,
                            phase_ref=phase_ref, return_eigenvalues=return_eigenvalues)

    def shift_time(self, delay, dim: str = DIMS.time, pad_to=None, dwell=None):
        """Each row along `dim` evaluated `delay` earlier, one fused launch (an addition of this backend; DESIGN.md
        section 18)."""
        from .processing.timeshift import shift_time

        return shift_time(self._obj, delay, dim=dim, pad_to=pad_to, dwell=dwell)

    def separate_species(self, frequencies, echo_times=None, dim: str = DIMS.echo, out_dim: str = DIMS.species, decay=None,
                         readout_time=None, sample_dim: str = DIMS.sample, field_map=None, fit_field: bool = False,
                         max_field=None, share=(DIMS.coil,), return_field: bool = False):
        """Chemical-species amplitudes from a few echoes by least squares (an addition of this backend; DESIGN.md
        section 23)."""
        from .processing.species import separate_species

        return separate_species(self._obj, frequencies, echo_times=echo_times, dim=dim, out_dim=out_dim, decay=decay,
                                readout_time=readout_time, sample_dim=sample_dim, field_map=field_map,
                                fit_field=fit_field, max_field=max_field, share=share, return_field=return_field)

    def remove_lipids(self, lipid_mask=None, *, basis=None, dims=None, level: float = 0.01, rank=None, apply_mask=None,
                      return_basis: bool = False, dim: str = DIMS.time):
        """Lipid-subspace (L2) suppression: every row minus its weighted projection onto the subspace of the scalp
        voxels' FIDs, one launch (an addition of this backend)."""
        from .processing.lipids import remove_lipids

        return remove_lipids(self._obj, lipid_mask, basis=basis, dims=dims, level=level, rank=rank,
                             apply_mask=apply_mask, return_basis=return_basis, dim=dim)

    def correct_readout_time(self, offsets, dim: str = DIMS.time, sample_dim: str = DIMS.sample, pad_to=None, dwell=None,
                             inverse: bool = False):
        """Undo the acquisition delay of each sample of a non-Cartesian readout."""
        from .processing.timeshift import correct_readout_time

        return correct_readout_time(self._obj, offsets, dim=dim, sample_dim=sample_dim, pad_to=pad_to, dwell=dwell,
                                    inverse=inverse)

    def unfold_sense(self, sensitivities, accel, dims=(DIMS.x, DIMS.y), coil_dim: str = DIMS.coil,
                     time_dim: str = DIMS.time, noise_cov=None, regularization: float = 0.0, return_maps: bool = False):
        """SENSE unfolding of the aliased images of a regularly undersampled k-space, one launch for all voxel groups
        (an addition of this backend)."""
        from .processing.sense import unfold_sense

        return unfold_sense(self._obj, sensitivities, accel, dims=dims, coil_dim=coil_dim, time_dim=time_dim,
                            noise_cov=noise_cov, regularization=regularization, return_maps=return_maps)

    def grappa_fill(self, weights=None, *, acs=None, accel=None, kernel=None, dims=None, coil_dim: str = DIMS.coil,
                    time_dim: str = DIMS.time, acs_points: int = 8, regularization: float = 1e-4,
                    return_weights: bool = False):
        """GRAPPA fill of a regularly undersampled k-space to the full grid, the weights given or calibrated from a
        fully sampled centre block, one launch (an addition of this backend)."""
        from .processing.grappa import grappa_fill

        return grappa_fill(self._obj, weights, acs=acs, accel=accel, kernel=kernel, dims=dims, coil_dim=coil_dim,
                           time_dim=time_dim, acs_points=acs_points, regularization=regularization,
                           return_weights=return_weights)


class XmrisFittingMixin:
    def fit_amares(self, prior_knowledge_file, dim: str = "time", mhz: float = None, sw: float = None,
                   deadtime: float = None, method: str = "leastsq", initialize_with_lm: bool = True,
                   num_workers: int = 4, init_fid=None, verbose: bool = False):
        from .fitting.amares import fit_amares

        return fit_amares(self._obj, prior_knowledge_file, dim=dim, mhz=mhz, sw=sw, deadtime=deadtime, method=method,
                          initialize_with_lm=initialize_with_lm, num_workers=num_workers, init_fid=init_fid,
                          verbose=verbose)

    def fit_basis(self, basis, dim: str = "time", names=None, groups=None, lineshape: str = "voigt",
                  max_shift: float = 10.0, max_broadening: float = 20.0, broadening_start: float = 2.0,
                  max_gaussian: float = 20.0, gaussian_start: float = 2.0, fit_phase: bool = True, skip: int = 0,
                  amplitude_start=None, max_iter: int = 200, return_fit: bool = True):
        """Basis-set (linear-combination) quantification of every FID (an addition of this backend; DESIGN.md
        section 15)."""
        from .fitting.basis import fit_basis

        return fit_basis(self._obj, basis, dim=dim, names=names, groups=groups, lineshape=lineshape,
                         max_shift=max_shift, max_broadening=max_broadening, broadening_start=broadening_start,
                         max_gaussian=max_gaussian, gaussian_start=gaussian_start, fit_phase=fit_phase, skip=skip,
                         amplitude_start=amplitude_start, max_iter=max_iter, return_fit=return_fit)

    def fit_kinetics(self, substrate, products, dim: str = "repetition", times=None, flip_angle=None,
                     r1=(1.0 / 60.0, 1.0 / 10.0), rate_bounds=(0.0, 1.0), fit_initial: bool = False, sigma=None,
                     metabolite_dim: str = "Metabolite", max_iter: int = 200):
        """Per-voxel conversion rates of a dynamic series of amplitudes (an addition of this backend; DESIGN.md
        section 19)."""
        from .fitting.kinetics import fit_kinetics

        return fit_kinetics(self._obj, substrate, products, dim=dim, times=times, flip_angle=flip_angle, r1=r1,
                            rate_bounds=rate_bounds, fit_initial=fit_initial, sigma=sigma, metabolite_dim=metabolite_dim,
                            max_iter=max_iter)


class XmrisAccessor(XmrisFourierMixin, XmrisProcessingMixin, XmrisPhasingMixin, XmrisVendorMixin, XmrisFusedMixin,
                    XmrisFittingMixin, XmrisMrsiMixin):
    """``obj.xmr.<method>`` for the hot-path methods."""

    def __init__(self, obj):
        self._obj = obj


def register_xarray_accessor(name: str = "xmr", force: bool = False) -> bool:
    """Register the accessor on ``xarray.DataArray``.  Returns False when xarray is missing or the
    name is already taken (e.g. by the reference package) and `force` is not set."""
    try:
        import xarray as xr
    except ImportError:
        return False
    if hasattr(xr.DataArray, name) and not force:
        return False
    import warnings

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        xr.register_dataarray_accessor(name)(XmrisAccessor)
    return True
