/* xmris_hip.h -- C ABI of libxmris_hip.so: the MI355X (gfx950) backend of the xmris `.xmr`
 * spectral hot path  zero_fill -> apodize_exp -> to_spectrum (ortho FFT + fftshift) -> autophase.
 *
 * The reference (andrewendlinger/xmris v0.6.1) is pure Python and has no FFI; the seam these
 * entry points replace is the ndarray boundary inside `src/xmris/processing/*.py`
 * (`da.values` + `da.get_axis_num(dim)` on the way in, `da.copy(data=...)` on the way out).
 * Each function cites the reference statement it stands in for.  All metadata (dims, coords,
 * attrs, validation, exceptions) stays in the Python host layer (`xmris_amd/`).
 *
 * Conventions
 *  - Plain C types only.  All array pointers are DEVICE-ACCESSIBLE pointers owned by the caller (device
 *    memory; small outputs may also live in hipHostMalloc'd host memory, which the selection stage uses
 *    to hand (max, flat index, winning spectrum) to the host without memcpy nodes); the
 *    library never frees or retains them.  `stream` is a hipStream_t passed as void* (NULL =
 *    the default stream).  Calls are asynchronous on that stream; nothing synchronises.
 *  - Layout: `n_batch` spectra, C-contiguous, FID / frequency axis last, interleaved complex
 *    (re, im).  dtype XM_C64 = 2 x float32, XM_C128 = 2 x float64.
 *  - Return value: 0 on success, negative xm_status on failure (no exceptions, no aborts);
 *    `xm_last_error_string()` describes the last failure on the calling thread.
 *  - Twiddle / chirp tables are computed in fp64 on the host, rounded once to the storage
 *    precision and cached per (length, dtype, device) inside the library (mutex-guarded);
 *    `xm_clear_cache()` frees them.  Reentrant otherwise.
 *  - Device: the device that owns the input buffer is made current for the duration of a call (tables, occupancy
 *    caches and scratch are per device); `stream` must belong to that device.
 */
#ifndef XMRIS_HIP_H
#define XMRIS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum { XM_C64 = 0, XM_C128 = 1 } xm_dtype;

typedef enum {
  XM_OK = 0,
  XM_ERR_INVALID_ARG = -1,   /* null pointer, negative size, bad dtype/flag combination   */
  XM_ERR_UNSUPPORTED_N = -2, /* transform length has no in-LDS plan (see xm_fft_supported) */
  XM_ERR_HIP = -3,           /* a HIP runtime call failed; see xm_last_error_string()      */
  XM_ERR_NO_DEVICE = -4
} xm_status;

/* xm_fft1d_batched / xm_pipeline_fused flags */
#define XM_FFT_INVERSE 1u   /* e^{+2 pi i km/N}  (np.fft.ifftn, fourier.py:210)             */
#define XM_FFT_ORTHO 2u     /* scale 1/sqrt(N)   (norm="ortho", fourier.py:153)             */
#define XM_FFT_SHIFT_IN 4u  /* roll the INPUT by (N+1)/2 first  (ifftshift, fourier.py:57)  */
#define XM_FFT_SHIFT_OUT 8u /* roll the OUTPUT by N/2 afterwards (fftshift, fourier.py:31)  */
#define XM_AMAX_VALUE_ONLY 16u /* xm_pipeline_fused: absmax2[b] only, argidx[b] is written as 0 (the caller
                                  recovers the index along the axis from the winning spectrum itself)      */

#define XM_AMAX_GLOBAL_KEY 32u /* xm_pipeline_fused(_ramp), geometries of xm_pipeline_ramp_native only: `absmax2` points to
                                  an arg-max KEY BUFFER (XM_KEY_BYTES bytes, zero at launch) that receives the global
                                  arg-max of the launch as partial keys, max |X|^2 float bits << 32 | (0xffffffff - row);
                                  no per-row outputs.  `argidx` == NULL: the key stays for xm_argmax_key_take (merges,
                                  decodes, clears).  `argidx` != NULL: it points to a result record `xm_argmax_result`, device-accessible --
                                  e.g. pinned host memory -- that the kernel's last workgroup fills itself, clearing the key. */
#define XM_KEY_BYTES 131072   /* 64 partial keys on cache lines of their own (8 KiB), scratch words of the consumers, and from
                                 byte 65536 the per-wave (value, row) slots of the complex128 kernels */
typedef struct {
  float max2;   /* max |X|^2 of the launch (XM_C128: these eight bytes hold it as a double) */
  float pad_;
  int64_t flat; /* winning row * n_out (index along the axis: 0) */
} xm_argmax_result;
/* XM_C64 without a >= 2x zero fill (the plans of k_fft2: 512 ... 8192, 3 * 2^k) takes the key in the
 * xm_pipeline_fused_ramp form only, with an output and at least two rows.
 * XM_C128 takes XM_AMAX_GLOBAL_KEY on the geometries of xm_pipeline_key_native (half lengths 4096 and 8192) and only with a
 * result record: 64 bits of value + a row do not fit one atomic, so every wave leaves its (value, row) pair in a slot
 * of the key buffer and the last workgroup out merges them; the key buffer needs no clearing. */

int xm_version(void); /* 10000*major + 100*minor + patch */
const char* xm_last_error_string(void);
int xm_clear_cache(void);
/* The kernel the fused dispatcher (xm_pipeline_fused / _ramp, xm_fft1d_batched, xm_guess_*) launched last ON THE
 * CALLING THREAD, spelled as the profiler spells it, e.g. "k_zf2p<FftPlan<4096,256,16,16,16>, 13, 11>" (template, plan,
 * mode words): reports and counter files are matched against this, not against a string typed by hand. */
const char* xm_last_kernel_string(void);
/* 1 if a length-n transform of `dtype` has an in-LDS plan (direct or Bluestein), else 0. */
int xm_fft_supported(int n, int dtype);
/* Build (and cache) the tables for length n so that later calls do no allocation. */
int xm_plan_prepare(int n, int dtype);

/* A1  zero_fill  (processing/fid.py:251  da.pad(..., constant_values=0)).
 * out[b, j] = in[b, j - pad_left] for pad_left <= j < pad_left + n_in, else 0.  Bit-exact copy. */
int xm_zero_fill(const void* in, void* out, int64_t n_batch, int n_in, int n_out, int pad_left,
                 int dtype, void* stream);

/* A2  apodize  (processing/fid.py:139  da * weight).  out[b, j] = in[b, j] * window[j];
 * `window` is n real values of the storage precision (host computes exp(-pi*lb*t), fid.py:136).
 * in == out allowed. */
int xm_apodize(const void* in, void* out, const void* window, int64_t n_batch, int n, int dtype,
               void* stream);

/* A1 + A2 in ONE pass  (processing/fid.py:251 `da.pad(...)` followed by fid.py:136-139 `da * exp(-pi lb t)`):
 *   out[b, j] = in[b, j - pad_left] * window[j]  for pad_left <= j < pad_left + n_in,  +0 elsewhere.
 * The fused zero-fill + apodisation launch for chains that stop before the FFT: 16-byte loads of the FID axis, the
 * window staged through the LDS, nontemporal 16-byte stores, rows handed out by a device-scope counter.  `window`:
 * n_out reals of the OUTPUT precision.  `out_dtype` = `in_dtype`, or XM_C128 for XM_C64 rows (numpy's promotion when a
 * complex64 FID meets the float64 window, fid.py:136-139: each product is then the exact complex128 product numpy
 * computes).  n_out * sizeof(real) <= 96 KiB.  in != out. */
int xm_zf_apod(const void* in, int64_t in_row_stride, void* out, const void* window, int64_t n_batch, int n_in, int n_out,
               int pad_left, int in_dtype, int out_dtype, void* stream);

/* A3/A4/A5  fft / ifft / fftshift folded  (processing/fourier.py:153, 210, 31, 57).
 * out[b, (m + s_out) mod n] = scale * sum_k in[b, (k - s_in) mod n] * e^{-+2 pi i k m / n}. */
/* 1 when xm_pipeline_fused(_ramp) accepts XM_AMAX_GLOBAL_KEY for this geometry and dtype, else 0. */
int xm_pipeline_key_native(const void* in, int64_t in_row_stride, int n_in, int n_out, int pad_left, unsigned flags,
                           int dtype);

int xm_fft1d_batched(const void* in, void* out, int64_t n_batch, int n, unsigned flags, int dtype,
                     void* stream);

/* A4 alone  (fourier.py:31-32, 57-58  da.roll).  out[b, (j + shift) mod n] = in[b, j]. */
int xm_roll(const void* in, void* out, int64_t n_batch, int n, int shift, int dtype, void* stream);

/* A8  phase apply  (processing/phasing.py:73  da * exp(1j*phase_array)).
 * out[b, j] = in[b, j] * phase_table[j]  (n complex values; host computes e^{i phi}, phasing.py:62-69).
 * in == out allowed. */
int xm_phase_apply(const void* in, void* out, const void* phase_table, int64_t n_batch, int n,
                   int dtype, void* stream);

/* A6  per-spectrum max |X|^2 and its first index  (first half of phasing.py:229).
 * absmax2[b] (real, storage precision) and argidx[b] (int32) for every spectrum of an existing array. */
int xm_absmax_rows(const void* in, int64_t n_batch, int n, void* absmax2, int32_t* argidx, int dtype,
                   void* stream);

/* A6, speculative schedule: norm[b] = sum_j |in[b, j]| * |window[j + pad_left]| (window may be NULL), the windowed
 * L1 norm of every FID.  sum|z| / sqrt(N) bounds every |X[k]| of the row and equals the peak of a single decaying
 * resonance, so the row with the largest norm is the guess for the row through the global maximum
 * (phasing.py:229) that lets the host search (p0, p1) BEFORE any spectrum exists; the fused main pass then
 * returns the true per-row maxima, and a wrong guess is repaired (see xmris_amd/pipeline.py::run_stream).
 * Only a ranking is needed, so the sum may run over a regular subset: the 1-KiB blocks (128 complex64 / 64
 * complex128 samples) whose index is a multiple of `sub_step` (1 = every sample), i.e. whole cache lines spread
 * over the n_in leading samples.
 * `norm`: n_batch reals of the storage precision. */
int xm_row_l1(const void* in, int64_t in_row_stride, const void* window, int64_t n_batch, int n_in, int pad_left,
              int sub_step, void* norm, uint64_t* key, int dtype, void* stream);
/* `key` (complex64 only, may be NULL): an arg-max key buffer (XM_KEY_BYTES, zero at launch) that receives the row with
 * the largest norm as float bits << 32 | (0xffffffff - row) -- the launch then needs no separate arg-max reduction;
 * `norm` may be NULL. */

/* A6: consumer of an arg-max key buffer written by xm_row_l1 / XM_AMAX_GLOBAL_KEY: out_max2[0] (float) = the value,
 * out_flat[0] = row * n_per_row, buffer := 0 for its next producer.  With `in` (n_batch x n_in rows, dtype) also
 * out_row[j] = (complex128) in[row, j] -- xm_gather_row_c128 of the winning row in the same launch.  `in` / `out_row`
 * may be NULL.  out_* are device-accessible (the selection stage passes pinned host memory). */
int xm_argmax_key_take(uint64_t* key, int n_per_row, void* out_max2, int64_t* out_flat, const void* in,
                       int64_t in_row_stride, int n_in, void* out_row, int dtype, void* stream);

/* A6, speculative schedule, guess stage (replaces xm_row_l1 + xm_argmax_key_take where xm_guess_supported() says so).
 * The host searches (p0, p1) on the spectrum of the row that holds the global max |X| (phasing.py:229, 241-242)
 * BEFORE the spectra exist; these two calls find that row without transforming every row in full:
 *   xm_guess_rows    est[b] = max_k |X_c[b, k]|^2 of a COARSE spectrum of row b -- its first n_guess (<= 512; 0 = 512)
 *                    samples times their window weights on a 1024-bin grid (one wave per row; 4 KiB of a 32 KiB row
 *                    read) -- and the largest estimate in `key` (an arg-max key buffer, zero at launch).  A truncated,
 *                    coarsely sampled spectrum underestimates a line's height by a bounded factor (scalloping of the
 *                    grid, the missing tail), so the true arg-max row lies among the rows whose estimate is within
 *                    that band of the largest one.  Rows of 512 samples and more are transformed on the matrix
 *                    cores (fp16 operands behind a per-row power-of-two scale, fp32 sums: est within 2e-3 of the exact
 *                    coarse spectrum's maximum; a NaN sample gives NaN), other rows by the fp32 FFT (2e-5);
 *   xm_guess_refine  transforms every row with est[b] >= band^2 * max(est) exactly (all n_in samples -> n_out bins, the
 *                    arithmetic of xm_pipeline_fused; at most 16 rows per resident workgroup) and leaves the winner
 *                    like xm_argmax_key_take does: out_max2[0] = its max |X|^2 (float), out_flat[0] = row * n_out,
 *                    out_row[j] = (complex128) in[row, j].  `guess_key` is consumed (left zero), `work_key` is a second
 *                    key buffer (zero at launch, left zero).
 * Geometry: "end" zero fill to >= 2x (pad_left = 0, n_out/2 in {512 ... 8192}); `window`: n_out FLOAT32 weights for
 * either dtype; XM_C128 rows are converted to float on load (a ranking; the main pass's own maxima verify the guess,
 * xmris_amd/pipeline.py::run_stream).  `est`: n_batch floats.  out_* device-accessible (pinned host memory is fine). */
int xm_guess_supported(const void* in, int64_t in_row_stride, int n_in, int n_out, int pad_left, unsigned flags, int dtype);
int xm_guess_rows(const void* in, int64_t in_row_stride, const void* window, int64_t n_batch, int n_in, int n_out,
                  int n_guess, unsigned flags, float* est, uint64_t* key, int dtype, void* stream);
int xm_guess_refine(const void* in, int64_t in_row_stride, const void* window, int64_t n_batch, int n_in, int n_out,
                    unsigned flags, const float* est, uint64_t* guess_key, float band, uint64_t* work_key,
                    float* out_max2, int64_t* out_flat, void* out_row, int dtype, void* stream);

/* A6  global arg-max  (phasing.py:229  np.argmax(np.abs(values)), first maximum in C order).
 * Reduces the per-spectrum pairs: out_max2[0] = max_b absmax2[b], out_flat[0] = b*n + argidx[b]
 * of the first such b.  Both outputs are device-accessible scalars. */
int xm_argmax_reduce(const void* absmax2, const int32_t* argidx, int64_t n_batch, int n, void* out_max2,
                     int64_t* out_flat, int dtype, void* stream);

/* A6  the ONE spectrum through the global maximum (phasing.py:241-242 `da.isel(...)`), fetched without a host
 * round trip: out[j] = (complex128) in[row, j], j < n_in, with row = flat_index[0] / n_per_row read from DEVICE
 * memory (the output of xm_argmax_reduce).  Feeds the complex128 recomputation of that spectrum for the solver. */
int xm_gather_row_c128(const void* in, int64_t in_row_stride, int n_in, const int64_t* flat_index, int n_per_row,
                       void* out, int dtype, void* stream);

/* The fused hot path, one launch:
 *   z[j]   = (pad_left <= j < pad_left + n_in) ? in[b, j - pad_left] * window[j] : 0   (A1+A2)
 *   X      = FFT_n_out(z) * scale, optionally rolled                                    (A3+A4)
 *   absmax2[b], argidx[b] = max |X|^2 and its first index (after the roll)              (A6)
 *   out[b, k] = X[k] * phase_table[k]                                                   (A8)
 * `window` (n_out reals), `phase_table` (n_out complex), `out`, `absmax2`, `argidx` may each be
 * NULL to skip that part (out == NULL -> the arg-max pre-pass, nothing is written but the pairs).
 * `in_row_stride` = elements between consecutive input spectra (>= n_in). */
int xm_pipeline_fused(const void* in, int64_t in_row_stride, void* out, const void* window,
                      const void* phase_table, int64_t n_batch, int n_in, int n_out, int pad_left,
                      unsigned flags, void* absmax2, int32_t* argidx, int dtype, void* stream);

/* The fused hot path with the autophase ramp in closed form (A8, processing/phasing.py:62-73: on a uniform axis
 * phi[k] = rad(p0) + rad(p1) * (c[k] - pivot) / range is linear in the output index k):
 *   out[b, k] = X[k] * e^{i (phase0 + dphase * k)},   phase0 / dphase in radians, fp64.
 * Everything else as xm_pipeline_fused (`out` must be given).  On the ">= 2x end zero fill" geometries
 * (xm_pipeline_ramp_native: complex64 with 16-byte aligned rows, complex128 always) the kernel applies the ramp in
 * factorised form -- no table exists, nothing is read per output; other geometries expand the ramp into a
 * stream-ordered scratch table first. */
int xm_pipeline_fused_ramp(const void* in, int64_t in_row_stride, void* out, const void* window, double phase0,
                           double dphase, int64_t n_batch, int n_in, int n_out, int pad_left, unsigned flags,
                           void* absmax2, int32_t* argidx, int dtype, void* stream);
/* 1 if xm_pipeline_fused_ramp applies the ramp natively for this geometry (see above), else 0. */
int xm_pipeline_ramp_native(const void* in, int64_t in_row_stride, int n_in, int n_out, int pad_left, unsigned flags,
                            int dtype);

/* "next" (SURVEY 8f rank 4): asymmetric-least-squares baseline (processing/baseline.py:10-40 `_als_core`
 * applied along the last axis by `xr.apply_ufunc`, :102-110).  For every spectrum: n_iter rounds of
 * (W + lam*D'D) z = W y (pentadiagonal SPD, band LDL' in fp64) and w = p (y > z) + (1 - p) (y < z);
 * out[b, j] = y[b, j] - z[b, j] in float64, y = the REAL part of the input (is_complex) or the input itself
 * (real float32 / float64 for XM_C64 / XM_C128); n >= 4.  `workspace`: device scratch of
 * xm_baseline_als_workspace_bytes(n_batch, n) bytes owned by the caller. */
int64_t xm_baseline_als_workspace_bytes(int64_t n_batch, int n);
int xm_baseline_als(const void* in, int is_complex, int64_t n_batch, int n, double lam, double p, int n_iter, void* out,
                    void* workspace, int64_t workspace_bytes, int dtype, void* stream);

/* ---- quantification: AMARES time-domain fitting (reference fitting/amares.py:207-488, fitting/simulation.py:9-96).
 * Model: x^(t) = sum_k a_k e^{i phi_k} exp(-d_k (1 - g_k + g_k t) t) e^{i 2 pi f_k t}, t_j = j dt + t0.  Parameters of
 * peak k are params[5k + c], c = 0 amplitude, 1 frequency [Hz], 2 damping [1/s], 3 phase [rad], 4 lineshape g; fp64.
 *
 * xm_amares_model: out[b, j] (complex128) = x^(t_j) for the parameters params[b, :, :] ([n_batch, n_peaks, 5]). */
int xm_amares_model(const double* params, int64_t n_batch, int n_peaks, int n, double dt, double t0, void* out,
                    void* stream);
/* xm_amares_fit: one Levenberg-Marquardt fit per row of `in` (n_batch rows of n complex samples, dtype XM_C64 / XM_C128,
 * `in_row_stride` elements apart) in lmfit's internal bound variables, every row from the same start.  Prior
 * knowledge: HOST arrays of 5 n_peaks values -- `init` (clipped into its bounds), `lower` / `upper` (+-inf: unbounded
 * side), `fixed` (nonzero, or lower == upper: held at its value, not fitted).  Stops when the scaled step
 * ||D d|| <= xtol (||D u|| + xtol), the relative cost reduction of an accepted step is <= ftol, or after max_iter trial
 * steps.  Outputs (device): params[n_batch, n_peaks, 5] physical, amp_sd[n_batch, n_peaks] = sqrt of the amplitude's
 * diagonal entry of (J^T J)^{-1} over the physical free parameters at the solution (the caller scales it by sigma;
 * 0 for a fixed amplitude, NaN when J^T J is singular), rss[n_batch] = sum |x - x^|^2, status[n_batch] (0 converged,
 * 1 iteration cap, 2 non-finite: params, amp_sd and fit_data zero, rss NaN), iters[n_batch]; `fit_data` (may be NULL):
 * [n_batch, n] complex128 model at the solution.  `workspace`: xm_amares_workspace_bytes() bytes of device memory.
 * n_peaks in 1 ... 16, n >= free parameters. */
int64_t xm_amares_workspace_bytes(int64_t n_batch, int n, int n_peaks);
int xm_amares_fit(const void* in, int64_t in_row_stride, int64_t n_batch, int n, double dt, double t0, int n_peaks,
                  const double* init, const double* lower, const double* upper, const int32_t* fixed, int max_iter,
                  double ftol, double xtol, double* params, double* amp_sd, double* rss, int32_t* status,
                  int32_t* iters, void* fit_data, void* workspace, int64_t workspace_bytes, int dtype, void* stream);
/* xm_amares_fit_linked: xm_amares_fit with linked prior knowledge.  Three more HOST arrays of 5 n_peaks values (all
 * NULL: no links): link_to[q] = the root m of parameter q, or -1; then p_q = link_scale[q] p_m + link_offset[q], q
 * shares m's free column (and m's bounds transform; q's own init / lower / upper / fixed are not read), and a q whose
 * root is fixed is fixed at the mapped value.  The free parameters P -- n >= P, amp_sd's J^T J -- are the distinct free
 * columns; amp_sd of a linked amplitude is |link_scale| times its root's.  The root must be the same kind of parameter
 * (m % 5 == q % 5) of another peak and not itself linked (the caller composes chains); link_scale finite and nonzero,
 * link_offset finite: otherwise XM_ERR_INVALID_ARG before any HIP call.  xm_amares_fit is this call without links. */
int xm_amares_fit_linked(const void* in, int64_t in_row_stride, int64_t n_batch, int n, double dt, double t0,
                         int n_peaks, const double* init, const double* lower, const double* upper,
                         const int32_t* fixed, const int32_t* link_to, const double* link_scale,
                         const double* link_offset, int max_iter, double ftol, double xtol, double* params,
                         double* amp_sd, double* rss, int32_t* status, int32_t* iters, void* fit_data, void* workspace,
                         int64_t workspace_bytes, int dtype, void* stream);

/* ---- quantification: basis-set (linear-combination) fitting (this backend's own definition).
 * Model: x^_n = e^{i phi} sum_m a_m B_m[n] exp(-d_g t_n - s_g t_n^2 + i 2 pi f_g t_n), g = group[m], t_n = n dt; the
 * cost is the sum over n >= skip of |x_n - x^_n|^2.  `basis`: device, [n_metab, n] complex128, shared by every row.
 * `group`: HOST array of n_metab indices in 0 ... n_groups - 1, no group empty.  A row has Q = n_metab + 3 n_groups + 1
 * parameters, fp64: a_m at m, then the shifts f_g [Hz], the Lorentzian dampings d_g [1/s], the Gaussian dampings s_g
 * [1/s^2], then phi [rad].
 *
 * xm_basis_model: out[b, j] (complex128) = x^_j for the parameters params[b, :] ([n_batch, Q], device). */
int xm_basis_model(const double* params, int64_t n_batch, const void* basis, int n_metab, const int32_t* group,
                   int n_groups, int n, double dt, void* out, void* stream);
/* xm_basis_fit: one Levenberg-Marquardt fit per row of `in`, iteration, stopping rules and status codes as
 * xm_amares_fit.  HOST arrays of Q values: `init` (clipped into its bounds; NaN for a free amplitude: the automatic
 * start ||x|| / (n_metab ||B_m||), norms over the fitted points, per row), `lower` / `upper` (+-inf: unbounded side,
 * amplitudes and phi only: a free f, d or s needs two finite bounds), `fixed` (nonzero, or lower == upper: held).
 * Outputs (device): params[n_batch, Q] physical, amp_sd[n_batch, n_metab] = sqrt of the amplitude's diagonal entry of
 * (J^T J)^{-1} over the physical free parameters (the caller scales by sigma; 0 for a fixed amplitude, NaN when J^T J
 * is singular), rss, status, iters [n_batch]; `fit_data` (may be NULL): [n_batch, n] complex128 model at the solution,
 * all n points.  Status 2: params, amp_sd and fit_data zero, rss NaN.  `workspace`: xm_basis_workspace_bytes() bytes of
 * device memory whose first 8 bytes are zero between calls (the kernel leaves them so).  XM_ERR_INVALID_ARG before any
 * HIP call, outputs and counters untouched: a group index out of range or an empty group, n_metab < 1, Q > 128, more
 * than 80 free parameters P, n - skip < P, a NaN bound, lower > upper, an infinite bound of a free f, d or s. */
int64_t xm_basis_workspace_bytes(int64_t n_batch, int n, int n_metab);
int xm_basis_fit(const void* in, int64_t in_row_stride, int64_t n_batch, int n, double dt, int skip, const void* basis,
                 int n_metab, const int32_t* group, int n_groups, const double* init, const double* lower,
                 const double* upper, const int32_t* fixed, int max_iter, double ftol, double xtol, double* params,
                 double* amp_sd, double* rss, int32_t* status, int32_t* iters, void* fit_data, void* workspace,
                 int64_t workspace_bytes, int dtype, void* stream);

/* ---- coil combination (this backend's own definition, the reference has none).
 * The data are viewed as (n_outer, C, n_inner, N), C-contiguous: voxel (a, b) holds the C x N matrix X of its FIDs, its
 * coils n_inner N elements apart.  `ref_or_null`: the reference R, (n_outer, C, n_inner, N_R) of the same dtype, or NULL
 * (R = X, N_R must equal N).  `linv_or_null`: L^{-1} of the noise covariance Psi = L L^H, C x C complex128 row-major on
 * the device, or NULL for the identity.  Per voxel: G = L^{-1} (R R^H) L^{-H}; u = the unit eigenvector of G's largest
 * eigenvalue (XM_COIL_SVD; XM_COIL_SVD_FMA, not a user method: the same with the Gram matrix on plain FMAs at every C, the
 * form the tests and the timing script hold the matrix-core form against) or L^{-1} mean(R[:, :n_points]) normalised (XM_COIL_FIRST_POINT); w = L^{-H} u turned
 * so that w^H R[:, 0] >= 0; y = w^H X.  Outputs (device): y (n_outer, n_inner, N) of the input's dtype, w (n_outer,
 * n_inner, C) complex128, quality = u^H G u / trace(G), status: 0 combined; 1 nothing to go by (R all zero, or a zero
 * mean for first_point): y, w, quality zero; 2 a non-finite sample in R or X, or finite
 * samples so large that R R^H or its squared norm overflows fp64: y, w zero, quality NaN; 3 the Jacobi
 * sweep cap was reached (the result is what it had).  All arithmetic fp64.  `workspace`: XM_COIL_WORKSPACE_BYTES of
 * device memory, zero on entry to the first call and left zero by every call.  1 <= C <= 64, N >= 1, N_R >= 1,
 * 1 <= n_points <= N_R, a known method and non-NULL x / y / w / quality / status / workspace: otherwise
 * XM_ERR_INVALID_ARG before any HIP call. */
#define XM_COIL_SVD 0
#define XM_COIL_FIRST_POINT 1
#define XM_COIL_SVD_FMA 2
#define XM_COIL_WORKSPACE_BYTES 256
int xm_coil_combine(const void* x, const void* ref_or_null, void* y, void* w, double* quality, int32_t* status,
                    int64_t n_outer, int C, int64_t n_inner, int N, int N_R, const void* linv_or_null, int method,
                    int n_points, int is_complex128, void* workspace, void* stream);

/* ---- alignment of repeated transients (this backend's own definition, the reference has none).
 * The data are viewed as (n_outer, A, n_inner, N), C-contiguous, time last: transient (o, a, i) starts at
 * ((o A + a) n_inner + i) N.  `r`: the references, N_r points each, the one of voxel v = o n_inner + i at
 * v r_voxel_stride elements (0: one row shared by all voxels), the data's dtype.  With tau_t = t0 + t dt and
 * z_t = r_t conj(x_t), t < L: C(f) = sum_t z_t e^{-2 pi i f tau_t}; g* = the arg-max of |C|^2 on the grid g delta,
 * delta = 1 / (4 L dt), |g| <= G = floor(max_shift / delta) (G = 0 when L < 2), a tie going to the smallest |g|, then to
 * the negative g; f* = the zero of d|C|^2 / df in [(g* - 1) delta, (g* + 1) delta] within +-max_shift (safeguarded
 * Newton, at most 40 steps, until a step <= 2^-40 delta); phi* = arg C(f*); y_t = x_t e^{i (2 pi f* tau_t + phi*)},
 * t < N.  Outputs (device), per transient in the layout (n_outer, A, n_inner): shift = f* (Hz), phase = phi* (rad),
 * quality = |C(f*)| / (||r|| ||x||), status: 0 aligned; 1 |g*| = G and |C|^2 still rises at that end of the window:
 * f* = +-max_shift, unrefined; 2 a non-finite sample among the L points of x or r, or a sum that overflows: y zero,
 * shift, phase, quality NaN; 3 C zero on the whole grid: y = x, shift, phase, quality 0; 4 the step cap was reached
 * (the result is what the iteration had).  `y`: as x, the input's dtype.  Averaging form (`mean_or_null` given): per
 * voxel the mean (n_outer, n_inner, N) of the y with status != 2 and quality >= min_quality, summed in fp64 in
 * ascending a and divided by their number, which goes to `n_averaged_or_null` (int32 per voxel; zero: a zero mean);
 * `y` may then be NULL.  `dtype`: XM_C64 / XM_C128; XM_ALIGN_SKIP_* on top of it leave a stage out (timing only).
 * `workspace`: xm_align_workspace_bytes(...) of device memory, zero on entry to the first call and left zero by
 * every call.  XM_ERR_INVALID_ARG before any HIP call for: a NULL pointer other than the optional ones, L < 1,
 * L > min(N, N_r), L > 8192, 2 G + 1 > 1025, dt <= 0, max_shift < 0, a stride between 1 and N_r - 1, an unknown dtype. */
#define XM_ALIGN_WORKSPACE_BYTES 256
#define XM_ALIGN_SKIP_COARSE 0x100
#define XM_ALIGN_SKIP_REFINE 0x200
#define XM_ALIGN_SKIP_APPLY 0x400
int64_t xm_align_workspace_bytes(int64_t n_outer, int A, int64_t n_inner, int N);
int xm_align_rows(const void* x, const void* r, int64_t r_voxel_stride, void* y, void* mean_or_null, double* shift,
                  double* phase, double* quality, int32_t* status, int32_t* n_averaged_or_null, int64_t n_outer, int A,
                  int64_t n_inner, int N, int N_r, int L, double dt, double t0, double max_shift, double min_quality,
                  int dtype, void* workspace, void* stream);

/* ---- residual-signal (water) removal by HSVD (this backend's own definition, the reference has
 * none).  `x`: n_batch rows of N samples, row_stride elements apart.  Per row, all in fp64: H[l][j] = x[l + j], N - M + 1
 * rows and M columns; G = H^H H; W = conj(U), U the eigenvectors of G's K largest eigenvalues (a tie going to the lower
 * index); Q = (I + w w^H / (1 - ||w||^2)) W[0:M-1]^H W[1:M], w^H the last row of W (the least-squares shift matrix);
 * z_k = eig(Q) (Hessenberg form, shifted QR), f_k = arg(z_k) / (2 pi dt), d_k = -ln|z_k| / dt, sorted by f_k ascending; a
 * minimises sum_{t<N} |x_t - sum_k a_k z_k^t|^2 with z_k^t = exp(t log z_k) per point (normal equations, Cholesky);
 * y_t = x_t - sum of a_k z_k^t over the k with f_lo <= f_k <= f_hi, rounded once to the input's dtype.  Outputs
 * (device): y (n_batch, N) of the input's dtype, or NULL for the components alone; freq (Hz), damp (1/s), amp = |a_k|,
 * phase = arg a_k (rad), removed (0 / 1), each (n_batch, K); n_removed and status per row: 0 done; 1 no pole in the band
 * (y = x bitwise), or x all zero (y = x, components NaN); 2 a non-finite sample, or samples so large that G or its squared
 * norm overflows: y zero, components NaN; 3 the Jacobi sweep cap (30) or the QR iteration cap (30 K) was reached: y = x,
 * components NaN; 4 1 - ||w||^2 <= 0, a pole that is zero or not finite, a z_k^t that is not finite, or a pivot of the
 * amplitude system that is not positive and finite: y = x, components NaN.  `dtype`: XM_C64 / XM_C128;
 * XM_HSVD_GRAM_FMA on top of it forms G on plain FMAs instead of the matrix cores (not a user option: what the tests and
 * the timing script hold the matrix-core form against); XM_HSVD_STOP_* end every row after the named stage (timing
 * only: status 0, components NaN, y untouched).  `workspace`: XM_HSVD_WORKSPACE_BYTES of device memory, zero on entry to
 * the first call and left zero by every call.  2 <= M <= 64, 1 <= K <= min(M - 1, 32), 2 M <= N <= 16384,
 * row_stride >= N, dt > 0, finite f_lo <= f_hi, a known dtype and non-NULL pointers other than y: otherwise
 * XM_ERR_INVALID_ARG before any HIP call. */
#define XM_HSVD_WORKSPACE_BYTES 256
#define XM_HSVD_GRAM_FMA 0x100
#define XM_HSVD_STOP_GRAM 0x200
#define XM_HSVD_STOP_EIG 0x400
#define XM_HSVD_STOP_POLES 0x600
#define XM_HSVD_STOP_AMPL 0x800
int xm_hsvd_rows(const void* x, int64_t row_stride, void* y_or_null, double* freq, double* damp, double* amp,
                 double* phase, int32_t* removed, int32_t* n_removed, int32_t* status, int64_t n_batch, int N, int M,
                 int K, double dt, double f_lo, double f_hi, int dtype, void* workspace, void* stream);

/* ---- Marchenko-Pastur patch PCA denoising (this backend's own definition, the reference has
 * none).  The data are viewed as (n_outer, s1, s2, s3, N), C-contiguous, time last; a patch dim that is not used has size
 * and patch size 1.  Per voxel i = (i1, i2, i3), all in fp64: the window starts at o_a = min(max(i_a - p_a / 2, 0),
 * s_a - p_a) in every patch dim (integer division; always full, shifted inward at an edge); X = the P x N matrix of the
 * window's FIDs, P = p1 p2 p3, rows in row-major order of the window offsets, c the row that is voxel i; G = X X^H;
 * lambda_k = max(eig_k, 0) / N descending (a tie going to the lower index), U the matching eigenvectors.  Rank r: `rank`
 * when it is >= 0; with rank = -1 the first p in 0 ... P - 1 with (lambda_p - lambda_{P-1}) / (4 sqrt((P - p) / N)) <
 * (sum_{i>=p} lambda_i) / (P - p), the sum accumulated from i = P - 1 downwards, and P when no p qualifies.
 * w_j = sum_{k<r} U[c][k] conj(U[j][k]); y_i[t] = sum_j w_j X[j][t] in ascending j, rounded once to the input's dtype;
 * only voxel i's own row is written.  Outputs (device): y as x (must not be x: the windows overlap); rank_out (int32),
 * sigma = sqrt(mean(lambda_r ... lambda_{P-1})) (0 when r = P; the standard deviation of the complex noise) and status
 * per voxel: 0 done; 1 the window is all zero: y zero, rank 0, sigma 0; 2 a non-finite sample in the window, or samples
 * so large that G or its squared norm overflows: y zero, rank 0, sigma NaN; 3 the Jacobi sweep cap (30) was reached:
 * y = x for this voxel, rank 0, sigma NaN.  `dtype`: XM_C64 / XM_C128; XM_DENOISE_GRAM_FMA on top of it forms G on plain
 * FMAs at every P instead of the matrix cores (P >= 8; not a user option: what the tests and the timing script hold the
 * matrix-core form against); XM_DENOISE_STOP_* end every voxel after the named stage (timing only: status 0, y
 * untouched).  `workspace`: XM_DENOISE_WORKSPACE_BYTES of device memory, zero on entry to the first call and left zero
 * by every call.  1 <= p_a <= s_a, 2 <= P <= 64, P <= N <= 16384, -1 <= rank <= P, n_outer >= 0, at most 2^32 - 1
 * voxels, a known dtype, non-NULL pointers and y != x: otherwise XM_ERR_INVALID_ARG before any HIP call. */
#define XM_DENOISE_WORKSPACE_BYTES 256
#define XM_DENOISE_GRAM_FMA 0x100
#define XM_DENOISE_STOP_GRAM 0x200
#define XM_DENOISE_STOP_EIG 0x400
int xm_denoise_patches(const void* x, void* y, int32_t* rank_out, double* sigma, int32_t* status, int64_t n_outer, int s1,
                       int s2, int s3, int p1, int p2, int p3, int N, int rank, int dtype, void* workspace, void* stream);

/* ---- MRSI spatial reconstruction: a small dense matrix along one axis (this backend's own
 * definition, the reference has none beyond zero_fill + ifftc).  x is viewed as (n_outer, n, n_inner) and y as (n_outer,
 * m, n_inner), both C-contiguous: any axis of a contiguous tensor is such a view, so nothing is transposed.  `table`:
 * m x n complex128, row-major, in device memory.  y[o][p][i] = sum_j table[p][j] x[o][j][i], the products and the sum in
 * fp64 (ascending j, every step a fused multiply-add), rounded once to `dtype` (XM_C64 / XM_C128).  The kernel applies a
 * general matrix: filter, zero fill, voxel shift, the centring rolls and the ortho scale of to_image / to_kspace are all
 * in the table the host builds.  A pencil (o, i) depends on its own n samples only.  1 <= n, m <= 64, n_outer, n_inner
 * >= 0, at most 2^50 pencils, non-NULL pointers, y != x and a known dtype: otherwise XM_ERR_INVALID_ARG before any HIP
 * call.  n_outer = 0 or n_inner = 0 launches nothing. */
int xm_axis_dft(const void* x, void* y, const void* table, int64_t n_outer, int n, int m, int64_t n_inner, int dtype,
                void* stream);

/* ---- SENSE unfolding of regularly undersampled MRSI (this backend's own definition, the reference
 * has none).  `a`: the aliased reduced-FOV images of C coils, n[0] x n[1] x n[2] voxels (an unused dim has n = accel = 1)
 * and N_t time points; `a_strides`: element strides of its outer, coil and three spatial axes, `y_strides`: of the outer
 * and three spatial axes of `y`, which holds N_d = accel[d] n[d] voxels per dim; time is contiguous and last in both.
 * `sens`: [C, N_0, N_1, N_2] complex128, contiguous; `linv_or_null`: L^-1 of the noise covariance L L^H, C x C complex128
 * row-major, or NULL for the identity.  The group of the reduced voxel p holds the R = accel[0] accel[1] accel[2] voxels
 * q_d = (p_d - n[d] / 2 + N_d / 2 + k_d n[d]) mod N_d, member k = (k_0 accel[1] + k_1) accel[2] + k_2.  Its active members
 * are those whose sensitivity is not zero in every coil; S = their C x Ra columns, Sw = Linv S, A = Sw^H Sw,
 * lambda' = regularization trace(A) / Ra, B = (A + lambda' I)^-1 Sw^H by Cholesky, U = sqrt(R) B Linv;
 * y[q_k, t] = sum_c U[k][c] a_c[p, t] in ascending c, every step a fused multiply-add in fp64, rounded once to `dtype`
 * (XM_C64 / XM_C128); g[q_k] = sqrt((B B^H)_kk A_kk).  `g_or_null` (fp64) and `status_or_null` (int32): [n_outer, N_0,
 * N_1, N_2], per full-FOV voxel: 0 unfolded; 1 a masked member (y zero, g 0), also every member of a group without an
 * active one; 2 a non-finite sensitivity or data sample in the group, 3 a Cholesky pivot <= 0 or non-finite, and always Ra > C at regularization 0 (2 wins over 3): y zero and
 * g NaN for every member of the group.  A group depends on its own samples only.  `workspace`:
 * XM_SENSE_WORKSPACE_BYTES of device memory, zero on entry to the first call and left zero by every call.  Non-NULL
 * pointers (g and status may be NULL), 1 <= C <= 64, accel >= 1, R <= 16, n >= 1, N_t >= 1, n_outer >= 0, at most
 * 2^32 - 1 groups, a finite regularization >= 0, a known dtype and y != a: otherwise XM_ERR_INVALID_ARG before any HIP
 * call.  n_outer = 0 launches nothing. */
#define XM_SENSE_WORKSPACE_BYTES 256
int xm_sense_unfold(const void* a, void* y, const void* sens, const void* linv_or_null, double* g_or_null,
                    int32_t* status_or_null, int64_t n_outer, int C, const int32_t n[3], const int32_t accel[3], int N_t,
                    const int64_t a_strides[5], const int64_t y_strides[4], double regularization, int dtype,
                    void* workspace, void* stream);

/* ---- GRAPPA fill of regularly undersampled Cartesian MRSI (this backend's own definition, the
 * reference has none).  `a`: the kept k-space lines of C coils, n[0] x n[1] x n[2] lines (an unused dim has n = accel =
 * kernel = 1) and N_t time points; `y`: the full grid, N_d = accel[d] n[d] lines per dim, the dtype of `a`.  `a_strides`,
 * `y_strides`: element strides of the outer axis, the coil axis and the three spatial axes; time is contiguous and last
 * in both.  Per dim the kept lines of the full centred k-space are j = j0 + accel l, j0 = N / 2 - accel (n / 2).  A full
 * position j has l = floor((j - j0) / accel) (-1 below j0) and o = (j - j0) mod accel >= 0 per dim.  o = 0 in every dim:
 * the position is acquired and copied bit for bit.  Any other offset tuple is a type tau = ((o_0 accel[1] + o_1)
 * accel[2] + o_2) - 1, and with b = kernel, S = b_0 b_1 b_2,
 *   y[c, j, t] = sum_s sum_c' W[tau][c][s][c'] a[c', l + s, t],   s_d = -((b_d - 1) / 2) ... b_d / 2,
 * s row-major over (s_0, s_1, s_2); a neighbour outside 0 ... n_d - 1 is skipped.  The sum runs in ascending s, then
 * ascending c', in fp64, every step a fused multiply-add (complex64 samples are widened on load), and is rounded once to
 * `dtype` (XM_C64 / XM_C128).  `weights`: [R - 1][C][S][C] complex128, contiguous, in device memory, R = accel[0]
 * accel[1] accel[2]; NULL only when R = 1 (the call is then a copy).  One launch of a plain grid writes every element
 * of y exactly once; an output depends on its own sources only, so results are bitwise independent of the batch and of
 * the layout, and a non-finite sample reaches exactly the outputs whose source set holds it.  Non-NULL pointers,
 * 1 <= C <= 64, accel >= 1, R <= 16, kernel >= 1, S <= 64, C S <= 1024, n >= 1, N_t >= 1, n_outer >= 0, y != a, a known
 * dtype, and at most 2^31 - 2^16 work items (n_outer x positions x coil blocks x time tiles): otherwise
 * XM_ERR_INVALID_ARG before any HIP call, with nothing written.  n_outer = 0 launches nothing. */
int xm_grappa_fill(const void* a, void* y, const void* weights, int64_t n_outer, int C, const int32_t n[3],
                   const int32_t accel[3], const int32_t kernel[3], int N_t, const int64_t a_strides[5],
                   const int64_t y_strides[5], int dtype, void* stream);

/* ---- Non-Cartesian gridding: a sparse real matrix along one axis (this backend's own definition,
 * the reference has none).  x is viewed as (n_outer, n, n_inner) and y as (n_outer, n_rows, n_inner), both C-contiguous:
 * any axis of a contiguous tensor is such a view, so nothing is transposed.  The matrix is in CSR form in device memory:
 * `rowptr` (n_rows + 1 int32, ascending from 0), `col` (rowptr[n_rows] int32, each in [0, n)) and `val` (as many fp64).
 *   y[o][r][i] = sum_{e = rowptr[r]}^{rowptr[r+1]-1} val[e] x[o][col[e]][i],
 * the products and the sum in fp64 (ascending e, every step a fused multiply-add), rounded once to `dtype` (XM_C64 /
 * XM_C128); a row without entries is written as zero.  No atomics: an output is one wave's sum in one fixed order and
 * depends on its own entries only, so results are bitwise reproducible and independent of the batch.  The kernel trusts
 * the table: the caller has checked it (xmris_amd.device.SparseTable does so on the host; a column out of range would
 * read out of bounds); the entry count is bounded by rowptr's int32.  1 <= n, n_rows < 2^31, n_outer, n_inner >= 0, at
 * most 2^50 elements in x or y, non-NULL pointers aligned to the element size, y != x and a known dtype: otherwise
 * XM_ERR_INVALID_ARG before any HIP call.  n_outer = 0 or n_inner = 0 launches nothing. */
int xm_axis_sparse(const void* x, void* y, const int32_t* rowptr, const int32_t* col, const double* val, int64_t n_outer,
                   int64_t n, int64_t n_rows, int64_t n_inner, int dtype, void* stream);

/* ---- CG-SENSE: the image-sized half of a conjugate-gradient step (this backend's own definition,
 * the reference has none).  V = n_vox voxels, T = n_cols independent columns, C = n_coils; all arrays C-contiguous in
 * device memory: x, r, p, q [V, T] complex128; s [C, V] complex128; u [C, V, T] of `dtype` (XM_C64 / XM_C128), the coil
 * images that enter or leave a NUFFT chain.  A sum over voxels is kept as partials [NB, T] fp64, NB = ceil(V /
 * XM_CGS_VOXELS): partial [b, t] is the sum over the voxels of block b in ascending v, and a total is the sum of the NB
 * partials of a column in ascending b.  Every product-sum is a fused multiply-add in fp64; u rounds once to `dtype`.
 *   xm_cgs_expand: for a column with status[t] == 0, p <- r + (rho_new / rho_old) p (the totals of the two partial
 *     arrays; `first` != 0: p <- r and the partials are not read, though the pointers must be valid); then for every column u[c, v, t] = s[c, v] p[v, t].
 *   xm_cgs_reduce: q[v, t] = sum_c conj(s[c, v]) u[c, v, t] (ascending c) + lambda p[v, t], part[b, t] = sum_v Re(conj(p) q).
 *     `initial` != 0: no lambda term, p is not read (may be NULL) and part[b, t] = sum_v |q|^2: q is then b = E^H D y.
 *   xm_cgs_step: for a column with status_in[t] == 0, in this order: the total of rho0 not finite -> status 3 and
 *     x[:, t] = NaN; the total of rho <= max(tol, 1e-14)^2 x that of rho0 -> status 1; `final_test` != 0 -> status stays
 *     0; the total of delta not > 0 or not finite -> status 2; otherwise alpha = rho / delta, x += alpha p, r -= alpha q,
 *     rho_out[b, t] = sum_v |r|^2, n_iter[t] = iteration.  status_out[t] is written for every column; residual[t] =
 *     sqrt(rho / rho0) (0 for rho0 = 0, NaN with status 3) for a column that leaves status 0 in this call, and in a final test for one that
 *     stays 0.  A column with status_in[t] != 0 is not touched.  With `final_test`, delta is not read (may be NULL).
 * No call reads a per-column value that the same call writes (the caller alternates two buffers for the partials of rho
 * and for status), there are no atomics, and a column depends on its own values only: results are bitwise independent of
 * the other columns of the call.  All sizes in 1 ... 2^31 - 1, at most 2^50 elements in u, non-NULL pointers aligned to
 * their element size, no output equal to an input or to another output, a known dtype, a finite lambda and tol >= 0 and
 * iteration >= 0: otherwise XM_ERR_INVALID_ARG before any HIP call. */
#define XM_CGS_VOXELS 16
int xm_cgs_expand(const void* r, void* p, const void* s, void* u, const double* rho_new, const double* rho_old,
                  const int32_t* status, int64_t n_coils, int64_t n_vox, int64_t n_cols, int first, int dtype,
                  void* stream);
int xm_cgs_reduce(const void* u, const void* s, const void* p, void* q, double* part, int64_t n_coils, int64_t n_vox,
                  int64_t n_cols, double lambda, int initial, int dtype, void* stream);
int xm_cgs_step(void* x, void* r, const void* p, const void* q, const double* rho, const double* rho0,
                const double* delta, double* rho_out, const int32_t* status_in, int32_t* status_out, int32_t* n_iter,
                double* residual, int64_t n_vox, int64_t n_cols, double tol, int iteration, int final_test, void* stream);

/* ---- Wavelet-sparse SENSE: the image-sized half of a proximal-gradient (FISTA) step (this
 * backend's own definition, the reference has none).  The image has n_dims <= 3 dims of m_0 x m_1 x m_2 voxels in C order
 * (a dim beyond n_dims: size 1, level 0, shift 0), V their product, and T = n_cols independent columns; x, v, q, b [V, T]
 * complex128, mask [V] bytes, all C-contiguous in device memory.  The image is cut into blocks of 2^l_d voxels per dim,
 * B = 2^(l_0 + l_1 + l_2) <= 16, on a lattice moved by the shift s_d (0 <= s_d < 2^l_d) with periodic wrap: block
 * (n_0, n_1, n_2) holds the voxels ((n_d << l_d) + i_d + s_d) mod m_d; NBL = V / B blocks, numbered in C order.  Each
 * block is transformed by the orthonormal decimated Haar transform of l_d levels per dim: dims ascending, levels fine to
 * coarse, every butterfly (a + b) r, (a - b) r with r = 1 / sqrt(2).  A sum over voxels is kept as partials [NBL, T] fp64
 * (per block in ascending in-block index i_0 + (i_1 << l_0) + (i_2 << (l_0 + l_1))), a total is the sum of a column's
 * partials in ascending block order.
 *   xm_l1_start, finish == 0: bpart[r, t] = max |b[v, t]|^2 over the 16 consecutive voxels of run r (bpart: [ceil(V / 16),
 *     T] fp64; the other pointers are not used and may be NULL).  finish != 0: bmax[t] = sqrt(max_r bpart[r, t]) and
 *     status[t] = 0; where that maximum is not finite, status[t] = 3, bmax[t] = change[t] = NaN and x[:, t] = NaN (b is not
 *     used and may be NULL).
 *   xm_l1_prox, for a column with status_in[t] == 0.  Unless mode == 1, first the test on the totals d2, n2 of d2_in and
 *     n2_in: either not finite -> status 3 and x[:, t] = NaN; d2 <= tol^2 n2 -> status 1; mode == 2 (final test) -> status
 *     stays 0 and nothing else happens.  Otherwise the step:  w = v - tau (q - b)  (mode == 1, the first step: q is taken
 *     as 0 and, like d2_in and n2_in, may be NULL),  c = Haar(w),  every coefficient but the one at in-block index 0 (with
 *     B = 1: every coefficient) becomes c max(0, 1 - theta / |c|) with theta = theta_scale bmax[t],  x' = mask ? Haar^-1(c)
 *     : 0,  v <- x' + beta (x' - x),  x <- x',  d2_out[n, t] = sum |x' - x|^2 and n2_out[n, t] = sum |x'|^2 over block n,
 *     n_iter[t] = iteration.  status_out[t] is written for every column; change[t] = sqrt(d2 / n2) (0 for d2 = 0, NaN
 *     with status 3) for a column that leaves status 0 in this call, and in a final test for one that stays 0.  A column
 *     with status_in[t] != 0 is not touched.
 * No call reads a per-column value that the same call writes (the caller alternates two buffers for the partials and for
 * status), there are no atomics, and a column depends on its own values only: results are bitwise independent of the
 * other columns of the call.  n_dims in 1 ... 3, every m_d, V and T in 1 ... 2^31 - 1, at most 2^50 elements, m_d divisible
 * by 2^l_d, B <= 16, a shift inside its block, tau, theta_scale, beta and tol finite and >= 0, iteration >= 0, mode in
 * 0 ... 2, non-NULL pointers aligned to their element size, no output equal to an input or to another output: otherwise
 * XM_ERR_INVALID_ARG before any HIP call. */
int xm_l1_start(const void* b, double* bpart, double* bmax, int32_t* status, double* change, void* x, int64_t n_vox,
                int64_t n_cols, int finish, void* stream);
int xm_l1_prox(void* x, void* v, const void* q, const void* b, const uint8_t* mask, const double* bmax,
               const double* d2_in, const double* n2_in, double* d2_out, double* n2_out, const int32_t* status_in,
               int32_t* status_out, int32_t* n_iter, double* change, int n_dims, int64_t m0, int64_t m1, int64_t m2, int l0,
               int l1, int l2, int s0, int s1, int s2, int64_t n_cols, double tau, double theta_scale, double beta, double tol,
               int iteration, int mode, void* stream);

/* ---- ESPIRiT: per-voxel eigen-decomposition of a coil x coil Hermitian matrix (this backend's own
 * definition, the reference has none).  h: [n_vox, E] complex128, E = C (C + 1) / 2, C = n_coils: per voxel the upper
 * triangle (i <= j) of its matrix in row-major order; the lower triangle is the conjugate and the imaginary part of the
 * diagonal is ignored.  One launch of k_espirit_eig, one 256-thread workgroup per voxel, parallel cyclic Jacobi in fp64.
 * For m < n_maps the m-th largest eigenvalue (a tie goes to the lower column of the Jacobi result) goes to values[m, v]
 * and its eigenvector to maps[m, :, v] (maps: [n_maps, C, n_vox] complex128; values: [n_maps, n_vox] fp64), of unit norm
 * and multiplied by the phase that makes component `phase_ref` real and >= 0 (left as it is when that component is
 * exactly 0).  A map whose eigenvalue is < crop is written as exact zeros.  status[v] (int32): 0 ok; 1 the sweep cap was
 * reached, the outputs are those of the last sweep; 2 a non-finite entry (or finite ones whose norm overflows): maps 0,
 * values NaN.  A zero matrix has status 0 and eigenvalue 0.  No atomics, no voxel reads another's data and every sum has
 * a fixed order: a voxel's outputs are bitwise independent of n_vox and of its place in the batch.  n_coils in 1 ... 64,
 * n_maps in 1 ... min(2, n_coils), n_vox in 1 ... 2^31 - 1, phase_ref in 0 ... n_coils - 1, a finite crop, non-NULL
 * pointers aligned to their element size, no output equal to the input or to another output: otherwise
 * XM_ERR_INVALID_ARG before any HIP call. */
int xm_espirit_eig(const void* h, void* maps, double* values, int32_t* status, int64_t n_vox, int n_coils, int n_maps,
                   int phase_ref, double crop, void* stream);

/* ---- Per-row time shift of FIDs (this backend's own definition, the reference has none).
 * `in`: n_rows rows of n points, `in_row_stride` elements apart; `out`: n_rows contiguous rows of n points.  Row r is
 * delayed by phi = frac[(r / delay_div) % n_delay] dwells (`frac`: n_delay fp64 in device memory):
 *   X[k] = sum_{j<n} in[r][j] e^{-2 pi i k j / L},  out[r][j] = (1/L) sum_{k<L} X[k] e^{-2 pi i kappa_k phi / L} e^{+2 pi i k j / L},
 * kappa_k = k for k < L/2 and k - L from there on (numpy.fft.fftfreq(L) L; the Nyquist bin is -L/2).  One launch of
 * k_shift_time: load, transform, ramp, transform back, store.  The ramp is formed in fp64 with kappa_k phi / L reduced
 * modulo 1 on the integer part of phi and rounded once to `dtype` (XM_C64 / XM_C128); the transforms run in `dtype`.
 * A row depends on its own samples and delay only, and a zero delay takes the same arithmetic as any other.
 * xm_shift_time_fused(L, dtype) is 1 for the lengths that have the kernel -- the direct in-LDS plans; 16384 in
 * complex64 only -- and 0 otherwise: callers compose those from xm_zero_fill, xm_fft1d_batched and a phase product.
 * 1 <= n <= L, L in the fused set, n_rows >= 0 (at most 2^31 - 1), in_row_stride >= n, n_delay >= 1, delay_div >= 1,
 * non-NULL pointers aligned to their element size, out != in and a known dtype: otherwise XM_ERR_INVALID_ARG before
 * any HIP call, and nothing is written.  n_rows = 0 launches nothing. */
int xm_shift_time_fused(int L, int dtype);
int xm_shift_time(const void* in, int64_t in_row_stride, void* out, int64_t n_rows, int n, int L, const double* frac,
                  int64_t n_delay, int64_t delay_div, int dtype, void* stream);

/* ---- Per-voxel rate fitting of a dynamic series (this backend's own definition, the reference
 * has none).  One substrate and M = n_products products over T = n_times repetitions at times[T] (HOST, seconds,
 * increasing), flip angles flip_s[T] and flip_p[M, T] (HOST, radians, inside (0, pi / 2)).  Device arrays, fp64:
 * substrate [n_batch, T], products and weights [n_batch, M, T] (weights NULL: all 1; a point of weight 0 is missing
 * and its sample is not read).  Each (voxel, product) pair is one fit of k [1/s], rho [1/s] and z:
 *   Zs_n = S_n / sin flip_s[n],  Zs+_n = Zs_n cos flip_s[n],  D_n = times[n+1] - times[n],  x = rho D_n
 *   Z_0 = z,  Z_{n+1} = e^{-x} cos flip_p[m, n] Z_n + k (w0_n Zs+_n + w1_n Zs_{n+1}),
 *   w1_n = D_n (x - 1 + e^{-x}) / x^2,  w0_n = D_n (1 - e^{-x}) / x - w1_n,  P^_n = Z_n sin flip_p[m, n],
 *   cost = sum_n weights[n]^2 (P_n - P^_n)^2,
 * by Levenberg-Marquardt in lmfit's bound variables, the iteration and the stopping rules of xm_basis_fit, one wave
 * per fit (k_kinetics_fit).  init / lower / upper / fixed: HOST [M, 3] in the order k, rho, z, shared by the batch; a
 * parameter is fixed when flagged or when lower == upper.  A free k or rho needs two finite bounds; z any.  A NaN
 * init of a free z starts it per fit at |P_j| / sin flip_p[m, j], j the first repetition of positive weight.
 * Outputs: params and param_sd [n_batch, M, 3]; rss, status, iters, auc_ratio [n_batch, M]; fit [n_batch, M, T] (the
 * model at every repetition; may be NULL).  status: 0 converged, 1 iteration cap, 2 non-finite, 3 fewer points of
 * positive weight (T_w) than free parameters (P); for 2 and 3 every output of the fit is 0 and rss is NaN.
 * param_sd: sqrt(diag((J^T W J)^{-1}) rss / (T_w - P)) over the physical free parameters, 0 for a fixed one, NaN when
 * the matrix is singular or T_w = P.  auc_ratio: the trapezoid area over `times` of P_m divided by that of S, both over
 * the points of positive weight.
 * XM_ERR_INVALID_ARG before any HIP call, nothing written: T outside 2 ... 256, M outside 1 ... 8, n_batch < 0, times
 * not finite or not increasing, a flip angle outside (0, pi / 2), a NaN bound or lower > upper, an infinite bound of a
 * free k or rho, a negative lower bound of rho, a non-finite init (but the NaN of z), every parameter of a product
 * fixed, max_iter < 1, a negative or NaN tolerance, a null pointer (but weights and fit).  n_batch = 0 returns 0. */
int xm_kinetics_fit(const double* substrate, const double* products, const double* weights, int64_t n_batch,
                    int n_products, int n_times, const double* times, const double* flip_s, const double* flip_p,
                    const double* init, const double* lower, const double* upper, const int32_t* fixed, int max_iter,
                    double ftol, double xtol, double* params, double* param_sd, double* rss, int32_t* status,
                    int32_t* iters, double* fit, double* auc_ratio, void* stream);

/* ---- Multi-echo chemical-species separation (this backend's own definition, the reference has
 * none).  A row (a k-space sample or a voxel) has E = n_echoes echoes at t_e = TE_e + tau_r and columns (coils) that
 * share its readout delay tau_r [s] and field offset psi_r [Hz]; M = n_species species of frequency f_m [Hz] and decay
 * R_m [1/s]:  y[e, c] = sum_m rho[m, c] e^{(2 pi i f_m - R_m) t_e} e^{2 pi i psi_r t_e}.  One launch of k_species writes
 *   rho[m, c] = e^{-(2 pi i f_m - R_m) tau_r} sum_e P0[m, e] e^{-2 pi i psi_r t_e} y[e, c],   P0 = pinv(A0),
 *   A0[e, m] = e^{(2 pi i f_m - R_m) TE_e}, all arithmetic fp64, the result rounded once to `dtype`.
 * The data are addressed where they lie.  `dims` (HOST, 4): sizes of the outer and inner row level and of the outer
 * and inner column level (>= 1; a level that is not needed has size 1).  `x_strides`, `y_strides` (HOST, 5): strides
 * in elements of these four levels and of the echo (in y: the species) level.  `tau`, `psi`: fp64 device arrays read at
 * r0 s0 + r1 s1 with the strides given (0 repeats a value), or NULL for 0.  Lanes run along the inner row level.
 * `tables` (device, fp64): TE[E], f[M], R[M], P0[M][E] as (re, im); with `fit` also Pi[e][e] (E values) and Pi[e'][e] as
 * (re, im) for the pairs e < e' in ascending order (e, e'), Pi = Q Q^H the projector onto range(A0).
 * fit != 0: psi is not read; per row psi* maximises G(psi) = sum_e W[e, e] + 2 sum_{e<e'} Re(W[e, e'] e^{2 pi i psi
 * (TE_e' - TE_e)}), W[e, e'] = Pi[e', e] sum_c y[e, c] conj(y[e', c]): the arg-max on the grid g delta, |g| <= G =
 * floor(max_field / delta), delta = 1 / (4 span), span = max TE - min TE (HOST argument), a tie to the smaller |g|,
 * then to the negative g; then the zero of G' in [(g* - 1) delta, (g* + 1) delta] within +-max_field by the
 * safeguarded Newton iteration of xm_align_rows (step <= 2^-40 delta, or 40 steps).
 * Outputs per row (nr0, nr1 contiguous): field (psi* or the given psi), residual (fit only, max(0, 1 - G(psi*) /
 * sum |y|^2); may be NULL otherwise and is then not written), status: 0 done; 1 |g*| = G > 0 and G still rises at that
 * end of the window (psi* is the end, unrefined); 2 a non-finite sample, tau or psi (species 0, field and residual
 * NaN); 3 an all-zero row (psi* = 0 with fit, species 0, residual 0); 4 the step cap.  A row's outputs depend on its own
 * samples and the scalar arguments only, bit for bit.
 * `dtype`: XM_C64 / XM_C128; XM_SPECIES_SKIP_* on top of it leave a stage out (timing only).
 * XM_ERR_INVALID_ARG before any HIP call, nothing written: E outside 2 ... 32 (2 ... 16 with fit), M outside 1 ... 8,
 * M > E (M >= E with fit), a size < 1 (the row sizes may be 0: nothing is launched), more than 2^31 - 1 tiles of 64
 * rows, a null pointer (but tau, psi, and residual without fit), with fit a max_field or span that is not finite and
 * positive or a grid 2 G + 1 > 1025, an unknown dtype. */
#define XM_SPECIES_SKIP_GRAM 0x100
#define XM_SPECIES_SKIP_COARSE 0x200
#define XM_SPECIES_SKIP_REFINE 0x400
#define XM_SPECIES_SKIP_APPLY 0x800
int xm_species_separate(const void* x, void* y, const int64_t* dims, const int64_t* x_strides, const int64_t* y_strides,
                        int n_echoes, int n_species, const double* tables, const double* tau, int64_t tau_s0,
                        int64_t tau_s1, const double* psi, int64_t psi_s0, int64_t psi_s1, double* field,
                        double* residual, int32_t* status, int fit, double max_field, double span, int dtype,
                        void* stream);

/* ---- Lipid-subspace (L2) suppression of 1H MRSI (this backend's own definition, the reference
 * has none).  A row is one FID of T samples, time stride 1, rows `x_row_stride` / `y_row_stride` elements apart.  With
 * the orthonormal vectors u_k (k < rank) of the lipid subspace and the weights w_k, one launch of k_lipid_project writes
 *   y[t] = x[t] - sum_k u_k[t] w_k c_k,   c_k = sum_t conj(u_k[t]) x[t],
 * for every row, all arithmetic fp64, every sum in one defined order, the result rounded once to `dtype`.
 * `tables` (device, fp64, 16-byte aligned): U[T][rank] as (re, im), then w[rank].  `apply`: a device byte per row, or
 * NULL for every row; a row whose byte is 0 is copied bit for bit.  `status` (device, one int32 per row): 0 done, 1
 * copied (apply 0), 2 a non-finite sample (the row's output is NaN; no other row is touched).  A row's output depends
 * on its own samples and the tables only, bit for bit: not on the batch, its place in a tile of 16 rows, or the strides.
 * x == y with equal strides is allowed (a workgroup writes only the rows it alone reads); any other overlap is refused.
 * `dtype`: XM_C64 / XM_C128; on top of it XM_LIPID_FMA selects the plain-FMA form of both stages (default: the fp64
 * matrix cores), XM_LIPID_SKIP_COEF / XM_LIPID_SKIP_APPLY leave a stage out (timing only).
 * XM_ERR_INVALID_ARG before any HIP call, nothing written: T outside 2 ... 65536, rank outside 1 ... 64, n_rows < 0 or
 * more than 2^31 - 1 tiles of 16 rows, a null x, y, tables or status, a row stride < T, tables not 16-byte aligned, x or
 * y not aligned to an element, overlapping x and y, an unknown dtype.  n_rows == 0 (with T, rank and dtype in range) returns 0 without a launch,
 * whatever the pointers hold. */
#define XM_LIPID_FMA 0x100
#define XM_LIPID_SKIP_COEF 0x200
#define XM_LIPID_SKIP_APPLY 0x400
int xm_lipid_project(const void* x, void* y, int64_t n_rows, int64_t x_row_stride, int64_t y_row_stride, int T, int rank,
                     const double* tables, const uint8_t* apply, int32_t* status, int dtype, void* stream);

/* ---- Temporal-subspace SENSE (this backend's own definition, the reference has none).  With the
 * basis V [rank, n_time] complex128 (rows need not be orthonormal), rank <= XM_SUB_MAX_RANK, three kernels around the
 * xm_cgs_* iteration and the NUFFT chains:
 *   xm_sub_project  b[c, s, r, f] = sum_t m[s, t] conj(V[r, t]) y[c, s, f, t]    (k_sub_project: the one pass over y)
 *   xm_sub_mix      z[c, s, r, f] = sum_r' K[s, r, r'] a[c, s, r', f]            (k_sub_mix; z == a is allowed)
 *   xm_sub_expand   x[v, f, t]    = sum_r U[v, r, f] V[r, t]                      (k_sub_expand; x complex128)
 * y is addressed where it lies: element (c, s, f, t) at y + c coil_stride + s sample_stride + f frame_stride + t (in
 * elements; the time stride is 1).  b, a, z: [C, S, rank, F] contiguous in `dtype`; `sampling`: a device byte per
 * (s, t), [S, T] contiguous, or NULL for all ones -- a position whose byte is 0 is selected out, whatever y holds there
 * (NaN included) reaches no output.  K: [S, rank, rank] complex128; U: [V, rank, F] complex128.  All arithmetic fp64 in
 * spelt-out FMAs, every sum one chain in ascending t / r' / r from zero, rounded once to the output dtype; no atomics.
 * An output depends on its own inputs only, bit for bit: not on the batch, its place in a tile, F or the strides.
 * XM_ERR_INVALID_ARG before any HIP call, nothing written: an unknown dtype, rank outside 1 ... 32 or (project, expand)
 * above n_time, a size outside 1 ... 2^31 - 1, more than 2^50 elements (for y: reached through the strides), a null y, b,
 * basis, a, z, kernel, u or x, a negative stride, a pointer not aligned to its element (the complex128 tables: 16
 * bytes), an output that overlaps an input (other than z == a). */
#define XM_SUB_MAX_RANK 32
int xm_sub_project(const void* y, void* b, const void* basis, const uint8_t* sampling, int64_t n_coils, int64_t n_samples,
                   int64_t n_frames, int64_t n_time, int rank, int64_t coil_stride, int64_t sample_stride,
                   int64_t frame_stride, int dtype, void* stream);
int xm_sub_mix(const void* a, void* z, const void* kernel, int64_t n_coils, int64_t n_samples, int64_t n_frames, int rank,
               int dtype, void* stream);
int xm_sub_expand(const void* u, const void* basis, void* x, int64_t n_vox, int64_t n_frames, int64_t n_time, int rank,
                  void* stream);

/* ---- A7  host-side autophase search (no GPU involved; O(1) per dataset) ------------------------
 * Objectives of processing/phasing.py:100-157 and the differential-evolution driver the reference
 * reaches through scipy (phasing.py:276-284: best1bin, tol, seed, bounds p0 in [-180,180] deg,
 * p1 in [-4000,4000] deg).  `slice_re_im`: n interleaved complex128 samples of the ONE spectrum through the
 * global maximum; `coords`: its n float64 coordinates; method 0 = acme, 1 = peak_minima, 2 = positivity. */
void* xm_solver_create(const double* slice_re_im, const double* coords, int n, double pivot, int method,
                       int target_idx, int index_width);
void xm_solver_destroy(void* solver);
/* objective value at x = (p0[, p1]) in degrees */
double xm_solver_score(void* solver, const double* x, int nx);
/* `count` parameter vectors, stored 2 doubles apart (p0[, p1] in degrees), evaluated in one hand-off to the worker
 * team -> out[count]; each value equals xm_solver_score's for the same vector */
void xm_solver_score_batch(void* solver, const double* xs, int nx, int count, double* out);
/* objective evaluations performed so far (xm_solver_de evaluates some trials speculatively, so this can exceed the
 * nfev it reports, which counts the evaluations of the sequential algorithm) */
long xm_solver_nfev(void* solver);
/* team size of one objective evaluation inside xm_solver_de (<= 0: min(16, hardware threads / 2); 1 = serial);
 * returns the value set.  Outside xm_solver_de evaluations are always serial. */
int xm_solver_set_threads(void* solver, int threads);
/* f(x) and its forward-difference gradient (n = 1 or 2 parameters in degrees, box [lb, ub]) exactly as scipy's L-BFGS-B
 * requests them for the polish of phasing.py:276-284 (approx_derivative "2-point", abs_step 1e-8, bounds-aware steps);
 * n + 1 evaluations in one batch.  Returns 0, or -1 for bad arguments. */
int xm_solver_fg(void* solver, const double* x, int n, const double* lb, const double* ub, double* f_out, double* g_out);
/* diagnostics: work shares that a search's own thread computed in place of a team member that was not there in time
 * (still asleep, descheduled) -- the value of every evaluation is the same either way */
long xm_solver_pool_backups(void);
/* the differential-evolution generations (no polish); returns 0 = converged, 1 = maxiter reached */
int xm_solver_de(void* solver, int p0_only, unsigned seed, double tol, int maxiter, double* x_out /*[2]*/,
                 double* fun_out, int* nfev_out, int* nit_out);

/* A8, host side: the phase table e^{i phi}, phi[k] = rad(p0) + rad(p1) * (coords[k] - pivot) / (max - min coords)
 * (processing/phasing.py:56-73; scalar phase for a zero range), fp64 arithmetic rounded once to the storage
 * precision.  `out`: n interleaved (re, im) pairs in HOST memory, float32 if as_float != 0 else float64 (the caller's
 * pinned staging buffer for xm_phase_apply / xm_pipeline_fused).  Returns 0, or -1 for bad arguments. */
int xm_phase_table(const double* coords, int n, double p0_deg, double p1_deg, double pivot, void* out, int as_float);

/* A8 with one ramp per row (`autophase_each`): out[r, k] = in[r, k] e^{i phi}, phi = rad(p0[r]) + rad(p1[r]) *
 * (coords[k] - pivot[r]) / (max coords - min coords), the statements of phasing.py:56-73 in fp64 (a zero range gives
 * phi = rad(p0[r])).  `coords` (n doubles, any axis, uniform or not), `p0` / `p1` (degrees) / `pivot` (n_rows doubles
 * each) and `skip` (NULL, or n_rows int32: nonzero rows are copied through unchanged, whatever their p0 / p1 / pivot
 * hold) are DEVICE arrays; data XM_C64 / XM_C128, contiguous rows, in == out allowed.  The angle of every bin is the
 * reference's to the bit; a thread takes sincos once per eight consecutive bins and turns from bin to bin by the
 * angle's exact difference (a short series; differences above 1/4 rad take sincos again). */
int xm_phase_apply_rows(const void* in, void* out, const double* coords, int64_t n_rows, int n, const double* p0,
                        const double* p1, const double* pivot, const int32_t* skip, int dtype, void* stream);

/* ---- A7 on the device: the (p0, p1) search of processing/phasing.py:276-284 for the ACME objective (:100-122) as ONE
 * workgroup beside the streaming kernels (csrc/xm_search.hip): scipy 1.15.3's differential evolution for the
 * reference's configuration (seed -> numpy RandomState stream, latin hypercube, best1bin, dither U[0.5, 1), CR 0.7,
 * immediate updating, tol on std/mean) -- the trial vectors are scipy's bit for bit given equal comparisons of the
 * energies -- followed by the test scipy's L-BFGS-B polish starts with (f and its forward-difference gradient at the
 * best member; projected gradient against pgtol = 1e-5).  `slice`: the n complex128 bins of the spectrum through the
 * global maximum, device-accessible (the selection stage leaves it in pinned host memory); its coordinate axis must
 * be uniform, c[k] = c0 + k cstep, x_range = max c - min c > 0 (phasing.py:56-59).  The pivot is the coordinate of the
 * first arg-max of |slice| (phasing.py:229-238).  `out` (device-accessible, e.g. pinned host memory) is filled when
 * the search ends, `seq` last (system-scope release): poll it with xm_atomic_load_acquire_i64.  Asynchronous on
 * `stream`; the stream's device must be current.  n <= 16576. */
typedef struct {
  double x[2];          /* p0, p1 in degrees (p1 = 0 with p0_only)                                                  */
  double fun;           /* objective at x                                                                            */
  double pg_norm;       /* L-BFGS-B's projected-gradient norm at x (forward differences, approx_derivative's steps) */
  int32_t nfev, nit;    /* evaluations and generations of the differential evolution (the gradient test's n + 1
                           evaluations are not counted)                                                              */
  int32_t status;       /* 0 = converged, 1 = maxiter reached                                                        */
  int32_t needs_polish; /* 0: pg_norm <= pgtol / 2, scipy's polish would return x unchanged; 1: the caller polishes
                           (xmris_amd/autophase_solver.py, the reference's route)                                    */
  int32_t target_idx;   /* first arg-max of |slice| (index of the pivot coordinate)                                  */
  int32_t pad_;
  uint64_t seq;         /* the launch's `seq`, written last                                                          */
  double t_us[8];       /* diagnostics, microseconds as the optimiser's wave saw them: [0] naming the points,
                           [1] phase tables, [2] drawing the next trial's random part (overlaps the workers' sums),
                           [3] waiting for the sums, [4] taking the scores, [5] the whole search                     */
} xm_search_result;
int xm_search_supported(int n, int method, double x_range);
int xm_search_launch(const void* slice, int n, double c0, double cstep, double x_range, int method, int p0_only,
                     unsigned seed, double tol, int maxiter, uint64_t seq, xm_search_result* out, void* stream);
/* The device objective alone (tests; cross-checks against the numpy statement): fs[e] = ACME score at
 * (xs[2e], xs[2e+1]) degrees, e < count, pivot = coordinate of bin `target_idx` (< 0: the first arg-max of |slice|).
 * `xs` / `fs` device-accessible. */
int xm_search_eval(const void* slice, int n, double c0, double cstep, double x_range, int target_idx, int p0_only,
                   const double* xs, int count, double* fs, void* stream);

/* ---- A7 for every spectrum of a dataset (`autophase_each`): the search above for each row of in[n_rows, n] (XM_C64 /
 * XM_C128, contiguous rows, read only; samples are widened to fp64 on load), one workgroup per row over all CUs of
 * `stream` (rows go round the resident workgroups by a grid stride).  Each row's search is the same function of its
 * samples as a lone xm_search_launch.  `pivot`: NaN -- every row's pivot is the coordinate of its first arg-max of |X|
 * (`target_idx` must be -1); otherwise that pivot for every row, with `target_idx` the bin nearest to it
 * (phasing.py:233-235).  `records`: n_rows records in plain device memory, complete when the stream reaches the
 * launch's end (no sequence word).  A row without a search -- all bins zero, or a sample that is not finite: the ACME
 * score is 0/0 there -- ends before the first evaluation with x, fun, pg_norm = NaN and its own status.
 * Support is xm_search_supported's: ACME (method 0), a uniform axis with x_range > 0, 2 <= n <= 16576. */
enum { XM_SEARCH_CONVERGED = 0, XM_SEARCH_MAXITER = 1, XM_SEARCH_ALL_ZERO = 2, XM_SEARCH_NOT_FINITE = 3 };
typedef struct {
  double x[2];          /* p0, p1 in degrees (p1 = 0 with p0_only)                                     */
  double fun;           /* objective at x                                                               */
  double pg_norm;       /* projected-gradient norm at x, as in xm_search_result                         */
  int32_t nfev, nit;    /* evaluations and generations (the gradient test's are not counted)            */
  int32_t target_idx;   /* the target bin: first arg-max of |row|, or the one given (-1: not finite)    */
  int32_t status;       /* XM_SEARCH_*                                                                  */
  int32_t needs_polish; /* 1: the caller polishes on the reference's route (see xm_search_result)       */
  int32_t pad_;
} xm_search_row;
int xm_search_rows_supported(int n, int method, double x_range, int dtype);
int xm_search_rows(const void* in, int64_t n_rows, int n, int dtype, double c0, double cstep, double x_range, int p0_only,
                   unsigned seed, double tol, int maxiter, double pivot, int target_idx, xm_search_row* records,
                   void* stream);

/* ---- A7 on the host without the interpreter: the same search -- xm_solver_de's generations, then the projected-
 * gradient test of the polish (xm_solver_fg) -- run by a native thread of the library's search service; `out` (HOST
 * memory) is filled like a search kernel fills it, `seq` last (poll it with xm_atomic_load_acquire_i64).  `slice`
 * (n complex128, host-readable) and `coords` (n float64) are copied at submission; `out` must stay valid until the
 * search has ended.  `target_idx` < 0: the first
 * arg-max of |slice| (phasing.py:229); the pivot is coords[target_idx].  `threads`: team size of the generations
 * (<= 0: the library's default).  Returns at once. */
int xm_hostsearch_submit(const void* slice, int n, const double* coords, int method, int target_idx, int index_width,
                         int p0_only, unsigned seed, double tol, int maxiter, int threads, uint64_t seq,
                         xm_search_result* out);

/* searches the service runs side by side (1 ... 8, default 4): further submissions wait in its queue, in order */
int xm_hostsearch_set_workers(int n);

/* ---- streams with a partition of the chip.  A search kernel (above) needs a whole CU's registers for milliseconds,
 * and the streaming kernels are persistent grids sized to fill every CU: sharing one pool of CUs, searches wait for a
 * kernel boundary to start and the streaming kernels then find CUs taken (measured: main pass +7 %, stalls of
 * milliseconds).  So the chip is split: `reserved_cus` CUs -- the first mask bits, i.e. spread round-robin over the
 * eight XCDs -- belong to the search streams (partition 1), the rest to the compute stream (partition 0).  Persistent
 * launches size their grids by the CUs of the stream they are given.  The stream's device is the current one. */
int xm_stream_create(void** stream, int reserved_cus, int partition);
int xm_stream_destroy(void* stream);
/* CUs `stream` may use (all of the device's for an ordinary stream); negative xm_status on failure */
int xm_stream_cus(void* stream);

/* ---- (e) multi-GPU: publication primitives of the one-node O(1) exchange (xmris_amd/sharding.py::ShmExchange; the
 * global arg-max and the one (p0, p1) of phasing.py:229, 276-290 cross the ranks through a shared-memory page).  HOST
 * pointers.  The payload of a slot is written with plain stores, its sequence word with a release store, and readers
 * poll the sequence words with acquire loads. */
int64_t xm_atomic_load_acquire_i64(const int64_t* p);
void xm_atomic_store_release_i64(int64_t* p, int64_t value);
/* 1 once all `count` words (`stride_words` apart) are >= value; 0 if not within `spin_us` microseconds of busy polling */
int xm_atomic_wait_all_ge_i64(const int64_t* p, int stride_words, int count, int64_t value, int spin_us);

#ifdef __cplusplus
}
#endif
#endif /* XMRIS_HIP_H */
