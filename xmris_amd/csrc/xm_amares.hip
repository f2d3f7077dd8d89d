// Host side of the AMARES entry points (xm_amares_* in include/xmris_hip.h); kernels in xm_amares.h.
#include "xm_host.h"
#include "xm_amares.h"

#include <cmath>
#include <string>

static int am_fail(const std::string& msg) { return xm_fail(XM_ERR_INVALID_ARG, "amares: " + msg); }

namespace {
XmResidency g_am_res, g_am_res_linked;  // one residency record per kernel instantiation
}  // namespace

extern "C" {

int64_t xm_amares_workspace_bytes(int64_t n_batch, int n, int n_peaks) {
  (void)n_batch;
  (void)n;
  (void)n_peaks;
  return 256;  // the row counter pair
}

int xm_amares_model(const double* params, int64_t n_batch, int n_peaks, int n, double dt, double t0, void* out,
                    void* stream) {
  if (n_batch < 0 || n < 1 || n_peaks < 1 || n_peaks > XM_AM_MAXK) return am_fail("model: needs n >= 1, 1 <= n_peaks <= 16");
  if (n_batch > 0 && (!params || !out)) return am_fail("model: null pointer");
  if (!std::isfinite(dt) || !std::isfinite(t0)) return am_fail("model: dt and t0 must be finite");
  if (n_batch == 0) return XM_OK;
  DeviceGuard guard(out);
  const long long total = (long long)n_batch * n;
  long long blocks = (total + 255) / 256;
  if (blocks > 65536) blocks = 65536;
  hipLaunchKernelGGL(k_amares_model, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, params,
                     (long long)n_batch, n_peaks, n, dt, t0, (double*)out);
  HIP_TRY(hipGetLastError());
  return XM_OK;
}

int xm_amares_fit(const void* in, int64_t in_row_stride, int64_t n_batch, int n, double dt, double t0, int n_peaks,
                  const double* init, const double* lower, const double* upper, const int32_t* fixed, int max_iter,
                  double ftol, double xtol, double* params, double* amp_sd, double* rss, int32_t* status,
                  int32_t* iters, void* fit_data, void* workspace, int64_t workspace_bytes, int dtype, void* stream) {
  return xm_amares_fit_linked(in, in_row_stride, n_batch, n, dt, t0, n_peaks, init, lower, upper, fixed, nullptr, nullptr,
                              nullptr, max_iter, ftol, xtol, params, amp_sd, rss, status, iters, fit_data, workspace,
                              workspace_bytes, dtype, stream);
}

int xm_amares_fit_linked(const void* in, int64_t in_row_stride, int64_t n_batch, int n, double dt, double t0,
                         int n_peaks, const double* init, const double* lower, const double* upper,
                         const int32_t* fixed, const int32_t* link_to, const double* link_scale,
                         const double* link_offset, int max_iter, double ftol, double xtol, double* params,
                         double* amp_sd, double* rss, int32_t* status, int32_t* iters, void* fit_data, void* workspace,
                         int64_t workspace_bytes, int dtype, void* stream) {
  if (n_peaks < 1 || n_peaks > XM_AM_MAXK) return am_fail("n_peaks must be in 1 ... 16");
  if (n_batch < 0 || n < 1 || in_row_stride < n) return am_fail("needs n_batch >= 0, n >= 1, row stride >= n");
  if (dtype != XM_C64 && dtype != XM_C128) return am_fail("dtype must be XM_C64 or XM_C128");
  if (!init || !lower || !upper || !fixed) return am_fail("null prior-knowledge pointer");
  if (link_to && (!link_scale || !link_offset)) return am_fail("link_to needs link_scale and link_offset");
  if (n_batch > 0 && (!in || !params || !amp_sd || !rss || !status || !iters || !workspace))
    return am_fail("null pointer");
  if (workspace_bytes < xm_amares_workspace_bytes(n_batch, n, n_peaks))
    return am_fail("workspace too small (see xm_amares_workspace_bytes)");
  if (max_iter < 1 || !(ftol >= 0.0) || !(xtol >= 0.0)) return am_fail("needs max_iter >= 1, ftol >= 0, xtol >= 0");
  if (!(dt > 0.0) || !std::isfinite(dt) || !std::isfinite(t0)) return am_fail("dt must be positive and finite, t0 finite");
  if (n_batch > 0xffffffffLL) return am_fail("n_batch too large (> 2^32 - 1)");

  AmaresFitArgs A{};
  A.x = in;
  A.stride = in_row_stride;
  A.nb = n_batch;
  A.n = n;
  A.is_c64 = dtype == XM_C64;
  A.dt = dt;
  A.t0 = t0;
  A.K = n_peaks;
  A.max_iter = max_iter;
  A.ftol = ftol;
  A.xtol = xtol;
  // bounds and the internal start values (HOST arrays of 5 n_peaks values: the prior knowledge is shared by the batch)
  const int Q = 5 * n_peaks;
  auto linked = [&](int q) { return link_to && link_to[q] >= 0; };
  for (int q = 0; q < Q; ++q) {
    A.sc[q] = 1.0;
    A.off[q] = 0.0;
    if (!link_to || link_to[q] == -1) continue;
    const int m = link_to[q];
    const std::string who = "parameter " + std::to_string(q) + ": ";
    if (m < -1 || m >= Q) return am_fail(who + "link_to " + std::to_string(m) + " is out of range");
    if (m == q) return am_fail(who + "linked to itself");
    if (m % 5 != q % 5) return am_fail(who + "linked to another kind of parameter (" + std::to_string(m) + ")");
    if (link_to[m] != -1) return am_fail(who + "its root " + std::to_string(m) + " is itself linked (compose chains)");
    if (!std::isfinite(link_scale[q]) || link_scale[q] == 0.0 || !std::isfinite(link_offset[q]))
      return am_fail(who + "link_scale must be finite and nonzero, link_offset finite");
  }
  int P = 0;
  for (int q = 0; q < Q; ++q) {
    if (linked(q)) continue;  // takes everything from its root, below
    const double lo = lower[q], hi = upper[q];
    if (std::isnan(lo) || std::isnan(hi) || lo > hi || !std::isfinite(init[q]))
      return am_fail("parameter " + std::to_string(q) + ": bounds must satisfy lo <= hi, initial value finite");
    const double v = std::fmin(std::fmax(init[q], lo), hi);  // initial values are clipped into their bounds
    A.lo[q] = lo;
    A.hi[q] = hi;
    if (fixed[q] || lo == hi) {
      if (!std::isfinite(v)) return am_fail("parameter " + std::to_string(q) + ": a fixed value must be finite");
      A.bt[q] = XM_WG_FIXED;
      A.col[q] = -1;
      A.u0[q] = v;
      continue;
    }
    A.col[q] = (signed char)P++;
    A.bt[q] = lm_bound_type(lo, hi);
    A.u0[q] = lm_start_value(A.bt[q], v, lo, hi);
  }
  // A linked parameter: the root's column, transform and bounds; its own `lower` / `upper` / `init` / `fixed` are not
  // read.  A follower of a fixed root is fixed at the mapped value.
  bool any_link = false;
  for (int q = 0; q < Q; ++q) {
    if (!linked(q)) continue;
    const int m = link_to[q];
    A.lo[q] = A.lo[m];
    A.hi[q] = A.hi[m];
    A.bt[q] = A.bt[m];
    A.col[q] = A.col[m];
    if (A.col[m] < 0) {
      A.u0[q] = link_scale[q] * A.u0[m] + link_offset[q];
      if (!std::isfinite(A.u0[q])) return am_fail("parameter " + std::to_string(q) + ": a fixed value must be finite");
      continue;
    }
    A.u0[q] = A.u0[m];
    A.lk[q] = 1;
    A.sc[q] = link_scale[q];
    A.off[q] = link_offset[q];
    any_link = true;
  }
  if (P < 1) return am_fail("every parameter is fixed");
  if (n < P) return am_fail("n (" + std::to_string(n) + ") smaller than the free parameters (" + std::to_string(P) + ")");
  if (n_batch == 0) return XM_OK;

  A.P = P;
  A.lda = P + 1;
  A.q_pts = lm_q_pts(A.lda);
  A.params = params;
  A.asd = amp_sd;
  A.rss = rss;
  A.status = status;
  A.iters = iters;
  A.fit = (double*)fit_data;
  A.counter = (unsigned*)workspace;

  DeviceGuard guard(in);
  hipStream_t st = (hipStream_t)stream;
  const size_t lds = lm_lds_bytes(P, A.lda, A.q_pts, XM_AM_MAXQ);
  if (any_link)  // <LINKED, free columns>
    return xm_launch_items(g_am_res_linked, k_amares_fit<true>, XM_WG_NT, lds, n_batch, A, st, "k_amares_fit", "true", P, -1);
  return xm_launch_items(g_am_res, k_amares_fit<false>, XM_WG_NT, lds, n_batch, A, st, "k_amares_fit", "false", P, -1);
}

}  // extern "C"
