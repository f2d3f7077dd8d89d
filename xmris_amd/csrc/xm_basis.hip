// Host side of the basis-set fitting entry points (xm_basis_* in include/xmris_hip.h); kernels in xm_basis.h.
#include "xm_host.h"
#include "xm_basis.h"

#include <cmath>
#include <string>

static int bs_fail(const std::string& msg) { return xm_fail(XM_ERR_INVALID_ARG, "basis: " + msg); }

namespace {
XmResidency g_bs_res;

// ord / gs: the metabolites sorted by group (ascending m within a group).  Nonzero: an index out of range or an empty group
template <class Args>
int bs_groups(Args& A, const int32_t* group, int M, int G) {
  if (M < 1) return bs_fail("n_metab must be at least 1");
  if (G < 1 || G > M) return bs_fail("n_groups must be in 1 ... n_metab");
  if (M + 3 * G + 1 > XM_BS_MAXQ) return bs_fail("n_metab + 3 n_groups + 1 must not exceed " + std::to_string(XM_BS_MAXQ));
  if (!group) return bs_fail("null group array");
  int k = 0;
  for (int g = 0; g < G; ++g) {
    A.gs[g] = (unsigned char)k;
    for (int m = 0; m < M; ++m) {
      if (group[m] < 0 || group[m] >= G)
        return bs_fail("metabolite " + std::to_string(m) + ": group " + std::to_string(group[m]) + " is out of range");
      if (group[m] == g) A.ord[k++] = (unsigned char)m;
    }
    if (k == A.gs[g]) return bs_fail("group " + std::to_string(g) + " has no metabolite");
  }
  A.gs[G] = (unsigned char)k;
  return XM_OK;
}
}  // namespace

extern "C" {

int64_t xm_basis_workspace_bytes(int64_t n_batch, int n, int n_metab) {
  (void)n_batch;
  (void)n;
  return 256 + 8 * (int64_t)(n_metab > 0 ? n_metab : 0);  // the row counter pair, then ||B_m||
}

int xm_basis_model(const double* params, int64_t n_batch, const void* basis, int n_metab, const int32_t* group,
                   int n_groups, int n, double dt, void* out, void* stream) {
  BasisModelArgs A{};
  if (const int rc = bs_groups(A, group, n_metab, n_groups)) return rc;
  if (n_batch < 0 || n < 1) return bs_fail("model: needs n_batch >= 0, n >= 1");
  if (n_batch > 0 && (!params || !basis || !out)) return bs_fail("model: null pointer");
  if (!std::isfinite(dt)) return bs_fail("model: dt must be finite");
  if (n_batch == 0) return XM_OK;
  A.params = params;
  A.basis = (const double*)basis;
  A.out = (double*)out;
  A.nb = n_batch;
  A.n = n;
  A.M = n_metab;
  A.G = n_groups;
  A.dt = dt;
  DeviceGuard guard(out);
  const long long total = (long long)n_batch * n;
  long long blocks = (total + 255) / 256;
  if (blocks > 65536) blocks = 65536;
  hipLaunchKernelGGL(k_basis_model, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, A);
  HIP_TRY(hipGetLastError());
  return XM_OK;
}

int xm_basis_fit(const void* in, int64_t in_row_stride, int64_t n_batch, int n, double dt, int skip, const void* basis,
                 int n_metab, const int32_t* group, int n_groups, const double* init, const double* lower,
                 const double* upper, const int32_t* fixed, int max_iter, double ftol, double xtol, double* params,
                 double* amp_sd, double* rss, int32_t* status, int32_t* iters, void* fit_data, void* workspace,
                 int64_t workspace_bytes, int dtype, void* stream) {
  BasisFitArgs A{};
  if (const int rc = bs_groups(A, group, n_metab, n_groups)) return rc;
  const int M = n_metab, G = n_groups, Q = M + 3 * G + 1;
  if (n_batch < 0 || n < 1 || in_row_stride < n) return bs_fail("needs n_batch >= 0, n >= 1, row stride >= n");
  if (skip < 0 || skip >= n) return bs_fail("skip must be in 0 ... n - 1");
  if (dtype != XM_C64 && dtype != XM_C128) return bs_fail("dtype must be XM_C64 or XM_C128");
  if (!init || !lower || !upper || !fixed) return bs_fail("null parameter array");
  if (n_batch > 0 && (!in || !basis || !params || !amp_sd || !rss || !status || !iters || !workspace))
    return bs_fail("null pointer");
  if (workspace_bytes < xm_basis_workspace_bytes(n_batch, n, M))
    return bs_fail("workspace too small (see xm_basis_workspace_bytes)");
  if (max_iter < 1 || !(ftol >= 0.0) || !(xtol >= 0.0)) return bs_fail("needs max_iter >= 1, ftol >= 0, xtol >= 0");
  if (!(dt > 0.0) || !std::isfinite(dt)) return bs_fail("dt must be positive and finite");
  if (n_batch > 0xffffffffLL) return bs_fail("n_batch too large (> 2^32 - 1)");

  // bounds and the internal start values (HOST arrays of Q values: shared by the batch)
  int P = 0;
  for (int q = 0; q < Q; ++q) {
    const std::string who = "parameter " + std::to_string(q) + ": ";
    const double lo = lower[q], hi = upper[q];
    const bool amplitude = q < M, nonlinear = q >= M && q < M + 3 * G;
    if (std::isnan(lo) || std::isnan(hi) || lo > hi) return bs_fail(who + "bounds must satisfy lo <= hi");
    if (lo == INFINITY || hi == -INFINITY) return bs_fail(who + "a lower bound of +inf or an upper bound of -inf");
    const bool is_fixed = fixed[q] || lo == hi;
    if (nonlinear && !is_fixed && !(std::isfinite(lo) && std::isfinite(hi)))
      return bs_fail(who + "a free shift or damping needs two finite bounds");
    const bool automatic = amplitude && std::isnan(init[q]);
    if (!automatic && !std::isfinite(init[q])) return bs_fail(who + "the initial value must be finite");
    A.lo[q] = lo;
    A.hi[q] = hi;
    if (is_fixed) {
      if (automatic) return bs_fail(who + "a fixed amplitude needs a value");
      A.bt[q] = XM_WG_FIXED;
      A.col[q] = -1;
      A.u0[q] = std::fmin(std::fmax(init[q], lo), hi);
      continue;
    }
    if (P >= XM_BS_MAXP) return bs_fail("more than " + std::to_string(XM_BS_MAXP) + " free parameters");
    A.col[q] = (signed char)P++;
    A.bt[q] = lm_bound_type(lo, hi);
    if (automatic) {
      A.u0[q] = NAN;  // the kernel starts it per voxel
      continue;
    }
    const double v = std::fmin(std::fmax(init[q], lo), hi);  // initial values are clipped into their bounds
    A.u0[q] = lm_start_value(A.bt[q], v, lo, hi);
  }
  if (P < 1) return bs_fail("every parameter is fixed");
  if (n - skip < P)
    return bs_fail("fitted points (" + std::to_string(n - skip) + ") fewer than the free parameters (" + std::to_string(P) + ")");
  if (n_batch == 0) return XM_OK;

  A.x = in;
  A.basis = (const double*)basis;
  A.bnorm = (const double*)((const char*)workspace + 256);
  A.stride = in_row_stride;
  A.nb = n_batch;
  A.n = n;
  A.skip = skip;
  A.is_c64 = dtype == XM_C64;
  A.dt = dt;
  A.M = M;
  A.G = G;
  A.Q = Q;
  A.P = P;
  A.max_iter = max_iter;
  A.lda = P + 1;
  A.q_pts = lm_q_pts(A.lda);
  A.ftol = ftol;
  A.xtol = xtol;
  A.params = params;
  A.asd = amp_sd;
  A.rss = rss;
  A.status = status;
  A.iters = iters;
  A.fit = (double*)fit_data;
  A.counter = (unsigned*)workspace;

  DeviceGuard guard(in);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_basis_norms, dim3((unsigned)M), dim3(XM_WG_NT), 0, st, A.basis, n, skip,
                     (double*)((char*)workspace + 256));
  HIP_TRY(hipGetLastError());
  return xm_launch_items(g_bs_res, k_basis_fit, XM_WG_NT, lm_lds_bytes(P, A.lda, A.q_pts, XM_BS_MAXQ), n_batch, A, st,
                         "k_basis_fit", "fma", P, M);  // <J^T J form, free columns, metabolites>
}

}  // extern "C"
