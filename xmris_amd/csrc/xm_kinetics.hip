// Host side of xm_kinetics_fit (include/xmris_hip.h); the kernel is in xm_kinetics.h.
#include "xm_host.h"
#include "xm_kinetics.h"
#include "xm_lm.h"  // lm_bound_type, lm_start_value: the host-side start transform is all the kernel shares with it

#include <cmath>
#include <string>
#include <vector>

static int kin_fail(const std::string& msg) { return xm_fail(XM_ERR_INVALID_ARG, "kinetics: " + msg); }

namespace {
template <int C>
int kin_launch(const KineticsArgs& A, hipStream_t st) {
  const long long blocks = (A.n_items + XM_KIN_WAVES - 1) / XM_KIN_WAVES;  // <= 2^31 - 1: checked by the caller
  xm_note_kernel("k_kinetics_fit", nullptr, "double", C, -1);  // <scalar, repetitions per lane>
  hipLaunchKernelGGL(k_kinetics_fit<C>, dim3((unsigned)blocks), dim3(64 * XM_KIN_WAVES), 0, st, A);
  HIP_TRY(hipGetLastError());
  return XM_OK;
}
}  // namespace

extern "C" int xm_kinetics_fit(const double* substrate, const double* products, const double* weights, int64_t n_batch,
                               int n_products, int n_times, const double* times, const double* flip_s,
                               const double* flip_p, const double* init, const double* lower, const double* upper,
                               const int32_t* fixed, int max_iter, double ftol, double xtol, double* params,
                               double* param_sd, double* rss, int32_t* status, int32_t* iters, double* fit,
                               double* auc_ratio, void* stream) {
  const int M = n_products, T = n_times;
  if (T < 2 || T > XM_KIN_MAXT) return kin_fail("needs 2 <= T <= " + std::to_string(XM_KIN_MAXT));
  if (M < 1 || M > XM_KIN_MAXM) return kin_fail("needs 1 <= M <= " + std::to_string(XM_KIN_MAXM));
  if (n_batch < 0) return kin_fail("needs n_batch >= 0");
  if (!times || !flip_s || !flip_p || !init || !lower || !upper || !fixed) return kin_fail("null host array");
  if (n_batch > 0 && (!substrate || !products || !params || !param_sd || !rss || !status || !iters || !auc_ratio))
    return kin_fail("null pointer");
  if (max_iter < 1 || !(ftol >= 0.0) || !(xtol >= 0.0)) return kin_fail("needs max_iter >= 1, ftol >= 0, xtol >= 0");
  for (int n = 0; n < T; ++n) {
    if (!std::isfinite(times[n])) return kin_fail("times must be finite");
    if (n > 0 && !(times[n] > times[n - 1])) return kin_fail("times must increase");
  }
  const double half_pi = 1.5707963267948966;
  for (int n = 0; n < (M + 1) * T; ++n) {
    const double th = n < T ? flip_s[n] : flip_p[n - T];
    if (!(th > 0.0 && th < half_pi)) return kin_fail("flip angles must lie inside (0, pi / 2)");
  }

  KineticsArgs A{};
  static const char* const names[3] = {"k", "rho", "z"};
  for (int m = 0; m < M; ++m) {
    int P = 0;
    for (int q = 0; q < 3; ++q) {
      const std::string who = "product " + std::to_string(m) + ", " + names[q] + ": ";
      const double lo = lower[m * 3 + q], hi = upper[m * 3 + q], v0 = init[m * 3 + q];
      if (std::isnan(lo) || std::isnan(hi) || lo > hi) return kin_fail(who + "bounds must satisfy lo <= hi");
      if (lo == INFINITY || hi == -INFINITY) return kin_fail(who + "a lower bound of +inf or an upper bound of -inf");
      if (q == 1 && lo < 0.0) return kin_fail(who + "the lower bound must not be negative");
      const bool is_fixed = fixed[m * 3 + q] || lo == hi;
      if (q < 2 && !is_fixed && !(std::isfinite(lo) && std::isfinite(hi)))
        return kin_fail(who + "a free rate or decay needs two finite bounds");
      const bool automatic = q == 2 && !is_fixed && std::isnan(v0);
      if (!automatic && !std::isfinite(v0)) return kin_fail(who + "the initial value must be finite");
      A.lo[m][q] = lo;
      A.hi[m][q] = hi;
      if (is_fixed) {
        A.bt[m][q] = XM_WG_FIXED;
        A.col[m][q] = -1;
        A.u0[m][q] = std::fmin(std::fmax(v0, lo), hi);
        continue;
      }
      A.col[m][q] = P++;
      A.bt[m][q] = lm_bound_type(lo, hi);
      if (automatic) {
        A.u0[m][q] = NAN;  // the kernel starts it per item
        continue;
      }
      const double v = std::fmin(std::fmax(v0, lo), hi);  // initial values are clipped into their bounds
      A.u0[m][q] = lm_start_value(A.bt[m][q], v, lo, hi);
    }
    if (P < 1) return kin_fail("product " + std::to_string(m) + ": every parameter is fixed");
    A.n_free[m] = P;
  }
  if (n_batch > 0x7fffffffLL / M * XM_KIN_WAVES) return kin_fail("n_batch too large");
  if (n_batch == 0) return XM_OK;

  // the shared tables: times, then sine and cosine of every flip angle
  const size_t n_tab = (size_t)T * (3 + 2 * (size_t)M);
  std::vector<double> tab(n_tab);
  for (int n = 0; n < T; ++n) {
    tab[n] = times[n];
    tab[T + n] = std::sin(flip_s[n]);
    tab[2 * T + n] = std::cos(flip_s[n]);
  }
  for (int n = 0; n < M * T; ++n) {
    tab[3 * (size_t)T + n] = std::sin(flip_p[n]);
    tab[(3 + (size_t)M) * T + n] = std::cos(flip_p[n]);
  }

  DeviceGuard guard(substrate);
  hipStream_t st = (hipStream_t)stream;
  double* dtab = nullptr;
  HIP_TRY(hipMallocAsync((void**)&dtab, n_tab * sizeof(double), st));
  hipError_t e = hipMemcpyAsync(dtab, tab.data(), n_tab * sizeof(double), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);  // `tab` is pageable host memory that ends with this call
  if (e != hipSuccess) {
    (void)hipFreeAsync(dtab, st);
    HIP_TRY(e);
  }

  A.sub = substrate;
  A.prod = products;
  A.wts = weights;
  A.tab = dtab;
  A.params = params;
  A.psd = param_sd;
  A.rss = rss;
  A.fit = fit;
  A.auc = auc_ratio;
  A.status = status;
  A.iters = iters;
  A.n_items = n_batch * M;
  A.ftol = ftol;
  A.xtol = xtol;
  A.T = T;
  A.M = M;
  A.max_iter = max_iter;
  const int C = (T + 63) / 64;
  const int rc = C == 1 ? kin_launch<1>(A, st) : C == 2 ? kin_launch<2>(A, st) : C == 3 ? kin_launch<3>(A, st) : kin_launch<4>(A, st);
  (void)hipFreeAsync(dtab, st);
  return rc;
}
