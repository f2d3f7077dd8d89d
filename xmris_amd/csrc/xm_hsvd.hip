// Host side of xm_hsvd_rows (include/xmris_hip.h); the kernel is in xm_hsvd.h.
#include "xm_host.h"
#include "xm_hsvd.h"

#include <string>

static int hs_fail(const std::string& msg) { return xm_fail(XM_ERR_INVALID_ARG, "hsvd_rows: " + msg); }

namespace {
XmResidency g_hs_res[2];  // one residency record per kernel instantiation

template <int FORM>
int hs_launch(const HsvdArgs& A, hipStream_t st) {
  return xm_launch_items(g_hs_res[FORM], k_hsvd<FORM>, XM_HS_NT, hs_lds_bytes(A.M, A.K), A.nb, A, st, "k_hsvd",
                         FORM == XM_HS_FORM_MFMA ? "mfma" : "fma", A.M, A.K);  // <form, M, K>
}
}  // namespace

extern "C" int xm_hsvd_rows(const void* x, int64_t row_stride, void* y_or_null, double* freq, double* damp, double* amp,
                            double* phase, int32_t* removed, int32_t* n_removed, int32_t* status, int64_t n_batch, int N,
                            int M, int K, double dt, double f_lo, double f_hi, int dtype, void* workspace, void* stream) {
  const int dt_code = dtype & 0xff, stop = (dtype >> 9) & 7;
  if (dt_code != XM_C64 && dt_code != XM_C128 || (dtype & ~0xfff) || stop > XM_HS_STOP_AMPL)
    return hs_fail("unknown dtype " + std::to_string(dtype));
  if (M < 2 || M > XM_HS_MAXM) return hs_fail("M (n_cols) must be in 2 ... 64");
  if (K < 1 || K > M - 1 || K > XM_HS_MAXK) return hs_fail("K (rank) must be in 1 ... min(M - 1, 32)");
  if (N < 2 * M) return hs_fail("N must be at least 2 M");
  if (N > XM_HS_MAXN) return hs_fail("N must not exceed 16384 points");
  if (!(dt > 0.0) || !std::isfinite(dt)) return hs_fail("needs a finite dt > 0");
  if (!std::isfinite(f_lo) || !std::isfinite(f_hi) || !(f_lo <= f_hi)) return hs_fail("needs finite f_lo <= f_hi (band)");
  if (n_batch < 0) return hs_fail("needs n_batch >= 0");
  if (row_stride < N) return hs_fail("row_stride must be at least N");
  if (!x || !freq || !damp || !amp || !phase || !removed || !n_removed || !status || !workspace) return hs_fail("null pointer");
  if (n_batch > 0xffffffffLL) return hs_fail("too many rows (> 2^32 - 1)");
  if (n_batch == 0) return XM_OK;

  HsvdArgs A{};
  A.x = x;
  A.stride = row_stride;
  A.y = y_or_null;
  A.freq = freq;
  A.damp = damp;
  A.amp = amp;
  A.phase = phase;
  A.removed = removed;
  A.n_removed = n_removed;
  A.status = status;
  A.nb = n_batch;
  A.N = N;
  A.M = M;
  A.K = K;
  A.is_c128 = dt_code == XM_C128;
  A.stop = stop;
  A.dt = dt;
  A.f_lo = f_lo;
  A.f_hi = f_hi;
  A.counter = (unsigned*)workspace;

  DeviceGuard guard(x);
  hipStream_t st = (hipStream_t)stream;
  return (dtype & XM_HSVD_GRAM_FMA) ? hs_launch<XM_HS_FORM_FMA>(A, st) : hs_launch<XM_HS_FORM_MFMA>(A, st);
}
