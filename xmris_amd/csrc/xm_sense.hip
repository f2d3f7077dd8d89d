// Host side of xm_sense_unfold (include/xmris_hip.h); the kernel is in xm_sense.h.
#include "xm_host.h"
#include "xm_sense.h"

#include <string>

static int sn_fail(const std::string& msg) { return xm_fail(XM_ERR_INVALID_ARG, "sense_unfold: " + msg); }

namespace {
XmResidency g_sn_res[2][5];  // one residency record per kernel instantiation: dtype, log2 RB

template <class T, int RB>
int sn_launch(const SenseArgs& A, XmResidency& res, hipStream_t st) {
  return xm_launch_items(res, k_sense_unfold<T, RB>, XM_SN_NT, sn_lds_bytes(A.C, A.Rtot, RB), A.ngroups, A, st,
                         "k_sense_unfold", sizeof(T) == 8 ? "c128" : "c64", RB, A.C);  // <dtype, RB, coils>
}

template <class T>
int sn_dispatch(const SenseArgs& A, XmResidency* res, hipStream_t st) {
  if (A.Rtot <= 1) return sn_launch<T, 1>(A, res[0], st);
  if (A.Rtot <= 2) return sn_launch<T, 2>(A, res[1], st);
  if (A.Rtot <= 4) return sn_launch<T, 4>(A, res[2], st);
  if (A.Rtot <= 8) return sn_launch<T, 8>(A, res[3], st);
  return sn_launch<T, 16>(A, res[4], st);
}
}  // namespace

extern "C" int xm_sense_unfold(const void* a, void* y, const void* sens, const void* linv_or_null, double* g_or_null,
                               int32_t* status_or_null, int64_t n_outer, int C, const int32_t n[3],
                               const int32_t accel[3], int N_t, const int64_t a_strides[5], const int64_t y_strides[4],
                               double regularization, int dtype, void* workspace, void* stream) {
  if (!a || !y || !sens || !n || !accel || !a_strides || !y_strides || !workspace) return sn_fail("null pointer");
  if (C < 1 || C > XM_SN_MAXC) return sn_fail("C must be in 1 ... 64");
  long long R = 1, groups = 1;
  for (int d = 0; d < 3; ++d) {
    if (accel[d] < 1) return sn_fail("every accel must be at least 1");
    if (n[d] < 1) return sn_fail("every n must be at least 1");
    R *= accel[d];
    if (R > XM_SN_MAXR) return sn_fail("R = the product of accel must not exceed 16");
    groups *= n[d];
    if (groups > 0xffffffffLL) return sn_fail("too many groups (> 2^32 - 1)");
  }
  if (N_t < 1) return sn_fail("needs N_t >= 1");
  if (!(regularization >= 0.0) || !std::isfinite(regularization))
    return sn_fail("regularization must be finite and not negative");
  if (dtype != XM_C64 && dtype != XM_C128) return sn_fail("unknown dtype " + std::to_string(dtype));
  if (y == a) return sn_fail("y must not be a");
  if (n_outer < 0) return sn_fail("needs n_outer >= 0");
  if (n_outer > 0 && groups > 0xffffffffLL / n_outer) return sn_fail("too many groups (> 2^32 - 1)");
  if (n_outer == 0) return XM_OK;

  SenseArgs A{};
  A.a = a;
  A.y = y;
  A.sens = (const double*)sens;
  A.linv = (const double*)linv_or_null;
  A.g = g_or_null;
  A.status = status_or_null;
  A.ngroups = n_outer * groups;
  for (int d = 0; d < 5; ++d) A.as[d] = a_strides[d];
  for (int d = 0; d < 4; ++d) A.ys[d] = y_strides[d];
  A.C = C;
  for (int d = 0; d < 3; ++d) {
    A.n[d] = n[d];
    A.R[d] = accel[d];
  }
  A.Nt = N_t;
  A.Rtot = (int)R;
  A.reg = regularization;
  A.pair = dtype == XM_C64 && N_t % 2 == 0 && (((size_t)a | (size_t)y) & 15u) == 0;
  for (int d = 0; d < 5; ++d) A.pair = A.pair && a_strides[d] % 2 == 0;
  for (int d = 0; d < 4; ++d) A.pair = A.pair && y_strides[d] % 2 == 0;
  A.counter = (unsigned*)workspace;

  DeviceGuard guard(a);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == XM_C128) return sn_dispatch<double>(A, g_sn_res[1], st);
  return sn_dispatch<float>(A, g_sn_res[0], st);
}
