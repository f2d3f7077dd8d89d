// Host side of xm_coil_combine (include/xmris_hip.h); the kernel is in xm_coils.h.
#include "xm_host.h"
#include "xm_coils.h"

#include <string>

static int cc_fail(const std::string& msg) { return xm_fail(XM_ERR_INVALID_ARG, "coil_combine: " + msg); }

namespace {
XmResidency g_cc_res[3];  // one residency record per kernel instantiation

template <int FORM>
int cc_launch(const CoilArgs& A, const char* form, hipStream_t st) {
  return xm_launch_items(g_cc_res[FORM], k_coil_combine<FORM>, XM_CC_NT, cc_lds_bytes(A.C), A.nv, A, st,
                         "k_coil_combine", form, A.C, -1);  // <form, coils>
}
}  // namespace

extern "C" int xm_coil_combine(const void* x, const void* ref_or_null, void* y, void* w, double* quality,
                               int32_t* status, int64_t n_outer, int C, int64_t n_inner, int N, int N_R,
                               const void* linv_or_null, int method, int n_points, int is_complex128, void* workspace,
                               void* stream) {
  if (C < 1 || C > XM_CC_MAXC) return cc_fail("C must be in 1 ... 64");
  if (N < 1 || N_R < 1) return cc_fail("needs N >= 1 and N_R >= 1");
  if (!ref_or_null && N_R != N) return cc_fail("without a reference N_R must equal N");
  if (n_points < 1 || n_points > N_R) return cc_fail("n_points must be in 1 ... N_R");
  if (method != XM_COIL_SVD && method != XM_COIL_FIRST_POINT && method != XM_COIL_SVD_FMA)
    return cc_fail("unknown method " + std::to_string(method));
  if (n_outer < 0 || n_inner < 0) return cc_fail("needs n_outer >= 0 and n_inner >= 0");
  if (!x || !y || !w || !quality || !status || !workspace) return cc_fail("null pointer");
  const long long nv = (long long)n_outer * n_inner;
  if (nv > 0xffffffffLL) return cc_fail("too many voxels (> 2^32 - 1)");
  if (nv == 0) return XM_OK;

  CoilArgs A{};
  A.x = x;
  A.ref = ref_or_null ? ref_or_null : x;
  A.y = y;
  A.w = (double*)w;
  A.quality = quality;
  A.status = status;
  A.linv = (const double*)linv_or_null;
  A.nv = nv;
  A.n_inner = n_inner;
  A.C = C;
  A.N = N;
  A.NR = N_R;
  A.n_points = n_points;
  A.is_c128 = is_complex128 != 0;
  A.counter = (unsigned*)workspace;

  DeviceGuard guard(x);
  hipStream_t st = (hipStream_t)stream;
  if (method == XM_COIL_FIRST_POINT) return cc_launch<XM_CC_FORM_FIRST>(A, "first_point", st);
  if (method == XM_COIL_SVD && C >= 8) return cc_launch<XM_CC_FORM_MFMA>(A, "mfma", st);
  return cc_launch<XM_CC_FORM_FMA>(A, "fma", st);  // below 8 coils a 16-row block would be mostly padding
}
