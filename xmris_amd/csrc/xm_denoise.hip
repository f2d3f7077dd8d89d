// Host side of xm_denoise_patches (include/xmris_hip.h); the kernel is in xm_denoise.h.
#include "xm_host.h"
#include "xm_denoise.h"

#include <string>

static int dn_fail(const std::string& msg) { return xm_fail(XM_ERR_INVALID_ARG, "denoise_patches: " + msg); }

namespace {
XmResidency g_dn_res[2];  // one residency record per kernel instantiation

template <int FORM>
int dn_launch(const DenoiseArgs& A, hipStream_t st) {
  return xm_launch_items(g_dn_res[FORM], k_denoise<FORM>, XM_DN_NT, dn_lds_bytes(A.P), A.nv, A, st, "k_denoise",
                         FORM == XM_DN_FORM_MFMA ? "mfma" : "fma", A.P, A.rank_in);  // <form, P[, rank]>
}
}  // namespace

extern "C" int xm_denoise_patches(const void* x, void* y, int32_t* rank_out, double* sigma, int32_t* status,
                                  int64_t n_outer, int s1, int s2, int s3, int p1, int p2, int p3, int N, int rank,
                                  int dtype, void* workspace, void* stream) {
  const int dt_code = dtype & 0xff, stop = (dtype >> 9) & 3;
  if (dt_code != XM_C64 && dt_code != XM_C128 || (dtype & ~0x7ff) || stop > XM_DN_STOP_EIG)
    return dn_fail("unknown dtype " + std::to_string(dtype));
  if (s1 < 1 || s2 < 1 || s3 < 1) return dn_fail("the sizes s1, s2, s3 must be at least 1");
  if (p1 < 1 || p1 > s1 || p2 < 1 || p2 > s2 || p3 < 1 || p3 > s3)
    return dn_fail("every patch size must be in 1 ... the size of its dim");
  const long long P = (long long)p1 * p2 * p3;
  if (P < 2 || P > XM_DN_MAXP) return dn_fail("the patch P = p1 p2 p3 must hold 2 ... 64 voxels");
  if (N < P) return dn_fail("N must be at least P");
  if (N > XM_DN_MAXN) return dn_fail("N must not exceed 16384 points");
  if (rank < -1 || rank > P) return dn_fail("rank must be -1 (Marchenko-Pastur rule) or in 0 ... P");
  if (n_outer < 0) return dn_fail("needs n_outer >= 0");
  if (!x || !y || !rank_out || !sigma || !status || !workspace) return dn_fail("null pointer");
  if (x == y) return dn_fail("y must not be x (windows overlap)");
  const long long grid = (long long)s1 * s2 * s3;
  if (n_outer > 0 && grid > 0xffffffffLL / n_outer) return dn_fail("too many voxels (> 2^32 - 1)");
  if (n_outer == 0) return XM_OK;

  DenoiseArgs A{};
  A.x = x;
  A.y = y;
  A.rank = rank_out;
  A.sigma = sigma;
  A.status = status;
  A.nv = n_outer * grid;
  A.s1 = s1;
  A.s2 = s2;
  A.s3 = s3;
  A.p1 = p1;
  A.p2 = p2;
  A.p3 = p3;
  A.P = (int)P;
  A.N = N;
  A.rank_in = rank;
  A.is_c128 = dt_code == XM_C128;
  A.stop = stop;
  A.counter = (unsigned*)workspace;

  DeviceGuard guard(x);
  hipStream_t st = (hipStream_t)stream;
  if ((dtype & XM_DENOISE_GRAM_FMA) || P < 8) return dn_launch<XM_DN_FORM_FMA>(A, st);  // below 8 rows a 16-row block would be mostly padding
  return dn_launch<XM_DN_FORM_MFMA>(A, st);
}
