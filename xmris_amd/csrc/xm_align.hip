// Host side of xm_align_rows (include/xmris_hip.h); the kernel is in xm_align.h.
#include "xm_host.h"
#include "xm_align.h"

#include <string>

static int al_fail(const std::string& msg) { return xm_fail(XM_ERR_INVALID_ARG, "align_rows: " + msg); }

namespace {
XmResidency g_al_res[2];  // one residency record per kernel instantiation

template <bool AVERAGE>
int al_launch(const AlignArgs& A, hipStream_t st) {
  return xm_launch_items(g_al_res[AVERAGE], k_align<AVERAGE>, XM_AL_NT, al_lds_bytes(A.L, A.G, A.R), A.nwork, A, st,
                         "k_align", AVERAGE ? "average" : "each", A.L, A.G);  // <form, L, G>
}
}  // namespace

extern "C" int64_t xm_align_workspace_bytes(int64_t n_outer, int A, int64_t n_inner, int N) {
  (void)n_outer, (void)A, (void)n_inner, (void)N;  // the counter pair, whatever the shape
  return XM_ALIGN_WORKSPACE_BYTES;
}

extern "C" int xm_align_rows(const void* x, const void* r, int64_t r_voxel_stride, void* y, void* mean_or_null,
                             double* shift, double* phase, double* quality, int32_t* status,
                             int32_t* n_averaged_or_null, int64_t n_outer, int A, int64_t n_inner, int N, int N_r, int L,
                             double dt, double t0, double max_shift, double min_quality, int dtype, void* workspace,
                             void* stream) {
  const int skip = (dtype >> 8) & 7, dt_code = dtype & 0xff;
  if (dt_code != XM_C64 && dt_code != XM_C128 || (dtype & ~0x7ff)) return al_fail("unknown dtype " + std::to_string(dtype));
  if (N < 1 || N_r < 1 || A < 1) return al_fail("needs N >= 1, N_r >= 1 and A >= 1");
  if (L < 1) return al_fail("L must be at least 1");
  if (L > N || L > N_r) return al_fail("L must not exceed N or N_r");
  if (L > XM_AL_MAXL) return al_fail("L must not exceed 8192 points (t_max / n_points)");
  if (!(dt > 0.0) || !std::isfinite(dt) || !std::isfinite(t0)) return al_fail("needs a finite dt > 0 and a finite t0");
  if (!(max_shift >= 0.0) || !std::isfinite(max_shift)) return al_fail("max_shift must be finite and not negative");
  if (std::isnan(min_quality)) return al_fail("min_quality is NaN");
  // (one point says nothing about a frequency: no grid)
  const double delta = 1.0 / (4.0 * L * dt), gd = L < 2 ? 0.0 : std::floor(max_shift / delta);
  if (!(2.0 * gd + 1.0 <= (double)XM_AL_MAXGRID))
    return al_fail("the coarse grid 2 G + 1, G = floor(4 L dt max_shift), must not exceed 1025 points (max_shift, t_max)");
  if (n_outer < 0 || n_inner < 0) return al_fail("needs n_outer >= 0 and n_inner >= 0");
  if (r_voxel_stride != 0 && r_voxel_stride < N_r) return al_fail("r_voxel_stride must be 0 (one shared row) or at least N_r");
  if (!x || !r || !shift || !phase || !quality || !status || !workspace) return al_fail("null pointer");
  if (!mean_or_null && !y) return al_fail("y may be null in the averaging form only");
  if (mean_or_null && !n_averaged_or_null) return al_fail("the averaging form needs n_averaged");
  const long long nvox = (long long)n_outer * n_inner;
  if (nvox * A > 0xffffffffLL) return al_fail("too many transients (> 2^32 - 1)");
  if (nvox == 0) return XM_OK;

  AlignArgs P{};
  P.x = x;
  P.r = r;
  P.y = y;
  P.mean = mean_or_null;
  P.shift = shift;
  P.phase = phase;
  P.quality = quality;
  P.status = status;
  P.n_avg = n_averaged_or_null;
  P.nwork = mean_or_null ? nvox : nvox * A;
  P.n_inner = n_inner;
  P.rstride = r_voxel_stride;
  P.A = A;
  P.N = N;
  P.L = L;
  P.G = (int)gd;
  P.is_c128 = dt_code == XM_C128;
  P.skip = skip;
  P.dt = dt;
  P.t0 = t0;
  P.delta = delta;
  P.max_shift = max_shift;
  P.min_quality = min_quality;
  P.counter = (unsigned*)workspace;
  if (mean_or_null) {  // as many points per pass as the LDS has room for next to z
    P.R = (N + XM_AL_NT - 1) / XM_AL_NT < XM_AL_R ? (N + XM_AL_NT - 1) / XM_AL_NT : XM_AL_R;
    while (P.R > 1 && al_lds_bytes(P.L, P.G, P.R) > XM_AL_LDS_MAX) P.R /= 2;
  }

  DeviceGuard guard(x);
  hipStream_t st = (hipStream_t)stream;
  return mean_or_null ? al_launch<true>(P, st) : al_launch<false>(P, st);
}
