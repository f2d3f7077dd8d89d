// Host side of xm_species_separate (include/xmris_hip.h); the kernel is in xm_species.h.
#include "xm_host.h"
#include "xm_species.h"

#include <string>

static int sp_fail(const std::string& msg) { return xm_fail(XM_ERR_INVALID_ARG, "species_separate: " + msg); }

namespace {
template <bool FIT, bool C128>
int sp_launch(const SpeciesArgs& A, long long blocks, hipStream_t st) {
  const size_t lds = sp_lds_bytes(A.E, A.M, FIT);
  if (lds > 48 * 1024)
    HIP_TRY(hipFuncSetAttribute((const void*)k_species<FIT, C128>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  xm_note_kernel("k_species", nullptr, FIT ? "fit" : "known", A.E, A.M);  // <form, E, M>
  hipLaunchKernelGGL((k_species<FIT, C128>), dim3((unsigned)blocks), dim3(XM_SP_NT), lds, st, A);
  HIP_TRY(hipGetLastError());
  return XM_OK;
}
}  // namespace

extern "C" int xm_species_separate(const void* x, void* y, const int64_t* dims, const int64_t* x_strides,
                                   const int64_t* y_strides, int n_echoes, int n_species, const double* tables,
                                   const double* tau, int64_t tau_s0, int64_t tau_s1, const double* psi, int64_t psi_s0,
                                   int64_t psi_s1, double* field, double* residual, int32_t* status, int fit,
                                   double max_field, double span, int dtype, void* stream) {
  const int skip = (dtype >> 8) & 15, dt_code = dtype & 0xff;
  const int E = n_echoes, M = n_species;
  if (dt_code != XM_C64 && dt_code != XM_C128 || (dtype & ~0xfff)) return sp_fail("unknown dtype " + std::to_string(dtype));
  if (E < 2 || E > XM_SP_MAXE) return sp_fail("needs 2 ... 32 echoes");
  if (fit && E > XM_SP_MAXE_FIT) return sp_fail("the field fit takes at most 16 echoes");
  if (M < 1 || M > XM_SP_MAXM) return sp_fail("needs 1 ... 8 species");
  if (M > E) return sp_fail("more species than echoes");
  if (fit && M >= E) return sp_fail("the field fit needs fewer species than echoes");
  if (!dims || !x_strides || !y_strides) return sp_fail("null pointer");
  if (dims[0] < 0 || dims[1] < 0 || dims[2] < 1 || dims[3] < 1) return sp_fail("needs row sizes >= 0 and column sizes >= 1");
  if (!x || !y || !tables || !field || !status || (fit && !residual)) return sp_fail("null pointer");
  double delta = 0.0, gd = 0.0;
  if (fit) {
    if (!(max_field > 0.0) || !std::isfinite(max_field)) return sp_fail("max_field must be finite and positive");
    if (!(span > 0.0) || !std::isfinite(span)) return sp_fail("the echo span must be finite and positive");
    delta = 1.0 / (4.0 * span);
    gd = std::floor(max_field / delta);
    if (!(2.0 * gd + 1.0 <= (double)XM_SP_MAXGRID))
      return sp_fail("the coarse grid 2 G + 1, G = floor(4 span max_field), must not exceed 1025 points (max_field)");
  }
  const long long tiles1 = (dims[1] + XM_SP_ROWS - 1) / XM_SP_ROWS;
  if (dims[0] > 0 && tiles1 > 0x7fffffffLL / dims[0]) return sp_fail("too many rows (> 2^31 - 1 tiles of 64)");
  const long long blocks = dims[0] * tiles1;
  if (blocks == 0) return XM_OK;

  SpeciesArgs A{};
  A.x = x;
  A.y = y;
  A.tab = tables;
  A.tau = tau;
  A.psi = fit ? nullptr : psi;
  A.field = field;
  A.residual = residual;
  A.status = status;
  A.nr0 = dims[0];
  A.nr1 = dims[1];
  A.nc0 = dims[2];
  A.nc1 = dims[3];
  A.xs_r0 = x_strides[0], A.xs_r1 = x_strides[1], A.xs_c0 = x_strides[2], A.xs_c1 = x_strides[3], A.xs_e = x_strides[4];
  A.ys_r0 = y_strides[0], A.ys_r1 = y_strides[1], A.ys_c0 = y_strides[2], A.ys_c1 = y_strides[3], A.ys_m = y_strides[4];
  A.tau_s0 = tau_s0, A.tau_s1 = tau_s1, A.psi_s0 = psi_s0, A.psi_s1 = psi_s1;
  A.tiles1 = tiles1;
  A.E = E;
  A.M = M;
  A.NP = fit ? E * (E - 1) / 2 : 0;
  A.G = (int)gd;
  A.is_c128 = dt_code == XM_C128;
  A.skip = skip;
  A.delta = delta;
  A.max_field = max_field;

  DeviceGuard guard(x);
  hipStream_t st = (hipStream_t)stream;
  if (A.is_c128) return fit ? sp_launch<true, true>(A, blocks, st) : sp_launch<false, true>(A, blocks, st);
  return fit ? sp_launch<true, false>(A, blocks, st) : sp_launch<false, false>(A, blocks, st);
}
