// Host side of xm_lipid_project (include/xmris_hip.h); the kernel is in xm_lipids.h.
#include "xm_host.h"
#include "xm_lipids.h"

#include <string>

static int lp_fail(const std::string& msg) { return xm_fail(XM_ERR_INVALID_ARG, "lipid_project: " + msg); }

namespace {
template <bool MFMA, bool C128, int NJ>
int lp_launch_nj(const LipidArgs& A, long long blocks, hipStream_t st) {
  const size_t lds = lp_lds_bytes(A.r);
  if (lds > 48 * 1024)
    HIP_TRY(hipFuncSetAttribute((const void*)k_lipid_project<MFMA, C128, NJ>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  xm_note_kernel("k_lipid_project", nullptr, MFMA ? "mfma" : "fma", A.T, A.r);  // <form, T, rank>
  hipLaunchKernelGGL((k_lipid_project<MFMA, C128, NJ>), dim3((unsigned)blocks), dim3(XM_LP_NT), lds, st, A);
  HIP_TRY(hipGetLastError());
  return XM_OK;
}

// the rank class sizes the registers that hold the next chunk of the table: 16, 32 or 64 columns
template <bool MFMA, bool C128>
int lp_launch(const LipidArgs& A, long long blocks, hipStream_t st) {
  if (A.r <= 16) return lp_launch_nj<MFMA, C128, XM_LP_TC * 16 / XM_LP_NT>(A, blocks, st);
  if (A.r <= 32) return lp_launch_nj<MFMA, C128, XM_LP_TC * 32 / XM_LP_NT>(A, blocks, st);
  return lp_launch_nj<MFMA, C128, XM_LP_TC * 64 / XM_LP_NT>(A, blocks, st);
}
}  // namespace

extern "C" int xm_lipid_project(const void* x, void* y, int64_t n_rows, int64_t x_row_stride, int64_t y_row_stride, int T,
                                int rank, const double* tables, const uint8_t* apply, int32_t* status, int dtype,
                                void* stream) {
  const int flags = (dtype >> 8) & 7, dt_code = dtype & 0xff;
  if (dt_code != XM_C64 && dt_code != XM_C128 || (dtype & ~0x7ff)) return lp_fail("unknown dtype " + std::to_string(dtype));
  if (T < 2 || T > 65536) return lp_fail("needs 2 ... 65536 time points");
  if (rank < 1 || rank > XM_LP_MAXR) return lp_fail("needs rank 1 ... 64");
  if (n_rows < 0) return lp_fail("n_rows must be >= 0");
  if (n_rows == 0) return XM_OK;  // nothing is launched, whatever the pointers hold
  if (!x || !y || !tables || !status) return lp_fail("null pointer");
  if (x_row_stride < T || y_row_stride < T) return lp_fail("the rows must not overlap (row stride >= T)");
  if (reinterpret_cast<size_t>(tables) & 15u) return lp_fail("tables must be 16-byte aligned");
  const size_t esz = dt_code == XM_C128 ? 16 : 8;
  if ((reinterpret_cast<size_t>(x) | reinterpret_cast<size_t>(y)) & (esz - 1)) return lp_fail("x and y must be aligned to an element");
  if (n_rows > 0x7fffffffLL * XM_LP_ROWS) return lp_fail("too many rows (> 2^31 - 1 tiles of 16)");
  if (!(x == y && x_row_stride == y_row_stride)) {  // in place over the same rows, or apart
    const char* xb = (const char*)x;
    const char* yb = (const char*)y;
    const char* xe = xb + ((size_t)(n_rows - 1) * x_row_stride + T) * esz;
    const char* ye = yb + ((size_t)(n_rows - 1) * y_row_stride + T) * esz;
    if (xb < ye && yb < xe) return lp_fail("x and y overlap (only x == y with equal strides is allowed)");
  }

  LipidArgs A{};
  A.x = x;
  A.y = y;
  A.tab = tables;
  A.apply = apply;
  A.status = status;
  A.n_rows = n_rows;
  A.xs = x_row_stride;
  A.ys = y_row_stride;
  A.T = T;
  A.r = rank;
  A.pitch = lp_pitch(rank);
  A.nblk = lp_blocks(rank);
  // complex64: a pair of samples is one aligned 16-byte word when the rows start on one
  A.vec = dt_code == XM_C64 && x_row_stride % 2 == 0 && y_row_stride % 2 == 0 &&
          ((reinterpret_cast<size_t>(x) | reinterpret_cast<size_t>(y)) & 15u) == 0;
  A.skip = flags;
  const long long blocks = (n_rows + XM_LP_ROWS - 1) / XM_LP_ROWS;

  DeviceGuard guard(x);
  hipStream_t st = (hipStream_t)stream;
  const bool mfma = !(flags & XM_LP_FMA);
  if (dt_code == XM_C128) return mfma ? lp_launch<true, true>(A, blocks, st) : lp_launch<false, true>(A, blocks, st);
  return mfma ? lp_launch<true, false>(A, blocks, st) : lp_launch<false, false>(A, blocks, st);
}
