// Host side of xm_axis_dft (include/xmris_hip.h); the kernel is in xm_mrsi.h.
#include "xm_host.h"
#include "xm_mrsi.h"

#include <string>

static int dft_fail(const std::string& msg) { return xm_fail(XM_ERR_INVALID_ARG, "axis_dft: " + msg); }

namespace {
template <class S, int PT>
int dft_launch(const AxisDftArgs& A, hipStream_t st) {
  const size_t lds = (size_t)A.n * XM_DFT_TILE * sizeof(Cx<S>);
  static XmResidency res;  // one residency record per kernel instantiation
  int resident = 0;
  const int rc = xm_resident_blocks(res, k_axis_dft<S, PT>, XM_DFT_NT, lds, &resident, st);
  if (rc) return rc;
  // a few tiles per resident workgroup at most: the grid-stride loop takes the rest
  const long long cap = 8LL * resident;
  const long long blocks = A.n_tiles < cap ? A.n_tiles : cap;
  xm_note_kernel("k_axis_dft", nullptr, sizeof(S) == 4 ? "c64" : "c128", PT, -1);  // <dtype, outputs per wave>
  hipLaunchKernelGGL((k_axis_dft<S, PT>), dim3((unsigned)blocks), dim3(XM_DFT_NT), lds, st, A);
  HIP_TRY(hipGetLastError());
  return XM_OK;
}

template <class S>
int dft_dispatch(const AxisDftArgs& A, hipStream_t st) {
  if (A.m <= 16) return dft_launch<S, 4>(A, st);
  if (A.m <= 32) return dft_launch<S, 8>(A, st);
  return dft_launch<S, 16>(A, st);
}
}  // namespace

extern "C" int xm_axis_dft(const void* x, void* y, const void* table, int64_t n_outer, int n, int m, int64_t n_inner,
                           int dtype, void* stream) {
  if (dtype != XM_C64 && dtype != XM_C128) return dft_fail("unknown dtype " + std::to_string(dtype));
  if (n < 1 || n > XM_DFT_MAX || m < 1 || m > XM_DFT_MAX) return dft_fail("n and m must be in 1 ... 64");
  if (n_outer < 0 || n_inner < 0) return dft_fail("needs n_outer >= 0 and n_inner >= 0");
  if (!x || !y || !table) return dft_fail("null pointer");
  if (x == y) return dft_fail("y must not be x");
  if (n_outer > 0 && n_inner > (1LL << 50) / n_outer) return dft_fail("too many pencils (> 2^50)");
  if (n_outer == 0 || n_inner == 0) return XM_OK;

  AxisDftArgs A{};
  A.x = x;
  A.y = y;
  A.table = static_cast<const double*>(table);
  A.n_pencils = n_outer * n_inner;
  A.n_inner = n_inner;
  A.n_tiles = (A.n_pencils + XM_DFT_TILE - 1) / XM_DFT_TILE;
  A.n = n;
  A.m = m;

  DeviceGuard guard(x);
  hipStream_t st = (hipStream_t)stream;
  return dtype == XM_C64 ? dft_dispatch<float>(A, st) : dft_dispatch<double>(A, st);
}
