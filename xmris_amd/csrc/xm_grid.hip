// Host side of xm_axis_sparse (include/xmris_hip.h); the kernel is in xm_grid.h.
#include "xm_host.h"
#include "xm_grid.h"

#include <string>

static int sparse_fail(const std::string& msg) { return xm_fail(XM_ERR_INVALID_ARG, "axis_sparse: " + msg); }

namespace {
struct SparsePtrs {
  const void* x;
  void* y;
  const int32_t *rowptr, *col;
  const double* val;
};

template <class S, int VEC>
int sparse_launch(const SparsePtrs& P, AxisSparseArgs A, int64_t n_outer, hipStream_t st) {
  A.n_slices = (unsigned)(n_outer * A.n_itiles);
  const long long groups = (A.n_rows + XM_SPARSE_ROWS - 1) / XM_SPARSE_ROWS;  // < 2^29
  const long long max_x = 1LL << 20, max_y = 65535;
  A.groups_x = (unsigned)(groups < max_x ? groups : max_x);
  const unsigned runs = (unsigned)((groups + A.groups_x - 1) / A.groups_x);  // <= 2^9
  const long long rounds = ((long long)A.n_slices + XM_SPARSE_XCDS - 1) / XM_SPARSE_XCDS;
  xm_note_kernel("k_axis_sparse", nullptr, sizeof(S) == 4 ? "c64" : "c128", VEC, -1);  // <dtype, elements per lane>
  for (long long r0 = 0; r0 < rounds; r0 += max_y) {  // (one launch unless there are more than 524,280 slices)
    const long long ny = rounds - r0 < max_y ? rounds - r0 : max_y;
    A.round0 = (unsigned)r0;
    hipLaunchKernelGGL((k_axis_sparse<S, VEC>), dim3(A.groups_x * XM_SPARSE_XCDS, (unsigned)ny, runs),
                       dim3(XM_SPARSE_NT), 0, st, P.x, P.y, P.rowptr, P.col, P.val, A);
    HIP_TRY(hipGetLastError());
  }
  return XM_OK;
}
}  // namespace

extern "C" int xm_axis_sparse(const void* x, void* y, const int32_t* rowptr, const int32_t* col, const double* val,
                              int64_t n_outer, int64_t n, int64_t n_rows, int64_t n_inner, int dtype, void* stream) {
  if (dtype != XM_C64 && dtype != XM_C128) return sparse_fail("unknown dtype " + std::to_string(dtype));
  if (n < 1 || n >= (1LL << 31)) return sparse_fail("n must be in 1 ... 2^31 - 1");
  if (n_rows < 1 || n_rows >= (1LL << 31)) return sparse_fail("n_rows must be in 1 ... 2^31 - 1");
  if (n_outer < 0 || n_inner < 0) return sparse_fail("needs n_outer >= 0 and n_inner >= 0");
  if (!x || !y || !rowptr || !col || !val) return sparse_fail("null pointer");
  if (x == y) return sparse_fail("y must not be x");
  const size_t elem = dtype == XM_C64 ? 8 : 16;
  if ((reinterpret_cast<size_t>(x) | reinterpret_cast<size_t>(y)) & (elem - 1))
    return sparse_fail("x and y must be aligned to their element size");
  const int64_t longest = n > n_rows ? n : n_rows;
  if (n_outer > 0 && n_inner > 0 && (n_inner > (1LL << 50) / n_outer || n_outer * n_inner > (1LL << 50) / longest))
    return sparse_fail("too many elements (> 2^50)");
  if (n_outer == 0 || n_inner == 0) return XM_OK;
  // two complex64 per lane where every row of x and y starts on a 16-byte boundary
  const bool wide = dtype == XM_C64 && n_inner % 2 == 0 &&
                    ((reinterpret_cast<size_t>(x) | reinterpret_cast<size_t>(y)) & 15) == 0;
  const int64_t tile = XM_WAVE * (wide ? 2 : 1);
  const int64_t n_itiles = (n_inner + tile - 1) / tile;
  if (n_itiles > ((1LL << 31) - 1) / n_outer) return sparse_fail("too many (outer, inner tile) slices (> 2^31 - 1)");

  AxisSparseArgs A{};
  A.n = n;
  A.n_rows = n_rows;
  A.n_inner = n_inner;
  A.n_itiles = (unsigned)n_itiles;
  const SparsePtrs P{x, y, rowptr, col, val};

  DeviceGuard guard(x);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == XM_C128) return sparse_launch<double, 1>(P, A, n_outer, st);
  return wide ? sparse_launch<float, 2>(P, A, n_outer, st) : sparse_launch<float, 1>(P, A, n_outer, st);
}
