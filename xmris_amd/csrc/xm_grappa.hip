// Host side of xm_grappa_fill (include/xmris_hip.h); the kernel is in xm_grappa.h.
#include "xm_host.h"
#include "xm_grappa.h"

#include <string>

static int gr_fail(const std::string& msg) { return xm_fail(XM_ERR_INVALID_ARG, "grappa_fill: " + msg); }

namespace {
template <class T, int CB, int TP>
int gr_launch(const GrappaArgs& A, hipStream_t st) {
  const unsigned gy = (unsigned)((A.nitems + A.gx - 1) / A.gx);  // at most 65535
  xm_note_kernel("k_grappa_fill", nullptr, sizeof(T) == 8 ? "c128" : "c64", CB, TP);  // <dtype, coil block, points per lane>
  hipLaunchKernelGGL((k_grappa_fill<T, CB, TP>), dim3(A.gx, gy), dim3(XM_GR_NT), 0, st, A);
  HIP_TRY(hipGetLastError());
  return XM_OK;
}

template <class T, int TP>
int gr_dispatch(const GrappaArgs& A, int cb, hipStream_t st) {
  switch (cb) {
    case 1: return gr_launch<T, 1, TP>(A, st);
    case 2: return gr_launch<T, 2, TP>(A, st);
    case 4: return gr_launch<T, 4, TP>(A, st);
    case 8: return gr_launch<T, 8, TP>(A, st);
    default: return gr_launch<T, 16, TP>(A, st);
  }
}

// Output coils per workgroup: 1 and 2 coils as they are; otherwise of 4, 8 and 16 the size that pads C the least (a block
// short of coils repeats its last row), the larger one on a tie: 12 coils run as 3 x 4, 20 as 5 x 4, 24 as 3 x 8.
int gr_coil_block(int C) {
  if (C <= 2) return C;
  int best = 4;
  for (int cb = 8; cb <= XM_GR_CB; cb *= 2)
    if ((C + cb - 1) / cb * cb <= (C + best - 1) / best * best) best = cb;
  return best;
}
}  // namespace

extern "C" int xm_grappa_fill(const void* a, void* y, const void* weights, int64_t n_outer, int C, const int32_t n[3],
                              const int32_t accel[3], const int32_t kernel[3], int N_t, const int64_t a_strides[5],
                              const int64_t y_strides[5], int dtype, void* stream) {
  if (!a || !y || !n || !accel || !kernel || !a_strides || !y_strides) return gr_fail("null pointer");
  if (C < 1 || C > XM_GR_MAXC) return gr_fail("C must be in 1 ... 64");
  long long R = 1, S = 1, npos = 1;
  for (int d = 0; d < 3; ++d) {
    if (accel[d] < 1) return gr_fail("every accel must be at least 1");
    if (kernel[d] < 1) return gr_fail("every kernel size must be at least 1");
    if (n[d] < 1) return gr_fail("every n must be at least 1");
    R *= accel[d];
    if (R > XM_GR_MAXR) return gr_fail("R = the product of accel must not exceed 16");
    S *= kernel[d];
    if (S > XM_GR_MAXS) return gr_fail("S = the product of kernel must not exceed 64");
    npos *= (long long)accel[d] * n[d];
    if (npos > 0x7fffffffLL) return gr_fail("too many positions (> 2^31 - 1)");
  }
  if (S * C > XM_GR_MAXK) return gr_fail("C S must not exceed 1024");
  if (N_t < 1) return gr_fail("needs N_t >= 1");
  if (dtype != XM_C64 && dtype != XM_C128) return gr_fail("unknown dtype " + std::to_string(dtype));
  if (y == a) return gr_fail("y must not be a");
  if (n_outer < 0) return gr_fail("needs n_outer >= 0");
  if (R > 1 && !weights) return gr_fail("weights may be NULL at R = 1 only");
  bool pair = dtype == XM_C64 && N_t % 2 == 0 && (((size_t)a | (size_t)y) & 15u) == 0;
  for (int d = 0; d < 5; ++d) pair = pair && a_strides[d] % 2 == 0 && y_strides[d] % 2 == 0;
  // work items: (outer, position, block of output coils, time tile), the blocks and tiles of the kernel that will run
  const int cb = gr_coil_block(C), tile = XM_GR_NT * (pair ? 2 : 1);
  const long long ncb = (C + cb - 1) / cb, ntiles = ((long long)N_t + tile - 1) / tile;
  if (n_outer > 0x7fff0000LL / npos || n_outer * npos > 0x7fff0000LL / (ncb * ntiles))
    return gr_fail("too many work items (> 2^31 - 2^16)");  // a grid of 32768 x at most 65535 workgroups
  if (n_outer == 0) return XM_OK;

  GrappaArgs A{};
  A.a = a;
  A.y = y;
  A.w = (const double*)weights;
  for (int d = 0; d < 5; ++d) {
    A.as[d] = a_strides[d];
    A.ys[d] = y_strides[d];
  }
  A.npos = npos;
  A.ncb = (int)ncb;
  A.ntiles = (int)ntiles;
  A.nitems = n_outer * npos * ncb * ntiles;
  A.gx = (unsigned)(A.nitems < 32768 ? A.nitems : 32768);
  A.C = C;
  for (int d = 0; d < 3; ++d) {
    A.n[d] = n[d];
    A.R[d] = accel[d];
    A.b[d] = kernel[d];
  }
  A.Nt = N_t;
  A.S = (int)S;

  DeviceGuard guard(a);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == XM_C128) return gr_dispatch<double, 1>(A, cb, st);
  return pair ? gr_dispatch<float, 2>(A, cb, st) : gr_dispatch<float, 1>(A, cb, st);
}
