// Host side of xm_sub_project / xm_sub_mix / xm_sub_expand (include/xmris_hip.h); the kernels are in xm_subspace.h.
#include "xm_host.h"
#include "xm_subspace.h"

#include <initializer_list>
#include <string>

namespace {
int sub_fail(const char* who, const std::string& msg) { return xm_fail(XM_ERR_INVALID_ARG, std::string(who) + ": " + msg); }

const int64_t kTop = (1LL << 31) - 1, kMost = 1LL << 50;

// every size in 1 ... 2^31 - 1 and their product at most 2^50
int sub_sizes(const char* who, std::initializer_list<int64_t> sizes) {
  int64_t total = 1;
  for (const int64_t n : sizes) {
    if (n < 1 || n > kTop) return sub_fail(who, "every size must be in 1 ... 2^31 - 1");
    if (total > kMost / n) return sub_fail(who, "too many elements (> 2^50)");
    total *= n;
  }
  return XM_OK;
}

int sub_rank(const char* who, int rank) {
  if (rank < 1 || rank > XM_SUB_MAX_RANK) return sub_fail(who, "needs rank 1 ... " + std::to_string(XM_SUB_MAX_RANK));
  return XM_OK;
}

bool sub_misaligned(const void* p, size_t align) { return (reinterpret_cast<size_t>(p) & (align - 1)) != 0; }

bool sub_overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
  const char* a0 = static_cast<const char*>(a);
  const char* b0 = static_cast<const char*>(b);
  return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

template <class K, class Args>
int sub_launch(K kern, dim3 grid, size_t lds, hipStream_t st, const char* name, const char* form, int mode, int opt,
               const Args& A) {
  if (lds > 48 * 1024) HIP_TRY(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  xm_note_kernel(name, nullptr, form, mode, opt);
  hipLaunchKernelGGL(kern, grid, dim3(XM_SUB_NT), lds, st, A);
  HIP_TRY(hipGetLastError());
  return XM_OK;
}
}  // namespace

extern "C" int xm_sub_project(const void* y, void* b, const void* basis, const uint8_t* sampling, int64_t n_coils,
                              int64_t n_samples, int64_t n_frames, int64_t n_time, int rank, int64_t coil_stride,
                              int64_t sample_stride, int64_t frame_stride, int dtype, void* stream) {
  const char* who = "sub_project";
  if (dtype != XM_C64 && dtype != XM_C128) return sub_fail(who, "unknown dtype " + std::to_string(dtype));
  if (const int rc = sub_rank(who, rank)) return rc;
  if (const int rc = sub_sizes(who, {n_coils, n_samples, n_frames, n_time})) return rc;
  if (const int rc = sub_sizes(who, {n_coils, n_samples, n_frames, (int64_t)rank})) return rc;
  if (rank > n_time) return sub_fail(who, "needs rank <= n_time");
  if (!y || !b || !basis) return sub_fail(who, "null pointer");
  const size_t elem = dtype == XM_C64 ? 8 : 16;
  if (sub_misaligned(y, elem) || sub_misaligned(b, elem) || sub_misaligned(basis, 16))
    return sub_fail(who, "a pointer is not aligned to its element size");
  if (coil_stride < 0 || sample_stride < 0 || frame_stride < 0) return sub_fail(who, "the strides must be >= 0");
  // the extent of y, in elements: at most 2^50 as well
  int64_t extent = n_time;
  const int64_t dims[3] = {n_coils, n_samples, n_frames}, strides[3] = {coil_stride, sample_stride, frame_stride};
  for (int a = 0; a < 3; ++a) {
    if (dims[a] > 1 && strides[a] > (kMost - extent) / (dims[a] - 1)) return sub_fail(who, "the strides reach too far (> 2^50 elements)");
    extent += (dims[a] - 1) * strides[a];
  }
  const size_t y_bytes = (size_t)extent * elem, b_bytes = (size_t)(n_coils * n_samples * rank * n_frames) * elem;
  const size_t v_bytes = (size_t)rank * n_time * 16, m_bytes = (size_t)(n_samples * n_time);
  if (sub_overlap(b, b_bytes, y, y_bytes) || sub_overlap(b, b_bytes, basis, v_bytes) ||
      (sampling && sub_overlap(b, b_bytes, sampling, m_bytes)))
    return sub_fail(who, "the output overlaps an input");

  SubProjectArgs A{};
  A.y = y, A.b = b, A.basis = static_cast<const double2*>(basis), A.m = sampling;
  A.n_rows = n_coils * n_samples * n_frames;
  A.cs = coil_stride, A.ss = sample_stride, A.fs = frame_stride;
  A.S = n_samples, A.F = n_frames, A.C = (int)n_coils, A.T = (int)n_time, A.R = rank;
  const int64_t blocks = (A.n_rows + XM_SP_ROWS - 1) / XM_SP_ROWS;
  if (blocks > kTop) return sub_fail(who, "too many rows (> 2^31 - 1 tiles of 16)");
  const size_t lds = (size_t)(XM_SP_ROWS + rank) * XM_SP_PITCH * sizeof(double2);
  DeviceGuard guard(y);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)blocks);
  const char* form = dtype == XM_C64 ? "c64" : "c128";
  const int nr = rank <= 16 ? 1 : 2;
  if (dtype == XM_C128)
    return nr == 1 ? sub_launch(k_sub_project<true, 1>, grid, lds, st, "k_sub_project", form, nr, rank, A)
                   : sub_launch(k_sub_project<true, 2>, grid, lds, st, "k_sub_project", form, nr, rank, A);
  return nr == 1 ? sub_launch(k_sub_project<false, 1>, grid, lds, st, "k_sub_project", form, nr, rank, A)
                 : sub_launch(k_sub_project<false, 2>, grid, lds, st, "k_sub_project", form, nr, rank, A);
}

extern "C" int xm_sub_mix(const void* a, void* z, const void* kernel, int64_t n_coils, int64_t n_samples, int64_t n_frames,
                          int rank, int dtype, void* stream) {
  const char* who = "sub_mix";
  if (dtype != XM_C64 && dtype != XM_C128) return sub_fail(who, "unknown dtype " + std::to_string(dtype));
  if (const int rc = sub_rank(who, rank)) return rc;
  if (const int rc = sub_sizes(who, {n_coils, n_samples, n_frames, (int64_t)rank})) return rc;
  if (const int rc = sub_sizes(who, {n_samples, (int64_t)rank, (int64_t)rank})) return rc;
  if (!a || !z || !kernel) return sub_fail(who, "null pointer");
  const size_t elem = dtype == XM_C64 ? 8 : 16;
  if (sub_misaligned(a, elem) || sub_misaligned(z, elem) || sub_misaligned(kernel, 16))
    return sub_fail(who, "a pointer is not aligned to its element size");
  const size_t bytes = (size_t)(n_coils * n_samples * rank * n_frames) * elem, k_bytes = (size_t)(n_samples * rank * rank) * 16;
  if ((a != z && sub_overlap(z, bytes, a, bytes)) || sub_overlap(z, bytes, kernel, k_bytes))
    return sub_fail(who, "the output overlaps an input (only z == a is allowed)");

  SubMixArgs A{};
  A.a = a, A.z = z, A.K = static_cast<const double2*>(kernel);
  A.S = n_samples, A.F = n_frames, A.n_cols = n_coils * n_frames, A.R = rank;
  const int64_t tiles = (A.n_cols + XM_SM_COLS - 1) / XM_SM_COLS;
  if (tiles > kTop / n_samples) return sub_fail(who, "too many work items (> 2^31 - 1)");
  A.tiles = (unsigned)tiles;
  const size_t lds = (size_t)(rank * (rank + 1) + XM_SM_COLS * rank) * sizeof(double2);
  DeviceGuard guard(a);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)(tiles * n_samples));
  if (dtype == XM_C128) return sub_launch(k_sub_mix<true>, grid, lds, st, "k_sub_mix", "c128", a == z, rank, A);
  return sub_launch(k_sub_mix<false>, grid, lds, st, "k_sub_mix", "c64", a == z, rank, A);
}

extern "C" int xm_sub_expand(const void* u, const void* basis, void* x, int64_t n_vox, int64_t n_frames, int64_t n_time,
                             int rank, void* stream) {
  const char* who = "sub_expand";
  if (const int rc = sub_rank(who, rank)) return rc;
  if (const int rc = sub_sizes(who, {n_vox, n_frames, n_time})) return rc;
  if (const int rc = sub_sizes(who, {n_vox, n_frames, (int64_t)rank})) return rc;
  if (rank > n_time) return sub_fail(who, "needs rank <= n_time");
  if (!u || !basis || !x) return sub_fail(who, "null pointer");
  if (sub_misaligned(u, 16) || sub_misaligned(basis, 16) || sub_misaligned(x, 16))
    return sub_fail(who, "a pointer is not aligned to its element size");
  const size_t x_bytes = (size_t)(n_vox * n_frames * n_time) * 16;
  if (sub_overlap(x, x_bytes, u, (size_t)(n_vox * n_frames * rank) * 16) || sub_overlap(x, x_bytes, basis, (size_t)rank * n_time * 16))
    return sub_fail(who, "the output overlaps an input");

  SubExpandArgs A{};
  A.U = static_cast<const double2*>(u), A.basis = static_cast<const double2*>(basis), A.x = static_cast<double2*>(x);
  A.n_rows = n_vox * n_frames, A.F = n_frames, A.T = (int)n_time, A.R = rank;
  const int64_t gx = (A.n_rows + XM_SE_ROWS - 1) / XM_SE_ROWS, gy = (n_time + XM_SUB_NT - 1) / XM_SUB_NT;
  if (gx > kTop) return sub_fail(who, "too many rows (> 2^31 - 1 tiles of 4)");
  if (gy > 65535) return sub_fail(who, "n_time must be at most 65535 tiles of 256 points");
  DeviceGuard guard(u);
  return sub_launch(k_sub_expand, dim3((unsigned)gx, (unsigned)gy), 0, (hipStream_t)stream, "k_sub_expand", "c128", 1, rank, A);
}
