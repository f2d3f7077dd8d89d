// Host side of xm_cgs_expand / xm_cgs_reduce / xm_cgs_step (include/xmris_hip.h); the kernels are in xm_cgsense.h.
#include "xm_host.h"
#include "xm_cgsense.h"

#include <initializer_list>
#include <string>

namespace {
int cgs_fail(const char* who, const std::string& msg) { return xm_fail(XM_ERR_INVALID_ARG, std::string(who) + ": " + msg); }

struct Ptr {
  const void* p;
  size_t align;
};

// sizes in 1 ... 2^31 - 1, at most 2^50 elements, non-null pointers aligned to their element, no output among the
// inputs or twice among the outputs
int cgs_check(const char* who, int64_t C, int64_t V, int64_t T, std::initializer_list<Ptr> in, std::initializer_list<Ptr> out) {
  const int64_t top = (1LL << 31) - 1;
  if (C < 1 || C > top || V < 1 || V > top || T < 1 || T > top)
    return cgs_fail(who, "n_coils, n_vox and n_cols must be in 1 ... 2^31 - 1");
  if (V > (1LL << 50) / C || C * V > (1LL << 50) / T) return cgs_fail(who, "too many elements (> 2^50)");
  for (const std::initializer_list<Ptr>* l : {&in, &out})
    for (const Ptr& a : *l) {
      if (!a.p) return cgs_fail(who, "null pointer");
      if (reinterpret_cast<size_t>(a.p) & (a.align - 1)) return cgs_fail(who, "a pointer is not aligned to its element size");
    }
  for (const Ptr& o : out) {
    int same = 0;
    for (const Ptr& a : in) same += a.p == o.p;
    for (const Ptr& a : out) same += a.p == o.p;
    if (same != 1) return cgs_fail(who, "an output aliases an input or another output");
  }
  return XM_OK;
}

CgsArgs cgs_args(int64_t C, int64_t V, int64_t T) {
  CgsArgs A{};
  A.n_coils = (int)C;
  A.n_vox = V;
  A.n_cols = T;
  A.n_blocks = (unsigned)((V + XM_CGS_VOXELS - 1) / XM_CGS_VOXELS);
  return A;
}

// two complex64 per lane where every row of u starts on a 16-byte boundary
bool cgs_wide(const void* u, int64_t T, int dtype) {
  return dtype == XM_C64 && T % 2 == 0 && (reinterpret_cast<size_t>(u) & 15) == 0;
}

// f(grid, A) once per run of at most 65535 column tiles of `per_tile` columns (one launch up to 4 million columns)
template <class F>
int cgs_tiles(CgsArgs A, int per_tile, F&& f) {
  const long long tiles = (A.n_cols + per_tile - 1) / per_tile, max_y = 65535;
  const unsigned gx = (A.n_blocks + XM_CGS_ITEMS - 1) / XM_CGS_ITEMS;  // < 2^26
  for (long long y0 = 0; y0 < tiles; y0 += max_y) {
    A.tile0 = (unsigned)y0;
    f(dim3(gx, (unsigned)(tiles - y0 < max_y ? tiles - y0 : max_y)), A);
    HIP_TRY(hipGetLastError());
  }
  return XM_OK;
}
}  // namespace

extern "C" int xm_cgs_expand(const void* r, void* p, const void* s, void* u, const double* rho_new, const double* rho_old,
                             const int32_t* status, int64_t n_coils, int64_t n_vox, int64_t n_cols, int first, int dtype,
                             void* stream) {
  const char* who = "cgs_expand";
  if (dtype != XM_C64 && dtype != XM_C128) return cgs_fail(who, "unknown dtype " + std::to_string(dtype));
  const size_t elem = dtype == XM_C64 ? 8 : 16;
  if (const int rc = cgs_check(who, n_coils, n_vox, n_cols, {{r, 16}, {s, 16}, {rho_new, 8}, {rho_old, 8}, {status, 4}},
                               {{p, 16}, {u, elem}}))
    return rc;
  CgsArgs A = cgs_args(n_coils, n_vox, n_cols);
  A.mode = first != 0;
  const Cx<double>* rr = static_cast<const Cx<double>*>(r);
  Cx<double>* pp = static_cast<Cx<double>*>(p);
  const Cx<double>* ss = static_cast<const Cx<double>*>(s);
  DeviceGuard guard(u);
  hipStream_t st = (hipStream_t)stream;
  const bool wide = cgs_wide(u, n_cols, dtype);
  xm_note_kernel("k_cgs_expand", nullptr, dtype == XM_C64 ? "c64" : "c128", wide ? 2 : 1, -1);
  return cgs_tiles(A, XM_WAVE * (wide ? 2 : 1), [&](dim3 grid, const CgsArgs& B) {
    if (dtype == XM_C128)
      hipLaunchKernelGGL((k_cgs_expand<double, 1>), grid, dim3(XM_CGS_NT), 0, st, rr, pp, ss, u, rho_new, rho_old, status, B);
    else if (wide)
      hipLaunchKernelGGL((k_cgs_expand<float, 2>), grid, dim3(XM_CGS_NT), 0, st, rr, pp, ss, u, rho_new, rho_old, status, B);
    else
      hipLaunchKernelGGL((k_cgs_expand<float, 1>), grid, dim3(XM_CGS_NT), 0, st, rr, pp, ss, u, rho_new, rho_old, status, B);
  });
}

extern "C" int xm_cgs_reduce(const void* u, const void* s, const void* p, void* q, double* part, int64_t n_coils,
                             int64_t n_vox, int64_t n_cols, double lambda, int initial, int dtype, void* stream) {
  const char* who = "cgs_reduce";
  if (dtype != XM_C64 && dtype != XM_C128) return cgs_fail(who, "unknown dtype " + std::to_string(dtype));
  if (!initial && !(lambda >= 0.0 && std::isfinite(lambda))) return cgs_fail(who, "lambda must be finite and >= 0");
  const size_t elem = dtype == XM_C64 ? 8 : 16;
  if (initial) p = s;  // (not read)
  if (const int rc = cgs_check(who, n_coils, n_vox, n_cols, {{u, elem}, {s, 16}, {p, 16}}, {{q, 16}, {part, 8}})) return rc;
  CgsArgs A = cgs_args(n_coils, n_vox, n_cols);
  A.mode = initial != 0;
  A.lambda = lambda;
  const Cx<double>* ss = static_cast<const Cx<double>*>(s);
  const Cx<double>* pp = static_cast<const Cx<double>*>(p);
  Cx<double>* qq = static_cast<Cx<double>*>(q);
  DeviceGuard guard(u);
  hipStream_t st = (hipStream_t)stream;
  const bool wide = cgs_wide(u, n_cols, dtype);
  xm_note_kernel("k_cgs_reduce", nullptr, dtype == XM_C64 ? "c64" : "c128", wide ? 2 : 1, -1);
  return cgs_tiles(A, XM_WAVE * (wide ? 2 : 1), [&](dim3 grid, const CgsArgs& B) {
    if (dtype == XM_C128)
      hipLaunchKernelGGL((k_cgs_reduce<double, 1>), grid, dim3(XM_CGS_NT), 0, st, u, ss, pp, qq, part, B);
    else if (wide)
      hipLaunchKernelGGL((k_cgs_reduce<float, 2>), grid, dim3(XM_CGS_NT), 0, st, u, ss, pp, qq, part, B);
    else
      hipLaunchKernelGGL((k_cgs_reduce<float, 1>), grid, dim3(XM_CGS_NT), 0, st, u, ss, pp, qq, part, B);
  });
}

extern "C" int xm_cgs_step(void* x, void* r, const void* p, const void* q, const double* rho, const double* rho0,
                           const double* delta, double* rho_out, const int32_t* status_in, int32_t* status_out,
                           int32_t* n_iter, double* residual, int64_t n_vox, int64_t n_cols, double tol, int iteration,
                           int final_test, void* stream) {
  const char* who = "cgs_step";
  if (!(tol >= 0.0 && std::isfinite(tol))) return cgs_fail(who, "tol must be finite and >= 0");
  if (iteration < 0) return cgs_fail(who, "iteration must be >= 0");
  if (final_test) delta = rho0;  // (not read)
  // (rho is rho0 itself in the first step: the inputs may repeat one another, the outputs may not)
  if (const int rc = cgs_check(who, 1, n_vox, n_cols, {{p, 16}, {q, 16}, {rho, 8}, {rho0, 8}, {delta, 8}, {status_in, 4}},
                               {{x, 16}, {r, 16}, {rho_out, 8}, {status_out, 4}, {n_iter, 4}, {residual, 8}}))
    return rc;
  CgsArgs A = cgs_args(1, n_vox, n_cols);
  A.mode = final_test != 0;
  A.iteration = iteration;
  const double floor_ = tol > 1e-14 ? tol : 1e-14;
  A.tol2 = floor_ * floor_;
  DeviceGuard guard(x);
  hipStream_t st = (hipStream_t)stream;
  xm_note_kernel("k_cgs_step", nullptr, "c128", 1, -1);
  return cgs_tiles(A, XM_WAVE, [&](dim3 grid, const CgsArgs& B) {
    hipLaunchKernelGGL(k_cgs_step, grid, dim3(XM_CGS_NT), 0, st, static_cast<Cx<double>*>(x), static_cast<Cx<double>*>(r),
                       static_cast<const Cx<double>*>(p), static_cast<const Cx<double>*>(q), rho, rho0, delta, rho_out,
                       status_in, status_out, n_iter, residual, B);
  });
}
