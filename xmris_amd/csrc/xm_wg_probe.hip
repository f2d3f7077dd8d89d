// libxmris_wgprobe.so -- test-only probes of the workgroup toolbox (xm_wg.h) and of the normal-equation accumulation of
// the Levenberg-Marquardt driver built on it (xm_lm.h), outside the product library: it is not
// linked into libxmris_hip.so and not declared in include/xmris_hip.h.  Each kernel is one 256-thread workgroup per
// problem: it stages its input in the LDS, calls one toolbox function and copies everything out, so that
// tests/test_gpu_wg.py can hold every part to tests/_wg_oracle.py on its own.  The host side checks its arguments --
// nothing else stands between a test and an LDS overrun -- and returns XM_ERR_INVALID_ARG without a launch.  The complex
// Gram accumulation loops (wg_gram_*) are not restated here: they stay in the users and are tested through them.  The
// real one of the fitting kernels is lm_normal itself, probed below with a model that copies given rows.
#include "../../include/xmris_hip.h"
#include "xm_lm.h"

#define XM_WGP_MAXC 64       // coils, patch voxels, Hankel rows: the largest Hermitian matrix of any user
#define XM_WGP_MAXP XM_LM_MAXP  // XM_BS_MAXP, and AMARES's 5 x 16
#define XM_WGP_MAXN (1 << 20)  // problems per launch

static_assert(XM_WG_NT == 256, "the probes lay their outputs out per 256 threads");

// ---- kernels ---------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(XM_WG_NT) void k_wgp_sum(const double* in, double* out) {
  __shared__ double red[XM_WG_NT];
  const size_t at = (size_t)blockIdx.x * XM_WG_NT + threadIdx.x;
  out[at] = wg_sum(red, in[at]);
}

__global__ __launch_bounds__(XM_WG_NT) void k_wgp_mirror(const double* in, double* out, int C) {
  extern __shared__ double lds[];
  const int t = threadIdx.x, n = 2 * C * C;
  const size_t base = (size_t)blockIdx.x * n;
  for (int e = t; e < n; e += XM_WG_NT) lds[e] = in[base + e];
  __syncthreads();
  wg_mirror(lds, C);
  for (int e = t; e < n; e += XM_WG_NT) out[base + e] = lds[e];
}

// ci, cj [256][XM_WG_MAXE]
__global__ __launch_bounds__(XM_WG_NT) void k_wgp_gram_entries(int* ci, int* cj, int C) {
  int i[XM_WG_MAXE], j[XM_WG_MAXE];
  wg_gram_entries(C, C * (C + 1) / 2, i, j);
#pragma unroll
  for (int m = 0; m < XM_WG_MAXE; ++m) {
    ci[threadIdx.x * XM_WG_MAXE + m] = i[m];
    cj[threadIdx.x * XM_WG_MAXE + m] = j[m];
  }
}

// bi, bj, sl [256][XM_WG_MAXB]
__global__ __launch_bounds__(XM_WG_NT) void k_wgp_gram_items(int* bi, int* bj, int* sl, int nb) {
  int i[XM_WG_MAXB], j[XM_WG_MAXB], s[XM_WG_MAXB];
  wg_gram_items(nb, nb * (nb + 1) / 2, i, j, s);
#pragma unroll
  for (int m = 0; m < XM_WG_MAXB; ++m) {
    bi[threadIdx.x * XM_WG_MAXB + m] = i[m];
    bj[threadIdx.x * XM_WG_MAXB + m] = j[m];
    sl[threadIdx.x * XM_WG_MAXB + m] = s[m];
  }
}

// LDS of the Jacobi probe: G, V (2 C^2 doubles each), red, rot (32 rotations, then the 32 pairs as ints)
__host__ __device__ inline size_t wgp_jacobi_doubles(int C) {
  return 4 * (size_t)C * C + XM_WG_NT + XM_WG_ROT * 32 + 32;
}

__global__ __launch_bounds__(XM_WG_NT) void k_wgp_jacobi(const double* g, double* g_out, double* v_out, int* ret, int C) {
  extern __shared__ double lds[];
  const int t = threadIdx.x, n = 2 * C * C;
  double* G = lds;
  double* V = G + n;
  double* red = V + n;
  double* rot = red + XM_WG_NT;
  const size_t base = (size_t)blockIdx.x * n;
  for (int e = t; e < n; e += XM_WG_NT) G[e] = g[base + e];
  __syncthreads();
  const int r = wg_jacobi(G, V, red, rot, C);
  __syncthreads();
  for (int e = t; e < n; e += XM_WG_NT) {
    g_out[base + e] = G[e];
    v_out[base + e] = V[e];
  }
  ret[(size_t)blockIdx.x * XM_WG_NT + t] = r;
}

// h [n][P][P] (the upper triangle is read), hd, dsc, g [n][P], lam [n] -> h_out [n][P][P] (the whole matrix afterwards),
// ld, dl [n][P] (-7 where nothing was written), ok [n][2][256]: wg_cholesky's value, then wg_solve's (-1: not called)
__global__ __launch_bounds__(XM_WG_NT) void k_wgp_cholesky(const double* h, const double* hd, const double* dsc,
                                                          const double* g, const double* lam, double* h_out, double* ld,
                                                          double* dl, int* ok, int P) {
  extern __shared__ double lds[];
  const int t = threadIdx.x;
  double* H = lds;
  double* Lhd = H + P * P;
  double* Ldsc = Lhd + P;
  double* Lg = Ldsc + P;
  double* Lld = Lg + P;
  double* Ldl = Lld + P;
  const size_t b = blockIdx.x;
  for (int e = t; e < P * P; e += XM_WG_NT) H[e] = h[b * P * P + e];
  for (int e = t; e < P; e += XM_WG_NT) {
    Lhd[e] = hd[b * P + e];
    Ldsc[e] = dsc[b * P + e];
    Lg[e] = g[b * P + e];
    Lld[e] = -7.0;
    Ldl[e] = -7.0;
  }
  __syncthreads();
  const bool c = wg_cholesky(H, Lhd, Ldsc, Lld, P, lam[b]);
  int s = -1;
  if (c) s = wg_solve(H, Lld, Lg, Ldl, P) ? 1 : 0;
  __syncthreads();
  for (int e = t; e < P * P; e += XM_WG_NT) h_out[b * P * P + e] = H[e];
  for (int e = t; e < P; e += XM_WG_NT) {
    ld[b * P + e] = Lld[e];
    dl[b * P + e] = Ldl[e];
  }
  ok[(b * 2) * XM_WG_NT + t] = c ? 1 : 0;
  ok[(b * 2 + 1) * XM_WG_NT + t] = s;
}

__global__ __launch_bounds__(XM_WG_NT) void k_wgp_from_internal(const int* bt, const double* u, const double* lo,
                                                               const double* hi, double* p, double* s, long long n) {
  const long long i = (long long)blockIdx.x * XM_WG_NT + threadIdx.x;
  if (i < n) wg_from_internal(bt[i], u[i], lo[i], hi[i], p[i], s[i]);
}

__global__ __launch_bounds__(XM_WG_NT) void k_wgp_to_internal(const int* bt, const double* v, const double* lo,
                                                             const double* hi, double* u, long long n) {
  const long long i = (long long)blockIdx.x * XM_WG_NT + threadIdx.x;
  if (i < n) u[i] = wg_to_internal(bt[i], v[i], lo[i], hi[i]);
}

// lm_normal with a model whose staged rows are given: in [n][n_points][2][P + 1] -> h_out [n][P][P], vec_out [n][7][P]
// (hd, dsc, g, u, ut, dl, ld), all of it -7 before lm_normal: it writes the strict upper triangle of H, hd and g only
struct WgpLmArgs {
  const double* in;
  double *h_out, *vec_out;
  int n, P, lda, q_pts;
};

struct WgpLmModel {
  using Args = WgpLmArgs;
  XM_DEV static int first(const Args&) { return 0; }
  XM_DEV static int count(const Args& A) { return A.n; }
  XM_DEV static void stage_point(const Args& A, const LmLds&, long long row, int i, bool, double* r0, double* r1) {
    const double* src = A.in + ((size_t)row * A.n + i) * 2 * (A.P + 1);
    for (int c = 0; c <= A.P; ++c) {
      r0[c] = src[c];
      r1[c] = src[A.P + 1 + c];
    }
  }
};

__global__ __launch_bounds__(XM_WG_NT) void k_wgp_lm_normal(WgpLmArgs A) {
  extern __shared__ double lds[];
  const int t = threadIdx.x, P = A.P, nh = P * P + 7 * P;  // H and the seven vectors are contiguous from L.H
  const LmLds L = lm_carve(lds, P, 0);
  for (int e = t; e < nh; e += XM_WG_NT) L.H[e] = -7.0;
  __syncthreads();
  lm_normal<WgpLmModel>(A, L, blockIdx.x, false);
  const size_t b = blockIdx.x;
  for (int e = t; e < P * P; e += XM_WG_NT) A.h_out[b * P * P + e] = L.H[e];
  for (int e = t; e < 7 * P; e += XM_WG_NT) A.vec_out[b * 7 * P + e] = L.hd[e];
}

// the loop of every user: who[item] = the workgroup that drew it, drawn[item] += 1
__global__ __launch_bounds__(XM_WG_NT) void k_wgp_ticket(unsigned* counter, int* who, int* drawn, long long n_items) {
  __shared__ unsigned next;
  for (;;) {
    const long long v = wg_next_item(counter, &next);
    if (v >= n_items) break;
    if (threadIdx.x == 0) {
      who[v] = (int)blockIdx.x;
      atomicAdd(drawn + v, 1);
    }
  }
  wg_leave(counter);
}

// ---- host ------------------------------------------------------------------------------------------------------------

namespace {
bool count_ok(long long n) { return n >= 0 && n <= XM_WGP_MAXN; }

// the dynamic-LDS opt-in of xm_resident_blocks (xm_host.h), then the launch's own error
template <class K>
int opt_in(K kern, size_t lds) {
  if (lds > 48 * 1024 &&
      hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
    (void)hipGetLastError();
    return XM_ERR_HIP;
  }
  return XM_OK;
}
int launched() { return hipGetLastError() == hipSuccess ? XM_OK : XM_ERR_HIP; }
}  // namespace

extern "C" {

int xm_wgp_sum(const double* in, double* out, long long n_rows, void* stream) {
  if (!in || !out || !count_ok(n_rows)) return XM_ERR_INVALID_ARG;
  if (n_rows == 0) return XM_OK;
  hipLaunchKernelGGL(k_wgp_sum, dim3((unsigned)n_rows), dim3(XM_WG_NT), 0, (hipStream_t)stream, in, out);
  return launched();
}

int xm_wgp_mirror(const double* in, double* out, long long n, int C, void* stream) {
  if (!in || !out || !count_ok(n) || C < 1 || C > XM_WGP_MAXC) return XM_ERR_INVALID_ARG;
  if (n == 0) return XM_OK;
  const size_t lds = 2 * (size_t)C * C * sizeof(double);
  if (const int rc = opt_in(k_wgp_mirror, lds)) return rc;
  hipLaunchKernelGGL(k_wgp_mirror, dim3((unsigned)n), dim3(XM_WG_NT), lds, (hipStream_t)stream, in, out, C);
  return launched();
}

int xm_wgp_gram_entries(int* ci, int* cj, int C, void* stream) {
  if (!ci || !cj || C < 1 || C > XM_WGP_MAXC) return XM_ERR_INVALID_ARG;
  hipLaunchKernelGGL(k_wgp_gram_entries, dim3(1), dim3(XM_WG_NT), 0, (hipStream_t)stream, ci, cj, C);
  return launched();
}

int xm_wgp_gram_items(int* bi, int* bj, int* sl, int nb, void* stream) {
  if (!bi || !bj || !sl || nb < 1 || nb > XM_WGP_MAXC / 8) return XM_ERR_INVALID_ARG;
  hipLaunchKernelGGL(k_wgp_gram_items, dim3(1), dim3(XM_WG_NT), 0, (hipStream_t)stream, bi, bj, sl, nb);
  return launched();
}

int xm_wgp_jacobi(const double* g, double* g_out, double* v_out, int* ret, long long n, int C, void* stream) {
  if (!g || !g_out || !v_out || !ret || !count_ok(n) || C < 1 || C > XM_WGP_MAXC) return XM_ERR_INVALID_ARG;
  if (n == 0) return XM_OK;
  const size_t lds = wgp_jacobi_doubles(C) * sizeof(double);  // about 132 KiB at C = 64
  if (const int rc = opt_in(k_wgp_jacobi, lds)) return rc;
  hipLaunchKernelGGL(k_wgp_jacobi, dim3((unsigned)n), dim3(XM_WG_NT), lds, (hipStream_t)stream, g, g_out, v_out, ret, C);
  return launched();
}

int xm_wgp_cholesky(const double* h, const double* hd, const double* dsc, const double* g, const double* lam,
                    double* h_out, double* ld, double* dl, int* ok, long long n, int P, void* stream) {
  if (!h || !hd || !dsc || !g || !lam || !h_out || !ld || !dl || !ok || !count_ok(n) || P < 1 || P > XM_WGP_MAXP)
    return XM_ERR_INVALID_ARG;
  if (n == 0) return XM_OK;
  const size_t lds = ((size_t)P * P + 5 * (size_t)P) * sizeof(double);
  if (const int rc = opt_in(k_wgp_cholesky, lds)) return rc;
  hipLaunchKernelGGL(k_wgp_cholesky, dim3((unsigned)n), dim3(XM_WG_NT), lds, (hipStream_t)stream, h, hd, dsc, g, lam,
                     h_out, ld, dl, ok, P);
  return launched();
}

int xm_wgp_from_internal(const int* bt, const double* u, const double* lo, const double* hi, double* p, double* s,
                         long long n, void* stream) {
  if (!bt || !u || !lo || !hi || !p || !s || !count_ok(n)) return XM_ERR_INVALID_ARG;
  if (n == 0) return XM_OK;
  hipLaunchKernelGGL(k_wgp_from_internal, dim3((unsigned)((n + XM_WG_NT - 1) / XM_WG_NT)), dim3(XM_WG_NT), 0,
                     (hipStream_t)stream, bt, u, lo, hi, p, s, n);
  return launched();
}

int xm_wgp_to_internal(const int* bt, const double* v, const double* lo, const double* hi, double* u, long long n,
                       void* stream) {
  if (!bt || !v || !lo || !hi || !u || !count_ok(n)) return XM_ERR_INVALID_ARG;
  if (n == 0) return XM_OK;
  hipLaunchKernelGGL(k_wgp_to_internal, dim3((unsigned)((n + XM_WG_NT - 1) / XM_WG_NT)), dim3(XM_WG_NT), 0,
                     (hipStream_t)stream, bt, v, lo, hi, u, n);
  return launched();
}

int xm_wgp_lm_normal(const double* in, double* h_out, double* vec_out, long long n, int n_points, int P, void* stream) {
  if (!in || !h_out || !vec_out || !count_ok(n) || n_points < 1 || P < 1 || P > XM_WGP_MAXP) return XM_ERR_INVALID_ARG;
  if (n == 0) return XM_OK;
  WgpLmArgs A{in, h_out, vec_out, n_points, P, P + 1, lm_q_pts(P + 1)};
  const size_t lds = lm_lds_bytes(P, A.lda, A.q_pts, 0);  // about 100 KiB at P = 63
  if (const int rc = opt_in(k_wgp_lm_normal, lds)) return rc;
  hipLaunchKernelGGL(k_wgp_lm_normal, dim3((unsigned)n), dim3(XM_WG_NT), lds, (hipStream_t)stream, A);
  return launched();
}

// `counter`: the {ticket, workgroups done} pair, zero at launch (the caller's business, as xm_launch_items zeroes it for
// the product kernels); who, drawn [n_items], drawn zero at launch; an explicit grid of 1 ... 1024 workgroups
int xm_wgp_ticket(unsigned* counter, int* who, int* drawn, long long n_items, int grid, void* stream) {
  if (!counter || !who || !drawn || !count_ok(n_items) || grid < 1 || grid > 1024) return XM_ERR_INVALID_ARG;
  hipLaunchKernelGGL(k_wgp_ticket, dim3((unsigned)grid), dim3(XM_WG_NT), 0, (hipStream_t)stream, counter, who, drawn,
                     n_items);
  return launched();
}

}  // extern "C"
