// libxmris_wgprobe.so -- test-only probes of the workgroup toolbox (xm_wg.h) and of the normal-equation accumulation of
// the Levenberg-Marquardt driver built on it (xm_lm.h), outside the product library: it is not
// linked into libxmris_hip.so and not declared in include/xmris_hip.h.  Each kernel is one 256-thread workgroup per
// problem: it stages its input in the LDS, calls one toolbox function and copies everything out, so that
// tests/test_gpu_wg.py can hold every part to tests/_wg_oracle.py on its own.  The host side checks its arguments --
// nothing else stands between a test and an LDS overrun -- and returns XM_ERR_INVALID_ARG without a launch.  The complex
// Gram accumulation loops (wg_gram_*) are not restated here: they stay in the users and are tested through them.  The
// real one of the fitting kernels is lm_normal itself, probed below with a model that copies given rows.  The driver's
// loop, lm_fit_item, is probed whole by xm_wgp_lm_fit: standard least-squares problems in the persistent loop of the
// product kernels (tests/test_gpu_lm.py against tests/_lm_oracle.py).
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

// ---- lm_fit_item on standard least-squares problems ------------------------------------------------------------------
// The whole driver (start, LM loop, CRLB pass, outputs) inside the persistent loop of the product kernels, with a model
// that is none of theirs.  A point carries two real residuals; model x^ and data x, r = x - x^.  The closed-form kinds
// (More, Garbow, Hillstrom 1981) have x = 0 and x^ = -f.  Q physical parameters, the first NA of them "amplitudes".
//   start [nb, Q]     free parameter: the internal start value; fixed: the physical value
//   tab [nb, stride]  EXP2: n_res, then (t_k, y_k) per residual; TABLE: jadd, then 2 n rows of (A[k, 0 ... Q), y_k), with
//                     x^ = A p over all Q parameters and jadd added to the Jacobian column of parameter 0 (0, or NaN for
//                     a Jacobian that is not finite where the cost is); WALL: the wall w.  A residual past n_res is 0.
//   u_out [nb, P]     the internal vector the driver stopped at
enum { WGP_ROSENBROCK = 0, WGP_POWELL, WGP_FREUDENSTEIN, WGP_HELICAL, WGP_BROWN_DENNIS, WGP_BOX3D, WGP_EXP2, WGP_TABLE,
       WGP_WALL, WGP_KINDS };
#define XM_WGP_MAXQ 128      // physical parameters, as XM_BS_MAXQ
#define XM_WGP_MAXPTS 4096   // points of a problem

struct WgpFitArgs {
  const double *start, *tab, *factor;
  long long nb, tab_stride;
  int n, Q, NA, P, max_iter, lda, q_pts;
  double ftol, xtol;
  double *params, *asd, *rss;
  int *status, *iters;
  double *fit, *u_out;
  unsigned* counter;
  double lo[XM_WGP_MAXQ], hi[XM_WGP_MAXQ];
  signed char bt[XM_WGP_MAXQ], col[XM_WGP_MAXQ];
};
static_assert(sizeof(WgpFitArgs) <= 4096, "WgpFitArgs must fit the 4 KB kernel-argument limit");

// model pair m and data pair d of point i at the physical parameters p; `jac`: the rows d m / d p of the free columns
// times w[q] (w null: 1) into r0, r1 as well
template <int KIND>
XM_DEV void wgp_point(const WgpFitArgs& A, const double* p, const double* tab, int i, double (&m)[2], double (&d)[2],
                      bool jac, const double* w, double* r0, double* r1) {
  d[0] = d[1] = 0.0;
  if (KIND == WGP_TABLE) {
    const int Q = A.Q;
    const double jadd = tab[0];
    const double* a0 = tab + 1 + (size_t)(2 * i) * (Q + 1);
    const double* a1 = a0 + (Q + 1);
    double s0 = 0.0, s1 = 0.0;
    for (int q = 0; q < Q; ++q) {
      s0 += a0[q] * p[q];
      s1 += a1[q] * p[q];
    }
    m[0] = s0;
    m[1] = s1;
    d[0] = a0[Q];
    d[1] = a1[Q];
    if (jac)
      for (int q = 0; q < Q; ++q) {
        const int c = A.col[q];
        if (c >= 0) {
          const double ww = w ? w[q] : 1.0, add = q == 0 ? jadd : 0.0;
          r0[c] = (a0[q] + add) * ww;
          r1[c] = (a1[q] + add) * ww;
        }
      }
    return;
  }
  double f[2] = {0.0, 0.0}, df[2][4] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};  // m = -f except for EXP2
  if (KIND == WGP_ROSENBROCK || KIND == WGP_WALL) {
    if (i == 0) {
      f[0] = 10.0 * (p[1] - p[0] * p[0]);
      df[0][0] = -20.0 * p[0];
      df[0][1] = 10.0;
      f[1] = 1.0 - p[0];
      df[1][0] = -1.0;
    } else {  // WALL: 0 on this side of the wall, NaN beyond it
      f[0] = 0.0 * sqrt(tab[0] - p[0]);
    }
  } else if (KIND == WGP_POWELL) {
    if (i == 0) {
      f[0] = p[0] + 10.0 * p[1];
      df[0][0] = 1.0;
      df[0][1] = 10.0;
      f[1] = sqrt(5.0) * (p[2] - p[3]);
      df[1][2] = sqrt(5.0);
      df[1][3] = -sqrt(5.0);
    } else {
      const double a = p[1] - 2.0 * p[2], b = p[0] - p[3];
      f[0] = a * a;
      df[0][1] = 2.0 * a;
      df[0][2] = -4.0 * a;
      f[1] = sqrt(10.0) * (b * b);
      df[1][0] = 2.0 * sqrt(10.0) * b;
      df[1][3] = -2.0 * sqrt(10.0) * b;
    }
  } else if (KIND == WGP_FREUDENSTEIN) {
    f[0] = -13.0 + p[0] + ((5.0 - p[1]) * p[1] - 2.0) * p[1];
    df[0][0] = 1.0;
    df[0][1] = 10.0 * p[1] - 3.0 * p[1] * p[1] - 2.0;
    f[1] = -29.0 + p[0] + ((p[1] + 1.0) * p[1] - 14.0) * p[1];
    df[1][0] = 1.0;
    df[1][1] = 3.0 * p[1] * p[1] + 2.0 * p[1] - 14.0;
  } else if (KIND == WGP_HELICAL) {
    if (i == 0) {
      const double r2 = p[0] * p[0] + p[1] * p[1], r = sqrt(r2);
      double th = atan(p[1] / p[0]) / (2.0 * M_PI);
      if (p[0] < 0.0) th += 0.5;
      f[0] = 10.0 * (p[2] - 10.0 * th);
      df[0][0] = 100.0 * p[1] / (2.0 * M_PI * r2);
      df[0][1] = -100.0 * p[0] / (2.0 * M_PI * r2);
      df[0][2] = 10.0;
      f[1] = 10.0 * (r - 1.0);
      df[1][0] = 10.0 * p[0] / r;
      df[1][1] = 10.0 * p[1] / r;
    } else {
      f[0] = p[2];
      df[0][2] = 1.0;
    }
  } else if (KIND == WGP_BROWN_DENNIS) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const double t = (double)(2 * i + h + 1) / 5.0;
      double sn, cs;
      sincos(t, &sn, &cs);
      const double a = p[0] + t * p[1] - exp(t), b = p[2] + p[3] * sn - cs;
      f[h] = a * a + b * b;
      df[h][0] = 2.0 * a;
      df[h][1] = 2.0 * a * t;
      df[h][2] = 2.0 * b;
      df[h][3] = 2.0 * b * sn;
    }
  } else if (KIND == WGP_BOX3D) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const double t = 0.1 * (double)(2 * i + h + 1);
      const double e0 = exp(-t * p[0]), e1 = exp(-t * p[1]), c = exp(-t) - exp(-10.0 * t);
      f[h] = e0 - e1 - p[2] * c;
      df[h][0] = -t * e0;
      df[h][1] = t * e1;
      df[h][2] = -c;
    }
  } else if (KIND == WGP_EXP2) {
    const int n_res = (int)tab[0];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int k = 2 * i + h;
      if (k < n_res) {
        const double t = tab[1 + 2 * k];
        const double e0 = exp(-p[1] * t), e1 = exp(-p[3] * t);
        d[h] = tab[2 + 2 * k];
        f[h] = -(p[0] * e0 + p[2] * e1);  // so that m = -f is the model
        df[h][0] = -e0;
        df[h][1] = p[0] * t * e0;
        df[h][2] = -e1;
        df[h][3] = p[2] * t * e1;
      }
    }
  }
  m[0] = -f[0];
  m[1] = -f[1];
  if (jac) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (q < A.Q) {
        const int c = A.col[q];
        if (c >= 0) {
          const double ww = w ? w[q] : 1.0;
          r0[c] = -df[0][q] * ww;
          r1[c] = -df[1][q] * ww;
        }
      }
    }
  }
}

template <int KIND>
struct WgpFitModel {
  using Args = WgpFitArgs;
  XM_DEV static int first(const Args&) { return 0; }
  XM_DEV static int count(const Args& A) { return A.n; }
  XM_DEV static int n_phys(const Args& A) { return A.Q; }
  XM_DEV static int n_amp(const Args& A) { return A.NA; }
  XM_DEV static int amp_param(const Args&, int m) { return m; }
  XM_DEV static double amp_factor(const Args& A, int m) { return A.factor[m]; }

  // the row's start values; a fixed parameter's value and slope 0 go to L.p, L.s here, once per row
  XM_DEV static void start(const Args& A, const LmLds& L, long long row) {
    const int t = threadIdx.x;
    if (t < A.Q) {
      const double v = A.start[row * A.Q + t];
      const int j = A.col[t];
      if (j >= 0) {
        L.u[j] = v;
      } else {
        L.p[t] = v;
        L.s[t] = 0.0;
      }
    }
  }

  XM_DEV static void set_params(const Args& A, const LmLds& L, const double* u) {
    const int t = threadIdx.x;
    if (t < A.Q) {
      const int j = A.col[t];
      if (j >= 0) wg_from_internal(A.bt[t], u[j], A.lo[t], A.hi[t], L.p[t], L.s[t]);
    }
    __syncthreads();
  }

  XM_DEV static double cost(const Args& A, const LmLds& L, long long row, double* fit) {
    const double* tab = A.tab + row * A.tab_stride;
    double c = 0.0;
    for (int i = threadIdx.x; i < A.n; i += XM_WG_NT) {
      double m[2], d[2];
      wgp_point<KIND>(A, L.p, tab, i, m, d, false, nullptr, nullptr, nullptr);
      const double r0 = d[0] - m[0], r1 = d[1] - m[1];
      c += r0 * r0 + r1 * r1;
      if (fit) {
        fit[2 * (long long)i] = m[0];
        fit[2 * (long long)i + 1] = m[1];
      }
    }
    return wg_sum(L.red, c);
  }

  XM_DEV static void stage_point(const Args& A, const LmLds& L, long long row, int i, bool phys, double* r0, double* r1) {
    double m[2], d[2];
    wgp_point<KIND>(A, L.p, A.tab + row * A.tab_stride, i, m, d, true, phys ? nullptr : L.s, r0, r1);
    r0[A.P] = d[0] - m[0];
    r1[A.P] = d[1] - m[1];
  }
};

template <int KIND>
__global__ __launch_bounds__(XM_WG_NT) void k_wgp_lm_fit(WgpFitArgs A) {
  extern __shared__ double lds[];
  const LmLds L = lm_carve(lds, A.P, XM_WGP_MAXQ);
  __shared__ unsigned next;
  for (;;) {
    const long long row = wg_next_item(A.counter, &next);
    if (row >= A.nb) break;
    int z = 0;  // the arguments are read again from the kernel-argument segment, as in k_basis_fit
    asm volatile("" : "+s"(z));
    lm_fit_item<WgpFitModel<KIND>>((&A)[z], L, row);
    if (threadIdx.x < A.P) A.u_out[row * A.P + threadIdx.x] = L.u[threadIdx.x];
  }
  wg_leave(A.counter);
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

template <int KIND>
int launch_fit(const WgpFitArgs& A, size_t lds, int grid, void* stream) {
  if (const int rc = opt_in(k_wgp_lm_fit<KIND>, lds)) return rc;
  hipLaunchKernelGGL(k_wgp_lm_fit<KIND>, dim3((unsigned)grid), dim3(XM_WG_NT), lds, (hipStream_t)stream, A);
  return launched();
}

// (parameters, points) of a closed-form kind; 0: the caller's choice
const int FIT_Q[WGP_KINDS] = {2, 4, 2, 3, 4, 3, 4, 0, 2};
const int FIT_N[WGP_KINDS] = {1, 2, 1, 2, 10, 5, 0, 0, 2};
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

// lm_fit_item on problem `kind` (WGP_*), nb rows of it: start [nb, Q], tab [nb, tab_stride] (may be null where the kind
// reads none), factor [NA] on the device; bt (XM_WG_*, 0: fixed), lo, hi [Q] on the host, P = the free ones, which take
// the columns 0 ... P - 1 in ascending order.  Outputs on the device: params [nb, Q], asd [nb, NA], rss, status, iters
// [nb], fit [nb, n_points, 2] (or null), u_out [nb, P].  `counter` and `grid` as for xm_wgp_ticket.
int xm_wgp_lm_fit(int kind, const double* start, const double* tab, long long tab_stride, const double* factor,
                  const int* bt, const double* lo, const double* hi, long long nb, int n_points, int Q, int NA, int P,
                  int max_iter, double ftol, double xtol, double* params, double* asd, double* rss, int* status,
                  int* iters, double* fit, double* u_out, unsigned* counter, int grid, void* stream) {
  if (kind < 0 || kind >= WGP_KINDS || !start || !factor || !bt || !lo || !hi || !params || !asd || !rss || !status ||
      !iters || !u_out || !counter || !count_ok(nb) || grid < 1 || grid > 1024)
    return XM_ERR_INVALID_ARG;
  if (Q < 1 || Q > XM_WGP_MAXQ || (FIT_Q[kind] && Q != FIT_Q[kind]) || n_points < 1 || n_points > XM_WGP_MAXPTS ||
      (FIT_N[kind] && n_points != FIT_N[kind]) || NA < 1 || NA > Q || P < 1 || P > XM_WGP_MAXP || max_iter < 0 ||
      max_iter > 100000 || !(ftol >= 0.0) || !(xtol >= 0.0) || !std::isfinite(ftol) || !std::isfinite(xtol))
    return XM_ERR_INVALID_ARG;
  const long long need = kind == WGP_TABLE  ? 1 + 2 * (long long)n_points * (Q + 1)
                         : kind == WGP_EXP2 ? 1 + 4 * (long long)n_points
                         : kind == WGP_WALL ? 1
                                            : 0;
  if (tab_stride < need || (need && !tab)) return XM_ERR_INVALID_ARG;
  WgpFitArgs A{};
  int free_cols = 0;
  for (int q = 0; q < Q; ++q) {
    const bool fl = std::isfinite(lo[q]), fh = std::isfinite(hi[q]);
    if (bt[q] < XM_WG_FIXED || bt[q] > XM_WG_TWO || (bt[q] == XM_WG_TWO && !(fl && fh && lo[q] < hi[q])) ||
        (bt[q] == XM_WG_LO && !fl) || (bt[q] == XM_WG_HI && !fh))
      return XM_ERR_INVALID_ARG;
    A.bt[q] = (signed char)bt[q];
    A.lo[q] = lo[q];
    A.hi[q] = hi[q];
    A.col[q] = bt[q] == XM_WG_FIXED ? (signed char)-1 : (signed char)free_cols++;
  }
  if (free_cols != P) return XM_ERR_INVALID_ARG;
  if (nb == 0) return XM_OK;
  A.start = start;
  A.tab = tab;
  A.factor = factor;
  A.nb = nb;
  A.tab_stride = tab_stride;
  A.n = n_points;
  A.Q = Q;
  A.NA = NA;
  A.P = P;
  A.max_iter = max_iter;
  A.lda = P + 1;
  A.q_pts = lm_q_pts(A.lda);
  A.ftol = ftol;
  A.xtol = xtol;
  A.params = params;
  A.asd = asd;
  A.rss = rss;
  A.status = status;
  A.iters = iters;
  A.fit = fit;
  A.u_out = u_out;
  A.counter = counter;
  const size_t lds = lm_lds_bytes(P, A.lda, A.q_pts, XM_WGP_MAXQ);  // about 101 KiB at P = 80
  switch (kind) {
    case WGP_ROSENBROCK: return launch_fit<WGP_ROSENBROCK>(A, lds, grid, stream);
    case WGP_POWELL: return launch_fit<WGP_POWELL>(A, lds, grid, stream);
    case WGP_FREUDENSTEIN: return launch_fit<WGP_FREUDENSTEIN>(A, lds, grid, stream);
    case WGP_HELICAL: return launch_fit<WGP_HELICAL>(A, lds, grid, stream);
    case WGP_BROWN_DENNIS: return launch_fit<WGP_BROWN_DENNIS>(A, lds, grid, stream);
    case WGP_BOX3D: return launch_fit<WGP_BOX3D>(A, lds, grid, stream);
    case WGP_EXP2: return launch_fit<WGP_EXP2>(A, lds, grid, stream);
    case WGP_TABLE: return launch_fit<WGP_TABLE>(A, lds, grid, stream);
    default: return launch_fit<WGP_WALL>(A, lds, grid, stream);
  }
}

}  // extern "C"
