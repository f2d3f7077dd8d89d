// Basis-set (linear-combination) time-domain fitting kernels, DESIGN.md section 15.  Included by xm_basis.hip only.
//
// Model:  x^_n = e^{i phi} sum_m a_m B_m[n] exp(-d_g t_n - s_g t_n^2 + i 2 pi f_g t_n),  g = group(m),  t_n = n dt.
// Parameter q of a voxel (Q = M + 3 G + 1 of them): q = m amplitude a_m; M + g shift f_g [Hz]; M + G + g Lorentzian
// damping d_g [1/s]; M + 2 G + g Gaussian damping s_g [1/s^2]; M + 3 G the phase phi [rad].  The cost runs over the
// points n >= skip.
//
// k_basis_fit: one 256-thread workgroup per voxel, voxels handed out by a device counter (persistent grid), each fitted
// by the Levenberg-Marquardt driver of xm_lm.h, as k_amares_fit (xm_amares.h) is.  This file holds what is the basis
// model's own: the model term, its Jacobian rows, the automatic amplitude start and `skip`.
//
// Per point a thread computes one exp and one sincos per GROUP (the factor E_g =
// e^{i phi} exp(-d_g t - s_g t^2 + i 2 pi f_g t)), then walks the group's metabolites in ascending m, reading
// B_m[n] from global memory (the basis is shared by every voxel and stays in the L2): the a_m column is E_g B_m[n]
// (formed without a_m, so a_m = 0 is fine), and T_g = sum_m a_m E_g B_m[n] gives the group's f, d and s columns
// (i 2 pi t T_g, -t T_g, -t^2 T_g).  x^ = sum_g T_g (groups ascending) and the phi column is i x^.  Every column is
// chained through dp/du.
#pragma once
#include "xm_lm.h"

#define XM_BS_MAXQ 128                 // physical parameters M + 3 G + 1
#define XM_BS_MAXP XM_LM_MAXP          // free columns

struct BasisFitArgs {
  const void* x;        // rows of n complex samples (complex64 or complex128), `stride` elements apart
  const double* basis;  // [M, n] complex128 (interleaved), shared by every voxel
  const double* bnorm;  // [M] ||B_m||_2 over the fitted points (k_basis_norms, in the workspace)
  long long stride, nb;
  int n, skip, is_c64;
  double dt;
  int M, G, Q, P, max_iter;  // metabolites, groups, parameters, free columns
  int lda, q_pts;            // staged row stride (P + 1 doubles), points per staging round
  double ftol, xtol;
  double* params;      // [nb, Q] physical
  double* asd;         // [nb, M] standard deviation of a_m (0 for a fixed amplitude)
  double* rss;         // [nb]
  int* status;         // [nb] 0 converged, 1 iteration cap, 2 non-finite
  int* iters;          // [nb]
  double* fit;         // [nb, n] complex128, or nullptr
  unsigned* counter;   // [2] zero at launch: row ticket, workgroups done
  double u0[XM_BS_MAXQ];  // free: internal start value (NaN: an amplitude's automatic start); fixed: the physical value
  double lo[XM_BS_MAXQ], hi[XM_BS_MAXQ];
  signed char bt[XM_BS_MAXQ];       // XM_WG_* bound type (xm_wg.h)
  signed char col[XM_BS_MAXQ];      // free column of parameter q, -1 when fixed
  unsigned char ord[XM_BS_MAXQ];    // metabolites sorted by group, ascending m within a group
  unsigned char gs[XM_BS_MAXQ + 1]; // group g owns ord[gs[g] ... gs[g + 1])
};
static_assert(sizeof(BasisFitArgs) <= 4096, "BasisFitArgs must fit the 4 KB kernel-argument limit");

struct BasisModelArgs {
  const double* params;  // [nb, Q]
  const double* basis;   // [M, n] complex128
  double* out;           // [nb, n] complex128
  long long nb;
  int n, M, G;
  double dt;
  unsigned char ord[XM_BS_MAXQ];
  unsigned char gs[XM_BS_MAXQ + 1];
};

// E_g at time t: e^{i phi} exp(-d t - s t^2) e^{i 2 pi f t}.  One exp and one sincos.
XM_DEV void bs_group_factor(double f, double d, double s, double phi, double t, double& er, double& ei) {
  const double e = exp(-(d + s * t) * t);
  double sn, cs;
  sincos(phi + 2.0 * M_PI * f * t, &sn, &cs);
  er = e * cs;
  ei = e * sn;
}

// x^ at point i for the Q parameters p (LDS or global); ord / gs as in the argument structs
XM_DEV void bs_model_point(const double* p, const double* __restrict__ basis, const unsigned char* ord,
                           const unsigned char* gs, int M, int G, int n, double dt, int i, double& mr, double& mi) {
  const double t = (double)i * dt, phi = p[M + 3 * G];
  mr = 0.0;
  mi = 0.0;
  for (int g = 0; g < G; ++g) {
    double er, ei;
    bs_group_factor(p[M + g], p[M + G + g], p[M + 2 * G + g], phi, t, er, ei);
    double tr = 0.0, ti = 0.0;
    for (int k = gs[g]; k < gs[g + 1]; ++k) {
      const int m = ord[k];
      const double* b = basis + 2 * ((size_t)m * n + i);
      const double br = b[0], bi = b[1], a = p[m];
      tr += a * (er * br - ei * bi);
      ti += a * (er * bi + ei * br);
    }
    mr += tr;
    mi += ti;
  }
}

__global__ void k_basis_model(BasisModelArgs A) {
  const long long total = A.nb * (long long)A.n;
  const int Q = A.M + 3 * A.G + 1;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
    const long long b = e / A.n;
    const int i = (int)(e - b * A.n);
    double mr, mi;
    bs_model_point(A.params + b * Q, A.basis, A.ord, A.gs, A.M, A.G, A.n, A.dt, i, mr, mi);
    A.out[2 * e] = mr;
    A.out[2 * e + 1] = mi;
  }
}

// bnorm[m] = ||B_m[skip ...]||_2, one workgroup per metabolite, fixed summation order
__global__ __launch_bounds__(XM_WG_NT) void k_basis_norms(const double* __restrict__ basis, int n, int skip,
                                                          double* __restrict__ bnorm) {
  __shared__ double red[XM_WG_NT];
  const int t = threadIdx.x, m = blockIdx.x;
  double c = 0.0;
  for (int i = skip + t; i < n; i += XM_WG_NT) {
    const double* b = basis + 2 * ((size_t)m * n + i);
    c += b[0] * b[0] + b[1] * b[1];
  }
  const double s = wg_sum(red, c);
  if (t == 0) bnorm[m] = sqrt(s);
}

// The model of xm_lm.h's driver.
struct BsModel {
  using Args = BasisFitArgs;
  XM_DEV static int first(const Args& A) { return A.skip; }
  XM_DEV static int count(const Args& A) { return A.n - A.skip; }
  XM_DEV static int n_phys(const Args& A) { return A.Q; }
  XM_DEV static int n_amp(const Args& A) { return A.M; }
  XM_DEV static int amp_param(const Args&, int m) { return m; }
  XM_DEV static double amp_factor(const Args&, int) { return 1.0; }

  // start: the caller's values; an amplitude without one from ||x|| / (M ||B_m||) over the fitted points
  XM_DEV static void start(const Args& A, const LmLds& L, long long row) {
    const int t = threadIdx.x, M = A.M;
    double xx = 0.0;
    for (int i = A.skip + t; i < A.n; i += XM_WG_NT) {
      double xi;
      const double xr = lm_load(A.x, A.is_c64, A.stride, row, i, xi);
      xx += xr * xr + xi * xi;
    }
    const double xnorm = sqrt(wg_sum(L.red, xx));
    if (t < A.Q && A.col[t] >= 0) {
      double u = A.u0[t];
      if (t < M && isnan(u)) {
        const double bn = A.bnorm[t];
        u = wg_to_internal(A.bt[t], bn > 0.0 ? xnorm / ((double)M * bn) : 0.0, A.lo[t], A.hi[t]);
      }
      L.u[A.col[t]] = u;
    }
  }

  // p, s <- physical values / slopes of the internal vector `u` (free parameters; fixed ones keep A.u0)
  XM_DEV static void set_params(const Args& A, const LmLds& L, const double* u) {
    const int t = threadIdx.x;
    if (t < A.Q) {
      const int j = A.col[t];
      double p = A.u0[t], s = 0.0;
      if (j >= 0) wg_from_internal(A.bt[t], u[j], A.lo[t], A.hi[t], p, s);
      L.p[t] = p;
      L.s[t] = s;
    }
    __syncthreads();
  }

  // sum over the fitted points of |x - x^|^2 (every thread the same value; fixed summation order).  `fit`: x^ of ALL n
  // points is stored as well (the points before `skip` take no part in the sum).
  XM_DEV static double cost(const Args& A, const LmLds& L, long long row, double* fit) {
    const int t = threadIdx.x;
    double c = 0.0;
    for (int i = (fit ? 0 : A.skip) + t; i < A.n; i += XM_WG_NT) {
      double mr, mi;
      bs_model_point(L.p, A.basis, A.ord, A.gs, A.M, A.G, A.n, A.dt, i, mr, mi);
      if (i >= A.skip) {
        double xi;
        const double xr = lm_load(A.x, A.is_c64, A.stride, row, i, xi);
        const double rr = xr - mr, ri = xi - mi;
        c += rr * rr + ri * ri;
      }
      if (fit) {
        fit[2 * (long long)i] = mr;
        fit[2 * (long long)i + 1] = mi;
      }
    }
    return wg_sum(L.red, c);
  }

  // [J | r] rows of point i into r0 (real part) and r1 (imaginary part)
  XM_DEV static void stage_point(const Args& A, const LmLds& L, long long row, int i, bool phys, double* r0, double* r1) {
    const int M = A.M, G = A.G, P = A.P;
    const double* p = L.p;
    const double t = (double)i * A.dt, phi = p[M + 3 * G];
    double mr = 0.0, mi = 0.0;
    for (int g = 0; g < G; ++g) {
      double er, ei;
      bs_group_factor(p[M + g], p[M + G + g], p[M + 2 * G + g], phi, t, er, ei);
      double tr = 0.0, ti = 0.0;
      for (int k = A.gs[g]; k < A.gs[g + 1]; ++k) {
        const int m = A.ord[k];
        const double* b = A.basis + 2 * ((size_t)m * A.n + i);
        const double br = b[0], bi = b[1], a = p[m];
        const double vr = er * br - ei * bi, vi = er * bi + ei * br;  // d x^ / d a_m
        const int jc = A.col[m];
        if (jc >= 0) {
          const double w = phys ? 1.0 : L.s[m];
          r0[jc] = vr * w;
          r1[jc] = vi * w;
        }
        tr += a * vr;
        ti += a * vi;
      }
      int jc;
      if ((jc = A.col[M + g]) >= 0) {  // d/df = i 2 pi t T
        const double w = 2.0 * M_PI * t * (phys ? 1.0 : L.s[M + g]);
        r0[jc] = -ti * w;
        r1[jc] = tr * w;
      }
      if ((jc = A.col[M + G + g]) >= 0) {  // d/dd = -t T
        const double w = -t * (phys ? 1.0 : L.s[M + G + g]);
        r0[jc] = tr * w;
        r1[jc] = ti * w;
      }
      if ((jc = A.col[M + 2 * G + g]) >= 0) {  // d/ds = -t^2 T
        const double w = -t * t * (phys ? 1.0 : L.s[M + 2 * G + g]);
        r0[jc] = tr * w;
        r1[jc] = ti * w;
      }
      mr += tr;
      mi += ti;
    }
    const int jc = A.col[M + 3 * G];
    if (jc >= 0) {  // d/dphi = i x^
      const double w = phys ? 1.0 : L.s[M + 3 * G];
      r0[jc] = -mi * w;
      r1[jc] = mr * w;
    }
    double xi;
    const double xr = lm_load(A.x, A.is_c64, A.stride, row, i, xi);
    r0[P] = xr - mr;
    r1[P] = xi - mi;
  }
};

__global__ __launch_bounds__(XM_WG_NT) void k_basis_fit(BasisFitArgs A) {
  extern __shared__ double bs_sm[];
  const LmLds L = lm_carve(bs_sm, A.P, XM_BS_MAXQ);
  __shared__ unsigned next;
  for (;;) {
    const long long row = wg_next_item(A.counter, &next);
    if (row >= A.nb) break;

    // The voxel's arguments are read again from the kernel-argument segment: carried across this loop in scalar
    // registers they are spilled as whole tuples, which costs the kernel a private segment.  z is 0.
    int z = 0;
    asm volatile("" : "+s"(z));
    lm_fit_item<BsModel>((&A)[z], L, row);
  }
  wg_leave(A.counter);
}

