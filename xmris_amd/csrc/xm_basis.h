// Basis-set (linear-combination) time-domain fitting kernels, DESIGN.md section 15.  Included by xm_basis.hip only.
//
// Model:  x^_n = e^{i phi} sum_m a_m B_m[n] exp(-d_g t_n - s_g t_n^2 + i 2 pi f_g t_n),  g = group(m),  t_n = n dt.
// Parameter q of a voxel (Q = M + 3 G + 1 of them): q = m amplitude a_m; M + g shift f_g [Hz]; M + G + g Lorentzian
// damping d_g [1/s]; M + 2 G + g Gaussian damping s_g [1/s^2]; M + 3 G the phase phi [rad].  The cost runs over the
// points n >= skip.
//
// k_basis_fit takes the scheme of k_amares_fit (xm_amares.h): one 256-thread workgroup per voxel, voxels handed out by a
// device counter (persistent grid); Levenberg-Marquardt in lmfit's internal variables u with the analytic Jacobian; the
// augmented rows [J | r] of a round of points staged in the LDS (two rows per point); every thread accumulates its own
// entries of [J | r]^T [J | r] over the rounds in a fixed order, so a voxel's result does not depend on its batch or on
// the workgroup that fits it; Cholesky of the damped normal equations in the LDS.  All arithmetic fp64.
//
// What differs is the model term.  Per point a thread computes one exp and one sincos per GROUP (the factor
// E_g = e^{i phi} exp(-d_g t - s_g t^2 + i 2 pi f_g t)), then walks the group's metabolites in ascending m, reading
// B_m[n] from global memory (the basis is shared by every voxel and stays in the L2): the a_m column is E_g B_m[n]
// (formed without a_m, so a_m = 0 is fine), and T_g = sum_m a_m E_g B_m[n] gives the group's f, d and s columns
// (i 2 pi t T_g, -t T_g, -t^2 T_g).  x^ = sum_g T_g (groups ascending) and the phi column is i x^.  Every column is
// chained through dp/du.
#pragma once
#include "xm_wg.h"

#define XM_BS_MAXQ 128                 // physical parameters M + 3 G + 1
#define XM_BS_MAXP 80                  // free columns
#define XM_BS_NT 256                   // threads per workgroup
#define XM_BS_MAXE 13                  // accumulator entries per thread: ceil(((80+1)(80+2)/2 - 1) / 256)
#define XM_BS_STAGE_BYTES 65536        // LDS budget of the staged [J | r] rows
static_assert(XM_BS_NT == XM_WG_NT, "k_basis_fit and k_basis_norms run xm_wg.h's workgroup");

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
__global__ __launch_bounds__(XM_BS_NT) void k_basis_norms(const double* __restrict__ basis, int n, int skip,
                                                          double* __restrict__ bnorm) {
  __shared__ double red[XM_BS_NT];
  const int t = threadIdx.x, m = blockIdx.x;
  double c = 0.0;
  for (int i = skip + t; i < n; i += XM_BS_NT) {
    const double* b = basis + 2 * ((size_t)m * n + i);
    c += b[0] * b[0] + b[1] * b[1];
  }
  const double s = wg_sum(red, c);
  if (t == 0) bnorm[m] = sqrt(s);
}

// LDS layout of k_basis_fit (doubles): H[P*P] (upper: J^T J, lower: Cholesky factor), then vectors of P: hd (diag of
// J^T J), dsc (scale), g (J^T r), u, ut (trial), dl (step), ld (factor diagonal); then p[MAXQ], s[MAXQ] (physical
// values and slopes), red[NT], then the staged rows (xm_basis.hip: bs_lds_bytes).
struct BsLds {
  double *H, *hd, *dsc, *g, *u, *ut, *dl, *ld, *p, *s, *red, *stage;
};

XM_DEV double bs_load_re(const BasisFitArgs& A, long long row, int i, double& im) {
  if (A.is_c64) {
    const float* x = (const float*)A.x + 2 * (row * A.stride + i);
    im = (double)x[1];
    return (double)x[0];
  }
  const double* x = (const double*)A.x + 2 * (row * A.stride + i);
  im = x[1];
  return x[0];
}

// p, s <- physical values / slopes of the internal vector `u` (free parameters; fixed ones keep A.u0)
XM_DEV void bs_set_params(const BasisFitArgs& A, const BsLds& L, const double* u) {
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
XM_DEV double bs_cost(const BasisFitArgs& A, const BsLds& L, long long row, double* fit) {
  const int t = threadIdx.x;
  double c = 0.0;
  for (int i = (fit ? 0 : A.skip) + t; i < A.n; i += XM_BS_NT) {
    double mr, mi;
    bs_model_point(L.p, A.basis, A.ord, A.gs, A.M, A.G, A.n, A.dt, i, mr, mi);
    if (i >= A.skip) {
      double xi;
      const double xr = bs_load_re(A, row, i, xi);
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

// [J | r] rows of point i into r0 (real part) and r1 (imaginary part).  `phys`: J with respect to the physical
// parameters (CRLB), else to the internal ones (J_phys * dp/du).
XM_DEV void bs_stage_point(const BasisFitArgs& A, const BsLds& L, long long row, int i, bool phys, double* r0, double* r1) {
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
  const double xr = bs_load_re(A, row, i, xi);
  r0[P] = xr - mr;
  r1[P] = xi - mi;
}

// [J | r]^T [J | r] over the fitted points into H (upper), hd and g.  Thread t owns entries e = t + 256 m of the upper
// triangle of the (P+1) x (P+1) matrix in row-major order, (P, P) excluded.
XM_DEV void bs_normal(const BasisFitArgs& A, const BsLds& L, long long row, bool phys) {
  const int t = threadIdx.x, P = A.P, lda = A.lda, Q = A.q_pts, nf = A.n - A.skip;
  const int ne_all = (P + 1) * (P + 2) / 2 - 1;
  // Entries per thread.  A lane past the triangle's end sits on entry (P, P) of its row, which is staged: it sums
  // without a predicate of its own and its sum is never stored.
  const int n_own = (ne_all + XM_BS_NT - 1) / XM_BS_NT;
  int ci[XM_BS_MAXE], cj[XM_BS_MAXE];
  double acc[XM_BS_MAXE];
  {
    int i = 0, j = 0, e = 0;  // walk (i, j), i <= j <= P, to entry t, then in steps of 256
#pragma unroll
    for (int m = 0; m < XM_BS_MAXE; ++m) {
      const int target = t + XM_BS_NT * m;
      while (e < target && e < ne_all) {
        ++e;
        if (++j > P) {
          ++i;
          j = i;
        }
      }
      ci[m] = i;
      cj[m] = j;
      acc[m] = 0.0;
    }
  }
  for (int base = 0; base < nf; base += Q) {
    if (t < Q) {
      double* r0 = L.stage + (size_t)(2 * t) * lda;
      double* r1 = r0 + lda;
      if (base + t < nf) {
        bs_stage_point(A, L, row, A.skip + base + t, phys, r0, r1);
      } else {
        for (int c = 0; c <= P; ++c) r0[c] = r1[c] = 0.0;
      }
    }
    __syncthreads();
    const int rows = 2 * min(Q, nf - base);
    for (int r = 0; r < rows; ++r) {
      const double* a = L.stage + (size_t)r * lda;
#pragma unroll
      for (int m = 0; m < XM_BS_MAXE; ++m)
        if (m < n_own) acc[m] += a[ci[m]] * a[cj[m]];
    }
    __syncthreads();
  }
#pragma unroll
  for (int m = 0; m < XM_BS_MAXE; ++m) {
    if (t + XM_BS_NT * m < ne_all) {
      const int i = ci[m], j = cj[m];
      if (j == P)
        L.g[i] = acc[m];
      else if (i == j)
        L.hd[i] = acc[m];
      else
        L.H[i * P + j] = acc[m];
    }
  }
  __syncthreads();
}

// one voxel: start, Levenberg-Marquardt, CRLB pass, outputs
XM_DEV void bs_fit_row(const BasisFitArgs& A, const BsLds& L, long long row) {
  const int t = threadIdx.x, P = A.P, M = A.M, Q = A.Q;
  const int stage_doubles = 2 * A.q_pts * A.lda;
  // start: the caller's values; an amplitude without one from ||x|| / (M ||B_m||) over the fitted points
  double xx = 0.0;
  for (int i = A.skip + t; i < A.n; i += XM_BS_NT) {
    double xi;
    const double xr = bs_load_re(A, row, i, xi);
    xx += xr * xr + xi * xi;
  }
  const double xnorm = sqrt(wg_sum(L.red, xx));
  if (t < Q && A.col[t] >= 0) {
    double u = A.u0[t];
    if (t < M && isnan(u)) {
      const double bn = A.bnorm[t];
      u = wg_to_internal(A.bt[t], bn > 0.0 ? xnorm / ((double)M * bn) : 0.0, A.lo[t], A.hi[t]);
    }
    L.u[A.col[t]] = u;
  }
  if (t < P) L.dsc[t] = 0.0;
  __syncthreads();
  bs_set_params(A, L, L.u);
  double F = bs_cost(A, L, row, nullptr);
  int status = isfinite(F) ? 1 : 2, it = 0;
  double lam = 1e-3, nu = 2.0;
  bool need_jac = true;
  while (status == 1 && it < A.max_iter) {
    if (need_jac) {
      bs_set_params(A, L, L.u);
      bs_normal(A, L, row, false);
      // Marquardt scaling: the largest squared column norm seen so far (1 for a column that was always zero)
      if (t < P) L.dsc[t] = fmax(L.dsc[t], L.hd[t]);
      __syncthreads();
      need_jac = false;
    }
    ++it;
    bool ok = wg_cholesky(L.H, L.hd, L.dsc, L.ld, P, lam);
    if (ok) ok = wg_solve(L.H, L.ld, L.g, L.dl, P);
    if (!ok) {
      lam *= nu;
      nu *= 2.0;
      if (!isfinite(lam)) break;
      continue;
    }
    double dn = 0.0, un = 0.0, pred = 0.0;
    for (int j = 0; j < P; ++j) {
      const double dj = wg_lm_scale(L.dsc[j]);
      const double sd = sqrt(dj) * L.dl[j], su = sqrt(dj) * L.u[j];
      dn += sd * sd;
      un += su * su;
      pred += L.dl[j] * (lam * dj * L.dl[j] + L.g[j]);
    }
    const bool xconv = sqrt(dn) <= A.xtol * (sqrt(un) + A.xtol);
    if (t < P) L.ut[t] = L.u[t] + L.dl[t];
    __syncthreads();
    bs_set_params(A, L, L.ut);
    const double Ft = bs_cost(A, L, row, nullptr);
    if (isfinite(Ft) && Ft < F) {
      const double rho = fmin(fmax((F - Ft) / pred, 0.0), 1.0);
      const bool fconv = (F - Ft) <= A.ftol * F;
      if (t < P) L.u[t] = L.ut[t];
      __syncthreads();
      F = Ft;
      const double q = 2.0 * rho - 1.0;
      lam *= fmax(1.0 / 3.0, 1.0 - q * q * q);
      nu = 2.0;
      need_jac = true;
      if (fconv || xconv) status = 0;
    } else {
      lam *= nu;
      nu *= 2.0;
      if (xconv) status = 0;
      if (!isfinite(lam)) break;
    }
  }
  bs_set_params(A, L, L.u);
  for (int q = 0; q < Q; ++q)
    if (!isfinite(L.p[q])) status = 2;
  if (!isfinite(F)) status = 2;

  double* fit = A.fit ? A.fit + 2 * row * A.n : nullptr;
  if (status != 2) {
    // CRLB: (J^T J)^{-1} with J over the physical free columns at the solution; the caller scales by sigma
    bs_normal(A, L, row, true);
    const bool ok = wg_cholesky(L.H, L.hd, L.dsc, L.ld, P, 0.0);
    const int cap = stage_doubles / P;  // amplitudes per pass: each thread's forward substitution has P doubles
    for (int base = 0; base < M; base += cap) {
      const int m = base + t;
      if (t < cap && m < M) {
        const int j = A.col[m];
        double var = 0.0;
        if (j >= 0) {
          if (!ok) {
            var = NAN;
          } else {  // ||L^{-1} e_j||^2, forward substitution in this thread's slice of the staging area
            double* y = L.stage + (size_t)t * P;
            for (int r = j; r < P; ++r) {
              double v = r == j ? 1.0 : 0.0;
              for (int k = j; k < r; ++k) v -= L.H[r * P + k] * y[k];
              y[r] = v / L.ld[r];
              var += y[r] * y[r];
            }
          }
        }
        A.asd[row * M + m] = sqrt(var);
      }
    }
    __syncthreads();
    if (t < Q) A.params[row * Q + t] = L.p[t];
    if (fit) (void)bs_cost(A, L, row, fit);
    if (t == 0) A.rss[row] = F;
  } else {
    if (t < M) A.asd[row * M + t] = 0.0;
    if (t < Q) A.params[row * Q + t] = 0.0;
    if (fit)
      for (int i = t; i < 2 * A.n; i += XM_BS_NT) fit[i] = 0.0;
    if (t == 0) A.rss[row] = NAN;
  }
  if (t == 0) {
    A.status[row] = status;
    A.iters[row] = it;
  }
  __syncthreads();
}

__global__ __launch_bounds__(XM_BS_NT) void k_basis_fit(BasisFitArgs A) {
  extern __shared__ double bs_sm[];
  const int t = threadIdx.x, P = A.P;
  BsLds L;
  L.H = bs_sm;
  L.hd = L.H + (size_t)P * P;
  L.dsc = L.hd + P;
  L.g = L.dsc + P;
  L.u = L.g + P;
  L.ut = L.u + P;
  L.dl = L.ut + P;
  L.ld = L.dl + P;
  L.p = L.ld + P;
  L.s = L.p + XM_BS_MAXQ;
  L.red = L.s + XM_BS_MAXQ;
  L.stage = L.red + XM_BS_NT;
  __shared__ unsigned next;

  for (;;) {
    const long long row = wg_next_item(A.counter, &next);
    if (row >= A.nb) break;

    // The voxel's arguments are read again from the kernel-argument segment: carried across this loop in scalar
    // registers they are spilled as whole tuples, which costs the kernel a private segment.  z is 0.
    int z = 0;
    asm volatile("" : "+s"(z));
    bs_fit_row((&A)[z], L, row);
  }
  wg_leave(A.counter);
}
