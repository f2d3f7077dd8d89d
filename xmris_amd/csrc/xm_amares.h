// AMARES time-domain fitting kernels (reference fitting/amares.py:207-488, model fitting/simulation.py:9-96).
// Included by xm_amares.hip only.
//
// Model (Vanhamme 1997 eq. 6):  x^(t) = sum_k a_k e^{i phi_k} exp(-d_k (1 - g_k + g_k t) t) e^{i 2 pi f_k t},
// t_n = n dt + t0.  Parameter q = 5 k + c of peak k, c = 0 a, 1 f [Hz], 2 d [1/s], 3 phi [rad], 4 g.
//
// k_amares_fit: one 256-thread workgroup per voxel, voxels handed out by a device counter (persistent grid).
// Levenberg-Marquardt in lmfit's internal variables u (bounds transform), analytic Jacobian.  Per Jacobian the
// augmented rows [J | r] of a round of points are staged in the LDS (two rows per point: real and imaginary part)
// and every thread accumulates its own entries of [J | r]^T [J | r] (upper triangle: J^T J and J^T r) over the
// rounds, always in the same order -- a voxel's result does not depend on the batch it is in or on the workgroup that
// fits it.  The damped normal equations are solved by a Cholesky factorisation in the LDS.  All arithmetic fp64.
//
// Links (k_amares_fit<true>): a linked parameter q follows its root m (the same kind of parameter of another peak) as
// p_q = sc_q p_m + off_q and shares the root's free column, so P counts columns, not parameters.  The host fills
// col / bt / lo / hi of a linked q with the root's and composes chains; a follower of a fixed root arrives as a plain
// fixed parameter.  A staged row is zeroed and the contributions to a column are added in the order peak index
// ascending, then c ascending -- the order the oracle (tests/_amares_links.py) uses too.  k_amares_fit<false> is the
// kernel without links: it never reads lk / sc / off and every column has one contribution.
#pragma once
#include "xm_wg.h"

#define XM_AM_MAXK 16                  // peaks
#define XM_AM_MAXQ (5 * XM_AM_MAXK)    // physical parameters
#define XM_AM_NT 256                   // threads per workgroup
#define XM_AM_MAXE 13                  // accumulator entries per thread: ceil(((80+1)(80+2)/2 - 1) / 256)
#define XM_AM_STAGE_BYTES 65536        // LDS budget of the staged [J | r] rows
static_assert(XM_AM_NT == XM_WG_NT, "k_amares_fit runs xm_wg.h's workgroup");

struct AmaresFitArgs {
  const void* x;       // rows of n complex samples (complex64 or complex128), `stride` elements apart
  long long stride, nb;
  int n, is_c64;
  double dt, t0;
  int K, P, max_iter;  // peaks, free parameters
  int lda, q_pts;      // staged row stride (P + 1 doubles), points per staging round
  double ftol, xtol;
  double* params;      // [nb, K, 5] physical
  double* asd;         // [nb, K] standard deviation of a_k (0 for a fixed amplitude)
  double* rss;         // [nb]
  int* status;         // [nb] 0 converged, 1 iteration cap, 2 non-finite
  int* iters;          // [nb]
  double* fit;         // [nb, n] complex128, or nullptr
  unsigned* counter;   // [2] zero at launch: row ticket, workgroups done
  double u0[XM_AM_MAXQ];  // free: internal start value; fixed: the physical value
  double lo[XM_AM_MAXQ], hi[XM_AM_MAXQ];
  signed char bt[XM_AM_MAXQ];   // XM_WG_* bound type (xm_wg.h)
  signed char col[XM_AM_MAXQ];  // free column of parameter q, -1 when fixed
  signed char lk[XM_AM_MAXQ];   // 1: q follows the root that owns col[q] (free roots only)
  double sc[XM_AM_MAXQ], off[XM_AM_MAXQ];  // p_q = sc * p_root + off where lk[q]; 1 and 0 elsewhere
};
static_assert(sizeof(AmaresFitArgs) <= 4096, "AmaresFitArgs must fit the 4 KB kernel-argument limit");

// One peak's term at time t: T = a e^{-d (1 - g + g t) t} e^{i (phi + 2 pi f t)}.  One exp and one sincos.
XM_DEV void am_term(const double* p, double t, double& tr, double& ti) {
  const double e = p[0] * exp(-p[2] * (1.0 - p[4] + p[4] * t) * t);
  double s, c;
  sincos(p[3] + 2.0 * M_PI * p[1] * t, &s, &c);
  tr = e * c;
  ti = e * s;
}

__global__ void k_amares_model(const double* __restrict__ params, long long nb, int K, int n, double dt, double t0,
                               double* __restrict__ out) {
  const long long total = nb * (long long)n;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
    const long long b = e / n;
    const int i = (int)(e - b * n);
    const double t = (double)i * dt + t0;
    const double* p = params + b * 5 * K;
    double mr = 0.0, mi = 0.0;
    for (int k = 0; k < K; ++k) {
      double tr, ti;
      am_term(p + 5 * k, t, tr, ti);
      mr += tr;
      mi += ti;
    }
    out[2 * e] = mr;
    out[2 * e + 1] = mi;
  }
}

// LDS layout of k_amares_fit (doubles): H[P*P] (upper: J^T J, lower: Cholesky factor), then vectors of P: hd (diag of
// J^T J), dsc (scale), g (J^T r), u, ut (trial), dl (step), ld (factor diagonal); then p[MAXQ], s[MAXQ] (physical
// values and slopes), red[NT], then the staged rows (xm_amares.hip: am_lds_bytes).
struct AmLds {
  double *H, *hd, *dsc, *g, *u, *ut, *dl, *ld, *p, *s, *red, *stage;
};

XM_DEV double am_load_re(const AmaresFitArgs& A, long long row, int i, double& im) {
  if (A.is_c64) {
    const float* x = (const float*)A.x + 2 * (row * A.stride + i);
    im = (double)x[1];
    return (double)x[0];
  }
  const double* x = (const double*)A.x + 2 * (row * A.stride + i);
  im = x[1];
  return x[0];
}

// p, s <- physical values / slopes of the internal vector `u` (free parameters; fixed ones keep A.u0).  A linked
// parameter maps its root's value and slope; an unlinked one takes no part in that arithmetic.
template <bool LINKED>
XM_DEV void am_set_params(const AmaresFitArgs& A, const AmLds& L, const double* u) {
  const int t = threadIdx.x;
  if (t < 5 * A.K) {
    const int j = A.col[t];
    double p = A.u0[t], s = 0.0;
    if (j >= 0) wg_from_internal(A.bt[t], u[j], A.lo[t], A.hi[t], p, s);
    if (LINKED && A.lk[t]) {
      p = A.sc[t] * p + A.off[t];
      s = A.sc[t] * s;
    }
    L.p[t] = p;
    L.s[t] = s;
  }
  __syncthreads();
}

// sum over the row's points of |x - x^|^2 (every thread the same value; fixed summation order).  `fit`: also store x^.
XM_DEV double am_cost(const AmaresFitArgs& A, const AmLds& L, long long row, double* fit) {
  const int t = threadIdx.x;
  double c = 0.0;
  for (int i = t; i < A.n; i += XM_AM_NT) {
    const double tt = (double)i * A.dt + A.t0;
    double mr = 0.0, mi = 0.0;
    for (int k = 0; k < A.K; ++k) {
      double tr, ti;
      am_term(L.p + 5 * k, tt, tr, ti);
      mr += tr;
      mi += ti;
    }
    double xi;
    const double xr = am_load_re(A, row, i, xi);
    const double rr = xr - mr, ri = xi - mi;
    c += rr * rr + ri * ri;
    if (fit) {
      fit[2 * (long long)i] = mr;
      fit[2 * (long long)i + 1] = mi;
    }
  }
  return wg_sum(L.red, c);
}

// factor of parameter q in the physical Jacobian: its link scale (1 for an unlinked parameter, which is exact)
template <bool LINKED>
XM_DEV double am_phys(const AmaresFitArgs& A, int q) {
  return LINKED ? A.sc[q] : 1.0;
}

// one parameter's pair of entries into column jc of its point's staged rows
template <bool LINKED>
XM_DEV void am_put(double* r0, double* r1, int jc, double vr, double vi) {
  if (LINKED) {
    r0[jc] += vr;
    r1[jc] += vi;
  } else {
    r0[jc] = vr;
    r1[jc] = vi;
  }
}

// [J | r]^T [J | r] over the row's points into H (upper), hd and g.  `phys`: J with respect to the physical parameters
// (CRLB), else to the internal ones (J_phys * dp/du).  Thread t owns entries e = t + 256 m of the upper triangle of the
// (P+1) x (P+1) matrix in row-major order, (P, P) excluded.  LINKED: parameters may share a column, so a point's rows
// are zeroed and accumulated (peak ascending, then c ascending; one thread owns both rows of its point); the factor of
// a linked parameter is sc * dp/du, and sc alone in the `phys` pass.
template <bool LINKED>
XM_DEV void am_normal(const AmaresFitArgs& A, const AmLds& L, long long row, bool phys) {
  const int t = threadIdx.x, P = A.P, lda = A.lda, Q = A.q_pts;
  const int ne_all = (P + 1) * (P + 2) / 2 - 1;
  int ci[XM_AM_MAXE], cj[XM_AM_MAXE];
  double acc[XM_AM_MAXE];
  {
    int i = 0, j = 0, e = 0;  // walk (i, j), i <= j <= P, to entry t, then in steps of 256
#pragma unroll
    for (int m = 0; m < XM_AM_MAXE; ++m) {
      const int target = t + XM_AM_NT * m;
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
  for (int base = 0; base < A.n; base += Q) {
    if (t < Q) {
      double* r0 = L.stage + (size_t)(2 * t) * lda;
      double* r1 = r0 + lda;
      const int i = base + t;
      if (i < A.n) {
        const double tt = (double)i * A.dt + A.t0;
        double mr = 0.0, mi = 0.0;
        if (LINKED)
          for (int c = 0; c < P; ++c) r0[c] = r1[c] = 0.0;
        for (int k = 0; k < A.K; ++k) {
          const double* p = L.p + 5 * k;
          double tr, ti;
          am_term(p, tt, tr, ti);
          mr += tr;
          mi += ti;
          // d/da = T / a (recomputed from the exponent so that a = 0 is fine), d/df = i 2 pi t T,
          // d/dd = -(1 - g + g t) t T, d/dphi = i T, d/dg = d t (1 - t) T
          const int q = 5 * k;
          int jc = A.col[q];
          if (jc >= 0) {
            const double e = exp(-p[2] * (1.0 - p[4] + p[4] * tt) * tt);
            double sn, cs;
            sincos(p[3] + 2.0 * M_PI * p[1] * tt, &sn, &cs);
            const double sc = phys ? am_phys<LINKED>(A, q) : L.s[q];
            am_put<LINKED>(r0, r1, jc, e * cs * sc, e * sn * sc);
          }
          if ((jc = A.col[q + 1]) >= 0) {
            const double w = 2.0 * M_PI * tt * (phys ? am_phys<LINKED>(A, q + 1) : L.s[q + 1]);
            am_put<LINKED>(r0, r1, jc, -ti * w, tr * w);
          }
          if ((jc = A.col[q + 2]) >= 0) {
            const double w = -(1.0 - p[4] + p[4] * tt) * tt * (phys ? am_phys<LINKED>(A, q + 2) : L.s[q + 2]);
            am_put<LINKED>(r0, r1, jc, tr * w, ti * w);
          }
          if ((jc = A.col[q + 3]) >= 0) {
            const double w = phys ? am_phys<LINKED>(A, q + 3) : L.s[q + 3];
            am_put<LINKED>(r0, r1, jc, -ti * w, tr * w);
          }
          if ((jc = A.col[q + 4]) >= 0) {
            const double w = p[2] * tt * (1.0 - tt) * (phys ? am_phys<LINKED>(A, q + 4) : L.s[q + 4]);
            am_put<LINKED>(r0, r1, jc, tr * w, ti * w);
          }
        }
        double xi;
        const double xr = am_load_re(A, row, i, xi);
        r0[P] = xr - mr;
        r1[P] = xi - mi;
      } else {
        for (int c = 0; c <= P; ++c) r0[c] = r1[c] = 0.0;
      }
    }
    __syncthreads();
    const int rows = 2 * min(Q, A.n - base);
    for (int r = 0; r < rows; ++r) {
      const double* a = L.stage + (size_t)r * lda;
#pragma unroll
      for (int m = 0; m < XM_AM_MAXE; ++m)
        if (t + XM_AM_NT * m < ne_all) acc[m] += a[ci[m]] * a[cj[m]];
    }
    __syncthreads();
  }
#pragma unroll
  for (int m = 0; m < XM_AM_MAXE; ++m) {
    if (t + XM_AM_NT * m < ne_all) {
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

template <bool LINKED>
__global__ __launch_bounds__(XM_AM_NT) void k_amares_fit(AmaresFitArgs A) {
  extern __shared__ double am_sm[];
  const int t = threadIdx.x, P = A.P, K = A.K;
  AmLds L;
  L.H = am_sm;
  L.hd = L.H + (size_t)P * P;
  L.dsc = L.hd + P;
  L.g = L.dsc + P;
  L.u = L.g + P;
  L.ut = L.u + P;
  L.dl = L.ut + P;
  L.ld = L.dl + P;
  L.p = L.ld + P;
  L.s = L.p + XM_AM_MAXQ;
  L.red = L.s + XM_AM_MAXQ;
  L.stage = L.red + XM_AM_NT;
  __shared__ unsigned next;

  for (;;) {
    const long long row = wg_next_item(A.counter, &next);
    if (row >= A.nb) break;

    // start: every voxel from the prior knowledge
    for (int q = t; q < 5 * K; q += XM_AM_NT)
      if (A.col[q] >= 0 && !(LINKED && A.lk[q])) L.u[A.col[q]] = A.u0[q];
    if (t < P) L.dsc[t] = 0.0;
    __syncthreads();
    am_set_params<LINKED>(A, L, L.u);
    double F = am_cost(A, L, row, nullptr);
    int status = isfinite(F) ? 1 : 2, it = 0;
    double lam = 1e-3, nu = 2.0;
    bool need_jac = true;
    while (status == 1 && it < A.max_iter) {
      if (need_jac) {
        am_set_params<LINKED>(A, L, L.u);
        am_normal<LINKED>(A, L, row, false);
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
      am_set_params<LINKED>(A, L, L.ut);
      const double Ft = am_cost(A, L, row, nullptr);
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
    am_set_params<LINKED>(A, L, L.u);
    for (int q = 0; q < 5 * K; ++q)
      if (!isfinite(L.p[q])) status = 2;
    if (!isfinite(F)) status = 2;

    double* fit = A.fit ? A.fit + 2 * row * A.n : nullptr;
    if (status != 2) {
      // CRLB: sigma^2 (J^T J)^{-1} with J over the physical free columns at the solution; the caller scales.  A linked
      // amplitude's variance is sc^2 times its column's.
      am_normal<LINKED>(A, L, row, true);
      const bool ok = wg_cholesky(L.H, L.hd, L.dsc, L.ld, P, 0.0);
      if (t < K) {
        const int j = A.col[5 * t];
        double var = 0.0;
        if (j >= 0) {
          if (!ok) {
            var = NAN;
          } else {  // ||L^{-1} e_j||^2, forward substitution in this thread's slice of the staging area
            double* y = L.stage + (size_t)t * P;
            for (int m = j; m < P; ++m) {
              double v = m == j ? 1.0 : 0.0;
              for (int k = j; k < m; ++k) v -= L.H[m * P + k] * y[k];
              y[m] = v / L.ld[m];
              var += y[m] * y[m];
            }
          }
        }
        double sd = sqrt(var);
        if (LINKED && A.lk[5 * t]) sd *= fabs(A.sc[5 * t]);
        A.asd[row * K + t] = sd;
      }
      if (t < 5 * K) A.params[row * 5 * K + t] = L.p[t];
      if (fit) (void)am_cost(A, L, row, fit);
      if (t == 0) A.rss[row] = F;
    } else {
      if (t < K) A.asd[row * K + t] = 0.0;
      if (t < 5 * K) A.params[row * 5 * K + t] = 0.0;
      if (fit)
        for (int i = t; i < 2 * A.n; i += XM_AM_NT) fit[i] = 0.0;
      if (t == 0) A.rss[row] = NAN;
    }
    if (t == 0) {
      A.status[row] = status;
      A.iters[row] = it;
    }
    __syncthreads();
  }
  wg_leave(A.counter);
}
