// Levenberg-Marquardt driver of the per-voxel fitting kernels (k_amares_fit, k_basis_fit): one
// 256-thread workgroup fits one voxel in lmfit's internal variables u with an analytic Jacobian.  Per Jacobian the
// augmented rows [J | r] of a round of points are staged in the LDS (two rows per point: real and imaginary part) and
// every thread accumulates its own entries of [J | r]^T [J | r] over the rounds, always in the same order -- a voxel's
// result does not depend on the batch it is in or on the workgroup that fits it.  The damped normal equations are
// solved by wg_cholesky / wg_solve (xm_wg.h).  All arithmetic fp64.
//
// A kernel supplies a model type M of static functions over its own argument struct M::Args, which carries the fields
// the driver reads by name (n, P, lda, q_pts, max_iter, ftol, xtol, col, params, asd, rss, status, iters, fit):
//   first(A), count(A)                        the first fitted point and how many are fitted
//   stage_point(A, L, row, i, phys, r0, r1)   the [J | r] rows of point i, columns 0 ... P, from L.p and L.s; `phys`:
//                                             J with respect to the physical parameters (CRLB), else the internal ones
//   start(A, L, row)                          L.u <- the start vector (the driver's barrier follows)
//   set_params(A, L, u)                       L.p, L.s <- physical values and slopes dp/du of `u`, then a barrier
//   cost(A, L, row, fit)                      sum of |x - x^|^2 at L.p, the same value in every thread; `fit`: store x^
//   n_phys(A), n_amp(A), amp_param(A, m)      physical parameters (params is [nb, n_phys]), amplitudes (asd is
//                                             [nb, n_amp]) and the parameter that is amplitude m
//   amp_factor(A, m)                          factor of amplitude m's standard deviation on its column's
#pragma once
#include "xm_wg.h"

#include <cmath>

#define XM_LM_MAXP 80             // free columns
#define XM_LM_MAXE 13             // accumulator entries per thread: ceil(((80+1)(80+2)/2 - 1) / 256)
#define XM_LM_STAGE_BYTES 65536   // LDS budget of the staged [J | r] rows
static_assert(XM_WG_NT == 256, "the driver's entry map and XM_LM_MAXE are laid out for 256 threads");
static_assert(XM_LM_MAXE * XM_WG_NT >= (XM_LM_MAXP + 1) * (XM_LM_MAXP + 2) / 2 - 1, "XM_LM_MAXE entries per thread");

// LDS layout (doubles): H[P*P] (upper: J^T J, lower: Cholesky factor), then vectors of P: hd (diag of J^T J), dsc
// (scale), g (J^T r), u, ut (trial), dl (step), ld (factor diagonal); then p[maxq], s[maxq] (physical values and
// slopes), red[256], then the staged rows (lm_lds_bytes).
struct LmLds {
  double *H, *hd, *dsc, *g, *u, *ut, *dl, *ld, *p, *s, *red, *stage;
};

XM_DEV LmLds lm_carve(double* sm, int P, int maxq) {
  LmLds L;
  L.H = sm;
  L.hd = L.H + (size_t)P * P;
  L.dsc = L.hd + P;
  L.g = L.dsc + P;
  L.u = L.g + P;
  L.ut = L.u + P;
  L.dl = L.ut + P;
  L.ld = L.dl + P;
  L.p = L.ld + P;
  L.s = L.p + maxq;
  L.red = L.s + maxq;
  L.stage = L.red + XM_WG_NT;
  return L;
}

// ---- host side ---------------------------------------------------------------------------------------------------------

// points per staging round: 128, 64 or 32 so that 2 q lda doubles fit the staging budget
__host__ inline int lm_q_pts(int lda) {
  int q = 128;
  while (q > 32 && 2 * (size_t)q * lda * sizeof(double) > XM_LM_STAGE_BYTES) q >>= 1;
  return q;
}

__host__ inline size_t lm_lds_bytes(int P, int lda, int q, int maxq) {
  return ((size_t)P * P + 7 * (size_t)P + 2 * (size_t)maxq + XM_WG_NT + 2 * (size_t)q * lda) * sizeof(double);
}

// bound type of a free parameter (lmfit's transforms)
__host__ inline signed char lm_bound_type(double lo, double hi) {
  const bool fl = std::isfinite(lo), fh = std::isfinite(hi);
  return fl && fh ? XM_WG_TWO : fl ? XM_WG_LO : fh ? XM_WG_HI : XM_WG_FREE;
}

// internal start value of the physical value v, already clipped into its bounds
__host__ inline double lm_start_value(int bt, double v, double lo, double hi) {
  if (bt == XM_WG_TWO) return std::asin(std::fmin(std::fmax(2.0 * (v - lo) / (hi - lo) - 1.0, -1.0), 1.0));
  if (bt == XM_WG_LO) return std::sqrt((v - lo + 1.0) * (v - lo + 1.0) - 1.0);
  if (bt == XM_WG_HI) return std::sqrt((hi - v + 1.0) * (hi - v + 1.0) - 1.0);
  return v;
}

// ---- device side -------------------------------------------------------------------------------------------------------

// sample i of row `row` of x (complex64 or complex128, rows `stride` elements apart): the real part, `im` the imaginary
XM_DEV double lm_load(const void* x, int is_c64, long long stride, long long row, int i, double& im) {
  if (is_c64) {
    const float* v = (const float*)x + 2 * (row * stride + i);
    im = (double)v[1];
    return (double)v[0];
  }
  const double* v = (const double*)x + 2 * (row * stride + i);
  im = v[1];
  return v[0];
}

// [J | r]^T [J | r] over the fitted points into H (upper), hd and g.  Thread t owns entries e = t + 256 m of the upper
// triangle of the (P+1) x (P+1) matrix in row-major order, (P, P) excluded.
template <class M>
XM_DEV void lm_normal(const typename M::Args& A, const LmLds& L, long long row, bool phys) {
  const int t = threadIdx.x, P = A.P, lda = A.lda, Q = A.q_pts, nf = M::count(A);
  const int ne_all = (P + 1) * (P + 2) / 2 - 1;
  // Entries per thread.  A lane past the triangle's end sits on entry (P, P) of its row, which is staged: it sums
  // without a predicate of its own and its sum is never stored.
  const int n_own = (ne_all + XM_WG_NT - 1) / XM_WG_NT;
  int ci[XM_LM_MAXE], cj[XM_LM_MAXE];
  double acc[XM_LM_MAXE];
  {
    int i = 0, j = 0, e = 0;  // walk (i, j), i <= j <= P, to entry t, then in steps of 256
#pragma unroll
    for (int m = 0; m < XM_LM_MAXE; ++m) {
      const int target = t + XM_WG_NT * m;
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
        M::stage_point(A, L, row, M::first(A) + base + t, phys, r0, r1);
      } else {
        for (int c = 0; c <= P; ++c) r0[c] = r1[c] = 0.0;
      }
    }
    __syncthreads();
    const int rows = 2 * min(Q, nf - base);
    for (int r = 0; r < rows; ++r) {
      const double* a = L.stage + (size_t)r * lda;
#pragma unroll
      for (int m = 0; m < XM_LM_MAXE; ++m)
        if (m < n_own) acc[m] += a[ci[m]] * a[cj[m]];
    }
    __syncthreads();
  }
#pragma unroll
  for (int m = 0; m < XM_LM_MAXE; ++m) {
    if (t + XM_WG_NT * m < ne_all) {
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
template <class M>
XM_DEV void lm_fit_item(const typename M::Args& A, const LmLds& L, long long row) {
  const int t = threadIdx.x, P = A.P, NA = M::n_amp(A), NQ = M::n_phys(A);
  const int stage_doubles = 2 * A.q_pts * A.lda;
  M::start(A, L, row);
  if (t < P) L.dsc[t] = 0.0;
  __syncthreads();
  M::set_params(A, L, L.u);
  double F = M::cost(A, L, row, nullptr);
  int status = isfinite(F) ? 1 : 2, it = 0;
  double lam = 1e-3, nu = 2.0;
  bool need_jac = true;
  while (status == 1 && it < A.max_iter) {
    if (need_jac) {
      M::set_params(A, L, L.u);
      lm_normal<M>(A, L, row, false);
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
    M::set_params(A, L, L.ut);
    const double Ft = M::cost(A, L, row, nullptr);
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
  M::set_params(A, L, L.u);
  for (int q = 0; q < NQ; ++q)
    if (!isfinite(L.p[q])) status = 2;
  if (!isfinite(F)) status = 2;

  double* fit = A.fit ? A.fit + 2 * row * A.n : nullptr;
  if (status != 2) {
    // CRLB: (J^T J)^{-1} with J over the physical free columns at the solution; the caller scales by sigma
    lm_normal<M>(A, L, row, true);
    const bool ok = wg_cholesky(L.H, L.hd, L.dsc, L.ld, P, 0.0);
    // Amplitudes per pass: each thread's forward substitution has P doubles.  The 16 peaks of AMARES are one pass:
    // cap = 2 q_pts lda / P >= 2 q_pts >= 64.
    const int cap = stage_doubles / P;
    for (int base = 0; base < NA; base += cap) {
      const int m = base + t;
      if (t < cap && m < NA) {
        const int j = A.col[M::amp_param(A, m)];
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
        A.asd[row * NA + m] = sqrt(var) * M::amp_factor(A, m);
      }
    }
    __syncthreads();
    if (t < NQ) A.params[row * NQ + t] = L.p[t];
    if (fit) (void)M::cost(A, L, row, fit);
    if (t == 0) A.rss[row] = F;
  } else {
    if (t < NA) A.asd[row * NA + t] = 0.0;
    if (t < NQ) A.params[row * NQ + t] = 0.0;
    if (fit)
      for (int i = t; i < 2 * A.n; i += XM_WG_NT) fit[i] = 0.0;
    if (t == 0) A.rss[row] = NAN;
  }
  if (t == 0) {
    A.status[row] = status;
    A.iters[row] = it;
  }
  __syncthreads();
}
