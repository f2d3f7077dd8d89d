// AMARES time-domain fitting kernels (reference fitting/amares.py:207-488, model fitting/simulation.py:9-96).
// Included by xm_amares.hip only.
//
// Model (Vanhamme 1997 eq. 6):  x^(t) = sum_k a_k e^{i phi_k} exp(-d_k (1 - g_k + g_k t) t) e^{i 2 pi f_k t},
// t_n = n dt + t0.  Parameter q = 5 k + c of peak k, c = 0 a, 1 f [Hz], 2 d [1/s], 3 phi [rad], 4 g.
//
// k_amares_fit: one 256-thread workgroup per voxel, voxels handed out by a device counter (persistent grid), each
// fitted by the Levenberg-Marquardt driver of xm_lm.h.  This file holds what is AMARES's own: the model term, its
// Jacobian rows, the start from the prior knowledge and the links.
//
// Links (k_amares_fit<true>): a linked parameter q follows its root m (the same kind of parameter of another peak) as
// p_q = sc_q p_m + off_q and shares the root's free column, so P counts columns, not parameters.  The host fills
// col / bt / lo / hi of a linked q with the root's and composes chains; a follower of a fixed root arrives as a plain
// fixed parameter.  A staged row is zeroed and the contributions to a column are added in the order peak index
// ascending, then c ascending -- the order the oracle (tests/_amares_links.py) uses too.  k_amares_fit<false> is the
// kernel without links: it never reads lk / sc / off and every column has one contribution.
#pragma once
#include "xm_lm.h"

#define XM_AM_MAXK 16                  // peaks
#define XM_AM_MAXQ (5 * XM_AM_MAXK)    // physical parameters
static_assert(XM_AM_MAXQ <= XM_LM_MAXP, "every AMARES parameter may be a free column of the driver");

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

// The model of xm_lm.h's driver.  LINKED: parameters may share a column.
template <bool LINKED>
struct AmModel {
  using Args = AmaresFitArgs;
  XM_DEV static int first(const Args&) { return 0; }
  XM_DEV static int count(const Args& A) { return A.n; }
  XM_DEV static int n_phys(const Args& A) { return 5 * A.K; }
  XM_DEV static int n_amp(const Args& A) { return A.K; }
  XM_DEV static int amp_param(const Args&, int k) { return 5 * k; }
  // a linked amplitude's variance is sc^2 times its column's
  XM_DEV static double amp_factor(const Args& A, int k) { return LINKED && A.lk[5 * k] ? fabs(A.sc[5 * k]) : 1.0; }

  // start: every voxel from the prior knowledge
  XM_DEV static void start(const Args& A, const LmLds& L, long long) {
    for (int q = threadIdx.x; q < 5 * A.K; q += XM_WG_NT)
      if (A.col[q] >= 0 && !(LINKED && A.lk[q])) L.u[A.col[q]] = A.u0[q];
  }

  // p, s <- physical values / slopes of the internal vector `u` (free parameters; fixed ones keep A.u0).  A linked
  // parameter maps its root's value and slope; an unlinked one takes no part in that arithmetic.
  XM_DEV static void set_params(const Args& A, const LmLds& L, const double* u) {
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
  XM_DEV static double cost(const Args& A, const LmLds& L, long long row, double* fit) {
    const int t = threadIdx.x;
    double c = 0.0;
    for (int i = t; i < A.n; i += XM_WG_NT) {
      const double tt = (double)i * A.dt + A.t0;
      double mr = 0.0, mi = 0.0;
      for (int k = 0; k < A.K; ++k) {
        double tr, ti;
        am_term(L.p + 5 * k, tt, tr, ti);
        mr += tr;
        mi += ti;
      }
      double xi;
      const double xr = lm_load(A.x, A.is_c64, A.stride, row, i, xi);
      const double rr = xr - mr, ri = xi - mi;
      c += rr * rr + ri * ri;
      if (fit) {
        fit[2 * (long long)i] = mr;
        fit[2 * (long long)i + 1] = mi;
      }
    }
    return wg_sum(L.red, c);
  }

  // factor of parameter q in the Jacobian: dp/du, or in the `phys` pass its link scale (1 for an unlinked parameter,
  // which is exact); a linked parameter's slope L.s already carries sc
  XM_DEV static double factor(const Args& A, const LmLds& L, int q, bool phys) {
    return phys ? (LINKED ? A.sc[q] : 1.0) : L.s[q];
  }

  // one parameter's pair of entries into column jc of its point's staged rows
  XM_DEV static void put(double* r0, double* r1, int jc, double vr, double vi) {
    if (LINKED) {
      r0[jc] += vr;
      r1[jc] += vi;
    } else {
      r0[jc] = vr;
      r1[jc] = vi;
    }
  }

  // [J | r] rows of point i.  LINKED: the rows are zeroed and accumulated (peak ascending, then c ascending; one thread
  // owns both rows of its point).
  XM_DEV static void stage_point(const Args& A, const LmLds& L, long long row, int i, bool phys, double* r0, double* r1) {
    const int P = A.P;
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
        const double sc = factor(A, L, q, phys);
        put(r0, r1, jc, e * cs * sc, e * sn * sc);
      }
      if ((jc = A.col[q + 1]) >= 0) {
        const double w = 2.0 * M_PI * tt * factor(A, L, q + 1, phys);
        put(r0, r1, jc, -ti * w, tr * w);
      }
      if ((jc = A.col[q + 2]) >= 0) {
        const double w = -(1.0 - p[4] + p[4] * tt) * tt * factor(A, L, q + 2, phys);
        put(r0, r1, jc, tr * w, ti * w);
      }
      if ((jc = A.col[q + 3]) >= 0) {
        const double w = factor(A, L, q + 3, phys);
        put(r0, r1, jc, -ti * w, tr * w);
      }
      if ((jc = A.col[q + 4]) >= 0) {
        const double w = p[2] * tt * (1.0 - tt) * factor(A, L, q + 4, phys);
        put(r0, r1, jc, tr * w, ti * w);
      }
    }
    double xi;
    const double xr = lm_load(A.x, A.is_c64, A.stride, row, i, xi);
    r0[P] = xr - mr;
    r1[P] = xi - mi;
  }
};

template <bool LINKED>
__global__ __launch_bounds__(XM_WG_NT) void k_amares_fit(AmaresFitArgs A) {
  extern __shared__ double am_sm[];
  const LmLds L = lm_carve(am_sm, A.P, XM_AM_MAXQ);
  __shared__ unsigned next;
  for (;;) {
    const long long row = wg_next_item(A.counter, &next);
    if (row >= A.nb) break;

    // The voxel's arguments are read again from the kernel-argument segment, as in k_basis_fit (xm_basis.h): carried
    // across this loop in scalar registers they are spilled as whole tuples.  z is 0.
    int z = 0;
    asm volatile("" : "+s"(z));
    lm_fit_item<AmModel<LINKED>>((&A)[z], L, row);
  }
  wg_leave(A.counter);
}
