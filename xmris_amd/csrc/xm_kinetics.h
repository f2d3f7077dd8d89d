// k_kinetics_fit: per-(voxel, product) rate fitting of a dynamic series (xm_kinetics_fit in include/xmris_hip.h;
// DESIGN.md section 19).  One wave per item, four independent items per 256-thread workgroup, no LDS and no barrier:
// the waves of a workgroup stop after different numbers of trial steps.  Lane l holds the C = ceil(T / 64) consecutive
// repetitions l C ... l C + C - 1 in registers.
//
//   Z_0 = z,  Z_j = a_j Z_{j-1} + k c_j,   a_j = e^{-x} cos th_m[j-1],  c_j = w0 Zs+_{j-1} + w1 Zs_j,  x = rho D_{j-1}
//   P^_j = Z_j sin th_m[j]
//
// Z_j = z A_j + k B_j with A_j = a_j A_{j-1} (A_0 = 1) and B_j = a_j B_{j-1} + c_j (B_0 = 0): one affine scan of the
// pairs (a_j, c_j) gives the model and its z and k columns.  The rho column G_j = a_j G_{j-1} + (da_j Z_{j-1} + k dc_j)
// is a second scan whose offsets use Z from the first.  A scan composes a lane's C pairs, runs an inclusive
// Hillis-Steele scan of the lane totals over the 64 lanes with __shfl_up, and applies the exclusive prefix locally.
//
// The heavy leaves (exp and the weights; sincos of the bound transforms) are inlined once each: the iteration is one
// loop whose head is the only place that evaluates the model, at the start, at every trial and, when the last trial was
// rejected, once more at the accepted point; and lane q transforms parameter q for the whole wave.
#pragma once
#include "xm_common.h"
#include "xm_wg.h"

#define XM_KIN_MAXM 8
#define XM_KIN_MAXT 256
#define XM_KIN_WAVES 4       // items per workgroup
#define XM_KIN_SERIES_X 0.5  // x = rho D below this: the power series of the weights; from it on: the closed forms
#define XM_KIN_TERMS 16      // terms of each series (profiles/kinetics/tolerance.txt, part c)

struct KineticsArgs {
  const double* sub;   // [nb, T]
  const double* prod;  // [nb, M, T]
  const double* wts;   // [nb, M, T] or null (all 1)
  const double* tab;   // times [T], sin th_S [T], cos th_S [T], sin th_m [M, T], cos th_m [M, T]
  double* params;      // [nb, M, 3] k, rho, z
  double* psd;         // [nb, M, 3]
  double* rss;         // [nb, M]
  double* fit;         // [nb, M, T] or null
  double* auc;         // [nb, M]
  int* status;         // [nb, M] 0 converged, 1 iteration cap, 2 non-finite, 3 fewer weighted points than parameters
  int* iters;          // [nb, M]
  long long n_items;   // nb M
  double ftol, xtol;
  int T, M, max_iter;
  double lo[XM_KIN_MAXM][3], hi[XM_KIN_MAXM][3];
  double u0[XM_KIN_MAXM][3];   // internal start of a free parameter (NaN for z: from the first weighted sample); value of a fixed one
  int bt[XM_KIN_MAXM][3];      // XM_WG_* bound type
  int col[XM_KIN_MAXM][3];     // column of a free parameter, -1 for a fixed one
  int n_free[XM_KIN_MAXM];
};

XM_DEV double kin_wave_sum(double v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;  // every lane adds the same pairs: the same bits in all 64
}

XM_DEV int kin_wave_sum_int(int v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

// sum_{i < XM_KIN_TERMS} num(i) / (i + DEN)! (-x)^i by Horner's rule
// KIND 0: num = 1; 1: i + 1; 2: -(i + 1); 3: -(i + 1)(i + 2)
template <int DEN, int KIND>
XM_DEV double kin_series(double x) {
  double acc = 0.0;
#pragma unroll
  for (int i = XM_KIN_TERMS - 1; i >= 0; --i) {
    double f = 1.0;
    for (int q = 2; q <= i + DEN; ++q) f *= (double)q;  // folded at compile time
    const double num = KIND == 0 ? 1.0 : KIND == 1 ? (double)(i + 1) : KIND == 2 ? -(double)(i + 1) : -(double)((i + 1) * (i + 2));
    acc = fma(acc, -x, num / f);
  }
  return acc;
}

// E = e^{-x}; w1 = D f2(x), w0 = D (f1(x) - f2(x)) with f1 = (1 - e^{-x}) / x, f2 = (x - 1 + e^{-x}) / x^2, and their
// derivatives with respect to rho (x = rho D).  Below XM_KIN_SERIES_X every one is a series of positive leading term,
// so nothing cancels as x -> 0; from there on expm1 carries the differences.
XM_DEV void kin_weights(double rho, double D, double& E, double& w0, double& w1, double& dw0, double& dw1) {
  const double x = rho * D;
  E = exp(-x);
  if (x < XM_KIN_SERIES_X) {
    w1 = D * kin_series<2, 0>(x);
    w0 = D * kin_series<2, 1>(x);
    dw1 = D * D * kin_series<3, 2>(x);
    dw0 = D * D * kin_series<3, 3>(x);
  } else {
    const double em = expm1(-x), x2 = x * x;
    const double f2 = (x + em) / x2;
    const double df1 = (x + (x + 1.0) * em) / x2;
    const double df2 = -(2.0 * x + (x + 2.0) * em) / (x2 * x);
    w1 = D * f2;
    w0 = D * (-em / x - f2);
    dw1 = D * D * df2;
    dw0 = D * D * (df1 - df2);
  }
}

// the exclusive prefix, over the lanes below this one, of the affine maps (at, ct): v -> at v + ct (identity in lane 0)
XM_DEV void kin_scan_exclusive(double at, double ct, int lane, double& pa, double& pc) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const double a2 = __shfl_up(at, d, 64), c2 = __shfl_up(ct, d, 64);
    if (lane >= d) {
      ct = fma(at, c2, ct);
      at = at * a2;
    }
  }
  pa = __shfl_up(at, 1, 64);
  pc = __shfl_up(ct, 1, 64);
  if (lane == 0) {
    pa = 1.0;
    pc = 0.0;
  }
}

XM_DEV double kin_sel3(int i, double a, double b, double c) { return i == 0 ? a : i == 1 ? b : c; }

// Cholesky factor of the symmetric 3 x 3 matrix (upper triangle h), in every lane alike.  false when it is not
// positive definite.
XM_DEV bool kin_chol3(double h00, double h01, double h02, double h11, double h12, double h22, double& l00, double& l10,
                      double& l20, double& l11, double& l21, double& l22) {
  l00 = l10 = l20 = l11 = l21 = l22 = 0.0;
  if (!(h00 > 0.0) || !isfinite(h00)) return false;
  l00 = sqrt(h00);
  l10 = h01 / l00;
  l20 = h02 / l00;
  const double s1 = h11 - l10 * l10;
  if (!(s1 > 0.0) || !isfinite(s1)) return false;
  l11 = sqrt(s1);
  l21 = (h12 - l20 * l10) / l11;
  const double s2 = h22 - l20 * l20 - l21 * l21;
  if (!(s2 > 0.0) || !isfinite(s2)) return false;
  l22 = sqrt(s2);
  return true;
}

template <int C>
struct KinItem {
  // the item's data, element c is repetition j = lane C + c (weight 0 and the identity map beyond T and at j = 0)
  double wy[C], wsp[C];      // w P_j and w sin th_m[j] (both 0 where w = 0: the point drops out of every sum)
  double D[C], cpm[C];       // D_{j-1} (0: identity map), cos th_m[j-1]
  double za[C], zb[C];       // Zs+_{j-1}, Zs_j
  // of the last evaluation
  double a[C], dc[C], A[C], B[C];
  double pa, pb;             // A and B just below this lane's first element
  double G[C];               // of the last kin_rho_column
};

// a, dc, A and B at rho
template <int C>
XM_DEV void kin_forward(KinItem<C>& I, double rho, int lane) {
  double cc[C];
  double at = 1.0, ct = 0.0;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    double E = 1.0, w0 = 0.0, w1 = 0.0, dw0 = 0.0, dw1 = 0.0;
    if (I.D[c] > 0.0) kin_weights(rho, I.D[c], E, w0, w1, dw0, dw1);
    I.a[c] = I.D[c] > 0.0 ? E * I.cpm[c] : 1.0;
    cc[c] = w0 * I.za[c] + w1 * I.zb[c];
    I.dc[c] = dw0 * I.za[c] + dw1 * I.zb[c];
    ct = fma(I.a[c], ct, cc[c]);
    at = I.a[c] * at;
  }
  kin_scan_exclusive(at, ct, lane, I.pa, I.pb);
  double ra = I.pa, rb = I.pb;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    ra = I.a[c] * ra;
    rb = fma(I.a[c], rb, cc[c]);
    I.A[c] = ra;
    I.B[c] = rb;
  }
}

// G_j = dZ_j / d rho from the last kin_forward
template <int C>
XM_DEV void kin_rho_column(KinItem<C>& I, double k, double z, int lane) {
  double h[C];
  double at = 1.0, ct = 0.0;
  double zprev = z * I.pa + k * I.pb;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    h[c] = I.D[c] > 0.0 ? -I.D[c] * I.a[c] * zprev + k * I.dc[c] : 0.0;  // da_j = -D a_j; the identity map has no rho in it
    zprev = z * I.A[c] + k * I.B[c];
    ct = fma(I.a[c], ct, h[c]);
    at = I.a[c] * at;
  }
  double qa, qg;
  kin_scan_exclusive(at, ct, lane, qa, qg);
#pragma unroll
  for (int c = 0; c < C; ++c) {
    qg = fma(I.a[c], qg, h[c]);
    I.G[c] = qg;
  }
}

template <int C>
XM_DEV double kin_cost(const KinItem<C>& I, double k, double z) {
  double s = 0.0;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const double r = I.wy[c] - (z * I.A[c] + k * I.B[c]) * I.wsp[c];
    s = fma(r, r, s);
  }
  return kin_wave_sum(s);
}

// J^T J (upper triangle: 00 01 02 11 12 22) and J^T r over the columns; qj: the parameter in column j (3: none, a zero
// column); sq: dp/du of parameter q (all 1: the physical columns)
template <int C>
XM_DEV void kin_normal(const KinItem<C>& I, int q0, int q1, int q2, double s0, double s1, double s2, double k, double z,
                       double* h, double* g) {
  double acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const double ws = I.wsp[c];
    const double r = I.wy[c] - (z * I.A[c] + k * I.B[c]) * ws;
    const double jq0 = ws * I.B[c] * s0, jq1 = ws * I.G[c] * s1, jq2 = ws * I.A[c] * s2;
    const double j0 = q0 == 0 ? jq0 : q0 == 1 ? jq1 : q0 == 2 ? jq2 : 0.0;
    const double j1 = q1 == 0 ? jq0 : q1 == 1 ? jq1 : q1 == 2 ? jq2 : 0.0;
    const double j2 = q2 == 0 ? jq0 : q2 == 1 ? jq1 : q2 == 2 ? jq2 : 0.0;
    acc[0] = fma(j0, j0, acc[0]);
    acc[1] = fma(j0, j1, acc[1]);
    acc[2] = fma(j0, j2, acc[2]);
    acc[3] = fma(j1, j1, acc[3]);
    acc[4] = fma(j1, j2, acc[4]);
    acc[5] = fma(j2, j2, acc[5]);
    acc[6] = fma(j0, r, acc[6]);
    acc[7] = fma(j1, r, acc[7]);
    acc[8] = fma(j2, r, acc[8]);
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) h[i] = kin_wave_sum(acc[i]);
#pragma unroll
  for (int i = 0; i < 3; ++i) g[i] = kin_wave_sum(acc[6 + i]);
}

template <int C>
__global__ __launch_bounds__(64 * XM_KIN_WAVES) void k_kinetics_fit(KineticsArgs A) {
  const int lane = threadIdx.x & 63;
  const long long item = (long long)blockIdx.x * XM_KIN_WAVES + (threadIdx.x >> 6);
  if (item >= A.n_items) return;  // the whole wave; nothing below waits for another wave
  const int T = A.T, M = A.M;
  const int m = (int)(item % M);
  const long long b = item / M;
  const double* tm = A.tab;
  const double* sS = tm + T;
  const double* cS = sS + T;
  const double* sP = cS + T + (size_t)m * T;
  const double* cP = cS + T + (size_t)M * T + (size_t)m * T;
  const double* S = A.sub + b * T;
  const double* Y = A.prod + item * T;
  const double* W = A.wts ? A.wts + item * T : nullptr;

  KinItem<C> I;
  int tw = 0;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const int j = lane * C + c;
    const bool in = j < T;
    const double w = in ? (W ? W[j] : 1.0) : 0.0;
    I.wy[c] = w > 0.0 ? w * Y[j] : 0.0;
    I.wsp[c] = w > 0.0 ? w * sP[j] : 0.0;
    tw += w > 0.0 ? 1 : 0;
    if (in && j >= 1) {
      I.D[c] = tm[j] - tm[j - 1];
      I.cpm[c] = cP[j - 1];
      I.za[c] = S[j - 1] / sS[j - 1] * cS[j - 1];
      I.zb[c] = S[j] / sS[j];
    } else {
      I.D[c] = 0.0;
      I.cpm[c] = 1.0;
      I.za[c] = I.zb[c] = 0.0;
    }
    I.a[c] = 1.0;
    I.dc[c] = I.A[c] = I.B[c] = I.G[c] = 0.0;
  }
  I.pa = 1.0;
  I.pb = 0.0;
  tw = kin_wave_sum_int(tw);

  // lane q < 3 keeps parameter q's bounds and transforms it for the wave (the lanes above repeat parameter 0)
  const int P = A.n_free[m];
  const int ql = lane < 3 ? lane : 0;
  const int my_col = A.col[m][ql], my_bt = A.bt[m][ql];
  const double my_lo = A.lo[m][ql], my_hi = A.hi[m][ql];
  double my_start = A.u0[m][ql];  // internal start, or the value of a fixed parameter
  if (A.col[m][2] >= 0 && isnan(A.u0[m][2])) {
    // z without a start: |P_j| / sin th_m[j] at the first repetition j that has weight (one lane holds it)
    int first = XM_KIN_MAXT;
#pragma unroll
    for (int c = C - 1; c >= 0; --c)
      if (I.wsp[c] > 0.0) first = lane * C + c;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) first = min(first, __shfl_xor(first, d, 64));
    const double z0 = first < XM_KIN_MAXT ? fabs(Y[first]) / sP[first] : 0.0;
    if (ql == 2) my_start = wg_to_internal(my_bt, z0, my_lo, my_hi);
  }
  int col[3], qof[3] = {3, 3, 3};
  double u[3] = {0.0, 0.0, 0.0}, ut[3], p[3] = {0.0, 0.0, 0.0}, s[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    col[q] = A.col[m][q];
    const double v = __shfl(my_start, q, 64);
#pragma unroll
    for (int j = 0; j < 3; ++j)
      if (col[q] == j) {
        u[j] = v;
        qof[j] = q;
      }
  }
  const bool rho_free = col[1] >= 0;

  enum { START, TRIAL, FINISH };
  int mode = START, status = 1, it = 0;
  double F = NAN, Ft, lam = 1e-3, nu = 2.0, pred = 0.0;
  double dsc[3] = {0.0, 0.0, 0.0}, h[6], g[3], dl[3];
  bool need_jac = true, xconv = false, stale = false;
  if (tw < P) status = 3;
  ut[0] = u[0];
  ut[1] = u[1];
  ut[2] = u[2];
  while (status != 3) {
    // the model at ut: the only place that transforms parameters and evaluates the recurrence
    {
      double pq = my_start, sq = 0.0;
      if (my_col >= 0) wg_from_internal(my_bt, kin_sel3(my_col, ut[0], ut[1], ut[2]), my_lo, my_hi, pq, sq);
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        p[q] = __shfl(pq, q, 64);
        s[q] = __shfl(sq, q, 64);
      }
    }
    if (rho_free || mode == START) kin_forward(I, p[1], lane);
    Ft = kin_cost(I, p[0], p[2]);
    if (mode == FINISH) break;
    if (mode == START) {
      F = Ft;
      mode = TRIAL;
      if (!isfinite(F)) {
        status = 2;
        break;
      }
    } else if (isfinite(Ft) && Ft < F) {
      const double rho = fmin(fmax((F - Ft) / pred, 0.0), 1.0);
      const bool fconv = (F - Ft) <= A.ftol * F;
      u[0] = ut[0];
      u[1] = ut[1];
      u[2] = ut[2];
      F = Ft;
      const double q = 2.0 * rho - 1.0;
      lam *= fmax(1.0 / 3.0, 1.0 - q * q * q);
      nu = 2.0;
      need_jac = true;
      stale = false;
      if (fconv || xconv) status = 0;
    } else {
      lam *= nu;
      nu *= 2.0;
      stale = true;
      if (xconv) status = 0;
    }
    // the next trial step
    bool go = status == 1 && isfinite(lam);
    while (go) {
      if (it >= A.max_iter) {
        go = false;
        break;
      }
      if (need_jac) {
        if (rho_free) kin_rho_column(I, p[0], p[2], lane);
        kin_normal(I, qof[0], qof[1], qof[2], s[0], s[1], s[2], p[0], p[2], h, g);
        // Marquardt scaling: the largest squared column norm seen so far (1 for a column that was always zero)
        dsc[0] = fmax(dsc[0], h[0]);
        dsc[1] = fmax(dsc[1], h[3]);
        dsc[2] = fmax(dsc[2], h[5]);
        need_jac = false;
      }
      ++it;
      // a column beyond P is zero: its diagonal is lam alone and its step 0
      const double d0 = wg_lm_scale(dsc[0]), d1 = wg_lm_scale(dsc[1]), d2 = wg_lm_scale(dsc[2]);
      double l00, l10, l20, l11, l21, l22;
      bool ok = kin_chol3(h[0] + lam * d0, h[1], h[2], h[3] + lam * d1, h[4], h[5] + lam * d2, l00, l10, l20, l11, l21, l22);
      if (ok) {
        const double y0 = g[0] / l00, y1 = (g[1] - l10 * y0) / l11, y2 = (g[2] - l20 * y0 - l21 * y1) / l22;
        dl[2] = y2 / l22;
        dl[1] = (y1 - l21 * dl[2]) / l11;
        dl[0] = (y0 - l10 * dl[1] - l20 * dl[2]) / l00;
        ok = isfinite(dl[0]) && isfinite(dl[1]) && isfinite(dl[2]);
      }
      if (!ok) {
        lam *= nu;
        nu *= 2.0;
        if (!isfinite(lam)) go = false;
        continue;
      }
      double dn = 0.0, un = 0.0;
      pred = 0.0;
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        if (j < P) {
          const double dj = wg_lm_scale(dsc[j]);
          const double sd = sqrt(dj) * dl[j], su = sqrt(dj) * u[j];
          dn += sd * sd;
          un += su * su;
          pred += dl[j] * (lam * dj * dl[j] + g[j]);
        }
        ut[j] = u[j] + dl[j];
      }
      xconv = sqrt(dn) <= A.xtol * (sqrt(un) + A.xtol);
      break;
    }
    if (!go) {
      if (!stale) break;
      mode = FINISH;  // the registers hold a rejected trial: once more at the accepted point
      ut[0] = u[0];
      ut[1] = u[1];
      ut[2] = u[2];
    }
  }
  if (status < 2 && !(isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]) && isfinite(F))) status = 2;

  double sd[3] = {0.0, 0.0, 0.0}, auc = 0.0;
  if (status < 2) {
    // the physical columns at the solution
    if (rho_free) kin_rho_column(I, p[0], p[2], lane);
    kin_normal(I, qof[0], qof[1], qof[2], 1.0, 1.0, 1.0, p[0], p[2], h, g);
    double l00, l10, l20, l11, l21, l22;
    const bool ok = tw > P && kin_chol3(h[0], h[1], h[2], P > 1 ? h[3] : 1.0, h[4], P > 2 ? h[5] : 1.0, l00, l10, l20, l11,
                                        l21, l22);
    double var[3] = {NAN, NAN, NAN};
    if (ok) {  // ||L^{-1} e_j||^2
      const double y00 = 1.0 / l00, y01 = -l10 * y00 / l11, y02 = (-l20 * y00 - l21 * y01) / l22;
      const double y11 = 1.0 / l11, y12 = -l21 * y11 / l22, y22 = 1.0 / l22;
      var[0] = y00 * y00 + y01 * y01 + y02 * y02;
      var[1] = y11 * y11 + y12 * y12;
      var[2] = y22 * y22;
    }
    const double sigma = sqrt(F / (double)(tw - P));
#pragma unroll
    for (int q = 0; q < 3; ++q)
      if (col[q] >= 0) sd[q] = sqrt(kin_sel3(col[q], var[0], var[1], var[2])) * sigma;
    // trapezoid areas over the weighted points: each joins the nearest weighted point before it
    int last = -1;
#pragma unroll
    for (int c = 0; c < C; ++c)
      if (I.wsp[c] > 0.0) last = lane * C + c;
    int below = last;  // the maximum over the lanes up to this one ...
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int o = __shfl_up(below, d, 64);
      if (lane >= d) below = max(below, o);
    }
    int prev = __shfl_up(below, 1, 64);  // ... and over the lanes below it
    if (lane == 0) prev = -1;
    double ap = 0.0, as = 0.0;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const int j = lane * C + c;
      if (I.wsp[c] > 0.0) {
        if (prev >= 0) {
          const double dt = tm[j] - tm[prev];
          ap += 0.5 * dt * (Y[j] + Y[prev]);
          as += 0.5 * dt * (S[j] + S[prev]);
        }
        prev = j;
      }
    }
    auc = kin_wave_sum(ap) / kin_wave_sum(as);
  }
  double* fit = A.fit ? A.fit + item * T : nullptr;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const int j = lane * C + c;
    if (fit && j < T) fit[j] = status < 2 ? (p[2] * I.A[c] + p[0] * I.B[c]) * sP[j] : 0.0;
  }
  if (lane < 3) {
    A.params[item * 3 + lane] = status < 2 ? kin_sel3(lane, p[0], p[1], p[2]) : 0.0;
    A.psd[item * 3 + lane] = status < 2 ? kin_sel3(lane, sd[0], sd[1], sd[2]) : 0.0;
  }
  if (lane == 0) {
    A.rss[item] = status < 2 ? F : NAN;
    A.auc[item] = auc;
    A.status[item] = status;
    A.iters[item] = it;
  }
}
