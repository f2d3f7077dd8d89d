// Multi-echo chemical-species separation (the project's own definition, the reference has no such
// function).  Included by xm_species.hip only.
//
// A row r (a k-space sample or a voxel) has E echoes at t_e = TE_e + tau_r and C columns (coils) that share its delay
// tau_r and field offset psi_r:  y[e, c] = sum_m rho[m, c] e^{(2 pi i f_m - R_m) t_e} e^{2 pi i psi_r t_e}.  With
// A0[e, m] = e^{(2 pi i f_m - R_m) TE_e} and P0 = pinv(A0) from the host,
//     rho[m, c] = e^{-(2 pi i f_m - R_m) tau_r} sum_e P0[m, e] e^{-2 pi i psi_r t_e} y[e, c].
// FIT: psi_r maximises G(psi) = sum_e W[e, e] + 2 sum_{e < e'} Re(W[e, e'] e^{2 pi i psi (TE_e' - TE_e)}),
// W[e, e'] = Pi[e', e] sum_c y[e, c] conj(y[e', c]), Pi the projector onto range(A0): a coarse grid of spacing
// delta = 1 / (4 (max TE - min TE)), then the safeguarded Newton iteration of k_align on the sign of G'.
//
// k_species<FIT, C128>: one 256-thread workgroup per tile of 64 consecutive rows of the inner row level; lane l of every wave
// owns row l of the tile, the four waves split the work of a stage (pairs, grid points, columns) and every wave keeps
// the row's state, computed alike.  The data are addressed where they lie: two row levels, two column levels and the
// echo level, strides in elements.  All arithmetic fp64; complex64 is widened on load and rounded once on store.
//
// Stages of FIT.  Gram: a column's E samples of the 64 rows are staged in the LDS (each wave loads every fourth echo,
// one column ahead),
// wave w accumulates the pairs w, w + 4, ... in registers over the columns in ascending order.  Coarse: the phase
// e^{2 pi i g delta Delta_p} of a grid point does not depend on the row, so the workgroup forms a table of true sines
// and cosines for K grid indices at a time (no recurrence at all) and wave w takes the indices w, w + 4 of it, +g and -g
// from the same products.  Refine: wave w sums the pairs w, w + 4, ... at the lane's own psi with true sines and
// cosines, the four partial sums are added in ascending wave order.  Apply: the waves split the columns.
#pragma once
#include "xm_common.h"

#define XM_SP_NT 256
#define XM_SP_ROWS 64
#define XM_SP_MAXE 32
#define XM_SP_MAXE_FIT 16
#define XM_SP_MAXM 8
#define XM_SP_MAXGRID 1025
#define XM_SP_K 8       // grid indices g per coarse round (with -g: 16 field values)
#define XM_SP_STEPS 40  // refine step cap (status 4)
#define XM_SP_JMAX 30   // pairs per wave: ceil(16 * 15 / 2 / 4)

// test-only bits on top of the dtype argument of xm_species_separate: leave a stage out (timing split)
#define XM_SP_SKIP_GRAM 1
#define XM_SP_SKIP_COARSE 2
#define XM_SP_SKIP_REFINE 4
#define XM_SP_SKIP_APPLY 8

struct SpeciesArgs {
  const void* x;      // echoes: element (r0, r1, c0, c1, e) at r0 xs_r0 + r1 xs_r1 + c0 xs_c0 + c1 xs_c1 + e xs_e
  void* y;            // species: the same levels with m in place of e
  const double* tab;  // TE[E], f[M], R[M], P0[M][E] (re, im); FIT: Pi[e][e] (E), Pi[e'][e] of the pairs e < e' (re, im)
  const double* tau;  // per row, or nullptr (0)
  const double* psi;  // per row, or nullptr (0); not read with FIT
  double* field;      // (nr0, nr1)
  double* residual;   // (nr0, nr1), FIT only
  int* status;        // (nr0, nr1)
  long long nr0, nr1, nc0, nc1;
  long long xs_r0, xs_r1, xs_c0, xs_c1, xs_e;
  long long ys_r0, ys_r1, ys_c0, ys_c1, ys_m;
  long long tau_s0, tau_s1, psi_s0, psi_s1;
  long long tiles1;  // tiles per index of the outer row level
  int E, M, NP, G, is_c128, skip;
  double delta, max_field;
};

__host__ __device__ inline int sp_tab_doubles(int E, int M, bool fit) {
  return E + 2 * M + 2 * M * E + (fit ? E + E * (E - 1) : 0);
}

// LDS, in doubles: the table (made even), the pair list (two ints per pair), W, the shared region (a staged column |
// the coarse table | the apply stage's phase factors), the waves' partial sums
__host__ __device__ inline size_t sp_shared_doubles(int E, int M, int NP, bool fit) {
  size_t s = 2 * (size_t)XM_SP_ROWS * (E + M);  // d[e][lane], c[m][lane]
  if (fit) {
    const size_t col = 2 * (size_t)XM_SP_ROWS * E, rot = 2 * (size_t)XM_SP_K * NP;
    s = s > col ? s : col;
    s = s > rot ? s : rot;
  }
  return s;
}
__host__ __device__ inline size_t sp_lds_bytes(int E, int M, bool fit) {
  const int NP = fit ? E * (E - 1) / 2 : 0;
  const size_t tab = (size_t)((sp_tab_doubles(E, M, fit) + 1) & ~1);
  return (tab + (size_t)((NP + 1) & ~1) + 2 * (size_t)XM_SP_ROWS * NP + sp_shared_doubles(E, M, NP, fit) +
          4 * (size_t)XM_SP_ROWS * 4) * sizeof(double);
}

// (the dtype is a template parameter: a run-time branch around every load would keep the loads of an unrolled loop from
// being issued together)
template <bool C128>
XM_DEV void sp_load(const void* p, long long i, double& re, double& im) {
  if constexpr (C128) {
    const double2 q = ((const double2*)p)[i];
    re = q.x;
    im = q.y;
  } else {
    const float2 q = ((const float2*)p)[i];
    re = (double)q.x;
    im = (double)q.y;
  }
}

template <bool C128>
XM_DEV void sp_store(void* p, long long i, double re, double im) {
  if constexpr (C128)
    ((double2*)p)[i] = make_double2(re, im);
  else
    ((float2*)p)[i] = make_float2((float)re, (float)im);
}

// (c, s) = e^{2 pi i f t}: the turn count loses its integer part before the sine and cosine (k_align's al_unit)
XM_DEV void sp_unit(double f, double t, double& c, double& s) {
  const double k = rint(f * t);
  sincospi(2.0 * fma(f, t, -k), &s, &c);
}

// of two grid points the better one: the larger G; on a tie the smaller |g|, then the negative g
XM_DEV bool sp_better(double p1, int g1, double p2, int g2) {
  if (p1 != p2) return p1 > p2;
  const int a1 = g1 < 0 ? -g1 : g1, a2 = g2 < 0 ? -g2 : g2;
  return a1 != a2 ? a1 < a2 : g1 < g2;
}

template <bool FIT, bool C128>
__global__ __launch_bounds__(XM_SP_NT) void k_species(SpeciesArgs A) {
  extern __shared__ double sp_sm[];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int E = A.E, M = A.M, NP = A.NP;
  const int ntab = sp_tab_doubles(E, M, FIT);
  double* tab = sp_sm;
  int* pair = (int*)(tab + ((ntab + 1) & ~1));                  // (e, e') of pair p
  double* W = (double*)pair + ((NP + 1) & ~1);                  // [p][lane] (re, im)
  double* sh = W + 2 * (size_t)XM_SP_ROWS * NP;                 // the shared region
  double* red = sh + sp_shared_doubles(E, M, NP, FIT);          // [wave][lane][4]
  const double* te = tab;
  const double* fm = tab + E;
  const double* rm = fm + M;
  const double* p0 = rm + M;
  const double* pd = p0 + 2 * M * E;  // FIT
  const double* pp = pd + E;          // FIT

  for (int i = t; i < ntab; i += XM_SP_NT) tab[i] = A.tab[i];
  if (FIT)
    for (int p = t; p < NP; p += XM_SP_NT) {  // pairs in ascending order (e, e'), e < e'
      int e = 0, q = p;
      while (q >= E - 1 - e) {
        q -= E - 1 - e;
        ++e;
      }
      pair[2 * p] = e;
      pair[2 * p + 1] = e + 1 + q;
    }

  const long long r0 = (long long)blockIdx.x / A.tiles1;
  const long long i1 = ((long long)blockIdx.x - r0 * A.tiles1) * XM_SP_ROWS + lane;
  const bool live = i1 < A.nr1;
  const long long r1 = live ? i1 : A.nr1 - 1;  // (a lane past the end repeats the last row and stores nothing)
  const long long xrow = r0 * A.xs_r0 + r1 * A.xs_r1, yrow = r0 * A.ys_r0 + r1 * A.ys_r1;
  const long long NC = A.nc0 * A.nc1;
  const double tau = A.tau ? A.tau[r0 * A.tau_s0 + r1 * A.tau_s1] : 0.0;
  double psi = !FIT && A.psi ? A.psi[r0 * A.psi_s0 + r1 * A.psi_s1] : 0.0;
  int status = isfinite(tau) && isfinite(psi) ? 0 : 2;
  double resid = NAN;
  __syncthreads();

  if constexpr (FIT) {
    // ---- Gram ----------------------------------------------------------------------------------------------------
    double ar[XM_SP_JMAX], ai[XM_SP_JMAX], syy = 0.0, w0 = 0.0;
#pragma unroll
    for (int j = 0; j < XM_SP_JMAX; ++j) ar[j] = ai[j] = 0.0;
    if (!(A.skip & XM_SP_SKIP_GRAM)) {
      // this wave's echoes w, w + 4, ... (at most four) of the next column wait in registers while the pairs of the
      // column before are accumulated: the loads are in flight during the arithmetic
      double nr[4], ni[4];
      auto fetch = [&](long long cc) {
        const long long c0 = cc / A.nc1, xoff = xrow + c0 * A.xs_c0 + (cc - c0 * A.nc1) * A.xs_c1;
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (wave + 4 * j < E) sp_load<C128>(A.x, xoff + (wave + 4 * j) * A.xs_e, nr[j], ni[j]);
      };
      fetch(0);
#pragma unroll 1
      for (long long cc = 0; cc < NC; ++cc) {
        __syncthreads();  // the column before is read
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (wave + 4 * j < E) {
            sh[2 * ((wave + 4 * j) * XM_SP_ROWS + lane)] = nr[j];
            sh[2 * ((wave + 4 * j) * XM_SP_ROWS + lane) + 1] = ni[j];
          }
        __syncthreads();
        if (cc + 1 < NC) fetch(cc + 1);
#pragma unroll 1
        for (int e = 0; e < E; ++e) {  // every wave alike
          const double yr = sh[2 * (e * XM_SP_ROWS + lane)], yi = sh[2 * (e * XM_SP_ROWS + lane) + 1];
          if (!isfinite(yr) || !isfinite(yi)) status = 2;
          const double n = yr * yr + yi * yi;
          syy += n;
          w0 += pd[e] * n;
        }
#pragma unroll
        for (int j = 0; j < XM_SP_JMAX; ++j) {
          const int p = wave + 4 * j;
          if (p < NP) {
            const int e = pair[2 * p], f = pair[2 * p + 1];
            const double ur = sh[2 * (e * XM_SP_ROWS + lane)], ui = sh[2 * (e * XM_SP_ROWS + lane) + 1];
            const double vr = sh[2 * (f * XM_SP_ROWS + lane)], vi = sh[2 * (f * XM_SP_ROWS + lane) + 1];
            ar[j] += ur * vr + ui * vi;  // y_e conj(y_e')
            ai[j] += ui * vr - ur * vi;
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < XM_SP_JMAX; ++j) {
      const int p = wave + 4 * j;
      if (p < NP) {
        const double qr = pp[2 * p], qi = pp[2 * p + 1];
        W[2 * (p * XM_SP_ROWS + lane)] = qr * ar[j] - qi * ai[j];
        W[2 * (p * XM_SP_ROWS + lane) + 1] = qr * ai[j] + qi * ar[j];
      }
    }
    if (!isfinite(syy)) status = 2;
    __syncthreads();  // W is complete, the staged column is read

    // ---- coarse ---------------------------------------------------------------------------------------------------
    double gbest;
    int g = 0, nf = 0;
    {
      double a = 0.0;
#pragma unroll 1
      for (int p = 0; p < NP; ++p) a += W[2 * (p * XM_SP_ROWS + lane)];
      gbest = w0 + 2.0 * a;  // g = 0, every wave alike
    }
    if (!(A.skip & XM_SP_SKIP_COARSE))
#pragma unroll 1
      for (int g0 = 0; g0 < A.G; g0 += XM_SP_K) {
        __syncthreads();  // the table before is read
        for (int i = t; i < XM_SP_K * NP; i += XM_SP_NT) {
          const int k = i / NP, p = i - k * NP;
          double c, s;
          sp_unit((double)(g0 + 1 + k) * A.delta, te[pair[2 * p + 1]] - te[pair[2 * p]], c, s);
          sh[2 * i] = c;
          sh[2 * i + 1] = s;
        }
        __syncthreads();
        for (int k = wave; k < XM_SP_K; k += 4) {
          const int gk = g0 + 1 + k;
          if (gk > A.G) break;
          double a = 0.0, b = 0.0;
#pragma unroll 4
          for (int p = 0; p < NP; ++p) {
            a += W[2 * (p * XM_SP_ROWS + lane)] * sh[2 * (k * NP + p)];
            b += W[2 * (p * XM_SP_ROWS + lane) + 1] * sh[2 * (k * NP + p) + 1];
          }
          const double gp = w0 + 2.0 * (a - b), gm = w0 + 2.0 * (a + b);  // +g and -g
          if (!isfinite(gp) || !isfinite(gm)) nf = 1;
          if (sp_better(gp, gk, gbest, g)) {
            gbest = gp;
            g = gk;
          }
          if (sp_better(gm, -gk, gbest, g)) {
            gbest = gm;
            g = -gk;
          }
        }
      }
    red[4 * (wave * XM_SP_ROWS + lane)] = gbest;
    red[4 * (wave * XM_SP_ROWS + lane) + 1] = (double)g;
    red[4 * (wave * XM_SP_ROWS + lane) + 2] = (double)nf;
    __syncthreads();
    gbest = red[4 * lane];
    g = (int)red[4 * lane + 1];
    nf = red[4 * lane + 2] != 0.0;
    for (int w = 1; w < 4; ++w) {
      const double po = red[4 * (w * XM_SP_ROWS + lane)];
      const int go = (int)red[4 * (w * XM_SP_ROWS + lane) + 1];
      if (red[4 * (w * XM_SP_ROWS + lane) + 2] != 0.0) nf = 1;
      if (sp_better(po, go, gbest, g)) {
        gbest = po;
        g = go;
      }
    }
    __syncthreads();  // red is read
    if (nf || !isfinite(gbest)) status = 2;
    if (status == 0 && !(gbest > 0.0)) status = 3;  // G is zero on the whole grid: nothing to go by

    // ---- refine: the lane's own iteration, every wave alike -----------------------------------------------------------
    enum { EDGE, NEWTON, FINAL, DONE };
    const bool refine = !(A.skip & XM_SP_SKIP_REFINE);
    int mode = status != 0 ? DONE : !refine ? FINAL : (A.G > 0 && (g == A.G || g == -A.G)) ? EDGE : NEWTON, steps = 0;
    const double end = g > 0 ? A.max_field : -A.max_field, tol = A.delta * 0x1p-40;
    double a = fmax((double)(g - 1) * A.delta, -A.max_field), b = fmin((double)(g + 1) * A.delta, A.max_field);
    double f = (double)g * A.delta, gfin = gbest;
    while (__syncthreads_or(mode != DONE)) {
      const double fe = mode == EDGE ? end : f;
      double s0 = 0.0, s1 = 0.0, s2 = 0.0;
#pragma unroll 1
      for (int p = wave; p < NP; p += 4) {
        const double dl = te[pair[2 * p + 1]] - te[pair[2 * p]];
        const double wr = W[2 * (p * XM_SP_ROWS + lane)], wi = W[2 * (p * XM_SP_ROWS + lane) + 1];
        double c, s;
        sp_unit(fe, dl, c, s);
        const double re = wr * c - wi * s, im = wr * s + wi * c;
        s0 += re;
        s1 += dl * im;
        s2 += dl * dl * re;
      }
      red[4 * (wave * XM_SP_ROWS + lane)] = s0;
      red[4 * (wave * XM_SP_ROWS + lane) + 1] = s1;
      red[4 * (wave * XM_SP_ROWS + lane) + 2] = s2;
      __syncthreads();
#define SP_SUM(k) \
  (((red[4 * lane + k] + red[4 * (XM_SP_ROWS + lane) + k]) + red[4 * (2 * XM_SP_ROWS + lane) + k]) + red[4 * (3 * XM_SP_ROWS + lane) + k])
      const double gv = w0 + 2.0 * SP_SUM(0), d1 = SP_SUM(1), d2 = SP_SUM(2);  // G' = -4 pi d1, G'' = -8 pi^2 d2
#undef SP_SUM
      if (mode == FINAL) {
        gfin = gv;
        mode = DONE;
      } else if (mode == EDGE) {
        if (g > 0 ? d1 < 0.0 : d1 > 0.0) {  // G still rises where the window ends: that end, unrefined
          status = 1;
          f = end;
          gfin = gv;
          mode = DONE;
        } else {
          mode = NEWTON;
        }
      } else if (mode == NEWTON) {
        if (d1 < 0.0)
          a = f;
        else if (d1 > 0.0)
          b = f;
        else {
          gfin = gv;
          mode = DONE;
        }
        if (mode == NEWTON) {
          double fn = d2 > 0.0 ? f - d1 / (2.0 * M_PI * d2) : NAN;  // G' / G''
          if (!(fn >= a && fn <= b)) fn = 0.5 * (a + b);           // no maximum that way, or out of the bracket: bisect
          const double step = fabs(fn - f);
          f = fn;
          if (step <= tol) {
            mode = FINAL;
          } else if (++steps == XM_SP_STEPS) {
            status = 4;
            mode = FINAL;
          }
        }
      }
      // (the barrier of the loop's condition: red is read)
    }
    if (status == 2) {
      psi = NAN;
    } else if (status == 3) {
      psi = 0.0;
      resid = 0.0;
    } else {
      psi = f;
      resid = fmax(0.0, 1.0 - gfin / syy);
    }
  }

  // ---- apply: the waves split the columns ----------------------------------------------------------------------------
  double* dph = sh;                                // [e][lane]: e^{-2 pi i psi t_e}
  double* cph = sh + 2 * (size_t)XM_SP_ROWS * E;   // [m][lane]: e^{-(2 pi i f_m - R_m) tau}
  const double psi_a = status == 2 ? 0.0 : psi, tau_a = status == 2 ? 0.0 : tau;
  __syncthreads();  // the shared region is free
  for (int e = wave; e < E; e += 4) {
    double c, s;
    sp_unit(psi_a, te[e] + tau_a, c, s);
    dph[2 * (e * XM_SP_ROWS + lane)] = c;
    dph[2 * (e * XM_SP_ROWS + lane) + 1] = -s;
  }
  for (int m = wave; m < M; m += 4) {
    double c, s;
    sp_unit(fm[m], tau_a, c, s);
    const double mag = exp(rm[m] * tau_a);
    cph[2 * (m * XM_SP_ROWS + lane)] = mag * c;
    cph[2 * (m * XM_SP_ROWS + lane) + 1] = -mag * s;
  }
  __syncthreads();
  int bad = 0;
  double syy = 0.0;
  if (!(A.skip & XM_SP_SKIP_APPLY)) {
#pragma unroll 1
    for (long long cc = wave; cc < NC; cc += 4) {
      const long long c0 = cc / A.nc1, c1 = cc - c0 * A.nc1;
      const long long xoff = xrow + c0 * A.xs_c0 + c1 * A.xs_c1, yoff = yrow + c0 * A.ys_c0 + c1 * A.ys_c1;
      double qr[XM_SP_MAXM], qi[XM_SP_MAXM];
#pragma unroll
      for (int m = 0; m < XM_SP_MAXM; ++m) qr[m] = qi[m] = 0.0;
#pragma unroll 8
      for (int e = 0; e < E; ++e) {  // (eight echoes' loads in flight per lane)
        double yr, yi;
        sp_load<C128>(A.x, xoff + e * A.xs_e, yr, yi);
        if (!FIT) {
          if (!isfinite(yr) || !isfinite(yi)) bad = 1;
          syy += yr * yr + yi * yi;
        }
        const double dr = dph[2 * (e * XM_SP_ROWS + lane)], di = dph[2 * (e * XM_SP_ROWS + lane) + 1];
        const double zr = dr * yr - di * yi, zi = dr * yi + di * yr;
#pragma unroll
        for (int m = 0; m < XM_SP_MAXM; ++m)
          if (m < M) {
            const double pr = p0[2 * (m * E + e)], pi = p0[2 * (m * E + e) + 1];
            qr[m] += pr * zr - pi * zi;
            qi[m] += pr * zi + pi * zr;
          }
      }
      const bool zero = status == 2 || status == 3;
#pragma unroll
      for (int m = 0; m < XM_SP_MAXM; ++m)
        if (m < M && live) {
          const double cr = cph[2 * (m * XM_SP_ROWS + lane)], ci = cph[2 * (m * XM_SP_ROWS + lane) + 1];
          sp_store<C128>(A.y, yoff + m * A.ys_m, zero ? 0.0 : cr * qr[m] - ci * qi[m],
                   zero ? 0.0 : cr * qi[m] + ci * qr[m]);
        }
    }
  }
  if (!FIT) {
    // a non-finite sample or an all-zero row shows only now: the waves' findings together, then zeros over the row
    red[4 * (wave * XM_SP_ROWS + lane)] = (double)bad;
    red[4 * (wave * XM_SP_ROWS + lane) + 1] = syy;
    __syncthreads();
    int anybad = 0, anyset = 0, nonfin = 0;
    for (int w = 0; w < 4; ++w) {
      if (red[4 * (w * XM_SP_ROWS + lane)] != 0.0) anybad = 1;
      const double s = red[4 * (w * XM_SP_ROWS + lane) + 1];
      if (s != 0.0) anyset = 1;
      if (!isfinite(s)) nonfin = 1;
    }
    if (!(A.skip & XM_SP_SKIP_APPLY) && status == 0) {
      if (anybad || nonfin)
        status = 2;
      else if (!anyset)
        status = 3;
      if (status != 0 && live)
#pragma unroll 1
        for (long long cc = wave; cc < NC; cc += 4) {
          const long long c0 = cc / A.nc1, yoff = yrow + c0 * A.ys_c0 + (cc - c0 * A.nc1) * A.ys_c1;
          for (int m = 0; m < M; ++m) sp_store<C128>(A.y, yoff + m * A.ys_m, 0.0, 0.0);
        }
    }
    if (status == 2) psi = NAN;
  }
  if (wave == 0 && live) {
    const long long row = r0 * A.nr1 + i1;
    A.field[row] = psi;
    A.status[row] = status;
    if (FIT) A.residual[row] = status == 2 ? NAN : resid;
  }
}
