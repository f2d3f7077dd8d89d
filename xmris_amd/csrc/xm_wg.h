// Workgroup toolbox of the per-voxel kernels: what the persistent "one 256-thread workgroup per voxel or row" kernels
// (k_amares_fit, k_coil_combine, k_align, k_hsvd, k_denoise, k_basis_fit, k_sense_unfold) share.  Every function is
// forced inline and takes raw LDS pointers and sizes, never a kernel's own *Lds or *Args struct; every user asserts that
// its own thread count is XM_WG_NT.  Matrices are complex (interleaved re, im) and row-major unless said otherwise.
#pragma once
#include "xm_common.h"

#define XM_WG_NT 256
#define XM_WG_MAXE 9     // upper-triangle entries of a Gram matrix per thread, FMA form: ceil(64 * 65 / 2 / 256)
#define XM_WG_MAXB 9     // 16 x 16 blocks per wave, MFMA form: ceil(36 / 4)
#define XM_WG_SWEEPS 30  // Jacobi sweep cap
#define XM_WG_ROT 8      // doubles per Jacobi rotation: c, s, cos phi, sin phi, r, new G_pp, new G_qq

typedef double wg_d4 __attribute__((ext_vector_type(4)));

__host__ __device__ inline int wg_pad8(int C) { return (C + 7) & ~7; }

// ---- row ticket ------------------------------------------------------------------------------------------------------
// `counter` = {ticket, workgroups done}, zero at launch (xm_launch_items, xm_host.h).

// the workgroup's next item, the same value in every thread; `word`: an LDS word of the kernel's
XM_DEV long long wg_next_item(unsigned* counter, unsigned* word) {
  if (threadIdx.x == 0) *word = atomicAdd(counter, 1u);
  __syncthreads();
  const long long v = (long long)*word;
  __syncthreads();
  return v;
}

// the last workgroup out leaves the counters at zero
XM_DEV void wg_leave(unsigned* counter) {
  if (threadIdx.x == 0) {
    const unsigned d = atomicAdd(counter + 1, 1u);
    if (d == gridDim.x - 1u) {
      __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(counter + 1, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// ---- block sum -------------------------------------------------------------------------------------------------------

// sum of v over the workgroup, the same value in every thread (fixed tree); red: XM_WG_NT doubles
XM_DEV double wg_sum(double* red, double v) {
  const int t = threadIdx.x;
  red[t] = v;
  __syncthreads();
  for (int h = XM_WG_NT / 2; h > 0; h >>= 1) {
    if (t < h) red[t] += red[t + h];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

// ---- Hermitian C x C matrix: mirror, Gram helpers, Jacobi -----------------------------------------------------------

// lower triangle <- conjugate of the upper one, diagonal real
XM_DEV void wg_mirror(double* G, int C) {
  for (int e = threadIdx.x; e < C * C; e += XM_WG_NT) {
    const int i = e / C, j = e - i * C;
    if (i > j) {
      G[2 * e] = G[2 * (j * C + i)];
      G[2 * e + 1] = -G[2 * (j * C + i) + 1];
    } else if (i == j) {
      G[2 * e + 1] = 0.0;
    }
  }
  __syncthreads();
}

// FMA form: thread t owns entries t + 256 m of the upper triangle of G in row-major order; (ci, cj)[m] = its m-th entry,
// (0, 0) for a slot past the `ne` = C (C + 1) / 2 entries
XM_DEV void wg_gram_entries(int C, int ne, int (&ci)[XM_WG_MAXE], int (&cj)[XM_WG_MAXE]) {
  int i = 0, j = 0, e = 0;
#pragma unroll
  for (int m = 0; m < XM_WG_MAXE; ++m) {
    const int target = threadIdx.x + XM_WG_NT * m;
    while (e < target && e < ne) {
      ++e;
      if (++j >= C) {
        ++i;
        j = i;
      }
    }
    ci[m] = i < C ? i : 0;
    cj[m] = i < C ? j : 0;
  }
}

// ... and the sums of those entries into G, then the mirror
XM_DEV void wg_gram_entries_finish(double* G, int C, int ne, const int (&ci)[XM_WG_MAXE], const int (&cj)[XM_WG_MAXE],
                                   const double (&re)[XM_WG_MAXE], const double (&im)[XM_WG_MAXE]) {
#pragma unroll
  for (int m = 0; m < XM_WG_MAXE; ++m) {
    if (threadIdx.x + XM_WG_NT * m < ne) {
      G[2 * (ci[m] * C + cj[m])] = re[m];
      G[2 * (ci[m] * C + cj[m]) + 1] = im[m];
    }
  }
  __syncthreads();
  wg_mirror(G, C);
}

// MFMA form.  The real matrix Y has rows 2 c = Re and 2 c + 1 = Im of row c, so every 16 x 16 block of Y Y^T holds all
// four products of an 8 x 8 block of G.  Work items j = slice * nblk + blk (blk: a 16 x 16 block (I, J), I <= J, of
// Y Y^T, nb = wg_pad8(C) / 8 block rows, nblk = nb (nb + 1) / 2; slice: a quarter of each tile's points when nblk < 4,
// else the whole tile); wave v takes items v, v + 4, ...: (bi, bj, sl)[m] = block and slice of its m-th item.
XM_DEV void wg_gram_items(int nb, int nblk, int (&bi)[XM_WG_MAXB], int (&bj)[XM_WG_MAXB], int (&sl)[XM_WG_MAXB]) {
  const int wave = threadIdx.x >> 6;
#pragma unroll
  for (int m = 0; m < XM_WG_MAXB; ++m) {
    const int item = wave + 4 * m, blk = item % nblk;
    int i = 0, j = 0;
    for (int e = 0; e < blk; ++e)
      if (++j >= nb) {
        ++i;
        j = i;
      }
    bi[m] = i;
    bj[m] = j;
    sl[m] = item / nblk;
  }
}

// every accumulator (result r of lane l of v_mfma_f64_16x16x4_f64 is row (l >> 4) + 4 r, column l & 15) through its
// wave's scratch square (scr: 4 x 256 doubles) into the upper triangle of G, or of its slice's partial matrix
// part + sl 2 C^2 when the items are sliced (S = 4)
XM_DEV void wg_gram_store(const wg_d4 (&acc)[XM_WG_MAXB], const int (&bi)[XM_WG_MAXB], const int (&bj)[XM_WG_MAXB],
                          const int (&sl)[XM_WG_MAXB], int nitems, int S, double* scr, double* G, double* part, int C) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  scr += 256 * wave;
#pragma unroll
  for (int m = 0; m < XM_WG_MAXB; ++m) {
    const bool on = wave + 4 * m < nitems;
    if (on)
      for (int r = 0; r < 4; ++r) scr[((lane >> 4) + 4 * r) * 16 + (lane & 15)] = acc[m][r];
    __syncthreads();
    if (on) {
      const int ii = lane >> 3, jj = lane & 7, i = 8 * bi[m] + ii, j = 8 * bj[m] + jj;
      if (i < C && j < C && i <= j) {
        double* dst = S == 1 ? G : part + (size_t)sl[m] * 2 * C * C;
        dst[2 * (i * C + j)] = scr[(2 * ii) * 16 + 2 * jj] + scr[(2 * ii + 1) * 16 + 2 * jj + 1];
        dst[2 * (i * C + j) + 1] = scr[(2 * ii + 1) * 16 + 2 * jj] - scr[(2 * ii) * 16 + 2 * jj + 1];
      }
    }
    __syncthreads();
  }
}

// G <- the four partial matrices added in slice order (S = 4), then the mirror
XM_DEV void wg_gram_finish(double* G, const double* part, int C, int S) {
  if (S > 1) {
    const size_t m2 = 2 * (size_t)C * C;
    for (int e = threadIdx.x; e < C * C; e += XM_WG_NT) {
      const int i = e / C, j = e - i * C;
      if (i <= j) {
        G[2 * e] = ((part[2 * e] + part[m2 + 2 * e]) + part[2 * m2 + 2 * e]) + part[3 * m2 + 2 * e];
        G[2 * e + 1] = ((part[2 * e + 1] + part[m2 + 2 * e + 1]) + part[2 * m2 + 2 * e + 1]) + part[3 * m2 + 2 * e + 1];
      }
    }
    __syncthreads();
  }
  wg_mirror(G, C);
}

// Parallel cyclic Jacobi on the Hermitian G, eigenvectors accumulated in V (red: XM_WG_NT doubles; rot: 32 rotations of
// XM_WG_ROT doubles, then the 32 pairs of the step as ints).  Round-robin pairing of 2 ceil(C / 2) players (an odd C
// has a bye); the rotations of a step are computed by one thread each and applied by the workgroup: columns of G and V,
// then rows of G.  A pair (p, q) with G_pq = h e^{i phi}:
// J = [[c, s e^{i phi}], [-s e^{-i phi}, c]], tau = (G_qq - G_pp) / (2 h), t = sign(tau) / (|tau| + sqrt(1 + tau^2)).
// Every update is written as x - s (y + r x), y + s (x - r y) with r = s / (1 + c) (Rutishauser), and the pair's
// diagonal as G_pp - t h, G_qq + t h, so that a small rotation leaves a small rounding error.  Returns the sweeps done,
// XM_WG_SWEEPS + 1 when the off-diagonal norm never fell to eps ||G||_F, -1 when ||G||_F^2 is not finite.  Both
// norms are taken on G times the power of two that brings its largest diagonal entry to [1, 2), so the squares of small
// samples do not underflow to a test that is met at once (a G that is itself subnormal or zero is not helped by it).
XM_DEV int wg_jacobi(double* G, double* V, double* red, double* rot, int C) {
  const int t = threadIdx.x, np = (C + 1) / 2, players = 2 * np;
  for (int e = t; e < C * C; e += XM_WG_NT) {
    V[2 * e] = (e / C == e % C) ? 1.0 : 0.0;
    V[2 * e + 1] = 0.0;
  }
  double gmax = 0.0;  // (every thread alike: G is complete since wg_mirror's barrier)
  for (int i = 0; i < C; ++i) gmax = fmax(gmax, fabs(G[2 * (i * C + i)]));
  const int ex = gmax > 0.0 && isfinite(gmax) ? -ilogb(gmax) : 0;  // both norms on 2^ex G: exact, and no square underflows
  double f = 0.0;
  for (int e = t; e < 2 * C * C; e += XM_WG_NT) {
    const double g = ldexp(G[e], ex);
    f += g * g;
  }
  const double fro2 = wg_sum(red, f);  // (also the barrier after V's initialisation)
  // samples so large that G or its norm overflows: nothing to iterate on
  if (!isfinite(fro2) || !isfinite(ldexp(fro2, -2 * ex))) return -1;
  const double eps = 2.220446049250313e-16;
  int* pq = (int*)(rot + XM_WG_ROT * 32);  // pairs of the step, after the 32 rotations
  for (int sweep = 0;; ++sweep) {
    double o = 0.0;
    for (int e = t; e < C * C; e += XM_WG_NT)
      if (e / C != e % C) {
        const double gr = ldexp(G[2 * e], ex), gi = ldexp(G[2 * e + 1], ex);
        o += gr * gr + gi * gi;
      }
    const double off2 = wg_sum(red, o);
    if (!(off2 > eps * eps * fro2)) return sweep;
    if (sweep == XM_WG_SWEEPS) return XM_WG_SWEEPS + 1;
    for (int step = 0; step < players - 1; ++step) {
      if (t < np) {
        int a = t == 0 ? players - 1 : (step + t) % (players - 1);
        int b = t == 0 ? step : (step - t + players - 1) % (players - 1);
        const int p = a < b ? a : b, q = a < b ? b : a;
        double* r = rot + XM_WG_ROT * t;
        r[0] = 1.0;
        r[1] = 0.0;
        if (q < C) {
          const double gr = G[2 * (p * C + q)], gi = G[2 * (p * C + q) + 1];
          const double h = hypot(gr, gi);
          if (h > 0.0) {
            const double gpp = G[2 * (p * C + p)], gqq = G[2 * (q * C + q)];
            const double tau = (gqq - gpp) / (2.0 * h);
            const double tt = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
            const double c = 1.0 / sqrt(1.0 + tt * tt), s = tt * c;
            r[0] = c;
            r[1] = s;
            r[2] = gr / h;
            r[3] = gi / h;
            r[4] = s / (1.0 + c);
            r[5] = gpp - tt * h;
            r[6] = gqq + tt * h;
          }
        }
        pq[2 * t] = p;
        pq[2 * t + 1] = q;
      }
      __syncthreads();
      // columns: M[:, p] <- c M[:, p] - s e^{-i phi} M[:, q],  M[:, q] <- s e^{i phi} M[:, p] + c M[:, q]; M = G, V
      for (int it = t; it < 2 * C * np; it += XM_WG_NT) {
        const int e = it % (C * np), k = e % np, row = e / np;
        const double* r = rot + XM_WG_ROT * k;
        const double s = r[1];
        if (s == 0.0) continue;  // nothing to rotate (or the bye)
        const double er = r[2], ei = r[3], rr = r[4];
        double* M = it < C * np ? G : V;
        double* xp = M + 2 * (row * C + pq[2 * k]);
        double* xq = M + 2 * (row * C + pq[2 * k + 1]);
        const double xr = xp[0], xi = xp[1], yr = xq[0], yi = xq[1];
        const double ar = yr * er + yi * ei, ai = yi * er - yr * ei;  // e^{-i phi} y
        const double br = xr * er - xi * ei, bi = xi * er + xr * ei;  // e^{i phi} x
        xp[0] = xr - s * (ar + rr * xr);
        xp[1] = xi - s * (ai + rr * xi);
        xq[0] = yr + s * (br - rr * yr);
        xq[1] = yi + s * (bi - rr * yi);
      }
      __syncthreads();
      // rows: G[p, :] <- c G[p, :] - s e^{i phi} G[q, :],  G[q, :] <- s e^{-i phi} G[p, :] + c G[q, :]; the pair's own
      // 2 x 2 block is diagonal and real by construction and is stored so
      for (int it = t; it < C * np; it += XM_WG_NT) {
        const int k = it % np, j = it / np;
        const double* r = rot + XM_WG_ROT * k;
        const double s = r[1];
        if (s == 0.0) continue;
        const double er = r[2], ei = r[3], rr = r[4];
        const int p = pq[2 * k], q = pq[2 * k + 1];
        double* xp = G + 2 * (p * C + j);
        double* xq = G + 2 * (q * C + j);
        const double xr = xp[0], xi = xp[1], yr = xq[0], yi = xq[1];
        const double ar = yr * er - yi * ei, ai = yi * er + yr * ei;  // e^{i phi} y
        const double br = xr * er + xi * ei, bi = xi * er - xr * ei;  // e^{-i phi} x
        double pr = xr - s * (ar + rr * xr), pi = xi - s * (ai + rr * xi);
        double qr = yr + s * (br - rr * yr), qi = yi + s * (bi - rr * yi);
        if (j == p) {
          pr = r[5];
          pi = qr = qi = 0.0;
        } else if (j == q) {
          qr = r[6];
          qi = pr = pi = 0.0;
        }
        xp[0] = pr;
        xp[1] = pi;
        xq[0] = qr;
        xq[1] = qi;
      }
      __syncthreads();
    }
  }
}

// ---- Levenberg-Marquardt leaves (real P x P normal equations, row-major) ---------------------------------------------
// Used by the driver of k_amares_fit and k_basis_fit (xm_lm.h: the normal equations, the LM loop and the CRLB pass are
// there, once); k_kinetics_fit, one wave per item, uses the transforms, the bound types and the Marquardt scale alone.

// bound types (lmfit's transforms)
enum { XM_WG_FIXED = 0, XM_WG_FREE = 1, XM_WG_LO = 2, XM_WG_HI = 3, XM_WG_TWO = 4 };

// physical value and dp/du of a parameter from its internal value (lmfit's transforms).  A two-sided parameter at
// sin u = +-1 (on a bound) has slope exactly 0: it stays where it is, and its value is the bound itself (the formula's
// lo + (hi - lo) need not round to hi: lo = -1e6, hi = 1e-6 gives 1.0000076e-6, a value outside the bounds).
XM_DEV void wg_from_internal(int bt, double u, double lo, double hi, double& p, double& s) {
  if (bt == XM_WG_TWO) {
    double sn, cs;
    sincos(u, &sn, &cs);
    p = sn == 1.0 ? hi : lo + (sn + 1.0) * (hi - lo) * 0.5;
    s = (sn == 1.0 || sn == -1.0) ? 0.0 : cs * (hi - lo) * 0.5;
  } else if (bt == XM_WG_LO) {
    const double r = sqrt(u * u + 1.0);
    p = lo - 1.0 + r;
    s = u / r;
  } else if (bt == XM_WG_HI) {
    const double r = sqrt(u * u + 1.0);
    p = hi + 1.0 - r;
    s = -u / r;
  } else {
    p = u;
    s = 1.0;
  }
}

// internal value of the physical value v (clipped into its bounds): the inverse of wg_from_internal
XM_DEV double wg_to_internal(int bt, double v, double lo, double hi) {
  v = fmin(fmax(v, lo), hi);
  if (bt == XM_WG_TWO) return asin(fmin(fmax(2.0 * (v - lo) / (hi - lo) - 1.0, -1.0), 1.0));
  if (bt == XM_WG_LO) return sqrt((v - lo + 1.0) * (v - lo + 1.0) - 1.0);
  if (bt == XM_WG_HI) return sqrt((hi - v + 1.0) * (hi - v + 1.0) - 1.0);
  return v;
}

// Marquardt scale of a column: its largest squared norm so far, 1 for a column that has always been zero (MINPACK)
XM_DEV double wg_lm_scale(double d) { return d > 0.0 ? d : 1.0; }

// Cholesky factor of H + lam diag(dsc) (upper triangle of H and hd; lam = 0: H itself) into the lower triangle of H and
// ld.  Column by column, rows spread over the workgroup.  false (every thread alike) when not positive definite.
XM_DEV bool wg_cholesky(double* H, const double* hd, const double* dsc, double* ld, int P, double lam) {
  const int t = threadIdx.x;
  for (int j = 0; j < P; ++j) {
    double s = hd[j] + lam * wg_lm_scale(dsc[j]);
    for (int k = 0; k < j; ++k) s -= H[j * P + k] * H[j * P + k];
    if (!(s > 0.0) || !isfinite(s)) {
      __syncthreads();
      return false;
    }
    const double dj = sqrt(s);
    for (int i = j + 1 + t; i < P; i += XM_WG_NT) {
      double v = H[j * P + i];
      for (int k = 0; k < j; ++k) v -= H[i * P + k] * H[j * P + k];
      H[i * P + j] = v / dj;
    }
    if (t == 0) ld[j] = dj;
    __syncthreads();
  }
  return true;
}

// dl <- (L L^T)^{-1} g with the factor of wg_cholesky; true when every component is finite
XM_DEV bool wg_solve(const double* H, const double* ld, const double* g, double* dl, int P) {
  if (threadIdx.x == 0) {
    for (int j = 0; j < P; ++j) {
      double v = g[j];
      for (int k = 0; k < j; ++k) v -= H[j * P + k] * dl[k];
      dl[j] = v / ld[j];
    }
    for (int j = P - 1; j >= 0; --j) {
      double v = dl[j];
      for (int k = j + 1; k < P; ++k) v -= H[k * P + j] * dl[k];
      dl[j] = v / ld[j];
    }
  }
  __syncthreads();
  bool ok = true;
  for (int j = 0; j < P; ++j) ok = ok && isfinite(dl[j]);
  return ok;
}
