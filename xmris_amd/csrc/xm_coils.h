// Coil combination kernel (the project's own definition, the reference has no such function).
// Included by xm_coils.hip, and by xm_denoise.h for the staging and Gram functions.  The block sum, the mirror, the
// Gram maps and stores, the Jacobi iteration and the voxel ticket are xm_wg.h's.
//
// One voxel: X = its C x N FIDs (coil by time), R = the same voxel of the reference (or X), Linv = L^{-1} of the noise
// covariance Psi = L L^H (or the identity).  G = Linv (R R^H) Linv^H; u = the eigenvector of G's largest eigenvalue
// (svd) or Linv mean(R[:, :n_points]) normalised (first_point); w = Linv^H u, turned so that w^H R[:, 0] is real and
// non-negative; y = w^H X; quality = u^H G u / trace(G).
//
// k_coil_combine: one 256-thread workgroup per voxel, voxels handed out by a device counter (persistent grid, the
// idiom of k_amares_fit).  The data are viewed as (n_outer, C, n_inner, N): voxel (a, b) starts at
// ((a C) n_inner + b) N and its coils are n_inner N elements apart, so "coil next to time" and "coil in front" need no
// permuted copy.  All arithmetic fp64; complex64 input is widened on load.
//
// Pass 1 stages tiles of XM_CC_Q time points of R in the LDS as the real matrix Y with rows 2c = Re R_c and
// 2c + 1 = Im R_c (the rows of [Re R; Im R], interleaved so that every 16 x 16 block of Y Y^T holds all four products
// of an 8 x 8 block of G).  Rows are zero-filled up to a multiple of 16 and tiles up to XM_CC_Q points; nothing outside
// C or N_R is read.  The upper block triangle of Y Y^T is accumulated on v_mfma_f64_16x16x4_f64 (C >= 8), tile after
// tile and within a tile in ascending time, or by plain FMAs, one upper-triangle entry of G per thread slot (C < 8).
// The order over time never depends on the batch or on the workgroup.  With fewer than 4 blocks (C <= 16) the four
// waves take a quarter of each tile's points each and the four partial matrices are added in wave order.
#pragma once
#include "xm_wg.h"

#define XM_CC_MAXC 64
#define XM_CC_NT 256
#define XM_CC_Q 64       // time points per staged tile
#define XM_CC_LDQ 68     // row stride of the staged tile in doubles: lanes (i, k) of an MFMA operand hit banks 4 i + k
#define XM_CC_SMALL 1824 // doubles after the two matrices: scr[1024], red[256], w[128], u[128], rot[256], pairs[32]
static_assert(XM_CC_NT == XM_WG_NT, "k_coil_combine runs xm_wg.h's workgroup");
static_assert(XM_CC_MAXC * (XM_CC_MAXC + 1) / 2 <= XM_WG_MAXE * XM_WG_NT, "the FMA form's slots must hold XM_CC_MAXC coils");
static_assert((XM_CC_MAXC / 8) * (XM_CC_MAXC / 8 + 1) / 2 <= 4 * XM_WG_MAXB, "the MFMA form's slots must hold XM_CC_MAXC coils");

struct CoilArgs {
  const void* x;       // (n_outer, C, n_inner, N) complex64 / complex128
  const void* ref;     // (n_outer, C, n_inner, NR), or x itself
  void* y;             // (n_outer, n_inner, N), the input's dtype
  double* w;           // (n_outer, n_inner, C) complex128
  double* quality;     // (n_outer, n_inner)
  int* status;         // (n_outer, n_inner) 0 ok, 1 all-zero reference, 2 non-finite sample, 3 sweep cap
  const double* linv;  // C x C complex128 row-major, or nullptr for the identity
  long long nv, n_inner;
  int C, N, NR, n_points, is_c128;
  unsigned* counter;   // [2] zero at launch: voxel ticket, workgroups done
};

// doubles of the second LDS matrix: the staged tile, then L^{-1} G, then the eigenvectors
__host__ __device__ inline size_t cc_b_doubles(int C) {
  const size_t stage = 2 * (size_t)wg_pad8(C) * XM_CC_LDQ, mat = 2 * (size_t)C * C;
  return stage > mat ? stage : mat;
}
__host__ __device__ inline size_t cc_lds_bytes(int C) {
  return (2 * (size_t)C * C + cc_b_doubles(C) + XM_CC_SMALL) * sizeof(double);
}

struct CcLds {
  double *G, *B, *scr, *red, *w, *u, *rot;
};

// the voxel's reference (R) and data (X): first element and coil stride
struct CcVoxel {
  long long roff, rcs, xoff, xcs;
};

XM_DEV void cc_load(const void* p, int c128, long long i, double& re, double& im) {
  if (c128) {
    const double* q = (const double*)p + 2 * i;
    re = q[0];
    im = q[1];
  } else {
    const float* q = (const float*)p + 2 * i;
    re = (double)q[0];
    im = (double)q[1];
  }
}

// tile [t0, t0 + Q) of R into Y (the B matrix); flags: bit 0 a non-finite sample, bit 1 a nonzero one.  GATHER
// (k_denoise, xm_denoise.h): row c starts at rows[c], a table in the LDS, instead of V.roff + c V.rcs
template <bool GATHER = false>
XM_DEV void cc_stage(const CoilArgs& A, const CcLds& L, const CcVoxel& V, int t0, int& flags,
                     const long long* rows = nullptr) {
  const int t = threadIdx.x, tt = t & (XM_CC_Q - 1), Cp = wg_pad8(A.C);
  for (int c = t / XM_CC_Q; c < Cp; c += XM_CC_NT / XM_CC_Q) {
    double re = 0.0, im = 0.0;
    if (c < A.C && t0 + tt < A.NR) {
      cc_load(A.ref, A.is_c128, (GATHER ? rows[c] : V.roff + c * V.rcs) + t0 + tt, re, im);
      if (!isfinite(re) || !isfinite(im)) flags |= 1;
      if (re != 0.0 || im != 0.0) flags |= 2;
    }
    L.B[(size_t)(2 * c) * XM_CC_LDQ + tt] = re;
    L.B[(size_t)(2 * c + 1) * XM_CC_LDQ + tt] = im;
  }
}

// G <- R R^H by plain FMAs: thread t owns entries t + 256 m of the upper triangle in row-major order
template <bool GATHER = false>
XM_DEV void cc_gram_fma(const CoilArgs& A, const CcLds& L, const CcVoxel& V, int& flags,
                        const long long* rows = nullptr) {
  const int t = threadIdx.x, C = A.C, ne = C * (C + 1) / 2;
  int ci[XM_WG_MAXE], cj[XM_WG_MAXE];
  double re[XM_WG_MAXE] = {}, im[XM_WG_MAXE] = {};
  wg_gram_entries(C, ne, ci, cj);
  for (int t0 = 0; t0 < A.NR; t0 += XM_CC_Q) {
    cc_stage<GATHER>(A, L, V, t0, flags, rows);
    __syncthreads();
#pragma unroll
    for (int m = 0; m < XM_WG_MAXE; ++m) {
      if (t + XM_CC_NT * m < ne) {
        const double* ai = L.B + (size_t)(2 * ci[m]) * XM_CC_LDQ;
        const double* aj = L.B + (size_t)(2 * cj[m]) * XM_CC_LDQ;
#pragma unroll 4
        for (int k = 0; k < XM_CC_Q; ++k) {
          re[m] += ai[k] * aj[k] + ai[XM_CC_LDQ + k] * aj[XM_CC_LDQ + k];
          im[m] += ai[XM_CC_LDQ + k] * aj[k] - ai[k] * aj[XM_CC_LDQ + k];
        }
      }
    }
    __syncthreads();
  }
  wg_gram_entries_finish(L.G, C, ne, ci, cj, re, im);
}

// G <- R R^H on the fp64 matrix cores, work items (block (I, J), slice) as wg_gram_items hands them out.  Operands of
// v_mfma_f64_16x16x4_f64: lane l holds A[l & 15][l >> 4] and B[l >> 4][l & 15], i.e. Y[16 I + (l & 15)][k] and
// Y[16 J + (l & 15)][k] with k = 4 kk + (l >> 4).
template <bool GATHER = false>
XM_DEV void cc_gram_mfma(const CoilArgs& A, const CcLds& L, const CcVoxel& V, int& flags,
                         const long long* rows = nullptr) {
  const int t = threadIdx.x, C = A.C, wave = t >> 6, lane = t & 63;
  const int nb = wg_pad8(C) / 8, nblk = nb * (nb + 1) / 2, S = nblk < 4 ? 4 : 1, nitems = nblk * S;
  const int ksteps = XM_CC_Q / 4 / S;
  int bi[XM_WG_MAXB], bj[XM_WG_MAXB], sl[XM_WG_MAXB];
  wg_d4 acc[XM_WG_MAXB];
  wg_gram_items(nb, nblk, bi, bj, sl);
#pragma unroll
  for (int m = 0; m < XM_WG_MAXB; ++m) acc[m] = wg_d4{0.0, 0.0, 0.0, 0.0};
  for (int t0 = 0; t0 < A.NR; t0 += XM_CC_Q) {
    cc_stage<GATHER>(A, L, V, t0, flags, rows);
    __syncthreads();
#pragma unroll
    for (int m = 0; m < XM_WG_MAXB; ++m) {
      if (wave + 4 * m < nitems) {  // wave-uniform: the MFMA runs with every lane on
        const int k0 = 4 * ksteps * sl[m] + (lane >> 4);
        const double* ya = L.B + (size_t)(16 * bi[m] + (lane & 15)) * XM_CC_LDQ + k0;
        const double* yb = L.B + (size_t)(16 * bj[m] + (lane & 15)) * XM_CC_LDQ + k0;
        for (int kk = 0; kk < ksteps; ++kk)
          acc[m] = __builtin_amdgcn_mfma_f64_16x16x4f64(ya[4 * kk], yb[4 * kk], acc[m], 0, 0, 0);
      }
    }
    __syncthreads();
  }
  // the slices' partial matrices go to B: the tile is done
  wg_gram_store(acc, bi, bj, sl, nitems, S, L.scr, L.G, L.B, C);
  wg_gram_finish(L.G, L.B, C, S);
}

// G <- Linv G Linv^H through B
XM_DEV void cc_whiten(const CoilArgs& A, const CcLds& L) {
  const int C = A.C;
  for (int e = threadIdx.x; e < C * C; e += XM_CC_NT) {
    const int i = e / C, j = e - i * C;
    double sr = 0.0, si = 0.0;
    for (int k = 0; k < C; ++k) {
      const double lr = A.linv[2 * (i * C + k)], li = A.linv[2 * (i * C + k) + 1];
      const double gr = L.G[2 * (k * C + j)], gi = L.G[2 * (k * C + j) + 1];
      sr += lr * gr - li * gi;
      si += lr * gi + li * gr;
    }
    L.B[2 * e] = sr;
    L.B[2 * e + 1] = si;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < C * C; e += XM_CC_NT) {
    const int i = e / C, j = e - i * C;
    if (i > j) continue;
    double sr = 0.0, si = 0.0;
    for (int k = 0; k < C; ++k) {  // T[i][k] conj(Linv[j][k])
      const double tr = L.B[2 * (i * C + k)], ti = L.B[2 * (i * C + k) + 1];
      const double lr = A.linv[2 * (j * C + k)], li = A.linv[2 * (j * C + k) + 1];
      sr += tr * lr + ti * li;
      si += ti * lr - tr * li;
    }
    L.G[2 * e] = sr;
    L.G[2 * e + 1] = si;
  }
  __syncthreads();
  wg_mirror(L.G, C);
}

// the outputs of a voxel that is not combined: y and w zero, quality 0 (status 1) or NaN (status 2)
XM_DEV void cc_degenerate(const CoilArgs& A, long long v, int status) {
  const int t = threadIdx.x;
  for (int i = t; i < A.N; i += XM_CC_NT) {
    if (A.is_c128) {
      ((double*)A.y)[2 * (v * A.N + i)] = 0.0;
      ((double*)A.y)[2 * (v * A.N + i) + 1] = 0.0;
    } else {
      ((float*)A.y)[2 * (v * A.N + i)] = 0.0f;
      ((float*)A.y)[2 * (v * A.N + i) + 1] = 0.0f;
    }
  }
  for (int i = t; i < 2 * A.C; i += XM_CC_NT) A.w[2 * v * A.C + i] = 0.0;
  if (t == 0) {
    A.quality[v] = status == 2 ? NAN : 0.0;
    A.status[v] = status;
  }
}

// 1 when the voxel's X holds a non-finite sample
XM_DEV int cc_x_bad(const CoilArgs& A, const CcVoxel& V) {
  int bad = 0;
  for (int c = 0; c < A.C; ++c)
    for (int i = threadIdx.x; i < A.N; i += XM_CC_NT) {
      double re, im;
      cc_load(A.x, A.is_c128, V.xoff + c * V.xcs + i, re, im);
      if (!isfinite(re) || !isfinite(im)) bad = 1;
    }
  return __syncthreads_or(bad);
}

// w <- Linv^H u, turned so that w^H R[:, 0] >= 0 (left as it is when that product is zero)
XM_DEV void cc_weights(const CoilArgs& A, const CcLds& L, const CcVoxel& V) {
  const int t = threadIdx.x, C = A.C;
  if (t < C) {
    double wr = L.u[2 * t], wi = L.u[2 * t + 1];
    if (A.linv) {
      wr = wi = 0.0;
      for (int k = 0; k < C; ++k) {  // conj(Linv[k][t]) u_k
        const double lr = A.linv[2 * (k * C + t)], li = A.linv[2 * (k * C + t) + 1];
        wr += lr * L.u[2 * k] + li * L.u[2 * k + 1];
        wi += lr * L.u[2 * k + 1] - li * L.u[2 * k];
      }
    }
    L.w[2 * t] = wr;
    L.w[2 * t + 1] = wi;
  }
  __syncthreads();
  double sr = 0.0, si = 0.0;  // s0 = w^H R[:, 0], every thread alike
  for (int c = 0; c < C; ++c) {
    double re, im;
    cc_load(A.ref, A.is_c128, V.roff + c * V.rcs, re, im);
    sr += L.w[2 * c] * re + L.w[2 * c + 1] * im;
    si += L.w[2 * c] * im - L.w[2 * c + 1] * re;
  }
  const double a = hypot(sr, si);
  __syncthreads();
  if (t < C && a > 0.0 && isfinite(a)) {
    const double pr = sr / a, pi = si / a, wr = L.w[2 * t], wi = L.w[2 * t + 1];
    L.w[2 * t] = wr * pr - wi * pi;
    L.w[2 * t + 1] = wr * pi + wi * pr;
  }
  __syncthreads();
}

// first_point: u = m / ||m||, m = Linv mean(R[:, :n_points]); w; then trace(G) and u^H G u as two reductions over the
// reference, sum_t ||Linv R_t||^2 and sum_t |w^H R_t|^2.  Returns flags as cc_stage, bit 2: m is zero.
XM_DEV int cc_first_point(const CoilArgs& A, const CcLds& L, const CcVoxel& V, double& ugu, double& tr) {
  const int t = threadIdx.x, C = A.C;
  int flags = 0;
  if (t < C) {
    double sr = 0.0, si = 0.0;
    for (int i = 0; i < A.n_points; ++i) {
      double re, im;
      cc_load(A.ref, A.is_c128, V.roff + t * V.rcs + i, re, im);
      sr += re;
      si += im;
    }
    L.w[2 * t] = sr / (double)A.n_points;
    L.w[2 * t + 1] = si / (double)A.n_points;
  }
  if (A.linv)
    for (int e = t; e < 2 * C * C; e += XM_CC_NT) L.G[e] = A.linv[e];
  __syncthreads();
  if (t < C) {
    double mr = L.w[2 * t], mi = L.w[2 * t + 1];
    if (A.linv) {
      mr = mi = 0.0;
      for (int c = 0; c < C; ++c) {
        const double lr = L.G[2 * (t * C + c)], li = L.G[2 * (t * C + c) + 1];
        mr += lr * L.w[2 * c] - li * L.w[2 * c + 1];
        mi += lr * L.w[2 * c + 1] + li * L.w[2 * c];
      }
    }
    L.u[2 * t] = mr;
    L.u[2 * t + 1] = mi;
  }
  __syncthreads();
  double n2 = 0.0;
  for (int c = 0; c < 2 * C; ++c) n2 += L.u[c] * L.u[c];
  const double nrm = sqrt(n2);
  __syncthreads();
  if (!(nrm > 0.0)) flags |= 4;  // (NaN: the non-finite flag below decides)
  if (t < 2 * C) L.u[t] = L.u[t] / nrm;
  __syncthreads();
  cc_weights(A, L, V);
  double su = 0.0, st = 0.0;
  if (!A.linv) {
    for (int i = t; i < A.NR; i += XM_CC_NT) {
      double yr = 0.0, yi = 0.0, n = 0.0;
      for (int c = 0; c < C; ++c) {
        double re, im;
        cc_load(A.ref, A.is_c128, V.roff + c * V.rcs + i, re, im);
        if (!isfinite(re) || !isfinite(im)) flags |= 1;
        if (re != 0.0 || im != 0.0) flags |= 2;
        yr += L.w[2 * c] * re + L.w[2 * c + 1] * im;
        yi += L.w[2 * c] * im - L.w[2 * c + 1] * re;
        n += re * re + im * im;
      }
      su += yr * yr + yi * yi;
      st += n;
    }
  } else {
    // whitened: every sample is loaded once into a staged tile; thread (point tt, group g) forms rows g, g + 4, ... of
    // Linv R_t from it, group 0 also w^H R_t (points past N_R are staged as zeros and add nothing)
    const int tt = t & (XM_CC_Q - 1), g = t / XM_CC_Q;
    for (int t0 = 0; t0 < A.NR; t0 += XM_CC_Q) {
      cc_stage(A, L, V, t0, flags);
      __syncthreads();
      for (int k = g; k < C; k += XM_CC_NT / XM_CC_Q) {
        double zr = 0.0, zi = 0.0;
        for (int c = 0; c < C; ++c) {
          const double re = L.B[(size_t)(2 * c) * XM_CC_LDQ + tt], im = L.B[(size_t)(2 * c + 1) * XM_CC_LDQ + tt];
          const double lr = L.G[2 * (k * C + c)], li = L.G[2 * (k * C + c) + 1];
          zr += lr * re - li * im;
          zi += lr * im + li * re;
        }
        st += zr * zr + zi * zi;
      }
      if (g == 0) {
        double yr = 0.0, yi = 0.0;
        for (int c = 0; c < C; ++c) {
          const double re = L.B[(size_t)(2 * c) * XM_CC_LDQ + tt], im = L.B[(size_t)(2 * c + 1) * XM_CC_LDQ + tt];
          yr += L.w[2 * c] * re + L.w[2 * c + 1] * im;
          yi += L.w[2 * c] * im - L.w[2 * c + 1] * re;
        }
        su += yr * yr + yi * yi;
      }
      __syncthreads();
    }
  }
  ugu = wg_sum(L.red, su);
  tr = wg_sum(L.red, st);
  return __syncthreads_or(flags & 1) | (__syncthreads_or(flags & 2) ? 2 : 0) | (flags & 4);
}

// FORM: how u is found -- the Gram matrix on the matrix cores, on plain FMAs, or first_point (no Gram matrix)
enum { XM_CC_FORM_MFMA = 0, XM_CC_FORM_FMA = 1, XM_CC_FORM_FIRST = 2 };

template <int FORM>
__global__ __launch_bounds__(XM_CC_NT, 2) void k_coil_combine(CoilArgs A) {
  extern __shared__ double cc_sm[];
  const int t = threadIdx.x, C = A.C;
  CcLds L;
  L.G = cc_sm;
  L.B = L.G + 2 * (size_t)C * C;
  L.scr = L.B + cc_b_doubles(C);
  L.red = L.scr + 1024;
  L.w = L.red + XM_CC_NT;
  L.u = L.w + 2 * XM_CC_MAXC;
  L.rot = L.u + 2 * XM_CC_MAXC;
  __shared__ unsigned next;

  for (;;) {
    const long long v = wg_next_item(A.counter, &next);
    if (v >= A.nv) break;
    const long long a = v / A.n_inner, b = v - a * A.n_inner;
    CcVoxel V;
    V.xoff = (a * C * A.n_inner + b) * A.N;
    V.xcs = A.n_inner * A.N;
    V.roff = (a * C * A.n_inner + b) * A.NR;
    V.rcs = A.n_inner * A.NR;

    int flags = 0, status = 0;
    double lam = 0.0, tr = 0.0;
    if (FORM == XM_CC_FORM_FIRST) {
      flags = cc_first_point(A, L, V, lam, tr);
    } else {
      if (FORM == XM_CC_FORM_MFMA)
        cc_gram_mfma(A, L, V, flags);
      else
        cc_gram_fma(A, L, V, flags);
      flags = __syncthreads_or(flags & 1) | (__syncthreads_or(flags & 2) ? 2 : 0);
    }
    if ((flags & 1) || !(flags & 2) || (flags & 4)) {  // not combined: a non-finite sample, or nothing to go by
      const int st = (flags & 1) || (A.ref != A.x && cc_x_bad(A, V)) ? 2 : 1;
      cc_degenerate(A, v, st);
      __syncthreads();
      continue;
    }
    if (FORM != XM_CC_FORM_FIRST) {
      if (A.linv) cc_whiten(A, L);
      for (int c = 0; c < C; ++c) tr += L.G[2 * (c * C + c)];
      const int sweeps = wg_jacobi(L.G, L.B, L.red, L.rot, C);
      if (sweeps > XM_WG_SWEEPS) status = 3;
      int best = 0;  // the largest diagonal entry, the lowest index on a tie
      for (int c = 1; c < C; ++c)
        if (L.G[2 * (c * C + c)] > L.G[2 * (best * C + best)]) best = c;
      lam = sweeps < 0 ? NAN : L.G[2 * (best * C + best)];
      __syncthreads();
      if (t < C) {
        L.u[2 * t] = L.B[2 * (t * C + best)];
        L.u[2 * t + 1] = L.B[2 * (t * C + best) + 1];
      }
      __syncthreads();
    }
    if (!isfinite(lam) || !isfinite(tr)) {  // finite samples so large that R R^H overflows: as a non-finite sample
      cc_degenerate(A, v, 2);
      __syncthreads();
      continue;
    }
    if (FORM != XM_CC_FORM_FIRST) cc_weights(A, L, V);

    // pass 2: y = w^H X, coalesced along time
    int bad = 0;
    for (int i = t; i < A.N; i += XM_CC_NT) {
      double yr = 0.0, yi = 0.0;
#pragma unroll 4
      for (int c = 0; c < C; ++c) {
        double re, im;
        cc_load(A.x, A.is_c128, V.xoff + c * V.xcs + i, re, im);
        if (!isfinite(re) || !isfinite(im)) bad = 1;
        yr += L.w[2 * c] * re + L.w[2 * c + 1] * im;
        yi += L.w[2 * c] * im - L.w[2 * c + 1] * re;
      }
      if (A.is_c128) {
        ((double*)A.y)[2 * (v * A.N + i)] = yr;
        ((double*)A.y)[2 * (v * A.N + i) + 1] = yi;
      } else {
        ((float*)A.y)[2 * (v * A.N + i)] = (float)yr;
        ((float*)A.y)[2 * (v * A.N + i) + 1] = (float)yi;
      }
    }
    if (A.ref != A.x && __syncthreads_or(bad)) {  // (without a reference X is R, which pass 1 has looked at)
      cc_degenerate(A, v, 2);
    } else {
      if (t < 2 * C) A.w[2 * v * C + t] = L.w[t];
      if (t == 0) {
        A.quality[v] = lam / tr;
        A.status[v] = status;
      }
    }
    __syncthreads();
  }
  wg_leave(A.counter);
}
