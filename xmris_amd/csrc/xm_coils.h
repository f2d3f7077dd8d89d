// Coil combination kernel (the project's own definition, the reference has no such function).
// Included by xm_coils.hip, and by xm_denoise.h for the staging, Gram, mirror, sum and Jacobi functions.
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
#include "xm_common.h"

#define XM_CC_MAXC 64
#define XM_CC_NT 256
#define XM_CC_Q 64       // time points per staged tile
#define XM_CC_LDQ 68     // row stride of the staged tile in doubles: lanes (i, k) of an MFMA operand hit banks 4 i + k
#define XM_CC_MAXE 9     // upper-triangle entries of G per thread, FMA form: ceil(64 * 65 / 2 / 256)
#define XM_CC_MAXB 9     // 16 x 16 blocks per wave, MFMA form: ceil(36 / 4)
#define XM_CC_SWEEPS 30  // Jacobi sweep cap (status 3)
#define XM_CC_SMALL 1824 // doubles after the two matrices: scr[1024], red[256], w[128], u[128], rot[256], pairs[32]

typedef double cc_d4 __attribute__((ext_vector_type(4)));

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

__host__ __device__ inline int cc_pad8(int C) { return (C + 7) & ~7; }
// doubles of the second LDS matrix: the staged tile, then L^{-1} G, then the eigenvectors
__host__ __device__ inline size_t cc_b_doubles(int C) {
  const size_t stage = 2 * (size_t)cc_pad8(C) * XM_CC_LDQ, mat = 2 * (size_t)C * C;
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

// sum of v over the workgroup, the same value in every thread (fixed tree)
XM_DEV double cc_sum(const CcLds& L, double v) {
  const int t = threadIdx.x;
  L.red[t] = v;
  __syncthreads();
  for (int h = XM_CC_NT / 2; h > 0; h >>= 1) {
    if (t < h) L.red[t] += L.red[t + h];
    __syncthreads();
  }
  const double r = L.red[0];
  __syncthreads();
  return r;
}

// tile [t0, t0 + Q) of R into Y (the B matrix); flags: bit 0 a non-finite sample, bit 1 a nonzero one.  GATHER
// (k_denoise, xm_denoise.h): row c starts at rows[c], a table in the LDS, instead of V.roff + c V.rcs
template <bool GATHER = false>
XM_DEV void cc_stage(const CoilArgs& A, const CcLds& L, const CcVoxel& V, int t0, int& flags,
                     const long long* rows = nullptr) {
  const int t = threadIdx.x, tt = t & (XM_CC_Q - 1), Cp = cc_pad8(A.C);
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

// lower triangle <- conjugate of the upper one, diagonal real
XM_DEV void cc_mirror(const CcLds& L, int C) {
  for (int e = threadIdx.x; e < C * C; e += XM_CC_NT) {
    const int i = e / C, j = e - i * C;
    if (i > j) {
      L.G[2 * e] = L.G[2 * (j * C + i)];
      L.G[2 * e + 1] = -L.G[2 * (j * C + i) + 1];
    } else if (i == j) {
      L.G[2 * e + 1] = 0.0;
    }
  }
  __syncthreads();
}

// G <- R R^H by plain FMAs: thread t owns entries t + 256 m of the upper triangle in row-major order
template <bool GATHER = false>
XM_DEV void cc_gram_fma(const CoilArgs& A, const CcLds& L, const CcVoxel& V, int& flags,
                        const long long* rows = nullptr) {
  const int t = threadIdx.x, C = A.C, ne = C * (C + 1) / 2;
  int ci[XM_CC_MAXE], cj[XM_CC_MAXE];
  double re[XM_CC_MAXE], im[XM_CC_MAXE];
  {
    int i = 0, j = 0, e = 0;
#pragma unroll
    for (int m = 0; m < XM_CC_MAXE; ++m) {
      const int target = t + XM_CC_NT * m;
      while (e < target && e < ne) {
        ++e;
        if (++j >= C) {
          ++i;
          j = i;
        }
      }
      ci[m] = i < C ? i : 0;
      cj[m] = i < C ? j : 0;
      re[m] = im[m] = 0.0;
    }
  }
  for (int t0 = 0; t0 < A.NR; t0 += XM_CC_Q) {
    cc_stage<GATHER>(A, L, V, t0, flags, rows);
    __syncthreads();
#pragma unroll
    for (int m = 0; m < XM_CC_MAXE; ++m) {
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
#pragma unroll
  for (int m = 0; m < XM_CC_MAXE; ++m) {
    if (t + XM_CC_NT * m < ne) {
      L.G[2 * (ci[m] * C + cj[m])] = re[m];
      L.G[2 * (ci[m] * C + cj[m]) + 1] = im[m];
    }
  }
  __syncthreads();
  cc_mirror(L, C);
}

// G <- R R^H on the fp64 matrix cores.  Work items j = slice * nblk + blk (blk: a 16 x 16 block (I, J), I <= J, of
// Y Y^T; slice: a quarter of each tile's points when nblk < 4, else the whole tile); wave v takes items v, v + 4, ...
// Operands of v_mfma_f64_16x16x4_f64: lane l holds A[l & 15][l >> 4] and B[l >> 4][l & 15], i.e. Y[16 I + (l & 15)][k]
// and Y[16 J + (l & 15)][k] with k = 4 kk + (l >> 4); result r of lane l is row (l >> 4) + 4 r, column l & 15.
template <bool GATHER = false>
XM_DEV void cc_gram_mfma(const CoilArgs& A, const CcLds& L, const CcVoxel& V, int& flags,
                         const long long* rows = nullptr) {
  const int t = threadIdx.x, C = A.C, wave = t >> 6, lane = t & 63;
  const int nb = cc_pad8(C) / 8, nblk = nb * (nb + 1) / 2, S = nblk < 4 ? 4 : 1, nitems = nblk * S;
  const int ksteps = XM_CC_Q / 4 / S;
  int bi[XM_CC_MAXB], bj[XM_CC_MAXB], sl[XM_CC_MAXB];
  cc_d4 acc[XM_CC_MAXB];
#pragma unroll
  for (int m = 0; m < XM_CC_MAXB; ++m) {
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
    acc[m] = cc_d4{0.0, 0.0, 0.0, 0.0};
  }
  for (int t0 = 0; t0 < A.NR; t0 += XM_CC_Q) {
    cc_stage<GATHER>(A, L, V, t0, flags, rows);
    __syncthreads();
#pragma unroll
    for (int m = 0; m < XM_CC_MAXB; ++m) {
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
  // every block through its wave's scratch square into G (or into its slice's partial matrix, in B: the tile is done)
  double* scr = L.scr + 256 * wave;
#pragma unroll
  for (int m = 0; m < XM_CC_MAXB; ++m) {
    const bool on = wave + 4 * m < nitems;
    if (on)
      for (int r = 0; r < 4; ++r) scr[((lane >> 4) + 4 * r) * 16 + (lane & 15)] = acc[m][r];
    __syncthreads();
    if (on) {
      const int ii = lane >> 3, jj = lane & 7, i = 8 * bi[m] + ii, j = 8 * bj[m] + jj;
      if (i < C && j < C && i <= j) {
        double* dst = S == 1 ? L.G : L.B + (size_t)sl[m] * 2 * C * C;
        dst[2 * (i * C + j)] = scr[(2 * ii) * 16 + 2 * jj] + scr[(2 * ii + 1) * 16 + 2 * jj + 1];
        dst[2 * (i * C + j) + 1] = scr[(2 * ii + 1) * 16 + 2 * jj] - scr[(2 * ii) * 16 + 2 * jj + 1];
      }
    }
    __syncthreads();
  }
  if (S > 1) {
    const size_t m2 = 2 * (size_t)C * C;
    for (int e = t; e < C * C; e += XM_CC_NT) {
      const int i = e / C, j = e - i * C;
      if (i <= j) {
        L.G[2 * e] = ((L.B[2 * e] + L.B[m2 + 2 * e]) + L.B[2 * m2 + 2 * e]) + L.B[3 * m2 + 2 * e];
        L.G[2 * e + 1] = ((L.B[2 * e + 1] + L.B[m2 + 2 * e + 1]) + L.B[2 * m2 + 2 * e + 1]) + L.B[3 * m2 + 2 * e + 1];
      }
    }
    __syncthreads();
  }
  cc_mirror(L, C);
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
  cc_mirror(L, C);
}

// Parallel cyclic Jacobi on the Hermitian G (LDS), eigenvectors accumulated in B.  Round-robin pairing of
// 2 ceil(C / 2) players (an odd C has a bye); the rotations of a step are computed by one thread each and applied by
// the workgroup: columns of G and V, then rows of G.  A pair (p, q) with G_pq = h e^{i phi}:
// J = [[c, s e^{i phi}], [-s e^{-i phi}, c]], tau = (G_qq - G_pp) / (2 h), t = sign(tau) / (|tau| + sqrt(1 + tau^2)).
// Every update is written as x - s (y + r x), y + s (x - r y) with r = s / (1 + c) (Rutishauser), and the pair's
// diagonal as G_pp - t h, G_qq + t h, so that a small rotation leaves a small rounding error.  Returns the sweeps done,
// XM_CC_SWEEPS + 1 when the off-diagonal norm never fell to eps ||G||_F, -1 when ||G||_F^2 is not finite.  Both
// norms are taken on G times the power of two that brings its largest diagonal entry to [1, 2), so the squares of small
// samples do not underflow to a test that is met at once (a G that is itself subnormal or zero is not helped by it).
#define XM_CC_ROT 8  // doubles per rotation: c, s, cos phi, sin phi, r, new G_pp, new G_qq
XM_DEV int cc_jacobi(const CcLds& L, int C) {
  const int t = threadIdx.x, np = (C + 1) / 2, players = 2 * np;
  double* Vm = L.B;
  for (int e = t; e < C * C; e += XM_CC_NT) {
    Vm[2 * e] = (e / C == e % C) ? 1.0 : 0.0;
    Vm[2 * e + 1] = 0.0;
  }
  double gmax = 0.0;  // (every thread alike: G is complete since cc_mirror's barrier)
  for (int i = 0; i < C; ++i) gmax = fmax(gmax, fabs(L.G[2 * (i * C + i)]));
  const int ex = gmax > 0.0 && isfinite(gmax) ? -ilogb(gmax) : 0;  // both norms on 2^ex G: exact, and no square underflows
  double f = 0.0;
  for (int e = t; e < 2 * C * C; e += XM_CC_NT) {
    const double g = ldexp(L.G[e], ex);
    f += g * g;
  }
  const double fro2 = cc_sum(L, f);  // (also the barrier after V's initialisation)
  // samples so large that G or its norm overflows: nothing to iterate on
  if (!isfinite(fro2) || !isfinite(ldexp(fro2, -2 * ex))) return -1;
  const double eps = 2.220446049250313e-16;
  int* pq = (int*)(L.rot + XM_CC_ROT * 32);  // pairs of the step, after the 32 rotations
  for (int sweep = 0;; ++sweep) {
    double o = 0.0;
    for (int e = t; e < C * C; e += XM_CC_NT)
      if (e / C != e % C) {
        const double gr = ldexp(L.G[2 * e], ex), gi = ldexp(L.G[2 * e + 1], ex);
        o += gr * gr + gi * gi;
      }
    const double off2 = cc_sum(L, o);
    if (!(off2 > eps * eps * fro2)) return sweep;
    if (sweep == XM_CC_SWEEPS) return XM_CC_SWEEPS + 1;
    for (int step = 0; step < players - 1; ++step) {
      if (t < np) {
        int a = t == 0 ? players - 1 : (step + t) % (players - 1);
        int b = t == 0 ? step : (step - t + players - 1) % (players - 1);
        const int p = a < b ? a : b, q = a < b ? b : a;
        double* r = L.rot + XM_CC_ROT * t;
        r[0] = 1.0;
        r[1] = 0.0;
        if (q < C) {
          const double gr = L.G[2 * (p * C + q)], gi = L.G[2 * (p * C + q) + 1];
          const double h = hypot(gr, gi);
          if (h > 0.0) {
            const double gpp = L.G[2 * (p * C + p)], gqq = L.G[2 * (q * C + q)];
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
      for (int it = t; it < 2 * C * np; it += XM_CC_NT) {
        const int e = it % (C * np), k = e % np, row = e / np;
        const double* r = L.rot + XM_CC_ROT * k;
        const double s = r[1];
        if (s == 0.0) continue;  // nothing to rotate (or the bye)
        const double er = r[2], ei = r[3], rr = r[4];
        double* M = it < C * np ? L.G : Vm;
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
      for (int it = t; it < C * np; it += XM_CC_NT) {
        const int k = it % np, j = it / np;
        const double* r = L.rot + XM_CC_ROT * k;
        const double s = r[1];
        if (s == 0.0) continue;
        const double er = r[2], ei = r[3], rr = r[4];
        const int p = pq[2 * k], q = pq[2 * k + 1];
        double* xp = L.G + 2 * (p * C + j);
        double* xq = L.G + 2 * (q * C + j);
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
  ugu = cc_sum(L, su);
  tr = cc_sum(L, st);
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
    if (t == 0) next = atomicAdd(A.counter, 1u);
    __syncthreads();
    const long long v = (long long)next;
    __syncthreads();
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
      const int sweeps = cc_jacobi(L, C);
      if (sweeps > XM_CC_SWEEPS) status = 3;
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
  // the last workgroup out leaves the counters at zero
  if (t == 0) {
    const unsigned d = atomicAdd(A.counter + 1, 1u);
    if (d == gridDim.x - 1u) {
      __hip_atomic_store(A.counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(A.counter + 1, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}
