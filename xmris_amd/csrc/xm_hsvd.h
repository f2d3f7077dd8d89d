// Residual-signal removal by HSVD (the project's own definition, the reference has no such
// function).  Included by xm_hsvd.hip only, which is compiled with -ffp-contract=off.
//
// One FID x[t], t < N: the Hankel matrix H[l][j] = x[l + j] (R = N - M + 1 rows, M columns), G = H^H H.  W = conj(U), U
// the eigenvectors of G's K largest eigenvalues, are the eigenvectors of conj(G) = sum_l h_l h_l^H (h_l = x[l .. l + M)),
// which is what the kernel forms and diagonalises -- the Gram matrix of k_coil_combine with "coil i" = the FID delayed by
// i points.  Q = (I + w w^H / (1 - ||w||^2)) Wup^H Wdown with w^H the last row of W; z_k = eig(Q); a = the least-squares
// amplitudes of sum_k a_k z_k^t over all N points; y = x - sum over the poles with f_lo <= arg(z_k) / (2 pi dt) <= f_hi.
//
// k_hsvd<FORM>: one 256-thread workgroup per FID, FIDs handed out by a device counter (persistent grid, the idiom of
// k_coil_combine and k_align).  Rows are `stride` elements apart.  All arithmetic fp64; complex64 is widened on load.
//
// Gram.  Tiles of XM_HS_Q Hankel rows: the Q + 63 samples a tile touches are staged once (real parts, then imaginary
// parts 336 doubles on, which puts the two on opposite halves of the banks), and the real matrix Y of k_coil_combine,
// rows 2 i = Re x[l + i] and 2 i + 1 = Im x[l + i], is never stored: lane (row r, step k) of an MFMA operand reads
// part r & 1 of sample (r >> 1) + k.  Hankel rows past R are masked in the operand, not in the samples (a sample is
// shared by up to M rows).  The upper block triangle of Y Y^T accumulates on v_mfma_f64_16x16x4_f64, work items, stores
// and the slicing in four when there are fewer than 4 blocks being wg_gram_items / wg_gram_store / wg_gram_finish of
// xm_wg.h, or by plain FMAs, one upper-triangle entry per thread slot (wg_gram_entries; FORM = FMA).  Time order never
// depends on the batch or the workgroup.
// Eigenvectors.  wg_jacobi's parallel cyclic Jacobi (xm_wg.h), then a stable selection of the K largest diagonal entries.
// Poles.  Householder reduction of Q to Hessenberg form, then single-shift QR with Wilkinson's shift and deflation,
// eigenvalues only (the active window alone is updated).  One QR step: lane j of wave 0 owns column j and applies the
// Givens rotations of the step to it in order, rotation k being formed by lane k and passed on by v_readlane; then
// thread i owns row i and applies the same rotations from the right.  Every matrix element is in the LDS.
// Amplitudes.  Tiles of 128 time points: the K powers z_k^t = exp(t ln|z_k|) (cos, sin)(t arg z_k) and x are staged,
// every thread owns up to three entries of [B^H B | B^H x] and adds the tile's points in ascending order; complex
// Cholesky in the LDS.  Subtract.  One thread per time point, the powers formed again the same way.
#pragma once
#include "xm_wg.h"

#define XM_HS_NT 256
#define XM_HS_MAXM 64
#define XM_HS_MAXK 32
#define XM_HS_MAXN 16384
#define XM_HS_Q 256       // Hankel rows per staged tile
#define XM_HS_SEG 336     // doubles per part of the staged samples (Q + 64 used)
#define XM_HS_T 128       // time points per tile of the amplitude stage
#define XM_HS_LDT 129     // row stride of that tile in doubles
#define XM_HS_MAXP 3      // entries of [B^H B | B^H x] per thread: ceil((32 * 33 / 2 + 32) / 256)
// doubles after the big region: seg[672], scr[1024], red[256], rot[256 + 32], lam[64], z[64], lz[64], a[64], f[32], d[32],
// ints[64 as 32 doubles]
#define XM_HS_SMALL 2648
static_assert(XM_HS_NT == XM_WG_NT, "k_hsvd runs xm_wg.h's workgroup");
static_assert(XM_HS_MAXM * (XM_HS_MAXM + 1) / 2 <= XM_WG_MAXE * XM_WG_NT, "the FMA form's slots must hold XM_HS_MAXM columns");
static_assert((XM_HS_MAXM / 8) * (XM_HS_MAXM / 8 + 1) / 2 <= 4 * XM_WG_MAXB, "the MFMA form's slots must hold XM_HS_MAXM columns");

// `stop` (timing only): end every FID after the named stage
enum { XM_HS_STOP_NONE = 0, XM_HS_STOP_GRAM = 1, XM_HS_STOP_EIG = 2, XM_HS_STOP_POLES = 3, XM_HS_STOP_AMPL = 4 };

struct HsvdArgs {
  const void* x;       // n_batch rows of N complex64 / complex128, `stride` elements apart
  long long stride;
  void* y;             // (n_batch, N), the input's dtype, or nullptr
  double *freq, *damp, *amp, *phase;  // (n_batch, K)
  int* removed;        // (n_batch, K)
  int *n_removed, *status;  // (n_batch)
  long long nb;
  int N, M, K, is_c128, stop;
  double dt, f_lo, f_hi;
  unsigned* counter;   // [2] zero at launch: row ticket, workgroups done
};

// the eigenvector matrix, which first holds the four partial Gram matrices of the sliced form (M <= 16)
__host__ __device__ inline size_t hs_v_doubles(int M) {
  const size_t mm = 2 * (size_t)M * M;
  return mm > 2048 ? mm : 2048;
}
// the big region: G and the eigenvectors, later W, Q and the amplitude stage's tile, normal matrix and right-hand side
__host__ __device__ inline size_t hs_big_doubles(int M, int K) {
  const size_t eig = 2 * (size_t)M * M + hs_v_doubles(M);
  const size_t amp = 2 * (size_t)(K + 1) * XM_HS_LDT + 2 * (size_t)K * K + 2 * (size_t)K;
  return eig > amp ? eig : amp;
}
__host__ __device__ inline size_t hs_lds_bytes(int M, int K) { return (hs_big_doubles(M, K) + XM_HS_SMALL) * sizeof(double); }

struct HsLds {
  double *G, *V;  // M x M complex each (interleaved re, im), row-major
  double *seg, *scr, *red, *rot, *lam, *z, *lz, *a, *f, *d;
  int* idx;       // [64]
};

struct hz {
  double r, i;
};
XM_DEV hz hz_ld(const double* p, int e) { return hz{p[2 * e], p[2 * e + 1]}; }
XM_DEV void hz_st(double* p, int e, hz v) {
  p[2 * e] = v.r;
  p[2 * e + 1] = v.i;
}
XM_DEV hz hz_add(hz a, hz b) { return hz{a.r + b.r, a.i + b.i}; }
XM_DEV hz hz_sub(hz a, hz b) { return hz{a.r - b.r, a.i - b.i}; }
XM_DEV hz hz_mul(hz a, hz b) { return hz{a.r * b.r - a.i * b.i, a.r * b.i + a.i * b.r}; }
XM_DEV hz hz_mulc(hz a, hz b) { return hz{a.r * b.r + a.i * b.i, a.i * b.r - a.r * b.i}; }  // a conj(b)
XM_DEV hz hz_cmul(hz a, hz b) { return hz{a.r * b.r + a.i * b.i, a.r * b.i - a.i * b.r}; }  // conj(a) b
XM_DEV hz hz_scale(hz a, double s) { return hz{a.r * s, a.i * s}; }
XM_DEV double hz_abs2(hz a) { return a.r * a.r + a.i * a.i; }
XM_DEV double hz_abs1(hz a) { return fabs(a.r) + fabs(a.i); }
XM_DEV hz hz_div(hz a, hz b) {
  const double s = 1.0 / (fabs(b.r) + fabs(b.i));  // scaled: no overflow in |b|^2
  const double br = b.r * s, bi = b.i * s, d = br * br + bi * bi;
  return hz{((a.r * s) * br + (a.i * s) * bi) / d, ((a.i * s) * br - (a.r * s) * bi) / d};
}
XM_DEV hz hz_sqrt(hz a) {  // principal square root
  const double m = hypot(a.r, a.i);
  if (m == 0.0) return hz{0.0, 0.0};
  const double u = sqrt(0.5 * (m + fabs(a.r)));
  const double v = a.i / (2.0 * u);
  return a.r >= 0.0 ? hz{u, v} : hz{fabs(v), a.i >= 0.0 ? u : -u};
}

XM_DEV void hs_load(const void* p, int c128, long long i, double& re, double& im) {
  if (c128) {
    const double2 q = ((const double2*)p)[i];
    re = q.x;
    im = q.y;
  } else {
    const float2 q = ((const float2*)p)[i];
    re = (double)q.x;
    im = (double)q.y;
  }
}

XM_DEV void hs_store(void* p, int c128, long long i, double re, double im) {
  if (c128)
    ((double2*)p)[i] = make_double2(re, im);
  else
    ((float2*)p)[i] = make_float2((float)re, (float)im);
}

// the value of lane `lane` (wave-uniform) in every lane of the wave
XM_DEV double hs_bcast(double v, int lane) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  return __hiloint2double(hi, lo);
}

// samples [t0, t0 + Q + 64) into seg (zeros past N); flags: bit 0 a non-finite sample, bit 1 a nonzero one
XM_DEV void hs_stage(const HsvdArgs& A, const HsLds& L, long long xoff, int t0, int& flags) {
  for (int s = threadIdx.x; s < XM_HS_Q + 64; s += XM_HS_NT) {
    double re = 0.0, im = 0.0;
    if (t0 + s < A.N) {
      hs_load(A.x, A.is_c128, xoff + t0 + s, re, im);
      if (!isfinite(re) || !isfinite(im)) flags |= 1;
      if (re != 0.0 || im != 0.0) flags |= 2;
    }
    L.seg[s] = re;
    L.seg[XM_HS_SEG + s] = im;
  }
}

// G[i][j] <- sum_l x[l + i] conj(x[l + j]) by plain FMAs: thread t owns entries t + 256 m of the upper triangle
XM_DEV void hs_gram_fma(const HsvdArgs& A, const HsLds& L, long long xoff, int& flags) {
  const int t = threadIdx.x, M = A.M, ne = M * (M + 1) / 2, R = A.N - M + 1;
  int ci[XM_WG_MAXE], cj[XM_WG_MAXE];
  double re[XM_WG_MAXE] = {}, im[XM_WG_MAXE] = {};
  wg_gram_entries(M, ne, ci, cj);
  for (int t0 = 0; t0 < R; t0 += XM_HS_Q) {
    hs_stage(A, L, xoff, t0, flags);
    __syncthreads();
    const int lim = R - t0 < XM_HS_Q ? R - t0 : XM_HS_Q;
#pragma unroll
    for (int m = 0; m < XM_WG_MAXE; ++m) {
      if (t + XM_HS_NT * m < ne) {
        const double* ai = L.seg + ci[m];
        const double* aj = L.seg + cj[m];
#pragma unroll 4
        for (int k = 0; k < lim; ++k) {
          re[m] += ai[k] * aj[k] + ai[XM_HS_SEG + k] * aj[XM_HS_SEG + k];
          im[m] += ai[XM_HS_SEG + k] * aj[k] - ai[k] * aj[XM_HS_SEG + k];
        }
      }
    }
    __syncthreads();
  }
  wg_gram_entries_finish(L.G, M, ne, ci, cj, re, im);
}

// The same on the fp64 matrix cores, work items (block (I, J), slice) as wg_gram_items hands them out: lane l holds
// Y[16 I + (l & 15)][k] and Y[16 J + (l & 15)][k], k = 4 kk + (l >> 4).  Y[r][k] = part r & 1 of sample
// t0 + (r >> 1) + k, zero for Hankel rows t0 + k >= R.
XM_DEV void hs_gram_mfma(const HsvdArgs& A, const HsLds& L, long long xoff, int& flags) {
  const int t = threadIdx.x, M = A.M, wave = t >> 6, lane = t & 63, R = A.N - M + 1;
  const int nb = wg_pad8(M) / 8, nblk = nb * (nb + 1) / 2, S = nblk < 4 ? 4 : 1, nitems = nblk * S;
  const int ksteps = XM_HS_Q / 4 / S;
  int bi[XM_WG_MAXB], bj[XM_WG_MAXB], sl[XM_WG_MAXB];
  wg_d4 acc[XM_WG_MAXB];
  wg_gram_items(nb, nblk, bi, bj, sl);
#pragma unroll
  for (int m = 0; m < XM_WG_MAXB; ++m) acc[m] = wg_d4{0.0, 0.0, 0.0, 0.0};
  for (int t0 = 0; t0 < R; t0 += XM_HS_Q) {
    hs_stage(A, L, xoff, t0, flags);
    __syncthreads();
    const int lim = R - t0;  // Hankel rows of this tile: k < lim
#pragma unroll
    for (int m = 0; m < XM_WG_MAXB; ++m) {
      if (wave + 4 * m < nitems) {  // wave-uniform: the MFMA runs with every lane on
        const int kb = 4 * ksteps * sl[m], k0 = kb + (lane >> 4);
        const int ra = 16 * bi[m] + (lane & 15), rb = 16 * bj[m] + (lane & 15);
        const double* ya = L.seg + (ra & 1) * XM_HS_SEG + (ra >> 1) + k0;
        const double* yb = L.seg + (rb & 1) * XM_HS_SEG + (rb >> 1) + k0;
        if (kb + 4 * ksteps <= lim) {
          for (int kk = 0; kk < ksteps; ++kk)
            acc[m] = __builtin_amdgcn_mfma_f64_16x16x4f64(ya[4 * kk], yb[4 * kk], acc[m], 0, 0, 0);
        } else {
          for (int kk = 0; kk < ksteps && kb + 4 * kk < lim; ++kk) {
            const bool in = k0 + 4 * kk < lim;
            const double va = in ? ya[4 * kk] : 0.0, vb = in ? yb[4 * kk] : 0.0;
            acc[m] = __builtin_amdgcn_mfma_f64_16x16x4f64(va, vb, acc[m], 0, 0, 0);
          }
        }
      }
    }
    __syncthreads();
  }
  // the slices' partial matrices go to V
  wg_gram_store(acc, bi, bj, sl, nitems, S, L.scr, L.G, L.V, M);
  wg_gram_finish(L.G, L.V, M, S);
}

// W (M x K, into G's place) <- the eigenvectors of the K largest diagonal entries of G, the largest first, a tie going
// to the lower index
XM_DEV void hs_select(const HsLds& L, int M, int K) {
  const int t = threadIdx.x;
  if (t < M) L.lam[t] = L.G[2 * (t * M + t)];
  if (t < XM_HS_MAXK) L.idx[t] = 0;
  __syncthreads();
  if (t < M) {
    const double mine = L.lam[t];
    int rank = 0;
    for (int c = 0; c < M; ++c) {
      const double o = L.lam[c];
      if (o > mine || (o == mine && c < t)) ++rank;
    }
    if (rank < K) L.idx[rank] = t;
  }
  __syncthreads();
  for (int e = t; e < M * K; e += XM_HS_NT) {
    const int j = e / K, r = e - j * K;
    hz_st(L.G, e, hz_ld(L.V, j * M + L.idx[r]));
  }
  __syncthreads();
}

// Q (K x K, into V's place) from W (in G's place); false (every thread alike) when 1 - ||w||^2 <= 0
XM_DEV bool hs_shift_matrix(const HsLds& L, int M, int K) {
  const int t = threadIdx.x;
  const double* W = L.G;
  double* Q = L.V;
  for (int e = t; e < K * K; e += XM_HS_NT) {
    const int a = e / K, b = e - a * K;
    hz s{0.0, 0.0};
    for (int j = 0; j + 1 < M; ++j) s = hz_add(s, hz_cmul(hz_ld(W, j * K + a), hz_ld(W, (j + 1) * K + b)));
    hz_st(Q, e, s);
  }
  __syncthreads();
  const double* last = W + 2 * (size_t)(M - 1) * K;  // w^H
  if (t < K) {  // u_b = sum_a W[M-1][a] P[a][b]
    hz s{0.0, 0.0};
    for (int a = 0; a < K; ++a) s = hz_add(s, hz_mul(hz_ld(last, a), hz_ld(Q, a * K + t)));
    hz_st(L.a, t, s);
  }
  double n2 = 0.0;
  for (int a = 0; a < K; ++a) n2 += hz_abs2(hz_ld(last, a));
  const double den = 1.0 - n2;
  __syncthreads();
  if (!(den > 0.0)) return false;
  for (int e = t; e < K * K; e += XM_HS_NT) {
    const int a = e / K, b = e - a * K;
    const hz wa = hz_ld(last, a);  // w_a = conj of it
    const hz c = hz_scale(hz_cmul(wa, hz_ld(L.a, b)), 1.0 / den);
    hz_st(Q, e, hz_add(hz_ld(Q, e), c));
  }
  __syncthreads();
  return true;
}

// Q (K x K in V's place) to upper Hessenberg form by Householder reflections; what lies below the subdiagonal is left
// as it falls (the QR iteration never reads it)
XM_DEV void hs_hessenberg(const HsLds& L, int K) {
  const int t = threadIdx.x;
  double* H = L.V;
  double* hv = L.rot;  // the reflector, entries k + 1 ... K - 1
  for (int k = 0; k + 2 < K; ++k) {
    double sigma = 0.0;
    for (int i = k + 2; i < K; ++i) sigma += hz_abs2(hz_ld(H, i * K + k));
    if (sigma == 0.0) continue;  // (every thread alike: the same LDS words after a barrier)
    const hz x0 = hz_ld(H, (k + 1) * K + k);
    const double a0 = hypot(x0.r, x0.i), nrm = sqrt(a0 * a0 + sigma);
    const hz alpha = a0 > 0.0 ? hz_scale(x0, -nrm / a0) : hz{-nrm, 0.0};
    const hz v0 = hz_sub(x0, alpha);
    const double vn = sqrt(hz_abs2(v0) + sigma);
    if (t < K - k - 1) {
      const int i = k + 1 + t;
      hz_st(hv, i, hz_scale(t == 0 ? v0 : hz_ld(H, i * K + k), 1.0 / vn));
    }
    __syncthreads();
    if (t < K) {  // from the left, thread = column
      hz s{0.0, 0.0};
      for (int i = k + 1; i < K; ++i) s = hz_add(s, hz_cmul(hz_ld(hv, i), hz_ld(H, i * K + t)));
      s = hz_scale(s, 2.0);
      for (int i = k + 1; i < K; ++i) hz_st(H, i * K + t, hz_sub(hz_ld(H, i * K + t), hz_mul(hz_ld(hv, i), s)));
    }
    __syncthreads();
    if (t < K) {  // from the right, thread = row
      hz s{0.0, 0.0};
      for (int j = k + 1; j < K; ++j) s = hz_add(s, hz_mul(hz_ld(H, t * K + j), hz_ld(hv, j)));
      s = hz_scale(s, 2.0);
      for (int j = k + 1; j < K; ++j) hz_st(H, t * K + j, hz_sub(hz_ld(H, t * K + j), hz_mulc(s, hz_ld(hv, j))));
    }
    __syncthreads();
  }
}

// eigenvalues of the Hessenberg matrix in V's place into L.z; false (every thread alike) at the iteration cap 30 K
XM_DEV bool hs_qr(const HsLds& L, int K, double hnorm) {
  const int t = threadIdx.x;
  double* H = L.V;
  double* rot = L.rot;  // rotation k of the step: p (re, im), q (re, im)
  const double eps = 2.220446049250313e-16;
  int hi = K - 1, its = 0, total = 0;
  while (hi >= 0) {
    int l = hi;
    while (l > 0) {
      const double sub = hz_abs1(hz_ld(H, l * K + l - 1));
      double tst = hz_abs1(hz_ld(H, (l - 1) * K + l - 1)) + hz_abs1(hz_ld(H, l * K + l));
      if (tst == 0.0) tst = hnorm;
      if (sub <= eps * tst) break;
      --l;
    }
    if (l == hi) {  // deflated
      if (t == 0) hz_st(L.z, hi, hz_ld(H, hi * K + hi));
      --hi;
      its = 0;
      continue;
    }
    if (total == 30 * K) {
      __syncthreads();
      return false;
    }
    ++total;
    ++its;
    hz s;
    {
      const hz a = hz_ld(H, (hi - 1) * K + hi - 1), b = hz_ld(H, (hi - 1) * K + hi);
      const hz c = hz_ld(H, hi * K + hi - 1), d = hz_ld(H, hi * K + hi);
      if (its == 10 || its == 20) {  // exceptional shift
        s = hz{fabs(c.r) + (hi - 2 >= l ? fabs(H[2 * ((hi - 1) * K + hi - 2)]) : 0.0), 0.0};
      } else {  // Wilkinson: the eigenvalue of the trailing 2 x 2 block nearer to d
        const hz dl = hz_scale(hz_sub(a, d), 0.5), bc = hz_mul(b, c);
        hz disc = hz_sqrt(hz_add(hz_mul(dl, dl), bc));
        if (dl.r * disc.r + dl.i * disc.i < 0.0) disc = hz{-disc.r, -disc.i};
        const hz den = hz_add(dl, disc);
        s = (den.r == 0.0 && den.i == 0.0) ? d : hz_sub(d, hz_div(bc, den));
      }
    }
    __syncthreads();  // everybody has read H
    if (t < XM_WAVE) {  // H - s I = QR: lane = column, the rotations from the left
      const int j = l + t;
      const bool mine = j <= hi;
      if (mine) hz_st(H, j * K + j, hz_sub(hz_ld(H, j * K + j), s));
      for (int k = l; k < hi; ++k) {
        const bool on = mine && j >= k;
        const hz x = on ? hz_ld(H, k * K + j) : hz{0.0, 0.0};
        const hz y = on ? hz_ld(H, (k + 1) * K + j) : hz{0.0, 0.0};
        const double r = hypot(hypot(x.r, x.i), hypot(y.r, y.i));
        hz p{1.0, 0.0}, q{0.0, 0.0};
        if (r != 0.0) {  // G = [[p, q], [-conj(q), conj(p)]], G (x, y)^T = (r, 0)^T
          p = hz{x.r / r, -x.i / r};
          q = hz{y.r / r, -y.i / r};
        }
        const int src = k - l;
        p = hz{hs_bcast(p.r, src), hs_bcast(p.i, src)};
        q = hz{hs_bcast(q.r, src), hs_bcast(q.i, src)};
        if (on) {
          hz_st(H, k * K + j, hz_add(hz_mul(p, x), hz_mul(q, y)));
          hz_st(H, (k + 1) * K + j, hz_sub(hz_cmul(p, y), hz_cmul(q, x)));
        }
        if (t == 0) {
          hz_st(rot, 2 * src, p);
          hz_st(rot, 2 * src + 1, q);
        }
      }
    }
    __syncthreads();
    if (t <= hi - l) {  // R Q + s I: thread = row, the rotations from the right
      const int i = l + t;
      for (int k = (i - 1 > l ? i - 1 : l); k < hi; ++k) {
        const hz p = hz_ld(rot, 2 * (k - l)), q = hz_ld(rot, 2 * (k - l) + 1);
        const hz x = hz_ld(H, i * K + k), y = hz_ld(H, i * K + k + 1);
        hz_st(H, i * K + k, hz_add(hz_mulc(x, p), hz_mulc(y, q)));  // x conj(p) + y conj(q)
        hz_st(H, i * K + k + 1, hz_sub(hz_mul(y, p), hz_mul(x, q)));  // -x q + y p
      }
      hz_st(H, i * K + i, hz_add(hz_ld(H, i * K + i), s));
    }
    __syncthreads();
  }
  __syncthreads();
  return true;
}

// z_k^t = exp(t ln|z_k|) (cos, sin)(t arg z_k), the products rounded once, as the oracle's exp(t log z) forms them
XM_DEV hz hs_power(double lnr, double th, int t) {
  const double e = exp((double)t * lnr);
  double s, c;
  sincos((double)t * th, &s, &c);
  return hz{e * c, e * s};
}

// ln|z|, arg z, f, d of the poles, sorted by f ascending (a tie going to the lower index), into L.lz, L.f, L.d; idx[k] =
// 1 for a pole inside [f_lo, f_hi]; returns 0, or 1 (every thread alike) when a ln|z| or arg z is not finite
XM_DEV int hs_poles(const HsvdArgs& A, const HsLds& L) {
  const int t = threadIdx.x, K = A.K;
  double lnr = 0.0, th = 0.0, f = 0.0;
  if (t < K) {
    const hz z = hz_ld(L.z, t);
    lnr = log(hypot(z.r, z.i));
    th = atan2(z.i, z.r);
    f = th / (2.0 * M_PI * A.dt);
    L.a[t] = f;  // (unsorted, for the ranking)
  }
  const int bad = __syncthreads_or(t < K && (!isfinite(lnr) || !isfinite(th)));
  if (bad) return 1;
  if (t < K) {
    int rank = 0;
    for (int c = 0; c < K; ++c) {
      const double o = L.a[c];
      if (o < f || (o == f && c < t)) ++rank;
    }
    L.lz[2 * rank] = lnr;
    L.lz[2 * rank + 1] = th;
    L.f[rank] = f;
    L.d[rank] = -lnr / A.dt;
    L.idx[rank] = f >= A.f_lo && f <= A.f_hi;
  }
  __syncthreads();
  return 0;
}

// a <- argmin sum_t |x_t - sum_k a_k z_k^t|^2 by the normal equations; 0, or 4 (every thread alike) for a non-finite
// power or a pivot that is not positive and finite.  `big`: the big region, free by now.
XM_DEV int hs_amplitudes(const HsvdArgs& A, const HsLds& L, double* big, long long xoff) {
  const int t = threadIdx.x, K = A.K, ne = K * (K + 1) / 2 + K;
  double* Bre = big;                                   // [K + 1][LDT]: the powers, row K = x
  double* Bim = Bre + (size_t)(K + 1) * XM_HS_LDT;
  double* Nm = Bim + (size_t)(K + 1) * XM_HS_LDT;      // K x K complex: upper triangle B^H B, strictly lower its factor
  double* rhs = Nm + 2 * (size_t)K * K;                // B^H x, then the solution's intermediate
  double* ld = L.red;                                  // the factor's diagonal (red is free between sums)
  // entries t + 256 m of the rows a < K, columns b = a ... K (column K: the right-hand side)
  int ea[XM_HS_MAXP], eb[XM_HS_MAXP];
  double sr[XM_HS_MAXP], si[XM_HS_MAXP];
  {
    int a = 0, b = 0, e = 0;
#pragma unroll
    for (int m = 0; m < XM_HS_MAXP; ++m) {
      const int target = t + XM_HS_NT * m;
      while (e < target && e < ne) {
        ++e;
        if (++b > K) {
          ++a;
          b = a;
        }
      }
      ea[m] = a < K ? a : 0;
      eb[m] = a < K ? b : 0;
      sr[m] = si[m] = 0.0;
    }
  }
  int bad = 0;
  const int tt = t & (XM_HS_T - 1), h = t / XM_HS_T;
  for (int t0 = 0; t0 < A.N; t0 += XM_HS_T) {
    const int npts = A.N - t0 < XM_HS_T ? A.N - t0 : XM_HS_T;
    if (tt < npts) {
      for (int k = h; k < K; k += XM_HS_NT / XM_HS_T) {
        const hz p = hs_power(L.lz[2 * k], L.lz[2 * k + 1], t0 + tt);
        if (!isfinite(p.r) || !isfinite(p.i)) bad = 1;
        Bre[k * XM_HS_LDT + tt] = p.r;
        Bim[k * XM_HS_LDT + tt] = p.i;
      }
      if (h == 0) {
        double re, im;
        hs_load(A.x, A.is_c128, xoff + t0 + tt, re, im);
        Bre[K * XM_HS_LDT + tt] = re;
        Bim[K * XM_HS_LDT + tt] = im;
      }
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < XM_HS_MAXP; ++m) {
      if (t + XM_HS_NT * m < ne) {
        const double *ar = Bre + ea[m] * XM_HS_LDT, *ai = Bim + ea[m] * XM_HS_LDT;
        const double *br = Bre + eb[m] * XM_HS_LDT, *bi = Bim + eb[m] * XM_HS_LDT;
#pragma unroll 4
        for (int k = 0; k < npts; ++k) {  // conj(B_a) B_b
          sr[m] += ar[k] * br[k] + ai[k] * bi[k];
          si[m] += ar[k] * bi[k] - ai[k] * br[k];
        }
      }
    }
    __syncthreads();
  }
  if (__syncthreads_or(bad)) return 4;
#pragma unroll
  for (int m = 0; m < XM_HS_MAXP; ++m) {
    if (t + XM_HS_NT * m < ne) {
      double* dst = eb[m] < K ? Nm + 2 * (ea[m] * K + eb[m]) : rhs + 2 * ea[m];
      dst[0] = sr[m];
      dst[1] = si[m];
    }
  }
  __syncthreads();
  // Cholesky, column by column, rows spread over the workgroup (wg_cholesky of xm_wg.h, complex)
  for (int j = 0; j < K; ++j) {
    double s = Nm[2 * (j * K + j)];
    for (int k = 0; k < j; ++k) s -= hz_abs2(hz_ld(Nm, j * K + k));
    if (!(s > 0.0) || !isfinite(s)) {
      __syncthreads();
      return 4;
    }
    const double dj = sqrt(s);
    for (int i = j + 1 + t; i < K; i += XM_HS_NT) {
      hz v = hz_ld(Nm, j * K + i);
      v.i = -v.i;  // N[i][j] = conj(N[j][i])
      for (int k = 0; k < j; ++k) v = hz_sub(v, hz_mulc(hz_ld(Nm, i * K + k), hz_ld(Nm, j * K + k)));
      hz_st(Nm, i * K + j, hz_scale(v, 1.0 / dj));
    }
    if (t == 0) ld[j] = dj;
    __syncthreads();
  }
  if (t == 0) {
    for (int j = 0; j < K; ++j) {  // L u = B^H x
      hz v = hz_ld(rhs, j);
      for (int k = 0; k < j; ++k) v = hz_sub(v, hz_mul(hz_ld(Nm, j * K + k), hz_ld(rhs, k)));
      hz_st(rhs, j, hz_scale(v, 1.0 / ld[j]));
    }
    for (int j = K - 1; j >= 0; --j) {  // L^H a = u
      hz v = hz_ld(rhs, j);
      for (int k = j + 1; k < K; ++k) v = hz_sub(v, hz_cmul(hz_ld(Nm, k * K + j), hz_ld(L.a, k)));
      hz_st(L.a, j, hz_scale(v, 1.0 / ld[j]));
    }
  }
  __syncthreads();
  int nf = 0;
  for (int j = 0; j < 2 * K; ++j) nf |= !isfinite(L.a[j]);
  __syncthreads();
  return nf ? 4 : 0;
}

// the outputs of a FID that is not decomposed: y zero (status 2), x itself (1, 3, 4) or untouched (`copy` < 0: the
// timing-only stops), components NaN
XM_DEV void hs_degenerate(const HsvdArgs& A, long long v, long long xoff, int status, int copy) {
  const int t = threadIdx.x;
  if (A.y && copy >= 0)
    for (int i = t; i < A.N; i += XM_HS_NT) {
      double re = 0.0, im = 0.0;
      if (copy) hs_load(A.x, A.is_c128, xoff + i, re, im);
      hs_store(A.y, A.is_c128, v * A.N + i, re, im);
    }
  if (t < A.K) {
    A.freq[v * A.K + t] = NAN;
    A.damp[v * A.K + t] = NAN;
    A.amp[v * A.K + t] = NAN;
    A.phase[v * A.K + t] = NAN;
    A.removed[v * A.K + t] = 0;
  }
  if (t == 0) {
    A.n_removed[v] = 0;
    A.status[v] = status;
  }
}

enum { XM_HS_FORM_MFMA = 0, XM_HS_FORM_FMA = 1 };

template <int FORM>
__global__ __launch_bounds__(XM_HS_NT) void k_hsvd(HsvdArgs A) {
  extern __shared__ double hs_sm[];
  const int t = threadIdx.x, M = A.M, K = A.K;
  HsLds L;
  L.G = hs_sm;
  L.V = L.G + 2 * (size_t)M * M;
  L.seg = hs_sm + hs_big_doubles(M, K);
  L.scr = L.seg + 2 * XM_HS_SEG;
  L.red = L.scr + 1024;
  L.rot = L.red + XM_HS_NT;
  L.lam = L.rot + XM_WG_ROT * 32 + 32;
  L.z = L.lam + XM_HS_MAXM;
  L.lz = L.z + 2 * XM_HS_MAXK;
  L.a = L.lz + 2 * XM_HS_MAXK;
  L.f = L.a + 2 * XM_HS_MAXK;
  L.d = L.f + XM_HS_MAXK;
  L.idx = (int*)(L.d + XM_HS_MAXK);
  __shared__ unsigned next;

  for (;;) {
    const long long v = wg_next_item(A.counter, &next);
    if (v >= A.nb) break;
    const long long xoff = v * A.stride;

    int flags = 0;
    if (FORM == XM_HS_FORM_MFMA)
      hs_gram_mfma(A, L, xoff, flags);
    else
      hs_gram_fma(A, L, xoff, flags);
    flags = __syncthreads_or(flags & 1) | (__syncthreads_or(flags & 2) ? 2 : 0);
    if ((flags & 1) || !(flags & 2)) {  // a non-finite sample, or nothing but zeros
      hs_degenerate(A, v, xoff, (flags & 1) ? 2 : 1, (flags & 1) ? 0 : 1);
      __syncthreads();
      continue;
    }
    int status = 0;
    if (A.stop != XM_HS_STOP_GRAM) {
      const int sweeps = wg_jacobi(L.G, L.V, L.red, L.rot, M);
      if (sweeps < 0)
        status = 2;  // finite samples so large that G or its squared norm overflows
      else if (sweeps > XM_WG_SWEEPS)
        status = 3;
    }
    if (status == 0 && A.stop != XM_HS_STOP_GRAM && A.stop != XM_HS_STOP_EIG) {
      hs_select(L, M, K);
      if (!hs_shift_matrix(L, M, K)) {
        status = 4;
      } else {
        double f = 0.0;
        for (int e = t; e < 2 * K * K; e += XM_HS_NT) f += L.V[e] * L.V[e];
        const double hnorm = sqrt(wg_sum(L.red, f));
        hs_hessenberg(L, K);
        if (!hs_qr(L, K, hnorm))
          status = 3;
        else if (hs_poles(A, L))
          status = 4;
      }
    }
    if (status == 0 && (A.stop == XM_HS_STOP_NONE || A.stop == XM_HS_STOP_AMPL))
      status = hs_amplitudes(A, L, hs_sm, xoff);
    if (status != 0 || A.stop != XM_HS_STOP_NONE) {
      hs_degenerate(A, v, xoff, status, status == 2 ? 0 : status == 0 ? -1 : 1);
      __syncthreads();
      continue;
    }

    int nsel = 0;
    for (int k = 0; k < K; ++k) nsel += L.idx[k];
    if (t < K) {
      const hz a = hz_ld(L.a, t);
      A.freq[v * K + t] = L.f[t];
      A.damp[v * K + t] = L.d[t];
      A.amp[v * K + t] = hypot(a.r, a.i);
      A.phase[v * K + t] = atan2(a.i, a.r);
      A.removed[v * K + t] = L.idx[t];
    }
    if (t == 0) {
      A.n_removed[v] = nsel;
      A.status[v] = nsel ? 0 : 1;
    }
    if (A.y) {
#pragma unroll 1
      for (int p = t; p < A.N; p += XM_HS_NT) {
        double yr, yi;
        hs_load(A.x, A.is_c128, xoff + p, yr, yi);
        if (nsel)
          for (int k = 0; k < K; ++k)
            if (L.idx[k]) {
              const hz m = hz_mul(hz_ld(L.a, k), hs_power(L.lz[2 * k], L.lz[2 * k + 1], p));
              yr -= m.r;
              yi -= m.i;
            }
        hs_store(A.y, A.is_c128, v * A.N + p, yr, yi);
      }
    }
    __syncthreads();
  }
  wg_leave(A.counter);
}
