// SENSE unfolding kernel (the project's own definition, the reference has no such function).
// Included by xm_sense.hip alone; nothing but xm_common.h is shared with the other kernels.
//
// One group: a reduced-FOV voxel p = (p1, p2, p3) and the R = R1 R2 R3 full-FOV voxels that fold onto it,
// q_a = (p_a - n_a / 2 + N_a / 2 + k_a n_a) mod N_a, N_a = R_a n_a, member k = (k1 R2 + k2) R3 + k3.  The active members
// are those whose sensitivity column is not zero in every coil; S = their C x Ra columns, Sw = Linv S, A = Sw^H Sw,
// lambda' = regularization trace(A) / Ra, B = (A + lambda' I)^-1 Sw^H by Cholesky, U = sqrt(R) B Linv,
// rho[q_k, t] = sum_c U[k][c] a_c[p, t], g[q_k] = sqrt((B B^H)_kk A_kk).
//
// k_sense_unfold: one 256-thread workgroup per (outer, reduced voxel), groups handed out by a device counter (persistent
// grid).  The prologue runs in the LDS in fp64; then the group's C rows of a are streamed once: thread t takes the time
// points t, t + 256, ... (complex64 with 16-byte aligned rows: the pairs 2 t, 2 t + 512, ...), loads coil samples of them
// into registers, 128 bytes in flight per thread (each load a coalesced run along time over the workgroup; no sample is
// shared between threads, so the tile makes no trip through the LDS), and
// accumulates the Ra output rows from U in the LDS (every lane the same address: a broadcast) in ascending coil order,
// every step a fused multiply-add.  The rows are rounded once to the data's dtype and stored at the R full-FOV positions.
// RB is R rounded up to a power of two: the accumulators are a register array of that size, rows past Ra hold zeros.
#pragma once
#include "xm_wg.h"

#define XM_SN_MAXC 64
#define XM_SN_MAXR 16
#define XM_SN_NT 256  // threads, and time points per tile
#define XM_SN_PAD 16  // rows of U are padded to a multiple of this: the most coil samples a thread has in flight

struct SenseArgs {
  const void* a;       // aliased images: outer, coil, three spatial axes by strides, time contiguous
  void* y;             // unfolded images: outer, three spatial axes by strides, time contiguous; the dtype of a
  const double* sens;  // [C, N1, N2, N3] complex128
  const double* linv;  // C x C complex128 row-major, or nullptr for the identity
  double* g;           // [n_outer, N1, N2, N3] or nullptr
  int* status;         // [n_outer, N1, N2, N3] or nullptr
  long long ngroups;   // n_outer n1 n2 n3
  long long as[5], ys[4];
  int C, n[3], R[3], Nt, Rtot;
  int pair;  // complex64: every row of a and y starts on a 16-byte boundary and N_t is even
  double reg;
  unsigned* counter;  // [2] zero at launch: group ticket, workgroups done
};

__host__ __device__ inline int sn_pad(int C) { return (C + XM_SN_PAD - 1) / XM_SN_PAD * XM_SN_PAD; }
// doubles of the dynamic LDS: S / U (the larger of the two), Sw, B, A, then the small arrays
__host__ __device__ inline size_t sn_su_doubles(int C, int R, int RB) {
  const size_t s = 2 * (size_t)C * R, u = 2 * (size_t)sn_pad(C) * RB;
  return s > u ? s : u;
}
#define XM_SN_SMALL (6 * XM_SN_MAXR + 8)  // adiag, gk, yoff, qlin (8-byte words), alist + mlist, flags
__host__ __device__ inline size_t sn_lds_bytes(int C, int R, int RB) {
  return (sn_su_doubles(C, R, RB) + 4 * (size_t)C * R + 2 * (size_t)R * R + XM_SN_SMALL) * sizeof(double);
}

struct SnLds {
  double *SU, *Sw, *B, *A, *adiag, *gk;
  long long *yoff, *qlin;  // per member: first element of its row of y, its index in the full grid
  int *alist, *mlist;      // active members in ascending order, then the masked ones
  int* word;               // [0] ticket, [1] Ra, [2] flags of the prologue
};

template <class T>
XM_DEV void sn_store(void* y, long long i, double re, double im) {
  Cx<T>* p = (Cx<T>*)y + i;
  *p = mk<T>((T)re, (T)im);
}

// zero rows, g and status of every member of a group that is not unfolded (status 2 or 3: g NaN; no active member: 1, g 0)
template <class T>
XM_DEV void sn_degenerate(const SenseArgs& A, const SnLds& L, long long gbase, int status) {
  const int t = threadIdx.x;
  for (int k = 0; k < A.Rtot; ++k)
    for (int i = t; i < A.Nt; i += XM_SN_NT) sn_store<T>(A.y, L.yoff[k] + i, 0.0, 0.0);
  if (t < A.Rtot) {
    if (A.g) A.g[gbase + L.qlin[t]] = status == 1 ? 0.0 : NAN;
    if (A.status) A.status[gbase + L.qlin[t]] = status;
  }
}

// 1 when the group's C rows of a, which start at abase, hold a non-finite sample (the same value in every thread)
template <class T>
XM_DEV int sn_data_bad(const SenseArgs& A, long long abase) {
  const Cx<T>* a = (const Cx<T>*)A.a;
  int bad = 0;
  for (int c = 0; c < A.C; ++c)
    for (int i = threadIdx.x; i < A.Nt; i += XM_SN_NT) {
      const Cx<T> s = a[abase + c * A.as[1] + i];
      if (!isfinite((double)s.re) || !isfinite((double)s.im)) bad = 1;
    }
  return __syncthreads_or(bad);
}

// The prologue: members, S, Sw, A, Cholesky, B, U and g in the LDS.  Returns 0, or the status of a group that is not
// unfolded.  On 0: L.word[1] = Ra, U in L.SU as [sn_pad(C)][RB] (zero past C and past Ra), g in L.gk.
template <int RB>
XM_DEV int sn_prologue(const SenseArgs& A, const SnLds& L, long long o, int p1, int p2, int p3) {
  const int t = threadIdx.x, C = A.C, R = A.Rtot;
  const long long N2 = (long long)A.R[1] * A.n[1], N3 = (long long)A.R[2] * A.n[2], N1 = (long long)A.R[0] * A.n[0];
  const long long nfull = N1 * N2 * N3;
  if (t < R) {
    const int k3 = t % A.R[2], k2 = (t / A.R[2]) % A.R[1], k1 = t / (A.R[2] * A.R[1]);
    const long long q1 = ((long long)p1 - A.n[0] / 2 + N1 / 2 + (long long)k1 * A.n[0]) % N1;
    const long long q2 = ((long long)p2 - A.n[1] / 2 + N2 / 2 + (long long)k2 * A.n[1]) % N2;
    const long long q3 = ((long long)p3 - A.n[2] / 2 + N3 / 2 + (long long)k3 * A.n[2]) % N3;
    L.qlin[t] = (q1 * N2 + q2) * N3 + q3;
    L.yoff[t] = o * A.ys[0] + q1 * A.ys[1] + q2 * A.ys[2] + q3 * A.ys[3];
  }
  if (t == 0) L.word[2] = 0;
  __syncthreads();
  // 1. S[c][k], all R members
  int bad = 0;
  for (int e = t; e < C * R; e += XM_SN_NT) {
    const int c = e / R, k = e - c * R;
    const double* s = A.sens + 2 * (c * nfull + L.qlin[k]);
    const double re = s[0], im = s[1];
    if (!isfinite(re) || !isfinite(im)) bad = 1;
    L.SU[2 * e] = re;
    L.SU[2 * e + 1] = im;
  }
  if (__syncthreads_or(bad)) return 2;
  if (t == 0) {  // the active set, ascending
    int ra = 0, rm = 0;
    for (int k = 0; k < R; ++k) {
      int on = 0;
      for (int c = 0; c < C; ++c) on |= L.SU[2 * (c * R + k)] != 0.0 || L.SU[2 * (c * R + k) + 1] != 0.0;
      if (on)
        L.alist[ra++] = k;
      else
        L.mlist[rm++] = k;
    }
    L.word[1] = ra;
  }
  __syncthreads();
  const int Ra = L.word[1];
  if (Ra == 0) return 1;
  if (Ra > C && !(A.reg > 0.0)) return 3;  // more unknowns than coils: singular whatever the rounding does
  // 2. Sw[c][j] = sum_c' Linv[c][c'] S[c'][alist[j]], ascending c'
  for (int e = t; e < C * Ra; e += XM_SN_NT) {
    const int c = e / Ra, j = e - c * Ra, k = L.alist[j];
    double sr = L.SU[2 * (c * R + k)], si = L.SU[2 * (c * R + k) + 1];
    if (A.linv) {
      sr = si = 0.0;
      for (int d = 0; d < C; ++d) {
        const double lr = A.linv[2 * (c * C + d)], li = A.linv[2 * (c * C + d) + 1];
        const double xr = L.SU[2 * (d * R + k)], xi = L.SU[2 * (d * R + k) + 1];
        sr = fma(lr, xr, sr);
        sr = fma(-li, xi, sr);
        si = fma(lr, xi, si);
        si = fma(li, xr, si);
      }
    }
    L.Sw[2 * e] = sr;
    L.Sw[2 * e + 1] = si;
  }
  __syncthreads();
  // 3. the lower triangle of A[i][j] = sum_c conj(Sw[c][i]) Sw[c][j], ascending c; the diagonal real
  for (int e = t; e < Ra * Ra; e += XM_SN_NT) {
    const int i = e / Ra, j = e - i * Ra;
    if (i < j) continue;
    double sr = 0.0, si = 0.0;
    for (int c = 0; c < C; ++c) {
      const double ar = L.Sw[2 * (c * Ra + i)], ai = L.Sw[2 * (c * Ra + i) + 1];
      const double br = L.Sw[2 * (c * Ra + j)], bi = L.Sw[2 * (c * Ra + j) + 1];
      sr = fma(ar, br, sr);
      sr = fma(ai, bi, sr);
      si = fma(ar, bi, si);
      si = fma(-ai, br, si);
    }
    L.A[2 * e] = sr;
    L.A[2 * e + 1] = i == j ? 0.0 : si;
  }
  __syncthreads();
  double tr = 0.0;
  for (int k = 0; k < Ra; ++k) tr += L.A[2 * (k * Ra + k)];
  const double lam = A.reg * tr / (double)Ra;
  __syncthreads();
  if (t < Ra) {
    L.adiag[t] = L.A[2 * (t * Ra + t)];
    L.A[2 * (t * Ra + t)] += lam;
  }
  __syncthreads();
  // 4. Cholesky A + lambda' I = G G^H in place, column by column; a pivot <= 0 or non-finite ends it
  for (int j = 0; j < Ra; ++j) {
    if (t == 0) {
      double d = L.A[2 * (j * Ra + j)];
      for (int k = 0; k < j; ++k) {
        const double gr = L.A[2 * (j * Ra + k)], gi = L.A[2 * (j * Ra + k) + 1];
        d = fma(-gr, gr, d);
        d = fma(-gi, gi, d);
      }
      if (!(d > 0.0) || !isfinite(d)) L.word[2] = 3;
      L.A[2 * (j * Ra + j)] = sqrt(d);
    }
    __syncthreads();
    if (L.word[2]) break;
    const int i = j + 1 + t;
    if (i < Ra) {
      double sr = L.A[2 * (i * Ra + j)], si = L.A[2 * (i * Ra + j) + 1];
      for (int k = 0; k < j; ++k) {  // - G[i][k] conj(G[j][k])
        const double ar = L.A[2 * (i * Ra + k)], ai = L.A[2 * (i * Ra + k) + 1];
        const double br = L.A[2 * (j * Ra + k)], bi = L.A[2 * (j * Ra + k) + 1];
        sr = fma(-ar, br, sr);
        sr = fma(-ai, bi, sr);
        si = fma(-ai, br, si);
        si = fma(ar, bi, si);
      }
      const double piv = L.A[2 * (j * Ra + j)];
      L.A[2 * (i * Ra + j)] = sr / piv;
      L.A[2 * (i * Ra + j) + 1] = si / piv;
    }
    __syncthreads();
  }
  if (L.word[2]) return 3;
  // 5. B[:, c] = (G G^H)^-1 conj(Sw[c][:]): thread c substitutes forward and back in its own column of B
  if (t < C) {
    for (int i = 0; i < Ra; ++i) {
      double sr = L.Sw[2 * (t * Ra + i)], si = -L.Sw[2 * (t * Ra + i) + 1];
      for (int k = 0; k < i; ++k) {  // - G[i][k] B[k]
        const double gr = L.A[2 * (i * Ra + k)], gi = L.A[2 * (i * Ra + k) + 1];
        const double br = L.B[2 * (k * C + t)], bi = L.B[2 * (k * C + t) + 1];
        sr = fma(-gr, br, sr);
        sr = fma(gi, bi, sr);
        si = fma(-gr, bi, si);
        si = fma(-gi, br, si);
      }
      const double piv = L.A[2 * (i * Ra + i)];
      L.B[2 * (i * C + t)] = sr / piv;
      L.B[2 * (i * C + t) + 1] = si / piv;
    }
    for (int i = Ra - 1; i >= 0; --i) {
      double sr = L.B[2 * (i * C + t)], si = L.B[2 * (i * C + t) + 1];
      for (int k = i + 1; k < Ra; ++k) {  // - conj(G[k][i]) B[k]
        const double gr = L.A[2 * (k * Ra + i)], gi = L.A[2 * (k * Ra + i) + 1];
        const double br = L.B[2 * (k * C + t)], bi = L.B[2 * (k * C + t) + 1];
        sr = fma(-gr, br, sr);
        sr = fma(-gi, bi, sr);
        si = fma(-gr, bi, si);
        si = fma(gi, br, si);
      }
      const double piv = L.A[2 * (i * Ra + i)];
      L.B[2 * (i * C + t)] = sr / piv;
      L.B[2 * (i * C + t) + 1] = si / piv;
    }
  }
  for (int e = t; e < 2 * sn_pad(C) * RB; e += XM_SN_NT) L.SU[e] = 0.0;  // (S is not read any more)
  __syncthreads();
  // U[c][j] = sqrt(R) sum_d B[j][d] Linv[d][c], ascending d; g[j] = sqrt((B B^H)_jj A_jj)
  const double root = sqrt((double)R);
  for (int e = t; e < Ra * C; e += XM_SN_NT) {
    const int j = e / C, c = e - j * C;
    double ur = L.B[2 * e], ui = L.B[2 * e + 1];
    if (A.linv) {
      ur = ui = 0.0;
      for (int d = 0; d < C; ++d) {
        const double lr = A.linv[2 * (d * C + c)], li = A.linv[2 * (d * C + c) + 1];
        const double br = L.B[2 * (j * C + d)], bi = L.B[2 * (j * C + d) + 1];
        ur = fma(br, lr, ur);
        ur = fma(-bi, li, ur);
        ui = fma(br, li, ui);
        ui = fma(bi, lr, ui);
      }
    }
    L.SU[2 * (c * RB + j)] = root * ur;
    L.SU[2 * (c * RB + j) + 1] = root * ui;
  }
  if (t < Ra) {
    double s = 0.0;
    for (int c = 0; c < C; ++c) {
      const double br = L.B[2 * (t * C + c)], bi = L.B[2 * (t * C + c) + 1];
      s = fma(br, br, s);
      s = fma(bi, bi, s);
    }
    L.gk[t] = sqrt(s * L.adiag[t]);
  }
  __syncthreads();
  return 0;
}

// The stream of one group: y rows from U (L.SU) and the group's C rows of a, which start at abase.  TP time points per
// thread and step: 2 for complex64 up to R = 8 when every row of a and y starts on a 16-byte boundary and N_t is even (A.pair), so
// that a lane moves 16 bytes per load and store as it does in complex128.  The arithmetic per sample is the same in
// both forms.  Returns 1 when this thread met a non-finite sample.
template <class T, int RB, int TP>
XM_DEV int sn_stream(const SenseArgs& A, const SnLds& L, long long abase, int Ra) {
  constexpr int CB = 128 / (TP * (int)sizeof(Cx<T>));  // 128 bytes in flight per thread: 16, 8 (pairs) or 8 (complex128)
  typedef T sn_v __attribute__((ext_vector_type(2 * TP)));
  const int t = threadIdx.x, C = A.C, R = A.Rtot;
  const int Cp = (C + CB - 1) / CB * CB;
  const long long acs = A.as[1];
  const T* a = (const T*)A.a;
  int bad = 0;
  for (int t0 = 0; t0 < A.Nt; t0 += XM_SN_NT * TP) {
    const int i = t0 + TP * t;
    const bool in = i < A.Nt;  // (pairs: N_t is even, so both points are inside or both outside)
    double yr[TP][RB], yi[TP][RB];
#pragma unroll
    for (int h = 0; h < TP; ++h)
#pragma unroll
      for (int j = 0; j < RB; ++j) yr[h][j] = yi[h][j] = 0.0;
    for (int c0 = 0; c0 < Cp; c0 += CB) {
      sn_v s[CB];
#pragma unroll
      for (int m = 0; m < CB; ++m)
        s[m] = in && c0 + m < C ? *(const sn_v*)(a + 2 * (abase + (c0 + m) * acs + i)) : (sn_v)(T)0;
#pragma unroll
      for (int m = 0; m < CB; ++m) {
        const double* u = L.SU + 2 * (size_t)(c0 + m) * RB;
#pragma unroll
        for (int h = 0; h < TP; ++h) {
          const double re = (double)s[m][2 * h], im = (double)s[m][2 * h + 1];
          if (!isfinite(re) || !isfinite(im)) bad = 1;
#pragma unroll
          for (int j = 0; j < RB; ++j) {
            const double ur = u[2 * j], ui = u[2 * j + 1];
            yr[h][j] = fma(ur, re, yr[h][j]);
            yr[h][j] = fma(-ui, im, yr[h][j]);
            yi[h][j] = fma(ur, im, yi[h][j]);
            yi[h][j] = fma(ui, re, yi[h][j]);
          }
        }
      }
    }
    if (in) {
      T* y = (T*)A.y;
#pragma unroll
      for (int j = 0; j < RB; ++j)
        if (j < Ra) {
          sn_v o;
#pragma unroll
          for (int h = 0; h < TP; ++h) {
            o[2 * h] = (T)yr[h][j];
            o[2 * h + 1] = (T)yi[h][j];
          }
          *(sn_v*)(y + 2 * (L.yoff[L.alist[j]] + i)) = o;
        }
      for (int m = 0; m < R - Ra; ++m) *(sn_v*)(y + 2 * (L.yoff[L.mlist[m]] + i)) = (sn_v)(T)0;
    }
  }
  return bad;
}

template <class T, int RB>
__global__ __launch_bounds__(XM_SN_NT, 2) void k_sense_unfold(SenseArgs A) {
  extern __shared__ __attribute__((aligned(16))) double sn_sm[];
  const int t = threadIdx.x, C = A.C, R = A.Rtot;
  SnLds L;
  L.SU = sn_sm;
  L.Sw = L.SU + sn_su_doubles(C, R, RB);
  L.B = L.Sw + 2 * (size_t)C * R;
  L.A = L.B + 2 * (size_t)C * R;
  L.adiag = L.A + 2 * (size_t)R * R;
  L.gk = L.adiag + XM_SN_MAXR;
  L.yoff = (long long*)(L.gk + XM_SN_MAXR);
  L.qlin = L.yoff + XM_SN_MAXR;
  L.alist = (int*)(L.qlin + XM_SN_MAXR);
  L.mlist = L.alist + XM_SN_MAXR;
  L.word = L.mlist + XM_SN_MAXR;
  const long long nred = (long long)A.n[0] * A.n[1] * A.n[2];
  const long long nfull = nred * R;

  for (;;) {
    const long long v = wg_next_item(A.counter, (unsigned*)L.word);
    if (v >= A.ngroups) break;
    const long long o = v / nred, p = v - o * nred;
    const int p3 = (int)(p % A.n[2]), p2 = (int)((p / A.n[2]) % A.n[1]), p1 = (int)(p / ((long long)A.n[2] * A.n[1]));
    const long long gbase = o * nfull;

    int st = sn_prologue<RB>(A, L, o, p1, p2, p3);
    const long long abase = o * A.as[0] + p1 * A.as[2] + p2 * A.as[3] + p3 * A.as[4];
    if (st == 3 && sn_data_bad<T>(A, abase)) st = 2;  // 2 wins over 3: a group that cannot be solved still looks at its data
    if (st) {
      sn_degenerate<T>(A, L, gbase, st);
      __syncthreads();
      continue;
    }
    const int Ra = L.word[1];
    int bad;
    if constexpr (sizeof(T) == 4 && RB <= 8)  // (at RB = 16 two points' accumulators do not fit the registers)
      bad = A.pair ? sn_stream<T, RB, 2>(A, L, abase, Ra) : sn_stream<T, RB, 1>(A, L, abase, Ra);
    else
      bad = sn_stream<T, RB, 1>(A, L, abase, Ra);
    // A non-finite data sample: nothing of the group is kept.  The zeros go over rows that other threads of the workgroup
    // have stored (paired form: another split of the points), so those stores are made visible to the workgroup first.
    __threadfence_block();
    if (__syncthreads_or(bad)) {
      sn_degenerate<T>(A, L, gbase, 2);
    } else {
      if (t < Ra) {
        if (A.g) A.g[gbase + L.qlin[L.alist[t]]] = L.gk[t];
        if (A.status) A.status[gbase + L.qlin[L.alist[t]]] = 0;
      } else if (t < R) {
        if (A.g) A.g[gbase + L.qlin[L.mlist[t - Ra]]] = 0.0;
        if (A.status) A.status[gbase + L.qlin[L.mlist[t - Ra]]] = 1;
      }
    }
    __syncthreads();
  }
  wg_leave(A.counter);
}
