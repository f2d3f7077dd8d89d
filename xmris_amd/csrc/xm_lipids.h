// Lipid-subspace (L2) suppression of 1H MRSI (the project's own definition, the reference has no
// such function).  Included by xm_lipids.hip only.
//
// A row is one FID of T samples.  With the orthonormal time-domain vectors u_k (k < r) of the lipid subspace and the
// weights w_k from the host,
//     c_k = sum_t conj(u_k[t]) y[t],     out[t] = y[t] - sum_k u_k[t] (w_k c_k).
// All arithmetic fp64; complex64 is widened on load and the result rounded once on store.
//
// k_lipid_project<MFMA, C128, NJ>: one 256-thread workgroup per tile of 16 consecutive rows, the N of
// v_mfma_f64_16x16x4_f64.  The time axis is walked twice in chunks of XM_LP_TC points; a chunk of the table U[T][r] is
// staged in the LDS (row pitch = 2 (mod 32) doubles, which keeps both operand reads free of bank conflicts) and read by
// every wave; the next chunk's share of a thread waits in NJ 16-byte registers (NJ = 2, 4, 8 for ranks up to 16, 32, 64:
// the rank-64 size costs the smaller ranks a resident workgroup) while the matrix cores work on this one.  The complex
// products are embedded as real ones:
//   stage 1  C (2r x 16) = A1 (2r x 2T) Y (2T x 16):   A1[2k + p][2t + q] = (ur, ui; -ui, ur)[p][q],  Y[2t + q][n]
//   stage 2  S (2T x 16) = A2 (2T x 2r) D (2r x 16):   A2[2t + p][2k + q] = (ur, -ui; ui, ur)[p][q],  D = w C
// Operands of the MFMA: lane l holds A[l & 15][l >> 4] and B[l >> 4][l & 15]; result r of lane l is row (l >> 4) + 4 r,
// column l & 15.  A column of B (a row of the data) meets no other column, so a row's output depends on its own
// samples and the table only, whatever its place in the tile.
// Stage 1: wave w takes the points 8 w ... 8 w + 7 of every chunk into <= 8 accumulator blocks, chunks in ascending
// order; the four partial matrices are added in wave order through the LDS.  Stage 2: wave w takes the points
// 8 w ... 8 w + 7 of every chunk, K = 2r from the LDS coefficients D; the sums go through the LDS to the threads that
// load y again (from L2 / the Infinity Cache), subtract, round and store, 16 bytes at a time along time where the
// layout allows.  Tail tiles, tail chunks and K are padded with zeros in registers; nothing outside the rows, T or the
// table is read.
// The plain-FMA form (MFMA = false) keeps the staging and gives thread (row n, slot g) the coefficients g, g + 16, ...
// in stage 1 and the two samples it loads and stores in stage 2, every sum one chain in ascending order.
#pragma once
#include "xm_wg.h"

#define XM_LP_NT 256
#define XM_LP_ROWS 16
#define XM_LP_TC 32    // time points per chunk: 8 per wave
#define XM_LP_MAXR 64
#define XM_LP_MAXB 8   // 16-row blocks of the 2r coefficient rows
#define XM_LP_OP (2 * XM_LP_TC + 2)  // pitch of a row of the stage 2 sums, doubles

static_assert(XM_LP_NT == XM_WG_NT, "k_lipid_project is a 256-thread workgroup kernel");

// test-only bits on top of the dtype argument (XM_LIPID_* of xmris_hip.h, shifted down by 8)
#define XM_LP_FMA 1
#define XM_LP_SKIP_COEF 2
#define XM_LP_SKIP_APPLY 4

struct LipidArgs {
  const void* x;               // rows x_stride elements apart, time stride 1
  void* y;                     // rows y_stride elements apart
  const double* tab;           // U[T][r] (re, im), then w[r]
  const unsigned char* apply;  // per row, or nullptr (every row)
  int* status;                 // per row
  long long n_rows, xs, ys;
  int T, r, pitch, nblk, vec, skip;
};

// row pitch of the staged table: the smallest P >= 2r with P = 2 (mod 32)
__host__ __device__ inline int lp_pitch(int r) { return (2 * r - 2 + 31) / 32 * 32 + 2; }
__host__ __device__ inline int lp_blocks(int r) { return (2 * r + 15) / 16; }

// LDS, in doubles: the table chunk, the staged samples | the stage 2 sums, the coefficients, the weights; then the
// rows' flags (two ints per row)
__host__ __device__ inline size_t lp_lds_bytes(int r) {
  return ((size_t)XM_LP_TC * lp_pitch(r) + XM_LP_ROWS * XM_LP_OP + 256 * (size_t)lp_blocks(r) + XM_LP_MAXR) * sizeof(double) +
         2 * XM_LP_ROWS * sizeof(int);
}

template <bool C128>
struct LpPair {  // two consecutive samples of a row at storage precision
  typename std::conditional<C128, double, float>::type v[4];
};

// samples off, off + 1 of p (the second only when nv > 1, none when nv < 1; the rest zero)
template <bool C128>
XM_DEV LpPair<C128> lp_load(const void* p, long long off, int nv, bool vec) {
  LpPair<C128> q;
  q.v[0] = q.v[1] = q.v[2] = q.v[3] = 0;
  if constexpr (C128) {
    if (nv > 0) {
      const double2 a = ((const double2*)p)[off];
      q.v[0] = a.x, q.v[1] = a.y;
    }
    if (nv > 1) {
      const double2 a = ((const double2*)p)[off + 1];
      q.v[2] = a.x, q.v[3] = a.y;
    }
  } else {
    if (vec && nv > 1) {
      const float4 a = *(const float4*)((const float2*)p + off);
      q.v[0] = a.x, q.v[1] = a.y, q.v[2] = a.z, q.v[3] = a.w;
    } else {
      if (nv > 0) {
        const float2 a = ((const float2*)p)[off];
        q.v[0] = a.x, q.v[1] = a.y;
      }
      if (nv > 1) {
        const float2 a = ((const float2*)p)[off + 1];
        q.v[2] = a.x, q.v[3] = a.y;
      }
    }
  }
  return q;
}

template <bool C128>
XM_DEV void lp_store(void* p, long long off, int nv, bool vec, const LpPair<C128>& q) {
  if constexpr (C128) {
    if (nv > 0) ((double2*)p)[off] = make_double2(q.v[0], q.v[1]);
    if (nv > 1) ((double2*)p)[off + 1] = make_double2(q.v[2], q.v[3]);
  } else {
    if (vec && nv > 1) {
      *(float4*)((float2*)p + off) = make_float4(q.v[0], q.v[1], q.v[2], q.v[3]);
    } else {
      if (nv > 0) ((float2*)p)[off] = make_float2(q.v[0], q.v[1]);
      if (nv > 1) ((float2*)p)[off + 1] = make_float2(q.v[2], q.v[3]);
    }
  }
}

// A thread's share of a chunk of the table in registers: the loads of the next chunk are in flight while the matrix
// cores work on this one
template <int NJ>  // NJ = XM_LP_TC * (the rank class 16, 32 or 64) / XM_LP_NT
struct LpTab {
  double2 v[NJ];
};

// q <- the rows t0 ... t0 + XM_LP_TC - 1 of the table, zeros past T (nothing is read there)
template <int NJ>
XM_DEV void lp_fetch_table(const LipidArgs& A, int t0, LpTab<NJ>& q) {
  const int r = A.r;
  const double2* src = (const double2*)A.tab + (size_t)t0 * r;
  const int lim = (A.T - t0 < XM_LP_TC ? (A.T - t0 > 0 ? A.T - t0 : 0) : XM_LP_TC) * r;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int i = threadIdx.x + XM_LP_NT * j;
    q.v[j] = i < lim ? src[i] : make_double2(0.0, 0.0);
  }
}

// U <- q
template <int NJ>
XM_DEV void lp_put_table(const LipidArgs& A, double* U, const LpTab<NJ>& q) {
  const int r = A.r, P = A.pitch;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int i = threadIdx.x + XM_LP_NT * j;
    if (i < XM_LP_TC * r) {
      const int tl = i / r, k = i - tl * r;
      *(double2*)(U + tl * P + 2 * k) = q.v[j];
    }
  }
}

template <bool MFMA, bool C128, int NJ>
__global__ __launch_bounds__(XM_LP_NT) void k_lipid_project(LipidArgs A) {
  extern __shared__ double lp_sm[];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int T = A.T, r = A.r, P = A.pitch, nblk = A.nblk;
  double* U = lp_sm;                          // [tl][pitch]
  double* YO = U + (size_t)XM_LP_TC * P;      // stage 1: Y[2 tl + q][n]; stage 2: O[n][XM_LP_OP]
  double* D = YO + XM_LP_ROWS * XM_LP_OP;     // [16 nblk][n]
  double* W = D + 256 * (size_t)nblk;         // [r]
  int* bad = (int*)(W + XM_LP_MAXR);          // [n]
  int* app = bad + XM_LP_ROWS;                // [n]

  const long long row0 = (long long)blockIdx.x * XM_LP_ROWS;
  // the thread's own samples: row t >> 4 of the tile, points 2 (t & 15) and 2 (t & 15) + 1 of a chunk
  const int mrow = t >> 4, mtl = 2 * (t & 15);
  const long long grow = row0 + mrow;
  const bool live = grow < A.n_rows;
  const bool vec = A.vec != 0;

  if (t < XM_LP_ROWS) {
    bad[t] = 0;
    app[t] = row0 + t < A.n_rows && (!A.apply || A.apply[row0 + t] != 0);
  }
  for (int i = t; i < r; i += XM_LP_NT) W[i] = A.tab[2 * (size_t)T * r + i];
  __syncthreads();
  const bool any = __syncthreads_or(app[mrow]);  // a tile with nothing to project is copied

  // ---- stage 1: coefficients ---------------------------------------------------------------------------------------
  if (any && !(A.skip & XM_LP_SKIP_COEF)) {
    wg_d4 acc[XM_LP_MAXB];
    double cr[4], ci[4];
#pragma unroll
    for (int b = 0; b < XM_LP_MAXB; ++b) acc[b] = wg_d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < 4; ++j) cr[j] = ci[j] = 0.0;
    int nonfinite = 0;
    LpTab<NJ> tq;
    lp_fetch_table(A, 0, tq);
    LpPair<C128> q = lp_load<C128>(A.x, grow * A.xs + mtl, live ? T - mtl : 0, vec);
#pragma unroll 1
    for (int t0 = 0; t0 < T; t0 += XM_LP_TC) {
      lp_put_table(A, U, tq);
      {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const double v = (double)q.v[e];
          if (!isfinite(v)) nonfinite = 1;
          YO[(2 * mtl + e) * XM_LP_ROWS + mrow] = v;
        }
      }
      __syncthreads();
      if (t0 + XM_LP_TC < T) {  // the next chunk, on its way during the arithmetic
        lp_fetch_table(A, t0 + XM_LP_TC, tq);
        q = lp_load<C128>(A.x, grow * A.xs + t0 + XM_LP_TC + mtl, live ? T - (t0 + XM_LP_TC + mtl) : 0, vec);
      }
      if constexpr (MFMA) {
        if (t0 + 8 * wave < T) {  // wave-uniform: the MFMA runs with every lane on
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            const int tl = 8 * wave + 2 * s + (lane >> 5), qq = (lane >> 4) & 1;
            const double yb = YO[(2 * tl + qq) * XM_LP_ROWS + (lane & 15)];
            const double* ut = U + tl * P;
#pragma unroll
            for (int b = 0; b < XM_LP_MAXB; ++b)
              if (b < nblk) {
                const int m = 16 * b + (lane & 15), k = m >> 1, p = m & 1;
                double a = k < r ? ut[2 * k + (p ^ qq)] : 0.0;
                if (p == 1 && qq == 0) a = -a;
                acc[b] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, yb, acc[b], 0, 0, 0);
              }
          }
        }
      } else {
        const int n = t & 15, g = t >> 4, nt = T - t0 < XM_LP_TC ? T - t0 : XM_LP_TC;
#pragma unroll 1
        for (int tl = 0; tl < nt; ++tl) {
          const double yr = YO[(2 * tl) * XM_LP_ROWS + n], yi = YO[(2 * tl + 1) * XM_LP_ROWS + n];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int k = g + 16 * j;
            if (k < r) {
              const double ur = U[tl * P + 2 * k], ui = U[tl * P + 2 * k + 1];
              cr[j] += ur * yr + ui * yi;
              ci[j] += ur * yi - ui * yr;
            }
          }
        }
      }
      __syncthreads();  // the chunk is read
    }
    if (nonfinite) bad[mrow] = 1;  // (every writer stores the same value)
    if constexpr (MFMA) {
      for (int wv = 0; wv < 4; ++wv) {  // the waves' partial matrices, added in wave order
        if (wave == wv) {
#pragma unroll
          for (int b = 0; b < XM_LP_MAXB; ++b)
            if (b < nblk)
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                const int idx = (16 * b + (lane >> 4) + 4 * e) * XM_LP_ROWS + (lane & 15);
                D[idx] = wv == 0 ? acc[b][e] : D[idx] + acc[b][e];
              }
        }
        __syncthreads();
      }
      for (int i = t; i < 256 * nblk; i += XM_LP_NT) {
        const int k = i >> 5;
        D[i] = k < r ? D[i] * W[k] : 0.0;
      }
    } else {
      const int n = t & 15, g = t >> 4;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = g + 16 * j;
        if (k < r) {
          D[(2 * k) * XM_LP_ROWS + n] = cr[j] * W[k];
          D[(2 * k + 1) * XM_LP_ROWS + n] = ci[j] * W[k];
        }
      }
      for (int i = 2 * r * XM_LP_ROWS + t; i < 256 * nblk; i += XM_LP_NT) D[i] = 0.0;
    }
  } else {
    for (int i = t; i < 256 * nblk; i += XM_LP_NT) D[i] = 0.0;
  }
  __syncthreads();

  if (t < XM_LP_ROWS && row0 + t < A.n_rows) A.status[row0 + t] = !app[t] ? 1 : bad[t] ? 2 : 0;
  if (A.skip & XM_LP_SKIP_APPLY) return;

  // ---- stage 2: apply ----------------------------------------------------------------------------------------------
  const bool project = app[mrow] != 0, isbad = bad[mrow] != 0;
  LpTab<NJ> tq;
  if (any) lp_fetch_table(A, 0, tq);
#pragma unroll 1
  for (int t0 = 0; t0 < T; t0 += XM_LP_TC) {
    const int nv = live ? T - (t0 + mtl) : 0;
    const LpPair<C128> q = lp_load<C128>(A.x, grow * A.xs + t0 + mtl, nv, vec);
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    if (any) {
      lp_put_table(A, U, tq);
      __syncthreads();
      if (t0 + XM_LP_TC < T) lp_fetch_table(A, t0 + XM_LP_TC, tq);
      if constexpr (MFMA) {
        if (t0 + 8 * wave < T) {
          wg_d4 acc = wg_d4{0.0, 0.0, 0.0, 0.0};
          const int m = lane & 15, p = m & 1;
          const double* ut = U + (8 * wave + (m >> 1)) * P;
          const int nsteps = (2 * r + 3) / 4;
#pragma unroll 2
          for (int st = 0; st < nsteps; ++st) {
            const int kk = 4 * st + (lane >> 4), k = kk >> 1, qq = kk & 1;
            double a = k < r ? ut[2 * k + (p ^ qq)] : 0.0;
            if (p == 0 && qq == 1) a = -a;
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, D[kk * XM_LP_ROWS + (lane & 15)], acc, 0, 0, 0);
          }
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int mm = (lane >> 4) + 4 * e;
            YO[(lane & 15) * XM_LP_OP + 2 * (8 * wave + (mm >> 1)) + (mm & 1)] = acc[e];
          }
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 4; ++e) s[e] = YO[mrow * XM_LP_OP + 2 * mtl + e];
      } else {
        if (nv > 0) {
#pragma unroll 4
          for (int k = 0; k < r; ++k) {
            const double dr = D[(2 * k) * XM_LP_ROWS + mrow], di = D[(2 * k + 1) * XM_LP_ROWS + mrow];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
              const double ur = U[(mtl + h) * P + 2 * k], ui = U[(mtl + h) * P + 2 * k + 1];
              s[2 * h] += ur * dr - ui * di;
              s[2 * h + 1] += ur * di + ui * dr;
            }
          }
        }
        __syncthreads();  // the chunk is read
      }
    }
    LpPair<C128> o = q;  // a row that is not projected: the same bits
    if (project) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        using S = typename std::conditional<C128, double, float>::type;
        o.v[e] = isbad ? (S)NAN : (S)((double)q.v[e] - s[e]);
      }
    }
    lp_store<C128>(A.y, grow * A.ys + t0 + mtl, nv, vec, o);
    // (MFMA: the sums of this chunk are read before the next chunk's are written: the barrier after the table's staging)
  }
}
