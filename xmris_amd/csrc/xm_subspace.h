// k_sub_project, k_sub_mix, k_sub_expand: the three kernels of temporal-subspace SENSE (xm_sub_* in
// include/xmris_hip.h; DESIGN.md section 26, the project's own definition).  Included by xm_subspace.hip only.
//
// With the basis V [R, T] complex128 (rows need not be orthonormal) and the sampling flags m [S, T]:
//   project  b[c, s, r, f] = sum_t m[s, t] conj(V[r, t]) y[c, s, f, t]          the only pass over the full data
//   mix      z[c, s, r, f] = sum_r' K_s[r, r'] a[c, s, r', f]                    K [S, R, R] complex128
//   expand   x[v, f, t]    = sum_r U[v, r, f] V[r, t]                            once at the end, complex128
// All arithmetic is fp64, every product-sum is a spelt-out FMA, every sum is ONE chain in ascending order of its index
// (t, r', r), started at zero; per term the real part takes (re re) then (im im), the imaginary part (re im) then
// (im re), as written in sub_cmac / sub_cmac_conj below.  The result is rounded once to the output dtype.  No atomics,
// no cross-lane sums: one thread owns one output, so an output's bits depend on its own inputs only -- not on the
// batch, on its place in a tile, on F or on the strides.
//
// k_sub_project<C128, NR>.  A row is one (s, c, f): T samples with time stride 1 anywhere in y (coil, sample and frame
// strides are arguments).  One 256-thread workgroup takes a tile of XM_SP_ROWS = 16 consecutive rows in the order
// (s, c, f) -- the rows of a tile may belong to several samples, each reads its own flags -- and walks the time axis
// in chunks of XM_SP_TC = 64 points.  Per chunk the samples of the 16 rows (widened to fp64, an unsampled position
// SELECTED to zero: what lies in y there, NaN included, is loaded and dropped) and the R rows of the basis are staged in
// the LDS, so every load of a basis element from L2 serves 16 rows; the next chunk's loads wait in registers while this
// one is summed.  Thread (n = t & 15, g = t >> 4) owns row n and the coefficients g, g + 16 (NR = 1 for R <= 16, 2 for
// R <= 32).  LDS row pitch 65 words of 16 bytes: the 16 rows of the tile, and the 4 basis rows a wave reads, fall on
// distinct banks.  Nothing outside the rows, T, the flags or the basis is read; tails are zeros in registers.
//
// k_sub_mix<C128>.  One workgroup takes one sample s and XM_SM_COLS = 8 columns (c, f) of it: it stages K_s (pitch R + 1)
// and the 8 x R inputs in the LDS, then thread (column t >> 5, r = t & 31) forms one output.  All inputs of a workgroup
// are read before the barrier and no other workgroup touches them, so z == a is allowed and gives the same bits.  The
// lanes run along (r, column), never along F alone.
//
// k_sub_expand.  One workgroup takes XM_SE_ROWS = 4 rows (v, f) and a tile of 256 time points, the lanes along t; U is
// wave-uniform, a load of V[r, t] serves the 4 rows.
#pragma once
#include "xm_common.h"

#define XM_SUB_NT 256
#define XM_SP_ROWS 16
#define XM_SP_TC 64
#define XM_SP_PITCH (XM_SP_TC + 1)
#define XM_SP_NY (XM_SP_ROWS * XM_SP_TC / XM_SUB_NT)  // samples a thread stages per chunk: 4
#define XM_SM_COLS 8
#define XM_SE_ROWS 4
// (XM_SUB_MAX_RANK = 32 is part of the ABI: include/xmris_hip.h)

struct SubProjectArgs {
  const void* y;             // [c][s][f][t], strides cs, ss, fs, 1 (elements)
  void* b;                   // [C, S, R, F] contiguous, y's dtype
  const double2* basis;      // V [R, T]
  const unsigned char* m;    // [S, T] or nullptr
  long long n_rows, cs, ss, fs;
  long long S, F;
  int C, T, R;
};

struct SubMixArgs {
  const void* a;         // [C, S, R, F]
  void* z;               // the same layout; may be a
  const double2* K;      // [S, R, R]
  long long S, F, n_cols;  // n_cols = C F
  unsigned tiles;        // column tiles per sample
  int R;
};

struct SubExpandArgs {
  const double2* U;      // [V, R, F]
  const double2* basis;  // [R, T]
  double2* x;            // [V, F, T]
  long long n_rows, F;   // n_rows = V F
  int T, R;
};

// acc += a b
XM_DEV void sub_cmac(double2& acc, const double2 a, const double2 b) {
  acc.x = fma(a.x, b.x, acc.x);
  acc.x = fma(-a.y, b.y, acc.x);
  acc.y = fma(a.x, b.y, acc.y);
  acc.y = fma(a.y, b.x, acc.y);
}

// acc += conj(a) b
XM_DEV void sub_cmac_conj(double2& acc, const double2 a, const double2 b) {
  acc.x = fma(a.x, b.x, acc.x);
  acc.x = fma(a.y, b.y, acc.x);
  acc.y = fma(a.x, b.y, acc.y);
  acc.y = fma(-a.y, b.x, acc.y);
}

template <bool C128>
XM_DEV double2 sub_load(const void* p, long long i) {
  if constexpr (C128) {
    return ((const double2*)p)[i];
  } else {
    const float2 v = ((const float2*)p)[i];
    return make_double2((double)v.x, (double)v.y);
  }
}

template <bool C128>
XM_DEV void sub_store(void* p, long long i, const double2 v) {
  if constexpr (C128)
    ((double2*)p)[i] = v;
  else
    ((float2*)p)[i] = make_float2((float)v.x, (float)v.y);
}

// the next chunk of a thread: its 4 samples (row srow of the tile, points stl + 16 j) and its 4 NR basis elements
template <bool C128, int NR>
XM_DEV void sp_fetch(const SubProjectArgs& A, int t0, bool live, long long ybase, long long mbase, int stl,
                     double2 (&yq)[XM_SP_NY], double2 (&bq)[4 * NR]) {
  const int T = A.T, R = A.R, t = threadIdx.x;
#pragma unroll
  for (int j = 0; j < XM_SP_NY; ++j) {
    const int tt = t0 + stl + 16 * j;
    double2 v = make_double2(0.0, 0.0);
    if (live && tt < T) {
      const double2 w = sub_load<C128>(A.y, ybase + tt);
      const bool on = !A.m || A.m[mbase + tt] != 0;
      v.x = on ? w.x : 0.0;  // selected, not multiplied
      v.y = on ? w.y : 0.0;
    }
    yq[j] = v;
  }
#pragma unroll
  for (int j = 0; j < 4 * NR; ++j) {  // element i = t + 256 j of the chunk [R][TC]: r = i >> 6, tl = i & 63
    const int i = t + XM_SUB_NT * j, r = i >> 6, tt = t0 + (i & (XM_SP_TC - 1));
    bq[j] = make_double2(0.0, 0.0);
    if (r < R && tt < T) bq[j] = A.basis[(long long)r * T + tt];
  }
}

template <int NR>
XM_DEV void sp_put(double2* Y, double2* B, int R, int srow, int stl, const double2 (&yq)[XM_SP_NY], const double2 (&bq)[4 * NR]) {
  const int t = threadIdx.x;
#pragma unroll
  for (int j = 0; j < XM_SP_NY; ++j) Y[srow * XM_SP_PITCH + stl + 16 * j] = yq[j];
#pragma unroll
  for (int j = 0; j < 4 * NR; ++j) {
    const int i = t + XM_SUB_NT * j, r = i >> 6;
    if (r < R) B[r * XM_SP_PITCH + (i & (XM_SP_TC - 1))] = bq[j];
  }
}

template <bool C128, int NR>
__global__ __launch_bounds__(XM_SUB_NT) void k_sub_project(SubProjectArgs A) {
  extern __shared__ double2 sp_sm[];
  double2* Y = sp_sm;                               // [16][pitch]
  double2* B = sp_sm + XM_SP_ROWS * XM_SP_PITCH;    // [R][pitch]
  const int t = threadIdx.x, T = A.T, R = A.R;
  const long long row0 = (long long)blockIdx.x * XM_SP_ROWS;
  const long long cf = (long long)A.C * A.F;

  // staging: row t >> 4 of the tile, points (t & 15) + 16 j of a chunk
  const int srow = t >> 4, stl = t & 15;
  const long long q = row0 + srow;
  const bool live = q < A.n_rows;
  long long ybase = 0, mbase = 0;
  if (live) {
    const long long s = q / cf, rem = q - s * cf, c = rem / A.F, f = rem - c * A.F;
    ybase = c * A.cs + s * A.ss + f * A.fs;
    mbase = s * (long long)T;
  }
  double2 yq[XM_SP_NY], bq[4 * NR];  // the next chunk: 4 samples, 4 or 8 basis elements (16 NR x TC / 256)

  const int n = t & 15, g = t >> 4;
  double2 acc[NR];
#pragma unroll
  for (int j = 0; j < NR; ++j) acc[j] = make_double2(0.0, 0.0);

  sp_fetch<C128, NR>(A, 0, live, ybase, mbase, stl, yq, bq);
#pragma unroll 1
  for (int t0 = 0; t0 < T; t0 += XM_SP_TC) {
    sp_put<NR>(Y, B, R, srow, stl, yq, bq);
    __syncthreads();
    if (t0 + XM_SP_TC < T) sp_fetch<C128, NR>(A, t0 + XM_SP_TC, live, ybase, mbase, stl, yq, bq);
    const int nt = T - t0 < XM_SP_TC ? T - t0 : XM_SP_TC;
    if (g < R) {
      const double2* yr = Y + n * XM_SP_PITCH;
#pragma unroll 4
      for (int tl = 0; tl < nt; ++tl) {
        const double2 yv = yr[tl];
#pragma unroll
        for (int j = 0; j < NR; ++j)
          if (j == 0 || g + 16 * j < R) sub_cmac_conj(acc[j], B[(g + 16 * j) * XM_SP_PITCH + tl], yv);
      }
    }
    __syncthreads();  // the chunk is read
  }

  const long long qo = row0 + n;
  if (qo < A.n_rows) {
    const long long s = qo / cf, rem = qo - s * cf, c = rem / A.F, f = rem - c * A.F;
#pragma unroll
    for (int j = 0; j < NR; ++j) {
      const int r = g + 16 * j;
      if (r < R) sub_store<C128>(A.b, ((c * A.S + s) * R + r) * A.F + f, acc[j]);
    }
  }
}

template <bool C128>
__global__ __launch_bounds__(XM_SUB_NT) void k_sub_mix(const SubMixArgs A) {
  extern __shared__ double2 sm_sm[];
  const int R = A.R, P = R + 1, t = threadIdx.x;
  double2* Ks = sm_sm;                // [R][R + 1]
  double2* In = sm_sm + R * P;        // [8][R]
  const long long s = blockIdx.x / A.tiles;
  const long long col = (long long)(blockIdx.x - s * A.tiles) * XM_SM_COLS + (t >> 5);
  const int r = t & 31;
  const bool live = col < A.n_cols && r < R;
  long long at = 0;
  if (live) {
    const long long c = col / A.F, f = col - c * A.F;
    at = ((c * A.S + s) * R + r) * A.F + f;
    In[(t >> 5) * R + r] = sub_load<C128>(A.a, at);
  }
  for (int i = t; i < R * R; i += XM_SUB_NT) {
    const int a = i / R;
    Ks[a * P + (i - a * R)] = A.K[s * R * R + i];
  }
  __syncthreads();
  if (!live) return;
  double2 acc = make_double2(0.0, 0.0);
  const double2* in = In + (t >> 5) * R;
  for (int k = 0; k < R; ++k) sub_cmac(acc, Ks[r * P + k], in[k]);
  sub_store<C128>(A.z, at, acc);
}

__global__ __launch_bounds__(XM_SUB_NT) void k_sub_expand(const SubExpandArgs A) {
  const int tt = blockIdx.y * XM_SUB_NT + threadIdx.x, T = A.T, R = A.R;
  const long long row0 = (long long)blockIdx.x * XM_SE_ROWS;
  if (tt >= T) return;
  const double2* u[XM_SE_ROWS];
  double2 acc[XM_SE_ROWS];
#pragma unroll
  for (int k = 0; k < XM_SE_ROWS; ++k) {
    const long long row = row0 + k < A.n_rows ? row0 + k : A.n_rows - 1;  // (a tail row repeats the last; not stored)
    const long long v = row / A.F, f = row - v * A.F;
    u[k] = A.U + v * R * A.F + f;
    acc[k] = make_double2(0.0, 0.0);
  }
  for (int r = 0; r < R; ++r) {
    const double2 b = A.basis[(long long)r * T + tt];
#pragma unroll
    for (int k = 0; k < XM_SE_ROWS; ++k) sub_cmac(acc[k], u[k][(long long)r * A.F], b);
  }
#pragma unroll
  for (int k = 0; k < XM_SE_ROWS; ++k)
    if (row0 + k < A.n_rows) A.x[(row0 + k) * T + tt] = acc[k];
}
