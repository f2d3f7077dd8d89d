// GRAPPA fill kernel (the project's own definition, the reference has no such function).
// Included by xm_grappa.hip alone; nothing but xm_common.h is shared with the other kernels.
//
// Per dim a: n_a kept lines at acceleration R_a, N_a = R_a n_a; the kept lines of the full centred k-space are
// j = j0_a + R_a l, j0_a = N_a / 2 - R_a (n_a / 2).  A full-grid index j has l = floor((j - j0) / R) (-1 below j0) and
// o = (j - j0) mod R >= 0.  o = 0 in every dim: the position is acquired and copied bit for bit.  Any other offset tuple
// is a type tau = ((o_1 R_2 + o_2) R_3 + o_3) - 1, and
//   y[c, j, t] = sum_s sum_c' W[tau][c][s][c'] a[c', l + s, t],   s_a = -((b_a - 1) / 2) ... b_a / 2,
// s row-major over (s_1, s_2, s_3), ascending s then ascending c'; a neighbour outside 0 ... n_a - 1 is skipped.
//
// k_grappa_fill: a plain grid, one 256-thread workgroup per (outer, position, block of CB output coils, time tile); no
// LDS, no barrier, no atomics, nothing shared between workgroups.  Lanes run along time (TP = 2 points per lane for
// complex64 when every row starts on a 16-byte boundary and N_t is even, so that a lane moves 16 bytes per load and
// store as in complex128).  A lane keeps the CB x TP outputs as fp64 accumulators in registers, walks the sources in the
// defined order and loads each source sample once (coalesced along time, eight samples in flight).  The weights have
// the same address in every lane, and every load of the kernel comes before its first store, so the compiler reads them
// through the scalar cache: for one output coil the weights of a chunk of source coils are consecutive in memory and
// arrive in wide scalar loads.  Every step is a fused multiply-add; the sum of one output is the same sequence (ascending
// s, then ascending c') whatever CB, TP or the layout, so results are bitwise independent of the form and of the batch.
#pragma once
#include "xm_common.h"

#define XM_GR_MAXC 64
#define XM_GR_MAXR 16
#define XM_GR_MAXS 64
#define XM_GR_MAXK 1024  // C S
#define XM_GR_NT 256     // threads of a workgroup
#define XM_GR_CB 16      // output coils per workgroup at most
#define XM_GR_LD 8       // source samples in flight per lane

struct GrappaArgs {
  const void* a;     // kept lines: outer, coil, three spatial axes by strides, time contiguous
  void* y;           // full grid: the same axes, N_a = R_a n_a lines per dim; the dtype of a
  const double* w;   // [R - 1][C][S][C] complex128, or nullptr at R = 1
  long long as[5], ys[5];
  long long npos;    // N_1 N_2 N_3
  long long nitems;  // n_outer npos ncb ntiles
  int C, n[3], R[3], b[3], Nt, S;
  int ncb, ntiles;   // coil blocks, time tiles
  unsigned gx;       // gridDim.x: item = blockIdx.x + gx blockIdx.y
};

// floor((j - j0) / R) and the non-negative remainder
XM_DEV void gr_split(int j, int j0, int R, int& l, int& o) {
  const int d = j - j0;
  l = d >= 0 ? d / R : -((-d + R - 1) / R);
  o = d - l * R;
}

// NK source coils, from coil d0 on, of one neighbour into the CB outputs: the lane's NK samples (rows `src` + coil x
// `acs` of a), then per output coil 2 NK consecutive doubles of W (row m of `wk`, rows `wstep` apart) and its 4 NK TP
// fused multiply-adds in ascending source coil.  A block with fewer than CB coils repeats its last row: straight-line
// code, and the extra accumulators are never stored.
template <class T, int CB, int TP, int NK>
XM_DEV void gr_chunk(const T* a, long long src, long long acs, bool in, const double* wk, long long wstep, int mcount,
                     double (&yr)[CB][TP], double (&yi)[CB][TP]) {
  typedef T gr_v __attribute__((ext_vector_type(2 * TP)));
  double xr[NK][TP], xi[NK][TP];
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    const gr_v x = in ? *(const gr_v*)(a + 2 * (src + k * acs)) : (gr_v)(T)0;
#pragma unroll
    for (int h = 0; h < TP; ++h) {
      xr[k][h] = (double)x[2 * h];
      xi[k][h] = (double)x[2 * h + 1];
    }
  }
#pragma unroll
  for (int m = 0; m < CB; ++m) {
    const double* wm = wk + (m < mcount ? m : mcount - 1) * wstep;
    double u[2 * NK];
#pragma unroll
    for (int e = 0; e < 2 * NK; ++e) u[e] = wm[e];
#pragma unroll
    for (int k = 0; k < NK; ++k)
#pragma unroll
      for (int h = 0; h < TP; ++h) {
        yr[m][h] = fma(u[2 * k], xr[k][h], yr[m][h]);
        yr[m][h] = fma(-u[2 * k + 1], xi[k][h], yr[m][h]);
        yi[m][h] = fma(u[2 * k], xi[k][h], yi[m][h]);
        yi[m][h] = fma(u[2 * k + 1], xr[k][h], yi[m][h]);
      }
  }
}

template <class T, int CB, int TP>
__global__ __launch_bounds__(XM_GR_NT) void k_grappa_fill(GrappaArgs A) {
  typedef T gr_v __attribute__((ext_vector_type(2 * TP)));
  constexpr int LD = XM_GR_LD / TP;  // source coils per chunk: 8 samples in flight per lane
  long long v = (long long)blockIdx.x + (long long)A.gx * blockIdx.y;
  if (v >= A.nitems) return;
  const int tile = (int)(v % A.ntiles);
  v /= A.ntiles;
  const int c0 = (int)(v % A.ncb) * CB;
  v /= A.ncb;
  const long long pos = v % A.npos, outer = v / A.npos;
  const int C = A.C;
  const int N2 = A.R[1] * A.n[1], N3 = A.R[2] * A.n[2];
  const int j3 = (int)(pos % N3), j2 = (int)((pos / N3) % N2), j1 = (int)(pos / ((long long)N3 * N2));
  int l1, l2, l3, o1, o2, o3;
  gr_split(j1, A.R[0] * A.n[0] / 2 - A.R[0] * (A.n[0] / 2), A.R[0], l1, o1);
  gr_split(j2, N2 / 2 - A.R[1] * (A.n[1] / 2), A.R[1], l2, o2);
  gr_split(j3, N3 / 2 - A.R[2] * (A.n[2] / 2), A.R[2], l3, o3);
  const int type = (o1 * A.R[1] + o2) * A.R[2] + o3;

  const int i = tile * (XM_GR_NT * TP) + TP * (int)threadIdx.x;
  const bool in = i < A.Nt;  // (pairs: N_t is even, so both points are inside or both outside)
  const T* a = (const T*)A.a;
  T* y = (T*)A.y;
  const long long ybase = outer * A.ys[0] + j1 * A.ys[2] + j2 * A.ys[3] + j3 * A.ys[4] + i;
  const long long abase = outer * A.as[0] + i;

  if (type == 0) {  // acquired: the samples as they are
    if (!in) return;
    const long long src = abase + l1 * A.as[2] + l2 * A.as[3] + l3 * A.as[4];
#pragma unroll
    for (int m = 0; m < CB; ++m)
      if (c0 + m < C) *(gr_v*)(y + 2 * (ybase + (c0 + m) * A.ys[1])) = *(const gr_v*)(a + 2 * (src + (c0 + m) * A.as[1]));
    return;
  }

  double yr[CB][TP], yi[CB][TP];
#pragma unroll
  for (int m = 0; m < CB; ++m)
#pragma unroll
    for (int h = 0; h < TP; ++h) yr[m][h] = yi[m][h] = 0.0;
  // W[type - 1][c0 + m][s][c']: for one output coil and one s the weights of consecutive source coils are consecutive
  // in memory, so the LD weights of a chunk of source coils arrive in one or two wide scalar loads per output coil
  const long long wstep = 2LL * A.S * C;  // doubles from one output coil to the next
  const double* wrow = A.w + ((long long)(type - 1) * C + c0) * wstep;
  const int mcount = C - c0 < CB ? C - c0 : CB;  // output coils of this block
  const int h1 = (A.b[0] - 1) / 2, h2 = (A.b[1] - 1) / 2, h3 = (A.b[2] - 1) / 2;
  for (int s1 = 0; s1 < A.b[0]; ++s1) {
    const int q1 = l1 + s1 - h1;
    if (q1 < 0 || q1 >= A.n[0]) continue;
    for (int s2 = 0; s2 < A.b[1]; ++s2) {
      const int q2 = l2 + s2 - h2;
      if (q2 < 0 || q2 >= A.n[1]) continue;
      for (int s3 = 0; s3 < A.b[2]; ++s3) {
        const int q3 = l3 + s3 - h3;
        if (q3 < 0 || q3 >= A.n[2]) continue;
        const int s = (s1 * A.b[1] + s2) * A.b[2] + s3;
        const long long src = abase + q1 * A.as[2] + q2 * A.as[3] + q3 * A.as[4];
        const double* ws = wrow + 2LL * s * C;
        int d0 = 0;
        for (; d0 + LD <= C; d0 += LD)
          gr_chunk<T, CB, TP, LD>(a, src + d0 * A.as[1], A.as[1], in, ws + 2 * d0, wstep, mcount, yr, yi);
        // a coil count that is no multiple of LD: the rest in chunks of LD / 2, ... 1, so no weight past the row is read
        if constexpr (LD > 4)
          if ((C - d0) & 4) {
            gr_chunk<T, CB, TP, 4>(a, src + d0 * A.as[1], A.as[1], in, ws + 2 * d0, wstep, mcount, yr, yi);
            d0 += 4;
          }
        if ((C - d0) & 2) {
          gr_chunk<T, CB, TP, 2>(a, src + d0 * A.as[1], A.as[1], in, ws + 2 * d0, wstep, mcount, yr, yi);
          d0 += 2;
        }
        if ((C - d0) & 1) gr_chunk<T, CB, TP, 1>(a, src + d0 * A.as[1], A.as[1], in, ws + 2 * d0, wstep, mcount, yr, yi);
      }
    }
  }
  if (!in) return;
#pragma unroll
  for (int m = 0; m < CB; ++m)
    if (c0 + m < C) {
      gr_v o;
#pragma unroll
      for (int h = 0; h < TP; ++h) {
        o[2 * h] = (T)yr[m][h];
        o[2 * h + 1] = (T)yi[m][h];
      }
      *(gr_v*)(y + 2 * (ybase + (c0 + m) * A.ys[1])) = o;
    }
}
