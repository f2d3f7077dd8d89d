// k_axis_dft: a small dense complex matrix applied along one axis of a C-contiguous tensor (xm_axis_dft in
// include/xmris_hip.h).  x is viewed as (n_outer, n, n_inner), y as (n_outer, m, n_inner):
//   y[o][p][i] = sum_j table[p][j] x[o][j][i],  ascending j, in fp64, rounded once to the data's dtype.
//
// Geometry.  A pencil is one (o, i); the pencils are numbered L = o n_inner + i, so 64 consecutive pencils are 64
// consecutive addresses wherever n_inner >= 64 and runs of n_inner otherwise (a grid that is the tensor's last axes
// still fills its lanes).  A workgroup of 4 waves takes a tile of 64 pencils: its waves stage the tile's n rows into the
// LDS together, in the data's own dtype (n x 64 elements, at most 64 KiB), every load one coalesced row of the tile.
// Wave w then forms the outputs p = w PT ... w PT + PT - 1 (PT = 4, 8 or 16: the smallest with 4 PT >= m) in 2 PT fp64
// accumulators per lane, walking j: x[j] comes from the LDS once per j (consecutive lanes, consecutive words: no bank
// conflict), table[p][j] is the same for the whole wave and is read through the scalar unit (the table pointer is
// const, restrict and never written, the index is made of wave-uniform values only), so the vector unit does nothing
// but the four FMAs of each complex product.  Every store is one coalesced row of the tile.
#pragma once
#include "xm_common.h"

#define XM_DFT_NT 256         // 4 waves
#define XM_DFT_TILE XM_WAVE   // pencils per workgroup: one per lane
#define XM_DFT_MAX 64         // largest n and m

struct AxisDftArgs {
  const void* x;
  void* y;
  const double* table;  // m x n complex128, row-major, interleaved
  long long n_pencils;  // n_outer n_inner
  long long n_inner;
  long long n_tiles;
  int n, m;
};

template <class S>
XM_DEV void dft_mac(double& ar, double& ai, double tr, double ti, Cx<S> v) {
  const double xr = (double)v.re, xi = (double)v.im;
  ar = __builtin_fma(tr, xr, ar);
  ar = __builtin_fma(-ti, xi, ar);
  ai = __builtin_fma(tr, xi, ai);
  ai = __builtin_fma(ti, xr, ai);
}

// S: float (complex64 data) or double (complex128 data)
template <class S, int PT>
__global__ __launch_bounds__(XM_DFT_NT) void k_axis_dft(const AxisDftArgs A) {
  extern __shared__ __align__(16) unsigned char dft_lds[];
  Cx<S>* xs = reinterpret_cast<Cx<S>*>(dft_lds);  // [n][64]
  const Cx<S>* __restrict__ x = static_cast<const Cx<S>*>(A.x);
  Cx<S>* __restrict__ y = static_cast<Cx<S>*>(A.y);
  const double* __restrict__ tab = A.table;
  const int lane = threadIdx.x & (XM_WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / XM_WAVE);
  const int n = A.n, m = A.m;
  const int p0 = wave * PT;
  // columns of the table taken per step of the j loop: PT JB table entries (4 scalar registers each) are live at once
  constexpr int XM_DFT_JB = PT == 4 ? 4 : PT == 8 ? 2 : 1;
  const int n_main = n - n % XM_DFT_JB;

  for (long long tile = blockIdx.x; tile < A.n_tiles; tile += gridDim.x) {
    const long long pencil = tile * XM_DFT_TILE + lane;
    const bool live = pencil < A.n_pencils;
    const long long o = live ? pencil / A.n_inner : 0;
    const long long i = live ? pencil - o * A.n_inner : 0;
    const Cx<S>* __restrict__ xp = x + o * n * A.n_inner + i;  // row j of the pencil: xp[j n_inner]
    for (int j = wave; j < n; j += XM_DFT_NT / XM_WAVE)
      xs[j * XM_DFT_TILE + lane] = live ? xp[(long long)j * A.n_inner] : mk<S>(S(0), S(0));
    __syncthreads();

    if (p0 < m) {  // (wave-uniform)
      double ar[PT], ai[PT];
#pragma unroll
      for (int q = 0; q < PT; ++q) ar[q] = ai[q] = 0.0;
      // rows past m (the last wave with rows) repeat row m - 1 and are not stored: the loop body has no branch, so
      // the table entries of a step are fetched together and the FMAs follow in one run
      long long row[PT];
#pragma unroll
      for (int q = 0; q < PT; ++q) row[q] = 2LL * n * (p0 + q < m ? p0 + q : m - 1);
      for (int j0 = 0; j0 < n_main; j0 += XM_DFT_JB) {
        Cx<S> v[XM_DFT_JB];
#pragma unroll
        for (int jj = 0; jj < XM_DFT_JB; ++jj) v[jj] = xs[(j0 + jj) * XM_DFT_TILE + lane];
#pragma unroll
        for (int q = 0; q < PT; ++q) {
          const double* __restrict__ t = tab + row[q] + 2 * j0;
#pragma unroll
          for (int jj = 0; jj < XM_DFT_JB; ++jj) dft_mac(ar[q], ai[q], t[2 * jj], t[2 * jj + 1], v[jj]);
        }
      }
      for (int j = n_main; j < n; ++j) {
        const Cx<S> v = xs[j * XM_DFT_TILE + lane];
#pragma unroll
        for (int q = 0; q < PT; ++q) {
          const double* __restrict__ t = tab + row[q] + 2 * j;
          dft_mac(ar[q], ai[q], t[0], t[1], v);
        }
      }
      if (live) {
        Cx<S>* __restrict__ yp = y + o * m * A.n_inner + i;
#pragma unroll
        for (int q = 0; q < PT; ++q)
          if (p0 + q < m) yp[(long long)(p0 + q) * A.n_inner] = mk<S>((S)ar[q], (S)ai[q]);
      }
    }
    __syncthreads();  // the next tile overwrites the staged rows
  }
}
