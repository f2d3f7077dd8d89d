// k_axis_sparse: a sparse real matrix in CSR form applied along one axis of a C-contiguous complex tensor
// (xm_axis_sparse in include/xmris_hip.h).  x is viewed as (n_outer, n, n_inner), y as
// (n_outer, n_rows, n_inner):
//   y[o][r][i] = sum_{e = rowptr[r]}^{rowptr[r+1]-1} val[e] x[o][col[e]][i],  ascending e, in fp64, rounded once.
// The kernel knows nothing about gridding: gridding and degridding are this kernel with two host tables.
//
// Geometry.  Output-driven (a gather): one wave forms one output row r of one (o, inner tile), so nothing is added
// across waves, there is no atomic, every sum has one fixed order and an output depends on its own entries only.  The
// lanes run along the inner axis, one 16-byte word each (two complex64 or one complex128; VEC = 1 is the 8-byte
// complex64 form for an odd n_inner or a base that is not 16-byte aligned): every load and store of a wave is one
// contiguous run of the tensor.  The row r is the same for the whole wave, so rowptr, col and val are read through the
// scalar unit (the pointers are const, restrict and never written, the indices are made of wave-uniform values only);
// the vector unit issues the loads and the two FMAs per complex element (val is real).  Four entries are taken per step:
// four independent loads are in flight before the first FMA, the FMAs then follow in entry order.
//
// Order of the work items.  A slice is one (o, inner tile): its S input rows are what every output row of the slice
// gathers from, each of them W^d times.  A workgroup of 4 waves takes 4 neighbouring rows of one slice.  Workgroups are
// dispatched in ascending blockIdx.x and those whose index agrees mod 8 share an XCD (and its L2), so blockIdx.x =
// 8 (row group) + (slice mod 8) and blockIdx.y = slice / 8: at any moment an XCD works on one slice or two and, of each,
// on a run of neighbouring rows, whose samples overlap.  This is a placement for speed only: any other placement
// computes the same bits.  There is no loop over work items: the hardware hands the next workgroup to whichever CU is
// free, which is what hides a long row among many short ones, and no store precedes a load, so the compiler may keep
// the table reads on the scalar unit.
#pragma once
#include "xm_common.h"

#define XM_SPARSE_NT 256     // 4 waves, one output row each
#define XM_SPARSE_ROWS (XM_SPARSE_NT / XM_WAVE)
#define XM_SPARSE_XCDS 8     // workgroups with the same index mod 8 share an L2
#define XM_SPARSE_UNROLL 4   // entries per step of the row loop

struct AxisSparseArgs {
  long long n;          // input rows per o
  long long n_rows;     // output rows per o
  long long n_inner;
  unsigned n_itiles;    // inner tiles of 64 VEC elements
  unsigned n_slices;    // n_outer n_itiles
  unsigned groups_x;    // row groups along blockIdx.x (gridDim.x / 8); blockIdx.z counts the runs of groups_x
  unsigned round0;      // blockIdx.y + round0 = slice / 8
};

// S: float (complex64 data) or double (complex128 data); VEC: complex elements per lane (2 only with S = float).
// rowptr: n_rows + 1; col: rowptr[n_rows] entries, each in [0, n); val: as col.
template <class S, int VEC>
__global__ __launch_bounds__(XM_SPARSE_NT) void k_axis_sparse(const void* __restrict__ xv, void* __restrict__ yv,
                                                              const int* __restrict__ rowptr,
                                                              const int* __restrict__ col,
                                                              const double* __restrict__ val, const AxisSparseArgs A) {
  struct alignas(VEC * sizeof(Cx<S>)) Word {
    Cx<S> v[VEC];
  };
  const Cx<S>* __restrict__ x = static_cast<const Cx<S>*>(xv);
  Cx<S>* __restrict__ y = static_cast<Cx<S>*>(yv);
  const int lane = threadIdx.x & (XM_WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / XM_WAVE);

  // (everything but `lane` is wave-uniform)
  const unsigned slice = (blockIdx.y + A.round0) * XM_SPARSE_XCDS + (blockIdx.x & (XM_SPARSE_XCDS - 1));
  const long long r = ((long long)blockIdx.z * A.groups_x + (blockIdx.x / XM_SPARSE_XCDS)) * XM_SPARSE_ROWS + wave;
  if (slice >= A.n_slices || r >= A.n_rows) return;
  const unsigned o = slice / A.n_itiles;
  const long long i = (long long)(slice - o * A.n_itiles) * (XM_WAVE * VEC) + (long long)lane * VEC;
  const bool live = i < A.n_inner;  // VEC = 2 only with an even n_inner: both elements of a word or neither
  // a lane past the end reads the row's first word (in bounds) and stores nothing: the loads need no branch
  const Cx<S>* __restrict__ xp = x + (long long)o * A.n * A.n_inner + (live ? i : 0);

  double ar[VEC], ai[VEC];
#pragma unroll
  for (int k = 0; k < VEC; ++k) ar[k] = ai[k] = 0.0;
  const int e1 = rowptr[r + 1];
  int e = rowptr[r];
  for (; e + XM_SPARSE_UNROLL <= e1; e += XM_SPARSE_UNROLL) {
    Word w[XM_SPARSE_UNROLL];
    double v[XM_SPARSE_UNROLL];
#pragma unroll
    for (int q = 0; q < XM_SPARSE_UNROLL; ++q) {
      v[q] = val[e + q];
      w[q] = *reinterpret_cast<const Word*>(xp + (long long)col[e + q] * A.n_inner);
    }
#pragma unroll
    for (int q = 0; q < XM_SPARSE_UNROLL; ++q)
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        ar[k] = __builtin_fma(v[q], (double)w[q].v[k].re, ar[k]);
        ai[k] = __builtin_fma(v[q], (double)w[q].v[k].im, ai[k]);
      }
  }
  for (; e < e1; ++e) {
    const double v = val[e];
    const Word w = *reinterpret_cast<const Word*>(xp + (long long)col[e] * A.n_inner);
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      ar[k] = __builtin_fma(v, (double)w.v[k].re, ar[k]);
      ai[k] = __builtin_fma(v, (double)w.v[k].im, ai[k]);
    }
  }
  if (live) {  // an empty row stores zeros
    Word out;
#pragma unroll
    for (int k = 0; k < VEC; ++k) out.v[k] = mk<S>((S)ar[k], (S)ai[k]);
    *reinterpret_cast<Word*>(y + ((long long)o * A.n_rows + r) * A.n_inner + i) = out;
  }
}
