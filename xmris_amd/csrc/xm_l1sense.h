// k_l1_start, k_l1_prox: the image-sized half of one proximal-gradient (FISTA) step of wavelet-sparse SENSE (xm_l1_* in
// include/xmris_hip.h).  The coil-sized half is k_cgs_expand, the two NUFFT chains and k_cgs_reduce,
// unchanged: they leave q = (E^H D E + lambda2) v.
//
// Arrays.  x, v, q, b: [V, T] complex128, V = m_0 m_1 m_2 voxels in C order and T columns, T contiguous.  mask: [V] bytes.
// A sum over voxels is kept as partials [NBL, T] fp64, one per Haar block and column, and whoever needs the sum adds a
// column's NBL partials in ascending block order: all blocks of a column take the same decision without a word passing
// between them.  No launch reads a per-column value that it writes: the partials and the status word are double-buffered
// by the parity of the step (the host hands the two buffers over).
//
// Geometry.  A work item is one Haar block -- B = 2^(l_0 + l_1 + l_2) <= 16 voxels, gathered through the spatial strides
// and the cycle-spin shift with periodic wrap -- x one tile of 64 columns, and one wave takes it; lanes run along the
// columns, one 16-byte complex128 word each.  The block and its voxel addresses are wave-uniform (scalar unit).  The B
// values of a lane stay in registers: register r holds the voxel whose index inside the block is i_0 + (i_1 << l_0) +
// (i_2 << (l_0 + l_1)), so the butterfly of dim d, level j pairs the registers that differ in bit p = (offset of d) + j,
// among those whose lower bits of the same field are 0 (the approximations of the finer levels).  Bits ascending is dims
// ascending, levels fine to coarse.  Which registers take part is decided by four wave-uniform masks (L1Args::low), so one
// instantiation per B serves every split of its bits among the dims.  The approximation ends in register 0.  No LDS, no
// atomics, no cross-lane step.
#pragma once
#include "xm_common.h"

#define XM_L1_NT 256  // 4 waves, one work item each
#define XM_L1_ITEMS (XM_L1_NT / XM_WAVE)
#define XM_L1_MAX_BLOCK 16
#define XM_L1_DBL_MAX 1.79769313486231570815e308

struct L1Args {
  long long n_cols;     // T
  long long n_vox;      // V
  long long stride[3];  // voxels per step along a dim
  int m[3], l[3], s[3], nblk[3];  // matrix, levels, shift, blocks per dim
  unsigned low[4];      // per bit p of the register index: the bits of its own field below p
  unsigned n_blocks;    // NBL (start: voxel runs of XM_L1_MAX_BLOCK)
  unsigned tile0;       // blockIdx.y + tile0 = column tile
  int mode;             // prox: 0 step, 1 first step, 2 final test; start: 0 block maxima, 1 finish
  int iteration;        // n_iter of a column that is updated in this launch
  double tau, theta_scale, beta, tol2;
};

// the sum of a column's partials, ascending block
XM_DEV double l1_total(const double* __restrict__ part, unsigned n_blocks, long long n_cols, long long t) {
  double a = 0.0;
  for (unsigned b = 0; b < n_blocks; ++b) a += part[(long long)b * n_cols + t];
  return a;
}

// (everything but `lane` is wave-uniform)
#define XM_L1_ITEM                                                                      \
  const int lane = threadIdx.x & (XM_WAVE - 1);                                         \
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / XM_WAVE);               \
  const long long vb = (long long)blockIdx.x * XM_L1_ITEMS + wave;                      \
  if (vb >= (long long)A.n_blocks) return;                                              \
  const long long t = ((long long)blockIdx.y + A.tile0) * XM_WAVE + (long long)lane;    \
  if (t >= A.n_cols) return;

// Mode 0: bpart[vb, t] = max |b[v, t]|^2 over the voxels of run vb (XM_L1_MAX_BLOCK consecutive voxels; a maximum has no
// order, so the runs need not be the Haar blocks); a NaN stays.  Mode 1, one lane per column (n_blocks = 1 in the grid,
// `runs` the number of partials): bmax[t] = sqrt(max over the runs), status[t] = 0, or 3 with change[t] = NaN and
// x[:, t] = NaN when that is not finite.
__global__ __launch_bounds__(XM_L1_NT) void k_l1_start(const Cx<double>* __restrict__ b, double* __restrict__ bpart,
                                                       double* __restrict__ bmax, int* __restrict__ status,
                                                       double* __restrict__ change, Cx<double>* __restrict__ x,
                                                       unsigned runs, const L1Args A) {
  XM_L1_ITEM
  double top = 0.0;
  if (A.mode == 0) {
    const long long v0 = vb * XM_L1_MAX_BLOCK;
    const long long v1 = v0 + XM_L1_MAX_BLOCK < A.n_vox ? v0 + XM_L1_MAX_BLOCK : A.n_vox;
    for (long long v = v0; v < v1; ++v) {
      const Cx<double> bv = b[v * A.n_cols + t];
      const double a = __builtin_fma(bv.re, bv.re, bv.im * bv.im);
      top = (a > top || a != a) ? a : top;
    }
    bpart[vb * A.n_cols + t] = top;
    return;
  }
  for (unsigned r = 0; r < runs; ++r) {
    const double a = bpart[(long long)r * A.n_cols + t];
    top = (a > top || a != a) ? a : top;
  }
  const bool ok = top <= XM_L1_DBL_MAX;
  const double nan = __builtin_nan("");
  bmax[t] = ok ? __builtin_sqrt(top) : nan;
  status[t] = ok ? 0 : 3;
  if (ok) return;
  change[t] = nan;
  for (long long v = 0; v < A.n_vox; ++v) x[v * A.n_cols + t] = mk<double>(nan, nan);
}

// the voxel of register r of the block whose first voxel (shift included) is `base`
XM_DEV long long l1_voxel(const L1Args& A, const int (&base)[3], int r) {
  long long at = 0;
  int off = 0;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    int c = base[d] + ((r >> off) & ((1 << A.l[d]) - 1));
    off += A.l[d];
    c = c >= A.m[d] ? c - A.m[d] : c;
    at += (long long)c * A.stride[d];
  }
  return at;
}

// One step for the columns whose status_in is 0.
//   the test (not in mode 1) on the totals d2, n2 of d2_in, n2_in: either not finite -> status 3, x[:, t] = NaN;
//   d2 <= tol2 n2 -> status 1; mode 2 -> stays 0.  Block 0 alone writes status_out (for every column), and change =
//   sqrt(d2 / n2) (0 for d2 = 0, NaN with status 3) for a column that freezes here or, in mode 2, one still running.
//   otherwise  w = v - tau (q - b)  (mode 1: q is taken as 0 and not read),  c = Haar(w),  c_r <- c_r max(0, 1 - theta /
//   |c_r|) for r != 0 (every r when B = 1), theta = theta_scale bmax[t],  x' = mask ? Haar^-1(c) : 0,
//   v <- x' + beta (x' - x),  x <- x',  d2_out[vb, t] = sum |x' - x|^2,  n2_out[vb, t] = sum |x'|^2 (ascending r),
//   n_iter[t] = iteration.
// A column whose status_in is not 0 is not touched.
template <int B>
__global__ __launch_bounds__(XM_L1_NT) void k_l1_prox(Cx<double>* __restrict__ x, Cx<double>* __restrict__ v,
                                                      const Cx<double>* __restrict__ q, const Cx<double>* __restrict__ b,
                                                      const unsigned char* __restrict__ mask,
                                                      const double* __restrict__ bmax, const double* __restrict__ d2_in,
                                                      const double* __restrict__ n2_in, double* __restrict__ d2_out,
                                                      double* __restrict__ n2_out, const int* __restrict__ status_in,
                                                      int* __restrict__ status_out, int* __restrict__ n_iter,
                                                      double* __restrict__ change, const L1Args A) {
  constexpr int BITS = B == 16 ? 4 : B == 8 ? 3 : B == 4 ? 2 : B == 2 ? 1 : 0;
  constexpr double R = 0.70710678118654752440;
  XM_L1_ITEM
  const int before = status_in[t];
  int after = before;
  bool run = false;
  if (before == 0) {
    if (A.mode == 1) {
      run = true;
    } else {
      const double d2 = l1_total(d2_in, A.n_blocks, A.n_cols, t);
      const double n2 = l1_total(n2_in, A.n_blocks, A.n_cols, t);
      if (!(d2 <= XM_L1_DBL_MAX && n2 <= XM_L1_DBL_MAX))
        after = 3;
      else if (d2 <= A.tol2 * n2)
        after = 1;
      else
        run = A.mode == 0;
      if (vb == 0 && (after != 0 || A.mode == 2))
        change[t] = after == 3 ? __builtin_nan("") : d2 == 0.0 ? 0.0 : __builtin_sqrt(d2 / n2);
    }
    if (vb == 0 && run) n_iter[t] = A.iteration;
  }
  if (vb == 0) status_out[t] = after;
  if (!run && !(after == 3 && before == 0)) return;

  unsigned rem = (unsigned)vb;
  int base[3];
  base[2] = (int)((rem % (unsigned)A.nblk[2]) << A.l[2]) + A.s[2];
  rem /= (unsigned)A.nblk[2];
  base[1] = (int)((rem % (unsigned)A.nblk[1]) << A.l[1]) + A.s[1];
  base[0] = (int)((rem / (unsigned)A.nblk[1]) << A.l[0]) + A.s[0];

  if (!run) {
    const double nan = __builtin_nan("");
#pragma unroll
    for (int r = 0; r < B; ++r) x[l1_voxel(A, base, r) * A.n_cols + t] = mk<double>(nan, nan);
    return;
  }

  const double theta = A.theta_scale * bmax[t];
  Cx<double> w[B];
#pragma unroll
  for (int r = 0; r < B; ++r) {
    const long long at = l1_voxel(A, base, r) * A.n_cols + t;
    const Cx<double> vv = v[at], bv = b[at];
    const Cx<double> qv = A.mode == 1 ? mk<double>(0.0, 0.0) : q[at];
    w[r] = mk<double>(__builtin_fma(-A.tau, qv.re - bv.re, vv.re), __builtin_fma(-A.tau, qv.im - bv.im, vv.im));
  }
#pragma unroll
  for (int p = 0; p < BITS; ++p) {
    const unsigned low = A.low[p];
#pragma unroll
    for (int r = 0; r < B; ++r) {
      if ((r >> p) & 1) continue;
      if ((r & low) != 0) continue;
      const Cx<double> a = w[r], c = w[r | (1 << p)];
      w[r] = mk<double>((a.re + c.re) * R, (a.im + c.im) * R);
      w[r | (1 << p)] = mk<double>((a.re - c.re) * R, (a.im - c.im) * R);
    }
  }
#pragma unroll
  for (int r = (B == 1 ? 0 : 1); r < B; ++r) {
    const double mag = __builtin_sqrt(__builtin_fma(w[r].re, w[r].re, w[r].im * w[r].im));
    const double f = mag <= theta ? 0.0 : 1.0 - theta / mag;  // (a NaN stays a NaN)
    w[r] = mk<double>(w[r].re * f, w[r].im * f);
  }
#pragma unroll
  for (int p = BITS - 1; p >= 0; --p) {
    const unsigned low = A.low[p];
#pragma unroll
    for (int r = 0; r < B; ++r) {
      if ((r >> p) & 1) continue;
      if ((r & low) != 0) continue;
      const Cx<double> a = w[r], c = w[r | (1 << p)];
      w[r] = mk<double>((a.re + c.re) * R, (a.im + c.im) * R);
      w[r | (1 << p)] = mk<double>((a.re - c.re) * R, (a.im - c.im) * R);
    }
  }
  double d2 = 0.0, n2 = 0.0;
#pragma unroll
  for (int r = 0; r < B; ++r) {
    const long long vx = l1_voxel(A, base, r);
    const long long at = vx * A.n_cols + t;
    const Cx<double> xo = x[at];
    const Cx<double> xn = mask[vx] ? w[r] : mk<double>(0.0, 0.0);
    const Cx<double> dx = xn - xo;
    x[at] = xn;
    v[at] = mk<double>(__builtin_fma(A.beta, dx.re, xn.re), __builtin_fma(A.beta, dx.im, xn.im));
    d2 = __builtin_fma(dx.re, dx.re, d2);
    d2 = __builtin_fma(dx.im, dx.im, d2);
    n2 = __builtin_fma(xn.re, xn.re, n2);
    n2 = __builtin_fma(xn.im, xn.im, n2);
  }
  d2_out[vb * A.n_cols + t] = d2;
  n2_out[vb * A.n_cols + t] = n2;
}
