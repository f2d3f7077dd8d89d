// k_cgs_expand, k_cgs_reduce, k_cgs_step: the image-sized half of one conjugate-gradient step of CG-SENSE
// (xm_cgs_* in include/xmris_hip.h).  The coil-sized half -- the two NUFFT chains -- is the
// existing k_axis_dft / k_axis_sparse launches, unchanged.
//
// Arrays.  x, r, p, q: [V, T] complex128, V voxels and T columns (time points, repetitions ...), T contiguous.
// s: [C, V] complex128.  u: [C, V, T] in the data's dtype: the coil images that go into, or come out of, a chain.
// Per-column scalars are never stored as such: a kernel that forms a sum over voxels writes one partial per (voxel block,
// column), [NB, T] fp64 with NB = ceil(V / XM_CGS_VOXELS), and a kernel that needs the sum adds the NB partials of its
// column in ascending block order.  Every work item that does so gets the same bits, so all blocks of a column take the
// same decision without a word passing between them, and no launch reads what the same launch writes: the partials of
// rho and the status word are double-buffered by the parity of the iteration (the host hands the two buffers over).
//
// Geometry.  A work item is one voxel block of XM_CGS_VOXELS voxels x one tile of 64 VEC columns, and one wave takes it.
// The lanes run along the column axis, one 16-byte word of coil data each (two complex64 or one complex128; VEC = 1 with
// S = float is the 8-byte form for an odd T or a base that is not 16-byte aligned: the same arithmetic per element, so
// the same bits).  A lane owns its columns: it walks the voxels of the block in ascending v, so the block's partial is
// a sequential sum in one thread, and the sum over coils is ascending c.  No cross-lane step, no LDS, no atomics.  The
// voxel and the coil are wave-uniform, so s is read through the scalar unit.  Every product-sum is a spelt-out fp64 FMA.
#pragma once
#include "xm_common.h"

#define XM_CGS_NT 256  // 4 waves, one work item each
#define XM_CGS_ITEMS (XM_CGS_NT / XM_WAVE)
// (XM_CGS_VOXELS, the voxel block, is part of the ABI: include/xmris_hip.h)

struct CgsArgs {
  long long n_vox;    // V
  long long n_cols;   // T
  int n_coils;        // C
  unsigned n_blocks;  // NB
  unsigned tile0;     // blockIdx.y + tile0 = column tile
  int mode;           // expand: first step (copy r); reduce: initial (form b); step: final test only
  int iteration;      // step: n_iter of a column that is updated in this launch
  double lambda;      // reduce
  double tol2;        // step: max(tol, 1e-14)^2
};

// the sum of a column's NB partials, ascending block
XM_DEV double cgs_total(const double* __restrict__ part, unsigned n_blocks, long long n_cols, long long t) {
  double a = 0.0;
  for (unsigned b = 0; b < n_blocks; ++b) a += part[(long long)b * n_cols + t];
  return a;
}

// (everything but `lane` is wave-uniform)
#define XM_CGS_ITEM(VEC)                                                                                        \
  const int lane = threadIdx.x & (XM_WAVE - 1);                                                                 \
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / XM_WAVE);                                       \
  const long long vb = (long long)blockIdx.x * XM_CGS_ITEMS + wave;                                             \
  if (vb >= (long long)A.n_blocks) return;                                                                      \
  const long long t0 = ((long long)blockIdx.y + A.tile0) * (XM_WAVE * (VEC)) + (long long)lane * (VEC);         \
  if (t0 >= A.n_cols) return; /* VEC = 2 only with an even T: both columns of a word or neither */              \
  const long long v0 = vb * XM_CGS_VOXELS;                                                                      \
  const long long v1 = v0 + XM_CGS_VOXELS < A.n_vox ? v0 + XM_CGS_VOXELS : A.n_vox;

// p <- r + (rho_new / rho_old) p for the columns whose status is 0 (first step: p <- r), then u[c, v, t] = round(s[c, v]
// p[v, t]) for all c.  rho_new / rho_old: the partials of this step's and the previous step's rho.
template <class S, int VEC>
__global__ __launch_bounds__(XM_CGS_NT) void k_cgs_expand(const Cx<double>* __restrict__ r, Cx<double>* __restrict__ p,
                                                          const Cx<double>* __restrict__ s, void* __restrict__ uv,
                                                          const double* __restrict__ rho_new,
                                                          const double* __restrict__ rho_old,
                                                          const int* __restrict__ status, const CgsArgs A) {
  struct alignas(VEC * sizeof(Cx<S>)) Word {
    Cx<S> v[VEC];
  };
  Cx<S>* __restrict__ u = static_cast<Cx<S>*>(uv);
  XM_CGS_ITEM(VEC)
  bool live[VEC];
  double beta[VEC];
#pragma unroll
  for (int k = 0; k < VEC; ++k) {
    live[k] = status[t0 + k] == 0;
    beta[k] = 0.0;
    if (!A.mode && live[k])
      beta[k] = cgs_total(rho_new, A.n_blocks, A.n_cols, t0 + k) / cgs_total(rho_old, A.n_blocks, A.n_cols, t0 + k);
  }
  for (long long v = v0; v < v1; ++v) {
    Cx<double> pv[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      const long long at = v * A.n_cols + t0 + k;
      pv[k] = p[at];
      if (live[k]) {
        const Cx<double> rv = r[at];
        pv[k] = A.mode ? rv : mk<double>(__builtin_fma(beta[k], pv[k].re, rv.re), __builtin_fma(beta[k], pv[k].im, rv.im));
        p[at] = pv[k];
      }
    }
    for (int c = 0; c < A.n_coils; ++c) {
      const Cx<double> sv = s[(long long)c * A.n_vox + v];
      Word out;
#pragma unroll
      for (int k = 0; k < VEC; ++k)
        out.v[k] = mk<S>((S)__builtin_fma(sv.re, pv[k].re, -(sv.im * pv[k].im)),
                         (S)__builtin_fma(sv.re, pv[k].im, sv.im * pv[k].re));
      *reinterpret_cast<Word*>(u + ((long long)c * A.n_vox + v) * A.n_cols + t0) = out;
    }
  }
}

// q[v, t] = sum_c conj(s[c, v]) u[c, v, t] (ascending c) + lambda p[v, t], and part[vb, t] = sum_v Re(conj(p) q) over the
// block's voxels (ascending v).  Initial mode: q is b (no lambda term, p is not read) and the partial is sum_v |b|^2.
template <class S, int VEC>
__global__ __launch_bounds__(XM_CGS_NT) void k_cgs_reduce(const void* __restrict__ uv, const Cx<double>* __restrict__ s,
                                                          const Cx<double>* __restrict__ p, Cx<double>* __restrict__ q,
                                                          double* __restrict__ part, const CgsArgs A) {
  struct alignas(VEC * sizeof(Cx<S>)) Word {
    Cx<S> v[VEC];
  };
  const Cx<S>* __restrict__ u = static_cast<const Cx<S>*>(uv);
  XM_CGS_ITEM(VEC)
  double acc[VEC];
#pragma unroll
  for (int k = 0; k < VEC; ++k) acc[k] = 0.0;
  for (long long v = v0; v < v1; ++v) {
    double qr[VEC], qi[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) qr[k] = qi[k] = 0.0;
    for (int c = 0; c < A.n_coils; ++c) {
      const Cx<double> sv = s[(long long)c * A.n_vox + v];
      const Word w = *reinterpret_cast<const Word*>(u + ((long long)c * A.n_vox + v) * A.n_cols + t0);
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        const double ur = (double)w.v[k].re, ui = (double)w.v[k].im;
        qr[k] = __builtin_fma(sv.re, ur, qr[k]);
        qr[k] = __builtin_fma(sv.im, ui, qr[k]);
        qi[k] = __builtin_fma(sv.re, ui, qi[k]);
        qi[k] = __builtin_fma(-sv.im, ur, qi[k]);
      }
    }
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      const long long at = v * A.n_cols + t0 + k;
      Cx<double> w = mk<double>(qr[k], qi[k]);  // (initial mode: the inner product is with b itself)
      if (!A.mode) {
        w = p[at];
        qr[k] = __builtin_fma(A.lambda, w.re, qr[k]);
        qi[k] = __builtin_fma(A.lambda, w.im, qi[k]);
      }
      q[at] = mk<double>(qr[k], qi[k]);
      acc[k] = __builtin_fma(w.re, qr[k], acc[k]);
      acc[k] = __builtin_fma(w.im, qi[k], acc[k]);
    }
  }
#pragma unroll
  for (int k = 0; k < VEC; ++k) part[vb * A.n_cols + t0 + k] = acc[k];
}

// The per-column decision and the update.  rho, rho0, delta: partials (rho0 those of |b|^2); status_in / status_out: the
// two parities of the status word.  A column whose status_in is 0: rho0 not finite -> 3 and x = NaN; rho <= tol2 rho0
// -> 1; final mode -> stays 0; delta not > 0 or not finite -> 2; otherwise alpha = rho / delta, x += alpha p,
// r -= alpha q, rho_out[vb, t] = sum_v |r|^2 over the block, n_iter = iteration.  A column whose status_in is not 0 is not
// touched.  Voxel block 0 alone writes status_out, n_iter and residual = sqrt(rho / rho0) (of the rho that was tested;
// 0 for rho0 = 0, NaN with status 3) -- for a column that freezes in this launch or, in final mode, one that is still
// running.
// One column per lane: nothing here is coil-sized.
__global__ __launch_bounds__(XM_CGS_NT) void k_cgs_step(Cx<double>* __restrict__ x, Cx<double>* __restrict__ r,
                                                        const Cx<double>* __restrict__ p, const Cx<double>* __restrict__ q,
                                                        const double* __restrict__ rho, const double* __restrict__ rho0,
                                                        const double* __restrict__ delta, double* __restrict__ rho_out,
                                                        const int* __restrict__ status_in, int* __restrict__ status_out,
                                                        int* __restrict__ n_iter, double* __restrict__ residual,
                                                        const CgsArgs A) {
  XM_CGS_ITEM(1)
  const int before = status_in[t0];
  int after = before;
  double alpha = 0.0;
  bool update = false;
  if (before == 0) {
    const double r0 = cgs_total(rho0, A.n_blocks, A.n_cols, t0);
    const double rk = cgs_total(rho, A.n_blocks, A.n_cols, t0);
    if (!(__builtin_fabs(r0) <= 1.79769313486231570815e308)) {
      after = 3;
    } else if (rk <= A.tol2 * r0) {
      after = 1;
    } else if (!A.mode) {
      const double d = cgs_total(delta, A.n_blocks, A.n_cols, t0);
      if (!(d > 0.0 && d <= 1.79769313486231570815e308)) {
        after = 2;
      } else {
        alpha = rk / d;
        update = true;
      }
    }
    if (vb == 0) {
      if (after != 0 || A.mode) residual[t0] = after == 3 ? __builtin_nan("") : r0 == 0.0 ? 0.0 : __builtin_sqrt(rk / r0);
      if (update) n_iter[t0] = A.iteration;
    }
  }
  if (vb == 0) status_out[t0] = after;
  if (after == 3 && before == 0) {
    const double nan = __builtin_nan("");
    for (long long v = v0; v < v1; ++v) x[v * A.n_cols + t0] = mk<double>(nan, nan);
  }
  if (!update) return;
  double acc = 0.0;
  for (long long v = v0; v < v1; ++v) {
    const long long at = v * A.n_cols + t0;
    const Cx<double> pv = p[at], qv = q[at];
    Cx<double> xv = x[at], rv = r[at];
    xv = mk<double>(__builtin_fma(alpha, pv.re, xv.re), __builtin_fma(alpha, pv.im, xv.im));
    rv = mk<double>(__builtin_fma(-alpha, qv.re, rv.re), __builtin_fma(-alpha, qv.im, rv.im));
    x[at] = xv;
    r[at] = rv;
    acc = __builtin_fma(rv.re, rv.re, acc);
    acc = __builtin_fma(rv.im, rv.im, acc);
  }
  rho_out[vb * A.n_cols + t0] = acc;
}
