// Frequency-and-phase alignment of repeated transients (the project's own definition, the
// reference has no such function).  Included by xm_align.hip only, which is compiled with -ffp-contract=off: the time
// coordinate tau_t = t0 + t dt is data (two roundings, as numpy forms it), and the fused operations below are the ones
// spelled out.
//
// One transient x[t] against its voxel's reference r[t]: z_t = r_t conj(x_t) over the L leading points,
// C(f) = sum_t z_t e^{-2 pi i f tau_t}, P = |C|^2.  Coarse: arg-max of P on the grid f_g = g delta, |g| <= G.  Refine:
// the zero of P' = 4 pi Im(conj(C) S1) next to it, Newton steps with P'' = 8 pi^2 (|S1|^2 - Re(conj(C) S2)),
// S_k = sum_t tau_t^k z_t e^{-2 pi i f tau_t}, kept inside a bracket by bisection on the sign of P'.  Apply:
// y_t = x_t e^{i (2 pi f* tau_t + phi*)}, phi* = arg C(f*), for all N points.
//
// k_align<AVERAGE>: one 256-thread workgroup per transient (AVERAGE = false) or per voxel (true: the voxel's transients
// in ascending order, every thread's running sums of y in LDS slots of its own), handed out by a device counter (persistent grid, the idiom of
// k_amares_fit and k_coil_combine).  The data are viewed as (n_outer, A, n_inner, N): transient (o, a, i) starts at
// ((o A + a) n_inner + i) N.  All arithmetic fp64; complex64 is widened on load.
//
// Every sum over time is taken the same way: thread t adds its points t, t + 256, ... in ascending order, a tree over
// the 64 lanes of each wave, then the four waves in ascending order.
#pragma once
#include "xm_wg.h"

#define XM_AL_NT 256
static_assert(XM_AL_NT == XM_WG_NT, "k_align runs xm_wg.h's workgroup");
#define XM_AL_MAXL 8192     // points of z staged in the LDS (128 KiB as fp64)
#define XM_AL_MAXGRID 1025  // coarse grid points 2 G + 1
#define XM_AL_K 8           // grid indices g per coarse round; with -g: 16 frequencies, 32 sums per reduction
#define XM_AL_R 8           // most time points per thread and pass of the averaging form (running sum: 32 KiB of LDS)
#define XM_AL_STEPS 40      // refine step cap (status 4)
#define XM_AL_RED 32        // widest reduction
#define XM_AL_LDS_MAX (160 * 1024)

// test-only bits on top of the dtype argument of xm_align_rows: leave a stage out (timing split)
#define XM_AL_SKIP_COARSE 1
#define XM_AL_SKIP_REFINE 2
#define XM_AL_SKIP_APPLY 4

struct AlignArgs {
  const void* x;    // (n_outer, A, n_inner, N) complex64 / complex128
  const void* r;    // reference: voxel v = o n_inner + i starts at v rstride (rstride = 0: one row for all)
  void* y;          // as x, or nullptr (averaging form only)
  void* mean;       // (n_outer, n_inner, N), the input's dtype (averaging form)
  double *shift, *phase, *quality;  // (n_outer, A, n_inner)
  int* status;      // (n_outer, A, n_inner)
  int* n_avg;       // (n_outer, n_inner) (averaging form)
  long long nwork;  // transients, or voxels in the averaging form
  long long n_inner, rstride;
  int A, N, L, G, is_c128, skip;
  int R;  // averaging form: time points per thread and pass, 1 ... XM_AL_R
  double dt, t0, delta, max_shift, min_quality;
  unsigned* counter;  // [2] zero at launch: ticket, workgroups done
};

__host__ __device__ inline size_t al_lds_bytes(int L, int G, int R) {
  // z (re, im), P on the grid (an odd count, made even: the running sums are 16-byte words), the waves' partial sums,
  // the sums themselves, the ticket, the running sums of the averaging form
  return (2 * (size_t)L + (size_t)(2 * G + 2) + 4 * XM_AL_RED + XM_AL_RED + 2 + 2 * (size_t)R * XM_AL_NT) * sizeof(double);
}

struct AlLds {
  double *zr, *zi, *P, *red, *out;
  double2* sum;  // averaging form: R * 256 running sums
};

XM_DEV void al_load(const void* p, int c128, long long i, double& re, double& im) {
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

XM_DEV void al_store(void* p, int c128, long long i, double re, double im) {
  if (c128)
    ((double2*)p)[i] = make_double2(re, im);
  else
    ((float2*)p)[i] = make_float2((float)re, (float)im);
}

XM_DEV double al_tau(const AlignArgs& A, int t) { return A.t0 + (double)t * A.dt; }

// (c, s) = e^{2 pi i f tau}: the turn count f tau loses its integer part before the sine and cosine; the fma takes it
// from the exact product, so the fraction has one rounding whatever the size of f tau
XM_DEV void al_unit(double f, double tau, double& c, double& s) {
  const double k = rint(f * tau);
  sincospi(2.0 * fma(f, tau, -k), &s, &c);
}

// Sums of v[0 .. M) over the workgroup into L.out[0 .. M), the same values for every thread once it returns.  Tree
// over the lanes: at the stage with lane mask m a lane keeps one half of its values and gives the other half to its
// partner, so M values cost M + log2(64 / M) shuffles, not 6 M; then the waves in ascending order.
template <int M>
XM_DEV void al_reduce(const AlLds& L, double (&v)[M]) {
  static_assert(M >= 2 && M <= XM_AL_RED && (M & (M - 1)) == 0, "M: a power of two up to 32");
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  int idx = 0;  // which sum the lane ends up with
  constexpr int STAGES = M == 2 ? 1 : M == 4 ? 2 : M == 8 ? 3 : M == 16 ? 4 : 5;
#pragma unroll
  for (int st = 0; st < STAGES; ++st) {
    const int h = M >> (st + 1), m = 1 << st;
    const bool up = (lane & m) != 0;
    if (up) idx += h;
#pragma unroll
    for (int i = 0; i < h; ++i) {
      double lo = v[i], hi = v[i + h];
      asm("" : "+v"(lo), "+v"(hi));  // two values, not a choice of address: v stays in registers
      v[i] = (up ? hi : lo) + __shfl_xor(up ? lo : hi, m);
    }
  }
#pragma unroll
  for (int st = STAGES; st < 6; ++st) v[0] += __shfl_xor(v[0], 1 << st);
  if (lane < M) L.red[wave * M + idx] = v[0];
  __syncthreads();
  if (t < M) L.out[t] = ((L.red[t] + L.red[M + t]) + L.red[2 * M + t]) + L.red[3 * M + t];
  __syncthreads();
}

// of two grid points the better one: the larger P; on a tie the smaller |g|, then the negative g
XM_DEV bool al_better(double p1, int g1, double p2, int g2) {
  if (p1 != p2) return p1 > p2;
  const int a1 = g1 < 0 ? -g1 : g1, a2 = g2 < 0 ? -g2 : g2;
  return a1 != a2 ? a1 < a2 : g1 < g2;
}

// z into the LDS; sum z, ||r||^2, ||x||^2 over the L points into L.out[0 .. 4); returns 1 on a non-finite sample
XM_DEV int al_stage(const AlignArgs& A, const AlLds& L, long long xoff, long long roff) {
  int bad = 0;
  double v[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
  for (int t = threadIdx.x; t < A.L; t += XM_AL_NT) {
    double xr, xi, rr, ri;
    al_load(A.x, A.is_c128, xoff + t, xr, xi);
    al_load(A.r, A.is_c128, roff + t, rr, ri);
    if (!isfinite(xr) || !isfinite(xi) || !isfinite(rr) || !isfinite(ri)) bad = 1;
    const double zr = rr * xr + ri * xi, zi = ri * xr - rr * xi;  // r conj(x)
    L.zr[t] = zr;
    L.zi[t] = zi;
    v[0] += zr;
    v[1] += zi;
    v[2] += rr * rr + ri * ri;
    v[3] += xr * xr + xi * xi;
  }
  al_reduce<4>(L, v);  // (its barriers also publish z)
  return __syncthreads_or(bad);
}

// P on the grid points +-(g0 + 1 .. g0 + K) into L.P.  Every time point steps its own rotator w = e^{-2 pi i delta tau}
// from the power g0 + 1, which is a true sine and cosine, so a recurrence is never longer than K - 1 products.
XM_DEV void al_coarse_round(const AlignArgs& A, const AlLds& L, int g0) {
  double acc[4 * XM_AL_K];
#pragma unroll
  for (int k = 0; k < 4 * XM_AL_K; ++k) acc[k] = 0.0;
  const double f1 = (double)(g0 + 1) * A.delta;
#pragma unroll 1
  for (int t = threadIdx.x; t < A.L; t += XM_AL_NT) {
    const double tau = al_tau(A, t), zr = L.zr[t], zi = L.zi[t];
    double wc, ws, pc, ps;
    al_unit(-A.delta, tau, wc, ws);
    al_unit(-f1, tau, pc, ps);
#pragma unroll
    for (int k = 0; k < XM_AL_K; ++k) {
      const double a = zr * pc, b = zi * ps, c = zr * ps, d = zi * pc;
      acc[4 * k] += a - b;  // z p: the frequency +g
      acc[4 * k + 1] += c + d;
      acc[4 * k + 2] += a + b;  // z conj(p): -g
      acc[4 * k + 3] += d - c;
      const double nc = pc * wc - ps * ws;
      ps = pc * ws + ps * wc;
      pc = nc;
    }
  }
  al_reduce<4 * XM_AL_K>(L, acc);
  const int k = threadIdx.x >> 1, g = g0 + 1 + k;
  if (threadIdx.x < 2 * XM_AL_K && g <= A.G) {
    const int o = 4 * k + 2 * (threadIdx.x & 1);
    L.P[(threadIdx.x & 1) ? A.G - g : A.G + g] = L.out[o] * L.out[o] + L.out[o + 1] * L.out[o + 1];
  }
  // (the next writer of L.out passes a barrier first)
}

// the best grid point, every thread alike; `bad`: 1 when a P is not finite
XM_DEV int al_argmax(const AlignArgs& A, const AlLds& L, double& pbest, int& bad) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  double p = -1.0;  // (P >= 0: a thread without grid points never wins)
  int g = 0, nf = 0;
  __syncthreads();  // P is complete
  for (int n = t; n <= 2 * A.G; n += XM_AL_NT) {
    const double pn = L.P[n];
    if (!isfinite(pn)) nf = 1;
    if (al_better(pn, n - A.G, p, g)) {
      p = pn;
      g = n - A.G;
    }
  }
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    const double po = __shfl_xor(p, m);
    const int go = __shfl_xor(g, m);
    if (al_better(po, go, p, g)) {
      p = po;
      g = go;
    }
  }
  if (lane == 0) {
    L.red[wave] = p;
    L.red[4 + wave] = (double)g;
  }
  __syncthreads();
  p = L.red[0];
  g = (int)L.red[4];
  for (int w = 1; w < 4; ++w)
    if (al_better(L.red[w], (int)L.red[4 + w], p, g)) {
      p = L.red[w];
      g = (int)L.red[4 + w];
    }
  bad = __syncthreads_or(nf);  // (also: red is free again)
  pbest = p;
  return g;
}

// C, S1, S2 at f into L.out[0 .. 6), true sines and cosines of reduced arguments
XM_DEV void al_eval(const AlignArgs& A, const AlLds& L, double f) {
  double v[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
  for (int t = threadIdx.x; t < A.L; t += XM_AL_NT) {
    const double tau = al_tau(A, t), zr = L.zr[t], zi = L.zi[t];
    double c, s;
    al_unit(-f, tau, c, s);
    const double ur = zr * c - zi * s, ui = zr * s + zi * c;
    v[0] += ur;
    v[1] += ui;
    v[2] += tau * ur;
    v[3] += tau * ui;
    v[4] += tau * tau * ur;
    v[5] += tau * tau * ui;
  }
  al_reduce<8>(L, v);
}

// P' / 4 pi and P'' / 8 pi^2 from L.out
XM_DEV double al_d1(const AlLds& L) { return L.out[0] * L.out[3] - L.out[1] * L.out[2]; }
XM_DEV double al_d2(const AlLds& L) {
  return (L.out[2] * L.out[2] + L.out[3] * L.out[3]) - (L.out[0] * L.out[4] + L.out[1] * L.out[5]);
}

struct AlFit {
  double f, phi, uc, us, quality;  // (uc, us) = e^{i phi}
  int status;
};

XM_DEV void al_phase_unit(AlFit& F) {
  double s, c;
  sincos(F.phi, &s, &c);
  F.uc = c;
  F.us = s;
}

// coarse and refine stages of one transient whose z is staged; every thread returns the same
XM_DEV AlFit al_fit(const AlignArgs& A, const AlLds& L, int bad) {
  AlFit F;
  F.f = F.phi = F.quality = NAN;
  F.uc = F.us = 0.0;
  F.status = 2;
  const double c0r = L.out[0], c0i = L.out[1], nr2 = L.out[2], nx2 = L.out[3];
  __syncthreads();  // L.out is read
  if (threadIdx.x == 0) L.P[A.G] = c0r * c0r + c0i * c0i;
  if (!(A.skip & XM_AL_SKIP_COARSE))
    for (int g0 = 0; g0 < A.G; g0 += XM_AL_K) al_coarse_round(A, L, g0);
  double pbest;
  int pbad;
  int g = al_argmax(A, L, pbest, pbad);
  if (A.skip & XM_AL_SKIP_COARSE) {
    g = 0;
    pbest = L.P[A.G];
    pbad = !isfinite(pbest);
  }
  if (bad || pbad || !isfinite(nr2) || !isfinite(nx2)) return F;
  if (!(pbest > 0.0)) {  // C is zero on the whole grid: nothing to go by
    F.f = F.phi = F.quality = 0.0;
    F.uc = 1.0;
    F.status = 3;
    return F;
  }
  F.status = 0;
  // One loop holds the only call of al_eval: at the window's end when g* is the grid's last point (EDGE), at the Newton
  // iterates (NEWTON), and at f* for C(f*) (FINAL).
  enum { EDGE, NEWTON, FINAL };
  const bool refine = A.G > 0 && !(A.skip & XM_AL_SKIP_REFINE);
  int mode = !refine ? FINAL : (g == A.G || g == -A.G) ? EDGE : NEWTON, steps = 0;
  const double e = g > 0 ? A.max_shift : -A.max_shift, tol = A.delta * 0x1p-40;
  double a = fmax((double)(g - 1) * A.delta, -A.max_shift), b = fmin((double)(g + 1) * A.delta, A.max_shift);
  double f = (double)g * A.delta, cr, ci;
  for (;;) {
    const double fe = mode == EDGE ? e : f;
    al_eval(A, L, fe);
    const double d1 = al_d1(L), d2 = al_d2(L);
    cr = L.out[0];
    ci = L.out[1];
    __syncthreads();
    if (mode == FINAL) break;
    if (mode == EDGE) {
      if (g > 0 ? d1 > 0.0 : d1 < 0.0) {  // P still rises where the window ends: that end, unrefined
        F.status = 1;
        f = e;
        break;
      }
      mode = NEWTON;
      continue;
    }
    if (d1 > 0.0)
      a = f;
    else if (d1 < 0.0)
      b = f;
    else
      break;
    double fn = d2 < 0.0 ? f - d1 / (2.0 * M_PI * d2) : NAN;  // P' / P'' = (4 pi d1) / (8 pi^2 d2)
    if (!(fn >= a && fn <= b)) fn = 0.5 * (a + b);          // no maximum that way, or out of the bracket: bisect
    const double step = fabs(fn - f);
    f = fn;
    if (step <= tol) {
      mode = FINAL;
    } else if (++steps == XM_AL_STEPS) {
      F.status = 4;
      mode = FINAL;
    }
  }
  F.f = f;
  F.phi = atan2(ci, cr);
  al_phase_unit(F);
  F.quality = hypot(cr, ci) / (sqrt(nr2) * sqrt(nx2));
  return F;
}

// y_t of one point: x_t e^{i (2 pi f tau_t + phi)}; status 2 gives zero, status 3 x itself
XM_DEV void al_point(const AlignArgs& A, const AlFit& F, long long xoff, int t, double& yr, double& yi) {
  if (F.status == 2) {
    yr = yi = 0.0;
    return;
  }
  al_load(A.x, A.is_c128, xoff + t, yr, yi);
  if (F.status == 3) return;
  double c, s;
  al_unit(F.f, al_tau(A, t), c, s);
  const double qc = c * F.uc - s * F.us, qs = c * F.us + s * F.uc;
  const double xr = yr, xi = yi;
  yr = xr * qc - xi * qs;
  yi = xr * qs + xi * qc;
}

template <bool AVERAGE>
__global__ __launch_bounds__(XM_AL_NT) void k_align(AlignArgs A) {
  extern __shared__ double al_sm[];
  const int t = threadIdx.x;
  AlLds L;
  L.zr = al_sm;
  L.zi = L.zr + A.L;
  L.P = L.zi + A.L;
  L.red = L.P + (2 * A.G + 2);
  L.out = L.red + 4 * XM_AL_RED;
  unsigned* next = (unsigned*)(L.out + XM_AL_RED);
  L.sum = (double2*)(L.out + XM_AL_RED + 2);

  for (;;) {
    const long long w = wg_next_item(A.counter, next);
    if (w >= A.nwork) break;
    if (!AVERAGE) {
      // w = (o A + a) n_inner + i
      const long long oa = w / A.n_inner, i = w - oa * A.n_inner, v = (oa / A.A) * A.n_inner + i;
      const long long xoff = w * A.N;
      const int bad = al_stage(A, L, xoff, v * A.rstride);
      const AlFit F = al_fit(A, L, bad);
      if (t == 0) {
        A.shift[w] = F.f;
        A.phase[w] = F.phi;
        A.quality[w] = F.quality;
        A.status[w] = F.status;
      }
      if (!(A.skip & XM_AL_SKIP_APPLY))
#pragma unroll 1
        for (int p = t; p < A.N; p += XM_AL_NT) {
          double yr, yi;
          al_point(A, F, xoff, p, yr, yi);
          al_store(A.y, A.is_c128, xoff + p, yr, yi);
        }
    } else {
      // w = o n_inner + i; pass 0 fits every transient and sums the first R * 256 points of its y (every thread in LDS
      // slots of its own), the passes after it sum the next R * 256 points from the shift and phase that pass 0 stored
      const long long o = w / A.n_inner, i = w - o * A.n_inner;
      int count = 0;
      for (int p0 = 0; p0 < A.N; p0 += A.R * XM_AL_NT) {
        const int pend = p0 + A.R * XM_AL_NT < A.N ? p0 + A.R * XM_AL_NT : A.N;
        for (int j = 0; j < A.R; ++j) L.sum[j * XM_AL_NT + t] = make_double2(0.0, 0.0);  // (a thread's own slots)
        count = 0;
        for (int a = 0; a < A.A; ++a) {
          const long long row = (o * A.A + a) * A.n_inner + i, xoff = row * A.N;
          AlFit F;
          if (p0 == 0) {
            const int bad = al_stage(A, L, xoff, w * A.rstride);
            F = al_fit(A, L, bad);
            if (t == 0) {
              A.shift[row] = F.f;
              A.phase[row] = F.phi;
              A.quality[row] = F.quality;
              A.status[row] = F.status;
            }
          } else {  // written by this workgroup's thread 0 before the barrier that ended pass 0
            F.f = A.shift[row];
            F.phi = A.phase[row];
            F.quality = A.quality[row];
            F.status = A.status[row];
            al_phase_unit(F);
          }
          const bool in = F.status != 2 && F.quality >= A.min_quality;
          if (in) ++count;
          if ((A.skip & XM_AL_SKIP_APPLY) || !(in || A.y)) continue;
#pragma unroll 1
          for (int p = p0 + t, j = 0; p < pend; p += XM_AL_NT, ++j) {
            double yr, yi;
            al_point(A, F, xoff, p, yr, yi);
            if (A.y) al_store(A.y, A.is_c128, xoff + p, yr, yi);
            if (in) {
              const double2 q = L.sum[j * XM_AL_NT + t];
              L.sum[j * XM_AL_NT + t] = make_double2(q.x + yr, q.y + yi);
            }
          }
        }
        if (!(A.skip & XM_AL_SKIP_APPLY)) {
          const double n = (double)count;
          for (int p = p0 + t, j = 0; p < pend; p += XM_AL_NT, ++j) {
            const double2 q = L.sum[j * XM_AL_NT + t];
            al_store(A.mean, A.is_c128, w * A.N + p, count ? q.x / n : 0.0, count ? q.y / n : 0.0);
          }
        }
        __syncthreads();  // the outputs of pass 0 are visible to the workgroup
      }
      if (t == 0) A.n_avg[w] = count;
    }
    __syncthreads();
  }
  wg_leave(A.counter);
}
