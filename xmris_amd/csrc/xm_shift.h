// k_shift_time: a per-row time shift of FIDs in one pass (xm_shift_time in include/xmris_hip.h).
//   X[k] = sum_{n<N} x[n] e^{-2 pi i k n / L},   y[n] = (1/L) sum_k X[k] e^{-2 pi i kappa_k phi / L} e^{+2 pi i k n / L},
// kappa_k = k below L/2 and k - L from there on (numpy.fft.fftfreq(L) L), phi the row's delay in dwells.  The shape of
// k_bluestein (xm_kernels.h): two BlockFFT runs with a pointwise product between them, one row per PL::NT threads --
// the product is a closed-form ramp of the row's own delay, not a shared table.
#pragma once
#include "xm_blockfft.h"

template <class T>
struct ShiftArgs {
  const Cx<T>* in;
  Cx<T>* out;
  const Cx<T>* tw;     // stage twiddles of the plan
  const double* frac;  // n_delay delays in dwells; row r takes frac[(r / delay_div) % n_delay]
  long long in_stride, n_rows, n_delay, delay_div;
  int n;               // points per row, n <= L; the transform input is zero beyond them
};

// e^{-2 pi i c}, |c| <= 1.5
XM_DEV Cx<double> shift_unit(double c) {
  double s, co;
  sincospi(-2.0 * c, &s, &co);
  return mk<double>(co, s);
}

// k phi / L modulo 1 for an integer 0 <= k < 2^15, phi = pi_ + pf with pi_ = (rint(phi) mod L) in [0, L) and |pf| <= 1/2:
// the integer part reduces on integers, so a delay of 1000.25 dwells gives the angle as exactly as one of 0.25
XM_DEV double shift_cycles(int k, int pi_, double pf, int L) {
  const int m = (int)(((long long)k * pi_) % L);
  return ((double)m + (double)k * pf) / (double)L;
}

template <class T, class PL, int SPB>
__global__ __launch_bounds__(PL::NT* SPB) void k_shift_time(ShiftArgs<T> A) {
  constexpr int L = PL::N, NT = PL::NT, P = PL::P, H = P / 2;
  static_assert(P % 2 == 0, "bins t + NT q with q >= P/2 are the negative frequencies");
  extern __shared__ __attribute__((aligned(16))) char xm_smem[];
  const int t = threadIdx.x % NT;
  const int ls = threadIdx.x / NT;
  const long long s = (long long)blockIdx.x * SPB + ls;
  const bool live = s < A.n_rows;
  const long long r = live ? s : 0;  // (a dead row computes on row 0 and stores nothing: the barriers need its threads)
  const int n = A.n;
  Cx<T>* lds = reinterpret_cast<Cx<T>*>(xm_smem) + (size_t)ls * BlockFFT<T, PL>::lds_elems();

  const double phi = A.frac[(r / A.delay_div) % A.n_delay];
  Cx<T> v[P];
  const Cx<T>* __restrict__ row = A.in + r * A.in_stride;
#pragma unroll
  for (int q = 0; q < P; ++q) {
    const int pos = t + NT * q;
    const Cx<T> x = row[min(pos, n - 1)];  // clamped, not branched: the P loads go out back to back
    v[q] = pos < n ? x : mk<T>(T(0), T(0));
  }

  BlockFFT<T, PL>::run(v, lds, A.tw, t);

  // the ramp of bins k = t + NT q: one sincos for bin t, one for the step NT and one for the sign wrap, then complex
  // products in fp64.  Bins q >= P/2 have kappa = k - L: e^{-2 pi i (k - L) phi / L} at k = t + L/2 is the factor of bin
  // t times e^{+i pi phi}.  (Set up behind the first transform: in front of it the three factors would be live across it.)
  const double pr = rint(phi), pf = phi - pr;
  int pi_ = (int)fma(-rint(pr / (double)L), (double)L, pr);  // pr mod L in (-L, L), exact: the difference is a small integer
  if (pi_ < 0) pi_ += L;
  const Cx<double> step = shift_unit(shift_cycles(NT, pi_, pf, L));
  Cx<double> lo = shift_unit(shift_cycles(t, pi_, pf, L));
  Cx<double> hi = lo * shift_unit(-0.5 * pf);
  if (pi_ & 1) hi = mk<double>(-hi.re, -hi.im);  // (L is even: rint(phi) and pi_ have one parity)
#pragma unroll
  for (int q = 0; q < H; ++q) {
    v[q] = conj(v[q] * mk<T>((T)lo.re, (T)lo.im));  // conj -> inverse via forward
    v[q + H] = conj(v[q + H] * mk<T>((T)hi.re, (T)hi.im));
    lo = lo * step;
    hi = hi * step;
  }
  // a second pointer to the twiddles: with the same one the compiler keeps the first transform's twiddle registers
  // alive for the second (see k_bluestein)
  const Cx<T>* tw2 = A.tw;
  asm volatile("" : "+s"(tw2));
  BlockFFT<T, PL>::run(v, lds, tw2, t);

  const T scale = T(1.0 / (double)L);
  Cx<T>* __restrict__ orow = A.out + r * (long long)n;
  int ts = t;
  asm volatile("" : "+v"(ts));  // the stores form their addresses again: the P offsets of the loads do not stay in registers
#pragma unroll
  for (int q = 0; q < P; ++q) {
    const int pos = ts + NT * q;
    if (live && pos < n) orow[pos] = conj(v[q]) * scale;
  }
}
