// Device-resident autophase search (reference processing/phasing.py:100-122 ACME objective, :276-284
// scipy.optimize.differential_evolution(best1bin, tol=0.01, seed=42) and the first step of its L-BFGS-B polish).
//
// The (p0, p1) search is O(1) work per dataset, but it sits between a dataset's guess stage and its main pass, and on
// the host it costs 3 core-milliseconds per dataset (8192 bins): a node that streams small datasets -- or eight ranks
// of it -- runs out of cores long before the GPUs run out of bandwidth, and a shared host's scheduler decides the
// tail.  Here ONE workgroup per search runs scipy's algorithm on a CU of its own beside the streaming kernels:
//
//   wave 0        `Optimiser`: numpy's legacy RandomState (`Rng`, MT19937: state and tempered outputs in LDS, regenerated
//                 two generations ahead in parallel, consumed through a 64-word register window by v_readlane; the
//                 population-index shuffle takes its accepted draws from per-step ballots over that window), scipy 1.15.3's
//                 DifferentialEvolutionSolver for the reference's configuration (latin hypercube, best1bin, dither
//                 U[0.5, 1), CR 0.7, immediate updating, std/mean convergence) with the population held one member
//                 per LANE -- the same statements in the same order as xm_solver.cpp, IEEE arithmetic without
//                 contraction, so the trial vectors are scipy's bit for bit given equal comparisons of the energies;
//   waves 1..7    `Objective`: every thread keeps P + 1 consecutive bins of the arg-max spectrum (complex128) in
//                 registers for the whole search; e^{i phi_k} = A[t / 32] B[t % 32] C[j] from three small tables (one
//                 sincos per table entry and evaluation, 32 + 14 + P + 1 entries, instead of one per bin), one pass,
//                 five sums (the same five as xm_solver_obj.cpp), wave reductions through DPP, 7 partial sums to wave 0.
//   While the workers evaluate trial t, wave 0 already draws the random part of trial t + 1 (fill point, the
//   population-index shuffle, the crossover mask -- none of it depends on the population), so the serial part between
//   two evaluations is: combine, accept / reject, build the next trial, its phase tables.
//
// The search ends with the test scipy's polish starts with (f and its forward-difference gradient at the best member,
// `gradient_points`; `projected_gradient_norm` against pgtol): passed -- the usual case -- means scipy returns that
// member, and so does this kernel; failed is reported (`needs_polish`) and the caller polishes on the reference's
// own route (xmris_amd/autophase_solver.py, polish="exact").  `search_body` drives these parts for both kernels;
// `fill_record` writes the record (k_search: pinned host memory, its sequence word last).  gfx950 only.
#include "xm_host.h"

#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstring>
#include <map>
#include <type_traits>
#include <mutex>
#include <vector>

namespace {

constexpr int kThreads = 512;                 // 8 waves, up to 256 VGPRs each: the fp64 objective (sincos, log, divisions) needs room;
                                              // nine waves (512 workers) would cap them at 168 and spill hundreds
constexpr int kWaves = kThreads / XM_WAVE;
constexpr int kWorkers = kThreads - XM_WAVE;  // waves 1..7
constexpr int kTabA = kWorkers / 32;          // 14
constexpr int kMaxP = 37;

struct SearchArgs {             // of both kernels
  const void* in;               // k_search: n complex128 (re, im); k_search_rows: in[n_rows, n], complex64 or complex128
  const unsigned* mt0;          // MT19937 state right after seeding (624 words)
  xm_search_result* out;        // k_search: device-accessible result record
  xm_search_row* rec;           // k_search_rows: one record per row
  const double* xs;             // evaluation mode (k_search): n_eval parameter pairs (degrees)
  double* fs;                   // ... their scores
  double c0, cstep, x_range;    // uniform coordinate axis: c[k] = c0 + k cstep; x_range = max c - min c
  double tol;
  double pivot;                 // k_search_rows: the pivot of every row (NaN: the coordinate of its arg-max)
  unsigned long long seq;
  long long n_rows;
  int n, n_eval, p0_only, maxiter, target_idx;
};

struct alignas(16) SearchLds {
  unsigned mt[624];
  unsigned y[1248];          // tempered outputs of TWO generations of the state (the stream never waits at a seam)
  double tab[2 * 96];        // A[14] | B[32] | C[P + 1], (cos, sin) pairs
  double part[kWaves][6];    // per worker wave: sum ds, sum ds ln ds, sum a, sum (a/2)^2, max d
  double prm[4];             // p0r, p1r of the evaluation in flight
  double lhs[30][2];         // latin hypercube samples
  double en[32];             // energies (convergence test)
  double dv[32];             // ... their squared deviations
  double pts[3][2], dx[2], vals[4];  // gradient test: the points, the exact steps, the scores
  double amax_v[kWaves];
  int amax_i[kWaves];
  int stop;
};

#define SDEV __device__ __forceinline__

SDEV double rdlane_d(double v, int lane) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffffll), lane);
  const int hi = __builtin_amdgcn_readlane((int)(b >> 32), lane);
  return __longlong_as_double(((long long)hi << 32) | (unsigned long long)(unsigned)lo);
}

// numpy's pairwise summation for n <= 128 (xm_solver.cpp np_sum_small): the population has 15 or 30 members
SDEV double np_sum_small(const double* a, int n) {
  if (n < 8) {
    double r = 0.;
    for (int i = 0; i < n; ++i) r += a[i];
    return r;
  }
  double r[8];
  for (int j = 0; j < 8; ++j) r[j] = a[j];
  int i;
  for (i = 8; i < n - (n % 8); i += 8)
    for (int j = 0; j < 8; ++j) r[j] += a[i + j];
  double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (; i < n; ++i) res += a[i];
  return res;
}

// ln x for finite x > 0: fdlibm's reduction and polynomial, as xm_solver_obj.cpp::fast_log (no special cases: the
// caller multiplies by x and skips x == 0)
SDEV double log_pos(double x) {
  long long ix = __double_as_longlong(x);
  const long long k = (ix - 0x3fe6a09e667f3bcdLL) >> 52;
  const double m = __longlong_as_double(ix - (k << 52));
  const double kd = (double)(int)k;
  const double f = m - 1.0;
  // s = f / (2 + f): v_rcp_f64 + two Newton steps + one correction of the quotient (<= 1 ulp; an IEEE division is
  // twice the instructions, and this quotient only feeds a polynomial)
  const double y = 2.0 + f;
  double r = __builtin_amdgcn_rcp(y);
  r = fma(fma(-y, r, 1.0), r, r);
  r = fma(fma(-y, r, 1.0), r, r);
  double s = f * r;
  s = fma(fma(-y, s, f), r, s);
  const double z = s * s;
  const double w = z * z;
  const double t1 = w * fma(w, fma(w, 1.531383769920937332e-01, 2.222219843214978396e-01), 3.999999999940941908e-01);
  const double t2 = z * fma(w, fma(w, fma(w, 1.479819860511658591e-01, 1.818357216161805012e-01), 2.857142874366239149e-01),
                            6.666666666666735130e-01);
  return fma(kd, 6.93147180559945286227e-01, f - s * (f - (t2 + t1)));
}

// wave-wide sum / maximum of a double through DPP (no LDS round trips); the result is in lane 63
template <bool MAX, int CTRL, int ROW_MASK>
SDEV double dpp_step(double v) {  // v (+ or max) the lane that CTRL names; lanes outside ROW_MASK's rows keep v
  const long long ib = __double_as_longlong(MAX ? -DBL_MAX : 0.0);
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_update_dpp((int)(ib & 0xffffffffll), (int)(b & 0xffffffffll), CTRL, ROW_MASK, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp((int)(ib >> 32), (int)(b >> 32), CTRL, ROW_MASK, 0xf, false);
  const double o = __longlong_as_double(((long long)hi << 32) | (unsigned long long)(unsigned)lo);
  return MAX ? fmax(v, o) : v + o;
}
template <bool MAX>
SDEV double wave_reduce_d(double v) {
  v = dpp_step<MAX, 0xB1, 0xf>(v);   // quad_perm:[1,0,3,2]
  v = dpp_step<MAX, 0x4E, 0xf>(v);   // quad_perm:[2,3,0,1]
  v = dpp_step<MAX, 0x141, 0xf>(v);  // row_half_mirror
  v = dpp_step<MAX, 0x140, 0xf>(v);  // row_mirror
  v = dpp_step<MAX, 0x142, 0xa>(v);  // row_bcast:15 -> rows 1, 3
  return dpp_step<MAX, 0x143, 0xc>(v);  // row_bcast:31 -> rows 2, 3
}

// The optimiser's random stream (wave 0; every value here is wave-uniform unless it is "one per lane").
struct Rng {
  SearchLds* L;
  unsigned yw;    // one per lane: word (pos - widx + lane) of the stream
  int pos, widx;  // pos: index of the next word in y[0 .. 1247] (two generations, circular); widx: its place in the window

#define XM_LDS_ORDER() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")
  // Words FIRST .. FIRST + COUNT - 1 of the next state; mt[i + SRC] is the word 397 places on, already new when SRC < 0.
  // Lanes exchange words through the LDS inside one wave: a phase reads ALL of its inputs, then writes -- the waits
  // between are also compiler barriers (per-thread alias analysis would let a store pass another lane's load).  The
  // guard is on the lane's offset, not on i: that form decides how the compiler packs these integers, and the P = 37
  // kernels' scratch with it (profiles/search_refactor/resource_usage.txt).
  template <int FIRST, int COUNT, int SRC>
  static SDEV void twist(unsigned* mt, int lane) {
    const unsigned UPPER = 0x80000000u, LOWER = 0x7fffffffu, MATRIX = 0x9908b0dfu;
    constexpr int Q = (COUNT + XM_WAVE - 1) / XM_WAVE;
    unsigned v[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const int i = FIRST + lane + XM_WAVE * q;
      if (lane + XM_WAVE * q < COUNT) {
        const unsigned yv = (mt[i] & UPPER) | (mt[i + 1] & LOWER);
        v[q] = mt[i + SRC] ^ (yv >> 1) ^ ((0u - (yv & 1u)) & MATRIX);
      }
    }
    XM_LDS_ORDER();
#pragma unroll
    for (int q = 0; q < Q; ++q)
      if (lane + XM_WAVE * q < COUNT) mt[FIRST + lane + XM_WAVE * q] = v[q];
    XM_LDS_ORDER();
  }
  // numpy mt19937_gen in three dependency-free phases, then the tempering of all 624 words into half `half` of y
  SDEV void produce(int half, int lane) {
    unsigned* mt = L->mt;
    twist<0, 227, 397>(mt, lane);     // mt[i + 397] is an old word
    twist<227, 227, -227>(mt, lane);  // mt[i - 227] is a new word of the first phase
    twist<454, 169, -227>(mt, lane);  // ... of the second phase
    if (lane == 0) {  // word 623 reads the NEW word 0
      const unsigned yv = (mt[623] & 0x80000000u) | (mt[0] & 0x7fffffffu);
      mt[623] = mt[396] ^ (yv >> 1) ^ ((0u - (yv & 1u)) & 0x9908b0dfu);
    }
    XM_LDS_ORDER();
    unsigned* y = L->y + 624 * half;
    for (int i = lane; i < 624; i += XM_WAVE) {
      unsigned w = mt[i];
      w ^= (w >> 11);
      w ^= (w << 7) & 0x9d2c5680u;
      w ^= (w << 15) & 0xefc60000u;
      w ^= (w >> 18);
      y[i] = w;
    }
    XM_LDS_ORDER();
  }
  SDEV void start(int lane) {  // (the seeded state has produced nothing yet: numpy generates on the first draw)
    produce(0, lane);
    produce(1, lane);
    pos = 0;
    widx = XM_WAVE;
  }
  SDEV void refill(int lane) {  // the next 64 words of the stream, one per lane
    int i = pos + lane;
    i -= i >= 1248 ? 1248 : 0;
    yw = L->y[i];
    widx = 0;
  }
  // `k` (<= 64) words were consumed.  Leaving a half frees it for the generation after the one ahead: the words of a
  // loaded window that are still unread all lie beyond the seam.
  SDEV void advance(int k, int lane) {
    const int np = pos + k;
    if (pos < 624 && np >= 624) {
      produce(0, lane);
      pos = np;
    } else if (np >= 1248) {
      produce(1, lane);
      pos = np - 1248;
    } else {
      pos = np;
    }
  }
  SDEV unsigned next32(int lane) {
    if (widx == XM_WAVE) refill(lane);
    const unsigned w = (unsigned)__builtin_amdgcn_readlane((int)yw, widx);
    ++widx;
    advance(1, lane);
    return w;
  }
  SDEV double next_double(int lane) {  // random_double: 53 bits from two draws
    const int a = (int)(next32(lane) >> 5), b = (int)(next32(lane) >> 6);
    return ((double)a * 67108864.0 + (double)b) / 9007199254740992.0;
  }
  SDEV unsigned interval(unsigned max, int lane) {  // legacy random_interval: masked rejection
    if (max == 0) return 0;
    const unsigned mask = 0xffffffffu >> __builtin_clz(max);
    unsigned v;
    while ((v = (next32(lane) & mask)) > max) {
    }
    return v;
  }
  // RandomState._shuffle_raw (for i = n-1 .. 1: j = interval(i); swap(a[i], a[j])) on an array held one element per
  // lane.  The accepted draw of step i is the first word at or behind the stream position whose masked value is <= i:
  // a ballot over the 64-word window answers that for every position at once, so a step is a shift, a count of
  // trailing zeros and one v_readlane instead of a rejection loop; the swaps are tracked as "where has this lane's
  // element gone" (two compares and two selects per step, no cross-lane traffic) and applied by ONE ds_permute.
  // Fully unrolled and free of branches, so that the ballots, the scalar chain (position -> next position), the
  // v_readlanes and the tracking overlap in the wave's one instruction stream.  A window that runs out (more than
  // 64 draws for <= 29 steps: rare) leaves everything untouched and the plain loop does the shuffle.
  template <int NN>
  SDEV int shuffle_n(int arr, int lane) {
    refill(lane);
    int p = lane, cur = 0;
    bool ok = true;
#pragma unroll
    for (int i = NN - 1; i >= 1; --i) {
      const unsigned mask = 0xffffffffu >> __builtin_clz((unsigned)i);
      const unsigned long long acc = __ballot((yw & mask) <= (unsigned)i);
      const int c = cur < XM_WAVE - 1 ? cur : XM_WAVE - 1;
      const unsigned long long m = acc >> c;
      ok = ok && cur < XM_WAVE && m != 0ull;
      const int q0 = c + (int)__builtin_ctzll(m | 0x8000000000000000ull);
      const int q = q0 < XM_WAVE - 1 ? q0 : XM_WAVE - 1;
      const int j = (int)((unsigned)__builtin_amdgcn_readlane((int)yw, q) & mask);
      cur = q + 1;
      p = p == i ? j : (p == j ? i : p);
    }
    if (ok) {
      widx = cur;
      advance(cur, lane);
      return __builtin_amdgcn_ds_permute(p << 2, arr);  // lane l's element goes to lane p
    }
    for (int i = NN - 1; i >= 1; --i) {  // (the window is loaded, nothing was consumed)
      const int j = (int)interval((unsigned)i, lane);
      const int ai = __builtin_amdgcn_readlane(arr, i), aj = __builtin_amdgcn_readlane(arr, j);
      arr = lane == i ? aj : (lane == j ? ai : arr);
    }
    return arr;
  }
  SDEV int shuffle(int arr, int n, int lane) { return n == 30 ? shuffle_n<30>(arr, lane) : shuffle_n<15>(arr, lane); }
};

struct Drawn {  // the random part of one trial (does not depend on the population)
  int fill, r0, r1;
  bool cross[2];
};

// ---- the parts of one search, in the order search_body (below) runs them ------------------------------------------------
constexpr double kLo0 = -180.0, kHi0 = 180.0, kLo1 = -4000.0, kHi1 = 4000.0;  // the bounds of p0 and p1, degrees

// _scale_parameters: a population member's coordinate in [0, 1] -> degrees
SDEV double degrees0(double v) { return 0.5 * (kLo0 + kHi0) + (v - 0.5) * fabs(kLo0 - kHi0); }
SDEV double degrees1(double v) { return 0.5 * (kLo1 + kHi1) + (v - 0.5) * fabs(kLo1 - kHi1); }

// A worker's P + 1 consecutive bins from k0 on (the last one is the next worker's first); `load(k)`: bin k as complex128
template <int P, class Load>
SDEV void load_bins(Load load, int k0, int n, double (&re)[P + 1], double (&im)[P + 1]) {
#pragma unroll
  for (int j = 0; j <= P; ++j) {
    const int k = k0 + j;
    const bool ok = k < n;
    const double2 v = ok ? load(k) : make_double2(0., 0.);
    re[j] = v.x;
    im[j] = v.y;
  }
}

// A thread's place in the workgroup, worked out ONCE in search_body.  Parts that derive it again (even tw P) branch and
// index on values the compiler does not merge with the driver's, and the P = 19 and 37 kernels spill more for it.
struct Role {
  int lane, wave;
  bool worker;  // waves 1..7
  int tw, k0;   // worker index, its first bin
};

struct ArgMax {
  int bin;
  bool bad, zero;  // ROWS: a sample that is not finite; no bin above zero
};

// First arg-max of |slice| (phasing.py:229 on the winning row; np.argmax's tie order: the lowest bin), the same answer in
// every thread.  Every thread of the workgroup calls it (one barrier inside).
template <int P, bool ROWS>
SDEV ArgMax first_argmax(SearchLds& L, const Role& me, const double (&re)[P + 1], const double (&im)[P + 1], int n) {
  const int lane = me.lane, wave = me.wave, k0 = me.k0;
  double bv = -1.;
  int bi = 0x7fffffff;
  bool bad = false;
  if (me.worker) {
#pragma unroll
    for (int j = 0; j < P; ++j) {
      const double m2 = re[j] * re[j] + im[j] * im[j];
      if (ROWS) bad |= k0 + j < n && !(fabs(re[j]) <= DBL_MAX && fabs(im[j]) <= DBL_MAX);
      if (k0 + j < n && m2 > bv) {
        bv = m2;
        bi = k0 + j;
      }
    }
    for (int m = 1; m < XM_WAVE; m <<= 1) {
      const double ov = __shfl_xor(bv, m);
      const int oi = __shfl_xor(bi, m);
      if (ov > bv || (ov == bv && oi < bi)) {
        bv = ov;
        bi = oi;
      }
    }
    if (ROWS) bad = __any(bad);
    if (lane == 0) {
      L.amax_v[wave] = bv;
      L.amax_i[wave] = ROWS && bad ? -1 : bi;  // (a bin index is never negative)
    }
  }
  __syncthreads();
  bv = -1.;
  bi = 0x7fffffff;
  bad = false;
  for (int w = 1; w < kWaves; ++w) {
    const double ov = L.amax_v[w];
    const int oi = L.amax_i[w];
    if (ROWS && oi < 0) {
      bad = true;
      continue;
    }
    if (ov > bv || (ov == bv && oi < bi)) {
      bv = ov;
      bi = oi;
    }
  }
  return {bi, bad, !(bv > 0.)};
}

// The ACME objective of one spectrum.  Workers: the phase tables of (p0r, p1r) = L.prm, then each thread's share of the
// five sums; wave 0: the 7 partial sums -> the score.
template <int P, bool FULL>
struct Objective {
  double re[P + 1], im[P + 1];  // this worker's bins, for the whole search
  double u0, du;                // u[k] = (c[k] - pivot) / x_range = u0 + k du   (phasing.py:69 on a uniform axis)
  int n;

  SDEV void tables(SearchLds& L, const Role& me) const {
    const int tw = me.tw;
    if (me.worker && tw < kTabA + 32 + P + 1) {
      const double p0r = L.prm[0], p1r = L.prm[1];
      double ang;
      if (tw < kTabA)
        ang = p0r + p1r * (u0 + du * (double)(32 * P * tw));
      else if (tw < kTabA + 32)
        ang = p1r * (du * (double)(P * (tw - kTabA)));
      else
        ang = p1r * (du * (double)(tw - kTabA - 32));
      double sn, cs;
      sincos(ang, &sn, &cs);
      L.tab[2 * tw] = cs;
      L.tab[2 * tw + 1] = sn;
    }
  }
  SDEV void partial_sums(SearchLds& L, const Role& me) const {
    const int tw = me.tw, k0 = me.k0;
    if (!me.worker) return;
    const double* ta = L.tab + 2 * (tw >> 5);
    const double* tb = L.tab + 2 * (kTabA + (tw & 31));
    const double* tc = L.tab + 2 * (kTabA + 32);
    const double ar = ta[0], ai = ta[1], br = tb[0], bi = tb[1];
    const double xr = fma(ar, br, -(ai * bi)), xi = fma(ar, bi, ai * br);
    auto phased = [&](int j) {  // Re(slice[k] e^{i phi_k})   (phasing.py:73, 104)
      const double cr = tc[2 * j], ci = tc[2 * j + 1];
      const double tr = fma(xr, cr, -(xi * ci)), ti = fma(xr, ci, xi * cr);
      return fma(re[j], tr, -(im[j] * ti));
    };
    double s_ds = 0., s_dl = 0., s_as = 0., s_as2 = 0., mx = -DBL_MAX;
    double dj = phased(0);
#pragma unroll
    for (int j = 0; j < P; ++j) {
      const double dn = phased(j + 1);
      const int k = k0 + j;
      // FULL (n == 448 P): all bins exist, and only the very last one has no forward difference -- no per-bin predicates
      const bool bin = FULL || k < n, diff = FULL ? (j + 1 < P || k + 1 < n) : k + 1 < n;
      const double as_ = dj - fabs(dj);
      s_as += bin ? as_ : 0.;
      s_as2 = fma(0.5 * as_, bin ? 0.5 * as_ : 0., s_as2);
      mx = bin ? fmax(mx, dj) : mx;
      const double ds = diff ? fabs((dn - dj) * 0.5) : 0.;
      s_ds += ds;
      // zeros -> p = 1 -> contribute 0 (phasing.py:110): ds ln(max(ds, tiny)) is exactly 0 there, without a branch
      s_dl = fma(ds, log_pos(fmax(ds, 2.2250738585072014e-308)), s_dl);
      dj = dn;
      // (four bins at a time: let loose, the scheduler interleaves all P logarithms and spills hundreds of registers)
      if ((j & 3) == 3) __builtin_amdgcn_sched_barrier(0);
    }
    s_ds = wave_reduce_d<false>(s_ds);
    s_dl = wave_reduce_d<false>(s_dl);
    s_as = wave_reduce_d<false>(s_as);
    s_as2 = wave_reduce_d<false>(s_as2);
    mx = wave_reduce_d<true>(mx);
    if (me.lane == XM_WAVE - 1) {
      double* p = L.part[me.wave];
      p[0] = s_ds;
      p[1] = s_dl;
      p[2] = s_as;
      p[3] = s_as2;
      p[4] = mx;
    }
  }
  // xm_solver_obj.cpp::acme_combine's formula.  Lane q < 5 adds up quantity q in wave order.
  static SDEV double combine(const SearchLds& L, int n, int lane) {
    double acc = lane == 4 ? -DBL_MAX : 0.;
    if (lane < 5) {
#pragma unroll
      for (int w = 1; w < kWaves; ++w) {
        const double v = L.part[w][lane];
        acc = lane == 4 ? fmax(acc, v) : acc + v;
      }
    }
    const double s_ds = rdlane_d(acc, 0), s_dl = rdlane_d(acc, 1), s_as = rdlane_d(acc, 2), s_as2 = rdlane_d(acc, 3),
                 mx = rdlane_d(acc, 4);
    const double h = log(s_ds) - s_dl / s_ds;  // H = -sum p ln p,  p = ds / S
    const double pfun = s_as < 0. ? s_as2 : 0.;
    return (h + 1000.0 * pfun) / (double)n / mx;
  }
};

// The points of the test scipy's polish starts with -- x, x + h0 e0[, x + h1 e1] -- and the exact steps, by lane 0
// (xm_solver.cpp::xm_solver_fg: approx_derivative "2-point", abs_step 1e-8, bounds-aware steps)
SDEV void gradient_points(SearchLds& L, double x0, double x1, int N) {
  for (int r = 0; r < 3; ++r) {
    L.pts[r][0] = x0;
    L.pts[r][1] = x1;
  }
  for (int i = 0; i < N; ++i) {
    const double xc = i == 0 ? x0 : x1, lb = i == 0 ? kLo0 : kLo1, ub = i == 0 ? kHi0 : kHi1;
    double step = 1e-8;
    if ((xc + step) - xc == 0.0) step = 1.4901161193847656e-08 * (xc >= 0.0 ? 1.0 : -1.0) * fmax(1.0, fabs(xc));
    const double lower = xc - lb, upper = ub - xc;
    const double xt = xc + step;
    const bool violated = xt < lb || xt > ub;
    const bool fitting = fabs(step) <= fmax(lower, upper);
    if (violated && fitting) step = -step;
    if (!fitting) step = upper >= lower ? upper : -lower;
    const double pnt = xc + step;
    L.pts[1 + i][i] = pnt;
    L.dx[i] = pnt - xc;
  }
}

// ... and what the test compares with pgtol, from the scores at those points
SDEV double projected_gradient_norm(const SearchLds& L, double x0, double x1, int N) {
  double pgn = 0.;
  for (int i = 0; i < N; ++i) {
    const double xi = i == 0 ? x0 : x1, lb = i == 0 ? kLo0 : kLo1, ub = i == 0 ? kHi0 : kHi1;
    const double g = (L.vals[1 + i] - L.vals[0]) / L.dx[i];
    const double pg = g < 0. ? fmax(xi - ub, g) : fmin(xi - lb, g);  // L-BFGS-B's projgr, both bounds set
    pgn = fmax(pgn, fabs(pg));
  }
  return pgn;
}

enum { PH_LIST = 0, PH_INIT = 1, PH_TRIAL = 2, PH_GRAD = 3 };  // what an evaluation is for

// Wave 0's registers and steps: xm_solver.cpp::xm_solver_de, statement for statement.  Every value is wave-uniform
// unless it is "one per lane".
struct Optimiser {
  SearchLds& L;
  const SearchArgs& A;
  const int lane, N, M;  // dimensions of the search; M = max(5, popsize * N) members
  Rng rng;
  double px0 = 0., px1 = 0., en = DBL_MAX;  // one population member per lane (lanes >= M: unused)
  int ridx;                                 // one per lane: _random_population_index
  int nfev = 0, nit = 1, status = 1;
  double scl = 0., scl_next = 0., tr0 = 0., tr1 = 0.;  // the generation's dither, the next one's; the trial
  double x0 = 0., x1 = 0., fun = 0.;                   // the best member when the generations end, in degrees
  Drawn dr = {0, 0, 0, {false, false}};

  SDEV Optimiser(SearchLds& L_, const SearchArgs& A_, int lane_)
      : L(L_), A(A_), lane(lane_), N(A_.p0_only ? 1 : 2), M(15 * N), rng{&L_, 0u, 0, XM_WAVE}, ridx(lane_) {}

  SDEV void init_population() {  // init_population_lhs
    XM_LDS_ORDER();  // (the seeded state, copied on entry)
    rng.start(lane);
    const double seg = 1.0 / (double)M;
    for (int i = 0; i < M; ++i)
      for (int j = 0; j < N; ++j) {
        const double v = seg * rng.next_double(lane) + (double)i * (1.0 / (double)M);
        if (lane == 0) L.lhs[i][j] = v;
      }
    XM_LDS_ORDER();
    for (int j = 0; j < N; ++j) {
      const int order = rng.shuffle(lane, M, lane);  // rng.permutation(range(M))
      const double v = lane < M ? L.lhs[order][j] : 0.;
      if (j == 0)
        px0 = v;
      else
        px1 = v;
    }
  }
  SDEV void promote() {  // _promote_lowest_energy: first arg-min to slot 0
    double m = lane < M ? en : DBL_MAX;
    for (int s = 1; s < XM_WAVE; s <<= 1) m = fmin(m, __shfl_xor(m, s));
    const unsigned long long hit = __ballot(lane < M && en == m);
    const int l = hit ? (int)__builtin_ctzll(hit) : 0;
    if (l != 0) {
      const double a0 = rdlane_d(px0, 0), a1 = rdlane_d(px1, 0), ae = rdlane_d(en, 0);
      const double b0 = rdlane_d(px0, l), b1 = rdlane_d(px1, l), be = rdlane_d(en, l);
      if (lane == 0) {
        px0 = b0;
        px1 = b1;
        en = be;
      } else if (lane == l) {
        px0 = a0;
        px1 = a1;
        en = ae;
      }
    }
  }
  SDEV void draw(int cand) {  // _mutate's random part: fill point, _select_samples, crossover mask -> dr
    dr.fill = N > 1 ? (int)rng.interval((unsigned)(N - 1), lane) : 0;
    ridx = rng.shuffle(ridx, M, lane);
    const int a0 = __builtin_amdgcn_readlane(ridx, 0), a1 = __builtin_amdgcn_readlane(ridx, 1),
              a2 = __builtin_amdgcn_readlane(ridx, 2);
    if (a0 == cand) {
      dr.r0 = a1;
      dr.r1 = a2;
    } else if (a1 == cand) {
      dr.r0 = a0;
      dr.r1 = a2;
    } else {
      dr.r0 = a0;
      dr.r1 = a1;
    }
    dr.cross[0] = rng.next_double(lane) < 0.7;
    dr.cross[1] = N > 1 ? rng.next_double(lane) < 0.7 : false;
    if (dr.fill == 0)
      dr.cross[0] = true;
    else
      dr.cross[1] = true;
  }
  // While the workers sum trial idx: the next trial's random part (a new generation's dither comes first)
  SDEV void draw_ahead(int idx) {
    if (idx + 1 < M) {
      draw(idx + 1);
    } else {
      scl_next = 0.5 + (1.0 - 0.5) * rng.next_double(lane);  // dither: rng.uniform(0.5, 1)
      draw(0);
    }
  }
  // Names evaluation `idx` of `phase`: the point in degrees; true when there is none left (n_eval: the list's length)
  SDEV bool next_point(int phase, int idx, int n_eval, double& p0d, double& p1d) {
    bool fin = false;
    if (phase == PH_LIST) {
      fin = idx >= n_eval;
      if (!fin) {
        p0d = A.xs[2 * idx];
        p1d = A.p0_only ? 0. : A.xs[2 * idx + 1];
      }
    } else if (phase == PH_INIT) {  // initial energies
      p0d = degrees0(rdlane_d(px0, idx));
      p1d = N > 1 ? degrees1(rdlane_d(px1, idx)) : 0.;
    } else if (phase == PH_TRIAL) {
      // _mutate (best1bin) + _ensure_constraint on the population as it stands now
      const int c = idx;
      const double b0 = rdlane_d(px0, 0) + scl * (rdlane_d(px0, dr.r0) - rdlane_d(px0, dr.r1));
      const double b1 = rdlane_d(px1, 0) + scl * (rdlane_d(px1, dr.r0) - rdlane_d(px1, dr.r1));
      tr0 = dr.cross[0] ? b0 : rdlane_d(px0, c);
      tr1 = N > 1 ? (dr.cross[1] ? b1 : rdlane_d(px1, c)) : 0.;
      if (tr0 > 1 || tr0 < 0) tr0 = rng.next_double(lane);
      if (N > 1 && (tr1 > 1 || tr1 < 0)) tr1 = rng.next_double(lane);
      p0d = degrees0(tr0);
      p1d = N > 1 ? degrees1(tr1) : 0.;
    } else {  // PH_GRAD: x, x + h0 e0[, x + h1 e1]
      fin = idx > N;
      if (!fin) {
        p0d = L.pts[idx][0];
        p1d = L.pts[idx][1];
      }
    }
    return fin;
  }
  // converged()?  std(energies) <= atol + tol * |mean(energies)|
  SDEV bool converged() {
    if (lane < M) L.en[lane] = en;
    XM_LDS_ORDER();
    bool any_inf = false;
    for (int i = 0; i < M; ++i) any_inf |= !(fabs(L.en[i]) <= 1.79769313486231570815e308);
    bool stop = false;
    if (!any_inf) {
      const double mean = np_sum_small(L.en, M) / (double)M;
      if (lane < M) L.dv[lane] = (en - mean) * (en - mean);
      XM_LDS_ORDER();
      const double sd = sqrt(np_sum_small(L.dv, M) / (double)M);
      stop = sd <= A.tol * fabs(mean);
    }
    return stop;
  }
  // Takes the score f of evaluation `idx` of `phase` -- accept or reject, the end of a generation, the end of the
  // generations -- and moves both on to the next evaluation.
  SDEV void take_score(int& phase, int& idx, double f) {
    if (phase == PH_LIST) {
      if (lane == 0) A.fs[idx] = f;
      ++idx;
    } else if (phase == PH_INIT) {
      if (lane == idx) en = f;
      ++nfev;
      if (++idx == M) {
        promote();
        scl = 0.5 + (1.0 - 0.5) * rng.next_double(lane);
        draw(0);
        phase = PH_TRIAL;
        idx = 0;
      }
    } else if (phase == PH_TRIAL) {
      const int c = idx;
      ++nfev;
      if (f <= rdlane_d(en, c)) {
        if (lane == c) {
          px0 = tr0;
          px1 = tr1;
          en = f;
        }
        if (f <= rdlane_d(en, 0)) promote();
      }
      if (++idx == M) {  // end of a generation
        const bool stop = converged();
        if (stop) status = 0;
        if (stop || nit >= A.maxiter) {  // on to the polish's test at the best member
          x0 = degrees0(rdlane_d(px0, 0));
          x1 = N > 1 ? degrees1(rdlane_d(px1, 0)) : 0.;
          fun = rdlane_d(en, 0);
          if (lane == 0) gradient_points(L, x0, x1, N);
          XM_LDS_ORDER();
          phase = PH_GRAD;
          idx = 0;
        } else {
          ++nit;
          scl = scl_next;  // drawn, with candidate 0's random part, while the generation's last trial was summed
          idx = 0;
        }
      }
    } else {  // PH_GRAD
      if (lane == 0) L.vals[idx] = f;
      ++idx;
    }
  }
};

// The fields xm_search_result and xm_search_row share
template <class Rec>
SDEV void fill_record(Rec* o, double x0, double x1, double fun, double pg_norm, int nfev, int nit, int status,
                      int target_idx) {
  o->x[0] = x0;
  o->x[1] = x1;
  o->fun = fun;
  o->pg_norm = pg_norm;
  o->nfev = nfev;
  o->nit = nit;
  o->status = status;
  // (NaN only in a row without a search -- nothing to polish; projected_gradient_norm's fmax never hands one back)
  o->needs_polish = pg_norm > 0.5e-5 ? 1 : 0;
  o->target_idx = target_idx;
  o->pad_ = 0;
}

// Where a search's time goes (wave 0's view, ticks of the 100 MHz wall clock): naming the point, the tables, the
// overlapped draw, waiting for the workers' sums, taking the score.  ON = false (the compact record carries no
// timings): nothing.
template <bool ON>
struct Laps {
  unsigned long long tk[5] = {0, 0, 0, 0, 0}, t0 = wall_clock64(), start = t0;
  SDEV void lap(int which) {
    const unsigned long long now = wall_clock64();
    tk[which] += now - t0;
    t0 = now;
  }
  SDEV void report(double* t_us) const {
    for (int i = 0; i < 5; ++i) t_us[i] = 0.01 * (double)tk[i];
    t_us[5] = 0.01 * (double)(wall_clock64() - start);
    t_us[6] = t_us[7] = 0.;
  }
};
template <>
struct Laps<false> {
  SDEV void lap(int) {}
};

// One search by one workgroup: the body of both kernels below.  `load(k)` gives bin k of the spectrum as complex128.
// ROWS (k_search_rows): the record goes to `row_out` in plain device memory, A.pivot (not NaN) replaces the arg-max's
// coordinate as the pivot (with A.target_idx as the target bin), and a row that has no search -- all bins zero, or a
// sample that is not finite: the ACME score is 0/0 there -- ends before the first evaluation.  Everything the search
// keeps (MT19937 state, stop word, tables, the optimiser's registers) is set up anew on entry, so the result is a pure
// function of the row's samples.
template <int P, bool FULL, bool ROWS, class Load>
SDEV void search_body(SearchLds& L, const SearchArgs& A, Load load, xm_search_row* row_out) {
  const int t = (int)threadIdx.x, lane = t & (XM_WAVE - 1), wave = t / XM_WAVE;
  const bool worker = wave > 0;
  const Role me = {lane, wave, worker, t - XM_WAVE, (t - XM_WAVE) * P};
  const int n_eval = ROWS ? 0 : A.n_eval;     // (the rows have no evaluation mode)
  Objective<P, FULL> obj;
  obj.n = A.n;
  if (worker) {
    load_bins<P>(load, me.k0, A.n, obj.re, obj.im);
  } else {
    for (int i = lane; i < 624; i += XM_WAVE) L.mt[i] = A.mt0[i];
    if (lane == 0) L.stop = 0;
  }
  int kwin = A.target_idx;  // >= 0: given
  if (ROWS || kwin < 0) {
    const ArgMax am = first_argmax<P, ROWS>(L, me, obj.re, obj.im, A.n);
    if constexpr (ROWS) {
      if (am.bad || am.zero) {
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        const int status = am.bad ? XM_SEARCH_NOT_FINITE : XM_SEARCH_ALL_ZERO;
        if (t == 0) fill_record(row_out, nan, nan, nan, nan, 0, 0, status, am.bad ? -1 : am.bin);
        return;
      }
    }
    if (!ROWS || kwin < 0) kwin = am.bin;
  }
  __syncthreads();
  const double pivot = ROWS && A.pivot == A.pivot ? A.pivot : A.c0 + A.cstep * (double)kwin;
  obj.u0 = (A.c0 - pivot) / A.x_range;
  obj.du = A.cstep / A.x_range;
  const double kRad = 3.14159265358979323846 / 180.0;  // np.radians

  Optimiser opt(L, A, lane);
  Laps<!ROWS> laps;
  int phase = n_eval > 0 ? PH_LIST : PH_INIT, idx = 0;
  if (!worker && phase == PH_INIT) opt.init_population();

  // ---- ONE loop, one evaluation per turn: wave 0 names the point (or ends the search), the workers' tables and sums,
  // wave 0 takes the score.  While the workers sum, wave 0 draws the random part of the NEXT trial.
  for (;;) {
    if (!worker) {
      double p0d = 0., p1d = 0.;
      const bool fin = opt.next_point(phase, idx, n_eval, p0d, p1d);
      if (lane == 0) {
        L.stop = fin ? 1 : 0;
        L.prm[0] = p0d * kRad;
        L.prm[1] = p1d * kRad;
      }
      laps.lap(0);
    }
    __syncthreads();
    if (L.stop) break;
    obj.tables(L, me);
    __syncthreads();
    if (!worker) laps.lap(1);
    if (worker)
      obj.partial_sums(L, me);
    else if (phase == PH_TRIAL)
      opt.draw_ahead(idx);
    if (!worker) laps.lap(2);
    __syncthreads();
    if (!worker) {
      laps.lap(3);
      opt.take_score(phase, idx, Objective<P, FULL>::combine(L, A.n, lane));
      laps.lap(4);
    }
  }

  if (t != 0) return;
  if constexpr (ROWS) {
    fill_record(row_out, opt.x0, opt.x1, opt.fun, projected_gradient_norm(L, opt.x0, opt.x1, opt.N), opt.nfev, opt.nit,
                opt.status, kwin);
  } else {
    xm_search_result* o = A.out;
    if (n_eval > 0) {
      if (o) o->target_idx = kwin;
    } else {
      fill_record(o, opt.x0, opt.x1, opt.fun, projected_gradient_norm(L, opt.x0, opt.x1, opt.N), opt.nfev, opt.nit,
                  opt.status, kwin);
      laps.report(o->t_us);
    }
    if (o) {  // the sequence word last
      __threadfence_system();
      __hip_atomic_store((unsigned long long*)&o->seq, A.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

template <int P, bool FULL>
__global__ __launch_bounds__(kThreads) void k_search(SearchArgs A) {
  __shared__ SearchLds L;
  search_body<P, FULL, false>(
      L, A, [&](int k) { return reinterpret_cast<const double2*>(A.in)[k]; }, nullptr);
}

// The same search for every row of in[n_rows, n] (complex64 or complex128, widened to fp64 on load): the grid is the
// workgroups the stream's CUs hold, rows go round by a grid stride, one record per row.
template <int P, bool FULL, class T>
__global__ __launch_bounds__(kThreads) void k_search_rows(SearchArgs A) {
  __shared__ SearchLds L;
  using T2 = typename std::conditional<std::is_same<T, float>::value, float2, double2>::type;
  for (long long row = blockIdx.x; row < A.n_rows; row += gridDim.x) {
    const T2* src = reinterpret_cast<const T2*>(A.in) + row * (long long)A.n;
    search_body<P, FULL, true>(
        L, A,
        [&](int k) {
          const T2 v = src[k];
          return make_double2((double)v.x, (double)v.y);
        },
        A.rec + row);
    __syncthreads();  // the next row's set-up overwrites what a slower wave may still be reading
  }
}

// numpy/random/src/mt19937/mt19937.c mt19937_seed
void mt_seed(unsigned s, unsigned* mt) {
  mt[0] = s;
  for (int i = 1; i < 624; ++i) mt[i] = 1812433253u * (mt[i - 1] ^ (mt[i - 1] >> 30)) + (unsigned)i;
}

std::mutex g_seed_mu;
std::map<std::pair<int, unsigned>, unsigned*> g_seed_tables;  // (device, seed) -> 624 words in device memory

int seed_table(unsigned seed, const unsigned** out) {
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(g_seed_mu);
  auto it = g_seed_tables.find({dev, seed});
  if (it == g_seed_tables.end()) {
    unsigned h[624];
    mt_seed(seed, h);
    unsigned* d = nullptr;
    HIP_TRY(hipMalloc(&d, sizeof(h)));
    HIP_TRY(hipMemcpy(d, h, sizeof(h), hipMemcpyHostToDevice));
    it = g_seed_tables.emplace(std::make_pair(dev, seed), d).first;
  }
  *out = it->second;
  return XM_OK;
}

// f(std::integral_constant<int, P>, slot) with the smallest P of the launch table whose 448 P bins hold n; slot: P's place
// in the table
constexpr int kPoints[] = {1, 2, 3, 5, 10, 19, kMaxP};
constexpr int kSlots = (int)(sizeof(kPoints) / sizeof(kPoints[0]));

template <int SLOT = 0, class F>
int with_points(int n, F f) {
  if constexpr (SLOT == kSlots) {
    return xm_fail(XM_ERR_UNSUPPORTED_N, "device search: at most " + std::to_string(kWorkers * kMaxP) + " bins");
  } else {
    if (n <= kWorkers * kPoints[SLOT]) return f(std::integral_constant<int, kPoints[SLOT]>{}, SLOT);
    return with_points<SLOT + 1>(n, f);
  }
}

int launch(const SearchArgs& A, hipStream_t st) {
  return with_points(A.n, [&](auto p, int) {
    constexpr int P = decltype(p)::value;
    if (A.n == kWorkers * P)
      hipLaunchKernelGGL((k_search<P, true>), dim3(1), dim3(kThreads), 0, st, A);
    else
      hipLaunchKernelGGL((k_search<P, false>), dim3(1), dim3(kThreads), 0, st, A);
    HIP_TRY(hipGetLastError());
    return (int)XM_OK;
  });
}

XmResidency g_rows_residency[kSlots][2][2];  // [P slot][FULL][complex128]

template <int P, bool FULL, class T>
int launch_rows_t(const SearchArgs& A, int slot, hipStream_t st) {
  int resident = 0;
  const int rc = xm_resident_blocks(g_rows_residency[slot][FULL ? 1 : 0][std::is_same<T, double>::value ? 1 : 0],
                                    k_search_rows<P, FULL, T>, kThreads, 0, &resident, st);
  if (rc) return rc;
  const long long grid = A.n_rows < (long long)resident ? A.n_rows : (long long)resident;
  hipLaunchKernelGGL((k_search_rows<P, FULL, T>), dim3((unsigned)grid), dim3(kThreads), 0, st, A);
  HIP_TRY(hipGetLastError());
  return XM_OK;
}

int launch_rows(const SearchArgs& A, int dtype, hipStream_t st) {
  return with_points(A.n, [&](auto p, int slot) {
    constexpr int P = decltype(p)::value;
    const bool full = A.n == kWorkers * P;
    if (dtype == XM_C64)
      return full ? launch_rows_t<P, true, float>(A, slot, st) : launch_rows_t<P, false, float>(A, slot, st);
    return full ? launch_rows_t<P, true, double>(A, slot, st) : launch_rows_t<P, false, double>(A, slot, st);
  });
}

// What the three entry points share: the common argument checks (`own_ok`: the caller's own), then the arguments of a
// plain search -- one spectrum, no evaluation list, pivot and target bin from the arg-max -- for the caller to add to.
int fill_args(SearchArgs& A, const char* entry, bool own_ok, const void* in, int n, double c0, double cstep, double x_range,
              int p0_only, double tol, int maxiter) {
  if (!own_ok || n < 2 || maxiter < 1 || !(x_range > 0.0))
    return xm_fail(XM_ERR_INVALID_ARG, std::string(entry) + ": bad argument");
  A = SearchArgs{};
  A.in = in;
  A.c0 = c0;
  A.cstep = cstep;
  A.x_range = x_range;
  A.tol = tol;
  A.pivot = NAN;
  A.n_rows = 1;
  A.n = n;
  A.p0_only = p0_only ? 1 : 0;
  A.maxiter = maxiter;
  A.target_idx = -1;
  return XM_OK;
}

}  // namespace

extern "C" {

int xm_search_rows_supported(int n, int method, double x_range, int dtype) {
  return (dtype == XM_C64 || dtype == XM_C128) ? xm_search_supported(n, method, x_range) : 0;
}

int xm_search_rows(const void* in, int64_t n_rows, int n, int dtype, double c0, double cstep, double x_range, int p0_only,
                   unsigned seed, double tol, int maxiter, double pivot, int target_idx, xm_search_row* records,
                   void* stream) {
  SearchArgs A;
  const bool own_ok = n_rows >= 0 && (n_rows == 0 || (in && records)) && (dtype == XM_C64 || dtype == XM_C128);
  int rc = fill_args(A, "xm_search_rows", own_ok, in, n, c0, cstep, x_range, p0_only, tol, maxiter);
  if (rc) return rc;
  const bool given = pivot == pivot;
  if (given ? (target_idx < 0 || target_idx >= n) : target_idx >= 0)
    return xm_fail(XM_ERR_INVALID_ARG, "xm_search_rows: a pivot comes with its target index in [0, n), no pivot with -1");
  if (n_rows == 0) return XM_OK;
  if ((rc = seed_table(seed, &A.mt0))) return rc;
  A.rec = records;
  A.pivot = pivot;
  A.n_rows = n_rows;
  A.target_idx = given ? target_idx : -1;
  return launch_rows(A, dtype, (hipStream_t)stream);
}

int xm_search_supported(int n, int method, double x_range) {
  return n >= 2 && method == 0 && n <= kWorkers * kMaxP && x_range > 0.0 ? 1 : 0;
}

int xm_search_launch(const void* slice, int n, double c0, double cstep, double x_range, int method, int p0_only,
                     unsigned seed, double tol, int maxiter, uint64_t seq, xm_search_result* out, void* stream) {
  SearchArgs A;
  int rc = fill_args(A, "xm_search_launch", slice && out, slice, n, c0, cstep, x_range, p0_only, tol, maxiter);
  if (rc) return rc;
  if (method != 0)
    return xm_fail(XM_ERR_INVALID_ARG, "xm_search_launch: only the ACME objective (method 0) runs on the device");
  if ((rc = seed_table(seed, &A.mt0))) return rc;
  A.out = out;
  A.seq = seq;
  return launch(A, (hipStream_t)stream);
}

int xm_search_eval(const void* slice, int n, double c0, double cstep, double x_range, int target_idx, int p0_only,
                   const double* xs, int count, double* fs, void* stream) {
  SearchArgs A;
  int rc = fill_args(A, "xm_search_eval", slice && xs && fs && count >= 1 && target_idx < n, slice, n, c0, cstep, x_range,
                     p0_only, 0.0, 1);
  if (rc) return rc;
  if ((rc = seed_table(42u, &A.mt0))) return rc;
  A.xs = xs;
  A.fs = fs;
  A.n_eval = count;
  A.target_idx = target_idx;
  return launch(A, (hipStream_t)stream);
}

}  // extern "C"
