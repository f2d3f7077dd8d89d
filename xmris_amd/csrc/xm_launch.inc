// Kernel instantiation + dispatch for one storage precision.  Included by xm_launch_f32.hip
// (XM_REAL = float) and xm_launch_f64.hip (XM_REAL = double) so the two compile in parallel.
#include "xm_host.h"
#include "xm_kernels.h"
#include "xm_plans.h"
#include "xm_tables.h"

#include <cmath>
#include <cstdlib>
#include <cstring>

namespace {

using T = XM_REAL;
constexpr int kDtype = sizeof(T) == 8 ? XM_C128 : XM_C64;

// spectra per workgroup: fill 256 threads, but keep the exchange buffers within 64 KiB so that
// several workgroups stay resident per CU
template <class PL>
constexpr int spb_of() {
  int spb = PL::NT >= 256 ? 1 : 256 / PL::NT;
  const long per = (long)BlockFFT<T, PL>::lds_elems() * (long)sizeof(Cx<T>);
  while (spb > 1 && per * spb > 65536) spb /= 2;
  return spb;
}

template <class PL>
void gen_twiddles(int n, int m, const void* ctx, std::vector<double>& re, std::vector<double>& im) {
  xm_gen_twiddles<PL>(n, m, ctx, re, im);
}

void gen_half(int n, int m, const void* ctx, std::vector<double>& re, std::vector<double>& im) {
  xm_gen_half(n, m, ctx, re, im);
}

void gen_chirp(int n, int, const void*, std::vector<double>& re, std::vector<double>& im) {
  // a[k] = e^{-i pi k^2 / n} = e^{-2 pi i (k^2 mod 2n) / (2n)}
  re.resize(n);
  im.resize(n);
  for (int k = 0; k < n; ++k) xm_unit(((long long)k * k) % (2LL * n), 2LL * n, -1.0, re[k], im[k]);
}

// radix-2 host FFT in double: only for the Bluestein chirp spectrum, once per (n, m)
void host_fft(std::vector<double>& re, std::vector<double>& im) {
  const int n = (int)re.size();
  for (int i = 1, j = 0; i < n; ++i) {
    int bit = n >> 1;
    for (; j & bit; bit >>= 1) j ^= bit;
    j ^= bit;
    if (i < j) {
      std::swap(re[i], re[j]);
      std::swap(im[i], im[j]);
    }
  }
  for (int len = 2; len <= n; len <<= 1)
    for (int i = 0; i < n; i += len)
      for (int k = 0; k < len / 2; ++k) {
        double c, s;
        xm_unit(k, len, -1.0, c, s);
        const int a = i + k, b = i + k + len / 2;
        const double tr = re[b] * c - im[b] * s, ti = re[b] * s + im[b] * c;
        re[b] = re[a] - tr;
        im[b] = im[a] - ti;
        re[a] += tr;
        im[a] += ti;
      }
}

// m = 3 * 2^k: decimation in time by three over the radix-2 transform
void host_fft_any(std::vector<double>& re, std::vector<double>& im) {
  const int m = (int)re.size();
  if ((m & (m - 1)) == 0) return host_fft(re, im);
  const int h = m / 3;
  std::vector<double> sr[3], si[3];
  for (int r = 0; r < 3; ++r) {
    sr[r].resize(h);
    si[r].resize(h);
    for (int j = 0; j < h; ++j) {
      sr[r][j] = re[3 * j + r];
      si[r][j] = im[3 * j + r];
    }
    host_fft(sr[r], si[r]);
  }
  for (int k = 0; k < m; ++k) {
    double ar = 0.0, ai = 0.0;
    for (int r = 0; r < 3; ++r) {
      double c, s;
      xm_unit(((long long)r * k) % m, m, -1.0, c, s);
      const double xr = sr[r][k % h], xi = si[r][k % h];
      ar += xr * c - xi * s;
      ai += xr * s + xi * c;
    }
    re[k] = ar;
    im[k] = ai;
  }
}

void gen_chirp_fft(int n, int m, const void*, std::vector<double>& re, std::vector<double>& im) {
  // FFT_m of b[k] = conj(a[|k|]) wrapped to length m, divided by m (folds the inverse scale)
  std::vector<double> are, aim;
  gen_chirp(n, m, nullptr, are, aim);
  re.assign(m, 0.0);
  im.assign(m, 0.0);
  for (int k = 0; k < n; ++k) {
    re[k] = are[k];
    im[k] = -aim[k];
    if (k) {
      re[m - k] = are[k];
      im[m - k] = -aim[k];
    }
  }
  host_fft_any(re, im);
  for (int i = 0; i < m; ++i) {
    re[i] /= m;
    im[i] /= m;
  }
}

template <class KernelT>
int set_lds(KernelT kern, size_t bytes) {
  if (bytes > 48 * 1024)
    HIP_TRY(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  return XM_OK;
}

enum KernelSel { KS_GENERIC, KS_BLUESTEIN };

template <class PL, int SEL>
int launch_plan(PipeArgs<T> A, hipStream_t st) {
  constexpr int SPB = spb_of<PL>();
  const void* tw = nullptr;
  int rc = xm_table_get(TK_TWIDDLE, PL::N, PL::signature(), kDtype, gen_twiddles<PL>, nullptr, &tw);
  if (rc) return rc;
  A.tw = (const Cx<T>*)tw;
  size_t lds = (size_t)SPB * BlockFFT<T, PL>::lds_elems() * sizeof(Cx<T>);
  const size_t red = ((size_t)(PL::NT * SPB) / XM_WAVE + 2) * (sizeof(T) + sizeof(int));
  if (lds < red) lds = red;
  const long long blocks = (A.n_batch + SPB - 1) / SPB;
  if (blocks <= 0) return XM_OK;
  if (blocks > 0x7fffffffLL) return xm_fail(XM_ERR_INVALID_ARG, "n_batch too large for one launch");
  dim3 grid((unsigned)blocks), block(PL::NT * SPB);
  if constexpr (SEL == KS_GENERIC) {
    rc = set_lds(k_pipe<T, PL, SPB>, lds);
    if (rc) return rc;
    xm_note_kernel("k_pipe", &typeid(PL), sizeof(T) == 4 ? "float" : "double", SPB, -1);
    hipLaunchKernelGGL((k_pipe<T, PL, SPB>), grid, block, lds, st, A);
  } else {
    rc = set_lds(k_bluestein<T, PL, SPB>, lds);
    if (rc) return rc;
    xm_note_kernel("k_bluestein", &typeid(PL), sizeof(T) == 4 ? "float" : "double", SPB, -1);
    hipLaunchKernelGGL((k_bluestein<T, PL, SPB>), grid, block, lds, st, A);
  }
  HIP_TRY(hipGetLastError());
  return XM_OK;
}

// persistent ">= 2x zero-fill" kernel: PL is the plan of the half length; grid = CUs x resident
// workgroups per CU (from the occupancy query, cached), each looping over the spectra
template <class PL, int MODE>
int launch_zf2_mode(PipeArgs<T> A, hipStream_t st) {
  const void* tw = nullptr;
  int rc = xm_table_get(TK_TWIDDLE, PL::N, PL::signature(), kDtype, gen_twiddles<PL>, nullptr, &tw);
  if (rc) return rc;
  A.tw = (const Cx<T>*)tw;
  if (A.n_batch <= 0) return XM_OK;
  constexpr bool PACKED = sizeof(T) == 4;  // must mirror k_zf2
  using V = typename std::conditional<PACKED, typename PairOf<T>::type, T>::type;
  const size_t lds = (size_t)BlockFFT<V, PL>::lds_elems() * sizeof(Cx<V>) +
                     (size_t)HotTw<T, PL>::mid_size() * sizeof(Cx<T>) +
                     ((size_t)PL::NT / XM_WAVE + 2) * (sizeof(T) + sizeof(int));
  static XmResidency res;
  int resident = 0;
  rc = xm_resident_blocks(res, k_zf2<T, PL, MODE>, PL::NT, lds, &resident, st);
  if (rc) return rc;
  long long blocks = A.n_batch < resident ? A.n_batch : resident;
  if constexpr (sizeof(T) == 8 && (MODE & ZF2_WRITE) != 0) {
    // complex128 write modes are HBM bound: rows handed out dynamically, ~96 KiB of traffic per ticket (xm_zf2p.h)
    const long long row_bytes = (long long)sizeof(Cx<T>) * ((long long)A.n_in + 2 * PL::N);
    long long chunk = (98304 + row_bytes - 1) / row_bytes;
    chunk = chunk < 1 ? 1 : (chunk > 64 ? 64 : chunk);
    A.queue_chunk = (int)chunk;
    const long long nchunks = (A.n_batch + chunk - 1) / chunk;
    blocks = nchunks < resident ? nchunks : resident;
    rc = xm_queue_slot(&A.queue);
    if (rc) return rc;
  }
  if constexpr (sizeof(T) == 4 && (MODE & ZF2_AMAX) != 0 && (PL::NT > XM_WAVE)) {
    // value-only maxima are accumulated with one atomic max per wave: the slots start at +0.0
    if (A.amax_value_only) HIP_TRY(hipMemsetAsync(A.absmax2, 0, (size_t)A.n_batch * sizeof(T), st));
  }
  xm_note_kernel("k_zf2", &typeid(PL), sizeof(T) == 4 ? "float" : "double", MODE, -1);
  hipLaunchKernelGGL((k_zf2<T, PL, MODE>), dim3((unsigned)blocks), dim3(PL::NT), lds, st, A);
  HIP_TRY(hipGetLastError());
  return XM_OK;
}

// generic persistent kernel (complex64 only): two spectra per packed lane pair
template <class PL, int MODE>
int launch_fft2_mode(PipeArgs<T> A, hipStream_t st) {
  if constexpr (sizeof(T) == 4) {
    const void* tw = nullptr;
    int rc = xm_table_get(TK_TWIDDLE, PL::N, PL::signature(), kDtype, gen_twiddles<PL>, nullptr, &tw);
    if (rc) return rc;
    A.tw = (const Cx<T>*)tw;
    if (A.n_batch <= 0) return XM_OK;
    using V = typename PairOf<T>::type;
    const size_t lds = (size_t)BlockFFT<V, PL>::lds_elems() * sizeof(Cx<V>) +
                       (size_t)HotTw<T, PL>::mid_lds_size() * sizeof(Cx<T>) +
                       (2 * ((size_t)PL::NT / XM_WAVE) + 4) * (sizeof(T) + sizeof(int));
    static XmResidency res;
    int resident = 0;
    rc = xm_resident_blocks(res, k_fft2<PL, MODE>, PL::NT, lds, &resident, st);
    if (rc) return rc;
    const long long npairs = (A.n_batch + 1) / 2;
    const long long blocks = npairs < resident ? npairs : resident;
    if constexpr ((MODE & ZF2_GKEY) != 0) {  // the "last workgroup out" counter of the key's decoder
      rc = xm_queue_slot(&A.queue);
      if (rc) return rc;
    }
    xm_note_kernel("k_fft2", &typeid(PL), nullptr, MODE, -1);
    hipLaunchKernelGGL((k_fft2<PL, MODE>), dim3((unsigned)blocks), dim3(PL::NT), lds, st, A);
    HIP_TRY(hipGetLastError());
    return XM_OK;
  } else {
    return xm_fail(XM_ERR_INVALID_ARG, "k_fft2 is complex64 only");
  }
}

// scalar persistent kernel (used for complex128)
template <class PL, int MODE>
int launch_fft1_mode(PipeArgs<T> A, hipStream_t st) {
  const void* tw = nullptr;
  int rc = xm_table_get(TK_TWIDDLE, PL::N, PL::signature(), kDtype, gen_twiddles<PL>, nullptr, &tw);
  if (rc) return rc;
  A.tw = (const Cx<T>*)tw;
  if (A.n_batch <= 0) return XM_OK;
  const size_t lds = (size_t)BlockFFT<T, PL>::lds_elems() * sizeof(Cx<T>) +
                     (size_t)HotTw<T, PL>::mid_lds_size() * sizeof(Cx<T>) +
                     ((size_t)PL::NT / XM_WAVE + 2) * (sizeof(T) + sizeof(int));
  static XmResidency res;
  int resident = 0;
  rc = xm_resident_blocks(res, k_fft1<T, PL, MODE>, PL::NT, lds, &resident, st);
  if (rc) return rc;
  const long long blocks = A.n_batch < resident ? A.n_batch : resident;
  xm_note_kernel("k_fft1", &typeid(PL), sizeof(T) == 4 ? "float" : "double", MODE, -1);
  hipLaunchKernelGGL((k_fft1<T, PL, MODE>), dim3((unsigned)blocks), dim3(PL::NT), lds, st, A);
  HIP_TRY(hipGetLastError());
  return XM_OK;
}

// persistent Bluestein kernel: packed pairs for complex64, one spectrum per pass for complex128
template <class PL, int MODE, bool PAIRS = (sizeof(T) == 4)>
int launch_blue_mode(PipeArgs<T> A, hipStream_t st) {
  using V = typename std::conditional<PAIRS, typename PairOf<T>::type, T>::type;
  constexpr int NS = PAIRS ? 2 : 1;
  const void* tw = nullptr;
  int rc = xm_table_get(TK_TWIDDLE, PL::N, PL::signature(), kDtype, gen_twiddles<PL>, nullptr, &tw);
  if (rc) return rc;
  A.tw = (const Cx<T>*)tw;
  if (A.n_batch <= 0) return XM_OK;
  const size_t lds = (size_t)BlockFFT<V, PL>::lds_elems() * sizeof(Cx<V>) +
                     (size_t)HotTw<T, PL>::mid_lds_size() * sizeof(Cx<T>) +
                     NS * ((size_t)PL::NT / XM_WAVE + 2) * (sizeof(T) + sizeof(int));
  static XmResidency res;
  int resident = 0;
  rc = xm_resident_blocks(res, k_blue<V, PL, MODE>, PL::NT, lds, &resident, st);
  if (rc) return rc;
  const long long groups = (A.n_batch + NS - 1) / NS;
  const long long blocks = groups < resident ? groups : resident;
  xm_note_kernel("k_blue", &typeid(PL), sizeof(V) == 8 ? "xm_f2/float" : "double", MODE, -1);
  hipLaunchKernelGGL((k_blue<V, PL, MODE>), dim3((unsigned)blocks), dim3(PL::NT), lds, st, A);
  HIP_TRY(hipGetLastError());
  return XM_OK;
}

// 16384: radix 16 for complex64; complex128 exchanges plane by plane (xm_plans.h)
// convolution length 3072 of the chirp-z kernels: the odd factor last (compute bound: with the seam's 12.4.4.4.4 the
// kernel was 25 % SLOWER than with M = 4096)
using PlanBlue3072 = FftPlan<3072, 256, 4, 4, 4, 4, 12>;
// k_pipe, complex64: the plane-by-plane exchange (68 KiB) and 64 VGPRs leave room for two 1024-thread workgroups per CU,
// one loading / storing while the other transforms: 2.7 -> 3.1 TB/s
using Plan16kPipe = std::conditional<sizeof(T) == 4, SplitPlan<FftPlan<16384, 1024, 8, 8, 8, 8, 4>>, Plan16kD::type>::type;
using Plan16k = std::conditional<sizeof(T) == 4, PlanOf<16384>::type, Plan16kD::type>::type;


// ---- plans by length: f(Tag<PL>{}) for the plan of each family, kNoPlan when it has none ------------------------
template <class PL>
struct Tag {
  using type = PL;
};
constexpr int kNoPlan = 1;  // (XM_OK is 0, errors are negative)

#define XM_TAG_PLAN(N, NT, ...) \
  case N:                       \
    return f(Tag<typename PlanOf<N>::type>{});
#define XM_TAG_ZF2(N, NT, ...) \
  case N:                      \
    return f(Tag<typename Zf2PlanOf<N>::type>{});

template <class F>
int plan_pow2(int n, F&& f) {
  switch (n) {
    XM_PLANS_POW2(XM_TAG_PLAN)
    default: return kNoPlan;
  }
}
template <class F>
int plan_other(int n, F&& f) {
  switch (n) {
    XM_PLANS_OTHER(XM_TAG_PLAN)
    default: return kNoPlan;
  }
}

// k_zf2, half length h.  h = 4096, complex64 (the 4096 -> 8192 roofline shape): 256 threads x 16 points, radices
// 16.16.16 -- two LDS exchanges instead of three (the exchanges run at the ds_write rate), 2 workgroups/CU
template <class F>
int zf2_plan(int h, F&& f) {
  if constexpr (sizeof(T) == 4)
    if (h == 4096) return f(Tag<typename PlanOf<4096>::type>{});
  switch (h) {
    XM_PLANS_ZF2(XM_TAG_ZF2)
    default: return kNoPlan;
  }
}

// k_fft2 (complex64): 3*2^k / 5*2^k with 12 or 20 points per thread, radix-4 stages (2.5x / 1.6x / 2.7x k_pipe)
template <class F>
int fft2_plan(int n, F&& f) {
  if constexpr (sizeof(T) == 4) {
    switch (n) {
      XM_PLANS_ZF2(XM_TAG_ZF2)
      XM_PLANS_FFT2_EXTRA(XM_TAG_ZF2)
      case 768: return f(Tag<typename PlanOf<768>::type>{});
      case 1280: return f(Tag<typename PlanOf<1280>::type>{});
      case 1536: return f(Tag<typename PlanOf<1536>::type>{});  // BASELINE configs[4]: 128 threads x 12 points x 2 spectra
      case 2560: return f(Tag<typename PlanOf<2560>::type>{});
      case 3072: return f(Tag<typename PlanOf<3072>::type>{});
      case 5120: return f(Tag<typename PlanOf<5120>::type>{});
      case 6144: return f(Tag<typename PlanOf<6144>::type>{});
      default: break;
    }
  }
  return kNoPlan;
}

// k_fft1 (complex128).  Measured (1 GiB of rows, read + write): 5.1-5.4 TB/s for 512...4096, 4.9 TB/s for 8192 (k_pipe:
// 3.1-3.6); 512 and 4096 prefer the 8-point plans, 1024 / 2048 / 8192 the 16-point ones
constexpr bool fft1_length(int n) {
  return sizeof(T) == 8 && (n == 512 || n == 1024 || n == 2048 || n == 4096 || n == 8192 || n == 768 || n == 1280 ||
                            n == 1536 || n == 2560 || n == 3072 || n == 5120 || n == 6144);
}
template <class F>
int fft1_plan(int n, F&& f) {
  if constexpr (sizeof(T) == 8) {
    switch (n) {
      case 512: return f(Tag<typename Zf2PlanOf<512>::type>{});
      case 4096: return f(Tag<typename Zf2PlanOf<4096>::type>{});
      case 1024: return f(Tag<typename PlanOf<1024>::type>{});
      case 2048: return f(Tag<typename PlanOf<2048>::type>{});
      case 8192: return f(Tag<typename PlanOf<8192>::type>{});
      case 768: return f(Tag<typename PlanOf<768>::type>{});
      case 1280: return f(Tag<typename PlanOf<1280>::type>{});
      case 1536: return f(Tag<typename PlanOf<1536>::type>{});
      case 2560: return f(Tag<typename PlanOf<2560>::type>{});
      case 3072: return f(Tag<typename PlanOf<3072>::type>{});
      case 5120: return f(Tag<typename PlanOf<5120>::type>{});
      case 6144: return f(Tag<typename PlanOf<6144>::type>{});
      default: break;
    }
  }
  return kNoPlan;
}

// k_pipe: every direct plan (complex128: the lengths k_fft1 does not take, see launch())
template <class F>
int pipe_plan(int n, F&& f) {
  if (n == 16384) return f(Tag<Plan16kPipe>{});
  const int rc = plan_pow2(n, f);
  return rc == kNoPlan ? plan_other(n, f) : rc;
}

// k_blue, convolution lengths 512...4096 and (complex64) 8192.  3072 for n in (1024, 1536]: a quarter fewer flops than
// M = 4096, the same LDS traffic -- measured +5-9 %
template <class F>
int blue_plan(int m, F&& f) {
  if (m == 3072) return f(Tag<PlanBlue3072>{});
  if constexpr (sizeof(T) == 4)
    if (m == 8192) return f(Tag<typename PlanOf<8192>::type>{});
  switch (m) {
    XM_PLANS_ZF2(XM_TAG_ZF2)
    default: return kNoPlan;
  }
}

// k_bluestein: the chirp-z lengths of xm_supported_in_lds
template <class F>
int bluestein_plan(int m, F&& f) {
  if (m == 3072) return f(Tag<PlanBlue3072>{});
  if (m == 16384) return f(Tag<Plan16k>{});
  return plan_pow2(m, f);
}

// ---- the routing decision -----------------------------------------------------------------------------------------
enum Family { F_ZF2P, F_ZF2D, F_ZF2, F_FFT2, F_FFT2_WIDE, F_FFT1, F_PIPE, F_BLUE, F_BLUESTEIN, F_BIG };
constexpr int W = ZF2_WRITE, P = ZF2_PHASE, R = ZF2_RAMP, AM = ZF2_AMAX, VO = ZF2_VALUE_ONLY, K = ZF2_GKEY;

struct Route {
  Family family;
  int n;                          // plan length: the half length (">= 2x zero fill"), the transform or chirp-z length
  int mode;                       // ZF2_* words of the kernel (persistent families)
  bool ramp;                      // the kernel applies the requested ramp itself; otherwise it is expanded into a table
  const char* refuse = nullptr;   // the request has no kernel: why
};

// Which kernel serves a launch.  `req`: ZF2_* words of what the caller asks for -- W output, P phase table, R phase
// ramp, AM per-row maxima, VO value-only maxima, K the launch's arg-max key.  Every special case is spelled out here.
Route route(const void* in, int64_t in_stride, int64_t n_batch, int n_in, int n_out, int pad_left, unsigned flags,
            int req) {
  const bool ramp = req & R, key = req & K;
  // the request with the ramp as a table (run() expands it when there are rows to launch on)
  const int tab = (req & (W | P | AM)) | (ramp && n_batch > 0 ? P : 0);
  const int h = n_out / 2, out_shift = (flags & XM_FFT_SHIFT_OUT) ? n_out / 2 : 0;
  // ">= 2x end zero fill": the upper half of the transform input is structurally zero.  Half length 8192 (128 KB
  // exchange buffer, middle twiddles read from L2): only k_zf2p / k_zf2d have the plan
  bool zf2 = (xm_has_direct_plan(n_out, kDtype) || n_out == 16384) && n_out % 2 == 0 &&
             !(flags & (XM_FFT_SHIFT_IN | XM_FFT_INVERSE)) && pad_left + n_in <= h && h >= 512 &&
             (h <= 4096 || h == 8192) && (h == 8192 || xm_has_pow2_plan(h, kDtype)) && (out_shift == 0 || out_shift == h);
  Route r{F_PIPE, n_out, tab, false};
  if (sizeof(T) == 4 && zf2 && xm_pair_loads_ok(in, in_stride, n_in, pad_left)) {
    r = {F_ZF2P, h, req & (W | P | R | AM), ramp};  // the hot kernel: packed, the ramp in closed form
  } else if (sizeof(T) == 8 && zf2 && !(req & P) && ((req & W) ? (!(req & AM) || (req & VO)) : (req & VO)) &&
             (h == 4096 || (h == 8192 && n_batch > 0))) {
    r = {F_ZF2D, h, req & (W | R | AM | VO | K), ramp};  // complex128: two workgroups per CU, value-only maxima
  } else if (zf2 && h != 8192) {  // (half length 8192 otherwise: unaligned complex64 rows, the other complex128 modes)
    if (sizeof(T) == 8)           // the ramp in closed form; write + maxima: the variant without the index scan
      r = {F_ZF2, h, (req & (W | P | R | AM)) | ((req & W) && (req & VO) ? VO : 0), ramp};
    else
      r = {F_ZF2, h, tab, false};
  } else if (!xm_supported_in_lds(n_out, kDtype)) {
    r = {F_BIG, n_out, tab, false};  // four-step over global memory
  } else if (xm_has_direct_plan(n_out, kDtype)) {
    int nt = 0;  // k_fft2 plans with at most 16 points per thread take the ramp in closed form
    const bool fft2 = n_batch >= 2 && fft2_plan(n_out, [&](auto pl) {
      using PL = typename decltype(pl)::type;
      nt = PL::P <= 16 ? PL::NT : 0;
      return XM_OK;
    }) == XM_OK;
    const bool native = ramp && nt > 0 && !(flags & XM_FFT_INVERSE) && out_shift % nt == 0;
    if (fft2 && n_out == 1536 && !native && (req & W) && !(req & AM))
      r = {F_FFT2_WIDE, n_out, tab, false};  // the plain transform (staged seam): one wave x 24 points, xm_plans.h
    else if (fft2)
      r = {F_FFT2, n_out, native ? req & (W | R | AM | K) : tab, native};
    else if (fft1_length(n_out))
      r = {F_FFT1, n_out, tab, false};
  } else {
    const int m = xm_bluestein_m(n_out);
    const bool blue = n_batch >= 2 && blue_plan(m, [](auto) { return XM_OK; }) == XM_OK;
    r = {blue ? F_BLUE : F_BLUESTEIN, m, tab, false};
  }
  if (!(req & W)) r.mode &= ~P;  // without an output a phase table has nothing to act on: the maxima-only kernels
  if (key && !(r.family == F_ZF2P || r.family == F_ZF2D || (r.family == F_FFT2 && r.ramp)))
    r.refuse = "XM_AMAX_GLOBAL_KEY on this geometry needs xm_pipeline_fused_ramp with an output and at least two rows";
  return r;
}

int pipeline_big(PipeArgs<T> A, hipStream_t st);  // xm_bigfft.inc

// the kernel of a route; `ramp` = {a, b} when the route applies it natively.  (U = T: a template, so that `if constexpr`
// discards the other precision's kernels)
template <class U>
int launch(const Route& r, const PipeArgs<U>& A, const double* ramp, hipStream_t st) {
  int rc = kNoPlan;
  switch (r.family) {
    case F_ZF2P:
      if constexpr (sizeof(U) == 4) return xm_zf2p_launch(r.n, r.mode, A, ramp, st);
      break;
    case F_ZF2D:
      if constexpr (sizeof(U) == 8) return xm_zf2d_launch(r.n, r.mode, A, ramp, st);
      break;
    case F_ZF2:
      rc = zf2_plan(r.n, [&](auto pl) {
        using PL = typename decltype(pl)::type;
        PipeArgs<T> B = A;
        if (r.mode & R) xm_set_ramp<PL, true>(B, ramp);
        auto go = [&](auto m) { return launch_zf2_mode<PL, decltype(m)::value>(B, st); };
        if constexpr (sizeof(T) == 4)
          return xm_with_mode<W | P | AM, W | P, W | AM, W, AM>(r.mode, go);
        else if constexpr (PL::N == 4096)  // (k_zf2d takes the other modes of this half length)
          return xm_with_mode<W | R | AM, W | P | AM | VO, W | P | AM, W | P, W | AM, AM>(r.mode, go);
        else
          return xm_with_mode<W | R | AM | VO, W | R | AM, W | R, W | P | AM | VO, W | AM | VO, W | P | AM, W | P, W | AM,
                              W, AM>(r.mode, go);
      });
      break;
    case F_FFT2:
      rc = fft2_plan(r.n, [&](auto pl) {
        using PL = typename decltype(pl)::type;
        PipeArgs<T> B = A;
        auto go = [&](auto m) { return launch_fft2_mode<PL, decltype(m)::value>(B, st); };
        if constexpr (PL::P <= 16) {
          if (r.mode & R) xm_set_ramp<PL, false>(B, ramp);
          return xm_with_mode<W | R | AM | K, W | R | AM, W | R, W | P | AM, W | P, W | AM, W, AM>(r.mode, go);
        } else {
          return xm_with_mode<W | P | AM, W | P, W | AM, W, AM>(r.mode, go);
        }
      });
      break;
    case F_FFT2_WIDE:
      if constexpr (sizeof(T) == 4)
        return xm_with_mode<W | P, W>(
            r.mode, [&](auto m) { return launch_fft2_mode<typename Plan1536Wide::type, decltype(m)::value>(A, st); });
      break;
    case F_FFT1:
      rc = fft1_plan(r.n, [&](auto pl) {
        return xm_with_mode<W | P | AM, W | P, W | AM, W, AM>(
            r.mode, [&](auto m) { return launch_fft1_mode<typename decltype(pl)::type, decltype(m)::value>(A, st); });
      });
      break;
    case F_PIPE:
      rc = pipe_plan(r.n, [&](auto pl) {
        using PL = typename decltype(pl)::type;
        if constexpr (fft1_length(PL::N)) return kNoPlan;
        else return launch_plan<PL, KS_GENERIC>(A, st);
      });
      break;
    case F_BLUE:
      rc = blue_plan(r.n, [&](auto pl) {
        using PL = typename decltype(pl)::type;
        constexpr bool PAIRS = sizeof(T) == 4 && PL::N != 8192;  // (8192: one spectrum per pass -- a packed pair
                                                                 // would need 1024 threads x 165 VGPRs)
        return xm_with_mode<W | P | AM, W | P, W | AM, W, AM>(
            r.mode, [&](auto m) { return launch_blue_mode<PL, decltype(m)::value, PAIRS>(A, st); });
      });
      break;
    case F_BLUESTEIN:
      rc = bluestein_plan(r.n, [&](auto pl) { return launch_plan<typename decltype(pl)::type, KS_BLUESTEIN>(A, st); });
      break;
    case F_BIG:
      return pipeline_big(A, st);
  }
  return rc == kNoPlan ? xm_fail(XM_ERR_UNSUPPORTED_N, "no plan of length " + std::to_string(r.n)) : rc;
}

// the tables a route reads (half-length rotation, chirps, the ramp expanded into stream-ordered scratch), then its kernel
int run(const Route& r, PipeArgs<T>& A, int n_out, const double* ramp, hipStream_t st) {
  if (r.refuse) return xm_fail(XM_ERR_INVALID_ARG, r.refuse);
  int rc = XM_OK;
  const void *t1 = nullptr, *t2 = nullptr;
  if (r.family == F_ZF2P || r.family == F_ZF2D || r.family == F_ZF2) {
    rc = xm_table_get(TK_HALF, n_out, 0, kDtype, gen_half, nullptr, &t1);
    A.aux = (const Cx<T>*)t1;
  } else if (r.family == F_BLUE || r.family == F_BLUESTEIN) {
    rc = xm_table_get(TK_CHIRP, n_out, r.n, kDtype, gen_chirp, nullptr, &t1);
    if (!rc) rc = xm_table_get(TK_CHIRP_FFT, n_out, r.n, kDtype, gen_chirp_fft, nullptr, &t2);
    A.aux = (const Cx<T>*)t1;
    A.aux2 = (const Cx<T>*)t2;
  }
  if (rc) return rc;
  if (r.ramp || !ramp || A.n_batch <= 0) return launch(r, A, r.ramp ? ramp : nullptr, st);
  void* table = nullptr;
  HIP_TRY(hipMallocAsync(&table, (size_t)n_out * sizeof(Cx<T>), st));
  rc = xm_ramp_table_async(table, n_out, ramp[0], ramp[1], kDtype, st);
  if (rc == XM_OK) {
    A.phase = (const Cx<T>*)table;
    rc = launch(r, A, nullptr, st);
  }
  HIP_TRY(hipFreeAsync(table, st));
  return rc;
}

#include "xm_bigfft.inc"

bool ramp_native(const void* in, int64_t in_stride, int n_in, int n_out, int pad_left, unsigned flags) {
  return route(in, in_stride, 2, n_in, n_out, pad_left, flags, W | R).ramp;
}

// the geometries whose kernel leaves the launch's arg-max in a key (XM_AMAX_GLOBAL_KEY)
bool key_native(const void* in, int64_t in_stride, int n_in, int n_out, int pad_left, unsigned flags) {
  return !route(in, in_stride, 2, n_in, n_out, pad_left, flags, W | R | AM | VO | K).refuse;
}

int pipeline_typed(const void* in, int64_t in_stride, void* out, const void* window, const void* phase,
                   const double* ramp, int64_t n_batch, int n_in, int n_out, int pad_left, unsigned flags,
                   void* absmax2, int32_t* argidx, hipStream_t st) {
  PipeArgs<T> A;
  std::memset(&A, 0, sizeof(A));
  A.in = (const Cx<T>*)in;
  A.out = (Cx<T>*)out;
  A.window = (const T*)window;
  A.phase = (const Cx<T>*)phase;
  A.absmax2 = (T*)absmax2;
  A.argidx = argidx;
  A.in_stride = in_stride;
  A.n_batch = n_batch;
  A.n = n_out;
  A.n_in = n_in;
  A.pad_left = pad_left;
  A.in_shift = (flags & XM_FFT_SHIFT_IN) ? (n_out + 1) / 2 : 0;
  A.out_shift = (flags & XM_FFT_SHIFT_OUT) ? n_out / 2 : 0;
  A.inverse = (flags & XM_FFT_INVERSE) ? 1 : 0;
  A.amax_value_only = (flags & XM_AMAX_VALUE_ONLY) ? 1 : 0;
  if (flags & XM_AMAX_GLOBAL_KEY) {  // checked by the caller: value only, a geometry of key_native
    A.gkey = (unsigned long long*)absmax2;
    A.key_result = (XmKeyResult*)argidx;  // may be NULL: the key is then left for xm_argmax_key_take
    A.argidx = nullptr;
    A.amax_value_only = 1;
  }
  double sc = 1.0;
  if (flags & XM_FFT_ORTHO)
    sc = 1.0 / std::sqrt((double)n_out);
  else if (flags & XM_FFT_INVERSE)
    sc = 1.0 / (double)n_out;
  A.scale = (T)sc;
  const int req = (out ? W : 0) | (phase ? P : 0) | (ramp ? R : 0) | (absmax2 ? AM : 0) |
                  (absmax2 && A.amax_value_only ? VO : 0) | (A.gkey ? K : 0);
  return run(route(in, in_stride, n_batch, n_in, n_out, pad_left, flags, req), A, n_out, ramp, st);
}

}  // namespace
