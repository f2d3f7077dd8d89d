// Host side of xm_shift_time (include/xmris_hip.h); the kernel is in xm_shift.h.
#include "xm_host.h"
#include "xm_plans.h"
#include "xm_shift.h"
#include "xm_tables.h"

#include <string>

static int shift_fail(const std::string& msg) { return xm_fail(XM_ERR_INVALID_ARG, "shift_time: " + msg); }

namespace {
constexpr int kNoPlan = 1;  // (XM_OK is 0, errors are negative)

// rows per workgroup: fill 256 threads, but keep the exchange buffers within 64 KiB (as k_pipe / k_bluestein do)
template <class T, class PL>
constexpr int spb_of() {
  int spb = PL::NT >= 256 ? 1 : 256 / PL::NT;
  const long per = (long)BlockFFT<T, PL>::lds_elems() * (long)sizeof(Cx<T>);
  while (spb > 1 && per * spb > 65536) spb /= 2;
  return spb;
}

// The fused set: f(plan) for every direct in-LDS plan of xm_plans.h, kNoPlan for any other length.  16384 is
// complex64 only: the complex128 plan exchanges plane by plane and two of its transforms in one kernel do not pass the
// resource gate (k_bluestein spills there), so that length takes the staged route.
template <class T, class F>
int shift_plan(int L, F&& f) {
  switch (L) {
#define XM_CASE(N, NT, ...) \
  case N:                   \
    return f((typename PlanOf<N>::type*)nullptr);
    XM_PLANS_POW2(XM_CASE)
    XM_PLANS_OTHER(XM_CASE)
#undef XM_CASE
    case 16384:
      if constexpr (sizeof(T) == 4) return f((typename PlanOf<16384>::type*)nullptr);
      return kNoPlan;
    default:
      return kNoPlan;
  }
}

template <class T, class PL>
int shift_launch(ShiftArgs<T> A, hipStream_t st) {
  constexpr int SPB = spb_of<T, PL>();
  const void* tw = nullptr;
  int rc = xm_table_get(TK_TWIDDLE, PL::N, PL::signature(), sizeof(T) == 8 ? XM_C128 : XM_C64, xm_gen_twiddles<PL>,
                        nullptr, &tw);
  if (rc) return rc;
  A.tw = (const Cx<T>*)tw;
  const size_t lds = (size_t)SPB * BlockFFT<T, PL>::lds_elems() * sizeof(Cx<T>);
  if (lds > 48 * 1024)
    HIP_TRY(hipFuncSetAttribute((const void*)k_shift_time<T, PL, SPB>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)lds));
  const long long blocks = (A.n_rows + SPB - 1) / SPB;  // <= 2^31 - 1: checked by the caller
  xm_note_kernel("k_shift_time", &typeid(PL), sizeof(T) == 4 ? "float" : "double", SPB, -1);
  hipLaunchKernelGGL((k_shift_time<T, PL, SPB>), dim3((unsigned)blocks), dim3(PL::NT * SPB), lds, st, A);
  HIP_TRY(hipGetLastError());
  return XM_OK;
}

template <class T>
int shift_typed(const void* in, int64_t in_row_stride, void* out, int64_t n_rows, int n, int L, const double* frac,
                int64_t n_delay, int64_t delay_div, hipStream_t st) {
  ShiftArgs<T> A{};
  A.in = (const Cx<T>*)in;
  A.out = (Cx<T>*)out;
  A.frac = frac;
  A.in_stride = in_row_stride;
  A.n_rows = n_rows;
  A.n_delay = n_delay;
  A.delay_div = delay_div;
  A.n = n;
  return shift_plan<T>(L, [&](auto* pl) {
    return shift_launch<T, typename std::remove_pointer<decltype(pl)>::type>(A, st);
  });
}
}  // namespace

extern "C" int xm_shift_time_fused(int L, int dtype) {
  if (dtype != XM_C64 && dtype != XM_C128) return 0;
  auto yes = [](auto*) { return XM_OK; };
  return (dtype == XM_C64 ? shift_plan<float>(L, yes) : shift_plan<double>(L, yes)) == XM_OK ? 1 : 0;
}

extern "C" int xm_shift_time(const void* in, int64_t in_row_stride, void* out, int64_t n_rows, int n, int L,
                             const double* frac, int64_t n_delay, int64_t delay_div, int dtype, void* stream) {
  if (dtype != XM_C64 && dtype != XM_C128) return shift_fail("unknown dtype " + std::to_string(dtype));
  if (n < 1 || L < n) return shift_fail("needs 1 <= n <= L");
  if (!xm_shift_time_fused(L, dtype)) return shift_fail("L = " + std::to_string(L) + " has no fused kernel");
  if (n_rows < 0 || n_delay < 1 || delay_div < 1) return shift_fail("needs n_rows >= 0, n_delay >= 1 and delay_div >= 1");
  if (in_row_stride < n) return shift_fail("in_row_stride must be at least n");
  if (!in || !out || !frac) return shift_fail("null pointer");
  if (in == out) return shift_fail("out must not be in");
  const size_t elem = dtype == XM_C64 ? 8 : 16;
  if (((reinterpret_cast<size_t>(in) | reinterpret_cast<size_t>(out)) & (elem - 1)) || (reinterpret_cast<size_t>(frac) & 7))
    return shift_fail("in and out must be aligned to their element size, frac to 8 bytes");
  if (n_rows > 0x7fffffffLL) return shift_fail("too many rows (> 2^31 - 1)");
  if (n_rows == 0) return XM_OK;

  DeviceGuard guard(in);
  hipStream_t st = (hipStream_t)stream;
  return dtype == XM_C64 ? shift_typed<float>(in, in_row_stride, out, n_rows, n, L, frac, n_delay, delay_div, st)
                         : shift_typed<double>(in, in_row_stride, out, n_rows, n, L, frac, n_delay, delay_div, st);
}
