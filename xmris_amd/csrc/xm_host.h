// Host-side declarations shared by the translation units of libxmris_hip.so.
#pragma once
#include <cstdlib>
#include "../../include/xmris_hip.h"
#include "xm_common.h"

#include <cmath>
#include <map>
#include <mutex>
#include <string>
#include <type_traits>
#include <utility>
#include <typeinfo>
#include <vector>

int xm_fail(int code, const std::string& msg);
#define HIP_TRY(expr)                                                                \
  do {                                                                               \
    hipError_t e_ = (expr);                                                          \
    if (e_ != hipSuccess) {                                                          \
      (void)hipGetLastError(); /* clear the sticky error: the next call starts clean */ \
      return xm_fail(XM_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    }                                                                                \
  } while (0)

// The library keys its table cache, occupancy caches and scratch on the CURRENT device; the caller's buffers decide
// which device that has to be.  Entry points that launch kernels make the device of their (device-memory) input
// current for the duration of the call.
struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(const void* dev_ptr) {
    if (!dev_ptr) return;
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, dev_ptr) != hipSuccess) {
      (void)hipGetLastError();
      return;
    }
    if (at.type != hipMemoryTypeDevice) return;
    int cur = 0;
    if (hipGetDevice(&cur) != hipSuccess) return;
    if (cur != at.device && hipSetDevice(at.device) == hipSuccess) prev = cur;
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

enum XmTableKind { TK_TWIDDLE = 0, TK_HALF = 1, TK_CHIRP = 2, TK_CHIRP_FFT = 3, TK_BIG_WN = 4 };

// Cached device table (kind, n, m, dtype, current device).  `gen` fills re/im in fp64 when the table
// does not exist yet; it is rounded once to the storage precision and uploaded.
typedef void (*xm_table_gen)(int n, int m, const void* ctx, std::vector<double>& re, std::vector<double>& im);
int xm_table_get(int kind, int n, int m, int dtype, xm_table_gen gen, const void* ctx, const void** out);

// e^{sign * 2 pi i * num/den} with the range reduction done on the integers
void xm_unit(long long num, long long den, double sign, double& c, double& s);

bool xm_has_direct_plan(int n, int dtype);
bool xm_has_pow2_plan(int n, int dtype);
int xm_bluestein_m(int n);
bool xm_supported(int n, int dtype);

// defined in xm_launch_f32.hip / xm_launch_f64.hip.  `ramp`: nullptr, or {phase0, dphase} in radians -- the output is
// multiplied by e^{i (phase0 + dphase k)}, k = output index (then `phase` must be nullptr)
int xm_pipeline_f32(const void* in, int64_t in_stride, void* out, const void* window, const void* phase,
                    const double* ramp, int64_t n_batch, int n_in, int n_out, int pad_left, unsigned flags,
                    void* absmax2, int32_t* argidx, hipStream_t st);
int xm_pipeline_f64(const void* in, int64_t in_stride, void* out, const void* window, const void* phase,
                    const double* ramp, int64_t n_batch, int n_in, int n_out, int pad_left, unsigned flags,
                    void* absmax2, int32_t* argidx, hipStream_t st);
// 1 when length n has a path beyond the in-LDS plans (four-step over global memory, xm_bigfft.inc)
int xm_big_supported_f32(int n);
int xm_big_supported_f64(int n);
// ... and whether it has an in-LDS path (direct plan or chirp-z inside the LDS)
bool xm_supported_in_lds(int n, int dtype);
// 1 when a geometry has a kernel that applies the ramp natively (no table is built), else 0
int xm_ramp_native_f32(const void* in, int64_t in_stride, int n_in, int n_out, int pad_left, unsigned flags);
int xm_ramp_native_f64(const void* in, int64_t in_stride, int n_in, int n_out, int pad_left, unsigned flags);
// ... and whether it leaves the launch's arg-max in a key (XM_AMAX_GLOBAL_KEY)
int xm_key_native_f32(const void* in, int64_t in_stride, int n_in, int n_out, int pad_left, unsigned flags);
int xm_key_native_f64(const void* in, int64_t in_stride, int n_in, int n_out, int pad_left, unsigned flags);

// xm_launch_zf2p.hip: guess stage of the speculative schedule (xm_guess_* in xmris_hip.h)
template <class T>
struct PipeArgs;  // xm_kernels.h
// xm_launch_zf2p.hip / xm_launch_zf2d.hip: the packed complex64 and the complex128 ">= 2x zero fill" kernels of half
// length h, `mode` = ZF2_* words as route() (xm_launch.inc) decides them, `ramp` = {a, b} when mode has ZF2_RAMP
int xm_zf2p_launch(int h, int mode, const PipeArgs<float>& A, const double* ramp, hipStream_t st);
int xm_zf2d_launch(int h, int mode, const PipeArgs<double>& A, const double* ramp, hipStream_t st);
int xm_zf2p_guess_supported(const void* in, int64_t in_stride, int n_in, int n_out, int pad_left, unsigned flags, int dtype);
int xm_zf2p_guess_rows(const void* in, int64_t in_stride, const float* window, int64_t n_batch, int n_in, int n_out,
                       int n_guess, float scale, float* est, unsigned long long* key, int dtype, hipStream_t st);
int xm_zf2p_guess_refine(const void* in, int64_t in_stride, const float* window, int64_t n_batch, int n_in, int n_out,
                         unsigned flags, float scale, const float* est, unsigned long long* guess_key, float band,
                         unsigned long long* work_key, float* out_max2, long long* out_flat, void* out_row, int dtype,
                         hipStream_t st);

// {head, done} counter pair (zero) for one launch of a persistent kernel that hands out rows dynamically; the
// kernel's last workgroup leaves it zero again.  Slots come from a per-device ring of 1024.
int xm_queue_slot(unsigned** out);

// e^{i (phase0 + dphase k)}, k < n, into `table` (device, storage precision of `dtype`), fp64 sincos per entry
int xm_ramp_table_async(void* table, int n, double phase0, double dphase, int dtype, hipStream_t st);

// CUs a stream may use: the population count of its CU mask (all CUs for an ordinary stream; xm_stream_create makes
// streams with a partition of the chip).  Cached per stream handle.
extern "C" int xm_stream_cu_count(hipStream_t st, int* cus);  // (C linkage: defined among the ABI functions)

// Grid of a persistent kernel = CUs of its stream x resident workgroups per CU, at most `max_per_cu` when that is > 0
// (streaming kernels that want few, deep streams).  The occupancy query runs once per kernel instantiation, device and
// dynamic LDS size, under a lock (the launchers are re-entrant); the dynamic-LDS opt-in follows the largest size asked.
struct XmResidency {
  std::mutex mu;
  std::map<std::pair<int, size_t>, int> blocks;  // (device, dynamic LDS bytes) -> resident workgroups per CU
  size_t opt_in[16] = {0};                       // dynamic LDS bytes opted in per device
};
template <class K>
int xm_resident_blocks(XmResidency& r, K kern, int nt, size_t lds, int* out, hipStream_t st = nullptr, int max_per_cu = 0) {
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  if (dev < 0 || dev >= 16) return xm_fail(XM_ERR_INVALID_ARG, "device ordinal out of range");
  int per_cu = 0;
  {
    std::lock_guard<std::mutex> lk(r.mu);
    if (lds > 48 * 1024 && lds > r.opt_in[dev]) {
      HIP_TRY(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      r.opt_in[dev] = lds;
    }
    auto it = r.blocks.find({dev, lds});
    if (it == r.blocks.end()) {
      int q = 0;
      HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&q, kern, nt, lds));
      it = r.blocks.emplace(std::make_pair(dev, lds), q < 1 ? 1 : q).first;
    }
    per_cu = it->second;
  }
  if (max_per_cu > 0 && per_cu > max_per_cu) per_cu = max_per_cu;
  int cus = 0;
  const int rc = xm_stream_cu_count(st, &cus);
  if (rc) return rc;
  *out = per_cu * cus;
  return XM_OK;
}

// Calls f(std::integral_constant<int, MODE>) for the one MODE of Ms equal to the runtime `mode`: Ms lists the ZF2_* mode
// words a kernel family is built with, so a request outside them is an error, never a silent fall-back.
template <int... Ms, class F>
int xm_with_mode(int mode, F&& f) {
  int rc = XM_OK;
  const bool hit = ((mode == Ms ? (rc = f(std::integral_constant<int, Ms>{}), true) : false) || ...);
  return hit ? rc : xm_fail(XM_ERR_INVALID_ARG, "no kernel built for mode " + std::to_string(mode));
}

// Wave-uniform factors of the kernels that apply the linear phase e^{i (a + b k)} natively: ramp_c[2q], ramp_c[2q+1] =
// e^{i (a + b base_q)} with base_q = M NT q + (output roll) mod M N -- M = 2 for the paired half-length transforms
// (outputs 2t and 2t + 1 of a thread; ramp_e = e^{i b} for the odd bins), M = 1 for k_fft2.  `ramp` = {a, b}.
template <class PL, bool PAIRED, class Args>
void xm_set_ramp(Args& A, const double* ramp) {
  using R = typename std::remove_reference<decltype(A.ramp_c[0])>::type;
  constexpr long long M = PAIRED ? 2 : 1;
  for (int q = 0; q < PL::P; ++q) {
    const long long base = (M * PL::NT * q + A.out_shift) % (M * PL::N);
    const double a = ramp[0] + ramp[1] * (double)base;
    A.ramp_c[2 * q] = (R)std::cos(a);
    A.ramp_c[2 * q + 1] = (R)std::sin(a);
  }
  if (PAIRED) {
    A.ramp_e[0] = (R)std::cos(ramp[1]);
    A.ramp_e[1] = (R)std::sin(ramp[1]);
  }
  A.ramp_db = ramp[1];
  A.phase = nullptr;
}

// complex64 pair loads: every (even, odd) sample pair of a row is one aligned 16-byte word
inline bool xm_pair_loads_ok(const void* in, int64_t in_stride, int n_in, int pad_left) {
  return (pad_left % 2 == 0) && (n_in % 2 == 0) && (in_stride % 2 == 0) && ((reinterpret_cast<size_t>(in) & 15u) == 0);
}

// What the dispatcher launched last on this thread, as the profiler names it (`xm_last_kernel_string`): the fused
// launchers note the kernel template, its plan and its mode words right before the launch -- reports quote this
// instead of a string typed by hand.
void xm_note_kernel(const char* base, const std::type_info* plan, const char* scalar, int mode, int opt);

// One launch of a persistent per-item kernel (the row ticket of xm_wg.h): zeroes the counter pair A.counter, sizes the
// grid to min(n_items, resident workgroups of the stream), notes the kernel as <name><form, mode, opt> and launches it.
template <class K, class Args>
int xm_launch_items(XmResidency& res, K kern, int nt, size_t lds, long long n_items, const Args& A, hipStream_t st,
                    const char* name, const char* form, int mode, int opt) {
  HIP_TRY(hipMemsetAsync(A.counter, 0, 2 * sizeof(unsigned), st));
  int resident = 0;
  if (const int rc = xm_resident_blocks(res, kern, nt, lds, &resident, st)) return rc;
  const long long blocks = n_items < resident ? n_items : resident;
  xm_note_kernel(name, nullptr, form, mode, opt);
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(nt), lds, st, A);
  HIP_TRY(hipGetLastError());
  return XM_OK;
}
