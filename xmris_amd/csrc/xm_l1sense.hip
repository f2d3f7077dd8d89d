// Host side of xm_l1_start / xm_l1_prox (include/xmris_hip.h); the kernels are in xm_l1sense.h.
#include "xm_host.h"
#include "xm_l1sense.h"

#include <initializer_list>
#include <string>

namespace {
int l1_fail(const char* who, const std::string& msg) { return xm_fail(XM_ERR_INVALID_ARG, std::string(who) + ": " + msg); }

struct Ptr {
  const void* p;
  size_t align;
};

// non-null pointers aligned to their element, no output among the inputs or twice among the outputs
int l1_pointers(const char* who, std::initializer_list<Ptr> in, std::initializer_list<Ptr> out) {
  for (const std::initializer_list<Ptr>* l : {&in, &out})
    for (const Ptr& a : *l) {
      if (!a.p) return l1_fail(who, "null pointer");
      if (reinterpret_cast<size_t>(a.p) & (a.align - 1)) return l1_fail(who, "a pointer is not aligned to its element size");
    }
  for (const Ptr& o : out) {
    int same = 0;
    for (const Ptr& a : in) same += a.p == o.p;
    for (const Ptr& a : out) same += a.p == o.p;
    if (same != 1) return l1_fail(who, "an output aliases an input or another output");
  }
  return XM_OK;
}

// sizes in 1 ... 2^31 - 1, at most 2^50 elements
int l1_sizes(const char* who, int64_t V, int64_t T) {
  const int64_t top = (1LL << 31) - 1;
  if (V < 1 || V > top || T < 1 || T > top) return l1_fail(who, "n_vox and n_cols must be in 1 ... 2^31 - 1");
  if (V > (1LL << 50) / T) return l1_fail(who, "too many elements (> 2^50)");
  return XM_OK;
}

bool l1_weight(double a) { return a >= 0.0 && std::isfinite(a); }

// f(grid, A) once per run of at most 65535 column tiles of 64 columns
template <class F>
int l1_tiles(L1Args A, F&& f) {
  const long long tiles = (A.n_cols + XM_WAVE - 1) / XM_WAVE, max_y = 65535;
  const unsigned gx = (A.n_blocks + XM_L1_ITEMS - 1) / XM_L1_ITEMS;
  for (long long y0 = 0; y0 < tiles; y0 += max_y) {
    A.tile0 = (unsigned)y0;
    f(dim3(gx, (unsigned)(tiles - y0 < max_y ? tiles - y0 : max_y)), A);
    HIP_TRY(hipGetLastError());
  }
  return XM_OK;
}
}  // namespace

extern "C" int xm_l1_start(const void* b, double* bpart, double* bmax, int32_t* status, double* change, void* x,
                           int64_t n_vox, int64_t n_cols, int finish, void* stream) {
  const char* who = "l1_start";
  if (const int rc = l1_sizes(who, n_vox, n_cols)) return rc;
  if (finish) {
    if (const int rc = l1_pointers(who, {{bpart, 8}}, {{bmax, 8}, {status, 4}, {change, 8}, {x, 16}})) return rc;
  } else {
    if (const int rc = l1_pointers(who, {{b, 16}}, {{bpart, 8}})) return rc;
  }
  L1Args A{};
  A.n_vox = n_vox;
  A.n_cols = n_cols;
  A.mode = finish != 0;
  const unsigned runs = (unsigned)((n_vox + XM_L1_MAX_BLOCK - 1) / XM_L1_MAX_BLOCK);
  A.n_blocks = finish ? 1u : runs;
  DeviceGuard guard(bpart);
  hipStream_t st = (hipStream_t)stream;
  xm_note_kernel("k_l1_start", nullptr, "c128", A.mode, -1);
  return l1_tiles(A, [&](dim3 grid, const L1Args& B) {
    hipLaunchKernelGGL(k_l1_start, grid, dim3(XM_L1_NT), 0, st, static_cast<const Cx<double>*>(b), bpart, bmax, status,
                       change, static_cast<Cx<double>*>(x), runs, B);
  });
}

extern "C" int xm_l1_prox(void* x, void* v, const void* q, const void* b, const uint8_t* mask, const double* bmax,
                          const double* d2_in, const double* n2_in, double* d2_out, double* n2_out,
                          const int32_t* status_in, int32_t* status_out, int32_t* n_iter, double* change, int n_dims,
                          int64_t m0, int64_t m1, int64_t m2, int l0, int l1, int l2, int s0, int s1, int s2,
                          int64_t n_cols, double tau, double theta_scale, double beta, double tol, int iteration, int mode,
                          void* stream) {
  const char* who = "l1_prox";
  if (n_dims < 1 || n_dims > 3) return l1_fail(who, "n_dims must be 1, 2 or 3");
  if (mode < 0 || mode > 2) return l1_fail(who, "mode must be 0 (step), 1 (first step) or 2 (final test)");
  const int64_t m[3] = {m0, m1, m2};
  const int l[3] = {l0, l1, l2}, s[3] = {s0, s1, s2};
  const int64_t top = (1LL << 31) - 1;
  int64_t V = 1;
  int bits = 0;
  for (int d = 0; d < 3; ++d) {
    if (m[d] < 1 || m[d] > top) return l1_fail(who, "a matrix size outside 1 ... 2^31 - 1");
    if (d >= n_dims && (m[d] != 1 || l[d] != 0)) return l1_fail(who, "a dim beyond n_dims must have size 1 and level 0");
    if (l[d] < 0 || l[d] > 4) return l1_fail(who, "a level outside 0 ... 4");
    if (m[d] % (1LL << l[d])) return l1_fail(who, "a matrix size is not divisible by 2^level");
    if (s[d] < 0 || s[d] >= (1 << l[d])) return l1_fail(who, "a shift outside its block");
    if (V > top / m[d]) return l1_fail(who, "n_vox must be in 1 ... 2^31 - 1");
    V *= m[d];
    bits += l[d];
  }
  if (bits > 4) return l1_fail(who, "a block of more than 16 voxels");
  if (const int rc = l1_sizes(who, V, n_cols)) return rc;
  if (!l1_weight(tau) || !l1_weight(theta_scale) || !l1_weight(beta) || !l1_weight(tol))
    return l1_fail(who, "tau, theta_scale, beta and tol must be finite and >= 0");
  if (iteration < 0) return l1_fail(who, "iteration must be >= 0");
  if (mode == 1) d2_in = n2_in = bmax, q = b;  // (not read)
  if (const int rc = l1_pointers(who, {{q, 16}, {b, 16}, {mask, 1}, {bmax, 8}, {d2_in, 8}, {n2_in, 8}, {status_in, 4}},
                                 {{x, 16}, {v, 16}, {d2_out, 8}, {n2_out, 8}, {status_out, 4}, {n_iter, 4}, {change, 8}}))
    return rc;
  L1Args A{};
  A.n_cols = n_cols;
  A.n_vox = V;
  A.stride[0] = m[1] * m[2];
  A.stride[1] = m[2];
  A.stride[2] = 1;
  unsigned blocks = 1;
  int off = 0;
  for (int d = 0; d < 3; ++d) {
    A.m[d] = (int)m[d];
    A.l[d] = l[d];
    A.s[d] = s[d];
    A.nblk[d] = (int)(m[d] >> l[d]);
    blocks *= (unsigned)A.nblk[d];
    for (int j = 0; j < l[d]; ++j) A.low[off + j] = ((1u << j) - 1u) << off;
    off += l[d];
  }
  A.n_blocks = blocks;
  A.mode = mode;
  A.iteration = iteration;
  A.tau = tau;
  A.theta_scale = theta_scale;
  A.beta = beta;
  A.tol2 = tol * tol;
  DeviceGuard guard(x);
  hipStream_t st = (hipStream_t)stream;
  const int block = 1 << bits;
  xm_note_kernel("k_l1_prox", nullptr, "c128", block, mode);
  Cx<double>* xx = static_cast<Cx<double>*>(x);
  Cx<double>* vv = static_cast<Cx<double>*>(v);
  const Cx<double>* qq = static_cast<const Cx<double>*>(q);
  const Cx<double>* bb = static_cast<const Cx<double>*>(b);
  return l1_tiles(A, [&](dim3 grid, const L1Args& B) {
#define XM_L1_LAUNCH(N)                                                                                                  \
  hipLaunchKernelGGL((k_l1_prox<N>), grid, dim3(XM_L1_NT), 0, st, xx, vv, qq, bb, mask, bmax, d2_in, n2_in, d2_out, n2_out, \
                     status_in, status_out, n_iter, change, B)
    switch (block) {
      case 1: XM_L1_LAUNCH(1); break;
      case 2: XM_L1_LAUNCH(2); break;
      case 4: XM_L1_LAUNCH(4); break;
      case 8: XM_L1_LAUNCH(8); break;
      default: XM_L1_LAUNCH(16); break;
    }
#undef XM_L1_LAUNCH
  });
}
