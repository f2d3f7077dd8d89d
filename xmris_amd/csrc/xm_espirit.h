// ESPIRiT per-voxel eigen-decomposition kernel (the project's own definition, the reference has
// no such function).  Included by xm_espirit.hip.  The mirror, the Jacobi iteration and the entry map of the upper
// triangle are xm_wg.h's.
//
// One voxel: H = its C x C Hermitian matrix, given as the E = C (C + 1) / 2 entries of the upper triangle (i <= j,
// row-major, complex128).  The M largest eigenvalues (a tie goes to the lower column of the Jacobi result) and their
// eigenvectors, each of unit norm and turned so that component `phase_ref` is real and >= 0 (left as Jacobi gave it when
// that component is exactly 0); a map whose eigenvalue is < crop is written as exact zeros.
//
// k_espirit_eig: one 256-thread workgroup per voxel; the grid is the stream's resident workgroups and workgroup b takes
// the voxels b, b + gridDim.x, ...  (no ticket: a voxel's work does not depend on which workgroup runs it, and the
// kernel has no atomics).  Nothing of another voxel is read and every sum runs in a fixed order, so a voxel's outputs
// are bitwise independent of the batch.  All arithmetic fp64.
#pragma once
#include "xm_wg.h"

#define XM_ESP_MAXC 64
#define XM_ESP_NT 256
#define XM_ESP_SMALL (XM_WG_NT + XM_WG_ROT * 32 + 32)  // doubles after the two matrices: red[256], rot[256], pairs[32]
static_assert(XM_ESP_NT == XM_WG_NT, "k_espirit_eig runs xm_wg.h's workgroup");
static_assert(XM_ESP_MAXC * (XM_ESP_MAXC + 1) / 2 <= XM_WG_MAXE * XM_WG_NT, "the entry slots must hold XM_ESP_MAXC coils");

struct EspArgs {
  const double* h;  // (V, E) complex128
  double* maps;     // (M, C, V) complex128
  double* values;   // (M, V)
  int* status;      // (V) 0 ok, 1 sweep cap, 2 non-finite input
  long long V;
  int C, M, phase_ref;
  double crop;
};

__host__ __device__ inline size_t esp_lds_bytes(int C) { return (4 * (size_t)C * C + XM_ESP_SMALL) * sizeof(double); }

__global__ __launch_bounds__(XM_ESP_NT, 1) void k_espirit_eig(EspArgs A) {
  extern __shared__ double esp_sm[];
  const int t = threadIdx.x, C = A.C, ne = C * (C + 1) / 2;
  double* G = esp_sm;                    // H, then its diagonal form
  double* B = G + 2 * (size_t)C * C;     // the eigenvectors, one per column
  double* red = B + 2 * (size_t)C * C;
  double* rot = red + XM_WG_NT;
  int ci[XM_WG_MAXE], cj[XM_WG_MAXE];
  wg_gram_entries(C, ne, ci, cj);

  for (long long v = blockIdx.x; v < A.V; v += gridDim.x) {
    const double* hv = A.h + 2 * v * ne;
    int bad = 0;
#pragma unroll
    for (int m = 0; m < XM_WG_MAXE; ++m) {
      const int e = t + XM_ESP_NT * m;
      if (e < ne) {
        const double re = hv[2 * e], im = hv[2 * e + 1];
        if (!isfinite(re) || !isfinite(im)) bad = 1;
        G[2 * (ci[m] * C + cj[m])] = re;
        G[2 * (ci[m] * C + cj[m]) + 1] = im;
      }
    }
    bad = __syncthreads_or(bad);
    int sweeps = 0;
    if (!bad) {
      wg_mirror(G, C);
      sweeps = wg_jacobi(G, B, red, rot, C);
    }
    if (bad || sweeps < 0) {  // a non-finite entry, or finite ones so large that the norm overflows
      for (int i = t; i < A.M * C; i += XM_ESP_NT) {
        A.maps[2 * (i * A.V + v)] = 0.0;
        A.maps[2 * (i * A.V + v) + 1] = 0.0;
      }
      if (t < A.M) A.values[t * A.V + v] = NAN;
      if (t == 0) A.status[v] = 2;
      __syncthreads();
      continue;
    }
    int best[2] = {0, 0};  // the largest diagonal entries, the lower index on a tie (every thread alike)
    for (int c = 1; c < C; ++c)
      if (G[2 * (c * C + c)] > G[2 * (best[0] * C + best[0])]) best[0] = c;
    if (A.M > 1) {
      best[1] = best[0] == 0 ? 1 : 0;
      for (int c = best[1] + 1; c < C; ++c)
        if (c != best[0] && G[2 * (c * C + c)] > G[2 * (best[1] * C + best[1])]) best[1] = c;
    }
    for (int m = 0; m < A.M; ++m) {
      const int col = best[m];
      const double lam = G[2 * (col * C + col)];
      double n2 = 0.0;
      for (int c = 0; c < C; ++c) {
        const double xr = B[2 * (c * C + col)], xi = B[2 * (c * C + col) + 1];
        n2 += xr * xr + xi * xi;
      }
      const double nrm = sqrt(n2);
      const double pr = B[2 * (A.phase_ref * C + col)], pi = B[2 * (A.phase_ref * C + col) + 1];
      const double a = hypot(pr, pi);
      const double fr = a > 0.0 ? pr / a : 1.0, fi = a > 0.0 ? -pi / a : 0.0;  // conj(x_ref) / |x_ref|
      if (t < C) {
        const double xr = B[2 * (t * C + col)], xi = B[2 * (t * C + col) + 1];
        double yr = (xr * fr - xi * fi) / nrm, yi = (xr * fi + xi * fr) / nrm;
        if (t == A.phase_ref && a > 0.0) yi = 0.0;  // real by construction, stored so
        if (lam < A.crop) yr = yi = 0.0;
        const long long o = 2 * (((long long)m * C + t) * A.V + v);
        A.maps[o] = yr;
        A.maps[o + 1] = yi;
      }
      if (t == 0) A.values[m * A.V + v] = lam;
    }
    if (t == 0) A.status[v] = sweeps > XM_WG_SWEEPS ? 1 : 0;
    __syncthreads();  // G and B are read to the end: the next voxel's load waits
  }
}
