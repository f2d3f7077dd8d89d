// Marchenko-Pastur patch PCA denoising kernel (the project's own definition, the reference has no
// such function).  Included by xm_denoise.hip only.
//
// One voxel i of the grid (n_outer, s1, s2, s3, N): X = the P x N matrix of the FIDs of its window (p1 x p2 x p3 voxels,
// shifted inward at an edge, rows in row-major order of the window offsets), c = the row that is voxel i itself.
// G = X X^H; lambda_k = max(eig_k, 0) / N descending with eigenvectors U; r = the given rank or the first p with
// (lambda_p - lambda_{P-1}) / (4 sqrt((P - p) / N)) < mean(lambda_p ... lambda_{P-1}); w_j = sum_{k<r} U[c,k] conj(U[j,k]);
// y_i = sum_j w_j X[j, :].
//
// k_denoise: one 256-thread workgroup per voxel, voxels handed out by a device counter (persistent grid, as
// k_coil_combine).  The window's P row starts are formed once per voxel into the LDS; from there on a window is the
// "coils" of k_coil_combine: the staging and the Gram matrix (matrix cores or plain FMAs) are xm_coils.h's, on its LDS
// layout with C = P; the Jacobi iteration (wg_jacobi) and the voxel ticket are xm_wg.h's.  All arithmetic fp64; complex64
// is widened on load.
#pragma once
#include "xm_coils.h"

#define XM_DN_MAXP 64
#define XM_DN_MAXN 16384
#define XM_DN_NT XM_CC_NT
static_assert(XM_DN_NT == XM_WG_NT, "k_denoise runs xm_wg.h's workgroup");
#define XM_DN_EXTRA 160  // doubles after xm_coils.h's layout: rows[64] (long long), lam[64], ord[64] (int)

struct DenoiseArgs {
  const void* x;  // (n_outer, s1, s2, s3, N) complex64 / complex128
  void* y;        // the same shape and dtype
  int* rank;      // (n_outer, s1, s2, s3)
  double* sigma;  // (n_outer, s1, s2, s3)
  int* status;    // (n_outer, s1, s2, s3) 0 done, 1 all-zero window, 2 non-finite, 3 sweep cap
  long long nv;   // n_outer s1 s2 s3
  int s1, s2, s3, p1, p2, p3, P, N;
  int rank_in;    // 0 ... P, or -1 for the Marchenko-Pastur rule
  int is_c128, stop;
  unsigned* counter;  // [2] zero at launch: voxel ticket, workgroups done
};

enum { XM_DN_FORM_MFMA = 0, XM_DN_FORM_FMA = 1 };
enum { XM_DN_STOP_NONE = 0, XM_DN_STOP_GRAM = 1, XM_DN_STOP_EIG = 2 };

__host__ __device__ inline size_t dn_lds_bytes(int P) { return cc_lds_bytes(P) + XM_DN_EXTRA * sizeof(double); }

XM_DEV void dn_store(const DenoiseArgs& A, long long i, double re, double im) {
  if (A.is_c128) {
    ((double*)A.y)[2 * i] = re;
    ((double*)A.y)[2 * i + 1] = im;
  } else {
    ((float*)A.y)[2 * i] = (float)re;
    ((float*)A.y)[2 * i + 1] = (float)im;
  }
}

// the outputs of a voxel that is not denoised: y zero (or x itself: `copy`), rank 0, sigma as given
XM_DEV void dn_degenerate(const DenoiseArgs& A, long long v, int status, double sigma, bool copy) {
  const int t = threadIdx.x;
  for (int i = t; i < A.N; i += XM_DN_NT) {
    double re = 0.0, im = 0.0;
    if (copy) cc_load(A.x, A.is_c128, v * A.N + i, re, im);
    dn_store(A, v * A.N + i, re, im);
  }
  if (t == 0) {
    A.rank[v] = 0;
    A.sigma[v] = sigma;
    A.status[v] = status;
  }
}

// Thread 0: the rank r and sigma from lam[0 .. M) (descending).  suf[p] = sum_{i >= p} lam[i], accumulated from
// i = M - 1 downwards.  Marchenko-Pastur rule (rank_in < 0): the first p with sigma2^2(p) < sigma1^2(p); when no p
// qualifies (lam[M - 1] is zero: nothing in the window looks like noise) r = M and sigma = 0.
XM_DEV void dn_rank(const double* lam, double* suf, int M, int N, int rank_in, int& r_out, double& sigma_out) {
  double s = 0.0;
  for (int i = M - 1; i >= 0; --i) {
    s += lam[i];
    suf[i] = s;
  }
  int r = M;
  if (rank_in >= 0) {
    r = rank_in;
  } else {
    for (int p = 0; p < M; ++p) {
      const double s1 = suf[p] / (double)(M - p);
      const double gam = (double)(M - p) / (double)N;
      const double s2 = (lam[p] - lam[M - 1]) / (4.0 * sqrt(gam));
      if (s2 < s1) {
        r = p;
        break;
      }
    }
  }
  r_out = r;
  sigma_out = r < M ? sqrt(suf[r] / (double)(M - r)) : 0.0;
}

template <int FORM>
__global__ __launch_bounds__(XM_DN_NT, 2) void k_denoise(DenoiseArgs A) {
  extern __shared__ double dn_sm[];
  const int t = threadIdx.x, P = A.P;
  CcLds L;
  L.G = dn_sm;
  L.B = L.G + 2 * (size_t)P * P;
  L.scr = L.B + cc_b_doubles(P);
  L.red = L.scr + 1024;
  L.w = L.red + XM_CC_NT;
  L.u = L.w + 2 * XM_CC_MAXC;
  L.rot = L.u + 2 * XM_CC_MAXC;
  long long* rows = (long long*)(L.scr + XM_CC_SMALL);  // after xm_coils.h's small arrays
  double* lam = (double*)(rows + XM_DN_MAXP);
  int* ord = (int*)(lam + XM_DN_MAXP);
  __shared__ unsigned next;
  __shared__ int sh_rank, sh_c;
  __shared__ double sh_sigma;

  CoilArgs CA{};  // what the functions of xm_coils.h read: the "reference" is x, the "coils" are the window's rows
  CA.ref = A.x;
  CA.C = P;
  CA.NR = A.N;
  CA.is_c128 = A.is_c128;
  const CcVoxel V{};  // (unused with a row table)

  for (;;) {
    const long long v = wg_next_item(A.counter, &next);
    if (v >= A.nv) break;

    // the window: start o_a = min(max(i_a - p_a / 2, 0), s_a - p_a) per patch dim, rows in row-major order
    {
      const int i3 = (int)(v % A.s3), i2 = (int)((v / A.s3) % A.s2), i1 = (int)((v / ((long long)A.s3 * A.s2)) % A.s1);
      const long long a = v / ((long long)A.s3 * A.s2 * A.s1);
      const int o1 = min(max(i1 - A.p1 / 2, 0), A.s1 - A.p1), o2 = min(max(i2 - A.p2 / 2, 0), A.s2 - A.p2),
                o3 = min(max(i3 - A.p3 / 2, 0), A.s3 - A.p3);
      if (t < P) {
        const int d3 = t % A.p3, d2 = (t / A.p3) % A.p2, d1 = t / (A.p3 * A.p2);
        rows[t] = ((((a * A.s1 + o1 + d1) * A.s2 + o2 + d2) * A.s3) + o3 + d3) * A.N;
      }
      if (t == 0) sh_c = ((i1 - o1) * A.p2 + (i2 - o2)) * A.p3 + (i3 - o3);
    }
    __syncthreads();

    int flags = 0;
    if (FORM == XM_DN_FORM_MFMA)
      cc_gram_mfma<true>(CA, L, V, flags, rows);
    else
      cc_gram_fma<true>(CA, L, V, flags, rows);
    flags = __syncthreads_or(flags & 1) | (__syncthreads_or(flags & 2) ? 2 : 0);
    if ((flags & 1) || !(flags & 2)) {
      dn_degenerate(A, v, (flags & 1) ? 2 : 1, (flags & 1) ? NAN : 0.0, false);
      __syncthreads();
      continue;
    }
    if (A.stop == XM_DN_STOP_GRAM) {  // (timing only)
      if (t == 0) {
        A.rank[v] = 0;
        A.sigma[v] = L.G[0];
        A.status[v] = 0;
      }
      __syncthreads();
      continue;
    }
    const int sweeps = wg_jacobi(L.G, L.B, L.red, L.rot, P);
    if (sweeps < 0 || sweeps > XM_WG_SWEEPS) {
      dn_degenerate(A, v, sweeps < 0 ? 2 : 3, NAN, sweeps > XM_WG_SWEEPS);
      __syncthreads();
      continue;
    }
    // descending order by rank counting, a tie going to the lower index (every slot filled first: an eigenvalue that
    // is not a number would otherwise leave one unwritten)
    if (t < P) {
      lam[t] = 0.0;
      ord[t] = t;
    }
    __syncthreads();
    if (t < P) {
      const double e = L.G[2 * (t * P + t)];
      int pos = 0;
      for (int j = 0; j < P; ++j) {
        const double f = L.G[2 * (j * P + j)];
        if (f > e || (f == e && j < t)) ++pos;
      }
      lam[pos] = fmax(e, 0.0) / (double)A.N;
      ord[pos] = t;
    }
    __syncthreads();
    if (t == 0) {
      int r;
      double sg;
      dn_rank(lam, L.scr, P, A.N, A.rank_in, r, sg);
      sh_rank = r;
      sh_sigma = sg;
    }
    __syncthreads();
    const int r = sh_rank, c = sh_c;
    if (A.stop == XM_DN_STOP_EIG) {  // (timing only)
      if (t == 0) {
        A.rank[v] = r;
        A.sigma[v] = sh_sigma;
        A.status[v] = 0;
      }
      __syncthreads();
      continue;
    }
    // w = row c of the projector onto the top-r subspace (U in B, eigenvector k in column ord[k])
    if (t < P) {
      double wr = 0.0, wi = 0.0;
      for (int k = 0; k < r; ++k) {
        const int col = ord[k];
        const double ar = L.B[2 * (c * P + col)], ai = L.B[2 * (c * P + col) + 1];
        const double br = L.B[2 * (t * P + col)], bi = L.B[2 * (t * P + col) + 1];
        wr += ar * br + ai * bi;  // a conj(b)
        wi += ai * br - ar * bi;
      }
      L.w[2 * t] = wr;
      L.w[2 * t + 1] = wi;
    }
    __syncthreads();

    // apply pass: y = sum_j w_j X[j, :], one thread per time point, rows ascending
    for (int i = t; i < A.N; i += XM_DN_NT) {
      double yr = 0.0, yi = 0.0;
#pragma unroll 4
      for (int j = 0; j < P; ++j) {
        double re, im;
        cc_load(A.x, A.is_c128, rows[j] + i, re, im);
        yr += L.w[2 * j] * re - L.w[2 * j + 1] * im;
        yi += L.w[2 * j] * im + L.w[2 * j + 1] * re;
      }
      dn_store(A, v * A.N + i, yr, yi);
    }
    if (t == 0) {
      A.rank[v] = r;
      A.sigma[v] = sh_sigma;
      A.status[v] = 0;
    }
    __syncthreads();
  }
  wg_leave(A.counter);
}
