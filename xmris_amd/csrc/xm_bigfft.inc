// Transforms longer than the in-LDS plans (n > 8192 complex128 / 16384 complex64, and chirp-z sizes beyond them): the
// four-step algorithm over global memory.  n = n1 * n2 with both factors among the in-LDS plans; input index
// i = i1 n2 + i2, output index k = k1 + n1 k2:
//     X[k1 + n1 k2] = sum_{i2} W_{n2}^{i2 k2} [ W_n^{i2 k1} sum_{i1} x[i1 n2 + i2] W_{n1}^{i1 k1} ]
//   t1  A[i2][i1] = prep(x)[i1 n2 + i2]            tiled transpose; zero fill / window / input roll / conj folded in
//   f1  B[i2][k1] = FFT_{n1} of the rows of A      the batched in-LDS kernels (n2 * batch rows)
//   t2  C[k1][i2] = B[i2][k1] * W_n^{i2 k1}        tiled transpose + twiddle (fp64 table of W_n, rounded once)
//   f2  D[k1][k2] = FFT_{n2} of the rows of C
//   t3  out[k1 + n1 k2] = epi(D[k1][k2])           tiled transpose; scale / conj / output roll / phase folded in
// Five read+write passes instead of the one of an in-LDS transform: a correctness path for the rare long axes
// (pocketfft takes any length, processing/fourier.py:153), ~1/5 of the streaming rate.  Lengths without such a
// factorisation go through Bluestein's chirp-z on top of it (convolution length M = 2^k >= 2n - 1).
// Included by xm_launch.inc (T = storage real type).

template <class U>
struct BigPrep {  // FFT input position pos -> sample
  const Cx<U>* in;
  long long in_stride;
  const U* window;
  const Cx<U>* chirp;  // Bluestein: a[pos] (n entries), positions >= n are zero
  int n, n_in, pad_left, in_shift, inverse;
};
template <class U>
XM_DEV Cx<U> big_load(const BigPrep<U>& P, long long b, int pos) {
  Cx<U> x = mk<U>(U(0), U(0));
  if (pos < P.n) {
    int j = pos - P.in_shift;
    if (j < 0) j += P.n;
    const int src = j - P.pad_left;
    if (src >= 0 && src < P.n_in) {
      x = P.in[b * P.in_stride + src];
      if (P.window) x = x * P.window[j];
      if (P.inverse) x = conj(x);
      if (P.chirp) x = x * P.chirp[pos];
    }
  }
  return x;
}

template <class U>
struct BigEpi {  // transform output m -> stored element
  Cx<U>* out;
  long long out_stride;
  const Cx<U>* phase;
  const Cx<U>* chirp;  // Bluestein: result m = conj(v) a[m] (the inverse transform ran as a conjugated forward one)
  U scale;
  int n, out_shift, inverse;
};
template <class U>
XM_DEV void big_store(const BigEpi<U>& E, long long b, int m, Cx<U> v) {
  if (m >= E.n) return;
  if (E.chirp) v = conj(v) * E.chirp[m];
  Cx<U> x = v * E.scale;
  if (E.inverse) x = conj(x);
  int k = m + E.out_shift;
  if (k >= E.n) k -= E.n;
  if (E.phase) x = x * E.phase[k];
  E.out[b * E.out_stride + k] = x;
}

// 32 x 32 tiles through LDS (one pad column): reads and writes are both row-contiguous
template <class U>
__global__ __launch_bounds__(256) void k_big_t1(BigPrep<U> P, Cx<U>* __restrict__ A, int n1, int n2) {
  __shared__ Cx<U> tile[32][33];
  const long long b = blockIdx.z;
  const int i2_0 = blockIdx.x * 32, i1_0 = blockIdx.y * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int r = ty; r < 32; r += 8) {
    const int i1 = i1_0 + r, i2 = i2_0 + tx;
    tile[r][tx] = (i1 < n1 && i2 < n2) ? big_load(P, b, i1 * n2 + i2) : mk<U>(U(0), U(0));
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int i2 = i2_0 + r, i1 = i1_0 + tx;
    if (i2 < n2 && i1 < n1) A[(b * n2 + i2) * (long long)n1 + i1] = tile[tx][r];
  }
}

template <class U>
__global__ __launch_bounds__(256) void k_big_t2(const Cx<U>* __restrict__ B, Cx<U>* __restrict__ C, const Cx<U>* __restrict__ wn,
                                                 int n1, int n2) {
  __shared__ Cx<U> tile[32][33];
  const long long b = blockIdx.z, n = (long long)n1 * n2;
  const int k1_0 = blockIdx.x * 32, i2_0 = blockIdx.y * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int r = ty; r < 32; r += 8) {
    const int i2 = i2_0 + r, k1 = k1_0 + tx;
    if (i2 < n2 && k1 < n1) tile[r][tx] = B[(b * n2 + i2) * (long long)n1 + k1] * wn[((long long)i2 * k1) % n];
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int k1 = k1_0 + r, i2 = i2_0 + tx;
    if (k1 < n1 && i2 < n2) C[(b * n1 + k1) * (long long)n2 + i2] = tile[tx][r];
  }
}

template <class U>
__global__ __launch_bounds__(256) void k_big_t3(const Cx<U>* __restrict__ D, BigEpi<U> E, int n1, int n2) {
  __shared__ Cx<U> tile[32][33];
  const long long b = blockIdx.z;
  const int k2_0 = blockIdx.x * 32, k1_0 = blockIdx.y * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int r = ty; r < 32; r += 8) {
    const int k1 = k1_0 + r, k2 = k2_0 + tx;
    if (k1 < n1 && k2 < n2) tile[r][tx] = D[(b * n1 + k1) * (long long)n2 + k2];
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int k2 = k2_0 + r, k1 = k1_0 + tx;
    if (k2 < n2 && k1 < n1) big_store(E, b, k1 + n1 * k2, tile[tx][r]);
  }
}

// element-wise stages of the long chirp-z: z = prep(x) a (zero beyond n), u = conj(FFT(z) * bh)
template <class U>
__global__ void k_big_fill(BigPrep<U> P, Cx<U>* __restrict__ Z, int m_len, long long total) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long b = i / m_len;
    Z[i] = big_load(P, b, (int)(i - b * m_len));
  }
}
template <class U>
__global__ void k_big_mul_conj(Cx<U>* __restrict__ Z, const Cx<U>* __restrict__ bh, int m_len, long long total) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x)
    Z[i] = conj(Z[i] * bh[i % m_len]);
}

void gen_wn(int n, int, const void*, std::vector<double>& re, std::vector<double>& im) {  // W_n^m, m < n
  re.resize(n);
  im.resize(n);
  for (int m = 0; m < n; ++m) xm_unit(m, n, -1.0, re[m], im[m]);
}

// n = n1 * n2 with both factors in-LDS plans of this precision; prefers balanced factors.  false: no such split
bool big_split(int n, int* n1, int* n2) {
  int best = 0;
  for (int a = 2; (long long)a * a <= n; ++a) {
    if (n % a) continue;
    const int b = n / a;
    if (xm_has_direct_plan(a, kDtype) && xm_has_direct_plan(b, kDtype)) best = a;
  }
  if (!best) return false;
  *n1 = best;
  *n2 = n / best;
  return true;
}

// plain forward transform of `rows` contiguous rows of length m (an in-LDS plan)
int big_rows_fft(const Cx<T>* in, Cx<T>* out, long long rows, int m, hipStream_t st) {
  PipeArgs<T> S;
  std::memset(&S, 0, sizeof(S));
  S.in = in;
  S.out = out;
  S.in_stride = m;
  S.n_batch = rows;
  S.n = S.n_in = m;
  S.scale = T(1);
  return run(route(in, m, rows, m, m, 0, 0, W), S, m, nullptr, st);
}

// four-step transform of length n = n1 n2: P describes the input, E the output; scratch S0, S1: n_batch * n elements each
int big_fft(const BigPrep<T>& P, const BigEpi<T>& E, long long n_batch, int n, Cx<T>* S0, Cx<T>* S1, hipStream_t st) {
  int n1 = 0, n2 = 0;
  if (!big_split(n, &n1, &n2)) return xm_fail(XM_ERR_UNSUPPORTED_N, "no two-factor split of " + std::to_string(n));
  if (n_batch > 65535) return xm_fail(XM_ERR_INVALID_ARG, "long transforms: at most 65535 rows per call");
  const void* wn = nullptr;
  int rc = xm_table_get(TK_BIG_WN, n, 0, kDtype, gen_wn, nullptr, &wn);
  if (rc) return rc;
  const dim3 blk(256);
  hipLaunchKernelGGL(k_big_t1<T>, dim3((n2 + 31) / 32, (n1 + 31) / 32, (unsigned)n_batch), blk, 0, st, P, S0, n1, n2);
  rc = big_rows_fft(S0, S1, n_batch * n2, n1, st);
  if (rc) return rc;
  hipLaunchKernelGGL(k_big_t2<T>, dim3((n1 + 31) / 32, (n2 + 31) / 32, (unsigned)n_batch), blk, 0, st, S1, S0, (const Cx<T>*)wn, n1, n2);
  rc = big_rows_fft(S0, S1, n_batch * n1, n2, st);
  if (rc) return rc;
  hipLaunchKernelGGL(k_big_t3<T>, dim3((n2 + 31) / 32, (n1 + 31) / 32, (unsigned)n_batch), blk, 0, st, S1, E, n1, n2);
  HIP_TRY(hipGetLastError());
  return XM_OK;
}

int big_m(int n) {  // chirp-z convolution length
  int m = 16;
  while (m < 2 * n - 1) m <<= 1;
  return m;
}

bool big_supported(int n) {
  int a, b;
  if (n < 2 || n > (1 << 22)) return false;
  if (big_split(n, &a, &b)) return true;
  return big_m(n) <= (1 << 23) && big_split(big_m(n), &a, &b);
}

// The fused entry point for a length beyond the in-LDS plans.  Row chunks keep the scratch below ~1 GiB.
int pipeline_big(PipeArgs<T> A, hipStream_t st) {
  const int n = A.n;
  int n1, n2;
  const bool direct = big_split(n, &n1, &n2);
  const int m = direct ? n : big_m(n);
  if (!direct && !big_split(m, &n1, &n2)) return xm_fail(XM_ERR_UNSUPPORTED_N, "length " + std::to_string(n) + " is beyond the long-transform path");
  if (A.n_batch <= 0) return XM_OK;
  const void *ch = nullptr, *bh = nullptr;
  int rc;
  if (!direct) {
    rc = xm_table_get(TK_CHIRP, n, m, kDtype, gen_chirp, nullptr, &ch);
    if (rc) return rc;
    rc = xm_table_get(TK_CHIRP_FFT, n, m, kDtype, gen_chirp_fft, nullptr, &bh);
    if (rc) return rc;
  }
  long long rows_per = (1LL << 30) / ((long long)m * (long long)sizeof(Cx<T>));
  rows_per = rows_per < 1 ? 1 : (rows_per > 65535 ? 65535 : rows_per);
  if (rows_per > A.n_batch) rows_per = A.n_batch;
  const size_t elems = (size_t)rows_per * (size_t)m;
  // all the scratch in ONE stream-ordered block (a failing allocation leaves nothing behind): S0, S1, the chirp-z
  // pair Z, Y and, for an arg-max-only call, room for the spectra
  Cx<T>* out = A.out;
  const size_t n_tmp = out ? 0 : (size_t)rows_per * (size_t)n;
  const size_t n_block = elems * (direct ? 2 : 4) + n_tmp;
  Cx<T>* block = nullptr;
  HIP_TRY(hipMallocAsync((void**)&block, n_block * sizeof(Cx<T>), st));
  Cx<T>*S0 = block, *S1 = block + elems;
  Cx<T>*Zb = direct ? nullptr : block + 2 * elems, *Yb = direct ? nullptr : block + 3 * elems;
  Cx<T>* tmp_out = out ? nullptr : block + elems * (direct ? 2 : 4);
  rc = XM_OK;
  for (long long b0 = 0; b0 < A.n_batch && rc == XM_OK; b0 += rows_per) {
    const long long nb = std::min(rows_per, A.n_batch - b0);
    BigPrep<T> P{A.in + b0 * A.in_stride, A.in_stride, A.window, (const Cx<T>*)ch, n, A.n_in, A.pad_left, A.in_shift, A.inverse};
    Cx<T>* dst = out ? out + b0 * (long long)n : tmp_out;
    BigEpi<T> E{dst, (long long)n, out ? A.phase : nullptr, (const Cx<T>*)ch, A.scale, n, A.out_shift, A.inverse};
    if (direct) {
      rc = big_fft(P, E, nb, n, S0, S1, st);
    } else {
      // chirp-z: z = x a (length m) -> FFT -> * FFT(b)/m, conj -> FFT (the conjugate of the inverse) -> conj, * a
      Cx<T>*Z = Zb, *Y = Yb;
      const long long total = nb * (long long)m;
      const int grid = (int)std::min<long long>((total + 255) / 256, 256LL * 16);
      hipLaunchKernelGGL(k_big_fill<T>, dim3(grid), dim3(256), 0, st, P, Z, m, total);
      BigPrep<T> P1{Z, (long long)m, nullptr, nullptr, m, m, 0, 0, 0};
      BigEpi<T> E1{Y, (long long)m, nullptr, nullptr, T(1), m, 0, 0};
      rc = big_fft(P1, E1, nb, m, S0, S1, st);
      if (rc == XM_OK) {
        hipLaunchKernelGGL(k_big_mul_conj<T>, dim3(grid), dim3(256), 0, st, Y, (const Cx<T>*)bh, m, total);
        BigPrep<T> P2{Y, (long long)m, nullptr, nullptr, m, m, 0, 0, 0};
        rc = big_fft(P2, E, nb, m, S0, S1, st);  // E: conj, * a[m], scale, roll, phase; only m < n is stored
      }
    }
    if (rc == XM_OK && A.absmax2) {
      const int grid = (int)(nb < 65536 * 4 ? nb : 65536 * 4);
      // the maxima are taken BEFORE the phase multiply in the in-LDS kernels; a unit-modulus phase does not move them
      hipLaunchKernelGGL(k_absmax_rows<T>, dim3(grid), dim3(256), 0, st, (const Cx<T>*)dst, nb, n, A.absmax2 + b0, A.argidx + b0);
    }
  }
  (void)hipFreeAsync(block, st);
  if (rc == XM_OK) HIP_TRY(hipGetLastError());
  return rc;
}
