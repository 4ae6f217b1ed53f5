// The dense solve shared by the BSS-eval kernels (bsseval.hip: one system per sample / per source; bss_windows.hip: one per
// segment / per source group).  One workgroup of 1024 threads; the caller has built the M x M matrix A column-major in global
// memory (a thread owns rows tid, tid + 1024, ...: every access to a column is coalesced) and the `nrhs` right-hand sides x
// [nrhs][M] in LDS, and has synchronised.  LU with partial pivoting exactly as LAPACK getrf / numpy.linalg.solve (row swaps
// applied at once), then the two triangular solves on the right-hand sides.  *info = k + 1 when the k-th pivot is exactly zero
// (the solution is written as zeros and the caller falls back to minimum-norm least squares), else 0.  out: [M][nrhs].
#pragma once
#include "common.h"

__device__ __forceinline__ void bss_lu_solve(double* __restrict__ A, int M, int nrhs, double* rowk, double* x, int* __restrict__ info,
                                             double* __restrict__ out) {
  const int tid = threadIdx.x;
  __shared__ double red_v[16];
  __shared__ int red_i[16];
  __shared__ int s_piv;
  __shared__ double s_pivval;
  bool singular = false;
  for (int k = 0; k < M; ++k) {
    // pivot search in column k
    double best = -1.0;
    int bi = k;
    for (int r = tid; r < M; r += 1024)
      if (r >= k) {
        const double v = fabs(A[(long long)k * M + r]);
        if (v > best) { best = v; bi = r; }
      }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const double ov = __shfl_xor(best, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
    }
    if ((tid & 63) == 0) { red_v[tid >> 6] = best; red_i[tid >> 6] = bi; }
    __syncthreads();
    if (tid == 0) {
      double bv = red_v[0];
      int bx = red_i[0];
      for (int w = 1; w < 16; ++w)
        if (red_v[w] > bv || (red_v[w] == bv && red_i[w] < bx)) { bv = red_v[w]; bx = red_i[w]; }
      s_piv = bx;
      s_pivval = bv;
    }
    __syncthreads();
    const int p = s_piv;
    if (!(s_pivval > 0.0)) { singular = true; if (tid == 0) *info = k + 1; break; }   // exactly singular (or NaN)
    // swap rows k and p in every column and in the right-hand sides; stage row k of U
    for (int c = tid; c < M; c += 1024) {
      double vk = A[(long long)c * M + k];
      if (p != k) {
        const double vp = A[(long long)c * M + p];
        A[(long long)c * M + p] = vk;
        A[(long long)c * M + k] = vp;
        vk = vp;
      }
      rowk[c] = vk;
    }
    if (p != k && tid < nrhs) {
      const double t = x[tid * M + k];
      x[tid * M + k] = x[tid * M + p];
      x[tid * M + p] = t;
    }
    __syncthreads();
    const double inv = 1.0 / rowk[k];
    // column k of L, trailing update, and the forward substitution of the right-hand sides folded into the same sweep
    for (int r = tid; r < M; r += 1024)
      if (r > k) {
        const double l = A[(long long)k * M + r] * inv;
        A[(long long)k * M + r] = l;
        // the sweep is latency-bound (an 8 MB matrix per system, one row element per column): 16 independent loads in flight
        int c = k + 1;
        for (; c + 16 <= M; c += 16) {
          double v[16];
#pragma unroll
          for (int u = 0; u < 16; ++u) v[u] = A[(long long)(c + u) * M + r];
#pragma unroll
          for (int u = 0; u < 16; ++u) A[(long long)(c + u) * M + r] = fma(-l, rowk[c + u], v[u]);
        }
        for (; c < M; ++c) A[(long long)c * M + r] = fma(-l, rowk[c], A[(long long)c * M + r]);
        for (int q = 0; q < nrhs; ++q) x[q * M + r] = fma(-l, x[q * M + k], x[q * M + r]);
      }
    __syncthreads();
  }
  if (singular) {
    for (int q = 0; q < nrhs; ++q)
      for (int r = tid; r < M; r += 1024) out[(long long)r * nrhs + q] = 0.0;
    return;
  }
  if (tid == 0) *info = 0;
  // back substitution with U (the forward half was done on the fly)
  for (int k = M - 1; k >= 0; --k) {
    if (tid < nrhs) x[tid * M + k] /= A[(long long)k * M + k];
    __syncthreads();
    for (int r = tid; r < k; r += 1024) {
      const double u = A[(long long)k * M + r];
      for (int q = 0; q < nrhs; ++q) x[q * M + r] = fma(-u, x[q * M + k], x[q * M + r]);
    }
    __syncthreads();
  }
  for (int q = 0; q < nrhs; ++q)
    for (int r = tid; r < M; r += 1024) out[(long long)r * nrhs + q] = x[q * M + r];
}
