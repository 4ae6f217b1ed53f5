// BSS-eval, every form of it in this library: the windowed image form (SDR / ISR / SIR / SAR over all channels of a source; Vincent
// et al. 2006, bss_decomp_mtifilt for images) and mir_eval's bss_eval_sources on 6 s mono training batches (what the reference
// scores with, asteroid -> mir_eval, main.py:260-266: a batch [B, S, L] is S rows of B L samples, C = 1, sample b the segment
// [b L, b L + L)).  Float64 throughout.
// The rows are p = source * C + channel, P = S * C of them, each [L] samples.  A SEGMENT [a, a + n) is a stretch of the rows that
// is treated as zero outside itself; all segments of one call have the same length n.
//   1. bss_seg_corr_kernel + bss_seg_corr_reduce   lagged correlations of every segment, read in place from the [P, L] rows;
//                                                  register-tiled (8 lags x 8 samples per thread), no atomics: per-block partials,
//                                                  then a sum in ascending block order
//   2. bss_solve_groups_kernel                     the least-squares filters of a group of G rows (G = C: own source, G = P: all
//                                                  sources) by LU with partial pivoting, one workgroup per (segment, group)
//   3. bss_win_energy_kernel + bss_win_energy_reduce  both FIR projections of a row and the eight residual energies of a sample
//                                                  RANGE of its segment, in registers: no projected waveform is written out
// Every offset into the rows is formed in 64 bits (ten minutes at 48 kHz are 2.9e7 samples per row).
#include "common.h"

// LDS images whose readers sit 8 doubles apart (a thread owns 8 consecutive lags / outputs) get two pad doubles per 8: every
// block of 8 stays contiguous and 16-byte aligned (ds_read_b128), and lane l reads byte 80 l + const, bank 4 (5 l mod 16): the
// sixteen lanes of a ds_read_b128 group cover every bank once.
__device__ __forceinline__ int pad8(int x) { return x + ((x >> 3) << 1); }
// 8 contiguous doubles from a 16-byte aligned LDS address: four ds_read_b128 (two adjacent 8-byte loads become a ds_read2_b64, which
// moves half the bytes per LDS cycle)
typedef double f64x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void lds_read8(const double* p, double* v) {
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const f64x2 t = *(const f64x2*)(p + 2 * m);
    v[2 * m] = t.x;
    v[2 * m + 1] = t.y;
  }
}

// ---- 1. correlations of segments --------------------------------------------------------------------------------------------------
// R[seg][p][q][u], u = tau + flen - 1, tau in (-flen, flen):  sum_t r_p[t + tau] * r_q[t]
// D[seg][e][p][k], k in [0, flen):                            sum_t r_p[t - k]   * e_e[t]       (t and t + tau inside the segment)
// Every one of these is a sum X_ab[k] = sum_t a[t + k] * b[t] at a lag k in [0, flen): R[p][q][tau >= 0] = X_{r_p r_q}[tau],
// R[p][q][-tau] = R[q][p][tau] (each (pair, lag) is formed once and the reduce pass writes it to both places), and
// D[e][p][k] = X_{e_e r_p}[k].  So there are 2 P^2 jobs of flen lags, not P^2 (2 flen - 1) + P^2 flen lags, and all of them run
// the same code: two rows that hold the same samples (dual-mono) get the same bits in every block of R, which is therefore
// exactly symmetric and has exactly repeated rows.
// grid (parts, jobs, segments), 256 threads.  A block walks `cpb` chunks of SC_CH samples; per chunk the `a` row (with flen
// samples of margin on the right) and the `b` row go to LDS.  Thread (slice s, lag group g) owns the 8 lags 8 g .. 8 g + 7 and
// the samples of slice s of the chunk, and keeps a sliding window of 16 `a` values in registers: per 8 samples it reads 8 new `a`
// values and 8 `b` values (a broadcast) for 64 FMAs, 2 LDS bytes per FMA.  The slices of a lag are added in ascending order in
// LDS, the block's sums go to its own slot of `part`, and the reduce pass adds the slots in ascending order.
constexpr int SC_CH = 2048, SC_T = 8, SC_THREADS = 256, SC_MAXPART = 128;

struct sc_plan { int nchunks, cpb, npart; };
static inline sc_plan sc_plan_for(long long n) {       // a function of the segment length only: a segment's bits do not depend on its neighbours
  sc_plan p;
  p.nchunks = (int)((n + SC_CH - 1) / SC_CH);
  p.cpb = (p.nchunks + SC_MAXPART - 1) / SC_MAXPART;
  p.npart = (p.nchunks + p.cpb - 1) / p.cpb;
  return p;
}

__global__ __launch_bounds__(SC_THREADS) void bss_seg_corr_kernel(const double* __restrict__ refs, const double* __restrict__ ests, int P,
                                                                  long long L, int flen, const long long* __restrict__ seg_starts,
                                                                  long long n, int nchunks, int cpb, double* __restrict__ part) {
  extern __shared__ __align__(16) double sc_smem[];
  const int AWN = SC_CH + flen + SC_T;                 // logical length of the `a` image (what lies past the segment reads as zero)
  double* const aw = sc_smem;                          // a[t0 ...], padded by pad8
  double* const bw = sc_smem + ((pad8(AWN) + 3) & ~1); // b[t0 .. t0 + SC_CH), 16-byte aligned; afterwards the slices' sums
  const int tid = threadIdx.x, g = blockIdx.x, job = blockIdx.y, seg = blockIdx.z;
  const bool rr = job < P * P;
  const long long sa = seg_starts[seg];
  const double* const a = rr ? refs + (long long)(job / P) * L : ests + (long long)((job - P * P) / P) * L;
  const double* const b = refs + (long long)(job % P) * L;
  const int NG = (flen + SC_T - 1) / SC_T;             // lag groups
  int nsl = 1;
  while (nsl * 2 * NG <= SC_THREADS) nsl *= 2;         // time slices: a power of two, so a slice is a multiple of 8 samples
  const int SLn = SC_CH / nsl;
  const int grp = tid % NG, s = tid / NG, u0 = grp * SC_T;
  const bool active = s < nsl;
  double acc[SC_T];
#pragma unroll
  for (int j = 0; j < SC_T; ++j) acc[j] = 0.0;

  const int c_end = min((g + 1) * cpb, nchunks);
  for (int c = g * cpb; c < c_end; ++c) {
    const long long t0 = (long long)c * SC_CH;
    for (int x = tid; x < AWN; x += SC_THREADS) {
      const long long t = t0 + x, ta = sa + t;
      aw[pad8(x)] = (t < n && ta >= 0 && ta < L) ? a[ta] : 0.0;
    }
    for (int x = tid; x < SC_CH; x += SC_THREADS) {
      const long long t = t0 + x, ta = sa + t;
      bw[x] = (t < n && ta >= 0 && ta < L) ? b[ta] : 0.0;
    }
    __syncthreads();
    if (active) {
      const int xb0 = s * SLn;
      const double* ap = aw + pad8(xb0 + u0);          // xb0 + u0 is a multiple of 8: every block of 8 is contiguous
      const double* bp = bw + xb0;
      double A[2 * SC_T];
      lds_read8(ap, A);
#pragma unroll 2
      for (int xb = 0; xb < SLn; xb += SC_T) {
        ap += SC_T + 2;
        double Bv[SC_T];
        lds_read8(ap, A + SC_T);
        lds_read8(bp + xb, Bv);
#pragma unroll
        for (int i = 0; i < SC_T; ++i)
#pragma unroll
          for (int j = 0; j < SC_T; ++j) acc[j] = fma(A[i + j], Bv[i], acc[j]);
#pragma unroll
        for (int j = 0; j < SC_T; ++j) A[j] = A[SC_T + j];
      }
    }
    __syncthreads();
  }
  // the slices of a lag, in ascending order
  if (active) {
#pragma unroll
    for (int j = 0; j < SC_T; ++j) bw[s * NG * SC_T + u0 + j] = acc[j];
  }
  __syncthreads();
  double* const dst = part + (((long long)seg * gridDim.y + job) * gridDim.x + g) * flen;
  for (int u = tid; u < flen; u += SC_THREADS) {
    double v = bw[u];
    for (int k = 1; k < nsl; ++k) v += bw[k * NG * SC_T + u];
    dst[u] = v;
  }
}

// grid (jobs, segments): the parts of a (segment, job) in ascending order, written to R (at tau and, mirrored, at -tau) or D
__global__ __launch_bounds__(256) void bss_seg_corr_reduce(const double* __restrict__ part, int P, int flen, int npart, double* __restrict__ R,
                                                           double* __restrict__ D) {
  const int job = blockIdx.x, seg = blockIdx.y, NL = 2 * flen - 1;
  const bool rr = job < P * P;
  const int p = rr ? job / P : (job - P * P) / P, q = job % P;           // rr: a = r_p, b = r_q;  else a = e_p, b = r_q
  const double* const src = part + ((long long)seg * gridDim.x + job) * npart * flen;
  for (int u = threadIdx.x; u < flen; u += 256) {
    double v = src[u];
    for (int k = 1; k < npart; ++k) v += src[(long long)k * flen + u];
    if (rr) {
      R[(((long long)seg * P + p) * P + q) * NL + flen - 1 + u] = v;
      if (u > 0) R[(((long long)seg * P + q) * P + p) * NL + flen - 1 - u] = v;
    } else {
      D[(((long long)seg * P + p) * P + q) * flen + u] = v;
    }
  }
}

static inline bool sc_args_ok(int32_t nseg, int32_t P, int64_t n, int32_t flen) {
  return nseg > 0 && nseg <= 65535 && P > 0 && P <= 8 && n > 0 && flen > 0 && flen <= 512;
}
extern "C" size_t avsep_bss_seg_corr_workspace_bytes(int32_t nseg, int32_t P, int64_t n, int32_t flen) {
  if (!sc_args_ok(nseg, P, n, flen)) return 0;
  return sizeof(double) * (size_t)nseg * 2 * P * P * sc_plan_for(n).npart * (size_t)flen;
}
extern "C" int avsep_bss_seg_corr(const double* refs, const double* ests, int32_t P, int64_t L, int32_t flen, const int64_t* seg_starts,
                                  int32_t nseg, int64_t n, double* workspace, size_t workspace_bytes, double* R, double* D,
                                  avsep_stream_t stream) {
  if (!refs || !ests || !seg_starts || !workspace || !R || !D || L <= 0 || !sc_args_ok(nseg, P, n, flen)) return AVSEP_ERR_ARG;
  if (workspace_bytes < avsep_bss_seg_corr_workspace_bytes(nseg, P, n, flen)) return AVSEP_ERR_WORKSPACE;
  const sc_plan pl = sc_plan_for(n);
  const int njobs = 2 * P * P, AWN = SC_CH + flen + SC_T;
  const size_t lds = sizeof(double) * (size_t)(AWN + AWN / 8 * 2 + 4 + SC_CH);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(bss_seg_corr_kernel, dim3(pl.npart, njobs, nseg), dim3(SC_THREADS), lds, st, refs, ests, P, (long long)L, flen,
                     (const long long*)seg_starts, (long long)n, pl.nchunks, pl.cpb, workspace);
  AVSEP_LAUNCH_CHECK();
  hipLaunchKernelGGL(bss_seg_corr_reduce, dim3(njobs, nseg), dim3(256), 0, st, workspace, P, flen, pl.npart, R, D);
  AVSEP_LAUNCH_CHECK();
  return AVSEP_OK;
}

// ---- 2. the least-squares systems of row groups ------------------------------------------------------------------------------------
// System seg * (P / G) + g: the rows g G .. g G + G - 1 of segment seg.  M = G * flen unknowns, G right-hand sides (the estimate
// rows of the same group): A[(i,a)][(j,c)] = R[seg][gG+i][gG+j][c - a + flen - 1], right-hand side e: D[seg][gG+e][gG+i][a].
// C [system][M][G].
// bss_lu_solve: one workgroup of 1024 threads; the caller has built the M x M matrix A column-major in global memory (a thread owns
// rows tid, tid + 1024, ...: every access to a column is coalesced) and the `nrhs` right-hand sides x [nrhs][M] in LDS, and has
// synchronised.  LU with partial pivoting exactly as LAPACK getrf / numpy.linalg.solve (row swaps applied at once), then the two
// triangular solves on the right-hand sides.  *info = k + 1 when the k-th pivot is exactly zero (the solution is written as zeros
// and the caller falls back to minimum-norm least squares), else 0.  out: [M][nrhs].
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

__global__ __launch_bounds__(1024) void bss_solve_groups_kernel(const double* __restrict__ R, const double* __restrict__ D, int P, int G, int flen,
                                                                double* __restrict__ work, double* __restrict__ C, int* __restrict__ info) {
  extern __shared__ double sg_smem[];
  const int sys = blockIdx.x, tid = threadIdx.x, ng = P / G;
  const int seg = sys / ng, base = (sys % ng) * G;
  const int M = G * flen, NL = 2 * flen - 1;
  double* const A = work + (long long)sys * M * M;
  double* const rowk = sg_smem;                     // [M]
  double* const x = sg_smem + M;                    // [G][M]
  for (int c = 0; c < M; ++c) {
    const int j = base + c / flen, cc = c % flen;
    for (int r = tid; r < M; r += 1024) {
      const int i = base + r / flen, a = r % flen;
      A[(long long)c * M + r] = R[(((long long)seg * P + i) * P + j) * NL + (cc - a + flen - 1)];
    }
  }
  for (int e = 0; e < G; ++e)
    for (int r = tid; r < M; r += 1024) {
      const int i = base + r / flen, a = r % flen;
      x[e * M + r] = D[(((long long)seg * P + base + e) * P + i) * flen + a];
    }
  __syncthreads();
  bss_lu_solve(A, M, G, rowk, x, info + sys, C + (long long)sys * M * G);
}
static inline bool sg_args_ok(int32_t nseg, int32_t P, int32_t G, int32_t flen) {
  return nseg > 0 && P > 0 && P <= 8 && G > 0 && G <= P && P % G == 0 && flen > 0 && flen <= 512 && (long long)G * flen <= 2048 &&
         (long long)nseg * (P / G) <= 0x7fffffffLL;
}
extern "C" size_t avsep_bss_solve_groups_workspace_bytes(int32_t nseg, int32_t P, int32_t G, int32_t flen) {
  if (!sg_args_ok(nseg, P, G, flen)) return 0;
  const size_t M = (size_t)G * flen;
  return sizeof(double) * (size_t)nseg * (P / G) * M * M;
}
extern "C" int avsep_bss_solve_groups(const double* R, const double* D, int32_t nseg, int32_t P, int32_t G, int32_t flen, double* workspace,
                                      size_t workspace_bytes, double* C, int32_t* info, avsep_stream_t stream) {
  if (!R || !D || !workspace || !C || !info || !sg_args_ok(nseg, P, G, flen)) return AVSEP_ERR_ARG;
  if (workspace_bytes < avsep_bss_solve_groups_workspace_bytes(nseg, P, G, flen)) return AVSEP_ERR_WORKSPACE;
  const size_t lds = sizeof(double) * (size_t)G * flen * (1 + G);
  if (lds > 150 * 1024) return AVSEP_ERR_ARG;
  if (lds > 64 * 1024 &&
      hipFuncSetAttribute((const void*)bss_solve_groups_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return AVSEP_ERR_LAUNCH;
  hipLaunchKernelGGL(bss_solve_groups_kernel, dim3(nseg * (P / G)), dim3(1024), lds, (hipStream_t)stream, R, D, P, G, flen, workspace, C,
                     info);
  AVSEP_LAUNCH_CHECK();
  return AVSEP_OK;
}

// ---- 3. projections and residual energies of sample ranges ----------------------------------------------------------------------------
// Range rg = samples [off, off + rlen) of segment range_seg[rg] (relative to the segment's start; the projections live on
// [0, n + flen - 1), samples past that count as nothing).  For row q = j C + c of the range's segment and every sample t:
//   p_all = sum_p sum_k C_all[seg][(p,k)][q] r_p[t - k]           C_all [nseg][P * flen][P]
//   p_own = sum_i sum_k C_own[seg * S + j][(i,k)][c] r_{jC+i}[t - k]   C_own [nseg * S][C * flen][C]
//   s = r_q[t], e = e_q[t] (zero from n on), and the eight squares, each summed on its own
//   0: s^2   1: (e - s)^2   2: (p_own - s)^2   3: p_own^2   4: (p_all - p_own)^2   5: p_all^2   6: (e - p_all)^2   7: (e - p_own)^2
// (the image form uses 0 .. 6; mir_eval's SDR, sum 3 / sum 7, counts e_interf + e_artif = e - p_own as the distortion)
// grid (chunks of 1024 samples, P, ranges), 128 threads, a thread owns 8 consecutive samples.  The reference rows pass through
// LDS one at a time (window of 1024 + flen8 - 1 samples, padded by pad8, and that row's taps); per 8 taps a thread reads 8 new
// window values and 8 (16 on an own-source row) taps (a broadcast) for 64 (128) FMAs.  A block's sums (thread: ascending
// samples; wave: butterfly; waves: ascending) go to its slot of `part`; the reduce pass adds a range's slots, strided over the 64
// lanes of one wave in ascending order, then the butterfly: the order is a function of rlen alone.
constexpr int EN_OUT = 1024, EN_T = 8, EN_THREADS = 128, EN_TERMS = 8;

__global__ __launch_bounds__(EN_THREADS) void bss_win_energy_kernel(const double* __restrict__ refs, const double* __restrict__ ests, int P, int Cn,
                                                                    long long L, int flen, const long long* __restrict__ seg_starts, int nseg,
                                                                    long long n, const double* __restrict__ C_all,
                                                                    const double* __restrict__ C_own, const int* __restrict__ range_seg,
                                                                    const long long* __restrict__ range_off, long long rlen,
                                                                    double* __restrict__ part) {
  extern __shared__ __align__(16) double en_smem[];
  const int tid = threadIdx.x, q = blockIdx.y, rg = blockIdx.z, S = P / Cn, j = q / Cn, c = q % Cn;
  const int flen8 = (flen + EN_T - 1) / EN_T * EN_T, WN = EN_OUT + flen8;
  double* const rw = en_smem;                          // r_p[T0 - (flen8 - 1) ...], padded by pad8
  double* const ca = en_smem + pad8(WN) + 2;           // [flen8] taps of p_all, zero from flen on
  double* const co = ca + flen8;                       // [flen8] taps of p_own
  __shared__ double wsum[EN_THREADS / 64][EN_TERMS];
  double* const dst = part + (((long long)rg * gridDim.x + blockIdx.x) * P + q) * EN_TERMS;
  const int seg = range_seg[rg];
  if (seg < 0 || seg >= nseg) {                        // (uniform over the block)
    if (tid < EN_TERMS) dst[tid] = 0.0;
    return;
  }
  const long long sa = seg_starts[seg], off = range_off[rg];
  const long long T0 = off + (long long)blockIdx.x * EN_OUT;
  double pa[EN_T], po[EN_T];
#pragma unroll
  for (int i = 0; i < EN_T; ++i) pa[i] = po[i] = 0.0;

  for (int p = 0; p < P; ++p) {
    const bool own = p / Cn == j;
    const double* const r = refs + (long long)p * L;
    __syncthreads();
    for (int x = tid; x < WN; x += EN_THREADS) {
      const long long t = T0 - (flen8 - 1) + x, ta = sa + t;
      rw[pad8(x)] = (t >= 0 && t < n && ta >= 0 && ta < L) ? r[ta] : 0.0;
    }
    for (int k = tid; k < flen8; k += EN_THREADS) {
      ca[k] = k < flen ? C_all[(((long long)seg * P + p) * flen + k) * P + q] : 0.0;
      co[k] = (own && k < flen) ? C_own[((((long long)seg * S + j) * Cn + (p - j * Cn)) * flen + k) * Cn + c] : 0.0;
    }
    __syncthreads();
    // output i, tap k reads window index 8 tid + flen8 - 1 + i - k; rv[m] holds index b0 + m, b0 = 8 tid + flen8 - 8 - kb
    const double* rp = rw + pad8(EN_T * tid + flen8 - EN_T);
    double rv[2 * EN_T];
    lds_read8(rp, rv);
    lds_read8(rp + EN_T + 2, rv + EN_T);          // (the sixteenth value is never used)
    for (int kb = 0; kb < flen8; kb += EN_T) {
      double cv[EN_T];
      lds_read8(ca + kb, cv);
#pragma unroll
      for (int kk = 0; kk < EN_T; ++kk)
#pragma unroll
        for (int i = 0; i < EN_T; ++i) pa[i] = fma(cv[kk], rv[EN_T - 1 + i - kk], pa[i]);
      if (own) {
        lds_read8(co + kb, cv);
#pragma unroll
        for (int kk = 0; kk < EN_T; ++kk)
#pragma unroll
          for (int i = 0; i < EN_T; ++i) po[i] = fma(cv[kk], rv[EN_T - 1 + i - kk], po[i]);
      }
#pragma unroll
      for (int m = 0; m < EN_T; ++m) rv[EN_T + m] = rv[m];
      if (kb + EN_T < flen8) {
        rp -= EN_T + 2;
        lds_read8(rp, rv);
      }
    }
  }

  double sum[EN_TERMS];
#pragma unroll
  for (int m = 0; m < EN_TERMS; ++m) sum[m] = 0.0;
  const long long t_end = min(off + rlen, n + flen - 1);
#pragma unroll
  for (int i = 0; i < EN_T; ++i) {
    const long long t = T0 + EN_T * tid + i, ta = sa + t;
    if (t >= 0 && t < t_end) {
      const bool in = t < n && ta >= 0 && ta < L;
      const double s = in ? refs[(long long)q * L + ta] : 0.0, e = in ? ests[(long long)q * L + ta] : 0.0;
      const double d1 = e - s, d2 = po[i] - s, d4 = pa[i] - po[i], d6 = e - pa[i], d7 = e - po[i];
      sum[0] = fma(s, s, sum[0]);
      sum[1] = fma(d1, d1, sum[1]);
      sum[2] = fma(d2, d2, sum[2]);
      sum[3] = fma(po[i], po[i], sum[3]);
      sum[4] = fma(d4, d4, sum[4]);
      sum[5] = fma(pa[i], pa[i], sum[5]);
      sum[6] = fma(d6, d6, sum[6]);
      sum[7] = fma(d7, d7, sum[7]);
    }
  }
#pragma unroll
  for (int m = 0; m < EN_TERMS; ++m) {
    const double v = wave_sum_d(sum[m]);
    if ((tid & 63) == 0) wsum[tid >> 6][m] = v;
  }
  __syncthreads();
  if (tid < EN_TERMS) {
    double v = wsum[0][tid];
    for (int w = 1; w < EN_THREADS / 64; ++w) v += wsum[w][tid];
    dst[tid] = v;
  }
}

// grid (EN_TERMS, S, ranges), one wave: sums[rg][j][m] = sum over the range's chunks and the source's channels
__global__ __launch_bounds__(64) void bss_win_energy_reduce(const double* __restrict__ part, int P, int Cn, int nchunk, double* __restrict__ sums) {
  const int m = blockIdx.x, j = blockIdx.y, rg = blockIdx.z, S = P / Cn;
  double v = 0.0;
  for (int ch = threadIdx.x; ch < nchunk; ch += 64)
    for (int c = 0; c < Cn; ++c) v += part[(((long long)rg * nchunk + ch) * P + j * Cn + c) * EN_TERMS + m];
  v = wave_sum_d(v);
  if (threadIdx.x == 0) sums[((long long)rg * S + j) * EN_TERMS + m] = v;
}

static inline bool en_args_ok(int32_t nrange, int32_t P, int64_t rlen) {
  return nrange > 0 && nrange <= 65535 && P > 0 && P <= 8 && rlen > 0 && (rlen + EN_OUT - 1) / EN_OUT <= 0x7fffffffLL;
}
extern "C" size_t avsep_bss_window_energies_workspace_bytes(int32_t nrange, int32_t P, int64_t rlen) {
  if (!en_args_ok(nrange, P, rlen)) return 0;
  return sizeof(double) * (size_t)nrange * (size_t)((rlen + EN_OUT - 1) / EN_OUT) * P * EN_TERMS;
}
extern "C" int avsep_bss_window_energies(const double* refs, const double* ests, int32_t P, int32_t C, int64_t L, int32_t flen,
                                         const int64_t* seg_starts, int32_t nseg, int64_t n, const double* C_all, const double* C_own,
                                         const int32_t* range_seg, const int64_t* range_off, int32_t nrange, int64_t rlen,
                                         double* workspace, size_t workspace_bytes, double* sums, avsep_stream_t stream) {
  if (!refs || !ests || !seg_starts || !C_all || !C_own || !range_seg || !range_off || !workspace || !sums || !en_args_ok(nrange, P, rlen) ||
      C <= 0 || P % C != 0 || L <= 0 || flen <= 0 || flen > 512 || nseg <= 0 || n <= 0)
    return AVSEP_ERR_ARG;
  if (workspace_bytes < avsep_bss_window_energies_workspace_bytes(nrange, P, rlen)) return AVSEP_ERR_WORKSPACE;
  const int nchunk = (int)((rlen + EN_OUT - 1) / EN_OUT), flen8 = (flen + EN_T - 1) / EN_T * EN_T, WN = EN_OUT + flen8;
  const size_t lds = sizeof(double) * (size_t)(WN + WN / 8 * 2 + 2 + 2 * flen8);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(bss_win_energy_kernel, dim3(nchunk, P, nrange), dim3(EN_THREADS), lds, st, refs, ests, P, C, (long long)L, flen,
                     (const long long*)seg_starts, nseg, (long long)n, C_all, C_own, range_seg, (const long long*)range_off,
                     (long long)rlen, workspace);
  AVSEP_LAUNCH_CHECK();
  hipLaunchKernelGGL(bss_win_energy_reduce, dim3(EN_TERMS, P / C, nrange), dim3(64), 0, st, workspace, P, C, nchunk, sums);
  AVSEP_LAUNCH_CHECK();
  return AVSEP_OK;
}
