// Multichannel Wiener filter over a recording's stitched source images (include/avsep.h): per-bin spatial covariances of
// every source, then one Hermitian solve per time-frequency bin.  Two HBM-bound kernels and a tiny one between them; time is
// the contiguous axis of every tensor and lanes run along it.  The time-invariant filter and the one with
// time-varying covariances (§24) are the two instantiations, TV = false and TV = true, of one partial-sum kernel template
// and one apply kernel template, and their finishing kernels share mwf_finish_entry.
// No atomics in this file: every sum has a fixed order (a thread's chain in ascending t, the wave's butterfly, the four
// waves in ascending order, the chunk slabs in ascending order), so a second run gives the same bits.
#include <float.h>
#include <type_traits>
#include "common.h"

constexpr int MWF_BLOCK = 256;
constexpr int MWF_WAVES = MWF_BLOCK / 64;
constexpr int MWF_CHUNK = 2048;   // frames per covariance workgroup: a constant, so the summation order is a function of F only
constexpr int MWF_MAX_C = 8;      // resample.MAX_KEPT_CHANNELS
constexpr int MWF_MAX_N = 8;

// floats of one partial slab: the lower triangle of sum_t Y Y^H as (re, im) pairs, row-major (r >= c at r*(r+1)/2 + c), then
// sum_t v
static inline int mwf_nacc(int C) { return C * (C + 1) + 1; }
static inline long long mwf_chunks(int F) { return ((long long)F + MWF_CHUNK - 1) / MWF_CHUNK; }

static bool mwf_dims_ok(int N, int C, int Fin, int F) {
  return N > 0 && N <= MWF_MAX_N && C > 0 && C <= MWF_MAX_C && Fin > 0 && Fin <= 65535 && F > 0 && F <= 0x7fffffff - 2 * MWF_CHUNK;
}

// The run-time C in 1 ... 8 as a compile-time constant: launch(std::integral_constant<int, C>{}).  mwf_dims_ok has refused
// every other C before an entry point gets here, so default: is 8.
template <class Launch>
static void mwf_with_channels(int C, Launch launch) {
  switch (C) {
    case 1: launch(std::integral_constant<int, 1>{}); break;
    case 2: launch(std::integral_constant<int, 2>{}); break;
    case 3: launch(std::integral_constant<int, 3>{}); break;
    case 4: launch(std::integral_constant<int, 4>{}); break;
    case 5: launch(std::integral_constant<int, 5>{}); break;
    case 6: launch(std::integral_constant<int, 6>{}); break;
    case 7: launch(std::integral_constant<int, 7>{}); break;
    default: launch(std::integral_constant<int, 8>{}); break;
  }
}

extern "C" size_t avsep_mwf_workspace_bytes(int32_t N, int32_t C, int32_t Fin, int32_t F) {
  if (!mwf_dims_ok(N, C, Fin, F)) return 0;
  return (size_t)mwf_chunks(F) * N * Fin * mwf_nacc(C) * sizeof(float);
}

// ============================================================================
// covariance: partial slabs per (chunk, source, bin row), then their sum, normalised
// ============================================================================
// Entry (r, c) of one normalised covariance, for both finishing kernels (one wave): thread r*C + c has sum(i, nacc, re,
// im, den) add up, in the caller's order, floats i and i + 1 (the entry's pair in the lower triangle) and nacc - 1 (sum v)
// of the caller's slabs of nacc floats, divides by max(den, FLT_MIN) (a silent source gives R = 0) and stores to out
// [C, C, 2].  The upper triangle is the conjugate of the lower one, the diagonal is real.
template <class Sum>
__device__ __forceinline__ void mwf_finish_entry(int C, float* __restrict__ out, Sum sum) {
  if ((int)threadIdx.x >= C * C) return;
  const int r = threadIdx.x / C, c = threadIdx.x - r * C;
  const int lo = max(r, c), hi = min(r, c), i = 2 * (lo * (lo + 1) / 2 + hi), nacc = C * (C + 1) + 1;
  float re = 0.f, im = 0.f, den = 0.f;
  sum(i, nacc, re, im, den);
  den = fmaxf(den, FLT_MIN);
  float* __restrict__ o = out + 2 * (r * C + c);
  o[0] = re / den;
  o[1] = r == c ? 0.f : (r > c ? im : -im) / den;
}

// One partial-sum kernel template for both covariances.  A unit of work is a run of frames [t0, t0 + len) of one (source,
// bin row); `step` threads walk it in ascending t, each with the lower triangle's C*(C+1)/2 complex products and v in
// registers.  phase_stride is 0 when the N sources share one phase tensor [C, Fin, F].
// TV = false (§16): grid (chunks, Fin, N).  The unit is a chunk of MWF_CHUNK frames and the whole workgroup walks it.  The
// waves are reduced by the xor butterfly and summed in ascending order through LDS: one slab ws[chunk][n][f][NACC].  H and
// segments are not read.
// TV = true (§24): grid (ceil(segments / 4), Fin, N), ONE WAVE PER SEGMENT of H frames.  Its lanes keep two slabs, the
// (1 - u)-weighted sums (for centre s) and the u-weighted sums (for centre s + 1) of the rounded per-frame terms.  The wave
// is reduced by the butterfly and writes its 2 * NACC floats to ws[segment][n][f][2][NACC]; nothing is shared between the
// waves of a workgroup.  The order of every sum depends on (F, H) alone.
// The per-frame terms stand here once, in the kernel and not in a function it calls, for the reason given at
// mwf_apply_kernel: the compiler treats a callee on its own first, which cost registers, a wave of occupancy at two C, and time.
template <int C, bool TV>
__global__ __launch_bounds__(MWF_BLOCK) void mwf_cov_partial_kernel(const float* __restrict__ ymag, const float* __restrict__ yph,
                                                                    long long phase_stride, int Fin, int F, int H, int segments,
                                                                    float* __restrict__ ws) {
#pragma clang fp contract(off)
  constexpr int NACC = C * (C + 1) + 1;
  const int lane = threadIdx.x & 63;
  const int unit = TV ? blockIdx.x * MWF_WAVES + (threadIdx.x >> 6) : blockIdx.x;
  if (TV && unit >= segments) return;                            // the whole wave; the TV kernel has no barrier
  const int f = blockIdx.y, n = blockIdx.z, N = gridDim.z;
  const long long plane = (long long)Fin * F;
  const float* __restrict__ m = ymag + (long long)n * C * plane + (long long)f * F;
  const float* __restrict__ p = yph + (long long)n * phase_stride + (long long)f * F;
  // unit * span < F, F <= INT_MAX - 2 * MWF_CHUNK and span <= 4096: neither t0 + span nor j += step wraps
  const int span = TV ? H : MWF_CHUNK, t0 = unit * span, len = min(span, F - t0);
  const float fH = (float)H;
  float acc[NACC], accB[TV ? NACC : 1];                          // TV: acc is the (1 - u) slab, accB the u slab
#pragma unroll
  for (int i = 0; i < NACC; ++i) acc[i] = accB[TV ? i : 0] = 0.f;
  for (int j = TV ? lane : (int)threadIdx.x; j < len; j += TV ? 64 : MWF_BLOCK) {
    const int t = t0 + j;
    const float u = (float)j / fH, w = 1.f - u;                  // TV only
    auto add = [&](int i, float x) {
      if constexpr (TV) {
        acc[i] += w * x;
        accB[i] += u * x;
      } else {
        acc[i] += x;
      }
    };
    float re[C], im[C], sq = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float a = m[c * plane + t];
      float sn, cs;
      sincosf(p[c * plane + t], &sn, &cs);
      re[c] = a * cs;
      im[c] = a * sn;
      sq += a * a;
    }
    add(NACC - 1, sq * (1.f / C));
#pragma unroll
    for (int r = 0; r < C; ++r) {
#pragma unroll
      for (int c = 0; c <= r; ++c) {
        const int i = 2 * (r * (r + 1) / 2 + c);
        // Y_r conj(Y_c).  Contraction is off in this kernel and the one fused multiply-add is spelt out, so the roundings do
        // not depend on how the compiler treats each entry: two equal channels give four equal real parts and (both
        // products rounded) an imaginary part of exactly 0, before a weight and so after it, and a dual-mono recording
        // equal output channels.  A diagonal entry is real.
        add(i, fmaf(re[r], re[c], im[r] * im[c]));
        if (c < r) add(i + 1, im[r] * re[c] - re[r] * im[c]);
      }
    }
  }
  if constexpr (TV) {
    // lane i of output q keeps sum number 64 q + i: coalesced stores, and no register array indexed at run time
    constexpr int NOUT = (2 * NACC + 63) / 64;
    float o[NOUT];
#pragma unroll
    for (int q = 0; q < NOUT; ++q) o[q] = 0.f;
#pragma unroll
    for (int i = 0; i < 2 * NACC; ++i) {
      const float s = wave_sum(i < NACC ? acc[i < NACC ? i : 0] : accB[i < NACC ? 0 : i - NACC]);
      if ((i & 63) == lane) o[i >> 6] = s;
    }
    float* __restrict__ dst = ws + (((long long)unit * N + n) * Fin + f) * (2 * NACC);
#pragma unroll
    for (int q = 0; q < NOUT; ++q)
      if (q * 64 + lane < 2 * NACC) dst[q * 64 + lane] = o[q];
  } else {
    __shared__ float s_part[MWF_WAVES][NACC];
#pragma unroll
    for (int i = 0; i < NACC; ++i) {
      const float s = wave_sum(acc[i]);
      if (lane == 0) s_part[threadIdx.x >> 6][i] = s;
    }
    __syncthreads();
    if (threadIdx.x < NACC) {
      float s = s_part[0][threadIdx.x];
      for (int w = 1; w < MWF_WAVES; ++w) s += s_part[w][threadIdx.x];
      ws[(((long long)unit * N + n) * Fin + f) * NACC + threadIdx.x] = s;
    }
  }
}

// grid (Fin, N), one wave: entry (r, c) is the sum of the slabs in ascending chunk order over max(sum_t v, FLT_MIN).
__global__ __launch_bounds__(64) void mwf_cov_finish_kernel(const float* __restrict__ ws, int chunks, int C, int Fin,
                                                            float* __restrict__ cov) {
  const int f = blockIdx.x, n = blockIdx.y, N = gridDim.y;
  mwf_finish_entry(C, cov + 2 * ((long long)n * Fin + f) * C * C, [&](int i, int nacc, float& re, float& im, float& den) {
    for (int k = 0; k < chunks; ++k) {
      const float* __restrict__ s = ws + (((long long)k * N + n) * Fin + f) * nacc;
      re += s[i];
      im += s[i + 1];
      den += s[nacc - 1];
    }
  });
}

extern "C" int avsep_mwf_cov(const float* ymag, const float* yph, int32_t phase_per_source, int32_t N, int32_t C, int32_t Fin,
                             int32_t F, float* cov, float* ws, size_t ws_bytes, avsep_stream_t stream) {
  if (!ymag || !yph || !cov || !ws) return AVSEP_ERR_ARG;
  if (!mwf_dims_ok(N, C, Fin, F) || ws_bytes < avsep_mwf_workspace_bytes(N, C, Fin, F)) return AVSEP_ERR_ARG;
  const long long stride = phase_per_source ? (long long)C * Fin * F : 0;
  hipStream_t s = (hipStream_t)stream;
  mwf_with_channels(C, [&](auto c) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(mwf_cov_partial_kernel<decltype(c)::value, false>), dim3((unsigned)mwf_chunks(F), Fin, N),
                       dim3(MWF_BLOCK), 0, s, ymag, yph, stride, Fin, F, 0, 0, ws);
  });
  AVSEP_LAUNCH_CHECK();
  hipLaunchKernelGGL(mwf_cov_finish_kernel, dim3(Fin, N), dim3(64), 0, s, ws, (int)mwf_chunks(F), C, Fin, cov);
  AVSEP_LAUNCH_CHECK();
  return AVSEP_OK;
}

// ============================================================================
// time-varying covariances: one R_n per centre k H and bin row, blended between the two centres next to a frame
// ============================================================================
// H, the span, is a multiple of 64 in 64 ... 4096.  Frame t lies in segment s = t / H at u = (t - s H) / H; centre s weighs
// it with 1 - u and centre s + 1 with u.  A wave of 64 consecutive frames that starts at a multiple of 64 lies in one
// segment, so s is wave-uniform everywhere below and only u differs per lane.
constexpr int MWF_TV_MIN_SPAN = 64;
constexpr int MWF_TV_MAX_SPAN = 4096;
constexpr int MWF_TV_TILE_CENTRES = MWF_BLOCK / MWF_TV_MIN_SPAN + 1;   // a 256-frame tile meets at most 4 segments: 5 centres

static bool mwf_span_ok(int H) { return H >= MWF_TV_MIN_SPAN && H <= MWF_TV_MAX_SPAN && H % 64 == 0; }
static inline long long mwf_tv_segments(int F, int H) { return ((long long)F + H - 1) / H; }
// ceil((F - 1) / H) + 1: the last centre is the first one at or past the last frame (one centre for one frame)
static inline long long mwf_tv_centres(int F, int H) { return F == 1 ? 1 : ((long long)F + H - 2) / H + 1; }

extern "C" size_t avsep_mwf_tv_workspace_bytes(int32_t N, int32_t C, int32_t Fin, int32_t F, int32_t H) {
  if (!mwf_dims_ok(N, C, Fin, F) || !mwf_span_ok(H)) return 0;
  return (size_t)mwf_tv_segments(F, H) * N * Fin * 2 * mwf_nacc(C) * sizeof(float);
}

// grid (K, Fin, N), one wave: entry (r, c) of centre k is A_k + B_{k-1}, in that order (segment k's (1 - u) slab, then
// segment k - 1's u slab; the first centre has no B, a centre past the last segment no A), over max(sum w v, FLT_MIN): a
// source that is silent over the centre's support gives R = 0 there.
__global__ __launch_bounds__(64) void mwf_cov_tv_finish_kernel(const float* __restrict__ ws, int segments, int C, int Fin,
                                                               float* __restrict__ cov) {
  const int k = blockIdx.x, K = gridDim.x, f = blockIdx.y, n = blockIdx.z, N = gridDim.z;
  mwf_finish_entry(C, cov + 2 * (((long long)n * K + k) * Fin + f) * C * C, [&](int i, int nacc, float& re, float& im, float& den) {
    if (k < segments) {
      const float* __restrict__ a = ws + (((long long)k * N + n) * Fin + f) * (2 * nacc);
      re = a[i];
      im = a[i + 1];
      den = a[nacc - 1];
    }
    if (k >= 1) {                                               // K <= segments + 1: segment k - 1 exists
      const float* __restrict__ b = ws + (((long long)(k - 1) * N + n) * Fin + f) * (2 * nacc) + nacc;
      re += b[i];
      im += b[i + 1];
      den += b[nacc - 1];
    }
  });
}

extern "C" int avsep_mwf_cov_tv(const float* ymag, const float* yph, int32_t phase_per_source, int32_t N, int32_t C, int32_t Fin,
                                int32_t F, int32_t H, float* cov, float* ws, size_t ws_bytes, avsep_stream_t stream) {
  if (!ymag || !yph || !cov || !ws) return AVSEP_ERR_ARG;
  if (!mwf_dims_ok(N, C, Fin, F) || !mwf_span_ok(H) || ws_bytes < avsep_mwf_tv_workspace_bytes(N, C, Fin, F, H)) return AVSEP_ERR_ARG;
  const long long stride = phase_per_source ? (long long)C * Fin * F : 0;
  const int segments = (int)mwf_tv_segments(F, H);
  hipStream_t s = (hipStream_t)stream;
  mwf_with_channels(C, [&](auto c) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(mwf_cov_partial_kernel<decltype(c)::value, true>), dim3(cdiv(segments, MWF_WAVES), Fin, N),
                       dim3(MWF_BLOCK), 0, s, ymag, yph, stride, Fin, F, H, segments, ws);
  });
  AVSEP_LAUNCH_CHECK();
  hipLaunchKernelGGL(mwf_cov_tv_finish_kernel, dim3((unsigned)mwf_tv_centres(F, H), Fin, N), dim3(64), 0, s, ws, segments, C, Fin,
                     cov);
  AVSEP_LAUNCH_CHECK();
  return AVSEP_OK;
}

// ============================================================================
// apply: S = sum_n v_n R_n + lambda I, Cholesky, S z = X, Y_n' = v_n R_n z
// ============================================================================
// grid (ceil(F / 256), Fin), one kernel template for both filters; a thread owns one (f, t).  The two differ in where an
// entry of R_n comes from, which is what TV selects at compile time: its staging in LDS, and the accessor R.
// TV = false (§16): R_n[f] of all sources sits in LDS, and an entry is one word of it (every lane reads the same word: a
// broadcast); H and K are not read.
// TV = true (§24): the tile's (at most) five centres k0 ... k0 + 4 of all sources sit in LDS, centre indices clamped to
// K - 1 (a clamped centre is only ever read with weight u = 0).  A wave's segment, and with it the pair of centres it
// reads, is uniform: every LDS read stays a broadcast.  An entry of R_n[f,t] is formed as (1 - u) R[s] + u R[s + 1] where
// it is used, once for S and once for v_n R_n z; no blended copy is kept.
// Steps 3 to 5 stand here once, in the kernel and not in a function it calls: a callee is optimised on its own before it
// is inlined, and that moved the compiler's choice of which products to fuse, and with it the bits of the time-invariant
// filter.  The thread keeps the lower triangle of S, then of its Cholesky factor, in registers (every loop below is
// unrolled: no array is indexed at run time).  The diagonal of a Hermitian matrix is real: its imaginary parts are neither
// kept nor read.
template <int C, bool TV>
__global__ __launch_bounds__(MWF_BLOCK) void mwf_apply_kernel(const float* __restrict__ xmag, const float* __restrict__ xph,
                                                              const float* __restrict__ ymag, const float* __restrict__ cov,
                                                              int N, int Fin, int F, int H, int K, float reg,
                                                              float* __restrict__ out_mag, float* __restrict__ out_phase) {
  constexpr int TRI = C * (C + 1) / 2;
  constexpr int RC = C * C * 2;
  __shared__ float s_R[(TV ? MWF_TV_TILE_CENTRES : 1) * MWF_MAX_N * RC];
  const int f = blockIdx.y, tile0 = blockIdx.x * MWF_BLOCK, t = tile0 + threadIdx.x;
  const int k0 = TV ? tile0 / H : 0, per = N * RC;
  if constexpr (TV) {
    for (int i = threadIdx.x; i < MWF_TV_TILE_CENTRES * per; i += MWF_BLOCK) {
      const int j = i / per, rest = i - j * per, n = rest / RC, e = rest - n * RC;
      const int k = min(k0 + j, K - 1);
      s_R[i] = cov[(((long long)n * K + k) * Fin + f) * RC + e];
    }
  } else {
    for (int i = threadIdx.x; i < per; i += MWF_BLOCK) {
      const int n = i / RC, j = i - n * RC;
      s_R[i] = cov[((long long)n * Fin + f) * RC + j];
    }
  }
  __syncthreads();
  if (t >= F) return;
  const long long plane = (long long)Fin * F, ft = (long long)f * F + t;
  // the wave's first frame is a multiple of 64 and H is one: all 64 frames lie in segment seg
  const int seg = TV ? __builtin_amdgcn_readfirstlane((tile0 + (int)(threadIdx.x & ~63u)) / H) : 0;
  const float u = TV ? (float)(t - seg * H) / (float)H : 0.f, w = 1.f - u;
  const float* Ra = s_R + (seg - k0) * per;                    // seg - k0 in 0 ... 3
  const float* Rb = Ra + per;
  // float e of source n's covariance [C, C, 2] at this bin
  auto R = [&](int n, int e) {
    if constexpr (TV) return w * Ra[n * RC + e] + u * Rb[n * RC + e];
    else return s_R[n * RC + e];
  };

  float v[MWF_MAX_N];
#pragma unroll
  for (int n = 0; n < MWF_MAX_N; ++n) {
    v[n] = 0.f;
    if (n < N) {
      float sq = 0.f;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const float a = ymag[((long long)n * C + c) * plane + ft];
        sq += a * a;
      }
      v[n] = sq * (1.f / C);
    }
  }
  // S, lower triangle
  float Sr[TRI], Si[TRI];
#pragma unroll
  for (int i = 0; i < TRI; ++i) Sr[i] = Si[i] = 0.f;
#pragma unroll
  for (int n = 0; n < MWF_MAX_N; ++n) {
    if (n < N) {
#pragma unroll
      for (int r = 0; r < C; ++r)
#pragma unroll
        for (int c = 0; c <= r; ++c) {
          Sr[r * (r + 1) / 2 + c] += v[n] * R(n, 2 * (r * C + c));
          if (c < r) Si[r * (r + 1) / 2 + c] += v[n] * R(n, 2 * (r * C + c) + 1);
        }
    }
  }
  float tr = 0.f;
#pragma unroll
  for (int r = 0; r < C; ++r) tr += Sr[r * (r + 1) / 2 + r];
  const float lam = reg * tr * (1.f / C) + FLT_MIN;
#pragma unroll
  for (int r = 0; r < C; ++r) Sr[r * (r + 1) / 2 + r] += lam;
  // S = L L^H in place (Cholesky-Crout, column by column); dinv[j] = 1 / L[j][j]
  float dinv[C];
#pragma unroll
  for (int j = 0; j < C; ++j) {
    float d = Sr[j * (j + 1) / 2 + j];
#pragma unroll
    for (int k = 0; k < j; ++k) {
      const int jk = j * (j + 1) / 2 + k;
      d -= Sr[jk] * Sr[jk] + Si[jk] * Si[jk];
    }
    dinv[j] = 1.f / sqrtf(fmaxf(d, FLT_MIN));                       // reg > 0 keeps d far above rounding; never a NaN
#pragma unroll
    for (int i = j + 1; i < C; ++i) {
      const int ij = i * (i + 1) / 2 + j;
      float ar = Sr[ij], ai = Si[ij];
#pragma unroll
      for (int k = 0; k < j; ++k) {                                    // - L[i][k] conj(L[j][k])
        const int ik = i * (i + 1) / 2 + k, jk = j * (j + 1) / 2 + k;
        ar -= Sr[ik] * Sr[jk] + Si[ik] * Si[jk];
        ai -= Si[ik] * Sr[jk] - Sr[ik] * Si[jk];
      }
      Sr[ij] = ar * dinv[j];
      Si[ij] = ai * dinv[j];
    }
  }
  // L y = X, forward
  float zr[C], zi[C];
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const float a = xmag[c * plane + ft];
    float sn, cs;
    sincosf(xph[c * plane + ft], &sn, &cs);
    zr[c] = a * cs;
    zi[c] = a * sn;
  }
#pragma unroll
  for (int i = 0; i < C; ++i) {
#pragma unroll
    for (int k = 0; k < i; ++k) {
      const int ik = i * (i + 1) / 2 + k;
      zr[i] -= Sr[ik] * zr[k] - Si[ik] * zi[k];
      zi[i] -= Sr[ik] * zi[k] + Si[ik] * zr[k];
    }
    zr[i] *= dinv[i];
    zi[i] *= dinv[i];
  }
  // L^H z = y, backward
#pragma unroll
  for (int i = C - 1; i >= 0; --i) {
#pragma unroll
    for (int k = i + 1; k < C; ++k) {                                  // - conj(L[k][i]) z[k]
      const int ki = k * (k + 1) / 2 + i;
      zr[i] -= Sr[ki] * zr[k] + Si[ki] * zi[k];
      zi[i] -= Sr[ki] * zi[k] - Si[ki] * zr[k];
    }
    zr[i] *= dinv[i];
    zi[i] *= dinv[i];
  }
  // Y_n' = v_n R_n z.  v_n == 0 is an exact zero whatever z is (all sources silent at a bin the mixture is not: z overflows)
#pragma unroll
  for (int n = 0; n < MWF_MAX_N; ++n) {
    if (n < N) {
#pragma unroll
      for (int r = 0; r < C; ++r) {
        float wr = 0.f, wi = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) {
          const float rr = R(n, 2 * (r * C + c)), ri = R(n, 2 * (r * C + c) + 1);
          wr += rr * zr[c] - ri * zi[c];
          wi += rr * zi[c] + ri * zr[c];
        }
        const bool on = v[n] != 0.f;
        wr = on ? v[n] * wr : 0.f;
        wi = on ? v[n] * wi : 0.f;
        const long long o = ((long long)n * C + r) * plane + ft;
        out_mag[o] = sqrtf(wr * wr + wi * wi);
        out_phase[o] = (wr == 0.f && wi == 0.f) ? 0.f : atan2f(wi, wr);
      }
    }
  }
}

extern "C" int avsep_mwf_apply(const float* xmag, const float* xph, const float* ymag, const float* cov, int32_t N, int32_t C,
                               int32_t Fin, int32_t F, float reg, float* out_mag, float* out_phase, avsep_stream_t stream) {
  if (!xmag || !xph || !ymag || !cov || !out_mag || !out_phase) return AVSEP_ERR_ARG;
  if (!mwf_dims_ok(N, C, Fin, F) || !(reg >= 0.f)) return AVSEP_ERR_ARG;
  mwf_with_channels(C, [&](auto c) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(mwf_apply_kernel<decltype(c)::value, false>), dim3(cdiv(F, MWF_BLOCK), Fin),
                       dim3(MWF_BLOCK), 0, (hipStream_t)stream, xmag, xph, ymag, cov, N, Fin, F, 0, 1, reg, out_mag, out_phase);
  });
  AVSEP_LAUNCH_CHECK();
  return AVSEP_OK;
}

extern "C" int avsep_mwf_apply_tv(const float* xmag, const float* xph, const float* ymag, const float* cov, int32_t N, int32_t C,
                                  int32_t Fin, int32_t F, int32_t H, float reg, float* out_mag, float* out_phase,
                                  avsep_stream_t stream) {
  if (!xmag || !xph || !ymag || !cov || !out_mag || !out_phase) return AVSEP_ERR_ARG;
  if (!mwf_dims_ok(N, C, Fin, F) || !mwf_span_ok(H) || !(reg >= 0.f)) return AVSEP_ERR_ARG;
  mwf_with_channels(C, [&](auto c) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(mwf_apply_kernel<decltype(c)::value, true>), dim3(cdiv(F, MWF_BLOCK), Fin),
                       dim3(MWF_BLOCK), 0, (hipStream_t)stream, xmag, xph, ymag, cov, N, Fin, F, H, (int)mwf_tv_centres(F, H), reg,
                       out_mag, out_phase);
  });
  AVSEP_LAUNCH_CHECK();
  return AVSEP_OK;
}
