// Multichannel Wiener filter over a recording's stitched source images (include/avsep.h): per-bin spatial covariances of
// every source, then one Hermitian solve per time-frequency bin.  Two HBM-bound kernels and a tiny one between them; time is
// the contiguous axis of every tensor and lanes run along it.
// No atomics in this file: every sum has a fixed order (a thread's chain in ascending t, the wave's butterfly, the four
// waves in ascending order, the chunk slabs in ascending order), so a second run gives the same bits.
#include <float.h>
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

extern "C" size_t avsep_mwf_workspace_bytes(int32_t N, int32_t C, int32_t Fin, int32_t F) {
  if (!mwf_dims_ok(N, C, Fin, F)) return 0;
  return (size_t)mwf_chunks(F) * N * Fin * mwf_nacc(C) * sizeof(float);
}

// ============================================================================
// covariance: partial slabs per (chunk, source, bin row), then their sum, normalised
// ============================================================================
// grid (chunks, Fin, N).  A thread walks its frames of the chunk in ascending t with C*(C+1)/2 complex products and v in
// registers; phase_stride is 0 when the N sources share one phase tensor [C, Fin, F].
template <int C>
__global__ __launch_bounds__(MWF_BLOCK) void mwf_cov_partial_kernel(const float* __restrict__ ymag, const float* __restrict__ yph,
                                                                    long long phase_stride, int Fin, int F,
                                                                    float* __restrict__ ws) {
#pragma clang fp contract(off)
  constexpr int NACC = C * (C + 1) + 1;
  const int chunk = blockIdx.x, f = blockIdx.y, n = blockIdx.z, N = gridDim.z;
  const long long plane = (long long)Fin * F;
  const float* __restrict__ m = ymag + (long long)n * C * plane + (long long)f * F;
  const float* __restrict__ p = yph + (long long)n * phase_stride + (long long)f * F;
  const int t_end = min((chunk + 1) * MWF_CHUNK, F);       // F <= INT_MAX - 2 * MWF_CHUNK: neither this nor t += MWF_BLOCK wraps
  float acc[NACC];
#pragma unroll
  for (int i = 0; i < NACC; ++i) acc[i] = 0.f;
  for (int t = chunk * MWF_CHUNK + threadIdx.x; t < t_end; t += MWF_BLOCK) {
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
    acc[NACC - 1] += sq * (1.f / C);
#pragma unroll
    for (int r = 0; r < C; ++r) {
#pragma unroll
      for (int c = 0; c <= r; ++c) {
        const int i = 2 * (r * (r + 1) / 2 + c);
        // Y_r conj(Y_c).  Contraction is off in this kernel and the one fused multiply-add is spelt out, so the roundings do
        // not depend on how the compiler treats each entry: two equal channels give four equal real parts and (both
        // products rounded) an imaginary part of exactly 0, and a dual-mono recording equal output channels.  A diagonal
        // entry is real.
        acc[i] += fmaf(re[r], re[c], im[r] * im[c]);
        if (c < r) acc[i + 1] += im[r] * re[c] - re[r] * im[c];
      }
    }
  }
  __shared__ float s_part[MWF_WAVES][NACC];
#pragma unroll
  for (int i = 0; i < NACC; ++i) {
    const float s = wave_sum(acc[i]);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6][i] = s;
  }
  __syncthreads();
  if (threadIdx.x < NACC) {
    float s = s_part[0][threadIdx.x];
    for (int w = 1; w < MWF_WAVES; ++w) s += s_part[w][threadIdx.x];
    ws[(((long long)chunk * N + n) * Fin + f) * NACC + threadIdx.x] = s;
  }
}

// grid (Fin, N), one wave: thread r*C + c sums entry (r, c) of the slabs in ascending chunk order and divides by
// max(sum_t v, FLT_MIN): a silent source gives R = 0.  The upper triangle is the conjugate of the lower one.
__global__ __launch_bounds__(64) void mwf_cov_finish_kernel(const float* __restrict__ ws, int chunks, int C, int Fin,
                                                            float* __restrict__ cov) {
  const int f = blockIdx.x, n = blockIdx.y, N = gridDim.y;
  if ((int)threadIdx.x >= C * C) return;
  const int r = threadIdx.x / C, c = threadIdx.x - r * C;
  const int lo = max(r, c), hi = min(r, c), i = 2 * (lo * (lo + 1) / 2 + hi), nacc = C * (C + 1) + 1;
  float re = 0.f, im = 0.f, den = 0.f;
  for (int k = 0; k < chunks; ++k) {
    const float* __restrict__ s = ws + (((long long)k * N + n) * Fin + f) * nacc;
    re += s[i];
    im += s[i + 1];
    den += s[nacc - 1];
  }
  den = fmaxf(den, FLT_MIN);
  float* __restrict__ o = cov + 2 * ((((long long)n * Fin + f) * C + r) * C + c);
  o[0] = re / den;
  o[1] = r == c ? 0.f : (r > c ? im : -im) / den;
}

template <int C>
static void mwf_cov_launch(const float* ymag, const float* yph, long long phase_stride, int N, int Fin, int F, float* ws,
                           hipStream_t stream) {
  hipLaunchKernelGGL(mwf_cov_partial_kernel<C>, dim3((unsigned)mwf_chunks(F), Fin, N), dim3(MWF_BLOCK), 0, stream, ymag, yph,
                     phase_stride, Fin, F, ws);
}

extern "C" int avsep_mwf_cov(const float* ymag, const float* yph, int32_t phase_per_source, int32_t N, int32_t C, int32_t Fin,
                             int32_t F, float* cov, float* ws, size_t ws_bytes, avsep_stream_t stream) {
  if (!ymag || !yph || !cov || !ws) return AVSEP_ERR_ARG;
  if (!mwf_dims_ok(N, C, Fin, F) || ws_bytes < avsep_mwf_workspace_bytes(N, C, Fin, F)) return AVSEP_ERR_ARG;
  const long long stride = phase_per_source ? (long long)C * Fin * F : 0;
  hipStream_t s = (hipStream_t)stream;
  switch (C) {
    case 1: mwf_cov_launch<1>(ymag, yph, stride, N, Fin, F, ws, s); break;
    case 2: mwf_cov_launch<2>(ymag, yph, stride, N, Fin, F, ws, s); break;
    case 3: mwf_cov_launch<3>(ymag, yph, stride, N, Fin, F, ws, s); break;
    case 4: mwf_cov_launch<4>(ymag, yph, stride, N, Fin, F, ws, s); break;
    case 5: mwf_cov_launch<5>(ymag, yph, stride, N, Fin, F, ws, s); break;
    case 6: mwf_cov_launch<6>(ymag, yph, stride, N, Fin, F, ws, s); break;
    case 7: mwf_cov_launch<7>(ymag, yph, stride, N, Fin, F, ws, s); break;
    default: mwf_cov_launch<8>(ymag, yph, stride, N, Fin, F, ws, s); break;
  }
  AVSEP_LAUNCH_CHECK();
  hipLaunchKernelGGL(mwf_cov_finish_kernel, dim3(Fin, N), dim3(64), 0, s, ws, (int)mwf_chunks(F), C, Fin, cov);
  AVSEP_LAUNCH_CHECK();
  return AVSEP_OK;
}

// ============================================================================
// apply: S = sum_n v_n R_n + lambda I, Cholesky, S z = X, Y_n' = v_n R_n z
// ============================================================================
// grid (ceil(F / 256), Fin).  R_n[f] of all sources sits in LDS (every lane reads the same word: a broadcast); a thread owns
// one (f, t) and keeps the lower triangle of S, then of its Cholesky factor, in registers (every loop below is unrolled: no
// array is indexed at run time).  The diagonal of a Hermitian matrix is real: its imaginary parts are neither kept nor read.
template <int C>
__global__ __launch_bounds__(MWF_BLOCK) void mwf_apply_kernel(const float* __restrict__ xmag, const float* __restrict__ xph,
                                                              const float* __restrict__ ymag, const float* __restrict__ cov,
                                                              int N, int Fin, int F, float reg, float* __restrict__ out_mag,
                                                              float* __restrict__ out_phase) {
  constexpr int TRI = C * (C + 1) / 2;
  __shared__ float s_R[MWF_MAX_N * C * C * 2];
  const int f = blockIdx.y, t = blockIdx.x * MWF_BLOCK + threadIdx.x;
  for (int i = threadIdx.x; i < N * C * C * 2; i += MWF_BLOCK) {
    const int n = i / (C * C * 2), j = i - n * (C * C * 2);
    s_R[i] = cov[((long long)n * Fin + f) * (C * C * 2) + j];
  }
  __syncthreads();
  if (t >= F) return;
  const long long plane = (long long)Fin * F, ft = (long long)f * F + t;

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
      const float* R = s_R + n * (C * C * 2);
#pragma unroll
      for (int r = 0; r < C; ++r)
#pragma unroll
        for (int c = 0; c <= r; ++c) {
          Sr[r * (r + 1) / 2 + c] += v[n] * R[2 * (r * C + c)];
          if (c < r) Si[r * (r + 1) / 2 + c] += v[n] * R[2 * (r * C + c) + 1];
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
      const float* R = s_R + n * (C * C * 2);
#pragma unroll
      for (int r = 0; r < C; ++r) {
        float wr = 0.f, wi = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) {
          const float rr = R[2 * (r * C + c)], ri = R[2 * (r * C + c) + 1];
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

template <int C>
static void mwf_apply_launch(const float* xmag, const float* xph, const float* ymag, const float* cov, int N, int Fin, int F,
                             float reg, float* out_mag, float* out_phase, hipStream_t stream) {
  hipLaunchKernelGGL(mwf_apply_kernel<C>, dim3(cdiv(F, MWF_BLOCK), Fin), dim3(MWF_BLOCK), 0, stream, xmag, xph, ymag, cov, N, Fin,
                     F, reg, out_mag, out_phase);
}

extern "C" int avsep_mwf_apply(const float* xmag, const float* xph, const float* ymag, const float* cov, int32_t N, int32_t C,
                               int32_t Fin, int32_t F, float reg, float* out_mag, float* out_phase, avsep_stream_t stream) {
  if (!xmag || !xph || !ymag || !cov || !out_mag || !out_phase) return AVSEP_ERR_ARG;
  if (!mwf_dims_ok(N, C, Fin, F) || !(reg >= 0.f)) return AVSEP_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  switch (C) {
    case 1: mwf_apply_launch<1>(xmag, xph, ymag, cov, N, Fin, F, reg, out_mag, out_phase, s); break;
    case 2: mwf_apply_launch<2>(xmag, xph, ymag, cov, N, Fin, F, reg, out_mag, out_phase, s); break;
    case 3: mwf_apply_launch<3>(xmag, xph, ymag, cov, N, Fin, F, reg, out_mag, out_phase, s); break;
    case 4: mwf_apply_launch<4>(xmag, xph, ymag, cov, N, Fin, F, reg, out_mag, out_phase, s); break;
    case 5: mwf_apply_launch<5>(xmag, xph, ymag, cov, N, Fin, F, reg, out_mag, out_phase, s); break;
    case 6: mwf_apply_launch<6>(xmag, xph, ymag, cov, N, Fin, F, reg, out_mag, out_phase, s); break;
    case 7: mwf_apply_launch<7>(xmag, xph, ymag, cov, N, Fin, F, reg, out_mag, out_phase, s); break;
    default: mwf_apply_launch<8>(xmag, xph, ymag, cov, N, Fin, F, reg, out_mag, out_phase, s); break;
  }
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

// grid (ceil(segments / 4), Fin, N), one wave per segment: its lanes stride 64 through the segment's H frames in ascending
// t, each with two slabs in registers, the (1 - u)-weighted sums (for centre s) and the u-weighted sums (for centre s + 1)
// of the lower triangle and of v.  The wave is reduced by the xor butterfly and writes its 2 * NACC floats to
// ws[segment][n][f][2][NACC]; nothing is shared between the waves of a workgroup.  The order of every sum depends on
// (F, H) alone.
template <int C>
__global__ __launch_bounds__(MWF_BLOCK) void mwf_cov_tv_partial_kernel(const float* __restrict__ ymag, const float* __restrict__ yph,
                                                                       long long phase_stride, int Fin, int F, int H, int segments,
                                                                       float* __restrict__ ws) {
#pragma clang fp contract(off)
  constexpr int NACC = C * (C + 1) + 1;
  constexpr int NOUT = (2 * NACC + 63) / 64;
  const int lane = threadIdx.x & 63;
  const int seg = blockIdx.x * MWF_WAVES + (threadIdx.x >> 6);
  if (seg >= segments) return;                                  // the whole wave; there is no barrier in this kernel
  const int f = blockIdx.y, n = blockIdx.z, N = gridDim.z;
  const long long plane = (long long)Fin * F;
  const float* __restrict__ m = ymag + (long long)n * C * plane + (long long)f * F;
  const float* __restrict__ p = yph + (long long)n * phase_stride + (long long)f * F;
  const int t0 = seg * H;                                       // seg * H < F and F <= INT_MAX - 4096: t0 + H does not wrap
  const int len = min(H, F - t0);
  const float fH = (float)H;
  float accA[NACC], accB[NACC];
#pragma unroll
  for (int i = 0; i < NACC; ++i) accA[i] = accB[i] = 0.f;
  for (int j = lane; j < len; j += 64) {
    const int t = t0 + j;
    const float u = (float)j / fH, w = 1.f - u;
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
    const float vv = sq * (1.f / C);
    accA[NACC - 1] += w * vv;
    accB[NACC - 1] += u * vv;
#pragma unroll
    for (int r = 0; r < C; ++r) {
#pragma unroll
      for (int c = 0; c <= r; ++c) {
        const int i = 2 * (r * (r + 1) / 2 + c);
        // Y_r conj(Y_c) with the roundings of mwf_cov_partial_kernel: two equal channels give equal real parts and an
        // imaginary part of exactly 0 before the weight, and so after it
        const float pr = fmaf(re[r], re[c], im[r] * im[c]);
        accA[i] += w * pr;
        accB[i] += u * pr;
        if (c < r) {
          const float pi = im[r] * re[c] - re[r] * im[c];
          accA[i + 1] += w * pi;
          accB[i + 1] += u * pi;
        }
      }
    }
  }
  // lane i of output q keeps sum number 64 q + i: coalesced stores, and no register array indexed at run time
  float o[NOUT];
#pragma unroll
  for (int q = 0; q < NOUT; ++q) o[q] = 0.f;
#pragma unroll
  for (int i = 0; i < 2 * NACC; ++i) {
    const float s = wave_sum(i < NACC ? accA[i < NACC ? i : 0] : accB[i < NACC ? 0 : i - NACC]);
    if ((i & 63) == lane) o[i >> 6] = s;
  }
  float* __restrict__ dst = ws + (((long long)seg * N + n) * Fin + f) * (2 * NACC);
#pragma unroll
  for (int q = 0; q < NOUT; ++q)
    if (q * 64 + lane < 2 * NACC) dst[q * 64 + lane] = o[q];
}

// grid (K, Fin, N), one wave: thread r*C + c forms entry (r, c) of centre k as A_k + B_{k-1}, in that order (segment k's
// (1 - u) slab, then segment k - 1's u slab; the first centre has no B, a centre past the last segment no A), and divides
// by max(sum w v, FLT_MIN): a source that is silent over the centre's support gives R = 0 there.
__global__ __launch_bounds__(64) void mwf_cov_tv_finish_kernel(const float* __restrict__ ws, int segments, int C, int Fin,
                                                               float* __restrict__ cov) {
  const int k = blockIdx.x, K = gridDim.x, f = blockIdx.y, n = blockIdx.z, N = gridDim.z;
  if ((int)threadIdx.x >= C * C) return;
  const int r = threadIdx.x / C, c = threadIdx.x - r * C;
  const int lo = max(r, c), hi = min(r, c), i = 2 * (lo * (lo + 1) / 2 + hi), nacc = C * (C + 1) + 1;
  float re = 0.f, im = 0.f, den = 0.f;
  if (k < segments) {
    const float* __restrict__ a = ws + (((long long)k * N + n) * Fin + f) * (2 * nacc);
    re = a[i];
    im = a[i + 1];
    den = a[nacc - 1];
  }
  if (k >= 1) {                                                 // K <= segments + 1: segment k - 1 exists
    const float* __restrict__ b = ws + (((long long)(k - 1) * N + n) * Fin + f) * (2 * nacc) + nacc;
    re += b[i];
    im += b[i + 1];
    den += b[nacc - 1];
  }
  den = fmaxf(den, FLT_MIN);
  float* __restrict__ o = cov + 2 * (((((long long)n * K + k) * Fin + f) * C + r) * C + c);
  o[0] = re / den;
  o[1] = r == c ? 0.f : (r > c ? im : -im) / den;
}

template <int C>
static void mwf_cov_tv_launch(const float* ymag, const float* yph, long long phase_stride, int N, int Fin, int F, int H, float* ws,
                              hipStream_t stream) {
  const int segments = (int)mwf_tv_segments(F, H);
  hipLaunchKernelGGL(mwf_cov_tv_partial_kernel<C>, dim3(cdiv(segments, MWF_WAVES), Fin, N), dim3(MWF_BLOCK), 0, stream, ymag, yph,
                     phase_stride, Fin, F, H, segments, ws);
}

extern "C" int avsep_mwf_cov_tv(const float* ymag, const float* yph, int32_t phase_per_source, int32_t N, int32_t C, int32_t Fin,
                                int32_t F, int32_t H, float* cov, float* ws, size_t ws_bytes, avsep_stream_t stream) {
  if (!ymag || !yph || !cov || !ws) return AVSEP_ERR_ARG;
  if (!mwf_dims_ok(N, C, Fin, F) || !mwf_span_ok(H) || ws_bytes < avsep_mwf_tv_workspace_bytes(N, C, Fin, F, H)) return AVSEP_ERR_ARG;
  const long long stride = phase_per_source ? (long long)C * Fin * F : 0;
  hipStream_t s = (hipStream_t)stream;
  switch (C) {
    case 1: mwf_cov_tv_launch<1>(ymag, yph, stride, N, Fin, F, H, ws, s); break;
    case 2: mwf_cov_tv_launch<2>(ymag, yph, stride, N, Fin, F, H, ws, s); break;
    case 3: mwf_cov_tv_launch<3>(ymag, yph, stride, N, Fin, F, H, ws, s); break;
    case 4: mwf_cov_tv_launch<4>(ymag, yph, stride, N, Fin, F, H, ws, s); break;
    case 5: mwf_cov_tv_launch<5>(ymag, yph, stride, N, Fin, F, H, ws, s); break;
    case 6: mwf_cov_tv_launch<6>(ymag, yph, stride, N, Fin, F, H, ws, s); break;
    case 7: mwf_cov_tv_launch<7>(ymag, yph, stride, N, Fin, F, H, ws, s); break;
    default: mwf_cov_tv_launch<8>(ymag, yph, stride, N, Fin, F, H, ws, s); break;
  }
  AVSEP_LAUNCH_CHECK();
  hipLaunchKernelGGL(mwf_cov_tv_finish_kernel, dim3((unsigned)mwf_tv_centres(F, H), Fin, N), dim3(64), 0, s, ws,
                     (int)mwf_tv_segments(F, H), C, Fin, cov);
  AVSEP_LAUNCH_CHECK();
  return AVSEP_OK;
}

// grid (ceil(F / 256), Fin), as mwf_apply_kernel.  The tile's (at most) five centres k0 ... k0 + 4 of all sources sit in
// LDS, centre indices clamped to K - 1 (a clamped centre is only ever read with weight u = 0).  A wave's segment, and with
// it the pair of centres it reads, is uniform: every LDS read stays a broadcast.  An entry of R_n[f,t] is formed as
// (1 - u) R[s] + u R[s + 1] where it is used, once for S and once for v_n R_n z; no blended copy is kept.
template <int C>
__global__ __launch_bounds__(MWF_BLOCK) void mwf_apply_tv_kernel(const float* __restrict__ xmag, const float* __restrict__ xph,
                                                                 const float* __restrict__ ymag, const float* __restrict__ cov,
                                                                 int N, int Fin, int F, int H, int K, float reg,
                                                                 float* __restrict__ out_mag, float* __restrict__ out_phase) {
  constexpr int TRI = C * (C + 1) / 2;
  constexpr int RC = C * C * 2;
  __shared__ float s_R[MWF_TV_TILE_CENTRES * MWF_MAX_N * RC];
  const int f = blockIdx.y, tile0 = blockIdx.x * MWF_BLOCK, t = tile0 + threadIdx.x;
  const int k0 = tile0 / H, per = N * RC;
  for (int i = threadIdx.x; i < MWF_TV_TILE_CENTRES * per; i += MWF_BLOCK) {
    const int j = i / per, rest = i - j * per, n = rest / RC, e = rest - n * RC;
    const int k = min(k0 + j, K - 1);
    s_R[i] = cov[(((long long)n * K + k) * Fin + f) * RC + e];
  }
  __syncthreads();
  if (t >= F) return;
  const long long plane = (long long)Fin * F, ft = (long long)f * F + t;
  // the wave's first frame is a multiple of 64 and H is one: all 64 frames lie in segment seg
  const int seg = __builtin_amdgcn_readfirstlane((tile0 + (int)(threadIdx.x & ~63u)) / H);
  const float u = (float)(t - seg * H) / (float)H, w = 1.f - u;
  const float* Ra = s_R + (seg - k0) * per;                    // seg - k0 in 0 ... 3
  const float* Rb = Ra + per;

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
          const int e = n * RC + 2 * (r * C + c);
          Sr[r * (r + 1) / 2 + c] += v[n] * (w * Ra[e] + u * Rb[e]);
          if (c < r) Si[r * (r + 1) / 2 + c] += v[n] * (w * Ra[e + 1] + u * Rb[e + 1]);
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
  // Y_n' = v_n R_n[f,t] z.  v_n == 0 is an exact zero whatever z is
#pragma unroll
  for (int n = 0; n < MWF_MAX_N; ++n) {
    if (n < N) {
#pragma unroll
      for (int r = 0; r < C; ++r) {
        float wr = 0.f, wi = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) {
          const int e = n * RC + 2 * (r * C + c);
          const float rr = w * Ra[e] + u * Rb[e], ri = w * Ra[e + 1] + u * Rb[e + 1];
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

template <int C>
static void mwf_apply_tv_launch(const float* xmag, const float* xph, const float* ymag, const float* cov, int N, int Fin, int F,
                                int H, float reg, float* out_mag, float* out_phase, hipStream_t stream) {
  hipLaunchKernelGGL(mwf_apply_tv_kernel<C>, dim3(cdiv(F, MWF_BLOCK), Fin), dim3(MWF_BLOCK), 0, stream, xmag, xph, ymag, cov, N,
                     Fin, F, H, (int)mwf_tv_centres(F, H), reg, out_mag, out_phase);
}

extern "C" int avsep_mwf_apply_tv(const float* xmag, const float* xph, const float* ymag, const float* cov, int32_t N, int32_t C,
                                  int32_t Fin, int32_t F, int32_t H, float reg, float* out_mag, float* out_phase,
                                  avsep_stream_t stream) {
  if (!xmag || !xph || !ymag || !cov || !out_mag || !out_phase) return AVSEP_ERR_ARG;
  if (!mwf_dims_ok(N, C, Fin, F) || !mwf_span_ok(H) || !(reg >= 0.f)) return AVSEP_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  switch (C) {
    case 1: mwf_apply_tv_launch<1>(xmag, xph, ymag, cov, N, Fin, F, H, reg, out_mag, out_phase, s); break;
    case 2: mwf_apply_tv_launch<2>(xmag, xph, ymag, cov, N, Fin, F, H, reg, out_mag, out_phase, s); break;
    case 3: mwf_apply_tv_launch<3>(xmag, xph, ymag, cov, N, Fin, F, H, reg, out_mag, out_phase, s); break;
    case 4: mwf_apply_tv_launch<4>(xmag, xph, ymag, cov, N, Fin, F, H, reg, out_mag, out_phase, s); break;
    case 5: mwf_apply_tv_launch<5>(xmag, xph, ymag, cov, N, Fin, F, H, reg, out_mag, out_phase, s); break;
    case 6: mwf_apply_tv_launch<6>(xmag, xph, ymag, cov, N, Fin, F, H, reg, out_mag, out_phase, s); break;
    case 7: mwf_apply_tv_launch<7>(xmag, xph, ymag, cov, N, Fin, F, H, reg, out_mag, out_phase, s); break;
    default: mwf_apply_tv_launch<8>(xmag, xph, ymag, cov, N, Fin, F, H, reg, out_mag, out_phase, s); break;
  }
  AVSEP_LAUNCH_CHECK();
  return AVSEP_OK;
}
