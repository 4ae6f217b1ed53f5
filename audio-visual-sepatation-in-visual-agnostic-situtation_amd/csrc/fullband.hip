// Full-band stems (include/avsep.h): the model hears a file at its own low rate, so its masks end at that rate's Nyquist;
// these two kernels hand every stem its share of what the file holds above it.
// band_gains_kernel: one gain per source, row and STFT frame, the source's share of the mixture's RMS amplitude over the
// bins [lo_bin, bins).  A thread owns one (g, t): frames are the contiguous axis, so a wavefront reads 64 consecutive floats
// of every bin row it walks; the mixture's sum is formed once and the N sources' sums beside it.
// band_extend_kernel: the join at the file's rate.  A workgroup owns a resampler tile (resample_parts.h) of one row g: it
// stages the tile's samples of low[g] and of the N stem rows of that g side by side in LDS, makes the low chain once per
// output and then, per source, the stem chain and out = stem + gain * (file - low).  Every chain is rs_chains, so a stem's
// term is bit for bit what avsep_resample_poly gives that row.
// No atomics in either kernel; every sum has one fixed order.
#include "resample_parts.h"

constexpr int BG_BLOCK = 64;       // one wavefront of frames per workgroup: a ten-minute recording still gives every CU a few
constexpr int FB_MAX_N = 8;        // sources
constexpr int FB_MAX_G = 8;        // rows (channels) per source
constexpr int FB_MAX_HOP = 4096;   // up * hop < 2^24: the frame position of an output is exact in f32

// grid (ceil(F / BG_BLOCK), G).  stem [N, G, bins, F], mix [G, bins, F] -> gains [N, G, F].
__global__ __launch_bounds__(BG_BLOCK) void band_gains_kernel(const float* __restrict__ stem, const float* __restrict__ mix, int N, int G,
                                                              int bins, int F, int lo, float* __restrict__ gains) {
  const int t = blockIdx.x * BG_BLOCK + threadIdx.x, g = blockIdx.y;
  if (t >= F) return;
  const long long row = F, plane = (long long)bins * F;      // floats between bins, between (n, g) planes
  const float* __restrict__ m = mix + g * plane + t;
  const float* __restrict__ s = stem + g * plane + t;
  float den = 0.f, num[FB_MAX_N];
#pragma unroll
  for (int n = 0; n < FB_MAX_N; ++n) num[n] = 0.f;
#pragma unroll 4
  for (int f = lo; f < bins; ++f) {
    const float a = m[f * row];
    den = fmaf(a, a, den);
#pragma unroll
    for (int n = 0; n < FB_MAX_N; ++n) {
      if (n < N) {
        const float b = s[n * G * plane + f * row];
        num[n] = fmaf(b, b, num[n]);
      }
    }
  }
  const float d = den + 1e-20f * (float)(bins - lo);
#pragma unroll
  for (int n = 0; n < FB_MAX_N; ++n)
    if (n < N) gains[((long long)n * G + g) * F + t] = fminf(1.f, __fsqrt_rn(__fdiv_rn(num[n], d)));
}

// grid (ceil(Lout / (RS_R * S)), G).  The staged rows sit `pitch` slots apart: row 0 is low[g], row 1 + n is stems[n, g].
template <bool STAGED>
__global__ __launch_bounds__(RS_BLOCK) void band_extend_kernel(const float* __restrict__ stems, const float* __restrict__ low,
                                                               const float* __restrict__ file, const float* __restrict__ gains,
                                                               const float* __restrict__ ho, int N, int G, int Lm, int Ll, int Lf,
                                                               int F, int hop, int up, int down, int half, int M, int T, int S,
                                                               int Lout, int pitch, float* __restrict__ out) {
  __shared__ float s_x[STAGED ? RS_LDS : 1];
  const int g = blockIdx.y;
  const RsTile tl = rs_tile(up, down, half, T, S, Lout);
  const float* __restrict__ lrow = low + (long long)g * Ll;
  if (STAGED) {
    for (int s = threadIdx.x; s < tl.span; s += RS_BLOCK)
      s_x[rs_slot(s)] = rs_sample<true>(lrow, tl.n_lo + s, Ll, 0, -1, AVSEP_SAMPLE_F32);
    for (int n = 0; n < N; ++n) {
      const float* __restrict__ srow = stems + ((long long)n * G + g) * Lm;
      for (int s = threadIdx.x; s < tl.span; s += RS_BLOCK)
        s_x[(1 + n) * pitch + rs_slot(s)] = rs_sample<true>(srow, tl.n_lo + s, Lm, 0, -1, AVSEP_SAMPLE_F32);
    }
    __syncthreads();
  }
  // the frame position of the tile's first output, split once in 64 bits: output j0 + dj then sits at
  // (q0 * den + rem0 + dj * down) / den frames, and rem0 + dj * down < 2^24 stays 32-bit
  const int den = up * hop;
  const long long num0 = tl.j0 * down, q0 = num0 / den;
  const unsigned rem0 = (unsigned)(num0 - q0 * den);
  const float fden = (float)den;
  for (int t0 = threadIdx.x; t0 < S; t0 += RS_BLOCK) {
    if (t0 >= tl.nout) break;                                // none of this thread's outputs lies inside the row
    float l[RS_R], h[RS_R], fr[RS_R];
    int f0[RS_R], f1[RS_R];
    rs_chains<STAGED, true>(s_x, lrow, tl.n_lo, Ll, 0, -1, AVSEP_SAMPLE_F32, ho, up, down, M, T, S, tl.r0, t0, l);
#pragma unroll
    for (int r = 0; r < RS_R; ++r) {
      const int dj = t0 + r * S;
      const long long j = tl.j0 + dj;
      h[r] = (dj < tl.nout && j < Lf) ? file[(long long)g * Lf + j] - l[r] : 0.f;
      const unsigned v = rem0 + (unsigned)dj * (unsigned)down;
      const long long q = q0 + v / (unsigned)den;
      f0[r] = (int)min(q, (long long)(F - 1));
      f1[r] = min(f0[r] + 1, F - 1);
      fr[r] = __fdiv_rn((float)((q - f0[r]) * den + (long long)(v % (unsigned)den)), fden);
    }
    for (int n = 0; n < N; ++n) {
      const long long ng = (long long)n * G + g;
      float s[RS_R];
      rs_chains<STAGED, true>(s_x + (1 + n) * pitch, stems + ng * Lm, tl.n_lo, Lm, 0, -1, AVSEP_SAMPLE_F32, ho, up, down, M, T, S,
                              tl.r0, t0, s);
      const float* __restrict__ gr = gains + ng * F;
#pragma unroll
      for (int r = 0; r < RS_R; ++r) {
        const int dj = t0 + r * S;
        if (dj >= tl.nout) break;
        const float g0 = gr[f0[r]];
        const float gi = fmaf(fr[r], gr[f1[r]] - g0, g0);
        out[ng * Lout + tl.j0 + dj] = fmaf(gi, h[r], s[r]);
      }
    }
  }
}

extern "C" int avsep_band_gains(const float* stem_mag, const float* mix_mag, int32_t N, int32_t G, int32_t bins, int32_t F,
                                int32_t lo_bin, float* gains, avsep_stream_t stream) {
  if (!stem_mag || !mix_mag || !gains) return AVSEP_ERR_ARG;
  if (N < 1 || N > FB_MAX_N || G < 1 || G > FB_MAX_G || F < 1 || lo_bin < 1 || lo_bin >= bins) return AVSEP_ERR_ARG;
  hipLaunchKernelGGL(band_gains_kernel, dim3(cdiv(F, BG_BLOCK), G), dim3(BG_BLOCK), 0, (hipStream_t)stream, stem_mag, mix_mag, N, G,
                     bins, F, lo_bin, gains);
  AVSEP_LAUNCH_CHECK();
  return AVSEP_OK;
}

extern "C" int avsep_band_extend(const float* stems, const float* low, const float* file, const float* gains, const float* ho,
                                 int32_t N, int32_t G, int32_t Lm, int32_t Ll, int32_t Lf, int32_t F, int32_t hop, int32_t up,
                                 int32_t down, float* out, avsep_stream_t stream) {
  if (!stems || !low || !file || !gains || !ho || !out) return AVSEP_ERR_ARG;
  if (N < 1 || N > FB_MAX_N || G < 1 || G > FB_MAX_G || F < 1 || hop < 1 || hop > FB_MAX_HOP || Lf < 1 || Ll < Lm) return AVSEP_ERR_ARG;
  long long lout;
  if (!rs_ratio_ok(up, down, Lm, &lout) || up <= down) return AVSEP_ERR_ARG;
  const RsPlan p = rs_plan(up, down, lout, N + 1, RS_LDS);
  return rs_launch(p, band_extend_kernel<true>, band_extend_kernel<false>, dim3(p.tiles, G), stream, stems, low, file, gains, ho, N,
                   G, Lm, Ll, Lf, F, hop, up, down, p.half, p.M, p.T, p.S, (int)lout, p.pitch, out);
}
