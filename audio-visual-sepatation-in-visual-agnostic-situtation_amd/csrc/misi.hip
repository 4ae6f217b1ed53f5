// Multiple Input Spectrogram Inversion (Gunawan & Sen 2010) for the stems of one mixture: every pass inverts the stems,
// hands the mixture error back in equal shares, transforms again and keeps the new phase under the target magnitude
// (include/avsep.h has the arithmetic).  The two DFT GEMMs are stft.hip's; what is new are the two kernels at their seams:
//   misi_ola_kernel      inverse GEMM output -> overlap-add, normalise, e = x - sum_n s_n, s_n + e/N   (one read of td)
//   misi_rephase_kernel  forward GEMM output + target magnitude -> inverse GEMM operand A * Z / |Z|     (no angle formed)
// A group (the N rows that sum to one mixture) is processed on its own, one after the other on the stream, with GEMMs of N
// rows: a call with G groups gives, bit for bit, what G calls with one group give, and the workspace does not grow with G.
#include <float.h>
#include "common.h"
#include "stft_parts.h"

#define MISI_MAX_SOURCES 8
#define MISI_MAX_GROUPS 8
#define MISI_TJ 32      // hops per block
#define MISI_TC 32      // samples within a hop per block
#define MISI_LD (MISI_TC + 1)

static inline int bins_of(int n_fft) { return n_fft / 2 + 1; }
static inline size_t up64(size_t n) { return (n + 63) / 64 * 64; }

// window-sum-square at every output sample, with istft_ola_kernel's arithmetic (once per call)
__global__ __launch_bounds__(256) void misi_wss_kernel(int n_fft, int hop, int frames, int out_len, float* __restrict__ wss) {
  const int pad = n_fft / 2;
  for (int t = blockIdx.x * 256 + threadIdx.x; t < out_len; t += gridDim.x * 256) {
    const int g = t + pad;
    const int f_hi = min(frames - 1, g / hop), f_lo = max(0, (g - n_fft + hop) / hop);
    float s = 0.f;
    for (int f = f_lo; f <= f_hi; ++f) {
      const int n = g - f * hop;
      if (n < 0 || n >= n_fft) continue;
      const float w = 0.5f - 0.5f * cosf(2.f * (float)M_PI * (float)n / (float)n_fft);
      s += w * w;
    }
    wss[t] = s;
  }
}

// first inverse operand: op[n][bin | bins + bin][f] = mag * (cos | sin)(phase); rows of group g, phase shared or per source
__global__ __launch_bounds__(256) void misi_start_kernel(const float* __restrict__ mag, long long mag_stride,
                                                         const float* __restrict__ phase, long long phase_stride, long long n,
                                                         float* __restrict__ op) {
  const int r = blockIdx.y;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const float m = mag[(long long)r * mag_stride + i], p = phase[(long long)r * phase_stride + i];
    float s, c;
    sincosf(p, &s, &c);
    op[(long long)r * 2 * n + i] = m * c;
    op[(long long)r * 2 * n + n + i] = m * s;
  }
}

// Overlap-add and consistency.  td is [N][n_fft][frames] (synthesis window in the basis); sample g = hop * j + c of the
// untrimmed signal is sum_q td[hop * q + c][j - q].  Block = (32 hops j, 32 offsets c, all N rows): for a fixed (n, q, c) the
// 32 values along j are contiguous in td, so the reads are 128-byte runs; an LDS tile turns them so that the writes run along
// c, contiguous in the waveform.  PROJECT: out[n] = s_n + (mix - sum_n s_n) / N; otherwise out[n] = s_n.
template <bool PROJECT>
__global__ __launch_bounds__(256) void misi_ola_kernel(const float* __restrict__ td, const float* __restrict__ wss,
                                                       const float* __restrict__ mix, int N, int n_fft, int hop, int frames,
                                                       int out_len, int nq, int j_first, float* __restrict__ out,
                                                       long long out_stride) {
  extern __shared__ float tile[];                         // [N][MISI_TJ][MISI_LD]
  const int j0 = j_first + blockIdx.x * MISI_TJ, c0 = blockIdx.y * MISI_TC, pad = n_fft / 2;
  const long long plane = (long long)n_fft * frames;
  for (int i = threadIdx.x; i < N * MISI_TJ * MISI_TC; i += 256) {
    const int jj = i % MISI_TJ, c = (i / MISI_TJ) % MISI_TC, n = i / (MISI_TJ * MISI_TC);
    const int cc = c0 + c, j = j0 + jj;
    float acc = 0.f;
    if (cc < hop) {
      const float* p = td + (long long)n * plane;
      for (int q = nq - 1; q >= 0; --q) {                 // frames in ascending order, as istft_ola_kernel adds them
        const int k = q * hop + cc, f = j - q;
        if (k < n_fft && f >= 0 && f < frames) acc += p[(long long)k * frames + f];
      }
    }
    tile[(n * MISI_TJ + jj) * MISI_LD + c] = acc;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < MISI_TJ * MISI_TC; i += 256) {
    const int c = i % MISI_TC, jj = i / MISI_TC, cc = c0 + c;
    const long long t = (long long)(j0 + jj) * hop + cc - pad;
    if (cc >= hop || t < 0 || t >= out_len) continue;
    const float w = wss[t];
    float s[MISI_MAX_SOURCES], sum = 0.f;
#pragma unroll
    for (int n = 0; n < MISI_MAX_SOURCES; ++n) {
      s[n] = 0.f;
      if (n < N) {
        const float a = tile[(n * MISI_TJ + jj) * MISI_LD + c];
        s[n] = w > FLT_MIN ? a / w : a;
        sum += s[n];                                      // n ascending
      }
    }
    const float share = PROJECT ? (mix[t] - sum) / (float)N : 0.f;
#pragma unroll
    for (int n = 0; n < MISI_MAX_SOURCES; ++n)
      if (n < N) out[(long long)n * out_stride + t] = PROJECT ? s[n] + share : s[n];
  }
}

// Z = a + ib from the forward GEMM (co_major: [2*bins][N][frames], else [N][2*bins][frames]) and the target magnitude A ->
// the inverse GEMM's operand [N][2*bins][frames] = A * Z / |Z|, and A * (1, 0) where Z = 0 (atan2f(0, 0) = 0).
// Block = (one bin, 256 frames) of row blockIdx.y.  PHASE: also the angle of Z (the last pass only).
template <bool PHASE>
__global__ __launch_bounds__(256) void misi_rephase_kernel(const float* __restrict__ spec, const float* __restrict__ mag,
                                                           long long mag_stride, int bins, int frames, int chunks, int N,
                                                           int co_major, float* __restrict__ op, float* __restrict__ phase,
                                                           long long phase_stride) {
  const int r = blockIdx.y, m = blockIdx.x / chunks, f = (blockIdx.x % chunks) * 256 + threadIdx.x;
  if (f >= frames) return;
  const long long n = (long long)bins * frames, i = (long long)m * frames + f;
  float a, b;
  if (co_major) {
    a = spec[((long long)m * N + r) * frames + f];
    b = spec[((long long)(bins + m) * N + r) * frames + f];
  } else {
    a = spec[(long long)r * 2 * n + i];
    b = spec[(long long)r * 2 * n + n + i];
  }
  const float A = mag[(long long)r * mag_stride + i];
  const float m2 = a * a + b * b;
  const float inv = m2 > 0.f ? rsqrtf(m2) : 0.f;
  op[(long long)r * 2 * n + i] = A * (m2 > 0.f ? a * inv : 1.f);
  op[(long long)r * 2 * n + n + i] = A * (b * inv);
  if (PHASE) phase[(long long)r * phase_stride + i] = atan2f(b, a);
}

static bool misi_shape_ok(int N, int G, int n_fft, int hop, int frames) {
  if (N < 1 || N > MISI_MAX_SOURCES || G < 1 || G > MISI_MAX_GROUPS || n_fft < 2 || (n_fft & 1) || hop <= 0 || frames < 2)
    return false;
  const long long out_len = (long long)hop * (frames - 1);
  return out_len > n_fft / 2 && out_len + n_fft <= INT32_MAX && (long long)bins_of(n_fft) * frames <= INT32_MAX &&
         (long long)bins_of(n_fft) * cdiv(frames, 256) <= INT32_MAX && cdiv(hop, MISI_TC) <= 65535;
}

struct MisiWs { size_t wss, op, td, shat, stage, wp, spec, total; };   // offsets in floats
static MisiWs misi_layout(int N, int n_fft, int hop, int frames) {
  const size_t out_len = (size_t)hop * (frames - 1), b2 = 2 * (size_t)bins_of(n_fft);
  const bool fast = stft_fast_path(N, (int)out_len, n_fft, hop);
  MisiWs w{};
  size_t o = 0;
  w.wss = o;   o += up64(out_len);
  w.op = o;    o += up64((size_t)N * b2 * frames);
  w.td = o;    o += up64((size_t)N * n_fft * frames);
  w.shat = o;  o += up64((size_t)N * out_len);
  w.stage = o; o += up64(fast ? (size_t)hop * N * (frames + 3) : (size_t)N * (out_len + n_fft));
  w.wp = o;    o += fast ? up64((size_t)hop * 4 * roundup((int)b2, 128)) : 0;
  w.spec = o;  o += up64((size_t)N * b2 * frames);
  w.total = o;
  return w;
}

extern "C" size_t avsep_misi_workspace_bytes(int32_t N, int32_t G, int32_t n_fft, int32_t hop, int32_t frames) {
  if (!misi_shape_ok(N, G, n_fft, hop, frames)) return 0;
  return misi_layout(N, n_fft, hop, frames).total * sizeof(float);
}

extern "C" int avsep_misi(const float* mix, const float* mag, const float* phase, int32_t phase_per_source, int32_t N, int32_t G,
                          int32_t n_fft, int32_t hop, int32_t frames, int32_t reflect, int32_t iterations,
                          const float* fwd_basis, const float* inv_basis, float* wav_out, float* phase_out, void* ws,
                          size_t ws_bytes, avsep_stream_t stream) {
  if (!mix || !mag || !phase || !fwd_basis || !inv_basis || !wav_out || iterations < 1 || !misi_shape_ok(N, G, n_fft, hop, frames))
    return AVSEP_ERR_ARG;
  const MisiWs w = misi_layout(N, n_fft, hop, frames);
  if (!ws || ws_bytes < w.total * sizeof(float)) return AVSEP_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int bins = bins_of(n_fft), out_len = hop * (frames - 1), pad = n_fft / 2;
  const long long nbf = (long long)bins * frames;
  const bool fast = stft_fast_path(N, out_len, n_fft, hop);
  float* base = (float*)ws;
  float *wss = base + w.wss, *op = base + w.op, *td = base + w.td, *shat = base + w.shat, *stage = base + w.stage,
        *wp = base + w.wp, *spec = base + w.spec;

  hipLaunchKernelGGL(misi_wss_kernel, dim3(min(cdiv(out_len, 256), 1024)), dim3(256), 0, st, n_fft, hop, frames, out_len, wss);
  AVSEP_LAUNCH_CHECK();
  const float* basis = fwd_basis;
  if (fast) {                                             // once per call, not once per pass
    int rc = stft_repack_basis(fwd_basis, n_fft, hop, wp, st);
    if (rc) return rc;
    basis = wp;
  }
  const int nq = cdiv(n_fft, hop), j_first = pad / hop, j_last = (pad + out_len - 1) / hop;
  const dim3 ola_grid(cdiv(j_last - j_first + 1, MISI_TJ), cdiv(hop, MISI_TC));
  const size_t ola_lds = (size_t)N * MISI_TJ * MISI_LD * sizeof(float);
  const int chunks = cdiv(frames, 256);
  const dim3 bin_grid(bins * chunks, N);
  const dim3 flat_grid((int)min((nbf + 255) / 256, (long long)1024), N);

  for (int g = 0; g < G; ++g) {
    // row n of the group is row n * G + g of mag, wav_out and phase_out
    const float* mag_g = mag + (long long)g * nbf;
    const float* mix_g = mix + (long long)g * out_len;
    hipLaunchKernelGGL(misi_start_kernel, flat_grid, dim3(256), 0, st, mag_g, (long long)G * nbf, phase + (long long)g * nbf,
                       phase_per_source ? (long long)G * nbf : 0LL, nbf, op);
    AVSEP_LAUNCH_CHECK();
    int rc = istft_gemm(op, N, n_fft, frames, inv_basis, td, st);
    if (rc) return rc;
    for (int k = 1; k <= iterations; ++k) {
      hipLaunchKernelGGL(misi_ola_kernel<true>, ola_grid, dim3(256), ola_lds, st, td, wss, mix_g, N, n_fft, hop, frames, out_len,
                         nq, j_first, shat, (long long)out_len);
      AVSEP_LAUNCH_CHECK();
      rc = stft_pad_gemm(shat, N, out_len, n_fft, hop, reflect, basis, stage, spec, st);
      if (rc) return rc;
      if (k == iterations && phase_out)
        hipLaunchKernelGGL(misi_rephase_kernel<true>, bin_grid, dim3(256), 0, st, spec, mag_g, (long long)G * nbf, bins, frames,
                           chunks, N, fast ? 1 : 0, op, phase_out + (long long)g * nbf, (long long)G * nbf);
      else
        hipLaunchKernelGGL(misi_rephase_kernel<false>, bin_grid, dim3(256), 0, st, spec, mag_g, (long long)G * nbf, bins, frames,
                           chunks, N, fast ? 1 : 0, op, (float*)nullptr, 0LL);
      AVSEP_LAUNCH_CHECK();
      rc = istft_gemm(op, N, n_fft, frames, inv_basis, td, st);
      if (rc) return rc;
    }
    hipLaunchKernelGGL(misi_ola_kernel<false>, ola_grid, dim3(256), ola_lds, st, td, wss, mix_g, N, n_fft, hop, frames, out_len,
                       nq, j_first, wav_out + (long long)g * out_len, (long long)G * out_len);
    AVSEP_LAUNCH_CHECK();
  }
  return AVSEP_OK;
}
