// Rational polyphase FIR resampling (include/avsep.h): WAV files at any sample rate in, sources at the file's rate out.
// One kernel, bandwidth-bound on paper (<= 90 multiply-adds per 4-byte output).  A workgroup owns RS_R * S consecutive
// outputs of one row, S a multiple of `up`, starting at a multiple of `up`: it stages the input samples they touch in LDS
// (converted and down-mixed on the way when the input is interleaved PCM).  A thread then computes the RS_R outputs
// t0, t0 + S, t0 + 2S, ... of the tile: they share their phase, so each coefficient is loaded once (lanes on consecutive
// columns of the table: coalesced) and used RS_R times.
// No atomics: every output is one sequential f32 fused-multiply-add chain whose order depends on (up, down, j) only.
#include "common.h"

constexpr int RS_BLOCK = 256;
constexpr int RS_R = 4;            // outputs per thread and pass (independent accumulation chains)
constexpr int RS_SPAN = 12288;     // floats of staged input a tile may touch (48 KiB + 1/32 of padding in LDS)
constexpr int RS_MAX_S = 2048;
constexpr int RS_MAX_RATIO = 1280;
constexpr int RS_MAX_CH = 256;     // |sum of the channels| <= 256 * 32768 = 2^23: exact in f32, as is the divisor

// Sample n of a row; zero outside it.  in_ch >= 1: interleaved int16 [L, in_ch], the exact integer sum of the channels
// over in_ch * 32768 with a correctly rounded division (separate.read_wav's value for one and two channels).
__device__ __forceinline__ float rs_sample(const void* __restrict__ x, long long n, long long L, int in_ch) {
  if ((unsigned long long)n >= (unsigned long long)L) return 0.f;
  if (in_ch == 0) return ((const float*)x)[n];
  const int16_t* s = (const int16_t*)x + n * in_ch;
  int sum = 0;
  for (int c = 0; c < in_ch; ++c) sum += s[c];
  return __fdiv_rn((float)sum, (float)(in_ch * 32768));
}

// One padding slot per 32 samples: lanes that read with a stride of 2, 4 or 8 samples (decimation by that factor) then
// fall on 32 different banks instead of 16, 8 or 4.
__device__ __forceinline__ int rs_slot(int s) { return s + (s >> 5); }

// grid (ceil(Lout / (RS_R * S)), B).  Output j = j0 + dj sits at filter position pos = j * down + half = pos0 + dj * down:
// phase p = pos mod up, newest input n = pos div up, taps i = 0 .. T-1 pair x[n - i] with h[p + i * up] = ho[i][dj mod up]
// (j0 is a multiple of up, so the phase of dj is the phase of column dj mod up of the table).
// pos0 is split once per workgroup in 64 bits (j * down passes 2^31 on a ten-minute file); dj * down < 2^24 stays 32-bit.
// STAGED: the samples [n_lo, n_lo + span) of the tile are in LDS.  Otherwise (a ratio whose tile does not fit) every tap
// reads global memory: the same values in the same order, so the mode never shows in the result.
template <bool STAGED>
__global__ __launch_bounds__(RS_BLOCK) void resample_poly_kernel(const void* __restrict__ x, const float* __restrict__ ho, int up,
                                                                 int down, int half, int M, int T, int S, int L, int Lout,
                                                                 int in_ch, int out_s16, void* __restrict__ y) {
  __shared__ float s_x[STAGED ? RS_SPAN + RS_SPAN / 32 + 1 : 1];
  const int row = blockIdx.y;
  const long long j0 = (long long)blockIdx.x * (RS_R * S);
  const long long pos0 = j0 * down + half;
  const long long q0 = pos0 / up;
  const int r0 = (int)(pos0 - q0 * up);
  const int nout = (int)min((long long)(RS_R * S), (long long)Lout - j0);
  const void* xr = in_ch ? x : (const void*)((const float*)x + (long long)row * L);
  const long long n_lo = q0 - (T - 1);                       // oldest sample of the tile's first output
  if (STAGED) {
    const int span = (r0 + (nout - 1) * down) / up + T;      // <= RS_SPAN: checked by the host for a full tile
    for (int s = threadIdx.x; s < span; s += RS_BLOCK) s_x[rs_slot(s)] = rs_sample(xr, n_lo + s, L, in_ch);
    __syncthreads();
  }
  const int step = S / up * down;                            // input samples between a thread's outputs: S * down / up
  for (int t0 = threadIdx.x; t0 < S; t0 += RS_BLOCK) {
    if (t0 >= nout) break;                                   // none of this thread's outputs lies inside the row
    const int v = r0 + t0 * down, dq = v / up, p = v - dq * up;
    const float* __restrict__ h = ho + t0 % up;
    // a thread's outputs past the row's end compute on whatever the tile holds and are not stored; their reads stay
    // inside s_x (the host sized it for a full tile) or inside the row (rs_sample checks)
    int top[RS_R];                                           // newest sample of output r, relative to n_lo
    float acc[RS_R];
#pragma unroll
    for (int r = 0; r < RS_R; ++r) {
      top[r] = dq + r * step + T - 1;
      acc[r] = 0.f;
    }
#define RS_X(r, i) (STAGED ? s_x[rs_slot(top[r] - (i))] : rs_sample(xr, n_lo + top[r] - (i), L, in_ch))
#pragma unroll 4
    for (int i = 0; i < T - 1; ++i) {
      const float c = h[i * up];
#pragma unroll
      for (int r = 0; r < RS_R; ++r) acc[r] = fmaf(RS_X(r, i), c, acc[r]);
    }
    // only the last tap can fall off the filter's end (p + (T-1) * up >= M): it then takes no sample at all
    const float c = h[(T - 1) * up];
    const bool last = p + (T - 1) * up < M;
#pragma unroll
    for (int r = 0; r < RS_R; ++r) acc[r] = fmaf(last ? RS_X(r, T - 1) : 0.f, c, acc[r]);
#undef RS_X
#pragma unroll
    for (int r = 0; r < RS_R; ++r) {
      const int dj = t0 + r * S;
      if (dj >= nout) break;
      const long long o = (long long)row * Lout + j0 + dj;
      if (out_s16)
        ((int16_t*)y)[o] = (int16_t)(int)fminf(fmaxf(rintf(acc[r] * 32768.f), -32768.f), 32767.f);
      else
        ((float*)y)[o] = acc[r];
    }
  }
}

// Outputs between a thread's RS_R outputs: a multiple of `up`, at least one pass of the workgroup, chosen for the fewest idle
// lanes in the last pass among the sizes whose tile of RS_R * S outputs fits the LDS span (0: none does).
static int rs_stride(int up, int down, int T) {
  int best = 0;
  double best_fill = 0.0;
  for (int S = up; S <= RS_MAX_S; S += up) {
    if (S < RS_BLOCK) continue;
    const long long span = ((long long)(up - 1) + ((long long)RS_R * S - 1) * down) / up + T;
    if (span > RS_SPAN) break;
    const double fill = (double)S / roundup(S, RS_BLOCK);
    if (fill > best_fill + 1e-9) best = S, best_fill = fill;
  }
  return best;
}

extern "C" int avsep_resample_poly(const void* x, const float* ho, int32_t B, int32_t L, int32_t up, int32_t down,
                                   int32_t in_ch, int32_t out_s16, void* y, avsep_stream_t stream) {
  if (!x || !ho || !y) return AVSEP_ERR_ARG;
  if (up < 1 || up > RS_MAX_RATIO || down < 1 || down > RS_MAX_RATIO || L < 1 || B < 1 || B > 65535) return AVSEP_ERR_ARG;
  if (in_ch < 0 || in_ch > RS_MAX_CH || (in_ch >= 1 && B != 1) || (out_s16 != 0 && out_s16 != 1)) return AVSEP_ERR_ARG;
  const long long lout = ((long long)L * up + down - 1) / down;
  if (lout > 0x7fffffffLL) return AVSEP_ERR_ARG;
  const int m = up > down ? up : down, half = 10 * m, M = 2 * half + 1;
  const int T = (M + up - 1) / up;
  int S = rs_stride(up, down, T);
  const bool staged = S > 0;
  if (!staged) S = roundup(RS_BLOCK, up);
  const dim3 grid(cdiv(lout, (long long)RS_R * S), B);
  if (staged)
    hipLaunchKernelGGL(resample_poly_kernel<true>, grid, dim3(RS_BLOCK), 0, (hipStream_t)stream, x, ho, up, down, half, M, T, S,
                       L, (int)lout, in_ch, out_s16, y);
  else
    hipLaunchKernelGGL(resample_poly_kernel<false>, grid, dim3(RS_BLOCK), 0, (hipStream_t)stream, x, ho, up, down, half, M, T, S,
                       L, (int)lout, in_ch, out_s16, y);
  AVSEP_LAUNCH_CHECK();
  return AVSEP_OK;
}
