// What the resampling kernels share (resample.hip) and lend to the full-band join (fullband.hip): the sample formats, the
// staging slots, a workgroup's tile, the accumulation chains (rs_chains: the only arithmetic of the resampler) and the plan
// the entry points derive from (up, down).  Moving a chain elsewhere would move its bits: every kernel that states
// "the value avsep_resample_poly gives" calls rs_chains.
#pragma once
#include "common.h"

constexpr int RS_BLOCK = 256;
constexpr int RS_R = 4;            // outputs per thread and pass (independent accumulation chains)
constexpr int RS_SPAN = 12288;     // floats of staged input a tile may touch (48 KiB + 1/32 of padding in LDS)
constexpr int RS_MAX_S = 2048;
constexpr int RS_MAX_RATIO = 1280;
constexpr int RS_MAX_CH = 256;     // |sum of the channels| <= 256 * 32768 = 2^23: exact in f32, as is the divisor
constexpr int RS_LDS = RS_SPAN + RS_SPAN / 32 + 1;   // slots of the staging array
constexpr int RS_KEEP_CH = 8;      // channels split and join keep apart (7.1)
constexpr int RJ_SPAN = 8704;      // join: staged floats of all C rows together (34 KiB + padding, beside a 16 KiB output tile;
                                   // eight rows of a 1/1 tile still fit)
constexpr int RJ_LDS = RJ_SPAN + RJ_SPAN / 32 + 1;
constexpr int RJ_SPAN_F32 = 7936;  // join to f32 frames: the output tile is 32 KiB, the staged rows get what is left of 64 KiB
constexpr int RJ_LDS_F32 = RJ_SPAN_F32 + RJ_SPAN_F32 / 32 + 1;

__device__ __forceinline__ int rs_fmt_bytes(int fmt) { return fmt == AVSEP_SAMPLE_S16 ? 2 : fmt == AVSEP_SAMPLE_S24 ? 3 : 4; }
static inline bool rs_fmt_in_ok(int fmt) { return fmt >= AVSEP_SAMPLE_S16 && fmt <= AVSEP_SAMPLE_F32; }
static inline bool rs_fmt_out_ok(int fmt) { return fmt == AVSEP_SAMPLE_S16 || fmt == AVSEP_SAMPLE_S24 || fmt == AVSEP_SAMPLE_F32; }

// The `bytes` (2 ... 4) bytes at p, little-endian, in the low end of the result (the rest is whatever follows).  p has any
// alignment: the loads are the one or two ALIGNED dwords that hold the sample, funnel-shifted, so lanes on consecutive
// samples read consecutive (shared) dwords and nothing is loaded byte by byte.  No dword is touched that holds no byte of
// the sample, so nothing outside the 4-byte granules of the caller's buffer is read.
__device__ __forceinline__ uint32_t rs_bytes(const uint8_t* __restrict__ p, int bytes) {
  const int sh = (int)((size_t)p & 3);
  const uint32_t* __restrict__ q = (const uint32_t*)(p - sh);
  const uint32_t lo = q[0];
  const uint32_t hi = sh + bytes > 4 ? q[1] : 0u;
  return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * sh));
}

// A PCM sample's integer from rs_bytes' result.
__device__ __forceinline__ int rs_pcm(uint32_t v, int fmt) {
  return fmt == AVSEP_SAMPLE_S16 ? (int)(int16_t)v : fmt == AVSEP_SAMPLE_S24 ? (int)(v << 8) >> 8 : (int)v;
}

// Frame n of interleaved frames [L, C] of format fmt at any byte address (include/avsep.h).  ch >= 0: that channel, an exact
// scaling of the integer (s32: of the integer rounded to f32) or the float's own bits.  ch < 0: the down-mix, rounded once:
// the exact 64-bit sum over C * 2^(bits-1), both exact in f64, divided there and rounded to f32 (the double rounding of a
// quotient is innocuous at 53 >= 2 * 24 + 2 bits); floats are added in f64 in channel order.  One channel is its own mean.
__device__ __forceinline__ float rs_frame(const void* __restrict__ x, long long n, int C, int ch, int fmt) {
  const int bytes = rs_fmt_bytes(fmt);
  const uint8_t* __restrict__ p = (const uint8_t*)x + n * C * bytes;
  if (C == 1) ch = 0;
  if (ch >= 0) {
    const uint32_t v = rs_bytes(p + ch * bytes, bytes);
    if (fmt == AVSEP_SAMPLE_F32) return __uint_as_float(v);
    return (float)rs_pcm(v, fmt) * (fmt == AVSEP_SAMPLE_S16 ? 0x1p-15f : fmt == AVSEP_SAMPLE_S24 ? 0x1p-23f : 0x1p-31f);
  }
  if (fmt == AVSEP_SAMPLE_F32) {
    double sum = 0.0;
    for (int c = 0; c < C; ++c) sum += (double)__uint_as_float(rs_bytes(p + c * 4, 4));
    return (float)(sum / (double)C);
  }
  long long sum = 0;
  for (int c = 0; c < C; ++c) sum += rs_pcm(rs_bytes(p + c * bytes, bytes), fmt);
  return (float)((double)sum / (double)((long long)C << (8 * bytes - 1)));
}

// Sample n of a row; zero outside it.  in_ch = 0: an aligned f32 row; in_ch >= 1: frames [L, in_ch] of format fmt at any
// byte address, channel ch or (ch < 0) their down-mix (rs_frame).  FAST: the frames are int16 on a 2-byte boundary; the sum
// of up to 256 channels and the divisor are exact in f32 and the f32 division is correctly rounded: rs_frame's value.
template <bool FAST>
__device__ __forceinline__ float rs_sample(const void* __restrict__ x, long long n, long long L, int in_ch, int ch, int fmt) {
  if ((unsigned long long)n >= (unsigned long long)L) return 0.f;
  if (in_ch == 0) return ((const float*)x)[n];
  if (!FAST) return rs_frame(x, n, in_ch, ch, fmt);
  const int16_t* s = (const int16_t*)x + n * in_ch;
  if (ch >= 0) return (float)s[ch] * (1.f / 32768.f);
  int sum = 0;
  for (int c = 0; c < in_ch; ++c) sum += s[c];
  return __fdiv_rn((float)sum, (float)(in_ch * 32768));
}

// One padding slot per 32 samples: lanes that read with a stride of 2, 4 or 8 samples (decimation by that factor) then
// fall on 32 different banks instead of 16, 8 or 4.
__device__ __forceinline__ int rs_slot(int s) { return s + (s >> 5); }

__device__ __forceinline__ int16_t rs_s16(float v) { return (int16_t)(int)fminf(fmaxf(rintf(v * 32768.f), -32768.f), 32767.f); }
__device__ __forceinline__ int rs_s24(float v) { return (int)fminf(fmaxf(rintf(v * 8388608.f), -8388608.f), 8388607.f); }

// v as one sample of an output format, little-endian in the low bytes; the f32 form is the accumulator's bits.
__device__ __forceinline__ uint32_t rs_encode(float v, int fmt) {
  return fmt == AVSEP_SAMPLE_S16 ? (uint32_t)(uint16_t)rs_s16(v) : fmt == AVSEP_SAMPLE_S24 ? (uint32_t)rs_s24(v) & 0xffffffu
                                                                                            : __float_as_uint(v);
}

// The low `bytes` bytes of v to p (global memory or LDS): one store where p is aligned for it, else byte by byte.
__device__ __forceinline__ void rs_put(uint8_t* p, uint32_t v, int bytes) {
  if (bytes == 4 && !((size_t)p & 3)) {
    *(uint32_t*)p = v;
  } else if (bytes == 2 && !((size_t)p & 1)) {
    *(uint16_t*)p = (uint16_t)v;
  } else {
    for (int b = 0; b < bytes; ++b) p[b] = (uint8_t)(v >> (8 * b));
  }
}

// A workgroup's tile: the RS_R * S outputs from j0 on.  Output j = j0 + dj sits at filter position
// pos = j * down + half = pos0 + dj * down: phase p = pos mod up, newest input n = pos div up, taps i = 0 .. T-1 pair x[n - i]
// with h[p + i * up] = ho[i][dj mod up] (j0 is a multiple of up, so the phase of dj is the phase of column dj mod up of the table).
// pos0 is split once per workgroup in 64 bits (j * down passes 2^31 on a ten-minute file); dj * down < 2^24 stays 32-bit.
struct RsTile {
  long long j0, n_lo;     // first output; oldest sample of the tile's first output
  int r0, nout, span;     // pos0 mod up; outputs inside the row; samples [n_lo, n_lo + span) the tile touches
};

__device__ __forceinline__ RsTile rs_tile(int up, int down, int half, int T, int S, int Lout) {
  RsTile t;
  t.j0 = (long long)blockIdx.x * (RS_R * S);
  const long long pos0 = t.j0 * down + half;
  const long long q0 = pos0 / up;
  t.r0 = (int)(pos0 - q0 * up);
  t.nout = (int)min((long long)(RS_R * S), (long long)Lout - t.j0);
  t.n_lo = q0 - (T - 1);
  t.span = (t.r0 + (t.nout - 1) * down) / up + T;            // <= the staging array: checked by the host for a full tile
  return t;
}

// The accumulation chains of a thread's RS_R outputs t0, t0 + S, ... of one row: the only arithmetic of this file, shared
// by every kernel.  STAGED: the samples [n_lo, n_lo + span) of the row are in s_x.  Otherwise (a ratio whose tile does not
// fit) every tap reads global memory: the same values in the same order, so the mode never shows in the result.
// Outputs past the row's end compute on whatever the tile holds and are not stored by the callers; their reads stay inside
// s_x (the host sized it for a full tile) or inside the row (rs_sample checks).
template <bool STAGED, bool FAST>
__device__ __forceinline__ void rs_chains(const float* s_x, const void* __restrict__ xr, long long n_lo, int L, int in_ch, int ch,
                                          int fmt, const float* __restrict__ ho, int up, int down, int M, int T, int S, int r0,
                                          int t0, float acc[RS_R]) {
  const int step = S / up * down;                            // input samples between a thread's outputs: S * down / up
  const int v = r0 + t0 * down, dq = v / up, p = v - dq * up;
  const float* __restrict__ h = ho + t0 % up;
  int top[RS_R];                                             // newest sample of output r, relative to n_lo
#pragma unroll
  for (int r = 0; r < RS_R; ++r) {
    top[r] = dq + r * step + T - 1;
    acc[r] = 0.f;
  }
#define RS_X(r, i) (STAGED ? s_x[rs_slot(top[r] - (i))] : rs_sample<FAST>(xr, n_lo + top[r] - (i), L, in_ch, ch, fmt))
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
}

// Outputs between a thread's RS_R outputs: a multiple of `up`, at least one pass of the workgroup, chosen for the fewest idle
// lanes in the last pass among the sizes whose tile of RS_R * S outputs fits the staging array: `rows` rows of the tile's
// input side by side in `slots` slots (0: none does).
static int rs_stride(int up, int down, int T, int rows, int slots) {
  int best = 0;
  double best_fill = 0.0;
  for (int S = up; S <= RS_MAX_S; S += up) {
    if (S < RS_BLOCK) continue;
    const long long span = ((long long)(up - 1) + ((long long)RS_R * S - 1) * down) / up + T;
    if ((span + span / 32 + 1) * rows > slots) break;
    const double fill = (double)S / roundup(S, RS_BLOCK);
    if (fill > best_fill + 1e-9) best = S, best_fill = fill;
  }
  return best;
}

// What the three entry points derive from (up, down): the filter's geometry and the tile.
struct RsPlan {
  int half, M, T, S, pitch;   // pitch: slots per staged row of a full tile
  bool staged;
  unsigned tiles;
};

static RsPlan rs_plan(int up, int down, long long lout, int rows, int slots) {
  RsPlan p;
  const int m = up > down ? up : down;
  p.half = 10 * m, p.M = 2 * p.half + 1;
  p.T = (p.M + up - 1) / up;
  p.S = rs_stride(up, down, p.T, rows, slots);
  p.staged = p.S > 0;
  if (!p.staged) p.S = roundup(RS_BLOCK, up);
  const long long span = ((long long)(up - 1) + ((long long)RS_R * p.S - 1) * down) / up + p.T;
  p.pitch = p.staged ? (int)(span + span / 32 + 1) : 0;
  p.tiles = (unsigned)cdiv(lout, (long long)RS_R * p.S);
  return p;
}

static bool rs_ratio_ok(int up, int down, int L, long long* lout) {
  if (up < 1 || up > RS_MAX_RATIO || down < 1 || down > RS_MAX_RATIO || L < 1) return false;
  *lout = ((long long)L * up + down - 1) / down;
  return *lout <= 0x7fffffffLL;
}

// One launch of a kernel in the form the plan asks for.
template <typename... P, typename... A>
static int rs_launch(const RsPlan& p, void (*staged)(P...), void (*unstaged)(P...), dim3 grid, avsep_stream_t stream, A... args) {
  hipLaunchKernelGGL(p.staged ? staged : unstaged, grid, dim3(RS_BLOCK), 0, (hipStream_t)stream, args...);
  AVSEP_LAUNCH_CHECK();
  return AVSEP_OK;
}
