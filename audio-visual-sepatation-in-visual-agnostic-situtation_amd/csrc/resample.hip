// Rational polyphase FIR resampling (include/avsep.h): WAV files at any sample rate in, sources at the file's rate out.
// One kernel, bandwidth-bound on paper (<= 90 multiply-adds per 4-byte output).  A workgroup owns RS_R * S consecutive
// outputs of one row, S a multiple of `up`, starting at a multiple of `up`: it stages the input samples they touch in LDS
// (converted and down-mixed on the way when the input is interleaved PCM).  A thread then computes the RS_R outputs
// t0, t0 + S, t0 + 2S, ... of the tile: they share their phase, so each coefficient is loaded once (lanes on consecutive
// columns of the table: coalesced) and used RS_R times.
// No atomics: every output is one sequential f32 fused-multiply-add chain whose order depends on (up, down, j) only.
// Two more kernels keep a file's channels apart with the same tiles and the same chains (rs_chains): resample_split_kernel
// gives the down-mix and every channel of a file's frames in one pass, resample_join_kernel turns C rows back into frames
// and writes them whole.
// Frames are taken and given as the bytes they are in a file, in the sample formats of include/avsep.h, from and to any byte
// address: a format shows in the conversion of the staging loop (rs_frame) and at the store, never in the chains.
// 16-bit frames and f32 rows on their natural boundary are most of what arrives and have a compile-time form of their own in
// every kernel (FAST, and resample_join_s16_kernel): typed loads and stores in place of rs_bytes / rs_put, the same values.
// The entry points pick it from the formats and the addresses they are handed; a caller never does.
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

// grid (ceil(Lout / (RS_R * S)), B).  Frames (in_ch >= 1) and y have any byte alignment; one output per lane.
// FAST: f32 rows or aligned int16 frames in, s16 or f32 out on its own boundary.
template <bool STAGED, bool FAST>
__global__ __launch_bounds__(RS_BLOCK) void resample_poly_kernel(const void* __restrict__ x, const float* __restrict__ ho, int up,
                                                                 int down, int half, int M, int T, int S, int L, int Lout,
                                                                 int in_ch, int fmt, int out_fmt, void* __restrict__ y) {
  __shared__ float s_x[STAGED ? RS_LDS : 1];
  const int row = blockIdx.y;
  const RsTile tl = rs_tile(up, down, half, T, S, Lout);
  const void* xr = in_ch ? x : (const void*)((const float*)x + (long long)row * L);
  if (STAGED) {
    for (int s = threadIdx.x; s < tl.span; s += RS_BLOCK) s_x[rs_slot(s)] = rs_sample<FAST>(xr, tl.n_lo + s, L, in_ch, -1, fmt);
    __syncthreads();
  }
  for (int t0 = threadIdx.x; t0 < S; t0 += RS_BLOCK) {
    if (t0 >= tl.nout) break;                                // none of this thread's outputs lies inside the row
    float acc[RS_R];
    rs_chains<STAGED, FAST>(s_x, xr, tl.n_lo, L, in_ch, -1, fmt, ho, up, down, M, T, S, tl.r0, t0, acc);
#pragma unroll
    for (int r = 0; r < RS_R; ++r) {
      const int dj = t0 + r * S;
      if (dj >= tl.nout) break;
      const long long o = (long long)row * Lout + tl.j0 + dj;
      if (!FAST)
        rs_put((uint8_t*)y + o * rs_fmt_bytes(out_fmt), rs_encode(acc[r], out_fmt), rs_fmt_bytes(out_fmt));
      else if (out_fmt == AVSEP_SAMPLE_S16)
        ((int16_t*)y)[o] = rs_s16(acc[r]);
      else
        ((float*)y)[o] = acc[r];
    }
  }
}

// grid (ceil(Lout / (RS_R * S))).  Frames [L, C] of format fmt at any byte address -> f32 [1 + C, Lout]: the workgroup makes
// its tile of every row in turn, row 0 from the down-mix and row 1 + c from channel c, so the file is fetched from HBM once
// (the later rows find the tile's frames in L2) and no de-interleaved copy of it exists.  FAST: aligned int16 frames.
template <bool STAGED, bool FAST>
__global__ __launch_bounds__(RS_BLOCK) void resample_split_kernel(const void* __restrict__ x, const float* __restrict__ ho,
                                                                  int up, int down, int half, int M, int T, int S, int L,
                                                                  int Lout, int C, int fmt, float* __restrict__ y) {
  __shared__ float s_x[STAGED ? RS_LDS : 1];
  const RsTile tl = rs_tile(up, down, half, T, S, Lout);
  for (int row = 0; row <= C; ++row) {
    const int ch = row - 1;                                  // -1: the down-mix
    if (STAGED) {
      if (row) __syncthreads();                              // the previous row's chains have read s_x
      for (int s = threadIdx.x; s < tl.span; s += RS_BLOCK) s_x[rs_slot(s)] = rs_sample<FAST>(x, tl.n_lo + s, L, C, ch, fmt);
      __syncthreads();
    }
    for (int t0 = threadIdx.x; t0 < S; t0 += RS_BLOCK) {
      if (t0 >= tl.nout) break;
      float acc[RS_R];
      rs_chains<STAGED, FAST>(s_x, x, tl.n_lo, L, C, ch, fmt, ho, up, down, M, T, S, tl.r0, t0, acc);
#pragma unroll
      for (int r = 0; r < RS_R; ++r) {
        const int dj = t0 + r * S;
        if (dj >= tl.nout) break;
        y[(long long)row * Lout + tl.j0 + dj] = acc[r];
      }
    }
  }
}

// grid (ceil(Lout / (RS_R * S))).  f32 [C, L] -> frames [Lout, C] of int16 on a 2-byte boundary.  A pass of the workgroup makes
// RS_R runs of RS_BLOCK consecutive frames; it computes them for every channel into the LDS tile s_o, laid out as the file is
// ([run][frame][channel]), and then stores each run as one contiguous stretch of RS_BLOCK * C samples, lanes on consecutive
// 4-byte words (2-byte samples where the run starts on an odd sample): no store with a stride of 2C bytes.  The C rows of the
// input tile are staged side by side, `pitch` slots apart.
template <bool STAGED>
__global__ __launch_bounds__(RS_BLOCK) void resample_join_s16_kernel(const float* __restrict__ x, const float* __restrict__ ho, int up,
                                                                 int down, int half, int M, int T, int S, int L, int Lout,
                                                                 int C, int pitch, int16_t* __restrict__ y) {
  __shared__ float s_x[STAGED ? RJ_LDS : 1];
  __shared__ __align__(4) int16_t s_o[RS_R * RS_BLOCK * RS_KEEP_CH];
  const RsTile tl = rs_tile(up, down, half, T, S, Lout);
  if (STAGED) {
    for (int c = 0; c < C; ++c)
      for (int s = threadIdx.x; s < tl.span; s += RS_BLOCK)
        s_x[c * pitch + rs_slot(s)] = rs_sample<true>(x + (long long)c * L, tl.n_lo + s, L, 0, -1, AVSEP_SAMPLE_F32);
    __syncthreads();
  }
  const bool words = ((size_t)y & 3) == 0;
  for (int tb = 0; tb < S && tb < tl.nout; tb += RS_BLOCK) {   // the same for every thread: the loop holds barriers
    const int t0 = tb + threadIdx.x;
    if (t0 < S && t0 < tl.nout) {
      for (int c = 0; c < C; ++c) {
        float acc[RS_R];
        rs_chains<STAGED, true>(s_x + c * pitch, x + (long long)c * L, tl.n_lo, L, 0, -1, AVSEP_SAMPLE_F32, ho, up, down, M, T, S, tl.r0, t0, acc);
#pragma unroll
        for (int r = 0; r < RS_R; ++r) s_o[(r * RS_BLOCK + threadIdx.x) * C + c] = rs_s16(acc[r]);
      }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < RS_R; ++r) {
      const int first = tb + r * S;                            // the run's first frame, relative to j0
      if (first >= tl.nout) break;
      const int cnt = min(min(RS_BLOCK, S - tb), tl.nout - first) * C;      // samples of the run
      const long long e0 = (tl.j0 + first) * C;
      const int16_t* src = s_o + r * RS_BLOCK * C;
      if (words && !(e0 & 1)) {
        for (int i = threadIdx.x; i < (cnt >> 1); i += RS_BLOCK) ((uint32_t*)(y + e0))[i] = ((const uint32_t*)src)[i];
        if ((cnt & 1) && threadIdx.x == 0) y[e0 + cnt - 1] = src[cnt - 1];
      } else {
        for (int i = threadIdx.x; i < cnt; i += RS_BLOCK) y[e0 + i] = src[i];
      }
    }
    __syncthreads();                                           // s_o is free for the next pass
  }
}

// resample_join_s16_kernel for the frames of any output format at any byte address: f32 [C, L] -> interleaved samples of BYTES
// bytes (2: s16, 3: s24, 4: f32).  The tile holds bytes in file layout, BYTES a sample: 16, 24 or 32 KiB at eight channels.
// The 32 KiB of the f32 form do not fit beside RJ_LDS in 64 KiB, so that form stages the smaller RJ_LDS_F32 (the host plans S
// for it; the chains do not depend on S).  A run starts at byte phase (address & 3) of y, any of the four (three-byte
// samples, an odd channel count, a data chunk at an odd file offset): every run sits in the tile at the phase its first byte has in y, four
// spare bytes a run, so that an aligned dword of the file is an aligned dword of LDS.  The store is then a head of up to
// three single bytes, a body of whole dwords on consecutive lanes and a tail of up to three bytes.
template <bool STAGED, int BYTES>
__global__ __launch_bounds__(RS_BLOCK) void resample_join_kernel(const float* __restrict__ x, const float* __restrict__ ho,
                                                                     int up, int down, int half, int M, int T, int S, int L,
                                                                     int Lout, int C, int pitch, uint8_t* __restrict__ y) {
  constexpr int RUN = RS_BLOCK * RS_KEEP_CH * BYTES + 4;       // bytes of LDS per run: a multiple of 4
  constexpr int FMT = BYTES == 2 ? AVSEP_SAMPLE_S16 : BYTES == 3 ? AVSEP_SAMPLE_S24 : AVSEP_SAMPLE_F32;
  __shared__ float s_x[STAGED ? (BYTES == 4 ? RJ_LDS_F32 : RJ_LDS) : 1];
  __shared__ __align__(4) uint8_t s_o[RS_R * RUN];
  const RsTile tl = rs_tile(up, down, half, T, S, Lout);
  if (STAGED) {
    for (int c = 0; c < C; ++c)
      for (int s = threadIdx.x; s < tl.span; s += RS_BLOCK)
        s_x[c * pitch + rs_slot(s)] = rs_sample<true>(x + (long long)c * L, tl.n_lo + s, L, 0, -1, AVSEP_SAMPLE_F32);
    __syncthreads();
  }
  for (int tb = 0; tb < S && tb < tl.nout; tb += RS_BLOCK) {   // the same for every thread: the loop holds barriers
    const int t0 = tb + threadIdx.x;
    int phase[RS_R];                                           // of each run's first byte in y
#pragma unroll
    for (int r = 0; r < RS_R; ++r) phase[r] = (int)(((size_t)y + (size_t)((tl.j0 + tb + r * S) * C * BYTES)) & 3);
    if (t0 < S && t0 < tl.nout) {
      for (int c = 0; c < C; ++c) {
        float acc[RS_R];
        rs_chains<STAGED, true>(s_x + c * pitch, x + (long long)c * L, tl.n_lo, L, 0, -1, AVSEP_SAMPLE_F32, ho, up, down, M, T, S, tl.r0, t0, acc);
#pragma unroll
        for (int r = 0; r < RS_R; ++r)
          rs_put(s_o + r * RUN + phase[r] + ((int)threadIdx.x * C + c) * BYTES, rs_encode(acc[r], FMT), BYTES);
      }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < RS_R; ++r) {
      const int first = tb + r * S;                            // the run's first frame, relative to j0
      if (first >= tl.nout) break;
      const int cnt = min(min(RS_BLOCK, S - tb), tl.nout - first) * C * BYTES;      // bytes of the run
      uint8_t* dst = y + (tl.j0 + first) * C * BYTES;
      const uint8_t* src = s_o + r * RUN + phase[r];
      const int head = min(cnt, (4 - phase[r]) & 3), body = (cnt - head) >> 2, tail = cnt - head - 4 * body;
      if ((int)threadIdx.x < head) dst[threadIdx.x] = src[threadIdx.x];
      for (int i = threadIdx.x; i < body; i += RS_BLOCK) ((uint32_t*)(dst + head))[i] = ((const uint32_t*)(src + head))[i];
      if ((int)threadIdx.x < tail) dst[head + 4 * body + threadIdx.x] = src[head + 4 * body + threadIdx.x];
    }
    __syncthreads();                                           // s_o is free for the next pass
  }
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

// p is where a typed load or store of a sample of fmt (S16 or F32) may go.
static inline bool rs_aligned(const void* p, int fmt) { return !((size_t)p & (fmt == AVSEP_SAMPLE_S16 ? 1 : 3)); }

extern "C" int avsep_resample_poly(const void* x, const float* ho, int32_t B, int32_t L, int32_t up, int32_t down, int32_t in_ch,
                                   int32_t in_fmt, int32_t out_fmt, void* y, avsep_stream_t stream) {
  if (!x || !ho || !y) return AVSEP_ERR_ARG;
  long long lout;
  if (!rs_ratio_ok(up, down, L, &lout) || B < 1 || B > 65535) return AVSEP_ERR_ARG;
  if (in_ch < 0 || in_ch > RS_MAX_CH || (in_ch >= 1 && B != 1) || !rs_fmt_in_ok(in_fmt) || !rs_fmt_out_ok(out_fmt)) return AVSEP_ERR_ARG;
  if (in_ch == 0 && (in_fmt != AVSEP_SAMPLE_F32 || ((size_t)x & 3))) return AVSEP_ERR_ARG;      // rows are aligned floats
  const RsPlan p = rs_plan(up, down, lout, 1, RS_LDS);
  const bool fast = (in_ch == 0 || (in_fmt == AVSEP_SAMPLE_S16 && rs_aligned(x, in_fmt))) && out_fmt != AVSEP_SAMPLE_S24 &&
                    rs_aligned(y, out_fmt);
  return rs_launch(p, fast ? resample_poly_kernel<true, true> : resample_poly_kernel<true, false>,
                   fast ? resample_poly_kernel<false, true> : resample_poly_kernel<false, false>, dim3(p.tiles, B), stream, x, ho, up,
                   down, p.half, p.M, p.T, p.S, L, (int)lout, in_ch, in_fmt, out_fmt, y);
}

extern "C" int avsep_resample_split(const void* x, const float* ho, int32_t L, int32_t C, int32_t up, int32_t down, int32_t in_fmt,
                                    float* y, avsep_stream_t stream) {
  if (!x || !ho || !y) return AVSEP_ERR_ARG;
  long long lout;
  if (!rs_ratio_ok(up, down, L, &lout) || C < 1 || C > RS_KEEP_CH || !rs_fmt_in_ok(in_fmt)) return AVSEP_ERR_ARG;
  const RsPlan p = rs_plan(up, down, lout, 1, RS_LDS);
  const bool fast = in_fmt == AVSEP_SAMPLE_S16 && rs_aligned(x, in_fmt);
  return rs_launch(p, fast ? resample_split_kernel<true, true> : resample_split_kernel<true, false>,
                   fast ? resample_split_kernel<false, true> : resample_split_kernel<false, false>, dim3(p.tiles), stream, x, ho, up,
                   down, p.half, p.M, p.T, p.S, L, (int)lout, C, in_fmt, y);
}

extern "C" int avsep_resample_join(const float* x, const float* ho, int32_t C, int32_t L, int32_t up, int32_t down, int32_t out_fmt,
                                   void* y, avsep_stream_t stream) {
  if (!x || !ho || !y) return AVSEP_ERR_ARG;
  long long lout;
  if (!rs_ratio_ok(up, down, L, &lout) || C < 1 || C > RS_KEEP_CH || !rs_fmt_out_ok(out_fmt)) return AVSEP_ERR_ARG;
  const RsPlan p = rs_plan(up, down, lout, C, out_fmt == AVSEP_SAMPLE_F32 ? RJ_LDS_F32 : RJ_LDS);
  const dim3 grid(p.tiles);
  if (out_fmt == AVSEP_SAMPLE_S16 && rs_aligned(y, out_fmt))
    return rs_launch(p, resample_join_s16_kernel<true>, resample_join_s16_kernel<false>, grid, stream, x, ho, up, down, p.half, p.M,
                     p.T, p.S, L, (int)lout, C, p.pitch, (int16_t*)y);
  if (out_fmt == AVSEP_SAMPLE_S16)
    return rs_launch(p, resample_join_kernel<true, 2>, resample_join_kernel<false, 2>, grid, stream, x, ho, up, down, p.half, p.M,
                     p.T, p.S, L, (int)lout, C, p.pitch, (uint8_t*)y);
  if (out_fmt == AVSEP_SAMPLE_S24)
    return rs_launch(p, resample_join_kernel<true, 3>, resample_join_kernel<false, 3>, grid, stream, x, ho, up, down, p.half, p.M,
                     p.T, p.S, L, (int)lout, C, p.pitch, (uint8_t*)y);
  return rs_launch(p, resample_join_kernel<true, 4>, resample_join_kernel<false, 4>, grid, stream, x, ho, up, down, p.half, p.M,
                   p.T, p.S, L, (int)lout, C, p.pitch, (uint8_t*)y);
}
