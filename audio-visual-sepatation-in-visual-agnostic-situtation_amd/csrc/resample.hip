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
#include "resample_parts.h"

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
