// Stem levels (include/avsep.h): the two measurements of ITU-R BS.1770-4 that need every sample of a stem, taken where the
// stems lie just before they are encoded (neither writes a waveform), and the linked look-ahead limiter that keeps them under
// a true-peak ceiling there (avsep_limiter, at the end of this file: the meter's oversampler is its detector).
//
// avsep_loudness_energies: the K-weighting is a cascade of two biquads, a serial recurrence in time.  It is also a linear
// system with four state values (two per section, transposed direct form II), so a row is cut into PIECES that run in
// parallel:
//   plan (a function of h only): a sub-block of h samples is np = ceil(h / 128) pieces, the first h mod np of them one sample
//     longer than the others (la = h div np); every sub-block is cut alike, so no piece straddles a sub-block edge and only
//     two piece lengths exist.  The tail L mod h belongs to no sub-block and is not read.
//   pass 1 (lv_piece_kernel<false>): every piece runs from the zero state and leaves its end state e_k.
//   hand-over: the state at the start of piece k+1 is v_{k+1} = M_k v_k + e_k, M_k the 4x4 transition over a piece of that
//     length (the four unit states run through the same loop on the host).  It is done on two levels: lv_sub_kernel<false>
//     folds the np pieces of each sub-block into one (M_sub, e_sub) in parallel, lv_scan_kernel walks a row's sub-blocks
//     in order (one lane per row, tiles of the e_sub in LDS), lv_sub_kernel<true> unfolds the piece starts again.
//   pass 2 (lv_piece_kernel<true>): every piece runs again from its true start state and sums y^2; lv_fold_kernel adds the
//     piece sums of a sub-block in ascending order.
// Everything is float64 (a sample is converted once), nothing is atomic, and no sum's order depends on R, L or the grid:
// a row gives the same bits alone, in a batch, for a longer L and on a second call.
// One lane per piece walking its own stretch would read 64 cache lines per load; instead a workgroup stages 32 samples of
// each of its 256 pieces in LDS with 16-byte loads (lanes on consecutive quads of a piece's stretch), and every lane then
// reads its own line of the tile (pitch 37 words: odd, so 64 lanes fall on 64 banks).
//
// avsep_true_peak: the 4x (2x, 1x) oversampled peak of Annex 2 with resample.hip's filter indexing at down = 1, in float64:
// a workgroup stages a tile of the row with a halo of 10 samples as doubles, every lane reads the 28 samples of eight
// consecutive input positions once and makes all `os` phases of them in registers, and the maxima (order-free, exact) go
// per workgroup to the workspace and from there per row to `peaks`.
#include <math.h>
#include "common.h"

constexpr int LV_BLOCK = 256;
constexpr int LV_PIECE = 128;                    // longest piece, samples
constexpr int LV_CHUNK = 32;                     // samples of a piece staged per round
constexpr int LV_QUADS = LV_CHUNK / 4 + 1;       // aligned 16-byte quads that cover a chunk at any misalignment
constexpr int LV_PITCH = 4 * LV_QUADS + 1;       // words per piece in the tile

struct LvPlan { int np, la, rem; };              // pieces per sub-block; the short length; pieces (at the front) of la + 1
struct LvCoef { double c[10]; };                 // b0 b1 b2 a1 a2 of the first section, then of the second
struct LvMat { double m[16]; };                  // row-major 4x4

static LvPlan lv_plan(int h) {
  LvPlan p;
  p.np = (int)(((long long)h + LV_PIECE - 1) / LV_PIECE);   // h reaches 2^31 - 1
  p.la = h / p.np;
  p.rem = h % p.np;
  return p;
}

// One sample through both sections (transposed direct form II); v is the four state values.
__host__ __device__ __forceinline__ double lv_step(const LvCoef& k, double v[4], double x) {
  const double y1 = k.c[0] * x + v[0];
  v[0] = k.c[1] * x - k.c[3] * y1 + v[1];
  v[1] = k.c[2] * x - k.c[4] * y1;
  const double y2 = k.c[5] * y1 + v[2];
  v[2] = k.c[6] * y1 - k.c[8] * y2 + v[3];
  v[3] = k.c[7] * y1 - k.c[9] * y2;
  return y2;
}

// v = M v + e
__device__ __forceinline__ void lv_advance(const LvMat& M, double v[4], const double e[4]) {
  double o[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) o[i] = M.m[4 * i] * v[0] + M.m[4 * i + 1] * v[1] + M.m[4 * i + 2] * v[2] + M.m[4 * i + 3] * v[3] + e[i];
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] = o[i];
}

// grid (ceil(NP / LV_BLOCK), R), a lane per piece.  state [R][4][NP]: SUM = false writes the piece's end state from rest,
// SUM = true reads its start state and writes psum [R][NP] = sum of y^2 over the piece.  total = R * L.
template <bool SUM>
__global__ __launch_bounds__(LV_BLOCK) void lv_piece_kernel(const float* __restrict__ x, int L, long long total, int h, LvPlan pl,
                                                            long long NP, LvCoef k, double* __restrict__ state,
                                                            double* __restrict__ psum) {
  __shared__ float s_x[LV_BLOCK * LV_PITCH];
  __shared__ long long s_g[LV_BLOCK];            // element index in x of every piece's first staged quad (16-byte aligned address)
  __shared__ int s_need[LV_BLOCK];               // staged words of the piece that matter: misalignment + length (0: no piece)
  const int tid = threadIdx.x, r = blockIdx.y;
  const long long piece = (long long)blockIdx.x * LV_BLOCK + tid;
  int len = 0, mis = 0;
  if (piece < NP) {
    const long long s = piece / pl.np;
    const int j = (int)(piece - s * pl.np);
    const long long g = (long long)r * L + s * h + (long long)j * pl.la + min(j, pl.rem);
    len = pl.la + (j < pl.rem ? 1 : 0);
    mis = (int)(((size_t)(x + g) >> 2) & 3);
    s_g[tid] = g - mis;
  }
  s_need[tid] = len ? mis + len : 0;
  double v[4] = {0.0, 0.0, 0.0, 0.0}, acc = 0.0;
  double* st = state + (long long)r * 4 * NP;
  if (SUM && len) {
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = st[q * NP + piece];
  }
  const int rounds = (pl.la + (pl.rem ? 1 : 0) + LV_CHUNK - 1) / LV_CHUNK;    // the same for every lane: the loop holds barriers
  for (int c = 0; c < rounds; ++c) {
    __syncthreads();                             // s_g / s_need are written; the previous round's reads are done
    for (int idx = tid; idx < LV_BLOCK * LV_QUADS; idx += LV_BLOCK) {
      const int p = idx / LV_QUADS, q = idx - p * LV_QUADS;
      const int w = c * LV_CHUNK + 4 * q;        // first staged word of this quad, counted from the piece's aligned base
      if (w >= s_need[p]) continue;
      const long long g = s_g[p] + w;
      float* d = s_x + p * LV_PITCH + 4 * q;
      if (g >= 0 && g + 4 <= total) {
        const f32x4 t = *(const f32x4*)(x + g);
        d[0] = t.x, d[1] = t.y, d[2] = t.z, d[3] = t.w;
      } else {                                   // the quad hangs over an end of the buffer: only what lies inside is read
#pragma unroll
        for (int e = 0; e < 4; ++e) d[e] = (g + e >= 0 && g + e < total) ? x[g + e] : 0.f;
      }
    }
    __syncthreads();
    const int n = min(LV_CHUNK, len - c * LV_CHUNK);
    const float* mine = s_x + tid * LV_PITCH + mis;
    for (int i = 0; i < n; ++i) {
      const double y = lv_step(k, v, (double)mine[i]);
      if (SUM) acc += y * y;
    }
  }
  if (!len) return;
  if (SUM) {
    psum[(long long)r * NP + piece] = acc;
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q) st[q * NP + piece] = v[q];
  }
}

// grid (ceil(S / LV_BLOCK), R), a lane per sub-block.  EXPAND = false: the pieces' end states from rest (state) folded into
// the sub-block's own, sub [R][4][S].  EXPAND = true: sub holds the state at every sub-block's start; the pieces' slots get
// the state at their start.
template <bool EXPAND>
__global__ __launch_bounds__(LV_BLOCK) void lv_sub_kernel(int S, LvPlan pl, long long NP, LvMat m_long, LvMat m_short,
                                                          double* __restrict__ state, double* __restrict__ sub) {
  const int s = blockIdx.x * LV_BLOCK + threadIdx.x, r = blockIdx.y;
  if (s >= S) return;
  double* st = state + (long long)r * 4 * NP;
  double* sb = sub + (long long)r * 4 * S;
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  if (EXPAND) {
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = sb[(long long)q * S + s];
  }
  for (int j = 0; j < pl.np; ++j) {
    const long long p = (long long)s * pl.np + j;
    double e[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) e[q] = st[q * NP + p];
    if (EXPAND) {
#pragma unroll
      for (int q = 0; q < 4; ++q) st[q * NP + p] = v[q];
    }
    lv_advance(j < pl.rem ? m_long : m_short, v, e);
  }
  if (!EXPAND) {
#pragma unroll
    for (int q = 0; q < 4; ++q) sb[(long long)q * S + s] = v[q];
  }
}

// grid (R).  sub [R][4][S]: every sub-block's end state from rest in, the state at its start out.  The walk is serial; the
// workgroup moves tiles of LV_BLOCK sub-blocks through LDS so that the one walking lane never waits on memory.
__global__ __launch_bounds__(LV_BLOCK) void lv_scan_kernel(int S, LvMat m_sub, double* __restrict__ sub) {
  __shared__ double s_e[4][LV_BLOCK], s_v[4][LV_BLOCK];
  const int tid = threadIdx.x;
  double* sb = sub + (long long)blockIdx.x * 4 * S;
  double v[4] = {0.0, 0.0, 0.0, 0.0};            // the row starts from rest
  for (int s0 = 0; s0 < S; s0 += LV_BLOCK) {
    const int n = min(LV_BLOCK, S - s0);
    if (tid < n) {
#pragma unroll
      for (int q = 0; q < 4; ++q) s_e[q][tid] = sb[(long long)q * S + s0 + tid];
    }
    __syncthreads();
    if (tid == 0) {
      for (int i = 0; i < n; ++i) {
        double e[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) e[q] = s_e[q][i], s_v[q][i] = v[q];
        lv_advance(m_sub, v, e);
      }
    }
    __syncthreads();
    if (tid < n) {
#pragma unroll
      for (int q = 0; q < 4; ++q) sb[(long long)q * S + s0 + tid] = s_v[q][tid];
    }
  }
}

// grid (ceil(S / LV_BLOCK), R): E[r, s] = the sub-block's piece sums, added in ascending order.
__global__ __launch_bounds__(LV_BLOCK) void lv_fold_kernel(int S, int np, long long NP, const double* __restrict__ psum,
                                                           double* __restrict__ E) {
  const int s = blockIdx.x * LV_BLOCK + threadIdx.x, r = blockIdx.y;
  if (s >= S) return;
  const double* p = psum + (long long)r * NP + (long long)s * np;
  double acc = 0.0;
  for (int j = 0; j < np; ++j) acc += p[j];
  E[(long long)r * S + s] = acc;
}

// The transition over `len` samples of silence: column u is the unit state u run through the loop.
static LvMat lv_transition(const LvCoef& k, int len) {
  LvMat M;
  for (int u = 0; u < 4; ++u) {
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    v[u] = 1.0;
    for (int i = 0; i < len; ++i) lv_step(k, v, 0.0);
    for (int q = 0; q < 4; ++q) M.m[4 * q + u] = v[q];
  }
  return M;
}

static LvMat lv_matmul(const LvMat& A, const LvMat& B) {
  LvMat C;
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) {
      double a = 0.0;
      for (int t = 0; t < 4; ++t) a += A.m[4 * i + t] * B.m[4 * t + j];
      C.m[4 * i + j] = a;
    }
  return C;
}

static LvMat lv_matpow(LvMat A, int n) {
  LvMat P;
  for (int i = 0; i < 16; ++i) P.m[i] = (i % 5 == 0) ? 1.0 : 0.0;
  for (; n > 0; n >>= 1) {
    if (n & 1) P = lv_matmul(A, P);
    A = lv_matmul(A, A);
  }
  return P;
}

static bool lv_shape_ok(int R, int L, int h) { return R >= 1 && R <= 65535 && h >= 1 && L >= h; }

// doubles: the pieces' states [R][4][NP] and sums [R][NP], the sub-blocks' states [R][4][S]
static size_t lv_ws_doubles(int R, int L, int h) {
  const long long S = L / h, NP = S * lv_plan(h).np;
  return (size_t)R * (size_t)(5 * NP + 4 * S);
}

extern "C" size_t avsep_loudness_energies_workspace_bytes(int32_t R, int32_t L, int32_t h) {
  return lv_shape_ok(R, L, h) ? lv_ws_doubles(R, L, h) * sizeof(double) : 0;
}

extern "C" int avsep_loudness_energies(const float* x, const double* sos, int32_t R, int32_t L, int32_t h, double* E, void* ws,
                                       size_t ws_bytes, avsep_stream_t stream) {
  if (!x || !sos || !E || !ws || !lv_shape_ok(R, L, h)) return AVSEP_ERR_ARG;
  LvCoef k;
  for (int s = 0; s < 2; ++s) {
    const double* c = sos + 6 * s;
    for (int i = 0; i < 6; ++i)
      if (!isfinite(c[i])) return AVSEP_ERR_ARG;
    if (c[3] != 1.0) return AVSEP_ERR_ARG;       // normalised sections: b0 b1 b2 1 a1 a2
    k.c[5 * s] = c[0], k.c[5 * s + 1] = c[1], k.c[5 * s + 2] = c[2], k.c[5 * s + 3] = c[4], k.c[5 * s + 4] = c[5];
  }
  if (ws_bytes < lv_ws_doubles(R, L, h) * sizeof(double)) return AVSEP_ERR_WORKSPACE;
  const LvPlan pl = lv_plan(h);
  const int S = L / h;
  const long long NP = (long long)S * pl.np;
  const LvMat m_short = lv_transition(k, pl.la), m_long = lv_transition(k, pl.la + 1);
  const LvMat m_sub = lv_matmul(lv_matpow(m_short, pl.np - pl.rem), lv_matpow(m_long, pl.rem));   // the long pieces come first
  double* state = (double*)ws;
  double* psum = state + (size_t)R * 4 * NP;
  double* sub = psum + (size_t)R * NP;
  const hipStream_t st = (hipStream_t)stream;
  const dim3 pgrid((unsigned)cdiv(NP, LV_BLOCK), R), sgrid((unsigned)cdiv(S, LV_BLOCK), R);
  const long long total = (long long)R * L;
  hipLaunchKernelGGL(lv_piece_kernel<false>, pgrid, dim3(LV_BLOCK), 0, st, x, L, total, h, pl, NP, k, state, psum);
  AVSEP_LAUNCH_CHECK();
  hipLaunchKernelGGL(lv_sub_kernel<false>, sgrid, dim3(LV_BLOCK), 0, st, S, pl, NP, m_long, m_short, state, sub);
  AVSEP_LAUNCH_CHECK();
  hipLaunchKernelGGL(lv_scan_kernel, dim3(R), dim3(LV_BLOCK), 0, st, S, m_sub, sub);
  AVSEP_LAUNCH_CHECK();
  hipLaunchKernelGGL(lv_sub_kernel<true>, sgrid, dim3(LV_BLOCK), 0, st, S, pl, NP, m_long, m_short, state, sub);
  AVSEP_LAUNCH_CHECK();
  hipLaunchKernelGGL(lv_piece_kernel<true>, pgrid, dim3(LV_BLOCK), 0, st, x, L, total, h, pl, NP, k, state, psum);
  AVSEP_LAUNCH_CHECK();
  hipLaunchKernelGGL(lv_fold_kernel, sgrid, dim3(LV_BLOCK), 0, st, S, pl.np, NP, (const double*)psum, E);
  AVSEP_LAUNCH_CHECK();
  return AVSEP_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// true peak
// ---------------------------------------------------------------------------------------------------------------------
constexpr int TP_BLOCK = 256;
constexpr int TP_PER = 8;                        // input positions per lane
constexpr int TP_TILE = TP_BLOCK * TP_PER;
constexpr int TP_HALF = 10;                      // the filter reaches 10 input samples to either side
constexpr int TP_T = 2 * TP_HALF + 1;
constexpr int TP_WIN = TP_PER + 2 * TP_HALF;     // samples the TP_PER consecutive positions of a lane touch

// One padding slot per TP_PER doubles: lanes that read with a stride of TP_PER doubles then fall on 32 different bank pairs.
__device__ __forceinline__ int tp_slot(int s) { return s + s / TP_PER; }

// |v| with every non-finite value (NaN included) as +inf
__device__ __forceinline__ double tp_abs(double v) {
  const double a = fabs(v);
  return a <= 1.7976931348623157e308 ? a : (double)INFINITY;
}

__device__ __forceinline__ double tp_wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

// The workgroup's maximum of (a, b) to out[0], out[1] (all lanes call).
__device__ __forceinline__ void tp_block_max(double a, double b, double* out) {
  __shared__ double s_m[2][TP_BLOCK / 64];
  a = tp_wave_max(a), b = tp_wave_max(b);
  if ((threadIdx.x & 63) == 0) s_m[0][threadIdx.x >> 6] = a, s_m[1][threadIdx.x >> 6] = b;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < TP_BLOCK / 64; ++w) a = fmax(a, s_m[0][w]), b = fmax(b, s_m[1][w]);
    out[0] = a, out[1] = b;
  }
}

constexpr int TP_LDS = TP_TILE + 2 * TP_HALF + (TP_TILE + 2 * TP_HALF) / TP_PER + 1;   // doubles of a staged tile

// The oversampler, shared by the meter (tp_tile_kernel) and the limiter's detector (lim_detect_kernel).  The workgroup stages
// the tile of the row xr [L] that starts at q0, with its halo, as doubles; after the barrier every lane reads the samples its
// TP_PER consecutive positions touch once (xs; position k's own sample is xs[k + TP_HALF]) and makes all OS phases of them.
// Input position q in [0, L) carries the outputs m = q * OS + p: pos = m + 10 * OS, phase p, newest sample n0 = q + 10, so
// acc[k][p] = u[m] = sum_i x[q + 10 - i] * taps[i][p], i ascending.
template <int OS>
__device__ __forceinline__ void tp_oversample(const float* __restrict__ xr, const double* __restrict__ taps, int L, long long q0,
                                              double* s_x, double xs[TP_WIN], double acc[TP_PER][OS]) {
  const int tid = threadIdx.x;
  for (int s = tid; s < TP_TILE + 2 * TP_HALF; s += TP_BLOCK) {
    const long long n = q0 - TP_HALF + s;
    s_x[tp_slot(s)] = (n >= 0 && n < L) ? (double)xr[n] : 0.0;
  }
  __syncthreads();
  // the lane's window: the samples its TP_PER consecutive positions touch, read from LDS once
#pragma unroll
  for (int j = 0; j < TP_WIN; ++j) xs[j] = s_x[tp_slot(tid * TP_PER + j)];
#pragma unroll
  for (int k = 0; k < TP_PER; ++k)
#pragma unroll
    for (int p = 0; p < OS; ++p) acc[k][p] = 0.0;
#pragma unroll
  for (int i = 0; i < TP_T; ++i) {
#pragma unroll
    for (int p = 0; p < OS; ++p) {
      const double c = taps[i * OS + p];
#pragma unroll
      for (int k = 0; k < TP_PER; ++k) acc[k][p] = fma(xs[k + 2 * TP_HALF - i], c, acc[k][p]);
    }
  }
}

// grid (tiles, R).  part [R][tiles][2] = the tile's (sample peak, oversampled peak).
template <int OS>
__global__ __launch_bounds__(TP_BLOCK) void tp_tile_kernel(const float* __restrict__ x, const double* __restrict__ taps, int L,
                                                           double* __restrict__ part) {
  __shared__ double s_x[TP_LDS];
  const int tid = threadIdx.x;
  const long long q0 = (long long)blockIdx.x * TP_TILE;
  double xs[TP_WIN], acc[TP_PER][OS];
  tp_oversample<OS>(x + (long long)blockIdx.y * L, taps, L, q0, s_x, xs, acc);
  double ps = 0.0, pu = 0.0;
#pragma unroll
  for (int k = 0; k < TP_PER; ++k) {
    if (q0 + tid * TP_PER + k >= L) continue;
    ps = fmax(ps, tp_abs(xs[k + TP_HALF]));
#pragma unroll
    for (int p = 0; p < OS; ++p) pu = fmax(pu, tp_abs(acc[k][p]));
  }
  tp_block_max(ps, pu, part + ((long long)blockIdx.y * gridDim.x + blockIdx.x) * 2);
}

// grid (R): the row's maxima over its tiles; the true peak is never below the sample peak.
__global__ __launch_bounds__(TP_BLOCK) void tp_row_kernel(const double* __restrict__ part, int tiles, double* __restrict__ peaks) {
  const double* p = part + (long long)blockIdx.x * tiles * 2;
  double a = 0.0, b = 0.0;
  for (int t = threadIdx.x; t < tiles; t += TP_BLOCK) a = fmax(a, p[2 * t]), b = fmax(b, p[2 * t + 1]);
  double out[2] = {0.0, 0.0};
  tp_block_max(a, b, out);
  if (threadIdx.x == 0) {
    peaks[2 * blockIdx.x] = out[0];
    peaks[2 * blockIdx.x + 1] = fmax(out[0], out[1]);
  }
}

static bool tp_shape_ok(int R, int L, int os) {
  return R >= 1 && R <= 65535 && L >= 1 && (os == 1 || os == 2 || os == 4) && (long long)os * L < 0x80000000LL;
}

extern "C" size_t avsep_true_peak_workspace_bytes(int32_t R, int32_t L) {
  return (R >= 1 && R <= 65535 && L >= 1) ? (size_t)R * (size_t)cdiv(L, TP_TILE) * 2 * sizeof(double) : 0;
}

extern "C" int avsep_true_peak(const float* x, const double* taps, int32_t R, int32_t L, int32_t os, double* peaks, void* ws,
                               size_t ws_bytes, avsep_stream_t stream) {
  if (!x || !taps || !peaks || !ws || !tp_shape_ok(R, L, os)) return AVSEP_ERR_ARG;
  if (ws_bytes < avsep_true_peak_workspace_bytes(R, L)) return AVSEP_ERR_WORKSPACE;
  const int tiles = cdiv(L, TP_TILE);
  const dim3 grid(tiles, R);
  const hipStream_t st = (hipStream_t)stream;
  double* part = (double*)ws;
  if (os == 1)
    hipLaunchKernelGGL(tp_tile_kernel<1>, grid, dim3(TP_BLOCK), 0, st, x, taps, L, part);
  else if (os == 2)
    hipLaunchKernelGGL(tp_tile_kernel<2>, grid, dim3(TP_BLOCK), 0, st, x, taps, L, part);
  else
    hipLaunchKernelGGL(tp_tile_kernel<4>, grid, dim3(TP_BLOCK), 0, st, x, taps, L, part);
  AVSEP_LAUNCH_CHECK();
  hipLaunchKernelGGL(tp_row_kernel, dim3(R), dim3(TP_BLOCK), 0, st, (const double*)part, tiles, peaks);
  AVSEP_LAUNCH_CHECK();
  return AVSEP_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// linked look-ahead limiter (include/avsep.h states the definition)
// ---------------------------------------------------------------------------------------------------------------------
// Three launches over tiles of TP_TILE samples of a programme, grid (tiles, P):
//   lim_detect_kernel: the C rows of the tile go through tp_oversample one after the other, every lane keeps the running
//     maximum of its TP_PER positions in registers; r goes to the workspace [P][L], the tile's largest p to its partials.
//   lim_apply_kernel: stages r on [t0 - 2A, t0 + TP_TILE + 2A) in LDS (1 outside the row; the allocation follows A, so a
//     short look-ahead keeps several workgroups on a CU), takes the sliding minimum of width 2A + 1 in place by doubling
//     (m_2k[s] = min(m_k[s], m_k[s + k]); the last step joins two windows of the largest power of two), smooths 1 - h with w
//     in ascending k (every lane eight consecutive positions: one LDS read per eight fma, the weights are wave-uniform),
//     hands g to the workgroup through LDS and then walks the C rows with coalesced loads and stores.  A tile whose staged
//     r are all 1 skips minimum and sum: g = 1 - 0 there whatever the order.
//   lim_stats_kernel: a programme's partials to stats.
constexpr int LIM_MAX_A = 2048;
constexpr int LIM_MAX_C = 64;
constexpr int LIM_PAD = 16;                      // staged slots past the envelope that the unrolled sum touches with weight 0

static size_t lim_lds_doubles(int A) {
  const int n = TP_TILE + 4 * A + LIM_PAD;
  return (size_t)n + n / TP_PER + 1;
}

// r [P][L]; part [P][tiles][3]: slot 0 = the tile's largest p
template <int OS>
__global__ __launch_bounds__(TP_BLOCK) void lim_detect_kernel(const float* __restrict__ x, const double* __restrict__ taps, int C, int L,
                                                              double G, double ceiling, double* __restrict__ r,
                                                              double* __restrict__ part) {
  __shared__ double s_x[TP_LDS];
  const int tid = threadIdx.x;
  const long long q0 = (long long)blockIdx.x * TP_TILE;
  const float* xp = x + (long long)blockIdx.y * C * L;
  double pk[TP_PER];
#pragma unroll
  for (int k = 0; k < TP_PER; ++k) pk[k] = 0.0;
  for (int c = 0; c < C; ++c) {
    if (c) __syncthreads();                      // every lane has read its window of the previous row
    double xs[TP_WIN], acc[TP_PER][OS];
    tp_oversample<OS>(xp + (long long)c * L, taps, L, q0, s_x, xs, acc);
#pragma unroll
    for (int k = 0; k < TP_PER; ++k) {
      pk[k] = fmax(pk[k], tp_abs(xs[k + TP_HALF]));
#pragma unroll
      for (int p = 0; p < OS; ++p) pk[k] = fmax(pk[k], tp_abs(acc[k][p]));
    }
  }
  double* rr = r + (long long)blockIdx.y * L;
  double top = 0.0;
#pragma unroll
  for (int k = 0; k < TP_PER; ++k) {
    const long long n = q0 + tid * TP_PER + k;
    if (n >= L) continue;
    top = fmax(top, pk[k]);
    rr[n] = fmin(1.0, ceiling / (G * pk[k]));    // p = 0: c / 0 = +inf, so 1; p = +inf: 0
  }
  double out[2] = {0.0, 0.0};
  tp_block_max(top, 0.0, out);
  if (tid == 0) part[((long long)blockIdx.y * gridDim.x + blockIdx.x) * 3] = out[0];
}

// y may be x: a sample is read and written by the same lane.  part slots 1, 2 = the tile's smallest g, its count of g < 1.
__global__ __launch_bounds__(TP_BLOCK) void lim_apply_kernel(const float* x, const double* __restrict__ r, const double* __restrict__ w,
                                                             int C, int L, int A, double G, float* y, double* __restrict__ gain,
                                                             double* __restrict__ part) {
  extern __shared__ double s_m[];                // lim_lds_doubles(A)
  __shared__ double s_min[TP_BLOCK / 64];
  __shared__ int s_cnt[TP_BLOCK / 64];
  const int tid = threadIdx.x;
  const long long t0 = (long long)blockIdx.x * TP_TILE;
  const int n = TP_TILE + 4 * A, W = 2 * A + 1, reach = TP_TILE + 2 * A;
  const double* rr = r + (long long)blockIdx.y * L;
  int touched = 0;
  for (int s = tid; s < n + LIM_PAD; s += TP_BLOCK) {
    const long long idx = t0 - 2 * A + s;
    const double v = (s < n && idx >= 0 && idx < L) ? rr[idx] : 1.0;
    touched |= (v != 1.0) ? 1 : 0;
    s_m[tp_slot(s)] = v;
  }
  double g[TP_PER];                              // of the positions t0 + tid * TP_PER + i
#pragma unroll
  for (int i = 0; i < TP_PER; ++i) g[i] = 1.0;
  if (__syncthreads_or(touched)) {               // the same answer in every lane: the barriers below are met by all
    // m_k[s] = min of the staged r over [s, s + k), valid where s + k <= n.  A pass reads a chunk, waits, writes it: a later
    // chunk reads only slots that no earlier chunk has written.
    int k = 1;
    for (; 2 * k <= W; k *= 2) {
      for (int base = 0; base + 2 * k <= n; base += TP_TILE) {
        double v[TP_PER];
#pragma unroll
        for (int i = 0; i < TP_PER; ++i) {
          const int s = base + i * TP_BLOCK + tid;
          v[i] = (s + 2 * k <= n) ? fmin(s_m[tp_slot(s)], s_m[tp_slot(s + k)]) : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < TP_PER; ++i) {
          const int s = base + i * TP_BLOCK + tid;
          if (s + 2 * k <= n) s_m[tp_slot(s)] = v[i];
        }
      }
      __syncthreads();
    }
    // h[t0 - A + s] = min(m_k[s], m_k[s + W - k]) for s in [0, reach); the slot gets the reduction 1 - h
    const int rest = W - k;
    for (int base = 0; base < reach; base += TP_TILE) {
      double v[TP_PER];
#pragma unroll
      for (int i = 0; i < TP_PER; ++i) {
        const int s = base + i * TP_BLOCK + tid;
        v[i] = (s < reach) ? 1.0 - fmin(s_m[tp_slot(s)], s_m[tp_slot(s + rest)]) : 0.0;
      }
      __syncthreads();
#pragma unroll
      for (int i = 0; i < TP_PER; ++i) {
        const int s = base + i * TP_BLOCK + tid;
        if (s < reach) s_m[tp_slot(s)] = v[i];
      }
    }
    __syncthreads();
    // g[q] = 1 - sum_{kk = 0 .. 2A} w[kk] * d[q + kk].  Slot j = i + kk of the lane serves its eight positions i with the weights
    // w[j - i]; those before w's start and past its end are 0, and the slots from `reach` on hold finite values in [0, 1].
    double acc[TP_PER], wp[TP_PER];
#pragma unroll
    for (int i = 0; i < TP_PER; ++i) acc[i] = 0.0, wp[i] = 0.0;
    for (int jb = 0; jb < 2 * A + TP_PER; jb += TP_PER) {
      double wc[TP_PER];
#pragma unroll
      for (int u = 0; u < TP_PER; ++u) wc[u] = (jb + u < W) ? w[jb + u] : 0.0;
#pragma unroll
      for (int u = 0; u < TP_PER; ++u) {
        const double d = s_m[tp_slot(tid * TP_PER + jb + u)];
#pragma unroll
        for (int i = 0; i < TP_PER; ++i) acc[i] = fma(u >= i ? wc[u - i] : wp[TP_PER + u - i], d, acc[i]);
      }
#pragma unroll
      for (int u = 0; u < TP_PER; ++u) wp[u] = wc[u];
    }
#pragma unroll
    for (int i = 0; i < TP_PER; ++i) g[i] = 1.0 - acc[i];
    __syncthreads();                             // every lane has read its reductions: the slots are free for g
  }
  double gmin = (double)INFINITY;
  int cnt = 0;
#pragma unroll
  for (int i = 0; i < TP_PER; ++i) {
    s_m[tid * TP_PER + i] = g[i];
    if (t0 + tid * TP_PER + i >= L) continue;
    gmin = fmin(gmin, g[i]);
    cnt += g[i] < 1.0 ? 1 : 0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) gmin = fmin(gmin, __shfl_xor(gmin, o, 64)), cnt += __shfl_xor(cnt, o, 64);
  if ((tid & 63) == 0) s_min[tid >> 6] = gmin, s_cnt[tid >> 6] = cnt;
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int v = 1; v < TP_BLOCK / 64; ++v) gmin = fmin(gmin, s_min[v]), cnt += s_cnt[v];
    double* p = part + ((long long)blockIdx.y * gridDim.x + blockIdx.x) * 3;
    p[1] = gmin, p[2] = (double)cnt;
  }
  double gg[TP_PER];
#pragma unroll
  for (int i = 0; i < TP_PER; ++i) {
    const int q = i * TP_BLOCK + tid;
    const double v = s_m[q];
    if (gain && t0 + q < L) gain[(long long)blockIdx.y * L + t0 + q] = v;
    gg[i] = G * v;
  }
  for (int c = 0; c < C; ++c) {
    const long long row = ((long long)blockIdx.y * C + c) * L;
#pragma unroll
    for (int i = 0; i < TP_PER; ++i) {
      const long long q = t0 + i * TP_BLOCK + tid;
      if (q < L) y[row + q] = (float)((double)x[row + q] * gg[i]);
    }
  }
}

// grid (P): maximum, minimum and the sum of integer counts (exact in float64, so order-free) over the programme's tiles
__global__ __launch_bounds__(TP_BLOCK) void lim_stats_kernel(const double* __restrict__ part, int tiles, double* __restrict__ stats) {
  __shared__ double s_r[3][TP_BLOCK / 64];
  const double* p = part + (long long)blockIdx.x * tiles * 3;
  double a = 0.0, b = (double)INFINITY, c = 0.0;
  for (int t = threadIdx.x; t < tiles; t += TP_BLOCK) a = fmax(a, p[3 * t]), b = fmin(b, p[3 * t + 1]), c += p[3 * t + 2];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) a = fmax(a, __shfl_xor(a, o, 64)), b = fmin(b, __shfl_xor(b, o, 64)), c += __shfl_xor(c, o, 64);
  if ((threadIdx.x & 63) == 0) s_r[0][threadIdx.x >> 6] = a, s_r[1][threadIdx.x >> 6] = b, s_r[2][threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int v = 1; v < TP_BLOCK / 64; ++v) a = fmax(a, s_r[0][v]), b = fmin(b, s_r[1][v]), c += s_r[2][v];
    stats[3 * blockIdx.x] = a, stats[3 * blockIdx.x + 1] = b, stats[3 * blockIdx.x + 2] = c;
  }
}

static bool lim_shape_ok(int P, int C, int L) { return P >= 1 && P <= 65535 && C >= 1 && C <= LIM_MAX_C && L >= 1; }

// doubles: r [P][L], the partials [P][tiles][3]
static size_t lim_ws_doubles(int P, int L) { return (size_t)P * ((size_t)L + 3 * (size_t)cdiv(L, TP_TILE)); }

extern "C" size_t avsep_limiter_workspace_bytes(int32_t P, int32_t C, int32_t L) {
  return lim_shape_ok(P, C, L) ? lim_ws_doubles(P, L) * sizeof(double) : 0;
}

extern "C" int avsep_limiter(const float* x, const double* taps, const double* w, int32_t P, int32_t C, int32_t L, int32_t os, int32_t A,
                             double pre_gain, double ceiling, float* y, double* gain, double* stats, void* ws, size_t ws_bytes,
                             avsep_stream_t stream) {
  if (!x || !taps || !w || !y || !stats || !ws || !lim_shape_ok(P, C, L) || !tp_shape_ok(1, L, os)) return AVSEP_ERR_ARG;
  if (A < 1 || A > LIM_MAX_A || !isfinite(pre_gain) || !(pre_gain > 0.0) || !(ceiling > 0.0 && ceiling <= 1.0)) return AVSEP_ERR_ARG;
  if (ws_bytes < lim_ws_doubles(P, L) * sizeof(double)) return AVSEP_ERR_WORKSPACE;
  const int tiles = cdiv(L, TP_TILE);
  const dim3 grid(tiles, P);
  const hipStream_t st = (hipStream_t)stream;
  double* r = (double*)ws;
  double* part = r + (size_t)P * L;
  const size_t lds = lim_lds_doubles(A) * sizeof(double);
  if (lds > 64 * 1024 &&
      hipFuncSetAttribute((const void*)lim_apply_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return AVSEP_ERR_LAUNCH;
  if (os == 1)
    hipLaunchKernelGGL(lim_detect_kernel<1>, grid, dim3(TP_BLOCK), 0, st, x, taps, C, L, pre_gain, ceiling, r, part);
  else if (os == 2)
    hipLaunchKernelGGL(lim_detect_kernel<2>, grid, dim3(TP_BLOCK), 0, st, x, taps, C, L, pre_gain, ceiling, r, part);
  else
    hipLaunchKernelGGL(lim_detect_kernel<4>, grid, dim3(TP_BLOCK), 0, st, x, taps, C, L, pre_gain, ceiling, r, part);
  AVSEP_LAUNCH_CHECK();
  hipLaunchKernelGGL(lim_apply_kernel, grid, dim3(TP_BLOCK), lds, st, x, (const double*)r, w, C, L, A, pre_gain, y, gain, part);
  AVSEP_LAUNCH_CHECK();
  hipLaunchKernelGGL(lim_stats_kernel, dim3(P), dim3(TP_BLOCK), 0, st, (const double*)part, tiles, stats);
  AVSEP_LAUNCH_CHECK();
  return AVSEP_OK;
}
