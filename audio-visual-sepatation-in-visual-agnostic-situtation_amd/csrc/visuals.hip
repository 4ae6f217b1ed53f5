// Evaluation visuals (include/avsep.h): spectrogram, weight and mask images as the bytes an image file takes, one launch for
// a whole batch.  One kernel body for every image kind: mask product, reduction over the frames of an image column, log
// scale, 8-bit level, colour table and the row flip happen on the way from one read of the magnitudes to one write of the
// pixels.  No atomics: every sum has a fixed order.  gfx950, wave64.
#include "common.h"

// p = mag * m is ONE f32 multiply and the mean is a sum followed by a division (avsep.h): nothing here may become an fma.
#pragma clang fp contract(off)

constexpr int SI_BLOCK = 256;
constexpr int SI_WAVES = SI_BLOCK / 64;
constexpr int SI_PIX = 4;            // adjacent pixels per store: 12 RGB bytes = three whole dwords, 4 grey bytes = one
constexpr int SI_TILE = 256;         // staged form: image columns per pass, one per thread
constexpr int SI_MAX_STAGED = 32;    // cells of up to this many frames are staged in LDS; longer ones get a wave per column
constexpr int SI_MAX_BLOCKS = 2048;  // 256 CUs x 8 blocks; the rest of the work is strided over

struct SiArgs {
  const float* mag;
  const float* mask;
  const uint8_t* table;
  float thres, scale;
  int use_thres, R, F, T, W, cell, reduce, log, ch;
};

struct __attribute__((aligned(4))) SiBytes12 {
  uint32_t a, b, c;
};

// staged products live at i + i / 32: a thread's cell starts cell floats after its neighbour's, and the extra float per 32
// keeps even cells (2, 4, ... 32) off each other's LDS banks
__host__ __device__ __forceinline__ int si_pad(int i) { return i + (i >> 5); }

static size_t si_smem(int cell) {
  const size_t staged = cell > 1 && cell <= SI_MAX_STAGED ? (size_t)si_pad(SI_TILE * cell) + 1 : 0;
  return 768 + SI_TILE + staged * sizeof(float);
}

__device__ __forceinline__ float si_product(const SiArgs& a, float g, float mk) {
  const float m = a.use_thres ? (mk > a.thres ? 1.f : 0.f) : mk;
  return g * m;
}

// max that keeps a NaN once it has seen one (numpy's max): the NaN then becomes level 0 below
__device__ __forceinline__ float si_max(float c, float p) { return (p > c || p != p) ? p : c; }

__device__ __forceinline__ int si_level(const SiArgs& a, float c) {
  const float v = a.log ? log10f(c + 1.0f) * a.scale : c * a.scale;
  // v > 255 saturates as utils.py:94 does.  A negative value or a NaN is level 0, deliberately not the reference's
  // astype(np.uint8), which wraps a negative value around and leaves a NaN to the platform.
  return v > 255.0f ? 255 : (v > 0.0f ? (int)v : 0);
}

// n <= SI_PIX adjacent pixels of source row `row` = r * F + f, from column w on, to image row F - 1 - f (the [::-1] of
// main.py:358-386 happens here).  Whole dwords where the address allows, bytes elsewhere.
__device__ __forceinline__ void si_store(const SiArgs& a, const uint8_t* s_tab, uint8_t* __restrict__ out, long long row, int w,
                                         int n, const int* lv) {
  const long long r = row / a.F;
  const int f = (int)(row - r * a.F);
  uint8_t* dst = out + ((r * a.F + (a.F - 1 - f)) * a.W + w) * a.ch;
  const bool whole = n == SI_PIX && ((uintptr_t)dst & 3) == 0;
  if (a.ch == 3) {
    uint8_t bytes[3 * SI_PIX];
#pragma unroll
    for (int j = 0; j < SI_PIX; ++j)
#pragma unroll
      for (int c = 0; c < 3; ++c) bytes[j * 3 + c] = s_tab[lv[j] * 3 + c];
    if (whole) {
      SiBytes12 o;
      o.a = bytes[0] | bytes[1] << 8 | bytes[2] << 16 | (uint32_t)bytes[3] << 24;
      o.b = bytes[4] | bytes[5] << 8 | bytes[6] << 16 | (uint32_t)bytes[7] << 24;
      o.c = bytes[8] | bytes[9] << 8 | bytes[10] << 16 | (uint32_t)bytes[11] << 24;
      *(SiBytes12*)dst = o;
    } else {
      for (int j = 0; j < 3 * n; ++j) dst[j] = bytes[j];
    }
  } else {
    if (whole) {
      *(uint32_t*)dst = (uint32_t)lv[0] | (uint32_t)lv[1] << 8 | (uint32_t)lv[2] << 16 | (uint32_t)lv[3] << 24;
    } else {
      for (int j = 0; j < n; ++j) dst[j] = (uint8_t)lv[j];
    }
  }
}

// grid (blocks): the work is strided over the blocks, in one of three forms, the same for every thread of a launch.
//   cell == 1:              a thread takes four adjacent frames of a row (one 16-byte load where the row allows) to four pixels;
//   1 < cell <= 32:         a block stages the products of 256 columns of one row in LDS with consecutive lanes on
//                           consecutive frames, then thread i reduces column i in frame order and 64 threads store;
//   cell > 32:              a wave takes four adjacent columns one after the other, its lanes striding over the cell's frames
//                           (lane l sums frames l, l + 64, ... in that order, then the butterfly over the lanes).
__global__ __launch_bounds__(SI_BLOCK) void spec_image_kernel(SiArgs a, uint8_t* __restrict__ out) {
  extern __shared__ int si_sm[];
  uint8_t* s_tab = (uint8_t*)si_sm;                  // [768]
  uint8_t* s_lv = s_tab + 768;                       // [SI_TILE] levels of a pass
  float* s_p = (float*)(si_sm + (768 + SI_TILE) / 4);  // [si_pad(SI_TILE * cell) + 1] staged products
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int T = a.T, W = a.W, cell = a.cell;
  const long long rows = (long long)a.R * a.F;
  if (a.table)
    for (int i = tid; i < 768; i += SI_BLOCK) s_tab[i] = a.table[i];
  __syncthreads();

  if (cell == 1) {
    const int G = (W + SI_PIX - 1) / SI_PIX;
    const long long groups = rows * G;
    for (long long g = (long long)blockIdx.x * SI_BLOCK + tid; g < groups; g += (long long)gridDim.x * SI_BLOCK) {
      const long long row = g / G;
      const int w = (int)(g - row * G) * SI_PIX, n = min(SI_PIX, W - w);
      const float* mp = a.mag + row * T + w;
      const float* kp = a.mask ? a.mask + row * T + w : nullptr;
      float p[SI_PIX];
      if (n == SI_PIX && ((uintptr_t)mp & 15) == 0 && ((uintptr_t)kp & 15) == 0) {
        const f32x4 v = *(const f32x4*)mp;
        p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w;
        if (kp) {
          const f32x4 k = *(const f32x4*)kp;
          p[0] = si_product(a, p[0], k.x); p[1] = si_product(a, p[1], k.y);
          p[2] = si_product(a, p[2], k.z); p[3] = si_product(a, p[3], k.w);
        }
      } else {
#pragma unroll
        for (int j = 0; j < SI_PIX; ++j) p[j] = j < n ? (kp ? si_product(a, mp[j], kp[j]) : mp[j]) : 0.f;
      }
      int lv[SI_PIX];
#pragma unroll
      for (int j = 0; j < SI_PIX; ++j) lv[j] = si_level(a, p[j]);
      si_store(a, s_tab, out, row, w, n, lv);
    }
  } else if (cell <= SI_MAX_STAGED) {
    const int tiles_row = (W + SI_TILE - 1) / SI_TILE;
    const long long tiles = rows * tiles_row;
    for (long long tl = blockIdx.x; tl < tiles; tl += gridDim.x) {     // the same trip count for every thread of the block
      const long long row = tl / tiles_row;
      const int w0 = (int)(tl - row * tiles_row) * SI_TILE, npx = min(SI_TILE, W - w0);
      const long long t0 = (long long)w0 * cell;                       // < T: column w0 exists
      const int nfr = (int)min((long long)npx * cell, (long long)T - t0);
      const float* mp = a.mag + row * T + t0;
      const float* kp = a.mask ? a.mask + row * T + t0 : nullptr;
      int done = 0;
      if (((uintptr_t)mp & 15) == 0 && ((uintptr_t)kp & 15) == 0) {
        done = nfr & ~3;
        for (int i = tid * 4; i < done; i += SI_BLOCK * 4) {
          const f32x4 v = *(const f32x4*)(mp + i);
          float p[4] = {v.x, v.y, v.z, v.w};
          if (kp) {
            const f32x4 k = *(const f32x4*)(kp + i);
            p[0] = si_product(a, p[0], k.x); p[1] = si_product(a, p[1], k.y);
            p[2] = si_product(a, p[2], k.z); p[3] = si_product(a, p[3], k.w);
          }
#pragma unroll
          for (int j = 0; j < 4; ++j) s_p[si_pad(i + j)] = p[j];
        }
      }
      for (int i = done + tid; i < nfr; i += SI_BLOCK) s_p[si_pad(i)] = kp ? si_product(a, mp[i], kp[i]) : mp[i];
      __syncthreads();
      if (tid < npx) {
        const int k0 = tid * cell, cnt = min(cell, nfr - k0);          // cnt >= 1: column w0 + tid starts inside the row
        float c = s_p[si_pad(k0)];
        if (a.reduce) {
          for (int k = 1; k < cnt; ++k) c += s_p[si_pad(k0 + k)];
          c = c / (float)cnt;
        } else {
          for (int k = 1; k < cnt; ++k) c = si_max(c, s_p[si_pad(k0 + k)]);
        }
        s_lv[tid] = (uint8_t)si_level(a, c);
      }
      __syncthreads();
      if (tid * SI_PIX < npx) {
        const int n = min(SI_PIX, npx - tid * SI_PIX);
        int lv[SI_PIX];
#pragma unroll
        for (int j = 0; j < SI_PIX; ++j) lv[j] = j < n ? s_lv[tid * SI_PIX + j] : 0;
        si_store(a, s_tab, out, row, w0 + tid * SI_PIX, n, lv);
      }
    }
  } else {
    const int G = (W + SI_PIX - 1) / SI_PIX;
    const long long groups = rows * G;
    for (long long g = (long long)blockIdx.x * SI_WAVES + wave; g < groups; g += (long long)gridDim.x * SI_WAVES) {
      const long long row = g / G;
      const int w = (int)(g - row * G) * SI_PIX, n = min(SI_PIX, W - w);   // the same for every lane of the wave
      const float* mp = a.mag + row * T;
      const float* kp = a.mask ? a.mask + row * T : nullptr;
      int lv[SI_PIX] = {0, 0, 0, 0};
      for (int j = 0; j < n; ++j) {
        const long long t0 = (long long)(w + j) * cell, t1 = min(t0 + cell, (long long)T);
        float c = a.reduce ? 0.f : -INFINITY;                          // a lane without a frame leaves the result alone
        for (long long t = t0 + lane; t < t1; t += 64) {
          const float p = kp ? si_product(a, mp[t], kp[t]) : mp[t];
          c = a.reduce ? c + p : si_max(c, p);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          const float q = __shfl_xor(c, o, 64);
          c = a.reduce ? c + q : si_max(c, q);
        }
        if (a.reduce) c = c / (float)(t1 - t0);
        lv[j] = si_level(a, c);
      }
      if (lane == 0) si_store(a, s_tab, out, row, w, n, lv);
    }
  }
}

extern "C" int avsep_spec_image(const float* mag, const float* mask_or_null, float thres, int32_t R, int32_t F, int32_t T,
                                int32_t cell, int32_t reduce, int32_t log, float scale, const uint8_t* table_or_null,
                                uint8_t* out, avsep_stream_t stream) {
  if (!mag || !out) return AVSEP_ERR_ARG;
  if (R <= 0 || F <= 0 || T <= 0 || cell < 1 || (reduce != 0 && reduce != 1) || (log != 0 && log != 1)) return AVSEP_ERR_ARG;
  const long long rows = (long long)R * F;
  if (rows > 0x7fffffffLL) return AVSEP_ERR_ARG;                      // beyond what one launch is asked to cover
  SiArgs a{};
  a.mag = mag; a.mask = mask_or_null; a.table = table_or_null; a.thres = thres; a.scale = scale;
  a.use_thres = thres == thres;                                       // a NaN: the mask value itself
  a.R = R; a.F = F; a.T = T; a.cell = cell; a.reduce = reduce; a.log = log;
  a.W = (int)(((long long)T + cell - 1) / cell);
  a.ch = table_or_null ? 3 : 1;
  long long blocks;
  if (cell == 1)
    blocks = (rows * ((a.W + SI_PIX - 1) / SI_PIX) + SI_BLOCK - 1) / SI_BLOCK;
  else if (cell <= SI_MAX_STAGED)
    blocks = rows * ((a.W + SI_TILE - 1) / SI_TILE);
  else
    blocks = (rows * ((a.W + SI_PIX - 1) / SI_PIX) + SI_WAVES - 1) / SI_WAVES;
  if (blocks > SI_MAX_BLOCKS) blocks = SI_MAX_BLOCKS;
  hipLaunchKernelGGL(spec_image_kernel, dim3((unsigned)blocks), dim3(SI_BLOCK), si_smem(cell), (hipStream_t)stream, a, out);
  AVSEP_LAUNCH_CHECK();
  return AVSEP_OK;
}
