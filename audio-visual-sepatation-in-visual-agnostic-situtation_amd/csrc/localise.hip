// Sound-source localisation over a clip (include/avsep.h): the CoLoc similarity maps of every video frame in one launch,
// and their JET heat maps blended over the frames in one launch.  No atomics: every sum has a fixed order.  gfx950, wave64.
#include "common.h"

// The overlay is DEFINED by an order of fp32 operations that a NumPy restatement repeats bit for bit (avsep.h): nothing in
// this file may be contracted into an fma by the compiler.  The dot products below call fmaf() themselves.
#pragma clang fp contract(off)

#define LM_EPS 1e-8f
constexpr int LM_MAXC = 3;
constexpr int LM_WAVES = 16;
constexpr int LM_BLOCK = LM_WAVES * 64;

// itertools.permutations(range(C)) for C = 2 (first two rows, first two columns of PERM2) and C = 3
__device__ const signed char LM_PERM2[2][2] = {{0, 1}, {1, 0}};
__device__ const signed char LM_PERM3[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
__device__ __forceinline__ int lm_perm(int C, int p, int c) { return C == 2 ? LM_PERM2[p][c] : LM_PERM3[p][c]; }

struct LmArgs {
  const float* x;
  const int* win;
  const float* v[LM_MAXC];
  int T, K, C, Dc, D, FT, HW, att, vec;
};

static size_t lm_smem(int C, int Dc, int HW) {
  return ((size_t)C * Dc + (size_t)C * C * HW + (size_t)LM_WAVES * (C + 1) * HW + 4 + 12 + 4) * sizeof(float);
}

// grid (T): one workgroup per video frame.  Lanes run along hw (a row of v is contiguous: a wave reads whole lines), the
// Dc channels are dealt to the 16 waves, whose partial sums meet in LDS and are added in wave order.
__global__ __launch_bounds__(LM_BLOCK) void localise_maps_kernel(LmArgs a, float* __restrict__ maps, int* __restrict__ best_out,
                                                                 float* __restrict__ scores) {
  extern __shared__ float sm[];
  const int t = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int C = a.C, Dc = a.Dc, HW = a.HW, FT = a.FT, CD = C * Dc;
  float* s_a = sm;                                   // [C*Dc]   pooled audio blocks
  float* s_m = s_a + CD;                             // [C*C*HW] m[(k*C + c)*HW + hw]
  float* s_part = s_m + C * C * HW;                  // [LM_WAVES][C+1][HW] per-wave partial dots and |v|^2 of one visual input
  float* s_na = s_part + LM_WAVES * (C + 1) * HW;    // [4]
  float* s_mx = s_na + 4;                            // [12]
  int* s_perm = (int*)(s_mx + 12);                   // [4]
  const int k = min(max(a.win[t], 0), a.K - 1);      // a window index outside [0, K) is clamped, never followed

  // a_i = max over F x T of the first C*Dc bottleneck channels of window k (the rule of fusion_n.hip)
  for (int i = tid; i < CD; i += LM_BLOCK) {
    const float* p = a.x + ((long long)k * a.D + i) * FT;
    float m = p[0];
    for (int j = 1; j < FT; ++j) m = p[j] > m ? p[j] : m;
    s_a[i] = m;
  }
  __syncthreads();
  if (a.att == 0) {
    for (int i = wave; i < C; i += LM_WAVES) {
      float q = 0.f;
      for (int d = lane; d < Dc; d += 64) q = fmaf(s_a[i * Dc + d], s_a[i * Dc + d], q);
      q = wave_sum(q);
      if (lane == 0) s_na[i] = sqrtf(q);
    }
    __syncthreads();
  }
  const float inv_sqrt = 1.f / sqrtf((float)Dc);
  for (int c = 0; c < C; ++c) {
    if (c > 0 && a.v[c] == a.v[c - 1]) {             // duet: the same visual input again, the same maps
      for (int i = tid; i < C * HW; i += LM_BLOCK) {
        const int blk = i / HW, hw = i - blk * HW;
        s_m[(blk * C + c) * HW + hw] = s_m[(blk * C + c - 1) * HW + hw];
      }
      __syncthreads();
      continue;
    }
    const float* vp = a.v[c] + (long long)t * Dc * HW;
    if (a.vec) {                                     // four positions per lane: one 16-byte load per channel
      for (int h4 = lane * 4; h4 < HW; h4 += 256) {
        float dot[LM_MAXC][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}}, nv[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
        for (int d = wave; d < Dc; d += LM_WAVES) {
          const f32x4 vv = *(const f32x4*)(vp + (long long)d * HW + h4);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
#pragma unroll
            for (int i = 0; i < LM_MAXC; ++i)
              if (i < C) dot[i][j] = fmaf(s_a[i * Dc + d], vv[j], dot[i][j]);
            nv[j] = fmaf(vv[j], vv[j], nv[j]);
          }
        }
        float* o = s_part + (long long)wave * (C + 1) * HW + h4;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
          for (int i = 0; i < LM_MAXC; ++i)
            if (i < C) o[i * HW + j] = dot[i][j];
          o[C * HW + j] = nv[j];
        }
      }
    } else {
      for (int hw = lane; hw < HW; hw += 64) {
        float dot[LM_MAXC] = {0.f, 0.f, 0.f}, nv = 0.f;
#pragma unroll 8
        for (int d = wave; d < Dc; d += LM_WAVES) {
          const float vv = vp[(long long)d * HW + hw];
#pragma unroll
          for (int i = 0; i < LM_MAXC; ++i)
            if (i < C) dot[i] = fmaf(s_a[i * Dc + d], vv, dot[i]);
          nv = fmaf(vv, vv, nv);
        }
        float* o = s_part + (long long)wave * (C + 1) * HW + hw;
#pragma unroll
        for (int i = 0; i < LM_MAXC; ++i)
          if (i < C) o[i * HW] = dot[i];
        o[C * HW] = nv;
      }
    }
    __syncthreads();
    for (int hw = tid; hw < HW; hw += LM_BLOCK) {
      float dot[LM_MAXC] = {0.f, 0.f, 0.f}, nv = 0.f;
      for (int w = 0; w < LM_WAVES; ++w) {
        const float* o = s_part + (long long)w * (C + 1) * HW + hw;
#pragma unroll
        for (int i = 0; i < LM_MAXC; ++i)
          if (i < C) dot[i] += o[i * HW];
        nv += o[C * HW];
      }
      nv = sqrtf(nv);
#pragma unroll
      for (int i = 0; i < LM_MAXC; ++i)
        if (i < C)
          s_m[(i * C + c) * HW + hw] = a.att == 1 ? 1.f / (1.f + expf(-dot[i] * inv_sqrt))
                                                  : dot[i] / (fmaxf(s_na[i], LM_EPS) * fmaxf(nv, LM_EPS));
    }
    __syncthreads();
  }
  for (int q = wave; q < C * C; q += LM_WAVES) {       // per-map maximum
    float mx = -INFINITY;
    for (int hw = lane; hw < HW; hw += 64) mx = fmaxf(mx, s_m[q * HW + hw]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    if (lane == 0) s_mx[q] = mx;
  }
  __syncthreads();
  if (tid == 0) {                                      // all C! permutations in itertools order, the first maximum wins
    const int P = C == 2 ? 2 : 6;
    float sbest = -INFINITY;
    int best = 0;
    for (int p = 0; p < P; ++p) {
      float s = 0.f;
      for (int c = 0; c < C; ++c) s += s_mx[lm_perm(C, p, c) * C + c];
      scores[(long long)t * P + p] = s;
      if (s > sbest) { sbest = s; best = p; }
    }
    best_out[t] = best;
    for (int c = 0; c < C; ++c) s_perm[c] = lm_perm(C, best, c);
  }
  __syncthreads();
  for (int i = tid; i < C * HW; i += LM_BLOCK) {
    const int c = i / HW, hw = i - c * HW;
    maps[(long long)t * C * HW + i] = s_m[(s_perm[c] * C + c) * HW + hw];
  }
}

extern "C" int avsep_localise_maps(const float* x, const int32_t* win, const float* const* v, int32_t T, int32_t K, int32_t C,
                                   int32_t D, int32_t FT, int32_t HW, int32_t att, float* maps, int32_t* best, float* scores,
                                   avsep_stream_t stream) {
  if (!x || !win || !v || !maps || !best || !scores) return AVSEP_ERR_ARG;
  if (T <= 0 || K <= 0 || C < 2 || C > LM_MAXC || D < C || FT <= 0 || HW <= 0 || (att != 0 && att != 1)) return AVSEP_ERR_ARG;
  LmArgs a{};
  a.x = x; a.win = win; a.T = T; a.K = K; a.C = C; a.Dc = D / C; a.D = D; a.FT = FT; a.HW = HW; a.att = att;
  a.vec = HW % 4 == 0;                               // 16-byte loads need every row of v on such a boundary
  for (int c = 0; c < C; ++c) {
    if (!v[c]) return AVSEP_ERR_ARG;
    a.v[c] = v[c];
    if ((uintptr_t)v[c] % 16 != 0) a.vec = 0;
  }
  const size_t smem = lm_smem(C, a.Dc, HW);
  if (smem > 160 * 1024) return AVSEP_ERR_ARG;
  if (smem > 64 * 1024)
    (void)hipFuncSetAttribute((const void*)localise_maps_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
  hipLaunchKernelGGL(localise_maps_kernel, dim3(T), dim3(LM_BLOCK), smem, (hipStream_t)stream, a, maps, best, scores);
  AVSEP_LAUNCH_CHECK();
  return AVSEP_OK;
}

// ============================================================================
// heat-map overlay
// ============================================================================
constexpr int HO_BLOCK = 256;
constexpr int HO_PIX = 4;      // adjacent pixels per lane: 12 output bytes = three whole dwords
constexpr int HO_ITERS = 8;    // pixel groups per lane: the map's min / max / levels are set up once per 8192 pixels

struct HoArgs {
  const float* maps;
  const float* fr[LM_MAXC];
  const uint8_t* table;
  int T, C, h, w, H, W, alpha, vec;
};

struct __attribute__((aligned(4))) HoBytes12 {
  uint32_t a, b, c;
};

static size_t ho_smem(int h, int w, int H, int W) {
  return 768 + 64 + ((size_t)W + H) * sizeof(int) + (((size_t)h * w + 3) & ~(size_t)3);
}

// source cell and 11-bit weight of output coordinate X on an axis resized n -> N (half-pixel centres), packed as
// (x0 + 1) << 12 | c1 with x0 in [-1, n - 1] still unclamped
__device__ __forceinline__ int ho_axis(int X, int n, int N) {
  const long long num = (long long)(2 * X + 1) * n - N, den = 2LL * N;
  long long x0 = num / den;
  if (num - x0 * den < 0) --x0;                      // floor
  const long long rem = num - x0 * den;
  const int c1 = (int)((rem * 2048 + N) / den);
  return (int)((x0 + 1) << 12) | c1;
}

// grid (M = T*C maps, bands of HO_BLOCK * HO_PIX * HO_ITERS pixels)
__global__ __launch_bounds__(HO_BLOCK) void heatmap_overlay_kernel(HoArgs a, uint8_t* __restrict__ out) {
  extern __shared__ int sm_i[];
  const int m = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int t = m / a.C, c = m - t * a.C, h = a.h, w = a.w, H = a.H, W = a.W, hw = h * w;
  uint8_t* s_tab = (uint8_t*)sm_i;                   // [768]
  float* s_red = (float*)(sm_i + 192);               // [16]
  int* s_x = sm_i + 208;                             // [W]
  int* s_y = s_x + W;                                // [H]
  uint8_t* s_q = (uint8_t*)(s_y + H);                // [h*w] levels of the map's cells
  const float* mp = a.maps + (long long)m * hw;

  for (int i = tid; i < 768; i += HO_BLOCK) s_tab[i] = a.table[i];
  for (int i = tid; i < W; i += HO_BLOCK) s_x[i] = ho_axis(i, w, W);
  for (int i = tid; i < H; i += HO_BLOCK) s_y[i] = ho_axis(i, h, H);
  float mn = INFINITY, mx = -INFINITY;
  for (int i = tid; i < hw; i += HO_BLOCK) {
    const float v = mp[i];
    mn = fminf(mn, v);
    mx = fmaxf(mx, v);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mn = fminf(mn, __shfl_xor(mn, o, 64));
    mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  }
  if (lane == 0) { s_red[wave] = mn; s_red[4 + wave] = mx; }
  __syncthreads();
  mn = fminf(fminf(s_red[0], s_red[1]), fminf(s_red[2], s_red[3]));
  mx = fmaxf(fmaxf(s_red[4], s_red[5]), fmaxf(s_red[6], s_red[7]));
  const float range = mx - mn;
  for (int i = tid; i < hw; i += HO_BLOCK) {
    // fp32, this order, IEEE division: (255 * (m - mn)) / (mx - mn), truncated.  A constant map is level 0.
    const float num = 255.0f * (mp[i] - mn);
    s_q[i] = range > 0.f ? (uint8_t)(int)(num / range) : (uint8_t)0;
  }
  __syncthreads();

  const long long HWp = (long long)H * W;
  const float* fr = a.fr[c] + (long long)t * 3 * HWp;
  uint8_t* op = out + ((long long)c * a.T + t) * HWp * 3;
  const int al = a.alpha, be = 256 - a.alpha;
  const float mean[3] = {0.485f, 0.456f, 0.406f}, sd[3] = {0.229f, 0.224f, 0.225f};
  for (int it = 0; it < HO_ITERS; ++it) {
    const long long p0 = (((long long)blockIdx.y * HO_ITERS + it) * HO_BLOCK + tid) * HO_PIX;
    if (p0 >= HWp) break;
    const int n = (int)min((long long)HO_PIX, HWp - p0);
    const bool whole = a.vec && n == HO_PIX;
    float px[3][HO_PIX];
    if (whole) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const f32x4 v = *(const f32x4*)(fr + ch * HWp + p0);
        px[ch][0] = v.x; px[ch][1] = v.y; px[ch][2] = v.z; px[ch][3] = v.w;
      }
    } else {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch)
#pragma unroll
        for (int j = 0; j < HO_PIX; ++j) px[ch][j] = j < n ? fr[ch * HWp + p0 + j] : 0.f;
    }
    int y = (int)(p0 / W), x = (int)(p0 - (long long)y * W);
    uint8_t bytes[3 * HO_PIX];
#pragma unroll
    for (int j = 0; j < HO_PIX; ++j) {
      const int ex = s_x[min(x, W - 1)], ey = s_y[min(y, H - 1)];
      const int cx1 = ex & 0xfff, cx0 = 2048 - cx1, cy1 = ey & 0xfff, cy0 = 2048 - cy1;
      const int xa = (ex >> 12) - 1, ya = (ey >> 12) - 1;
      const int x0 = max(xa, 0), x1 = min(xa + 1, w - 1), y0 = max(ya, 0), y1 = min(ya + 1, h - 1);
      const int q00 = s_q[y0 * w + x0], q01 = s_q[y0 * w + x1], q10 = s_q[y1 * w + x0], q11 = s_q[y1 * w + x1];
      const int level = (q00 * cx0 * cy0 + q01 * cx1 * cy0 + q10 * cx0 * cy1 + q11 * cx1 * cy1 + (1 << 21)) >> 22;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        // the frame pixel back on 0..255: rounded, clamped (deliberately not the reference's truncate-and-wrap)
        const float f = floorf((px[ch][j] * sd[ch] + mean[ch]) * 255.0f + 0.5f);
        const int p = (int)fminf(fmaxf(f, 0.f), 255.f);
        bytes[j * 3 + ch] = (uint8_t)((s_tab[level * 3 + ch] * al + p * be + 128) >> 8);
      }
      if (++x == W) { x = 0; ++y; }
    }
    if (whole) {
      HoBytes12 o;
      o.a = bytes[0] | bytes[1] << 8 | bytes[2] << 16 | (uint32_t)bytes[3] << 24;
      o.b = bytes[4] | bytes[5] << 8 | bytes[6] << 16 | (uint32_t)bytes[7] << 24;
      o.c = bytes[8] | bytes[9] << 8 | bytes[10] << 16 | (uint32_t)bytes[11] << 24;
      *(HoBytes12*)(op + p0 * 3) = o;
    } else {
      for (int j = 0; j < 3 * n; ++j) op[p0 * 3 + j] = bytes[j];
    }
  }
}

extern "C" int avsep_heatmap_overlay(const float* maps, const float* const* frames, const uint8_t* table, int32_t T, int32_t C,
                                     int32_t h, int32_t w, int32_t H, int32_t W, int32_t alpha256, uint8_t* out,
                                     avsep_stream_t stream) {
  if (!maps || !frames || !table || !out) return AVSEP_ERR_ARG;
  if (T <= 0 || C < 1 || C > LM_MAXC || h <= 0 || w <= 0 || H <= 0 || W <= 0 || alpha256 < 0 || alpha256 > 256) return AVSEP_ERR_ARG;
  if (h > 65535 || w > 65535 || H > 65535 || W > 65535) return AVSEP_ERR_ARG;
  const size_t smem = ho_smem(h, w, H, W);
  if (smem > 64 * 1024) return AVSEP_ERR_ARG;
  const long long HWp = (long long)H * W, bands = (HWp + HO_BLOCK * HO_PIX * HO_ITERS - 1) / (HO_BLOCK * HO_PIX * HO_ITERS);
  if (bands > 65535) return AVSEP_ERR_ARG;
  HoArgs a{};
  a.maps = maps; a.table = table; a.T = T; a.C = C; a.h = h; a.w = w; a.H = H; a.W = W; a.alpha = alpha256;
  // whole-dword stores and 16-byte frame loads need every image to start on such a boundary
  a.vec = HWp % 4 == 0 && (uintptr_t)out % 4 == 0;
  for (int c = 0; c < C; ++c) {
    if (!frames[c]) return AVSEP_ERR_ARG;
    a.fr[c] = frames[c];
    if ((uintptr_t)frames[c] % 16 != 0) a.vec = 0;
  }
  hipLaunchKernelGGL(heatmap_overlay_kernel, dim3((unsigned)T * C, (unsigned)bands), dim3(HO_BLOCK), smem, (hipStream_t)stream, a, out);
  AVSEP_LAUNCH_CHECK();
  return AVSEP_OK;
}
