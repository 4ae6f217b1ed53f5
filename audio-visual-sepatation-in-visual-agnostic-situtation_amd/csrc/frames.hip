// Frames as shot (include/avsep.h): uint8 RGB frames [T,H,W,3] -> the float32 [T,3,S,S] the visual trunk is trained on,
// bit for bit what dataset.VideoTransform gives: Pillow's 8-bit bicubic resize, crop (zero outside the resized image), flip,
// ImageNet normalisation.  Every floating-point decision is taken on the host (avsep_amd/frames.py): the two fixed-point
// coefficient tables, one per axis, and the 256 x 3 table of normalised values.  The kernel adds products of int32 and looks
// values up; it divides nothing and rounds nothing but by an arithmetic shift.
//
// ONE fused kernel, not a horizontal and a vertical launch: the image between the passes is uint8 and a tile of it is small
// (a workgroup's 32 cropped columns x the input rows its output rows reach x 3 bytes, at most FP_MID_ROWS rows = 24 KiB), so it
// lives in LDS and never travels to HBM and back; two launches would add (H' x S x 3) bytes written and read per frame,
// half as much again for a 360-line frame (0.48 MB on the 1.0 MB it needs), and a workspace that grows with T.  LDS is dynamic and sized by the launcher for
// the frame size at hand (21 KiB for 360 x 640 -> 224, seven workgroups per CU; 53 KiB at the limits): the kernel waits on
// LDS reads, and resident wavefronts are what hides them.
// A workgroup owns FP_TC cropped columns x TR cropped rows of one frame (TR = the largest power of two <= 32 whose input rows
// fit the tile; 32 for any frame of up to ~7 times S).  Only those columns and only the input rows those output rows reach get
// the horizontal pass:
//   1. the input rows are staged in chunks: an RGB row starts at any byte, so a lane never loads bytes from HBM; the
//      workgroup loads the 16-byte aligned quads that cover the row's span (one global_load_dwordx4 per lane) and keeps the
//      row's misalignment as an offset into the staged bytes.  A quad that hangs over either end of the buffer is read byte
//      by byte, and only the bytes inside.
//   2. horizontal pass out of LDS (byte reads) with the tile's coefficient rows in LDS -> the uint8 tile;
//   3. vertical pass out of the uint8 tile with the rows' coefficients in LDS, then crop / flip / table look-up and plain
//      stores: lanes run along the output row, a wavefront writes two 128-byte segments per channel.
// The tables come from device memory and are not trusted with addresses: every (first, count) pair is clamped to the input and
// to what was staged, so a wrong table gives wrong pixels, never an access outside the buffers.
// The tile's work is one device function, fp_tile, under two kernels: frames of one size with the geometry in the kernel
// arguments (avsep_frames_prepare), and frames of many sizes, each with its own crop and flip, with the geometry in a row per
// frame of a table in device memory (avsep_frames_prepare_batch: the training loader's B x N clips in one launch).  What a
// geometry asks of a launch is decided in fp_plan_frame, on the host, for both.
#include "common.h"

constexpr int FP_BLOCK = 256;
constexpr int FP_TC = 32;                        // cropped columns per workgroup
constexpr int FP_TR = 32;                        // cropped rows per workgroup, at most
constexpr int FP_MAX_K = 81;                     // taps per output: a downscale of up to 20 (support 2 * 20 to either side, + 1)
constexpr int FP_MAX_SIDE = 4096;
constexpr int FP_MIN_S = 8, FP_MAX_S = 1024;
constexpr int FP_MID_ROWS = 256;                 // rows of the uint8 tile between the passes, at most
constexpr int FP_MID_PITCH = FP_TC * 3;
constexpr int FP_IN_BYTES = 16384;               // staged input rows per chunk, at most
constexpr int FP_BITS = 22;                      // Pillow's PRECISION_BITS for 8-bit images

struct FpAxis {                                  // one resize axis: n_in -> n_out with k taps per output
  const int32_t* __restrict__ coef;              // [n_out][k]
  const int32_t* __restrict__ bound;             // [n_out][2] = (first input index, count)
  int n_in, n_out, k;
};

__device__ __forceinline__ int fp_clamp(int v, int lo, int hi) { return min(max(v, lo), hi); }
__device__ __forceinline__ int fp_clip8(int acc) { return fp_clamp(acc >> FP_BITS, 0, 255); }

// One workgroup's work, whichever kernel it runs in: the tile (blockIdx.x, blockIdx.y) of the frame whose first byte is
// frames[base] and whose channel 0 starts at out[0] (channels `plane` floats apart; out_u8 likewise the frame's own, or null).
// The launcher's bounds: max_cols, the input columns a tile's columns reach, and the three sizes of the dynamic LDS: in_bytes
// of staged rows (a multiple of 16, at least one row of max_cols), mid_rows rows of the uint8 tile, and FP_TC * kmax
// coefficients (kmax = the larger tap count).
__device__ __forceinline__ void fp_tile(const uint8_t* __restrict__ frames, long long total, long long base, const FpAxis hx,
                                        const FpAxis vy, int S, int ci, int cj, int flip, int TR, int max_cols, int in_bytes,
                                        int mid_rows, int kmax, const float* __restrict__ lut, float* __restrict__ out,
                                        long long plane, uint8_t* __restrict__ out_u8) {
  extern __shared__ uint4 s_in[];                // every part below starts at a multiple of 16 bytes
  uint8_t* s_mid = (uint8_t*)s_in + in_bytes;
  int32_t* s_k = (int32_t*)(s_mid + mid_rows * FP_MID_PITCH);      // the tile's horizontal coefficient rows, later its vertical ones (FP_TR == FP_TC)
  float* s_lut = (float*)(s_k + FP_TC * kmax);
  const int tid = threadIdx.x, lx = tid & (FP_TC - 1), ly = tid / FP_TC;
  const int cx0 = blockIdx.x * FP_TC, cy0 = blockIdx.y * TR;
  const int H = vy.n_in, W = hx.n_in, h = vy.n_out, w = hx.n_out;
  for (int e = tid; e < 256 * 3; e += FP_BLOCK) s_lut[e] = lut[e];
  // the part of the tile that lies inside the resized image: columns [xa, xb), rows [ya, yb) of it
  const int xa = max(cx0 + cj, 0), xb = min(min(cx0 + FP_TC, S) + cj, w);
  const int ya = max(cy0 + ci, 0), yb = min(min(cy0 + TR, S) + ci, h);
  const bool any = xa < xb && ya < yb;           // the same for the whole workgroup: the barriers below are safe
  int rlo = 0, nrows = 0;
  if (any) {
    // input rows [rlo, rlo + nrows) and columns [clo, clo + ncols) the tile reaches (both bounds ascend with the output index)
    rlo = fp_clamp(vy.bound[2 * ya], 0, H);
    nrows = min(fp_clamp(vy.bound[2 * (yb - 1)] + vy.bound[2 * (yb - 1) + 1], rlo, H) - rlo, mid_rows);
    const int clo = fp_clamp(hx.bound[2 * xa], 0, W);
    const int ncols = min(fp_clamp(hx.bound[2 * (xb - 1)] + hx.bound[2 * (xb - 1) + 1], clo, W) - clo, max_cols);
    const int pitch = (ncols * 3 + 15 + 15) / 16 * 16;                         // a row's span at any misalignment, in whole quads
    const int chunk = in_bytes / pitch;                                         // >= 1: the launcher sized in_bytes from max_cols
    // this lane's column of the resized image, its taps and its coefficient row
    const int x = cx0 + lx + cj;
    const bool col = cx0 + lx < S && x >= 0 && x < w;
    int x0 = 0, xn = 0;
    if (col) {
      x0 = fp_clamp(hx.bound[2 * x], clo, clo + ncols);
      xn = fp_clamp(hx.bound[2 * x + 1], 0, min(hx.k, clo + ncols - x0));
    }
    for (int e = tid; e < FP_TC * hx.k; e += FP_BLOCK) {
      const int c = e / hx.k, xe = cx0 + c + cj;
      s_k[e] = (cx0 + c < S && xe >= 0 && xe < w) ? hx.coef[(long long)xe * hx.k + (e - c * hx.k)] : 0;
    }
    const size_t addr0 = (size_t)frames;
    for (int r0 = 0; r0 < nrows; r0 += chunk) {
      const int nr = min(chunk, nrows - r0);
      __syncthreads();                           // the previous chunk's reads are done (first round: s_k and s_lut are written)
      const int quads = pitch / 16;
      for (int e = tid; e < nr * quads; e += FP_BLOCK) {
        const int r = e / quads, q = e - r * quads;
        const long long off = base + ((long long)(rlo + r0 + r) * W + clo) * 3;          // the row's first byte, from `frames`
        const int mis = (int)((addr0 + (size_t)off) & 15);
        if (16 * q >= mis + ncols * 3) continue;                                // past the row's span
        const long long g = off - mis + 16 * q;                                 // 16-byte aligned address
        uint4 v;
        if (g >= 0 && g + 16 <= total) {
          v = *(const uint4*)(frames + g);
        } else {                                 // the quad hangs over an end of the buffer: only what lies inside is read
          uint32_t p[4] = {0u, 0u, 0u, 0u};
          for (int b = 0; b < 16; ++b)
            if (g + b >= 0 && g + b < total) p[b >> 2] |= (uint32_t)frames[g + b] << (8 * (b & 3));
          v = make_uint4(p[0], p[1], p[2], p[3]);
        }
        s_in[(r * pitch) / 16 + q] = v;
      }
      __syncthreads();
      if (col) {
        const uint8_t* bytes = (const uint8_t*)s_in;
        for (int r = ly; r < nr; r += FP_BLOCK / FP_TC) {
          const long long off = base + ((long long)(rlo + r0 + r) * W + clo) * 3;
          const uint8_t* p = bytes + r * pitch + (int)((addr0 + (size_t)off) & 15) + (x0 - clo) * 3;
          int a0 = 1 << (FP_BITS - 1), a1 = a0, a2 = a0;
#pragma unroll 4
          for (int k = 0; k < xn; ++k) {
            const int c = s_k[lx * hx.k + k];
            a0 += c * (int)p[3 * k], a1 += c * (int)p[3 * k + 1], a2 += c * (int)p[3 * k + 2];
          }
          uint8_t* m = s_mid + (r0 + r) * FP_MID_PITCH + lx * 3;
          m[0] = (uint8_t)fp_clip8(a0), m[1] = (uint8_t)fp_clip8(a1), m[2] = (uint8_t)fp_clip8(a2);
        }
      }
    }
    __syncthreads();                             // the uint8 tile is whole; s_k is free
    for (int e = tid; e < TR * vy.k; e += FP_BLOCK) {
      const int r = e / vy.k, ye = cy0 + r + ci;
      s_k[e] = (cy0 + r < S && ye >= 0 && ye < h) ? vy.coef[(long long)ye * vy.k + (e - r * vy.k)] : 0;
    }
  }
  __syncthreads();
  const int cx = cx0 + lx, x = cx + cj;
  if (cx >= S) return;
  const int ox = flip ? S - 1 - cx : cx;
  for (int r = ly; r < TR; r += FP_BLOCK / FP_TC) {
    const int cy = cy0 + r, y = cy + ci;
    if (cy >= S) break;
    int v0 = 0, v1 = 0, v2 = 0;                  // outside the resized image: black
    if (any && x >= 0 && x < w && y >= 0 && y < h) {
      const int y0 = fp_clamp(vy.bound[2 * y], rlo, rlo + nrows);
      const int yn = fp_clamp(vy.bound[2 * y + 1], 0, min(vy.k, rlo + nrows - y0));
      const uint8_t* p = s_mid + (y0 - rlo) * FP_MID_PITCH + lx * 3;
      int a0 = 1 << (FP_BITS - 1), a1 = a0, a2 = a0;
#pragma unroll 4
      for (int k = 0; k < yn; ++k) {
        const int c = s_k[r * vy.k + k];
        a0 += c * (int)p[k * FP_MID_PITCH], a1 += c * (int)p[k * FP_MID_PITCH + 1], a2 += c * (int)p[k * FP_MID_PITCH + 2];
      }
      v0 = fp_clip8(a0), v1 = fp_clip8(a1), v2 = fp_clip8(a2);
    }
    const long long o = (long long)cy * S + ox;
    out[o] = s_lut[v0 * 3], out[o + plane] = s_lut[v1 * 3 + 1], out[o + 2 * plane] = s_lut[v2 * 3 + 2];
    if (out_u8) {
      uint8_t* u = out_u8 + ((long long)cy * S + ox) * 3;
      u[0] = (uint8_t)v0, u[1] = (uint8_t)v1, u[2] = (uint8_t)v2;
    }
  }
}

constexpr int FP_LUT_BYTES = 256 * 3 * 4;
constexpr int FP_LDS_MIN = FP_LUT_BYTES;         // no launch needs less than the look-up table
constexpr int FP_LDS_MAX = FP_IN_BYTES + FP_MID_ROWS * FP_MID_PITCH + FP_TC * FP_MAX_K * 4 + FP_LUT_BYTES;      // 54 400

// Frames of one size, geometry in the kernel arguments: grid (ceil(S / FP_TC), ceil(S / TR), T), frame blockIdx.z of a dense
// stack into out [T][3][S][S].
__global__ __launch_bounds__(FP_BLOCK) void frames_prepare_kernel(const uint8_t* __restrict__ frames, long long total, FpAxis hx,
                                                                  FpAxis vy, int S, int ci, int cj, int flip, int TR, int max_cols,
                                                                  int in_bytes, int mid_rows, int kmax,
                                                                  const float* __restrict__ lut, float* __restrict__ out,
                                                                  uint8_t* __restrict__ out_u8) {
  const long long t = blockIdx.z, plane = (long long)S * S;
  fp_tile(frames, total, t * vy.n_in * hx.n_in * 3, hx, vy, S, ci, cj, flip, TR, max_cols, in_bytes, mid_rows, kmax, lut,
          out + t * 3 * plane, plane, out_u8 ? out_u8 + t * plane * 3 : nullptr);
}

// Frames of many sizes, geometry in row blockIdx.z of a table in device memory: grid (ceil(S / FP_TC), ceil(S / TR_min), n) and
// the LDS of the frame that needs most.  The row is not trusted with addresses: sizes are clamped to the limits, and a row
// whose tables, output or LDS need do not fit what the launch was given leaves its output untouched.  Every test below is on
// values the whole workgroup shares, and all of them come before the first barrier.
__global__ __launch_bounds__(FP_BLOCK) void frames_prepare_batch_kernel(const uint8_t* __restrict__ pixels, long long total,
                                                                        const avsep_frames_row* __restrict__ rows,
                                                                        const int32_t* __restrict__ tables, long long table_words,
                                                                        int S, int lds_bytes, const float* __restrict__ lut,
                                                                        float* __restrict__ out, long long out_floats,
                                                                        long long plane) {
  const avsep_frames_row r = rows[blockIdx.z];
  const int TR = fp_clamp(r.TR, 1, FP_TR);
  if ((long long)blockIdx.y * TR >= S) return;   // a frame of taller tiles than the batch's smallest: its rows are done
  const int H = fp_clamp(r.H, 1, FP_MAX_SIDE), W = fp_clamp(r.W, 1, FP_MAX_SIDE);
  const int h = fp_clamp(r.h, 1, FP_MAX_SIDE), w = fp_clamp(r.w, 1, FP_MAX_SIDE);
  const int kh = fp_clamp(r.kh, 1, FP_MAX_K), kv = fp_clamp(r.kv, 1, FP_MAX_K), kmax = max(kh, kv);
  const int max_cols = r.max_cols, mid_rows = fp_clamp(r.mid_rows, 1, FP_MID_ROWS);
  const int in_bytes = fp_clamp(r.in_bytes, 0, FP_IN_BYTES) & ~15;
  if (max_cols < 1 || max_cols > W) return;                                    // columns the frame does not have
  if ((max_cols * 3 + 30) / 16 * 16 > in_bytes) return;                        // not one staged row of the widest tile
  if (in_bytes + mid_rows * FP_MID_PITCH + FP_TC * kmax * 4 + FP_LUT_BYTES > lds_bytes) return;
  const long long hc = r.hcoef, hb = r.hbound, vc = r.vcoef, vb = r.vbound, oo = r.out_off;
  if (hc < 0 || hc > table_words - (long long)w * kh || hb < 0 || hb > table_words - 2LL * w || vc < 0 ||
      vc > table_words - (long long)h * kv || vb < 0 || vb > table_words - 2LL * h)
    return;
  if (oo < 0 || oo > out_floats - (2 * plane + (long long)S * S)) return;
  const long long base = min(max((long long)r.pix_off, 0LL), total);          // what lies past `total` is never read
  const FpAxis hx = {tables + hc, tables + hb, W, w, kh}, vy = {tables + vc, tables + vb, H, h, kv};
  fp_tile(pixels, total, base, hx, vy, S, fp_clamp(r.crop_i, -FP_MAX_SIDE, FP_MAX_SIDE), fp_clamp(r.crop_j, -FP_MAX_SIDE, FP_MAX_SIDE),
          r.flip & 1, TR, max_cols, in_bytes, mid_rows, kmax, lut, out + oo, plane, nullptr);
}

// Pillow's taps per output for n_in -> n_out: support 2 * max(n_in / n_out, 1) to either side; 0 when not a size
static int fp_ksize(int n_in, int n_out, double* reach) {
  if (n_in < 1 || n_out < 1) return 0;
  const double scale = (double)n_in / (double)n_out, support = 2.0 * (scale < 1.0 ? 1.0 : scale);
  *reach = support;
  return (int)ceil(support) * 2 + 1;
}

// the input positions n consecutive outputs reach, at most: their centres span (n - 1) * scale, the taps reach `support` to
// either side, and each end is rounded once
static int fp_span(int n_in, int n_out, int n, double support) {
  return (int)ceil((n - 1) * ((double)n_in / (double)n_out) + 2.0 * support) + 2;
}

// What one frame's geometry asks of a launch: the one place that decides it, for the single form and for every row of a batch.
struct FpSizing {
  int TR, max_cols, in_bytes, mid_rows, kmax, lds;
};

// The limits of one frame's geometry (sides, S, the tap counts the sizes imply, crop, flip) and its launch sizing; false = refused.
static bool fp_plan_frame(int H, int W, int w, int h, int kh, int kv, int S, int crop_i, int crop_j, int flip, FpSizing* z) {
  if (H < 1 || H > FP_MAX_SIDE || W < 1 || W > FP_MAX_SIDE || w < 1 || w > FP_MAX_SIDE || h < 1 || h > FP_MAX_SIDE ||
      S < FP_MIN_S || S > FP_MAX_S || (flip != 0 && flip != 1))
    return false;
  if (crop_i < -FP_MAX_SIDE || crop_i > FP_MAX_SIDE || crop_j < -FP_MAX_SIDE || crop_j > FP_MAX_SIDE) return false;
  double hreach = 0.0, vreach = 0.0;
  if (kh != fp_ksize(W, w, &hreach) || kv != fp_ksize(H, h, &vreach) || kh > FP_MAX_K || kv > FP_MAX_K) return false;
  z->max_cols = min(fp_span(W, w, FP_TC, hreach), W);
  const int pitch = (z->max_cols * 3 + 30) / 16 * 16;                          // the kernel's, for the widest tile
  if (pitch > FP_IN_BYTES) return false;                                       // cannot happen under FP_MAX_K: kept as the kernel's premise
  z->TR = FP_TR;
  while (z->TR > 1 && min(fp_span(H, h, z->TR, vreach), H) > FP_MID_ROWS) z->TR >>= 1;
  z->mid_rows = min(fp_span(H, h, z->TR, vreach), H);
  if (z->mid_rows > FP_MID_ROWS) return false;                                 // likewise
  z->in_bytes = min(z->mid_rows * pitch, FP_IN_BYTES / pitch * pitch);         // all rows at once where they fit
  z->kmax = max(kh, kv);
  z->lds = z->in_bytes + z->mid_rows * FP_MID_PITCH + FP_TC * z->kmax * 4 + FP_LUT_BYTES;          // <= FP_LDS_MAX
  return true;
}

extern "C" int avsep_frames_prepare(const uint8_t* frames, int32_t T, int32_t H, int32_t W, const int32_t* hcoef, const int32_t* hbound,
                                    int32_t w, int32_t kh, const int32_t* vcoef, const int32_t* vbound, int32_t h, int32_t kv,
                                    int32_t S, int32_t crop_i, int32_t crop_j, int32_t flip, const float* lut, float* out,
                                    uint8_t* out_u8, avsep_stream_t stream) {
  if (!frames || !hcoef || !hbound || !vcoef || !vbound || !lut || !out) return AVSEP_ERR_ARG;
  FpSizing z;
  if (T < 1 || T > 65535 || !fp_plan_frame(H, W, w, h, kh, kv, S, crop_i, crop_j, flip, &z)) return AVSEP_ERR_ARG;
  const FpAxis hx = {hcoef, hbound, W, w, kh}, vy = {vcoef, vbound, H, h, kv};
  hipLaunchKernelGGL(frames_prepare_kernel, dim3(cdiv(S, FP_TC), cdiv(S, z.TR), T), dim3(FP_BLOCK), (size_t)z.lds, (hipStream_t)stream,
                     frames, (long long)T * H * W * 3, hx, vy, S, crop_i, crop_j, flip, z.TR, z.max_cols, z.in_bytes, z.mid_rows,
                     z.kmax, lut, out, out_u8);
  AVSEP_LAUNCH_CHECK();
  return AVSEP_OK;
}

// [off, off + len) inside [0, size), without forming off + len
static bool fp_inside(long long off, long long len, long long size) { return off >= 0 && len >= 0 && len <= size && off <= size - len; }

extern "C" int avsep_frames_batch_plan(avsep_frames_row* rows, int32_t n, int32_t S, int64_t pixel_bytes, int64_t table_words,
                                       int64_t out_floats, int64_t plane, int32_t* launch) {
  if (!rows || !launch || n < 1 || n > 65535 || S < FP_MIN_S || S > FP_MAX_S || pixel_bytes < 1 || table_words < 1) return AVSEP_ERR_ARG;
  const long long SS = (long long)S * S;
  if (plane < SS || plane > (1LL << 40) || out_floats < 1) return AVSEP_ERR_ARG;
  int tr_min = FP_TR, lds = 0;
  for (int i = 0; i < n; ++i) {
    avsep_frames_row& r = rows[i];
    FpSizing z;
    if (!fp_plan_frame(r.H, r.W, r.w, r.h, r.kh, r.kv, S, r.crop_i, r.crop_j, r.flip, &z)) return AVSEP_ERR_ARG;
    if (!fp_inside(r.pix_off, (long long)r.H * r.W * 3, pixel_bytes) || !fp_inside(r.out_off, 2 * plane + SS, out_floats))
      return AVSEP_ERR_ARG;
    if (!fp_inside(r.hcoef, (long long)r.w * r.kh, table_words) || !fp_inside(r.hbound, 2LL * r.w, table_words) ||
        !fp_inside(r.vcoef, (long long)r.h * r.kv, table_words) || !fp_inside(r.vbound, 2LL * r.h, table_words))
      return AVSEP_ERR_ARG;
    r.TR = z.TR, r.max_cols = z.max_cols, r.in_bytes = z.in_bytes, r.mid_rows = z.mid_rows, r.reserved = 0;
    tr_min = min(tr_min, z.TR), lds = max(lds, z.lds);
  }
  launch[0] = cdiv(S, tr_min), launch[1] = lds, launch[2] = tr_min;
  return AVSEP_OK;
}

extern "C" int avsep_frames_prepare_batch(const uint8_t* pixels, int64_t pixel_bytes, const avsep_frames_row* rows, int32_t n,
                                          const int32_t* tables, int64_t table_words, int32_t S, const float* lut, float* out,
                                          int64_t out_floats, int64_t plane, int32_t grid_y, int32_t lds_bytes,
                                          avsep_stream_t stream) {
  if (!pixels || !rows || !tables || !lut || !out) return AVSEP_ERR_ARG;
  if (n < 1 || n > 65535 || S < FP_MIN_S || S > FP_MAX_S || pixel_bytes < 1 || table_words < 1) return AVSEP_ERR_ARG;
  const long long SS = (long long)S * S;
  if (plane < SS || plane > (1LL << 40) || out_floats < 2 * plane + SS) return AVSEP_ERR_ARG;
  if (grid_y < cdiv(S, FP_TR) || grid_y > S || lds_bytes < FP_LDS_MIN || lds_bytes > FP_LDS_MAX) return AVSEP_ERR_ARG;
  hipLaunchKernelGGL(frames_prepare_batch_kernel, dim3(cdiv(S, FP_TC), grid_y, n), dim3(FP_BLOCK), (size_t)lds_bytes, (hipStream_t)stream,
                     pixels, (long long)pixel_bytes, rows, tables, (long long)table_words, S, lds_bytes, lut, out,
                     (long long)out_floats, (long long)plane);
  AVSEP_LAUNCH_CHECK();
  return AVSEP_OK;
}
