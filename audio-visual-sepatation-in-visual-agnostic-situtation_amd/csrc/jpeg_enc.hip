// uint8 pictures -> the entropy-coded bytes of baseline JPEG files (include/avsep.h has the rule; avsep_amd/jpeg.py: encode), byte
// for byte libjpeg-turbo's default encoder.  Four stages on the caller's stream, every one of them parallel over the blocks,
// bytes or intervals of a whole batch of pictures of mixed sizes and forms:
//   coef   jpeg_enc_coef_kernel     one lane per block: colour, downsampling, islow forward DCT, quantisation -> 64 int16, zig-zag;
//   count  jpeg_enc_count_kernel    one lane per block: its Huffman bits; running sums; jpeg_enc_interval_kernel: an interval's bytes;
//   pack   jpeg_enc_pack_kernel     one lane per block: its bits at their place in a zeroed stream (shared words by atomicOr);
//          jpeg_enc_ff_kernel, jpeg_enc_stuffed_kernel: the 0xFF bytes per 64 bytes and per interval; running sums;
//   stuff  jpeg_enc_stuff_kernel    one lane per 64 bytes: the bytes at their stuffed place; jpeg_enc_marker_kernel: RSTn, EOI, sizes.
// Rows of images live in device memory and are not trusted with addresses: a lane checks the row it reads against the buffer
// sizes it was given, and every store whose address comes from device memory is checked against its buffer.
#include "common.h"
#include "jpeg_parts.h"

constexpr int JE_BLOCK = 256;          // lanes per workgroup, and elements per tile of the running sums
constexpr int JE_MAX_GRID = 4096;      // workgroups per launch; lanes stride over what is left
constexpr int JE_GROUP = 64;           // bytes of the unstuffed stream per lane of the stuffing kernels

static inline int je_grid(long long n) {
  const long long g = (n + JE_BLOCK - 1) / JE_BLOCK;
  return (int)(g < 1 ? 1 : (g > JE_MAX_GRID ? JE_MAX_GRID : g));
}

// the row whose block0 (by_interval: interval0) is the last one <= key; the rows run on in both
__device__ __forceinline__ int je_row_of(const avsep_jpeg_image* __restrict__ images, int n, long long key, bool by_interval) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    const long long v = by_interval ? images[mid].interval0 : images[mid].block0;
    if (v <= key) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// Block b of the workspace: its image's row (checked), and where it stands in it.
struct JeWhere {
  avsep_jpeg_image im;
  long long lb, mcu;                   // block and MCU inside the image
  int i, c, luma, per_mcu;             // block inside the MCU, its component, luma blocks and all blocks of an MCU
};
__device__ __forceinline__ bool je_where(const avsep_jpeg_image* __restrict__ images, int n_images, long long ws_blocks, long long b,
                                         JeWhere& w) {
  w.im = images[je_row_of(images, n_images, b, false)];
  long long nblocks = 0, nintervals = 0;
  if (!jp_image_ok(w.im, &nblocks, &nintervals) || !jp_inside(w.im.block0, nblocks, ws_blocks)) return false;
  w.lb = b - w.im.block0;
  if (w.lb < 0 || w.lb >= nblocks) return false;
  w.luma = w.im.hs * w.im.vs, w.per_mcu = w.luma + w.im.ncomp - 1;
  w.mcu = w.lb / w.per_mcu;
  w.i = (int)(w.lb - w.mcu * w.per_mcu);
  w.c = w.i < w.luma ? 0 : w.i - w.luma + 1;
  return true;
}

// sample (y, x) of component c's plane, downsampled: source coordinates clamped to the picture, and rows below the downsampled
// plane repeat its last row (include/avsep.h: edges)
__device__ __forceinline__ int je_sample(const uint8_t* __restrict__ px, const avsep_jpeg_image& im, int c, int y, int x) {
  if (im.ncomp == 1) return px[(long long)min(y, im.H - 1) * im.W + min(x, im.W - 1)];
  if (c == 0) {
    const uint8_t* p = px + ((long long)min(y, im.H - 1) * im.W + min(x, im.W - 1)) * 3;
    return (19595 * p[0] + 38470 * p[1] + 7471 * p[2] + 32768) >> 16;
  }
  y = min(y, (im.H + im.vs - 1) / im.vs - 1);               // below the plane: its last DOWNSAMPLED row again
  int sum = 0;
  for (int dy = 0; dy < im.vs; ++dy)
    for (int dx = 0; dx < im.hs; ++dx) {
      const uint8_t* p = px + ((long long)min(y * im.vs + dy, im.H - 1) * im.W + min(x * im.hs + dx, im.W - 1)) * 3;
      const int R = p[0], G = p[1], B = p[2];
      sum += c == 1 ? (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16
                    : (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16;
    }
  if (im.hs == 1) return sum;
  return im.vs == 1 ? (sum + (x & 1)) >> 1 : (sum + 1 + (x & 1)) >> 2;
}

// lane = one block: grid-strided over the workspace
__global__ __launch_bounds__(JE_BLOCK) void jpeg_enc_coef_kernel(const uint8_t* __restrict__ pixels, long long pixel_bytes,
                                                                 const avsep_jpeg_image* __restrict__ images, int n_images,
                                                                 const int32_t* __restrict__ tables, long long table_words,
                                                                 int16_t* __restrict__ coef, long long ws_blocks) {
  for (long long b = (long long)blockIdx.x * JE_BLOCK + threadIdx.x; b < ws_blocks; b += (long long)gridDim.x * JE_BLOCK) {
    JeWhere w;
    if (!je_where(images, n_images, ws_blocks, b, w)) continue;
    const avsep_jpeg_image& im = w.im;
    if (!jp_inside(im.pix_off, (long long)im.H * im.W * im.ncomp, pixel_bytes)) continue;
    const int qoff = w.c == 0 ? im.quant[0] : (w.c == 1 ? im.quant[1] : im.quant[2]);
    if (!jp_inside(qoff, JP_QUANT_WORDS, table_words)) continue;
    const int32_t* __restrict__ q = tables + qoff;
    const long long my = w.mcu / im.mcux;
    const int mx = (int)(w.mcu - my * im.mcux);
    // a luma block beyond the component's blocks is a dummy: the DC of the last real block before it in the MCU, no AC
    int by = (int)my, bx = mx, i = w.i;
    bool dummy = false;
    if (w.c == 0) {
      const int hb = (im.H + 7) >> 3, wb = (im.W + 7) >> 3;
      for (;; --i) {                                                          // block 0 of an MCU is always real
        by = (int)my * im.vs + i / im.hs, bx = mx * im.hs + i % im.hs;
        if ((by < hb && bx < wb) || i == 0) break;
        dummy = true;
      }
    }
    const uint8_t* __restrict__ px = pixels + im.pix_off;
    int d[64];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      int v[8];
#pragma unroll
      for (int x = 0; x < 8; ++x) v[x] = je_sample(px, im, w.c, by * 8 + r, bx * 8 + x) - 128;
      jp_fdct_1d(v, false);
#pragma unroll
      for (int x = 0; x < 8; ++x) d[r * 8 + x] = v[x];
    }
#pragma unroll
    for (int x = 0; x < 8; ++x) {
      int v[8];
#pragma unroll
      for (int r = 0; r < 8; ++r) v[r] = d[r * 8 + x];
      jp_fdct_1d(v, true);
#pragma unroll
      for (int r = 0; r < 8; ++r) d[r * 8 + x] = v[r];
    }
    uint4* __restrict__ dst = (uint4*)(coef + b * 64);                         // 128 bytes per block: aligned
#pragma unroll
    for (int g = 0; g < 8; ++g) {
      uint32_t u[4];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int k = g * 8 + j, nat = jp_natural(k);
        const uint32_t qv = 8u * (uint32_t)min(max(q[nat], 1), 255);
        const int a = d[nat];
        const int m = (int)(((uint32_t)abs(a) + (qv >> 1)) / qv);
        const uint32_t h = (dummy && k > 0) ? 0u : (uint32_t)(uint16_t)(int16_t)(a < 0 ? -m : m);
        if (j & 1) u[j >> 1] |= h << 16;
        else u[j >> 1] = h;
      }
      dst[g] = make_uint4(u[0], u[1], u[2], u[3]);
    }
  }
}

// The symbols of one block, handed to `put(code, length)` in stream order.  blk: its 64 coefficients; pred: the predictor.
template <class Put>
__device__ __forceinline__ void je_walk(const int16_t* __restrict__ blk, int pred, const int32_t* __restrict__ dct,
                                        const int32_t* __restrict__ act, Put& put) {
  const uint4* __restrict__ src = (const uint4*)blk;
  int run = 0;
  for (int g = 0; g < 8; ++g) {
    const uint4 v = src[g];
    const uint32_t u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      int val = (int)(int16_t)((j & 1) ? u[j >> 1] >> 16 : u[j >> 1] & 0xffffu);
      const bool is_dc = g == 0 && j == 0;
      if (is_dc) val -= pred;
      if (val == 0 && !is_dc) {
        ++run;
        continue;
      }
      const int s = 32 - __clz(abs(val));                                       // 0 for a DC difference of 0
      const uint32_t extra = (uint32_t)(val < 0 ? val + (1 << s) - 1 : val);
      if (is_dc) {
        const int32_t t = dct[s & 255];
        put((uint32_t)t & 0xffffu, (t >> 16) & 31);
      } else {
        const int32_t zrl = act[0xF0];
        for (; run > 15; run -= 16) put((uint32_t)zrl & 0xffffu, (zrl >> 16) & 31);
        const int32_t t = act[((run << 4) | s) & 255];
        put((uint32_t)t & 0xffffu, (t >> 16) & 31);
        run = 0;
      }
      if (s > 0) put(extra, min(s, 16));
    }
  }
  if (run > 0) {
    const int32_t t = act[0];
    put((uint32_t)t & 0xffffu, (t >> 16) & 31);
  }
}

// What a lane needs to code block b: its tables (checked) and its predictor.  first_block: the interval's first block in the
// workspace; last: b is the interval's last block.
struct JeCode {
  const int32_t *dct, *act;
  int pred;
  long long interval, first_block;
  bool last;
};
__device__ __forceinline__ bool je_code(const JeWhere& w, const int32_t* __restrict__ tables, long long table_words,
                                        const int16_t* __restrict__ coef, JeCode& k) {
  const avsep_jpeg_image& im = w.im;
  const int doff = w.c == 0 ? im.dc[0] : (w.c == 1 ? im.dc[1] : im.dc[2]);
  const int aoff = w.c == 0 ? im.ac[0] : (w.c == 1 ? im.ac[1] : im.ac[2]);
  if (!jp_inside(doff, JP_ENC_HUFF_WORDS, table_words) || !jp_inside(aoff, JP_ENC_HUFF_WORDS, table_words)) return false;
  k.dct = tables + doff, k.act = tables + aoff;
  const long long mcus = (long long)im.mcux * im.mcuy, per = im.restart ? im.restart : mcus;
  const long long iv = w.mcu / per, mcu0 = iv * per, mcu1 = min(mcu0 + per, mcus);
  k.interval = im.interval0 + iv;
  k.first_block = im.block0 + mcu0 * w.per_mcu;
  k.last = w.mcu == mcu1 - 1 && w.i == w.per_mcu - 1;
  // the component's block before this one: the one before it in the MCU, else the component's last one of the MCU before
  const bool head = w.c == 0 ? w.i == 0 : true;
  if (head && w.mcu == mcu0) {
    k.pred = 0;
  } else {
    const long long prev = !head ? w.lb - 1 : (w.c == 0 ? w.lb - w.per_mcu + w.luma - 1 : w.lb - w.per_mcu);
    k.pred = coef[(im.block0 + prev) * 64];
  }
  return true;
}

struct JeCount {
  int bits;
  __device__ __forceinline__ void operator()(uint32_t, int len) { bits += len; }
};

__global__ __launch_bounds__(JE_BLOCK) void jpeg_enc_count_kernel(const int16_t* __restrict__ coef, long long ws_blocks,
                                                                  const avsep_jpeg_image* __restrict__ images, int n_images,
                                                                  const int32_t* __restrict__ tables, long long table_words,
                                                                  int32_t* __restrict__ bits) {
  for (long long b = (long long)blockIdx.x * JE_BLOCK + threadIdx.x; b < ws_blocks; b += (long long)gridDim.x * JE_BLOCK) {
    JeWhere w;
    JeCode k;
    JeCount n = {0};
    if (je_where(images, n_images, ws_blocks, b, w) && je_code(w, tables, table_words, coef, k)) je_walk(coef + b * 64, k.pred, k.dct, k.act, n);
    bits[b] = n.bits;
  }
}

// ---- running sums: out[i] = in[0] + .. + in[i-1] for i = 0 .. n (int64), in tiles of JE_BLOCK elements
__device__ __forceinline__ long long je_block_exscan(long long v, long long* sh, long long* total) {
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int d = 1; d < JE_BLOCK; d <<= 1) {
    const long long a = t >= d ? sh[t - d] : 0;
    __syncthreads();
    sh[t] += a;
    __syncthreads();
  }
  *total = sh[JE_BLOCK - 1];
  const long long before = sh[t] - v;
  __syncthreads();
  return before;
}
__global__ __launch_bounds__(JE_BLOCK) void jpeg_enc_tile_sum_kernel(const int32_t* __restrict__ in, long long n, long long* __restrict__ tiles,
                                                                     long long ntiles) {
  __shared__ long long sh[JE_BLOCK];
  for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const long long i = t * JE_BLOCK + threadIdx.x;
    long long total;
    je_block_exscan(i < n ? in[i] : 0, sh, &total);
    if (threadIdx.x == 0) tiles[t] = total;
  }
}
// one workgroup: the tiles' sums -> their running sum, JE_BLOCK at a time with a carry; the total goes to *last
__global__ __launch_bounds__(JE_BLOCK) void jpeg_enc_tile_carry_kernel(long long* __restrict__ tiles, long long ntiles, long long* __restrict__ last) {
  __shared__ long long sh[JE_BLOCK];
  long long carry = 0;
  for (long long t0 = 0; t0 < ntiles; t0 += JE_BLOCK) {
    const long long t = t0 + threadIdx.x;
    long long total;
    const long long before = je_block_exscan(t < ntiles ? tiles[t] : 0, sh, &total);
    if (t < ntiles) tiles[t] = carry + before;
    carry += total;
  }
  if (threadIdx.x == 0) *last = carry;
}
__global__ __launch_bounds__(JE_BLOCK) void jpeg_enc_tile_scan_kernel(const int32_t* __restrict__ in, long long n, const long long* __restrict__ tiles,
                                                                      long long ntiles, long long* __restrict__ out) {
  __shared__ long long sh[JE_BLOCK];
  for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const long long i = t * JE_BLOCK + threadIdx.x;
    long long total;
    const long long before = je_block_exscan(i < n ? in[i] : 0, sh, &total);
    if (i < n) out[i] = tiles[t] + before;
  }
}
static int je_running_sum(const int32_t* in, long long n, long long* out, long long* tiles, hipStream_t stream) {
  const long long ntiles = (n + JE_BLOCK - 1) / JE_BLOCK;
  const int grid = (int)(ntiles > JE_MAX_GRID ? JE_MAX_GRID : ntiles);
  hipLaunchKernelGGL(jpeg_enc_tile_sum_kernel, dim3(grid), dim3(JE_BLOCK), 0, stream, in, n, tiles, ntiles);
  AVSEP_LAUNCH_CHECK();
  hipLaunchKernelGGL(jpeg_enc_tile_carry_kernel, dim3(1), dim3(JE_BLOCK), 0, stream, tiles, ntiles, out + n);
  AVSEP_LAUNCH_CHECK();
  hipLaunchKernelGGL(jpeg_enc_tile_scan_kernel, dim3(grid), dim3(JE_BLOCK), 0, stream, in, n, (const long long*)tiles, ntiles, out);
  AVSEP_LAUNCH_CHECK();
  return AVSEP_OK;
}

// Interval k of the batch: its image's row (checked) and its blocks [*b0, *b1) in the workspace; *local: its number in the image,
// *count: the image's intervals, *row: the image.
__device__ __forceinline__ bool je_interval(const avsep_jpeg_image* __restrict__ images, int n_images, long long ws_blocks, long long k,
                                            long long* b0, long long* b1, long long* local, long long* count, int* row) {
  *row = je_row_of(images, n_images, k, true);
  const avsep_jpeg_image im = images[*row];
  long long nblocks = 0;
  if (!jp_image_ok(im, &nblocks, count) || !jp_inside(im.block0, nblocks, ws_blocks)) return false;
  *local = k - im.interval0;
  if (*local < 0 || *local >= *count) return false;
  const long long mcus = (long long)im.mcux * im.mcuy, per = im.restart ? im.restart : mcus;
  const int per_mcu = im.hs * im.vs + im.ncomp - 1;
  *b0 = im.block0 + *local * per * per_mcu;
  *b1 = im.block0 + min((*local + 1) * per, mcus) * per_mcu;
  return true;
}

// lane = one interval: its bytes before stuffing
__global__ __launch_bounds__(JE_BLOCK) void jpeg_enc_interval_kernel(const avsep_jpeg_image* __restrict__ images, int n_images,
                                                                     long long ws_blocks, long long n_intervals,
                                                                     const long long* __restrict__ pos, int32_t* __restrict__ ivl_bytes) {
  for (long long k = (long long)blockIdx.x * JE_BLOCK + threadIdx.x; k < n_intervals; k += (long long)gridDim.x * JE_BLOCK) {
    long long b0, b1, local, count;
    int row;
    long long bytes = 0;
    if (je_interval(images, n_images, ws_blocks, k, &b0, &b1, &local, &count, &row)) bytes = (pos[b1] - pos[b0] + 7) >> 3;
    ivl_bytes[k] = (int32_t)min(max(bytes, 0LL), 0x7fffffffLL);
  }
}

// The bits of one lane, most significant first, into 32-bit words of the byte stream.  A word the lane fills alone is stored;
// the word it starts in the middle of, and the one it ends in the middle of, are ORed into the zeroed stream.
struct JePack {
  uint32_t* words;
  long long w, nwords;
  uint32_t acc;
  int n;                 // bits of `acc` in use, from the top
  bool shared;           // the current word began before this lane's bits
  __device__ __forceinline__ void flush(bool whole) {
    if (w < 0 || w >= nwords) return;
    const uint32_t v = __builtin_bswap32(acc);                                // the stream is bytes: the first bits in the first byte
    if (whole && !shared) words[w] = v;
    else if (v) atomicOr(words + w, v);
  }
  __device__ __forceinline__ void operator()(uint32_t code, int len) {
    if (len < 1) return;
    code &= 0xffffffffu >> (32 - len);
    const int room = 32 - n;
    if (len < room) {
      acc |= code << (room - len), n += len;
    } else {
      acc |= code >> (len - room);
      flush(true);
      ++w, shared = false, n = len - room;
      acc = n ? code << (32 - n) : 0u;
    }
  }
};

__global__ __launch_bounds__(JE_BLOCK) void jpeg_enc_pack_kernel(const int16_t* __restrict__ coef, long long ws_blocks,
                                                                 const avsep_jpeg_image* __restrict__ images, int n_images,
                                                                 long long n_intervals, const int32_t* __restrict__ tables,
                                                                 long long table_words, const long long* __restrict__ pos,
                                                                 const long long* __restrict__ ivl_off, uint32_t* __restrict__ words,
                                                                 long long nwords) {
  for (long long b = (long long)blockIdx.x * JE_BLOCK + threadIdx.x; b < ws_blocks; b += (long long)gridDim.x * JE_BLOCK) {
    JeWhere w;
    JeCode k;
    if (!je_where(images, n_images, ws_blocks, b, w) || !je_code(w, tables, table_words, coef, k)) continue;
    if (k.interval < 0 || k.interval >= n_intervals) continue;
    const long long at = ivl_off[k.interval] * 8 + (pos[b] - pos[k.first_block]);
    if (at < 0) continue;
    JePack p = {words, at >> 5, nwords, 0u, (int)(at & 31), (at & 31) != 0};
    je_walk(coef + b * 64, k.pred, k.dct, k.act, p);
    if (k.last) {
      const int used = (int)((pos[b + 1] - pos[k.first_block]) & 7);
      if (used) p((1u << (8 - used)) - 1u, 8 - used);                          // the interval's last byte: padded with 1-bits
    }
    if (p.n > 0) p.flush(false);
  }
}

__device__ __forceinline__ int je_ff_in_word(uint32_t v) {
  return ((v & 0xffu) == 0xffu) + ((v & 0xff00u) == 0xff00u) + ((v & 0xff0000u) == 0xff0000u) + ((v >> 24) == 0xffu);
}
// lane = 64 bytes of the stream: its 0xFF bytes
__global__ __launch_bounds__(JE_BLOCK) void jpeg_enc_ff_kernel(const uint32_t* __restrict__ words, long long nwords, long long ngroups,
                                                               int32_t* __restrict__ groups) {
  for (long long g = (long long)blockIdx.x * JE_BLOCK + threadIdx.x; g < ngroups; g += (long long)gridDim.x * JE_BLOCK) {
    int n = 0;
    for (int j = 0; j < JE_GROUP / 4; ++j) {
      const long long i = g * (JE_GROUP / 4) + j;
      if (i < nwords) n += je_ff_in_word(words[i]);
    }
    groups[g] = n;
  }
}
// the 0xFF bytes of stream[0 .. at), at <= stream_bytes
__device__ __forceinline__ long long je_ff_before(const uint8_t* __restrict__ stream, long long stream_bytes, const long long* __restrict__ ffpos,
                                                  long long ngroups, long long at) {
  at = min(max(at, 0LL), stream_bytes);
  const long long g = min(at / JE_GROUP, ngroups);
  long long n = ffpos[g];
  for (long long j = g * JE_GROUP; j < at; ++j) n += stream[j] == 0xFF;
  return n;
}
// lane = one interval: the 0xFF bytes before it, and its bytes once stuffed, with its marker
__global__ __launch_bounds__(JE_BLOCK) void jpeg_enc_stuffed_kernel(const uint8_t* __restrict__ stream, long long stream_bytes,
                                                                    long long n_intervals, const long long* __restrict__ ivl_off,
                                                                    const long long* __restrict__ ffpos, long long ngroups,
                                                                    long long* __restrict__ ff0, int32_t* __restrict__ ivl_out) {
  for (long long k = (long long)blockIdx.x * JE_BLOCK + threadIdx.x; k < n_intervals; k += (long long)gridDim.x * JE_BLOCK) {
    const long long a = ivl_off[k], e = ivl_off[k + 1];
    const long long fa = je_ff_before(stream, stream_bytes, ffpos, ngroups, a), fe = je_ff_before(stream, stream_bytes, ffpos, ngroups, e);
    ff0[k] = fa;
    ivl_out[k] = (int32_t)min(max(e - a + fe - fa + 2, 0LL), 0x7fffffffLL);
  }
}

// lane = 64 bytes of the stream: every byte to its place in the output, a 0x00 after every 0xFF
__global__ __launch_bounds__(JE_BLOCK) void jpeg_enc_stuff_kernel(const uint8_t* __restrict__ stream, long long stream_bytes,
                                                                  long long n_intervals, const long long* __restrict__ ivl_off,
                                                                  const long long* __restrict__ ffpos, const long long* __restrict__ ff0,
                                                                  const long long* __restrict__ out_off, uint8_t* __restrict__ out,
                                                                  long long out_bytes) {
  const long long used = min(ivl_off[n_intervals], stream_bytes), ngroups = (used + JE_GROUP - 1) / JE_GROUP;
  for (long long g = (long long)blockIdx.x * JE_BLOCK + threadIdx.x; g < ngroups; g += (long long)gridDim.x * JE_BLOCK) {
    const long long j0 = g * JE_GROUP, j1 = min(j0 + JE_GROUP, used);
    long long lo = 0, hi = n_intervals - 1;                                    // the interval of byte j0: the last one that starts at or before it
    while (lo < hi) {
      const long long mid = (lo + hi + 1) >> 1;
      if (ivl_off[mid] <= j0) lo = mid;
      else hi = mid - 1;
    }
    long long k = lo, next = ivl_off[k + 1], base = out_off[k] - ivl_off[k] - ff0[k], ff = ffpos[g];
    for (long long j = j0; j < j1; ++j) {
      while (j >= next && k + 1 < n_intervals) {
        ++k;
        next = ivl_off[k + 1], base = out_off[k] - ivl_off[k] - ff0[k];
      }
      const uint8_t v = stream[j];
      const long long o = base + j + ff;
      if (o >= 0 && o < out_bytes) out[o] = v;
      if (v == 0xFF) {
        if (o + 1 >= 0 && o + 1 < out_bytes) out[o + 1] = 0;
        ++ff;
      }
    }
  }
}
// lane = one interval: the marker after it, RSTn or EOI; an image's last interval also says where the image lies
__global__ __launch_bounds__(JE_BLOCK) void jpeg_enc_marker_kernel(const avsep_jpeg_image* __restrict__ images, int n_images,
                                                                   long long ws_blocks, long long n_intervals,
                                                                   const long long* __restrict__ out_off, uint8_t* __restrict__ out,
                                                                   long long out_bytes, long long* __restrict__ sizes) {
  for (long long k = (long long)blockIdx.x * JE_BLOCK + threadIdx.x; k < n_intervals; k += (long long)gridDim.x * JE_BLOCK) {
    long long b0, b1, local, count;
    int row;
    if (!je_interval(images, n_images, ws_blocks, k, &b0, &b1, &local, &count, &row)) continue;
    const long long at = out_off[k + 1] - 2;
    const bool last = local == count - 1;
    if (at >= 0 && at + 1 < out_bytes) out[at] = 0xFF, out[at + 1] = last ? 0xD9 : (uint8_t)(0xD0 + (local & 7));
    if (last) {
      const long long first = out_off[k - local];
      sizes[2 * row] = first, sizes[2 * row + 1] = out_off[k + 1] - first;
    }
  }
}

extern "C" int avsep_jpeg_enc_plan_check(const avsep_jpeg_image* images, int32_t n_images, int64_t pixel_bytes, int64_t table_words,
                                         int64_t ws_blocks, int64_t n_intervals) {
  if (!images || n_images < 1 || n_images > (1 << 24) || pixel_bytes < 1 || table_words < 1 || ws_blocks < 1 || ws_blocks > (1LL << 32) ||
      n_intervals < 1)
    return AVSEP_ERR_ARG;
  long long block = 0, interval = 0;
  for (int i = 0; i < n_images; ++i) {
    long long nblocks = 0, nintervals = 0;
    if (!jp_row_ok(images[i], images[i].ncomp, JP_ENC_HUFF_WORDS, pixel_bytes, table_words, &nblocks, &nintervals)) return AVSEP_ERR_ARG;
    if (images[i].block0 != block || images[i].interval0 != interval) return AVSEP_ERR_ARG;
    block += nblocks, interval += nintervals;
  }
  return block == ws_blocks && interval == n_intervals ? AVSEP_OK : AVSEP_ERR_ARG;
}

static bool je_counts_ok(int32_t n_images, int64_t ws_blocks, int64_t n_intervals, int64_t table_words) {
  return n_images >= 1 && n_images <= (1 << 24) && ws_blocks >= 1 && ws_blocks <= (1LL << 32) && n_intervals >= 1 &&
         n_intervals <= ws_blocks && table_words >= 1;
}

extern "C" int avsep_jpeg_enc_coef(const uint8_t* pixels, int64_t pixel_bytes, const avsep_jpeg_image* images, int32_t n_images,
                                   const int32_t* tables, int64_t table_words, int16_t* coef, int64_t ws_blocks, avsep_stream_t stream) {
  if (!pixels || !images || !tables || !coef || pixel_bytes < 1 || !je_counts_ok(n_images, ws_blocks, 1, table_words)) return AVSEP_ERR_ARG;
  if ((uintptr_t)coef % 16) return AVSEP_ERR_ARG;                              // a block is moved as eight 16-byte pieces
  hipLaunchKernelGGL(jpeg_enc_coef_kernel, dim3(je_grid(ws_blocks)), dim3(JE_BLOCK), 0, (hipStream_t)stream, pixels,
                     (long long)pixel_bytes, images, n_images, tables, (long long)table_words, coef, (long long)ws_blocks);
  AVSEP_LAUNCH_CHECK();
  return AVSEP_OK;
}

extern "C" int avsep_jpeg_enc_count(const int16_t* coef, int64_t ws_blocks, const avsep_jpeg_image* images, int32_t n_images,
                                    int64_t n_intervals, const int32_t* tables, int64_t table_words, int32_t* bits, int64_t* pos,
                                    int32_t* ivl_bytes, int64_t* ivl_off, int64_t* tiles, int64_t tile_words, avsep_stream_t stream) {
  if (!coef || !images || !tables || !bits || !pos || !ivl_bytes || !ivl_off || !tiles) return AVSEP_ERR_ARG;
  if (!je_counts_ok(n_images, ws_blocks, n_intervals, table_words) || (uintptr_t)coef % 16) return AVSEP_ERR_ARG;
  if (tile_words < (ws_blocks + JE_BLOCK - 1) / JE_BLOCK) return AVSEP_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(jpeg_enc_count_kernel, dim3(je_grid(ws_blocks)), dim3(JE_BLOCK), 0, s, coef, (long long)ws_blocks, images, n_images,
                     tables, (long long)table_words, bits);
  AVSEP_LAUNCH_CHECK();
  int rc = je_running_sum(bits, ws_blocks, (long long*)pos, (long long*)tiles, s);
  if (rc != AVSEP_OK) return rc;
  hipLaunchKernelGGL(jpeg_enc_interval_kernel, dim3(je_grid(n_intervals)), dim3(JE_BLOCK), 0, s, images, n_images, (long long)ws_blocks,
                     (long long)n_intervals, (const long long*)pos, ivl_bytes);
  AVSEP_LAUNCH_CHECK();
  return je_running_sum(ivl_bytes, n_intervals, (long long*)ivl_off, (long long*)tiles, s);
}

extern "C" int avsep_jpeg_enc_pack(const int16_t* coef, int64_t ws_blocks, const avsep_jpeg_image* images, int32_t n_images,
                                   int64_t n_intervals, const int32_t* tables, int64_t table_words, const int64_t* pos,
                                   const int64_t* ivl_off, uint8_t* stream_buf, int64_t stream_bytes, int32_t* groups, int64_t* ffpos,
                                   int64_t* ff0, int32_t* ivl_out, int64_t* out_off, int64_t* tiles, int64_t tile_words,
                                   avsep_stream_t stream) {
  if (!coef || !images || !tables || !pos || !ivl_off || !stream_buf || !groups || !ffpos || !ff0 || !ivl_out || !out_off || !tiles)
    return AVSEP_ERR_ARG;
  if (!je_counts_ok(n_images, ws_blocks, n_intervals, table_words) || (uintptr_t)coef % 16) return AVSEP_ERR_ARG;
  if (stream_bytes < 4 || stream_bytes % 4 || (uintptr_t)stream_buf % 4) return AVSEP_ERR_ARG;
  const long long ngroups = (stream_bytes + JE_GROUP - 1) / JE_GROUP, nwords = stream_bytes / 4;
  const long long most = ngroups > n_intervals ? ngroups : n_intervals;
  if (tile_words < (most + JE_BLOCK - 1) / JE_BLOCK) return AVSEP_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(stream_buf, 0, (size_t)stream_bytes, s) != hipSuccess) return AVSEP_ERR_LAUNCH;
  hipLaunchKernelGGL(jpeg_enc_pack_kernel, dim3(je_grid(ws_blocks)), dim3(JE_BLOCK), 0, s, coef, (long long)ws_blocks, images, n_images,
                     (long long)n_intervals, tables, (long long)table_words, (const long long*)pos, (const long long*)ivl_off,
                     (uint32_t*)stream_buf, nwords);
  AVSEP_LAUNCH_CHECK();
  hipLaunchKernelGGL(jpeg_enc_ff_kernel, dim3(je_grid(ngroups)), dim3(JE_BLOCK), 0, s, (const uint32_t*)stream_buf, nwords, ngroups, groups);
  AVSEP_LAUNCH_CHECK();
  int rc = je_running_sum(groups, ngroups, (long long*)ffpos, (long long*)tiles, s);
  if (rc != AVSEP_OK) return rc;
  hipLaunchKernelGGL(jpeg_enc_stuffed_kernel, dim3(je_grid(n_intervals)), dim3(JE_BLOCK), 0, s, (const uint8_t*)stream_buf,
                     (long long)stream_bytes, (long long)n_intervals, (const long long*)ivl_off, (const long long*)ffpos, ngroups,
                     (long long*)ff0, ivl_out);
  AVSEP_LAUNCH_CHECK();
  return je_running_sum(ivl_out, n_intervals, (long long*)out_off, (long long*)tiles, s);
}

extern "C" int avsep_jpeg_enc_stuff(const uint8_t* stream_buf, int64_t stream_bytes, const avsep_jpeg_image* images, int32_t n_images,
                                    int64_t n_intervals, const int64_t* ivl_off, const int64_t* ffpos, const int64_t* ff0,
                                    const int64_t* out_off, uint8_t* out, int64_t out_bytes, int64_t* sizes, avsep_stream_t stream) {
  if (!stream_buf || !images || !ivl_off || !ffpos || !ff0 || !out_off || !out || !sizes) return AVSEP_ERR_ARG;
  if (n_images < 1 || n_images > (1 << 24) || n_intervals < 1 || stream_bytes < 4 || stream_bytes % 4 || out_bytes < 1) return AVSEP_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(jpeg_enc_stuff_kernel, dim3(je_grid((stream_bytes + JE_GROUP - 1) / JE_GROUP)), dim3(JE_BLOCK), 0, s, stream_buf,
                     (long long)stream_bytes, (long long)n_intervals, (const long long*)ivl_off, (const long long*)ffpos,
                     (const long long*)ff0, (const long long*)out_off, out, (long long)out_bytes);
  AVSEP_LAUNCH_CHECK();
  hipLaunchKernelGGL(jpeg_enc_marker_kernel, dim3(je_grid(n_intervals)), dim3(JE_BLOCK), 0, s, images, n_images, (long long)(1LL << 32),
                     (long long)n_intervals, (const long long*)out_off, out, (long long)out_bytes, (long long*)sizes);
  AVSEP_LAUNCH_CHECK();
  return AVSEP_OK;
}
