// Baseline JPEG frames -> uint8 RGB (include/avsep.h; avsep_amd/jpeg.py), bit for bit libjpeg-turbo's default decoder.
// Three kernels on the caller's stream:
//   jpeg_entropy_kernel  one lane per entropy-coded segment: the Huffman stream -> int16 coefficients (jpeg_parts.h:
//                        jp_decode_segment; the same body runs on the host under the sanitizers in the damaged-input test);
//   jpeg_idct_kernel     one lane per block: dequantise, islow inverse DCT, + 128, clamp -> 64 bytes of the block's plane;
//   jpeg_colour_kernel   one lane per pixel: fancy chroma upsampling over the component's real size, YCbCr -> RGB.
// A progressive file (SOF2) fills the same workspace scan by scan: jpeg_scans_kernel, one lane per (scan, restart interval) of one
// level, launched level after level, then jpeg_bound_kernel over the finished coefficients (include/avsep.h).
// The rows of images and segments live in device memory and are not trusted with addresses: each kernel checks what it reads
// from a row against the buffer sizes it was given, and a row that fails leaves its output untouched.
#include "common.h"
#include "jpeg_parts.h"

constexpr int JP_BLOCK = 256;

// grid (n_segments), one lane each: a segment has a wavefront to itself.  Lanes of one wavefront that walk different streams
// take each other's branches; 4, 16 and 64 segments per wavefront were measured 1.4, 1.9 and 2.5 times slower.
__global__ __launch_bounds__(1) void jpeg_entropy_kernel(const uint8_t* __restrict__ bytes, long long nbytes,
                                                         const avsep_jpeg_image* __restrict__ images, int n_images,
                                                         const avsep_jpeg_segment* __restrict__ segments,
                                                         const int32_t* __restrict__ tables, long long table_words,
                                                         int16_t* __restrict__ coef, long long ws_blocks, int32_t* __restrict__ status) {
  jp_decode_segment(bytes, nbytes, images, n_images, segments[blockIdx.x], tables, table_words, coef, ws_blocks, status);
}

// grid (n_scans), one lane each, as above: the scan rows of ONE level of a chunk's progressive images (jpeg_parts.h: jp_decode_scan)
__global__ __launch_bounds__(1) void jpeg_scans_kernel(const uint8_t* __restrict__ bytes, long long nbytes,
                                                       const avsep_jpeg_image* __restrict__ images, int n_images,
                                                       const avsep_jpeg_scan* __restrict__ scans, int level,
                                                       const int32_t* __restrict__ tables, long long table_words,
                                                       int16_t* __restrict__ coef, long long ws_blocks, int32_t* status) {
  jp_decode_scan(bytes, nbytes, images, n_images, scans[blockIdx.x], level, tables, table_words, coef, ws_blocks, status);
}

// grid (ceil(max_blocks / JP_BLOCK), n_images): lane = one block of image blockIdx.y, whose 64 finished coefficients it holds
// against AVSEP_JPEG_MAX_COEF (a baseline lane does this as it decodes; a progressive coefficient is whole only after its last scan)
__global__ __launch_bounds__(JP_BLOCK) void jpeg_bound_kernel(const int16_t* __restrict__ coef, long long ws_blocks,
                                                              const avsep_jpeg_image* __restrict__ images,
                                                              const int32_t* __restrict__ tables, long long table_words,
                                                              int32_t* status) {
  const int img = blockIdx.y;
  const avsep_jpeg_image im = images[img];
  long long nblocks = 0, nintervals = 0;
  if (!jp_image_ok(im, &nblocks, &nintervals) || !jp_inside(im.block0, nblocks, ws_blocks)) return;
  const long long blk = (long long)blockIdx.x * JP_BLOCK + threadIdx.x;
  if (blk >= nblocks) return;
  const long long luma = (long long)im.mcux * im.mcuy * im.hs * im.vs;
  const int c = blk < luma ? 0 : 1 + (int)((blk - luma) / ((long long)im.mcux * im.mcuy));
  const int qoff = c == 0 ? im.quant[0] : (c == 1 ? im.quant[1] : im.quant[2]);
  if (c > 2 || !jp_inside(qoff, JP_QUANT_WORDS, table_words)) return;
  const int32_t* __restrict__ q = tables + qoff;
  const uint4* __restrict__ src = (const uint4*)(coef + (im.block0 + blk) * 64);
  bool over = false;
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const uint4 v = src[r];
    const uint32_t u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long long lo = (long long)(int16_t)(u[j] & 0xffffu) * q[r * 8 + 2 * j], hi = (long long)(int16_t)(u[j] >> 16) * q[r * 8 + 2 * j + 1];
      over |= lo > AVSEP_JPEG_MAX_COEF || lo < -AVSEP_JPEG_MAX_COEF || hi > AVSEP_JPEG_MAX_COEF || hi < -AVSEP_JPEG_MAX_COEF;
    }
  }
  if (over) atomicOr(status + img, JP_ST_BOUND);
}

// grid (ceil(max_blocks / JP_BLOCK), n_images): lane = one block of image blockIdx.y
__global__ __launch_bounds__(JP_BLOCK) void jpeg_idct_kernel(const int16_t* __restrict__ coef, uint8_t* __restrict__ planes,
                                                             long long ws_blocks, const avsep_jpeg_image* __restrict__ images,
                                                             const int32_t* __restrict__ tables, long long table_words,
                                                             const int32_t* __restrict__ status) {
  const int img = blockIdx.y;
  if (status[img] != 0) return;
  const avsep_jpeg_image im = images[img];
  long long nblocks = 0, nintervals = 0;
  if (!jp_image_ok(im, &nblocks, &nintervals) || !jp_inside(im.block0, nblocks, ws_blocks)) return;
  const long long blk = (long long)blockIdx.x * JP_BLOCK + threadIdx.x;
  if (blk >= nblocks) return;
  const long long luma = (long long)im.mcux * im.mcuy * im.hs * im.vs;
  const int c = blk < luma ? 0 : 1 + (int)((blk - luma) / ((long long)im.mcux * im.mcuy));
  const int qoff = c == 0 ? im.quant[0] : (c == 1 ? im.quant[1] : im.quant[2]);       // no run-time index into the row: it stays in registers
  if (c > 2 || !jp_inside(qoff, JP_QUANT_WORDS, table_words)) return;
  const int32_t* __restrict__ q = tables + qoff;
  const uint4* __restrict__ src = (const uint4*)(coef + (im.block0 + blk) * 64);           // 128 bytes per block: aligned
  int w[64];
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const uint4 v = src[r];
    const uint32_t u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      w[r * 8 + 2 * j] = (int)(int16_t)(u[j] & 0xffffu) * q[r * 8 + 2 * j];
      w[r * 8 + 2 * j + 1] = (int)(int16_t)(u[j] >> 16) * q[r * 8 + 2 * j + 1];
    }
  }
#pragma unroll
  for (int x = 0; x < 8; ++x) {
    int o[8];
    jp_idct_1d(w[x], w[8 + x], w[16 + x], w[24 + x], w[32 + x], w[40 + x], w[48 + x], w[56 + x], 11, o);
#pragma unroll
    for (int r = 0; r < 8; ++r) w[r * 8 + x] = o[r];
  }
  uint4* __restrict__ dst = (uint4*)(planes + (im.block0 + blk) * 64);
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    uint32_t p[4];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int r = 2 * rr + h;
      int o[8];
      jp_idct_1d(w[r * 8], w[r * 8 + 1], w[r * 8 + 2], w[r * 8 + 3], w[r * 8 + 4], w[r * 8 + 5], w[r * 8 + 6], w[r * 8 + 7], 18, o);
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = min(max(o[j] + 128, 0), 255);
      p[2 * h] = (uint32_t)o[0] | (uint32_t)o[1] << 8 | (uint32_t)o[2] << 16 | (uint32_t)o[3] << 24;
      p[2 * h + 1] = (uint32_t)o[4] | (uint32_t)o[5] << 8 | (uint32_t)o[6] << 16 | (uint32_t)o[7] << 24;
    }
    dst[rr] = make_uint4(p[0], p[1], p[2], p[3]);
  }
}

// sample (y, x) of a component plane whose blocks start at `base` and lie `bw` across
__device__ __forceinline__ int jp_sample(const uint8_t* __restrict__ planes, long long base, int bw, int y, int x) {
  return planes[(base + (long long)(y >> 3) * bw + (x >> 3)) * 64 + (y & 7) * 8 + (x & 7)];
}

// one chroma sample at output (y, x): libjpeg-turbo's fancy upsampling over the component's real size ch x cw
__device__ __forceinline__ int jp_chroma(const uint8_t* __restrict__ planes, long long base, int bw, int hs, int vs, int ch, int cw,
                                         int y, int x) {
  if (hs == 1) return jp_sample(planes, base, bw, y, x);
  const int i = x >> 1;
  if (cw <= 2) return jp_sample(planes, base, bw, vs == 2 ? y >> 1 : y, i);                 // replicated, not filtered
  const int side = (x & 1) ? min(i + 1, cw - 1) : max(i - 1, 0);                            // the neighbour; itself at the edge
  if (vs == 1) {
    const int cur = jp_sample(planes, base, bw, y, i);
    if (side == i) return cur;
    return (3 * cur + jp_sample(planes, base, bw, y, side) + ((x & 1) ? 2 : 1)) >> 2;
  }
  const int r = y >> 1, other = (y & 1) ? min(r + 1, ch - 1) : max(r - 1, 0);
  const int sum = 3 * jp_sample(planes, base, bw, r, i) + jp_sample(planes, base, bw, other, i);
  const int round = (x & 1) ? 7 : 8;
  if (side == i) return (4 * sum + round) >> 4;
  return (3 * sum + 3 * jp_sample(planes, base, bw, r, side) + jp_sample(planes, base, bw, other, side) + round) >> 4;
}

// grid (ceil(max_pixels / JP_BLOCK), n_images): lane = one pixel of image blockIdx.y
__global__ __launch_bounds__(JP_BLOCK) void jpeg_colour_kernel(const uint8_t* __restrict__ planes, long long ws_blocks,
                                                               const avsep_jpeg_image* __restrict__ images,
                                                               const int32_t* __restrict__ status, uint8_t* __restrict__ pixels,
                                                               long long pixel_bytes) {
  const int img = blockIdx.y;
  if (status[img] != 0) return;
  const avsep_jpeg_image im = images[img];
  long long nblocks = 0, nintervals = 0;
  if (!jp_image_ok(im, &nblocks, &nintervals) || !jp_inside(im.block0, nblocks, ws_blocks)) return;
  if (!jp_inside(im.pix_off, (long long)im.H * im.W * 3, pixel_bytes)) return;
  const long long p = (long long)blockIdx.x * JP_BLOCK + threadIdx.x;
  if (p >= (long long)im.H * im.W) return;
  const int y = (int)(p / im.W), x = (int)(p - (long long)y * im.W);
  const int Y = jp_sample(planes, im.block0, im.mcux * im.hs, y, x);
  int R = Y, G = Y, B = Y;
  if (im.ncomp == 3) {
    const long long mcus = (long long)im.mcux * im.mcuy, cb0 = im.block0 + mcus * im.hs * im.vs;
    const int ch = (im.H + im.vs - 1) / im.vs, cw = (im.W + im.hs - 1) / im.hs;
    const int cb = jp_chroma(planes, cb0, im.mcux, im.hs, im.vs, ch, cw, y, x) - 128;
    const int cr = jp_chroma(planes, cb0 + mcus, im.mcux, im.hs, im.vs, ch, cw, y, x) - 128;
    R = min(max(Y + ((91881 * cr + 32768) >> 16), 0), 255);
    B = min(max(Y + ((116130 * cb + 32768) >> 16), 0), 255);
    G = min(max(Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16), 0), 255);
  }
  uint8_t* o = pixels + im.pix_off + p * 3;
  o[0] = (uint8_t)R, o[1] = (uint8_t)G, o[2] = (uint8_t)B;
}

extern "C" int avsep_jpeg_plan_check(const avsep_jpeg_image* images, int32_t n_images, const avsep_jpeg_segment* segments,
                                     int32_t n_segments, int64_t nbytes, int64_t table_words, int64_t pixel_bytes, int64_t ws_blocks) {
  if (!images || !segments || n_images < 1 || n_segments < 1 || nbytes < 1 || table_words < 1 || pixel_bytes < 1 || ws_blocks < 1)
    return AVSEP_ERR_ARG;
  for (int i = 0; i < n_images; ++i) {
    long long nblocks = 0, nintervals = 0;
    if (!jp_row_ok(images[i], 3, JP_HUFF_WORDS, pixel_bytes, table_words, &nblocks, &nintervals)) return AVSEP_ERR_ARG;
    if (!jp_inside(images[i].block0, nblocks, ws_blocks)) return AVSEP_ERR_ARG;
  }
  for (int s = 0; s < n_segments; ++s) {
    const avsep_jpeg_segment& g = segments[s];
    if (g.image < 0 || g.image >= n_images) return AVSEP_ERR_ARG;
    const avsep_jpeg_image& im = images[g.image];
    const long long mcus = (long long)im.mcux * im.mcuy;
    if (g.begin < 0 || g.end < g.begin || g.end > nbytes) return AVSEP_ERR_ARG;
    if (g.mcus < 1 || !jp_inside(g.mcu0, g.mcus, mcus)) return AVSEP_ERR_ARG;
    // with a restart interval a segment is one interval (the last one what is left); without, the whole image
    const long long per = im.restart ? im.restart : mcus;
    if (g.mcu0 % per != 0 || g.mcus != (per < mcus - g.mcu0 ? per : mcus - g.mcu0)) return AVSEP_ERR_ARG;
  }
  return AVSEP_OK;
}

extern "C" int avsep_jpeg_entropy(const uint8_t* bytes, int64_t nbytes, const avsep_jpeg_image* images, int32_t n_images,
                                  const avsep_jpeg_segment* segments, int32_t n_segments, const int32_t* tables, int64_t table_words,
                                  int16_t* coef, int64_t ws_blocks, int32_t* status, avsep_stream_t stream) {
  if (!bytes || !images || !segments || !tables || !coef || !status) return AVSEP_ERR_ARG;
  if (nbytes < 1 || n_images < 1 || n_segments < 1 || table_words < 1 || ws_blocks < 1 || ws_blocks > (1LL << 32)) return AVSEP_ERR_ARG;
  if (hipMemsetAsync(coef, 0, (size_t)ws_blocks * 128, (hipStream_t)stream) != hipSuccess) return AVSEP_ERR_LAUNCH;
  hipLaunchKernelGGL(jpeg_entropy_kernel, dim3(n_segments), dim3(1), 0, (hipStream_t)stream, bytes, (long long)nbytes, images,
                     n_images, segments, tables, (long long)table_words, coef, (long long)ws_blocks, status);
  AVSEP_LAUNCH_CHECK();
  return AVSEP_OK;
}

extern "C" int avsep_jpeg_scan_check(const avsep_jpeg_image* images, int32_t n_images, const avsep_jpeg_scan* scans, int32_t n_scans,
                                     int64_t nbytes, int64_t table_words, int64_t pixel_bytes, int64_t ws_blocks) {
  if (!images || !scans || n_images < 1 || n_scans < 1 || nbytes < 1 || table_words < 1 || pixel_bytes < 1 || ws_blocks < 1)
    return AVSEP_ERR_ARG;
  for (int i = 0; i < n_images; ++i) {
    long long nblocks = 0, nintervals = 0;
    if (!jp_row_ok(images[i], 3, JP_HUFF_WORDS, pixel_bytes, table_words, &nblocks, &nintervals)) return AVSEP_ERR_ARG;
    if (!jp_inside(images[i].block0, nblocks, ws_blocks)) return AVSEP_ERR_ARG;
  }
  for (int s = 0; s < n_scans; ++s) {
    const avsep_jpeg_scan& g = scans[s];
    if (g.image < 0 || g.image >= n_images) return AVSEP_ERR_ARG;
    long long bw = 0, units_all = 0;
    int ncmp = 0, c1 = 0;
    if (!jp_scan_ok(images[g.image], g, &ncmp, &c1, &bw, &units_all)) return AVSEP_ERR_ARG;
    if (g.begin < 0 || g.end < g.begin || g.end > nbytes) return AVSEP_ERR_ARG;
    if (g.units < 1 || !jp_inside(g.unit0, g.units, units_all)) return AVSEP_ERR_ARG;
    if (g.ss > 0 || g.ah == 0)
      for (int c = 0; c < 3; ++c)
        if (((g.comps >> c) & 1) && !jp_inside(g.table[c], JP_HUFF_WORDS, table_words)) return AVSEP_ERR_ARG;
  }
  return AVSEP_OK;
}

extern "C" int avsep_jpeg_scans(const uint8_t* bytes, int64_t nbytes, const avsep_jpeg_image* images, int32_t n_images,
                                const avsep_jpeg_scan* scans, int32_t n_scans, int32_t level, int32_t zero, const int32_t* tables,
                                int64_t table_words, int16_t* coef, int64_t ws_blocks, int32_t* status, avsep_stream_t stream) {
  if (!bytes || !images || !scans || !tables || !coef || !status) return AVSEP_ERR_ARG;
  if (nbytes < 1 || n_images < 1 || n_scans < 1 || table_words < 1 || ws_blocks < 1 || ws_blocks > (1LL << 32)) return AVSEP_ERR_ARG;
  if (level < 0 || level >= AVSEP_JPEG_MAX_SCANS) return AVSEP_ERR_ARG;
  if (zero && hipMemsetAsync(coef, 0, (size_t)ws_blocks * 128, (hipStream_t)stream) != hipSuccess) return AVSEP_ERR_LAUNCH;
  hipLaunchKernelGGL(jpeg_scans_kernel, dim3(n_scans), dim3(1), 0, (hipStream_t)stream, bytes, (long long)nbytes, images, n_images,
                     scans, (int)level, tables, (long long)table_words, coef, (long long)ws_blocks, status);
  AVSEP_LAUNCH_CHECK();
  return AVSEP_OK;
}

extern "C" int avsep_jpeg_coef_bound(const int16_t* coef, int64_t ws_blocks, const avsep_jpeg_image* images, int32_t n_images,
                                     int32_t max_blocks, const int32_t* tables, int64_t table_words, int32_t* status,
                                     avsep_stream_t stream) {
  if (!coef || !images || !tables || !status) return AVSEP_ERR_ARG;
  if (ws_blocks < 1 || ws_blocks > (1LL << 32) || n_images < 1 || n_images > 65535 || table_words < 1) return AVSEP_ERR_ARG;
  if ((uintptr_t)coef % 16 || max_blocks < 1 || max_blocks > ws_blocks) return AVSEP_ERR_ARG;      // 16-byte loads of a block's rows
  hipLaunchKernelGGL(jpeg_bound_kernel, dim3(cdiv(max_blocks, JP_BLOCK), n_images), dim3(JP_BLOCK), 0, (hipStream_t)stream, coef,
                     (long long)ws_blocks, images, tables, (long long)table_words, status);
  AVSEP_LAUNCH_CHECK();
  return AVSEP_OK;
}

extern "C" int avsep_jpeg_pixels(const int16_t* coef, uint8_t* planes, int64_t ws_blocks, const avsep_jpeg_image* images,
                                 int32_t n_images, int32_t max_blocks, int32_t max_pixels, const int32_t* tables, int64_t table_words,
                                 const int32_t* status, uint8_t* pixels, int64_t pixel_bytes, avsep_stream_t stream) {
  if (!coef || !planes || !images || !tables || !status || !pixels) return AVSEP_ERR_ARG;
  if (ws_blocks < 1 || ws_blocks > (1LL << 32) || n_images < 1 || n_images > 65535 || table_words < 1 || pixel_bytes < 1)
    return AVSEP_ERR_ARG;
  if ((uintptr_t)coef % 16 || (uintptr_t)planes % 16) return AVSEP_ERR_ARG;       // the block kernel's 16-byte loads and stores
  if (max_blocks < 1 || max_blocks > ws_blocks || max_pixels < 1 || max_pixels > JP_MAX_SIDE * JP_MAX_SIDE) return AVSEP_ERR_ARG;
  hipLaunchKernelGGL(jpeg_idct_kernel, dim3(cdiv(max_blocks, JP_BLOCK), n_images), dim3(JP_BLOCK), 0, (hipStream_t)stream, coef,
                     planes, (long long)ws_blocks, images, tables, (long long)table_words, status);
  AVSEP_LAUNCH_CHECK();
  hipLaunchKernelGGL(jpeg_colour_kernel, dim3(cdiv(max_pixels, JP_BLOCK), n_images), dim3(JP_BLOCK), 0, (hipStream_t)stream, planes,
                     (long long)ws_blocks, images, status, pixels, (long long)pixel_bytes);
  AVSEP_LAUNCH_CHECK();
  return AVSEP_OK;
}
