// PNG frames -> uint8 RGB (include/avsep.h; avsep_amd/png.py), the pixels Pillow gives.  Three kernels on the caller's stream:
//   png_inflate_kernel   one lane per image: its zlib stream -> its filtered scanlines in the workspace, which are the LZ77
//                        window too (png_parts.h: pn_inflate; the same body runs on the host under the sanitizers);
//   png_unfilter_kernel  one wavefront per image, in place: lane k = row k of a group of 64 rows, one pixel behind lane k - 1;
//   png_colour_kernel    one lane per pixel: grey, RGB, palette, alpha dropped -> RGB.
// The rows live in device memory and are not trusted with addresses: each kernel checks what it reads from a row against the
// buffer sizes it was given, and a row that fails leaves its output untouched.
#include "common.h"
#include "png_parts.h"

constexpr int PN_BLOCK = 256;

// grid (n_images), one lane each: a stream has a wavefront to itself (lanes that walk different streams take each
// other's branches).  The block's Huffman tables are the lane's, in LDS.
__global__ __launch_bounds__(1) void png_inflate_kernel(const uint8_t* __restrict__ bytes, long long nbytes,
                                                        const avsep_png_image* __restrict__ images, uint8_t* __restrict__ ws,
                                                        long long ws_bytes, int32_t* __restrict__ status) {
  __shared__ PnTables t;
  const int bits = pn_inflate(bytes, nbytes, images[blockIdx.x], ws, ws_bytes, &t);
  if (bits) atomicOr(status + blockIdx.x, bits);
}

// grid (n_images), one wavefront each.  Rows g0 .. g0 + 63 go to lanes 0 .. 63; at step s lane k finishes pixel s - k of its
// row, so the pixel above it is what lane k - 1 finished one step earlier (one __shfl_up of the packed pixel), the pixel above
// left is last step's, and the pixel left is the lane's own.  Lane 0 reads the row above from the workspace: the last row of the
// group before, written by lane 63 through global memory and ordered by the barrier between groups (its workgroup-scope fence).
__global__ __launch_bounds__(64) void png_unfilter_kernel(uint8_t* __restrict__ ws, long long ws_bytes,
                                                          const avsep_png_image* __restrict__ images, int32_t* __restrict__ status) {
  const int img = blockIdx.x;
  if (status[img] != 0) return;
  const avsep_png_image im = images[img];
  long long raw = 0;
  if (!pn_image_ok(im, &raw) || !pn_inside(im.ws_off, raw, ws_bytes)) return;
  const int lane = threadIdx.x, bpp = im.channels;
  const long long stride = 1 + (long long)im.W * bpp;
  uint8_t* base = ws + im.ws_off;
  bool bad = false;
  for (int g0 = 0; g0 < im.H; g0 += 64) {
    const int r = g0 + lane;
    const bool live = r < im.H;
    uint8_t* row = base + (live ? r : g0) * stride;
    int ft = live ? row[0] : 0;
    if (ft > 4) bad = true, ft = 0;
    const int steps = im.W + min(64, im.H - g0) - 1;
    uint32_t a = 0, c = 0, out = 0;
    for (int s = 0; s < steps; ++s) {
      const uint32_t up = __shfl_up(out, 1);
      const int x = s - lane;
      if (live && x >= 0 && x < im.W) {
        uint8_t* p = row + 1 + (long long)x * bpp;
        const uint32_t b = lane ? up : (r > 0 ? pn_load_pixel(p - stride, bpp) : 0u);
        out = pn_unfilter_pixel(ft, pn_load_pixel(p, bpp), a, b, c, bpp);
        pn_store_pixel(p, bpp, out);
        a = out, c = b;
      }
    }
    __syncthreads();
  }
  if (bad) atomicOr(status + img, PN_ST_FILTER);
}

// grid (ceil(max_pixels / PN_BLOCK), n_images): lane = one pixel of image blockIdx.y
__global__ __launch_bounds__(PN_BLOCK) void png_colour_kernel(const uint8_t* __restrict__ ws, long long ws_bytes,
                                                              const avsep_png_image* __restrict__ images,
                                                              const uint8_t* __restrict__ tables, long long table_bytes,
                                                              int32_t* status, uint8_t* __restrict__ pixels, long long pixel_bytes) {
  const int img = blockIdx.y;
  if (status[img] != 0) return;
  const avsep_png_image im = images[img];
  long long raw = 0;
  if (!pn_image_ok(im, &raw) || !pn_inside(im.ws_off, raw, ws_bytes)) return;
  if (!pn_inside(im.pix_off, (long long)im.H * im.W * 3, pixel_bytes)) return;
  if (im.colour == 3 && !pn_inside(im.palette, (long long)im.entries * 3, table_bytes)) return;
  const long long p = (long long)blockIdx.x * PN_BLOCK + threadIdx.x;
  if (p >= (long long)im.H * im.W) return;
  const int y = (int)(p / im.W), x = (int)(p - (long long)y * im.W);
  const uint8_t* px = ws + im.ws_off + y * (1 + (long long)im.W * im.channels) + 1 + (long long)x * im.channels;
  uint8_t rgb[3];
  if (!pn_colour(im.colour, px, tables + im.palette, im.entries, rgb)) {
    atomicOr(status + img, PN_ST_PALETTE);
    return;
  }
  uint8_t* o = pixels + im.pix_off + p * 3;
  o[0] = rgb[0], o[1] = rgb[1], o[2] = rgb[2];
}

extern "C" int avsep_png_plan_check(const avsep_png_image* images, int32_t n_images, int64_t nbytes, int64_t table_bytes,
                                    int64_t pixel_bytes, int64_t ws_bytes) {
  if (!images || n_images < 1 || nbytes < 1 || table_bytes < 1 || pixel_bytes < 1 || ws_bytes < 1) return AVSEP_ERR_ARG;
  for (int i = 0; i < n_images; ++i) {
    const avsep_png_image& im = images[i];
    long long raw = 0;
    if (!pn_image_ok(im, &raw) || im.end > nbytes || !pn_inside(im.ws_off, raw, ws_bytes)) return AVSEP_ERR_ARG;
    if (!pn_inside(im.pix_off, (long long)im.H * im.W * 3, pixel_bytes)) return AVSEP_ERR_ARG;
    if (im.colour == 3 && !pn_inside(im.palette, (long long)im.entries * 3, table_bytes)) return AVSEP_ERR_ARG;
  }
  return AVSEP_OK;
}

extern "C" int avsep_png_inflate(const uint8_t* bytes, int64_t nbytes, const avsep_png_image* images, int32_t n_images, uint8_t* ws,
                                 int64_t ws_bytes, int32_t* status, avsep_stream_t stream) {
  if (!bytes || !images || !ws || !status) return AVSEP_ERR_ARG;
  if (nbytes < 1 || n_images < 1 || n_images > 65535 || ws_bytes < 1) return AVSEP_ERR_ARG;
  hipLaunchKernelGGL(png_inflate_kernel, dim3(n_images), dim3(1), 0, (hipStream_t)stream, bytes, (long long)nbytes, images, ws,
                     (long long)ws_bytes, status);
  AVSEP_LAUNCH_CHECK();
  return AVSEP_OK;
}

extern "C" int avsep_png_pixels(uint8_t* ws, int64_t ws_bytes, const avsep_png_image* images, int32_t n_images, int32_t max_pixels,
                                const uint8_t* tables, int64_t table_bytes, int32_t* status, uint8_t* pixels, int64_t pixel_bytes,
                                int32_t stages, avsep_stream_t stream) {
  if (!ws || !images || !tables || !status || !pixels) return AVSEP_ERR_ARG;
  if (ws_bytes < 1 || n_images < 1 || n_images > 65535 || table_bytes < 1 || pixel_bytes < 1) return AVSEP_ERR_ARG;
  if (max_pixels < 1 || max_pixels > PN_MAX_PIXELS || stages < 1 || stages > 3) return AVSEP_ERR_ARG;
  if (stages & 1) {
    hipLaunchKernelGGL(png_unfilter_kernel, dim3(n_images), dim3(64), 0, (hipStream_t)stream, ws, (long long)ws_bytes, images, status);
    AVSEP_LAUNCH_CHECK();
  }
  if (!(stages & 2)) return AVSEP_OK;
  hipLaunchKernelGGL(png_colour_kernel, dim3(cdiv(max_pixels, PN_BLOCK), n_images), dim3(PN_BLOCK), 0, (hipStream_t)stream, ws,
                     (long long)ws_bytes, images, tables, (long long)table_bytes, status, pixels, (long long)pixel_bytes);
  AVSEP_LAUNCH_CHECK();
  return AVSEP_OK;
}
