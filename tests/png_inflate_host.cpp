// The PNG decoder's lane bodies of csrc/png_parts.h on the CPU, for tests/test_png_host.py: a stand-alone program that the test
// compiles with the host compiler under -fsanitize=address,undefined and runs as a child process.
//   png_inflate_host CASE DUMP
// CASE: int64 nbytes, n_images, table_bytes, ws_bytes, pixel_bytes, then the bytes, the image rows and the tables, as the kernels
// get them.  Per image: pn_inflate, then its scanlines unfiltered in place pixel by pixel (pn_unfilter_pixel), then every pixel
// through pn_colour; a stage runs only while the image's status is 0.  DUMP: int32 status [n_images], uint8 pixels [pixel_bytes]
// (0xA5 where nothing was written).  Every buffer is allocated at its exact size, so a read or write past one is a sanitizer report.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "png_parts.h"

template <class T>
static T* read_array(FILE* f, long long n) {
  T* p = (T*)malloc(n > 0 ? (size_t)n * sizeof(T) : 1);
  if (n > 0 && fread(p, sizeof(T), (size_t)n, f) != (size_t)n) {
    fprintf(stderr, "short case file\n");
    exit(2);
  }
  return p;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  long long head[5];
  if (fread(head, sizeof(long long), 5, f) != 5) return 2;
  const long long nbytes = head[0], n_images = head[1], table_bytes = head[2], ws_bytes = head[3], pixel_bytes = head[4];
  uint8_t* bytes = read_array<uint8_t>(f, nbytes);
  avsep_png_image* images = read_array<avsep_png_image>(f, n_images);
  uint8_t* tables = read_array<uint8_t>(f, table_bytes);
  fclose(f);
  uint8_t* ws = (uint8_t*)malloc((size_t)ws_bytes);
  uint8_t* pixels = (uint8_t*)malloc((size_t)pixel_bytes);
  int32_t* status = (int32_t*)calloc((size_t)n_images, sizeof(int32_t));
  PnTables* t = (PnTables*)malloc(sizeof(PnTables));
  memset(pixels, 0xA5, (size_t)pixel_bytes);
  for (long long i = 0; i < n_images; ++i) {
    const avsep_png_image im = images[i];
    memset(ws, 0xA5, (size_t)ws_bytes);
    status[i] = pn_inflate(bytes, nbytes, im, ws, ws_bytes, t);
    long long raw = 0;
    if (status[i] || !pn_image_ok(im, &raw)) continue;
    if (!pn_inside(im.pix_off, (long long)im.H * im.W * 3, pixel_bytes) ||
        (im.colour == 3 && !pn_inside(im.palette, (long long)im.entries * 3, table_bytes))) {
      status[i] = PN_ST_ROW;
      continue;
    }
    const int bpp = im.channels;
    const long long stride = 1 + (long long)im.W * bpp;
    uint8_t* base = ws + im.ws_off;
    for (int r = 0; r < im.H; ++r) {
      uint8_t* row = base + r * stride;
      if (row[0] > 4) {
        status[i] |= PN_ST_FILTER;
        break;
      }
      uint32_t a = 0, c = 0;
      for (int x = 0; x < im.W; ++x) {
        uint8_t* p = row + 1 + (long long)x * bpp;
        const uint32_t b = r ? pn_load_pixel(p - stride, bpp) : 0u;
        const uint32_t out = pn_unfilter_pixel(row[0], pn_load_pixel(p, bpp), a, b, c, bpp);
        pn_store_pixel(p, bpp, out);
        a = out, c = b;
      }
    }
    if (status[i]) continue;
    for (long long p = 0; p < (long long)im.H * im.W; ++p) {
      const uint8_t* px = base + (p / im.W) * stride + 1 + (p % im.W) * bpp;
      if (!pn_colour(im.colour, px, tables + im.palette, im.entries, pixels + im.pix_off + p * 3)) status[i] |= PN_ST_PALETTE;
    }
  }
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 2;
  fwrite(status, sizeof(int32_t), (size_t)n_images, o);
  fwrite(pixels, 1, (size_t)pixel_bytes, o);
  fclose(o);
  free(bytes), free(images), free(tables), free(ws), free(pixels), free(status), free(t);
  return 0;
}
