// The scan decoder of csrc/jpeg_parts.h (jp_decode_scan) on the CPU, for tests/test_jpeg_prog_host.py: a stand-alone program that
// the test compiles with the host compiler under -fsanitize=address,undefined and runs as a child process.
//   jpeg_scan_host CASE DUMP
// CASE: int64 nbytes, n_images, n_scans, table_words, ws_blocks, then the bytes, the image rows, the scan rows, int32 [n_scans]
// the level of the launch each row is part of, and the tables, as the kernels get them.  The rows run in their order, which is
// the order of the launches (rising level).  DUMP: int32 status [n_images], int32 result [n_scans] (the bits each row's decoder
// returned), int16 coef [64 * ws_blocks].  Every buffer is allocated at its exact size, so a read or write past one is a
// sanitizer report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "jpeg_parts.h"

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
  const long long nbytes = head[0], n_images = head[1], n_scans = head[2], table_words = head[3], ws_blocks = head[4];
  uint8_t* bytes = read_array<uint8_t>(f, nbytes);
  avsep_jpeg_image* images = read_array<avsep_jpeg_image>(f, n_images);
  avsep_jpeg_scan* scans = read_array<avsep_jpeg_scan>(f, n_scans);
  int32_t* levels = read_array<int32_t>(f, n_scans);
  int32_t* tables = read_array<int32_t>(f, table_words);
  fclose(f);
  int16_t* coef = (int16_t*)calloc((size_t)ws_blocks * 64, sizeof(int16_t));
  int32_t* status = (int32_t*)calloc((size_t)n_images, sizeof(int32_t));
  std::vector<int32_t> result((size_t)n_scans);
  for (long long s = 0; s < n_scans; ++s)
    result[(size_t)s] = jp_decode_scan(bytes, nbytes, images, (int)n_images, scans[s], levels[s], tables, table_words, coef, ws_blocks, status);
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 2;
  fwrite(status, sizeof(int32_t), (size_t)n_images, o);
  fwrite(result.data(), sizeof(int32_t), (size_t)n_scans, o);
  fwrite(coef, sizeof(int16_t), (size_t)ws_blocks * 64, o);
  fclose(o);
  free(bytes), free(images), free(scans), free(levels), free(tables), free(coef), free(status);
  return 0;
}
