// The parts of the PNG decoder (include/avsep.h) that the device and a plain host compiler share: the limits of a row, the
// inflater of one zlib stream (pn_inflate: the body of png_inflate_kernel's lane, and of the host program tests/png_inflate_host.cpp
// that the no-false-accept test builds under the sanitizers), the five filters on one pixel and the colour rule of one pixel.
// No HIP header is needed to compile it.
#pragma once
#include <stdint.h>
#include "avsep.h"

#if defined(__HIPCC__)
#define PN_HD __host__ __device__ __forceinline__
#else
#define PN_HD static inline
#endif

constexpr int PN_MAX_SIDE = 16384;
constexpr long long PN_MAX_PIXELS = 1LL << 26;
enum {
  PN_ST_RANGE = 1, PN_ST_HEADER = 2, PN_ST_BTYPE = 4, PN_ST_STORED = 8, PN_ST_COUNTS = 16, PN_ST_REPEAT = 32, PN_ST_OVER = 64,
  PN_ST_INCOMPLETE = 128, PN_ST_NOEOB = 256, PN_ST_NOCODE = 512, PN_ST_SYMBOL = 1024, PN_ST_DISTANCE = 2048, PN_ST_OVERFLOW = 4096,
  PN_ST_SHORT = 8192, PN_ST_LEFTOVER = 16384, PN_ST_ADLER = 32768, PN_ST_LOOP = 65536, PN_ST_FILTER = 131072, PN_ST_PALETTE = 262144,
  PN_ST_ROW = 524288
};
static_assert(sizeof(avsep_png_image) == 64, "include/avsep.h; png.py's IMAGE is its dtype");

// [off, off + len) inside [0, size), without forming off + len
PN_HD bool pn_inside(long long off, long long len, long long size) { return off >= 0 && len >= 0 && len <= size && off <= size - len; }
// bytes per pixel of a colour type at bit depth 8; 0 = no such type
PN_HD int pn_channels(int colour) { return colour == 0 ? 1 : (colour == 2 ? 3 : (colour == 3 ? 1 : (colour == 4 ? 2 : (colour == 6 ? 4 : 0)))); }
// What a row says about its image, checked: false = outside the limits of include/avsep.h.  raw: the bytes of its filtered scanlines.
PN_HD bool pn_image_ok(const avsep_png_image& im, long long* raw) {
  if (im.H < 1 || im.H > PN_MAX_SIDE || im.W < 1 || im.W > PN_MAX_SIDE || (long long)im.H * im.W > PN_MAX_PIXELS) return false;
  const int ch = pn_channels(im.colour);
  if (ch == 0 || ch != im.channels) return false;
  if (im.colour == 3 ? (im.entries < 1 || im.entries > 256 || im.palette < 0) : (im.entries != 0 || im.palette != 0)) return false;
  if (im.pix_off < 0 || im.begin < 0 || im.end < im.begin || im.ws_off < 0) return false;
  *raw = (long long)im.H * (1 + (long long)im.W * ch);
  return true;
}

// One canonical Huffman code set (RFC 1951 3.2.2) as the lane reads it.  look: by the next 9 bits of the stream, (symbol << 4) |
// length of a code of up to 9 bits, 0 = a longer code or none; count / sym: codes per length and the symbols in code order, for
// the bit-by-bit walk of the longer ones; offs: scratch of the build.  The lane keeps two of them and the lengths in LDS.
struct PnHuff {
  uint16_t look[512];
  uint16_t count[16], offs[16];
  uint16_t sym[288];
};
struct PnTables {
  PnHuff lit, dist;
  uint8_t lens[320];
};

// lens[0 .. n) -> h.  Returns what the code space has left: 0 = complete, > 0 = incomplete, < 0 = over-subscribed (h is then
// not usable); *longest = the longest code, 0 = no code at all.
PN_HD int pn_build(const uint8_t* lens, int n, PnHuff* h, int* longest) {
  for (int i = 0; i < 16; ++i) h->count[i] = 0;
  for (int i = 0; i < n; ++i) h->count[lens[i] & 15] += 1;
  h->count[0] = 0;
  int left = 1, top = 0;
  for (int len = 1; len < 16; ++len) {
    left = (left << 1) - h->count[len];
    if (left < 0) return -1;
    if (h->count[len]) top = len;
  }
  *longest = top;
  h->offs[1] = 0;
  for (int len = 1; len < 15; ++len) h->offs[len + 1] = (uint16_t)(h->offs[len] + h->count[len]);
  for (int s = 0; s < n; ++s) {
    const int len = lens[s] & 15;
    if (len) h->sym[h->offs[len]++] = (uint16_t)s;            // at most n <= 288 of them
  }
  for (int i = 0; i < 512; ++i) h->look[i] = 0;
  int code = 0, at = 0;
  for (int len = 1; len <= 9; ++len) {
    for (int k = 0; k < h->count[len]; ++k, ++code, ++at) {
      int rev = 0;
      for (int j = 0; j < len; ++j) rev |= ((code >> j) & 1) << (len - 1 - j);      // the stream has a code's first bit lowest
      for (int j = rev; j < 512; j += 1 << len) h->look[j] = (uint16_t)((h->sym[at] << 4) | len);
    }
    code <<= 1;
  }
  return left;
}

// The bits of one stream, least significant first.  Bytes are read from p[pos], pos in [begin, end) only.
struct PnBits {
  const uint8_t* p;
  long long pos, end;
  uint64_t buf;        // the next n bits, lowest first
  int n;
};
PN_HD void pn_fill(PnBits& b) {
  while (b.n <= 56 && b.pos < b.end) {
    b.buf |= (uint64_t)b.p[b.pos] << b.n;
    b.pos += 1, b.n += 8;
  }
}
// k bits (0 <= k <= 16) are there to take
PN_HD bool pn_need(PnBits& b, int k) {
  pn_fill(b);
  return b.n >= k;
}
PN_HD uint32_t pn_take(PnBits& b, int k) {
  const uint32_t v = (uint32_t)b.buf & ((1u << k) - 1u);
  b.buf >>= k, b.n -= k;
  return v;
}
// one symbol of h -> the symbol, or -1 (no code within 15 bits, or one the set leaves unused), -2 (the stream ends inside it)
PN_HD int pn_symbol(PnBits& b, const PnHuff* h) {
  pn_fill(b);
  const uint32_t e = h->look[(uint32_t)b.buf & 511u];
  if (e) {
    if ((int)(e & 15) > b.n) return -2;
    pn_take(b, e & 15);
    return (int)(e >> 4);
  }
  int code = 0, first = 0, index = 0;
  for (int len = 1; len < 16; ++len) {
    if (len > b.n) return -2;
    code |= (int)(b.buf >> (len - 1)) & 1;
    const int cnt = h->count[len];
    if (code - cnt < first) {
      pn_take(b, len);
      return h->sym[index + (code - first)];                  // below the sum of the counts, at most 288
    }
    index += cnt, first += cnt;
    first <<= 1, code <<= 1;
  }
  return -1;
}

// One zlib stream, bytes[im.begin .. im.end), inflated into the image's filtered scanlines ws[im.ws_off ..), exactly
// H * (1 + W * channels) bytes.  Returns the status bits (0 = done); the caller ORs them into the image's status word.
// t: the lane's tables (LDS on the device).  Nothing is trusted: see include/avsep.h.
PN_HD int pn_inflate(const uint8_t* __restrict__ bytes, long long nbytes, const avsep_png_image im, uint8_t* __restrict__ ws,
                     long long ws_bytes, PnTables* t) {
  long long raw = 0;
  if (!pn_image_ok(im, &raw) || !pn_inside(im.ws_off, raw, ws_bytes)) return PN_ST_ROW;
  if (im.end > nbytes) return PN_ST_RANGE;
  uint8_t* out = ws + im.ws_off;
  long long n_out = 0;
  long long budget = raw + 8 * (im.end - im.begin) + 64;      // every round below takes a bit of the stream or gives a byte
  PnBits b = {bytes, im.begin, im.end, 0, 0};
  if (!pn_need(b, 16)) return PN_ST_RANGE;
  const uint32_t cmf = pn_take(b, 8), flg = pn_take(b, 8);
  if ((cmf & 15) != 8 || (cmf >> 4) > 7 || ((cmf << 8) | flg) % 31 != 0 || (flg & 32)) return PN_ST_HEADER;
  uint32_t s1 = 1, s2 = 0;
  int pending = 0;                                            // bytes summed since the last reduction modulo 65521
#define PN_PUT(v)                                          \
  do {                                                     \
    const uint32_t v__ = (v);                              \
    out[n_out++] = (uint8_t)v__;                           \
    s1 += v__, s2 += s1;                                   \
    if (++pending == 5552) s1 %= 65521u, s2 %= 65521u, pending = 0; \
  } while (0)
  bool last = false;
  while (!last) {
    if (--budget < 0) return PN_ST_LOOP;
    if (!pn_need(b, 3)) return PN_ST_RANGE;
    last = pn_take(b, 1) != 0;
    const uint32_t type = pn_take(b, 2);
    if (type == 3) return PN_ST_BTYPE;
    if (type == 0) {
      pn_take(b, b.n & 7);
      if (!pn_need(b, 32)) return PN_ST_RANGE;
      const uint32_t len = pn_take(b, 16), nlen = pn_take(b, 16);
      if (len != (~nlen & 0xffffu)) return PN_ST_STORED;
      if ((long long)len > raw - n_out) return PN_ST_OVERFLOW;
      for (uint32_t i = 0; i < len; ++i) {
        if (!pn_need(b, 8)) return PN_ST_RANGE;
        PN_PUT(pn_take(b, 8));
      }
      budget -= len;
      continue;
    }
    int longest = 0;
    if (type == 1) {
      for (int i = 0; i < 288; ++i) t->lens[i] = (uint8_t)(i < 144 ? 8 : (i < 256 ? 9 : (i < 280 ? 7 : 8)));
      pn_build(t->lens, 288, &t->lit, &longest);
      for (int i = 0; i < 32; ++i) t->lens[i] = 5;
      pn_build(t->lens, 32, &t->dist, &longest);
    } else {
      if (!pn_need(b, 14)) return PN_ST_RANGE;
      const int hlit = (int)pn_take(b, 5) + 257, hdist = (int)pn_take(b, 5) + 1, hclen = (int)pn_take(b, 4) + 4;
      if (hlit > 286 || hdist > 30) return PN_ST_COUNTS;
      for (int i = 0; i < 19; ++i) t->lens[i] = 0;
      for (int i = 0; i < hclen; ++i) {
        if (!pn_need(b, 3)) return PN_ST_RANGE;
        // RFC 1951 3.2.7: the order 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15, five bits each, packed
        const uint64_t order = i < 12 ? 0x022caa324e804a30ULL : 0x00000003c2e1346cULL;
        t->lens[(order >> (5 * (i < 12 ? i : i - 12))) & 31] = (uint8_t)pn_take(b, 3);
      }
      int left = pn_build(t->lens, 19, &t->lit, &longest);
      if (left < 0) return PN_ST_OVER;
      if (left > 0) return PN_ST_INCOMPLETE;
      int have = 0;
      while (have < hlit + hdist) {
        if (--budget < 0) return PN_ST_LOOP;
        const int s = pn_symbol(b, &t->lit);
        if (s < 0) return s == -1 ? PN_ST_NOCODE : PN_ST_RANGE;
        if (s < 16) {
          t->lens[have++] = (uint8_t)s;
          continue;
        }
        int prev = 0, rep;
        if (s == 16) {
          if (have == 0) return PN_ST_REPEAT;
          prev = t->lens[have - 1];
          if (!pn_need(b, 2)) return PN_ST_RANGE;
          rep = 3 + (int)pn_take(b, 2);
        } else if (s == 17) {
          if (!pn_need(b, 3)) return PN_ST_RANGE;
          rep = 3 + (int)pn_take(b, 3);
        } else {
          if (!pn_need(b, 7)) return PN_ST_RANGE;
          rep = 11 + (int)pn_take(b, 7);
        }
        if (have + rep > hlit + hdist) return PN_ST_REPEAT;
        while (rep--) t->lens[have++] = (uint8_t)prev;
      }
      if (t->lens[256] == 0) return PN_ST_NOEOB;
      // zlib's inftrees.c: an incomplete set is an error unless its longest code is 1 bit; a distance set may have no code at all
      left = pn_build(t->lens, hlit, &t->lit, &longest);
      if (left < 0) return PN_ST_OVER;
      if (left > 0 && longest != 1) return PN_ST_INCOMPLETE;
      left = pn_build(t->lens + hlit, hdist, &t->dist, &longest);
      if (left < 0) return PN_ST_OVER;
      if (left > 0 && longest > 1) return PN_ST_INCOMPLETE;
    }
    while (true) {
      if (--budget < 0) return PN_ST_LOOP;
      int s = pn_symbol(b, &t->lit);
      if (s < 0) return s == -1 ? PN_ST_NOCODE : PN_ST_RANGE;
      if (s < 256) {
        if (n_out >= raw) return PN_ST_OVERFLOW;
        PN_PUT((uint32_t)s);
        continue;
      }
      if (s == 256) break;
      if (s > 285) return PN_ST_SYMBOL;
      s -= 257;                                               // RFC 1951 3.2.5: base lengths and extra bits, computed
      int ext = s < 8 || s == 28 ? 0 : (s >> 2) - 1;
      if (!pn_need(b, ext)) return PN_ST_RANGE;
      const int len = (s < 8 ? 3 + s : (s == 28 ? 258 : 3 + ((4 + (s & 3)) << ext))) + (int)pn_take(b, ext);
      const int d = pn_symbol(b, &t->dist);
      if (d < 0) return d == -1 ? PN_ST_NOCODE : PN_ST_RANGE;
      if (d > 29) return PN_ST_SYMBOL;
      ext = d < 4 ? 0 : (d >> 1) - 1;
      if (!pn_need(b, ext)) return PN_ST_RANGE;
      const long long dist = (d < 4 ? 1 + d : 1 + ((2 + (d & 1)) << ext)) + (long long)pn_take(b, ext);
      if (dist > n_out) return PN_ST_DISTANCE;
      if (len > raw - n_out) return PN_ST_OVERFLOW;
      for (int i = 0; i < len; ++i) PN_PUT(out[n_out - dist]);    // byte by byte: a match with dist < len repeats itself
      budget -= len;
    }
  }
#undef PN_PUT
  if (n_out != raw) return PN_ST_SHORT;
  s1 %= 65521u, s2 %= 65521u;
  pn_take(b, b.n & 7);
  if (!pn_need(b, 32)) return PN_ST_RANGE;
  uint32_t sum = 0;
  for (int i = 0; i < 4; ++i) sum = (sum << 8) | pn_take(b, 8);
  if (b.n > 0 || b.pos < b.end) return PN_ST_LEFTOVER;
  if (sum != ((s2 << 16) | s1)) return PN_ST_ADLER;
  return 0;
}

// Paeth's predictor: the first of a, b, c nearest to a + b - c
PN_HD int pn_paeth(int a, int b, int c) {
  const int p = a + b - c;
  const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
  return pa <= pb && pa <= pc ? a : (pb <= pc ? b : c);
}
// One pixel of a scanline with filter ft (0 .. 4): its filtered bytes x and the finished pixels left (a), above (b) and above
// left (c), byte j of each word = channel j, bpp channels -> the finished pixel
PN_HD uint32_t pn_unfilter_pixel(int ft, uint32_t x, uint32_t a, uint32_t b, uint32_t c, int bpp) {
  uint32_t out = 0;
  for (int j = 0; j < 4; ++j) {
    if (j >= bpp) break;
    const int A = (a >> (8 * j)) & 255, B = (b >> (8 * j)) & 255, C = (c >> (8 * j)) & 255;
    const int pred = ft == 1 ? A : (ft == 2 ? B : (ft == 3 ? (A + B) >> 1 : (ft == 4 ? pn_paeth(A, B, C) : 0)));
    out |= ((((x >> (8 * j)) & 255) + (uint32_t)pred) & 255u) << (8 * j);
  }
  return out;
}
// bpp bytes at p as one word, and back
PN_HD uint32_t pn_load_pixel(const uint8_t* p, int bpp) {
  uint32_t v = p[0];
  if (bpp > 1) v |= (uint32_t)p[1] << 8;
  if (bpp > 2) v |= (uint32_t)p[2] << 16;
  if (bpp > 3) v |= (uint32_t)p[3] << 24;
  return v;
}
PN_HD void pn_store_pixel(uint8_t* p, int bpp, uint32_t v) {
  p[0] = (uint8_t)v;
  if (bpp > 1) p[1] = (uint8_t)(v >> 8);
  if (bpp > 2) p[2] = (uint8_t)(v >> 16);
  if (bpp > 3) p[3] = (uint8_t)(v >> 24);
}
// One finished pixel px (its `channels` bytes) -> rgb[3].  False: a palette index at or past the entry count (rgb untouched).
PN_HD bool pn_colour(int colour, const uint8_t* px, const uint8_t* pal, int entries, uint8_t* rgb) {
  if (colour == 3) {
    if (px[0] >= entries) return false;
    rgb[0] = pal[3 * px[0]], rgb[1] = pal[3 * px[0] + 1], rgb[2] = pal[3 * px[0] + 2];
  } else if (colour == 2 || colour == 6) {
    rgb[0] = px[0], rgb[1] = px[1], rgb[2] = px[2];
  } else {
    rgb[0] = rgb[1] = rgb[2] = px[0];
  }
  return true;
}
