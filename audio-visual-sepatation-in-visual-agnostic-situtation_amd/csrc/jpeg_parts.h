// The parts of the JPEG decoder and encoder (include/avsep.h) that the device and a plain host compiler share: the limits of a
// row (one row type and one check for both directions) and the two plan checks' test of a host row against its buffers, the
// entropy decoder of one segment (jp_decode_segment: the body of jpeg_entropy_kernel's lanes, and of the host program the
// damaged-input test builds under the sanitizers), the decoder of one scan row of a progressive file (jp_decode_scan: the body of
// jpeg_scans_kernel's lanes and of a second such host program), and the islow inverse DCT pass.  No HIP header is needed to compile it.
#pragma once
#include <stdint.h>
#include "avsep.h"

#if defined(__HIPCC__)
#define JP_HD __host__ __device__ __forceinline__
#else
#define JP_HD static inline
#endif

constexpr int JP_MAX_SIDE = 16384;
constexpr int JP_QUANT_WORDS = 64;
constexpr int JP_HUFF_LOOK = 0, JP_HUFF_MAXCODE = 256, JP_HUFF_VALOFF = 273, JP_HUFF_VALUES = 290, JP_HUFF_WORDS = 546;
enum {
  JP_ST_RANGE = 1, JP_ST_NOCODE = 2, JP_ST_DCSIZE = 4, JP_ST_INDEX = 8, JP_ST_MARKER = 16, JP_ST_BLOCK = 32, JP_ST_TABLE = 64,
  JP_ST_BOUND = 128, JP_ST_ROW = 256, JP_ST_LEFTOVER = 512, JP_ST_REFINE = 1024, JP_ST_EOBRUN = 2048
};
static_assert(sizeof(avsep_jpeg_scan) == 72, "include/avsep.h; jpeg.py's SCAN is its dtype");

constexpr int JP_ENC_HUFF_WORDS = 256;       // an encoder's table, by symbol: (code length << 16) | code, 0 = the table has no such symbol
static_assert(sizeof(avsep_jpeg_image) == 96, "one row for both directions (include/avsep.h); jpeg.py's IMAGE is its dtype");

// What a row says about its image, checked: false = outside the limits of include/avsep.h.  nblocks: all its blocks (an
// encoder's dummy ones included); nintervals: its restart intervals (1 without restarts).
JP_HD bool jp_image_ok(const avsep_jpeg_image& im, long long* nblocks, long long* nintervals) {
  if (im.H < 1 || im.H > JP_MAX_SIDE || im.W < 1 || im.W > JP_MAX_SIDE) return false;
  if (im.ncomp != 1 && im.ncomp != 3) return false;
  const bool form = im.ncomp == 1 ? (im.hs == 1 && im.vs == 1) : ((im.hs == 1 || im.hs == 2) && (im.vs == 1 || im.vs == 2) && im.vs <= im.hs);
  if (!form) return false;
  if (im.mcux != (im.W + 8 * im.hs - 1) / (8 * im.hs) || im.mcuy != (im.H + 8 * im.vs - 1) / (8 * im.vs)) return false;
  if (im.restart < 0 || im.restart > 65535 || im.pix_off < 0 || im.block0 < 0 || im.interval0 < 0) return false;
  const long long mcus = (long long)im.mcux * im.mcuy;
  *nblocks = mcus * (im.hs * im.vs + im.ncomp - 1);
  *nintervals = im.restart ? (mcus + im.restart - 1) / im.restart : 1;
  return true;
}
// [off, off + len) inside [0, size), without forming off + len
JP_HD bool jp_inside(long long off, long long len, long long size) { return off >= 0 && len >= 0 && len <= size && off <= size - len; }
// A HOST row against its limits and its buffers, for the two plan checks: its pixels (H*W*pixel_comps bytes) inside pixel_bytes
// and every component's three tables (Huffman tables of huff_words) inside table_words.
static inline bool jp_row_ok(const avsep_jpeg_image& im, int pixel_comps, int huff_words, long long pixel_bytes, long long table_words,
                             long long* nblocks, long long* nintervals) {
  if (!jp_image_ok(im, nblocks, nintervals) || !jp_inside(im.pix_off, (long long)im.H * im.W * pixel_comps, pixel_bytes)) return false;
  for (int c = 0; c < im.ncomp; ++c)
    if (!jp_inside(im.quant[c], JP_QUANT_WORDS, table_words) || !jp_inside(im.dc[c], huff_words, table_words) ||
        !jp_inside(im.ac[c], huff_words, table_words))
      return false;
  return true;
}

// The bits of one segment, most significant first.  Bytes are read from p[pos], pos in [begin, end) only; FF 00 is one FF;
// FF followed by anything else (or by the end) ends the real bits.  Past them the reader hands out zeros, as many as asked,
// and counts none of them as real: taking more than the real bits is the error, peeking is not.
struct JpBits {
  const uint8_t* p;
  long long pos, end;
  uint64_t buf;        // the next `n` bits, in its low bits
  int n, real;         // bits held; how many of them (the first ones) were read from the segment
  bool marker;         // the real bits ended at a marker
};
JP_HD void jp_fill(JpBits& b) {
  while (b.n <= 56) {
    uint32_t v = 0;
    if (!b.marker && b.pos < b.end) {
      v = b.p[b.pos];
      if (v == 0xFF) {
        if (b.pos + 1 < b.end && b.p[b.pos + 1] == 0) {
          b.pos += 2, b.real += 8;
        } else {
          b.marker = true, v = 0;
        }
      } else {
        b.pos += 1, b.real += 8;
      }
    }
    b.buf = (b.buf << 8) | v, b.n += 8;
  }
}
// the next k bits (1 <= k <= 16), not taken; more than 56 bits are held after a fill
JP_HD uint32_t jp_peek(const JpBits& b, int k) { return (uint32_t)(b.buf >> (b.n - k)) & ((1u << k) - 1u); }
// take k bits: false when they are not all real
JP_HD bool jp_take(JpBits& b, int k) {
  if (k > b.real) return false;
  b.n -= k, b.real -= k;
  return true;
}
// one Huffman symbol from the table at tables + h -> the value, or -1 (no code within 16 bits), -2 (ran out of real bits)
JP_HD int jp_symbol(JpBits& b, const int32_t* __restrict__ t) {
  jp_fill(b);
  const uint32_t code = jp_peek(b, 16);
  const int32_t look = t[JP_HUFF_LOOK + (code >> 8)];
  int len = (look >> 8) & 31, val = look & 255;
  if (len < 1 || len > 8) {
    for (len = 9; len <= 16; ++len) {
      const int32_t c = (int32_t)(code >> (16 - len));
      if (c <= t[JP_HUFF_MAXCODE + len]) {
        val = t[JP_HUFF_VALUES + ((t[JP_HUFF_VALOFF + len] + c) & 255)] & 255;
        break;
      }
    }
    if (len > 16) return -1;
  }
  return jp_take(b, len) ? val : -2;
}
// s further bits as a signed value (receive and extend), 0 <= s <= 15; false when they are not all real
JP_HD bool jp_receive(JpBits& b, int s, int* v) {
  *v = 0;
  if (s == 0) return true;
  jp_fill(b);
  const int r = (int)jp_peek(b, s);
  if (!jp_take(b, s)) return false;
  *v = r < (1 << (s - 1)) ? r - ((1 << s) - 1) : r;
  return true;
}

// natural (row-major) index of zig-zag position k, 0 <= k <= 63: the table as eight packed words, picked by compares, so that a
// lane waits for no memory here (it looks this up for every coefficient)
JP_HD int jp_natural(int k) {
  const uint64_t w = k < 32 ? (k < 16 ? (k < 8 ? 0x0a03020910080100ULL : 0x05040b1219201811ULL) : (k < 24 ? 0x22293028211a130cULL : 0x1c150e07060d141bULL))
                            : (k < 48 ? (k < 40 ? 0x242b323938312a23ULL : 0x332c251e170f161dULL) : (k < 56 ? 0x2e271f262d343b3aULL : 0x3f3e372f363d3c35ULL));
  return (int)(w >> (8 * (k & 7))) & 63;
}

#if defined(__HIP_DEVICE_COMPILE__)
#define JP_FLAG(word, bit) atomicOr((word), (bit))
#else
#define JP_FLAG(word, bit) (*(word) |= (bit))
#endif

// One segment: the Huffman stream bytes[seg.begin .. seg.end) -> the non-zero coefficients of its blocks, int16 in natural order,
// into coef (zeroed before).  Returns the status bits it set (0 = the segment decoded), also ORed into status[seg.image].
// Nothing is trusted: see include/avsep.h.
JP_HD int jp_decode_segment(const uint8_t* __restrict__ bytes, long long nbytes, const avsep_jpeg_image* __restrict__ images,
                            int n_images, const avsep_jpeg_segment seg, const int32_t* __restrict__ tables, long long table_words,
                            int16_t* __restrict__ coef, long long ws_blocks, int32_t* status) {
  if (seg.image < 0 || seg.image >= n_images) return JP_ST_ROW;              // no status word to set
  int32_t* word = status + seg.image;
#define JP_STOP(bit) do { JP_FLAG(word, (bit)); return (bit); } while (0)
  const avsep_jpeg_image im = images[seg.image];
  long long nblocks = 0, nintervals = 0;
  if (!jp_image_ok(im, &nblocks, &nintervals) || !jp_inside(im.block0, nblocks, ws_blocks)) JP_STOP(JP_ST_ROW);
  const long long mcus_all = (long long)im.mcux * im.mcuy;
  if (seg.mcus < 1 || !jp_inside(seg.mcu0, seg.mcus, mcus_all)) JP_STOP(JP_ST_BLOCK);
  if (seg.begin < 0 || seg.end < seg.begin || seg.end > nbytes) JP_STOP(JP_ST_RANGE);
  // no run-time index into the row or the predictors below: they stay in registers on the device
  for (int c = 0; c < 3; ++c)
    if (c < im.ncomp && (!jp_inside(im.quant[c], JP_QUANT_WORDS, table_words) || !jp_inside(im.dc[c], JP_HUFF_WORDS, table_words) ||
                         !jp_inside(im.ac[c], JP_HUFF_WORDS, table_words)))
      JP_STOP(JP_ST_TABLE);
  JpBits b = {bytes, seg.begin, seg.end, 0, 0, 0, false};
  const int luma = im.hs * im.vs, per_mcu = luma + im.ncomp - 1;
  const long long lw = (long long)im.mcux * im.hs;                           // luma blocks across
  const long long chroma0 = mcus_all * luma;                                 // first block of the first chroma plane
  int pred0 = 0, pred1 = 0, pred2 = 0;
  for (long long m = seg.mcu0; m < (long long)seg.mcu0 + seg.mcus; ++m) {
    const long long my = m / im.mcux, mx = m - my * im.mcux;
    for (int i = 0; i < per_mcu; ++i) {
      const int c = i < luma ? 0 : i - luma + 1;
      long long blk;
      if (c == 0) blk = (my * im.vs + i / im.hs) * lw + mx * im.hs + i % im.hs;
      else blk = chroma0 + (c - 1) * mcus_all + m;
      if (blk < 0 || blk >= nblocks) JP_STOP(JP_ST_BLOCK);                   // cannot happen under the checks above: kept as the store's premise
      int16_t* out = coef + (im.block0 + blk) * 64;
      const int32_t* q = tables + (c == 0 ? im.quant[0] : (c == 1 ? im.quant[1] : im.quant[2]));
      const int32_t* dc = tables + (c == 0 ? im.dc[0] : (c == 1 ? im.dc[1] : im.dc[2]));
      const int32_t* ac = tables + (c == 0 ? im.ac[0] : (c == 1 ? im.ac[1] : im.ac[2]));
      int s = jp_symbol(b, dc), v = 0;
      if (s < 0) JP_STOP(s == -1 ? JP_ST_NOCODE : (b.marker ? JP_ST_MARKER : JP_ST_RANGE));
      if (s > 11) JP_STOP(JP_ST_DCSIZE);
      if (!jp_receive(b, s, &v)) JP_STOP(b.marker ? JP_ST_MARKER : JP_ST_RANGE);
      const int pred = (c == 0 ? pred0 : (c == 1 ? pred1 : pred2)) + v;         // |both| < 2^16: the sum cannot wrap
      if (c == 0) pred0 = pred;
      else if (c == 1) pred1 = pred;
      else pred2 = pred;
      {
        const long long d = (long long)pred * q[0];
        if (d > AVSEP_JPEG_MAX_COEF || d < -AVSEP_JPEG_MAX_COEF || pred > 32767 || pred < -32768) JP_STOP(JP_ST_BOUND);
      }
      if (pred != 0) out[0] = (int16_t)pred;
      int k = 1;
      while (k < 64) {                                                       // every round moves k on by at least 1
        const int rs = jp_symbol(b, ac);
        if (rs < 0) JP_STOP(rs == -1 ? JP_ST_NOCODE : (b.marker ? JP_ST_MARKER : JP_ST_RANGE));
        const int run = rs >> 4;
        s = rs & 15;
        if (s == 0) {
          if (run != 15) break;                                              // EOB
          k += 16;                                                           // ZRL
          if (k > 64) JP_STOP(JP_ST_INDEX);
          continue;
        }
        k += run;
        if (k > 63) JP_STOP(JP_ST_INDEX);
        if (!jp_receive(b, s, &v)) JP_STOP(b.marker ? JP_ST_MARKER : JP_ST_RANGE);
        const int nat = jp_natural(k);
        const long long d = (long long)v * q[nat];
        if (d > AVSEP_JPEG_MAX_COEF || d < -AVSEP_JPEG_MAX_COEF) JP_STOP(JP_ST_BOUND);
        if (v != 0) out[nat] = (int16_t)v;
        ++k;
      }
    }
  }
  // what is left must be the padding of the last byte: less than 8 real bits, no byte unread, no marker met
  jp_fill(b);
  if (b.marker) JP_STOP(JP_ST_MARKER);
  if (b.pos < b.end || b.real >= 8) JP_STOP(JP_ST_LEFTOVER);
#undef JP_STOP
  return 0;
}

// ---- progressive files: one scan of one restart interval (include/avsep.h: avsep_jpeg_scan)
// k further bits as they stand (no sign extension), 0 <= k <= 16; false when they are not all real
JP_HD bool jp_bits(JpBits& b, int k, int* v) {
  *v = 0;
  if (k == 0) return true;
  jp_fill(b);
  const int r = (int)jp_peek(b, k);
  if (!jp_take(b, k)) return false;
  *v = r;
  return true;
}
// What a scan row says, checked against its (checked) image: false = outside the rules of include/avsep.h.  ncmp: components in
// the mask; c1: the component of a one-component scan and bw its REAL blocks across; units_all: the units the image has for the mask.
JP_HD bool jp_scan_ok(const avsep_jpeg_image& im, const avsep_jpeg_scan& sc, int* ncmp, int* c1, long long* bw, long long* units_all) {
  if (sc.comps < 1 || sc.comps >= (1 << im.ncomp)) return false;
  if (sc.ss < 0 || sc.se < sc.ss || sc.se > 63 || (sc.ss == 0 && sc.se != 0)) return false;
  if (sc.ah < 0 || sc.ah > 13 || sc.al < 0 || sc.al > 13 || (sc.ah != 0 && sc.al != sc.ah - 1)) return false;
  if (sc.level < 0 || sc.level >= AVSEP_JPEG_MAX_SCANS) return false;
  const int n = (sc.comps & 1) + ((sc.comps >> 1) & 1) + ((sc.comps >> 2) & 1);
  if (sc.ss > 0 && n != 1) return false;
  *ncmp = n, *c1 = sc.comps == 1 ? 0 : (sc.comps == 2 ? 1 : 2), *bw = 0;
  if (n == 1) {
    const long long cw = *c1 == 0 ? im.W : (im.W + im.hs - 1) / im.hs, ch = *c1 == 0 ? im.H : (im.H + im.vs - 1) / im.vs;
    *bw = (cw + 7) / 8;
    *units_all = *bw * ((ch + 7) / 8);
  } else {
    *units_all = (long long)im.mcux * im.mcuy;
  }
  return true;
}
// one correction bit for the non-zero coefficient *at (T.81 G.1.2.3): applied away from zero where bit `al` (p1 = 1 << al) is clear
JP_HD int jp_correct(JpBits& b, int16_t* at, int p1) {
  int bit = 0, v = *at;
  if (!jp_bits(b, 1, &bit)) return b.marker ? JP_ST_MARKER : JP_ST_RANGE;
  if (bit && (v & p1) == 0) {
    v += v >= 0 ? p1 : -p1;
    if (v > 32767 || v < -32768) return JP_ST_BOUND;
    *at = (int16_t)v;
  }
  return 0;
}

// The non-zero coefficients of one block as a mask by zig-zag position (bit k = position k, 1 <= k <= 63): 63 loads that wait for
// nothing but each other, so that a refinement lane, which passes every coefficient of its band, does not wait for memory at each
// one (DESIGN §34 has the measurement).  jp_natural folds to a constant in every round.
JP_HD uint64_t jp_nonzero_mask(const int16_t* __restrict__ blk) {
  uint64_t m = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int k = 1; k < 64; ++k) m |= (uint64_t)(blk[jp_natural(k)] != 0) << k;
  return m;
}

// One scan row: the stream bytes[sc.begin .. sc.end) -> its band and bit position of the coefficients of its blocks, in coef (zeroed
// before level 0; the earlier scans of its coefficients done).  `level`: the level this launch runs.  Returns the status bits it
// set, also ORed into status[sc.image].  Nothing is trusted, as in jp_decode_segment.
JP_HD int jp_decode_scan(const uint8_t* __restrict__ bytes, long long nbytes, const avsep_jpeg_image* __restrict__ images, int n_images,
                         const avsep_jpeg_scan sc, int level, const int32_t* __restrict__ tables, long long table_words,
                         int16_t* __restrict__ coef, long long ws_blocks, int32_t* status) {
  if (sc.image < 0 || sc.image >= n_images) return JP_ST_ROW;                // no status word to set
  int32_t* word = status + sc.image;
  if (level > 0 && *word != 0) return 0;                                     // an earlier level gave the image up
#define JP_STOP(bit) do { JP_FLAG(word, (bit)); return (bit); } while (0)
#define JP_OUT_OF_BITS (b.marker ? JP_ST_MARKER : JP_ST_RANGE)
  const avsep_jpeg_image im = images[sc.image];
  long long nblocks = 0, nintervals = 0, bw = 0, units_all = 0;
  int ncmp = 0, c1 = 0;
  if (!jp_image_ok(im, &nblocks, &nintervals) || !jp_inside(im.block0, nblocks, ws_blocks)) JP_STOP(JP_ST_ROW);
  if (!jp_scan_ok(im, sc, &ncmp, &c1, &bw, &units_all) || sc.level != level) JP_STOP(JP_ST_ROW);
  if (sc.units < 1 || !jp_inside(sc.unit0, sc.units, units_all)) JP_STOP(JP_ST_BLOCK);
  if (sc.begin < 0 || sc.end < sc.begin || sc.end > nbytes) JP_STOP(JP_ST_RANGE);
  const bool dc = sc.ss == 0, first = sc.ah == 0;
  const bool coded = !dc || first;                                           // a DC refinement scan reads no table
  for (int c = 0; c < 3; ++c)
    if (coded && ((sc.comps >> c) & 1) && !jp_inside(sc.table[c], JP_HUFF_WORDS, table_words)) JP_STOP(JP_ST_TABLE);
  JpBits b = {bytes, sc.begin, sc.end, 0, 0, 0, false};
  const int luma = im.hs * im.vs, per_unit = ncmp == 1 ? 1 : luma + im.ncomp - 1;
  const long long mcus_all = (long long)im.mcux * im.mcuy, lw = (long long)im.mcux * im.hs, chroma0 = mcus_all * luma;
  const long long base1 = c1 == 0 ? 0 : chroma0 + (c1 - 1) * mcus_all, stride1 = c1 == 0 ? lw : im.mcux;
  const long long last = (long long)sc.unit0 + sc.units;
  const int p1 = 1 << sc.al;
  int pred0 = 0, pred1 = 0, pred2 = 0, eobrun = 0;                           // no run-time index: they stay in registers
  for (long long u = sc.unit0; u < last; ++u) {
    for (int i = 0; i < per_unit; ++i) {
      int c;
      long long blk;
      if (ncmp == 1) {
        const long long by = u / bw;
        c = c1, blk = base1 + by * stride1 + (u - by * bw);
      } else {
        c = i < luma ? 0 : i - luma + 1;
        if (!((sc.comps >> c) & 1)) continue;
        const long long my = u / im.mcux, mx = u - my * im.mcux;
        if (c == 0) blk = (my * im.vs + i / im.hs) * lw + mx * im.hs + i % im.hs;
        else blk = chroma0 + (c - 1) * mcus_all + u;
      }
      if (blk < 0 || blk >= nblocks) JP_STOP(JP_ST_BLOCK);                   // cannot happen under the checks above: kept as the store's premise
      int16_t* out = coef + (im.block0 + blk) * 64;
      const int32_t* t = tables + (coded ? (c == 0 ? sc.table[0] : (c == 1 ? sc.table[1] : sc.table[2])) : 0);
      if (dc && first) {
        int v = 0;
        const int s = jp_symbol(b, t);
        if (s < 0) JP_STOP(s == -1 ? JP_ST_NOCODE : JP_OUT_OF_BITS);
        if (s > 11) JP_STOP(JP_ST_DCSIZE);
        if (!jp_receive(b, s, &v)) JP_STOP(JP_OUT_OF_BITS);
        const int pred = (c == 0 ? pred0 : (c == 1 ? pred1 : pred2)) + v;       // |both| < 2^16: the sum cannot wrap
        if (c == 0) pred0 = pred;
        else if (c == 1) pred1 = pred;
        else pred2 = pred;
        const int val = pred * p1;
        if (pred > 32767 || pred < -32768 || val > 32767 || val < -32768) JP_STOP(JP_ST_BOUND);
        out[0] = (int16_t)val;
      } else if (dc) {
        int bit = 0;
        if (!jp_bits(b, 1, &bit)) JP_STOP(JP_OUT_OF_BITS);
        if (bit) out[0] = (int16_t)(out[0] | p1);
      } else if (first) {
        if (eobrun > 0) {
          --eobrun;
          continue;
        }
        int k = sc.ss;
        while (k <= sc.se) {                                                 // every round moves k on by at least 1, or ends the block
          const int rs = jp_symbol(b, t);
          if (rs < 0) JP_STOP(rs == -1 ? JP_ST_NOCODE : JP_OUT_OF_BITS);
          const int run = rs >> 4, s = rs & 15;
          int v = 0;
          if (s == 0) {
            if (run == 15) {                                                 // ZRL
              k += 16;
              if (k > sc.se + 1) JP_STOP(JP_ST_INDEX);
              continue;
            }
            if (!jp_bits(b, run, &v)) JP_STOP(JP_OUT_OF_BITS);
            eobrun = (1 << run) + v - 1;                                     // further blocks that end at once
            if (eobrun > last - 1 - u) JP_STOP(JP_ST_EOBRUN);
            break;
          }
          k += run;
          if (k > sc.se) JP_STOP(JP_ST_INDEX);
          if (!jp_receive(b, s, &v)) JP_STOP(JP_OUT_OF_BITS);
          const int val = v * p1;                                            // |v| < 2^15, p1 <= 2^13
          if (val > 32767 || val < -32768) JP_STOP(JP_ST_BOUND);
          out[jp_natural(k)] = (int16_t)val;
          ++k;
        }
      } else {
        int k = sc.ss;
        const uint64_t nonzero = jp_nonzero_mask(out);                       // as the block stands before this scan: k only moves on
        if (eobrun == 0) {
          while (k <= sc.se) {                                               // every round moves k on by at least 1, or ends the block
            const int rs = jp_symbol(b, t);
            if (rs < 0) JP_STOP(rs == -1 ? JP_ST_NOCODE : JP_OUT_OF_BITS);
            int run = rs >> 4, val = 0;
            const int s = rs & 15;
            if (s != 0) {
              int bit = 0;
              if (s != 1) JP_STOP(JP_ST_REFINE);
              if (!jp_bits(b, 1, &bit)) JP_STOP(JP_OUT_OF_BITS);
              val = bit ? p1 : -p1;
            } else if (run != 15) {
              int v = 0;
              if (!jp_bits(b, run, &v)) JP_STOP(JP_OUT_OF_BITS);
              eobrun = (1 << run) + v;                                       // this block and eobrun - 1 further ones
              if (eobrun - 1 > last - 1 - u) JP_STOP(JP_ST_EOBRUN);
              break;
            }
            // over `run` coefficients that are still zero (16 for ZRL, the last one below); the non-zero ones passed are corrected
            while (k <= sc.se) {
              if ((nonzero >> k) & 1) {
                const int e = jp_correct(b, out + jp_natural(k), p1);
                if (e) JP_STOP(e);
              } else if (--run < 0) {
                break;
              }
              ++k;
            }
            if (s != 0) {
              if (k > sc.se) JP_STOP(JP_ST_INDEX);
              out[jp_natural(k)] = (int16_t)val;                             // where the run ends, not earlier
            }
            ++k;
          }
        }
        if (eobrun > 0) {                                                    // the rest of the band: correction bits only
          for (; k <= sc.se; ++k) {
            if ((nonzero >> k) & 1) {
              const int e = jp_correct(b, out + jp_natural(k), p1);
              if (e) JP_STOP(e);
            }
          }
          --eobrun;
        }
      }
    }
  }
  // what is left must be the padding of the last byte: less than 8 real bits, no byte unread, no marker met
  jp_fill(b);
  if (b.marker) JP_STOP(JP_ST_MARKER);
  if (b.pos < b.end || b.real >= 8) JP_STOP(JP_ST_LEFTOVER);
#undef JP_OUT_OF_BITS
#undef JP_STOP
  return 0;
}

// One pass of libjpeg's islow inverse DCT over eight values: CONST_BITS = 13, each output (x + 2^(shift-1)) >> shift with an
// arithmetic shift.  shift = 11 for the column pass (CONST_BITS - PASS1_BITS), 18 for the row pass (CONST_BITS + PASS1_BITS + 3).
// With every input at most AVSEP_JPEG_MAX_COEF in magnitude before the column pass, no value formed here in either pass leaves
// int32: the sum of the absolute weights of the inputs in any of them is at most 61214.
JP_HD void jp_idct_1d(const int d0, const int d1, const int d2, const int d3, const int d4, const int d5, const int d6, const int d7,
                      const int shift, int* o) {
  int z1 = (d2 + d6) * 4433;
  int tmp2 = z1 + d6 * -15137;
  int tmp3 = z1 + d2 * 6270;
  int tmp0 = (d0 + d4) * 8192;
  int tmp1 = (d0 - d4) * 8192;
  const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  tmp0 = d7, tmp1 = d5, tmp2 = d3, tmp3 = d1;
  z1 = tmp0 + tmp3;
  int z2 = tmp1 + tmp2, z3 = tmp0 + tmp2, z4 = tmp1 + tmp3;
  const int z5 = (z3 + z4) * 9633;
  tmp0 *= 2446, tmp1 *= 16819, tmp2 *= 25172, tmp3 *= 12299;
  z1 *= -7373, z2 *= -20995, z3 *= -16069, z4 *= -3196;
  z3 += z5, z4 += z5;
  tmp0 += z1 + z3, tmp1 += z2 + z4, tmp2 += z2 + z3, tmp3 += z1 + z4;
  const int half = 1 << (shift - 1);
  o[0] = (tmp10 + tmp3 + half) >> shift, o[7] = (tmp10 - tmp3 + half) >> shift;
  o[1] = (tmp11 + tmp2 + half) >> shift, o[6] = (tmp11 - tmp2 + half) >> shift;
  o[2] = (tmp12 + tmp1 + half) >> shift, o[5] = (tmp12 - tmp1 + half) >> shift;
  o[3] = (tmp13 + tmp0 + half) >> shift, o[4] = (tmp13 - tmp0 + half) >> shift;
}

// ---- the encoder (jpeg_enc.hip)
// One pass of libjpeg's islow forward DCT over eight values, in place: CONST_BITS = 13, PASS1_BITS = 2.  The row pass
// (second = false) leaves its results scaled up by 4, the column pass (second = true) takes that scaling out again, so a block
// ends 8 times the true DCT.  Samples are 8 bit less 128: no value formed in either pass leaves int32.
JP_HD void jp_fdct_1d(int* v, const bool second) {
  const int t0 = v[0] + v[7], t7 = v[0] - v[7], t1 = v[1] + v[6], t6 = v[1] - v[6];
  const int t2 = v[2] + v[5], t5 = v[2] - v[5], t3 = v[3] + v[4], t4 = v[3] - v[4];
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  const int n = second ? 15 : 11, half = 1 << (n - 1);
  v[0] = second ? (t10 + t11 + 2) >> 2 : (t10 + t11) * 4;
  v[4] = second ? (t10 - t11 + 2) >> 2 : (t10 - t11) * 4;
  int z1 = (t12 + t13) * 4433;
  v[2] = (z1 + t13 * 6270 + half) >> n;
  v[6] = (z1 - t12 * 15137 + half) >> n;
  z1 = t4 + t7;
  int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const int z5 = (z3 + z4) * 9633;
  const int a4 = t4 * 2446, a5 = t5 * 16819, a6 = t6 * 25172, a7 = t7 * 12299;
  z1 *= -7373, z2 *= -20995;
  z3 = z3 * -16069 + z5, z4 = z4 * -3196 + z5;
  v[7] = (a4 + z1 + z3 + half) >> n;
  v[5] = (a5 + z2 + z4 + half) >> n;
  v[3] = (a6 + z2 + z3 + half) >> n;
  v[1] = (a7 + z1 + z4 + half) >> n;
}
