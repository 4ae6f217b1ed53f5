"""The PNG files the decoder's tests share, made at run time: a writer that takes pixels, a colour type and a filter type per row
(filtering in NumPy, deflating with zlib at a chosen level and strategy, chunking with correct CRCs and a chosen IDAT split), a
deflate bit writer for streams zlib never emits, the grid, the crafted streams and the case file the host program of
tests/png_inflate_host.cpp reads.  A plain helper module: no fixtures, no tests."""
import functools
import io
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
SIZES = [(1, 1), (1, 9), (9, 1), (5, 7), (17, 33), (64, 65), (130, 67)]                                    # H x W
COLOURS = [(0, False), (2, False), (3, False), (3, True), (4, False), (6, False)]                          # colour type, with tRNS
FILTERS = [0, 1, 2, 3, 4, "cycle", "pillow"]
DEFLATES = [("stored", 0, zlib.Z_DEFAULT_STRATEGY), ("fixed", 6, zlib.Z_FIXED), ("6", 6, zlib.Z_DEFAULT_STRATEGY),
            ("9", 9, zlib.Z_DEFAULT_STRATEGY), ("rle", 6, zlib.Z_RLE), ("huffman", 6, zlib.Z_HUFFMAN_ONLY)]
PALETTE_ENTRIES = 37


def picture(H, W, channels=3, seed=0, top=256):
    """A seeded H x W picture with edges, gradients and noise -> uint8 [H,W,channels], values below ``top``."""
    rng = np.random.default_rng(seed * 1000003 + H * 1009 + W * 7 + channels)
    yy, xx = np.mgrid[0:H, 0:W]
    a = np.stack([(yy * (7 + c) + xx * (3 + 2 * c)) % 256 for c in range(channels)], axis=2)
    return ((a // 2 + rng.integers(0, 128, (H, W, channels))) % top).astype(np.uint8)


def palette(n=PALETTE_ENTRIES, seed=3):
    return np.random.default_rng(seed).integers(0, 256, (n, 3)).astype(np.uint8)


def paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else (b if pb <= pc else c)


def filter_rows(px, filters):
    """px uint8 [H,W,C], one filter type per row (a value above 4 is written as it is, over unfiltered bytes) -> the filtered
    scanlines, bytes."""
    H, W, C = px.shape
    rows = px.reshape(H, W * C).astype(np.int64)
    out = bytearray()
    for r in range(H):
        cur = rows[r]
        a = np.concatenate([np.zeros(C, dtype=np.int64), cur[:-C]]) if W * C > C else np.zeros(W * C, dtype=np.int64)
        b = rows[r - 1] if r else np.zeros(W * C, dtype=np.int64)
        c = np.concatenate([np.zeros(C, dtype=np.int64), b[:-C]]) if W * C > C else np.zeros(W * C, dtype=np.int64)
        ft = filters[r]
        if ft == 1:
            pred = a
        elif ft == 2:
            pred = b
        elif ft == 3:
            pred = (a + b) // 2
        elif ft == 4:
            pred = np.array([paeth(int(x), int(y), int(z)) for x, y, z in zip(a, b, c)], dtype=np.int64)
        else:
            pred = np.zeros(W * C, dtype=np.int64)
        out.append(ft)
        out += ((cur - pred) % 256).astype(np.uint8).tobytes()
    return bytes(out)


def chunk(kind, body=b""):
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body))


def deflate(raw, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, 15, 8, strategy)
    return c.compress(raw) + c.flush()


def wrap(stream, H, W, colour, plte=None, trns=None, split=None, empties=False, depth=8, interlace=0, before=(), after=()):
    """A zlib stream (or anything else) as the IDAT payload of a PNG file.  split: bytes per IDAT chunk; empties: an empty IDAT
    between them; before / after: whole chunks put before the first and after the last IDAT."""
    out = SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, depth, colour, 0, 0, interlace))
    if plte is not None:
        out += chunk(b"PLTE", np.asarray(plte, dtype=np.uint8).tobytes())
    if trns is not None:
        out += chunk(b"tRNS", bytes(trns))
    out += b"".join(before)
    step = split or max(len(stream), 1)
    for at in range(0, max(len(stream), 1), step):
        out += chunk(b"IDAT", stream[at:at + step]) + (chunk(b"IDAT") if empties else b"")
    return out + b"".join(after) + chunk(b"IEND")


def write_png(px, colour, filters=0, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, plte=None, trns=None, **kw):
    """px uint8 [H,W,channels of the colour type] -> a PNG file.  filters: one type for every row, a list with one per row, or
    "cycle" (0 .. 4 row by row)."""
    H, W, C = px.shape
    assert C == CHANNELS[colour]
    if filters == "cycle":
        filters = [r % 5 for r in range(H)]
    elif not isinstance(filters, (list, tuple)):
        filters = [filters] * H
    return wrap(deflate(filter_rows(px, filters), level, strategy), H, W, colour, plte=plte, trns=trns, **kw)


def pillow_png(px, colour, plte=None, trns=None, level=6):
    """The same picture saved by Pillow: its own choice of filters."""
    from PIL import Image
    mode = {0: "L", 2: "RGB", 3: "P", 4: "LA", 6: "RGBA"}[colour]
    im = Image.fromarray(px[:, :, 0] if px.shape[2] == 1 else px, mode)
    kw = {}
    if colour == 3:
        im.putpalette(np.asarray(plte, dtype=np.uint8).reshape(-1).tolist())
        if trns is not None:
            kw["transparency"] = bytes(trns)
    b = io.BytesIO()
    im.save(b, "PNG", compress_level=level, **kw)
    return b.getvalue()


def pillow(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"), dtype=np.uint8)


def source(H, W, colour, seed=0):
    """The pixels of a grid file -> (px [H,W,channels], palette or None)."""
    if colour == 3:
        return picture(H, W, 1, seed, top=PALETTE_ENTRIES), palette()
    return picture(H, W, CHANNELS[colour], seed), None


@functools.lru_cache(maxsize=1)
def grid():
    """The 49 files of the grid -> [(name, bytes)], in a fixed order: (size a, filter b, colour a + b, deflate a + 2 b) over
    a, b = 0 .. 6, indices modulo 7 and then modulo the axis: every pairing of two axes' values is there."""
    out = []
    for a in range(7):
        for b in range(7):
            (H, W), filt = SIZES[a], FILTERS[b]
            (colour, with_trns), (dname, level, strategy) = COLOURS[(a + b) % 7 % 6], DEFLATES[(a + 2 * b) % 7 % 6]
            px, plte = source(H, W, colour, seed=a * 7 + b)
            trns = bytes(range(0, 250, 10)) if with_trns else None
            name = f"{H}x{W}-c{colour}{'t' if with_trns else ''}-f{filt}-{dname}"
            if filt == "pillow":
                out.append((name, pillow_png(px, colour, plte, trns, level)))
            else:
                out.append((name, write_png(px, colour, filt, level, strategy, plte=plte, trns=trns)))
    return out


@functools.lru_cache(maxsize=1)
def grid_reference():
    """Per grid file the restatement's pixels uint8 [H,W,3]: computed once, read only."""
    import png_ref
    return [png_ref.decode(d) for _, d in grid()]


# ---- a deflate bit writer for streams zlib's own compressor never emits ---------------------------------------------------
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def canonical(lens):
    """{symbol: (code, length)} of the canonical Huffman code with these lengths (RFC 1951 3.2.2)."""
    out, code = {}, 0
    for length in range(1, 16):
        for s, n in enumerate(lens):
            if n == length:
                out[s] = (code, length)
                code += 1
        code <<= 1
    return out


class Bits:
    """Deflate's bit order: values lowest bit first, Huffman codes highest bit first."""

    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, value, n):
        self.acc |= (value & ((1 << n) - 1)) << self.n
        self.n += n

    def code(self, code, n):
        self.put(int(format(code, f"0{n}b")[::-1], 2), n)

    def align(self):
        self.n = -(-self.n // 8) * 8

    def bytes(self):
        return self.acc.to_bytes(-(-self.n // 8), "little")

    # -- blocks
    def head(self, last, kind):
        self.put(1 if last else 0, 1)
        self.put(kind, 2)

    def fixed_symbol(self, s):
        if s < 144:
            self.code(0x30 + s, 8)
        elif s < 256:
            self.code(0x190 + s - 144, 9)
        elif s < 280:
            self.code(s - 256, 7)
        else:
            self.code(0xC0 + s - 280, 8)

    def match(self, length, dist, lit=None, dst=None):
        """A match with the fixed codes, or with the canonical codes lit / dst ({symbol: (code, length)})."""
        ls = max(i for i, v in enumerate(LEN_BASE) if v <= length)
        ds = max(i for i, v in enumerate(DIST_BASE) if v <= dist)
        self.fixed_symbol(257 + ls) if lit is None else self.code(*lit[257 + ls])
        self.put(length - LEN_BASE[ls], LEN_EXTRA[ls])
        self.code(ds, 5) if dst is None else self.code(*dst[ds])
        self.put(dist - DIST_BASE[ds], DIST_EXTRA[ds])

    def dynamic_head(self, last, litlens, distlens, hlit=None, hdist=None):
        """The header of a dynamic block: the lengths written with the code-length symbols 0 .. 15 and 18 (zero runs of 11 or
        more), whose own code is symbols 0 .. 14 at 4 bits, 15 and 18 at 5 bits."""
        self.head(last, 2)
        self.put((len(litlens) if hlit is None else hlit) - 257, 5)
        self.put((len(distlens) if hdist is None else hdist) - 1, 5)
        self.put(19 - 4, 4)
        clens = [4] * 15 + [5, 0, 0, 5]
        for s in ORDER:
            self.put(clens[s], 3)
        cc = canonical(clens)
        lens, i = list(litlens) + list(distlens), 0
        while i < len(lens):
            run = 0
            while i + run < len(lens) and lens[i + run] == 0 and run < 138:
                run += 1
            if run >= 11:
                self.code(*cc[18])
                self.put(run - 11, 7)
                i += run
            else:
                self.code(*cc[lens[i]])
                i += 1


def zlib_wrap(raw_deflate, data, header=b"\x78\x9c", adler=None):
    """A raw deflate stream as a zlib stream that claims to hold ``data``."""
    return header + raw_deflate + struct.pack(">I", zlib.adler32(data) if adler is None else adler)


def window_stream():
    """The 1365 x 10 RGB picture whose rows 8 and 9 repeat rows 0 and 1, and its hand-written stream: 32 768 fixed-Huffman literals,
    then matches of length 258 at distance 32 768, the tail a shorter match -> (pixels [10,1365,3], the zlib stream)."""
    px = picture(8, 1365, 3, seed=11)
    px = np.concatenate([px, px[:2]], axis=0)
    raw = filter_rows(px, [0] * 10)
    assert len(raw) == 40960 and raw[32768:] == raw[:8192]
    w = Bits()
    w.head(True, 1)
    for v in raw[:32768]:
        w.fixed_symbol(v)
    for at in range(0, 8192, 258):                                       # 31 of 258 and a tail of 194
        w.match(min(258, 8192 - at), 32768)
    w.fixed_symbol(256)
    return px, zlib_wrap(w.bytes(), raw)


TARGET = np.zeros((2, 3, 1), dtype=np.uint8)          # the picture of the crafted streams: grey 2 x 3, 8 bytes of scanlines, all zero
TARGET_RAW = bytes(8)


def _fixed(literals, last=True, end=True):
    w = Bits()
    w.head(last, 1)
    for v in literals:
        w.fixed_symbol(v)
    if end:
        w.fixed_symbol(256)
    return w


@functools.lru_cache(maxsize=1)
def crafted():
    """One stream per status bit of the lane -> [(name, the PNG file, the bit or None where only "not accepted" is asked)].
    Every file passes ``png.probe``: it is the lane that meets the damage."""
    out = []

    def add(name, deflate_bytes, bit, **kw):
        out.append((name, wrap(zlib_wrap(deflate_bytes, TARGET_RAW, **kw), 2, 3, 0), bit))

    good = _fixed(TARGET_RAW).bytes()
    add("a good fixed block", good, 0)
    w = Bits(); w.head(True, 0); w.align(); w.put(8, 16); w.put(~8 ^ 1, 16)
    add("stored LEN/NLEN mismatch", w.bytes() + TARGET_RAW, 8)
    w = Bits(); w.head(True, 3)
    add("block type 3", w.bytes() + bytes(8), 4)
    for name, hlit, hdist in (("HLIT 287", 287, 1), ("HDIST 31", 257, 31)):
        w = Bits(); w.head(True, 2); w.put(hlit - 257, 5); w.put(hdist - 1, 5); w.put(15, 4)
        add(name, w.bytes() + bytes(40), 16)
    # code-length code of two 1-bit codes: symbol 0 = 0, symbol 16 (or 18) = 1
    w = Bits(); w.head(True, 2); w.put(0, 5); w.put(0, 5); w.put(0, 4)
    for n in (1, 0, 0, 1):
        w.put(n, 3)
    w.put(1, 1)
    add("repeat with no previous length", w.bytes() + bytes(8), 32)
    w = Bits(); w.head(True, 2); w.put(0, 5); w.put(0, 5); w.put(0, 4)
    for n in (0, 0, 1, 1):
        w.put(n, 3)
    for _ in range(2):
        w.put(1, 1); w.put(127, 7)
    add("repeat past the end", w.bytes() + bytes(8), 32)
    w = Bits(); w.head(True, 2); w.put(0, 5); w.put(0, 5); w.put(0, 4)
    for n in (1, 1, 1, 0):
        w.put(n, 3)
    add("an over-subscribed set", w.bytes() + bytes(8), 64)
    w = Bits(); w.dynamic_head(True, [2] + [0] * 255 + [2], [1])
    add("an incomplete set with a 2-bit longest code", w.bytes() + bytes(8), 128)
    w = Bits(); w.dynamic_head(True, [1, 1] + [0] * 255, [1])
    add("no end-of-block code", w.bytes() + bytes(8), 256)
    add("symbol 286", _fixed([0, 286]).bytes() + bytes(4), 1024)
    w = _fixed([0], end=False); w.fixed_symbol(257); w.code(30, 5)
    add("distance symbol 30", w.bytes() + bytes(4), 1024)
    w = _fixed([0], end=False); w.match(7, 2); w.fixed_symbol(256)
    add("distance one past the start", w.bytes(), 2048)
    add("one byte too many", _fixed(bytes(9)).bytes(), 4096)
    add("one byte too few", _fixed(bytes(7)).bytes(), 8192)
    add("a flipped Adler-32", good, 32768, adler=zlib.adler32(TARGET_RAW) ^ 0x100)
    out.append(("a missing Adler-32", wrap(b"\x78\x9c" + good, 2, 3, 0), 1))
    out.append(("four trailing bytes", wrap(zlib_wrap(good, TARGET_RAW) + bytes(4), 2, 3, 0), 16384))
    # the single exception to "incomplete": one distance code of 1 bit, as Z_RLE streams have; its unused code is an error
    lit = [2, 2] + [0] * 254 + [2, 2]
    for name, bit, status in (("the 1-bit distance set", 0, 0), ("the unused code of the 1-bit distance set", 1, 512)):
        w = Bits(); w.dynamic_head(True, lit, [1])
        cl = canonical(lit)
        w.code(*cl[0])
        for k in range(2):
            w.code(*cl[257]); w.put(bit if k else 0, 1)
        w.code(*cl[0]); w.code(*cl[256])
        add(name, w.bytes(), status)
    for name, header in (("CM 7", b"\x77\x85"), ("CINFO 8", b"\x88\x1c"), ("a failing FCHECK", b"\x78\x9d"), ("FDICT", b"\x78\xbb")):
        add(name, good, 2, header=header)
    name, d = grid()[4 * 7 + 3]                                          # 17 x 33 grey, Average, level 9
    body = _idat(d)
    for k in range(3):
        cut = len(body) * (2 * k + 1) // 6
        out.append((f"cut in third {k + 1}", _with_idat(d, body[:cut]), None))
    out.append(("filter byte 5", write_png(picture(5, 7, 3), 2, [0, 1, 5, 3, 4]), 131072))
    px = picture(5, 7, 1, top=PALETTE_ENTRIES)
    px[3, 4, 0] = PALETTE_ENTRIES
    out.append(("a palette index equal to the entry count", write_png(px, 3, "cycle", plte=palette()), 262144))
    return out


def _idat(data):
    from avsep_amd import png
    return png.probe(data).idat


def _with_idat(data, stream):
    """The file with its IDAT chunks replaced by one that holds ``stream``."""
    out, at, done = bytearray(data[:8]), 8, False
    while at + 12 <= len(data):
        n, kind = struct.unpack(">I", data[at:at + 4])[0], data[at + 4:at + 8]
        if kind != b"IDAT":
            out += data[at:at + 12 + n]
        elif not done:
            out += chunk(b"IDAT", stream)
            done = True
        at += 12 + n
    return bytes(out)


def bit_flips(count=300):
    """``count`` seeded single-bit flips inside the zlib stream of three grid files, CRCs signed again -> [(name, bytes)]."""
    rng = np.random.default_rng(20)
    out = []
    for g in (4 * 7 + 3, 4 * 7 + 0, 3 * 7 + 1):                          # 17 x 33 at level 9 and Z_RLE, 5 x 7 Huffman only
        name, d = grid()[g]
        body = _idat(d)
        for k in range(count):
            bit = int(rng.integers(0, 8 * len(body)))
            b = bytearray(body)
            b[bit // 8] ^= 1 << (bit % 8)
            out.append((f"{name} bit {bit}", _with_idat(d, bytes(b))))
    return out


def write_case(path, plan, chunk_):
    """One chunk of a png.plan as the case file of tests/png_inflate_host.cpp."""
    images = np.ascontiguousarray(plan.images[chunk_.a:chunk_.b])
    tables = plan.tables if len(plan.tables) else np.zeros(1, dtype=np.uint8)
    with open(path, "wb") as f:
        f.write(struct.pack("<5q", len(plan.bytes), len(images), len(tables), chunk_.ws_bytes, plan.pixel_bytes))
        for a in (plan.bytes, images, tables):
            f.write(np.ascontiguousarray(a).tobytes())


def read_dump(path, n_images, pixel_bytes):
    """-> (status int32 [n_images], pixels uint8 [pixel_bytes])."""
    raw = open(path, "rb").read()
    return np.frombuffer(raw[:4 * n_images], dtype=np.int32), np.frombuffer(raw[4 * n_images:], dtype=np.uint8)[:pixel_bytes]
