"""The PNG decoder restated: the chunk walk, zlib.decompress, the five scanline filters and the colour rule, in plain Python and
NumPy.  tests/test_png_host.py pins it to Pillow on the grid; the kernels and the host program are held against it."""
import struct
import zlib

import numpy as np

CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}


def chunks(data):
    """[(type, body)] of a file's chunks, up to IEND."""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, out = 8, []
    while True:
        n, kind = struct.unpack(">I", data[at:at + 4])[0], data[at + 4:at + 8]
        out.append((kind, data[at + 8:at + 8 + n]))
        at += 12 + n
        if kind == b"IEND":
            return out


def paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else (b if pb <= pc else c)


def unfilter(raw, H, W, bpp):
    """The filtered scanlines -> uint8 [H, W * bpp]."""
    stride = W * bpp
    assert len(raw) == H * (1 + stride)
    out = np.zeros((H, stride), dtype=np.uint8)
    prev = [0] * stride
    for r in range(H):
        ft, line = raw[r * (1 + stride)], raw[r * (1 + stride) + 1:(r + 1) * (1 + stride)]
        assert ft <= 4, f"filter byte {ft}"
        cur = [0] * stride
        for i, x in enumerate(line):
            a = cur[i - bpp] if i >= bpp else 0
            b = prev[i]
            c = prev[i - bpp] if i >= bpp else 0
            cur[i] = (x + (0, a, b, (a + b) // 2, paeth(a, b, c))[ft]) & 255
        out[r] = cur
        prev = cur
    return out


def decode(data):
    """One 8-bit, non-interlaced PNG file -> uint8 [H,W,3], what ``convert("RGB")`` gives: grey three times, RGB as it is, the
    alpha dropped, palette entries looked up (an index past the palette is an error here)."""
    cs = chunks(data)
    W, H, depth, colour, _, _, interlace = struct.unpack(">IIBBBBB", cs[0][1])
    assert cs[0][0] == b"IHDR" and depth == 8 and interlace == 0
    bpp = CHANNELS[colour]
    raw = zlib.decompress(b"".join(body for kind, body in cs if kind == b"IDAT"))
    px = unfilter(raw, H, W, bpp).reshape(H, W, bpp)
    if colour == 3:
        pal = np.frombuffer(next(body for kind, body in cs if kind == b"PLTE"), dtype=np.uint8).reshape(-1, 3)
        assert int(px.max()) < len(pal), "a palette index past the palette"
        return pal[px[:, :, 0]]
    if colour in (2, 6):
        return np.ascontiguousarray(px[:, :, :3])
    return np.repeat(px[:, :, :1], 3, axis=2)
