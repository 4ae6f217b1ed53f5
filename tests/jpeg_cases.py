"""The JPEG files the decoder's tests share, made by Pillow at run time: the grid of sizes and forms, the damaged set, and the
case file the host program of tests/jpeg_entropy_host.cpp reads.  A plain helper module: no fixtures, no tests."""
import functools
import io
import struct

import numpy as np

SIZES = [(1, 1), (5, 3), (8, 8), (16, 16), (17, 23), (24, 5), (9, 40), (33, 65), (40, 48)]                  # H x W
FORMS = [("444", dict(subsampling=0, quality=85)), ("422", dict(subsampling=1, quality=85)), ("420", dict(subsampling=2, quality=85)),
         ("420rst", dict(subsampling=2, quality=85, restart_marker_blocks=2)), ("420opt", dict(subsampling=2, optimize=True, quality=30)),
         ("444q100", dict(subsampling=0, quality=100)), ("grey", dict(grey=True))]


def picture(H, W, seed=0):
    """A seeded H x W picture with edges, gradients and noise -> uint8 [H,W,3]."""
    rng = np.random.default_rng(seed * 1000003 + H * 1009 + W)
    yy, xx = np.mgrid[0:H, 0:W]
    a = np.stack([(yy * 7 + xx * 3) % 256, (xx * 11) % 256, (yy * 5 + xx) % 256], axis=2)
    return (a // 2 + rng.integers(0, 128, (H, W, 3))).astype(np.uint8)


def encode(a, grey=False, fmt="JPEG", **form):
    from PIL import Image
    im = Image.fromarray(a)
    if grey:
        im = im.convert("L")
    b = io.BytesIO()
    im.save(b, fmt, **form)
    return b.getvalue()


def pillow(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"), dtype=np.uint8)


@functools.lru_cache(maxsize=1)
def grid():
    """The 63 files of the grid -> [(name, bytes)], in a fixed order."""
    return [(f"{H}x{W}-{name}", encode(picture(H, W), **form)) for H, W in SIZES for name, form in FORMS]


@functools.lru_cache(maxsize=1)
def grid_reference():
    """Per grid file (Info, pixels uint8 [H,W,3], coefficients) of the restatement: computed once, read only."""
    import jpeg_ref
    from avsep_amd import jpeg
    out = []
    for _, d in grid():
        info = jpeg.probe(d)
        out.append((info,) + jpeg_ref.decode(info, d))
    return out


def with_entropy(data, info, entropy):
    """The file ``data`` with its entropy-coded bytes replaced."""
    return data[:info.data_begin] + bytes(entropy) + data[info.data_end:]


def with_huffman_values(data, cls, value):
    """The file ``data`` with every value of its Huffman tables of class ``cls`` (0 DC, 1 AC) set to ``value``."""
    out, at = bytearray(data), 2
    while True:
        m, L = data[at + 1], struct.unpack(">H", data[at + 2:at + 4])[0]
        if m == 0xDA:
            return bytes(out)
        if m == 0xC4:
            p, end = at + 4, at + 2 + L
            while p < end:
                n = sum(data[p + 1:p + 17])
                if data[p] >> 4 == cls:
                    out[p + 17:p + 17 + n] = bytes([value]) * n
                p += 17 + n
        at += 2 + L


@functools.lru_cache(maxsize=1)
def damaged():
    """The damaged set, all of one good 33 x 65 4:2:0 file -> (the good file, [(name, bytes)])."""
    from avsep_amd import jpeg
    good = encode(picture(33, 65, seed=1), subsampling=2, quality=85)
    info = jpeg.probe(good)
    e = good[info.data_begin:info.data_end]
    flipped = bytearray(e)
    for i in range(48, len(e), 97):
        flipped[i] ^= 0xFF
    return good, [("cut at half", with_entropy(good, info, e[:len(e) // 2])),
                  ("cut one byte short", with_entropy(good, info, e[:-1])),
                  ("a flipped byte every 97", with_entropy(good, info, flipped)),
                  ("an AC run past 63", with_huffman_values(good, 1, 0xF1)),
                  ("a DC size of 15", with_huffman_values(good, 0, 15)),
                  ("a stray marker", with_entropy(good, info, e[:len(e) // 3] + b"\xff\x01" + e[len(e) // 3:]))]


def write_case(path, plan, chunk):
    """One chunk of a jpeg.plan as the case file of tests/jpeg_entropy_host.cpp."""
    images = np.ascontiguousarray(plan.images[chunk.a:chunk.b])
    with open(path, "wb") as f:
        f.write(struct.pack("<5q", len(plan.bytes), len(images), len(chunk.segs), len(plan.tables), chunk.blocks))
        for a in (plan.bytes, images, chunk.segs, plan.tables):
            f.write(np.ascontiguousarray(a).tobytes())


def read_dump(path, n_images, n_segments, blocks):
    """-> (status int32 [n_images], result int32 [n_segments], coef int16 [64 * blocks])."""
    raw = open(path, "rb").read()
    a, b = 4 * n_images, 4 * (n_images + n_segments)
    return (np.frombuffer(raw[:a], dtype=np.int32), np.frombuffer(raw[a:b], dtype=np.int32),
            np.frombuffer(raw[b:], dtype=np.int16)[:64 * blocks])
