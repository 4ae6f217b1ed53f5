"""not-gpu: the host side of the GPU PNG decoder.  The restatement (tests/png_ref.py) equals Pillow byte for byte on the grid of
sizes, colour types, filters and deflate forms; png.probe reads the chunks and refuses, with the reason, what the kernels do not
decode; png.plan packs streams, shared palettes and offsets, and avsep_png_plan_check refuses every range outside its buffer; and
the lane bodies themselves (csrc/png_parts.h), compiled with the host compiler under the address and undefined-behaviour
sanitizers into a stand-alone program, decode the grid to the restatement's pixels and never hand back pixels for a stream zlib
or Pillow rejects.  tests/test_gpu_png.py holds the kernels against Pillow."""
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

import avsep_amd as P
from avsep_amd import jpeg
from avsep_amd import png

import png_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement against Pillow ------------------------------------------------------------------------------------
def test_restatement_equals_pillow_on_the_grid():
    files, ref = PC.grid(), PC.grid_reference()
    assert len(files) == 49 and len({n for n, _ in files}) == 49
    for (name, d), px in zip(files, ref):
        assert np.array_equal(px, PC.pillow(d)), name
    # every pairing of two axes' values is in the grid
    axes = [(a, b, (a + b) % 7 % 6, (a + 2 * b) % 7 % 6) for a in range(7) for b in range(7)]
    for i, ni in enumerate((7, 7, 6, 6)):
        for j, nj in enumerate((7, 7, 6, 6)):
            if i < j:
                assert {(t[i], t[j]) for t in axes} == {(u, v) for u in range(ni) for v in range(nj)}


def test_deflate_forms_are_what_they_claim():
    """Level 0 is stored blocks, Z_FIXED a fixed block, the rest dynamic ones."""
    raw = PC.filter_rows(PC.picture(17, 33), [0] * 17)
    kinds = {name: (PC.deflate(raw, level, strategy)[2] >> 1) & 3 for name, level, strategy in PC.DEFLATES}
    assert kinds == {"stored": 0, "fixed": 1, "6": 2, "9": 2, "rle": 2, "huffman": 2}


# ---- probe -------------------------------------------------------------------------------------------------------------
def test_probe_fields():
    px, plte = PC.source(5, 7, 3)
    d = PC.write_png(px, 3, "cycle", plte=plte, trns=bytes(5), split=3, empties=True,
                     before=[PC.chunk(b"gAMA", struct.pack(">I", 45455))], after=[PC.chunk(b"tEXt", b"k\0v"), PC.chunk(b"tIME", bytes(7))])
    info = png.probe(d)
    assert (info.H, info.W, info.colour, info.channels) == (5, 7, 3, 1)
    assert info.palette.dtype == np.uint8 and np.array_equal(info.palette, plte)
    assert zlib.decompress(info.idat) == PC.filter_rows(px, [0, 1, 2, 3, 4]) and png.scanline_bytes(info) == 5 * 8
    for colour, ch in PC.CHANNELS.items():
        if colour != 3:
            i = png.probe(PC.write_png(PC.picture(3, 4, ch), colour, 1))
            assert (i.H, i.W, i.colour, i.channels, i.palette) == (3, 4, colour, ch, None)
    # a suggested palette in an RGB file is read past; bytes after IEND are not the file's
    rgb = PC.write_png(PC.picture(3, 4), 2, 0, plte=plte)
    assert png.probe(rgb).palette is None and png.probe(rgb + b"junk").idat == png.probe(rgb).idat


def _flip_crc(data, kind):
    at = data.index(kind) + 4 + struct.unpack(">I", data[data.index(kind) - 4:data.index(kind)])[0]
    return data[:at] + bytes([data[at] ^ 1]) + data[at + 1:]


def test_probe_refuses_with_the_reason():
    px = PC.picture(4, 6)
    good = PC.write_png(px, 2, 0, after=[PC.chunk(b"tEXt", b"k\0v")])
    stream = PC.deflate(PC.filter_rows(px, [0] * 4))
    idat, iend, ihdr = PC.chunk(b"IDAT", stream), PC.chunk(b"IEND"), good[8:33]
    plte = PC.chunk(b"PLTE", bytes(9))
    cases = [(jpeg.encode_header((4, 6, 3)), "not a PNG file"),
             (_flip_crc(good, b"IDAT"), "'IDAT'.*CRC does not match"),
             (_flip_crc(good, b"tEXt"), "'tEXt'.*CRC does not match"),
             (_flip_crc(good, b"IHDR"), "'IHDR'.*CRC does not match")]
    cases += [(PC.wrap(stream, 4, 6, 2, depth=depth), f"bit depth {depth}") for depth in (1, 2, 4, 16)]
    cases += [(PC.wrap(stream, 4, 6, 2, interlace=1), "Adam7 interlace"),
              (PC.wrap(stream, 4, 6, 2, before=[PC.chunk(b"acTL", bytes(8))]), "animated PNG"),
              (PC.wrap(stream, 4, 6, 2, before=[PC.chunk(b"iCCP", b"x\0\0" + zlib.compress(b"p"))]), "chunk 'iCCP'"),
              (PC.wrap(stream, 4, 6, 2, before=[PC.chunk(b"zTXt", b"k\0\0" + zlib.compress(b"v"))]), "chunk 'zTXt'"),
              (PC.wrap(stream, 4, 6, 3, plte=np.zeros(4, dtype=np.uint8)), "PLTE chunk of 4 bytes"),
              (PC.wrap(stream, 4, 6, 3), "without a PLTE"),
              (PC.wrap(stream, 4, 6, 5), "colour type 5"),
              (PC.SIGNATURE + plte + ihdr + idat + iend, "out of order: IHDR is not the first"),
              (PC.SIGNATURE + ihdr + ihdr + idat + iend, "out of order: a second IHDR"),
              (PC.SIGNATURE + ihdr + idat + plte + iend, "out of order: PLTE after IDAT"),
              (PC.SIGNATURE + ihdr + idat + PC.chunk(b"tEXt", b"k\0v") + idat + iend, "out of order: IDAT chunks that are not consecutive"),
              (PC.SIGNATURE + ihdr + iend, "IEND before any IDAT"),
              (PC.wrap(stream, 4, 16385, 2), "sides above 16384"),
              (PC.wrap(stream, 16384, 8192, 2), "more than 67108864 pixels"),
              (PC.wrap(stream, 0, 6, 2), "a frame of 0 x 6"),
              (good[:-12], "no IEND chunk"),
              (good[:-5], "ends inside a chunk"),
              (good[:60], "ends inside a chunk")]
    for d, reason in cases:
        with pytest.raises(png.Unsupported, match=reason):
            png.probe(d)
    assert png.probe(PC.wrap(stream, 8192, 8192, 2)).H == 8192                                   # the limit itself is taken
    assert isinstance(png.Unsupported("x"), ValueError) and "\n" not in str(png.Unsupported("one line"))
    assert sorted(png.STATUS) == [1 << k for k in range(20)]


# ---- plan --------------------------------------------------------------------------------------------------------------
def _three():
    px, plte = PC.source(5, 7, 3)
    a = PC.write_png(PC.picture(9, 4), 2, "cycle")
    b = PC.write_png(px, 3, 4, plte=plte)
    c = PC.write_png(PC.source(17, 33, 3, seed=5)[0], 3, 1, plte=plte, trns=bytes(3))
    d = PC.write_png(PC.picture(3, 3, 2), 4, 2)
    return a, b, c, d, plte


def test_plan_streams_palettes_and_offsets():
    a, b, c, d, plte = _three()
    lace = PC.wrap(png.probe(a).idat, 9, 4, 2, interlace=1)
    p = png.plan([a, lace, b, c, d])
    assert p.fallback == [1] and "Adam7" in p.reasons[1] and p.index == [0, 2, 3, 4]
    assert p.shapes == [(9, 4), (9, 4), (5, 7), (17, 33), (3, 3)]
    assert p.offsets.tolist() == np.concatenate([[0], np.cumsum([108, 108, 105, 1683, 27])]).tolist() and p.pixel_bytes == 2031
    assert p.images["pix_off"].tolist() == [0, 216, 321, 2004]
    streams = [png.probe(f).idat for f in (a, b, c, d)]
    assert bytes(p.bytes) == b"".join(streams)
    assert p.images["begin"].tolist() == np.cumsum([0] + [len(s) for s in streams[:-1]]).tolist()
    assert (p.images["end"] - p.images["begin"]).tolist() == [len(s) for s in streams]
    need = [9 * 13, 5 * 8, 17 * 34, 3 * 7]
    assert p.images["ws_off"].tolist() == np.cumsum([0] + need[:-1]).tolist() and len(p.chunks) == 1
    assert (p.chunks[0].ws_bytes, p.chunks[0].max_pixels) == (sum(need), 17 * 33)
    assert p.images["colour"].tolist() == [2, 3, 3, 4] and p.images["channels"].tolist() == [3, 1, 1, 2]
    # equal palettes are stored once
    assert bytes(p.tables) == plte.tobytes() and p.images["palette"].tolist() == [0, 0, 0, 0]
    assert p.images["entries"].tolist() == [0, PC.PALETTE_ENTRIES, PC.PALETTE_ENTRIES, 0]
    other = PC.write_png(PC.source(5, 7, 3)[0], 3, 0, plte=PC.palette(40, seed=9))
    q = png.plan([b, other, c])
    assert q.images["palette"].tolist() == [0, 3 * PC.PALETTE_ENTRIES, 0] and len(q.tables) == 3 * (PC.PALETTE_ENTRIES + 40)
    # a tiny cap gives chunks, each counting its workspace from 0; a file above the cap on its own is Pillow's
    small = png.plan([a, b, c, d], cap=600)
    assert [(ch.a, ch.b, ch.ws_bytes) for ch in small.chunks] == [(0, 2, 157), (2, 3, 578), (3, 4, 21)]
    assert small.images["ws_off"].tolist() == [0, 117, 0, 0]
    tiny = png.plan([a, b, c, d], cap=500)
    assert tiny.fallback == [2] and "workspace cap" in tiny.reasons[2] and tiny.index == [0, 1, 3]
    with pytest.raises(jpeg.Unsupported, match="not a JPEG"):
        jpeg.probe(a)


def test_plan_check_refusals():
    L = P.lib.load()
    a, b, c, d, _ = _three()
    p = png.plan([a, b, c, d])
    ch = p.chunks[0]

    def check(images=None, **kw):
        images = np.ascontiguousarray(p.images if images is None else images)
        v = dict(nbytes=len(p.bytes), tables=len(p.tables), pixels=p.pixel_bytes, ws=ch.ws_bytes)
        v.update(kw)
        return L.avsep_png_plan_check(images.ctypes.data, len(images), *v.values())

    assert check() == 0
    for kw in (dict(nbytes=len(p.bytes) - 1), dict(tables=len(p.tables) - 1), dict(pixels=p.pixel_bytes - 1), dict(ws=ch.ws_bytes - 1),
               dict(nbytes=0), dict(tables=0), dict(pixels=0), dict(ws=0)):
        assert check(**kw) == -1, kw
    for field, row, value in (("H", 0, 0), ("W", 0, 0), ("H", 0, 16385), ("W", 3, 16385), ("colour", 0, 1), ("colour", 0, 6),
                              ("channels", 0, 4), ("channels", 1, 3), ("colour", 1, 0), ("entries", 1, 0), ("entries", 1, 257),
                              ("entries", 0, 1), ("palette", 0, 3), ("palette", 1, -1), ("palette", 2, 1), ("pix_off", 3, -1),
                              ("pix_off", 3, 2005), ("ws_off", 3, 736), ("ws_off", 0, -1), ("begin", 0, -1),
                              ("end", 3, len(p.bytes) + 1), ("end", 2, int(p.images["begin"][2]) - 1)):
        im = p.images.copy()
        im[field][row] = value
        assert check(images=im) == -1, (field, row, value)
    big = p.images.copy()                                                                         # H * W above 2^26
    big["H"][0], big["W"][0] = 16384, 8192
    assert check(images=big, pixels=1 << 40, ws=1 << 40) == -1
    big["W"][0] = 4096
    assert check(images=big, pixels=1 << 40, ws=1 << 40) == 0
    assert L.avsep_png_plan_check(None, 1, 1, 1, 1, 1) == -1
    with pytest.raises(P.lib.AvsepError, match="avsep_png_plan_check refused"):
        P.kernels.png_plan_check(p.images, len(p.bytes), len(p.tables), p.pixel_bytes, ch.ws_bytes - 1)
    assert np.dtype(P.lib.PngImage).itemsize == 64


# ---- the lane bodies on the CPU, under the sanitizers ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "the no-false-accept test needs a host C++ compiler"
    exe = str(tmp_path_factory.mktemp("png_host") / "png_inflate_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(os.path.dirname(P.lib.LIB_PATH), "csrc"),
                    os.path.join(ROOT, "tests", "png_inflate_host.cpp"), "-o", exe], check=True)
    return exe


def _run(exe, tmp_path, p):
    """Every chunk of a plan through the host program -> (status [images], pixels [bytes])."""
    status, pixels = [], np.full(p.pixel_bytes, 0xA5, dtype=np.uint8)
    for ch in p.chunks:
        case, dump = str(tmp_path / "case.bin"), str(tmp_path / "dump.bin")
        PC.write_case(case, p, ch)
        r = subprocess.run([exe, case, dump], capture_output=True, text=True)
        assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
        st, px = PC.read_dump(dump, ch.b - ch.a, p.pixel_bytes)
        status.append(st)
        pixels = np.where(px != 0xA5, px, pixels)
    return np.concatenate(status), pixels


def _slot(pixels, p, i):
    H, W = p.shapes[i]
    return pixels[int(p.offsets[i]):int(p.offsets[i + 1])].reshape(H, W, 3)


def test_host_program_decodes_the_grid(host_program, tmp_path):
    """Also what a decoder that flags everything fails: nothing of the grid is refused and every status word is 0."""
    files = PC.grid()
    p = png.plan([d for _, d in files])
    assert p.fallback == [] and len(p.chunks) == 1 and len(p.images) == 49
    status, pixels = _run(host_program, tmp_path, p)
    assert not status.any(), [(n, s) for (n, _), s in zip(files, status) if s]
    for i, ((name, _), px) in enumerate(zip(files, PC.grid_reference())):
        assert np.array_equal(_slot(pixels, p, i), px), name
    px, stream = PC.window_stream()                                                               # distance 32 768, and chunks
    q = png.plan([PC.wrap(stream, 10, 1365, 2, split=1, empties=True)], cap=40960)
    status, pixels = _run(host_program, tmp_path, q)
    assert zlib.decompress(stream) == PC.filter_rows(px, [0] * 10) and not status.any() and np.array_equal(_slot(pixels, q, 0), px)


def _pillow_or_none(d):
    try:
        return PC.pillow(d)
    except Exception:
        return None


def _zlib_ok(d):
    try:
        zlib.decompress(png.probe(d).idat)
        return True
    except zlib.error:
        return False


def test_no_false_accept(host_program, tmp_path):
    """For every crafted stream and every single-bit flip: status 0 only if zlib takes the stream and Pillow's pixels are the
    program's; a stream zlib rejects has a status bit."""
    crafted = PC.crafted()
    flips = PC.bit_flips(300)
    assert len(flips) == 900
    files = [d for _, d, _ in crafted] + [d for _, d in flips]
    names = [n for n, _, _ in crafted] + [n for n, _ in flips]
    p = png.plan(files)
    assert p.fallback == [], p.reasons                    # every file passes the chunk walk: it is the lane that meets the damage
    status, pixels = _run(host_program, tmp_path, p)
    for (name, _, bit), st in zip(crafted, status):
        assert st in png.STATUS or st == 0, (name, st)
        assert (st == bit) if bit is not None else (st != 0), (name, st)
    accepted = 0
    for i, (name, d) in enumerate(zip(names, files)):
        ok = _zlib_ok(d)
        if status[i] == 0:
            want = _pillow_or_none(d)
            assert ok and want is not None and np.array_equal(_slot(pixels, p, i), want), name
            accepted += 1
        assert ok or status[i] != 0, name
    assert 2 <= accepted < len(files)


def test_rows_the_lane_must_not_trust(host_program, tmp_path):
    """Each bad row stops the lane with the row bit, and nothing out of range is touched (the sanitizers watch)."""
    a, b, c, d, _ = _three()
    for field, row, value in (("ws_off", 3, 737), ("H", 0, 0), ("W", 2, 0), ("channels", 1, 2), ("entries", 1, 300), ("begin", 1, -1)):
        q = png.plan([a, b, c, d])
        q.images[field][row] = value
        status, _ = _run(host_program, tmp_path, q)
        assert status[row] == 524288 and not np.delete(status, row).any(), (field, status)
    q = png.plan([a, b, c, d])
    q.images["end"][3] = len(q.bytes) + 1
    assert _run(host_program, tmp_path, q)[0].tolist() == [0, 0, 0, 1]
    q = png.plan([a, b, c, d])
    q.images["pix_off"][3] = q.pixel_bytes - 26
    assert _run(host_program, tmp_path, q)[0].tolist() == [0, 0, 0, 524288]
