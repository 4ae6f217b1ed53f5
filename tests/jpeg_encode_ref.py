"""The JPEG encoder's rule (include/avsep.h) restated in integer NumPy and plain Python: what
tests/test_jpeg_encode_host.py pins to Pillow's own files, and what tests/test_gpu_jpeg_encode.py holds the kernels' stage
buffers against.  A plain helper module: no fixtures, no tests.  Only the Annex K tables are shared with the package."""
import struct
from dataclasses import dataclass

import numpy as np

from avsep_amd.jpeg import STD_HUFFMAN, STD_QUANT, ZIGZAG

SAMPLING = {0: (1, 1), 1: (2, 1), 2: (2, 2), "4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2)}


def quantisers(quality, table):
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.clip((STD_QUANT[table].astype(np.int64) * scale + 50) // 100, 1, 255)                # natural order


def codes(counts, values):
    """{symbol: (code, length)} of a Huffman table."""
    c, k, out = 0, 0, {}
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            out[values[k]] = (c, length)
            k, c = k + 1, c + 1
        c <<= 1
    return out


def geometry(shape, subsampling, restart_blocks=0, restart_rows=0):
    """-> (components, hs, vs, MCUs across, MCUs down, restart interval in MCUs)."""
    ncomp = 1 if len(shape) == 2 else 3
    hs, vs = SAMPLING[subsampling] if ncomp == 3 else (1, 1)
    mcux, mcuy = -(-shape[1] // (8 * hs)), -(-shape[0] // (8 * vs))
    return ncomp, hs, vs, mcux, mcuy, (min(restart_rows * mcux, 65535) if restart_rows else restart_blocks)


def header(shape, quality, subsampling, restart_blocks=0, restart_rows=0):
    H, W = shape[:2]
    ncomp, hs, vs, _, _, restart = geometry(shape, subsampling, restart_blocks, restart_rows)

    def seg(m, body):
        return bytes([0xFF, m]) + struct.pack(">H", len(body) + 2) + body
    out = b"\xff\xd8" + seg(0xE0, bytes.fromhex("4a46494600" "0101" "00" "0001" "0001" "0000"))
    tabs = (0, 1) if ncomp == 3 else (0,)
    for t in tabs:
        out += seg(0xDB, bytes([t]) + bytes(int(v) for v in quantisers(quality, t)[ZIGZAG]))
    comps = [(1, hs * 16 + vs, 0), (2, 0x11, 1), (3, 0x11, 1)][:ncomp]
    out += seg(0xC0, struct.pack(">BHHB", 8, H, W, ncomp) + b"".join(bytes(c) for c in comps))
    for t in tabs:
        for cls in (0, 1):
            counts, values = STD_HUFFMAN[(cls, t)]
            out += seg(0xC4, bytes([cls * 16 + t]) + bytes(counts) + bytes(values))
    if restart:
        out += seg(0xDD, struct.pack(">H", restart))
    return out + seg(0xDA, bytes([ncomp]) + b"".join(bytes([c[0], c[2] * 17]) for c in comps) + bytes([0, 63, 0]))


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_pass(v, second):
    """libjpeg's islow forward pass along the last axis of v (int64 [..., 8])."""
    t0, t7, t1, t6 = v[..., 0] + v[..., 7], v[..., 0] - v[..., 7], v[..., 1] + v[..., 6], v[..., 1] - v[..., 6]
    t2, t5, t3, t4 = v[..., 2] + v[..., 5], v[..., 2] - v[..., 5], v[..., 3] + v[..., 4], v[..., 3] - v[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o = np.empty_like(v)
    n = 15 if second else 11
    o[..., 0] = _descale(t10 + t11, 2) if second else (t10 + t11) * 4
    o[..., 4] = _descale(t10 - t11, 2) if second else (t10 - t11) * 4
    z1 = (t12 + t13) * 4433
    o[..., 2], o[..., 6] = _descale(z1 + t13 * 6270, n), _descale(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = -z1 * 7373, -z2 * 20995, -z3 * 16069 + z5, -z4 * 3196 + z5
    o[..., 7], o[..., 5] = _descale(t4 + z1 + z3, n), _descale(t5 + z2 + z4, n)
    o[..., 3], o[..., 1] = _descale(t6 + z2 + z3, n), _descale(t7 + z1 + z4, n)
    return o


def _edge(p, H, W):
    return np.pad(p, ((0, H - p.shape[0]), (0, W - p.shape[1])), mode="edge")


def planes(a, hs, vs, mcuy):
    """The component planes as the DCT sees them -> [(plane int64 [mcuy*8*v, wb*8], height in blocks, width in blocks, h, v)]."""
    H, W = a.shape[:2]
    if a.ndim == 3:
        R, G, B = (a[..., k].astype(np.int64) for k in range(3))
        comps = [((19595 * R + 38470 * G + 7471 * B + 32768) >> 16, hs, vs),
                 ((-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16, 1, 1),
                 ((32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16, 1, 1)]
    else:
        comps = [(a.astype(np.int64), 1, 1)]
    out = []
    for p, h, v in comps:
        cw, ch = -(-W * h // hs), -(-H * v // vs)
        wb, hb, fh, fv = -(-cw // 8), -(-ch // 8), hs // h, vs // v
        p = _edge(p, -(-H // vs) * vs, wb * 8 * fh)                  # right: to the blocks' width; bottom: to a multiple of vmax only
        if (fh, fv) == (2, 1):
            s = p[:, 0::2] + p[:, 1::2]
            p = (s + (np.arange(s.shape[1]) & 1)) >> 1
        elif (fh, fv) == (2, 2):
            s = p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2]
            p = (s + 1 + (np.arange(s.shape[1]) & 1)) >> 2
        out.append((_edge(p, mcuy * 8 * v, p.shape[1]), hb, wb, h, v))
    return out


@dataclass
class Encoded:
    file: bytes
    coef: np.ndarray          # int16 [blocks, 64]: scan order, zig-zag inside, the dummy blocks included
    bits: np.ndarray          # int32 [blocks]
    dummy: np.ndarray         # bool [blocks]
    intervals: list           # per restart interval (first block, blocks, bytes before stuffing)


def encode(a, quality=75, subsampling=2, restart_blocks=0, restart_rows=0):
    """uint8 [H,W] or [H,W,3] -> Encoded: the whole file and what every stage of the kernels holds on the way."""
    a = np.asarray(a)
    ncomp, hs, vs, mcux, mcuy, restart = geometry(a.shape, subsampling, restart_blocks, restart_rows)
    comp = []
    for c, (p, hb, wb, h, v) in enumerate(planes(a, hs, vs, mcuy)):
        rows, cols = mcuy * v, mcux * h
        blocks = np.zeros((rows, cols, 8, 8), dtype=np.int64)
        blocks[:, :wb] = p.reshape(rows, 8, wb, 8).transpose(0, 2, 1, 3) - 128
        d = _fdct_pass(blocks, False)                                                   # rows
        d = _fdct_pass(d.swapaxes(-1, -2), True).swapaxes(-1, -2)                       # columns
        qv = quantisers(quality, 0 if c == 0 else 1).reshape(8, 8) * 8
        q = (np.abs(d) + (qv >> 1)) // qv
        q = np.where(d < 0, -q, q).reshape(rows, cols, 64)[..., ZIGZAG]
        real = np.zeros((rows, cols), dtype=bool)
        real[:hb, :wb] = True
        comp.append((q, real, h, v))
    dc_codes = [codes(*STD_HUFFMAN[(0, t)]) for t in (0, 1)]
    ac_codes = [codes(*STD_HUFFMAN[(1, t)]) for t in (0, 1)]
    coef, bits, dummy, intervals, body = [], [], [], [], bytearray()
    acc, nb, first, pred, rst = 0, 0, 0, [0] * ncomp, 0

    def put(code, length):
        nonlocal acc, nb
        acc, nb = (acc << length) | code, nb + length

    def flush():
        nonlocal acc, nb, first
        if nb & 7:
            put((1 << (8 - (nb & 7))) - 1, 8 - (nb & 7))
        raw = acc.to_bytes(nb // 8, "big")
        intervals.append((first, len(coef) - first, len(raw)))
        body.extend(raw.replace(b"\xff", b"\xff\x00"))
        acc, nb, first = 0, 0, len(coef)

    for m in range(mcux * mcuy):
        my, mx = divmod(m, mcux)
        if restart and m and m % restart == 0:
            flush()
            body.extend(bytes([0xFF, 0xD0 + rst]))
            rst, pred = (rst + 1) & 7, [0] * ncomp
        for c, (q, real, h, v) in enumerate(comp):
            t, before = (0 if c == 0 else 1), None
            for y in range(v):
                for x in range(h):
                    by, bx = my * v + y, mx * h + x
                    if real[by, bx]:
                        blk = [int(z) for z in q[by, bx]]
                    else:
                        blk = [before] + [0] * 63                                      # a dummy block: the DC of the block before it
                    before, start = blk[0], nb
                    diff, pred[c] = blk[0] - pred[c], blk[0]
                    s = abs(diff).bit_length()
                    put(*dc_codes[t][s])
                    if s:
                        put(diff if diff >= 0 else diff + (1 << s) - 1, s)
                    run = 0
                    for k in range(1, 64):
                        z = blk[k]
                        if z == 0:
                            run += 1
                            continue
                        while run > 15:
                            put(*ac_codes[t][0xF0])
                            run -= 16
                        s = abs(z).bit_length()
                        put(*ac_codes[t][(run << 4) | s])
                        put(z if z >= 0 else z + (1 << s) - 1, s)
                        run = 0
                    if run:
                        put(*ac_codes[t][0])
                    coef.append(blk)
                    bits.append(nb - start)
                    dummy.append(not real[by, bx])
    flush()
    file = header(a.shape, quality, subsampling, restart_blocks, restart_rows) + bytes(body) + b"\xff\xd9"
    return Encoded(file, np.array(coef, dtype=np.int16), np.array(bits, dtype=np.int32), np.array(dummy), intervals)
