"""Baseline JPEG frames decoded on the GPU (csrc/jpeg.hip), bit for bit what ``Image.open(p).convert("RGB")`` gives.

The host reads the markers (``probe``), packs what the kernels read (``plan``) and launches (``decode``): one lane per
entropy-coded segment decodes the Huffman stream into an int16 coefficient workspace, then one kernel dequantises and inverts
the DCT (libjpeg's "islow" integers) and one upsamples the chroma ("fancy") and converts to RGB.  Supported is what ffmpeg and
Pillow write by default: SOF0, 8 bit, Huffman, one interleaved scan, grey or YCbCr at 4:4:4, 4:2:2 (2x1) or 4:2:0 (2x2), with or
without restart intervals.  Anything else is *refused* by ``probe`` with a reason (``Unsupported``), anything a lane cannot decode
is *flagged* in a status word, and both kinds of file are decoded by Pillow into their slot: ``decode`` returns Pillow's pixels
for every input, and a file Pillow cannot read raises as it does there.

The output layout is the one ``frames.plan_batch`` takes: every frame [H,W,3] uint8, back to back, in file order."""
import io
import os
import struct
from dataclasses import dataclass

import numpy as np
import torch

from . import kernels as K
from .lib import AvsepError, JpegImage, JpegSegment

IMAGE = np.dtype(JpegImage)          # include/avsep.h: avsep_jpeg_image
SEGMENT = np.dtype(JpegSegment)      # include/avsep.h: avsep_jpeg_segment
MAX_SIDE = 16384                     # csrc/jpeg_parts.h: JP_MAX_SIDE
HUFF_WORDS = 256 + 17 + 17 + 256     # look-ahead, maxcode, value offset, values (csrc/jpeg_parts.h: JP_HUFF_WORDS)
QUANT_WORDS = 64
WORKSPACE_CAP = 1 << 30              # bytes of int16 coefficients per chunk of images (the uint8 planes add half as much)
BLOCK_BYTES = 128                    # 64 int16
MAX_IMAGES = 65535                   # images per chunk (a grid dimension)

# natural (row-major) index of zig-zag position k
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                   28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
                   54, 47, 55, 62, 63])

STATUS = {1: "a read outside the segment", 2: "no Huffman code within 16 bits", 4: "a DC size above 11",
          8: "a coefficient index past 63", 16: "a marker inside the segment", 32: "a block outside the segment's blocks",
          64: "a table outside the table buffer", 128: "a coefficient beyond the 32-bit bound", 256: "a row outside its limits",
          512: "bytes left over after the last block"}


class Unsupported(ValueError):
    """A file outside what the kernels decode; str() is the one-line reason."""


@dataclass
class Info:
    H: int
    W: int
    components: list                 # per component (id, h, v, quantisation-table index)
    qtables: dict                    # index -> uint8 [64], zig-zag order
    huffman: dict                    # (class 0 = DC | 1 = AC, index) -> (counts uint8 [16], values uint8 [n])
    restart: int                     # MCUs per restart interval, 0 = none
    scan: list                       # per component (DC table index, AC table index)
    data_begin: int                  # the entropy-coded bytes are data[data_begin:data_end]; data_end is the EOI marker
    data_end: int


_SOF_NAMES = {0xC1: "extended sequential (SOF1)", 0xC2: "progressive (SOF2)", 0xC3: "lossless (SOF3)"}


def probe(data):
    """Walk the markers of one file up to SOS -> Info; raises Unsupported with the reason for anything the kernels do not decode."""
    data = bytes(data)
    n = len(data)
    if n < 4 or data[0:2] != b"\xff\xd8":
        raise Unsupported("not a JPEG file: no SOI marker")
    at, frame, qt, huff, restart, jfif, adobe = 2, None, {}, {}, 0, False, None
    while True:
        if at + 2 > n:
            raise Unsupported("the file ends before its SOS marker")
        if data[at] != 0xFF:
            raise Unsupported(f"byte {at}: 0x{data[at]:02x} where a marker starts")
        m = data[at + 1]
        if m == 0xFF:                                # fill byte
            at += 1
            continue
        at += 2
        if m == 0x01 or 0xD0 <= m <= 0xD7:           # stand-alone
            continue
        if m == 0xD9:
            raise Unsupported("EOI before any scan")
        if at + 2 > n:
            raise Unsupported("the file ends before its SOS marker")
        L = struct.unpack(">H", data[at:at + 2])[0]
        if L < 2 or at + L > n:
            raise Unsupported("the file ends before its SOS marker" if at + L > n else f"marker 0x{m:02x} of length {L}")
        body = data[at + 2:at + L]
        if m == 0xDA:
            break
        at += L
        if m == 0xC0:
            if frame is not None:
                raise Unsupported("more than one frame header")
            if len(body) < 6 or len(body) != 6 + 3 * body[5]:
                raise Unsupported("a malformed SOF0 marker")
            P, H, W, nf = body[0], struct.unpack(">H", body[1:3])[0], struct.unpack(">H", body[3:5])[0], body[5]
            if P != 8:
                raise Unsupported(f"{P}-bit samples")
            frame = (H, W, [(body[6 + 3 * i], body[7 + 3 * i] >> 4, body[7 + 3 * i] & 15, body[8 + 3 * i]) for i in range(nf)])
        elif m in _SOF_NAMES or (0xC5 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC)):
            raise Unsupported(_SOF_NAMES.get(m, f"SOF{m - 0xC0} (differential or arithmetic-coded)"))
        elif m == 0xCC:
            raise Unsupported("arithmetic coding (DAC)")
        elif m == 0xDC:
            raise Unsupported("a DNL marker")
        elif m == 0xDB:
            p = 0
            while p < len(body):
                if body[p] >> 4:
                    raise Unsupported("a 16-bit quantisation table")
                if (body[p] & 15) > 3 or p + 65 > len(body):
                    raise Unsupported("a malformed DQT marker")
                qt[body[p] & 15] = np.frombuffer(body[p + 1:p + 65], dtype=np.uint8)
                p += 65
        elif m == 0xC4:
            p = 0
            while p < len(body):
                if p + 17 > len(body) or (body[p] >> 4) > 1 or (body[p] & 15) > 3:
                    raise Unsupported("a malformed DHT marker")
                counts = np.frombuffer(body[p + 1:p + 17], dtype=np.uint8)
                total = int(counts.sum())
                if total > 256 or p + 17 + total > len(body):
                    raise Unsupported("a malformed DHT marker")
                code = 0
                for length, c in enumerate(counts, 1):               # the codes of a length must fit that length
                    code += int(c)
                    if code > (1 << length):
                        raise Unsupported("a Huffman table with more codes than a length holds")
                    code <<= 1
                huff[(body[p] >> 4, body[p] & 15)] = (counts, np.frombuffer(body[p + 17:p + 17 + total], dtype=np.uint8))
                p += 17 + total
        elif m == 0xDD:
            if len(body) != 2:
                raise Unsupported("a malformed DRI marker")
            restart = struct.unpack(">H", body)[0]
        elif m == 0xE0 and body[:5] == b"JFIF\0":
            jfif = True
        elif m == 0xEE and body[:5] == b"Adobe" and len(body) >= 12:
            adobe = body[11]
        # any other APPn, COM: skipped
    if frame is None:
        raise Unsupported("SOS before a frame header")
    H, W, comps = frame
    if H == 0 or W == 0:
        raise Unsupported(f"a frame of {H} x {W}")
    if H > MAX_SIDE or W > MAX_SIDE:
        raise Unsupported(f"a frame of {H} x {W}: sides above {MAX_SIDE}")
    if len(comps) not in (1, 3):
        raise Unsupported(f"{len(comps)} components")
    if len(comps) == 3:
        if adobe is not None and adobe != 1:
            raise Unsupported(f"Adobe colour transform {adobe}")
        ids = tuple(c[0] for c in comps)
        if ids != (1, 2, 3):
            raise Unsupported(f"three components with ids {ids}" + ("" if jfif or adobe is not None else
                                                                    " and neither a JFIF nor an Adobe marker"))
        if (comps[1][1], comps[1][2], comps[2][1], comps[2][2]) != (1, 1, 1, 1):
            raise Unsupported("chroma sampling other than 1x1")
        if (comps[0][1], comps[0][2]) not in ((1, 1), (2, 1), (2, 2)):
            raise Unsupported(f"luma sampling {comps[0][1]}x{comps[0][2]}")
    else:
        comps = [(comps[0][0], 1, 1, comps[0][3])]   # one component: not interleaved, its factors do not count
    if len(body) < 1 or len(body) != 4 + 2 * body[0]:
        raise Unsupported("a malformed SOS marker")
    if body[0] != len(comps):
        raise Unsupported("more than one scan")
    scan = []
    for i, c in enumerate(comps):
        if body[1 + 2 * i] != c[0]:
            raise Unsupported("scan components out of frame order")
        scan.append((body[2 + 2 * i] >> 4, body[2 + 2 * i] & 15))
    ss, se, a = body[-3], body[-2], body[-1]
    if (ss, se, a) != (0, 63, 0):
        raise Unsupported(f"a scan with Ss={ss}, Se={se}, Ah={a >> 4}, Al={a & 15}")
    for c, (d, a) in zip(comps, scan):
        if c[3] not in qt:
            raise Unsupported(f"quantisation table {c[3]} is referenced but not defined")
        for cls, idx in ((0, d), (1, a)):
            if (cls, idx) not in huff:
                raise Unsupported(f"{'AD'[cls]}C Huffman table {idx} is referenced but not defined")
    begin = at + L
    # the scan ends at the first marker that is neither a stuffed FF 00, a fill FF FF nor RSTn: it must be EOI
    b = np.frombuffer(data, dtype=np.uint8)[begin:]
    nxt = b[1:]
    hits = np.flatnonzero((b[:-1] == 0xFF) & (nxt != 0) & (nxt != 0xFF) & ((nxt < 0xD0) | (nxt > 0xD7))) if len(b) > 1 else []
    end = None
    for p in hits:
        m = int(b[p + 1])
        if m == 0xD9:
            end = begin + int(p)
            break
        if m == 0xDC:
            raise Unsupported("a DNL marker")
        if m in (0xDA, 0xC4, 0xDB, 0xDD) or 0xC0 <= m <= 0xCF:
            raise Unsupported("more than one scan")
        # any other marker inside the scan is left to the lane that meets it
    if end is None:
        raise Unsupported("no EOI marker")
    return Info(H, W, comps, qt, huff, restart, scan, begin, end)


def geometry(info):
    """-> (hs, vs, MCUs across, MCUs down, blocks) of a probed file."""
    hs, vs = info.components[0][1], info.components[0][2]
    mcux, mcuy = -(-info.W // (8 * hs)), -(-info.H // (8 * vs))
    return hs, vs, mcux, mcuy, mcux * mcuy * (hs * vs + len(info.components) - 1)


def segments(info, data):
    """The entropy-coded segments of a probed file -> [(begin, end, first MCU, MCUs)], from a search for the RSTn markers.
    Unsupported when the markers do not match the restart interval."""
    hs, vs, mcux, mcuy, _ = geometry(info)
    a = np.frombuffer(data, dtype=np.uint8)[info.data_begin:info.data_end]
    at = np.flatnonzero((a[:-1] == 0xFF) & (a[1:] >= 0xD0) & (a[1:] <= 0xD7)) if len(a) > 1 else np.zeros(0, dtype=np.int64)
    total = mcux * mcuy
    per = info.restart if info.restart else total
    want = -(-total // per)
    if len(at) != want - 1:
        raise Unsupported(f"{len(at)} restart markers where the interval of {info.restart} MCUs asks for {want - 1}")
    if len(at) and not np.array_equal(a[at + 1] - 0xD0, np.arange(len(at)) % 8):
        raise Unsupported("restart markers out of order")
    begins = np.concatenate([[0], at + 2]) + info.data_begin
    ends = np.concatenate([at, [len(a)]]) + info.data_begin
    return [(int(b), int(e), k * per, min(per, total - k * per)) for k, (b, e) in enumerate(zip(begins, ends))]


def huffman_words(counts, values):
    """One Huffman table as the kernels read it -> int32 [HUFF_WORDS]: look[256] ((length << 8) | value for codes of up to 8
    bits, by the next 8 bits; 0 = longer), maxcode[17] (by length; -1 = no code of that length), valoff[17] (index of a code's
    value = valoff[length] + code), values[256]."""
    w = np.zeros(HUFF_WORDS, dtype=np.int32)
    look, maxcode, valoff, vals = w[:256], w[256:273], w[273:290], w[290:]
    maxcode[:] = -1
    vals[:len(values)] = values
    code, k = 0, 0
    for length in range(1, 17):
        c = int(counts[length - 1])
        if c:
            valoff[length] = k - code
            if length <= 8:
                for i in range(c):
                    lo = (code + i) << (8 - length)
                    look[lo:lo + (1 << (8 - length))] = (length << 8) | int(values[k + i])
            code, k = code + c, k + c
            maxcode[length] = code - 1
        code <<= 1
    return w


class Chunk:
    """The images [a, b) of a plan's rows that share one coefficient workspace: their segment rows (image indices count from
    a), the blocks they need, and the most blocks and pixels any one of them has (the launch grids)."""

    def __init__(self, a, b, segs, blocks, max_blocks, max_pixels):
        self.a, self.b, self.segs, self.blocks, self.max_blocks, self.max_pixels = a, b, segs, blocks, max_blocks, max_pixels


class DecodePlan:
    """What the kernels read for a list of files: see ``plan``."""

    def __init__(self, data, images, index, chunks, tables, fallback, reasons, shapes, offsets, pixel_bytes):
        self.bytes, self.images, self.index, self.chunks, self.tables = data, images, index, chunks, tables
        self.fallback, self.reasons, self.shapes, self.offsets, self.pixel_bytes = fallback, reasons, shapes, offsets, pixel_bytes


def _pillow(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"), dtype=np.uint8)


def plan(files, cap=WORKSPACE_CAP):
    """Pack what the kernels read for ``files`` (a list of bytes) -> DecodePlan:
    bytes: the entropy-coded bytes of the supported files back to back (uint8);
    images: one IMAGE row per supported file (``index`` = its position in ``files``), block offsets counted per chunk;
    chunks: the images cut so that a chunk's coefficient workspace stays within ``cap`` bytes, each with its SEGMENT rows;
    tables: quantisation tables (64 words, natural order) and Huffman tables (``huffman_words``) in one int32 buffer, equal
      tables shared;
    fallback: the indices of files ``probe`` (or the limits here) refused, ``reasons`` why; their sizes come from Pillow;
    shapes, offsets, pixel_bytes: every file's (H, W) and its first byte in the output, all frames back to back."""
    files = [bytes(f) for f in files]
    if not files:
        raise AvsepError("jpeg.plan takes at least one file")
    cap_blocks = int(cap) // BLOCK_BYTES
    if cap_blocks < 1:
        raise AvsepError(f"jpeg.plan takes a workspace cap of at least {BLOCK_BYTES} bytes, got {cap!r}")
    shapes, fallback, reasons, kept = [], [], {}, []
    for i, f in enumerate(files):
        try:
            info = probe(f)
            segs = segments(info, f)
            if geometry(info)[4] > cap_blocks:
                raise Unsupported(f"{geometry(info)[4]} blocks, more than the workspace cap of {cap_blocks}")
            kept.append((i, info, segs))
            shapes.append((info.H, info.W))
        except Unsupported as e:
            from PIL import Image
            fallback.append(i)
            reasons[i] = str(e)
            w, h = Image.open(io.BytesIO(f)).size
            shapes.append((h, w))
    offsets = np.concatenate([[0], np.cumsum([h * w * 3 for h, w in shapes], dtype=np.int64)])
    parts, where, words = [], {}, 0

    def table(key, make):
        nonlocal words
        if key not in where:
            t = make()
            where[key] = words
            parts.append(t)
            words += len(t)
        return where[key]

    images = np.zeros(len(kept), dtype=IMAGE)
    chunks, data, nbytes = [], [], 0
    a, block0, segs_rows, max_blocks, max_pixels = 0, 0, [], 0, 0
    # chunks of about equal size: as few as the cap allows, none of them a small remainder
    total = sum(geometry(info)[4] for _, info, _ in kept)
    target = -(-total // max(1, -(-total // cap_blocks)))
    for r, (i, info, segs) in enumerate(kept):
        hs, vs, mcux, mcuy, blocks = geometry(info)
        if block0 and (block0 + blocks > cap_blocks or block0 >= target or r - a >= MAX_IMAGES):
            chunks.append(Chunk(a, r, np.array(segs_rows, dtype=SEGMENT), block0, max_blocks, max_pixels))
            a, block0, segs_rows, max_blocks, max_pixels = r, 0, [], 0, 0
        row = images[r]
        row["pix_off"], row["block0"], row["H"], row["W"], row["ncomp"] = offsets[i], block0, info.H, info.W, len(info.components)
        row["hs"], row["vs"], row["mcux"], row["mcuy"], row["restart"] = hs, vs, mcux, mcuy, info.restart
        for c, (comp, (d, ac)) in enumerate(zip(info.components, info.scan)):
            q = info.qtables[comp[3]]

            def natural(q=q):
                t = np.zeros(64, dtype=np.int32)
                t[ZIGZAG] = q
                return t
            row["quant"][c] = table(("q", q.tobytes()), natural)
            for name, cls, idx in (("dc", 0, d), ("ac", 1, ac)):
                counts, values = info.huffman[(cls, idx)]
                row[name][c] = table(("h", counts.tobytes(), values.tobytes()), lambda: huffman_words(counts, values))
        shift = nbytes - info.data_begin
        segs_rows += [(b + shift, e + shift, r - a, m0, n, 0) for b, e, m0, n in segs]
        data.append(np.frombuffer(files[i], dtype=np.uint8)[info.data_begin:info.data_end])
        nbytes += info.data_end - info.data_begin
        block0 += blocks
        max_blocks, max_pixels = max(max_blocks, blocks), max(max_pixels, info.H * info.W)
    if kept:
        chunks.append(Chunk(a, len(kept), np.array(segs_rows, dtype=SEGMENT), block0, max_blocks, max_pixels))
    data = np.concatenate(data) if data else np.zeros(0, dtype=np.uint8)
    tables = np.concatenate(parts) if parts else np.zeros(0, dtype=np.int32)
    p = DecodePlan(data, images, [i for i, _, _ in kept], chunks, tables, fallback, reasons, shapes, offsets, int(offsets[-1]))
    for ch in chunks:
        K.jpeg_plan_check(images[ch.a:ch.b], ch.segs, max(len(data), 1), len(tables), p.pixel_bytes, ch.blocks)
    return p


def launch(p, device, pixels=None, coef=None, planes=None):
    """Upload a plan and run its chunks on the current stream of ``device`` -> (pixels uint8 [bytes], status int32 [images] on the
    device, the coefficient workspace and planes as the last chunk left them).  Nothing is read back.  pixels, coef (int16) and
    planes (uint8), when given, are the buffers to use: the plan's bytes, and 64 per block of the largest chunk."""
    device = torch.device(device)
    if pixels is None:
        pixels = torch.empty(p.pixel_bytes, dtype=torch.uint8, device=device)
    status = torch.zeros(max(len(p.images), 1), dtype=torch.int32, device=device)
    if p.chunks:
        data = torch.from_numpy(p.bytes).to(device, non_blocking=True)
        tables = torch.from_numpy(p.tables).to(device, non_blocking=True)
        images = torch.from_numpy(p.images.view(np.uint8)).to(device, non_blocking=True)
        blocks = max(ch.blocks for ch in p.chunks)
        coef = torch.empty(blocks * 64, dtype=torch.int16, device=device) if coef is None else coef
        planes = torch.empty(blocks * 64, dtype=torch.uint8, device=device) if planes is None else planes
        for ch in p.chunks:
            rows = images[ch.a * IMAGE.itemsize:ch.b * IMAGE.itemsize]
            segs = torch.from_numpy(ch.segs.view(np.uint8)).to(device, non_blocking=True)
            st = status[ch.a:ch.b]
            K.jpeg_entropy(data, rows, segs, tables, coef, ch.blocks, st)
            K.jpeg_pixels(coef, planes, ch.blocks, rows, ch.max_blocks, ch.max_pixels, tables, st, pixels)
    return pixels, status, coef, planes


def decode(files, device, cap=WORKSPACE_CAP, decoded=None):
    """files: a list of bytes, each one image file -> (pixels uint8 [bytes] on ``device``, every frame [H,W,3] back to back in
    file order, and shapes [(H, W)]).  Supported files are decoded by the kernels; the status words are read once, and every
    refused or flagged file is decoded by Pillow and copied into its slot, so the result is Pillow's for every input.
    ``decoded`` {index: uint8 [H,W,3]} hands over pixels the caller already has for refused files."""
    files = [bytes(f) for f in files]
    p = plan(files, cap)
    pixels, status, _, _ = launch(p, device)
    again = list(p.fallback)
    if len(p.images):
        st = status.cpu().numpy()
        again += [p.index[r] for r in np.flatnonzero(st[:len(p.images)])]
    for i in sorted(again):
        a = decoded[i] if decoded is not None and i in decoded else _pillow(files[i])
        if a.shape != p.shapes[i] + (3,):
            raise AvsepError(f"jpeg.decode: file {i} is {p.shapes[i]} by its header and {a.shape[:2]} once decoded")
        pixels[int(p.offsets[i]):int(p.offsets[i + 1])] = torch.from_numpy(np.array(a)).reshape(-1).to(pixels.device)
    return pixels, list(p.shapes)


def decode_stack(paths, device):
    """The image files ``paths`` of one clip -> uint8 [T,H,W,3] on ``device``: baseline JPEGs through the kernels, everything else
    through Pillow.  Frames of unequal size end with SystemExit, as in ``frames.load_stack``."""
    paths = list(paths)
    files = []
    for q in paths:
        with open(q, "rb") as f:
            files.append(f.read())
    pixels, shapes = decode(files, device)
    for q, s in zip(paths, shapes):
        if s != shapes[0]:
            raise SystemExit(f"{os.path.dirname(q)}: frames of unequal size: {os.path.basename(q)} is {s[0]} x {s[1]}, "
                             f"{os.path.basename(paths[0])} is {shapes[0][0]} x {shapes[0][1]}")
    return pixels.view(len(paths), shapes[0][0], shapes[0][1], 3)
