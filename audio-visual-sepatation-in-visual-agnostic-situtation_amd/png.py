"""PNG frames decoded on the GPU (csrc/png.hip), bit for bit what ``Image.open(p).convert("RGB")`` gives.

The contract is ``jpeg.py``'s.  The host walks the chunks and checks their CRCs (``probe``), packs what the kernels read
(``plan``) and launches (``launch``): one lane per file inflates its zlib stream into the file's filtered scanlines, one
wavefront per file undoes the scanline filters in place, one lane per pixel writes RGB.  Supported is what ffmpeg, screen
recorders and Pillow write by default: bit depth 8, grey, RGB, palette, grey + alpha or RGBA (the alpha is dropped, as
``convert("RGB")`` drops it), not interlaced.  Anything else is *refused* by ``probe`` with a reason (``Unsupported``), anything a
lane cannot finish is *flagged* in a status word (``STATUS``; the lane is at least as strict as zlib), and both kinds of file are
decoded by Pillow into their slot: ``decode`` returns Pillow's pixels for every input, and a file Pillow cannot read raises as it
does there.

``decode_stack`` is the reader of a clip's folder (``frames.load_stack``): PNG files through these kernels, everything else
through ``jpeg.plan`` / ``jpeg.launch``, into one pixel buffer.  DESIGN §35."""
import io
import os
import struct
import zlib
from dataclasses import dataclass

import numpy as np
import torch

from . import jpeg
from . import kernels as K
from .lib import AvsepError, PngImage

IMAGE = np.dtype(PngImage)           # include/avsep.h: avsep_png_image
SIGNATURE = b"\x89PNG\r\n\x1a\n"
MAX_SIDE = 16384                     # csrc/png_parts.h: PN_MAX_SIDE
MAX_PIXELS = 1 << 26                 # csrc/png_parts.h: PN_MAX_PIXELS; Pillow warns of a decompression bomb above 89 478 485
WORKSPACE_CAP = 1 << 30              # bytes of filtered scanlines per chunk of images
MAX_IMAGES = 65535                   # images per chunk (a grid dimension)
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
KNOWN = (b"IHDR", b"PLTE", b"tRNS", b"IDAT", b"IEND", b"gAMA", b"cHRM", b"sRGB", b"sBIT", b"pHYs", b"tIME", b"bKGD", b"tEXt", b"eXIf")

STATUS = {1: "a read outside the stream", 2: "a zlib header other than deflate with a window of up to 32 KiB and no dictionary",
          4: "block type 3", 8: "a stored block whose LEN is not the complement of NLEN", 16: "HLIT above 286 or HDIST above 30",
          32: "a length repeat with no previous length or past the last length", 64: "an over-subscribed code set",
          128: "an incomplete code set", 256: "no end-of-block code", 512: "no code within 15 bits, or a code the set leaves unused",
          1024: "literal/length symbol 286 or 287, or distance symbol 30 or 31", 2048: "a distance beyond the bytes written",
          4096: "output past the image's scanlines", 8192: "a final block that ends short of the image's scanlines",
          16384: "bytes left after the Adler-32", 32768: "an Adler-32 that does not match", 65536: "the loop bound exceeded",
          131072: "a filter byte above 4", 262144: "a palette index at or past the entry count", 524288: "a row outside its limits"}


class Unsupported(ValueError):
    """A file outside what the kernels decode; str() is the one-line reason."""


@dataclass
class Info:
    H: int
    W: int
    colour: int                      # colour type 0 | 2 | 3 | 4 | 6
    channels: int                    # bytes per pixel
    palette: object                  # uint8 [n,3] for colour type 3, else None
    idat: bytes                      # the IDAT payloads joined: one zlib stream


def probe(data):
    """Walk the chunks of one file up to IEND -> Info; raises Unsupported with the reason for anything the kernels do not decode."""
    data = bytes(data)
    n = len(data)
    if data[:8] != SIGNATURE:
        raise Unsupported("not a PNG file: no PNG signature")
    at, head, palette, idat, state = 8, None, None, [], "before"          # state: before | in | after the IDAT chunks
    while True:
        if at == n:
            raise Unsupported("no IEND chunk")
        if at + 12 > n:
            raise Unsupported("the file ends inside a chunk")
        length, kind = struct.unpack(">I", data[at:at + 4])[0], data[at + 4:at + 8]
        if at + 12 + length > n:
            raise Unsupported("the file ends inside a chunk")
        body = data[at + 8:at + 8 + length]
        name = kind.decode("latin-1")
        if zlib.crc32(data[at + 4:at + 8 + length]) != struct.unpack(">I", data[at + 8 + length:at + 12 + length])[0]:
            raise Unsupported(f"chunk {name!r} at byte {at}: its CRC does not match")
        at += 12 + length
        if kind == b"acTL":
            raise Unsupported("an animated PNG (acTL)")
        if kind not in KNOWN:
            raise Unsupported(f"chunk {name!r}: left to Pillow")
        if (head is None) != (kind == b"IHDR"):
            raise Unsupported("chunks out of order: IHDR is not the first chunk" if head is None else "chunks out of order: a second IHDR")
        if kind != b"IDAT" and state == "in":
            state = "after"
        if kind == b"IHDR":
            if length != 13:
                raise Unsupported("a malformed IHDR chunk")
            W, H, depth, colour, compression, method, interlace = struct.unpack(">IIBBBBB", body)
            if colour not in CHANNELS:
                raise Unsupported(f"colour type {colour}")
            if depth != 8:
                raise Unsupported(f"bit depth {depth}")
            if compression != 0 or method != 0:
                raise Unsupported(f"compression method {compression}, filter method {method}")
            if interlace != 0:
                raise Unsupported("Adam7 interlace" if interlace == 1 else f"interlace method {interlace}")
            if H == 0 or W == 0:
                raise Unsupported(f"a frame of {H} x {W}")
            if H > MAX_SIDE or W > MAX_SIDE:
                raise Unsupported(f"a frame of {H} x {W}: sides above {MAX_SIDE}")
            if H * W > MAX_PIXELS:
                raise Unsupported(f"a frame of {H} x {W}: more than {MAX_PIXELS} pixels")
            head = (H, W, colour)
        elif kind == b"PLTE":
            if palette is not None or state != "before":
                raise Unsupported("chunks out of order: a second PLTE" if palette is not None else "chunks out of order: PLTE after IDAT")
            if length % 3 or not 1 <= length // 3 <= 256:
                raise Unsupported(f"a PLTE chunk of {length} bytes")
            palette = np.frombuffer(body, dtype=np.uint8).reshape(-1, 3)
        elif kind == b"IDAT":
            if state == "after":
                raise Unsupported("chunks out of order: IDAT chunks that are not consecutive")
            if head[2] == 3 and palette is None:
                raise Unsupported("a palette image without a PLTE chunk before its IDAT")
            state = "in"
            idat.append(body)
        elif kind == b"IEND":
            if state == "before":
                raise Unsupported("IEND before any IDAT chunk")
            break
    H, W, colour = head
    return Info(H, W, colour, CHANNELS[colour], palette if colour == 3 else None, b"".join(idat))


def scanline_bytes(info):
    """The bytes of a probed file's filtered scanlines: what its zlib stream inflates to."""
    return info.H * (1 + info.W * info.channels)


class Chunk:
    """The images [a, b) of a plan that share one scanline workspace: their rows (``images``, a view; ws_off counts from 0 in the
    chunk), the workspace's bytes and the most pixels any one image has (the launch grid)."""

    def __init__(self, a, b, images, ws_bytes, max_pixels):
        self.a, self.b, self.images, self.ws_bytes, self.max_pixels = a, b, images, ws_bytes, max_pixels


class DecodePlan:
    """What the kernels read for a list of files: see ``plan``."""

    def __init__(self, data, images, index, chunks, tables, fallback, reasons, shapes, offsets, pixel_bytes):
        self.bytes, self.images, self.index, self.chunks, self.tables = data, images, index, chunks, tables
        self.fallback, self.reasons, self.shapes, self.offsets, self.pixel_bytes = fallback, reasons, shapes, offsets, pixel_bytes


def plan(files, cap=WORKSPACE_CAP):
    """Pack what the kernels read for ``files`` (a list of bytes) -> DecodePlan:
    bytes: the zlib streams of the supported files back to back (uint8);
    images: one IMAGE row per supported file (``index`` = its position in ``files``): sizes, colour type, channels, palette
      offset and entry count, the byte range of its stream, ws_off = its scanlines in its chunk's workspace, pix_off;
    chunks: the images cut so that a chunk's scanline workspace stays within ``cap`` bytes;
    tables: the palettes, 3 bytes per entry, in one uint8 buffer, equal palettes stored once;
    fallback: the indices of files ``probe`` (or the cap) refused, ``reasons`` why; their sizes come from Pillow;
    shapes, offsets, pixel_bytes: every file's (H, W) and its first byte in the output, all frames back to back."""
    files = [bytes(f) for f in files]
    if not files:
        raise AvsepError("png.plan takes at least one file")
    if int(cap) < 1:
        raise AvsepError(f"png.plan takes a workspace cap of at least 1 byte, got {cap!r}")
    shapes, fallback, reasons, kept = [], [], {}, []
    for i, f in enumerate(files):
        try:
            info = probe(f)
            if scanline_bytes(info) > int(cap):
                raise Unsupported(f"{scanline_bytes(info)} bytes of scanlines, more than the workspace cap of {int(cap)}")
            kept.append((i, info))
            shapes.append((info.H, info.W))
        except Unsupported as e:
            from PIL import Image
            fallback.append(i)
            reasons[i] = str(e)
            w, h = Image.open(io.BytesIO(f)).size
            shapes.append((h, w))
    offsets = np.concatenate([[0], np.cumsum([h * w * 3 for h, w in shapes], dtype=np.int64)])
    rows = np.zeros(len(kept), dtype=IMAGE)
    palettes, where, table_bytes, data, nbytes = [], {}, 0, [], 0
    for r, (i, info) in enumerate(kept):
        rows[r]["pix_off"], rows[r]["H"], rows[r]["W"] = offsets[i], info.H, info.W
        rows[r]["colour"], rows[r]["channels"] = info.colour, info.channels
        rows[r]["begin"], rows[r]["end"] = nbytes, nbytes + len(info.idat)
        data.append(np.frombuffer(info.idat, dtype=np.uint8))
        nbytes += len(info.idat)
        if info.palette is not None:
            key = info.palette.tobytes()
            if key not in where:
                where[key] = table_bytes
                palettes.append(info.palette.reshape(-1))
                table_bytes += len(key)
            rows[r]["palette"], rows[r]["entries"] = where[key], len(info.palette)
    need = [scanline_bytes(info) for _, info in kept]
    chunks = []
    for a, b in jpeg._cut(need, int(cap), MAX_IMAGES):
        rows["ws_off"][a:b] = np.cumsum([0] + need[a:b - 1], dtype=np.int64)
        chunks.append(Chunk(a, b, rows[a:b], int(sum(need[a:b])), max(info.H * info.W for _, info in kept[a:b])))
    data = np.concatenate(data) if data else np.zeros(0, dtype=np.uint8)
    tables = np.concatenate(palettes) if palettes else np.zeros(0, dtype=np.uint8)
    p = DecodePlan(data, rows, [i for i, _ in kept], chunks, tables, fallback, reasons, shapes, offsets, int(offsets[-1]))
    _check(p)
    return p


def _check(p):
    for ch in p.chunks:
        K.png_plan_check(ch.images, max(len(p.bytes), 1), max(len(p.tables), 1), p.pixel_bytes, ch.ws_bytes)


def rebase(p, offsets, pixel_bytes):
    """Move a plan into a pixel buffer it shares with other decoders: file i of the plan starts at offsets[i] of a buffer of
    pixel_bytes bytes.  The rows are checked again against the new size."""
    p.offsets, p.pixel_bytes = np.asarray(offsets, dtype=np.int64), int(pixel_bytes)
    p.images["pix_off"] = [p.offsets[i] for i in p.index]
    _check(p)


def launch(p, device, pixels=None, ws=None):
    """Upload a plan and run its chunks on the current stream of ``device`` -> (pixels uint8 [bytes], status int32 [images] on
    the device, the scanline workspace as the last chunk left it).  Nothing is read back.  pixels and ws (uint8), when given,
    are the buffers to use: the plan's bytes, and the largest chunk's ws_bytes.  Per chunk: avsep_png_inflate, then
    avsep_png_pixels (unfilter in place, colour)."""
    device = torch.device(device)
    if pixels is None:
        pixels = torch.empty(p.pixel_bytes, dtype=torch.uint8, device=device)
    status = torch.zeros(max(len(p.images), 1), dtype=torch.int32, device=device)
    if p.chunks:
        data = torch.from_numpy(p.bytes if len(p.bytes) else np.zeros(1, dtype=np.uint8)).to(device, non_blocking=True)
        tables = torch.from_numpy(p.tables if len(p.tables) else np.zeros(1, dtype=np.uint8)).to(device, non_blocking=True)
        images = torch.from_numpy(p.images.view(np.uint8)).to(device, non_blocking=True)
        ws = torch.empty(max(ch.ws_bytes for ch in p.chunks), dtype=torch.uint8, device=device) if ws is None else ws
        for ch in p.chunks:
            rows = images[ch.a * IMAGE.itemsize:ch.b * IMAGE.itemsize]
            st = status[ch.a:ch.b]
            K.png_inflate(data, rows, ws, ch.ws_bytes, st)
            K.png_pixels(ws, ch.ws_bytes, rows, ch.max_pixels, tables, st, pixels)
    return pixels, status, ws


def decode(files, device, cap=WORKSPACE_CAP, decoded=None):
    """files: a list of bytes, each one image file -> (pixels uint8 [bytes] on ``device``, every frame [H,W,3] back to back in
    file order, and shapes [(H, W)]).  Supported files are decoded by the kernels; the status words are read once, and every
    refused or flagged file is decoded by Pillow and copied into its slot, so the result is Pillow's for every input.
    ``decoded`` {index: uint8 [H,W,3]} hands over pixels the caller already has for refused files."""
    files = [bytes(f) for f in files]
    p = plan(files, cap)
    pixels, status, _ = launch(p, device)
    jpeg.fill_from_pillow(pixels, files, p.fallback + flagged(p, status), p.shapes, p.offsets, decoded, "png.decode")
    return pixels, list(p.shapes)


def flagged(p, status):
    """The files (indices) of a launched plan whose status word is set; this reads the words back."""
    if not len(p.images):
        return []
    return [p.index[r] for r in np.flatnonzero(status.cpu().numpy()[:len(p.images)])]


def decode_stack(paths, device):
    """The image files ``paths`` of one clip -> uint8 [T,H,W,3] on ``device``.  A file that starts with the PNG signature goes to
    the PNG kernels, every other file through ``jpeg.plan`` / ``jpeg.launch`` (baseline and progressive JPEGs), both into one
    pixel buffer; what neither takes, and what a lane flags, is decoded by Pillow.  Frames of unequal size end with SystemExit,
    as in ``frames.load_stack``."""
    paths = list(paths)
    files = []
    for q in paths:
        with open(q, "rb") as f:
            files.append(f.read())
    if not files:
        raise AvsepError("png.decode_stack takes at least one file")
    groups = [[i for i, f in enumerate(files) if (f[:8] == SIGNATURE) == is_png] for is_png in (True, False)]
    plans = [(plan if is_png else lambda fs: jpeg.plan(fs, progressive=True))([files[i] for i in idx]) if idx else None
             for is_png, idx in zip((True, False), groups)]
    shapes = [None] * len(files)
    for idx, p in zip(groups, plans):
        for k, i in enumerate(idx):
            shapes[i] = tuple(p.shapes[k])
    for q, s in zip(paths, shapes):
        if s != shapes[0]:
            raise SystemExit(f"{os.path.dirname(q)}: frames of unequal size: {os.path.basename(q)} is {s[0]} x {s[1]}, "
                             f"{os.path.basename(paths[0])} is {shapes[0][0]} x {shapes[0][1]}")
    frame = shapes[0][0] * shapes[0][1] * 3
    offsets = np.arange(len(files) + 1, dtype=np.int64) * frame
    pixels = torch.empty(int(offsets[-1]), dtype=torch.uint8, device=torch.device(device))
    again = []
    for idx, p, mod in zip(groups, plans, (None, jpeg)):
        if p is None:
            continue
        (rebase if mod is None else jpeg.rebase)(p, np.append(offsets[idx], offsets[-1]), int(offsets[-1]))
        status = (launch if mod is None else jpeg.launch)(p, device, pixels)[1]
        again += [idx[k] for k in p.fallback + flagged(p, status)]
    jpeg.fill_from_pillow(pixels, files, again, shapes, offsets, None, "png.decode_stack")
    return pixels.view(len(paths), shapes[0][0], shapes[0][1], 3)
