"""Baseline JPEG frames decoded on the GPU (csrc/jpeg.hip), bit for bit what ``Image.open(p).convert("RGB")`` gives.

The host reads the markers (``probe``), packs what the kernels read (``plan``) and launches (``decode``): one lane per
entropy-coded segment decodes the Huffman stream into an int16 coefficient workspace, then one kernel dequantises and inverts
the DCT (libjpeg's "islow" integers) and one upsamples the chroma ("fancy") and converts to RGB.  Supported is what ffmpeg and
Pillow write by default: SOF0, 8 bit, Huffman, one interleaved scan, grey or YCbCr at 4:4:4, 4:2:2 (2x1) or 4:2:0 (2x2), with or
without restart intervals.  Anything else is *refused* by ``probe`` with a reason (``Unsupported``), anything a lane cannot decode
is *flagged* in a status word, and both kinds of file are decoded by Pillow into their slot: ``decode`` returns Pillow's pixels
for every input, and a file Pillow cannot read raises as it does there.

With ``progressive=True`` (what the ``--gpu_decode`` paths pass) progressive files (SOF2) are decoded too: ``probe_scans`` reads
every scan, ``plan`` adds one SCAN row per scan and restart interval, and the scans of a file run as lanes of their own, level
after level (csrc/jpeg_parts.h: jp_decode_scan), into the same workspace and the same pixel stage.

The output layout is the one ``frames.plan_batch`` takes: every frame [H,W,3] uint8, back to back, in file order.
PNG files are not this module's: ``plan`` refuses them as "not a JPEG", and ``png.decode_stack`` (what ``frames.load_stack``
calls) sends them to the kernels of csrc/png.hip and everything else here.

The way back (csrc/jpeg_enc.hip): ``encode`` writes uint8 pictures on the device as baseline JPEG files, byte for byte the files
Pillow's ``save`` writes; ``encode_header`` / ``encode_plan`` / ``encode_launch`` are its parts.  See the second half of this file.
Both planners lay pictures out through the same pieces: ``Form``, ``Tables``, ``_cut``, ``_rows`` and ``Chunk``, over one IMAGE row."""
import io
import os
import struct
from collections import namedtuple
from dataclasses import dataclass

import numpy as np
import torch

from . import kernels as K
from .lib import AvsepError, JpegImage, JpegScan, JpegSegment, got

IMAGE = np.dtype(JpegImage)          # include/avsep.h: avsep_jpeg_image, the row of both directions
SEGMENT = np.dtype(JpegSegment)      # include/avsep.h: avsep_jpeg_segment
SCAN = np.dtype(JpegScan)            # include/avsep.h: avsep_jpeg_scan, one (scan, restart interval) of a progressive file
MAX_SCANS = 64                       # include/avsep.h: AVSEP_JPEG_MAX_SCANS, scans per progressive file
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
          512: "bytes left over after the last block", 1024: "a refinement symbol of a size other than 0 or 1",
          2048: "an end-of-band run past the segment's blocks"}


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


def _read_dqt(body, qt):
    """The tables of one DQT marker into qt {index: uint8 [64], zig-zag order}."""
    p = 0
    while p < len(body):
        if body[p] >> 4:
            raise Unsupported("a 16-bit quantisation table")
        if (body[p] & 15) > 3 or p + 65 > len(body):
            raise Unsupported("a malformed DQT marker")
        qt[body[p] & 15] = np.frombuffer(body[p + 1:p + 65], dtype=np.uint8)
        p += 65


def _read_dht(body, huff):
    """The tables of one DHT marker into huff {(class, index): (counts uint8 [16], values)}."""
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


def _frame_rules(frame, jfif, adobe):
    """The frame header (H, W, components) against what the kernels decode -> (H, W, components as the readers return them)."""
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
    return H, W, comps


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
            _read_dqt(body, qt)
        elif m == 0xC4:
            _read_dht(body, huff)
        elif m == 0xDD:
            if len(body) != 2:
                raise Unsupported("a malformed DRI marker")
            restart = struct.unpack(">H", body)[0]
        elif m == 0xE0 and body[:5] == b"JFIF\0":
            jfif = True
        elif m == 0xEE and body[:5] == b"Adobe" and len(body) >= 12:
            adobe = body[11]
        # any other APPn, COM: skipped
    H, W, comps = _frame_rules(frame, jfif, adobe)
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


class Form(namedtuple("Form", "H W ncomp hs vs mcux mcuy restart")):
    """One picture as both directions lay it out: its size, components (1 | 3), luma sampling, MCUs across and down, and MCUs
    per restart interval (0 = none).  ``of`` counts the MCUs; restart_rows = MCU rows per interval, which win, as in libjpeg."""
    __slots__ = ()

    @classmethod
    def of(cls, H, W, ncomp, hs, vs, restart, restart_rows=0):
        mcux = -(-W // (8 * hs))
        return cls(H, W, ncomp, hs, vs, mcux, -(-H // (8 * vs)), min(restart_rows * mcux, 65535) if restart_rows else restart)

    @property
    def blocks(self):
        return self.mcux * self.mcuy * (self.hs * self.vs + self.ncomp - 1)

    @property
    def intervals(self):
        return -(-(self.mcux * self.mcuy) // self.restart) if self.restart else 1


def _form(info):
    return Form.of(info.H, info.W, len(info.components), info.components[0][1], info.components[0][2], info.restart)


def geometry(info):
    """-> (hs, vs, MCUs across, MCUs down, blocks) of a probed file."""
    f = _form(info)
    return f.hs, f.vs, f.mcux, f.mcuy, f.blocks


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


@dataclass
class Scan:
    """One scan of a progressive file, as its SOS header and the markers before it give it."""
    comps: list                      # indices of its components in the frame, rising
    ss: int                          # the band of zig-zag positions [ss, se] ...
    se: int
    ah: int                          # ... and the bit positions: ah = 0 a first scan, else a refinement down to al = ah - 1
    al: int
    tables: list                     # per component (counts, values) of the DC (ss = 0) or AC table in force; None when DC is refined
    restart: int                     # units per restart interval in force, 0 = none
    begin: int                       # the entropy-coded bytes are data[begin:end]; end is the next marker
    end: int
    rst: np.ndarray                  # where in the file its RSTn markers stand
    units: int                       # MCUs (several components) or the component's own blocks over its real size (one)
    level: int                       # 1 + the highest level of an earlier scan with a component and a coefficient in common; else 0


@dataclass
class ScanInfo:
    H: int
    W: int
    components: list                 # as Info's
    qtables: dict
    scans: list                      # Scan, in file order
    restart = 0                      # the image row of a progressive file has none: every scan row carries its own units


def _scan_units(H, W, comps, which):
    """The units of a scan over the components ``which`` (indices): MCUs, or one component's blocks over its real size."""
    hs, vs = comps[0][1], comps[0][2]
    if len(which) > 1:
        return -(-W // (8 * hs)) * -(-H // (8 * vs))
    cw, ch = (W, H) if which[0] == 0 else (-(-W // hs), -(-H // vs))
    return -(-cw // 8) * -(-ch // 8)


def probe_scans(data):
    """Walk every marker of a progressive (SOF2) file from SOI to EOI -> ScanInfo; raises Unsupported with the reason for anything
    outside what avsep_jpeg_scans decodes: the baseline limits on the frame, T.81 G.1.1.1's rules for every scan, a complete
    progression (every coefficient of every component down to Al = 0 at EOI: libjpeg smooths an incomplete one, the kernels do
    not), no quantisation table after the first scan, at most MAX_SCANS scans, restart markers that match each scan's interval."""
    data = bytes(data)
    n = len(data)
    if n < 4 or data[0:2] != b"\xff\xd8":
        raise Unsupported("not a JPEG file: no SOI marker")
    a = np.frombuffer(data, dtype=np.uint8)
    ff = np.flatnonzero(a[:-1] == 0xFF)
    nxt = a[ff + 1]
    is_rst = (nxt >= 0xD0) & (nxt <= 0xD7)
    # RSTn; what ends a scan's bytes: the next marker with a meaning (a stray TEM, FF 01, is left to the lane that meets it)
    rst_at, stop_at = ff[is_rst], ff[(nxt > 1) & (nxt != 0xFF) & ~is_rst]
    at, frame, qt, huff, restart, jfif, adobe = 2, None, {}, {}, 0, False, None
    H = W = comps = state = None
    scans = []
    while True:
        if at + 2 > n:
            raise Unsupported("no EOI marker")
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
            break
        if at + 2 > n:
            raise Unsupported("no EOI marker")
        L = struct.unpack(">H", data[at:at + 2])[0]
        if L < 2 or at + L > n:
            raise Unsupported("no EOI marker" if at + L > n else f"marker 0x{m:02x} of length {L}")
        body = data[at + 2:at + L]
        at += L
        if m == 0xC2:
            if frame is not None:
                raise Unsupported("more than one frame header")
            if len(body) < 6 or len(body) != 6 + 3 * body[5]:
                raise Unsupported("a malformed SOF2 marker")
            if body[0] != 8:
                raise Unsupported(f"{body[0]}-bit samples")
            frame = (struct.unpack(">H", body[1:3])[0], struct.unpack(">H", body[3:5])[0],
                     [(body[6 + 3 * i], body[7 + 3 * i] >> 4, body[7 + 3 * i] & 15, body[8 + 3 * i]) for i in range(body[5])])
        elif m == 0xC0:
            raise Unsupported("not progressive: a baseline frame (SOF0)")
        elif m in _SOF_NAMES or (0xC5 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC)):
            raise Unsupported(_SOF_NAMES.get(m, f"SOF{m - 0xC0} (differential or arithmetic-coded)"))
        elif m == 0xCC:
            raise Unsupported("arithmetic coding (DAC)")
        elif m == 0xDC:
            raise Unsupported("a DNL marker")
        elif m == 0xDB:
            if scans:
                raise Unsupported("a quantisation table after the first scan")
            _read_dqt(body, qt)
        elif m == 0xC4:
            _read_dht(body, huff)
        elif m == 0xDD:
            if len(body) != 2:
                raise Unsupported("a malformed DRI marker")
            restart = struct.unpack(">H", body)[0]
        elif m == 0xE0 and body[:5] == b"JFIF\0":
            jfif = True
        elif m == 0xEE and body[:5] == b"Adobe" and len(body) >= 12:
            adobe = body[11]
        elif m == 0xDA:
            if state is None:
                H, W, comps = _frame_rules(frame, jfif, adobe)
                for c in comps:
                    if c[3] not in qt:
                        raise Unsupported(f"quantisation table {c[3]} is referenced but not defined")
                state = [[-1] * 64 for _ in comps]               # per component and coefficient: the Al reached, -1 = untouched
            if len(scans) >= MAX_SCANS:
                raise Unsupported(f"more than {MAX_SCANS} scans")
            if len(body) < 1 or len(body) != 4 + 2 * body[0] or not 1 <= body[0] <= len(comps):
                raise Unsupported("a malformed SOS marker")
            ids = [c[0] for c in comps]
            which = [ids.index(body[1 + 2 * i]) if body[1 + 2 * i] in ids else -1 for i in range(body[0])]
            if -1 in which:
                raise Unsupported("a scan component the frame does not have")
            if any(y <= x for x, y in zip(which, which[1:])):
                raise Unsupported("scan components out of frame order")
            ss, se, ah, al = body[-3], body[-2], body[-1] >> 4, body[-1] & 15
            what = f"a scan with Ss={ss}, Se={se}, Ah={ah}, Al={al}"
            if (ss == 0 and se != 0) or (ss > 0 and not ss <= se <= 63):
                raise Unsupported(f"{what}: a band outside T.81 G.1.1.1")
            if ss > 0 and len(which) != 1:
                raise Unsupported(f"{what} over {len(which)} components: an AC scan takes one")
            if ah > 13 or al > 13:
                raise Unsupported(f"{what}: a bit position above 13")
            for c in which:
                if ss > 0 and state[c][0] < 0:
                    raise Unsupported(f"{what}: AC of component {c} before its DC")
                for k in range(ss, se + 1):
                    if (ah != 0) if state[c][k] < 0 else (ah != state[c][k] or al != ah - 1):
                        raise Unsupported(f"{what}: coefficient {k} of component {c} " +
                                          ("has no first scan" if state[c][k] < 0 else f"stands at Al={state[c][k]}"))
                    state[c][k] = al
            chosen = []
            for i, c in enumerate(which):
                cls, idx = (0, body[2 + 2 * i] >> 4) if ss == 0 else (1, body[2 + 2 * i] & 15)
                if ss == 0 and ah != 0:
                    chosen.append(None)
                    continue
                if (cls, idx) not in huff:
                    raise Unsupported(f"{'AD'[cls]}C Huffman table {idx} is referenced but not defined")
                chosen.append(huff[cls, idx])
            begin = at
            j = int(np.searchsorted(stop_at, begin))
            if j == len(stop_at):
                raise Unsupported("no EOI marker")
            end = int(stop_at[j])
            rst = rst_at[np.searchsorted(rst_at, begin):np.searchsorted(rst_at, end)]
            units = _scan_units(H, W, comps, which)
            want = -(-units // restart) if restart else 1
            if len(rst) != want - 1:
                raise Unsupported(f"scan {len(scans)}: {len(rst)} restart markers where the interval of {restart} units asks for {want - 1}")
            if len(rst) and not np.array_equal(a[rst + 1] - 0xD0, np.arange(len(rst)) % 8):
                raise Unsupported("restart markers out of order")
            level = 1 + max((s.level for s in scans if set(s.comps) & set(which) and s.ss <= se and ss <= s.se), default=-1)
            scans.append(Scan(which, ss, se, ah, al, chosen, restart, begin, end, rst, units, level))
            at = end
        # any other APPn, COM: skipped
    if not scans:
        raise Unsupported("EOI before any scan")
    for c, st in enumerate(state):
        if any(v != 0 for v in st):
            k = next(k for k, v in enumerate(st) if v != 0)
            raise Unsupported(f"an incomplete progression: coefficient {k} of component {c} " +
                              ("has no scan" if st[k] < 0 else f"ends at Al={st[k]}"))
    return ScanInfo(H, W, comps, qt, scans)


def scan_segments(scan):
    """The entropy-coded segments of one scan -> [(begin, end, first unit, units)], cut at its RSTn markers."""
    per = scan.restart if scan.restart else scan.units
    begins = [scan.begin] + [int(p) + 2 for p in scan.rst]
    ends = [int(p) for p in scan.rst] + [scan.end]
    return [(b, e, k * per, min(per, scan.units - k * per)) for k, (b, e) in enumerate(zip(begins, ends))]


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


class Tables:
    """Tables interned into one int32 buffer: ``at(key, make, *args)`` -> the word offset of the table of ``key``, which
    ``make(*args)`` gives the first time the key is seen; ``buffer()`` -> all of them back to back."""

    def __init__(self):
        self.parts, self.where, self.words = [], {}, 0

    def at(self, key, make, *args):
        if key not in self.where:
            t = np.asarray(make(*args), dtype=np.int32)
            self.where[key] = self.words
            self.parts.append(t)
            self.words += len(t)
        return self.where[key]

    def buffer(self):
        return np.concatenate(self.parts) if self.parts else np.zeros(0, dtype=np.int32)


class Chunk:
    """The images [a, b) of a plan that share one coefficient workspace: their rows (``images``, a view; blocks and intervals
    count from 0 in the chunk) and how many blocks and restart intervals they have.  ``plan`` adds what decoding needs: the
    SEGMENT rows of its baseline images and the SCAN rows of its progressive ones, in rising order of level (image indices
    count from a), ``levels`` = [(level, first row, end row)] of those, one launch each, and the most blocks and pixels any one
    image has (the launch grids)."""

    def __init__(self, a, b, images, blocks, intervals):
        self.a, self.b, self.images, self.blocks, self.intervals = a, b, images, blocks, intervals
        self.segs, self.scans, self.levels, self.max_blocks, self.max_pixels = None, None, [], 0, 0


def _cap_blocks(who, cap):
    if int(cap) // BLOCK_BYTES < 1:
        raise AvsepError(f"{who} takes a workspace cap of at least {BLOCK_BYTES} bytes, got {cap!r}")
    return int(cap) // BLOCK_BYTES


def _cut(blocks, cap_blocks, most):
    """Images of ``blocks`` blocks each (none above cap_blocks) -> the ranges [(a, b)] that share a workspace of at most
    cap_blocks blocks and ``most`` images: chunks of about equal size, as few as the cap allows, none of them a small remainder."""
    total = sum(blocks)
    target = -(-total // max(1, -(-total // cap_blocks)))
    cuts, a, block0 = [], 0, 0
    for r, nb in enumerate(blocks):
        if block0 and (block0 + nb > cap_blocks or block0 >= target or r - a >= most):
            cuts.append((a, r))
            a, block0 = r, 0
        block0 += nb
    return cuts + [(a, len(blocks))] if blocks else cuts


def _rows(forms, pix_off, table_off, cuts):
    """One IMAGE row per form -> (rows, [Chunk]).  pix_off: every image's first byte in the pixel buffer; table_off: per image
    and component the word offsets (quantiser, DC table, AC table); block0 and interval0 count from 0 in each range of ``cuts``."""
    rows = np.zeros(len(forms), dtype=IMAGE)
    rows["pix_off"] = pix_off
    for name, column in zip(Form._fields, zip(*forms)):
        rows[name] = column
    for r, t in enumerate(table_off):
        rows["quant"][r, :len(t)], rows["dc"][r, :len(t)], rows["ac"][r, :len(t)] = zip(*t)
    counts = np.array([(f.blocks, f.intervals) for f in forms], dtype=np.int64).reshape(-1, 2)
    before = np.cumsum(counts, axis=0) - counts                              # blocks and intervals before an image, over all rows
    chunks = []
    for a, b in cuts:
        rows["block0"][a:b], rows["interval0"][a:b] = (before[a:b] - before[a]).T
        chunks.append(Chunk(a, b, rows[a:b], *(int(v) for v in counts[a:b].sum(axis=0))))
    return rows, chunks


class DecodePlan:
    """What the kernels read for a list of files: see ``plan``."""

    def __init__(self, data, images, index, chunks, tables, fallback, reasons, shapes, offsets, pixel_bytes):
        self.bytes, self.images, self.index, self.chunks, self.tables = data, images, index, chunks, tables
        self.fallback, self.reasons, self.shapes, self.offsets, self.pixel_bytes = fallback, reasons, shapes, offsets, pixel_bytes


def _pillow(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"), dtype=np.uint8)


def _natural(q):
    t = np.zeros(64, dtype=np.int32)
    t[ZIGZAG] = q
    return t


def _read(f, cap_blocks, progressive):
    """One file for ``plan`` -> (Info, its segments, Form), or (ScanInfo, None, Form) for a progressive file when those are
    taken; Unsupported otherwise."""
    try:
        info = probe(f)
        segs = segments(info, f)
    except Unsupported as e:
        if not progressive or str(e) != _SOF_NAMES[0xC2]:
            raise
        info, segs = probe_scans(f), None
    form = _form(info)
    if form.blocks > cap_blocks:
        raise Unsupported(f"{form.blocks} blocks, more than the workspace cap of {cap_blocks}")
    return info, segs, form


def plan(files, cap=WORKSPACE_CAP, progressive=False):
    """Pack what the kernels read for ``files`` (a list of bytes) -> DecodePlan:
    bytes: the entropy-coded bytes of the supported files back to back (uint8);
    images: one IMAGE row per supported file (``index`` = its position in ``files``), block offsets counted per chunk and
      interval0 = the image's first row in its chunk's segments;
    chunks: the images cut so that a chunk's coefficient workspace stays within ``cap`` bytes, each with its SEGMENT rows;
    tables: quantisation tables (64 words, natural order) and Huffman tables (``huffman_words``) in one int32 buffer, equal
      tables shared;
    fallback: the indices of files ``probe`` (or the limits here) refused, ``reasons`` why; their sizes come from Pillow;
    shapes, offsets, pixel_bytes: every file's (H, W) and its first byte in the output, all frames back to back.
    progressive: a file ``probe`` refuses as progressive (SOF2) is read by ``probe_scans``; one it takes gets an IMAGE row like
      any other (dc / ac: its first DC table, restart 0) and, in its chunk's ``scans``, one SCAN row per (scan, restart interval)
      with the tables, band, units and level of that scan, the rows of a chunk in rising order of level.  Its bytes in ``bytes``
      are its scans' entropy-coded bytes back to back."""
    files = [bytes(f) for f in files]
    if not files:
        raise AvsepError("jpeg.plan takes at least one file")
    cap_blocks = _cap_blocks("jpeg.plan", cap)
    shapes, fallback, reasons, kept, forms = [], [], {}, [], []
    for i, f in enumerate(files):
        try:
            info, segs, form = _read(f, cap_blocks, progressive)
            kept.append((i, info, segs))
            forms.append(form)
            shapes.append((info.H, info.W))
        except Unsupported as e:
            from PIL import Image
            fallback.append(i)
            reasons[i] = str(e)
            w, h = Image.open(io.BytesIO(f)).size
            shapes.append((h, w))
    offsets = np.concatenate([[0], np.cumsum([h * w * 3 for h, w in shapes], dtype=np.int64)])
    tables = Tables()

    def huffman_at(table):
        return tables.at(("h", table[0].tobytes(), table[1].tobytes()), huffman_words, *table)

    def tables_of(info):
        if isinstance(info, ScanInfo):               # the scan rows carry the tables: the image row points at a valid one
            pairs = [(info.scans[0].tables[0],) * 2] * len(info.components)
        else:
            pairs = [(info.huffman[0, d], info.huffman[1, ac]) for d, ac in info.scan]
        for comp, pair in zip(info.components, pairs):
            q = info.qtables[comp[3]]
            yield [tables.at(("q", q.tobytes()), _natural, q)] + [huffman_at(t) for t in pair]
    images, chunks = _rows(forms, [offsets[i] for i, _, _ in kept], [list(tables_of(info)) for _, info, _ in kept],
                           _cut([f.blocks for f in forms], cap_blocks, MAX_IMAGES))
    data, nbytes = [], 0
    for ch in chunks:
        segs_rows, scan_rows = [], []
        for r in range(ch.a, ch.b):
            i, info, segs = kept[r]
            if segs is None:
                for s in info.scans:
                    shift = nbytes - s.begin
                    at = [huffman_at(s.tables[s.comps.index(c)]) if c in s.comps and s.tables[s.comps.index(c)] is not None else 0
                          for c in range(3)]
                    scan_rows += [(b + shift, e + shift, r - ch.a, sum(1 << c for c in s.comps), s.ss, s.se, s.ah, s.al, at, u0, n,
                                   s.level, (0, 0)) for b, e, u0, n in scan_segments(s)]
                    data.append(np.frombuffer(files[i], dtype=np.uint8)[s.begin:s.end])
                    nbytes += s.end - s.begin
                continue
            shift = nbytes - info.data_begin
            segs_rows += [(b + shift, e + shift, r - ch.a, m0, n, 0) for b, e, m0, n in segs]
            data.append(np.frombuffer(files[i], dtype=np.uint8)[info.data_begin:info.data_end])
            nbytes += info.data_end - info.data_begin
        ch.segs = np.array(segs_rows, dtype=SEGMENT)
        ch.scans = np.array(scan_rows, dtype=SCAN)
        ch.scans = ch.scans[np.argsort(ch.scans["level"], kind="stable")]
        levels, first = np.unique(ch.scans["level"], return_index=True)
        ch.levels = list(zip(levels.tolist(), first.tolist(), first.tolist()[1:] + [len(ch.scans)]))
        ch.max_blocks, ch.max_pixels = max(f.blocks for f in forms[ch.a:ch.b]), max(f.H * f.W for f in forms[ch.a:ch.b])
    data = np.concatenate(data) if data else np.zeros(0, dtype=np.uint8)
    p = DecodePlan(data, images, [i for i, _, _ in kept], chunks, tables.buffer(), fallback, reasons, shapes, offsets, int(offsets[-1]))
    _check(p)
    return p


def _check(p):
    """Every chunk of a DecodePlan against its buffer sizes (avsep_jpeg_plan_check, avsep_jpeg_scan_check)."""
    for ch in p.chunks:
        if len(ch.segs) or not len(ch.scans):
            K.jpeg_plan_check(ch.images, ch.segs, max(len(p.bytes), 1), len(p.tables), p.pixel_bytes, ch.blocks)
        if len(ch.scans):
            K.jpeg_scan_check(ch.images, ch.scans, max(len(p.bytes), 1), len(p.tables), p.pixel_bytes, ch.blocks)


def rebase(p, offsets, pixel_bytes):
    """Move a DecodePlan into a pixel buffer it shares with other decoders (png.decode_stack): file i of the plan starts at
    offsets[i] of a buffer of pixel_bytes bytes.  The rows are checked again against the new size."""
    p.offsets, p.pixel_bytes = np.asarray(offsets, dtype=np.int64), int(pixel_bytes)
    p.images["pix_off"] = [p.offsets[i] for i in p.index]
    _check(p)


def launch(p, device, pixels=None, coef=None, planes=None):
    """Upload a plan and run its chunks on the current stream of ``device`` -> (pixels uint8 [bytes], status int32 [images] on the
    device, the coefficient workspace and planes as the last chunk left them).  Nothing is read back.  pixels, coef (int16) and
    planes (uint8), when given, are the buffers to use: the plan's bytes, and 64 per block of the largest chunk.  Per chunk: the
    baseline segments (avsep_jpeg_entropy), then the scan rows of its progressive images level after level (avsep_jpeg_scans, the
    first launch zeroing the workspace when the chunk has no baseline segment) and the bound check of the finished coefficients
    (avsep_jpeg_coef_bound), then the pixel stage."""
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
            st = status[ch.a:ch.b]
            if len(ch.segs):
                segs = torch.from_numpy(ch.segs.view(np.uint8)).to(device, non_blocking=True)
                K.jpeg_entropy(data, rows, segs, tables, coef, ch.blocks, st)
            if ch.scans is not None and len(ch.scans):
                # level after level: the rows are in rising order of level, and a level's lanes touch disjoint coefficients
                scans = torch.from_numpy(ch.scans.view(np.uint8)).to(device, non_blocking=True)
                for level, a, b in ch.levels:
                    K.jpeg_scans(data, rows, scans[a * SCAN.itemsize:b * SCAN.itemsize], level, a == 0 and not len(ch.segs), tables,
                                 coef, ch.blocks, st)
                K.jpeg_coef_bound(coef, ch.blocks, rows, ch.max_blocks, tables, st)
            K.jpeg_pixels(coef, planes, ch.blocks, rows, ch.max_blocks, ch.max_pixels, tables, st, pixels)
    return pixels, status, coef, planes


def decode(files, device, cap=WORKSPACE_CAP, decoded=None, progressive=False):
    """files: a list of bytes, each one image file -> (pixels uint8 [bytes] on ``device``, every frame [H,W,3] back to back in
    file order, and shapes [(H, W)]).  Supported files are decoded by the kernels; the status words are read once, and every
    refused or flagged file is decoded by Pillow and copied into its slot, so the result is Pillow's for every input.
    ``decoded`` {index: uint8 [H,W,3]} hands over pixels the caller already has for refused files.  ``progressive``: progressive
    files go through the kernels too (``plan``)."""
    files = [bytes(f) for f in files]
    p = plan(files, cap, progressive)
    pixels, status, _, _ = launch(p, device)
    again = list(p.fallback)
    if len(p.images):
        st = status.cpu().numpy()
        again += [p.index[r] for r in np.flatnonzero(st[:len(p.images)])]
    fill_from_pillow(pixels, files, again, p.shapes, p.offsets, decoded)
    return pixels, list(p.shapes)


def fill_from_pillow(pixels, files, again, shapes, offsets, decoded=None, who="jpeg.decode"):
    """The files ``again`` (indices into ``files``) decoded by Pillow, each copied into its slot of ``pixels``: H * W * 3 bytes
    from offsets[i].  ``decoded`` {index: uint8 [H,W,3]} hands over pixels the caller already has.  A file Pillow cannot read
    raises as it does there."""
    for i in sorted(again):
        a = decoded[i] if decoded is not None and i in decoded else _pillow(files[i])
        if a.shape != tuple(shapes[i]) + (3,):
            raise AvsepError(f"{who}: file {i} is {shapes[i]} by its header and {a.shape[:2]} once decoded")
        at = int(offsets[i])
        pixels[at:at + a.size] = torch.from_numpy(np.array(a)).reshape(-1).to(pixels.device)


def decode_stack(paths, device, progressive=False):
    """The image files ``paths`` of one clip -> uint8 [T,H,W,3] on ``device``: baseline JPEGs (with ``progressive``, progressive
    ones too) through the kernels, everything else through Pillow.  Frames of unequal size end with SystemExit, as in ``frames.load_stack``."""
    paths = list(paths)
    files = []
    for q in paths:
        with open(q, "rb") as f:
            files.append(f.read())
    pixels, shapes = decode(files, device, progressive=progressive)
    for q, s in zip(paths, shapes):
        if s != shapes[0]:
            raise SystemExit(f"{os.path.dirname(q)}: frames of unequal size: {os.path.basename(q)} is {s[0]} x {s[1]}, "
                             f"{os.path.basename(paths[0])} is {shapes[0][0]} x {shapes[0][1]}")
    return pixels.view(len(paths), shapes[0][0], shapes[0][1], 3)


# ---- writing: uint8 pictures on the device -> baseline JPEG files, byte for byte what Pillow's save gives (csrc/jpeg_enc.hip;
# include/avsep.h and DESIGN §33 have the rule)

ENC_HUFF_WORDS = 256                 # by symbol: (length << 16) | code (csrc/jpeg_parts.h: JP_ENC_HUFF_WORDS)
MAX_PICTURES = 1 << 24               # images per chunk
SAMPLING = {0: (1, 1), 1: (2, 1), 2: (2, 2), "4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2)}

# ITU-T T.81 Annex K: the example quantisers (natural order) and the typical Huffman tables (counts by length, values)
STD_QUANT = (np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51,
                       87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120,
                       101, 72, 92, 95, 98, 112, 100, 103, 99]),
             np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99]
                      + [99] * 36))
STD_HUFFMAN = {
    (0, 0): ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], bytes(range(12))),
    (0, 1): ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], bytes(range(12))),
    (1, 0): ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125], bytes.fromhex(
        "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a43"
        "4445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2"
        "b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")),
    (1, 1): ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119], bytes.fromhex(
        "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a"
        "434445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9"
        "aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")),
}


def quantisers(quality, chroma):
    """The quantisation table of ``quality`` (1 .. 100) -> int [64], natural order: libjpeg's scaling of the Annex K table."""
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.clip((STD_QUANT[1 if chroma else 0] * scale + 50) // 100, 1, 255)


def huffman_codes(counts, values):
    """One Huffman table as the encoding kernels read it -> int32 [ENC_HUFF_WORDS]: by symbol, (length << 16) | code."""
    w = np.zeros(ENC_HUFF_WORDS, dtype=np.int32)
    code, k = 0, 0
    for length in range(1, 17):
        for _ in range(int(counts[length - 1])):
            w[values[k]] = (length << 16) | code
            code, k = code + 1, k + 1
        code <<= 1
    return w


def _encode_form(shape, quality, subsampling, restart_blocks, restart_rows):
    """One picture's arguments, checked -> its Form (restart: the interval in MCUs)."""
    shape = tuple(int(s) for s in shape)
    if len(shape) not in (2, 3) or (len(shape) == 3 and shape[2] != 3):
        raise AvsepError(f"jpeg.encode takes pictures [H,W] (grey) or [H,W,3] (RGB), got a shape of {shape}")
    H, W = shape[:2]
    if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
        raise AvsepError(f"jpeg.encode takes sides of 1 .. {MAX_SIDE}, got {H} x {W}")
    if isinstance(quality, bool) or not isinstance(quality, (int, np.integer)) or not 1 <= quality <= 100:
        raise AvsepError(f"jpeg.encode takes a quality of 1 .. 100, got {quality!r}")
    if isinstance(subsampling, bool) or not isinstance(subsampling, (int, np.integer, str)) or subsampling not in SAMPLING:
        raise AvsepError(f"jpeg.encode takes subsampling 0 / 1 / 2 or '4:4:4' / '4:2:2' / '4:2:0', got {subsampling!r}")
    for name, v in (("restart_blocks", restart_blocks), ("restart_rows", restart_rows)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= v <= 65535:
            raise AvsepError(f"jpeg.encode takes {name} of 0 .. 65535, got {v!r}")
    ncomp = 1 if len(shape) == 2 else 3
    return Form.of(H, W, ncomp, *(SAMPLING[subsampling] if ncomp == 3 else (1, 1)), int(restart_blocks), int(restart_rows))


def _segment(marker, body):
    return bytes([0xFF, marker]) + struct.pack(">H", len(body) + 2) + bytes(body)


def encode_header(shape, quality=75, subsampling="4:2:0", restart_blocks=0, restart_rows=0):
    """Everything of the file before its entropy-coded bytes, SOI up to and including SOS -> bytes.  Pure Python, no GPU."""
    H, W, ncomp, hs, vs, _, _, restart = _encode_form(shape, quality, subsampling, restart_blocks, restart_rows)
    out = b"\xff\xd8" + _segment(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    for t in range(2 if ncomp == 3 else 1):
        out += _segment(0xDB, bytes([t]) + bytes(int(v) for v in quantisers(int(quality), t)[ZIGZAG]))
    comps = [(1, hs << 4 | vs, 0)] + ([(2, 0x11, 1), (3, 0x11, 1)] if ncomp == 3 else [])
    out += _segment(0xC0, struct.pack(">BHHB", 8, H, W, ncomp) + b"".join(bytes(c) for c in comps))
    for t in range(2 if ncomp == 3 else 1):
        for cls in (0, 1):
            counts, values = STD_HUFFMAN[(cls, t)]
            out += _segment(0xC4, bytes([cls << 4 | t]) + bytes(counts) + values)
    if restart:
        out += _segment(0xDD, struct.pack(">H", restart))
    scan = b"".join(bytes([c[0], c[2] << 4 | c[2]]) for c in comps)
    return out + _segment(0xDA, bytes([ncomp]) + scan + bytes([0, 63, 0]))


class EncodePlan:
    """What the encoding kernels read for a list of pictures: see ``encode_plan``."""

    def __init__(self, shapes, forms, headers, chunks, tables, offsets, pixel_bytes):
        self.shapes, self.forms, self.headers, self.chunks, self.tables = shapes, forms, headers, chunks, tables
        self.offsets, self.pixel_bytes = offsets, pixel_bytes


def _per_image(v, n, name):
    if isinstance(v, (list, tuple)):
        if len(v) != n:
            raise AvsepError(f"jpeg.encode_plan: {len(v)} values of {name} for {n} pictures")
        return list(v)
    return [v] * n


def encode_plan(shapes, quality=75, subsampling="4:2:0", restart_blocks=0, restart_rows=0, cap=WORKSPACE_CAP):
    """Pack what the kernels read to encode pictures of ``shapes`` ((H, W) grey, (H, W, 3) RGB; uint8, back to back in one buffer)
    -> EncodePlan.  quality, subsampling, restart_blocks and restart_rows are one value for all pictures or a list with one
    per picture.
    forms: per picture its Form (H, W, components, hs, vs, MCUs across, MCUs down, restart interval); headers: its bytes up to SOS;
    chunks: the pictures cut so that a chunk's coefficient workspace stays within ``cap`` bytes, each with its IMAGE rows;
    tables: quantisers (64 words, natural order) and Huffman code tables (``huffman_codes``) in one int32 buffer;
    offsets, pixel_bytes: every picture's first byte in the pixel buffer."""
    shapes = [tuple(int(x) for x in s) for s in shapes]
    n = len(shapes)
    if n < 1:
        raise AvsepError("jpeg.encode_plan takes at least one picture")
    cap_blocks = _cap_blocks("jpeg.encode_plan", cap)
    args = [_per_image(v, n, name) for v, name in ((quality, "quality"), (subsampling, "subsampling"),
                                                   (restart_blocks, "restart_blocks"), (restart_rows, "restart_rows"))]
    forms = [_encode_form(s, *a) for s, a in zip(shapes, zip(*args))]
    headers = [encode_header(s, *a) for s, a in zip(shapes, zip(*args))]
    offsets = np.concatenate([[0], np.cumsum([f.H * f.W * f.ncomp for f in forms], dtype=np.int64)])
    for i, f in enumerate(forms):
        if f.blocks > cap_blocks:
            raise AvsepError(f"jpeg.encode_plan: picture {i} has {f.blocks} blocks, more than the workspace cap of {cap_blocks}")
    tables = Tables()
    table_off = [[(tables.at(("q", int(q), t), quantisers, int(q), t), tables.at(("h", 0, t), huffman_codes, *STD_HUFFMAN[0, t]),
                   tables.at(("h", 1, t), huffman_codes, *STD_HUFFMAN[1, t])) for t in (0, 1, 1)[:f.ncomp]]
                 for f, q in zip(forms, args[0])]
    _, chunks = _rows(forms, offsets[:-1], table_off, _cut([f.blocks for f in forms], cap_blocks, MAX_PICTURES))
    p = EncodePlan(shapes, forms, headers, chunks, tables.buffer(), offsets, int(offsets[-1]))
    for ch in chunks:
        K.jpeg_enc_plan_check(ch.images, p.pixel_bytes, len(p.tables), ch.blocks, ch.intervals)
    return p


def encode_launch(p, device, pixels, coef=None, bits=None, stream=None):
    """Run an encoding plan on the current stream of ``device`` over ``pixels`` (uint8 [plan.pixel_bytes], the pictures back to
    back) -> (outs, coef, bits, stream): outs = per chunk (out uint8 [bytes], sizes int64 [2 * images]: every image's first byte
    and byte count in out), on the device; coef (int16, 64 per block), bits (int32, one per block) and stream (uint8, the
    unstuffed bytes) as the last chunk left them.  coef, bits and stream, when given, are the buffers to use: 64 and 1 per block
    of the largest chunk, and at least the largest chunk's unstuffed bytes rounded up to 4.  Two 8-byte totals per chunk are read
    back, the sizes of the stream and of the output; nothing else."""
    device = torch.device(device)
    if not torch.is_tensor(pixels) or pixels.dtype != torch.uint8 or pixels.dim() != 1 or pixels.numel() != p.pixel_bytes \
            or pixels.device.type != device.type:
        raise AvsepError(f"jpeg.encode_launch takes pixels uint8 [{p.pixel_bytes}] on {device}, got {got(pixels)}")
    device = pixels.device
    tables = torch.from_numpy(p.tables).to(device, non_blocking=True)
    blocks, intervals = max(ch.blocks for ch in p.chunks), max(ch.intervals for ch in p.chunks)
    coef = torch.empty(blocks * 64, dtype=torch.int16, device=device) if coef is None else coef
    bits = torch.empty(blocks, dtype=torch.int32, device=device) if bits is None else bits
    i64 = lambda m: torch.empty(m, dtype=torch.int64, device=device)
    i32 = lambda m: torch.empty(m, dtype=torch.int32, device=device)
    pos, ivl_off, out_off, ff0, ivl_bytes, ivl_out = i64(blocks + 1), i64(intervals + 1), i64(intervals + 1), i64(intervals), \
        i32(intervals), i32(intervals)
    outs, own_stream = [], stream is None
    for ch in p.chunks:
        rows = torch.from_numpy(np.ascontiguousarray(ch.images).view(np.uint8)).to(device, non_blocking=True)
        B, I = ch.blocks, ch.intervals
        tiles = i64(-(-B // 256))
        K.jpeg_enc_coef(pixels, rows, tables, coef, B)
        K.jpeg_enc_count(coef, B, rows, I, tables, bits, pos, ivl_bytes, ivl_off, tiles)
        nbytes = max(4, -(-int(ivl_off[I].item()) // 4) * 4)
        if own_stream and (stream is None or stream.numel() < nbytes):
            stream = torch.empty(nbytes, dtype=torch.uint8, device=device)
        if stream.numel() < nbytes:
            raise AvsepError(f"jpeg.encode_launch: the stream buffer has {stream.numel()} bytes, the chunk's unstuffed stream {nbytes}")
        groups = -(-nbytes // 64)
        tiles = i64(max(-(-groups // 256), -(-I // 256)))
        grp, ffpos = i32(groups), i64(groups + 1)
        K.jpeg_enc_pack(coef, B, rows, I, tables, pos, ivl_off, stream[:nbytes], grp, ffpos, ff0, ivl_out, out_off, tiles)
        out = torch.empty(int(out_off[I].item()), dtype=torch.uint8, device=device)
        sizes = i64(2 * (ch.b - ch.a))
        K.jpeg_enc_stuff(stream[:nbytes], rows, I, ivl_off, ffpos, ff0, out_off, out, sizes)
        outs.append((out, sizes))
    return outs, coef, bits, stream


def encode(images, quality=75, subsampling="4:2:0", restart_blocks=0, restart_rows=0, cap=WORKSPACE_CAP):
    """uint8 pictures on the GPU -> a list of ``bytes``, one JPEG file per picture, each byte for byte what
    ``Image.fromarray(picture).save(f, "JPEG", quality=, subsampling=, restart_marker_blocks=, restart_marker_rows=)`` writes.
    images: a list of tensors [H,W] (grey) or [H,W,3] (RGB), or one tensor [T,H,W] / [T,H,W,3].  The four settings are one
    value for all pictures or a list with one per picture.  Everything else Pillow's save takes (optimize, progressive,
    quality="keep", qtables, other modes) is not offered, and anything outside the limits raises: there is no fallback.  Only
    the encoded bytes and their sizes cross to the host."""
    if torch.is_tensor(images):
        if images.dim() not in (3, 4) or (images.dim() == 4 and images.shape[3] != 3):
            raise AvsepError(f"jpeg.encode takes one tensor [T,H,W] or [T,H,W,3], got {got(images)}")
        images = images.contiguous()
    seq = list(images.unbind(0)) if torch.is_tensor(images) else list(images)
    if not seq:
        raise AvsepError("jpeg.encode takes at least one picture")
    for t in seq:
        if not torch.is_tensor(t) or t.dtype != torch.uint8 or not t.is_cuda or t.device != seq[0].device:
            raise AvsepError(f"jpeg.encode takes uint8 tensors on one GPU, got {got(t)}")
    p = encode_plan([tuple(t.shape) for t in seq], quality, subsampling, restart_blocks, restart_rows, cap)
    pixels = images.reshape(-1) if torch.is_tensor(images) else torch.cat([t.reshape(-1) for t in seq])
    outs, _, _, _ = encode_launch(p, seq[0].device, pixels)
    files = []
    for ch, (out, sizes) in zip(p.chunks, outs):
        out, sizes = out.cpu().numpy(), sizes.cpu().numpy().reshape(-1, 2)
        for r, (at, n) in enumerate(sizes):
            files.append(p.headers[ch.a + r] + out[int(at):int(at + n)].tobytes())
    return files
