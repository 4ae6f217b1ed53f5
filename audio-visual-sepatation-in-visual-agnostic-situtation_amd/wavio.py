"""RIFF/WAVE files in the four sample formats of include/avsep.h, on ``struct`` alone.

The standard library's ``wave`` opens neither IEEE-float files nor WAVE_FORMAT_EXTENSIBLE headers, and a 24-bit stem is
what a DAW exports.  Nothing is converted here on the way in or out: ``read_frames`` hands back the data chunk's bytes as
they lie in the file, the kernels of csrc/resample.hip take them as they are (resample.resample_frames / split_frames)
and give back bytes in file layout (resample.join_frames) for ``write_frames``.  ``decode`` is the host statement of what a
sample means, for ``score`` and for the tests.

    code   file encoding                one sample as a number
    s16    2 bytes LE, tag 1            v / 2^15
    s24    3 bytes LE packed, tag 1     sign-extended v / 2^23
    s32    4 bytes LE, tag 1            v / 2^31
    f32    IEEE binary32 LE, tag 3      the value itself

RF64, files past 4 GiB, 8-bit, 64-bit float and compressed forms are refused.
"""
import os
import struct
from collections import namedtuple

import numpy as np

from .lib import AvsepError

BYTES = {"s16": 2, "s24": 3, "s32": 4, "f32": 4}      # container bytes of one sample
WRITTEN = ("s16", "s24", "f32")                       # what write_frames and the kernels' output side give
TAG_PCM, TAG_FLOAT, TAG_EXTENSIBLE = 1, 3, 0xFFFE
_GUID_TAIL = bytes.fromhex("000000001000800000aa00389b71")      # KSDATAFORMAT_SUBTYPE_*: the tag, then these 14 bytes
_REFUSED_TAGS = {2: "MS ADPCM", 6: "A-law", 7: "mu-law", 0x11: "IMA ADPCM", 0x55: "MPEG layer 3"}

WavInfo = namedtuple("WavInfo", "rate channels fmt frames")


def _parse_fmt(path, body):
    """The ``fmt `` chunk's body -> (rate, channels, fmt)."""
    if len(body) < 16:
        raise AvsepError(f"{path}: the fmt chunk has {len(body)} bytes, a WAVE format needs at least 16")
    tag, ch, rate, _, align, bits = struct.unpack("<HHIIHH", body[:16])
    what = f"format tag {tag}"
    if tag == TAG_EXTENSIBLE:
        if len(body) < 40:
            raise AvsepError(f"{path}: an extensible fmt chunk has 40 bytes, this one has {len(body)}")
        valid, = struct.unpack("<H", body[18:20])
        guid = body[24:40]
        tag, = struct.unpack("<H", guid[:2])
        what = f"extensible sub-format {tag}"
        if guid[2:] != _GUID_TAIL:
            raise AvsepError(f"{path}: extensible sub-format GUID {guid.hex()} is neither PCM nor IEEE float")
        if valid != bits:
            raise AvsepError(f"{path}: {valid} valid bits in {bits}-bit containers; only full containers are read")
    if tag in _REFUSED_TAGS:
        raise AvsepError(f"{path}: {_REFUSED_TAGS[tag]} ({what}); only uncompressed PCM and 32-bit float are read")
    if tag == TAG_PCM:
        fmt = {16: "s16", 24: "s24", 32: "s32"}.get(bits)
        if fmt is None:
            raise AvsepError(f"{path}: {bits}-bit PCM; 16-, 24- and 32-bit PCM and 32-bit float are read")
    elif tag == TAG_FLOAT:
        if bits != 32:
            raise AvsepError(f"{path}: {bits}-bit float; 16-, 24- and 32-bit PCM and 32-bit float are read")
        fmt = "f32"
    else:
        raise AvsepError(f"{path}: {what} is neither PCM (1) nor IEEE float (3)")
    if ch < 1 or rate < 1:
        raise AvsepError(f"{path}: {ch} channel(s) at {rate} Hz")
    if align != ch * BYTES[fmt]:
        raise AvsepError(f"{path}: block align {align} for {ch} channel(s) of {BYTES[fmt]} bytes (expected {ch * BYTES[fmt]})")
    return rate, ch, fmt


def _open(path):
    """-> (file object positioned anywhere, WavInfo, offset and byte count of the frames).  Chunks in any order, a pad byte
    after an odd size; a data size of 0, 0xFFFFFFFF or one that runs past the end of the file means "to the end of the file"."""
    f = open(path, "rb")
    try:
        end = os.fstat(f.fileno()).st_size
        head = f.read(12)
        if len(head) < 12 or head[:4] != b"RIFF" or head[8:12] != b"WAVE":
            kind = "an RF64 file (not read)" if head[:4] == b"RF64" else "not a RIFF/WAVE file"
            raise AvsepError(f"{path}: {kind}")
        fmt = data = None
        pos = 12
        while pos + 8 <= end and (fmt is None or data is None):
            f.seek(pos)
            cid, size = struct.unpack("<4sI", f.read(8))
            pos += 8
            if cid == b"fmt ":
                fmt = _parse_fmt(path, f.read(min(size, end - pos)))
            elif cid == b"data":
                if size in (0, 0xFFFFFFFF) or pos + size > end:
                    size = end - pos
                data = (pos, size)
            pos += size + (size & 1)
        if fmt is None or data is None:
            raise AvsepError(f"{path}: no {'fmt' if fmt is None else 'data'} chunk")
        rate, ch, code = fmt
        frames = data[1] // (ch * BYTES[code])                      # whole frames only
        return f, WavInfo(rate, ch, code, frames), data[0], frames * ch * BYTES[code]
    except BaseException:
        f.close()
        raise


def probe(path):
    """-> WavInfo(rate, channels, fmt, frames) from the header; AvsepError (naming the file and what it holds) for
    anything that is not s16 / s24 / s32 PCM or f32."""
    f, info, _, _ = _open(path)
    f.close()
    return info


def read_frames(path):
    """-> (np.uint8 [frames * channels * bytes], WavInfo): the frames as they lie in the file, nothing converted."""
    f, info, off, n = _open(path)
    with f:
        f.seek(off)
        raw = np.fromfile(f, dtype=np.uint8, count=n)
    if raw.size != n:
        raise AvsepError(f"{path}: {raw.size} of {n} data bytes could be read")
    return raw, info


def write_frames(path, raw, rate, channels, fmt):
    """raw: uint8 [frames * channels * bytes] in file layout (join_frames' result) -> a WAV file.  s16 / s24: the plain
    44-byte header; f32: tag 3 with an 18-byte fmt chunk and a fact chunk."""
    if fmt not in WRITTEN:
        raise AvsepError(f"write_frames writes {', '.join(WRITTEN)}, got {fmt!r}")
    raw = np.ascontiguousarray(raw)
    rate, channels = int(rate), int(channels)
    align = channels * BYTES[fmt]
    if raw.dtype != np.uint8 or raw.ndim != 1 or channels < 1 or channels > 65535 or rate < 1 or raw.size % align:
        raise AvsepError(f"write_frames takes uint8 [frames * {channels} * {BYTES[fmt]}] and a positive rate, got {raw.dtype} "
                         f"{raw.shape} at {rate} Hz")
    n = raw.size
    pad = n & 1
    if n + pad + 50 > 0xFFFFFFFF:
        raise AvsepError(f"{path}: {n} bytes of frames do not fit a RIFF file (4 GiB)")
    body = struct.pack("<HHIIHH", TAG_FLOAT if fmt == "f32" else TAG_PCM, channels, rate, rate * align, align, 8 * BYTES[fmt])
    if fmt == "f32":
        chunks = b"fmt " + struct.pack("<I", 18) + body + struct.pack("<H", 0) + b"fact" + struct.pack("<II", 4, n // align)
    else:
        chunks = b"fmt " + struct.pack("<I", 16) + body
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 4 + len(chunks) + 8 + n + pad) + b"WAVE" + chunks + b"data" + struct.pack("<I", n))
        raw.tofile(f)
        if pad:
            f.write(b"\0")


def decode(raw, fmt, channels):
    """raw: the bytes of read_frames -> float64 [L, channels], every sample's exact value (table above)."""
    if fmt not in BYTES:
        raise AvsepError(f"decode takes one of {', '.join(BYTES)}, got {fmt!r}")
    raw = np.ascontiguousarray(raw)
    channels = int(channels)
    if raw.dtype != np.uint8 or raw.ndim != 1 or channels < 1 or raw.size % (channels * BYTES[fmt]):
        raise AvsepError(f"decode takes uint8 [frames * {channels} * {BYTES[fmt]}], got {raw.dtype} {raw.shape}")
    if fmt == "s24":
        b = raw.reshape(-1, 3).astype(np.int32)
        v = ((b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)) ^ 0x800000) - 0x800000          # sign-extended
        x = v.astype(np.float64) / 2.0 ** 23
    elif fmt == "f32":
        x = raw.view("<f4").astype(np.float64)
    else:
        x = raw.view("<i2" if fmt == "s16" else "<i4").astype(np.float64) / 2.0 ** (8 * BYTES[fmt] - 1)
    return x.reshape(-1, channels)
