"""not-gpu: the RIFF/WAVE reader and writer (avsep_amd/wavio.py), the host statement of the four sample formats
(wavio.decode, tests/sample_formats_ref.py), the resample entry points' format checks and the --out_format flag."""
import os
import re
import struct
import wave
from fractions import Fraction

import numpy as np
import pytest
import torch

import avsep_amd
from avsep_amd import resample as RS
from avsep_amd import score as SC
from avsep_amd import separate as S
from avsep_amd import wavio as W
from avsep_amd.lib import AvsepError

import sample_formats_ref as F

PCM_GUID = struct.pack("<H", 1) + bytes.fromhex("000000001000800000aa00389b71")
FLOAT_GUID = struct.pack("<H", 3) + bytes.fromhex("000000001000800000aa00389b71")


def _fmt_chunk(tag, ch, rate, bits, extra=b"", align=None):
    align = ch * bits // 8 if align is None else align
    body = struct.pack("<HHIIHH", tag, ch, rate, rate * align, align, bits) + extra
    return b"fmt " + struct.pack("<I", len(body)) + body + (b"\0" if len(body) & 1 else b"")


def _extensible(ch, rate, bits, guid, valid=None):
    return _fmt_chunk(0xFFFE, ch, rate, bits, struct.pack("<HHI", 22, bits if valid is None else valid, 0) + guid)


def _chunk(cid, body, size=None):
    return cid + struct.pack("<I", len(body) if size is None else size) + body + (b"\0" if len(body) & 1 else b"")


def _file(path, *chunks):
    body = b"WAVE" + b"".join(chunks)
    with open(str(path), "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", len(body)) + body)
    return str(path)


def _frames(fmt, L, C, seed=0):
    rng = np.random.default_rng(seed)
    if fmt == "f32":
        return F.pack(rng.uniform(-1.5, 1.5, (L, C)), "f32")
    top = 2 ** (F.BITS[fmt] - 1)
    v = rng.integers(-top, top, size=(L, C))
    v.reshape(-1)[:2] = (-top, top - 1)[:v.size]
    return F.pack(v, fmt)


# ---------------------------------------------------------------------------------------------------------------------
# 1. every accepted header form
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,C", [("s16", 2), ("s24", 1), ("s24", 3), ("s32", 2), ("f32", 1), ("f32", 6)])
@pytest.mark.parametrize("form", ["plain", "extensible"])
def test_reads_every_accepted_header_form(tmp_path, fmt, C, form):
    raw = _frames(fmt, 7, C)                                         # 7 frames: s24 mono data has an odd size
    tag, bits = (3 if fmt == "f32" else 1), 8 * F.BYTES[fmt]
    if form == "plain":
        head = _fmt_chunk(tag, C, 44100, bits, struct.pack("<H", 0) if fmt == "f32" else b"")      # 18- and 16-byte forms
    else:
        head = _extensible(C, 44100, bits, FLOAT_GUID if fmt == "f32" else PCM_GUID)
    path = _file(tmp_path / "x.wav", head, _chunk(b"data", raw.tobytes()))
    assert W.probe(path) == W.WavInfo(44100, C, fmt, 7)
    got, info = W.read_frames(path)
    assert info == W.probe(path) and got.dtype == np.uint8 and np.array_equal(got, raw)


def test_float_file_with_a_16_byte_fmt_chunk(tmp_path):
    raw = _frames("f32", 5, 2)
    path = _file(tmp_path / "x.wav", _fmt_chunk(3, 2, 8000, 32), _chunk(b"data", raw.tobytes()))
    assert W.probe(path) == W.WavInfo(8000, 2, "f32", 5) and np.array_equal(W.read_frames(path)[0], raw)


def test_chunks_in_any_order_and_pad_bytes(tmp_path):
    raw = _frames("s24", 5, 1)                                       # 15 bytes: a pad byte follows
    fmt = _fmt_chunk(1, 1, 22050, 24)
    odd = _chunk(b"LIST", b"abc")                                    # odd size, padded
    for name, chunks in (("list_first", (odd, fmt, _chunk(b"data", raw.tobytes()))),
                         ("fmt_last", (odd, _chunk(b"data", raw.tobytes()), _chunk(b"bext", b"12345"), fmt)),
                         ("fact_between", (fmt, _chunk(b"fact", struct.pack("<I", 5)), odd, _chunk(b"data", raw.tobytes()), odd))):
        path = _file(tmp_path / f"{name}.wav", *chunks)
        got, info = W.read_frames(path)
        assert info == W.WavInfo(22050, 1, "s24", 5) and np.array_equal(got, raw), name


@pytest.mark.parametrize("size", [0, 0xFFFFFFFF, "one_past", "far_past"])
def test_open_ended_data_chunk_runs_to_the_end_of_the_file_in_whole_frames(tmp_path, size):
    raw = _frames("s24", 9, 2)                                       # 54 bytes of frames
    body = raw.tobytes() + b"\x01\x02\x03\x04"                       # and two thirds of a frame
    n = {"one_past": len(body) + 1, "far_past": len(body) + 1000}.get(size, size)
    path = _file(tmp_path / "x.wav", _fmt_chunk(1, 2, 48000, 24), _chunk(b"data", body, size=n))
    got, info = W.read_frames(path)
    assert info == W.WavInfo(48000, 2, "s24", 9) and np.array_equal(got, raw)


def test_a_stated_data_size_is_honoured(tmp_path):
    raw = _frames("s16", 6, 1)
    path = _file(tmp_path / "x.wav", _fmt_chunk(1, 1, 8000, 16), _chunk(b"data", raw.tobytes()), _chunk(b"LIST", b"\x11" * 40))
    assert W.probe(path).frames == 6 and np.array_equal(W.read_frames(path)[0], raw)


# ---------------------------------------------------------------------------------------------------------------------
# 2. every refusal names the file and what it found
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,head,word", [
    ("eight_bit", _fmt_chunk(1, 1, 8000, 8), "8-bit"),
    ("double", _fmt_chunk(3, 1, 8000, 64), "64-bit float"),
    ("alaw", _fmt_chunk(6, 1, 8000, 8), "A-law"),
    ("mulaw", _fmt_chunk(7, 1, 8000, 8), "mu-law"),
    ("adpcm", _fmt_chunk(2, 1, 8000, 4, align=256), "ADPCM"),
    ("ima", _fmt_chunk(0x11, 1, 8000, 4, align=256), "ADPCM"),
    ("short_fmt", b"fmt " + struct.pack("<I", 14) + struct.pack("<HHIIH", 1, 1, 8000, 16000, 2), "14 bytes"),
    ("align", _fmt_chunk(1, 2, 8000, 24, align=8), "block align 8"),
    ("valid_bits", _extensible(2, 8000, 24, PCM_GUID, valid=20), "20 valid bits"),
    ("other_guid", _extensible(2, 8000, 24, struct.pack("<H", 1) + b"\x01" * 14), "GUID"),
    ("ext_alaw", _extensible(1, 8000, 8, struct.pack("<H", 6) + PCM_GUID[2:]), "A-law"),
    ("short_ext", _fmt_chunk(0xFFFE, 2, 8000, 24, struct.pack("<H", 0)), "40 bytes"),
    ("tag", _fmt_chunk(0x674F, 1, 8000, 16), "format tag 26447"),
    ("no_channels", _fmt_chunk(1, 0, 8000, 16), "0 channel"),
])
def test_refusals(tmp_path, name, head, word):
    path = _file(tmp_path / f"{name}.wav", head, _chunk(b"data", b"\0" * 48))
    for fn in (W.probe, W.read_frames):
        with pytest.raises(AvsepError) as e:
            fn(path)
        assert f"{name}.wav" in str(e.value) and word in str(e.value), str(e.value)


def test_refuses_what_is_no_wave_file(tmp_path):
    cases = {"empty.wav": b"", "riff.wav": b"RIFF\x04\0\0\0AVI ", "rf64.wav": b"RF64\xff\xff\xff\xffWAVE" + b"\0" * 40,
             "nofmt.wav": b"RIFF\x10\0\0\0WAVE" + _chunk(b"data", b"\0" * 4), "nodata.wav": b"RIFF\x20\0\0\0WAVE" + _fmt_chunk(1, 1, 8000, 16)}
    for name, blob in cases.items():
        with open(str(tmp_path / name), "wb") as f:
            f.write(blob)
        with pytest.raises(AvsepError) as e:
            W.probe(str(tmp_path / name))
        assert name in str(e.value)
    with pytest.raises(AvsepError, match="RF64"):
        W.probe(str(tmp_path / "rf64.wav"))
    with pytest.raises(AvsepError, match="no fmt chunk"):
        W.probe(str(tmp_path / "nofmt.wav"))
    with pytest.raises(AvsepError, match="no data chunk"):
        W.probe(str(tmp_path / "nodata.wav"))


def test_the_16_bit_readers_still_refuse_a_24_bit_file(tmp_path):
    path = str(tmp_path / "s24.wav")
    W.write_frames(path, _frames("s24", 10, 1), 11025, 1, "s24")
    for fn in (S.read_wav, S.read_wav_pcm):
        with pytest.raises(AvsepError, match="16-bit"):
            fn(path)


# ---------------------------------------------------------------------------------------------------------------------
# 3. writer and round trips
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["s16", "s24", "f32"])
@pytest.mark.parametrize("L,C", [(1, 1), (7, 1), (8, 3), (1001, 2)])
def test_write_read_decode_round_trip(tmp_path, fmt, L, C):
    raw = _frames(fmt, L, C, seed=L + C)
    path = str(tmp_path / "x.wav")
    W.write_frames(path, raw, 96000, C, fmt)
    back, info = W.read_frames(path)
    assert info == W.WavInfo(96000, C, fmt, L) and np.array_equal(back, raw)
    blob = open(path, "rb").read()
    assert len(blob) % 2 == 0 and struct.unpack("<I", blob[4:8])[0] == len(blob) - 8           # padded to an even size
    if fmt == "f32":
        assert blob[12:16] == b"fmt " and struct.unpack("<IH", blob[16:22]) == (18, 3) and blob[38:42] == b"fact"
        assert struct.unpack("<II", blob[42:50]) == (4, L) and blob[50:54] == b"data"
        want = np.frombuffer(raw.tobytes(), "<f4").astype(np.float64)
    else:
        assert struct.unpack("<IH", blob[16:22]) == (16, 1) and blob[36:40] == b"data"
        assert struct.unpack("<I", blob[40:44])[0] == raw.size and len(blob) == 44 + raw.size + (raw.size & 1)
        want = F.integers(raw, fmt, C).astype(np.float64).reshape(-1) / 2.0 ** (F.BITS[fmt] - 1)
    x = W.decode(back, fmt, C)
    assert x.dtype == np.float64 and x.shape == (L, C) and np.array_equal(x.reshape(-1), want)


def test_s16_files_are_the_standard_librarys_bytes(tmp_path):
    pcm = np.random.default_rng(1).integers(-32768, 32768, size=(333, 2)).astype("<i2")
    with wave.open(str(tmp_path / "std.wav"), "wb") as w:
        w.setnchannels(2); w.setsampwidth(2); w.setframerate(48000)
        w.writeframes(pcm.tobytes())
    W.write_frames(str(tmp_path / "ours.wav"), np.frombuffer(pcm.tobytes(), np.uint8), 48000, 2, "s16")
    assert open(str(tmp_path / "ours.wav"), "rb").read() == open(str(tmp_path / "std.wav"), "rb").read()
    back, rate = S.read_wav_pcm(str(tmp_path / "ours.wav"))
    assert rate == 48000 and np.array_equal(back, pcm)


def test_writer_refusals(tmp_path):
    path = str(tmp_path / "x.wav")
    raw = np.zeros(24, np.uint8)
    with pytest.raises(AvsepError, match="s16, s24, f32"):
        W.write_frames(path, raw, 8000, 1, "s32")                    # no s32 output
    with pytest.raises(AvsepError):
        W.write_frames(path, raw[:23], 8000, 1, "s24")               # not whole frames
    with pytest.raises(AvsepError):
        W.write_frames(path, raw.astype(np.int16), 8000, 1, "s16")
    with pytest.raises(AvsepError):
        W.write_frames(path, raw, 0, 1, "s16")
    with pytest.raises(AvsepError):
        W.decode(raw[:23], "s24", 1)
    with pytest.raises(AvsepError):
        W.decode(raw, "u8", 1)


# ---------------------------------------------------------------------------------------------------------------------
# 4. what a sample means
# ---------------------------------------------------------------------------------------------------------------------
def test_decode_is_exact_at_the_extreme_samples():
    s24 = np.array([0x00, 0x00, 0x80, 0xFF, 0xFF, 0x7F, 0xFF, 0xFF, 0xFF, 0x01, 0x00, 0x00], np.uint8)      # 0x800000 0x7FFFFF 0xFFFFFF 1
    x = W.decode(s24, "s24", 1)[:, 0]
    want = [Fraction(-2 ** 23, 2 ** 23), Fraction(2 ** 23 - 1, 2 ** 23), Fraction(-1, 2 ** 23), Fraction(1, 2 ** 23)]
    assert [Fraction(float(v)) for v in x] == want and x[0] == -1.0
    s32 = np.frombuffer(struct.pack("<iiii", -2 ** 31, 2 ** 31 - 1, -1, 1), np.uint8)
    x = W.decode(s32, "s32", 2)
    assert x.shape == (2, 2)
    assert [Fraction(float(v)) for v in x.reshape(-1)] == [Fraction(-1), Fraction(2 ** 31 - 1, 2 ** 31), Fraction(-1, 2 ** 31), Fraction(1, 2 ** 31)]
    s16 = np.frombuffer(struct.pack("<hhh", -32768, 32767, -1), np.uint8)
    assert [Fraction(float(v)) for v in W.decode(s16, "s16", 1)[:, 0]] == [Fraction(-1), Fraction(32767, 32768), Fraction(-1, 32768)]
    f32 = np.frombuffer(struct.pack("<ffff", -3.5, 1e-40, np.inf, 2.0 ** -24), np.uint8)
    assert np.array_equal(W.decode(f32, "f32", 1)[:, 0], np.array([-3.5, np.float32(1e-40), np.inf, 2.0 ** -24], np.float64))
    # the reference module reads the same integers byte by byte
    assert F.integers(s24, "s24", 1)[:, 0].tolist() == [-2 ** 23, 2 ** 23 - 1, -1, 1]
    assert F.integers(s32, "s32", 1)[:, 0].tolist() == [-2 ** 31, 2 ** 31 - 1, -1, 1]


@pytest.mark.parametrize("fmt", ["s16", "s24", "s32"])
def test_down_mix_reference_is_the_correctly_rounded_quotient(fmt):
    """(float)((double)sum / (double)(C * 2^(bits-1))) against exact rationals: the f32 neighbours of the result bracket the
    exact quotient with the result at least as close as either (ties: even mantissa)."""
    rng = np.random.default_rng(F.BITS[fmt])
    top = 2 ** (F.BITS[fmt] - 1)
    for C in (2, 3, 5, 6, 7, 255, 256):
        v = rng.integers(-top, top, size=(40, C))
        v[0], v[1], v[2, :] = -top, top - 1, top - 1
        v[2, 0] = top - 2
        got = F.down_mix(F.pack(v, fmt), fmt, C)
        assert got.dtype == np.float32
        for row, g in zip(v, got):
            exact = Fraction(int(row.sum()), C * top)
            lo, hi = np.nextafter(g, np.float32(-np.inf)), np.nextafter(g, np.float32(np.inf))
            err = abs(Fraction(float(g)) - exact)
            for other in (lo, hi):
                d = abs(Fraction(float(other)) - exact)
                assert err < d or (err == d and (g.view(np.uint32) & 1) == 0), (fmt, C, row.sum())


def test_channel_reference_rounds_s32_once():
    v = np.array([[2 ** 31 - 1, -2 ** 31, 2 ** 24 + 1, 2 ** 24 + 3, -(2 ** 25 + 2), 12345]])
    got = F.channel(F.pack(v.T, "s32"), "s32", 1, 0)
    want = np.array([1.0, -1.0, 2.0 ** -7, (2 ** 24 + 4) / 2.0 ** 31, -(2 ** 25) / 2.0 ** 31, 12345 / 2.0 ** 31], np.float32)      # ties to even
    assert np.array_equal(got, want)
    assert np.array_equal(F.down_mix(F.pack(v.T, "s32"), "s32", 1), want)


def test_encode_reference_rounds_ties_to_even_and_clips():
    y = np.array([0.5 * 2.0 ** -23, 1.5 * 2.0 ** -23, -0.5 * 2.0 ** -23, 1.0, -1.0, 1.7, -1.7, 1.0 - 2.0 ** -24], np.float32)
    assert F.integers(F.encode(y, "s24"), "s24", 1)[:, 0].tolist() == [0, 2, 0, 2 ** 23 - 1, -2 ** 23, 2 ** 23 - 1, -2 ** 23, 2 ** 23 - 1]
    assert np.array_equal(F.encode(y, "f32"), np.frombuffer(y.tobytes(), np.uint8))
    assert F.integers(F.encode(y[3:7], "s16"), "s16", 1)[:, 0].tolist() == [32767, -32768, 32767, -32768]


def test_scipy_reads_our_files_and_we_read_its_float_files(tmp_path):
    wavfile = pytest.importorskip("scipy.io.wavfile")
    raw24 = _frames("s24", 100, 2)
    W.write_frames(str(tmp_path / "s24.wav"), raw24, 44100, 2, "s24")
    rate, data = wavfile.read(str(tmp_path / "s24.wav"))             # int32, the 24 bits in the high bytes
    assert rate == 44100 and np.array_equal(data.astype(np.int64), F.integers(raw24, "s24", 2) * 256)
    raw32 = _frames("f32", 100, 3)
    W.write_frames(str(tmp_path / "f32.wav"), raw32, 48000, 3, "f32")
    rate, data = wavfile.read(str(tmp_path / "f32.wav"))
    assert rate == 48000 and data.dtype == np.float32 and np.array_equal(data, np.frombuffer(raw32.tobytes(), "<f4").reshape(-1, 3))
    x = np.random.default_rng(2).uniform(-1, 1, (321, 2)).astype(np.float32)
    wavfile.write(str(tmp_path / "theirs.wav"), 22050, x)
    raw, info = W.read_frames(str(tmp_path / "theirs.wav"))
    assert info == W.WavInfo(22050, 2, "f32", 321) and np.array_equal(W.decode(raw, "f32", 2), x.astype(np.float64))


# ---------------------------------------------------------------------------------------------------------------------
# 5. host layers and flags
# ---------------------------------------------------------------------------------------------------------------------
def test_out_format_flag():
    a = S.parse_args(["--wav", "mix.wav", "--audio_only"])
    assert a.out_format == "file"
    for f in ("s16", "s24", "f32", "file"):
        assert S.parse_args(["--wav", "mix.wav", "--audio_only", "--out_format", f]).out_format == f
    for bad in ("s32", "u8", "24"):
        with pytest.raises(SystemExit):
            S.parse_args(["--wav", "mix.wav", "--audio_only", "--out_format", bad])
    for mod in (S, avsep_amd.localise, SC):
        assert "16-bit PCM WAV" not in mod.build_parser().format_help()


def test_score_reads_every_format_on_the_host(tmp_path):
    names = []
    for k, fmt in enumerate(("s24", "s24", "s24", "s24")):
        raw = _frames(fmt, 500 + 10 * k, 2, seed=k)
        W.write_frames(str(tmp_path / f"{k}.wav"), raw, 16000, 2, fmt)
        names.append((str(tmp_path / f"{k}.wav"), raw))
    refs, ests, rate = SC.read_stems([n for n, _ in names[:2]], [n for n, _ in names[2:]])
    assert rate == 16000 and refs.shape == ests.shape == (2, 2, 500) and refs.dtype == np.float64
    for got, (_, raw) in zip(list(refs) + list(ests), names):
        assert np.array_equal(got, W.decode(raw, "s24", 2)[:500].T)
    W.write_frames(str(tmp_path / "f.wav"), _frames("f32", 500, 2), 16000, 2, "f32")      # formats may differ between files
    refs, _, _ = SC.read_stems([str(tmp_path / "f.wav")], [names[0][0]])
    assert np.array_equal(refs[0], W.decode(_frames("f32", 500, 2), "f32", 2).T)
    bad = _file(tmp_path / "alaw.wav", _fmt_chunk(6, 1, 8000, 8), _chunk(b"data", b"\0" * 48))
    with pytest.raises(SystemExit, match="A-law"):
        SC.read_stems([bad], [bad])


def test_frames_functions_refuse_before_any_gpu_call(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a refusal must come before any GPU work")
    monkeypatch.setattr(avsep_amd.lib, "call", boom)
    monkeypatch.setattr(avsep_amd.kernels, "call", boom)
    monkeypatch.setattr(avsep_amd.lib, "require_gpu", boom)
    monkeypatch.setattr(RS, "filter_table", boom)
    raw = torch.zeros(48, dtype=torch.uint8)
    with pytest.raises(AvsepError, match="s16, s24, s32, f32"):
        RS.resample_frames(raw, "u8", 1, 48000, 11025)
    with pytest.raises(AvsepError, match="uint8"):
        RS.resample_frames(raw[:47], "s24", 1, 48000, 11025)         # not whole frames
    with pytest.raises(AvsepError, match="uint8"):
        RS.resample_frames(raw.to(torch.int16), "s16", 1, 48000, 11025)
    with pytest.raises(AvsepError, match="1 to 256"):
        RS.resample_frames(torch.zeros(4 * 257, dtype=torch.uint8), "s32", 257, 48000, 11025)
    with pytest.raises(AvsepError, match="1 to 8"):
        RS.split_frames(torch.zeros(27, dtype=torch.uint8), "s24", 9, 48000, 11025)
    with pytest.raises(AvsepError, match="11024"):
        RS.split_frames(raw, "s24", 2, 11024, 11025)
    with pytest.raises(AvsepError, match="s16, s24, f32"):
        RS.join_frames(torch.zeros(2, 10), 11025, 48000, "s32")      # no s32 output
    with pytest.raises(AvsepError, match="1 to 8"):
        RS.join_frames(torch.zeros(9, 10), 11025, 48000, "s24")
    with pytest.raises(AvsepError, match="float32"):
        RS.join_frames(torch.zeros(2, 10, dtype=torch.float64), 11025, 48000, "s24")


def test_fmt_entry_points_refuse_bad_arguments_before_launching():
    """include/avsep.h: a format code outside the table, an S32 output, f32 rows declared as PCM or off a 4-byte boundary,
    channel counts outside their limits, bad ratios and null pointers are argument errors (-1), returned without a launch."""
    import ctypes as C
    lib = avsep_amd.lib.load()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    S16, S24, S32, F32 = 1, 2, 3, 4
    f = lib.avsep_resample_poly
    assert f(p, p, 1, 16, 1, 4, 2, 0, F32, p, None) == -1                # no such input format
    assert f(p, p, 1, 16, 1, 4, 2, 5, F32, p, None) == -1
    assert f(p, p, 1, 16, 1, 4, 2, S24, S32, p, None) == -1              # no S32 output
    assert f(p, p, 1, 16, 1, 4, 2, S24, 0, p, None) == -1
    assert f(p, p, 1, 16, 1, 4, 0, S24, F32, p, None) == -1              # rows are floats
    assert f(p + 1, p, 1, 16, 1, 4, 0, F32, F32, p, None) == -1          # ... on a 4-byte boundary
    assert f(p, p, 2, 16, 1, 4, 2, S24, F32, p, None) == -1              # frames are one recording
    assert f(p, p, 1, 16, 1, 4, 257, S24, F32, p, None) == -1
    assert f(p, p, 1, 16, 0, 4, 2, S24, F32, p, None) == -1
    assert f(p, p, 1, 0, 1, 4, 2, S24, F32, p, None) == -1
    assert f(None, p, 1, 16, 1, 4, 2, S24, F32, p, None) == -1
    assert f(p, p, 1, 16, 1, 4, 2, S24, F32, None, None) == -1
    g = lib.avsep_resample_split
    assert g(p, p, 16, 2, 1, 4, 0, p, None) == -1
    assert g(p, p, 16, 2, 1, 4, 5, p, None) == -1
    assert g(p, p, 16, 9, 1, 4, S24, p, None) == -1
    assert g(p, p, 16, 0, 1, 4, S24, p, None) == -1
    assert g(p, p, 16, 2, 1281, 4, S24, p, None) == -1
    assert g(p, None, 16, 2, 1, 4, S24, p, None) == -1
    h = lib.avsep_resample_join
    assert h(p, p, 2, 16, 1, 4, S32, p, None) == -1
    assert h(p, p, 2, 16, 1, 4, 0, p, None) == -1
    assert h(p, p, 9, 16, 1, 4, S24, p, None) == -1
    assert h(p, p, 2, 2 ** 31 - 1, 4, 1, S24, p, None) == -1             # Lout >= 2^31
    assert h(p, p, 2, 16, 1, 4, S24, None, None) == -1
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "avsep.h")).read()
    codes = {n.lower(): int(v) for n, v in re.findall(r"#define AVSEP_SAMPLE_(\w+) (\d+)", hdr)}
    assert codes == {k: v[0] for k, v in avsep_amd.kernels.SAMPLE_FORMATS.items()} == {"s16": S16, "s24": S24, "s32": S32, "f32": F32}
    assert {k: v[1] for k, v in avsep_amd.kernels.SAMPLE_FORMATS.items()} == W.BYTES
