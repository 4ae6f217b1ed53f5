"""gpu: a file's frames in any sample format through the PCM kernels (the entry points of csrc/resample.hip,
resample.resample_frames / split_frames / join_frames, wavio.py and the command lines).

Every comparison is bit for bit.  The accumulation chains are shared with avsep_resample_poly, so a format can only show in
what is staged and in how a result is stored, and both are exactly specified (include/avsep.h): the input side equals the
f32 path fed the host's conversion (tests/sample_formats_ref.py), the output side equals the host's rounding of the kernel's
own f32 output.  Frames and outputs are placed at every byte phase of a dword."""
import json
import math
import wave

import numpy as np
import pytest
import torch

import avsep_amd as P
from avsep_amd import localise as LOC
from avsep_amd import resample as RS
from avsep_amd import score as SC
from avsep_amd import separate as S
from avsep_amd import wavio as W

import sample_formats_ref as F
from recipes import file_bytes as _bytes, nets as _nets, tone_mix_panned as _tone_mix

pytestmark = pytest.mark.gpu

RATIOS = [(1, 1), (640, 147), (1, 4), (4, 1), (1, 1280)]        # the last one takes the kernels' un-staged path
BASE = 11025


def _rates(up, down):
    return BASE * down, BASE * up


def _values(fmt, Ln, C, seed):
    rng = np.random.default_rng(seed)
    if fmt == "f32":
        v = rng.uniform(-1.0, 1.0, (Ln, C)).astype(np.float32)
        v.reshape(-1)[:3] = (-1.0, 1.0, 2.0 ** -30)[:v.size]
        return v
    top = 2 ** (F.BITS[fmt] - 1)
    v = rng.integers(-top, top, size=(Ln, C))
    v.reshape(-1)[:3] = (-top, top - 1, -1)[:v.size]
    return v


def _at_phase(raw, k, dev):
    """The bytes ``raw`` on the device, their first byte k bytes past a dword boundary."""
    buf = torch.empty(raw.size + k, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 4 == 0
    buf[k:] = torch.from_numpy(raw).to(dev)
    return buf[k:]


def _f32_path(mono, up, down, dev):
    return P.kernels.resample_poly(torch.from_numpy(np.ascontiguousarray(mono))[None].to(dev), RS.filter_table(up, down, dev), up, down)[0]


# ---------------------------------------------------------------------------------------------------------------------
# 1. input side
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("up,down", RATIOS)
@pytest.mark.parametrize("fmt", ["s16", "s24", "s32", "f32"])
def test_frames_input_is_the_f32_path_fed_the_down_mix(dev, fmt, up, down):
    """C in {1, 2, 3, 6}; L in {1, 2, 3, 4, 4001}: the last s24 frame ends on every dword phase; the frames start on each of
    the four byte phases."""
    rate_in, rate_out = _rates(up, down)
    for C in (1, 2, 3, 6):
        for Ln in (1, 2, 3, 4, 4001):
            raw = F.pack(_values(fmt, Ln, C, 100 * C + Ln), fmt)
            want = _f32_path(F.down_mix(raw, fmt, C), up, down, dev)
            assert want.shape == (RS.out_length(Ln, up, down),)
            for k in range(4):
                got = RS.resample_frames(_at_phase(raw, k, dev), fmt, C, rate_in, rate_out)
                assert got.dtype == torch.float32 and torch.equal(got, want), (fmt, C, Ln, k)
            if Ln == 4001 and up >= down:
                assert want.abs().max().item() > 0.1


@pytest.mark.parametrize("fmt", ["s16", "s24", "s32", "f32"])
def test_down_mix_of_256_channels_at_both_ends_of_the_range(dev, fmt):
    """Every channel at the most negative and at the most positive value: the integer sum passes 32 bits (256 * 2^31 = 2^39)
    and a float sum passes f32's range (added in f64); the mean is the value itself."""
    C, Ln = 256, 300
    if fmt == "f32":
        lo, hi = -np.finfo(np.float32).max, np.finfo(np.float32).max
        v = np.where(np.arange(Ln)[:, None] < Ln // 2, np.float32(lo), np.float32(hi)) * np.ones((1, C), np.float32)
    else:
        top = 2 ** (F.BITS[fmt] - 1)
        lo, hi = -1.0, (top - 1) / top
        v = np.where(np.arange(Ln)[:, None] < Ln // 2, -top, top - 1) * np.ones((1, C), np.int64)
    raw = F.pack(v, fmt)
    mono = F.down_mix(raw, fmt, C)
    assert mono[0] == np.float32(lo) and mono[-1] == np.float32(hi)
    for k in (0, 1, 2, 3):
        got = RS.resample_frames(_at_phase(raw, k, dev), fmt, C, BASE, BASE)          # the unit impulse: the down-mix itself
        assert np.array_equal(got.cpu().numpy(), mono), (fmt, k)
    if fmt != "f32":                                                                   # (a filter would overflow the floats)
        for up, down in ((640, 147), (1, 4)):
            got = RS.resample_frames(_at_phase(raw, 1, dev), fmt, C, *_rates(up, down))
            assert torch.equal(got, _f32_path(mono, up, down, dev)), (fmt, up, down)


@pytest.mark.parametrize("up,down", RATIOS)
@pytest.mark.parametrize("fmt", ["s16", "s24", "s32", "f32"])
def test_split_rows_are_the_single_row_results(dev, fmt, up, down):
    rate_in, rate_out = _rates(up, down)
    for C in (1, 2, 8):
        for Ln in (3, 4001):
            raw = F.pack(_values(fmt, Ln, C, 7 * C + Ln), fmt)
            rows = [_f32_path(F.down_mix(raw, fmt, C), up, down, dev)] + [_f32_path(F.channel(raw, fmt, C, c), up, down, dev) for c in range(C)]
            want = torch.stack(rows)
            for k in range(4):
                dev_raw = _at_phase(raw, k, dev)
                got = RS.split_frames(dev_raw, fmt, C, rate_in, rate_out)
                assert got.shape == (1 + C, RS.out_length(Ln, up, down)) and torch.equal(got, want), (fmt, C, Ln, k)
                assert torch.equal(got[0], RS.resample_frames(dev_raw, fmt, C, rate_in, rate_out))


# ---------------------------------------------------------------------------------------------------------------------
# 2. output side
# ---------------------------------------------------------------------------------------------------------------------
def _stems(C, Ln, seed=5):
    """Row c is one of: uniform * 1.7 (overshoots +-1: both clips occur), a +-1.0 plateau, uniform."""
    x = np.random.default_rng(seed).uniform(-1, 1, (C, Ln)).astype(np.float32)
    for c in range(C):
        if c % 3 == 0:
            x[c] *= 1.7
        elif c % 3 == 1:
            x[c, :Ln // 2], x[c, Ln // 2:] = 1.0, -1.0
    return x


@pytest.mark.parametrize("up,down", [(4, 1), (640, 147), (1, 4), (1, 1), (1279, 1280), (1, 1280)])
@pytest.mark.parametrize("C", [1, 2, 3, 8])
def test_frames_output_is_the_rounding_of_the_f32_output(dev, C, up, down):
    """s24 = clip(rint(y32 * 2^23)) packed, f32 = y32's bytes, s16 = join_pcm's bytes; the output starts on each of the four
    byte phases.  1279/1280 has runs of 1279 frames: with one and with three channels of s24 the runs of one workgroup start
    on all four phases by themselves."""
    Ln = 4001 if (up, down) == (1279, 1280) else 3001
    x = _stems(C, Ln)
    xt = torch.from_numpy(x).to(dev)
    filt = RS.filter_table(up, down, dev)
    y32 = P.kernels.resample_poly(xt, filt, up, down).cpu().numpy()                   # [C, Lout]
    Lout = y32.shape[1]
    assert Lout == RS.out_length(Ln, up, down)
    rate_in, rate_out = _rates(up, down)
    for fmt in ("s24", "f32", "s16"):
        want = F.encode(y32.T, fmt)
        if fmt == "s24" and up >= down:                                               # both clips occur
            ints = F.integers(want, "s24", C)
            assert ints.max() == 2 ** 23 - 1 and ints.min() == -2 ** 23
            assert (y32 * 2.0 ** 23 > 2 ** 23 - 0.5).any() and (y32 * 2.0 ** 23 < -2 ** 23 - 0.5).any()
        if fmt == "s16":
            assert np.array_equal(want, RS.join_pcm(xt, rate_in, rate_out).cpu().numpy().view(np.uint8).reshape(-1))
        for k in range(4):
            buf = torch.full((want.size + k + 8,), 0xA5, dtype=torch.uint8, device=dev)
            got = RS.join_frames(xt, rate_in, rate_out, fmt, out=buf[k:k + want.size])
            assert got.data_ptr() % 4 == k and np.array_equal(got.cpu().numpy(), want), (fmt, C, k)
            edge = buf.cpu().numpy()
            assert (edge[:k] == 0xA5).all() and (edge[k + want.size:] == 0xA5).all()  # not a byte outside the frames
        fresh = RS.join_frames(xt, rate_in, rate_out, fmt)
        assert fresh.dtype == torch.uint8 and fresh.shape == (Lout * C * F.BYTES[fmt],) and np.array_equal(fresh.cpu().numpy(), want)


def test_equal_rates_only_round(dev):
    x = _stems(3, 1000)
    xt = torch.from_numpy(x).to(dev)
    for fmt in ("s16", "s24", "f32"):
        assert np.array_equal(RS.join_frames(xt, BASE, BASE, fmt).cpu().numpy(), F.encode(x.T, fmt)), fmt


@pytest.mark.parametrize("up,down", [(640, 147), (1, 4), (1, 1), (1, 1280)])
def test_int16_adapters_are_the_byte_calls_and_poly_rows_sit_at_any_byte_address(dev, up, down):
    """resample_pcm / split_pcm / join_pcm on an int16 tensor are resample_frames / split_frames / join_frames on its bytes
    (what those give at every byte phase is tied to the host's down-mix by the tests above); rows of resample_poly in every
    output format, from byte offsets 1 to 3, are the host's encoding of its f32 output."""
    rate_in, rate_out = _rates(up, down)
    filt = RS.filter_table(up, down, dev)
    for C in (1, 2, 6):
        pcm = np.random.default_rng(C).integers(-32768, 32768, size=(4001, C)).astype(np.int16)
        pcm[:2] = np.array([-32768, 32767], np.int16)[:, None]
        raw = np.ascontiguousarray(pcm.astype("<i2")).view(np.uint8).reshape(-1)
        pt = torch.from_numpy(pcm).to(dev)
        dev_raw = _at_phase(raw, 0, dev)
        assert torch.equal(RS.resample_pcm(pt, rate_in, rate_out), RS.resample_frames(dev_raw, "s16", C, rate_in, rate_out)), C
        assert torch.equal(RS.split_pcm(pt, rate_in, rate_out), RS.split_frames(dev_raw, "s16", C, rate_in, rate_out)), C
    x = torch.from_numpy(_stems(3, 3001)).to(dev)
    y32 = P.kernels.resample_poly(x, filt, up, down)
    y16 = P.kernels.resample_poly(x, filt, up, down, out_fmt="s16")
    assert y16.dtype == torch.int16 and y16.shape == y32.shape
    assert np.array_equal(y16.cpu().numpy().view(np.uint8).reshape(-1), F.encode(y32.cpu().numpy().reshape(-1), "s16"))
    got24 = P.kernels.resample_poly(x, filt, up, down, 0, "f32", "s24")
    assert got24.shape == (3, 3 * y32.shape[1]) and np.array_equal(got24.cpu().numpy().reshape(-1), F.encode(y32.cpu().numpy().reshape(-1), "s24"))
    for k in (1, 2, 3):                                                                # rows of samples at any byte address
        for fmt in ("s16", "s24", "f32"):
            n = 3 * y32.shape[1] * F.BYTES[fmt]
            buf = torch.zeros(n + k, dtype=torch.uint8, device=dev)
            got = P.kernels.resample_poly(x, filt, up, down, 0, "f32", fmt, out=buf[k:])
            assert np.array_equal(got.cpu().numpy(), F.encode(y32.cpu().numpy().reshape(-1), fmt)), (fmt, k)
    assert np.array_equal(RS.join_frames(x, rate_in, rate_out, "s16").cpu().numpy(),
                          RS.join_pcm(x, rate_in, rate_out).cpu().numpy().view(np.uint8).reshape(-1))


def test_wrapper_refusals(dev):
    raw = torch.zeros(48, dtype=torch.uint8, device=dev)
    x = torch.zeros(2, 100, device=dev)
    filt = RS.filter_table(1, 4, dev)
    with pytest.raises(P.lib.AvsepError):
        P.kernels.resample_poly(raw, RS.filter_table(1, 2, dev), 1, 4, 2, "s24", "f32")      # another ratio's table
    with pytest.raises(P.lib.AvsepError):
        P.kernels.resample_poly(raw, filt, 1, 4, 5, "s24", "f32")                            # 48 bytes are no 5-channel frames
    with pytest.raises(P.lib.AvsepError):
        P.kernels.resample_poly(x, filt, 1, 4, 0, "s24", "f32")                              # rows are f32
    with pytest.raises(P.lib.AvsepError):
        P.kernels.resample_split(raw, filt, 1, 4, 2, "s20")
    with pytest.raises(P.lib.AvsepError):
        P.kernels.resample_join(x, filt, 1, 4, "s32")
    with pytest.raises(P.lib.AvsepError):
        P.kernels.resample_join(x, filt, 1, 4, "s24", out=torch.zeros(10, dtype=torch.uint8, device=dev))      # too small
    with pytest.raises(P.lib.AvsepError):
        RS.resample_frames(raw.cpu(), "s24", 2, 48000, 11025)                                    # no CPU fallback


# ---------------------------------------------------------------------------------------------------------------------
# 3. command lines
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cli_case(tmp_path_factory):
    """Small nets saved as a checkpoint; a 2 s 48 kHz stereo mix as a 16-bit file and as the 24-bit file whose samples are
    the 16-bit ones shifted left by 8; the 16-bit file's run of the command line."""
    d = tmp_path_factory.mktemp("formats_cli")
    mb = P.ModelBuilder()
    torch.manual_seed(11)
    snd = mb.build_sound(arch="unet5", fc_dim=2, fusion_type="hidsep", att_type="sig")
    frm = mb.build_frame(arch="resnet18dilated", fc_dim=256, pool_type="maxpool")
    torch.save(snd.state_dict(), str(d / "sound.pth"))
    torch.save(frm.state_dict(), str(d / "frame.pth"))
    pcm = np.clip(np.rint(_tone_mix(2 * 48000, 48000, 8) * 32768.0), -32768, 32767).astype(np.int16)
    with wave.open(str(d / "mix16.wav"), "wb") as w:
        w.setnchannels(2); w.setsampwidth(2); w.setframerate(48000)
        w.writeframes(pcm.astype("<i2").tobytes())
    W.write_frames(str(d / "mix24.wav"), F.pack(pcm.astype(np.int64) * 256, "s24"), 48000, 2, "s24")
    rng = np.random.default_rng(3)
    ones = []
    for n in range(2):
        np.save(str(d / f"one{n}.npy"), rng.standard_normal((3, 64, 64)).astype(np.float32))
        ones.append(str(d / f"one{n}.npy"))
        np.save(str(d / f"stack{n}.npy"), rng.standard_normal((4, 3, 64, 64)).astype(np.float32))
    flags = ["--arch_sound", "unet5", "--num_channels", "2", "--vis_channels", "256", "--img_pool", "maxpool", "--not_pool_vis",
             "--fusion_type", "hidsep", "--att_type", "sig", "--weights_sound", str(d / "sound.pth"),
             "--weights_frame", str(d / "frame.pth"), "--frames", *ones, "--binary_mask", "0"]
    out16 = S.cli(["--wav", str(d / "mix16.wav"), "--out", str(d / "out16"), *flags])
    return d, flags, pcm, out16


def test_separate_cli_hears_a_24_bit_file_as_its_16_bit_twin(dev, cli_case, tmp_path):
    d, flags, pcm, out16 = cli_case
    raw, info = W.read_frames(str(d / "mix24.wav"))
    assert info == W.WavInfo(48000, 2, "s24", 96000)
    # the network's input, hence its masks, are the 16-bit file's
    assert torch.equal(RS.resample_frames(torch.from_numpy(raw).to(dev), "s24", 2, 48000, 11025),
                       RS.resample_pcm(torch.from_numpy(pcm).to(dev), 48000, 11025))
    out = S.cli(["--wav", str(d / "mix24.wav"), "--out", str(tmp_path / "s16"), "--out_format", "s16", *flags])
    assert torch.equal(out["wavs"], out16["wavs"]) and torch.equal(out["perms"], out16["perms"]) and out["wavs"].abs().max().item() > 0.01
    for n in range(2):
        assert _bytes(tmp_path / "s16" / f"source{n}.wav") == _bytes(d / "out16" / f"source{n}.wav")


def test_separate_cli_answers_a_24_bit_file_in_24_bits(dev, cli_case, tmp_path):
    d, flags, _, out16 = cli_case
    out = S.cli(["--wav", str(d / "mix24.wav"), "--out", str(tmp_path / "file"), *flags])                # --out_format file
    assert torch.equal(out["wavs"], out16["wavs"])
    model = S.cli(["--wav", str(d / "mix24.wav"), "--out", str(tmp_path / "model"), "--out_rate", "model", *flags])
    for n in range(2):
        got, info = W.read_frames(str(tmp_path / "file" / f"source{n}.wav"))
        want = RS.join_frames(out["wavs"][n][None], 11025, 48000, "s24").cpu().numpy()
        assert info == W.WavInfo(48000, 1, "s24", want.size // 3) and np.array_equal(got, want)
        assert info.frames == math.ceil(out["wavs"].shape[1] * 640 / 147) and np.abs(F.integers(got, "s24", 1)).max() > 300 * 256
        got, info = W.read_frames(str(tmp_path / "model" / f"source{n}.wav"))                            # the model's rate: only rounded
        assert info == W.WavInfo(11025, 1, "s24", out["wavs"].shape[1])
        assert np.array_equal(got, F.encode(model["wavs"][n].cpu().numpy(), "s24"))


def test_separate_cli_keeps_the_channels_of_a_float_extensible_file(dev, cli_case, tmp_path):
    import struct
    d, flags, _, _ = cli_case
    x = (_tone_mix(2 * 44100, 44100, 9, pans=(0.8, 0.3, 0.55)) * 1.2).astype(np.float32)
    raw = F.pack(x, "f32")
    guid = struct.pack("<H", 3) + bytes.fromhex("000000001000800000aa00389b71")
    fmt = struct.pack("<HHIIHH", 0xFFFE, 3, 44100, 44100 * 12, 12, 32) + struct.pack("<HHI", 22, 32, 7) + guid
    junk = b"LIST" + struct.pack("<I", 3) + b"abc\0"                                   # an odd chunk, padded, before fmt
    body = b"WAVE" + junk + b"fmt " + struct.pack("<I", 40) + fmt + b"data" + struct.pack("<I", raw.size) + raw.tobytes()
    with open(str(tmp_path / "mix.wav"), "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", len(body)) + body)
    assert W.probe(str(tmp_path / "mix.wav")) == W.WavInfo(44100, 3, "f32", 2 * 44100)
    argv = ["--wav", str(tmp_path / "mix.wav"), "--channels", "keep", "--wiener", "1", *flags]
    out = S.cli(argv + ["--out", str(tmp_path / "out")])
    # the same composition by hand
    args = S.parse_args(argv)
    rows = RS.split_frames(torch.from_numpy(raw).to(dev), "f32", 3, 44100, args.audRate)
    frames = [torch.from_numpy(np.load(p)).float()[None].to(dev) for p in args.frames]
    hand = S.separate_long(_nets(args, dev), rows[0], frames, args, channels=rows[1:], wiener=1)
    assert torch.equal(out["channel_wavs"], hand["channel_wavs"]) and out["channel_wavs"].shape[:2] == (2, 3)
    for n in range(2):
        got, info = W.read_frames(str(tmp_path / "out" / f"source{n}.wav"))
        want = RS.join_frames(hand["channel_wavs"][n], args.audRate, 44100, "f32").cpu().numpy()
        assert info == W.WavInfo(44100, 3, "f32", want.size // 12) and np.array_equal(got, want)
        assert np.abs(W.decode(got, "f32", 3)).max() > 0.01


def test_localise_cli_hears_a_24_bit_file_as_its_16_bit_twin(dev, cli_case, tmp_path):
    d, flags, _, _ = cli_case
    base = flags[:flags.index("--frames")] + ["--frames", str(d / "stack0.npy"), str(d / "stack1.npy"), "--fps", "2"]
    want = LOC.cli(["--wav", str(d / "mix16.wav"), "--out", str(tmp_path / "loc16"), *base])
    got = LOC.cli(["--wav", str(d / "mix24.wav"), "--out", str(tmp_path / "loc24"), *base])
    assert got["maps"].shape == (4, 2, 4, 4) and torch.equal(got["maps"], want["maps"]) and torch.equal(got["overlays"], want["overlays"])


def test_score_cli_on_24_bit_stems(dev, tmp_path):
    rng = np.random.default_rng(4)
    Ln, rate = 24000, 16000
    src = rng.standard_normal((2, 2, Ln)) * 0.1
    est = src + 0.02 * rng.standard_normal(src.shape) + 0.05 * src[::-1]
    paths = []
    for name, stems in (("ref", src), ("est", est)):
        for j in range(2):
            v = np.clip(np.rint(stems[j].T * 2.0 ** 23), -2 ** 23, 2 ** 23 - 1)
            W.write_frames(str(tmp_path / f"{name}{j}.wav"), F.pack(v, "s24"), rate, 2, "s24")
            paths.append(str(tmp_path / f"{name}{j}.wav"))
    res = SC.cli(["--ref", *paths[:2], "--est", *paths[2:], "--flen", "64", "--json", str(tmp_path / "s.json")])
    dec = [W.decode(*W.read_frames(p)[0:1], "s24", 2).T for p in paths]
    assert np.abs(np.stack(dec) * 2.0 ** 23 % 256).max() > 0                           # the low byte is in use
    want = SC.score_stems(torch.from_numpy(np.stack(dec[:2])).to(dev), torch.from_numpy(np.stack(dec[2:])).to(dev), rate, rate, "track", 64)
    doc = json.load(open(str(tmp_path / "s.json")))
    assert doc["rate"] == rate and doc["perm"] == want["perm"] == res["perm"]
    for k in ("sdr", "isr", "sir", "sar"):
        assert torch.equal(res[k], want[k]) and doc[k] == SC._jsonable(want[k]) and doc["frames"][k] == SC._jsonable(want["frames"][k])
        assert doc["track"][k] == SC._jsonable(want["track"][k])
    assert min(doc["sdr"]) > 5.0
