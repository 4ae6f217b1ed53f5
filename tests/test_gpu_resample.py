"""gpu: sample-rate conversion (csrc/resample.hip, avsep_amd/resample.py and the --wav paths of separate.py / localise.py).

Values are compared with the float64 direct sum of tests/resample_ref.py under a DERIVED bound: an output is a chain of at
most T = ceil(M / up) f32 multiply-adds, so |y - ref| <= (T + 2) * 2^-24 * sum_n |x[n]| |h[..]| — T roundings of the running
sum (sequential or tree), one for the filter rounded to f32 and one for the product — and exactly 0 where that sum is 0.
Formats, row independence and the command lines are bit-for-bit statements."""
import math

import numpy as np
import pytest
import torch

import avsep_amd as P
from avsep_amd import localise as L
from avsep_amd import resample as RS
from avsep_amd import separate as S

import resample_ref as R
from recipes import file_bytes as _bytes, nets as _nets, tone_mix_stereo as _tone_mix_stereo, write_pcm as _write_pcm

pytestmark = pytest.mark.gpu

RATIOS = [(1, 4), (4, 1), (1, 2), (2, 1), (3, 7), (7, 3), (147, 640), (640, 147), (441, 320), (320, 441), (441, 1280), (1280, 441)]
EPS = 2.0 ** -24


def _table(up, down, dev):
    return RS.filter_table(up, down, dev)


def _check(y, x, up, down, idx, what):
    """y: the kernel's f32 row (NumPy), x: its input row; -> worst |y - ref| / bound over ``idx``."""
    ref, absref = R.ref_outputs(x, up, down, idx)
    bound = (R.taps(up, down) + 2) * EPS * absref
    err = np.abs(y[idx].astype(np.float64) - ref)
    bad = err > bound
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {len(idx)} outputs miss the bound, first j={int(np.asarray(idx)[bad][0])}: "
                           f"|d|={err[bad][0]:.3e} bound={bound[bad][0]:.3e}")
    live = bound > 0
    return float((err[live] / bound[live]).max()) if live.any() else 0.0


def _rows(Ln, seed):
    """The input kinds of one length: two seeded uniform rows, a unit impulse at either end, all ones."""
    rng = np.random.default_rng(seed)
    first, last = np.zeros(Ln, np.float32), np.zeros(Ln, np.float32)
    first[0], last[-1] = 1.0, 1.0
    return {"uniform": rng.uniform(-1, 1, Ln).astype(np.float32), "uniform2": rng.uniform(-1, 1, Ln).astype(np.float32),
            "impulse0": first, "impulseL": last, "ones": np.ones(Ln, np.float32)}


# ---------------------------------------------------------------------------------------------------------------------
# 1. values
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("up,down", RATIOS)
def test_values_vs_float64_direct_sum(dev, up, down):
    """Lengths 1, 2, 79, 1025 (shorter than the filter: both zero edges overlap; one sample; one past a power of two) with
    every output checked, 30 011 with both ends and a seeded sample; a B = 3 call of different rows and two B = 1 calls."""
    filt = _table(up, down, dev)
    worst = 0.0
    for Ln in (1, 2, 79, 1025, 30011):
        rows = _rows(Ln, 1000 * up + down + Ln)
        Lout = R.out_length(Ln, up, down)
        if Lout <= 4608:
            idx = np.arange(Lout)
        else:
            mid = np.random.default_rng(Ln).choice(Lout - 512, size=4096, replace=False) + 256
            idx = np.concatenate([np.arange(256), np.sort(mid), np.arange(Lout - 256, Lout)])
        for names in (("uniform", "impulse0", "ones"), ("impulseL",), ("uniform2",)):
            x = torch.from_numpy(np.stack([rows[n] for n in names])).to(dev)
            y = P.kernels.resample_poly(x, filt, up, down)
            assert y.shape == (len(names), Lout) and y.dtype == torch.float32
            y = y.cpu().numpy()
            for r, n in enumerate(names):
                worst = max(worst, _check(y[r], rows[n], up, down, idx, f"{up}/{down} L={Ln} B={len(names)} row {n}"))
    print(f"resample {up}/{down}: worst |y - ref| / bound = {worst:.3f}")


@pytest.mark.parametrize("up,down,Ln", [(1, 1280, 30011), (1280, 1, 37), (1, 16, 5000), (1280, 1279, 2000)])
def test_values_where_the_tile_does_not_fit_in_lds(dev, up, down, Ln):
    """Ratios this far from 1 have no use, but the limit admits them: 1/1280 and 1/16 take the kernel's unstaged path
    (1024 outputs span more input than its LDS tile holds), 1280/1 and 1280/1279 are the largest tables."""
    x = np.random.default_rng(Ln).uniform(-1, 1, Ln).astype(np.float32)
    y = P.kernels.resample_poly(torch.from_numpy(x)[None].to(dev), _table(up, down, dev), up, down)[0].cpu().numpy()
    Lout = R.out_length(Ln, up, down)
    assert y.shape == (Lout,)
    idx = np.arange(Lout) if Lout <= 4608 else np.concatenate([np.arange(2304), np.arange(Lout - 2304, Lout)])
    print(f"resample {up}/{down}: worst |y - ref| / bound = {_check(y, x, up, down, idx, f'{up}/{down}'):.3f}")


# ---------------------------------------------------------------------------------------------------------------------
# 2. 64-bit indexing: j * down + half and n * up pass 2^31 on a ten-minute file
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate_in,rate_out,Ln", [(11025, 48000, 6_615_000), (48000, 11025, 28_800_000)])
def test_ten_minute_file_is_indexed_in_64_bits(dev, rate_in, rate_out, Ln):
    up, down = RS.rational(rate_in, rate_out)
    x = np.random.default_rng(7).random(Ln, dtype=np.float32) * 2.0 - 1.0
    y = RS.resample(torch.from_numpy(x).to(dev), rate_in, rate_out)
    Lout = R.out_length(Ln, up, down)
    assert y.shape == (Lout,) and (Lout - 1) * down + 10 * max(up, down) > 2 ** 31
    mid = np.random.default_rng(8).choice(Lout - 256, size=4096, replace=False)
    idx = np.concatenate([np.sort(mid), np.arange(Lout - 256, Lout)])
    got = np.zeros(Lout, np.float32)
    got[idx] = y[torch.from_numpy(idx).to(dev)].cpu().numpy()
    print(f"resample {rate_in} -> {rate_out}, {Ln} samples: worst |y - ref| / bound = {_check(got, x, up, down, idx, 'long'):.3f}")


# ---------------------------------------------------------------------------------------------------------------------
# 3. rows are independent, calls repeat
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("up,down", [(1, 4), (640, 147)])
def test_row_alone_in_a_batch_and_again_bit_identical(dev, up, down):
    x = torch.from_numpy(np.random.default_rng(3).uniform(-1, 1, (3, 5003)).astype(np.float32)).to(dev)
    filt = _table(up, down, dev)
    y = P.kernels.resample_poly(x, filt, up, down)
    assert torch.equal(P.kernels.resample_poly(x, filt, up, down), y)
    for r in range(3):
        assert torch.equal(P.kernels.resample_poly(x[r:r + 1].contiguous(), filt, up, down)[0], y[r])
    assert not torch.equal(y[0], y[1])
    rate_in, rate_out = 11025 * down, 11025 * up
    assert torch.equal(RS.resample(x, rate_in, rate_out), y) and torch.equal(RS.resample(x[1], rate_in, rate_out), y[1])
    assert RS.resample(x, 11025, 11025) is x


# ---------------------------------------------------------------------------------------------------------------------
# 4. formats
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 2, 6])
@pytest.mark.parametrize("rate_in", [48000, 44100, 11025])
def test_pcm_input_is_the_f32_path_fed_the_down_mix(dev, tmp_path, C, rate_in):
    rng = np.random.default_rng(C)
    pcm = rng.integers(-32768, 32768, size=(4001, C)).astype(np.int16)
    pcm[:3] = np.array([-32768, 32767, 0], np.int16)[:, None]
    mono = (pcm.astype(np.float64).sum(1) / (C * 32768.0)).astype(np.float32)        # rounded once
    if C <= 2:
        import wave
        with wave.open(str(tmp_path / "x.wav"), "wb") as w:
            w.setnchannels(C); w.setsampwidth(2); w.setframerate(rate_in)
            w.writeframes(pcm.astype("<i2").tobytes())
        assert np.array_equal(S.read_wav(str(tmp_path / "x.wav"))[0], mono)
    got = RS.resample_pcm(torch.from_numpy(pcm).to(dev), rate_in, 11025)
    if rate_in == 11025:
        assert np.array_equal(got.cpu().numpy(), mono)                                # equal rates: read_wav's own bits
    else:
        up, down = RS.rational(rate_in, 11025)
        want = P.kernels.resample_poly(torch.from_numpy(mono)[None].to(dev), _table(up, down, dev), up, down)[0]
        assert got.shape == want.shape == (R.out_length(4001, up, down),) and torch.equal(got, want)
        assert got.abs().max().item() > 0.1


@pytest.mark.parametrize("up,down", [(4, 1), (640, 147), (1, 4)])
def test_s16_output_is_write_wavs_rounding_of_the_f32_output(dev, up, down):
    x = np.random.default_rng(5).uniform(-1, 1, (3, 3001)).astype(np.float32)
    x[1] *= 1.7                                                                       # overshoots +-1: both clips occur
    x[2, :1500] = 1.0                                                                 # a full-scale plateau: +1.0 -> 32767
    x[2, 1500:] = -1.0
    xt = torch.from_numpy(x).to(dev)
    filt = _table(up, down, dev)
    y32 = P.kernels.resample_poly(xt, filt, up, down).cpu().numpy()
    y16 = P.kernels.resample_poly(xt, filt, up, down, out_fmt="s16")
    assert y16.dtype == torch.int16 and y16.shape == y32.shape
    want = np.clip(np.rint(y32.astype(np.float64) * 32768.0), -32768, 32767).astype(np.int16)
    assert np.array_equal(y16.cpu().numpy(), want)
    assert (y32 * 32768.0 > 32767.5).any() and (y32 * 32768.0 < -32768.5).any() and want.max() == 32767 and want.min() == -32768
    rate_in, rate_out = 11025 * down, 11025 * up
    assert torch.equal(RS.resample(xt, rate_in, rate_out, out_s16=True), y16)
    same = RS.resample(xt, 11025, 11025, out_s16=True).cpu().numpy()                  # equal rates: only the rounding
    assert np.array_equal(same, np.clip(np.rint(x.astype(np.float64) * 32768.0), -32768, 32767).astype(np.int16))


def test_wrapper_refusals(dev):
    x = torch.zeros(2, 100, device=dev)
    with pytest.raises(P.lib.AvsepError):
        P.kernels.resample_poly(x, _table(1, 2, dev), 1, 4)                           # another ratio's table
    with pytest.raises(P.lib.AvsepError):
        P.kernels.resample_poly(x.double(), _table(1, 4, dev), 1, 4)
    with pytest.raises(P.lib.AvsepError):
        P.kernels.resample_poly(x.to(torch.int16), _table(1, 4, dev), 1, 4, in_ch=3)
    with pytest.raises(P.lib.AvsepError) as e:
        RS.resample(x, 11024, 11025)
    assert "11024" in str(e.value) and "11025" in str(e.value)
    with pytest.raises(P.lib.AvsepError):
        RS.resample_pcm(x, 48000, 11025)                                              # PCM means int16


# ---------------------------------------------------------------------------------------------------------------------
# 5. command lines
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cli_case(tmp_path_factory):
    """Small nets saved as a checkpoint, a 3 s 48 kHz stereo mix, its 11 025 Hz twin and two frame stacks."""
    d = tmp_path_factory.mktemp("resample_cli")
    mb = P.ModelBuilder()
    torch.manual_seed(11)
    snd = mb.build_sound(arch="unet5", fc_dim=2, fusion_type="hidsep", att_type="sig")
    frm = mb.build_frame(arch="resnet18dilated", fc_dim=256, pool_type="maxpool")
    torch.save(snd.state_dict(), str(d / "sound.pth"))
    torch.save(frm.state_dict(), str(d / "frame.pth"))
    _write_pcm(str(d / "mix48.wav"), _tone_mix_stereo(3 * 48000, 48000, 8), 48000)
    _write_pcm(str(d / "mix11.wav"), _tone_mix_stereo(3 * 11025, 11025, 8), 11025)
    rng = np.random.default_rng(3)
    T = 5
    stacks = []
    for n in range(2):
        np.save(str(d / f"f{n}.npy"), rng.standard_normal((T, 3, 64, 64)).astype(np.float32))
        np.save(str(d / f"one{n}.npy"), rng.standard_normal((3, 64, 64)).astype(np.float32))
        stacks.append(str(d / f"f{n}.npy"))
    flags = ["--arch_sound", "unet5", "--num_channels", "2", "--vis_channels", "256", "--img_pool", "maxpool", "--not_pool_vis",
             "--fusion_type", "hidsep", "--att_type", "sig", "--weights_sound", str(d / "sound.pth"),
             "--weights_frame", str(d / "frame.pth")]
    return d, flags, stacks, [str(d / f"one{n}.npy") for n in range(2)]


def test_separate_cli_takes_a_48k_stereo_file_and_answers_at_48k(dev, cli_case, tmp_path):
    d, flags, _, ones = cli_case
    argv = ["--wav", str(d / "mix48.wav"), "--frames", *ones, "--binary_mask", "0", *flags]      # ratio masks: never silent
    S.cli(argv + ["--out", str(tmp_path / "file")])
    # the same composition by hand
    args = S.parse_args(argv)
    pcm, rate = S.read_wav_pcm(args.wav)
    assert rate == 48000 and pcm.shape == (144000, 2)
    wav = RS.resample_pcm(torch.from_numpy(pcm).to(dev), rate, args.audRate)
    assert wav.shape == (33075,)
    frames = [torch.from_numpy(np.load(p)).float()[None].to(dev) for p in ones]
    out = S.separate_long(_nets(args, dev), wav, frames, args)
    F = 33075 // 256 + 1
    assert out["wavs"].shape == (2, 256 * (F - 1))
    pcm_out = RS.resample(out["wavs"], args.audRate, rate, out_s16=True).cpu().numpy()
    assert pcm_out.shape == (2, math.ceil(256 * (F - 1) * 640 / 147)) and np.abs(pcm_out).max() > 300
    for n in range(2):
        got, r = S.read_wav_pcm(str(tmp_path / "file" / f"source{n}.wav"))
        assert r == 48000 and got.shape == (pcm_out.shape[1], 1)
        S.write_wav_pcm(str(tmp_path / f"hand{n}.wav"), pcm_out[n], rate)
        assert _bytes(tmp_path / "file" / f"source{n}.wav") == _bytes(tmp_path / f"hand{n}.wav")
    # --out_rate model: the model's rate, through write_wav as for a file that needs no resampling
    S.cli(argv + ["--out", str(tmp_path / "model"), "--out_rate", "model"])
    for n, w in enumerate(out["wavs"].cpu().numpy()):
        S.write_wav(str(tmp_path / f"hand_model{n}.wav"), w, 11025)
        assert _bytes(tmp_path / "model" / f"source{n}.wav") == _bytes(tmp_path / f"hand_model{n}.wav")
        assert S.wav_rate(str(tmp_path / "model" / f"source{n}.wav")) == 11025


def test_separate_cli_leaves_a_file_at_the_models_rate_alone(dev, cli_case, tmp_path):
    d, flags, _, ones = cli_case
    argv = ["--wav", str(d / "mix11.wav"), "--frames", *ones, "--binary_mask", "0", *flags]
    S.cli(argv + ["--out", str(tmp_path / "cli")])
    args = S.parse_args(argv)
    data, rate = S.read_wav(args.wav)
    assert rate == 11025
    frames = [torch.from_numpy(np.load(p)).float()[None].to(dev) for p in ones]
    out = S.separate_long(_nets(args, dev), torch.from_numpy(data).to(dev), frames, args)
    for n, w in enumerate(out["wavs"].cpu().numpy()):
        S.write_wav(str(tmp_path / f"hand{n}.wav"), w, rate)
        assert _bytes(tmp_path / "cli" / f"source{n}.wav") == _bytes(tmp_path / f"hand{n}.wav")


def test_localise_cli_takes_a_48k_file(dev, cli_case, tmp_path):
    d, flags, stacks, _ = cli_case
    argv = ["--wav", str(d / "mix48.wav"), "--frames", *stacks, "--fps", "2", *flags]
    got = L.cli(argv + ["--out", str(tmp_path / "loc")])
    args = L.parse_args(argv)
    pcm, rate = S.read_wav_pcm(args.wav)
    wav = RS.resample_pcm(torch.from_numpy(pcm).to(dev), rate, args.audRate)
    frames = [torch.from_numpy(np.load(p)).float().to(dev) for p in stacks]
    times = torch.arange(5, dtype=torch.float64) / 2.0
    want = L.localise(_nets(args, dev), wav, frames, times, args)
    assert torch.equal(got["maps"], want["maps"]) and torch.equal(got["overlays"], want["overlays"])
    assert np.array_equal(np.load(str(tmp_path / "loc" / "maps.npy")), want["maps"].cpu().numpy())
    assert want["maps"].shape == (5, 2, 4, 4)


def test_cli_refuses_a_rate_outside_the_limit(cli_case, tmp_path):
    d, flags, stacks, ones = cli_case
    _write_pcm(str(tmp_path / "odd.wav"), np.zeros((2000, 1), np.int16), 11024)
    with pytest.raises(SystemExit) as e:
        S.cli(["--wav", str(tmp_path / "odd.wav"), "--frames", *ones, *flags])
    assert "11024" in str(e.value) and "1280" in str(e.value)
    with pytest.raises(SystemExit):
        L.cli(["--wav", str(tmp_path / "odd.wav"), "--frames", *stacks, "--fps", "2", *flags])
