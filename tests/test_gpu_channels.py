"""gpu: keeping a recording's channels (avsep_mask_stitch with C channels in csrc/longform.hip, avsep_resample_split / _join in
csrc/resample.hip, separate_long(channels=...) and --channels keep of avsep_amd/separate.py).

Every comparison is torch.equal / equal bytes against the same result composed from the entry points that were there
before: the new kernels share their arithmetic (one __device__ body per file), so identity is derived, not a tolerance.
The values of those older entry points are held to float64 restatements in test_gpu_longform.py and test_gpu_resample.py."""
import math

import numpy as np
import pytest
import torch

import avsep_amd as P
from avsep_amd import resample as RS
from avsep_amd import separate as S
from recipes import (args as _args, file_bytes as _bytes, nets as _nets, random_perms as _random_perms,
                     small_nets as _small_nets, starts_t as _starts_t, tone_mix as _tone_mix,
                     tone_mix_stereo as _tone_mix_stereo, write_pcm as _write_pcm)

pytestmark = pytest.mark.gpu

W = 256            # frames per window
FOUT = 256         # warped bins
FIN = 512          # linear bins of the 1022-point STFT


# ---------------------------------------------------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------------------------------------------------
def _stitch_case(dev, C, N, fin, fout, width, Fr, stride, binary, seed):
    g = torch.Generator().manual_seed(seed)
    starts = S.plan_windows(Fr, stride, width)
    Kw = len(starts)
    masks = torch.rand(Kw, N, fout, width, generator=g).to(dev)
    mag_c = (torch.rand(C, fin, Fr, generator=g) ** 2 * 3.0).to(dev)
    perm = torch.tensor(_random_perms(Kw, N, seed + 1), dtype=torch.int32, device=dev)
    st = _starts_t(starts, dev)
    out, lin = P.kernels.mask_stitch_channels(masks, st, perm, mag_c, binary, 0.5, want_mask=True)
    assert out.shape == (N, C, fin, Fr) and lin.shape == (N, fin, Fr)
    for c in range(C):
        want, want_lin = P.kernels.mask_stitch(masks, st, perm, mag_c[c].contiguous(), binary, 0.5, want_mask=True)
        assert torch.equal(out[:, c], want), f"channel {c}"
        assert torch.equal(lin, want_lin)
    assert out.abs().max().item() > 0.1                                               # not a silent agreement
    if binary:                                                                        # mag or nothing
        assert bool(((out == 0) | (out == mag_c[None])).all())
    out2, none = P.kernels.mask_stitch_channels(masks, st, perm, mag_c, binary, 0.5)  # the optional output may be left out
    assert none is None and torch.equal(out, out2)


@pytest.mark.parametrize("binary", [False, True])
@pytest.mark.parametrize("Fr,stride", [(600, 128), (600, 64), (300, 256), (100, 128)])
@pytest.mark.parametrize("N", [2, 3])
@pytest.mark.parametrize("C", [1, 2, 3])
def test_stitch_channels_is_mask_stitch_per_channel(dev, C, N, Fr, stride, binary):
    """F = 600: several blocks along time, one to four covering windows; F = 300: a right-aligned last window; F = 100: one
    window reaching past the recording.  Random permutation tables."""
    _stitch_case(dev, C, N, FIN, FOUT, W, Fr, stride, binary, 1000 * C + 100 * N + Fr + stride)


@pytest.mark.parametrize("binary", [False, True])
def test_stitch_channels_odd_sizes(dev, binary):
    """Fin = 37 (a row tail of 5 in the last workgroup) with F = 75 (a frame tail), W = 32, Fout = 16, stride 16."""
    _stitch_case(dev, 2, 2, 37, 16, 32, 75, 16, binary, 5)


def _pcm(L, C, seed):
    pcm = np.random.default_rng(seed).integers(-32768, 32768, size=(L, C)).astype(np.int16)
    pcm[:3] = np.array([-32768, 32767, 0], np.int16)[:, None]
    return pcm


@pytest.mark.parametrize("up,down", [(147, 640), (1, 4), (1, 1), (1, 1280)])
@pytest.mark.parametrize("C", [1, 2, 6])
def test_split_rows_are_the_existing_paths(dev, C, up, down):
    """Row 0 is resample_pcm's down-mix, row 1 + c is the f32 path fed channel c over 32768; 1/1280 takes the kernel's
    unstaged mode, 1/1 the unit-impulse table (the converted samples themselves)."""
    rate_in, rate_out = 11025 * down, 11025 * up
    pcm = torch.from_numpy(_pcm(30011, C, 10 * C + up)).to(dev)
    rows = RS.split_pcm(pcm, rate_in, rate_out)
    assert rows.dtype == torch.float32 and rows.shape == (1 + C, RS.out_length(30011, up, down))
    assert torch.equal(rows[0], RS.resample_pcm(pcm, rate_in, rate_out))
    for c in range(C):
        x = (pcm[:, c].float() / 32768)[None].contiguous()
        assert torch.equal(rows[1 + c], RS.resample(x, rate_in, rate_out)[0]), f"channel {c}"
    assert rows.abs().max().item() > 1e-3            # not silent (white noise through a 1/1280 low-pass keeps ~0.016 rms)
    if C > 1:
        assert not torch.equal(rows[1], rows[2])
    if up == down:
        assert torch.equal(rows[1:], pcm.t().float() / 32768)
    assert torch.equal(RS.split_pcm(pcm, rate_in, rate_out), rows)                   # a second call: the same bits


@pytest.mark.parametrize("up,down", [(640, 147), (4, 1), (1, 1), (1280, 1)])
@pytest.mark.parametrize("C", [1, 2, 6])
def test_join_is_the_s16_output_interleaved(dev, C, up, down):
    """Column c is resample(x[c], out_s16=True); values overshoot +-1 (both clips occur) and a row holds full-scale plateaus."""
    rate_in, rate_out = 11025 * down, 11025 * up
    x = np.random.default_rng(20 * C + up).uniform(-1, 1, (C, 7001)).astype(np.float32)
    x[0] *= 1.7
    x[-1, :3000] = 1.0
    x[-1, 3000:6000] = -1.0
    xt = torch.from_numpy(x).to(dev)
    got = RS.join_pcm(xt, rate_in, rate_out)
    assert got.dtype == torch.int16 and got.shape == (RS.out_length(7001, up, down), C) and got.is_contiguous()
    want = RS.resample(xt, rate_in, rate_out, out_s16=True).t()
    assert torch.equal(got, want)
    assert got.max().item() == 32767 and got.min().item() == -32768
    y32 = P.kernels.resample_poly(xt, RS.filter_table(up, down, dev), up, down) * 32768.0
    assert (y32 > 32767.5).any() and (y32 < -32768.5).any()
    assert torch.equal(RS.join_pcm(xt, rate_in, rate_out), got)                      # a second call: the same bits


def test_join_where_the_tile_does_not_fit_in_lds(dev):
    """Decimation: 1/4 with six rows staged side by side leaves the staged mode, 1/1280 leaves it for any C."""
    for (up, down), C, Ln in (((1, 4), 6, 30011), ((1, 1280), 2, 30011), ((147, 640), 2, 30011)):
        x = torch.from_numpy(np.random.default_rng(Ln + C).uniform(-1.2, 1.2, (C, Ln)).astype(np.float32)).to(dev)
        got = RS.join_pcm(x, 11025 * down, 11025 * up)
        assert torch.equal(got, RS.resample(x, 11025 * down, 11025 * up, out_s16=True).t())


def test_split_and_join_wrapper_refusals(dev):
    with pytest.raises(P.lib.AvsepError):
        P.kernels.resample_split(torch.zeros(400, dtype=torch.uint8, device=dev), RS.filter_table(1, 2, dev), 1, 4, 2, "s16")
    with pytest.raises(P.lib.AvsepError):
        P.kernels.resample_join(torch.zeros(2, 100, device=dev), RS.filter_table(1, 2, dev), 1, 4, "s16")
    with pytest.raises(P.lib.AvsepError):
        P.kernels.resample_split(torch.zeros(1800, dtype=torch.uint8, device=dev), RS.filter_table(1, 4, dev), 1, 4, 9, "s16")
    with pytest.raises(P.lib.AvsepError):
        P.kernels.resample_join(torch.zeros(9, 100, device=dev), RS.filter_table(1, 4, dev), 1, 4, "s16")


# ---------------------------------------------------------------------------------------------------------------------
# separate_long(channels=...)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("binary,use_vis", [(1, True), (0, True), (1, False)])
def test_separate_long_with_channels(dev, binary, use_vis):
    """3 s of audio, channels = (wav, wav / 2): nothing on the mono path moves, channel_wavs is the composition by hand from
    mask_stitch per channel and one iSTFT over N*C rows, and the half-scale channel is half the full-scale one (1e-6
    absolute, the bound of test_one_tile_equals_reconstruct; a power of two passes every linear stage exactly)."""
    nets, gen = _small_nets(dev, 3)
    args = _args(binary_mask=binary)
    wav = _tone_mix(3 * 11025, 4).to(dev)
    ch = torch.stack([wav, 0.5 * wav])
    frames = [torch.randn(1, 3, 64, 64, generator=gen).to(dev) for _ in range(2)] if use_vis else None
    with torch.no_grad():
        base = S.separate_long(nets, wav, frames, args, use_vis=use_vis, return_masks=True)
        out = S.separate_long(nets, wav, frames, args, use_vis=use_vis, return_masks=True, channels=ch)
        assert "channel_wavs" not in base
        for k in ("wavs", "masks", "lin_masks"):
            assert torch.equal(out[k], base[k]), k
        assert torch.equal(out["perms"], base["perms"]) and out["starts"] == base["starts"]
        plan = P.kernels.Stft(dev, 1022, 256, "reflect")
        mag_c, phase_c = plan.stft(ch)
        Fr = mag_c.shape[2]
        st = _starts_t(out["starts"], dev)
        mags = torch.stack([P.kernels.mask_stitch(out["masks"], st, out["perms"].to(dev), mag_c[c].contiguous(), bool(binary), 0.5)[0]
                            for c in range(2)], 1).contiguous()
        assert mags.shape == (2, 2, FIN, Fr)
        hand = plan.istft(mags.reshape(4, FIN, Fr), phase_c[None].expand(2, -1, -1, -1).reshape(4, FIN, Fr).contiguous())
        hand = hand.clamp_(-1.0, 1.0).reshape(2, 2, -1)
    cw = out["channel_wavs"]
    assert cw.shape == (2, 2, 256 * (Fr - 1)) and torch.equal(cw, hand)
    err = (cw[:, 1] - 0.5 * cw[:, 0]).abs().max().item()
    print(f"binary={binary} use_vis={use_vis}: |half-scale channel - half of full-scale| = {err:.3e}, peak {cw.abs().max().item():.3f}")
    assert err <= 1e-6
    if not binary:
        assert cw.abs().max().item() > 1e-3                                           # ratio masks: never silent


def test_separate_long_refuses_bad_channels(dev):
    nets, gen = _small_nets(dev, 3)
    args = _args()
    wav = _tone_mix(3 * 11025, 4).to(dev)
    frames = [torch.randn(1, 3, 64, 64, generator=gen).to(dev) for _ in range(2)]
    for bad in (wav, torch.stack([wav, wav])[:, :-1], torch.stack([wav, wav]).double(), torch.stack([wav, wav]).cpu(),
                torch.stack([wav, wav])[None]):
        with pytest.raises(P.lib.AvsepError):
            S.separate_long(nets, wav, frames, args, channels=bad)


# ---------------------------------------------------------------------------------------------------------------------
# command line
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cli_case(tmp_path_factory):
    """Small nets saved as a checkpoint, a 3 s 48 kHz stereo mix, its 11 025 Hz twin, their first channels as mono files
    and one frame per source (the recipe of test_gpu_resample.py)."""
    d = tmp_path_factory.mktemp("channels_cli")
    mb = P.ModelBuilder()
    torch.manual_seed(11)
    snd = mb.build_sound(arch="unet5", fc_dim=2, fusion_type="hidsep", att_type="sig")
    frm = mb.build_frame(arch="resnet18dilated", fc_dim=256, pool_type="maxpool")
    torch.save(snd.state_dict(), str(d / "sound.pth"))
    torch.save(frm.state_dict(), str(d / "frame.pth"))
    for rate, name in ((48000, "48"), (11025, "11")):
        pcm = _tone_mix_stereo(3 * rate, rate, 8)
        _write_pcm(str(d / f"mix{name}.wav"), pcm, rate)
        _write_pcm(str(d / f"mono{name}.wav"), pcm[:, :1], rate)
    rng = np.random.default_rng(3)
    for n in range(2):
        np.save(str(d / f"one{n}.npy"), rng.standard_normal((3, 64, 64)).astype(np.float32))
    flags = ["--arch_sound", "unet5", "--num_channels", "2", "--vis_channels", "256", "--img_pool", "maxpool", "--not_pool_vis",
             "--fusion_type", "hidsep", "--att_type", "sig", "--weights_sound", str(d / "sound.pth"),
             "--weights_frame", str(d / "frame.pth"), "--binary_mask", "0"]                       # ratio masks: never silent
    return d, flags, [str(d / f"one{n}.npy") for n in range(2)]


def test_cli_keeps_the_channels_of_a_48k_stereo_file(dev, cli_case, tmp_path, capsys):
    d, flags, ones = cli_case
    argv = ["--wav", str(d / "mix48.wav"), "--frames", *ones, "--channels", "keep", *flags]
    S.cli(argv + ["--out", str(tmp_path / "file")])
    assert "2 channels" in capsys.readouterr().out
    # the same composition by hand
    args = S.parse_args(argv)
    pcm, rate = S.read_wav_pcm(args.wav)
    assert rate == 48000 and pcm.shape == (144000, 2)
    rows = RS.split_pcm(torch.from_numpy(pcm).to(dev), rate, args.audRate)
    assert rows.shape == (3, 33075)
    frames = [torch.from_numpy(np.load(p)).float()[None].to(dev) for p in ones]
    out = S.separate_long(_nets(args, dev), rows[0], frames, args, channels=rows[1:])
    F = 33075 // 256 + 1
    assert out["channel_wavs"].shape == (2, 2, 256 * (F - 1))
    Lout = math.ceil(256 * (F - 1) * 640 / 147)
    for n in range(2):
        got, r = S.read_wav_pcm(str(tmp_path / "file" / f"source{n}.wav"))
        assert r == 48000 and got.shape == (Lout, 2)
        hand = RS.join_pcm(out["channel_wavs"][n], args.audRate, rate).cpu().numpy()
        S.write_wav_pcm_channels(str(tmp_path / f"hand{n}.wav"), hand, rate)
        assert _bytes(tmp_path / "file" / f"source{n}.wav") == _bytes(tmp_path / f"hand{n}.wav")
        # a stereo image: a down-mix copied into both channels would be equal columns
        assert np.abs(got).max() > 300 and np.abs(got[:, 0].astype(np.int32) - got[:, 1]).max() > 300
    # --out_rate model: the channels at the model's rate
    S.cli(argv + ["--out", str(tmp_path / "model"), "--out_rate", "model"])
    for n in range(2):
        got, r = S.read_wav_pcm(str(tmp_path / "model" / f"source{n}.wav"))
        assert r == 11025 and got.shape == (256 * (F - 1), 2)
        want = np.clip(np.rint(out["channel_wavs"][n].cpu().numpy().astype(np.float64) * 32768.0), -32768, 32767).astype(np.int16).T
        assert np.array_equal(got, want)


def test_cli_keeps_the_channels_of_a_file_at_the_models_rate(dev, cli_case, tmp_path):
    d, flags, ones = cli_case
    argv = ["--wav", str(d / "mix11.wav"), "--frames", *ones, "--channels", "keep", *flags]
    S.cli(argv + ["--out", str(tmp_path / "cli")])
    data, rate = S.read_wav(str(d / "mix11.wav"))
    pcm, _ = S.read_wav_pcm(str(d / "mix11.wav"))
    rows = RS.split_pcm(torch.from_numpy(pcm).to(dev), rate, 11025)
    assert rate == 11025 and np.array_equal(rows[0].cpu().numpy(), data)             # the network hears read_wav's array
    assert np.array_equal(rows[1:].cpu().numpy(), pcm.T.astype(np.float32) / 32768.0)
    args = S.parse_args(argv)
    frames = [torch.from_numpy(np.load(p)).float()[None].to(dev) for p in ones]
    out = S.separate_long(_nets(args, dev), rows[0], frames, args, channels=rows[1:])
    for n in range(2):
        got, r = S.read_wav_pcm(str(tmp_path / "cli" / f"source{n}.wav"))
        assert r == 11025 and got.shape == (out["channel_wavs"].shape[2], 2)
        assert np.array_equal(got, RS.join_pcm(out["channel_wavs"][n], 11025, 11025).cpu().numpy())
        assert np.abs(got[:, 0].astype(np.int32) - got[:, 1]).max() > 300


@pytest.mark.parametrize("name", ["mono48", "mono11"])
def test_cli_keep_on_a_mono_file_writes_what_mix_writes(dev, cli_case, tmp_path, name):
    """C = 1: the same STFT row count, the same stitch bits, the same iSTFT rows, and join with one channel is the s16
    output (at the model's rate: write_wav's rounding)."""
    d, flags, ones = cli_case
    argv = ["--wav", str(d / f"{name}.wav"), "--frames", *ones, *flags]
    S.cli(argv + ["--out", str(tmp_path / "mix")])
    S.cli(argv + ["--out", str(tmp_path / "keep"), "--channels", "keep"])
    for n in range(2):
        a, b = _bytes(tmp_path / "mix" / f"source{n}.wav"), _bytes(tmp_path / "keep" / f"source{n}.wav")
        assert len(a) > 44 + 2 * 30000 and a == b
