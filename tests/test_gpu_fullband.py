"""gpu: full-band stems (avsep_band_gains / avsep_band_extend in csrc/fullband.hip, kernels.band_gains / band_extend,
resample.band_extend, separate_long(band_gains=True) and --band full of avsep_amd/separate.py).

Values are compared with the float64 statements of tests/fullband_ref.py under DERIVED bounds, u = 2^-24:

gains.  num and den are sums of B = bins - lo_bin non-negative terms, each term a square: accumulated in any order with B
roundings, on squares rounded once, a sum is off by at most (B + 1) u of itself.  The quotient num / (den + eps) adds one
rounding for the eps add and one for the division: at most (2 B + 4) u.  The square root halves a relative error and adds a
rounding of its own: (B + 3) u; min(1, .) moves nothing apart.  The bound (B + 6) u * ref leaves the second-order terms
room, and is exactly 0 where ref is 0.  (The kernel fuses square and add, which drops one of the roundings.)

join.  out = fma(gi, h, s).  Per output, with T = ceil(M / up) taps:
  e_s  = (T + 2) u sum|x||h| of the stem chain, e_l the same of the low chain (the bound of tests/test_gpu_resample.py);
  e_h  = e_l + u (|h| + e_l)                       file - l, rounded once (0 where j >= Lf: h is the constant 0);
  e_gi = u |gi| + (2 u + 4 u^2) fr |g1 - g0|       fr = num / den rounded once (both operands exact in f32), the
                                                   difference g1 - g0 rounded once, then the rounding of the fma;
  E    = (|gi| + e_gi) e_h + e_gi |h| + e_s        the exact product and sum of the three computed operands;
  |out - ref| <= E + u (|ref| + E)                 the rounding of the final fma.
The low chain's error thus enters weighted by gi.  Where every term is 0 the output is exactly 0.
Bit-for-bit statements carry no tolerance.  Worst |error| / bound seen on an MI355X is recorded in DESIGN.md."""
import json
import math

import numpy as np
import pytest
import torch

import avsep_amd as P
from avsep_amd import levels as LV
from avsep_amd import resample as RS
from avsep_amd import separate as S
from avsep_amd import wavio

import fullband_ref as FB
import resample_ref as R
from recipes import (args as _args, file_bytes as _bytes, nets as _nets, small_nets as _small_nets, tone_mix as _tone_mix,
                     tone_mix_stereo as _tone_mix_stereo, write_pcm as _write_pcm)
from test_gpu_levels import _check_figures
from test_gpu_resample import _rows

pytestmark = pytest.mark.gpu

K = P.kernels
Err = P.lib.AvsepError


# ---------------------------------------------------------------------------------------------------------------------
# 1. gains
# ---------------------------------------------------------------------------------------------------------------------
def _gains_case(N, G, bins, lo, F, seed):
    """Random masks on a random mixture; frame t is scaled by 1, 1e-3, 1e3 in turn; frame 1 is silent in the band, frame 2
    silent below lo only, in frame 3 source 0 is twice the mixture."""
    g = np.random.default_rng(seed)
    mix = (g.uniform(0, 1, (G, bins, F)) ** 2 * 3.0).astype(np.float32)
    stem = (mix[None] * g.uniform(0, 1, (N, G, bins, F))).astype(np.float32)
    scale = np.array([1.0, 1e-3, 1e3], np.float32)[np.arange(F) % 3]
    mix, stem = mix * scale, stem * scale
    if F > 1:
        mix[:, lo:, 1] = 0.0
        stem[:, :, lo:, 1] = 0.0
    if F > 2:
        mix[:, :lo, 2] = 0.0
        stem[:, :, :lo, 2] = 0.0
    if F > 3:
        stem[0, :, :, 3] = 2.0 * mix[:, :, 3]
    return stem, mix


@pytest.mark.parametrize("bins,lo", [(512, 256), (129, 64), (5, 4)])
def test_gains_vs_float64(dev, bins, lo):
    worst = 0.0
    for F in (1, 2, 63, 64, 65, 257):
        for N, G in ((1, 1), (3, 2), (8, 8), (1, 8), (8, 1), (3, 1)):
            stem, mix = _gains_case(N, G, bins, lo, F, 1000 * bins + 10 * F + N + G)
            st, mt = torch.from_numpy(stem).to(dev), torch.from_numpy(mix).to(dev)
            got_t = K.band_gains(st, mt, lo)
            assert got_t.shape == (N, G, F) and got_t.dtype == torch.float32
            got = got_t.cpu().numpy().astype(np.float64)
            ref = FB.ref_gains(stem, mix, lo)
            bound = FB.gains_bound(ref, bins, lo)
            err = np.abs(got - ref)
            assert (err <= bound).all(), f"bins={bins} lo={lo} F={F} N={N} G={G}: worst {np.max(err - bound):.3e} over the bound"
            live = bound > 0
            worst = max(worst, float((err[live] / bound[live]).max()))
            if F > 1:
                assert (got[:, :, 1] == 0.0).all()                                    # silent in the band
            if F > 2:
                assert (got[:, :, 2] > 0.0).all()                                     # silent below lo only
            if F > 3:
                assert (got[0, :, 3] == 1.0).all() and got.max() <= 1.0               # louder than the mixture
            # a second call, and every (n, g) row alone
            assert torch.equal(K.band_gains(st, mt, lo), got_t)
            if F in (2, 65) and N * G <= 8:
                for n in range(N):
                    for gg in range(G):
                        alone = K.band_gains(st[n:n + 1, gg:gg + 1].contiguous(), mt[gg:gg + 1].contiguous(), lo)
                        assert torch.equal(alone[0, 0], got_t[n, gg])
    print(f"band_gains bins={bins} lo={lo}: worst |g - ref| / bound = {worst:.3f}")


def test_gains_default_band_is_the_top_octave(dev):
    stem, mix = _gains_case(2, 2, 512, 256, 65, 5)
    st, mt = torch.from_numpy(stem).to(dev), torch.from_numpy(mix).to(dev)
    assert torch.equal(K.band_gains(st, mt), K.band_gains(st, mt, 256))
    assert not torch.equal(K.band_gains(st, mt), K.band_gains(st, mt, 255))


# ---------------------------------------------------------------------------------------------------------------------
# 2. the join
# ---------------------------------------------------------------------------------------------------------------------
RATIOS = [(4, 1), (2, 1), (640, 147), (320, 147), (1280, 441), (640, 441)]
# hop, F, N, G, Ll - Lm, Lf - Lout: every value of the issue's lists occurs, the largest of each together
CASES = [(256, 33, 3, 2, 700, 0), (64, 5, 1, 1, 0, -3), (64, 2, 2, 2, 700, 5), (256, 5, 2, 1, 0, 5), (64, 33, 3, 1, 0, -3),
         (256, 2, 1, 2, 700, -3)]
KINDS = ("uniform", "impulse0", "ones", "uniform2", "impulseL")


def _join_case(up, down, hop, F, N, G, dLl, dLf, seed):
    Lm = hop * (F - 1)
    Lout = R.out_length(Lm, up, down)
    rs, rl, rf = _rows(Lm, seed), _rows(Lm + dLl, seed + 1), _rows(Lout + dLf, seed + 2)
    stems = np.stack([np.stack([rs[KINDS[(n * G + g) % 5]] for g in range(G)]) for n in range(N)])
    low = np.stack([rl[KINDS[(g + 3) % 5]] for g in range(G)])
    file = np.stack([rf[KINDS[(3 * g) % 5]] for g in range(G)])
    gains = np.random.default_rng(seed + 3).uniform(0, 1, (N, G, F)).astype(np.float32)
    if N * G >= 2:
        gains[0, 0] = 0.0                                                             # a row of exact zeros
        gains[N - 1, G - 1] = 1.0                                                     # and a row of ones
    return stems, low, file, gains, Lm, Lout


def _to(dev, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


@pytest.mark.parametrize("up,down", RATIOS)
def test_join_vs_float64(dev, up, down):
    filt = RS.filter_table(up, down, dev)
    worst = 0.0
    for hop, F, N, G, dLl, dLf in CASES:
        stems, low, file, gains, Lm, Lout = _join_case(up, down, hop, F, N, G, dLl, dLf, 1000 * up + down + hop + F)
        st, lt, ft, gt = _to(dev, stems, low, file, gains)
        out_t = K.band_extend(st, lt, ft, gt, filt, up, down, hop)
        assert out_t.shape == (N, G, Lout) and out_t.dtype == torch.float32
        ref = FB.ref_extend(stems, low, file, gains, up, down, hop)
        bound = FB.extend_bound(ref, up, down)
        err = np.abs(out_t.cpu().numpy().astype(np.float64) - ref["out"])
        bad = err > bound
        assert not bad.any(), (f"{up}/{down} hop={hop} F={F} N={N} G={G} Ll-Lm={dLl} Lf-Lout={dLf}: {int(bad.sum())} outputs miss the "
                               f"bound, first at {np.argwhere(bad)[0]}: |d|={err[bad][0]:.3e} bound={bound[bad][0]:.3e}")
        live = bound > 0
        worst = max(worst, float((err[live] / bound[live]).max()))
        assert np.abs(ref["out"] - ref["s"]).max() > 0.05                             # the high band is really there
        # bit statements: a second call; the resampler's own entry through resample.py; rows alone; past the file's end
        assert torch.equal(K.band_extend(st, lt, ft, gt, filt, up, down, hop), out_t)
        assert torch.equal(RS.band_extend(st, lt, ft, gt, 11025 * down, 11025 * up, hop), out_t)
        plain = RS.resample(st.reshape(N * G, Lm), 11025 * down, 11025 * up).reshape(N, G, Lout)
        assert torch.equal(K.band_extend(st, lt, ft, torch.zeros_like(gt), filt, up, down, hop), plain)
        if N * G >= 2:
            assert torch.equal(out_t[0, 0], plain[0, 0])                              # the row of zero gains
        if dLf < 0:
            assert torch.equal(out_t[:, :, Lout + dLf:], plain[:, :, Lout + dLf:])
            assert not torch.equal(out_t[:, :, :Lout + dLf], plain[:, :, :Lout + dLf])
        for n in range(N):
            for g in range(G):
                alone = K.band_extend(st[n:n + 1, g:g + 1].contiguous(), lt[g:g + 1].contiguous(), ft[g:g + 1].contiguous(),
                                      gt[n:n + 1, g:g + 1].contiguous(), filt, up, down, hop)
                assert torch.equal(alone[0, 0], out_t[n, g]), f"row ({n}, {g}) alone"
    print(f"band_extend {up}/{down}: worst |out - ref| / bound = {worst:.3f}")


def test_join_where_the_rows_do_not_fit_in_lds(dev):
    """1280/441 with N = 8: nine staged rows of a tile pass the staging array, so every tap reads global memory: the same
    values in the same order."""
    up, down, hop, F = 1280, 441, 64, 5
    stems, low, file, gains, Lm, Lout = _join_case(up, down, hop, F, 8, 1, 700, 0, 77)
    st, lt, ft, gt = _to(dev, stems, low, file, gains)
    out_t = RS.band_extend(st, lt, ft, gt, 11025 * down, 11025 * up, hop)
    ref = FB.ref_extend(stems, low, file, gains, up, down, hop)
    err, bound = np.abs(out_t.cpu().numpy().astype(np.float64) - ref["out"]), FB.extend_bound(ref, up, down)
    assert (err <= bound).all()
    for n in (0, 7):                                                                  # the staged form of the same rows
        alone = RS.band_extend(st[n:n + 1].contiguous(), lt, ft, gt[n:n + 1].contiguous(), 11025 * down, 11025 * up, hop)
        assert torch.equal(alone[0], out_t[n])
    print(f"band_extend {up}/{down} N=8 unstaged: worst |out - ref| / bound = {float((err[bound > 0] / bound[bound > 0]).max()):.3f}")


@pytest.mark.parametrize("up,down", [(4, 1), (640, 147)])
def test_join_with_gain_one_returns_the_file(dev, up, down):
    """N = 1, gains = 1, stems = low: l + (file - l) is the file to 2^-23 * max(|file|, |l|)."""
    hop, F, G = 256, 9, 2
    _, low, file, _, Lm, Lout = _join_case(up, down, hop, F, 1, G, 0, 0, 31)
    lt, ft = _to(dev, low, file)
    out = RS.band_extend(lt[None].contiguous(), lt, ft, torch.ones(1, G, F, device=dev), 11025 * down, 11025 * up, hop)
    l = RS.resample(lt, 11025 * down, 11025 * up)
    err = (out[0].double() - ft.double()).abs()
    bound = 2.0 ** -23 * torch.maximum(ft.abs(), l.abs()).double()
    live = bound > 0
    print(f"band_extend {up}/{down} gain 1: worst |out - file| / bound = {(err[live] / bound[live]).max().item():.3f}")
    assert bool((err <= bound).all())


def test_wrapper_refusals(dev):
    up, down, hop, F = 4, 1, 64, 3
    stems, low, file, gains, Lm, Lout = _join_case(up, down, hop, F, 2, 2, 0, 0, 1)
    st, lt, ft, gt = _to(dev, stems, low, file, gains)
    filt = RS.filter_table(up, down, dev)
    ok = dict(stems=st, low=lt, file=ft, gains=gt, filt=filt, up=up, down=down, hop=hop)
    assert K.band_extend(**ok).shape == (2, 2, Lout)
    for change in (dict(stems=st.double()), dict(low=lt.half()), dict(stems=st[0]), dict(low=lt[:1].contiguous()),
                   dict(low=lt[:, :-1].contiguous()), dict(file=ft[None]), dict(gains=gt[:1].contiguous()), dict(gains=gt[:, :, 0]),
                   dict(file=ft.cpu()), dict(gains=gt.cpu()), dict(filt=filt.cpu()), dict(filt=RS.filter_table(2, 1, dev)),
                   dict(stems=st[:1].expand(9, -1, -1).contiguous(), gains=gt[:1].expand(9, -1, -1).contiguous()),
                   dict(up=1, down=4, filt=RS.filter_table(1, 4, dev)), dict(up=1, down=1, filt=RS.filter_table(1, 1, dev)),
                   dict(hop=0), dict(hop=4097), dict(hop=64.5)):
        with pytest.raises(Err):
            K.band_extend(**{**ok, **change})
    with pytest.raises(Err) as e:
        RS.band_extend(st, lt, ft, gt, 48000, 11025, hop)
    assert "48000" in str(e.value) and "11025" in str(e.value)
    with pytest.raises(Err):
        RS.band_extend(st, lt, ft, gt, 11025, 11025, hop)
    with pytest.raises(Err):
        RS.band_extend(st, lt, ft, gt, 11024, 11025, hop)                             # past check_rates
    stem, mix = _gains_case(2, 2, 8, 4, 5, 2)
    sm, mm = _to(dev, stem, mix)
    assert K.band_gains(sm, mm, 4).shape == (2, 2, 5)
    for a, b, lo in ((sm.double(), mm, 4), (sm, mm.double(), 4), (sm[0], mm, 4), (sm, mm[:1].contiguous(), 4), (sm, mm.cpu(), 4),
                     (sm.cpu(), mm.cpu(), 4), (sm[:1].expand(9, -1, -1, -1).contiguous(), mm, 4), (sm, mm, 8), (sm, mm, 0), (sm, mm, 4.0)):
        with pytest.raises(Err):
            K.band_gains(a, b, lo)


# ---------------------------------------------------------------------------------------------------------------------
# 3. separate_long(band_gains=True)
# ---------------------------------------------------------------------------------------------------------------------
def _same(a, b, what):
    if torch.is_tensor(a):
        assert torch.equal(a, b), what
    else:
        assert a == b, what


@pytest.mark.parametrize("keep,wiener", [(False, 0), (True, 0), (True, 1)])
def test_separate_long_band_gains(dev, keep, wiener):
    nets, gen = _small_nets(dev, 3)
    args = _args(binary_mask=0)
    wav = _tone_mix(3 * 11025, 4).to(dev)
    ch = torch.stack([wav, 0.5 * wav.flip(0)]) if keep else None
    frames = [torch.randn(1, 3, 64, 64, generator=gen).to(dev) for _ in range(2)]
    with torch.no_grad():
        base = S.separate_long(nets, wav, frames, args, return_masks=True, channels=ch, wiener=wiener, clamp=False)
        out = S.separate_long(nets, wav, frames, args, return_masks=True, channels=ch, wiener=wiener, clamp=False, band_gains=True)
        assert set(out) == set(base) | {"band_gains"}
        for k in base:
            _same(out[k], base[k], k)
        # the magnitudes that went into the inverse transform, again
        plan = K.Stft(dev, 1022, 256, "reflect")
        st = torch.tensor(out["starts"], dtype=torch.int32, device=dev)
        if keep:
            mag_c, phase_c = plan.stft(ch)
            mags_c, _ = K.mask_stitch(out["masks"], st, out["perms"].to(dev), mag_c, False, 0.5)
            if wiener:
                mags_c, _ = K.mwf(mag_c, phase_c, mags_c, phase_c, iterations=wiener)
            want = K.band_gains(mags_c, mag_c)
        else:
            mag, _ = plan.stft(wav[None])
            mags, _ = K.mask_stitch(out["masks"], st, out["perms"].to(dev), mag[0], False, 0.5)
            want = K.band_gains(mags[:, None].contiguous(), mag)
    g = out["band_gains"]
    assert g.shape == (2, 2 if keep else 1, 3 * 11025 // 256 + 1) and torch.equal(g, want)
    assert 0.0 < g.min().item() and g.max().item() <= 1.0 and g.std().item() > 0.0


# ---------------------------------------------------------------------------------------------------------------------
# 4. command line
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cli_case(tmp_path_factory):
    """Small nets saved as a checkpoint, a 3 s 48 kHz stereo mix (partials below the model's Nyquist on a noise floor that
    fills the band above it), its 11 025 Hz twin and one frame per source: the recipe of test_gpu_channels.py."""
    d = tmp_path_factory.mktemp("fullband_cli")
    mb = P.ModelBuilder()
    torch.manual_seed(11)
    snd = mb.build_sound(arch="unet5", fc_dim=2, fusion_type="hidsep", att_type="sig")
    frm = mb.build_frame(arch="resnet18dilated", fc_dim=256, pool_type="maxpool")
    torch.save(snd.state_dict(), str(d / "sound.pth"))
    torch.save(frm.state_dict(), str(d / "frame.pth"))
    for rate, name in ((48000, "48"), (11025, "11")):
        _write_pcm(str(d / f"mix{name}.wav"), _tone_mix_stereo(3 * rate, rate, 8), rate)
    rng = np.random.default_rng(3)
    for n in range(2):
        np.save(str(d / f"one{n}.npy"), rng.standard_normal((3, 64, 64)).astype(np.float32))
    flags = ["--arch_sound", "unet5", "--num_channels", "2", "--vis_channels", "256", "--img_pool", "maxpool", "--not_pool_vis",
             "--fusion_type", "hidsep", "--att_type", "sig", "--weights_sound", str(d / "sound.pth"),
             "--weights_frame", str(d / "frame.pth"), "--binary_mask", "0"]
    return d, flags, [str(d / f"one{n}.npy") for n in range(2)]


def _by_hand(dev, argv, ones):
    """separate_long and the full-band rows composed from the public pieces -> (args, out, rows [N,C,Lout] unclamped, mix)."""
    args = S.parse_args(argv)
    pcm, rate = S.read_wav_pcm(args.wav)
    pt = torch.from_numpy(pcm).to(dev)
    rows = RS.split_pcm(pt, rate, args.audRate)
    frames = [torch.from_numpy(np.load(p)).float()[None].to(dev) for p in ones]
    out = S.separate_long(_nets(args, dev), rows[0], frames, args, channels=rows[1:], clamp=False, band_gains=True)
    mix = RS.split_pcm(pt, rate, rate)[1:]
    full = RS.band_extend(out["channel_wavs"], rows[1:], mix, out["band_gains"], args.audRate, rate, args.stft_hop)
    return args, out, full, mix


def _share_above(x, rate, hz):
    """Energy of the rows x [C, L] above ``hz``, summed over the rows."""
    spec = np.abs(np.fft.rfft(np.asarray(x, dtype=np.float64), axis=-1)) ** 2
    return float(spec[:, np.fft.rfftfreq(x.shape[-1], 1.0 / rate) > hz].sum())


def test_cli_band_full_on_a_48k_stereo_file(dev, cli_case, tmp_path, capsys):
    d, flags, ones = cli_case
    argv = ["--wav", str(d / "mix48.wav"), "--frames", *ones, "--channels", "keep", *flags]
    S.cli(argv + ["--out", str(tmp_path / "full"), "--band", "full"])
    assert ", full band" in capsys.readouterr().out
    S.cli(argv + ["--out", str(tmp_path / "model")])
    assert "full band" not in capsys.readouterr().out
    args, out, full, mix = _by_hand(dev, argv, ones)
    Lout = math.ceil(out["channel_wavs"].shape[2] * 640 / 147)
    assert full.shape == (2, 2, Lout)
    rows = full.clamp(-1.0, 1.0)
    t0, t1, fr = FB.frame_position(np.arange(Lout), 640, 147, 256, out["band_gains"].shape[2])
    gains = out["band_gains"].cpu().numpy().astype(np.float64)
    mix_np = mix.cpu().numpy()[:, :Lout]
    for n in range(2):
        wavio.write_frames(str(tmp_path / f"hand{n}.wav"), RS.join_frames(rows[n].contiguous(), 48000, 48000, "s16").cpu().numpy(),
                           48000, 2, "s16")
        assert _bytes(tmp_path / "full" / f"source{n}.wav") == _bytes(tmp_path / f"hand{n}.wav")
        got, r = S.read_wav_pcm(str(tmp_path / "full" / f"source{n}.wav"))
        model, _ = S.read_wav_pcm(str(tmp_path / "model" / f"source{n}.wav"))
        assert r == 48000 and got.shape == model.shape == (Lout, 2)
        # energy above 6 kHz: what the gains hand over of the mixture's, and essentially none without them
        gi = gains[n][:, t0] + fr * (gains[n][:, t1] - gains[n][:, t0])               # [C, Lout]
        hi_full = _share_above(got.T / 32768.0, 48000, 6000.0)
        hi_model = _share_above(model.T / 32768.0, 48000, 6000.0)
        hi_want = sum((gi[c] ** 2).mean() * _share_above(mix_np[c:c + 1], 48000, 6000.0) for c in range(2))
        print(f"source {n}: energy above 6 kHz full {hi_full:.4e}, mean(gi^2) * mixture's {hi_want:.4e}, model {hi_model:.4e} "
              f"({hi_model / hi_full:.2e} of full)")
        assert 0.5 * hi_want <= hi_full <= 2.0 * hi_want
        assert hi_model < 1e-4 * hi_full


def test_cli_band_full_at_the_models_rate_is_band_model(dev, cli_case, tmp_path, capsys):
    d, flags, ones = cli_case
    argv = ["--wav", str(d / "mix11.wav"), "--frames", *ones, "--channels", "keep", *flags]
    S.cli(argv + ["--out", str(tmp_path / "full"), "--band", "full"])
    said = capsys.readouterr().out
    assert "--band model" in said and ", full band" not in said
    S.cli(argv + ["--out", str(tmp_path / "model")])
    for n in range(2):
        assert _bytes(tmp_path / "full" / f"source{n}.wav") == _bytes(tmp_path / "model" / f"source{n}.wav")


def test_cli_band_full_with_a_peak_ceiling(dev, cli_case, tmp_path):
    d, flags, ones = cli_case
    argv = ["--wav", str(d / "mix48.wav"), "--frames", *ones, "--channels", "keep", *flags]
    S.cli(argv + ["--out", str(tmp_path / "o"), "--band", "full", "--peak", "-1", "--out_format", "f32"])
    rep = json.loads(_bytes(tmp_path / "o" / "levels.json"))
    args, out, full, mix = _by_hand(dev, argv, ones)
    m, mm = LV.measure(full, 48000), LV.measure(mix, 48000)
    gain, by = LV.output_gain(mm["integrated"][0], m["true_peak"], None, -1.0)
    assert rep["limited_by"] == by and abs(rep["gain_db"] - 20.0 * math.log10(gain)) < 1e-9
    for n in range(2):
        for c in range(2):
            want = 20.0 * math.log10(m["true_peak"][n, c].item() * gain)
            assert abs(rep["sources"][n]["true_peak_dbtp"][c] - want) < 1e-9
        raw, info = wavio.read_frames(str(tmp_path / "o" / f"source{n}.wav"))
        assert info.rate == 48000 and info.channels == 2
        hand = RS.join_frames((full[n] * gain).contiguous(), 48000, 48000, "f32").cpu().numpy()
        assert np.array_equal(raw, hand)
    # and they are not the peaks of the band-limited rows
    plain = LV.measure(RS.resample(out["channel_wavs"].reshape(4, -1), args.audRate, 48000).reshape(2, 2, -1), 48000)
    assert not torch.equal(plain["true_peak"], m["true_peak"])


def test_cli_band_full_with_levels_reports_and_changes_nothing(dev, cli_case, tmp_path):
    """--band full --levels: the files are those of --band full alone, and the report holds the figures of the clamped
    full-band rows and of the file's channels, under no gain."""
    d, flags, ones = cli_case
    argv = ["--wav", str(d / "mix48.wav"), "--frames", *ones, "--channels", "keep", *flags]
    S.cli(argv + ["--out", str(tmp_path / "full"), "--band", "full"])
    S.cli(argv + ["--out", str(tmp_path / "lv"), "--band", "full", "--levels"])
    assert not (tmp_path / "full" / "levels.json").exists()
    for n in range(2):
        assert _bytes(tmp_path / "lv" / f"source{n}.wav") == _bytes(tmp_path / "full" / f"source{n}.wav")
    rep = json.loads(_bytes(tmp_path / "lv" / "levels.json"))
    assert rep["gain_db"] == 0.0 and rep["limited_by"] is None and rep["rate"] == 48000 and len(rep["sources"]) == 2
    args, out, full, mix = _by_hand(dev, argv, ones)
    m = LV.measure(full.clamp(-1.0, 1.0), 48000)
    for n in range(2):
        _check_figures(rep["sources"][n], m, n)
    _check_figures(rep["mixture"], LV.measure(mix, 48000), 0)
