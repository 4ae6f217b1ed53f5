"""gpu: csrc/levels.hip and avsep_amd/levels.py against the float64 reference tests/levels_ref.py, and the level flags of
avsep_amd.separate.  Bounds are the reference's derived ones (levels_ref.energy_bound, levels_ref.true_peak); the worst
ratios are printed (pytest -s) before they are asserted."""
import json
import math
import wave

import numpy as np
import pytest
import torch

import avsep_amd as P
from avsep_amd import levels as LV
from avsep_amd import resample as RS
from avsep_amd import separate as S
from avsep_amd import wavio as W
from avsep_amd.lib import AvsepError

import levels_ref as REF
from recipes import file_bytes as _bytes, nets as _nets, tone_mix_panned as _tone_mix

pytestmark = pytest.mark.gpu

RATES = (8000, 11025, 48000)


def _lengths(rate):
    h = REF.sub_block(rate)
    return [h, 4 * h, 4 * h + 1, 13 * h + 517] + ([40 * h + 3] if rate == 11025 else [])


def _rows(rate, L, seed=0):
    """float32 [7, L]: two seeded uniform rows, a 997 Hz sine, a unit impulse at sample 0 and one at L - 1, all ones (after the
    high-pass has swallowed the step every later sub-block's energy is inherited state and nothing else), all zeros."""
    g = np.random.default_rng(seed + rate + L)
    x = np.zeros((7, L), dtype=np.float32)
    x[0], x[1] = g.uniform(-1, 1, L), g.uniform(-1, 1, L)
    x[2] = np.sin(2 * np.pi * 997.0 * np.arange(L) / rate)
    x[3, 0] = 1.0
    x[4, L - 1] = 1.0
    x[5] = 1.0
    return x


_cache = {}


def _energy_case(rate, L, dev):
    """(x, the kernel's E, the reference's E and per-element bound), computed once per (rate, L)."""
    key = (rate, L)
    if key not in _cache:
        x = _rows(rate, L)
        h = REF.sub_block(rate)
        E = P.kernels.loudness_energies(torch.from_numpy(x).to(dev), LV.k_weighting(rate), h)
        want, A = REF.energies(x.astype(np.float64), rate)
        bound = np.stack([REF.energy_bound(rate, float(np.abs(x[r]).max()), A[r], h) for r in range(x.shape[0])])
        _cache[key] = (x, E, want, bound)
    return _cache[key]


@pytest.mark.parametrize("rate,L", [(r, L) for r in RATES for L in _lengths(r)])
def test_energies_are_inside_the_bound(dev, rate, L):
    x, E, want, bound = _energy_case(rate, L, dev)
    h = REF.sub_block(rate)
    assert E.dtype == torch.float64 and tuple(E.shape) == (7, L // h) == want.shape
    got = E.cpu().numpy()
    assert np.isfinite(got).all()
    err = np.abs(got - want)
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    print(f"energies rate={rate} L={L}: worst |E - E_ref| / bound = {ratio.max():.3e} (row {ratio.max(1).argmax()}), "
          f"worst relative {np.max(err / np.maximum(want, 1e-300) * (want > 1e-12)):.3e}")
    assert (got[6] == 0.0).all(), "a silent row has no energy at all"
    assert (err <= bound).all(), f"worst ratio to the bound {ratio.max():.3e}"
    if L >= 2 * h:
        assert (want[5, 1:] > 0).all() and (got[5, 1:] > 0).all()


def test_energies_do_not_depend_on_the_batch_the_call_or_the_length(dev):
    rate = 11025
    h = REF.sub_block(rate)
    L = 13 * h + 517
    x, E, _, _ = _energy_case(rate, L, dev)
    xd = torch.from_numpy(x).to(dev)
    sos = LV.k_weighting(rate)
    for r in (1, 5):
        alone = P.kernels.loudness_energies(xd[r:r + 1].contiguous(), sos, h)
        assert torch.equal(alone[0], E[r])
        assert torch.equal(P.kernels.loudness_energies(xd[[0, r, 2]].contiguous(), sos, h)[1], E[r])        # another row offset: L is odd
        assert torch.equal(P.kernels.loudness_energies(xd[[4, 3, 0, 2, r]].contiguous(), sos, h)[4], E[r])
    assert torch.equal(P.kernels.loudness_energies(xd, sos, h), E), "a second call"
    for Ls in (h, 4 * h, 4 * h + 1):
        short = P.kernels.loudness_energies(xd[:, :Ls].contiguous(), sos, h)
        assert torch.equal(short, E[:, :Ls // h]), "the first sub-blocks do not change when L grows"
    long = _energy_case(rate, 40 * h + 3, dev)
    assert torch.equal(long[1][[3, 5, 6], :13], E[[3, 5, 6]]), "impulse, step and silence are the same rows at every L"


PEAK_RATES = (8000, 11025, 48000, 96000, 192000)


def _peak_rows(L, seed):
    g = np.random.default_rng(seed + L)
    x = np.zeros((6, L), dtype=np.float32)
    x[0], x[1] = g.uniform(-1, 1, L), 0.25 * g.standard_normal(L)
    x[2] = np.sin(2 * np.pi * np.arange(L) / 4.0 + np.pi / 4.0)
    x[3, 0] = 1.0
    x[4, L - 1] = -1.0
    return x


@pytest.mark.parametrize("L", [1, 2, 79, 1025, 30011])
@pytest.mark.parametrize("rate", PEAK_RATES)
def test_true_peak_is_inside_the_bound(dev, rate, L):
    x = _peak_rows(L, rate)
    os, taps = LV.peak_table(rate, dev)
    assert os == REF.oversampling(rate) and tuple(taps.shape) == (21, os) and taps.dtype == torch.float64
    peaks = P.kernels.true_peak(torch.from_numpy(x).to(dev), taps, os).cpu().numpy()
    assert peaks.shape == (6, 2) and peaks.dtype == np.float64
    worst = 0.0
    for r in range(6):
        sample, peak, bound = REF.true_peak(x[r].astype(np.float64), rate)
        assert peaks[r, 0] == sample == float(np.abs(x[r]).max()), "the sample peak is exact"
        worst = max(worst, abs(peaks[r, 1] - peak) / bound) if bound > 0 else worst
        assert abs(peaks[r, 1] - peak) <= bound and peaks[r, 1] >= peaks[r, 0], (r, peaks[r, 1], peak, bound)
    print(f"true peak rate={rate} L={L}: worst |peak - ref| / bound = {worst:.3e}")
    assert (peaks[5] == 0.0).all()


@pytest.mark.parametrize("rate", [8000, 11025, 48000, 96000])
def test_true_peak_of_the_quarter_rate_sine(dev, rate):
    x = torch.from_numpy(_peak_rows(4096, 0)[2:3]).to(dev)
    m = LV.measure(x, rate)
    assert abs(20 * math.log10(m["sample_peak"][0, 0].item()) + 3.0103) < 1e-3
    assert -0.4 <= 20 * math.log10(m["true_peak"][0, 0].item()) <= 0.2


@pytest.mark.parametrize("bad", [math.nan, math.inf, -math.inf])
def test_a_non_finite_sample_gives_infinite_peaks_and_measure_raises(dev, bad):
    x = _peak_rows(5000, 1)
    x[1, 4097] = bad
    os, taps = LV.peak_table(48000, dev)
    peaks = P.kernels.true_peak(torch.from_numpy(x).to(dev), taps, os).cpu().numpy()
    assert (peaks[1] == math.inf).all() and np.isfinite(np.delete(peaks, 1, 0)).all()
    with pytest.raises(AvsepError, match="programme 0, channel 1"):
        LV.measure(torch.from_numpy(x).to(dev), 48000)
    with pytest.raises(AvsepError, match="programme 1, channel 0"):
        LV.measure(torch.from_numpy(x[[0, 2, 1, 3]]).to(dev).reshape(2, 2, -1), 48000)


# ---------------------------------------------------------------------------------------------------------------------
# measure end to end
# ---------------------------------------------------------------------------------------------------------------------
def _same_lufs(got, want):
    return got == want if math.isinf(want) or math.isinf(got) else abs(got - want) <= 1e-6


def _check_measure(m, p, x, rate, weights=None):
    want = REF.loudness(x.astype(np.float64), rate, weights)
    got = tuple(m[k][p].item() for k in ("integrated", "momentary_max", "short_term_max"))
    print(f"measure: got {got} reference {want}")
    assert all(_same_lufs(a, b) for a, b in zip(got, want)), (got, want)
    return want


def test_measure_loud_quiet_silent(dev):
    """A 997 Hz sine of amplitude 0.5: ten sub-blocks loud, ten 30 dB down (they pass the absolute gate and fall to the relative
    one), the rest silent, at 11 025 Hz: -9.6946 LUFS by the reference."""
    rate, h = 11025, 1103
    L = 30 * h + 517
    x = (0.5 * np.sin(2 * np.pi * 997.0 * np.arange(L) / rate)).astype(np.float32)
    x[10 * h:20 * h] *= np.float32(10.0 ** (-30.0 / 20.0))
    x[20 * h:] = 0.0
    silent = np.zeros_like(x)
    m = LV.measure(torch.from_numpy(np.stack([x, silent])[:, None]).to(dev), rate)           # two programmes of one channel
    want = _check_measure(m, 0, x[None], rate)
    assert abs(want[0] + 9.6946) < 2e-4 and math.isfinite(want[2])
    assert tuple(m[k][1].item() for k in ("integrated", "momentary_max", "short_term_max")) == (-math.inf,) * 3
    assert tuple(m["energies"].shape) == (2, 1, 30) and m["energies"].dtype == torch.float64 and not m["energies"].is_cuda
    assert tuple(m["true_peak"].shape) == tuple(m["sample_peak"].shape) == (2, 1) and m["sample_peak"][1, 0] == 0
    short = LV.measure(torch.from_numpy(x[None, :29 * h]).to(dev), rate)                      # [C, L]: one programme; S = 29
    assert short["short_term_max"][0].item() == -math.inf and math.isfinite(short["integrated"][0].item())
    _check_measure(short, 0, x[None, :29 * h], rate)
    tiny = LV.measure(torch.from_numpy(x[None, :h - 1]).to(dev), rate)                        # not one sub-block
    assert tiny["energies"].shape[-1] == 0 and tiny["integrated"][0].item() == -math.inf and tiny["sample_peak"][0, 0] > 0.49


def test_measure_weights_and_the_lfe(dev):
    rate = 48000
    g = np.random.default_rng(5)
    L = 31 * 4800 + 17
    two = (0.2 * g.standard_normal((2, L))).astype(np.float32)
    two[1] *= 0.5
    m = LV.measure(torch.from_numpy(two).to(dev), rate, weights=[1.0, 1.41])
    _check_measure(m, 0, two, rate, [1.0, 1.41])
    assert not _same_lufs(m["integrated"][0].item(), REF.loudness(two.astype(np.float64), rate)[0])
    six = (0.05 * g.standard_normal((6, L))).astype(np.float32)
    six[3] = 0.9 * np.sin(2 * np.pi * 60.0 * np.arange(L) / rate)                            # a loud LFE: it must not count
    m6 = LV.measure(torch.from_numpy(six).to(dev), rate)
    want = _check_measure(m6, 0, six, rate)
    quiet = six.copy()
    quiet[3] = 0.0
    assert abs(want[0] - REF.loudness(quiet.astype(np.float64), rate)[0]) < 1e-9
    assert m6["sample_peak"][0, 3].item() > 0.89


# ---------------------------------------------------------------------------------------------------------------------
# separate
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """A tiny random-weight model saved as a checkpoint; a 2 s 48 kHz stereo mixture as a 16-bit file and, eight times as hot
    (so that its stems overshoot full scale), as a float file."""
    d = tmp_path_factory.mktemp("levels_cli")
    mb = P.ModelBuilder()
    torch.manual_seed(11)
    snd = mb.build_sound(arch="unet5", fc_dim=2, fusion_type="hidsep", att_type="sig")
    frm = mb.build_frame(arch="resnet18dilated", fc_dim=256, pool_type="maxpool")
    torch.save(snd.state_dict(), str(d / "sound.pth"))
    torch.save(frm.state_dict(), str(d / "frame.pth"))
    mix = _tone_mix(2 * 48000, 48000, 8)
    pcm = np.clip(np.rint(mix * 32768.0), -32768, 32767).astype(np.int16)
    with wave.open(str(d / "mix16.wav"), "wb") as w:
        w.setnchannels(2); w.setsampwidth(2); w.setframerate(48000)
        w.writeframes(pcm.astype("<i2").tobytes())
    W.write_frames(str(d / "hot.wav"), np.frombuffer((8.0 * mix).astype("<f4").tobytes(), dtype=np.uint8), 48000, 2, "f32")
    rng = np.random.default_rng(3)
    ones = []
    for n in range(2):
        np.save(str(d / f"one{n}.npy"), rng.standard_normal((3, 64, 64)).astype(np.float32))
        ones.append(str(d / f"one{n}.npy"))
    flags = ["--arch_sound", "unet5", "--num_channels", "2", "--vis_channels", "256", "--img_pool", "maxpool", "--not_pool_vis",
             "--fusion_type", "hidsep", "--att_type", "sig", "--weights_sound", str(d / "sound.pth"),
             "--weights_frame", str(d / "frame.pth"), "--frames", *ones, "--binary_mask", "0"]
    return d, flags


def _frames(args, dev):
    return [torch.from_numpy(np.load(p)).float()[None].to(dev) for p in args.frames]


def _read_rows(path, dev):
    raw, info = W.read_frames(str(path))
    return RS.split_frames(torch.from_numpy(raw).to(dev), info.fmt, info.channels, info.rate, info.rate)[1:], info


def test_clamp_false_only_lifts_the_clip(dev, case):
    d, flags = case
    args = S.parse_args(["--wav", str(d / "hot.wav"), "--out", str(d / "unused"), *flags])
    info = W.probe(args.wav)
    wav, channels = S.load_mixture(args.wav, info, args.audRate, dev, keep=True)
    nets, frames = _nets(args, dev), _frames(args, dev)
    a = S.separate_long(nets, wav, frames, args, channels=channels)
    b = S.separate_long(nets, wav, frames, args, channels=channels, clamp=False)
    assert torch.equal(a["perms"], b["perms"]) and a["starts"] == b["starts"]
    for key in ("wavs", "channel_wavs"):
        inside = a[key].abs() < 1.0
        assert torch.equal(a[key][inside], b[key][inside]), key
        assert (~inside).sum().item() > 0, f"{key}: the hot mixture must overshoot for this test to see anything"
        assert (b[key][~inside].abs() >= 1.0).all() and (b[key].abs() > 1.0).sum().item() > 0
        assert torch.equal(b[key].clamp(-1.0, 1.0), a[key])


def test_cli_peak_ceiling_round_trip(dev, case, tmp_path):
    d, flags = case
    out = S.cli(["--wav", str(d / "hot.wav"), "--out", str(tmp_path / "o"), "--peak", "-1", "--out_format", "f32", *flags])
    rep = json.loads(_bytes(tmp_path / "o" / "levels.json"))
    assert rep["rate"] == 48000 and rep["limited_by"] == "peak" and rep["gain_db"] < 0.0 and len(rep["sources"]) == 2
    gain = 10.0 ** (rep["gain_db"] / 20.0)
    assert out["wavs"].abs().max().item() > 1.0, "the stems come back unclamped"
    rows = RS.resample(out["wavs"], 11025, 48000)
    worst = -math.inf
    for n in range(2):
        got, info = _read_rows(tmp_path / "o" / f"source{n}.wav", dev)
        assert info.fmt == "f32" and info.rate == 48000 and info.channels == 1
        m = LV.measure(got, 48000)
        dbtp = 20.0 * math.log10(m["true_peak"].max().item())
        worst = max(worst, dbtp)
        assert dbtp <= -1.0 + 1e-3
        assert torch.equal(got[0], rows[n] * gain) or torch.allclose(got[0], rows[n] * gain, rtol=1e-6, atol=0.0), "one gain for every stem"
        # the report scales the figures measured before the gain; the file holds f32 products, each within 2^-24 of exact:
        # 20 log10(1 + 2^-24) = 5.2e-7 dB
        assert abs(rep["sources"][n]["true_peak_dbtp"][0] - dbtp) < 1e-6
        assert abs(rep["sources"][n]["integrated_lufs"] - m["integrated"][0].item()) < 1e-6
    assert abs(worst + 1.0) < 1e-3, "the loudest stem sits at the ceiling"
    assert set(rep["mixture"]) == {"integrated_lufs", "momentary_max_lufs", "short_term_max_lufs", "true_peak_dbtp", "sample_peak_dbfs"}
    assert rep["mixture"]["short_term_max_lufs"] is None and len(rep["mixture"]["true_peak_dbtp"]) == 1      # 2 s: no 3 s window


def test_cli_loudness_target_keeps_channels(dev, case, tmp_path):
    """The gain is set from the MIXTURE's loudness; the stems' sum misses the mixture by what the separation loses.  The
    written sum may miss -23 LUFS by that much and by the 16-bit rounding of the files (1e-3 LU is three orders above it)."""
    d, flags = case
    out = S.cli(["--wav", str(d / "mix16.wav"), "--out", str(tmp_path / "o"), "--loudness", "-23", "--channels", "keep", *flags])
    rep = json.loads(_bytes(tmp_path / "o" / "levels.json"))
    assert rep["limited_by"] == "loudness" and abs(rep["mixture"]["integrated_lufs"] + 23.0) < 1e-4
    mix, _ = _read_rows(d / "mix16.wav", dev)
    mix_lufs = LV.measure(mix, 48000)["integrated"][0].item()
    assert abs(rep["gain_db"] - (-23.0 - mix_lufs)) < 1e-9 and rep["gain_db"] < 0.0, "a 16-bit file that is turned down cannot clip"
    N, Cc, Lm = out["channel_wavs"].shape
    rows = RS.resample(out["channel_wavs"].reshape(N * Cc, Lm).contiguous(), 11025, 48000).reshape(N, Cc, -1)
    before = abs(LV.measure(rows.sum(0), 48000)["integrated"][0].item() - mix_lufs)
    written = [_read_rows(tmp_path / "o" / f"source{n}.wav", dev) for n in range(2)]
    assert all(info.channels == 2 and info.fmt == "s16" and info.rate == 48000 for _, info in written)
    after = abs(LV.measure(written[0][0] + written[1][0], 48000)["integrated"][0].item() + 23.0)
    print(f"stems' sum against the mixture before {before:.6f} LU, against -23 LUFS after {after:.6f} LU")
    assert after <= before + 1e-3


def test_cli_without_the_flags_writes_the_bytes_it_wrote_before(dev, case, tmp_path):
    d, flags = case
    argv = ["--wav", str(d / "mix16.wav"), *flags]
    S.cli(argv + ["--out", str(tmp_path / "plain")])
    args = S.parse_args(argv + ["--out", str(tmp_path / "old")])
    # separate_long and the branch the command line has always taken for a 16-bit file at another rate than the model's
    wav, _ = S.load_mixture(args.wav, W.probe(args.wav), args.audRate, dev)
    out = S.separate_long(_nets(args, dev), wav, _frames(args, dev), args)
    assert out["wavs"].abs().max().item() <= 1.0
    (tmp_path / "old").mkdir()
    for n, w in enumerate(RS.resample(out["wavs"], args.audRate, 48000, out_s16=True).cpu().numpy()):
        S.write_wav_pcm(str(tmp_path / "old" / f"source{n}.wav"), w, 48000)
    for n in range(2):
        assert _bytes(tmp_path / "plain" / f"source{n}.wav") == _bytes(tmp_path / "old" / f"source{n}.wav")
    assert not (tmp_path / "plain" / "levels.json").exists()
    # --levels reports and changes nothing
    S.cli(argv + ["--out", str(tmp_path / "lv"), "--levels"])
    for n in range(2):
        assert _bytes(tmp_path / "lv" / f"source{n}.wav") == _bytes(tmp_path / "plain" / f"source{n}.wav")
    rep = json.loads(_bytes(tmp_path / "lv" / "levels.json"))
    assert rep["gain_db"] == 0.0 and rep["limited_by"] is None and rep["rate"] == 48000 and len(rep["sources"]) == 2
    m = LV.measure(RS.resample(out["wavs"], args.audRate, 48000)[:, None], 48000)
    for n in range(2):
        assert abs(rep["sources"][n]["integrated_lufs"] - m["integrated"][n].item()) < 1e-9
        assert abs(rep["sources"][n]["true_peak_dbtp"][0] - 20 * math.log10(m["true_peak"][n, 0].item())) < 1e-9


def _check_figures(fig, m, p, tol=1e-9):
    """One entry of levels.json against programme p of an LV.measure result: the loudness figures as they are (None for -inf),
    the peaks per channel in dB."""
    for key in ("integrated", "momentary_max", "short_term_max"):
        got, want = fig[key + "_lufs"], m[key][p].item()
        assert got is None if math.isinf(want) else abs(got - want) < tol, (key, got, want)
    for key, name in (("true_peak", "true_peak_dbtp"), ("sample_peak", "sample_peak_dbfs")):
        assert len(fig[name]) == m[key].shape[1]
        for c, v in enumerate(m[key][p].tolist()):
            assert abs(fig[name][c] - 20.0 * math.log10(v)) < tol, (name, c, fig[name][c], v)


def test_cli_levels_with_kept_channels_reports_and_changes_nothing(dev, case, tmp_path):
    """--levels --channels keep: the files are those of the run without --levels, and the report holds the figures of every
    source's channels (the clamped stems at the output rate, as the join wrote them) and of the file's own channels."""
    d, flags = case
    argv = ["--wav", str(d / "mix16.wav"), "--channels", "keep", *flags]
    S.cli(argv + ["--out", str(tmp_path / "plain")])
    out = S.cli(argv + ["--out", str(tmp_path / "lv"), "--levels"])
    assert not (tmp_path / "plain" / "levels.json").exists()
    for n in range(2):
        assert _bytes(tmp_path / "lv" / f"source{n}.wav") == _bytes(tmp_path / "plain" / f"source{n}.wav")
        assert _read_rows(tmp_path / "lv" / f"source{n}.wav", dev)[1].channels == 2
    rep = json.loads(_bytes(tmp_path / "lv" / "levels.json"))
    assert rep["gain_db"] == 0.0 and rep["limited_by"] is None and rep["rate"] == 48000 and len(rep["sources"]) == 2
    N, Cc, Lm = out["channel_wavs"].shape
    assert (N, Cc) == (2, 2) and out["channel_wavs"].abs().max().item() <= 1.0
    rows = RS.resample(out["channel_wavs"].reshape(N * Cc, Lm).contiguous(), 11025, 48000).reshape(N, Cc, -1)
    m = LV.measure(rows, 48000)
    for n in range(2):
        assert len(rep["sources"][n]["true_peak_dbtp"]) == 2
        _check_figures(rep["sources"][n], m, n)
    _check_figures(rep["mixture"], LV.measure(_read_rows(d / "mix16.wav", dev)[0], 48000), 0)


def test_levels_cli(dev, case, tmp_path, capsys):
    d, _ = case
    res = LV.cli([str(d / "mix16.wav"), str(d / "hot.wav"), "--json", str(tmp_path / "l.json")])
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 2 and all("LUFS" in l and "dBTP" in l and "dBFS" in l for l in lines)
    saved = json.loads(_bytes(tmp_path / "l.json"))
    a, b = saved[str(d / "mix16.wav")], saved[str(d / "hot.wav")]
    assert saved == json.loads(json.dumps(res)) and a["rate"] == 48000 and a["channels"] == 2
    # the float file is the same mixture eight times as hot (the 16-bit file's rounding is 1e-4 of its level)
    assert abs(b["integrated_lufs"] - a["integrated_lufs"] - 20 * math.log10(8.0)) < 1e-3
    mix = _tone_mix(2 * 48000, 48000, 8)
    assert abs(b["sample_peak_dbfs"][0] - 20 * math.log10(np.abs((8.0 * mix[:, 0]).astype(np.float32)).max())) < 1e-9
    assert abs(b["integrated_lufs"] - REF.loudness((8.0 * mix).astype(np.float32).T.astype(np.float64), 48000)[0]) < 1e-6
