"""not-gpu: the host side of full-band stems (--band of separate.py) and the properties of the float64 definitions in
tests/fullband_ref.py that the GPU kernels are held to: the split file = up(down(file)) + high is exact, gains of 0 leave
the resampled stems, the high band is divided (not duplicated) among the sources, and on the two-source signal of DESIGN.md
the full-band stems beat the band-limited ones by more than 2 dB of SDR per source."""
import numpy as np
import pytest

from avsep_amd import separate as S

import fullband_ref as FB
import resample_ref as R
import stftref


def test_cli_band_flag():
    a = S.parse_args(["--wav", "mix.wav", "--audio_only"])
    assert a.band == "model"
    b = S.parse_args(["--wav", "mix.wav", "--audio_only", "--band", "full"])
    assert b.band == "full" and b.out_rate == "file"
    with pytest.raises(SystemExit) as e:
        S.parse_args(["--wav", "mix.wav", "--audio_only", "--band", "full", "--out_rate", "model"])
    assert "--band full" in str(e.value)
    with pytest.raises(SystemExit):
        S.parse_args(["--wav", "mix.wav", "--audio_only", "--band", "wide"])


def _case(N, G, up, down, hop, F, seed, extra_low=0, extra_file=0):
    g = np.random.default_rng(seed)
    Lm = hop * (F - 1)
    Lout = R.out_length(Lm, up, down)
    return (g.uniform(-1, 1, (N, G, Lm)), g.uniform(-1, 1, (G, Lm + extra_low)), g.uniform(-1, 1, (G, Lout + extra_file)),
            g.uniform(0, 1, (N, G, F)))


@pytest.mark.parametrize("up,down", [(4, 1), (640, 147)])
def test_reference_gain_one_returns_the_file(up, down):
    """N = 1, gains = 1, stems = low: up(low) + 1 * (file - up(low)) = file to 1e-12, whatever the file is."""
    _, low, file, _ = _case(1, 2, up, down, 64, 5, 1)
    ref = FB.ref_extend(low[None], low, file, np.ones((1, 2, 5)), up, down, 64)
    assert ref["out"].shape == (1, 2, file.shape[1]) and np.abs(ref["out"][0] - file).max() <= 1e-12


@pytest.mark.parametrize("up,down", [(4, 1), (640, 147)])
def test_reference_gain_zero_returns_the_resampled_stems(up, down):
    stems, low, file, gains = _case(2, 2, up, down, 64, 5, 2, extra_low=100, extra_file=-3)
    ref = FB.ref_extend(stems, low, file, np.zeros_like(gains), up, down, 64)
    for n in range(2):
        for g in range(2):
            want = R.ref_outputs(stems[n, g], up, down, np.arange(ref["out"].shape[2]))[0]
            assert np.array_equal(ref["out"][n, g], want)
    assert not ref["inside"][-3:].any() and ref["inside"][:-3].all()


def test_reference_high_band_is_divided_among_the_sources():
    """sum_n (out_n - s_n) = (sum_n gi_n) * h: one high band, shared out by the gains."""
    stems, low, file, gains = _case(3, 2, 640, 147, 64, 6, 3, extra_low=50)
    ref = FB.ref_extend(stems, low, file, gains, 640, 147, 64)
    lhs = (ref["out"] - ref["s"]).sum(0)
    rhs = ref["gi"].sum(0) * ref["h"]
    assert np.abs(lhs - rhs).max() <= 1e-12 and np.abs(rhs).max() > 0.1
    # the interpolated gain runs through the frames' own gains at the frames' centres: output j = t * hop * up / down
    t0, t1, fr = FB.frame_position(np.arange(ref["out"].shape[2]), 640, 147, 64, 6)
    assert fr.min() >= 0.0 and fr.max() < 1.0 and t0.max() == 4 and t1.max() == 5
    t0, _, fr = FB.frame_position(np.arange(4 * 64 * 5), 4, 1, 64, 6)
    assert np.array_equal(fr[::256], np.zeros(5)) and np.array_equal(t0[::256], np.arange(5))


def test_reference_gains():
    g = np.random.default_rng(4)
    mix = g.uniform(0, 1, (2, 8, 5))
    stem = mix[None] * g.uniform(0, 1, (3, 2, 8, 5))
    mix[0, 4:, 1] = 0.0                                # silent in the band: 0
    stem[:, 0, 4:, 1] = 0.0
    stem[1, 1, :, 2] = 2.0 * mix[1, :, 2]              # louder than the mixture: 1
    ref = FB.ref_gains(stem, mix, 4)
    assert ref.shape == (3, 2, 5) and (ref[:, 0, 1] == 0.0).all() and ref[1, 1, 2] == 1.0
    want = np.sqrt((stem[2, 1, 4:, 3] ** 2).sum() / (mix[1, 4:, 3] ** 2).sum())
    assert abs(ref[2, 1, 3] - want) <= 1e-12 and 0.0 < want < 1.0


def test_reference_full_band_stems_beat_band_limited_ones_by_2_db():
    """Two harmonic sources at 44 100 Hz (ratio 4/1 to the model's 11 025 Hz), 2 s, oracle ratio masks at 1022 / 256 from
    stftref: SDR against the true 44.1 kHz sources, full-band stems against the band-limited ones."""
    rate, up, down, n_fft, hop = 44100, 4, 1, 1022, 256
    src = FB.two_sources(rate, 2.0)
    mix = src.sum(0)
    lo = np.stack([R.ref_outputs(x, down, up, np.arange(R.out_length(x.size, down, up)))[0] for x in (mix, src[0], src[1])])
    re, im, _, _ = stftref.stft(lo.astype(np.float32), n_fft, hop, True)
    mag = np.hypot(re, im)
    masks = mag[1:] / (mag[1:].sum(0) + 1e-12)
    stem_mag = (masks * mag[0]).astype(np.float32)
    phase = np.arctan2(im[0], re[0]).astype(np.float32)
    F = mag.shape[2]
    Lm = hop * (F - 1)
    stems = stftref.istft(stem_mag, np.broadcast_to(phase, stem_mag.shape).copy(), n_fft, hop, Lm)[0]
    gains = FB.ref_gains(stem_mag[:, None], mag[:1].astype(np.float32), 256)
    ref = FB.ref_extend(stems[:, None], lo[:1], mix[None], gains, up, down, hop)
    Lout = ref["out"].shape[2]
    assert Lout == 4 * Lm
    for n in range(2):
        band = FB.sdr(src[n, :Lout], ref["s"][n, 0])
        full = FB.sdr(src[n, :Lout], ref["out"][n, 0])
        print(f"source {n}: band-limited {band:.2f} dB, full band {full:.2f} dB, gain {full - band:+.2f} dB")
        assert full - band > 2.0
