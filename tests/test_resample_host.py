"""not-gpu: the host side of sample-rate conversion (avsep_amd/resample.py, the WAV helpers and --out_rate of separate.py)
and the float64 restatement the GPU tests compare the kernel with (tests/resample_ref.py), checked against scipy."""
import wave

import numpy as np
import pytest
import torch

import avsep_amd  # noqa: F401  (registers the alias)
from avsep_amd import resample as RS
from avsep_amd import separate as S
from avsep_amd.lib import AvsepError

import resample_ref as R

RATIOS = [(1, 4), (4, 1), (147, 640), (640, 147), (441, 320)]


@pytest.mark.parametrize("up,down", RATIOS + [(441, 1280), (1280, 441), (1, 2), (3, 7)])
def test_design_filter_is_scipys_default(up, down):
    from scipy.signal import firwin
    m = max(up, down)
    want = up * firwin(20 * m + 1, 1.0 / m, window=("kaiser", 5.0))
    for got in (RS.design_filter(up, down), R.design(up, down)):
        assert got.dtype == np.float64 and got.shape == want.shape
        err = np.abs(got - want).max()
        assert err <= 1e-14, err


@pytest.mark.parametrize("up,down", RATIOS)
def test_restatement_vs_scipy_resample_poly(up, down):
    from scipy.signal import resample_poly
    L = 3001
    x = np.random.default_rng(up * 10000 + down).uniform(-1.0, 1.0, L)
    want = resample_poly(x, up, down)                                    # float64, padtype='constant'
    assert want.shape == (R.out_length(L, up, down),) == (RS.out_length(L, up, down),)
    got, absref = R.ref_outputs(x, up, down, np.arange(want.size))
    err = np.abs(got - want).max()
    print(f"{up}/{down}: restatement vs scipy {err:.2e}")
    assert err <= 1e-12
    assert (absref >= np.abs(got) - 1e-15).all()


def test_rational_out_length_and_the_limit():
    assert RS.rational(48000, 11025) == (147, 640) and RS.rational(11025, 48000) == (640, 147)
    assert RS.rational(44100, 11025) == (1, 4) and RS.rational(11025, 44100) == (4, 1)
    assert RS.rational(22050, 11025) == (1, 2) and RS.rational(11025, 11025) == (1, 1)
    assert RS.rational(8000, 11025) == (441, 320) and RS.rational(16000, 11025) == (441, 640)
    assert RS.rational(32000, 11025) == (441, 1280) and RS.rational(96000, 11025) == (147, 1280)
    assert RS.rational(88200, 11025) == (1, 8)
    for bad in ((0, 11025), (11025, -1), (44100.5, 11025)):
        with pytest.raises(ValueError):
            RS.rational(*bad)
    assert RS.out_length(3001, 147, 640) == 690 and RS.out_length(4, 1, 4) == 1 and RS.out_length(5, 1, 4) == 2
    assert RS.out_length(1, 640, 147) == 5 and RS.out_length(28_800_000, 147, 640) == 6_615_000
    assert RS.out_length(6_615_000, 640, 147) == 28_800_000
    for rate in (8000, 16000, 22050, 32000, 44100, 48000, 88200, 96000):
        assert max(RS.check_rates(rate, 11025)) <= RS.MAX_RATIO and max(RS.check_rates(11025, rate)) <= RS.MAX_RATIO
    for rate_in, rate_out in ((11024, 11025), (11025, 47999), (192000, 11025)):
        with pytest.raises(AvsepError) as e:
            RS.check_rates(rate_in, rate_out)
        assert str(rate_in) in str(e.value) and str(rate_out) in str(e.value)


def test_cpu_tensors_are_refused():
    with pytest.raises(AvsepError):
        RS.resample(torch.zeros(100), 48000, 11025)
    with pytest.raises(AvsepError):
        RS.resample(torch.zeros(2, 100), 11025, 11025)                   # equal rates too: no CPU path of any kind
    with pytest.raises(AvsepError):
        RS.resample_pcm(torch.zeros(100, 2, dtype=torch.int16), 48000, 11025)
    with pytest.raises(AvsepError):
        avsep_amd.kernels.resample_poly(torch.zeros(1, 100), torch.zeros(81, 1), 1, 4)


def test_entry_point_refuses_bad_arguments_before_launching():
    """include/avsep.h: up or down outside [1, 1280], L < 1, interleaved PCM with B != 1, more channels than the exact sum
    allows and a null pointer are argument errors (-1), returned without a launch."""
    import ctypes as C
    lib = avsep_amd.lib.load()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    f = lib.avsep_resample_poly
    S16, F32 = 1, 4                                                      # AVSEP_SAMPLE_*
    assert f(p, p, 1, 16, 0, 1, 0, F32, F32, p, None) == -1             # up = 0
    assert f(p, p, 1, 16, 1, 1281, 0, F32, F32, p, None) == -1          # down over the limit
    assert f(p, p, 1, 16, 1281, 1, 0, F32, F32, p, None) == -1
    assert f(p, p, 1, 16, 1, -4, 0, F32, F32, p, None) == -1
    assert f(p, p, 1, 0, 1, 4, 0, F32, F32, p, None) == -1              # L = 0
    assert f(p, p, 0, 16, 1, 4, 0, F32, F32, p, None) == -1             # B = 0
    assert f(p, p, 2, 16, 1, 4, 2, S16, F32, p, None) == -1             # PCM input is one recording
    assert f(p, p, 1, 16, 1, 4, 257, S16, F32, p, None) == -1
    assert f(p, p, 1, 16, 1, 4, -1, S16, F32, p, None) == -1
    assert f(p, p, 1, 16, 1, 4, 0, F32, 5, p, None) == -1               # no such output format
    assert f(p, p, 1, 2 ** 31 - 1, 4, 1, 0, F32, F32, p, None) == -1    # Lout >= 2^31
    assert f(None, p, 1, 16, 1, 4, 0, F32, F32, p, None) == -1
    assert f(p, None, 1, 16, 1, 4, 0, F32, F32, p, None) == -1
    assert f(p, p, 1, 16, 1, 4, 0, F32, F32, None, None) == -1


@pytest.mark.parametrize("C", range(1, 9))
def test_read_wav_is_the_once_rounded_mean(tmp_path, C):
    """include/avsep.h's down-mix of 16-bit frames, (float32)(sum / (C * 32768)) with one rounding, is what read_wav's own
    arithmetic (each sample to f32 over 32768, then NumPy's mean over the channels) gives: the kernels' value at the model's
    rate is the array the standard-library reader returns."""
    rng = np.random.default_rng(C)
    pcm = rng.integers(-32768, 32768, size=(20000, C)).astype(np.int16)
    edge = np.array([-32768, 32767, 0, 1], np.int16)
    pcm[:4] = edge[:, None]                                              # every channel at the same extreme
    pcm[4:8, 0] = edge                                                   # one channel at an extreme beside random ones
    path = str(tmp_path / "x.wav")
    S.write_wav_pcm_channels(path, pcm, 11025)
    got, rate = S.read_wav(path)
    want = (pcm.astype(np.int64).sum(1).astype(np.float64) / (C * 32768.0)).astype(np.float32)
    assert rate == 11025 and got.dtype == np.float32 and np.array_equal(got, want)


def test_polyphase_table_layout():
    """filter_table's column t is the phase of the outputs j = t (mod up) of design_filter, rounded once to f32, zero past
    the filter's end: what output j multiplies x[(j*down + half) // up - i] with is table[i, j % up]."""
    for up, down in ((3, 7), (4, 1), (147, 640), (640, 147)):
        h = RS.design_filter(up, down)
        half = (h.size - 1) // 2
        t = RS.filter_table(up, down, "cpu").numpy()
        T = R.taps(up, down)
        assert t.dtype == np.float32 and t.shape == (T, up)
        for j in (0, 1, 2, up - 1, up, 5 * up + 3, 1000003):
            col = h[(j * down + half) % up::up].astype(np.float32)
            assert np.array_equal(t[:col.size, j % up], col) and not t[col.size:, j % up].any()
        assert RS.filter_table(up, down, "cpu") is RS.filter_table(up, down, "cpu")      # cached
    one = RS.filter_table(1, 1, "cpu").numpy()
    assert one.shape == (21, 1) and one[10, 0] == 1.0 and np.count_nonzero(one) == 1


def test_cli_out_rate_flag():
    a = S.parse_args(["--wav", "mix.wav", "--frames", "a.npy", "b.npy"])
    assert a.out_rate == "file"
    b = S.parse_args(["--wav", "mix.wav", "--audio_only", "--out_rate", "model"])
    assert b.out_rate == "model" and b.audRate == 11025
    with pytest.raises(SystemExit):
        S.parse_args(["--wav", "mix.wav", "--audio_only", "--out_rate", "22050"])


def test_wav_pcm_round_trip(tmp_path):
    rng = np.random.default_rng(0)
    mono = rng.integers(-32768, 32768, size=1000).astype(np.int16)
    mono[:2] = (-32768, 32767)
    path = str(tmp_path / "mono.wav")
    S.write_wav_pcm(path, mono, 48000)
    back, rate = S.read_wav_pcm(path)
    assert rate == 48000 == S.wav_rate(path) and back.dtype == np.int16 and back.shape == (1000, 1)
    assert np.array_equal(back[:, 0], mono)
    f, _ = S.read_wav(path)
    assert np.array_equal(f, mono.astype(np.float32) / 32768.0)          # the two readers see the same samples
    # what write_wav rounds to is what write_wav_pcm stores
    S.write_wav(str(tmp_path / "f.wav"), f, 48000)
    assert open(str(tmp_path / "f.wav"), "rb").read() == open(path, "rb").read()
    stereo = rng.integers(-32768, 32768, size=(777, 2)).astype(np.int16)
    with wave.open(str(tmp_path / "stereo.wav"), "wb") as w:
        w.setnchannels(2); w.setsampwidth(2); w.setframerate(44100)
        w.writeframes(stereo.astype("<i2").tobytes())
    back, rate = S.read_wav_pcm(str(tmp_path / "stereo.wav"))
    assert rate == 44100 and back.shape == (777, 2) and np.array_equal(back, stereo)
    f, _ = S.read_wav(str(tmp_path / "stereo.wav"))
    want = (stereo.astype(np.float64).sum(1) / 65536.0).astype(np.float32)
    assert np.array_equal(f, want)                                       # the mono signal the kernel's PCM input mode forms
    with pytest.raises(AvsepError):
        S.write_wav_pcm(str(tmp_path / "bad.wav"), stereo, 44100)        # mono only
    with pytest.raises(AvsepError):
        S.write_wav_pcm(str(tmp_path / "bad.wav"), f, 44100)             # int16 only
    with wave.open(str(tmp_path / "wide.wav"), "wb") as w:
        w.setnchannels(1); w.setsampwidth(3); w.setframerate(11025)
        w.writeframes(b"\0" * 30)
    with pytest.raises(AvsepError):
        S.read_wav_pcm(str(tmp_path / "wide.wav"))
