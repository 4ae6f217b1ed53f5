"""not-gpu: the host side of keeping a recording's channels (--channels of separate.py, write_wav_pcm_channels, and the
argument checks of resample.split_pcm / join_pcm, which refuse before anything touches a GPU)."""
import numpy as np
import pytest
import torch

import avsep_amd
from avsep_amd import resample as RS
from avsep_amd import separate as S
from avsep_amd.lib import AvsepError


def test_cli_channels_flag():
    a = S.parse_args(["--wav", "mix.wav", "--frames", "a.npy", "b.npy"])
    assert a.channels == "mix"
    b = S.parse_args(["--wav", "mix.wav", "--audio_only", "--channels", "keep"])
    assert b.channels == "keep" and b.out_rate == "file"
    with pytest.raises(SystemExit):
        S.parse_args(["--wav", "mix.wav", "--audio_only", "--channels", "stereo"])


def test_wav_pcm_channels_round_trip(tmp_path):
    rng = np.random.default_rng(0)
    pcm = rng.integers(-32768, 32768, size=(1001, 3)).astype(np.int16)
    pcm[0] = (-32768, 32767, 0)
    path = str(tmp_path / "three.wav")
    S.write_wav_pcm_channels(path, pcm, 48000)
    back, rate = S.read_wav_pcm(path)
    assert rate == 48000 == S.wav_rate(path) and back.dtype == np.int16 and back.shape == (1001, 3)
    assert np.array_equal(back, pcm)
    # a transposed view is written in frame order too
    S.write_wav_pcm_channels(str(tmp_path / "view.wav"), np.ascontiguousarray(pcm.T).T, 48000)
    assert open(str(tmp_path / "view.wav"), "rb").read() == open(path, "rb").read()
    # one channel: the file write_wav_pcm writes
    S.write_wav_pcm_channels(str(tmp_path / "one.wav"), pcm[:, :1], 11025)
    S.write_wav_pcm(str(tmp_path / "mono.wav"), np.ascontiguousarray(pcm[:, 0]), 11025)
    assert open(str(tmp_path / "one.wav"), "rb").read() == open(str(tmp_path / "mono.wav"), "rb").read()
    with pytest.raises(AvsepError):
        S.write_wav_pcm_channels(str(tmp_path / "bad.wav"), pcm.astype(np.float32) / 32768.0, 48000)      # int16 only
    with pytest.raises(AvsepError):
        S.write_wav_pcm_channels(str(tmp_path / "bad.wav"), pcm[:, 0], 48000)                             # frames are [L,C]


def _no_gpu_call(monkeypatch):
    """Any kernel call or table upload from here on fails the test: the refusals below come from the argument checks."""
    def boom(*a, **k):
        raise AssertionError("reached the GPU path")
    monkeypatch.setattr(avsep_amd.lib, "call", boom)
    monkeypatch.setattr(avsep_amd.kernels, "call", boom)
    monkeypatch.setattr(avsep_amd.lib, "require_gpu", boom)
    monkeypatch.setattr(RS, "filter_table", boom)


def test_split_pcm_refusals(monkeypatch):
    _no_gpu_call(monkeypatch)
    assert RS.MAX_KEPT_CHANNELS == 8
    with pytest.raises(AvsepError) as e:
        RS.split_pcm(torch.zeros(100, 9, dtype=torch.int16), 48000, 11025)
    assert "8" in str(e.value) and "9" in str(e.value)
    with pytest.raises(AvsepError):
        RS.split_pcm(torch.zeros(100, 0, dtype=torch.int16), 48000, 11025)
    with pytest.raises(AvsepError) as e:
        RS.split_pcm(torch.zeros(100, 2, dtype=torch.int16), 11024, 11025)
    assert "11024" in str(e.value) and str(RS.MAX_RATIO) in str(e.value)
    with pytest.raises(AvsepError):
        RS.split_pcm(torch.zeros(100, 2), 48000, 11025)                                  # PCM means int16
    with pytest.raises(AvsepError):
        RS.split_pcm(torch.zeros(100, dtype=torch.int16), 48000, 11025)                  # frames are [L,C]


def test_join_pcm_refusals(monkeypatch):
    _no_gpu_call(monkeypatch)
    with pytest.raises(AvsepError) as e:
        RS.join_pcm(torch.zeros(9, 100), 11025, 48000)
    assert "8" in str(e.value) and "9" in str(e.value)
    with pytest.raises(AvsepError) as e:
        RS.join_pcm(torch.zeros(2, 100), 11025, 11024)
    assert "11024" in str(e.value) and str(RS.MAX_RATIO) in str(e.value)
    with pytest.raises(AvsepError):
        RS.join_pcm(torch.zeros(2, 100, dtype=torch.float64), 11025, 48000)
    with pytest.raises(AvsepError):
        RS.join_pcm(torch.zeros(2, 100, dtype=torch.int16), 11025, 48000)
    with pytest.raises(AvsepError):
        RS.join_pcm(torch.zeros(100), 11025, 48000)                                      # rows are [C,L]


def test_cpu_tensors_are_refused_by_split_and_join():
    """Valid arguments on the CPU: no fallback of any kind, equal rates included."""
    with pytest.raises(AvsepError):
        RS.split_pcm(torch.zeros(100, 2, dtype=torch.int16), 48000, 11025)
    with pytest.raises(AvsepError):
        RS.join_pcm(torch.zeros(2, 100), 11025, 11025)


def test_new_entry_points_refuse_bad_arguments_before_launching():
    """include/avsep.h: C outside [1, 8], a ratio term outside [1, 1280], L < 1, Lout >= 2^31 and null pointers are argument
    errors (-1) of avsep_resample_split / _join; C = 0 and null pointers of avsep_mask_stitch."""
    import ctypes as C
    lib = avsep_amd.lib.load()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    S16 = 1                                                                              # AVSEP_SAMPLE_S16
    for f in (lib.avsep_resample_split, lib.avsep_resample_join):
        la = (lambda L, Cc: (L, Cc)) if f is lib.avsep_resample_split else (lambda L, Cc: (Cc, L))
        assert f(p, p, *la(16, 0), 1, 4, S16, p, None) == -1
        assert f(p, p, *la(16, 9), 1, 4, S16, p, None) == -1
        assert f(p, p, *la(0, 2), 1, 4, S16, p, None) == -1
        assert f(p, p, *la(16, 2), 0, 4, S16, p, None) == -1
        assert f(p, p, *la(16, 2), 1281, 1, S16, p, None) == -1
        assert f(p, p, *la(16, 2), 1, 1281, S16, p, None) == -1
        assert f(p, p, *la(2 ** 31 - 1, 2), 4, 1, S16, p, None) == -1
        assert f(None, p, *la(16, 2), 1, 4, S16, p, None) == -1
        assert f(p, None, *la(16, 2), 1, 4, S16, p, None) == -1
        assert f(p, p, *la(16, 2), 1, 4, S16, None, None) == -1
    g = lib.avsep_mask_stitch
    assert g(p, p, p, p, 1, 2, 4, 4, 0, 4, 4, 0, 0.5, p, None, None) == -1              # C = 0
    assert g(p, p, p, p, 1, 2, 4, 4, 65536, 4, 4, 0, 0.5, p, None, None) == -1
    assert g(p, p, p, None, 1, 2, 4, 4, 2, 4, 4, 0, 0.5, p, None, None) == -1
    assert g(p, p, p, p, 1, 2, 4, 4, 2, 4, 4, 0, 0.5, None, None, None) == -1
