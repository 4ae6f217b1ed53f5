"""not-gpu: host logic of long-form separation (avsep_amd/separate.py): the window plan, the alignment of the
audio-only branch's source order across windows, the command line and the 16-bit WAV reader / writer."""
import itertools

import numpy as np
import pytest
import torch

import avsep_amd                                   # noqa: F401  (registers the alias)
from avsep_amd import separate as S


@pytest.mark.parametrize("stride", [64, 128, 256])
@pytest.mark.parametrize("F", [1, 255, 256, 257, 384, 385, 2584])
def test_plan_windows_covers_every_frame(F, stride):
    starts = S.plan_windows(F, stride)
    assert starts[0] == 0 and all(isinstance(s, int) for s in starts)
    covered = np.zeros(F, dtype=bool)
    for s in starts:
        assert 0 <= s
        covered[s:s + 256] = True
    assert covered.all()
    gaps = np.diff(starts)
    assert (gaps > 0).all() and (gaps <= stride).all()                   # strictly ascending, never further than stride
    if F > 256:
        assert starts[-1] + 256 == F                                      # the last window is right-aligned
        assert all(s + 256 < F for s in starts[:-1])
        regular = starts[:-1]
        assert regular == list(range(0, stride * len(regular), stride))
    else:
        assert starts == [0]


def test_plan_windows_known_tables_and_bad_arguments():
    assert S.plan_windows(384, 128) == [0, 128]
    assert S.plan_windows(385, 128) == [0, 128, 129]
    assert S.plan_windows(600, 256) == [0, 256, 344]
    assert S.plan_windows(300, 64, width=100) == [0, 64, 128, 192, 200]
    for bad in ((0, 128), (300, 0), (300, 257)):
        with pytest.raises(ValueError):
            S.plan_windows(*bad)


def test_align_permutations_two_sources():
    same = [[0.0, 5.0], [5.0, 0.0]]          # channel i of window k is channel i of window k+1
    swap = [[5.0, 0.0], [0.0, 5.0]]          # ... is channel 1-i
    # the swap accumulates: after one swap the NEXT "same" keeps the swapped order, a second swap restores it
    D = torch.tensor([same, swap, same, swap, swap])
    p = S.align_permutations(D)
    assert p.dtype == torch.int32 and p.shape == (6, 2)
    assert p.tolist() == [[0, 1], [0, 1], [1, 0], [1, 0], [0, 1], [1, 0]]
    # a tie keeps the first candidate of itertools.permutations, the identity
    tie = torch.full((1, 2, 2), 3.0)
    assert S.align_permutations(tie).tolist() == [[0, 1], [0, 1]]
    # no boundaries: one window, identity
    assert S.align_permutations(torch.zeros(0, 2, 2)).tolist() == [[0, 1]]


def _D_for(true_perm_prev, true_perm_next, N):
    """D[k] when channel c of a window carries true source true_perm[c]: 0 where the sources agree, 1 elsewhere."""
    return [[0.0 if true_perm_prev[i] == true_perm_next[j] else 1.0 for j in range(N)] for i in range(N)]


def test_align_permutations_three_sources_chain():
    N = 3
    # channel -> true source of four windows; output source n of window 0 is its channel n
    truth = [(0, 1, 2), (2, 0, 1), (1, 2, 0), (1, 0, 2)]
    D = torch.tensor([_D_for(truth[k], truth[k + 1], N) for k in range(3)], dtype=torch.float64)
    p = S.align_permutations(D).tolist()
    assert p[0] == [0, 1, 2]
    for k in range(4):                                   # output n must read, in every window, the channel carrying source n
        assert [truth[k][c] for c in p[k]] == [0, 1, 2], (k, p[k])
    # tie between all six candidates: first of itertools.permutations
    assert S.align_permutations(torch.ones(1, 3, 3)).tolist()[1] == list(next(itertools.permutations(range(3))))
    # a tie between two candidates only: (0,2,1) comes before (1,0,2)... the earlier one in enumeration order wins
    D2 = torch.tensor([[[0.0, 1.0, 0.0], [1.0, 0.5, 0.5], [1.0, 0.5, 0.5]]])
    costs = {c: sum(D2[0, n, c[n]].item() for n in range(3)) for c in itertools.permutations(range(3))}
    first_best = min(costs.values())
    expect = next(c for c in itertools.permutations(range(3)) if costs[c] == first_best)
    assert S.align_permutations(D2).tolist()[1] == list(expect)
    with pytest.raises(ValueError):
        S.align_permutations(torch.zeros(2, 4, 4))
    with pytest.raises(ValueError):
        S.align_permutations(torch.zeros(2, 2, 3))


def test_cli_arguments():
    a = S.parse_args(["--wav", "mix.wav", "--frames", "a.npy", "b.npy", "--id", "Exp5", "--out", "o"])
    assert (a.wav, a.frames, a.id, a.out) == ("mix.wav", ["a.npy", "b.npy"], "Exp5", "o")
    assert (a.window_stride, a.window_batch, a.audio_only, a.latest) == (128, 16, False, False)
    # the reference's flag set rides along with its defaults
    assert (a.audRate, a.stft_frame, a.stft_hop, a.num_mix, a.mask_thres) == (11025, 1022, 256, 2, 0.5)
    b = S.parse_args(["--wav", "m.wav", "--audio_only", "--window_stride", "64", "--arch_sound", "unet7", "--latest"])
    assert b.audio_only and b.frames == [] and b.window_stride == 64 and b.arch_sound == "unet7" and b.latest
    with pytest.raises(SystemExit):
        S.parse_args(["--wav", "m.wav", "--frames", "only_one.npy"])       # two sources need two frame files
    with pytest.raises(SystemExit):
        S.parse_args(["--frames", "a.npy", "b.npy"])                       # --wav is required


def test_wav_round_trip(tmp_path):
    rate = 11025
    t = np.arange(3 * rate) / rate
    x = (0.6 * np.sin(2 * np.pi * 440 * t) + 0.3 * np.sin(2 * np.pi * 1250 * t)).astype(np.float32)
    x[:4] = [1.0, -1.0, 0.0, 2.0]                          # full scale, and a sample that must clip
    path = str(tmp_path / "tone.wav")
    S.write_wav(path, x, rate)
    y, r = S.read_wav(path)
    assert r == rate and y.dtype == np.float32 and y.shape == x.shape
    assert np.abs(y - np.clip(x, -1, 1)).max() <= 1.0 / 32768 + 1e-7     # half a step of rounding; one step where +1.0 clips
    # writing what was read is lossless
    S.write_wav(str(tmp_path / "again.wav"), y, rate)
    z, _ = S.read_wav(str(tmp_path / "again.wav"))
    assert np.array_equal(y, z)
    # stereo is averaged, other sample widths are refused
    import wave
    with wave.open(str(tmp_path / "stereo.wav"), "wb") as w:
        w.setnchannels(2); w.setsampwidth(2); w.setframerate(rate)
        w.writeframes(np.array([[1000, 3000], [-2000, 2000]], dtype="<i2").tobytes())
    s, _ = S.read_wav(str(tmp_path / "stereo.wav"))
    assert np.allclose(s, np.array([2000, 0]) / 32768.0)
    with wave.open(str(tmp_path / "wide.wav"), "wb") as w:
        w.setnchannels(1); w.setsampwidth(3); w.setframerate(rate)
        w.writeframes(b"\x00" * 30)
    with pytest.raises(avsep_amd.lib.AvsepError):
        S.read_wav(str(tmp_path / "wide.wav"))


def test_separate_long_refuses_cpu_tensors():
    import argparse
    args = argparse.Namespace(stft_frame=1022, stft_hop=256, num_mix=2, fusion_type="hidsep")
    with pytest.raises(avsep_amd.lib.AvsepError):
        S.separate_long((None, None), torch.zeros(4096), [], args)         # no CPU fallback
