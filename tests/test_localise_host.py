"""not-gpu: the host side of localisation (avsep_amd/localise.py) and the NumPy restatement of the overlay that the GPU
tests compare the kernel with (tests/localise_ref.py)."""
import numpy as np
import pytest
import torch

import avsep_amd  # noqa: F401  (registers the alias)
from avsep_amd import localise as L
from avsep_amd.separate import plan_windows

import localise_ref as R


# ---------------------------------------------------------------------------------------------------------------------
# window_of_frames
# ---------------------------------------------------------------------------------------------------------------------
def test_window_of_frames_one_window_is_the_same_audio_for_every_frame():
    times = np.arange(180) / 30.0
    w = L.window_of_frames(times, plan_windows(256, 128), 11025, 256)
    assert w.dtype == torch.int32 and w.shape == (180,) and w.tolist() == [0] * 180
    assert L.window_of_frames([0.0, 5.9], plan_windows(100, 128), 11025, 256).tolist() == [0, 0]      # shorter than a tile


def test_window_of_frames_nearest_centre_ties_and_clamping():
    rate, hop = 11025, 256
    starts = plan_windows(700, 128)                     # [0, 128, 256, 384, 444]: right-aligned last window
    assert starts == [0, 128, 256, 384, 444]
    centres = [s + 128 for s in starts]                 # 128, 256, 384, 512, 572

    def at(col):
        return col * hop / rate
    # exactly on a centre; one column either side of the midpoint 192 between centres 128 and 256; the tie itself
    assert L.window_of_frames([at(c) for c in centres], starts, rate, hop).tolist() == [0, 1, 2, 3, 4]
    assert L.window_of_frames([at(191), at(192), at(193)], starts, rate, hop).tolist() == [0, 0, 1]
    # the uneven last gap: centres 512 and 572, midpoint 542
    assert L.window_of_frames([at(541), at(542), at(543)], starts, rate, hop).tolist() == [3, 3, 4]
    # before the start and past the end clamp to the first / last column
    assert L.window_of_frames([-3.0, 0.0, at(699), 1e4], starts, rate, hop).tolist() == [0, 0, 4, 4]
    # the column of a time is the NEAREST one: columns are centred on j * hop
    assert L.window_of_frames([at(192.4), at(192.6)], starts, rate, hop).tolist() == [0, 1]
    # brute force over every column
    cols = np.arange(700)
    got = L.window_of_frames(cols * hop / rate, starts, rate, hop).numpy()
    want = [min(range(5), key=lambda k: (abs(centres[k] - c), k)) for c in cols]
    assert got.tolist() == want
    with pytest.raises(ValueError):
        L.window_of_frames([0.0], [128, 0], rate, hop)
    with pytest.raises(ValueError):
        L.window_of_frames([float("nan")], starts, rate, hop)


# ---------------------------------------------------------------------------------------------------------------------
# colour table
# ---------------------------------------------------------------------------------------------------------------------
def test_jet_table_entries_and_segments():
    t = L.jet_table()
    assert t.dtype == np.uint8 and t.shape == (256, 3)
    assert tuple(t[0]) == (0, 0, 128) and tuple(t[96]) == (0, 255, 255)
    assert tuple(t[128]) == (128, 255, 128) and tuple(t[255]) == (131, 0, 0)
    assert np.array_equal(t, R.jet_ref())
    for ch, k in enumerate((3, 2, 1)):                   # each channel: 0, rising ramp, plateau at 255, falling ramp, 0
        v = t[:, ch].astype(int)
        peak = 64 * k
        lo, hi = max(peak - 96, 0), min(peak + 96, 256)
        assert (np.diff(v[lo:peak + 1]) >= 0).all() and (np.diff(v[peak:hi]) <= 0).all()
        assert (v[:lo] == 0).all() and (v[hi + 1:] == 0).all() and v[max(peak - 32, 0):min(peak + 33, 256)].min() == 255


# ---------------------------------------------------------------------------------------------------------------------
# the restatement of the overlay
# ---------------------------------------------------------------------------------------------------------------------
def test_integer_resize_fixed_case_identity_and_distance_to_float_bilinear():
    q = np.array([[0, 255], [100, 200]], dtype=np.uint8)
    assert R.resize_levels(q, 4, 4).tolist() == [[0, 64, 191, 255], [25, 79, 187, 241], [75, 110, 179, 214], [100, 125, 175, 200]]
    rng = np.random.default_rng(0)
    q = rng.integers(0, 256, size=(7, 9), dtype=np.uint8)
    assert np.array_equal(R.resize_levels(q, 7, 9), q)
    big = R.resize_levels(q, 100, 60)
    ref = torch.nn.functional.interpolate(torch.from_numpy(q.astype(np.float64))[None, None], size=(100, 60), mode="bilinear",
                                          align_corners=False)[0, 0].numpy()
    assert big.shape == (100, 60) and np.abs(big.astype(np.float64) - ref).max() <= 0.55


def test_levels_frame_pixels_and_blend():
    m = np.array([[0.25, 0.5], [0.75, 0.3]], dtype=np.float32)
    assert R.levels(m).tolist() == [[0, 127], [255, 25]]
    assert R.levels(np.full((3, 3), 0.5, dtype=np.float32)).tolist() == [[0] * 3] * 3          # the reference gives NaN here
    # every 8-bit value survives normalisation (dataset.py's float32 arithmetic) and the rounded de-normalisation
    img = np.repeat(np.arange(256, dtype=np.uint8)[:, None, None], 3, axis=2)                   # [256,1,3]
    assert np.array_equal(R.frame_pixels(R.normalise(img)), img)
    assert R.frame_pixels(np.full((3, 1, 1), 9.0, np.float32)).tolist() == [[[255, 255, 255]]]  # clamped, not wrapped
    assert R.frame_pixels(np.full((3, 1, 1), -9.0, np.float32)).tolist() == [[[0, 0, 0]]]
    frame = R.normalise(np.array([[[10, 200, 30]]], dtype=np.uint8))
    table = L.jet_table()
    one = np.zeros((1, 1), dtype=np.float32)
    assert R.overlay(one, frame, table, 0).tolist() == [[[10, 200, 30]]]
    assert R.overlay(one, frame, table, 256).tolist() == [[[0, 0, 128]]]
    assert R.overlay(one, frame, table, 102).tolist() == [[[(0 * 102 + 10 * 154 + 128) >> 8, (200 * 154 + 128) >> 8,
                                                             (128 * 102 + 30 * 154 + 128) >> 8]]]


# ---------------------------------------------------------------------------------------------------------------------
# command line and argument errors that need no GPU
# ---------------------------------------------------------------------------------------------------------------------
def test_cli_arguments():
    a = L.parse_args(["--wav", "mix.wav", "--frames", "a.npy", "b.npy", "--fps", "8", "--id", "run1", "--out", "o"])
    assert (a.wav, a.frames, a.fps, a.frame_offset, a.id, a.out) == ("mix.wav", ["a.npy", "b.npy"], 8.0, 0.0, "run1", "o")
    assert (a.alpha, a.window_stride, a.window_batch, a.png, a.latest) == (0.4, 128, 16, False, False)
    assert (a.audRate, a.stft_frame, a.stft_hop, a.num_mix) == (11025, 1022, 256, 2)           # the reference's flag set
    d = L.parse_args(["--wav", "m.wav", "--frames", "duet.npy", "--fps", "30", "--frame_offset", "0.5", "--png"])
    assert d.frames == ["duet.npy"] and d.num_mix == 2 and d.frame_offset == 0.5 and d.png
    t = L.parse_args(["--wav", "m.wav", "--frames", "a.npy", "b.npy", "c.npy", "--fps", "8", "--num_mix", "3"])
    assert len(t.frames) == 3
    for bad in (["--frames", "a.npy", "--fps", "8"],                                            # --wav is required
                ["--wav", "m.wav", "--frames", "a.npy"],                                        # --fps is required
                ["--wav", "m.wav", "--frames", "a.npy", "b.npy", "c.npy", "--fps", "8"],         # three files, two sources
                ["--wav", "m.wav", "--frames", "a.npy", "--fps", "8", "--num_mix", "3"],         # a duet has two sources
                ["--wav", "m.wav", "--frames", "a.npy", "b.npy", "--fps", "0"],
                ["--wav", "m.wav", "--frames", "a.npy", "b.npy", "--fps", "8", "--alpha", "1.5"],
                ["--wav", "m.wav", "--frames", "a.npy", "b.npy", "--fps", "8", "--window_stride", "300"],
                ["--wav", "m.wav", "--frames", "a.npy", "b.npy", "--fps", "8", "--num_mix", "4"]):
        with pytest.raises(SystemExit):
            L.parse_args(bad)


def test_localise_refuses_cpu_tensors():
    import argparse
    args = argparse.Namespace(num_mix=2, fusion_type="hidsep", not_pool_vis=False, stft_frame=1022, stft_hop=256, audRate=11025)
    with pytest.raises(avsep_amd.lib.AvsepError):
        L.localise((None, None), torch.zeros(4096), [torch.zeros(1, 3, 8, 8)] * 2, [0.0], args)


def test_entry_points_refuse_what_does_not_fit_before_launching():
    """include/avsep.h: an HW whose maps do not fit in LDS, more than three sources, a null visual pointer, an overlay whose
    map and resize tables exceed 64 KiB and an alpha outside [0, 256] are argument errors (-1), returned without a launch."""
    import ctypes as C
    lib = avsep_amd.lib.load()
    buf = (C.c_float * 4)()
    p = C.addressof(buf)
    three = (C.c_void_p * 3)(p, p, p)
    hole = (C.c_void_p * 3)(p, None, p)
    maps = lib.avsep_localise_maps
    assert maps(p, p, three, 1, 1, 2, 8, 4, 100000, 1, p, p, p, None) == -1
    assert maps(p, p, three, 1, 1, 4, 8, 4, 16, 1, p, p, p, None) == -1
    assert maps(p, p, three, 1, 1, 2, 8, 4, 16, 2, p, p, p, None) == -1
    assert maps(p, p, hole, 1, 1, 2, 8, 4, 16, 1, p, p, p, None) == -1
    assert maps(p, p, three, 1, 1, 2, 1, 4, 16, 1, p, p, p, None) == -1                  # fewer channels than sources
    over = lib.avsep_heatmap_overlay
    assert over(p, three, p, 1, 2, 300, 300, 8, 8, 102, p, None) == -1
    assert over(p, three, p, 1, 2, 4, 4, 8, 8, 257, p, None) == -1
    assert over(p, three, p, 1, 2, 4, 4, 8, 70000, 102, p, None) == -1
    assert over(p, hole, p, 1, 2, 4, 4, 8, 8, 102, p, None) == -1
