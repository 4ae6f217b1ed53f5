"""not-gpu: the host layer of frames as shot (avsep_amd/frames.py) and the NumPy restatement the GPU tests compare with
(tests/frames_ref.py).  The restatement is held against dataset.VideoTransform itself, which runs Pillow: bit for bit, in the
validation form, with the zero-filled crop of very wide frames, and in the training form with the crop and flip that
VideoTransform drew (learnt by replaying the seed).  frames.resize_tables is held against the restatement's tables."""
import random

import numpy as np
import pytest
import torch

import avsep_amd as P
from avsep_amd import dataset as D
from avsep_amd import frames as F

import frames_ref as R

from PIL import Image

S = 24
SHAPES = [(36, 64), (64, 36), (24, 24), (17, 23), (25, 31)]          # (H, W): wide, tall, no resize, upscale, nearly square
WIDE = [(20, 70), (70, 20), (9, 40)]                                  # under max_size = 48 the short side ends below S


def stack(H, W, T=2, seed=0):
    """uint8 [T,H,W,3]: noise, with a block of saturated two-level pixels (bicubic overshoot past 0 and 255)."""
    g = np.random.default_rng(1000 * H + W + seed)
    a = g.integers(0, 256, (T, H, W, 3), dtype=np.uint8)
    a[:, : H // 2, : W // 2] = (a[:, : H // 2, : W // 2] > 127) * 255
    return a


def video_transform(frames, size, train, max_size=448):
    out = D.VideoTransform(size, train, max_size)([Image.fromarray(f) for f in frames])
    return out.permute(1, 0, 2, 3).contiguous().numpy()                 # [T,3,S,S]


@pytest.mark.parametrize("H,W", SHAPES)
def test_restatement_equals_video_transform_validation(H, W):
    fr = stack(H, W)
    got = R.prepare(fr, S)
    assert got["out"].dtype == np.float32 and got["out"].shape == (2, 3, S, S)
    assert np.array_equal(got["out"], video_transform(fr, S, False))
    if (H, W) == (24, 24):
        assert np.array_equal(got["cropped"], fr)                      # no resize, no crop: the bytes themselves


def test_restatement_equals_video_transform_360p_at_224():
    fr = stack(360, 640, T=1)
    got = R.prepare(fr, 224)
    assert got["size"] == (398, 224) and got["crop"] == (0, 87)
    assert np.array_equal(got["out"], video_transform(fr, 224, False))


@pytest.mark.parametrize("H,W", WIDE)
def test_restatement_zero_fills_the_crop_of_very_wide_frames(H, W):
    fr = stack(H, W)
    got = R.prepare(fr, S, max_size=48)
    w, h = got["size"]
    assert min(w, h) < S and max(w, h) == 48 and min(got["crop"]) < 0
    assert (got["cropped"] == 0).all(axis=(0, 3)).any()                # rows or columns outside the resized image
    assert np.array_equal(got["out"], video_transform(fr, S, False, 48))


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("H,W", SHAPES)
def test_restatement_equals_video_transform_training(H, W, seed):
    """VideoTransform draws randint(0, h - S), randint(0, w - S) and random() < 0.5, in this order, unless the resized frame is
    S x S already: the same draws after the same seed tell the crop and the flip it took."""
    fr = stack(H, W, seed=seed)
    random.seed(seed)
    want = video_transform(fr, S, True)
    w, h = D._resize_size(W, H, int(S * 1.1), 448)
    random.seed(seed)
    crop = (0, 0) if (w, h) == (S, S) else (random.randint(0, h - S), random.randint(0, w - S))
    flip = random.random() < 0.5
    got = R.prepare(fr, S, train=True, crop=crop, flip=flip)
    assert got["size"] == (w, h)
    assert np.array_equal(got["out"], want)


def _pairs():
    """The (n_in, n_out) of every axis the cases above resize, validation and training form, of the GPU tests' 270 x 480 case,
    and of a 2160 x 3840 frame at 224 (41 taps)."""
    pairs = {(360, 224), (640, 398), (270, 224), (480, 398), (2160, 224), (3840, 398)}
    for (H, W), ms in [(s, 448) for s in SHAPES] + [(s, 48) for s in WIDE]:
        for size in (S, int(S * 1.1)):
            w, h = D._resize_size(W, H, size, ms)
            pairs |= {(W, w), (H, h)}
    return sorted(pairs)


def test_resize_tables_equal_the_restatement():
    pairs = _pairs()
    assert len(pairs) >= 20 and any(a == b for a, b in pairs) and any(a < b for a, b in pairs) and any(a > 9 * b for a, b in pairs)
    for n_in, n_out in pairs:
        coef, bound = F.resize_tables(n_in, n_out)
        rcoef, rbound = R.tables(n_in, n_out)
        assert coef.dtype == bound.dtype == np.int32 and coef.shape == rcoef.shape and bound.shape == (n_out, 2)
        assert np.array_equal(coef, rcoef) and np.array_equal(bound, rbound), (n_in, n_out)
        assert (bound[:, 0] >= 0).all() and (bound[:, 1] >= 1).all() and (bound.sum(1) <= n_in).all()
        assert (np.diff(bound[:, 0]) >= 0).all() and (np.diff(bound.sum(1)) >= 0).all()      # the kernel's tiles rely on it


def test_a_table_of_scale_one_is_the_identity():
    for n in (1, 2, 5, 24, 224):
        coef, bound = F.resize_tables(n, n)
        assert coef.shape == (n, 5)
        for xx in range(n):
            row = np.zeros(5, dtype=np.int32)
            row[xx - bound[xx, 0]] = 1 << 22
            assert np.array_equal(coef[xx], row), (n, xx)


def test_plan_holds_what_the_restatement_derives():
    for (H, W), ms in [(s, 448) for s in SHAPES] + [(s, 48) for s in WIDE] + [((360, 640), 448), ((2160, 3840), 448)]:
        size = 224 if H >= 360 else S
        p = F.plan(H, W, size, max_size=ms)
        w, h = D._resize_size(W, H, size, ms)
        assert p.size == (w, h) and p.crop == R.centre_crop(h, w, size) and p.flip is False and p.img_size == size
        hcoef, hbound, vcoef, vbound, lut = p.tables
        assert tuple(hcoef.shape) == (w, hcoef.shape[1]) and tuple(vbound.shape) == (h, 2) and hcoef.shape[1] <= F.MAX_KSIZE
        assert lut.dtype == torch.float32 and np.array_equal(lut.numpy(), R.norm_table())
    assert F.plan(2160, 3840, 224).tables[2].shape[1] == 41            # the cap admits 2160-line frames
    assert F.plan(37, 61, S).crop == (0, 8) and F.plan(61, 37, S).crop == (8, 0)      # (39 - 24) / 2 = 7.5 rounds to even
    p = F.plan(36, 64, S, train=True, crop=(2, 5), flip=True)
    assert p.size == D._resize_size(64, 36, 26, 448) and p.crop == (2, 5) and p.flip is True
    pt = F.plan(36, 64, S, train=True)
    assert pt.crop == R.centre_crop(pt.size[1], pt.size[0], S)


def test_plan_refusals():
    E = P.lib.AvsepError
    for bad in [dict(H=0, W=10), dict(H=10, W=4097), dict(H=10.0, W=10), dict(H=True, W=10)]:
        with pytest.raises(E):
            F.plan(bad["H"], bad["W"], S)
    for size in (7, 1025, 24.0):
        with pytest.raises(E):
            F.plan(36, 64, size)
    with pytest.raises(E, match="taps"):
        F.plan(4096, 4096, 8)                                          # a downscale of 512
    with pytest.raises(E, match="taps"):
        F.plan(21 * 24, 21 * 24, S)                                    # just past 20
    F.plan(20 * 24, 20 * 24, S)
    with pytest.raises(E):
        F.plan(36, 64, S, crop=(0, 0))                                 # the validation form crops the centre
    for crop in [(0,), (0.0, 1), (0, 5000), "ab"]:
        with pytest.raises(E):
            F.plan(36, 64, S, train=True, crop=crop)
    with pytest.raises(E):
        F.plan(36, 64, S, train=1)
    with pytest.raises(E):
        F.plan(36, 64, S, max_size=0)
    with pytest.raises(E):
        F.resize_tables(0, 4)


def test_prepare_refuses_what_is_not_a_stack_of_bytes():
    E = P.lib.AvsepError
    p = F.plan(36, 64, S)
    ok = torch.zeros(2, 36, 64, 3, dtype=torch.uint8)
    for bad in [ok.float(), ok[0], ok[:0], torch.zeros(2, 36, 64, 4, dtype=torch.uint8), ok.permute(0, 2, 1, 3), ok.numpy()]:
        with pytest.raises(E):
            F.prepare(bad, p)
    with pytest.raises(E, match="plan"):
        F.prepare(torch.zeros(2, 64, 36, 3, dtype=torch.uint8), p)
    with pytest.raises(E, match="no CPU fallback"):
        F.prepare(ok, p)                                               # on the host: there is no fallback


def test_load_stack_reads_npy_files_and_folders(tmp_path):
    fr = stack(17, 23, T=3)
    np.save(str(tmp_path / "u8.npy"), fr)
    np.save(str(tmp_path / "one.npy"), fr[0])
    got = F.load_stack(str(tmp_path / "u8.npy"))
    assert got.dtype == torch.uint8 and np.array_equal(got.numpy(), fr) and got.is_contiguous()
    assert np.array_equal(F.load_stack(str(tmp_path / "one.npy")).numpy(), fr[:1])
    fl = np.random.default_rng(0).standard_normal((3, 3, 8, 8)).astype(np.float32)
    np.save(str(tmp_path / "f32.npy"), fl)
    back = F.load_stack(str(tmp_path / "f32.npy"))
    assert back.dtype == torch.float32 and np.array_equal(back.numpy(), fl)             # prepared frames come back as they are
    for name, bad in (("chw.npy", np.zeros((3, 3, 8, 8), np.uint8)), ("flat.npy", np.zeros((8, 8), np.uint8)),
                      ("rgba.npy", np.zeros((2, 8, 8, 4), np.uint8)), ("none.npy", np.zeros((0, 8, 8, 3), np.uint8))):
        np.save(str(tmp_path / name), bad)
        with pytest.raises(SystemExit, match=str(bad.shape).replace("(", r"\(").replace(")", r"\)")):
            F.load_stack(str(tmp_path / name))
    folder = tmp_path / "clip"
    folder.mkdir()
    for t in (2, 0, 1):                                                # written out of order, read in name order
        Image.fromarray(fr[t]).save(str(folder / f"{t:06d}.png"))
    (folder / "notes.txt").write_text("not a frame")
    got = F.load_stack(str(folder))
    assert got.dtype == torch.uint8 and np.array_equal(got.numpy(), fr)
    Image.fromarray(fr[0, :, :, 0]).save(str(folder / "000003.PNG"))    # a grey file becomes RGB, as dataset._load_frames reads it
    assert np.array_equal(F.load_stack(str(folder))[3].numpy(), np.repeat(fr[0, :, :, :1], 3, 2))
    Image.fromarray(fr[0, :10]).save(str(folder / "000004.png"))
    with pytest.raises(SystemExit, match="unequal"):
        F.load_stack(str(folder))
    empty = tmp_path / "empty"
    empty.mkdir()
    (empty / "readme.txt").write_text("nothing")
    with pytest.raises(SystemExit, match="no .jpg"):
        F.load_stack(str(empty))


def test_load_stack_without_pillow(tmp_path, monkeypatch):
    import sys
    folder = tmp_path / "clip"
    folder.mkdir()
    Image.fromarray(stack(8, 8)[0]).save(str(folder / "0.png"))
    monkeypatch.setitem(sys.modules, "PIL", None)                      # `from PIL import Image` now raises ImportError
    with pytest.raises(SystemExit, match="Pillow"):
        F.load_stack(str(folder))
