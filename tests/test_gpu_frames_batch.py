"""gpu: frames of many sizes in one launch (avsep_frames_prepare_batch in csrc/frames.hip, frames.plan_batch / prepare_batch, the
raw-frames path of the training loader) against the NumPy restatement of tests/frames_ref.py, one frame at a time, and against
the classic loader.  Every comparison is torch.equal: the kernel does integer arithmetic and table look-ups, so there is no
tolerance to state.  A 300 x 300 frame is the one whose tiles are 16 rows high (see tests/test_frames_batch_host.py on the
200 x 200 frame the cases also keep)."""
import numpy as np
import pytest
import torch

import avsep_amd as P
from avsep_amd import dataset as D
from avsep_amd import frames as F

import frames_ref as R
import test_frames_host as FH
import test_frames_batch_host as BH

pytestmark = pytest.mark.gpu

S = FH.S
MIXED = FH.SHAPES + [(200, 200), (300, 300)]           # 36 x 64, 64 x 36, 24 x 24, 17 x 23, 25 x 31, then the two large ones


def _frames(shapes, seed=0):
    return [FH.stack(H, W, 1, seed=seed + r)[0] for r, (H, W) in enumerate(shapes)]


def _buffer(frames, dev):
    """the frames back to back in a buffer exactly as long as they are"""
    return torch.from_numpy(np.concatenate([f.reshape(-1) for f in frames])).to(dev)


def _want(frames, size, train, crops, flips, max_size=448):
    return [torch.from_numpy(R.prepare(f[None], size, train=train, crop=crops[r] if train else None,
                                       flip=bool(train and flips[r]), max_size=max_size)["out"][0])
            for r, f in enumerate(frames)]


def _draws(shapes, size):
    """a different corner and flip per frame, inside the resized frame where it is larger than the crop"""
    crops, flips = [], []
    for r, (H, W) in enumerate(shapes):
        w, h = D._resize_size(W, H, int(size * 1.1), 448)
        crops.append(((r * 5) % (h - size + 1), (r * 3 + 1) % (w - size + 1)))
        flips.append(r % 2 == 0)
    return crops, flips


@pytest.mark.parametrize("train", [False, True])
def test_mixed_sizes_in_one_launch(dev, train):
    shapes = MIXED
    frames = _frames(shapes)
    assert frames[3].size == 1173 and sum(f.size for f in frames[:4]) % 2 == 1      # every later frame starts at an odd byte
    crops, flips = _draws(shapes, S) if train else (None, None)
    want = _want(frames, S, train, crops, flips)
    px = _buffer(frames, dev)
    bp = F.plan_batch(shapes, S, train=train, crops=crops, flips=flips)
    assert len(bp.launches) == 1 and sorted(set(int(v) for v in bp.rows["TR"])) == [16, 32] and bp.launches[0][4] == 16
    out = F.prepare_batch(px, bp)
    assert out.shape == (len(shapes), 3, S, S) and out.dtype == torch.float32
    for r in range(len(shapes)):
        assert torch.equal(out[r].cpu(), want[r]), (shapes[r], train)
    # the loader's layout, [B,3,T,S,S] with B = 3, T = 2, from the issue's six frames, and B = 4 with the 300 x 300 frame
    for B, T, pick in ((3, 2, [0, 1, 2, 3, 4, 5]), (4, 2, [6, 0, 1, 2, 3, 4, 5, 6])):
        sub = [frames[r] for r in pick]
        bp = F.plan_batch([shapes[r] for r in pick], S, train=train, crops=[crops[r] for r in pick] if train else None,
                          flips=[flips[r] for r in pick] if train else None, layout=(B, T))
        out = F.prepare_batch(_buffer(sub, dev), bp)
        assert out.shape == (B, 3, T, S, S)
        for k, r in enumerate(pick):
            assert torch.equal(out[k // T, :, k % T].cpu(), want[r]), (B, T, k)


def test_first_and_last_frame_of_an_exact_buffer(dev):
    """17 x 23 frames of 1173 bytes in a buffer of exactly 3 x 1173 bytes that itself starts off a 16-byte boundary: the first
    frame's first quad and the last frame's last quad hang over the ends of what the kernel may read."""
    frames = _frames([(17, 23)] * 3, seed=4)
    want = _want(frames, S, False, None, None)
    bp = F.plan_batch([(17, 23)] * 3, S)
    for off in (0, 1, 7):
        whole = torch.full((off + 3 * 1173 + 5,), 255, dtype=torch.uint8, device=dev)
        view = whole[off:off + 3 * 1173]
        view.copy_(_buffer(frames, dev))
        assert view.data_ptr() % 16 == off
        out = F.prepare_batch(view, bp)
        for r in range(3):
            assert torch.equal(out[r].cpu(), want[r]), (off, r)


def test_zero_filled_crops_of_very_wide_frames(dev):
    frames = _frames(FH.WIDE)
    want = _want(frames, S, False, None, None, max_size=48)
    out = F.prepare_batch(_buffer(frames, dev), F.plan_batch(FH.WIDE, S, max_size=48))
    for r in range(len(frames)):
        assert torch.equal(out[r].cpu(), want[r]), FH.WIDE[r]


def test_batch_of_equal_frames_equals_the_single_form(dev):
    T = 4
    for (H, W), kw in (((36, 64), {}), ((25, 31), dict(train=True, crop=(1, 2), flip=True)), ((300, 300), {})):
        st = torch.from_numpy(FH.stack(H, W, T)).to(dev)
        single = F.prepare(st, F.plan(H, W, S, **kw))
        bp = F.plan_batch([(H, W)] * T, S, train=kw.get("train", False), crops=[kw["crop"]] * T if kw else None,
                          flips=[True] * T if kw else None)
        assert torch.equal(F.prepare_batch(st.reshape(-1), bp), single), (H, W)


def test_real_sizes_together(dev):
    """360 x 640 and 270 x 480 at 224: seven tiles a side, 9 and 5 / 7 taps, LDS sized by the larger frame."""
    shapes = [(360, 640), (270, 480)]
    frames = _frames(shapes)
    want = _want(frames, 224, False, None, None)
    out = F.prepare_batch(_buffer(frames, dev), F.plan_batch(shapes, 224))
    for r in range(2):
        assert torch.equal(out[r].cpu(), want[r]), shapes[r]


def test_a_wrong_device_table_leaves_memory_alone(dev):
    """Rows that the plan entry would refuse, written into the device table behind its back: offsets past every buffer, sizes
    past the limits, a tile height and an LDS need the launch did not provide.  The frames of the good rows are right, the
    output of a refused row is untouched, and nothing outside the output is written (the guard floats keep their value)."""
    shapes = [(36, 64), (25, 31), (64, 36), (17, 23)]
    frames = _frames(shapes)
    want = _want(frames, S, False, None, None)
    bp = F.plan_batch(shapes, S)
    px = _buffer(frames, dev)
    tables, lut = bp.packed.on(dev)
    _, _, grid_y, lds, _ = bp.launches[0]
    n, guard = len(shapes), 64
    for field, value, untouched in (("out_off", n * 3 * S * S - S * S + 1, True), ("out_off", -8, True), ("hcoef", 1 << 30, True),
                                    ("vbound", -4, True), ("in_bytes", 16384, True), ("mid_rows", 256, True),
                                    ("max_cols", 4096, True), ("pix_off", 1 << 40, False), ("pix_off", -(1 << 40), False),
                                    ("H", 4096, False), ("TR", 1 << 20, False), ("crop_i", 1 << 30, False)):
        rows = bp.rows.copy()
        rows[field][1] = value
        out = torch.full((n * 3 * S * S + guard,), -7.0, device=dev)
        P.kernels.frames_prepare_batch(px, torch.from_numpy(rows.view(np.uint8)).to(dev), tables, lut, S, out, S * S, grid_y, lds)
        got = out.cpu()
        assert bool((got[n * 3 * S * S:] == -7.0).all()), (field, value)
        got = got[:n * 3 * S * S].view(n, 3, S, S)
        for r in (0, 2, 3):
            assert torch.equal(got[r], want[r]), (field, value, r)
        if untouched:
            assert bool((got[1] == -7.0).all()), (field, value)
    torch.cuda.synchronize()


def test_library_refuses_a_wrong_batch_launch(dev):
    lib = P.lib.load()
    bp = F.plan_batch([(36, 64), (25, 31)], S)
    tables, lut = bp.packed.on(dev)
    px = torch.zeros(bp.pixel_bytes, dtype=torch.uint8, device=dev)
    rows = torch.from_numpy(bp.rows.view(np.uint8)).to(dev)
    out = torch.empty(2, 3, S, S, device=dev)
    _, _, grid_y, lds, _ = bp.launches[0]

    def call(**kw):
        a = dict(px=px.data_ptr(), nb=px.numel(), rows=rows.data_ptr(), n=2, tables=tables.data_ptr(), words=tables.numel(), S=S,
                 lut=lut.data_ptr(), out=out.data_ptr(), outf=out.numel(), plane=S * S, gy=grid_y, lds=lds)
        a.update(kw)
        return lib.avsep_frames_prepare_batch(*a.values(), P.lib.stream())

    assert call() == 0
    for kw in (dict(px=None), dict(rows=None), dict(tables=None), dict(lut=None), dict(out=None), dict(n=0), dict(n=65536), dict(S=7),
               dict(S=1025), dict(nb=0), dict(words=0), dict(plane=S * S - 1), dict(outf=3 * S * S - 1), dict(gy=0), dict(gy=S + 1),
               dict(lds=3071), dict(lds=54401)):
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()


@pytest.mark.parametrize("split", ["train", "val"])
def test_loader_end_to_end_equals_the_classic_loader(dev, tmp_path, split):
    lst = BH.make_disk_dataset(tmp_path)
    a = BH.loader_args()
    classic = D.to_device(next(iter(D.make_loader([lst], a, split, batch_size=4, shuffle=False))), dev)
    host = next(iter(D.make_loader([lst], a, split, batch_size=4, shuffle=False, raw_frames=True)))
    assert "frames" not in host and len(set(map(tuple, host["frame_shapes"].reshape(-1, 2).tolist()))) == 3
    raw = D.to_device(host, dev)
    for n in range(2):
        assert raw["frames"][n].shape == (4, 3, 3, 64, 64) and raw["frames"][n].is_contiguous()
        assert torch.equal(raw["frames"][n], classic["frames"][n]), (split, n)
        assert torch.equal(raw["audios"][n], classic["audios"][n])
    assert torch.equal(raw["audio_mix"], classic["audio_mix"]) and raw["id"] == classic["id"]
    assert torch.equal(raw["class"], classic["class"])
