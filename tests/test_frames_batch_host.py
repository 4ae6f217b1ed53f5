"""not-gpu: the host side of the training loader's GPU frames.  MUSICMixDataset(raw_frames=True) makes the classic dataset's
``random`` calls in the classic order and records what they drew; frames.plan_batch builds, per frame, what frames.plan builds
for that frame alone; avsep_frames_batch_plan (host only) refuses every range outside its buffer and sizes the launch;
dataset.collate packs a raw batch and leaves a classic one as it was.  The CPU restatement (tests/frames_ref.py) stands for
the kernel here: tests/test_gpu_frames_batch.py holds the kernel against it.

One figure differs from the issue that asked for these tests.  It expected a 200 x 200 frame at S = 24 to take tiles of 16
rows; the library's sizing rule (fp_span, capped at the frame's height) gives it 32, since all of its 200 rows fit the 256-row
tile.  The 200 x 200 case stays as stated wherever it is listed, and a 300 x 300 frame, whose 32-row tile would reach 300 > 256
input rows, is added as the frame that does take 16."""
import ctypes
import random

import numpy as np
import pytest
import torch

import avsep_amd as P
from avsep_amd import dataset as D
from avsep_amd import frames as F

import frames_ref as R
import test_dataset as TD

E = P.lib.AvsepError
SIZES = [(160, 120), (120, 160), (96, 96)]             # (width, height) of the videos, by class index % 3


def make_disk_dataset(root, sizes=SIZES, secs=9.0):
    """test_dataset._make_disk_dataset, then the frames of video c rewritten at sizes[c % len(sizes)] -> the list's path."""
    from PIL import Image
    lst = TD._make_disk_dataset(str(root), secs=secs, size=sizes[0])
    rs = np.random.RandomState(5)
    for c, row in enumerate(D.read_list(lst)):
        w, h = sizes[c % len(sizes)]
        if (w, h) == sizes[0]:
            continue
        for i in range(int(row[2]) + 1):
            Image.fromarray(rs.randint(0, 255, (h, w, 3), dtype=np.uint8)).save(f"{row[1]}/{i:06d}.jpg", quality=60)
    return lst


def loader_args(img=64, extra=()):
    return P.ArgParser().parse_train_arguments(
        ["--num_frames", "3", "--stride_frames", "2", "--imgSize", str(img), "--audLen", "16383", "--margin", "1.0",
         "--train_repeat", "2", "--val_repeat", "2", *extra], verbose=False)


@pytest.fixture(scope="module")
def disk(tmp_path_factory):
    return make_disk_dataset(tmp_path_factory.mktemp("raw"))


def _pair(lst, split, a):
    kw = dict(split=split, seed=a.seed)
    return D.MUSICMixDataset(lst, vars(a), **kw), D.MUSICMixDataset(lst, vars(a), raw_frames=True, **kw)


def _clip(item, n):
    """source n of a raw item -> its frames, a list of uint8 arrays [H,W,3]"""
    px, out, at = item["frames_u8"][n].numpy(), [], 0
    for H, W in item["frame_shapes"][n].tolist():
        out.append(px[at:at + H * W * 3].reshape(H, W, 3))
        at += H * W * 3
    assert at == px.size
    return out


def _restated(item, n, S, train):
    """[3,T,S,S]: the restatement of the clip under the item's recorded draws, frame by frame (they may differ in size)"""
    crop, flip = item["frame_crops"][n], item["frame_flips"][n]
    outs = [R.prepare(f[None], S, train=train, crop=crop, flip=flip)["out"][0] for f in _clip(item, n)]
    return np.stack(outs, 1)


@pytest.mark.parametrize("split", ["train", "val"])
def test_raw_items_draw_what_classic_items_draw(disk, split):
    a = loader_args()
    classic, raw = _pair(disk, split, a)
    seen = set()
    for k, i in ((0, 0), (7, 1), (123, 2), (5, 5), (99, 12), (1, 21)):
        random.seed(k)
        c = classic[i]
        sc = random.getstate()
        random.seed(k + 1000)                                          # whatever was drawn before
        r = raw[i]
        assert random.getstate() == sc, (split, i)
        assert "frames" not in r and r["id"] == c["id"] and torch.equal(r["class"], c["class"]) and r["infos"] == c["infos"]
        assert torch.equal(r["audio_mix"], c["audio_mix"]) and all(torch.equal(x, y) for x, y in zip(r["audios"], c["audios"]))
        assert r["imgSize"] == 64 and r["split"] == split
        for n in range(2):
            assert r["frames_u8"][n].dtype == torch.uint8 and r["frames_u8"][n].dim() == 1
            assert r["frame_shapes"][n].dtype == torch.int32 and tuple(r["frame_shapes"][n].shape) == (3, 2)
            assert isinstance(r["frame_flips"][n], bool)
            assert (r["frame_crops"][n] is None) == (split == "val") and (split == "train" or r["frame_flips"][n] is False)
            seen.add(tuple(r["frame_shapes"][n][0].tolist()))
            assert np.array_equal(_restated(r, n, 64, split == "train"), c["frames"][n].numpy()), (split, i, n)
    assert seen == {(120, 160), (160, 120), (96, 96)}                  # all three frame sizes came by


def test_raw_items_with_one_frame_and_without_crop_draws(tmp_path):
    # one_frame: the shift is drawn before the crop, T = 1
    lst = make_disk_dataset(tmp_path / "a")
    a = loader_args()
    a.one_frame = True
    classic, raw = _pair(lst, "train", a)
    for i in (0, 3, 4):
        c = classic[i]
        sc = random.getstate()
        r = raw[i]
        assert random.getstate() == sc and tuple(r["frame_shapes"][0].shape) == (1, 2)
        for n in range(2):
            assert np.array_equal(_restated(r, n, 64, True), c["frames"][n].numpy())
    # square frames at imgSize 8: int(8 * 1.1) == 8, the resized frame is the crop and neither randint is called
    lst = make_disk_dataset(tmp_path / "b", sizes=[(20, 20)], secs=4.0)
    a = loader_args(img=8)
    classic, raw = _pair(lst, "train", a)
    for i in (0, 6):
        c = classic[i]
        sc = random.getstate()
        r = raw[i]
        assert random.getstate() == sc and r["frame_crops"] == [(0, 0), (0, 0)]
        for n in range(2):
            assert np.array_equal(_restated(r, n, 8, True), c["frames"][n].numpy())


def test_a_frame_too_small_for_the_crop_raises_what_it_raised(tmp_path):
    """The long side capped at max_size leaves the short one below the crop: randint(0, negative) in both forms of the item."""
    lst = make_disk_dataset(tmp_path, sizes=[(200, 20)], secs=4.0)
    a = loader_args(img=64)
    classic, raw = _pair(lst, "train", a)
    with pytest.raises(ValueError) as ec:
        classic[0]
    with pytest.raises(ValueError) as er:
        raw[0]
    assert str(ec.value) == str(er.value)


SHAPES = [(36, 64), (64, 36), (24, 24), (17, 23), (25, 31), (200, 200), (36, 64), (300, 300)]


def test_plan_batch_rows_hold_what_plan_holds(monkeypatch):
    F.axis_tables.cache_clear()
    F._packed.cache_clear()
    calls = []
    real = F.resize_tables
    monkeypatch.setattr(F, "resize_tables", lambda a, b: (calls.append((a, b)), real(a, b))[1])
    S = 24
    for train in (False, True):
        crops = [(r % 3, (2 * r) % 3) for r in range(len(SHAPES))] if train else None
        flips = [r % 2 == 1 for r in range(len(SHAPES))] if train else None
        bp = F.plan_batch(SHAPES, S, train=train, crops=crops, flips=flips)
        assert bp.n == len(SHAPES) and bp.out_shape == (len(SHAPES), 3, S, S) and bp.plane == S * S
        packed, at = bp.packed.host.numpy(), 0
        for r, (H, W) in enumerate(SHAPES):
            p = F.plan(H, W, S, train=train, crop=crops[r] if train else None, flip=bool(train and flips[r]))
            row = bp.rows[r]
            assert (row["H"], row["W"], row["w"], row["h"]) == (H, W) + p.size and (row["crop_i"], row["crop_j"]) == p.crop
            assert row["flip"] == int(p.flip) and row["pix_off"] == at and row["out_off"] == r * 3 * S * S
            assert bp.sizes[r] == p.size and bp.crops[r] == p.crop
            hc, hb, vc, vb = (t.numpy() for t in p.tables[:4])
            assert (row["kh"], row["kv"]) == (hc.shape[1], vc.shape[1])
            for off, want in ((row["hcoef"], hc), (row["hbound"], hb), (row["vcoef"], vc), (row["vbound"], vb)):
                assert np.array_equal(packed[off:off + want.size], want.reshape(-1)), (r, train)
            at += H * W * 3
        assert bp.pixel_bytes == at
        same = [bp.rows[0][k] == bp.rows[6][k] for k in ("hcoef", "hbound", "vcoef", "vbound")]
        assert all(same), "two frames of one size share their tables"
    assert len(calls) == len(set(calls)), "resize_tables ran more than once for an axis pair"
    want = set()
    for train in (False, True):
        for H, W in SHAPES:
            w, h = D._resize_size(W, H, int(S * 1.1) if train else S, 448)
            want |= {(W, w), (H, h)}
    assert set(calls) == want
    # the loader's layout: frame r is clip r // T, time r % T of [B,3,T,S,S]
    bp = F.plan_batch(SHAPES, S, layout=(4, 2))
    assert bp.out_shape == (4, 3, 2, S, S) and bp.plane == 2 * S * S
    assert [int(v) for v in bp.rows["out_off"]] == [((r // 2) * 3 * 2 + r % 2) * S * S for r in range(8)]
    F.axis_tables.cache_clear()                                        # nothing counted stays behind
    F._packed.cache_clear()


def test_axis_tables_are_computed_once_and_equal_resize_tables():
    a, b = F.axis_tables(64, 42), F.axis_tables(64, 42)
    assert a is b
    for x, y in zip(a, F.resize_tables(64, 42)):
        assert x.dtype == y.dtype and np.array_equal(x, y)
    assert torch.equal(F.plan(36, 64, 24).tables[0], torch.from_numpy(R.tables(64, 42)[0]))


def test_plan_batch_refuses(monkeypatch):
    ok = [(36, 64), (25, 31)]
    F.plan_batch(ok, 24)
    for kw in (dict(shapes=[]), dict(shapes=[(36,)]), dict(shapes=[(36, 4097)]), dict(shapes=[(0, 5)]), dict(img_size=7),
               dict(img_size=24.0), dict(img_size=1025), dict(train=1), dict(crops=[(0, 0), None]), dict(train=True, crops=[(0, 0)]),
               dict(train=True, crops=[(0, 5000), None]), dict(flips=[True]), dict(flips=[1, 0]), dict(layout=(3, 1)),
               dict(layout=(2,)), dict(max_size=0), dict(shapes=[(21 * 24, 21 * 24)])):
        a = dict(shapes=ok, img_size=24)
        a.update(kw)
        with pytest.raises(E):
            F.plan_batch(a.pop("shapes"), a.pop("img_size"), **a)
    bp = F.plan_batch(ok, 24)
    n = bp.pixel_bytes
    for bad in (torch.zeros(n, dtype=torch.int8), torch.zeros(n - 1, dtype=torch.uint8), torch.zeros(n + 1, dtype=torch.uint8),
                torch.zeros(1, n, dtype=torch.uint8), torch.zeros(2 * n, dtype=torch.uint8)[::2], np.zeros(n, np.uint8)):
        with pytest.raises(E):
            F.prepare_batch(bad, bp)
    with pytest.raises(E):
        F.prepare_batch(torch.zeros(n, dtype=torch.uint8), F.plan(36, 64, 24))
    with pytest.raises(E, match="no CPU fallback"):
        F.prepare_batch(torch.zeros(n, dtype=torch.uint8), bp)         # on the host: there is no fallback


def test_plan_entry_refuses_without_a_gpu():
    S = 24
    bp = F.plan_batch([(36, 64), (25, 31)], S)
    words, px, outf, plane = bp.packed.host.numel(), bp.pixel_bytes, 2 * 3 * S * S, S * S

    def call(n=2, S=S, px=px, words=words, outf=outf, plane=plane, **fields):
        rows = bp.rows.copy()
        for k, v in fields.items():
            rows[k][1] = v
        return P.lib.load().avsep_frames_batch_plan(rows.ctypes.data_as(ctypes.POINTER(P.lib.FramesRow)), n, S, px, words, outf,
                                                    plane, (ctypes.c_int32 * 3)())

    assert call() == 0
    last = bp.rows[1]
    for kw in (dict(px=px - 1), dict(pix_off=int(last["pix_off"]) + 1), dict(pix_off=-1),          # a pixel range past the buffer
               dict(words=words - 1), dict(vbound=int(last["vbound"]) + 1), dict(hcoef=-1), dict(hcoef=words),      # a table range
               dict(outf=outf - 1), dict(out_off=int(last["out_off"]) + 1), dict(out_off=-1), dict(plane=plane - 1),
               dict(plane=plane + 1),                                  # the last frame's third channel leaves the output
               dict(kh=int(last["kh"]) + 2), dict(kv=1), dict(w=3),    # k not what the sizes imply
               dict(S=7), dict(S=1025), dict(W=4097), dict(H=4097), dict(H=0), dict(h=4097), dict(crop_i=4097), dict(crop_j=-4097),
               dict(flip=2), dict(n=0), dict(n=-1)):
        assert call(**kw) == -1, kw
    with pytest.raises(E):
        P.kernels.frames_batch_plan(bp.rows[:0], S, px, words, outf, plane)
    with pytest.raises(E):
        P.kernels.frames_batch_plan(bp.rows.copy(), 7, px, words, outf, plane)
    lib = P.lib.load()
    assert lib.avsep_frames_batch_plan(None, 2, S, px, words, outf, plane, (ctypes.c_int32 * 3)()) == -1
    assert lib.avsep_frames_batch_plan(bp.rows.copy().ctypes.data_as(ctypes.POINTER(P.lib.FramesRow)), 2, S, px, words, outf, plane,
                                       None) == -1


def test_launch_bounds_of_mixed_tile_heights():
    S = 24
    # the issue's pair: all 200 rows of the tall frame fit the 256-row tile, so both take 32-row tiles (see the module docstring)
    bp = F.plan_batch([(200, 200), (36, 64)], S)
    assert [int(v) for v in bp.rows["TR"]] == [32, 32] and bp.launches[0][2:] == (1, bp.launches[0][3], 32)
    assert [int(v) for v in bp.rows["mid_rows"]] == [200, 36]
    # 300 rows do not: scale 12.5, support 25; 32 output rows reach ceil(31 * 12.5 + 50) + 2 = 440 > 256, 16 reach 240
    bp = F.plan_batch([(300, 300), (36, 64), (200, 200)], S)
    assert [int(v) for v in bp.rows["TR"]] == [16, 32, 32] and [int(v) for v in bp.rows["mid_rows"]] == [240, 36, 200]
    a, b, grid_y, lds, tr_min = bp.launches[0]
    assert (a, b, grid_y, tr_min) == (0, 3, 2, 16)
    per_row = [int(r["in_bytes"]) + int(r["mid_rows"]) * 96 + 32 * max(int(r["kh"]), int(r["kv"])) * 4 + 3072 for r in bp.rows]
    assert lds == max(per_row) and per_row[0] == lds and lds <= 54400
    for r in bp.rows:                                                   # one staged row of the widest tile fits, in whole quads
        assert r["in_bytes"] % 16 == 0 and r["in_bytes"] >= (int(r["max_cols"]) * 3 + 30) // 16 * 16 and r["max_cols"] <= r["W"]
    # the single form sizes a frame alone the same way: a batch of one is that launch
    one = F.plan_batch([(300, 300)], S)
    assert int(one.rows["TR"][0]) == 16 and one.launches[0][2:] == (2, lds, 16)


@pytest.mark.parametrize("split", ["train", "val"])
def test_collate_of_raw_and_classic_batches(disk, split):
    a = loader_args()
    classic, raw = _pair(disk, split, a)
    idx = [0, 1, 2, 5]
    items = [classic[i] for i in idx]
    got = D.collate(items)
    # today's collate, restated
    assert set(got) == {"audios", "audio_mix", "frames", "id", "class", "infos"}
    for n in range(2):
        assert torch.equal(got["audios"][n], torch.stack([s["audios"][n] for s in items]))
        assert torch.equal(got["frames"][n], torch.stack([s["frames"][n] for s in items]))
        assert got["infos"][n] == [[s["infos"][n][k] for s in items] for k in range(6)]
    assert torch.equal(got["audio_mix"], torch.stack([s["audio_mix"] for s in items]))
    assert got["id"] == [s["id"] for s in items] and torch.equal(got["class"], torch.stack([s["class"] for s in items]))
    ritems = [raw[i] for i in idx]
    rb = D.collate(ritems)
    assert set(rb) == {"audios", "audio_mix", "id", "class", "infos", "frames_u8", "frame_shapes", "frame_crops", "frame_flips",
                       "imgSize", "split"}
    for k in ("audio_mix", "class"):
        assert torch.equal(rb[k], got[k])
    assert rb["id"] == got["id"] and rb["infos"] == got["infos"] and all(torch.equal(x, y) for x, y in zip(rb["audios"], got["audios"]))
    assert rb["frames_u8"].dtype == torch.uint8 and rb["frames_u8"].dim() == 1
    assert rb["frame_shapes"].dtype == torch.int32 and tuple(rb["frame_shapes"].shape) == (2, 4, 3, 2)
    assert rb["frame_flips"].dtype == torch.bool and tuple(rb["frame_flips"].shape) == (2, 4)
    assert rb["imgSize"] == 64 and rb["split"] == split
    if split == "train":
        assert rb["frame_crops"].dtype == torch.int32 and tuple(rb["frame_crops"].shape) == (2, 4, 2)
        assert rb["frame_crops"].tolist() == [[list(s["frame_crops"][n]) for s in ritems] for n in range(2)]
    else:
        assert rb["frame_crops"] is None and not rb["frame_flips"].any()
    assert rb["frame_flips"].tolist() == [[s["frame_flips"][n] for s in ritems] for n in range(2)]
    assert torch.equal(rb["frames_u8"], torch.cat([s["frames_u8"][n] for n in range(2) for s in ritems]))
    assert rb["frames_u8"].numel() == int((rb["frame_shapes"].long().prod(-1) * 3).sum())


def test_train_command_line_has_its_own_flag():
    from avsep_amd import train as T
    own, rest = T.own_flags(["--gpu_frames", "--imgSize", "64"])
    assert own.gpu_frames is True and rest == ["--imgSize", "64"]
    own, rest = T.own_flags(["--imgSize", "64"])
    assert own.gpu_frames is False and rest == ["--imgSize", "64"]
    assert not hasattr(P.ArgParser().parse_train_arguments([], verbose=False), "gpu_frames")      # not in the reference's table
