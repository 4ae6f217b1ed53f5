"""gpu: the JPEG decoder's kernels (csrc/jpeg.hip) against the NumPy restatement (tests/jpeg_ref.py), which
tests/test_jpeg_host.py pins to Pillow: the whole grid of sizes and forms in ONE plan (pixels and the int16 coefficient
workspace, with guard bytes around every buffer), the chunked path, the damaged set inside a batch of good files, and the
public surface: decode_stack against load_stack, the loader's jpeg_bytes batch against its raw batch, and `separate` with and
without --gpu_decode."""
import os

import numpy as np
import pytest
import torch

import avsep_amd as P
from avsep_amd import dataset as D
from avsep_amd import frames as F
from avsep_amd import jpeg
from avsep_amd import separate as S

import jpeg_cases as JC
import jpeg_ref as R
from recipes import _guarded, _guards_intact, tone_mix

pytestmark = pytest.mark.gpu


def _launch(p, dev):
    blocks = max(ch.blocks for ch in p.chunks)
    bufs = {"pixels": _guarded(p.pixel_bytes, torch.uint8, 0xA5, dev), "coef": _guarded(blocks * 64, torch.int16, 0x5A5A, dev),
            "planes": _guarded(blocks * 64, torch.uint8, 0xA5, dev)}
    pixels, status, coef, planes = jpeg.launch(p, dev, *(bufs[k][1] for k in ("pixels", "coef", "planes")))
    torch.cuda.synchronize()
    for k, t in (("pixels", pixels), ("coef", coef), ("planes", planes)):                    # the kernels worked in the guarded views
        assert t.data_ptr() == bufs[k][1].data_ptr() and t.numel() == bufs[k][1].numel(), k
    assert not bool((planes == 0xA5).all())
    for k, fill in (("pixels", 0xA5), ("coef", 0x5A5A), ("planes", 0xA5)):
        assert _guards_intact(bufs[k][0], fill), k
    return pixels.cpu().numpy(), status.cpu().numpy(), coef.cpu().numpy()


def _slot(pixels, p, i):
    H, W = p.shapes[i]
    return pixels[int(p.offsets[i]):int(p.offsets[i + 1])].reshape(H, W, 3)


def test_grid_in_one_plan(dev):
    files, ref = JC.grid(), JC.grid_reference()
    p = jpeg.plan([d for _, d in files])
    assert not p.fallback and len(p.chunks) == 1 and len(p.images) == 63
    pixels, status, coef = _launch(p, dev)
    assert not status.any(), status
    for i, ((name, _), (info, px, co)) in enumerate(zip(files, ref)):
        w, at = R.workspace(info, co), int(p.images["block0"][i]) * 64
        assert np.array_equal(coef[at:at + len(w)], w), name                                 # the int16 workspace
        assert np.array_equal(_slot(pixels, p, i), px), name                                 # and so Pillow's pixels


def test_chunked_equals_unchunked(dev):
    files = [d for _, d in JC.grid()]
    whole, shapes = jpeg.decode(files, dev)
    small = jpeg.plan(files, cap=150 * 128)                                                  # at most 150 blocks per chunk
    assert len(small.chunks) > 10 and not small.fallback
    pixels, status, _ = _launch(small, dev)
    assert not status.any() and np.array_equal(pixels, whole.cpu().numpy())
    cut, shapes2 = jpeg.decode(files, dev, cap=150 * 128)
    assert torch.equal(cut, whole) and shapes == shapes2 == [(i.H, i.W) for i, _, _ in JC.grid_reference()]
    # a cap below one file's need sends that file to Pillow: the same bytes still
    at = jpeg.plan(files).offsets
    assert [i for i in jpeg.plan(files[28:35], cap=20 * 128).fallback] == [0, 1, 2, 3, 4, 5]     # 17 x 23: all but the grey file
    tiny, _ = jpeg.decode(files[28:35], dev, cap=20 * 128)
    assert torch.equal(tiny, whole[int(at[28]):int(at[35])])


def test_damaged_files_inside_a_batch(dev):
    good, bad = JC.damaged()
    some = [d for _, d in JC.grid()[40:47]]
    files = [good] + [d for _, d in bad] + [good] + some
    p = jpeg.plan(files)
    assert not p.fallback, p.reasons
    pixels, status, _ = _launch(p, dev)
    want = JC.pillow(good)
    assert status[0] == 0 and status[len(bad) + 1] == 0 and not status[len(bad) + 2:].any()
    for i in (0, len(bad) + 1):
        assert np.array_equal(_slot(pixels, p, i), want)
    for i, (_, (_, px, _)) in enumerate(zip(some, JC.grid_reference()[40:47]), len(bad) + 2):
        assert np.array_equal(_slot(pixels, p, i), px)
    expect = {"cut at half": 1, "cut one byte short": 1, "an AC run past 63": 8, "a DC size of 15": 4, "a stray marker": 16}
    for i, (name, _) in enumerate(bad, 1):
        assert status[i] != 0 and status[i] == expect.get(name, status[i]), (name, status[i])
        assert (_slot(pixels, p, i) == 0xA5).all(), name                                     # a flagged image is not written
    # the public entry: every slot is what Pillow gives that file
    out, shapes = jpeg.decode(files, dev)
    out = out.cpu().numpy()
    for i, d in enumerate(files):
        assert np.array_equal(_slot(out, p, i), JC.pillow(d)), i


def test_decode_stack_equals_load_stack(dev, tmp_path):
    from PIL import Image
    pics = [JC.picture(40, 48, seed=s) for s in range(6)]
    forms = [dict(subsampling=2, quality=85), dict(progressive=True), dict(fmt="PNG"), dict(subsampling=1, quality=70),
             dict(grey=True), dict(subsampling=2, quality=85, restart_marker_blocks=3)]
    for t, (a, form) in enumerate(zip(pics, forms)):
        ext = "png" if form.get("fmt") == "PNG" else ("jpeg" if t == 3 else "jpg")
        (tmp_path / f"{t:06d}.{ext}").write_bytes(JC.encode(a, **form))
    host = F.load_stack(str(tmp_path))
    got = F.load_stack(str(tmp_path), dev)
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (6, 40, 48, 3) and got.is_contiguous()
    assert torch.equal(got.cpu(), host)
    p = jpeg.plan([(tmp_path / n).read_bytes() for n in sorted(os.listdir(tmp_path))])
    assert p.fallback == [1, 2] and "progressive" in p.reasons[1]                            # those two came from Pillow
    Image.fromarray(JC.picture(24, 48)).save(str(tmp_path / "000009.jpg"))
    with pytest.raises(SystemExit, match="frames of unequal size: 000009.jpg is 24 x 48, 000000.jpg is 40 x 48"):
        F.load_stack(str(tmp_path), dev)


@pytest.mark.parametrize("split", ["train", "val"])
def test_loader_batch_equals_the_raw_batch(dev, tmp_path, split):
    import test_frames_batch_host as BH
    from PIL import Image
    lst = BH.make_disk_dataset(tmp_path)
    a = BH.loader_args()
    # one frame the GPU decoder refuses: a progressive file
    row = D.read_list(lst)[0]
    for name in sorted(os.listdir(row[1]))[::5]:
        Image.open(os.path.join(row[1], name)).save(os.path.join(row[1], name), "JPEG", progressive=True, quality=60)
    raw = D.to_device(next(iter(D.make_loader([lst], a, split, batch_size=4, shuffle=False, raw_frames=True))), dev)
    host = next(iter(D.make_loader([lst], a, split, batch_size=4, shuffle=False, raw_frames=True, jpeg_bytes=True)))
    assert "frames" not in host and "frames_u8" not in host and host["frames_jpeg"].dtype == torch.uint8
    byt = D.to_device(host, dev)
    for n in range(2):
        assert byt["frames"][n].shape == (4, 3, 3, 64, 64) and torch.equal(byt["frames"][n], raw["frames"][n]), (split, n)
        assert torch.equal(byt["audios"][n], raw["audios"][n])
    assert torch.equal(byt["audio_mix"], raw["audio_mix"]) and byt["id"] == raw["id"]


def test_separate_with_and_without_gpu_decode(dev, tmp_path):
    mb = P.ModelBuilder()
    torch.manual_seed(13)
    snd = mb.build_sound(arch="unet5", fc_dim=2, fusion_type="hidsep", att_type="sig")
    frm = mb.build_frame(arch="resnet18dilated", fc_dim=256, pool_type="maxpool")
    torch.save(snd.state_dict(), str(tmp_path / "sound.pth"))
    torch.save(frm.state_dict(), str(tmp_path / "frame.pth"))
    S.write_wav(str(tmp_path / "mix.wav"), tone_mix(90000, 8).numpy(), 11025)
    folders = []
    for n in range(2):
        folder = tmp_path / f"clip{n}"
        folder.mkdir()
        for t in range(17):
            (folder / f"{t:06d}.jpg").write_bytes(JC.encode(JC.picture(16, 24, seed=100 * n + t), subsampling=2, quality=85))
        folders.append(str(folder))
    common = ["--wav", str(tmp_path / "mix.wav"), "--fps", "2", "--imgSize", "64", "--arch_sound", "unet5", "--num_channels", "2",
              "--vis_channels", "256", "--img_pool", "maxpool", "--not_pool_vis", "--fusion_type", "hidsep", "--att_type", "sig",
              "--binary_mask", "0", "--weights_sound", str(tmp_path / "sound.pth"), "--weights_frame", str(tmp_path / "frame.pth"),
              "--frames", *folders]
    stems = {}
    for name, flag in (("cpu", []), ("gpu", ["--gpu_decode"])):
        out = S.cli(common + flag + ["--out", str(tmp_path / name)])
        assert len(out["starts"]) == 2
        stems[name] = [(tmp_path / name / f"source{n}.wav").read_bytes() for n in range(2)]
    assert len(stems["cpu"][0]) > 44 + 2 * 80000 and stems["cpu"][0] != stems["cpu"][1]
    assert stems["gpu"] == stems["cpu"]


def test_pixels_entry_refuses_unaligned_workspaces(dev):
    """The block kernel moves 16 bytes at a time: coef or planes off a 16-byte boundary is refused before any launch."""
    p = jpeg.plan([JC.grid()[16][1]])
    ch = p.chunks[0]
    coef = torch.zeros(ch.blocks * 64 + 8, dtype=torch.int16, device=dev)
    planes = torch.zeros(ch.blocks * 64 + 16, dtype=torch.uint8, device=dev)
    pixels = torch.zeros(p.pixel_bytes, dtype=torch.uint8, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    images, tables = torch.from_numpy(p.images.view(np.uint8)).to(dev), torch.from_numpy(p.tables).to(dev)
    L = P.lib.load()

    def call(c, pl):
        return L.avsep_jpeg_pixels(c.data_ptr(), pl.data_ptr(), ch.blocks, images.data_ptr(), 1, ch.max_blocks, ch.max_pixels,
                                   tables.data_ptr(), tables.numel(), status.data_ptr(), pixels.data_ptr(), pixels.numel(), P.lib.stream())
    assert call(coef, planes) == 0 and call(coef[8:], planes[16:]) == 0
    for c, pl in ((coef[1:], planes), (coef[4:], planes), (coef, planes[1:]), (coef, planes[8:])):
        assert call(c, pl) == -1
    torch.cuda.synchronize()
