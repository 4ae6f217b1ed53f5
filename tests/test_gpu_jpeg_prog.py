"""gpu: the progressive JPEG kernels (csrc/jpeg.hip: jpeg_scans_kernel, jpeg_bound_kernel) against the NumPy restatement
(tests/jpeg_prog_ref.py), which tests/test_jpeg_prog_host.py pins to each file's baseline twin and to Pillow: the progressive grid
and the written files mixed with baseline files in ONE plan (pixels and the int16 workspace, guard bytes around every buffer), a
chunk of progressive files only (the zeroing path), the chunked path, the damaged set inside a batch of good files, a
coefficient over the arithmetic bound, decode_stack against load_stack, and `separate` on folders of progressive frames with and
without --gpu_decode."""
import os

import numpy as np
import pytest
import torch

import avsep_amd as P
from avsep_amd import frames as F
from avsep_amd import jpeg
from avsep_amd import separate as S

import jpeg_cases as JC
import jpeg_prog_cases as PC
import jpeg_prog_ref as PR
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
    for k, fill in (("pixels", 0xA5), ("coef", 0x5A5A), ("planes", 0xA5)):
        assert _guards_intact(bufs[k][0], fill), k
    return pixels.cpu().numpy(), status.cpu().numpy(), coef.cpu().numpy()


def _slot(pixels, p, i):
    H, W = p.shapes[i]
    return pixels[int(p.offsets[i]):int(p.offsets[i + 1])].reshape(H, W, 3)


def _progressive_cases():
    """(name, file, Info | ScanInfo, Pillow's pixels, coefficients): the progressive grid and the written files."""
    out = [(n, d, info, px, co) for (n, d, _), (info, px, co) in zip(PC.grid(), PC.grid_reference())]
    return out + [(n, d, info, JC.pillow(d), co) for n, d, info, co in PC.written()]


def _check(cases, p, pixels, status, coef):
    assert not status.any(), status
    for i, (name, _, info, px, co) in enumerate(cases):
        w, at = R.workspace(info, co), int(p.images["block0"][i]) * 64
        assert np.array_equal(coef[at:at + len(w)], w), name                                 # the int16 workspace
        assert np.array_equal(_slot(pixels, p, i), px), name                                 # and so Pillow's pixels


def test_progressive_and_baseline_files_in_one_plan(dev):
    base = [(n, d, info, px, co) for (n, d), (info, px, co) in list(zip(JC.grid(), JC.grid_reference()))[3::5]]
    cases = _progressive_cases()
    assert len(base) == 12 and len(cases) == 85
    mixed = [c for k in range(len(cases)) for c in ([cases[k]] + ([base[k // 7]] if k % 7 == 0 and k // 7 < 12 else []))]
    p = jpeg.plan([d for _, d, _, _, _ in mixed], progressive=True)
    assert not p.fallback and len(p.chunks) == 1 and len(p.images) == 97 and len(p.chunks[0].segs) >= 12
    assert sorted(set(p.chunks[0].scans["level"].tolist())) == [0, 1, 2]
    _check(mixed, p, *_launch(p, dev))


def test_a_chunk_of_progressive_files_only(dev):
    """No baseline segment: avsep_jpeg_entropy does not run, and the level-0 launch zeroes the workspace (0x5A5A before)."""
    cases = _progressive_cases()[20:40]
    p = jpeg.plan([d for _, d, _, _, _ in cases], progressive=True)
    assert not p.fallback and len(p.chunks) == 1 and len(p.chunks[0].segs) == 0 and len(p.chunks[0].scans) > 100
    _check(cases, p, *_launch(p, dev))


def test_chunked_equals_unchunked(dev):
    cases = _progressive_cases()
    files = [d for _, d, _, _, _ in cases] + [d for _, d in JC.grid()[::9]]
    whole, shapes = jpeg.decode(files, dev, progressive=True)
    small = jpeg.plan(files, cap=150 * 128, progressive=True)                                # at most 150 blocks per chunk
    assert len(small.chunks) > 10 and [cases[i][0] for i in small.fallback] == ["128x128-flat"]
    pixels, status, _ = _launch(small, dev)
    keep = np.ones(small.pixel_bytes, dtype=bool)
    for i in small.fallback:                                                                 # the 128 x 128 file is above that cap
        keep[int(small.offsets[i]):int(small.offsets[i + 1])] = False
    assert not status.any() and np.array_equal(pixels[keep], whole.cpu().numpy()[keep])
    cut, shapes2 = jpeg.decode(files, dev, cap=150 * 128, progressive=True)
    assert torch.equal(cut, whole) and shapes == shapes2
    for i, (name, _, _, px, _) in enumerate(cases):
        assert np.array_equal(_slot(whole.cpu().numpy(), small, i), px), name


def test_damaged_files_inside_a_batch(dev):
    good, bad = PC.damaged()
    some = _progressive_cases()[40:47]
    files = [good] + [d for _, d in bad] + [good] + [d for _, d, _, _, _ in some]
    p = jpeg.plan(files, progressive=True)
    assert not p.fallback, p.reasons
    pixels, status, _ = _launch(p, dev)
    want = JC.pillow(good)
    assert status[0] == 0 and status[len(bad) + 1] == 0 and not status[len(bad) + 2:].any()
    for i in (0, len(bad) + 1):
        assert np.array_equal(_slot(pixels, p, i), want)
    for i, (name, _, _, px, _) in enumerate(some, len(bad) + 2):
        assert np.array_equal(_slot(pixels, p, i), px), name
    expect = {"a scan cut at half": 1, "a scan cut one byte short": 1, "a refinement symbol of size 2": 1024,
              "an end-of-band run past the segment": 2048, "a stray marker": 16}
    for i, (name, _) in enumerate(bad, 1):
        assert status[i] != 0 and status[i] == expect.get(name, status[i]), (name, status[i])
        assert (_slot(pixels, p, i) == 0xA5).all(), name                                     # a flagged image is not written
    # rows the lanes must not trust, inside the same batch: the image is flagged, its slot unwritten, its neighbours whole
    ch = p.chunks[0]
    mine = np.flatnonzero((ch.scans["image"] == 0) & (ch.scans["ss"] > 0))
    for field, value, bit in (("se", 64, 256), ("level", 2, 256), ("unit0", 40, 32), ("table", len(p.tables) - 545, 64)):
        q = jpeg.plan(files, progressive=True)
        if field == "table":
            q.chunks[0].scans[field][mine[0]][0] = value
        else:
            q.chunks[0].scans[field][mine[0]] = value
        px, st, _ = _launch(q, dev)
        assert st[0] == bit and (_slot(px, q, 0) == 0xA5).all() and st[len(bad) + 1] == 0, (field, st[0])
        assert np.array_equal(_slot(px, q, len(bad) + 1), want)
    # the public entry: every slot is what Pillow gives that file
    out, shapes = jpeg.decode(files, dev, progressive=True)
    out = out.cpu().numpy()
    for i, d in enumerate(files):
        assert np.array_equal(_slot(out, p, i), JC.pillow(d)), i


def test_a_coefficient_over_the_arithmetic_bound(dev):
    """Inside int16 and over |coefficient x quantiser| <= 1173: only the finished coefficient can tell, so it is
    avsep_jpeg_coef_bound that sets bit 128, and decode hands the file to Pillow."""
    names = [n for n, _, _ in PC.grid()]
    info, _, co = PC.grid_reference()[names.index("33x65-420")]
    co = [c.copy() for c in PR.real_only(info, co)]
    q = int(info.qtables[info.components[0][3]][2])                                          # zig-zag position 2 = natural index 8
    co[0][1, 2, 8] = 1173 // q + 1
    over = PC.write_progressive(co, info, PC.PILLOW_COLOUR)
    co[0][1, 2, 8] = 1173 // q
    under = PC.write_progressive(co, info, PC.PILLOW_COLOUR)
    p = jpeg.plan([over, under], progressive=True)
    assert not p.fallback
    pixels, status, coef = _launch(p, dev)
    assert status.tolist() == [128, 0] and (_slot(pixels, p, 0) == 0xA5).all()
    assert coef[int(p.images["block0"][0]) * 64:][(1 * 10 + 2) * 64 + 8] == 1173 // q + 1    # every lane decoded it: the bound flagged it
    assert np.array_equal(_slot(pixels, p, 1), JC.pillow(under))
    out, _ = jpeg.decode([over, under], dev, progressive=True)
    for i, d in enumerate((over, under)):
        assert np.array_equal(_slot(out.cpu().numpy(), p, i), JC.pillow(d))


def test_decode_stack_of_a_mixed_folder(dev, tmp_path):
    pics = [JC.picture(40, 48, seed=s) for s in range(6)]
    forms = [dict(subsampling=2, quality=85, progressive=True), dict(progressive=True), dict(fmt="PNG"), dict(subsampling=1, quality=70),
             dict(grey=True, progressive=True), dict(subsampling=2, quality=85, restart_marker_blocks=3, progressive=True)]
    for t, (a, form) in enumerate(zip(pics, forms)):
        ext = "png" if form.get("fmt") == "PNG" else ("jpeg" if t == 3 else "jpg")
        (tmp_path / f"{t:06d}.{ext}").write_bytes(JC.encode(a, **form))
    host = F.load_stack(str(tmp_path))
    got = F.load_stack(str(tmp_path), dev)
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (6, 40, 48, 3) and got.is_contiguous()
    assert torch.equal(got.cpu(), host)
    p = jpeg.plan([(tmp_path / n).read_bytes() for n in sorted(os.listdir(tmp_path))], progressive=True)
    assert p.fallback == [2] and "not a JPEG" in p.reasons[2]                                # only the PNG came from Pillow


def test_separate_progressive_frames_with_and_without_gpu_decode(dev, tmp_path):
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
            (folder / f"{t:06d}.jpg").write_bytes(JC.encode(JC.picture(16, 24, seed=100 * n + t), subsampling=2, quality=85, progressive=True))
        folders.append(str(folder))
        p = jpeg.plan([(folder / f"{t:06d}.jpg").read_bytes() for t in range(17)], progressive=True)
        assert not p.fallback and len(p.chunks[0].segs) == 0                                 # every frame goes through the scan kernel
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
