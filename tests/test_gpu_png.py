"""gpu: the PNG decoder's kernels (csrc/png.hip) against Pillow: the whole grid of sizes, colour types, filters and deflate forms
in ONE plan (with guard bytes around every buffer), the window and block edges, the chunked path, a mixed batch of PNGs and JPEGs
through png.decode_stack with refused and damaged files in it, and the public surface: frames.load_stack with and without a
device, and the command lines' --gpu_decode."""
import os

import numpy as np
import pytest
import torch

from avsep_amd import frames as F
from avsep_amd import localise as L
from avsep_amd import png
from avsep_amd import separate as S

import jpeg_cases as JC
import png_cases as PC
from recipes import _guarded, _guards_intact

pytestmark = pytest.mark.gpu


def _launch(p, dev):
    ws_bytes = max(ch.ws_bytes for ch in p.chunks)
    bufs = {"pixels": _guarded(p.pixel_bytes, torch.uint8, 0xA5, dev), "ws": _guarded(ws_bytes, torch.uint8, 0xA5, dev)}
    pixels, status, ws = png.launch(p, dev, bufs["pixels"][1], bufs["ws"][1])
    torch.cuda.synchronize()
    for k, t in (("pixels", pixels), ("ws", ws)):                                            # the kernels worked in the guarded views
        assert t.data_ptr() == bufs[k][1].data_ptr() and t.numel() == bufs[k][1].numel(), k
        assert _guards_intact(bufs[k][0], 0xA5), k
    return pixels.cpu().numpy(), status.cpu().numpy()


def _slot(pixels, p, i):
    H, W = p.shapes[i]
    return pixels[int(p.offsets[i]):int(p.offsets[i + 1])].reshape(H, W, 3)


def test_grid_in_one_call(dev):
    files = PC.grid()
    data = [d for _, d in files]
    p = png.plan(data)
    assert p.fallback == [] and len(p.chunks) == 1 and len(p.images) == 49
    pixels, status = _launch(p, dev)
    assert not status.any(), [(n, s) for (n, _), s in zip(files, status) if s]
    out, shapes = png.decode(data, dev)
    out = out.cpu().numpy()
    assert np.array_equal(out, pixels) and shapes == p.shapes
    for i, (name, d) in enumerate(files):
        assert np.array_equal(_slot(out, p, i), PC.pillow(d)), name


def test_window_and_block_edges(dev):
    noise = np.random.default_rng(5).integers(0, 256, (150, 150, 3)).astype(np.uint8)
    stored, dynamic = PC.write_png(noise, 2, 0, level=0), PC.write_png(noise, 2, 0, level=6)
    assert len(png.probe(stored).idat) > 65535 + 150 and len(dynamic) > 60000                      # more than one stored block
    slide = PC.write_png(PC.picture(96, 128), 2, "cycle", level=9)                                   # 36.9 KB raw: the window slides
    px, stream = PC.window_stream()
    far = PC.wrap(stream, 10, 1365, 2)
    ones = PC.write_png(PC.picture(17, 33), 2, 4, split=1, empties=True)                             # IDAT in 1-byte chunks, empty ones between
    files = [stored, dynamic, slide, far, ones]
    p = png.plan(files)
    assert p.fallback == []
    pixels, status = _launch(p, dev)
    assert not status.any(), status
    for i, d in enumerate(files):
        assert np.array_equal(_slot(pixels, p, i), PC.pillow(d)), i
    assert np.array_equal(_slot(pixels, p, 3), px) and np.array_equal(_slot(pixels, p, 0), noise)


def test_chunked_equals_unchunked(dev):
    files = [d for _, d in PC.grid()]
    whole, shapes = png.decode(files, dev)
    small = png.plan(files, cap=70000)                                                       # 176 894 bytes of scanlines in all
    assert [(ch.a, ch.b) for ch in small.chunks] == [(0, 42), (42, 47), (47, 49)] and small.fallback == []
    pixels, status = _launch(small, dev)
    assert not status.any() and np.array_equal(pixels, whole.cpu().numpy())
    cut, shapes2 = png.decode(files, dev, cap=70000)
    assert torch.equal(cut, whole) and shapes == shapes2


def _mixed(folder):
    """A clip of 40 x 48 frames in every form -> {name: bytes}, and the name of the damaged one."""
    pic = lambda s, ch=3: PC.picture(40, 48, ch, seed=s)
    rgb = PC.write_png(pic(6), 2, "cycle")
    body = bytearray(png.probe(rgb).idat)
    body[len(body) // 2] ^= 0x10
    files = {"000000.png": PC.write_png(pic(0), 2, 4, level=9),
             "000001.png": PC.write_png(pic(1, 1), 0, 3),
             "000002.jpg": JC.encode(JC.picture(40, 48, seed=2), subsampling=2, quality=85),
             "000003.jpg": JC.encode(JC.picture(40, 48, seed=3), progressive=True),
             "000004.png": _interlaced(pic(4)),
             "000005.png": _sixteen(pic(5)),
             "000006.png": PC._with_idat(rgb, bytes(body)),
             "000007.png": PC.pillow_png(pic(7, 4), 6)}
    for n, d in files.items():
        (folder / n).write_bytes(d)
    return files, "000006.png"


def _interlaced(px):
    """Pillow does not write Adam7: the interlaced file is made by hand, pass by pass."""
    raw = bytearray()
    for y0, x0, dy, dx in ((0, 0, 8, 8), (0, 4, 8, 8), (4, 0, 8, 4), (0, 2, 4, 4), (2, 0, 4, 2), (0, 1, 2, 2), (1, 0, 2, 1)):
        sub = px[y0::dy, x0::dx]
        if sub.size:
            raw += PC.filter_rows(np.ascontiguousarray(sub), [0] * sub.shape[0])
    return PC.wrap(PC.deflate(bytes(raw)), px.shape[0], px.shape[1], 2, interlace=1)


def _sixteen(px):
    wide = np.repeat(px.reshape(px.shape[0], px.shape[1] * 3, 1), 2, axis=2).reshape(px.shape[0], px.shape[1], 6)
    return PC.wrap(PC.deflate(PC.filter_rows(wide, [0] * px.shape[0])), px.shape[0], px.shape[1], 2, depth=16)


def test_mixed_batch_through_decode_stack(dev, tmp_path):
    files, damaged = _mixed(tmp_path)
    names = sorted(files)
    good = [n for n in names if n != damaged]
    # the damaged file: the only one with a status bit, and the call raises what Pillow raises for it
    pngs = [files[n] for n in names if n.endswith(".png")]
    p = png.plan(pngs)
    assert p.fallback == [2, 3] and "Adam7" in p.reasons[2] and "bit depth 16" in p.reasons[3]
    pixels, status = _launch(p, dev)
    assert [i for i, s in enumerate(status) if s] == [2] and p.index[2] == 4 and int(status[2]) in png.STATUS
    with pytest.raises(Exception) as pil:
        PC.pillow(files[damaged])
    with pytest.raises(type(pil.value)):
        png.decode_stack([str(tmp_path / n) for n in names], dev)
    with pytest.raises(type(pil.value)):
        png.decode(pngs, dev)
    # without it: every frame is Pillow's, and the stack is what load_stack reads
    stack = png.decode_stack([str(tmp_path / n) for n in good], dev)
    assert stack.is_cuda and stack.dtype == torch.uint8 and tuple(stack.shape) == (7, 40, 48, 3) and stack.is_contiguous()
    for t, n in enumerate(good):
        assert np.array_equal(stack[t].cpu().numpy(), PC.pillow(files[n])), n
    os.remove(str(tmp_path / damaged))
    assert torch.equal(stack.cpu(), F.load_stack(str(tmp_path))) and torch.equal(F.load_stack(str(tmp_path), dev), stack)
    (tmp_path / "000009.png").write_bytes(PC.write_png(PC.picture(24, 48), 2, 1))
    with pytest.raises(SystemExit, match="frames of unequal size: 000009.png is 24 x 48, 000000.png is 40 x 48"):
        F.load_stack(str(tmp_path), dev)


def test_truncated_file_raises_as_pillow(dev):
    d = PC.grid()[4 * 7 + 3][1]
    cut = PC._with_idat(d, png.probe(d).idat[:40])
    with pytest.raises(OSError):
        PC.pillow(cut)
    with pytest.raises(OSError):
        png.decode([PC.grid()[0][1], cut], dev)


def test_load_stack_of_pngs(dev, tmp_path):
    for t in range(5):
        (tmp_path / f"{t:06d}.png").write_bytes(PC.pillow_png(PC.picture(33, 65, 3, seed=t), 2))
    host = F.load_stack(str(tmp_path))
    got = F.load_stack(str(tmp_path), dev)
    assert got.is_cuda and tuple(got.shape) == (5, 33, 65, 3) and torch.equal(got.cpu(), host)
    assert png.plan([(tmp_path / n).read_bytes() for n in sorted(os.listdir(tmp_path))]).fallback == []
    assert S.parse_args(["--wav", "x.wav", "--frames", "a", "b", "--gpu_decode"]).gpu_decode
    assert L.parse_args(["--wav", "x.wav", "--frames", "a", "b", "--fps", "8", "--gpu_decode"]).gpu_decode
