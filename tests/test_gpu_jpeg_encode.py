"""gpu: the JPEG encoder's kernels (csrc/jpeg_enc.hip) against the integer restatement (tests/jpeg_encode_ref.py), which
tests/test_jpeg_encode_host.py pins to Pillow, and against Pillow's own files: the whole grid in ONE plan (the int16
coefficient workspace, the per-block bit counts and every file, with guard bytes around the stage buffers), the chunked path,
a mixed batch through the public call, decode(encode(x)), two runs of the same input, and the two places the encoder is used:
visuals.output_visuals with args.gpu_encode and `localise --jpg`."""
import os

import numpy as np
import pytest
import torch

import avsep_amd as P
from avsep_amd import jpeg
from avsep_amd import localise as L
from avsep_amd import visuals as V

import jpeg_encode_cases as EC
import recipes
from recipes import _guarded, _guards_intact

pytestmark = pytest.mark.gpu
KEYS = ("quality", "subsampling", "restart_blocks", "restart_rows")


def _grid_args():
    cases = EC.grid()
    return [a.shape for _, a, _ in cases], {k: [kw[k] for _, _, kw in cases] for k in KEYS}


def _pixels(dev):
    return torch.from_numpy(np.concatenate([a.reshape(-1) for _, a, _ in EC.grid()])).to(dev)


def _launch(p, dev):
    """encode_launch in guarded stage buffers -> (files, coef, bits of the last chunk)."""
    ref = EC.grid_reference()
    blocks = max(ch.blocks for ch in p.chunks)
    # a chunk's unstuffed stream, from the restatement: its intervals' bytes, rounded up to whole words
    need = max(max(4, -(-sum(n for r in ref[ch.a:ch.b] for _, _, n in r.intervals) // 4) * 4) for ch in p.chunks)
    bufs = {"coef": _guarded(blocks * 64, torch.int16, 0x5A5A, dev), "bits": _guarded(blocks, torch.int32, 0x5A5A5A5A, dev),
            "stream": _guarded(need, torch.uint8, 0xA5, dev)}
    assert bufs["coef"][1].data_ptr() % 16 == 0 and bufs["stream"][1].data_ptr() % 4 == 0
    outs, coef, bits, stream = jpeg.encode_launch(p, dev, _pixels(dev), *(bufs[k][1] for k in ("coef", "bits", "stream")))
    torch.cuda.synchronize()
    for k, t in (("coef", coef), ("bits", bits), ("stream", stream)):                        # the kernels worked in the guarded views
        assert t.data_ptr() == bufs[k][1].data_ptr() and t.numel() == bufs[k][1].numel(), k
    for k, fill in (("coef", 0x5A5A), ("bits", 0x5A5A5A5A), ("stream", 0xA5)):
        assert _guards_intact(bufs[k][0], fill), k
    files = []
    for ch, (out, sizes) in zip(p.chunks, outs):
        o, s = out.cpu().numpy(), sizes.cpu().numpy().reshape(-1, 2)
        assert s[0, 0] == 0 and np.array_equal(s[1:, 0], np.cumsum(s[:-1, 1])) and s[:, 1].sum() == len(o)   # back to back, all of out
        files += [p.headers[ch.a + r] + o[at:at + n].tobytes() for r, (at, n) in enumerate(s)]
    return files, coef.cpu().numpy(), bits.cpu().numpy()


def test_grid_in_one_plan(dev):
    cases, want, ref = EC.grid(), EC.grid_pillow(), EC.grid_reference()
    shapes, args = _grid_args()
    p = jpeg.encode_plan(shapes, **args)
    assert len(p.chunks) == 1
    files, coef, bits = _launch(p, dev)
    at = 0
    for (name, _, _), w, r, f in zip(cases, want, ref, files):
        n = len(r.bits)
        assert np.array_equal(coef[at * 64:(at + n) * 64], r.coef.reshape(-1)), name         # the int16 workspace, dummy blocks included
        assert np.array_equal(bits[at:at + n], r.bits), name                                 # every block's Huffman bits
        assert f == w, name                                                                  # and Pillow's file
        at += n
    assert at == p.chunks[0].blocks


def test_chunked_equals_pillow(dev):
    shapes, args = _grid_args()
    p = jpeg.encode_plan(shapes, cap=1600 * 128, **args)
    assert len(p.chunks) >= 3
    files, _, _ = _launch(p, dev)
    for (name, _, _), w, f in zip(EC.grid(), EC.grid_pillow(), files):
        assert f == w, name


def test_mixed_batch_in_one_call(dev):
    """Grey and colour, every sampling and restart setting, list arguments and the defaults, through jpeg.encode."""
    cases, want = EC.grid(), EC.grid_pillow()
    pick = [i for i, (n, _, _) in enumerate(cases) if n.startswith(("17x23-", "24x5-", "33x65-", "40x48-"))]
    assert {f for i in pick for f, _ in EC.FORMS if f"-{f}-" in cases[i][0]} == {f for f, _ in EC.FORMS}
    assert {r for i in pick for r, _ in EC.RESTARTS if cases[i][0].endswith(r)} == {r for r, _ in EC.RESTARTS}
    files = jpeg.encode([torch.from_numpy(cases[i][1]).to(dev) for i in pick], **{k: [cases[i][2][k] for i in pick] for k in KEYS})
    for i, f in zip(pick, files):
        assert f == want[i], cases[i][0]
    # one stack, Pillow's defaults (quality 75, 4:2:0); grey ignores the sampling
    rgb = np.stack([EC.content(c, 40, 48, False, seed=3) for c in ("noise", "smooth", "checker")])
    for stack in (rgb, rgb[..., 1].copy()):
        files = jpeg.encode(torch.from_numpy(stack).to(dev))
        assert files == [EC.pillow_file(a) for a in stack]
    files = jpeg.encode(torch.from_numpy(rgb).to(dev), quality=90, subsampling="4:2:2", restart_rows=2)
    assert files == [EC.pillow_file(a, quality=90, subsampling=1, restart_marker_rows=2) for a in rgb]
    with pytest.raises(P.lib.AvsepError):
        jpeg.encode(torch.from_numpy(rgb).to(dev).float())


def test_decode_of_encode_is_pillows(dev):
    import jpeg_cases as JC
    pics = [EC.content(c, H, W, grey, seed=5) for c, H, W, grey in (("smooth", 33, 65, False), ("noise", 17, 23, False),
                                                                     ("smooth", 40, 48, True), ("checker", 9, 40, False))]
    subs = [2, 1, 2, 0]
    files = jpeg.encode([torch.from_numpy(a).to(dev) for a in pics], quality=85, subsampling=subs, restart_blocks=[0, 2, 0, 0])
    pixels, shapes = jpeg.decode(files, dev)
    assert shapes == [a.shape[:2] for a in pics]
    pixels, at = pixels.cpu().numpy(), 0
    for a, sub, rb in zip(pics, subs, [0, 2, 0, 0]):
        kw = dict(quality=85, restart_marker_blocks=rb)
        if a.ndim == 3:
            kw["subsampling"] = sub
        want = JC.pillow(EC.pillow_file(a, **kw))                                            # Pillow's decode of Pillow's file
        n = want.size
        assert np.array_equal(pixels[at:at + n].reshape(want.shape), want)
        at += n


def test_two_runs_give_the_same_bytes(dev):
    a = torch.from_numpy(np.stack([EC.content("noise", 72, 136, False, seed=s) for s in range(4)])).to(dev)
    one = jpeg.encode(a, quality=100, subsampling=0, restart_blocks=2)
    two = jpeg.encode(a, quality=100, subsampling=0, restart_blocks=2)
    assert one == two and one[0] == EC.pillow_file(a[0].cpu().numpy(), quality=100, subsampling=0, restart_marker_blocks=2)


def test_output_visuals_with_gpu_encode(dev, tmp_path):
    (snd, frm), gen = recipes.small_nets(dev, 7)
    mb = P.ModelBuilder()
    wrap = P.NetWrapper((snd, frm), mb.build_criterion("bce", use_pit=True), mb.build_criterion("bce"))
    wrap.eval()
    B, Fin, T = 2, 65, 64
    srcs = [torch.rand(B, 1, Fin, T, generator=gen) ** 2 * 4 for _ in range(2)]
    batch = {"mag_mix": (srcs[0] + srcs[1]).to(dev), "mags": [s.to(dev) for s in srcs],
             "phase_mix": (torch.rand(B, 1, Fin, T, generator=gen) * 6.0 - 3.0).to(dev), "id": ["first", "second"],
             "frames": [torch.randn(B, 3, 2, 64, 64, generator=gen).to(dev) for _ in range(2)]}
    metrics = {"pred_wavs": (torch.rand(2, B, 2016, generator=gen) - 0.5).to(dev)}
    written = {}
    with torch.no_grad():
        _, outputs = wrap.forward(batch, recipes.args(weighted_loss=1, match_weight=0.1, stft_frame=128, stft_hop=32, mask_thres=0.5), True)
    for name, flag in (("pillow", False), ("gpu", True)):
        args = recipes.args(weighted_loss=1, match_weight=0.1, stft_frame=128, stft_hop=32, mask_thres=0.5, audRate=11025,
                            vis=str(tmp_path / name), num_vis=2, gpu_encode=flag)
        rows = []
        assert V.output_visuals(rows, batch, outputs, args, metrics, True) == 2 and len(rows) == 2
        root = tmp_path / name / "av"
        written[name] = {os.path.join(d, f): recipes.file_bytes(root / d / f) for d in sorted(os.listdir(root)) for f in sorted(os.listdir(root / d))}
    # the GPU's files against Pillow's save of the rendered images, whatever the other path wrote
    for key, stack in V.item_images(batch, outputs, args, 2).items():
        for j, item in enumerate(("first", "second")):
            assert written["gpu"][os.path.join(item, key + ".jpg")] == EC.pillow_file(stack[j].cpu().numpy()), (item, key)
    jpgs = [k for k in written["pillow"] if k.endswith(".jpg")]
    assert len(jpgs) == 2 * (2 + 4 * 2) and sorted(written["gpu"]) == sorted(written["pillow"])
    for k in jpgs:
        assert written["gpu"][k] == written["pillow"][k], k                                  # byte for byte
    assert all(written["gpu"][k] == written["pillow"][k] for k in written["pillow"] if k.endswith(".png"))   # still Pillow's


def test_localise_cli_writes_pillows_jpgs(dev, tmp_path):
    from avsep_amd.separate import write_wav
    mb = P.ModelBuilder()
    torch.manual_seed(11)
    snd = mb.build_sound(arch="unet5", fc_dim=2, fusion_type="hidsep", att_type="sig")
    frm = mb.build_frame(arch="resnet18dilated", fc_dim=256, pool_type="maxpool")
    torch.save(snd.state_dict(), str(tmp_path / "sound.pth"))
    torch.save(frm.state_dict(), str(tmp_path / "frame.pth"))
    write_wav(str(tmp_path / "mix.wav"), recipes.tone_mix(30000, 8).numpy(), 11025)
    T = 5
    rng = np.random.default_rng(3)
    mean, std = np.array(V.MEAN, dtype=np.float32), np.array(V.STD, dtype=np.float32)
    paths = []
    for n in range(2):
        shot = rng.integers(0, 256, size=(T, 64, 64, 3), dtype=np.uint8)
        np.save(str(tmp_path / f"f{n}.npy"), np.ascontiguousarray(((shot / np.float32(255.0) - mean) / std).astype(np.float32).transpose(0, 3, 1, 2)))
        paths.append(str(tmp_path / f"f{n}.npy"))
    out = L.cli(["--wav", str(tmp_path / "mix.wav"), "--fps", "2", "--arch_sound", "unet5", "--num_channels", "2", "--vis_channels", "256",
                 "--img_pool", "maxpool", "--not_pool_vis", "--fusion_type", "hidsep", "--att_type", "sig", "--weights_sound",
                 str(tmp_path / "sound.pth"), "--weights_frame", str(tmp_path / "frame.pth"), "--frames", *paths, "--out",
                 str(tmp_path / "out"), "--jpg", "--jpg_quality", "80"])
    assert tuple(out["overlays"].shape) == (2, T, 64, 64, 3)
    names = sorted(os.listdir(tmp_path / "out"))
    assert names == sorted(["maps.npy", "overlay_source0.npy", "overlay_source1.npy"] + [f"source{c}_frame{t:05d}.jpg" for c in range(2) for t in range(T)])
    for c in range(2):
        ov = np.load(str(tmp_path / "out" / f"overlay_source{c}.npy"))
        for t in range(T):
            assert recipes.file_bytes(tmp_path / "out" / f"source{c}_frame{t:05d}.jpg") == EC.pillow_file(ov[t], quality=80), (c, t)
