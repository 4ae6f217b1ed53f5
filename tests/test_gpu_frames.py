"""gpu: frames as shot (avsep_frames_prepare in csrc/frames.hip, frames.prepare, the uint8 paths of separate_long, localise and
the command line) against the NumPy restatement of tests/frames_ref.py and dataset.VideoTransform itself: never the code under
test.  Everything is an equality of bits: the kernel does integer arithmetic and table look-ups only, so there is no
tolerance to state.  The optional uint8 output tells a resize error (the bytes differ) from a table error (only the floats do).
Helpers of test_gpu_longform.py, test_gpu_localise.py and test_frames_host.py are imported, not copied."""
import types

import numpy as np
import pytest
import torch

import avsep_amd as P
from avsep_amd import dataset as D
from avsep_amd import frames as F
from avsep_amd import localise as L
from avsep_amd import separate as S

import frames_ref as R
import test_frames_host as FH
from recipes import args as _args, tone_mix as _tone_mix
import test_gpu_longform as LF

pytestmark = pytest.mark.gpu

SZ, T = FH.S, 3


def _check(dev, fr, size, what, **kw):
    """frames.prepare of fr uint8 [T,H,W,3] under plan(**kw) against the restatement: the bytes, then the floats."""
    fr = np.ascontiguousarray(fr)
    want = R.prepare(fr, size, **kw)
    plan = F.plan(fr.shape[1], fr.shape[2], size, **kw)
    assert plan.size == want["size"] and plan.crop == want["crop"], what
    out, u8 = F.prepare(torch.from_numpy(fr).to(dev), plan, return_u8=True)
    assert out.shape == (fr.shape[0], 3, size, size) and out.dtype == torch.float32 and u8.dtype == torch.uint8
    bad = (u8.cpu().numpy() != want["cropped"])
    assert not bad.any(), f"{what}: {bad.sum()} of {bad.size} bytes differ, first at {np.argwhere(bad)[0].tolist()}"
    assert torch.equal(out.cpu(), torch.from_numpy(want["out"])), f"{what}: the bytes agree, the normalised values do not"
    assert torch.equal(F.prepare(torch.from_numpy(fr).to(dev), plan), out), what      # without the second output: the same floats
    return out


@pytest.mark.parametrize("H,W", FH.SHAPES)
def test_kernel_equals_the_restatement_validation_form(dev, H, W):
    _check(dev, FH.stack(H, W, T), SZ, f"{H}x{W}")


@pytest.mark.parametrize("H,W", FH.WIDE)
def test_kernel_zero_fills_the_crop_of_very_wide_frames(dev, H, W):
    _check(dev, FH.stack(H, W, T), SZ, f"{H}x{W} under max_size 48", max_size=48)


@pytest.mark.parametrize("H,W", FH.SHAPES)
def test_kernel_equals_the_restatement_training_form(dev, H, W):
    """A crop at each corner of the resized frame and one inside, flip on and off."""
    fr = FH.stack(H, W, T)
    w, h = D._resize_size(W, H, int(SZ * 1.1), 448)
    corners = {(0, 0), (0, w - SZ), (h - SZ, 0), (h - SZ, w - SZ), ((h - SZ) // 2, (w - SZ) // 3)}
    for crop in sorted(corners):
        for flip in (False, True):
            _check(dev, fr, SZ, f"{H}x{W} crop {crop} flip {flip}", train=True, crop=crop, flip=flip)


def test_kernel_clips_a_two_level_image(dev):
    """A 0 / 255 checkerboard of 23 x 17 is upscaled: bicubic overshoots past both ends and the clip to [0, 255] decides."""
    H, W = 23, 17
    board = ((np.add.outer(np.arange(H) // 2, np.arange(W) // 2) % 2) * 255).astype(np.uint8)
    fr = np.stack([np.repeat(board[:, :, None], 3, 2), 255 - np.repeat(board[:, :, None], 3, 2),
                   np.repeat(board[:, ::-1, None], 3, 2)])
    px = R.prepare(fr, SZ)["cropped"]
    assert (px == 0).any() and (px == 255).any() and ((px > 0) & (px < 255)).any()
    _check(dev, fr, SZ, "checkerboard")


def test_kernel_at_360p_to_224(dev):
    """The shape of the host tests' large case and of the bench: 360 x 640 to 224 x 398, 9 taps on both axes, crop column 87,
    49 workgroups per frame."""
    plan = F.plan(360, 640, 224)
    assert plan.size == (398, 224) and plan.crop == (0, 87) and plan.tables[0].shape[1] == plan.tables[2].shape[1] == 9
    _check(dev, FH.stack(360, 640, T), 224, "360x640 -> 224")


def test_kernel_at_270p_to_224(dev):
    """More than one tile on both axes (224 = 7 x 32), tiles that start inside the crop offset, a non-square downscale."""
    out = _check(dev, FH.stack(270, 480, T), 224, "270x480 -> 224")
    assert bool(torch.isfinite(out).all())


def test_kernel_takes_a_stack_that_starts_at_any_byte(dev):
    """Frames of 17 x 23 x 3 = 1173 bytes: a stack sliced out of a longer one, or out of a byte buffer, starts off every
    alignment, and its first and last 16-byte quads hang over the ends of what the kernel may read."""
    H, W = 17, 23
    fr = FH.stack(H, W, 5)
    want = torch.from_numpy(R.prepare(fr, SZ)["out"])
    plan = F.plan(H, W, SZ)
    whole = torch.from_numpy(fr).to(dev)
    for a in range(1, 4):
        assert whole[a:].data_ptr() % 16 != 0
        assert torch.equal(F.prepare(whole[a:], plan).cpu(), want[a:]), a
    for off in (1, 2, 3, 7):
        buf = torch.zeros(off + fr.size + 64, dtype=torch.uint8, device=dev)
        view = buf[off:off + fr.size].view(5, H, W, 3)
        view.copy_(whole)
        assert view.data_ptr() % 16 == off
        assert torch.equal(F.prepare(view, plan).cpu(), want), off


@pytest.mark.parametrize("H,W,size,train", [(36, 64, SZ, False), (360, 640, 224, False), (270, 480, 224, True)])
def test_kernel_equals_video_transform(dev, H, W, size, train):
    """The statement itself, not its restatement: Pillow through dataset.VideoTransform, with the draws replayed."""
    import random
    fr = FH.stack(H, W, T)
    random.seed(5)
    want = FH.video_transform(fr, size, train)
    kw = {}
    if train:
        w, h = D._resize_size(W, H, int(size * 1.1), 448)
        random.seed(5)
        kw = dict(train=True, crop=(random.randint(0, h - size), random.randint(0, w - size)), flip=random.random() < 0.5)
    got = F.prepare(torch.from_numpy(fr).to(dev), F.plan(H, W, size, **kw))
    assert torch.equal(got.cpu(), torch.from_numpy(want))


def test_library_refuses_what_the_host_layer_would_not_send(dev):
    lib = P.lib.load()
    plan = F.plan(36, 64, SZ)
    hc, hb, vc, vb, lut = plan.on(dev)
    fr = torch.zeros(1, 36, 64, 3, dtype=torch.uint8, device=dev)
    out = torch.empty(1, 3, SZ, SZ, device=dev)
    w, h = plan.size

    def call(**kw):
        a = dict(fr=fr.data_ptr(), T=1, H=36, W=64, hc=hc.data_ptr(), hb=hb.data_ptr(), w=w, kh=hc.shape[1], vc=vc.data_ptr(),
                 vb=vb.data_ptr(), h=h, kv=vc.shape[1], S=SZ, i=0, j=9, flip=0, lut=lut.data_ptr(), out=out.data_ptr(), u8=None)
        a.update(kw)
        return lib.avsep_frames_prepare(*a.values(), P.lib.stream())

    assert call() == 0
    for kw in (dict(fr=None), dict(lut=None), dict(out=None), dict(T=0), dict(T=65536), dict(H=0), dict(W=4097), dict(S=7),
               dict(S=1025), dict(flip=2), dict(kh=hc.shape[1] + 2), dict(kv=1), dict(i=5000), dict(w=3, kh=hc.shape[1])):
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# the pipeline: uint8 frames against the same call with the restatement's float frames
# ---------------------------------------------------------------------------------------------------------------------
RATE, HOP, FRAMES, STRIDE, BATCH, IMG = 11025, 256, 400, 128, 2, 64
H0, W0 = 50, 90


def _floats(u8):
    return torch.from_numpy(R.prepare(u8.numpy(), IMG)["out"])


@pytest.fixture(scope="module")
def pipe(dev):
    nets, _, _ = LF._small_nets(dev, 5)
    wav = _tone_mix(HOP * (FRAMES - 1) + 9, 2).to(dev)
    starts = S.plan_windows(FRAMES, STRIDE)
    assert len(starts) == 3
    g = np.random.default_rng(11)
    shot = [torch.from_numpy(g.integers(0, 256, (7, H0, W0, 3), dtype=np.uint8)) for _ in range(2)]
    return types.SimpleNamespace(nets=nets, wav=wav, K=len(starts), shot=shot, prepared=[_floats(s) for s in shot],
                                 times=torch.arange(7, dtype=torch.float64) * 1.3, args=_args(audRate=RATE, imgSize=IMG))


def _both(c, pick, **kw):
    """separate_long with the frames pick(...) makes of the uint8 stacks and of the prepared ones."""
    outs = []
    for stacks in (c.shot, c.prepared):
        with torch.no_grad():
            outs.append(S.separate_long(c.nets, c.wav, pick(stacks), c.args, True, STRIDE, batch=BATCH, return_maps=True, **kw))
    got, want = outs
    assert got["starts"] == want["starts"] and torch.equal(got["perms"], want["perms"])
    for k in ("wavs", "maps"):
        assert torch.equal(got[k], want[k]), k
    assert bool(torch.isfinite(got["wavs"]).all()) and got["wavs"].abs().max().item() > 1e-3
    return got


def test_separate_long_one_shared_uint8_frame(pipe, dev):
    _both(pipe, lambda st: [s[:1].to(dev) for s in st])


def test_separate_long_one_uint8_frame_per_window(pipe, dev):
    _both(pipe, lambda st: [s[:pipe.K].to(dev) for s in st])


def test_separate_long_uint8_clip_on_the_host(pipe, dev):
    """The stacks stay on the host and go up BATCH frames at a time, as bytes: the trunk sees prepared batches."""
    frm = pipe.nets[1]
    seen, trunk = [], frm._trunk
    frm._trunk = lambda x: (seen.append((tuple(x.shape), x.dtype)), trunk(x))[1]
    try:
        _both(pipe, lambda st: list(st), frame_times=pipe.times)
    finally:
        frm._trunk = trunk
    assert all(s == ((n, 3, IMG, IMG), torch.float32) for s, n in zip(seen, [2, 2, 2, 1] * 4)) and len(seen) == 16, seen


def test_separate_long_uint8_duet(pipe, dev):
    _both(pipe, lambda st: [st[0]], frame_times=pipe.times)
    _both(pipe, lambda st: [st[0][:1].to(dev)])


def test_separate_long_refuses_mixed_and_sizeless_uint8_frames(pipe, dev):
    c = pipe
    E = P.lib.AvsepError
    with pytest.raises(E):
        S.separate_long(c.nets, c.wav, [c.shot[0], c.prepared[1]], c.args, True, STRIDE, frame_times=c.times)
    with pytest.raises(E, match="one kind"):
        S.separate_long(c.nets, c.wav, [c.shot[0][:1].to(dev), c.prepared[1][:1].to(dev)], c.args, True, STRIDE)
    with pytest.raises(E, match="imgSize"):
        S.separate_long(c.nets, c.wav, [s[:1].to(dev) for s in c.shot], _args(audRate=RATE), True, STRIDE)
    with pytest.raises(E):
        S.separate_long(c.nets, c.wav, [s[:1, :, :, :2].to(dev) for s in c.shot], c.args, True, STRIDE)


@pytest.mark.parametrize("duet", [False, True])
def test_localise_with_uint8_frames(pipe, dev, duet):
    c = pipe
    outs = []
    for stacks in (c.shot, c.prepared):
        frames = [s.to(dev) for s in (stacks[:1] if duet else stacks)]
        outs.append(L.localise(c.nets, c.wav, frames, c.times, c.args, stride_frames=STRIDE, batch=BATCH))
    got, want = outs
    assert got["overlays"].shape == (2, 7, IMG, IMG, 3)
    for k in ("maps", "best", "scores", "window", "overlays"):
        assert torch.equal(got[k], want[k]), k


# ---------------------------------------------------------------------------------------------------------------------
# command line
# ---------------------------------------------------------------------------------------------------------------------
def test_cli_takes_a_folder_of_pngs_and_a_uint8_npy(dev, tmp_path):
    """python -m avsep_amd.separate in process: a folder of PNGs, a uint8 .npy and the float .npy of the restatement give the
    same files, byte for byte; localise likewise."""
    from PIL import Image
    mb = P.ModelBuilder()
    torch.manual_seed(13)
    snd = mb.build_sound(arch="unet5", fc_dim=2, fusion_type="hidsep", att_type="sig")
    frm = mb.build_frame(arch="resnet18dilated", fc_dim=256, pool_type="maxpool")
    torch.save(snd.state_dict(), str(tmp_path / "sound.pth"))
    torch.save(frm.state_dict(), str(tmp_path / "frame.pth"))
    S.write_wav(str(tmp_path / "mix.wav"), _tone_mix(30000, 8).numpy(), RATE)
    g = np.random.default_rng(3)
    forms = {"png": [], "u8": [], "f32": []}
    for n in range(2):
        shot = g.integers(0, 256, (4, H0, W0, 3), dtype=np.uint8)
        folder = tmp_path / f"clip{n}"
        folder.mkdir()
        for t in range(4):
            Image.fromarray(shot[t]).save(str(folder / f"{t:06d}.png"))
        np.save(str(tmp_path / f"u8_{n}.npy"), shot)
        np.save(str(tmp_path / f"f32_{n}.npy"), R.prepare(shot, IMG)["out"])
        forms["png"].append(str(folder)), forms["u8"].append(str(tmp_path / f"u8_{n}.npy")), forms["f32"].append(str(tmp_path / f"f32_{n}.npy"))
    common = ["--wav", str(tmp_path / "mix.wav"), "--fps", "2", "--imgSize", str(IMG), "--arch_sound", "unet5", "--num_channels", "2",
              "--vis_channels", "256", "--img_pool", "maxpool", "--not_pool_vis", "--fusion_type", "hidsep", "--att_type", "sig",
              "--binary_mask", "0", "--weights_sound", str(tmp_path / "sound.pth"), "--weights_frame", str(tmp_path / "frame.pth")]
    stems, overlays = {}, {}
    for name, files in forms.items():
        out = S.cli(common + ["--frames", *files, "--out", str(tmp_path / f"sep_{name}")])
        assert len(out["starts"]) == 1
        stems[name] = [(tmp_path / f"sep_{name}" / f"source{n}.wav").read_bytes() for n in range(2)]
        L.cli(common + ["--frames", *files, "--out", str(tmp_path / f"loc_{name}")])
        overlays[name] = [np.load(str(tmp_path / f"loc_{name}" / f)) for f in ("maps.npy", "overlay_source0.npy", "overlay_source1.npy")]
    assert len(stems["f32"][0]) > 44 + 2 * 20000 and stems["f32"][0] != stems["f32"][1]
    for name in ("png", "u8"):
        assert stems[name] == stems["f32"], name
        for a, b in zip(overlays[name], overlays["f32"]):
            assert np.array_equal(a, b), name
    # one frame per source without --fps: a uint8 [H,W,3] file
    np.save(str(tmp_path / "one0.npy"), np.load(forms["u8"][0])[0])
    np.save(str(tmp_path / "one1.npy"), np.load(forms["u8"][1])[0])
    np.save(str(tmp_path / "onef0.npy"), np.load(forms["f32"][0])[0])
    np.save(str(tmp_path / "onef1.npy"), np.load(forms["f32"][1])[0])
    still = common[:2] + common[4:]                                   # without --fps 2
    for name, files in (("one", ["one0.npy", "one1.npy"]), ("onef", ["onef0.npy", "onef1.npy"])):
        S.cli(still + ["--frames", *[str(tmp_path / f) for f in files], "--out", str(tmp_path / f"sep_{name}")])
    for n in range(2):
        assert (tmp_path / "sep_one" / f"source{n}.wav").read_bytes() == (tmp_path / "sep_onef" / f"source{n}.wav").read_bytes()
    np.save(str(tmp_path / "chw.npy"), np.zeros((4, 3, H0, W0), np.uint8))
    with pytest.raises(SystemExit, match=r"\(4, 3, 50, 90\)"):
        S.cli(common + ["--frames", str(tmp_path / "chw.npy"), forms["u8"][1], "--out", str(tmp_path / "bad")])
