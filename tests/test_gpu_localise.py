"""gpu: localisation (csrc/localise.hip, avsep_amd/localise.py).  The maps kernel against the CPU oracle's fusion run once
per frame, the overlay kernel bit for bit against the NumPy restatement in tests/localise_ref.py, and localise() against the
existing slow path: inference.NetWrapper.forward called once per video frame."""
import argparse
import itertools
import math

import numpy as np
import pytest
import torch

from conftest import assert_close

import avsep_amd as P
from avsep_amd import localise as L
from avsep_amd.separate import plan_windows
from oracle import nets as O

import localise_ref as R

pytestmark = pytest.mark.gpu

MARGIN = 1e-4          # `best` is compared wherever the oracle's two top scores are further apart than this


# ---------------------------------------------------------------------------------------------------------------------
# maps kernel
# ---------------------------------------------------------------------------------------------------------------------
def oracle_frame(att, x1, vs1):
    """The oracle's fusion on ONE frame: x1 [1,D,Fq,Tq], vs1 C tensors [1,Dc,h,w] -> (att_maps [C,h,w], scores [C!])."""
    maps = O.Fusion("hidsep", att)(x1, vs1)[1][1][0]
    C, Dc = len(vs1), x1.shape[1] // len(vs1)
    a = torch.amax(x1, dim=(2, 3))[:, :C * Dc].view(1, C, Dc)
    table = torch.tensor(list(itertools.permutations(range(C))))
    m = O._attend(att, a[:, table], torch.stack(vs1, 1)[:, None], Dc)                # [1,P,C,h,w]
    return maps, torch.amax(m, dim=(3, 4)).sum(-1)[0]


def _map_case(att, C, duet, Kw, hw, Dc, D, seed, T=10, Fq=2, Tq=3):
    """Inputs of one case and the oracle's answer per frame (CPU only)."""
    g = torch.Generator().manual_seed(100 * seed + (att == "cos"))
    x = torch.randn(Kw, D, Fq, Tq, generator=g)
    vs = [torch.randn(T, Dc, *hw, generator=g) for _ in range(1 if duet else C)]
    if duet:
        vs = vs * 2
    win = torch.tensor([(2 * t + 1) % Kw for t in range(T)], dtype=torch.int32)
    assert Kw == 1 or len(set(win.tolist())) == Kw
    ref_maps, ref_scores = zip(*[oracle_frame(att, x[win[t]][None], [v[t][None] for v in vs]) for t in range(T)])
    ref_maps, ref_scores = torch.stack(ref_maps), torch.stack(ref_scores)
    top2 = ref_scores.sort(1, descending=True)[0][:, :2]
    return x, vs, win, ref_maps, ref_scores, top2[:, 0] - top2[:, 1]


MAP_CASES = [
    # C, duet, K, (h, w), Dc, D, seed
    (2, False, 1, (14, 14), 256, 512, 1),
    (2, False, 3, (7, 9), 37, 74, 2),
    (2, True, 3, (14, 14), 256, 512, 3),
    (2, True, 1, (7, 9), 37, 74, 4),
    (3, False, 3, (14, 14), 256, 768, 8),
    (3, False, 1, (7, 9), 37, 112, 6),          # D = 3 * 37 + 1: the remainder channel takes no part
]


@pytest.mark.parametrize("att", ["sig", "cos"])
@pytest.mark.parametrize("C,duet,Kw,hw,Dc,D,seed", MAP_CASES)
def test_maps_kernel_vs_oracle_fusion_per_frame(dev, att, C, duet, Kw, hw, Dc, D, seed):
    """1e-5 through assert_close: the bound tests/test_gpu_model.py applies to the fusion kernel's att_maps."""
    x, vs, win, ref_maps, ref_scores, margin = _map_case(att, C, duet, Kw, hw, Dc, D, seed)
    T = win.numel()
    dv = [v.to(dev) for v in (vs[:1] if duet else vs)]
    maps, best, scores = P.kernels.localise_maps(x.to(dev), win.to(dev), dv * 2 if duet else dv, att)
    assert maps.shape == (T, C, *hw) and best.dtype == torch.int32 and scores.shape == (T, math.factorial(C))
    print(f"maps {att} C={C} duet={duet} K={Kw} hw={hw} Dc={Dc}: min margin {margin.min().item():.3e}, "
          f"max|d| {(maps.cpu() - ref_maps).abs().max().item():.3e} of max|ref| {ref_maps.abs().max().item():.3e}")
    assert_close(maps, ref_maps, 1e-5, "maps")
    assert_close(scores, ref_scores, 1e-5, "scores")
    if duet:
        assert (margin == 0).all()                       # both permutations tie by construction
        assert best.cpu().tolist() == [0] * T
        assert not torch.equal(maps[:, 0], maps[:, 1])   # one visual input, two audio blocks: two different maps
    else:
        assert (margin > MARGIN).all(), margin           # seeds chosen so that every frame is decided
        assert best.cpu().tolist() == ref_scores.argmax(1).tolist()
        assert len(set(best.cpu().tolist())) > 1         # not one permutation throughout


def test_maps_kernel_argument_errors(dev):
    x = torch.zeros(1, 8, 4, device=dev)
    v = torch.zeros(2, 4, 3, 3, device=dev)
    win = torch.zeros(2, dtype=torch.int32, device=dev)
    with pytest.raises(P.lib.AvsepError):
        P.kernels.localise_maps(x.reshape(1, 8, 2, 2), win, [v], "sig")                      # one visual input
    with pytest.raises(P.lib.AvsepError):
        P.kernels.localise_maps(x.reshape(1, 8, 2, 2), win, [v, v[:, :3].contiguous()], "sig")
    # window indices outside [0, K) are clamped, not followed
    maps, _, _ = P.kernels.localise_maps(torch.randn(2, 8, 2, 2, device=dev), torch.tensor([-5, 9], dtype=torch.int32, device=dev),
                                         [torch.randn(2, 4, 3, 3, device=dev)] * 2, "sig")
    assert bool(torch.isfinite(maps).all())


# ---------------------------------------------------------------------------------------------------------------------
# overlay kernel
# ---------------------------------------------------------------------------------------------------------------------
def _normalised(img):
    """uint8 [T,H,W,3] -> float32 [T,3,H,W] by the package's normalisation (dataset.py:100-102)."""
    mean = torch.tensor(P.dataset._MEAN).view(3, 1, 1)
    std = torch.tensor(P.dataset._STD).view(3, 1, 1)
    return torch.stack([(torch.from_numpy(f.copy()).permute(2, 0, 1).float().div_(255.0) - mean) / std for f in img])


OVERLAY_CASES = [
    # (h, w), (H, W), what
    ((14, 14), (224, 224), "x16"),
    ((7, 9), (100, 60), "non-integer ratios"),
    ((7, 9), (7, 9), "identity"),
    ((5, 3), (15, 13), "odd pixel count: byte stores"),
    ((4, 4), (64, 64), "constant"),
]


@pytest.mark.parametrize("alpha256", [0, 102, 256])
@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("hw,HW,what", OVERLAY_CASES)
def test_overlay_kernel_bit_exact(dev, hw, HW, what, shared, alpha256):
    T, C = 3, 2
    rng = np.random.default_rng(1000 * hw[0] + 10 * HW[1] + int(shared))
    maps = (1.0 / (1.0 + np.exp(-rng.normal(size=(T, C, *hw)) * 2.0))).astype(np.float32)
    if what == "constant":
        maps[0, 0] = 0.5
        maps[1, 1] = 0.0
    imgs = [rng.integers(0, 256, size=(T, *HW, 3), dtype=np.uint8) for _ in range(1 if shared else C)]
    frames = [_normalised(i) for i in imgs]
    table = L.jet_table()
    dframes = [f.to(dev) for f in frames]
    out = P.kernels.heatmap_overlay(torch.from_numpy(maps).to(dev), dframes * 2 if shared else dframes,
                                    torch.from_numpy(table).to(dev), alpha256)
    assert out.dtype == torch.uint8 and out.shape == (C, T, *HW, 3)
    got = out.cpu().numpy()
    for c in range(C):
        fr = frames[0 if shared else c].numpy()
        for t in range(T):
            want = R.overlay(maps[t, c], fr[t], table, alpha256)
            bad = int((got[c, t] != want).sum())
            assert bad == 0, f"{what} source {c} frame {t}: {bad} of {want.size} bytes differ, max " \
                             f"{np.abs(got[c, t].astype(int) - want.astype(int)).max()} levels"
    if alpha256 == 0:                                      # the frame alone: the uint8 image the frame was made from
        for c in range(C):
            assert np.array_equal(got[c], imgs[0 if shared else c])
    if alpha256 == 256 and what == "constant":
        assert (got[0, 0] == table[0]).all() and (got[1, 1] == table[0]).all()


def test_overlay_kernel_argument_errors(dev):
    maps = torch.rand(1, 2, 4, 4, device=dev)
    fr = torch.zeros(1, 3, 8, 8, device=dev)
    table = torch.from_numpy(L.jet_table()).to(dev)
    with pytest.raises(P.lib.AvsepError):
        P.kernels.heatmap_overlay(maps, [fr, fr], table, 257)
    with pytest.raises(P.lib.AvsepError):
        P.kernels.heatmap_overlay(maps, [fr], table, 100)
    with pytest.raises(P.lib.AvsepError):
        P.kernels.heatmap_overlay(maps, [fr, fr], table[:, :2].contiguous(), 100)


# ---------------------------------------------------------------------------------------------------------------------
# localise() against one NetWrapper.forward per frame
# ---------------------------------------------------------------------------------------------------------------------
def _args(**kw):
    a = argparse.Namespace(num_mix=2, log_freq=1, binary_mask=1, mask_thres=0.5, output_activation="sigmoid",
                           img_activation="relu", not_pool_vis=False, fusion_type="hidsep", stft_frame=1022, stft_hop=256,
                           stft_pad_mode="reflect", audRate=11025)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _small_nets(dev, seed, fusion_type="hidsep"):
    """unet5 / ngf 8 + ResnetDilated(fc_dim=32), wide init (the default init gives maps == 0.5 everywhere), eval mode."""
    torch.manual_seed(seed)
    gen = torch.Generator().manual_seed(seed)
    osnd = O.Unet(fc_dim=2, num_downs=5, ngf=8, fusion_type=fusion_type, att_type="sig")
    O.wide_init(osnd, gen)
    ofrm = O.VisualNet(fc_dim=32, pool_type="maxpool", dilate_scale=16)
    snd = P.models.Unet(fc_dim=2, num_downs=5, ngf=8, fusion_type=fusion_type, att_type="sig")
    frm = P.models.ResnetDilated(None, fc_dim=32, pool_type="maxpool")
    snd.load_state_dict(osnd.state_dict()); frm.load_state_dict(ofrm.state_dict())
    return (snd.to(dev).eval(), frm.to(dev).eval()), gen


def _tone_mix(Ls, seed, rate=11025):
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(Ls, dtype=torch.float64) / rate
    x = torch.zeros(Ls, dtype=torch.float64)
    for f0, a, v in ((220.0, 0.25, 0.3), (523.25, 0.2, 0.11), (1318.5, 0.12, 0.05), (3200.0, 0.06, 0.7)):
        x += a * torch.sin(2 * np.pi * f0 * t * (1 + 0.01 * torch.sin(2 * np.pi * v * t))) * (0.5 + 0.5 * torch.sin(2 * np.pi * 0.4 * v * t))
    x += 0.02 * torch.randn(Ls, generator=g, dtype=torch.float64)
    return x.float()


def _slow_maps(nets, mag_slice, frames, t, args):
    """The existing path: the whole inference wrapper on one spectrogram tile and ONE video frame."""
    wrap = P.inference.NetWrapper(nets)
    with torch.no_grad():
        out = wrap.forward((mag_slice[None, None].contiguous(), None), [f[t:t + 1].contiguous() for f in frames], args, True)
    return out["maps"][0]


@pytest.mark.parametrize("duet", [False, True])
def test_localise_one_tile_vs_wrapper_per_frame(dev, duet):
    """One tile, T = 12: every frame's maps against NetWrapper.forward on that frame; 2e-4, the bound tests/test_gpu_model.py
    applies to model-level maps."""
    nets, gen = _small_nets(dev, 3)
    args = _args()
    T = 12
    wav = _tone_mix(65535, 4).to(dev)
    imgs = [np.random.default_rng(7 + n).integers(0, 256, size=(T, 64, 64, 3), dtype=np.uint8) for n in range(1 if duet else 2)]
    frames = [_normalised(i).to(dev) for i in imgs]
    times = torch.arange(T, dtype=torch.float64) * (65535 / 11025 / T)
    out = L.localise(nets, wav, frames, times, args, batch=5)
    assert out["starts"] == [0] and out["window"].tolist() == [0] * T and out["window"].dtype == torch.int32
    assert out["maps"].shape == (T, 2, 4, 4) and out["best"].shape == (T,) and out["scores"].shape == (T, 2)
    assert out["overlays"].shape == (2, T, 64, 64, 3) and out["overlays"].dtype == torch.uint8
    with torch.no_grad():
        mag = P.kernels.Stft(dev, 1022, 256, "reflect").stft(wav[None], want_phase=False)[0][0].contiguous()
    assert mag.shape == (512, 256)
    worst = 0.0
    for t in range(T):
        ref = _slow_maps(nets, mag, frames, t, args)
        worst = max(worst, (out["maps"][t] - ref).abs().max().item() / ref.abs().max().item())
        assert_close(out["maps"][t], ref, 2e-4, f"maps of frame {t}")
    spread = (out["maps"].amax(dim=(2, 3)) - out["maps"].amin(dim=(2, 3))).min().item()
    print(f"one tile duet={duet}: worst max|d|/max|ref| {worst:.3e}, least spread within a map {spread:.3e}")
    assert spread > 1e-3                                   # not the flat 0.5 of an untrained default init
    if duet:
        assert out["best"].cpu().tolist() == [0] * T
    # the overlays are the restatement applied to those maps
    table = L.jet_table()
    maps = out["maps"].cpu().numpy()
    got = out["overlays"].cpu().numpy()
    for c in range(2):
        fr = frames[0 if duet else c].cpu().numpy()
        for t in (0, T - 1):
            assert np.array_equal(got[c, t], R.overlay(maps[t, c], fr[t], table, 102))
    no = L.localise(nets, wav, frames, times, args, render=False)
    assert "overlays" not in no and torch.equal(no["maps"], out["maps"])


def test_localise_three_windows_vs_wrapper_on_slices(dev):
    """Fr = 500 frames -> windows [0, 128, 244]: frame t against the wrapper on the materialised slice of window[t]."""
    nets, gen = _small_nets(dev, 5)
    args = _args()
    T, Fr = 12, 500
    Ls = 256 * (Fr - 1) + 17
    wav = _tone_mix(Ls, 6).to(dev)
    frames = [torch.randn(T, 3, 64, 64, generator=gen).to(dev) for _ in range(2)]
    times = torch.linspace(0.0, Ls / 11025, T, dtype=torch.float64)
    out = L.localise(nets, wav, frames, times, args, stride_frames=128, batch=4)
    starts = plan_windows(Fr, 128)
    assert out["starts"] == starts == [0, 128, 244]
    assert out["window"].tolist() == L.window_of_frames(times, starts, 11025, 256).tolist()
    assert sorted(set(out["window"].tolist())) == [0, 1, 2]
    with torch.no_grad():
        mag = P.kernels.Stft(dev, 1022, 256, "reflect").stft(wav[None], want_phase=False)[0][0].contiguous()
    assert mag.shape == (512, Fr)
    for t in range(T):
        s = starts[out["window"][t]]
        ref = _slow_maps(nets, mag[:, s:s + 256].contiguous(), frames, t, args)
        assert_close(out["maps"][t], ref, 2e-4, f"maps of frame {t} (window {out['window'][t]})")
    # the windows do differ: scoring every frame against window 0 is not the same thing
    one = L.localise(nets, wav[:65535].contiguous(), frames, times, args, render=False)
    assert (one["maps"] - out["maps"]).abs().max().item() > 1e-3


def test_localise_refusals(dev):
    nets, gen = _small_nets(dev, 3)
    snd, frm = nets
    args = _args()
    wav = _tone_mix(65535, 4).to(dev)
    frames = [torch.randn(2, 3, 64, 64, generator=gen).to(dev) for _ in range(2)]
    times = [0.0, 1.0]
    snd.train()
    with pytest.raises(P.lib.AvsepError):
        L.localise(nets, wav, frames, times, args)
    snd.eval(); frm.train()
    with pytest.raises(P.lib.AvsepError):
        L.localise(nets, wav, frames, times, args)
    frm.eval()
    with pytest.raises(NotImplementedError):
        L.localise(nets, wav, frames, times, _args(fusion_type="MixVis"))
    with pytest.raises(P.lib.AvsepError):
        L.localise(nets, wav, frames, times, _args(not_pool_vis=True))          # pooled features: no spatial map
    with pytest.raises(P.lib.AvsepError):
        L.localise(nets, wav, frames, [0.0], args)                              # one time per frame
    with pytest.raises(P.lib.AvsepError):
        L.localise(nets, wav, frames[:1], times, _args(num_mix=3))              # a duet has two sources
    with pytest.raises(P.lib.AvsepError):
        L.localise(nets, wav[:100].contiguous(), frames, times, args)


def test_cli_writes_maps_and_overlay_stacks(dev, tmp_path):
    """python -m avsep_amd.localise in process: a WAV and one (duet) or two frame stacks in, maps.npy and one overlay stack
    per source out, equal to what localise() returns for the same inputs."""
    from avsep_amd.separate import write_wav
    mb = P.ModelBuilder()
    torch.manual_seed(11)
    snd = mb.build_sound(arch="unet5", fc_dim=2, fusion_type="hidsep", att_type="sig")
    frm = mb.build_frame(arch="resnet18dilated", fc_dim=256, pool_type="maxpool")
    torch.save(snd.state_dict(), str(tmp_path / "sound.pth"))
    torch.save(frm.state_dict(), str(tmp_path / "frame.pth"))
    write_wav(str(tmp_path / "mix.wav"), _tone_mix(30000, 8).numpy(), 11025)
    T = 5
    rng = np.random.default_rng(3)
    paths = []
    for n in range(2):
        np.save(str(tmp_path / f"f{n}.npy"), _normalised(rng.integers(0, 256, size=(T, 64, 64, 3), dtype=np.uint8)).numpy())
        paths.append(str(tmp_path / f"f{n}.npy"))
    common = ["--wav", str(tmp_path / "mix.wav"), "--fps", "2", "--arch_sound", "unet5", "--num_channels", "2", "--vis_channels", "256",
              "--img_pool", "maxpool", "--not_pool_vis", "--fusion_type", "hidsep", "--att_type", "sig", "--weights_sound", str(tmp_path / "sound.pth"),
              "--weights_frame", str(tmp_path / "frame.pth")]
    for files, name in ((paths, "two"), (paths[:1], "duet")):
        outdir = tmp_path / name
        out = L.cli(common + ["--frames", *files, "--out", str(outdir)])
        maps = np.load(str(outdir / "maps.npy"))
        assert maps.shape == (T, 2, 4, 4) and maps.dtype == np.float32 and np.array_equal(maps, out["maps"].cpu().numpy())
        for c in range(2):
            ov = np.load(str(outdir / f"overlay_source{c}.npy"))
            assert ov.shape == (T, 64, 64, 3) and ov.dtype == np.uint8 and np.array_equal(ov, out["overlays"][c].cpu().numpy())
        assert sorted(p.name for p in outdir.iterdir()) == ["maps.npy", "overlay_source0.npy", "overlay_source1.npy"]
