"""gpu: long-form separation (csrc/longform.hip, avsep_amd/separate.py) against restatements written here from
torch.nn.functional.grid_sample on the oracle's warpgrid, float64 blending and the oracle STFT — never the code under test."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import assert_close

import avsep_amd as P
from avsep_amd import separate as S
from oracle import step as OS, stft as OST
from recipes import args as _args, random_perms as _random_perms, starts_t as _starts_t, tone_mix as _tone_mix

pytestmark = pytest.mark.gpu

W = 256            # frames per window
FOUT = 256         # warped bins
FIN = 512          # linear bins of the 1022-point STFT


# ---------------------------------------------------------------------------------------------------------------------
# restatements (CPU)
# ---------------------------------------------------------------------------------------------------------------------
def ref_resample(x, hout, wout, warp):
    """x [B,C,H,W] float32 -> grid_sample on warpgrid(B, hout, wout, warp), as main.py / inference.py call it."""
    grid = torch.from_numpy(OS.warpgrid(x.shape[0], hout, wout, warp=warp))
    return F.grid_sample(x, grid, align_corners=False)


def ref_slices(mag, starts):
    """mag [Fin,F] -> the materialised windows [K,1,Fin,W], zero past the recording's end."""
    Fr = mag.shape[1]
    out = torch.zeros(len(starts), 1, mag.shape[0], W)
    for k, s in enumerate(starts):
        n = min(W, Fr - s)
        out[k, 0, :, :n] = mag[:, s:s + n]
    return out


def ref_stitch(masks, starts, perm, Fr, fin=FIN):
    """masks [K,N,FOUT,W] float32, perm [K][N] -> float64 [N,fin,Fr]: un-warp each window, triangular cross-fade."""
    Kw, N = masks.shape[:2]
    acc = torch.zeros(N, fin, Fr, dtype=torch.float64)
    wsum = torch.zeros(Fr, dtype=torch.float64)
    j = torch.arange(W)
    tri = torch.minimum(j + 1, W - j).double()
    lin = ref_resample(masks.reshape(Kw * N, 1, FOUT, W), fin, W, False).reshape(Kw, N, fin, W).double()
    for k, s in enumerate(starts):
        n = min(W, Fr - s)
        wsum[s:s + n] += tri[:n]
        for src in range(N):
            acc[src, :, s:s + n] += tri[:n] * lin[k, perm[k][src], :, :n]
    return acc / wsum


def ref_agreement(masks, starts):
    Kw, N = masks.shape[:2]
    D = torch.zeros(Kw - 1, N, N, dtype=torch.float64)
    m = masks.double()
    for k in range(Kw - 1):
        d = starts[k + 1] - starts[k]
        for i in range(N):
            for j in range(N):
                D[k, i, j] = (m[k, i, :, d:] - m[k + 1, j, :, :W - d]).abs().sum()
    return D


def _small_nets(dev, seed):
    """The unet5 / ngf 8 + ResnetDilated(fc_dim=32) pair of test_inference_wrapper_vs_oracle, wide init, eval mode."""
    from oracle import nets as O
    torch.manual_seed(seed)
    gen = torch.Generator().manual_seed(seed)
    osnd = O.Unet(fc_dim=2, num_downs=5, ngf=8, fusion_type="hidsep", att_type="sig")
    O.wide_init(osnd, gen)
    ofrm = O.VisualNet(fc_dim=32, pool_type="maxpool", dilate_scale=16)
    snd = P.models.Unet(fc_dim=2, num_downs=5, ngf=8, fusion_type="hidsep", att_type="sig")
    frm = P.models.ResnetDilated(None, fc_dim=32, pool_type="maxpool")
    snd.load_state_dict(osnd.state_dict()); frm.load_state_dict(ofrm.state_dict())
    return (snd.to(dev).eval(), frm.to(dev).eval()), (osnd.eval(), ofrm.eval()), gen


# ---------------------------------------------------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Fr,stride", [(600, 128), (600, 64), (300, 256), (385, 128), (100, 128), (256, 256)])
def test_window_prepare_vs_sliced_warp(dev, Fr, stride):
    """avsep_window_prepare against slicing the spectrogram on the CPU and warping every slice (F < 256: zero-padded
    window; F = 300 / 385: right-aligned last window).  1e-5: the bound K.warp is held to ('warped mixture')."""
    g = torch.Generator().manual_seed(Fr + stride)
    mag = torch.rand(FIN, Fr, generator=g) ** 2 * 3.0
    starts = S.plan_windows(Fr, stride)
    mix_w, logm = P.kernels.window_prepare(mag.to(dev), _starts_t(starts, dev))
    ref = ref_resample(ref_slices(mag, starts) + 1e-10, FOUT, W, True)
    assert mix_w.shape == ref.shape == (len(starts), 1, FOUT, W)
    assert_close(mix_w, ref, 1e-5, "warped windows")
    assert_close(logm, torch.log(ref), 1e-5, "log of warped windows")
    # per window exactly what the one-tile path makes of the materialised slice
    tile = P.kernels.warp((ref_slices(mag, starts).to(dev) + 1e-10).contiguous(), FOUT, W, 1)
    assert torch.equal(mix_w, tile)


@pytest.mark.parametrize("N", [2, 3])
@pytest.mark.parametrize("Fr,stride", [(600, 64), (600, 128), (600, 256), (300, 64), (300, 128), (300, 256)])
def test_mask_stitch_ratio_masks(dev, Fr, stride, N):
    """Blended linear-frequency mask and mask x magnitude against the float64 restatement, with a non-identity
    permutation table."""
    g = torch.Generator().manual_seed(7 * Fr + stride + N)
    starts = S.plan_windows(Fr, stride)
    Kw = len(starts)
    masks = torch.rand(Kw, N, FOUT, W, generator=g)
    mag = torch.rand(FIN, Fr, generator=g) ** 2 * 3.0
    perm = _random_perms(Kw, N, Fr + N)
    assert any(p != list(range(N)) for p in perm)
    out, lin = P.kernels.mask_stitch(masks.to(dev), _starts_t(starts, dev), torch.tensor(perm, dtype=torch.int32, device=dev),
                                     mag.to(dev), False, 0.5, want_mask=True)
    ref = ref_stitch(masks, starts, perm, Fr)
    assert lin.shape == ref.shape == (N, FIN, Fr)
    assert_close(lin, ref, 1e-5, "blended mask")
    assert_close(out, ref * mag.double(), 1e-5, "mask x magnitude")
    # the optional output may be left out
    out2, none = P.kernels.mask_stitch(masks.to(dev), _starts_t(starts, dev), torch.tensor(perm, dtype=torch.int32, device=dev),
                                       mag.to(dev), False, 0.5)
    assert none is None and torch.equal(out, out2)


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("Fr,stride,N", [(600, 128, 2), (600, 64, 3), (300, 256, 2)])
def test_mask_stitch_binary_masks(dev, Fr, stride, N, seed):
    """Threshold after blending: the binary masks agree element-wise with the float64 restatement outside a band of 1e-5
    (the kernel's own bound) around mask_thres; the band may hold at most 1e-3 of the elements (the restatement alone puts
    3.3e-5 ... 6.2e-5 of them there on these inputs)."""
    thres = 0.5
    g = torch.Generator().manual_seed(seed)
    starts = S.plan_windows(Fr, stride)
    Kw = len(starts)
    masks = torch.rand(Kw, N, FOUT, W, generator=g)
    perm = [list(range(N))] * Kw
    ones = torch.ones(FIN, Fr)
    out, _ = P.kernels.mask_stitch(masks.to(dev), _starts_t(starts, dev), torch.tensor(perm, dtype=torch.int32, device=dev),
                                   ones.to(dev), True, thres)
    ref = ref_stitch(masks, starts, perm, Fr)
    band = (ref - thres).abs() <= 1e-5
    share = band.double().mean().item()
    got = out.cpu()
    wrong = ((got != (ref > thres).float()) & ~band).sum().item()
    print(f"binary stitch F={Fr} stride={stride} N={N} seed={seed}: band share {share:.2e}, mismatches outside {wrong}")
    assert set(got.unique().tolist()) <= {0.0, 1.0}
    assert share <= 1e-3
    assert wrong == 0


@pytest.mark.parametrize("N", [2, 3])
def test_agreement_and_alignment_undo_swapped_windows(dev, N):
    """A smooth mask field over 900 frames cut into windows whose source channels are shuffled: the agreement tensor equals
    its float64 restatement, is bit-identical between runs, and align_permutations recovers the shuffles so that stitching
    gives what the unshuffled windows give."""
    Fr = 900
    g = torch.Generator().manual_seed(11 + N)
    field = F.interpolate(torch.rand(1, N, 9, 31, generator=g), size=(FOUT, Fr), mode="bicubic", align_corners=True)[0]
    field = field.clamp(0, 1)
    starts = S.plan_windows(Fr, 128)
    Kw = len(starts)
    assert starts[-1] - starts[-2] not in (0, 128)                       # a last pair with an odd overlap
    clean = torch.stack([field[:, :, s:s + W] for s in starts])          # [K,N,FOUT,W], channel n = source n
    chan = _random_perms(Kw, N, 5 + N)                                   # chan[k][n]: channel of window k carrying source n
    chan[0] = list(range(N))
    assert sum(c != list(range(N)) for c in chan) >= 2
    shuffled = torch.empty_like(clean)
    for k in range(Kw):
        for n in range(N):
            shuffled[k, chan[k][n]] = clean[k, n]
    st = _starts_t(starts, dev)
    D1 = P.kernels.window_agreement(shuffled.to(dev), st)
    D2 = P.kernels.window_agreement(shuffled.to(dev).clone(), st)
    assert D1.dtype == torch.float64 and D1.shape == (Kw - 1, N, N)
    assert torch.equal(D1, D2)
    Dref = ref_agreement(shuffled, starts)
    assert ((D1.cpu() - Dref).abs() <= 1e-6 * Dref.abs()).all(), ((D1.cpu() - Dref).abs() / Dref.abs().clamp_min(1e-300)).max()
    perms = S.align_permutations(D1)
    assert perms.tolist() == chan
    mag = torch.rand(FIN, Fr, generator=g)
    _, lin = P.kernels.mask_stitch(shuffled.to(dev), st, perms.to(dev), mag.to(dev), False, 0.5, want_mask=True)
    ident = torch.arange(N, dtype=torch.int32).repeat(Kw, 1)
    _, lin0 = P.kernels.mask_stitch(clean.to(dev), st, ident.to(dev), mag.to(dev), False, 0.5, want_mask=True)
    assert_close(lin, lin0, 1e-5, "stitched after alignment vs never shuffled")
    assert_close(lin, ref_stitch(clean, starts, ident.tolist(), Fr), 1e-5, "stitched vs restatement")


# ---------------------------------------------------------------------------------------------------------------------
# whole path
# ---------------------------------------------------------------------------------------------------------------------
def test_masks_to_waveform_sixty_seconds(dev):
    """Given masks -> stitched magnitude -> ONE iSTFT at L = 661 500 (60 s, F = 2 584) against the oracle STFT / iSTFT of the
    restated magnitude: max abs error < 2e-4, the bound of test_eval_path_vs_oracle for the same chain on one tile."""
    L, N = 661500, 2
    wav = _tone_mix(L, 3)
    mag_ref, ph_ref = OST.stft_mag_phase(wav.numpy())
    Fr = mag_ref.shape[1]
    assert Fr == 2584
    starts = S.plan_windows(Fr, 128)
    Kw = len(starts)
    g = torch.Generator().manual_seed(9)
    masks = F.interpolate(torch.rand(Kw * N, 1, 32, 32, generator=g), size=(FOUT, W), mode="bilinear").reshape(Kw, N, FOUT, W)
    perm = [list(range(N))] * Kw
    plan = P.kernels.Stft(dev, 1022, 256, "reflect")
    mag, phase = plan.stft(wav.to(dev)[None])
    assert mag.shape == (1, FIN, Fr)
    assert_close(mag[0], torch.from_numpy(mag_ref), 2e-5, "60 s STFT magnitude")     # the bound of test_stft_against_numpy
    mags, _ = P.kernels.mask_stitch(masks.to(dev), _starts_t(starts, dev), torch.tensor(perm, dtype=torch.int32, device=dev),
                                    mag[0].contiguous(), False, 0.5)
    got = plan.istft(mags, phase.expand(N, -1, -1).contiguous()).clamp_(-1, 1).cpu().numpy()
    assert got.shape == (N, 256 * (Fr - 1))
    M = ref_stitch(masks, starts, perm, Fr)
    for n in range(N):
        ref = OST.istft_reconstruction((mag_ref * M[n].float().numpy()).astype(np.float32), ph_ref)
        err = np.abs(got[n] - ref).max()
        print(f"60 s reconstruction, source {n}: max abs error {err:.3e} (peak {np.abs(ref).max():.3f})")
        assert err < 2e-4


@pytest.mark.parametrize("binary", [1, 0])
def test_one_tile_equals_reconstruct(dev, binary):
    """L = 65 535 with stride 256 is one window: separate_long's waveforms equal evaluate.reconstruct on the same masks."""
    nets, _, gen = _small_nets(dev, 3)
    args = _args(binary_mask=binary)
    wav = _tone_mix(65535, 4).to(dev)
    frames = [torch.randn(1, 3, 64, 64, generator=gen).to(dev) for _ in range(2)]
    with torch.no_grad():
        out = S.separate_long(nets, wav, frames, args, use_vis=True, stride_frames=256, return_masks=True)
        assert out["starts"] == [0] and out["masks"].shape == (1, 2, FOUT, W) and out["perms"].tolist() == [[0, 1]]
        mag, phase = P.kernels.Stft(dev, 1022, 256, "reflect").stft(wav[None])
        data = {"mag_mix": mag[:, None].contiguous(), "phase_mix": phase[:, None].contiguous()}
        rec = P.evaluate.reconstruct(data, {"pred_masks": [out["masks"][:, n:n + 1] for n in range(2)]}, args)
    assert out["wavs"].shape == (2, 256 * 255) == rec[:, 0].shape
    assert (out["wavs"] - rec[:, 0]).abs().max().item() <= 1e-6
    assert out["wavs"].abs().max().item() > 1e-3                          # not a silent agreement


def test_separate_long_masks_vs_oracle_nets(dev):
    """Per-window warped masks of separate_long against the oracle nets run on CPU-sliced windows of the same spectrogram:
    3e-4 (the mask bound of test_inference_wrapper_vs_oracle); shared-frame and per-window-frame forms, AV and AO; the
    shared frame goes through the visual trunk once per source; train-mode nets are refused."""
    from oracle import inference as OI
    nets, onets, gen = _small_nets(dev, 3)
    snd, frm = nets
    args = _args()
    Fr = 700
    wav = _tone_mix(256 * (Fr - 1) + 17, 6)
    with torch.no_grad():
        mag = P.kernels.Stft(dev, 1022, 256, "reflect").stft(wav.to(dev)[None])[0][0].cpu()
    assert mag.shape == (FIN, Fr)
    starts = S.plan_windows(Fr, 128)
    Kw = len(starts)
    assert Kw == 5
    slices = ref_slices(mag, starts)
    shared = [torch.randn(1, 3, 64, 64, generator=gen) for _ in range(2)]
    per_win = [torch.randn(Kw, 3, 64, 64, generator=gen) for _ in range(2)]
    seen = []
    trunk = frm._trunk
    frm._trunk = lambda x: (seen.append(x.shape[0]), trunk(x))[1]

    def check(out, ref, what):
        assert out["starts"] == starts and out["masks"].shape == (Kw, 2, FOUT, W)
        assert out["wavs"].shape == (2, 256 * (Fr - 1)) and bool(torch.isfinite(out["wavs"]).all())
        for n in range(2):
            assert_close(out["masks"][:, n:n + 1], ref["pred_masks"][n], 3e-4, f"{what} mask {n}")
    with torch.no_grad():
        out = S.separate_long(nets, wav.to(dev), [f.to(dev) for f in shared], args, True, 128, batch=2, return_masks=True)
        assert seen == [1, 1], seen
        check(out, OI.forward(onets, (slices, None), [f.expand(Kw, -1, -1, -1).clone() for f in shared], args, True), "AV shared")
        assert out["perms"].tolist() == [[0, 1]] * Kw
        out = S.separate_long(nets, wav.to(dev), [f.to(dev) for f in per_win], args, True, 128, batch=2, return_masks=True)
        check(out, OI.forward(onets, (slices, None), [f.clone() for f in per_win], args, True), "AV per window")
        onets[0].levels()[-1].fusion.ao_draws = torch.zeros(Kw, dtype=torch.bool)
        out = S.separate_long(nets, wav.to(dev), None, args, False, 128, batch=2, return_masks=True)
        check(out, OI.forward(onets, (slices, None), None, args, False), "AO")
        assert snd.ao_draws is None                                       # the pin is taken back
        # stitched masks are the blend of those windows under the permutations found
        ref = ref_stitch(out["masks"].cpu(), starts, out["perms"].tolist(), Fr)
        assert_close(out["lin_masks"], ref, 1e-5, "AO blended masks")
    snd.train()
    with pytest.raises(P.lib.AvsepError):
        S.separate_long(nets, wav.to(dev), [f.to(dev) for f in shared], args, True)
    snd.eval(); frm.train()
    with pytest.raises(P.lib.AvsepError):
        S.separate_long(nets, wav.to(dev), [f.to(dev) for f in shared], args, True)
