"""gpu: the mixture-consistent phase iterations (avsep_misi in csrc/misi.hip, kernels.Stft.misi, separate_long(phase_iters=...)
and --phase_iters of avsep_amd/separate.py) against the float64 restatement tests/misi_ref.py fed the same fp32 inputs.
Waveforms are compared with max|d| / max|ref| per case; the returned phase only through A e^{i phase}, never as an angle
(the phase of a near-zero value is arbitrary).

The tolerance is derived, not chosen.  The restatement's float32 mode (float32 window, complex64 FFTs, float32 overlap-add
and division by |Z|) was run on the CPU over exactly the value cases below (misi_ref.VALUE_CASES; test_misi_host.py
re-measures it): its worst distance from the float64 mode is 9.160e-06 (1022/256/9, N = 2, G = 2, two passes, a phase per
source; most cases stay below 1e-06).  Recorded rounded up as misi_ref.F32_WORST = 9.2e-06, the kernels get 16 x:
    BOUND = 1.472e-04.
The factor covers another summation order in the GEMMs and in the overlap-add, rsqrt against a division, and sincosf on the
start phase.  On an MI355X the waveforms sit at 1.4e-07 ... 4.7e-06 over those cases and A e^{i phase} at 0.9e-07 ... 9.0e-05.

separate_long: the outputs are compared with the restatement run on the call's own fp32 magnitudes and start phase (the
blended masks of return_masks times the STFT the plan gives outside the call, the same kernels and so the same bits as
inside it).  The recording has 411 frames where the value cases have 37 at the most, and the bound is stated for the last
inverse transform's input: as in test_gpu_mwf.py a spectrogram within e of another's gives samples within
    G * e,   G = max_n sum_m w[n - m hop] / sum_m w[n - m hop]^2   (periodic Hann, 1022 / 256: G = 1.34, computed below),
so the waveforms get BOUND * G * max|ref|; the clamp to [-1, 1] moves nothing further apart."""
import argparse
import math

import numpy as np
import pytest
import torch

import avsep_amd as P
from avsep_amd import separate as S

import misi_ref as M
from recipes import istft_gain as _istft_gain, small_nets as _small_nets, tones as _tones

pytestmark = pytest.mark.gpu

K = P.kernels


def _plan(dev, n_fft, hop, reflect=True, cache={}):
    key = (str(dev), n_fft, hop, reflect)
    if key not in cache:
        cache[key] = K.Stft(dev, n_fft, hop, "reflect" if reflect else "constant")
    return cache[key]


# ---------------------------------------------------------------------------------------------------------------------
# values against float64
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft,hop,F,N,G,it,per_source,reflect", M.VALUE_CASES)
def test_misi_values(dev, n_fft, hop, F, N, G, it, per_source, reflect):
    mix, A, ph = M.value_inputs(n_fft, hop, F, N, G, per_source, reflect)
    ref = M.misi(mix, A, ph, it, n_fft, hop, reflect)
    plan = _plan(dev, n_fft, hop, reflect)
    wav, pout = plan.misi(mix.to(dev), A.to(dev), ph.to(dev), it, want_phase=True)
    assert wav.shape == (N, G, hop * (F - 1)) and pout.shape == A.shape and wav.dtype == pout.dtype == torch.float32
    assert bool(torch.isfinite(wav).all()) and bool(torch.isfinite(pout).all())
    e_w = M.rel_err(wav.cpu(), ref["wav"])
    e_y = M.rel_err(M.polar(A, pout.cpu()), ref["Y"])
    print(f"{n_fft}/{hop}/{F} N={N} G={G} K={it} per_source={per_source} reflect={reflect}: wav {e_w:.3e}, "
          f"A e^(i phase) {e_y:.3e} (bound {M.BOUND:.3e})")
    assert e_w <= M.BOUND and e_y <= M.BOUND
    # without the phase output: the same waveform; a second call: the same bits (no atomics, fixed summation order)
    assert torch.equal(plan.misi(mix.to(dev), A.to(dev), ph.to(dev), it), wav)
    wav2, pout2 = plan.misi(mix.to(dev), A.to(dev), ph.to(dev), it, want_phase=True)
    assert torch.equal(wav2, wav) and torch.equal(pout2, pout)


def test_misi_values_at_2048_512(dev):
    """2048/512, 33 frames: every pass's forward transform goes through stft_pad_t_kernel with 32 * 513 * 4 = 65 664 bytes of
    dynamic LDS, above 64 KB and without the hipFuncSetAttribute opt-in (tests/stft_cases.py row F4 is the same launch
    through avsep_stft_mag).  Not one of misi_ref.VALUE_CASES, which size the bound: the float32 mode of the
    restatement sits 5.4e-07 (waveforms) and 5.1e-06 (A e^{i phase}) from the float64 mode on this case, inside
    misi_ref.F32_WORST = 9.2e-06."""
    test_misi_values(dev, 2048, 512, 33, 2, 1, 2, True, True)


# ---------------------------------------------------------------------------------------------------------------------
# against the existing entry points, no restatement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft,hop,F", [(1022, 256, 37), (64, 32, 21)])
def test_one_source_one_pass_is_the_mixtures_phase(dev, n_fft, hop, F):
    """N = 1: the whole error goes back to the one stem, so a pass is plan.istft(A, phase of plan.stft(x))."""
    mix, A, ph = M.value_inputs(n_fft, hop, F, 1, 1, True, True)
    plan = _plan(dev, n_fft, hop)
    mix, A, ph = mix.to(dev), A.to(dev), ph.to(dev)
    got = plan.misi(mix, A, ph, 1)[0]
    want = plan.istft(A[0], plan.stft(mix)[1])
    e = M.rel_err(got.cpu(), want.cpu())
    print(f"{n_fft}/{hop}/{F}: {e:.3e}")
    assert e <= M.BOUND and want.abs().max().item() > 0.05


@pytest.mark.parametrize("n_fft,hop,F", [(1022, 256, 37), (64, 32, 21)])
def test_consistent_input_is_a_fixed_point(dev, n_fft, hop, F):
    """A_n = |STFT(s_n)|, phi0 = angle STFT(s_n), x = sum_n s_n: three passes give the sources back."""
    g = torch.Generator().manual_seed(F)
    src = (0.1 * torch.randn(3, hop * (F - 1), generator=g)).to(dev)
    plan = _plan(dev, n_fft, hop)
    mag, ph = plan.stft(src)
    got = plan.misi(src.sum(0, keepdim=True), mag[:, None].contiguous(), ph[:, None].contiguous(), 3)[:, 0]
    e = M.rel_err(got.cpu(), src.cpu())
    print(f"{n_fft}/{hop}/{F}: {e:.3e}")
    assert e <= M.BOUND


@pytest.mark.parametrize("n_fft,hop,F,per_source", [(1022, 256, 37, False), (1022, 256, 9, True), (30, 8, 37, True)])
def test_two_groups_are_their_two_calls_bit_for_bit(dev, n_fft, hop, F, per_source):
    mix, A, ph = (t.to(dev) for t in M.value_inputs(n_fft, hop, F, 3, 2, per_source, True))
    plan = _plan(dev, n_fft, hop)
    wav, pout = plan.misi(mix, A, ph, 2, want_phase=True)
    for g in range(2):
        ph_g = ph[:, g:g + 1] if per_source else ph[g:g + 1]
        w1, p1 = plan.misi(mix[g:g + 1], A[:, g:g + 1].contiguous(), ph_g.contiguous(), 2, want_phase=True)
        assert torch.equal(w1[:, 0], wav[:, g]) and torch.equal(p1[:, 0], pout[:, g])
    assert not torch.equal(wav[:, 0], wav[:, 1])


@pytest.mark.parametrize("n_fft,hop,F", [(1022, 256, 37), (64, 32, 21)])
def test_silence_stays_silent(dev, n_fft, hop, F):
    """A source with A_n = 0 comes out exactly zero whatever the others do; zero magnitudes under an all-zero mixture give
    zeros, not NaN (every |Z| is 0 there)."""
    mix, A, ph = (t.to(dev) for t in M.value_inputs(n_fft, hop, F, 3, 1, False, True))
    plan = _plan(dev, n_fft, hop)
    A[1] = 0
    wav = plan.misi(mix, A, ph, 2)
    assert bool((wav[1] == 0).all()) and wav[0].abs().max().item() > 0.01 and bool(torch.isfinite(wav).all())
    wav, pout = plan.misi(torch.zeros_like(mix), torch.zeros_like(A), ph, 2, want_phase=True)
    assert bool((wav == 0).all()) and bool((pout == 0).all())


def test_misi_refuses_what_it_is_not_given_right(dev):
    plan = _plan(dev, 64, 32)
    mix, A, ph = (t.to(dev) for t in M.value_inputs(64, 32, 21, 2, 1, False, True))
    for bad, what in (((mix[:, :-1], A, ph, 1), "mix"), ((mix, A[:, :, :-1], ph, 1), "mag"), ((mix, A, ph[:, :, :-1], 1), "phase"),
                      ((mix, A.double(), ph, 1), "mag"), ((mix, A, ph, 0), "iterations"), ((mix, A, ph, True), "iterations"),
                      ((mix, A[:1].expand(9, -1, -1, -1), ph, 1), "N"), ((mix, A[:, :, :, :2], ph[:, :, :2], 1), "n_fft")):
        with pytest.raises(P.lib.AvsepError) as e:
            plan.misi(*bad)
        assert what in str(e.value), (what, str(e.value))


# ---------------------------------------------------------------------------------------------------------------------
# the point of it
# ---------------------------------------------------------------------------------------------------------------------
def test_sdr_of_the_scene_is_the_restatements(dev):
    """misi_ref.sdr_scene through the kernels: the mean SDR at K = 0 (the plain inverse), 1 and 4 is the float64
    restatement's (which test_misi_host.py holds to a strict rise and >= 2 dB at K = 4) within 0.02 dB."""
    sc = M.sdr_scene()
    plan = _plan(dev, M.SCENE_N_FFT, M.SCENE_HOP)
    mix, A, ph = sc["mix"].to(dev), sc["A"].to(dev), sc["phase"].to(dev)
    got = {0: M.mean_sdr(plan.istft(A[:, 0].contiguous(), ph.expand(2, -1, -1).contiguous()).cpu(), sc["src"])}
    for k in (1, 4):
        got[k] = M.mean_sdr(plan.misi(mix, A, ph, k).cpu(), sc["src"])
    want = {k: M.scene_sdr(sc, k) for k in (0, 1, 4)}
    print("mean SDR, device / float64: " + ", ".join(f"K={k} {got[k]:.3f} / {want[k]:.3f} dB" for k in (0, 1, 4)))
    assert all(abs(got[k] - want[k]) <= 0.02 for k in (0, 1, 4)) and got[0] < got[1] < got[4]


# ---------------------------------------------------------------------------------------------------------------------
# separate_long(phase_iters=...)
# ---------------------------------------------------------------------------------------------------------------------
def _args(**kw):
    a = argparse.Namespace(num_mix=2, log_freq=1, binary_mask=0, mask_thres=0.5, output_activation="sigmoid",
                           img_activation="relu", not_pool_vis=False, fusion_type="hidsep", stft_frame=1022, stft_hop=256,
                           stft_pad_mode="reflect")
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _stereo(Ln, rate=11025):
    """Two instruments at two places: a is mostly left, b mostly right.  -> (down-mix [Ln], channels [2, Ln])."""
    a = _tones(Ln, ((220.0, 0.25, 0.3), (523.25, 0.2, 0.11)), 1, rate)
    b = _tones(Ln, ((1318.5, 0.2, 0.05), (3200.0, 0.1, 0.7)), 2, rate)
    ch = torch.stack([0.9 * a + 0.3 * b, 0.35 * a + 0.8 * b])
    return ch.mean(0), ch


@pytest.fixture(scope="module")
def long_run(dev):
    """A three-window stereo recording (F = 411 frames) through separate_long: without the argument, with phase_iters = 0,
    with 2 passes, and with 2 passes after one pass of the Wiener filter."""
    nets, gen = _small_nets(dev, 3)
    args = _args()
    wav, ch = _stereo(256 * 410 + 17)
    wav, ch = wav.to(dev), ch.to(dev).contiguous()
    frames = [torch.randn(1, 3, 64, 64, generator=gen).to(dev) for _ in range(2)]
    with torch.no_grad():
        base = S.separate_long(nets, wav, frames, args, return_masks=True, channels=ch)
        p0 = S.separate_long(nets, wav, frames, args, return_masks=True, channels=ch, phase_iters=0)
        p2 = S.separate_long(nets, wav, frames, args, return_masks=True, channels=ch, phase_iters=2)
        p2w = S.separate_long(nets, wav, frames, args, return_masks=True, channels=ch, wiener=1, phase_iters=2)
    return {"wav": wav, "ch": ch, "base": base, "p0": p0, "p2": p2, "p2w": p2w, "plan": K.Stft(dev, 1022, 256, "reflect")}


def test_separate_long_phase_iters_0_is_the_call_without_it(long_run):
    base, p0 = long_run["base"], long_run["p0"]
    assert len(base["starts"]) == 3 and p0["starts"] == base["starts"]
    for k in ("wavs", "channel_wavs", "perms", "masks", "lin_masks"):
        assert torch.equal(p0[k], base[k]), k


def _check(got, ref, what):
    G = _istft_gain(1022, 256, 411)
    scale = float(ref.abs().max())
    tol = M.BOUND * G * scale
    err = float((got.double().cpu() - ref.clamp(-1.0, 1.0)).abs().max())
    print(f"{what}: |device - restatement| = {err:.3e}, bound {tol:.3e} (G = {G:.3f}, max|ref| = {scale:.3f})")
    assert 1.3 < G < 1.4 and err <= tol and scale > 0.05


def test_separate_long_wavs_are_the_restatement_on_the_calls_own_magnitudes(long_run):
    base, p2, plan, wav = long_run["base"], long_run["p2"], long_run["plan"], long_run["wav"]
    for k in ("perms", "masks", "lin_masks"):
        assert torch.equal(p2[k], base[k]), k
    mag, phase = plan.stft(wav[None])
    assert mag.shape == (1, 512, 411) and p2["wavs"].shape == (2, 256 * 410)
    A = (p2["lin_masks"] * mag)[:, None]                                                # what the soft stitch stores
    ref = M.misi(wav[None, :256 * 410].cpu(), A.cpu(), phase.cpu(), 2, 1022, 256)["wav"][:, 0]
    _check(p2["wavs"], ref, "wavs, 2 passes")
    # the argument is not ignored: two passes move the stems by far more than the bound
    moved = float((p2["wavs"] - base["wavs"]).abs().max())
    print(f"2 passes move the stems by {moved:.3e}")
    assert moved > 10 * M.BOUND * float(ref.abs().max())


def test_separate_long_channel_wavs_are_the_restatement(long_run):
    p2, p2w, plan, ch = long_run["p2"], long_run["p2w"], long_run["plan"], long_run["ch"]
    mag_c, phase_c = plan.stft(ch)
    ymag = (p2["lin_masks"][:, None] * mag_c[None]).contiguous()
    x = ch[:, :256 * 410].cpu()
    ref = M.misi(x, ymag.cpu(), phase_c.cpu(), 2, 1022, 256)["wav"]
    assert p2["channel_wavs"].shape == (2, 2, 256 * 410)
    _check(p2["channel_wavs"], ref, "channel_wavs, 2 passes")
    assert not torch.equal(p2["channel_wavs"], long_run["base"]["channel_wavs"])
    # after the Wiener filter: its magnitudes and its per-source phases are the start
    assert torch.equal(p2w["wavs"], p2["wavs"])
    wmag, wph = K.mwf(mag_c, phase_c, ymag, phase_c, iterations=1)
    ref = M.misi(x, wmag.cpu(), wph.cpu(), 2, 1022, 256)["wav"]
    _check(p2w["channel_wavs"], ref, "channel_wavs, Wiener x1 then 2 passes")
    assert not torch.equal(p2w["channel_wavs"], p2["channel_wavs"])


# ---------------------------------------------------------------------------------------------------------------------
# command line
# ---------------------------------------------------------------------------------------------------------------------
def test_cli_phase_iters_on_a_48k_stereo_file(dev, tmp_path, capsys):
    """--channels keep --wiener 1 --phase_iters 2 on a 3 s stereo file at 48 kHz: stereo stems at the file's rate, as long as
    the stems of the recording are (hop * (F - 1) samples at the model's rate, converted back), and the last line says so."""
    mb = P.ModelBuilder()
    torch.manual_seed(11)
    snd = mb.build_sound(arch="unet5", fc_dim=2, fusion_type="hidsep", att_type="sig")
    frm = mb.build_frame(arch="resnet18dilated", fc_dim=256, pool_type="maxpool")
    torch.save(snd.state_dict(), str(tmp_path / "sound.pth"))
    torch.save(frm.state_dict(), str(tmp_path / "frame.pth"))
    _, ch = _stereo(3 * 48000, 48000)
    pcm = np.clip(np.rint(ch.t().numpy().astype(np.float64) * 32768.0), -32768, 32767).astype(np.int16)
    S.write_wav_pcm_channels(str(tmp_path / "mix.wav"), pcm, 48000)
    rng = np.random.default_rng(3)
    ones = []
    for n in range(2):
        np.save(str(tmp_path / f"one{n}.npy"), rng.standard_normal((3, 64, 64)).astype(np.float32))
        ones.append(str(tmp_path / f"one{n}.npy"))
    argv = ["--wav", str(tmp_path / "mix.wav"), "--frames", *ones, "--channels", "keep", "--arch_sound", "unet5", "--num_channels", "2",
            "--vis_channels", "256", "--img_pool", "maxpool", "--not_pool_vis", "--fusion_type", "hidsep", "--att_type", "sig",
            "--weights_sound", str(tmp_path / "sound.pth"), "--weights_frame", str(tmp_path / "frame.pth"), "--binary_mask", "0"]
    S.cli(argv + ["--out", str(tmp_path / "out"), "--wiener", "1", "--phase_iters", "2"])
    said = capsys.readouterr().out
    assert "2 channels" in said and "Wiener filter x1" in said and "phase iterations x2" in said
    frames = 33075 // 256 + 1                                    # 144 000 samples at 48 kHz are 33 075 at 11 025 Hz
    want_len = math.ceil(256 * (frames - 1) * 640 / 147)
    for n in range(2):
        got, rate = S.read_wav_pcm(str(tmp_path / "out" / f"source{n}.wav"))
        assert rate == 48000 and got.shape == (want_len, 2)
        assert np.abs(got).max() > 300 and np.abs(got[:, 0].astype(np.int32) - got[:, 1]).max() > 30
