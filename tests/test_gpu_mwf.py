"""gpu: the multichannel Wiener filter (avsep_mwf_cov / avsep_mwf_apply in csrc/mwf.hip, kernels.mwf_cov / kernels.mwf,
separate_long(wiener=...) and --wiener of avsep_amd/separate.py) against the float64 restatement tests/mwf_ref.py fed the
same fp32 inputs.  Results are compared as complex numbers, never as phases (the phase of a near-zero value is arbitrary),
with max|d| / max|ref| per case.

The tolerance is derived, not chosen.  The restatement's float32 mode (complex64 einsum and LAPACK solve, polar <-> Cartesian
conversions included) was run on the CPU over exactly the value cases below (mwf_ref.VALUE_CASES, Fin = 5; test_mwf_host.py
re-measures it): its worst distance from the float64 mode is 1.897e-06 for the filtered images (C = 2, N = 2, F = 4173, two
passes) and 2.462e-06 for the covariances (the same shape: numpy's sequential float32 sum over 4173 frames).  Recorded
rounded up as mwf_ref.F32_WORST_Y = 1.9e-06 and F32_WORST_COV = 2.5e-06, the kernels get 16 x:
    BOUND_Y = 3.04e-05,   BOUND_COV = 4.0e-05.
The factor covers another summation order over t, sincosf / atan2f on both sides and a Cholesky where LAPACK pivots.

separate_long: channel_wavs is an iSTFT of the filtered images, the reference is the same iSTFT (plan.istft) of the
restatement's images cast to fp32.  The iSTFT is linear: a spectrogram whose bins are all within e of another's gives frames
within e of the other's (irfft: |x[n]| <= (1/n_fft) * sum of the n_fft coefficient magnitudes <= e), and the overlap-add
divides the windowed sum by the window-sum-square, so a sample moves by at most
    G * e,   G = max_n sum_m w[n - m hop] / sum_m w[n - m hop]^2   (periodic Hann, 1022 / 256: G = 1.34, computed below),
and the clamp to [-1, 1] moves nothing further apart.  With e = BOUND_Y * max|Y_ref| that is the bound used; the iSTFT
kernel's own rounding is common to both sides up to a term four orders below it."""
import numpy as np
import pytest
import torch

import avsep_amd as P
from avsep_amd import separate as S

import mwf_ref as M
from recipes import (args as _args, file_bytes as _bytes, istft_gain as _istft_gain, small_nets as _small_nets,
                     tones as _tones)

pytestmark = pytest.mark.gpu

K = P.kernels


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _complex(mag, ph):
    """fp32 magnitude and phase off the device -> complex128, the conversion done in float64."""
    return M.polar_to_complex(mag.cpu().numpy(), ph.cpu().numpy(), np.float64)


def _cov_np(cov):
    return cov.cpu().numpy().astype(np.complex128)


# ---------------------------------------------------------------------------------------------------------------------
# values
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,N,F,it", M.VALUE_CASES)
def test_mwf_values(dev, C, N, F, it):
    xmag, xph, ymag = M.value_inputs(C, N, F)
    ref = M.mwf(xmag, xph, ymag, xph, it)
    xm, xp, ym = _dev(xmag, dev), _dev(xph, dev), _dev(ymag, dev)
    cov = K.mwf_cov(ym, xp)
    assert cov.dtype == torch.complex64 and cov.shape == (N, M.FIN, C, C)
    e_cov = M.rel_err(_cov_np(cov), ref["cov"])
    mag, ph = K.mwf(xm, xp, ym, xp, iterations=it)
    assert mag.shape == ph.shape == (N, C, M.FIN, F) and mag.dtype == ph.dtype == torch.float32
    assert bool(torch.isfinite(mag).all()) and bool(torch.isfinite(ph).all()) and bool((mag >= 0).all())
    e_y = M.rel_err(_complex(mag, ph), ref["Y"])
    print(f"C={C} N={N} F={F} passes={it}: cov {e_cov:.3e} (bound {M.BOUND_COV:.2e}), images {e_y:.3e} (bound {M.BOUND_Y:.2e})")
    assert e_cov <= M.BOUND_COV and e_y <= M.BOUND_Y
    # Hermitian by construction: real diagonal, upper triangle the conjugate of the lower, bit for bit
    c = torch.view_as_real(cov)
    assert bool((torch.diagonal(c[..., 1], dim1=-2, dim2=-1) == 0).all())
    assert torch.equal(c[..., 0], c[..., 0].transpose(-1, -2)) and bool((c[..., 1] == -c[..., 1].transpose(-1, -2)).all())
    # a second call: the same bits (no atomics, fixed summation order)
    mag2, ph2 = K.mwf(xm, xp, ym, xp, iterations=it)
    assert torch.equal(mag, mag2) and torch.equal(ph, ph2) and torch.equal(torch.view_as_real(K.mwf_cov(ym, xp)), c)


@pytest.mark.parametrize("C,N,F", [(3, 2, 63), (2, 3, M.F_LONG)])
def test_mwf_cov_with_a_phase_per_source(dev, C, N, F):
    """What the second pass reads: [N,C,Fin,F] phases; and mwf with such a phase from the start."""
    xmag, xph, ymag = M.value_inputs(C, N, F)
    yph = np.random.default_rng(F).uniform(-np.pi, np.pi, ymag.shape).astype(np.float32)
    ref = M.mwf(xmag, xph, ymag, yph, 1)
    cov = K.mwf_cov(_dev(ymag, dev), _dev(yph, dev))
    assert M.rel_err(_cov_np(cov), ref["cov"]) <= M.BOUND_COV
    assert M.rel_err(M.cov(ymag, xph)[0], ref["cov"]) > 100 * M.BOUND_COV               # the phases matter
    mag, ph = K.mwf(_dev(xmag, dev), _dev(xph, dev), _dev(ymag, dev), _dev(yph, dev))
    assert M.rel_err(_complex(mag, ph), ref["Y"]) <= M.BOUND_Y


# ---------------------------------------------------------------------------------------------------------------------
# degenerate inputs
# ---------------------------------------------------------------------------------------------------------------------
def _degenerate(kind):
    xmag, xph, ymag = M.value_inputs(2, 2, 63, seed=77)
    if kind == "dual_mono":
        xmag[1], xph[1], ymag[:, 1] = xmag[0], xph[0], ymag[:, 0]
    elif kind == "silent_channel":
        xmag[1], ymag[:, 1] = 0, 0
    elif kind == "zero_row":
        xmag[:, 2], ymag[:, :, 2] = 0, 0
    elif kind == "zero_mask":
        ymag[1] = 0
    return xmag, xph, ymag


@pytest.mark.parametrize("it", [1, 2])
@pytest.mark.parametrize("kind", ["dual_mono", "silent_channel", "zero_row", "zero_mask"])
def test_mwf_degenerate_inputs(dev, kind, it):
    xmag, xph, ymag = _degenerate(kind)
    ref = M.mwf(xmag, xph, ymag, xph, it)
    mag, ph = K.mwf(_dev(xmag, dev), _dev(xph, dev), _dev(ymag, dev), _dev(xph, dev), iterations=it)
    cov = K.mwf_cov(_dev(ymag, dev), _dev(xph, dev))
    assert bool(torch.isfinite(mag).all()) and bool(torch.isfinite(ph).all()) and bool(torch.isfinite(torch.view_as_real(cov)).all())
    e_y, e_cov = M.rel_err(_complex(mag, ph), ref["Y"]), M.rel_err(_cov_np(cov), ref["cov"])
    print(f"{kind} passes={it}: cov {e_cov:.3e}, images {e_y:.3e}")
    assert e_y <= M.BOUND_Y and e_cov <= M.BOUND_COV
    assert mag.abs().max().item() > 1.0                                                 # not a silent agreement
    if kind == "dual_mono":
        assert torch.equal(mag[:, 0], mag[:, 1]) and torch.equal(ph[:, 0], ph[:, 1])
    elif kind == "silent_channel":
        assert bool((mag[:, 1] == 0).all()) and bool((ph[:, 1] == 0).all()) and bool((torch.view_as_real(cov)[:, :, 1] == 0).all())
    elif kind == "zero_row":
        assert bool((mag[:, :, 2] == 0).all()) and bool((ph[:, :, 2] == 0).all()) and bool((torch.view_as_real(cov)[:, 2] == 0).all())
    elif kind == "zero_mask":
        assert bool((mag[1] == 0).all()) and bool((ph[1] == 0).all()) and bool((torch.view_as_real(cov)[1] == 0).all())


def test_mwf_where_every_source_is_silent_but_the_mixture_is_not(dev):
    """v_n = 0 for all n at bins where X is about 30: S = FLT_MIN * I and z overflows in fp32; the output is the exact 0 the
    float64 arithmetic gives, not a NaN."""
    xmag, xph, ymag = M.value_inputs(2, 2, 63, seed=78)
    ymag[:, :, 1, 10:20] = 0
    ref = M.mwf(xmag, xph, ymag, xph, 1)
    mag, ph = K.mwf(_dev(xmag, dev), _dev(xph, dev), _dev(ymag, dev), _dev(xph, dev))
    assert bool(torch.isfinite(mag).all()) and bool(torch.isfinite(ph).all())
    assert bool((mag[:, :, 1, 10:20] == 0).all()) and M.rel_err(_complex(mag, ph), ref["Y"]) <= M.BOUND_Y


# ---------------------------------------------------------------------------------------------------------------------
# the point of it
# ---------------------------------------------------------------------------------------------------------------------
def test_mwf_raises_the_sdr_of_panned_sources_as_the_restatement_does(dev):
    """mwf_ref.panned_sources through the kernels: the gain over per-channel masking is the restatement's (which
    test_mwf_host.py holds to >= 3 dB) within 0.05 dB."""
    sc = M.panned_sources()
    base = M.masking_sdr(sc)
    want = M.mean_sdr(M.mwf(sc["xmag"], sc["xph"], sc["ymag"], sc["xph"], 1)["Y"], sc["images"]) - base
    mag, ph = K.mwf(_dev(sc["xmag"], dev), _dev(sc["xph"], dev), _dev(sc["ymag"], dev), _dev(sc["xph"], dev))
    got = M.mean_sdr(_complex(mag, ph), sc["images"]) - base
    print(f"panned sources: masking {base:.2f} dB; one pass gains {got:.3f} dB on the device, {want:.3f} dB in float64")
    assert abs(got - want) <= 0.05 and got >= 3.0 - 0.05


# ---------------------------------------------------------------------------------------------------------------------
# separate_long(wiener=...)
# ---------------------------------------------------------------------------------------------------------------------
def _stereo(Ln):
    """Two instruments at two places: a is mostly left, b mostly right.  -> (down-mix [Ln], channels [2, Ln])."""
    a = _tones(Ln, ((220.0, 0.25, 0.3), (523.25, 0.2, 0.11)), 1)
    b = _tones(Ln, ((1318.5, 0.2, 0.05), (3200.0, 0.1, 0.7)), 2)
    ch = torch.stack([0.9 * a + 0.3 * b, 0.35 * a + 0.8 * b])
    return ch.mean(0), ch


def test_separate_long_with_wiener(dev):
    """A three-window stereo recording (F = 411 frames): wiener=0 is the call without the argument, the mono outputs do not
    move, wiener=1 is the restatement on the run's own soft masks, and args.binary_mask does not reach the filter."""
    nets, gen = _small_nets(dev, 3)
    args = _args(binary_mask=1)
    Ln = 256 * 410 + 17
    wav, ch = _stereo(Ln)
    wav, ch = wav.to(dev), ch.to(dev).contiguous()
    frames = [torch.randn(1, 3, 64, 64, generator=gen).to(dev) for _ in range(2)]
    with torch.no_grad():
        base = S.separate_long(nets, wav, frames, args, channels=ch)
        w0 = S.separate_long(nets, wav, frames, args, channels=ch, wiener=0)
        w1 = S.separate_long(nets, wav, frames, args, return_masks=True, channels=ch, wiener=1)
        soft = S.separate_long(nets, wav, frames, _args(binary_mask=0), channels=ch, wiener=1)
        assert len(base["starts"]) == 3
        assert torch.equal(w0["channel_wavs"], base["channel_wavs"]) and torch.equal(w0["wavs"], base["wavs"])
        assert torch.equal(w1["wavs"], base["wavs"]) and torch.equal(w1["perms"], base["perms"]) and w1["starts"] == base["starts"]
        assert torch.equal(soft["channel_wavs"], w1["channel_wavs"])                     # binary_mask=1 took the soft mask too
        assert not torch.equal(w1["channel_wavs"], base["channel_wavs"])
        plan = K.Stft(dev, 1022, 256, "reflect")
        mag_c, phase_c = plan.stft(ch)
        Fr = mag_c.shape[2]
        assert Fr == 411 and w1["lin_masks"].shape == (2, 512, Fr)
        ymag = (w1["lin_masks"][:, None] * mag_c[None]).contiguous()                     # what the soft channel stitch stores
        ref = M.mwf(mag_c.cpu().numpy(), phase_c.cpu().numpy(), ymag.cpu().numpy(), phase_c.cpu().numpy(), 1)
        hand = plan.istft(_dev(ref["mag"].astype(np.float32), dev).reshape(4, 512, Fr),
                          _dev(ref["phase"].astype(np.float32), dev).reshape(4, 512, Fr))
        hand = hand.clamp_(-1.0, 1.0).reshape(2, 2, -1)
    cw = w1["channel_wavs"]
    G = _istft_gain(1022, 256, Fr)
    tol = M.BOUND_Y * G * float(np.abs(ref["Y"]).max())
    err = (cw - hand).abs().max().item()
    print(f"wiener=1: |channel_wavs - iSTFT of the restatement| = {err:.3e}, bound {tol:.3e} (G = {G:.3f}, max|Y| = "
          f"{np.abs(ref['Y']).max():.2f}), peak {cw.abs().max().item():.3f}")
    assert cw.shape == (2, 2, 256 * (Fr - 1)) and 1.3 < G < 1.4
    assert err <= tol and cw.abs().max().item() > 0.05


# ---------------------------------------------------------------------------------------------------------------------
# command line
# ---------------------------------------------------------------------------------------------------------------------
def test_cli_wiener(dev, tmp_path, capsys):
    """A stereo 16-bit file at the model's rate: --wiener 0 writes the bytes --channels keep writes, --wiener 1 stereo files
    of the same length that differ from them."""
    mb = P.ModelBuilder()
    torch.manual_seed(11)
    snd = mb.build_sound(arch="unet5", fc_dim=2, fusion_type="hidsep", att_type="sig")
    frm = mb.build_frame(arch="resnet18dilated", fc_dim=256, pool_type="maxpool")
    torch.save(snd.state_dict(), str(tmp_path / "sound.pth"))
    torch.save(frm.state_dict(), str(tmp_path / "frame.pth"))
    _, ch = _stereo(3 * 11025)
    pcm = np.clip(np.rint(ch.t().numpy().astype(np.float64) * 32768.0), -32768, 32767).astype(np.int16)
    S.write_wav_pcm_channels(str(tmp_path / "mix.wav"), pcm, 11025)
    rng = np.random.default_rng(3)
    ones = []
    for n in range(2):
        np.save(str(tmp_path / f"one{n}.npy"), rng.standard_normal((3, 64, 64)).astype(np.float32))
        ones.append(str(tmp_path / f"one{n}.npy"))
    argv = ["--wav", str(tmp_path / "mix.wav"), "--frames", *ones, "--channels", "keep", "--arch_sound", "unet5", "--num_channels", "2",
            "--vis_channels", "256", "--img_pool", "maxpool", "--not_pool_vis", "--fusion_type", "hidsep", "--att_type", "sig",
            "--weights_sound", str(tmp_path / "sound.pth"), "--weights_frame", str(tmp_path / "frame.pth"), "--binary_mask", "0"]
    S.cli(argv + ["--out", str(tmp_path / "keep")])
    assert "Wiener" not in capsys.readouterr().out
    S.cli(argv + ["--out", str(tmp_path / "w0"), "--wiener", "0"])
    assert "Wiener" not in capsys.readouterr().out
    S.cli(argv + ["--out", str(tmp_path / "w1"), "--wiener", "1"])
    said = capsys.readouterr().out
    assert "2 channels" in said and "Wiener filter x1" in said
    for n in range(2):
        keep, w0 = _bytes(tmp_path / "keep" / f"source{n}.wav"), _bytes(tmp_path / "w0" / f"source{n}.wav")
        assert len(keep) > 44 + 4 * 30000 and keep == w0
        a, ra = S.read_wav_pcm(str(tmp_path / "keep" / f"source{n}.wav"))
        b, rb = S.read_wav_pcm(str(tmp_path / "w1" / f"source{n}.wav"))
        assert ra == rb == 11025 and a.shape == b.shape and b.shape[1] == 2
        assert np.abs(a.astype(np.int32) - b).max() > 30 and np.abs(b).max() > 300
