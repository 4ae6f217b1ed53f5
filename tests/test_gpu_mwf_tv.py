"""gpu: the Wiener filter's time-varying covariances (avsep_mwf_cov_tv / avsep_mwf_apply_tv in csrc/mwf.hip,
kernels.mwf_cov(span=H) / kernels.mwf(span=H), separate_long(wiener_span=H)) against the float64 restatement
tests/mwf_tv_ref.py fed the same fp32 inputs.  Results are compared as complex numbers, never as phases, with
max|d| / max|ref| per case, as in test_gpu_mwf.py.

The tolerance is derived as there.  The restatement's float32 mode (weights, sums, LAPACK solve and polar conversions in
single precision) was run on the CPU over exactly the value cases below (mwf_tv_ref.VALUE_CASES, Fin = 5;
test_mwf_tv_host.py re-measures it): its worst distance from the float64 mode is 4.703e-07 for the filtered images and
8.474e-07 for the covariances (both at C = 8, N = 3, F = 4173, H = 192).  Recorded rounded up as F32_WORST_Y = 4.8e-07 and
F32_WORST_COV = 8.5e-07, the kernels get 16 x:
    BOUND_Y = 7.68e-06,   BOUND_COV = 1.36e-05.
The factor covers another summation order over t, sincosf / atan2f on both sides and a Cholesky where LAPACK pivots.

separate_long: the bound of test_gpu_mwf.py's header, BOUND_Y x iSTFT gain G x max|Y_ref|, with this file's BOUND_Y."""
import numpy as np
import pytest
import torch

import avsep_amd as P
from avsep_amd import separate as S
from avsep_amd.lib import AvsepError

import mwf_ref as M
import mwf_tv_ref as T
from recipes import args as _args, file_bytes as _bytes, istft_gain as _istft_gain, small_nets as _small_nets
from test_gpu_mwf import _complex, _cov_np, _dev, _stereo

pytestmark = pytest.mark.gpu

K = P.kernels


# ---------------------------------------------------------------------------------------------------------------------
# values
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,N,F,H,it", T.VALUE_CASES)
def test_mwf_tv_values(dev, C, N, F, H, it):
    xmag, xph, ymag = T.value_inputs(C, N, F)
    ref = T.mwf(xmag, xph, ymag, xph, H, it)
    xm, xp, ym = _dev(xmag, dev), _dev(xph, dev), _dev(ymag, dev)
    cov = K.mwf_cov(ym, xp, span=H)
    assert cov.dtype == torch.complex64 and cov.shape == (N, T.centres(F, H), T.FIN, C, C)
    e_cov = M.rel_err(_cov_np(cov), ref["cov"])
    mag, ph = K.mwf(xm, xp, ym, xp, iterations=it, span=H)
    assert mag.shape == ph.shape == (N, C, T.FIN, F) and mag.dtype == ph.dtype == torch.float32
    assert bool(torch.isfinite(mag).all()) and bool(torch.isfinite(ph).all()) and bool((mag >= 0).all())
    e_y = M.rel_err(_complex(mag, ph), ref["Y"])
    print(f"C={C} N={N} F={F} H={H} passes={it}: cov {e_cov:.3e} (bound {T.BOUND_COV:.2e}), images {e_y:.3e} (bound {T.BOUND_Y:.2e})")
    assert e_cov <= T.BOUND_COV and e_y <= T.BOUND_Y
    # Hermitian by construction: real diagonal, upper triangle the conjugate of the lower, bit for bit
    c = torch.view_as_real(cov)
    assert bool((torch.diagonal(c[..., 1], dim1=-2, dim2=-1) == 0).all())
    assert torch.equal(c[..., 0], c[..., 0].transpose(-1, -2)) and bool((c[..., 1] == -c[..., 1].transpose(-1, -2)).all())
    # a second call: the same bits (no atomics, fixed summation order)
    mag2, ph2 = K.mwf(xm, xp, ym, xp, iterations=it, span=H)
    assert torch.equal(mag, mag2) and torch.equal(ph, ph2) and torch.equal(torch.view_as_real(K.mwf_cov(ym, xp, span=H)), c)


def test_mwf_tv_cov_with_a_phase_per_source(dev):
    """What the second pass reads: [N,C,Fin,F] phases."""
    xmag, xph, ymag = T.value_inputs(3, 2, 257)
    yph = np.random.default_rng(257).uniform(-np.pi, np.pi, ymag.shape).astype(np.float32)
    ref = T.mwf(xmag, xph, ymag, yph, 128, 1)
    cov = K.mwf_cov(_dev(ymag, dev), _dev(yph, dev), span=128)
    assert M.rel_err(_cov_np(cov), ref["cov"]) <= T.BOUND_COV
    assert M.rel_err(T.cov(ymag, xph, 128)[0], ref["cov"]) > 100 * T.BOUND_COV           # the phases matter
    mag, ph = K.mwf(_dev(xmag, dev), _dev(xph, dev), _dev(ymag, dev), _dev(yph, dev), span=128)
    assert M.rel_err(_complex(mag, ph), ref["Y"]) <= T.BOUND_Y


def test_mwf_span_zero_is_the_invariant_filter_and_bad_spans_are_refused(dev):
    xmag, xph, ymag = T.value_inputs(2, 2, 65)
    xm, xp, ym = _dev(xmag, dev), _dev(xph, dev), _dev(ymag, dev)
    a, b = K.mwf(xm, xp, ym, xp, iterations=2), K.mwf(xm, xp, ym, xp, iterations=2, span=0)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(torch.view_as_real(K.mwf_cov(ym, xp)), torch.view_as_real(K.mwf_cov(ym, xp, span=0)))
    assert not torch.equal(a[0], K.mwf(xm, xp, ym, xp, iterations=2, span=64)[0])
    for bad in (63, 96, 4160, -64, 64.0, True, None):
        with pytest.raises(AvsepError) as e:
            K.mwf(xm, xp, ym, xp, span=bad)
        assert "multiple of 64" in str(e.value)
        with pytest.raises(AvsepError):
            K.mwf_cov(ym, xp, span=bad)


@pytest.mark.parametrize("C,N,F,H", T.TIE_SHAPES)
def test_apply_tv_with_one_covariance_at_every_centre_is_the_invariant_apply(dev, C, N, F, H):
    """The two apply kernels are one template (mwf_apply_kernel<C, TV>) and differ in where an entry of R_n comes from.  With the time-invariant
    covariance repeated at all K centres the blend w R + u R is R up to rounding, so avsep_mwf_apply_tv must give what
    avsep_mwf_apply gives on the same inputs, the whole output, within BOUND_Y (the float32 restatements do:
    test_mwf_tv_host.py).  Not bit-equal, not even where u == 0: the two instantiations may fuse differently."""
    xmag, xph, ymag = T.value_inputs(C, N, F)
    xm, xp, ym = _dev(xmag, dev), _dev(xph, dev), _dev(ymag, dev)
    cov = K._mwf_cov(ym, xp, 0)                                                          # f32 [N, Fin, C, C, 2]
    rep = cov[:, None].expand(N, T.centres(F, H), T.FIN, C, C, 2).contiguous()
    ref = _complex(*K._mwf_apply(xm, xp, ym, cov, 0, M.REG))
    got = _complex(*K._mwf_apply(xm, xp, ym, rep, H, M.REG))
    err = M.rel_err(got, ref)
    print(f"C={C} N={N} F={F} H={H}: apply_tv against apply {err:.3e} (bound {T.BOUND_Y:.2e})")
    assert got.shape == (N, C, T.FIN, F) and np.abs(ref).max() > 10.0
    assert err <= T.BOUND_Y


# ---------------------------------------------------------------------------------------------------------------------
# exactness
# ---------------------------------------------------------------------------------------------------------------------
def _degenerate(kind):
    xmag, xph, ymag = T.value_inputs(2, 2, 257, seed=77)
    if kind == "dual_mono":
        xmag[1], xph[1], ymag[:, 1] = xmag[0], xph[0], ymag[:, 0]
    elif kind == "silent_channel":
        xmag[1], ymag[:, 1] = 0, 0
    elif kind == "silent_support":
        ymag[1, :, :, 64:192] = 0              # H = 64: the support of centre 2 is frames 65 ... 191; centres 1 and 3 keep some
    return xmag, xph, ymag


@pytest.mark.parametrize("it", [1, 2])
@pytest.mark.parametrize("kind", ["dual_mono", "silent_channel", "silent_support"])
def test_mwf_tv_degenerate_inputs(dev, kind, it):
    xmag, xph, ymag = _degenerate(kind)
    ref = T.mwf(xmag, xph, ymag, xph, 64, it)
    mag, ph = K.mwf(_dev(xmag, dev), _dev(xph, dev), _dev(ymag, dev), _dev(xph, dev), iterations=it, span=64)
    cov = K.mwf_cov(_dev(ymag, dev), _dev(xph, dev), span=64)
    assert bool(torch.isfinite(mag).all()) and bool(torch.isfinite(ph).all()) and bool(torch.isfinite(torch.view_as_real(cov)).all())
    e_y, e_cov = M.rel_err(_complex(mag, ph), ref["Y"]), M.rel_err(_cov_np(cov), ref["cov"])
    print(f"{kind} passes={it}: cov {e_cov:.3e}, images {e_y:.3e}")
    assert e_y <= T.BOUND_Y and e_cov <= T.BOUND_COV
    assert mag.abs().max().item() > 1.0                                                 # not a silent agreement
    c = torch.view_as_real(cov)                                                         # [N, K, Fin, C, C, 2]
    if kind == "dual_mono":
        assert torch.equal(mag[:, 0], mag[:, 1]) and torch.equal(ph[:, 0], ph[:, 1])
    elif kind == "silent_channel":
        assert bool((mag[:, 1] == 0).all()) and bool((ph[:, 1] == 0).all())
        assert bool((c[:, :, :, 1] == 0).all()) and bool((c[:, :, :, :, 1] == 0).all())
    elif kind == "silent_support":
        assert bool((c[1, 2] == 0).all()) and bool((c[1, 1, ..., 0].abs().amax((-1, -2)) > 0).all())
        assert bool((c[1, 3, ..., 0].abs().amax((-1, -2)) > 0).all())
        assert bool((mag[1, :, :, 64:192] == 0).all()) and bool((ph[1, :, :, 64:192] == 0).all())
        assert mag[1, :, :, :64].abs().max().item() > 1.0 and mag[0, :, :, 64:192].abs().max().item() > 1.0


# ---------------------------------------------------------------------------------------------------------------------
# the point of it
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("it", [1, 2])
def test_mwf_tv_follows_moving_sources_as_the_restatement_does(dev, it):
    """mwf_tv_ref.moving_sources(2, 2, 48, 640, 0, 90) through the kernels at H = 64: the device's mean SDR is the
    restatement's (which test_mwf_tv_host.py holds 2 / 3 dB above the time-invariant filter's) within 0.01 dB."""
    sc = T.moving_sources(2, 2, 48, 640, 0, 90)
    want = M.mean_sdr(T.mwf(sc["xmag"], sc["xph"], sc["ymag"], sc["xph"], 64, it)["Y"], sc["images"])
    mag, ph = K.mwf(_dev(sc["xmag"], dev), _dev(sc["xph"], dev), _dev(sc["ymag"], dev), _dev(sc["xph"], dev), iterations=it, span=64)
    got = M.mean_sdr(_complex(mag, ph), sc["images"])
    print(f"moving sources, {it} pass(es), H = 64: {got:.4f} dB on the device, {want:.4f} dB in float64")
    assert abs(got - want) <= 0.01


# ---------------------------------------------------------------------------------------------------------------------
# separate_long(wiener_span=...)
# ---------------------------------------------------------------------------------------------------------------------
def test_separate_long_with_wiener_span(dev):
    """The three-window stereo recording of test_gpu_mwf.py (F = 411 frames): wiener_span=0 is the call without the
    argument, the mono outputs and masks do not move, wiener_span=64 is the restatement on the run's own soft masks, and
    the span composes with phase_iters."""
    nets, gen = _small_nets(dev, 3)
    args = _args(binary_mask=1)
    Ln = 256 * 410 + 17
    wav, ch = _stereo(Ln)
    wav, ch = wav.to(dev), ch.to(dev).contiguous()
    frames = [torch.randn(1, 3, 64, 64, generator=gen).to(dev) for _ in range(2)]
    with torch.no_grad():
        base = S.separate_long(nets, wav, frames, args, return_masks=True, channels=ch, wiener=1)
        s0 = S.separate_long(nets, wav, frames, args, channels=ch, wiener=1, wiener_span=0)
        tv = S.separate_long(nets, wav, frames, args, return_masks=True, channels=ch, wiener=1, wiener_span=64)
        both = S.separate_long(nets, wav, frames, args, channels=ch, wiener=1, wiener_span=64, phase_iters=1)
        assert len(base["starts"]) == 3
        assert torch.equal(s0["channel_wavs"], base["channel_wavs"]) and torch.equal(s0["wavs"], base["wavs"])
        assert torch.equal(tv["wavs"], base["wavs"]) and torch.equal(tv["perms"], base["perms"]) and tv["starts"] == base["starts"]
        assert torch.equal(tv["masks"], base["masks"]) and torch.equal(tv["lin_masks"], base["lin_masks"])
        assert not torch.equal(tv["channel_wavs"], base["channel_wavs"])
        assert both["channel_wavs"].shape == tv["channel_wavs"].shape and bool(torch.isfinite(both["channel_wavs"]).all())
        plan = K.Stft(dev, 1022, 256, "reflect")
        mag_c, phase_c = plan.stft(ch)
        Fr = mag_c.shape[2]
        assert Fr == 411 and tv["lin_masks"].shape == (2, 512, Fr)
        ymag = (tv["lin_masks"][:, None] * mag_c[None]).contiguous()                     # what the soft channel stitch stores
        ref = T.mwf(mag_c.cpu().numpy(), phase_c.cpu().numpy(), ymag.cpu().numpy(), phase_c.cpu().numpy(), 64, 1)
        hand = plan.istft(_dev(ref["mag"].astype(np.float32), dev).reshape(4, 512, Fr),
                          _dev(ref["phase"].astype(np.float32), dev).reshape(4, 512, Fr))
        hand = hand.clamp_(-1.0, 1.0).reshape(2, 2, -1)
    cw = tv["channel_wavs"]
    G = _istft_gain(1022, 256, Fr)
    tol = T.BOUND_Y * G * float(np.abs(ref["Y"]).max())
    err = (cw - hand).abs().max().item()
    print(f"wiener_span=64: |channel_wavs - iSTFT of the restatement| = {err:.3e}, bound {tol:.3e} (G = {G:.3f}, max|Y| = "
          f"{np.abs(ref['Y']).max():.2f}), peak {cw.abs().max().item():.3f}")
    assert cw.shape == (2, 2, 256 * (Fr - 1)) and 1.3 < G < 1.4
    assert err <= tol and cw.abs().max().item() > 0.05


# ---------------------------------------------------------------------------------------------------------------------
# command line
# ---------------------------------------------------------------------------------------------------------------------
def test_cli_wiener_span(dev, tmp_path, capsys):
    """The stereo 16-bit file of test_gpu_mwf.py's command-line test: --wiener_span 0 writes the bytes --wiener 1 writes,
    --wiener_span 64 stereo files of the same length that differ from them, and the closing line names the span."""
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
            "--weights_sound", str(tmp_path / "sound.pth"), "--weights_frame", str(tmp_path / "frame.pth"), "--binary_mask", "0",
            "--wiener", "1"]
    S.cli(argv + ["--out", str(tmp_path / "w1")])
    assert "local covariances" not in capsys.readouterr().out
    S.cli(argv + ["--out", str(tmp_path / "s0"), "--wiener_span", "0"])
    assert "local covariances" not in capsys.readouterr().out
    S.cli(argv + ["--out", str(tmp_path / "s64"), "--wiener_span", "64"])
    said = capsys.readouterr().out
    assert "Wiener filter x1 with local covariances every 64 frames (1.49 s)" in said             # 64 * 256 / 11025
    for n in range(2):
        w1, s0 = _bytes(tmp_path / "w1" / f"source{n}.wav"), _bytes(tmp_path / "s0" / f"source{n}.wav")
        assert len(w1) > 44 + 4 * 30000 and w1 == s0
        a, ra = S.read_wav_pcm(str(tmp_path / "w1" / f"source{n}.wav"))
        b, rb = S.read_wav_pcm(str(tmp_path / "s64" / f"source{n}.wav"))
        assert ra == rb == 11025 and a.shape == b.shape and b.shape[1] == 2
        assert not np.array_equal(a, b) and np.abs(b).max() > 300
