"""not-gpu: the host side of the Wiener filter's time-varying covariances (--wiener_span of separate.py,
separate_long(wiener_span=...), the avsep_mwf_*_tv entry points, which refuse before anything touches a GPU), and checks on
the float64 restatement tests/mwf_tv_ref.py itself, so that the GPU tests do not trust it blindly."""
import ctypes as C

import numpy as np
import pytest
import torch

import avsep_amd
from avsep_amd import separate as S
from avsep_amd.lib import AvsepError

import mwf_ref as M
import mwf_tv_ref as T
from recipes import no_gpu_call as _no_gpu_call

BAD_SPANS = (63, 96, 4160, -64, -1, 32, 1)


# ---------------------------------------------------------------------------------------------------------------------
# flags and refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_cli_wiener_span_flag():
    base = ["--wav", "mix.wav", "--audio_only"]
    assert S.parse_args(base).wiener_span == 0
    assert S.parse_args(base + ["--channels", "keep", "--wiener", "1"]).wiener_span == 0
    for ok in (64, 128, 192, 4096):
        assert S.parse_args(base + ["--channels", "keep", "--wiener", "2", "--wiener_span", str(ok)]).wiener_span == ok
    assert S.parse_args(base + ["--wiener_span", "0"]).wiener_span == 0                         # 0 needs nothing
    with pytest.raises(SystemExit) as e:
        S.parse_args(base + ["--channels", "keep", "--wiener_span", "64"])
    assert "--wiener" in str(e.value)
    with pytest.raises(SystemExit):
        S.parse_args(base + ["--channels", "keep", "--wiener", "0", "--wiener_span", "64"])
    for bad in BAD_SPANS:
        with pytest.raises(SystemExit) as e:
            S.parse_args(base + ["--channels", "keep", "--wiener", "1", "--wiener_span", str(bad)])
        assert "multiple of 64" in str(e.value), bad


def test_separate_long_refuses_bad_spans_before_touching_the_gpu(monkeypatch):
    _no_gpu_call(monkeypatch)
    wav, ch = torch.zeros(4096), torch.zeros(2, 4096)
    for bad in BAD_SPANS + (64.0, "64", True, None):
        with pytest.raises(AvsepError) as e:
            S.separate_long((None, None), wav, [], None, channels=ch, wiener=1, wiener_span=bad)
        assert "multiple of 64" in str(e.value), bad
    with pytest.raises(AvsepError) as e:
        S.separate_long((None, None), wav, [], None, channels=ch, wiener_span=64)
    assert "wiener >= 1" in str(e.value)
    with pytest.raises(AvsepError) as e:
        S.separate_long((None, None), wav, [], None, channels=ch, wiener=0, wiener_span=128)
    assert "wiener >= 1" in str(e.value)
    K = avsep_amd.kernels
    assert (K.MWF_MIN_SPAN, K.MWF_MAX_SPAN) == (T.MIN_SPAN, T.MAX_SPAN) == (64, 4096)
    for bad in BAD_SPANS:
        assert not T.span_ok(bad)
        with pytest.raises(AvsepError):
            K.mwf_span_check("mwf", bad)
    assert K.mwf_span_check("mwf", 0) == 0 and K.mwf_span_check("mwf", 192) == 192 and T.span_ok(192)


def test_mwf_tv_entry_points_refuse_bad_arguments_before_launching():
    """include/avsep.h: an H that is no multiple of 64 or outside 64 ... 4096, C or N outside [1, 8], a workspace that is
    too small and null pointers are argument errors (-1); the workspace query answers 0 for the same arguments."""
    lib = avsep_amd.lib.load()
    buf = (C.c_float * 4096)()
    p = C.addressof(buf)
    wsb, cov, app = lib.avsep_mwf_tv_workspace_bytes, lib.avsep_mwf_cov_tv, lib.avsep_mwf_apply_tv
    need = wsb(2, 2, 5, 63, 64)
    assert need == 1 * 2 * 5 * 2 * (2 * 3 + 1) * 4                            # one segment: 2 sources x 5 rows x 2 slabs x 7 floats
    assert wsb(2, 2, 5, 64, 64) == need and wsb(2, 2, 5, 65, 64) == 2 * need and wsb(2, 2, 5, 65, 128) == need
    assert wsb(3, 8, 5, 257, 192) == 2 * 3 * 5 * 2 * 73 * 4
    for H in (0, 63, 96, 4160, -64, 32):
        assert wsb(2, 2, 5, 63, H) == 0, H
        assert cov(p, p, 0, 2, 2, 5, 63, H, p, p, 1 << 20, None) == -1, H
        assert app(p, p, p, p, 2, 2, 5, 63, H, 1e-3, p, p, None) == -1, H
    for N, Cc in ((2, 9), (9, 2), (0, 2), (2, 0)):
        assert wsb(N, Cc, 5, 63, 64) == 0
        assert cov(p, p, 0, N, Cc, 5, 63, 64, p, p, 1 << 20, None) == -1, (N, Cc)
        assert app(p, p, p, p, N, Cc, 5, 63, 64, 1e-3, p, p, None) == -1, (N, Cc)
    assert cov(p, p, 0, 2, 2, 5, 63, 64, p, p, need - 1, None) == -1          # workspace one byte short
    assert cov(p, p, 0, 2, 2, 0, 63, 64, p, p, need, None) == -1
    assert cov(p, p, 0, 2, 2, 5, 0, 64, p, p, need, None) == -1
    for k in (0, 1, 8, 9):
        a = [p, p, 0, 2, 2, 5, 63, 64, p, p, need, None]
        a[k] = None
        assert cov(*a) == -1, k
    assert app(p, p, p, p, 2, 2, 5, 63, 64, -1.0, p, p, None) == -1           # reg < 0
    assert app(p, p, p, p, 2, 2, 5, 63, 64, float("nan"), p, p, None) == -1
    for k in (0, 1, 2, 3, 10, 11):
        a = [p, p, p, p, 2, 2, 5, 63, 64, 1e-3, p, p, None]
        a[k] = None
        assert app(*a) == -1, k


# ---------------------------------------------------------------------------------------------------------------------
# the restatement itself
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [64, 128, 192])
def test_hat_weights_sum_to_one_and_centres_are_counted_right(H):
    last = {64: 5, 128: 4, 192: 4}[H]                                         # 2 H + 76 is past 3 H only at H = 64
    for F, K in ((1, 1), (2, 2), (H, 2), (H + 1, 2), (2 * H + 77, last)):
        assert T.centres(F, H) == K and avsep_amd.kernels.mwf_centres(F, H) == K, (F, H)
        W = T.hat_weights(F, H)
        assert W.shape == (K, F) and (W >= 0).all()
        hat = np.maximum(0.0, 1.0 - np.abs(np.arange(F)[None, :] - H * np.arange(K)[:, None]) / H)
        assert np.abs(W - hat).max() <= 1e-15
        assert np.abs(W.sum(0) - 1.0).max() <= 1e-15 and ((W > 0).sum(0) <= 2).all()
        assert (K - 1) * H >= F - 1 and (K == 1 or (K - 2) * H < F - 1)       # the last centre is the first at or past F - 1
        W32 = T.hat_weights(F, H, np.float32)
        assert W32.dtype == np.float32 and np.abs(W32 - W).max() <= 6e-8


@pytest.mark.parametrize("H", [64, 192])
def test_restatement_with_one_covariance_at_every_centre_is_the_invariant_filter(H):
    """One source whose image is h * s[f,t] with a fixed h: every centre's R is h h^H C / |h|^2, the blend of two equal
    matrices is that matrix, and the local filter gives what mwf_ref gives."""
    g = np.random.default_rng(5)
    Cc, Fin, F = 3, 4, 2 * H + 77
    h = (g.standard_normal(Cc) + 1j * g.standard_normal(Cc))
    s = 30.0 * (g.standard_normal((Fin, F)) + 1j * g.standard_normal((Fin, F)))
    img = h[:, None, None] * s[None]
    X = img + 3.0 * (g.standard_normal((Cc, Fin, F)) + 1j * g.standard_normal((Cc, Fin, F)))
    ymag, yph = np.abs(img)[None], np.angle(img)[None]                          # float64 in: Y is h s to rounding
    for it in (1, 2):
        a = M.mwf(np.abs(X), np.angle(X), ymag, yph, it)
        b = T.mwf(np.abs(X), np.angle(X), ymag, yph, H, it)
        assert b["cov"].shape == (1, T.centres(F, H), Fin, Cc, Cc)
        assert M.rel_err(b["cov"], np.broadcast_to(a["cov"][:, None], b["cov"].shape)) <= 1e-12
        assert M.rel_err(b["Y"], a["Y"]) <= 1e-12 and np.abs(a["Y"]).max() > 10.0


def test_restatement_handles_silence_without_nan():
    """A source that is silent over a centre's whole support has R = 0 at that centre (and only there); a bin where every
    source is silent gives 0 whatever X is."""
    xmag, xph, ymag = T.value_inputs(2, 2, 257)
    ymag[1, :, :, 64:192] = 0                                                   # the support of centre 2 at H = 64 is (64, 192)
    ymag[:, :, 3, 5] = 0
    for dtype in (np.float64, np.float32):
        out = T.mwf(xmag, xph, ymag, xph, 64, 2, dtype=dtype)
        assert np.isfinite(out["mag"]).all() and np.isfinite(out["phase"]).all()
        assert (out["cov"][1, 2] == 0).all() and (np.abs(out["cov"][1, 1]).max((-1, -2)) > 0).all()
        assert (out["mag"][1, :, :, 64:192] == 0).all() and (out["mag"][:, :, 3, 5] == 0).all()


def test_local_covariances_follow_moving_sources():
    """The scene gate, a condition on the REFERENCE: on moving_sources(2, 2, 48, 640, 0, 90) (each source sweeps 90 degrees
    over the recording) the float64 local filter at H = 64 beats the float64 time-invariant filter by at least 2 dB mean SDR
    of the source images with one pass and by at least 3 dB with two.  Measured: masking 5.82 dB; invariant 7.15 / 6.88 dB,
    local 9.76 / 10.77 dB (one / two passes)."""
    sc = T.moving_sources(2, 2, 48, 640, 0, 90)
    fixed = M.panned_sources(F=640)
    still = T.moving_sources(2, 2, 48, 640, 0, 0)
    assert all(np.array_equal(still[k], fixed[k]) for k in fixed)               # no sweep: the scene of mwf_ref
    base = M.masking_sdr(sc)
    for it, need in ((1, 2.0), (2, 3.0)):
        inv = M.mean_sdr(M.mwf(sc["xmag"], sc["xph"], sc["ymag"], sc["xph"], it)["Y"], sc["images"])
        loc = M.mean_sdr(T.mwf(sc["xmag"], sc["xph"], sc["ymag"], sc["xph"], 64, it)["Y"], sc["images"])
        print(f"sources sweeping 90 degrees, {it} pass(es): masking {base:.2f} dB, invariant {inv:.2f} dB, H = 64 {loc:.2f} dB")
        assert loc - inv >= need


def test_float32_restatement_error_is_what_the_gpu_tolerance_was_sized_from():
    """test_gpu_mwf_tv.py gives the kernels 16 x the worst distance of the float32 restatement from the float64 one over its
    value cases.  The constants recorded in mwf_tv_ref.py must still be that distance (within a factor of two below, never
    above)."""
    worst_y = worst_cov = 0.0
    for Cc, N, F, H, it in T.VALUE_CASES:
        xmag, xph, ymag = T.value_inputs(Cc, N, F)
        a, b = T.mwf(xmag, xph, ymag, xph, H, it), T.mwf(xmag, xph, ymag, xph, H, it, dtype=np.float32)
        assert b["mag"].dtype == np.float32 and b["cov"].dtype == np.complex64
        worst_y, worst_cov = max(worst_y, M.rel_err(b["Y"], a["Y"])), max(worst_cov, M.rel_err(b["cov"], a["cov"]))
    print(f"float32 restatement vs float64 over {len(T.VALUE_CASES)} cases: Y {worst_y:.3e}, cov {worst_cov:.3e}")
    assert T.F32_WORST_Y / 2 <= worst_y <= T.F32_WORST_Y and T.F32_WORST_COV / 2 <= worst_cov <= T.F32_WORST_COV
    assert T.BOUND_Y == 16 * T.F32_WORST_Y and T.BOUND_COV == 16 * T.F32_WORST_COV
    assert {c[0] for c in T.VALUE_CASES} == {1, 2, 3, 8} and {c[1] for c in T.VALUE_CASES} == {1, 2, 3}
    assert {c[2] for c in T.VALUE_CASES} == {1, 63, 64, 65, 257, 2 * 2048 + 77} and {c[3] for c in T.VALUE_CASES} == {64, 128, 192}
    assert {c[4] for c in T.VALUE_CASES} == {1, 2} and T.FIN == 5


@pytest.mark.parametrize("Cc,N,F,H", T.TIE_SHAPES)
def test_float32_restatements_agree_when_every_centre_holds_the_invariant_covariance(Cc, N, F, H):
    """What test_gpu_mwf_tv.py asks of the two apply kernels, asked of the references first: with the time-invariant
    covariance repeated at all K centres the blend (1 - u) R + u R is R up to one rounding, so the float32 mode of
    mwf_tv_ref.apply must give what the float32 mode of mwf_ref.apply gives, polar conversions included, within BOUND_Y
    (measured: 0.9e-07 ... 1.9e-07); in float64 the two agree to 1e-12, the figure of the test above (measured: 4e-16)."""
    xmag, xph, ymag = T.value_inputs(Cc, N, F)
    for dtype, bound in ((np.float64, 1e-12), (np.float32, T.BOUND_Y)):
        R, v = M.cov(ymag, xph, dtype)
        rep = np.ascontiguousarray(np.broadcast_to(R[:, None], (N, T.centres(F, H)) + R.shape[1:]))
        a = M.polar_to_complex(*M.complex_to_polar(M.apply(xmag, xph, v, R, dtype=dtype), dtype))
        b = M.polar_to_complex(*M.complex_to_polar(T.apply(xmag, xph, v, rep, H, dtype=dtype), dtype))
        err = M.rel_err(b, a)
        print(f"C={Cc} N={N} F={F} H={H} {np.dtype(dtype).name}: local against invariant restatement {err:.3e} (bound {bound:.2e})")
        assert err <= bound and np.abs(a).max() > 10.0
