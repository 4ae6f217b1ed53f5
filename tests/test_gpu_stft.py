"""avsep_stft_mag / avsep_istft (csrc/stft.hip) and the 1x4-conv launch c1x4_stft_fwd (csrc/conv3x3.hip) against float64, element
by element, over every row of tests/stft_cases.py.  The reference, its magnitude bound and the gates are tests/stftref.py (held
against torch.stft / torch.istft in float64, a float32 control and nine mutants in tests/test_stftref.py); tau = 2e-5 for every
element, nothing excluded, and an output under a zero bound (a silent row, a silent frame) must be exactly zero.

Every row first asserts the path it takes -- the workspace formula of its path, which differs from the other path's -- and, where a
conv descriptor decides the kernel, the family the library reports for the descriptor stft_pad_gemm / istft_gemm fill.  A moved
guard fails the row instead of testing the other path.  test_rows_take_their_path needs the library but no device.

A failure prints the worst |error| / bound with its (row, bin or sample, frame).  The ratios measured on an MI355X are beside the
rows in tests/stft_cases.py."""
import ctypes

import numpy as np
import pytest
import torch

import stft_cases as SC
import stftref as SR
from recipes import pkg as _pkg

ERR_ARG, ERR_LAUNCH, ERR_WORKSPACE = -1, -2, -3


def _plan(dev, n_fft, hop, mode, cache={}):
    key = (str(dev), n_fft, hop, mode)
    if key not in cache:
        cache[key] = _pkg().kernels.Stft(dev, n_fft, hop, mode)
    return cache[key]


def _family(d):
    return _pkg().lib.load().avsep_conv_kernel_name(ctypes.byref(d), 0, 0).decode()


def _forward_desc(R, L, n_fft, hop):
    """The descriptor stft_pad_gemm fills on the fallback path: one input channel, a 1 x n_fft window, stride hop."""
    d = _pkg().lib.ConvDesc()
    d.N, d.Cin, d.H, d.W, d.Cout, d.Ho, d.Wo = R, 1, 1, L + 2 * (n_fft // 2), 2 * SR.bins_of(n_fft), 1, 1 + L // hop
    d.KH, d.KW, d.stride, d.pad, d.dil, d.C0, d.x0 = 1, n_fft, hop, 0, 1, 1, 256
    return d


def _inverse_desc(R, n_fft, frames):
    """The descriptor istft_gemm fills: a 1x1 conv over [R, 2 bins, 1, frames]."""
    d = _pkg().lib.ConvDesc()
    d.N, d.Cin, d.H, d.W, d.Cout, d.Ho, d.Wo = R, 2 * SR.bins_of(n_fft), 1, frames, n_fft, 1, frames
    d.KH, d.KW, d.stride, d.pad, d.dil, d.C0, d.x0 = 1, 1, 1, 0, 1, d.Cin, 256
    return d


def _assert_forward_path(name):
    n_fft, hop, R, L, _, path, fam = SC.FORWARD[name]
    other = "fallback" if path == "fast" else "fast"
    got = _pkg().lib.load().avsep_stft_workspace_bytes(R, L, n_fft, hop)
    assert SC.workspace_bytes(R, L, n_fft, hop, path) != SC.workspace_bytes(R, L, n_fft, hop, other)
    assert got == SC.workspace_bytes(R, L, n_fft, hop, path), (name, path, got)
    if path == "fallback":
        assert _family(_forward_desc(R, L, n_fft, hop)) == fam, name
    else:
        assert fam == SC.HALO           # c1x4_stft_fwd launches conv3x3_kernel itself, no descriptor


def _assert_inverse_family(name):
    n_fft, hop, R, frames, fam = SC.INVERSE[name]
    assert _family(_inverse_desc(R, n_fft, frames)) == fam, name


def test_rows_take_their_path():
    for name in SC.FORWARD:
        _assert_forward_path(name)
    for name in SC.INVERSE:
        _assert_inverse_family(name)


def _check(what, ratio, at):
    print(f"{what}: worst |error| / bound = {ratio:.4f} at (row, bin or sample, frame) = {at}")
    assert ratio <= 1.0, f"{what}: |error| / bound = {ratio:.4g} at (row, bin or sample, frame) = {at}"


@pytest.mark.gpu
@pytest.mark.parametrize("name,mode", SC.FORWARD_ROWS)
def test_stft_rows(dev, name, mode):
    _assert_forward_path(name)
    n_fft, hop, R, L = SC.FORWARD[name][:4]
    wav = torch.from_numpy(SC.forward_input(name)).to(dev)
    ref = SC.forward_ref(name, mode)
    plan = _plan(dev, n_fft, hop, mode)
    mag, phase = plan.stft(wav)
    assert mag.shape == phase.shape == ref[0].shape and mag.dtype == phase.dtype == torch.float32
    mag, phase = mag.cpu().numpy(), phase.cpu().numpy()
    _check(f"{name} {mode} magnitude", *SR.gate_mag(mag, ref))
    _check(f"{name} {mode} phase", *SR.gate_phase(mag, phase, ref))
    if name == "F1":
        only, none = plan.stft(wav, want_phase=False)
        assert none is None
        _check(f"{name} {mode} magnitude without phase", *SR.gate_mag(only.cpu().numpy(), ref))


@pytest.mark.gpu
@pytest.mark.parametrize("name,kind", SC.INVERSE_ROWS)
def test_istft_rows(dev, name, kind):
    _assert_inverse_family(name)
    n_fft, hop, R, frames = SC.INVERSE[name][:4]
    mag, phase = (torch.from_numpy(t).to(dev) for t in SC.inverse_input(name, kind))
    wav = _plan(dev, n_fft, hop, "reflect").istft(mag, phase)
    assert wav.shape == (R, hop * (frames - 1)) and wav.dtype == torch.float32
    _check(f"{name} {kind}", *SR.gate_inverse(wav.cpu().numpy(), SC.inverse_ref(name, kind)))


@pytest.mark.gpu
@pytest.mark.parametrize("name,cut", SC.SHORT_ROWS)
def test_istft_short_output(dev, name, cut):
    """out_len below hop * (frames - 1), called directly: the written part passes the gate, the 8 floats behind it stay NaN."""
    K = _pkg().kernels
    n_fft, hop, R, frames = SC.INVERSE[name][:4]
    out_len = SC.short_len(name, cut)
    plan = _plan(dev, n_fft, hop, "reflect")
    nbytes = _pkg().lib.load().avsep_istft_workspace_bytes(R, n_fft, frames)
    ws = torch.empty((nbytes // 4,), dtype=torch.float32, device=dev)
    for kind in "ab":
        mag, phase = (torch.from_numpy(t).to(dev) for t in SC.inverse_input(name, kind))
        buf = torch.full((R * out_len + SC.GUARD,), float("nan"), dtype=torch.float32, device=dev)
        K.call("avsep_istft", K.ptr(mag), K.ptr(phase), R, n_fft, hop, frames, K.ptr(plan.inv_basis), K.ptr(buf), out_len,
               K.ptr(ws), nbytes)
        got = buf.cpu().numpy()
        assert np.isnan(got[R * out_len:]).all(), "wrote past out_len"
        _check(f"{name} {kind} out_len {out_len}", *SR.gate_inverse(got[:R * out_len].reshape(R, out_len),
                                                                    SC.inverse_ref(name, kind, out_len)))


@pytest.mark.gpu
def test_round_trip_at_f1(dev):
    """iSTFT(STFT(x)) on the device against the float64 round trip (the inverse of the float32 cast of the float64 STFT)."""
    n_fft, hop, R, L = SC.FORWARD["F1"][:4]
    re, im, _, _ = SC.forward_ref("F1", "reflect")
    ref = SR.istft(np.hypot(re, im).astype(np.float32), np.arctan2(im, re).astype(np.float32), n_fft, hop, hop * (L // hop))
    plan = _plan(dev, n_fft, hop, "reflect")
    wav = plan.istft(*plan.stft(torch.from_numpy(SC.forward_input("F1")).to(dev)))
    assert wav.shape == ref[0].shape
    _check("F1 round trip", *SR.gate_inverse(wav.cpu().numpy(), ref))


@pytest.mark.gpu
def test_refusals_leave_the_output_alone(dev):
    """Bad arguments give AVSEP_ERR_ARG, a workspace 4 bytes short AVSEP_ERR_WORKSPACE, and neither writes anything."""
    K, L = _pkg().kernels, _pkg().lib.load()
    n_fft, hop, R, Ln, frames = 1022, 256, 2, 2048, 9
    plan = _plan(dev, n_fft, hop, "reflect")
    bins = SR.bins_of(n_fft)
    wav = torch.zeros(R, Ln, device=dev)
    spec = torch.ones(R, bins, frames, device=dev)
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=dev)
    ws = torch.empty(1 << 20, dtype=torch.float32, device=dev)
    st = K.lib.stream()

    def fwd(R=R, Ln=Ln, n_fft=n_fft, nbytes=None):
        mag, phase = nan(2, bins, frames), nan(2, bins, frames)
        nbytes = L.avsep_stft_workspace_bytes(max(R, 1), Ln, n_fft + (n_fft & 1), hop) if nbytes is None else nbytes
        rc = L.avsep_stft_mag(K.ptr(wav), R, Ln, n_fft, hop, 1, K.ptr(plan.fwd_basis), K.ptr(mag), K.ptr(phase), K.ptr(ws), nbytes, st)
        torch.cuda.synchronize()
        assert bool(torch.isnan(mag).all()) and bool(torch.isnan(phase).all()), "a refused call wrote its output"
        return rc

    def inv(R=R, n_fft=n_fft, out_len=hop * (frames - 1), nbytes=None):
        out = nan(2, hop * (frames - 1) + 1)
        nbytes = L.avsep_istft_workspace_bytes(max(R, 1), n_fft + (n_fft & 1), frames) if nbytes is None else nbytes
        rc = L.avsep_istft(K.ptr(spec), K.ptr(spec), R, n_fft, hop, frames, K.ptr(plan.inv_basis), K.ptr(out), out_len, K.ptr(ws),
                           nbytes, st)
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all()), "a refused call wrote its output"
        return rc

    assert 4 * ws.numel() >= L.avsep_stft_workspace_bytes(R, Ln, n_fft, hop) > 0
    assert 4 * ws.numel() >= L.avsep_istft_workspace_bytes(R, n_fft, frames) > 0
    assert fwd(n_fft=1021) == ERR_ARG and inv(n_fft=1021) == ERR_ARG
    assert fwd(Ln=n_fft // 2) == ERR_ARG
    assert fwd(R=0) == ERR_ARG and inv(R=0) == ERR_ARG
    assert inv(out_len=hop * (frames - 1) + 1) == ERR_ARG and inv(out_len=0) == ERR_ARG
    assert fwd(nbytes=L.avsep_stft_workspace_bytes(R, Ln, n_fft, hop) - 4) == ERR_WORKSPACE
    assert inv(nbytes=L.avsep_istft_workspace_bytes(R, n_fft, frames) - 4) == ERR_WORKSPACE
