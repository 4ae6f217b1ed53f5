"""not-gpu: the host side of the mixture-consistent phase iterations (--phase_iters of separate.py,
separate_long(phase_iters=...), the argument checks of kernels.Stft.misi and of avsep_misi, which refuse before anything
touches a GPU), and checks on the float64 restatement tests/misi_ref.py itself, so that the GPU tests do not trust it blindly.

Measured with misi_ref.sdr_scene (two harmonic sources with vibrato, oracle magnitudes, mixture phase as the start; float64):
mean SDR 14.77 dB at K = 0, 15.62 (K = 1, +0.85), 16.52 (K = 2, +1.75), 17.66 (K = 4, +2.89), 20.54 (K = 8, +5.77)."""
import ctypes as C

import pytest
import torch

import avsep_amd
from avsep_amd import separate as S
from avsep_amd.lib import AvsepError

import misi_ref as M
from recipes import no_gpu_call as _no_gpu_call

MAX_ITERS = S.MAX_PHASE_ITERS          # the feature's own constant: without the feature this file does not even import

# ---------------------------------------------------------------------------------------------------------------------
# flags and refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_cli_phase_iters_flag():
    base = ["--wav", "mix.wav", "--audio_only"]
    assert S.parse_args(base).phase_iters == 0
    assert S.parse_args(base + ["--phase_iters", "4"]).phase_iters == 4
    assert S.parse_args(base + ["--phase_iters", str(MAX_ITERS)]).phase_iters == MAX_ITERS == 32
    assert S.parse_args(base + ["--channels", "keep", "--wiener", "1", "--phase_iters", "2"]).phase_iters == 2
    for bad in (str(MAX_ITERS + 1), "-1"):
        with pytest.raises(SystemExit) as e:
            S.parse_args(base + ["--phase_iters", bad])
        assert "--phase_iters" in str(e.value)


def test_separate_long_refuses_phase_iters_out_of_range(monkeypatch):
    _no_gpu_call(monkeypatch)
    wav = torch.zeros(4096)
    for bad in (True, False, -1, MAX_ITERS + 1, 2.0, "2", None):
        with pytest.raises(AvsepError) as e:
            S.separate_long((None, None), wav, [], None, phase_iters=bad)
        assert "phase_iters" in str(e.value) and repr(bad) in str(e.value)


def test_misi_refuses_cpu_tensors():
    """Valid arguments on the CPU: no fallback of any kind."""
    plan = avsep_amd.kernels.Stft.__new__(avsep_amd.kernels.Stft)          # the constructor builds the bases on a GPU
    plan.n_fft, plan.hop, plan.reflect = 64, 32, 1
    with pytest.raises(AvsepError):
        plan.misi(torch.zeros(1, 640), torch.zeros(2, 1, 33, 21), torch.zeros(1, 33, 21), 1)


def test_misi_entry_point_refuses_bad_arguments_before_launching():
    """include/avsep.h: N or G outside [1, 8], no pass, too short a signal, null pointers and a workspace that is too small
    are refused before any launch; the workspace query answers 0 for dimensions the call refuses."""
    lib = avsep_amd.lib.load()
    buf = (C.c_float * 4096)()
    p = C.addressof(buf)
    ws, call = lib.avsep_misi_workspace_bytes, lib.avsep_misi
    need = ws(2, 1, 64, 32, 21)
    assert need > 0 and need % 4 == 0
    assert ws(2, 8, 64, 32, 21) == need                                   # the groups run one after the other
    assert ws(3, 1, 64, 32, 21) > need
    ok = dict(N=2, G=1, n_fft=64, hop=32, frames=21, it=1)

    def run(ptrs=(p,) * 6, ws_ptr=p, ws_bytes=need, **kw):
        a = dict(ok, **kw)
        mix, mag, ph, fb, ib, out = ptrs
        return call(mix, mag, ph, 0, a["N"], a["G"], a["n_fft"], a["hop"], a["frames"], 1, a["it"], fb, ib, out, None, ws_ptr,
                    ws_bytes, None)
    for kw in (dict(N=0), dict(N=9), dict(G=0), dict(G=9), dict(it=0), dict(it=-1), dict(n_fft=63), dict(n_fft=0), dict(hop=0),
               dict(frames=1), dict(frames=0), dict(frames=2)):           # frames = 2: 32 samples, not more than n_fft / 2
        assert run(**kw) == -1, kw
        if "it" not in kw:
            a = dict(ok, **kw)
            assert ws(a["N"], a["G"], a["n_fft"], a["hop"], a["frames"]) == 0, kw
    for k in range(6):
        ptrs = [p] * 6
        ptrs[k] = None
        assert run(ptrs=tuple(ptrs)) == -1, k
    assert run(ws_ptr=None) != 0 and run(ws_bytes=need - 1) != 0 and run(ws_bytes=0) != 0


# ---------------------------------------------------------------------------------------------------------------------
# the restatement itself
# ---------------------------------------------------------------------------------------------------------------------
def test_restatement_transform_pair_is_torchs():
    """misi_ref.stft / istft against torch.stft / torch.istft (periodic Hann, centred): the same numbers."""
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, 256 * 12, generator=g, dtype=torch.float64)
    w = M.window(1022)
    for reflect in (True, False):
        Z = M.stft(x, 1022, 256, reflect)
        want = torch.stft(x, 1022, 256, window=w, center=True, pad_mode="reflect" if reflect else "constant", return_complex=True)
        assert Z.shape == want.shape == (2, 512, 13) and M.rel_err(Z, want) <= 1e-12
    back = M.istft(Z, 1022, 256)
    want = torch.istft(Z, 1022, 256, window=w, center=True, length=256 * 12)
    assert back.shape == (2, 256 * 12) and M.rel_err(back[:, 600:-600], want[:, 600:-600]) <= 1e-12
    assert M.rel_err(M.istft(M.stft(x, 1022, 256), 1022, 256)[:, 600:-600], x[:, 600:-600]) <= 1e-12


def test_one_pass_with_one_source_keeps_the_mixtures_phase():
    """N = 1: e / N hands the whole error back, so the projected stem IS the mixture and one pass is
    istft(A * phase of stft(x)), whatever the start phase was."""
    mix, A, ph = M.value_inputs(64, 32, 21, 1, 2, True, True)
    got = M.misi(mix, A, ph, 1, 64, 32)["wav"]
    X = M.stft(mix, 64, 32)
    want = M.istft(A.double()[0] * M.unit(X), 64, 32)
    assert M.rel_err(got[0], want) <= 1e-12


def test_consistent_input_is_a_fixed_point():
    """A_n = |STFT(s_n)|, phi0 = angle STFT(s_n), x = sum_n s_n over out_len samples: the window-sum-square normalisation
    makes the inverse exact at every sample, so every pass finds e = 0 and the spectra it started from."""
    g = torch.Generator().manual_seed(4)
    for reflect in (True, False):
        src = 0.1 * torch.randn(3, 1, 32 * 20, generator=g, dtype=torch.float64)
        Z = M.stft(src, 64, 32, reflect)
        out = M.misi(src.sum(0), Z.abs(), torch.atan2(Z.imag, Z.real), 3, 64, 32, reflect)
        assert M.rel_err(out["wav"], src) <= 1e-9 and M.rel_err(out["Y"], Z) <= 1e-9


def test_sdr_rises_with_the_passes_on_oracle_magnitudes():
    """A condition on the REFERENCE (the scene and the measured figures: the header): strictly rising at K = 1, 2, 4 and at
    least 2 dB over the mixture phase at K = 4."""
    sc = M.sdr_scene()
    sdr = {k: M.scene_sdr(sc, k) for k in (0, 1, 2, 4)}
    print("mean SDR: " + ", ".join(f"K={k} {v:.2f} dB (+{v - sdr[0]:.2f})" for k, v in sdr.items()))
    assert sdr[0] < sdr[1] < sdr[2] < sdr[4] and sdr[4] - sdr[0] >= 2.0


def test_float32_restatement_error_is_what_the_gpu_tolerance_was_sized_from():
    """test_gpu_misi.py gives the kernels 16 x the worst distance of the float32 restatement from the float64 one over its
    value cases.  The constant recorded in misi_ref.py must still be that distance (within a factor of two below, never
    above), and the cases must cover what they claim."""
    worst = 0.0
    for n_fft, hop, F, N, G, K, per_source, reflect in M.VALUE_CASES:
        mix, A, ph = M.value_inputs(n_fft, hop, F, N, G, per_source, reflect)
        a = M.misi(mix, A, ph, K, n_fft, hop, reflect)
        b = M.misi(mix, A, ph, K, n_fft, hop, reflect, dtype=torch.float32)
        assert b["wav"].dtype == torch.float32 and b["Y"].dtype == torch.complex64
        worst = max(worst, M.rel_err(b["wav"], a["wav"]))
    print(f"float32 restatement vs float64 over {len(M.VALUE_CASES)} cases: {worst:.3e}")
    assert M.F32_WORST / 2 <= worst <= M.F32_WORST and M.BOUND == 16 * M.F32_WORST
    shapes = {c[:3] for c in M.VALUE_CASES}
    assert shapes == {(1022, 256, 37), (1022, 256, 9), (64, 32, 21), (30, 8, 37)}
    for sh in shapes:
        mine = [c for c in M.VALUE_CASES if c[:3] == sh]
        assert {c[3] for c in mine} == {1, 2, 3} and {c[4] for c in mine} == {1, 2}
        assert {c[6] for c in mine} == {True, False} and {c[7] for c in mine} == {True, False}
    assert {c[5] for c in M.VALUE_CASES} == {1, 2, 4}
