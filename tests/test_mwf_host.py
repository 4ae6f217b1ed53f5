"""not-gpu: the host side of the multichannel Wiener filter (--wiener of separate.py, separate_long(wiener=...), the argument
checks of kernels.mwf / mwf_cov and of the avsep_mwf_* entry points, which refuse before anything touches a GPU), and checks
on the float64 restatement tests/mwf_ref.py itself, so that the GPU tests do not trust it blindly."""
import ctypes as C

import numpy as np
import pytest
import torch

import avsep_amd
from avsep_amd import separate as S
from avsep_amd.lib import AvsepError

import mwf_ref as M
from recipes import no_gpu_call as _no_gpu_call


# ---------------------------------------------------------------------------------------------------------------------
# flags and refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_cli_wiener_flag():
    a = S.parse_args(["--wav", "mix.wav", "--audio_only"])
    assert a.wiener == 0 and a.channels == "mix"
    b = S.parse_args(["--wav", "mix.wav", "--audio_only", "--channels", "keep", "--wiener", "2"])
    assert b.wiener == 2
    assert S.parse_args(["--wav", "mix.wav", "--audio_only", "--channels", "keep", "--wiener", "0"]).wiener == 0
    assert S.parse_args(["--wav", "mix.wav", "--audio_only", "--wiener", "0"]).wiener == 0      # 0 needs nothing
    with pytest.raises(SystemExit) as e:
        S.parse_args(["--wav", "mix.wav", "--audio_only", "--wiener", "1"])
    assert "--channels keep" in str(e.value)
    with pytest.raises(SystemExit):
        S.parse_args(["--wav", "mix.wav", "--audio_only", "--channels", "mix", "--wiener", "1"])
    for bad in ("9", "-1"):
        with pytest.raises(SystemExit):
            S.parse_args(["--wav", "mix.wav", "--audio_only", "--channels", "keep", "--wiener", bad])


def test_separate_long_refuses_wiener_without_channels_and_out_of_range(monkeypatch):
    _no_gpu_call(monkeypatch)
    wav = torch.zeros(4096)
    ch = torch.zeros(2, 4096)
    with pytest.raises(AvsepError) as e:
        S.separate_long((None, None), wav, [], None, wiener=1)
    assert "channels" in str(e.value)
    for bad in (-1, 9, 1.0, "1", True, None):
        with pytest.raises(AvsepError) as e:
            S.separate_long((None, None), wav, [], None, channels=ch, wiener=bad)
        assert "wiener" in str(e.value)
    assert S.MAX_WIENER == 8


def test_mwf_refuses_cpu_tensors_and_bad_shapes():
    """Valid arguments on the CPU: no fallback of any kind."""
    K = avsep_amd.kernels
    x, y = torch.zeros(2, 5, 7), torch.zeros(3, 2, 5, 7)
    with pytest.raises(AvsepError):
        K.mwf(x, x, y, x)
    with pytest.raises(AvsepError):
        K.mwf(x, x, y, y, iterations=2)
    with pytest.raises(AvsepError):
        K.mwf_cov(y, x)
    with pytest.raises(AvsepError):
        K.mwf_cov(y, y)


def test_mwf_entry_points_refuse_bad_arguments_before_launching():
    """include/avsep.h: C or N outside [1, 8], a workspace that is too small and null pointers are argument errors (-1);
    the workspace query answers 0 for the same dimensions."""
    lib = avsep_amd.lib.load()
    buf = (C.c_float * 4096)()
    p = C.addressof(buf)
    need = lib.avsep_mwf_workspace_bytes(2, 2, 5, 63)
    assert need == 1 * 2 * 5 * (2 * 3 + 1) * 4                               # one chunk: 2 sources x 5 rows x 7 floats
    assert lib.avsep_mwf_workspace_bytes(2, 2, 5, 2049) == 2 * need          # chunks of 2048 frames
    assert lib.avsep_mwf_workspace_bytes(3, 8, 5, 63) == 3 * 5 * 73 * 4
    cov, app = lib.avsep_mwf_cov, lib.avsep_mwf_apply
    for N, Cc in ((2, 9), (9, 2), (0, 2), (2, 0)):
        assert lib.avsep_mwf_workspace_bytes(N, Cc, 5, 63) == 0
        assert cov(p, p, 0, N, Cc, 5, 63, p, p, 1 << 20, None) == -1, (N, Cc)
        assert app(p, p, p, p, N, Cc, 5, 63, 1e-3, p, p, None) == -1, (N, Cc)
    assert cov(p, p, 0, 2, 2, 5, 63, p, p, need - 1, None) == -1             # workspace one byte short
    assert cov(p, p, 0, 2, 2, 5, 63, p, p, 0, None) == -1
    assert cov(p, p, 0, 2, 2, 0, 63, p, p, need, None) == -1
    assert cov(p, p, 0, 2, 2, 5, 0, p, p, need, None) == -1
    assert cov(None, p, 0, 2, 2, 5, 63, p, p, need, None) == -1
    assert cov(p, None, 0, 2, 2, 5, 63, p, p, need, None) == -1
    assert cov(p, p, 0, 2, 2, 5, 63, None, p, need, None) == -1
    assert cov(p, p, 0, 2, 2, 5, 63, p, None, need, None) == -1
    assert app(p, p, p, p, 2, 2, 5, 63, -1.0, p, p, None) == -1              # reg < 0
    assert app(p, p, p, p, 2, 2, 5, 63, float("nan"), p, p, None) == -1
    for k in range(4):
        a = [p, p, p, p]
        a[k] = None
        assert app(*a, 2, 2, 5, 63, 1e-3, p, p, None) == -1
    assert app(p, p, p, p, 2, 2, 5, 63, 1e-3, None, p, None) == -1
    assert app(p, p, p, p, 2, 2, 5, 63, 1e-3, p, None, None) == -1


# ---------------------------------------------------------------------------------------------------------------------
# the restatement itself
# ---------------------------------------------------------------------------------------------------------------------
def test_restatement_is_the_single_channel_wiener_gain_for_one_channel():
    """C = 1: R_n = 1, v_n = M_n^2 |X|^2, S = (1 + reg) sum_n v_n, so Y_n' = M_n^2 / sum_m M_m^2 * X / (1 + reg) in closed form."""
    g = np.random.default_rng(1)
    Fin, F, N = 5, 63, 3
    xmag = (30 * g.random((1, Fin, F)) + 1).astype(np.float32)
    xph = g.uniform(-np.pi, np.pi, (1, Fin, F)).astype(np.float32)
    ymag = (g.random((N, 1, Fin, F)).astype(np.float32) * xmag[None]).astype(np.float32)
    out = M.mwf(xmag, xph, ymag, xph, 1)
    assert np.allclose(out["cov"], 1.0, rtol=0, atol=1e-12) and out["cov"].shape == (N, Fin, 1, 1)
    m = ymag.astype(np.float64)[:, 0] / xmag.astype(np.float64)[0]                     # the masks the inputs really hold
    want = (m ** 2 / (m ** 2).sum(0))[:, None] * M.polar_to_complex(xmag, xph)[None] / (1 + M.REG)
    assert M.rel_err(out["Y"], want) <= 1e-12
    # the stems of a pass sum to the mixture over 1 + reg
    assert M.rel_err(out["Y"].sum(0), M.polar_to_complex(xmag, xph) / (1 + M.REG)) <= 1e-12


def test_restatement_handles_silence_without_nan():
    """A source that is silent in a row has R_n = 0 and output 0; a bin where every source is silent gives 0 whatever X is."""
    xmag, xph, ymag = M.value_inputs(2, 2, 63)
    ymag[1, :, 2] = 0
    ymag[:, :, 3, 5] = 0
    for dtype in (np.float64, np.float32):
        out = M.mwf(xmag, xph, ymag, xph, 2, dtype=dtype)
        assert np.isfinite(out["mag"]).all() and np.isfinite(out["phase"]).all()
        assert (out["cov"][1, 2] == 0).all() and (out["mag"][1, :, 2] == 0).all() and (out["mag"][:, :, 3, 5] == 0).all()


def test_one_pass_raises_the_sdr_of_panned_sources_by_3_db():
    """A condition on the REFERENCE: on the scene of mwf_ref.panned_sources (two sources at two places of a stereo image,
    noisy ratio masks) one pass must beat per-channel masking by at least 3 dB mean SDR of the source images, a second pass
    must not lose that.  Measured: masking 5.79 dB, one pass 9.95 dB (+4.16), two passes 11.21 dB."""
    sc = M.panned_sources()
    base = M.masking_sdr(sc)
    one = M.mean_sdr(M.mwf(sc["xmag"], sc["xph"], sc["ymag"], sc["xph"], 1)["Y"], sc["images"])
    two = M.mean_sdr(M.mwf(sc["xmag"], sc["xph"], sc["ymag"], sc["xph"], 2)["Y"], sc["images"])
    print(f"panned sources: masking {base:.2f} dB, one pass {one:.2f} dB (+{one - base:.2f}), two passes {two:.2f} dB")
    assert one - base >= 3.0 and two - base >= 3.0


def test_float32_restatement_error_is_what_the_gpu_tolerance_was_sized_from():
    """test_gpu_mwf.py gives the kernels 16 x the worst distance of the float32 restatement from the float64 one over its
    value cases.  The constants recorded in mwf_ref.py must still be that distance (within a factor of two below, never
    above)."""
    G = M
    worst_y = worst_cov = 0.0
    for Cc, N, F, it in M.VALUE_CASES:
        xmag, xph, ymag = M.value_inputs(Cc, N, F)
        a, b = M.mwf(xmag, xph, ymag, xph, it), M.mwf(xmag, xph, ymag, xph, it, dtype=np.float32)
        assert b["mag"].dtype == np.float32 and b["cov"].dtype == np.complex64
        worst_y, worst_cov = max(worst_y, M.rel_err(b["Y"], a["Y"])), max(worst_cov, M.rel_err(b["cov"], a["cov"]))
    print(f"float32 restatement vs float64 over {len(M.VALUE_CASES)} cases: Y {worst_y:.3e}, cov {worst_cov:.3e}")
    assert G.F32_WORST_Y / 2 <= worst_y <= G.F32_WORST_Y and G.F32_WORST_COV / 2 <= worst_cov <= G.F32_WORST_COV
    assert G.BOUND_Y == 16 * G.F32_WORST_Y and G.BOUND_COV == 16 * G.F32_WORST_COV
    assert {c[0] for c in M.VALUE_CASES} == {1, 2, 3, 8} and {c[1] for c in M.VALUE_CASES} == {1, 2, 3}
    assert {c[2] for c in M.VALUE_CASES} == {1, 63, M.F_LONG} and M.F_LONG > 2 * 2048 and M.F_LONG % 2 == 1
