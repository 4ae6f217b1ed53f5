"""torch-CPU restatement of the mixture-consistent phase iterations (MISI; include/avsep.h), the reference of
test_misi_host.py and test_gpu_misi.py.  ``dtype=torch.float64`` is the reference; ``dtype=torch.float32`` runs the same
formula in float32 / complex64 throughout (window, FFTs, overlap-add, the division by |Z|): its distance from the float64
mode on a test's inputs is the size of an honest fp32 implementation's error, and is used only to size the tolerance.

R = N * G rows, group g = the N rows that sum to mixture x[g] of out_len = hop * (F - 1) samples; A [N,G,bins,F] the target
magnitudes, phi0 [G,bins,F] (shared) or [N,G,bins,F] the start phase:
  1. s_n = iSTFT(A_n e^{i phi0})              librosa's inverse: synthesis window, window-sum-square normalisation, centre trim
  2. for k = 1 ... K:  e = x - sum_n s_n (n ascending);  Z_n = STFT(s_n + e / N);  U = Z / |Z| (1 where |Z| = 0);
                       s_n = iSTFT(A_n U_n)
  3. the result is s after the last pass (the plain iSTFT of the last spectrum), with the last phase angle(U).

``sdr_scene`` is the two-source scene both test files use to show what the iterations are for."""
import math

import numpy as np
import torch

FLT_MIN = float(np.finfo(np.float32).tiny)


def _cplx(dtype):
    return torch.complex64 if dtype == torch.float32 else torch.complex128


def window(n_fft, dtype=torch.float64):
    n = torch.arange(n_fft, dtype=torch.float64)
    return (0.5 - 0.5 * torch.cos(2.0 * math.pi * n / n_fft)).to(dtype)


def stft(x, n_fft, hop, reflect=True, dtype=torch.float64):
    """x [..., L] -> complex [..., n_fft/2+1, 1 + L // hop] (centred, periodic Hann, reflect or zero padding)."""
    x = torch.as_tensor(x).to(dtype)
    pad = n_fft // 2
    flat = x.reshape(1, -1, x.shape[-1])
    xp = torch.nn.functional.pad(flat, (pad, pad), mode="reflect") if reflect else torch.nn.functional.pad(flat, (pad, pad))
    fr = xp.reshape(*x.shape[:-1], -1).unfold(-1, n_fft, hop) * window(n_fft, dtype)       # [..., F, n_fft]
    return torch.fft.rfft(fr, dim=-1).transpose(-1, -2).to(_cplx(dtype))


def istft(Z, n_fft, hop, dtype=torch.float64):
    """complex [..., bins, F] -> [..., hop * (F - 1)]."""
    Z = torch.as_tensor(Z).to(_cplx(dtype))
    F = Z.shape[-1]
    w = window(n_fft, dtype)
    fr = torch.fft.irfft(Z.transpose(-1, -2), n=n_fft, dim=-1).to(dtype) * w                # [..., F, n_fft]
    y = torch.zeros(*Z.shape[:-2], n_fft + hop * (F - 1), dtype=dtype)
    wss = torch.zeros(n_fft + hop * (F - 1), dtype=dtype)
    for f in range(F):                                                                      # frames in ascending order
        y[..., f * hop:f * hop + n_fft] += fr[..., f, :]
        wss[f * hop:f * hop + n_fft] += w * w
    y = torch.where(wss > FLT_MIN, y / wss.clamp_min(FLT_MIN), y)
    return y[..., n_fft // 2:n_fft // 2 + hop * (F - 1)]


def polar(mag, ph, dtype=torch.float64):
    mag, ph = torch.as_tensor(mag).to(dtype), torch.as_tensor(ph).to(dtype)
    return torch.complex(mag * torch.cos(ph), mag * torch.sin(ph))


def unit(Z):
    """Z / |Z|, and 1 where |Z| = 0."""
    a = Z.abs()
    safe = torch.where(a > 0, a, torch.ones_like(a))
    return torch.where(a > 0, Z / safe.to(Z.dtype), torch.ones((), dtype=Z.dtype))


def misi(mix, A, phase, iterations, n_fft, hop, reflect=True, dtype=torch.float64):
    """mix [G,out_len], A [N,G,bins,F], phase [G,bins,F] or [N,G,bins,F] -> {"wav" [N,G,out_len], "Y" = A U complex
    [N,G,bins,F] (the last spectrum), "phase" its angle}.  iterations = 0: the plain iSTFT on the start phase."""
    mix, A = torch.as_tensor(mix).to(dtype), torch.as_tensor(A).to(dtype)
    N = A.shape[0]
    phase = torch.as_tensor(phase).to(dtype).expand(A.shape)
    Y = polar(A, phase, dtype)
    s = istft(Y, n_fft, hop, dtype)
    for _ in range(int(iterations)):
        tot = torch.zeros_like(s[0])
        for n in range(N):
            tot = tot + s[n]
        e = mix - tot
        Z = stft(s + e / N, n_fft, hop, reflect, dtype)
        Y = A.to(Z.dtype) * unit(Z)
        s = istft(Y, n_fft, hop, dtype)
    return {"wav": s, "Y": Y, "phase": torch.atan2(Y.imag, Y.real)}


def rel_err(a, b):
    """max|a - b| / max|b| in float64 (complex or real)."""
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    ct = torch.complex128 if (a.is_complex() or b.is_complex()) else torch.float64
    return float((a.to(ct) - b.to(ct)).abs().max() / b.to(ct).abs().max())


# ---------------------------------------------------------------------------------------------------------------------
# value cases of test_gpu_misi.py: (n_fft, hop, F, N, G, K, phase per source, reflect).  1022/256/37 and 30/8/37 take the
# hop-transposed GEMM (37 frames: not a multiple of the 32-hop block), 1022/256/9 (fewer than 32 frames) and 64/32/21 the
# generic one.  Every shape sees N = 1, 2, 3, both G, shared and per-source phases and both paddings; K = 1, 2, 4 overall.
# ---------------------------------------------------------------------------------------------------------------------
VALUE_CASES = [
    (1022, 256, 37, 1, 1, 1, False, True), (1022, 256, 37, 2, 1, 2, True, True), (1022, 256, 37, 3, 2, 4, False, True),
    (1022, 256, 37, 2, 2, 1, True, False),
    (1022, 256, 9, 1, 2, 2, False, True), (1022, 256, 9, 2, 1, 4, True, True), (1022, 256, 9, 3, 1, 1, False, False),
    (1022, 256, 9, 2, 2, 2, True, True),
    (64, 32, 21, 1, 1, 4, True, True), (64, 32, 21, 2, 2, 1, False, False), (64, 32, 21, 3, 1, 2, False, True),
    (64, 32, 21, 3, 2, 4, True, False),
    (30, 8, 37, 1, 2, 1, True, False), (30, 8, 37, 2, 1, 4, False, True), (30, 8, 37, 3, 2, 2, True, True),
    (30, 8, 37, 2, 2, 4, False, False),
]
# Worst max|d| / max|ref| of the float32 mode against the float64 mode over VALUE_CASES, measured on the CPU
# (test_misi_host.py re-measures it), rounded up; the kernels get 16 x that.  9.160e-06 at 1022/256/9, N = 2, G = 2, K = 2 with
# a phase per source; most cases stay below 1e-06.  The passes that follow a bin with a small |Z| carry its badly conditioned
# direction on under a magnitude that does not shrink with it, which is why the worst case is several times the median.
F32_WORST = 9.2e-06
BOUND = 16 * F32_WORST


def value_inputs(n_fft, hop, F, N, G, per_source, reflect, seed=0):
    """fp32 inputs of a value case: coloured Gaussian noise sources (white noise plus half its one-sample shift, times 0.1),
    mixture = their sum, A = random ratio masks times |X|; the start phase is the mixture's, or every source's own.
    -> (mix [G,L], A [N,G,bins,F], phase [G,bins,F] | [N,G,bins,F]), L = hop * (F - 1)."""
    g = torch.Generator().manual_seed(1000 * n_fft + 10 * F + N + 100 * G + seed)
    L = hop * (F - 1)
    w = torch.randn(N, G, L + 1, generator=g, dtype=torch.float64)
    src = (0.1 * (w[..., 1:] + 0.5 * w[..., :-1])).float()
    mix = src.double().sum(0).float()
    X = stft(mix, n_fft, hop, reflect)
    r = torch.rand(N, G, *X.shape[1:], generator=g, dtype=torch.float64) + 1e-3
    A = (r / r.sum(0, keepdim=True) * X.abs()[None]).float()
    Z = stft(src, n_fft, hop, reflect) if per_source else X
    return mix.contiguous(), A.contiguous(), torch.atan2(Z.imag, Z.real).float().contiguous()


# ---------------------------------------------------------------------------------------------------------------------
# the SDR scene: two harmonic sources with vibrato and a tremolo each plus weak noise, 63 hops at 11 025 Hz
# ---------------------------------------------------------------------------------------------------------------------
SCENE_N_FFT, SCENE_HOP, SCENE_RATE = 1022, 256, 11025


def sdr_scene():
    """-> {"src" f64 [2,L], "mix" f32 [1,L], "A" f32 [2,1,bins,F] (oracle magnitudes), "phase" f32 [1,bins,F] (mixture)}."""
    L = 63 * SCENE_HOP
    t = torch.arange(L, dtype=torch.float64) / SCENE_RATE
    g = torch.Generator().manual_seed(5)
    src = []
    for n, (f0, v) in enumerate(((220.0, 3.0), (331.0, 5.0))):
        th = 2 * math.pi * f0 * t + v * torch.sin(2 * math.pi * 5 * t)
        env = 0.5 + 0.5 * torch.sin(2 * math.pi * (1.3 + n) * t)
        src.append(0.2 * env * sum(torch.sin(h * th) / h for h in range(1, 6)) + 0.01 * torch.randn(L, generator=g, dtype=torch.float64))
    src = torch.stack(src).float().double()                      # the sources as fp32 numbers
    mix = src.sum(0, keepdim=True).float()
    X = stft(mix, SCENE_N_FFT, SCENE_HOP)
    A = stft(src, SCENE_N_FFT, SCENE_HOP).abs()[:, None].float()
    return {"src": src, "mix": mix, "A": A.contiguous(), "phase": torch.atan2(X.imag, X.real).float().contiguous()}


def mean_sdr(est, src):
    """Mean over the sources of 10 log10(|s|^2 / |s - est|^2); est [N,L] or [N,1,L]."""
    est = torch.as_tensor(est).double().reshape(src.shape)
    return float((10 * torch.log10((src ** 2).sum(-1) / ((src - est) ** 2).sum(-1))).mean())


def scene_sdr(sc, K, dtype=torch.float64):
    return mean_sdr(misi(sc["mix"], sc["A"], sc["phase"], K, SCENE_N_FFT, SCENE_HOP, True, dtype)["wav"], sc["src"])
