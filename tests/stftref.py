"""float64 reference of the STFT / iSTFT (csrc/stft.hip) with the magnitude bound of every output element, and the gates of
tests/test_gpu_stft.py.  Written from the librosa algorithm as oracle/stft.py states it (centred frames, periodic Hann window,
one-sided DFT; windowed inverse DFT, overlap-add, division by the window-sum-square, centre trim), as plain matrix products in
numpy float64 -- no FFT, nothing taken from the kernels.  tests/test_stftref.py holds it against torch.stft / torch.istft in
float64 and against oracle.stft.

Next to every value the reference returns the same linear map applied to absolute values (tests/convref.py calls it absref):
an fp32 evaluation in any summation order stays within  terms * 2^-24 * absref  of the exact value, whatever cancels.

The gates.  One tau for every element, not fitted to the kernels: the project's ceiling for direct-form fp32 kernels,
CEIL_DIRECT = 2e-5 of tests/convref.py (the fp32 worst case at K = 4096 terms is K * 2^-24 = 2.4e-4; the
direct-form ratios measured there stay below 2e-6 up to K = 8192; the float32 numpy control of tests/test_stftref.py reaches
3.2e-7, the kernels 4.0e-7 on an MI355X).  With z = re + i im and g = tau * hypot(a_re, a_im):
    magnitude   |mag - |z||               <= g + 2^-22 |z|     (two squares, an add and sqrtf)
    phase       |mag e^{i phase} - z|     <= g + 2^-21 |z|     (one fp32 ulp at pi is 2^-22, another 2^-22 for atan2f; the
                                                                ROCm headers here state no bound for atan2f, so this one stays)
    inverse     |wav - wav_ref|           <= tau * absref
    zero        where the bound is exactly 0 (a silent frame, a silent row) the output is exactly 0.
The phase is judged through the complex value, so a bin with |z| ~ 0 needs no exclusion; no element is left out of any gate.
A gate returns the worst ratio |error| / bound (inf for a non-zero output under a zero bound, nan counts as inf) and where."""
import functools

import numpy as np

TAU = 2e-5
ULP_MAG = 2.0 ** -22
ULP_PHASE = 2.0 ** -21
TINY = float(np.finfo(np.float32).tiny)


def bins_of(n_fft):
    return n_fft // 2 + 1


@functools.lru_cache(maxsize=None)
def window(n_fft):
    """Periodic Hann (scipy.signal.get_window("hann", n_fft, fftbins=True)); read-only, shared."""
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft, dtype=np.float64) / n_fft)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def dft_angles(n_fft):
    """2 pi k n / n_fft for k < bins, n < n_fft, with k n reduced modulo n_fft in integers first -> [bins, n_fft]; read-only."""
    k = np.arange(bins_of(n_fft), dtype=np.int64)[:, None]
    n = np.arange(n_fft, dtype=np.int64)[None, :]
    a = 2.0 * np.pi * ((k * n) % n_fft).astype(np.float64) / n_fft
    a.setflags(write=False)
    return a


def frame(x, n_fft, hop, reflect):
    """x [R, L] float64 -> centred frames [R, n_fft, 1 + L // hop]."""
    pad = n_fft // 2
    xp = np.pad(x, ((0, 0), (pad, pad)), mode="reflect" if reflect else "constant")
    frames = 1 + x.shape[1] // hop
    idx = np.arange(n_fft)[:, None] + hop * np.arange(frames)[None, :]
    return xp[:, idx]


def stft(wav_f32, n_fft, hop, reflect):
    """wav [R, L] float32 -> re, im, a_re, a_im, each float64 [R, bins, frames]."""
    wav_f32 = np.asarray(wav_f32)
    assert wav_f32.dtype == np.float32 and wav_f32.ndim == 2
    fr = frame(wav_f32.astype(np.float64), n_fft, hop, reflect)
    ang, win = dft_angles(n_fft), window(n_fft)
    c, s = win * np.cos(ang), -win * np.sin(ang)                      # [bins, n_fft]
    return c @ fr, s @ fr, np.abs(c) @ np.abs(fr), np.abs(s) @ np.abs(fr)


def window_sum_square(n_fft, hop, frames):
    w2 = window(n_fft) ** 2
    wss = np.zeros(n_fft + hop * (frames - 1))
    for f in range(frames):
        wss[f * hop:f * hop + n_fft] += w2
    return wss


def overlap_add(td, hop):
    """td [R, n_fft, frames] -> [R, n_fft + hop * (frames - 1)], frames added in ascending order."""
    R, n_fft, frames = td.shape
    y = np.zeros((R, n_fft + hop * (frames - 1)), dtype=td.dtype)
    for f in range(frames):
        y[:, f * hop:f * hop + n_fft] += td[:, :, f]
    return y


def istft(mag_f32, phase_f32, n_fft, hop, out_len):
    """mag, phase [R, bins, frames] float32 -> wav, absref, each float64 [R, out_len]."""
    mag_f32, phase_f32 = np.asarray(mag_f32), np.asarray(phase_f32)
    assert mag_f32.dtype == np.float32 and phase_f32.dtype == np.float32 and mag_f32.shape == phase_f32.shape
    R, bins, frames = mag_f32.shape
    assert bins == bins_of(n_fft) and 0 < out_len <= hop * (frames - 1)
    mag, ph = mag_f32.astype(np.float64), phase_f32.astype(np.float64)
    re, im = mag * np.cos(ph), mag * np.sin(ph)
    im[:, 0] = 0.0                                                    # irfft: the imaginary part of DC and Nyquist is ignored
    im[:, n_fft // 2] = 0.0
    ang, win = dft_angles(n_fft), window(n_fft)
    ck = np.full(bins, 2.0)
    ck[0] = ck[n_fft // 2] = 1.0
    bc = (win[None, :] * ck[:, None] * np.cos(ang) / n_fft).T         # [n_fft, bins]
    bs = (-win[None, :] * ck[:, None] * np.sin(ang) / n_fft).T
    td = bc @ re + bs @ im                                            # [R, n_fft, frames], synthesis window included
    ta = np.abs(bc) @ np.abs(re) + np.abs(bs) @ np.abs(im)
    wss = window_sum_square(n_fft, hop, frames)
    ok = wss > TINY
    y, ya = overlap_add(td, hop), overlap_add(ta, hop)
    y[:, ok] /= wss[ok]
    ya[:, ok] /= wss[ok]
    pad = n_fft // 2
    return y[:, pad:pad + out_len], ya[:, pad:pad + out_len]


# ---------------------------------------------------------------------------------------------------------------------
# gates
# ---------------------------------------------------------------------------------------------------------------------
def worst(err, bound):
    """-> (worst |err| / bound, its index).  Under a zero bound the error must be zero: anything else, and any nan, is inf."""
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    assert err.shape == bound.shape and err.size
    safe = np.where(bound > 0, bound, 1.0)
    ratio = np.where(bound > 0, err / safe, np.where(err == 0, 0.0, np.inf))
    ratio = np.where(np.isfinite(err), ratio, np.inf)
    at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return float(ratio[at]), tuple(int(i) for i in at)


def forward_bound(ref):
    re, im, a_re, a_im = ref
    return TAU * np.hypot(a_re, a_im), np.hypot(re, im)


def gate_mag(mag, ref):
    g, az = forward_bound(ref)
    return worst(np.abs(np.asarray(mag, np.float64) - az), g + ULP_MAG * az)


def gate_phase(mag, phase, ref):
    g, az = forward_bound(ref)
    mag, phase = np.asarray(mag, np.float64), np.asarray(phase, np.float64)
    z = mag * np.cos(phase) + 1j * (mag * np.sin(phase))
    return worst(np.abs(z - (ref[0] + 1j * ref[1])), g + ULP_PHASE * az)


def gate_inverse(wav, ref):
    y, ya = ref
    return worst(np.abs(np.asarray(wav, np.float64) - y), TAU * ya)
