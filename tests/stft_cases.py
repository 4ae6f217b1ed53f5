"""The case table of tests/test_gpu_stft.py (and of the float32 control and the mutants of tests/test_stftref.py): every
geometry edge of avsep_stft_mag / avsep_istft (csrc/stft.hip) and of the two conv launches behind them, each row with the path
it must take.  The inputs are built here from a seed; the float64 references (tests/stftref.py) are computed once per row and
shared.

Forward input: randn * 0.3 under an exponential decay of 80 dB over the clip (a loud start, a quiet end: a bound relative to the
peak would let the last frames be anything), three hops of exact zeros from L // 3, row 1 all zero (R > 1), row 2 times 1e-3
(R > 2).  The zero row must come out exactly zero, the frames inside the zero stretch too.

The path: stft_fast() in csrc/stft.hip sends 3 hop < n_fft <= 4 hop, hop % 4 == 0, hop <= 1024, frames >= 32 to the 1x4 conv on
the halo kernel (tiles of 4 rows x 32 frames x 128 channels), everything else to the im2col kernel as a Cin = 1, 1 x n_fft,
stride-hop conv; avsep_stft_workspace_bytes has one formula per path, and a row states which it must see.

The figures behind "gpu" are the worst |error| / bound of the row on an MI355X, magnitude / phase gate (inverse rows: input a /
input b), those behind "f32" the same of the float32 numpy control (tests/test_stftref.py).  They are reported, not gated."""
import functools

import numpy as np
import torch

import stftref

IGEMM, HALO = "igemm_kernel<fwd>", "conv3x3_kernel"

# id: (n_fft, hop, R, L, pad modes, path, conv family of the GEMM)
FORWARD = {
    # fast path
    "F1": (1022, 256, 5, 256 * 31 + 100, ("reflect",), "fast", HALO),    # frames = 32, the guard's lower edge; ragged row tile | gpu 0.0102 / 0.0106, f32 0.0133 / 0.0133
    "F2": (1022, 256, 4, 256 * 32, ("reflect", "constant"), "fast", HALO),  # L % hop == 0: frames = 33 (ragged frame tile), last frame all padding | gpu 0.0093 / 0.0093, f32 0.0125 / 0.0128
    "F3": (1024, 256, 3, 8192 + 17, ("constant",), "fast", HALO),        # n_fft == 4 hop, no zero taps; 1026 channels, last M tile 2 rows | gpu 0.0113 / 0.0116, f32 0.0114 / 0.0124
    "F4": (2048, 512, 2, 512 * 31 + 7, ("reflect",), "fast", HALO),      # pad kernel asks for 65 664 B of LDS; 2050 channels | gpu 0.0100 / 0.0108, f32 0.0160 / 0.0161
    "F5": (4096, 1024, 1, 1024 * 31, ("reflect",), "fast", HALO),        # hop == 1024, the guard's upper edge; 131 200 B of LDS | gpu 0.0105 / 0.0113, f32 0.0033 / 0.0034
    "F6": (200, 64, 3, 64 * 40 + 63, ("reflect",), "fast", HALO),        # 56 zero taps; 202 channels | gpu 0.0082 / 0.0085, f32 0.0095 / 0.0105
    "F7": (16, 4, 9, 200, ("reflect",), "fast", HALO),                   # 4 input channels (one K-tile); three row tiles, the last ragged | gpu 0.0073 / 0.0105, f32 0.0067 / 0.0104
    # fallback
    "B1": (1022, 256, 5, 256 * 31 - 1, ("reflect",), "fallback", IGEMM),  # frames = 31: the other side of F1's guard | gpu 0.0118 / 0.0122, f32 0.0118 / 0.0120
    "B2": (766, 254, 2, 254 * 40, ("reflect",), "fallback", IGEMM),      # hop % 4 == 2: the other side of the alignment guard | gpu 0.0090 / 0.0092, f32 0.0090 / 0.0090
    "B3": (1024, 128, 3, 3000, ("reflect",), "fallback", IGEMM),         # n_fft = 8 hop | gpu 0.0145 / 0.0155, f32 0.0145 / 0.0155
    "B4": (256, 192, 2, 192 * 35 + 5, ("reflect",), "fallback", IGEMM),  # n_fft < 2 hop; frames wholly inside the zero stretch | gpu 0.0079 / 0.0080, f32 0.0079 / 0.0079
    "B5": (1022, 256, 2, 512, ("reflect",), "fallback", IGEMM),          # L = n_fft / 2 + 1, the shortest the API takes; frames = 3 | gpu 0.0085 / 0.0089, f32 0.0097 / 0.0097
    "B6": (512, 128, 3, 128 * 19 + 3, ("reflect",), "fallback", IGEMM),  # n_fft == 4 hop but 20 frames | gpu 0.0126 / 0.0125, f32 0.0116 / 0.0115
}
FORWARD_ROWS = [(name, mode) for name, row in FORWARD.items() for mode in row[4]]

# id: (n_fft, hop, R, frames, conv family of the 1x1 conv [R, 2 bins, 1, frames] -> [R, n_fft, 1, frames]).  Each row runs on a
# consistent spectrum (a) and on an arbitrary one (b).
INVERSE = {
    "I1": (1022, 256, 5, 2, IGEMM),      # f_lo / f_hi clip to two frames everywhere | gpu 0.0178 / 0.0079, f32 0.0061 / 0.0024
    "I2": (1022, 256, 5, 5, IGEMM), # gpu 0.0080 / 0.0124, f32 0.0044 / 0.0041
    "I3": (1022, 256, 5, 33, IGEMM),     # one column past a 32-column tile | gpu 0.0098 / 0.0077, f32 0.0049 / 0.0033
    "I4": (256, 128, 3, 2, IGEMM),       # 50 % overlap: one or two frames per sample | gpu 0.0107 / 0.0063, f32 0.0107 / 0.0047
    "I5": (256, 128, 3, 5, IGEMM), # gpu 0.0061 / 0.0086, f32 0.0058 / 0.0070
    "I6": (256, 128, 3, 33, IGEMM), # gpu 0.0136 / 0.0107, f32 0.0104 / 0.0058
    "I7": (1024, 256, 3, 5, IGEMM),      # K = 1026: ragged last K-tile | gpu 0.0102 / 0.0101, f32 0.0081 / 0.0035
    "I8": (1024, 256, 3, 33, IGEMM), # gpu 0.0091 / 0.0066, f32 0.0038 / 0.0030
    "I9": (2048, 512, 3, 5, IGEMM),      # K = 2050 | gpu 0.0101 / 0.0088, f32 0.0051 / 0.0027
    "I10": (254, 128, 3, 33, IGEMM),     # n_fft just under 2 hop: one or two frames per sample | gpu 0.0198 / 0.0110, f32 0.0081 / 0.0063
    "I11": (200, 64, 3, 33, IGEMM),      # Cout = 200 = 128 + 72 | gpu 0.0115 / 0.0067, f32 0.0059 / 0.0062
    "I12": (16, 4, 3, 33, IGEMM),        # K = 18, Cout = 16 | gpu 0.0106 / 0.0048, f32 0.0077 / 0.0070
}
INVERSE_ROWS = [(name, kind) for name in INVERSE for kind in "ab"]
# avsep_istft called directly with a shorter output (out_len < hop * (frames - 1)) into a NaN-filled buffer 8 elements longer
SHORT_ROWS = [(name, cut) for name in ("I3", "I11") for cut in ("minus37", "one")]
GUARD = 8


def short_len(name, cut):
    n_fft, hop, R, frames, _ = INVERSE[name]
    return hop * (frames - 1) - 37 if cut == "minus37" else 1


def _seed(name):
    return 7919 * (ord(name[0]) - 60) + int(name[1:])


def envelope(n):
    """80 dB of exponential decay over n samples (1 -> 1e-4)."""
    return 10.0 ** (-4.0 * np.arange(n, dtype=np.float64) / max(n - 1, 1))


def signal(seed, R, L, hop):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(R, L, generator=g, dtype=torch.float64).numpy() * 0.3 * envelope(L)[None, :]
    x[:, L // 3:L // 3 + 3 * hop] = 0.0
    if R > 1:
        x[1] = 0.0
    if R > 2:
        x[2] *= 1e-3
    return np.ascontiguousarray(x.astype(np.float32))


@functools.lru_cache(maxsize=None)
def forward_input(name):
    n_fft, hop, R, L = FORWARD[name][:4]
    return signal(_seed(name), R, L, hop)


@functools.lru_cache(maxsize=None)
def forward_ref(name, mode):
    n_fft, hop = FORWARD[name][:2]
    return stftref.stft(forward_input(name), n_fft, hop, mode == "reflect")


@functools.lru_cache(maxsize=None)
def inverse_input(name, kind):
    """-> mag, phase float32 [R, bins, frames].  a: the STFT of an enveloped signal of hop * (frames - 1) + hop / 2 samples
    (reflect padding where the clip is longer than the padding, zeros otherwise).  b: |randn| under the 80 dB decay along the
    frames with frames 1 and 2 all zero (frame 1 only when there are two) and row 1 all zero, phases uniform in (-3 pi, 3 pi),
    none of them zero at DC and Nyquist."""
    n_fft, hop, R, frames = INVERSE[name][:4]
    bins = stftref.bins_of(n_fft)
    if kind == "a":
        L = hop * (frames - 1) + hop // 2
        re, im, _, _ = stftref.stft(signal(_seed(name), R, L, hop), n_fft, hop, L > n_fft // 2)
        return np.hypot(re, im).astype(np.float32), np.arctan2(im, re).astype(np.float32)
    g = torch.Generator().manual_seed(_seed(name) + 1)
    env = envelope(max(frames, 2) * 8)[::8][:frames]
    mag = np.abs(torch.randn(R, bins, frames, generator=g, dtype=torch.float64).numpy()) * env[None, None, :]
    mag[:, :, 1:min(3, frames)] = 0.0
    mag[1] = 0.0
    phase = (torch.rand(R, bins, frames, generator=g, dtype=torch.float64).numpy() * 2.0 - 1.0) * 3.0 * np.pi
    edge = phase[:, (0, n_fft // 2), :]
    phase[:, (0, n_fft // 2), :] = np.where(np.abs(np.sin(edge)) < 0.1, edge + 0.5, edge)
    return np.ascontiguousarray(mag.astype(np.float32)), np.ascontiguousarray(phase.astype(np.float32))


@functools.lru_cache(maxsize=None)
def inverse_ref(name, kind, out_len=None):
    n_fft, hop, R, frames = INVERSE[name][:4]
    mag, phase = inverse_input(name, kind)
    return stftref.istft(mag, phase, n_fft, hop, hop * (frames - 1) if out_len is None else out_len)


def workspace_bytes(R, L, n_fft, hop, path):
    """The two formulas of avsep_stft_workspace_bytes."""
    bins, frames = stftref.bins_of(n_fft), 1 + L // hop
    spec = R * 2 * bins * frames
    if path == "fast":
        return (hop * R * (frames + 3) + hop * 4 * (-(-2 * bins // 128) * 128) + spec) * 4
    return (R * (L + n_fft) + spec) * 4
