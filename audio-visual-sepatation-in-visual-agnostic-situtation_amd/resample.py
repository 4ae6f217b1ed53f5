"""Sample-rate conversion on the GPU: WAV files at any rate in, sources at the file's own rate out.

A rational polyphase FIR resampler with the filter ``scipy.signal.resample_poly`` uses by default (the training loader's
choice, dataset.read_wav_segment, which stays on the CPU for its GPU-free workers).  The filter is designed here in
float64 with NumPy alone, rounded once to f32 and handed to ``avsep_resample_poly`` (include/avsep.h, csrc/resample.hip) as
a polyphase table cached per (up, down, device).  The kernels read a file's frames directly (down-mix and conversion fused
into their staging) and write them directly, so a long recording never exists as an f32 copy at the file's rate on the
host.  The ``*_frames`` functions take and give frames as the bytes they are in the file (wavio.read_frames /
write_frames), in any of the sample formats of include/avsep.h (s16 / s24 / s32 PCM and f32 in, s16 / s24 / f32 out);
``resample_pcm`` / ``split_pcm`` / ``join_pcm`` are the same calls for frames held as an int16 tensor [L, C].
"""
import math

import numpy as np
import torch

from . import kernels as K
from . import lib
from .lib import AvsepError

MAX_RATIO = 1280       # largest up / down after reduction: 8 ... 96 kHz to and from 11 025 Hz (441/1280, 147/1280)
MAX_CHANNELS = 256
MAX_KEPT_CHANNELS = K.RESAMPLE_MAX_KEPT_CHANNELS      # split_pcm / join_pcm: up to 7.1

_tables = {}


def rational(rate_in, rate_out):
    """-> (up, down), the reduced ratio rate_out / rate_in.  Rates are positive integers (Hz)."""
    if int(rate_in) != rate_in or int(rate_out) != rate_out or rate_in < 1 or rate_out < 1:
        raise ValueError(f"sample rates are positive integers, got {rate_in!r} and {rate_out!r}")
    rate_in, rate_out = int(rate_in), int(rate_out)
    g = math.gcd(rate_in, rate_out)
    return rate_out // g, rate_in // g


def check_rates(rate_in, rate_out):
    """rational(), refusing a ratio the kernel does not take: AvsepError that names both rates."""
    up, down = rational(rate_in, rate_out)
    if max(up, down) > MAX_RATIO:
        raise AvsepError(f"{rate_in} Hz -> {rate_out} Hz reduces to {up}/{down}: the resampler takes ratios whose terms are "
                         f"at most {MAX_RATIO} (8, 16, 22.05, 32, 44.1, 48, 88.2 and 96 kHz to and from 11 025 Hz)")
    return up, down


def design_filter(up, down):
    """float64 [20*max(up,down)+1]: up * firwin(M, 1/m, window=('kaiser', 5.0)), the filter of scipy.signal.resample_poly."""
    m = max(int(up), int(down))
    half = 10 * m
    M = 2 * half + 1
    w = np.sinc((np.arange(M, dtype=np.float64) - half) / m) / m * np.kaiser(M, 5.0)
    return w / w.sum() * int(up)


def out_length(L, up, down):
    """ceil(L * up / down)."""
    return -(-int(L) * int(up) // int(down))


def filter_table(up, down, device):
    """The f32 polyphase table [T, up] of include/avsep.h on ``device``, T = ceil(M / up): column t holds the phase of the
    outputs j = t (mod up), ho[i][t] = h[(t*down + half) % up + i*up], zero past the filter's end.  Built once per
    (up, down, device).  For up = down = 1 the filter is the exact
    unit impulse (sinc vanishes at the non-zero integers; the 1e-17 residue of sin(k*pi) in float64 is dropped), so that equal
    rates give the input's own bits."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (int(up), int(down), str(device))
    t = _tables.get(key)
    if t is None:
        up, down = key[:2]
        h = design_filter(up, down)
        if up == 1 and down == 1:
            h = (np.arange(h.size) == h.size // 2).astype(np.float64)
        T = -(-h.size // up)
        full = np.zeros(T * up, dtype=np.float64)
        full[:h.size] = h
        phase = (np.arange(up, dtype=np.int64) * down + (h.size - 1) // 2) % up
        ho = np.ascontiguousarray(full.reshape(T, up)[:, phase]).astype(np.float32)
        t = _tables[key] = torch.from_numpy(ho).to(device)
    return t


def _check_length(L, up, down):
    if L < 1 or L >= 2 ** 31 or out_length(L, up, down) >= 2 ** 31:
        raise AvsepError(f"resampling takes 1 <= L and L, ceil(L*{up}/{down}) < 2^31 samples, got L={L}")


def resample(x, rate_in, rate_out, out_s16=False):
    """x: f32 [L] or [B,L] on the GPU -> the same rows at rate_out, f32 or (out_s16) int16 = clip(rint(y * 32768)).
    Equal rates return x itself for f32."""
    lib.require_gpu(x)
    if x.dtype != torch.float32 or x.dim() not in (1, 2):
        raise AvsepError(f"resample takes a float32 waveform [L] or [B,L], got {x.dtype} {tuple(x.shape)}")
    up, down = check_rates(rate_in, rate_out)
    if up == down and not out_s16:
        return x
    _check_length(x.shape[-1], up, down)
    rows = x.contiguous() if x.dim() == 2 else x.contiguous()[None]
    y = K.resample_poly(rows, filter_table(up, down, x.device), up, down, out_fmt="s16" if out_s16 else "f32")
    return y if x.dim() == 2 else y[0]


def band_extend(stems, low, file_rows, gains, rate_model, rate_file, hop):
    """Full-band stems (include/avsep.h, avsep_band_extend): stems f32 [N,G,Lm] at ``rate_model``, low f32 [G,Ll] the
    model-rate mixture rows they were made from (Ll >= Lm), file_rows f32 [G,Lf] the same rows at ``rate_file``, gains f32
    [N,G,F] (kernels.band_gains), hop the STFT hop -> f32 [N,G,ceil(Lm*up/down)] at ``rate_file``:
    resample(stems) + gain * (file_rows - resample(low)).  The resampler is zero-phase, so the bracket is exactly what the
    model never heard; with gains of 0 the result is resample(stems), bit for bit."""
    up, down = check_rates(rate_model, rate_file)
    if up <= down:
        raise AvsepError(f"band_extend adds what a file holds above the model's band: the file's rate ({rate_file} Hz) has to "
                         f"exceed the model's ({rate_model} Hz)")
    if not torch.is_tensor(stems) or stems.dim() != 3:
        raise AvsepError(f"band_extend takes stems as float32 [N,G,Lm], got {lib.got(stems)}")
    lib.require_gpu(stems)
    _check_length(stems.shape[-1], up, down)
    return K.band_extend(stems, low, file_rows, gains, filter_table(up, down, stems.device), up, down, hop)


# ---------------------------------------------------------------------------------------------------------------------
# a file's frames as bytes, in any sample format (wavio.py)
# ---------------------------------------------------------------------------------------------------------------------
def _raw_length(what, raw, fmt, C, most):
    """The frame count of raw uint8 [L*C*bytes]; AvsepError for another format, tensor or channel count."""
    if fmt not in K.SAMPLE_FORMATS:
        raise AvsepError(f"{what} takes the sample formats {', '.join(K.SAMPLE_FORMATS)}, got {fmt!r}")
    if int(C) != C or not 1 <= C <= most:
        raise AvsepError(f"{what} takes 1 to {most} channels, got {C!r}")
    return K.raw_frames(what, raw, int(C), K.SAMPLE_FORMATS[fmt][1])


def resample_frames(raw, fmt, C, rate_in, rate_out):
    """raw: a file's frames, uint8 [L*C*bytes] on the GPU at any byte address, fmt 's16' | 's24' | 's32' | 'f32', 1 <= C <= 256
    -> f32 mono [Lout] at rate_out: the correctly rounded mean of the channels (include/avsep.h), resampled, in one kernel.
    Equal rates go through the same kernel with the unit-impulse filter: the converted mono signal."""
    L = _raw_length("resample_frames", raw, fmt, C, MAX_CHANNELS)
    up, down = check_rates(rate_in, rate_out)
    _check_length(L, up, down)
    lib.require_gpu(raw)
    return K.resample_poly(raw, filter_table(up, down, raw.device), up, down, int(C), fmt, "f32")[0]


def split_frames(raw, fmt, C, rate_in, rate_out):
    """raw as for resample_frames, 1 <= C <= 8 -> f32 [1+C, Lout] at rate_out in one kernel: row 0 is resample_frames'
    down-mix (the network's input), row 1+c is channel c through the same filter."""
    L = _raw_length("split_frames", raw, fmt, C, MAX_KEPT_CHANNELS)
    up, down = check_rates(rate_in, rate_out)
    _check_length(L, up, down)
    lib.require_gpu(raw)
    return K.resample_split(raw, filter_table(up, down, raw.device), up, down, int(C), fmt)


def join_frames(x, rate_in, rate_out, fmt, out=None):
    """x: f32 [C,L] on the GPU, 1 <= C <= 8 -> uint8 [Lout*C*bytes] at rate_out: the frames of a WAV file in fmt 's16' | 's24' |
    'f32', in one kernel: s16 clip(rint(v * 2^15)) and s24 clip(rint(v * 2^23)) of the same f32 value v, f32 its bits.  Equal
    rates go through the kernel with the unit-impulse filter: only the rounding.  ``out``: a uint8 view of that size at any
    byte address, filled and returned."""
    if fmt not in K.SAMPLE_OUT_FORMATS:
        raise AvsepError(f"join_frames writes the sample formats {', '.join(K.SAMPLE_OUT_FORMATS)}, got {fmt!r}")
    if not torch.is_tensor(x) or x.dtype != torch.float32 or x.dim() != 2:
        raise AvsepError(f"join_frames takes float32 [C,L], got {lib.got(x)}")
    if not 1 <= x.shape[0] <= MAX_KEPT_CHANNELS:
        raise AvsepError(f"join_frames writes 1 to {MAX_KEPT_CHANNELS} channels (up to 7.1), got {x.shape[0]}")
    up, down = check_rates(rate_in, rate_out)
    _check_length(x.shape[1], up, down)
    lib.require_gpu(x)
    return K.resample_join(x, filter_table(up, down, x.device), up, down, fmt, out=out)


# ---------------------------------------------------------------------------------------------------------------------
# the same three for 16-bit frames held as an int16 tensor [L, C] (what separate.read_wav_pcm returns)
# ---------------------------------------------------------------------------------------------------------------------
def _pcm_bytes(pcm):
    return pcm.contiguous().view(torch.uint8).reshape(-1)


def resample_pcm(pcm, rate_in, rate_out):
    """pcm: interleaved int16 [L,C] on the GPU (a WAV file's frames) -> f32 mono [Lout] at rate_out: resample_frames of its
    bytes as 's16'.  At equal rates, bit for bit separate.read_wav's array."""
    lib.require_gpu(pcm)
    if pcm.dtype != torch.int16 or pcm.dim() != 2 or not 1 <= pcm.shape[1] <= MAX_CHANNELS:
        raise AvsepError(f"resample_pcm takes interleaved int16 [L,C] with 1 <= C <= {MAX_CHANNELS}, got {pcm.dtype} {tuple(pcm.shape)}")
    return resample_frames(_pcm_bytes(pcm), "s16", pcm.shape[1], rate_in, rate_out)


def split_pcm(pcm, rate_in, rate_out):
    """pcm: interleaved int16 [L,C] on the GPU, 1 <= C <= 8 -> f32 [1+C, Lout] at rate_out: split_frames of its bytes as
    's16'; row 0 is resample_pcm's down-mix, row 1+c is channel c over 32768 through the same filter."""
    if pcm.dtype != torch.int16 or pcm.dim() != 2:
        raise AvsepError(f"split_pcm takes interleaved int16 [L,C], got {pcm.dtype} {tuple(pcm.shape)}")
    if not 1 <= pcm.shape[1] <= MAX_KEPT_CHANNELS:
        raise AvsepError(f"split_pcm keeps 1 to {MAX_KEPT_CHANNELS} channels (up to 7.1), got {pcm.shape[1]}")
    return split_frames(_pcm_bytes(pcm), "s16", pcm.shape[1], rate_in, rate_out)


def join_pcm(x, rate_in, rate_out):
    """x: f32 [C,L] on the GPU, 1 <= C <= 8 -> interleaved int16 [Lout,C] at rate_out: join_frames(.., 's16') as a typed
    tensor; column c is resample(x[c], .., out_s16=True)."""
    if not torch.is_tensor(x) or x.dtype != torch.float32 or x.dim() != 2:
        raise AvsepError(f"join_pcm takes float32 [C,L], got {lib.got(x)}")
    if not 1 <= x.shape[0] <= MAX_KEPT_CHANNELS:
        raise AvsepError(f"join_pcm writes 1 to {MAX_KEPT_CHANNELS} channels (up to 7.1), got {x.shape[0]}")
    return join_frames(x, rate_in, rate_out, "s16").view(torch.int16).reshape(-1, x.shape[0])
