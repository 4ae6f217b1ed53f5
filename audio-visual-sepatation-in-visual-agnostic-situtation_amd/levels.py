"""How loud a stem is and whether it will clip: ITU-R BS.1770-4 loudness and true peak, and one peak-safe gain for a run.

The stems lie on the GPU just before they are encoded, so both measurements that need every sample are taken there
(``avsep_loudness_energies`` and ``avsep_true_peak``, include/avsep.h, csrc/levels.hip): the K-weighted energy of every
100 ms sub-block and the oversampled peak of every row.  What is left is a few thousand numbers per row: the 400 ms blocks
(four sub-blocks, 75 % overlap), the absolute and the relative gate and the 3 s short-term window are float64 NumPy on the
host (``loudness_from_energies``), because a gate is a data-dependent selection over a handful of values, not a hot path.

    measure(x, rate)          -> integrated / momentary-max / short-term-max LUFS, true and sample peak, the energies
    output_gain(...)          -> the ONE gain that brings a run to a loudness and keeps its largest true peak under a ceiling

CLI: ``python -m avsep_amd.levels a.wav b.wav ... [--json out.json]`` prints the five figures of every file (any format and
rate wavio.py reads, up to eight channels).
"""
import json
import math

import numpy as np
import torch

from . import kernels as K
from . import lib
from . import resample as R
from .lib import AvsepError

MIN_RATE, MAX_RATE = 8000, 192000
ABSOLUTE_GATE = -70.0          # LUFS
RELATIVE_GATE = -10.0          # LU below the absolutely gated loudness
BLOCK_SUBS = 4                 # a 400 ms gating block is four sub-blocks: 75 % overlap at a step of one
SHORT_TERM_SUBS = 30           # 3 s

_taps = {}


def _check_rate(rate):
    if isinstance(rate, bool) or not isinstance(rate, (int, np.integer)) or not MIN_RATE <= rate <= MAX_RATE:
        raise AvsepError(f"levels are measured at integer sample rates in [{MIN_RATE}, {MAX_RATE}] Hz, got {rate!r}")
    return int(rate)


def k_weighting(rate):
    """-> float64 [2, 6], scipy's sos layout (b0 b1 b2 1 a1 a2): the shelf and the high-pass of BS.1770's K-weighting at
    ``rate``, from the analogue prototypes behind the standard's 48 kHz table (which this reproduces to 1e-15)."""
    rate = _check_rate(rate)
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    Kt = math.tan(math.pi * f0 / rate)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + Kt / Q + Kt * Kt
    shelf = [(Vh + Vb * Kt / Q + Kt * Kt) / a0, 2.0 * (Kt * Kt - Vh) / a0, (Vh - Vb * Kt / Q + Kt * Kt) / a0,
             1.0, 2.0 * (Kt * Kt - 1.0) / a0, (1.0 - Kt / Q + Kt * Kt) / a0]
    f0, Q = 38.13547087602444, 0.5003270373238773
    Kt = math.tan(math.pi * f0 / rate)
    a0 = 1.0 + Kt / Q + Kt * Kt
    highpass = [1.0, -2.0, 1.0, 1.0, 2.0 * (Kt * Kt - 1.0) / a0, (1.0 - Kt / Q + Kt * Kt) / a0]
    return np.array([shelf, highpass], dtype=np.float64)


def peak_filter(rate):
    """-> (os, g): the oversampling factor of the true-peak meter at ``rate`` (4 below 96 kHz, 2 below 192 kHz, else 1) and
    its interpolation filter, float64 [20*os + 1]: the resampler's (resample.design_filter); the exact unit impulse for 1."""
    rate = _check_rate(rate)
    os = 4 if rate < 96000 else 2 if rate < 192000 else 1
    g = R.design_filter(os, 1)
    if os == 1:
        g = (np.arange(g.size) == g.size // 2).astype(np.float64)
    return os, g


def peak_table(rate, device):
    """The polyphase table f64 [21, os] avsep_true_peak takes, on ``device``: row i holds g[i*os : (i+1)*os], zero past g."""
    os, g = peak_filter(rate)
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (os, str(device))
    t = _taps.get(key)
    if t is None:
        full = np.zeros(K.TRUE_PEAK_TAPS * os, dtype=np.float64)
        full[:g.size] = g
        t = _taps[key] = torch.from_numpy(full.reshape(K.TRUE_PEAK_TAPS, os)).to(device)
    return os, t


def channel_weights(C):
    """BS.1770's channel weights in WAVE channel order: 1 everywhere, but 0 for the LFE and 1.41 for the surrounds of 5.1
    (L R C LFE Ls Rs) and 7.1 (L R C LFE, then four surrounds)."""
    C = int(C)
    if C < 1:
        raise AvsepError(f"channel_weights takes C >= 1, got {C}")
    if C == 6:
        return np.array([1.0, 1.0, 1.0, 0.0, 1.41, 1.41])
    if C == 8:
        return np.array([1.0, 1.0, 1.0, 0.0, 1.41, 1.41, 1.41, 1.41])
    return np.ones(C, dtype=np.float64)


def _lufs(p):
    with np.errstate(divide="ignore"):
        return -0.691 + 10.0 * np.log10(p)


def _window_power(E, h, weights, subs):
    """E float64 [C, S] -> the weighted mean-square of every run of ``subs`` sub-blocks, [S - subs + 1] (empty for S < subs)."""
    S = E.shape[1]
    n = S - subs + 1
    if n < 1:
        return np.zeros(0, dtype=np.float64)
    z = np.zeros((E.shape[0], n), dtype=np.float64)
    for j in range(subs):
        z += E[:, j:j + n]
    return weights @ (z / (subs * h))


def loudness_from_energies(E, h, weights=None):
    """The host half of ``measure``.  E: float64 [P, C, S] (or [C, S]), the K-weighted energy of every sub-block of h samples
    -> {"integrated", "momentary_max", "short_term_max"}: float64 [P] in LUFS (-inf: nothing to measure).
    Blocks are four sub-blocks at a step of one; integrated is the mean power over the blocks above -70 LUFS and above the
    relative gate, 10 LU under the loudness of the blocks above -70."""
    E = np.asarray(E, dtype=np.float64)
    if E.ndim == 2:
        E = E[None]
    if E.ndim != 3:
        raise AvsepError(f"loudness_from_energies takes energies [P,C,S] or [C,S], got {E.shape}")
    P, C, S = E.shape
    w = channel_weights(C) if weights is None else np.asarray(weights, dtype=np.float64)
    if w.shape != (C,):
        raise AvsepError(f"{C} channels take {C} weights, got {w.shape}")
    out = {k: np.full(P, -np.inf) for k in ("integrated", "momentary_max", "short_term_max")}
    for p in range(P):
        pj = _window_power(E[p], h, w, BLOCK_SUBS)
        if pj.size:
            lj = _lufs(pj)
            out["momentary_max"][p] = lj.max()
            gate = lj > ABSOLUTE_GATE
            if gate.any():
                gamma = _lufs(pj[gate].mean()) + RELATIVE_GATE
                keep = gate & (lj > gamma)
                if keep.any():
                    out["integrated"][p] = _lufs(pj[keep].mean())
        ps = _window_power(E[p], h, w, SHORT_TERM_SUBS)
        if ps.size:
            out["short_term_max"][p] = _lufs(ps).max()
    return out


def measure(x, rate, weights=None):
    """x: f32 [P, C, L] on the GPU, P programmes of C channels (or [C, L], one programme) at ``rate`` -> dict of CPU float64
    tensors: "integrated", "momentary_max", "short_term_max" [P] in LUFS; "true_peak", "sample_peak" [P, C], linear;
    "energies" [P, C, S], the K-weighted energy of every 100 ms sub-block (S = L // h, h = (rate + 5) // 10).
    One launch of each kernel over the P*C rows; the energies come to the host once.  weights: one per channel
    (``channel_weights`` by default).  A NaN or an infinity in a row raises AvsepError naming the programme and channel."""
    rate = _check_rate(rate)
    if not torch.is_tensor(x) or x.dtype != torch.float32 or x.dim() not in (2, 3) or x.shape[-1] < 1 or x.shape[-2] < 1:
        raise AvsepError(f"measure takes float32 [P,C,L] or [C,L], got {lib.got(x)}")
    if x.dim() == 2:
        x = x[None]
    P, C, L = x.shape
    if P * C > 65535 or P < 1:
        raise AvsepError(f"measure takes up to 65535 rows in one call, got {P} x {C}")
    w = channel_weights(C) if weights is None else np.asarray(weights, dtype=np.float64)
    if w.shape != (C,) or not np.isfinite(w).all() or (w < 0).any():
        raise AvsepError(f"measure takes one finite weight >= 0 per channel ({C}), got {weights!r}")
    lib.require_gpu(x)
    rows = x.contiguous().reshape(P * C, L)
    h = (rate + 5) // 10
    os, taps = peak_table(rate, x.device)
    peaks = K.true_peak(rows, taps, os)
    E = K.loudness_energies(rows, k_weighting(rate), h) if L >= h else torch.zeros((P * C, 0), dtype=torch.float64, device=x.device)
    peaks = peaks.cpu().reshape(P, C, 2)
    bad = torch.nonzero(~torch.isfinite(peaks[..., 1]))
    if bad.numel():
        p, c = bad[0].tolist()
        raise AvsepError(f"measure: programme {p}, channel {c} holds a NaN or an infinity: it has no level")
    E = E.cpu().reshape(P, C, -1)
    out = {k: torch.from_numpy(v) for k, v in loudness_from_energies(E.numpy(), h, w).items()}
    out.update(true_peak=peaks[..., 1].contiguous(), sample_peak=peaks[..., 0].contiguous(), energies=E)
    return out


def output_gain(mix_lufs, true_peaks, loudness=None, peak=None):
    """-> (gain, limited_by): the one linear gain for every stem and channel of a run.  ``loudness`` (LUFS): the gain that
    brings the mixture from ``mix_lufs`` there; ``peak`` (dBTP): no more than what leaves the largest of ``true_peaks``
    (linear, at gain 1) at that ceiling.  limited_by: "loudness", "peak" (the ceiling decided) or None (gain 1)."""
    gain, limited_by = 1.0, None
    if loudness is not None:
        mix_lufs = float(mix_lufs)
        if not math.isfinite(mix_lufs):
            raise AvsepError(f"the mixture measures {mix_lufs} LUFS: a silent file has no level to move to {loudness} LUFS")
        gain, limited_by = 10.0 ** ((float(loudness) - mix_lufs) / 20.0), "loudness"
    if peak is not None:
        top = float(np.max(np.asarray(true_peaks, dtype=np.float64)))
        if top > 0.0 and 10.0 ** (float(peak) / 20.0) / top < gain:
            gain, limited_by = 10.0 ** (float(peak) / 20.0) / top, "peak"
    return gain, limited_by


def scaled(m, gain):
    """A ``measure`` result after every sample is multiplied by ``gain`` > 0: the filter and the oversampler are linear, so
    loudness moves by 20 log10(gain), peaks scale by gain and energies by its square (up to the f32 rounding of the products)."""
    gain = float(gain)
    out = {k: m[k] + 20.0 * math.log10(gain) for k in ("integrated", "momentary_max", "short_term_max")}
    out.update(true_peak=m["true_peak"] * gain, sample_peak=m["sample_peak"] * gain, energies=m["energies"] * gain * gain)
    return out


def _db(v):
    v = float(v)
    return 20.0 * math.log10(v) if v > 0.0 else -math.inf


def _json_number(v):
    v = float(v)
    return v if math.isfinite(v) else None


def figures(m, p=0):
    """The five figures of programme p of a ``measure`` result, as JSON takes them (-inf: None; the peaks per channel, in dB)."""
    return {"integrated_lufs": _json_number(m["integrated"][p]), "momentary_max_lufs": _json_number(m["momentary_max"][p]),
            "short_term_max_lufs": _json_number(m["short_term_max"][p]),
            "true_peak_dbtp": [_json_number(_db(v)) for v in m["true_peak"][p]],
            "sample_peak_dbfs": [_json_number(_db(v)) for v in m["sample_peak"][p]]}


def report(rate, gain, limited_by, mixture, stems):
    """What ``separate`` writes as levels.json: mixture, stems: ``measure`` results (one programme; one per source) AFTER the gain."""
    return {"rate": int(rate), "gain_db": _db(gain), "limited_by": limited_by, "mixture": figures(mixture),
            "sources": [figures(stems, n) for n in range(stems["integrated"].shape[0])]}


def _line(name, f):
    def num(v, unit):
        return f"{'-inf' if v is None else format(v, '.2f')} {unit}"
    peak = max((v for v in f["true_peak_dbtp"] if v is not None), default=None)
    sample = max((v for v in f["sample_peak_dbfs"] if v is not None), default=None)
    return (f"{name}: integrated {num(f['integrated_lufs'], 'LUFS')}, momentary max {num(f['momentary_max_lufs'], 'LUFS')}, "
            f"short-term max {num(f['short_term_max_lufs'], 'LUFS')}, true peak {num(peak, 'dBTP')}, sample peak {num(sample, 'dBFS')}")


def measure_file(path, device):
    """-> (WavInfo, measure result) of a WAV file: its frames go up as bytes and are measured at the file's own rate."""
    from . import wavio
    raw, info = wavio.read_frames(path)
    if info.channels > R.MAX_KEPT_CHANNELS:
        raise AvsepError(f"{path}: levels are measured for up to {R.MAX_KEPT_CHANNELS} channels, this file has {info.channels}")
    _check_rate(info.rate)
    rows = R.split_frames(torch.from_numpy(raw).to(device), info.fmt, info.channels, info.rate, info.rate)[1:]
    return info, measure(rows, info.rate)


def cli(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description="BS.1770-4 loudness and true peak of WAV files, measured on the GPU.")
    ap.add_argument("wavs", nargs="+", help="WAV files (16-, 24- or 32-bit PCM or 32-bit float, any rate from 8 to 192 kHz)")
    ap.add_argument("--json", default=None, help="also write the figures to this file")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise AvsepError("levels are measured on an MI355X; there is no CPU fallback")
    dev = torch.device("cuda", 0)
    out = {}
    for path in args.wavs:
        try:
            info, m = measure_file(path, dev)
        except AvsepError as e:
            raise SystemExit(str(e))
        out[path] = dict(figures(m), rate=info.rate, channels=info.channels)
        print(_line(path, out[path]))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    return out


if __name__ == "__main__":
    cli()
