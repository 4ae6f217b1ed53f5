"""How loud a stem is and whether it will clip: ITU-R BS.1770-4 loudness and true peak, and one peak-safe gain for a run.

The stems lie on the GPU just before they are encoded, so both measurements that need every sample are taken there
(``avsep_loudness_energies`` and ``avsep_true_peak``, include/avsep.h, csrc/levels.hip): the K-weighted energy of every
100 ms sub-block and the oversampled peak of every row.  What is left is a few thousand numbers per row: the 400 ms blocks
(four sub-blocks, 75 % overlap), the absolute and the relative gate and the 3 s short-term window are float64 NumPy on the
host (``loudness_from_energies``), because a gate is a data-dependent selection over a handful of values, not a hot path.

    measure(x, rate)          -> integrated / momentary-max / short-term-max LUFS, true and sample peak, the energies
    output_gain(...)          -> the ONE gain that brings a run to a loudness and keeps its largest true peak under a ceiling
    limit(x, rate, dbtp, ...) -> the rows under a true-peak ceiling by ONE look-ahead gain curve per programme (avsep_limiter:
                                 the meter's oversampler as the detector, a hold and a raised-cosine smoothing, all on the GPU)

CLI: ``python -m avsep_amd.levels a.wav b.wav ... [--json out.json]`` prints the five figures of every file (any format and
rate wavio.py reads, up to eight channels); ``python -m avsep_amd.levels in.wav --limit DBTP --out out.wav [--limit_lookahead
MS]`` writes the file limited to DBTP in its own format, its channels linked, and prints the figures before and after.
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


def limiter_plan(rate, lookahead_ms):
    """-> (A, w): the limiter's half-width in samples, max(1, round(rate * ms / 1000)), and its smoothing weights, float64
    [2A + 1]: w[k + A] = (1 + cos(pi k / (A + 1))) / sum for k = -A .. A (symmetric, sum 1)."""
    rate = _check_rate(rate)
    try:
        ms = float(lookahead_ms)
    except (TypeError, ValueError):
        ms = math.nan
    if not (math.isfinite(ms) and ms > 0.0):
        raise AvsepError(f"the limiter's look-ahead is a finite time > 0 in milliseconds, got {lookahead_ms!r}")
    A = max(1, int(round(rate * ms / 1000.0)))
    if A > K.LIMITER_MAX_A:
        raise AvsepError(f"the limiter looks ahead by at most {K.LIMITER_MAX_A} samples ({1000.0 * K.LIMITER_MAX_A / rate:.2f} ms at "
                         f"{rate} Hz), {ms} ms are {A}")
    k = np.arange(-A, A + 1, dtype=np.float64)
    w = 1.0 + np.cos(np.pi * k / (A + 1))
    return A, w / w.sum()


def limit(x, rate, ceiling_db, gain=1.0, lookahead_ms=5.0, trim=True, return_gain=False):
    """The linked look-ahead true-peak limiter (avsep_limiter, include/avsep.h).  x: f32 [P, C, L] on the GPU, P
    programmes of C rows (or [C, L], one programme) at ``rate``; every row of a programme gets the SAME gain curve: the
    pre-gain ``gain`` everywhere, turned down around the peaks only, so that no sample of gain * x passes the ceiling
    ``ceiling_db`` (dBTP, <= 0) where the oversampled detector sees it.  -> (y like x, info); info holds CPU float64 [P]
    tensors: "peak_in" (the programme's largest true peak, linear, the pre-gain included), "min_gain" (the curve's lowest
    value, the pre-gain not included), "limited_share" (the share of samples whose gain is below 1), "trim" (linear).
    trim: the curve moves a row's inter-sample peaks, so y is measured with avsep_true_peak and a programme whose true peak
    still passes the ceiling is multiplied by ceiling / true peak (1: nothing to do).  return_gain: info["gain"] is the
    curve, f64 [P, L] on the GPU, without pre-gain and trim.  A NaN or an infinity raises AvsepError naming the programme."""
    rate = _check_rate(rate)
    if not torch.is_tensor(x) or x.dtype != torch.float32 or x.dim() not in (2, 3) or x.shape[-1] < 1 or x.shape[-2] < 1:
        raise AvsepError(f"limit takes float32 [P,C,L] or [C,L], got {lib.got(x)}")
    single = x.dim() == 2
    if single:
        x = x[None]
    P, C, L = x.shape
    if not 1 <= P <= 65535 or C > K.LIMITER_MAX_C or P * C > 65535:
        raise AvsepError(f"limit takes up to 65535 rows in one call and up to {K.LIMITER_MAX_C} rows per programme, got {P} x {C}")
    try:
        ceiling_db, gain = float(ceiling_db), float(gain)
    except (TypeError, ValueError):
        raise AvsepError(f"limit takes a ceiling in dBTP and a linear pre-gain, got {ceiling_db!r} and {gain!r}")
    if not (math.isfinite(ceiling_db) and ceiling_db <= 0.0):
        raise AvsepError(f"limit takes a finite ceiling of at most 0 dBTP, got {ceiling_db}")
    if not (math.isfinite(gain) and gain > 0.0):
        raise AvsepError(f"limit takes a finite pre-gain > 0, got {gain}")
    _, w = limiter_plan(rate, lookahead_ms)          # refused before the device is looked at
    lib.require_gpu(x)
    c = 10.0 ** (ceiling_db / 20.0)
    os, taps = peak_table(rate, x.device)
    w = torch.from_numpy(w).to(taps.device)          # at most 32 KiB a call: nothing is kept on the device
    y, curve, stats = K.limiter(x, taps, w, os, gain, c, return_gain=return_gain)
    after = K.true_peak(y.reshape(P * C, L), taps, os)[:, 1].reshape(P, C).amax(1) if trim else None
    stats = stats.cpu()
    bad = torch.nonzero(~torch.isfinite(stats[:, 0]))
    if bad.numel():
        raise AvsepError(f"limit: programme {bad[0, 0].item()} holds a NaN or an infinity: it has no level")
    info = {"peak_in": stats[:, 0] * gain, "min_gain": stats[:, 1].contiguous(), "limited_share": stats[:, 2] / L,
            "trim": torch.ones(P, dtype=torch.float64)}
    if trim:
        after = after.cpu()
        for p in torch.nonzero(after > c)[:, 0].tolist():
            info["trim"][p] = c / after[p].item()
            y[p] = (y[p].double() * info["trim"][p].item()).float()       # one f32 rounding per sample
    if return_gain:
        info["gain"] = curve
    return (y[0] if single else y), info


def limiter_figures(info, ceiling_db, lookahead_ms, p=0):
    """The "limiter" block of levels.json from programme p of ``limit``'s info (-inf and +inf: None)."""
    return {"ceiling_dbtp": float(ceiling_db), "lookahead_ms": float(lookahead_ms),
            "max_reduction_db": _json_number(max(0.0, -_db(info["min_gain"][p]))), "limited_share": float(info["limited_share"][p]),
            "trim_db": _json_number(_db(info["trim"][p]))}


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


def report(rate, gain, limited_by, mixture, stems, limiter=None):
    """What ``separate`` writes as levels.json: mixture, stems: ``measure`` results (one programme; one per source) AFTER the gain
    (and after the limiter: ``limiter`` is then ``limiter_figures``' block and ``gain`` the limiter's pre-gain)."""
    out = {"rate": int(rate), "gain_db": _db(gain), "limited_by": limited_by, "mixture": figures(mixture),
           "sources": [figures(stems, n) for n in range(stems["integrated"].shape[0])]}
    if limiter is not None:
        out["limiter"] = dict(limiter)
    return out


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


def _limit_file(args, dev):
    """``--limit``: one file in, the same file under the ceiling out (its own rate, channels and sample format; a 32-bit PCM
    file is written as 24-bit, as ``separate`` writes it)."""
    from . import wavio
    path = args.wavs[0]
    raw, info = wavio.read_frames(path)
    if info.channels > R.MAX_KEPT_CHANNELS:
        raise AvsepError(f"{path}: levels are measured for up to {R.MAX_KEPT_CHANNELS} channels, this file has {info.channels}")
    _check_rate(info.rate)
    limiter_plan(info.rate, args.limit_lookahead)
    rows = R.split_frames(torch.from_numpy(raw).to(dev), info.fmt, info.channels, info.rate, info.rate)[1:]
    before = measure(rows, info.rate)
    y, lim = limit(rows, info.rate, args.limit, lookahead_ms=args.limit_lookahead)
    fmt = "s24" if info.fmt == "s32" else info.fmt
    wavio.write_frames(args.out, R.join_frames(y.contiguous(), info.rate, info.rate, fmt).cpu().numpy(), info.rate, info.channels, fmt)
    after = measure(y, info.rate)
    out = {"input": dict(figures(before), rate=info.rate, channels=info.channels), "output": figures(after),
           "limiter": limiter_figures(lim, args.limit, args.limit_lookahead)}
    print(_line(path, out["input"]))
    print(_line(args.out, out["output"]))
    f = out["limiter"]
    most = "to silence" if f["max_reduction_db"] is None else f"by up to {f['max_reduction_db']:.2f} dB"
    print(f"limiter at {f['ceiling_dbtp']:.2f} dBTP, look-ahead {f['lookahead_ms']:g} ms: {100.0 * f['limited_share']:.2f} % of the "
          f"samples turned down, {most}; trim {f['trim_db']:.4f} dB")
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)
    return out


def cli(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description="BS.1770-4 loudness and true peak of WAV files, measured on the GPU.")
    ap.add_argument("wavs", nargs="+", help="WAV files (16-, 24- or 32-bit PCM or 32-bit float, any rate from 8 to 192 kHz)")
    ap.add_argument("--json", default=None, help="also write the figures to this file")
    ap.add_argument("--limit", type=float, default=None, metavar="DBTP",
                    help="limit the ONE input file to this true-peak ceiling (<= 0) with a look-ahead limiter, its channels "
                         "linked, and write it to --out in the file's own format")
    ap.add_argument("--limit_lookahead", type=float, default=5.0, metavar="MS", help="with --limit: the look-ahead, milliseconds")
    ap.add_argument("--out", default=None, help="with --limit: the file to write")
    args = ap.parse_args(argv)
    if args.limit is not None:
        if len(args.wavs) != 1 or not args.out:
            raise SystemExit("--limit takes exactly one input file and --out OUT.wav")
        if not args.limit <= 0.0 or math.isinf(args.limit):
            raise SystemExit(f"--limit takes a finite true-peak ceiling of at most 0 dBTP, got {args.limit}")
    elif args.out:
        raise SystemExit("--out is where --limit writes: it needs --limit DBTP")
    if not torch.cuda.is_available():
        raise AvsepError("levels are measured on an MI355X; there is no CPU fallback")
    dev = torch.device("cuda", 0)
    if args.limit is not None:
        try:
            return _limit_file(args, dev)
        except AvsepError as e:
            raise SystemExit(str(e))
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
