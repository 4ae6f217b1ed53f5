"""float64 NumPy restatement of avsep_band_gains and avsep_band_extend (include/avsep.h), with the magnitudes the GPU tests'
error bounds scale with.  The filter and the chains are tests/resample_ref.py's.  Nothing here imports the package."""
import numpy as np

import resample_ref as R

EPS = 2.0 ** -24
TINY = float(np.float32(1e-20))     # the kernel's constant as f32 holds it


def ref_gains(stem_mag, mix_mag, lo_bin):
    """stem_mag [N,G,bins,F], mix_mag [G,bins,F] -> float64 [N,G,F]: min(1, sqrt(num / (den + 1e-20 * B))) over the bins
    [lo_bin, bins)."""
    s = np.asarray(stem_mag, dtype=np.float64)[:, :, lo_bin:]
    m = np.asarray(mix_mag, dtype=np.float64)[:, lo_bin:]
    B = m.shape[1]
    return np.minimum(1.0, np.sqrt((s * s).sum(2) / ((m * m).sum(1)[None] + TINY * B)))


def gains_bound(ref, bins, lo_bin):
    """|g - ref| <= (B + 6) * 2^-24 * ref (the module docstring of tests/test_gpu_fullband.py derives it)."""
    return (bins - lo_bin + 6) * EPS * ref


def frame_position(j, up, down, hop, F):
    """-> t0, t1 (int64), fr (float64, exact) of the outputs j: output j sits at model sample j * down / up."""
    num = np.asarray(j, dtype=np.int64) * int(down)
    den = int(up) * int(hop)
    t0 = np.minimum(num // den, F - 1)
    t1 = np.minimum(t0 + 1, F - 1)
    return t0, t1, (num - t0 * den).astype(np.float64) / den


def ref_extend(stems, low, file, gains, up, down, hop, idx=None):
    """stems [N,G,Lm], low [G,Ll], file [G,Lf], gains [N,G,F] -> dict of float64 arrays over the outputs ``idx`` (default: all
    Lout = ceil(Lm * up / down)): out [N,G,J] and what the bound needs: s, abs_s [N,G,J] (the stem chains and their sums
    of absolute terms), l, abs_l, h [G,J], gi [N,G,J], frd [N,G,J] = fr * |gains[t1] - gains[t0]|."""
    stems, low, file, gains = (np.asarray(a, dtype=np.float64) for a in (stems, low, file, gains))
    N, G, Lm = stems.shape
    Lf, F = file.shape[1], gains.shape[2]
    Lout = R.out_length(Lm, up, down)
    j = np.arange(Lout, dtype=np.int64) if idx is None else np.asarray(idx, dtype=np.int64)
    J = j.size
    s, abs_s = np.empty((N, G, J)), np.empty((N, G, J))
    l, abs_l, h = np.empty((G, J)), np.empty((G, J)), np.zeros((G, J))
    inside = j < Lf
    for g in range(G):
        l[g], abs_l[g] = R.ref_outputs(low[g], up, down, j)
        h[g, inside] = file[g, j[inside]] - l[g, inside]
        for n in range(N):
            s[n, g], abs_s[n, g] = R.ref_outputs(stems[n, g], up, down, j)
    t0, t1, fr = frame_position(j, up, down, hop, F)
    g0, g1 = gains[:, :, t0], gains[:, :, t1]
    d = g1 - g0
    gi = g0 + np.where(d != 0.0, fr * d, 0.0)                 # past the last frame t1 = t0: fr takes no part
    return {"out": s + gi * h[None], "s": s, "abs_s": abs_s, "l": l, "abs_l": abs_l, "h": h, "gi": gi, "frd": fr * np.abs(d),
            "inside": inside}


def extend_bound(ref, up, down):
    """The bound of tests/test_gpu_fullband.py's docstring on |out - ref["out"]|, term by term, u = 2^-24."""
    u = EPS
    T = R.taps(up, down)
    e_s = (T + 2) * u * ref["abs_s"]                          # the stem chain
    e_l = (T + 2) * u * ref["abs_l"]                          # the low chain
    e_h = np.where(ref["inside"], e_l + u * (np.abs(ref["h"]) + e_l), 0.0)        # file - l, rounded once
    gi, h = np.abs(ref["gi"]), np.abs(ref["h"])[None]
    e_gi = u * gi + (2 * u + 4 * u * u) * ref["frd"]          # fr and the difference rounded once each, then the fma
    E = (gi + e_gi) * e_h[None] + e_gi * h + e_s
    return E + u * (np.abs(ref["out"]) + E)                   # the final fma


def two_sources(rate, seconds):
    """The two harmonic sources of DESIGN.md's full-band experiment at ``rate``: 440 Hz with 40 harmonics and 587 Hz with
    30, amplitudes k^-0.7, under on/off note envelopes at 0.7 and 1.1 Hz; float64 [2, L], the mixture's peak below 1."""
    t = np.arange(int(round(rate * seconds)), dtype=np.float64) / rate
    src = []
    for f0, K, fe in ((440.0, 40, 0.7), (587.0, 30, 1.1)):
        x = sum(k ** -0.7 * np.sin(2 * np.pi * k * f0 * t + 0.3 * k * k) for k in range(1, K + 1))
        src.append(x * np.clip(0.5 + 4.0 * np.sin(2 * np.pi * fe * t), 0.0, 1.0))
    src = np.stack(src)
    return src * (0.9 / np.abs(src.sum(0)).max())


def sdr(ref, est):
    return 10.0 * np.log10((ref * ref).sum() / ((ref - est) ** 2).sum())
