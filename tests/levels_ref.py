"""float64 NumPy / SciPy restatement of ITU-R BS.1770-4 loudness and true peak: the yardstick of test_levels_host.py and
test_gpu_levels.py.  Nothing here is shared with avsep_amd/levels.py: the whole row goes through scipy.signal.sosfilt, the
blocks and gates are plain loops, and the oversampler is one direct convolution of the zero-stuffed row."""
import math

import numpy as np
from scipy import signal

U = 2.0 ** -53
TAPS = 21


def k_weighting(rate):
    """-> float64 [2, 6] sos (shelf, high-pass) of the K-weighting at ``rate``: the bilinear transforms of the analogue
    prototypes behind the standard's 48 kHz table."""
    def denominator(f0, Q):
        K = math.tan(math.pi * f0 / rate)
        a0 = 1.0 + K / Q + K * K
        return K, a0, [1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    Q = 0.7071752369554196
    K, a0, a = denominator(1681.974450955533, Q)
    Vh = 10.0 ** (3.999843853973347 / 20.0)
    Vb = Vh ** 0.4996667741545416
    shelf = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0] + a
    _, _, a = denominator(38.13547087602444, 0.5003270373238773)
    return np.array([shelf, [1.0, -2.0, 1.0] + a], dtype=np.float64)


def sub_block(rate):
    return (rate + 5) // 10


def filtered(x, rate):
    """x float64 [..., L] -> the K-weighted rows, every row from rest."""
    return signal.sosfilt(k_weighting(rate), np.asarray(x, dtype=np.float64), axis=-1)


def energies(x, rate, h=None):
    """x float64 [R, L] -> (E [R, S], A [R, S]): the sum of y^2 and of |y| over every sub-block of h samples of the filtered rows."""
    h = sub_block(rate) if h is None else h
    y = filtered(x, rate)
    S = y.shape[-1] // h
    y = y[..., :S * h].reshape(*y.shape[:-1], S, h)
    return (y * y).sum(-1), np.abs(y).sum(-1)


def sample_bound(rate, xmax):
    """B with |y - y_ref| <= B for a float64 filter whose rounding differs from sosfilt's: rounding injected in a section is
    amplified by that section's recursive part (g1, g2: absolute sums of the impulse responses of 1/A_shelf and 1/A_highpass;
    n2: that of the whole high-pass section, through which the shelf's error passes), each over 2 * rate samples.  64 covers
    about ten rounded operations per sample and section on values up to ~2 max|x|, both sides' error and the state hand-over."""
    sos = k_weighting(rate)
    imp = np.zeros(2 * rate)
    imp[0] = 1.0
    g1 = np.abs(signal.lfilter([1.0], sos[0, 3:], imp)).sum()
    g2 = np.abs(signal.lfilter([1.0], sos[1, 3:], imp)).sum()
    n2 = np.abs(signal.lfilter(sos[1, :3], sos[1, 3:], imp)).sum()
    return 64.0 * U * (g1 * n2 + g2) * xmax


def energy_bound(rate, xmax, A, h):
    """|E - E_ref| <= 2 B sum|y_ref| + h B^2 per sub-block (A: the sums of |y_ref| from ``energies``)."""
    B = sample_bound(rate, xmax)
    return 2.0 * B * A + h * B * B


def lufs(p):
    return -0.691 + 10.0 * math.log10(p) if p > 0.0 else -math.inf


def gating(E, h, weights):
    """E float64 [C, S] -> (integrated, momentary_max, short_term_max) in LUFS, -inf where there is nothing to measure."""
    E = np.asarray(E, dtype=np.float64)
    C, S = E.shape

    def power(j, n):
        return sum(weights[c] * (sum(E[c, j + i] for i in range(n)) / (n * h)) for c in range(C))
    p = [power(j, 4) for j in range(S - 3)]
    l = [lufs(v) for v in p]
    momentary = max(l, default=-math.inf)
    above = [j for j in range(len(p)) if l[j] > -70.0]
    integrated = -math.inf
    if above:
        gamma = lufs(sum(p[j] for j in above) / len(above)) - 10.0
        kept = [j for j in above if l[j] > gamma]
        if kept:
            integrated = lufs(sum(p[j] for j in kept) / len(kept))
    short = max((lufs(power(j, 30)) for j in range(S - 29)), default=-math.inf)
    return integrated, momentary, short


def channel_weights(C):
    return {6: [1.0, 1.0, 1.0, 0.0, 1.41, 1.41], 8: [1.0, 1.0, 1.0, 0.0, 1.41, 1.41, 1.41, 1.41]}.get(C, [1.0] * C)


def loudness(x, rate, weights=None):
    """x float64 [C, L] -> (integrated, momentary_max, short_term_max)."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    return gating(energies(x, rate)[0], sub_block(rate), channel_weights(x.shape[0]) if weights is None else weights)


def oversampling(rate):
    return 4 if rate < 96000 else 2 if rate < 192000 else 1


def interpolation_filter(os):
    """os * firwin(20 * os + 1, 1 / os, window=('kaiser', 5.0)), scipy.signal.resample_poly's filter; the unit impulse for 1."""
    if os == 1:
        return (np.arange(TAPS) == TAPS // 2).astype(np.float64)
    return os * signal.firwin(20 * os + 1, 1.0 / os, window=("kaiser", 5.0))


def oversampled(x, os, g):
    """x float64 [L] -> (u [os * L], s [os * L]): u[m] = sum_i x[n0 - i] g[p + i os] with pos = m + 10 os = n0 os + p, as one
    convolution of the zero-stuffed row, and the same sum over |x| |g| (the scale of its rounding error)."""
    x = np.asarray(x, dtype=np.float64)
    stuffed = np.zeros(os * x.size)
    stuffed[::os] = x
    lo = 10 * os
    return np.convolve(stuffed, g)[lo:lo + os * x.size], np.convolve(np.abs(stuffed), np.abs(g))[lo:lo + os * x.size]


def true_peak(x, rate):
    """x float64 [L] -> (sample peak, true peak, bound on |true peak - a float64 kernel's|)."""
    os = oversampling(rate)
    u, s = oversampled(x, os, interpolation_filter(os))
    sample = np.abs(x).max()
    return sample, max(sample, np.abs(u).max()), (TAPS + 2) * U * s.max()
