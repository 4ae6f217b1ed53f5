"""float64 NumPy / SciPy restatement of the linked look-ahead true-peak limiter (include/avsep.h): the yardstick of
test_limiter_host.py and test_gpu_limiter.py.  Nothing here is shared with avsep_amd/levels.py: the detector is
levels_ref.oversampled (one convolution of the zero-stuffed row), the hold is scipy's minimum filter over the padded row, the
smoothing one matrix product over a sliding window view."""
import math

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view
from scipy import ndimage

import levels_ref as LREF

U = LREF.U
T = LREF.TAPS
MAX_A = 2048


def plan(rate, lookahead_ms):
    """-> (A, w): the half-width in samples and the raised-cosine weights w[k + A], k = -A .. A, float64, sum 1."""
    A = max(1, int(round(rate * lookahead_ms / 1000.0)))
    return A, weights(A)


def weights(A):
    k = np.arange(-A, A + 1, dtype=np.float64)
    w = 1.0 + np.cos(np.pi * k / (A + 1))
    return w / w.sum()


def detector(x, rate):
    """x float64 [C, L] -> (p [L], s [L]): the largest of |x[n]| and |u[os n + q]| over the rows, and the same maximum over
    sum |x| |g| (the scale of the oversampler's rounding error at n)."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    os = LREF.oversampling(rate)
    g = LREF.interpolation_filter(os)
    p, s = np.zeros(x.shape[1]), np.zeros(x.shape[1])
    for row in x:
        u, su = LREF.oversampled(row, os, g)
        p = np.maximum(p, np.maximum(np.abs(row), np.abs(u).reshape(-1, os).max(1)))
        s = np.maximum(s, np.maximum(np.abs(row), su.reshape(-1, os).max(1)))
    return p, s


def required(p, G, c):
    """r[n] = min(1, c / (G p[n])); p = 0 gives 1."""
    with np.errstate(divide="ignore"):
        return np.minimum(1.0, c / (G * p))


def hold(r, A):
    """r [L] -> h [L + 2A]: h[j + A] = min of r over |i - j| <= A for -A <= j < L + A, r = 1 outside [0, L)."""
    padded = np.concatenate([np.ones(2 * A), r, np.ones(2 * A)])
    return ndimage.minimum_filter1d(padded, 2 * A + 1, mode="constant", cval=1.0)[A:A + r.size + 2 * A]


def smooth(h, w, reverse=False):
    """h [L + 2A] -> g [L]: 1 - sum_k w[k] (1 - h[n + k]); reverse: the same sum with its terms in the opposite order."""
    win = sliding_window_view(1.0 - h, w.size)
    if reverse:
        return 1.0 - win[:, ::-1].copy() @ w[::-1].copy()
    return 1.0 - win @ w


def limit(x, rate, ceiling_db, G=1.0, A=None, lookahead_ms=5.0):
    """x [C, L] (one programme; its f32 values taken as float64) -> dict: p, r, h (on [-A, L + A)), g, y (float32: the f32
    nearest to x * (G g)), s_max = max over rows and positions of sum |x| |taps| (never below max |x|), c, A, w."""
    x64 = np.atleast_2d(np.asarray(x, dtype=np.float64))
    if A is None:
        A = plan(rate, lookahead_ms)[0]
    w = weights(A)
    c = 10.0 ** (ceiling_db / 20.0)
    p, s = detector(x64, rate)
    r = required(p, G, c)
    h = hold(r, A)
    g = smooth(h, w)
    y = (x64 * (G * g)).astype(np.float32)
    return {"p": p, "r": r, "h": h, "g": g, "y": y, "s_max": float(s.max()), "c": c, "A": A, "w": w, "G": G}


def gain_bound(G, s_max, c, A):
    """Bg with |g - g_ref| <= Bg for a float64 implementation whose roundings differ from this one's.  The detector's error is
    the meter's, (T + 2) U s_max; where the limiter is active G p > c, so |d r / d p| = c / (G p^2) < G / c; the hold selects;
    the smoothing is a sum of 2A + 1 products that are at most 1, and 7 more roundings cover G p, the division, 1 - h and
    the final 1 - sum on both sides."""
    return U * ((T + 2) * G * s_max / c + 2 * A + 8)


def output_bound(y_ref, x, G, Bg):
    """|y - y_ref| <= 1.01 * 2^-24 |y_ref| + G |x| Bg: the f32 rounding of the product and the gain's error carried to it."""
    return 1.01 * 2.0 ** -24 * np.abs(np.asarray(y_ref, dtype=np.float64)) + G * np.abs(np.asarray(x, dtype=np.float64)) * Bg


def true_peak(y, rate):
    """y [C, L] -> (the largest true peak of the rows, the meter's bound on it, s_max of y)."""
    top, bound, s_max = 0.0, 0.0, 0.0
    os = LREF.oversampling(rate)
    for row in np.atleast_2d(np.asarray(y, dtype=np.float64)):
        _, tp, b = LREF.true_peak(row, rate)
        top, bound = max(top, tp), max(bound, b)
        s_max = max(s_max, float(np.abs(row).max()), float(LREF.oversampled(row, os, LREF.interpolation_filter(os))[1].max()))
    return top, bound, s_max


def overshoot_db(y, rate, c):
    """How far the true peak of y lies above c, in dB (negative: under it)."""
    top = true_peak(y, rate)[0]
    return 20.0 * math.log10(top / c) if top > 0.0 else -math.inf


def recipe(rate, A, L, C, seed=0):
    """The GPU tests' input: 0.25 * uniform noise rounded to f32, with spikes of +-1.5 at 0, A, 2047, 2048, L - 1 and L // 2
    (those that exist), the spike at ``pos`` in row pos % C; float32 [C, L]."""
    g = np.random.default_rng(seed + 7919 * rate + 31 * L + C)
    x = (0.25 * g.uniform(-1.0, 1.0, (C, L))).astype(np.float32)
    for i, pos in enumerate(sorted({q for q in (0, A, 2047, 2048, L - 1, L // 2) if 0 <= q < L})):
        x[pos % C, pos] = np.float32(1.5 if i % 2 == 0 else -1.5)
    return x
