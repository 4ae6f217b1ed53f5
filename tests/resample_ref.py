"""float64 NumPy restatement of avsep_resample_poly (include/avsep.h): the filter and the direct sum, with the sum of
absolute terms that the GPU tests' error bound scales with.  Nothing here imports the package."""
import numpy as np


def design(up, down):
    """up * firwin(20*max(up,down)+1, 1/max(up,down), window=('kaiser', 5.0)) without scipy."""
    m = max(int(up), int(down))
    half = 10 * m
    M = 2 * half + 1
    w = np.sinc((np.arange(M, dtype=np.float64) - half) / m) / m * np.kaiser(M, 5.0)
    return w / w.sum() * int(up)


def out_length(L, up, down):
    return -(-int(L) * int(up) // int(down))


def taps(up, down):
    """T = ceil(M / up): the most filter taps one output touches."""
    return -(-(20 * max(int(up), int(down)) + 1) // int(up))


def ref_outputs(x, up, down, idx):
    """y[j] = sum_n x[n] * h[j*down - n*up + half] over 0 <= n < L with the filter index in [0, M), for the output indexes
    ``idx``, in float64 with the float64 filter.  -> (y, absref) with absref[j] = sum_n |x[n]| * |h[...]|."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    up, down = int(up), int(down)
    h = design(up, down)
    M, half, L = h.size, (h.size - 1) // 2, x.size
    j = np.asarray(idx, dtype=np.int64).reshape(-1)
    pos = j * down + half                                            # int64: passes 2^31 on a ten-minute file
    i = np.arange(taps(up, down), dtype=np.int64)[None, :]
    n = (pos // up)[:, None] - i
    k = (pos % up)[:, None] + i * up
    ok = (k < M) & (n >= 0) & (n < L)
    terms = np.where(ok, x[np.clip(n, 0, L - 1)] * h[np.clip(k, 0, M - 1)], 0.0)
    return terms.sum(1), np.abs(terms).sum(1)
