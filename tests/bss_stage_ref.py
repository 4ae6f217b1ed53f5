"""The three stages of csrc/bss_windows.hip restated one at a time in numpy, so that each can be compared on its own inputs:
lagged correlations of a segment that overhangs its rows (with the sum of absolute products, the scale of its rounding
error), a Gaussian elimination with partial pivoting in long double that also reports what it did (row swaps, the first
exactly zero pivot), the normwise backward error of a solution, and the eight energy sums of a sample range from GIVEN
filters.  TEST INFRASTRUCTURE ONLY: numpy, shares no code with the package; the Gram matrix of a group is score_ref.gram.

Layouts are the kernels': rows q = source * C + channel; R [P, P, 2 flen - 1], D [P(ref), P(est), flen] as score_ref has them
(the entry point's D is [P(est), P(ref), flen]); C_all [P * flen, P] with row (p, k) the tap k on reference row p and column q
the estimate row; C_own [S, C * flen, C] likewise within a source."""
import numpy as np

import score_ref as SR


def segment(rows, start, n):
    """rows [P, L] -> [P, n]: the samples [start, start + n), zero where that lies outside [0, L)."""
    rows = np.asarray(rows)
    P, L = rows.shape
    out = np.zeros((P, n), rows.dtype)
    lo, hi = max(start, 0), min(start + n, L)
    if hi > lo:
        out[:, lo - start:hi - start] = rows[:, lo:hi]
    return out


def correlations_padded(rows_ref, rows_est, start, n, flen):
    """score_ref.correlations on the segment [start, start + n) of rows that read as zero outside [0, L).
    -> R, D, absR, absD: the correlations, and for every entry the sum of |a| |b| over the same products."""
    r, e = segment(rows_ref, start, n), segment(rows_est, start, n)
    R, D = SR.correlations(r, e, flen)
    absR, absD = SR.correlations(np.abs(r), np.abs(e), flen)
    return R, D, absR, absD


def solve_ld(A, b):
    """Gaussian elimination with partial pivoting (the first largest entry of the column, rows swapped at once) in long
    double.  -> x [M, nrhs] in long double, the number of row swaps, the column of the first exactly zero (or NaN) pivot or
    None; with such a pivot x is all zeros and the count is that of the columns before it."""
    A = np.array(A, dtype=np.longdouble)
    M = A.shape[0]
    x = np.array(b, dtype=np.longdouble).reshape(M, -1)
    swaps = 0
    # Panels of `nb` columns (the same pivots and the same products as column-by-column elimination; the trailing matrix gets a
    # panel's updates as one long-double matrix product, which is what makes 2048 unknowns take seconds and not a minute).
    # The multipliers stay below the diagonal.
    nb = 32
    for k0 in range(0, M, nb):
        k1 = min(k0 + nb, M)
        for k in range(k0, k1):
            p = k + int(np.argmax(np.abs(A[k:, k])))
            if not np.abs(A[p, k]) > 0:
                return np.zeros_like(x), swaps, k
            if p != k:
                A[[k, p]] = A[[p, k]]
                x[[k, p]] = x[[p, k]]
                swaps += 1
            A[k + 1:, k] /= A[k, k]
            A[k + 1:, k + 1:k1] -= A[k + 1:, k][:, None] * A[k, k + 1:k1][None, :]
        for k in range(k0, k1):                                # the panel's rows of U right of the panel
            A[k + 1:k1, k1:] -= A[k + 1:k1, k][:, None] * A[k, k1:][None, :]
        A[k1:, k1:] -= A[k1:, k0:k1] @ A[k0:k1, k1:]
    for k in range(M):
        x[k + 1:] -= A[k + 1:, k][:, None] * x[k][None, :]
    for k in range(M - 1, -1, -1):
        x[k] /= A[k, k]
        x[:k] -= A[:k, k][:, None] * x[k][None, :]
    return x, swaps, None


def backward_error(A, x, b):
    """|| A x - b ||inf / (|| A ||inf || x ||inf + || b ||inf), the products and sums in long double; x and b [M] or [M, nrhs],
    the norms over the whole block."""
    A, x, b = (np.asarray(v, dtype=np.longdouble) for v in (A, x, b))
    x, b = x.reshape(A.shape[0], -1), b.reshape(A.shape[0], -1)
    res = np.stack([(A * x[:, q][None, :]).sum(1) for q in range(x.shape[1])], 1) - b
    return float(np.abs(res).max() / (np.abs(A).sum(1).max() * np.abs(x).max() + np.abs(b).max()))


def energy_terms(refs, ests, C, flen, seg_start, n, C_all, C_own, off, rlen, dtype=np.float64):
    """The eight sums [S, 8] of the range [off, off + rlen) of the segment [seg_start, seg_start + n) of the rows refs, ests
    [P, L], from the given filters, as the comment above bss_win_energy_kernel defines them:
        0: s^2  1: (e - s)^2  2: (p_own - s)^2  3: p_own^2  4: (p_all - p_own)^2  5: p_all^2  6: (e - p_all)^2  7: (e - p_own)^2
    The rows are zero outside the segment and outside [0, L), the projections live on [0, n + flen - 1) and the range is
    clipped to that.  dtype: np.float64 or np.longdouble, used for every product and sum."""
    P = np.asarray(refs).shape[0]
    S, T = P // C, n + flen - 1
    r = segment(refs, seg_start, n).astype(dtype)
    pad = np.zeros((P, flen - 1), dtype)
    s, e = np.concatenate([r, pad], 1), np.concatenate([segment(ests, seg_start, n).astype(dtype), pad], 1)
    C_all, C_own = np.asarray(C_all).astype(dtype), np.asarray(C_own).astype(dtype)
    p_all, p_own = np.zeros((P, T), dtype), np.zeros((P, T), dtype)
    for q in range(P):
        j, c = divmod(q, C)
        for p in range(P):
            p_all[q] += np.convolve(C_all[p * flen:(p + 1) * flen, q], r[p])
        for i in range(C):
            p_own[q] += np.convolve(C_own[j][i * flen:(i + 1) * flen, c], r[j * C + i])
    lo, hi = max(off, 0), min(off + rlen, T)
    out = np.zeros((S, 8), dtype)
    if hi <= lo:
        return out
    for j in range(S):
        en = lambda x: (x[j * C:j * C + C, lo:hi] ** 2).sum()                  # noqa: E731
        out[j] = [en(s), en(e - s), en(p_own - s), en(p_own), en(p_all - p_own), en(p_all), en(e - p_all), en(e - p_own)]
    return out
