"""Windowed image-form BSS-eval (SDR / ISR / SIR / SAR) restated in numpy float64, straight from the definitions: lagged
correlations with np.correlate, explicit Gram matrices, np.linalg.solve (lstsq when singular), np.convolve, one plain loop
over windows.  TEST INFRASTRUCTURE ONLY: it shares no code with the package and is written for clarity, not speed.

Rows are q = source * C + channel.  A segment is a stretch of the signal treated as zero outside itself; for a segment of
n samples, reference rows r_p and estimate rows e_q,
    R[p][q][tau] = sum_t r_p[t + tau] r_q[t], |tau| < flen        D[p][q][k] = sum_t r_p[t - k] e_q[t], 0 <= k < flen
p_all[q] is the least-squares projection of e_q on the flen delays of ALL reference rows, p_own[q] on the delays of the
rows of q's own source; both live on n + flen - 1 samples."""
import itertools

import numpy as np


def plan_windows(L, win, hop):
    """Window w covers [w hop, w hop + win), w = 0 ... (L - win) // hop; a signal shorter than win is one window."""
    if L < win:
        return [0], L
    return [w * hop for w in range((L - win) // hop + 1)], win


def correlations(refs, ests, flen):
    """refs, ests [P, n] -> R [P, P, 2 flen - 1] (index tau + flen - 1), D [P(ref), P(est), flen]."""
    P, n = refs.shape
    R = np.zeros((P, P, 2 * flen - 1))
    D = np.zeros((P, P, flen))
    z = np.zeros(flen - 1)
    for p in range(P):
        for q in range(P):
            # "valid" of a row padded for every lag: out[u] = sum_t pad[t + u] b[t]
            R[p, q] = np.correlate(np.concatenate([z, refs[p], z]), refs[q], "valid")      # pad[t + u] = r_p[t + u - (flen - 1)]
            D[p, q] = np.correlate(np.concatenate([ests[q], z]), refs[p], "valid")         # sum_t e_q[t + k] r_p[t] = sum_t r_p[t - k] e_q[t]
    return R, D


def gram(R, rows, flen):
    """A[(i,a)][(j,c)] = sum_t r_i[t - a] r_j[t - c] = R[i][j][c - a]."""
    M = len(rows) * flen
    A = np.zeros((M, M))
    for bi, i in enumerate(rows):
        for bj, j in enumerate(rows):
            for a in range(flen):
                A[bi * flen + a, bj * flen:(bj + 1) * flen] = R[i, j, np.arange(flen) - a + flen - 1]
    return A


def project(refs, R, D, rows, qs, flen):
    """The projections of the estimate rows `qs` on the flen delays of the reference rows `rows`: [len(qs), n + flen - 1]."""
    A = gram(R, rows, flen)
    b = np.stack([np.concatenate([D[i, q] for i in rows]) for q in qs], 1)
    try:
        coef = np.linalg.solve(A, b)
    except np.linalg.LinAlgError:
        coef = np.linalg.lstsq(A, b, rcond=None)[0]
    out = np.zeros((len(qs), refs.shape[1] + flen - 1))
    for x in range(len(qs)):
        for bi, i in enumerate(rows):
            out[x] += np.convolve(coef[bi * flen:(bi + 1) * flen, x], refs[i])
    return out


def decompose(refs, ests, C, flen):
    """refs, ests [P, n] (one segment) -> s, e, p_own, p_all, each [P, n + flen - 1]."""
    P, n = refs.shape
    R, D = correlations(refs, ests, flen)
    pad = lambda x: np.concatenate([x, np.zeros((P, flen - 1))], 1)     # noqa: E731
    p_all = project(refs, R, D, list(range(P)), list(range(P)), flen)
    p_own = np.concatenate([project(refs, R, D, list(range(j, j + C)), list(range(j, j + C)), flen) for j in range(0, P, C)])
    return pad(refs), pad(ests), p_own, p_all


def scores(s, e, p_own, p_all, C, lo, hi):
    """The four scores of every source over the samples [lo, hi): [4, S] (sdr, isr, sir, sar)."""
    S = s.shape[0] // C
    out = np.zeros((4, S))
    with np.errstate(divide="ignore", invalid="ignore"):
        for j in range(S):
            rows = slice(j * C, j * C + C)
            en = lambda x: np.sum(x[rows, lo:hi] ** 2)                   # noqa: E731
            e_spat, e_interf, e_artif = p_own - s, p_all - p_own, e - p_all
            out[0, j] = 10 * np.log10(en(s) / en(e - s))
            out[1, j] = 10 * np.log10(en(s) / en(e_spat))
            out[2, j] = 10 * np.log10(en(s + e_spat) / en(e_interf)) if S > 1 else np.inf
            out[3, j] = 10 * np.log10(en(p_all) / en(e_artif))
    return out


def best_permutation(refs, ests):
    """perm[j] = the estimate matched to reference j: the largest mean plain SDR over the track, first permutation on ties."""
    S = refs.shape[0]
    with np.errstate(divide="ignore"):
        sdr = np.array([[10 * np.log10(np.sum(refs[j] ** 2) / np.sum((ests[i] - refs[j]) ** 2)) for j in range(S)] for i in range(S)])
    best, best_mean = None, None
    for perm in itertools.permutations(range(S)):
        m = np.mean([sdr[perm[j], j] for j in range(S)])
        if best is None or m > best_mean:
            best, best_mean = list(perm), m
    return best


def silent(refs, ests, lo, hi):
    """Some reference source or some estimate has exactly zero energy over all its channels in [lo, hi)."""
    return any(np.sum(x[j, :, lo:hi] ** 2) == 0 for x in (refs, ests) for j in range(x.shape[0]))


def score_stems(refs, ests, win, hop, filters="track", flen=512, permute=True):
    """refs, ests [S, C, L] (or [S, L]) -> the dict avsep_amd.score.score_stems returns, in numpy."""
    refs, ests = np.asarray(refs, np.float64), np.asarray(ests, np.float64)
    if refs.ndim == 2:
        refs, ests = refs[:, None], ests[:, None]
    S, C, L = refs.shape
    perm = best_permutation(refs, ests) if permute else list(range(S))
    ests = ests[perm]
    starts, wlen = plan_windows(L, win, hop)
    rr, er = refs.reshape(S * C, L), ests.reshape(S * C, L)
    frames = np.full((4, S, len(starts)), np.nan)
    out = {"perm": perm, "window_starts": starts}
    if filters == "track":
        parts = decompose(rr, er, C, flen)
        for w, a in enumerate(starts):
            if not silent(refs, ests, a, a + wlen):
                frames[:, :, w] = scores(*parts, C, a, a + wlen)
        out["track"] = dict(zip(("sdr", "isr", "sir", "sar"), scores(*parts, C, 0, L + flen - 1)))
    else:
        for w, a in enumerate(starts):
            if not silent(refs, ests, a, a + wlen):
                parts = decompose(rr[:, a:a + wlen], er[:, a:a + wlen], C, flen)
                frames[:, :, w] = scores(*parts, C, 0, wlen + flen - 1)
    out["frames"] = dict(zip(("sdr", "isr", "sir", "sar"), frames))
    with np.errstate(all="ignore"):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)                 # (an all-NaN row is NaN)
            for k in ("sdr", "isr", "sir", "sar"):
                out[k] = np.nanmedian(out["frames"][k], axis=1)
    return out
