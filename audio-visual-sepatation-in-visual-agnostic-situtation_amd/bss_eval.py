"""BSS-eval on the GPU: the host layer of csrc/bss_windows.hip, and SDR / SIR / SAR of training batches.

The reference scores separation with asteroid's `get_metrics(..., ['sdr','sir','sar','si_sdr'])` (main.py:260-266),
i.e. mir_eval.separation.bss_eval_sources(reference, estimate, compute_permutation=False): each estimate is projected
(least squares) on the span of 512 delayed copies of (a) its own true source and (b) all true sources; the three
residuals give SDR, SIR, SAR (Vincent et al. 2006, `bss_decomp_mtifilt`).  mir_eval runs this per sample in numpy
on the CPU and dominates the reference's evaluate().  Here rows [P, L] (p = source * C + channel) are scored in SEGMENTS,
stretches [a, a + n) treated as zero outside themselves, through three float64 entry points: lagged correlations read in
place (the block-Toeplitz Gram matrices and the right-hand sides), one LU-with-partial-pivoting solve per (segment, group
of rows) (numpy.linalg.solve's algorithm, one workgroup each), and both FIR projections with their eight residual energies
(no projected waveform is stored).  No atomics: two calls give the same bits, and a segment's bits do not depend on the
other segments of the call.  Exactly singular Gram matrices (a silent source; dual-mono) take mir_eval's fallback: minimum-
norm least squares, on the host, for that system only.

bss_eval_sources scores a mono batch [B, S, L] as S rows of B * L samples, sample b the segment [b L, b L + L).  score.py
scores whole recordings in windows (the image form, with ISR) on the same functions.
"""
import torch

from . import lib
from .lib import AvsepError, call, ptr

FLEN = 512
MAX_ROWS = 8                 # P = S * C
MAX_UNKNOWNS = 2048          # P * flen: the dense solver's size (one workgroup per system)
TERMS = 8                    # s^2, (e-s)^2, e_spat^2, (s+e_spat)^2, e_interf^2, p_all^2, e_artif^2, (e_interf+e_artif)^2
_BATCH_BYTES = 8 << 30       # workspace budget of one batch of segments with filters of their own (50 MB each at 2048 unknowns)


def check_limits(S, C, flen):
    P = S * C
    if S < 1 or C < 1:
        raise AvsepError(f"BSS-eval needs at least one source and one channel (1 <= S), got S={S} C={C}")
    if P > MAX_ROWS:
        raise AvsepError(f"BSS-eval takes at most P = S * C <= {MAX_ROWS} rows, got {S} sources x {C} channels = {P}")
    if flen < 1 or P * flen > MAX_UNKNOWNS:
        raise AvsepError(f"BSS-eval solves at most P * flen <= {MAX_UNKNOWNS} unknowns (the dense solver's size), "
                         f"got {P} rows x flen {flen} = {P * flen}")


def _i64(vals, dev):
    return torch.tensor(list(vals), dtype=torch.int64, device=dev)


def seg_corr(refs, ests, flen, starts, n):
    """refs, ests [P, L] float64; segments [starts[i], starts[i] + n).  -> R [nseg, P, P, 2 flen - 1], D [nseg, P(est), P(ref), flen]."""
    Lb = lib.load()
    P, L = refs.shape
    dev, nseg = refs.device, len(starts)
    nbytes = Lb.avsep_bss_seg_corr_workspace_bytes(nseg, P, n, flen)
    ws = torch.empty((max(nbytes // 8, 1),), dtype=torch.float64, device=dev)
    R = torch.empty((nseg, P, P, 2 * flen - 1), dtype=torch.float64, device=dev)
    D = torch.empty((nseg, P, P, flen), dtype=torch.float64, device=dev)
    seg = _i64(starts, dev)
    call("avsep_bss_seg_corr", ptr(refs), ptr(ests), P, L, flen, ptr(seg), nseg, n, ptr(ws), nbytes, ptr(R), ptr(D))
    return R, D


def _gram(R, seg, rows, flen):
    """The Gram matrix of the rows `rows` of segment `seg` from the lagged correlations (host-side fallback only)."""
    k = torch.arange(flen, device=R.device)
    lag = (k[None, :] - k[:, None]) + flen - 1                              # [a, c] -> c - a + flen - 1
    return torch.cat([torch.cat([R[seg, i, j][lag] for j in rows], 1) for i in rows], 0)


def solve_groups(R, D, G, flen):
    """The filters of every (segment, group of G rows): [nseg * P / G, G * flen, G]."""
    Lb = lib.load()
    nseg, P = R.shape[:2]
    ng, M = P // G, G * flen
    nbytes = Lb.avsep_bss_solve_groups_workspace_bytes(nseg, P, G, flen)
    ws = torch.empty((nbytes // 8,), dtype=torch.float64, device=R.device)
    C = torch.empty((nseg * ng, M, G), dtype=torch.float64, device=R.device)
    info = torch.empty((nseg * ng,), dtype=torch.int32, device=R.device)
    call("avsep_bss_solve_groups", ptr(R), ptr(D), nseg, P, G, flen, ptr(ws), nbytes, ptr(C), ptr(info))
    bad = info != 0
    if G > 1:
        # Two rows with the same samples (dual-mono) give two bit-identical block rows of the Gram matrix: exactly singular,
        # but the LU only meets an exact zero when every multiplier x * (1 / x) rounds to 1, which it need not.  Found here.
        g = torch.arange(ng, device=R.device)
        Rg = R.reshape(nseg, ng, G, ng, G, -1)[:, g, :, g]                    # [ng, nseg, G(i), G(j), lags]: R[seg, gG+i, gG+j]
        for i in range(G):
            for k in range(i + 1, G):
                bad |= (Rg[:, :, i] == Rg[:, :, k]).flatten(2).all(2).t().reshape(-1)
    # (one host sync; the metrics are eval-only)
    for s in bad.nonzero().flatten().tolist():        # exactly singular (dual-mono, a silent row): minimum-norm least squares,
        seg, base = s // ng, (s % ng) * G             # as mir_eval does
        rows = list(range(base, base + G))
        A = _gram(R, seg, rows, flen).cpu()
        rhs = D[seg, base:base + G, base:base + G].permute(1, 2, 0).reshape(M, G).cpu()
        # driver gelsd = numpy.linalg.lstsq's (what mir_eval falls back to).  torch's CPU default, gelsy, returned wrong
        # minimum-norm solutions for this exactly rank-deficient system on some calls (errors of 0.2-0.9 in the filters on a
        # 128-thread host, 1e-16 on others: scratch probe of round 5); gelsd / gelss / an eigendecomposition agree to 3e-15
        C[s] = torch.linalg.lstsq(A, rhs.contiguous(), driver="gelsd").solution.to(C.device)
    return C


def window_energies(refs, ests, C, flen, starts, n, C_all, C_own, range_seg, range_off, rlen):
    """-> [nrange, S, 8]: the eight energy sums of every (range, source)."""
    Lb = lib.load()
    P, L = refs.shape
    dev, nrange = refs.device, len(range_seg)
    nbytes = Lb.avsep_bss_window_energies_workspace_bytes(nrange, P, rlen)
    ws = torch.empty((nbytes // 8,), dtype=torch.float64, device=dev)
    sums = torch.empty((nrange, P // C, TERMS), dtype=torch.float64, device=dev)
    # (the index arrays stay referenced until the launch is queued: a temporary's block would go to the next temporary)
    seg, rseg, roff = _i64(starts, dev), torch.tensor(list(range_seg), dtype=torch.int32, device=dev), _i64(range_off, dev)
    call("avsep_bss_window_energies", ptr(refs), ptr(ests), P, C, L, flen, ptr(seg), len(starts), n, ptr(C_all), ptr(C_own),
         ptr(rseg), ptr(roff), nrange, rlen, ptr(ws), nbytes, ptr(sums))
    return sums


def segment_energies(refs, ests, C, flen, starts, n):
    """Every segment [starts[i], starts[i] + n) fitted on its own and scored over its whole padded span [0, n + flen - 1):
    -> [nseg, S, 8].  The segments go through in batches that keep the workspaces within _BATCH_BYTES."""
    P = refs.shape[0]
    per_seg = 8 * ((P * flen) ** 2 + (P // C) * (C * flen) ** 2) + lib.load().avsep_bss_seg_corr_workspace_bytes(1, P, n, flen)
    nb = int(max(1, min(256, _BATCH_BYTES // per_seg)))
    out = torch.empty((len(starts), P // C, TERMS), dtype=torch.float64, device=refs.device)
    for b0 in range(0, len(starts), nb):
        seg = starts[b0:b0 + nb]
        R, D = seg_corr(refs, ests, flen, seg, n)
        C_all, C_own = solve_groups(R, D, P, flen), solve_groups(R, D, C, flen)
        out[b0:b0 + nb] = window_energies(refs, ests, C, flen, seg, n, C_all, C_own, range(len(seg)), [0] * len(seg), n + flen - 1)
    return out


def bss_eval_sources(refs, ests, flen=FLEN):
    """refs, ests: [B, S, L] (estimate j against reference j).  Returns sdr, sir, sar: float64 [B, S] in dB.
    With s_filt = p_own and e_interf + e_artif = e - p_own (mir_eval's SDR; score.py's is the plain ratio):
    SDR = sum p_own^2 / sum (e - p_own)^2, SIR = sum p_own^2 / sum (p_all - p_own)^2, SAR = sum p_all^2 / sum (e - p_all)^2."""
    lib.require_gpu(refs)
    B, S, L = refs.shape
    if ests.shape[1] != S:
        raise AvsepError("bss_eval_sources scores estimate j against reference j: as many estimates as references")
    check_limits(S, 1, flen)
    rows = lambda x: x.double().transpose(0, 1).reshape(S, B * L).contiguous()          # noqa: E731
    sums = segment_energies(rows(refs), rows(ests), 1, flen, [b * L for b in range(B)], L)
    db = lambda a, b: 10 * torch.log10(a / b)                              # noqa: E731
    # (S = 1: p_all and p_own are the same bits, sum 4 is exactly zero and SIR +inf)
    return db(sums[..., 3], sums[..., 7]), db(sums[..., 3], sums[..., 4]), db(sums[..., 5], sums[..., 6])
