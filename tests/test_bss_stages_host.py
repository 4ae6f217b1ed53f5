"""not-gpu: the conditions that tests/bss_cases.py must meet for test_gpu_bss_stages.py to mean what it says (the energy
cases cancel nowhere, the solve cases need pivoting and are well conditioned), the per-stage reference tests/bss_stage_ref.py
against tests/score_ref.py and numpy, and the refusals of the three entry points of csrc/bss_windows.hip."""
import ctypes

import numpy as np
import pytest

import avsep_amd as P

import bss_cases as BC
import bss_stage_ref as BR
import score_ref as SR

ERR_ARG, ERR_WORKSPACE = -1, -3


# ---- stage 3: the energy cases ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", BC.EN_CASES, ids=lambda c: c[0])
def test_energy_cases_do_not_cancel(case):
    """energy_terms in float64 against long double: at most 1e-13 relative on every term of every valid range.  A condition
    on the inputs: a case that fails it cancels somewhere and must be redrawn."""
    name, S, C, flen, L, starts, n, ranges, rlen, _ = case
    terms = BC.en_inputs(case)[4]
    valid = [i for i, (seg, _) in enumerate(ranges) if 0 <= seg < len(starts)]
    f64, ld = terms["f64"][valid], terms["ld"][valid]
    assert f64.shape == (len(valid), S, 8)
    # a term is exactly zero only where every square in it is: s^2 and (e - s)^2 of a range that lies in the tail
    zero = ld == 0
    in_tail = np.array([ranges[i][1] >= n for i in valid])
    assert (f64[zero] == 0).all() and not zero[~in_tail].any() and not zero[:, :, 2:].any()
    rel = (np.abs(f64 - ld)[~zero] / ld[~zero]).astype(np.float64)
    print(f"{name}: smallest term {float(ld[~zero].min()):.3g}, float64 against long double at most {rel.max():.2e} relative")
    assert rel.max() <= 1e-13
    invalid = [i for i in range(len(ranges)) if i not in valid]
    assert (terms["ld"][invalid] == 0).all()


def test_energy_cases_cover_what_they_are_for():
    """The table itself: every tap count, row count and range edge the kernels treat differently."""
    cases = {c[0]: c for c in BC.EN_CASES}
    assert {c[3] for c in BC.EN_CASES} >= {1, 5, 13, 24, 100}
    assert {c[1] * c[2] for c in BC.EN_CASES} >= {1, 2, 4, 8} and {(c[1], c[2]) for c in BC.EN_CASES} >= {(1, 2), (4, 2)}
    assert {c[8] for c in BC.EN_CASES} >= {1, 1024, 1025, 66004}
    name, S, C, flen, L, starts, n, ranges, rlen, _ = cases["offsets"]
    assert {off for _, off in ranges} >= {0, 37, 1000, 1023, -5} and len({seg for seg, _ in ranges}) == 3
    assert any(n <= off < n + flen - 1 for _, off in ranges), "a range that starts inside the tail"
    assert any(off < n and off + rlen > n + flen - 1 for _, off in ranges), "a range that runs past the tail"
    name, S, C, flen, L, starts, n, ranges, rlen, _ = cases["65-chunks"]
    assert (rlen + 1023) // 1024 == 65 and n == 66000 and rlen == n + flen - 1
    name, S, C, flen, L, starts, n, ranges, rlen, _ = cases["invalid"]
    assert {seg for seg, _ in ranges} == {-1, 0, 1, len(starts)}
    name, S, C, flen, L, starts, n, ranges, rlen, guard = cases["overhang"]
    assert guard and min(starts) < 0 and max(starts) + n > L


def test_energy_terms_with_solved_filters_are_the_restatements_scores():
    """The two references agree: the filters that score_ref solves, handed to energy_terms, give score_ref.scores (1e-9 dB),
    over the whole padded span and over an inner range."""
    S, C, n, flen = 2, 2, 700, 6
    Pn = S * C
    s, e = BC.coloured_mix(Pn, n, 31)
    R, D = SR.correlations(s, e, flen)

    def coef(rows):
        b = np.stack([np.concatenate([D[i, q] for i in rows]) for q in rows], 1)
        return np.linalg.solve(SR.gram(R, rows, flen), b)
    C_all = coef(list(range(Pn)))
    C_own = np.stack([coef(list(range(j * C, j * C + C))) for j in range(S)])
    parts = SR.decompose(s, e, C, flen)
    for lo, hi in ((0, n + flen - 1), (100, 450)):
        t = BR.energy_terms(s, e, C, flen, 0, n, C_all, C_own, lo, hi - lo)
        got = 10 * np.log10(np.stack([t[:, 0] / t[:, 1], t[:, 0] / t[:, 2], t[:, 3] / t[:, 4], t[:, 5] / t[:, 6]]))
        want = SR.scores(*parts, C, lo, hi)
        assert np.isfinite(want).all() and np.abs(got - want).max() < 1e-9, (got, want)


def test_a_segment_reads_zero_outside_its_rows():
    rows = np.arange(1.0, 11.0)[None]
    assert BR.segment(rows, -3, 6).tolist() == [[0, 0, 0, 1, 2, 3]] and BR.segment(rows, 7, 5).tolist() == [[8, 9, 10, 0, 0]]
    assert BR.segment(rows, 2, 3).tolist() == [[3, 4, 5]] and BR.segment(rows, 12, 2).tolist() == [[0, 0]]
    R, D, aR, aD = BR.correlations_padded(rows, -rows, 8, 4, 3)              # the segment is 9, 10, 0, 0
    assert R[0, 0].tolist() == [0, 90, 181, 90, 0] and D[0, 0].tolist() == [-181, -90, 0]
    assert aR[0, 0].tolist() == [0, 90, 181, 90, 0] and aD[0, 0].tolist() == [181, 90, 0]


# ---- stage 2: the solve cases ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", BC.SOLVE_CASES, ids=BC.case_id)
def test_solve_cases_need_pivoting_and_are_well_conditioned(case):
    """Every system: the long-double elimination swaps at least M / 2 rows, the condition number is at most 1e6, and
    numpy.linalg.solve agrees with it (1e-9 of the largest unknown: cond * 2^-52 * a growth allowance)."""
    nseg, Pn, G, flen, _ = case
    R, D = BC.solve_inputs(case)
    M = G * flen
    for sys in range(nseg * (Pn // G)):
        A, b = BC.system(R, D, Pn, G, flen, sys)
        x, swaps, zero = BR.solve_ld(A, b)
        cond = np.linalg.cond(A)
        err = float(np.abs(np.linalg.solve(A, b) - x).max() / np.abs(x).max())
        print(f"{case} system {sys}: M = {M}, {swaps} swaps, cond {cond:.3g}, numpy against long double {err:.2e}")
        assert zero is None and 2 * swaps >= M and cond <= 1e6 and err <= 1e-9


def test_the_suites_signal_made_gram_matrices_never_swap():
    """Why the cases above exist: the Gram matrix of coloured noise (a row of test_gpu_score.CASES, its recipe and seed) is
    diagonally dominant enough that partial pivoting never leaves the diagonal."""
    S, C, L, flen = 2, 2, 3001, 16
    s, e = BC.coloured_mix(S * C, L, 1000 * S + 100 * C + flen)
    R, D = SR.correlations(s, e, flen)
    for rows in (list(range(S * C)), [0, 1]):
        A = SR.gram(R, rows, flen)
        b = np.stack([np.concatenate([D[i, q] for i in rows]) for q in rows], 1)
        x, swaps, zero = BR.solve_ld(A, b)
        assert swaps == 0 and zero is None and np.linalg.cond(A) < 100
        assert np.abs(np.linalg.solve(A, b) - x).max() <= 1e-12 * np.abs(x).max()


def test_solve_ld_reports_the_first_zero_pivot():
    rs = np.random.RandomState(0)
    A = rs.randn(6, 6)
    A[3, :] = 0.0
    A[:, 3] = 0.0
    x, swaps, zero = BR.solve_ld(A, rs.randn(6, 2))
    assert zero == 3 and (x == 0).all() and x.shape == (6, 2)
    assert BR.solve_ld(np.full((4, 4), np.nan), np.ones(4))[2] == 0
    A = np.array([[1.0, 2.0], [3.0, 4.0]])                                   # one swap; backward error of the exact solution
    x, swaps, zero = BR.solve_ld(A, np.array([5.0, 6.0]))
    assert swaps == 1 and zero is None and np.abs(x[:, 0] - np.array([-4.0, 4.5])).max() < 1e-18
    assert BR.backward_error(A, x, np.array([5.0, 6.0])) < 1e-19
    assert abs(BR.backward_error(A, np.array([-4.0, 4.0]), np.array([5.0, 6.0])) - 2.0 / (7.0 * 4.0 + 6.0)) < 1e-15


# ---- refusals of the entry points ------------------------------------------------------------------------------------
def test_entry_points_refuse_before_any_launch():
    """Every refusal is AVSEP_ERR_ARG (-1), or AVSEP_ERR_WORKSPACE (-3) for a workspace 8 bytes short: a launch on this
    machine would be AVSEP_ERR_LAUNCH.  The workspace queries return 0 for the arguments they share with a refused call."""
    L = P.lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    big = 1 << 40

    # avsep_bss_seg_corr
    def corr(refs=p, ests=p, Pn=2, Ln=1000, flen=16, starts=p, nseg=2, n=500, ws=p, nbytes=big, R=p, D=p):
        return L.avsep_bss_seg_corr(refs, ests, Pn, Ln, flen, starts, nseg, n, ws, nbytes, R, D, None)
    for kw in (dict(Pn=0), dict(Pn=9), dict(flen=0), dict(flen=513), dict(n=0), dict(n=-1), dict(Ln=0), dict(Ln=-5), dict(nseg=0),
               dict(nseg=65536), dict(refs=None), dict(ests=None), dict(starts=None), dict(ws=None), dict(R=None), dict(D=None)):
        assert corr(**kw) == ERR_ARG, kw
    q = L.avsep_bss_seg_corr_workspace_bytes
    need = q(2, 2, 500, 16)
    assert need == 8 * 2 * 2 * 2 * 2 * 1 * 16 and corr(nbytes=need - 8) == ERR_WORKSPACE
    assert q(65535, 8, 500, 512) > 0, "the largest accepted arguments are planned"
    for args in ((2, 0, 500, 16), (2, 9, 500, 16), (2, 2, 500, 0), (2, 2, 500, 513), (2, 2, 0, 16), (0, 2, 500, 16), (65536, 2, 500, 16)):
        assert q(*args) == 0, args

    # avsep_bss_solve_groups
    def solve(R=p, D=p, nseg=1, Pn=4, G=2, flen=16, ws=p, nbytes=big, C=p, info=p):
        return L.avsep_bss_solve_groups(R, D, nseg, Pn, G, flen, ws, nbytes, C, info, None)
    for kw in (dict(Pn=0), dict(Pn=9, G=3), dict(flen=0), dict(flen=513, G=1), dict(G=3), dict(G=0), dict(Pn=4, G=8), dict(Pn=8, G=8, flen=257),
               dict(Pn=6, G=6, flen=342), dict(nseg=0), dict(nseg=-1), dict(R=None), dict(D=None), dict(ws=None), dict(C=None),
               dict(info=None)):
        assert solve(**kw) == ERR_ARG, kw
    q = L.avsep_bss_solve_groups_workspace_bytes
    need = q(1, 4, 2, 16)
    assert need == 8 * 2 * 32 * 32 and solve(nbytes=need - 8) == ERR_WORKSPACE
    assert q(1, 8, 8, 256) == 8 * 2048 * 2048 and solve(Pn=8, G=8, flen=256, nbytes=8 * 2048 * 2048 - 8) == ERR_WORKSPACE, \
        "the largest system is accepted up to its workspace"
    for args in ((1, 0, 2, 16), (1, 9, 3, 16), (1, 4, 2, 0), (1, 4, 1, 513), (1, 4, 3, 16), (1, 4, 0, 16), (1, 8, 8, 257), (0, 4, 2, 16)):
        assert q(*args) == 0, args

    # avsep_bss_window_energies
    def energies(refs=p, ests=p, Pn=4, C=2, Ln=1000, flen=16, starts=p, nseg=2, n=500, C_all=p, C_own=p, rseg=p, roff=p, nrange=3,
                 rlen=515, ws=p, nbytes=big, sums=p):
        return L.avsep_bss_window_energies(refs, ests, Pn, C, Ln, flen, starts, nseg, n, C_all, C_own, rseg, roff, nrange, rlen, ws,
                                           nbytes, sums, None)
    for kw in (dict(Pn=0), dict(Pn=9, C=3), dict(flen=0), dict(flen=513), dict(C=3), dict(C=0), dict(C=8), dict(n=0), dict(n=-1), dict(Ln=0),
               dict(rlen=0), dict(rlen=-1), dict(nseg=0), dict(nrange=0), dict(nrange=65536), dict(refs=None), dict(ests=None),
               dict(starts=None), dict(C_all=None), dict(C_own=None), dict(rseg=None), dict(roff=None), dict(ws=None), dict(sums=None)):
        assert energies(**kw) == ERR_ARG, kw
    q = L.avsep_bss_window_energies_workspace_bytes
    need = q(3, 4, 515)
    assert need == 8 * 3 * 1 * 4 * 8 and energies(nbytes=need - 8) == ERR_WORKSPACE
    assert q(3, 4, 1025) == 2 * need and q(65535, 8, 1024) > 0
    for args in ((3, 0, 515), (3, 9, 515), (3, 4, 0), (3, 4, -1), (0, 4, 515), (65536, 4, 515)):
        assert q(*args) == 0, args
