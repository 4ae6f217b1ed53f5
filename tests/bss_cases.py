"""The case tables and seeded input makers of the per-stage BSS-eval gates (test_bss_stages_host.py pins their conditions on the
CPU, test_gpu_bss_stages.py runs the kernels on them).  numpy only.  Everything made here is cached and shared: never modify
what a maker returns."""
import numpy as np

import bss_stage_ref as BR
import score_ref as SR

GUARD = 1e6          # what the rows above and below an overhanging segment's rows hold: a broken guard reads it


def coloured_mix(P, L, seed):
    """test_gpu_score.make_inputs' recipe on P rows: AR(1)-coloured references, estimates from a random mixing matrix over all
    rows plus 3 % noise."""
    rs = np.random.RandomState(seed)
    s = rs.randn(P, L)
    s[:, 1:] += 0.6 * s[:, :-1]
    e = (np.eye(P) + 0.2 * rs.randn(P, P)) @ s + 0.03 * rs.randn(P, L)
    return s, e


def guarded(rows):
    """[P, L] -> [P + 2, L] whose first and last rows hold GUARD: the kernels get the middle P rows, so a read before or past
    a row stays inside the allocation and shows up in the result."""
    P, L = rows.shape
    buf = np.full((P + 2, L), GUARD)
    buf[1:P + 1] = rows
    return buf


def case_id(c):
    return "-".join(str(v) for v in c if not isinstance(v, (list, tuple, bool))) + ("-guard" if c[-1] is True else "")


# ---- stage 1: avsep_bss_seg_corr ---------------------------------------------------------------------------------------
# NG = ceil(flen / 8) lag groups, nsl = the largest power of two with nsl * NG <= 256 time slices: threads past nsl * NG idle
#              P  L     flen starts              n     guard rows
CORR_CASES = [(2, 900, 1, (3, 117, 599), 300, False),
              (3, 5000, 5, (1, 2222), 2047, False),              # NG 1, flen < 8: seven discarded lags
              (2, 6001, 13, (7, 1001, 3950), 2048, False),       # NG 2, exactly one chunk
              (2, 50, 13, (5, 46), 3, False),                    # a segment shorter than the filter
              (2, 5003, 24, (3, 2951), 2049, False),             # NG 3: 192 of 256 threads work; a chunk and one sample
              (1, 9001, 100, (11, 4903), 4097, False),           # NG 13: 208 threads; three chunks
              (2, 6000, 509, (9, 1234, 3499), 2500, False),      # NG 64, flen % 8 = 5
              (8, 2100, 8, (13, 1099), 1000, False),             # 128 jobs
              (2, 1500, 13, (-3, 305), 1200, True)]              # both segments overhang: starts -3 and L - n + 5

_corr = {}


def corr_inputs(case):
    """-> refs, ests [P, L] and per segment (R, D, absR, absD) of bss_stage_ref.correlations_padded."""
    if case not in _corr:
        P, L, flen, starts, n, _ = case
        s, e = coloured_mix(P, L, 7000 + 100 * P + flen)
        _corr[case] = (s, e, [BR.correlations_padded(s, e, a, n, flen) for a in starts])
    return _corr[case]


# ---- stage 2: avsep_bss_solve_groups -----------------------------------------------------------------------------------
# R and D are standard normal, not correlations of signals: general block-Toeplitz systems that need pivoting
#               nseg P  G  flen seed
SOLVE_CASES = [(1, 2, 2, 5, 1),                # M = 10
               (1, 3, 3, 13, 1),               # M = 39
               (3, 4, 2, 24, 1),               # M = 48, six systems
               (1, 8, 8, 5, 1),                # M = 40, eight right-hand sides
               (2, 8, 1, 7, 129),              # M = 7, sixteen systems of one right-hand side (a draw in which each swaps >= 4 rows)
               (1, 5, 5, 206, 1),              # M = 1030: threads own two rows, the second sweep is partial
               (1, 8, 8, 256, 1)]              # M = 2048 and the 144 KB LDS request
SMALL_SOLVES, LARGE_SOLVES = SOLVE_CASES[:5], SOLVE_CASES[5:]

_solve = {}


def solve_inputs(case):
    """-> R [nseg, P, P, 2 flen - 1], D [nseg, P(est), P(ref), flen] (the entry point's layouts)."""
    if case not in _solve:
        nseg, P, G, flen, seed = case
        rs = np.random.RandomState(9000 + 1000 * seed + 10 * P + G + flen)
        _solve[case] = (rs.randn(nseg, P, P, 2 * flen - 1), rs.randn(nseg, P, P, flen))
    return _solve[case]


def system(R, D, P, G, flen, sys):
    """System sys = seg * (P / G) + g of a call: the Gram matrix [M, M] and the right-hand sides [M, G]."""
    seg, base = sys // (P // G), (sys % (P // G)) * G
    A = SR.gram(R[seg], list(range(base, base + G)), flen)
    b = D[seg, base:base + G, base:base + G].transpose(1, 2, 0).reshape(G * flen, G)
    return A, b


_systems = {}


def solved_systems(case):
    """Per system of a case: A, b, numpy.linalg.solve's x; for the small cases also solve_ld's (x, swaps, zero column)."""
    if case not in _systems:
        nseg, P, G, flen, _ = case
        R, D = solve_inputs(case)
        out = []
        for sys in range(nseg * (P // G)):
            A, b = system(R, D, P, G, flen, sys)
            out.append({"A": A, "b": b, "np": np.linalg.solve(A, b), "ld": BR.solve_ld(A, b) if case in SMALL_SOLVES else None})
        _systems[case] = out
    return _systems[case]


# ---- stage 3: avsep_bss_window_energies --------------------------------------------------------------------------------
# ranges are (segment, offset); every range of a call has the same length rlen.  A segment index of -1 or nseg is invalid.
#             name        S  C  flen L      starts             n      ranges                                               rlen   guard
EN_CASES = [("flen1", 1, 1, 1, 1500, (0, 476), 1024, ((0, 0), (1, 0)), 1024, False),                     # exactly one chunk, no tail
            ("one-sample", 2, 1, 5, 1200, (7, 333), 800, ((0, 0), (1, 37), (0, 799), (1, 802), (0, 803)), 1, False),
            # segments of their own at offsets 0, 37, 1000, 1023; one from -5; one that starts inside the tail [2100, 2112);
            # one that runs past it (clipped)
            ("offsets", 1, 2, 13, 5000, (11, 1501, 2222), 2100,
             ((0, 0), (1, 37), (2, 1000), (0, 1023), (1, -5), (1, 2105), (2, 1500)), 1024, False),
            ("two-chunks", 4, 2, 24, 3000, (5, 901), 1999, ((0, 0), (1, 998), (0, -5), (1, 2000)), 1025, False),
            ("65-chunks", 2, 1, 5, 66100, (33, 77), 66000, ((0, 0), (1, 0)), 66004, False),                 # the reduce loop's second trip
            ("invalid", 2, 2, 100, 2500, (3, 700), 1500, ((0, 0), (-1, 0), (1, 37), (2, 0), (1, 1000)), 1024, False),
            ("overhang", 2, 1, 13, 1200, (-3, 205), 1000, ((0, 0), (1, 0), (0, -5), (1, 1000)), 1012, True)]

_en = {}


def en_inputs(case):
    """-> refs, ests [P, L], C_all [nseg, P flen, P], C_own [nseg S, C flen, C] (the entry point's layouts), and
    terms["f64"], terms["ld"] [nrange, S, 8] from bss_stage_ref.energy_terms in float64 and long double (zeros for an invalid
    segment)."""
    if case not in _en:
        name, S, C, flen, L, starts, n, ranges, rlen, _ = case
        P, nseg = S * C, len(starts)
        rs = np.random.RandomState(5000 + 100 * P + flen + len(name))
        s = rs.randn(P, L)
        s[:, 1:] += 0.6 * s[:, :-1]
        e = rs.randn(P, L)                                     # independent noise: none of the eight terms cancels
        C_all = rs.randn(nseg, P * flen, P) / np.sqrt(P * flen)
        C_own = rs.randn(nseg * S, C * flen, C) / np.sqrt(C * flen)
        terms = {}
        for dt in (np.float64, np.longdouble):
            t = np.zeros((len(ranges), S, 8), dt)
            for i, (seg, off) in enumerate(ranges):
                if 0 <= seg < nseg:
                    t[i] = BR.energy_terms(s, e, C, flen, starts[seg], n, C_all[seg], C_own[seg * S:seg * S + S], off, rlen, dt)
            terms["ld" if dt is np.longdouble else "f64"] = t
        _en[case] = (s, e, C_all, C_own, terms)
    return _en[case]
