"""The rows of the Wiener filter's per-entry gates: test_mwf_gates_host.py runs them through the float32
controls and the mutants without a device, test_gpu_mwf_gates.py through kernels._mwf_cov / _mwf_apply.  Every row runs BOTH
launchers of its filter: H = 0 is avsep_mwf_cov / avsep_mwf_apply (TV = false), H > 0 avsep_mwf_cov_tv / avsep_mwf_apply_tv.
Fin = 5 throughout; the largest tensor of a row is 3.3 MB (I15's ymag).

Inputs (``inputs``): float32, seeded, drawn on the CPU.
  * kind "mix": masks U(0, 1) on a complex normal mixture of magnitude about 30 (mwf_ref.value_inputs' draw): well conditioned
    once a row has enough loud frames; "rank1": mwf_ref.panned_sources (H = 0) or mwf_tv_ref.moving_sources (H > 0): every
    source's covariance is nearly h h^H and kappa_2(S) reaches C / reg;
  * |X| decays by 80 dB along t, 10^(-4 frac(t / F + phi_f)), phi = DECAY_PHASE per bin row: every row's jump from -80 dB back
    to 0 dB sits at another frame, so a chunk's or a segment's last frame is loud in one bin row at least;
  * bin row 3 is 120 dB below the others, bin row 2 is exactly zero in xmag and ymag;
  * the last source is exactly zero over frames [1, 2 H) where F > 2 H (the whole support of centre 1: R[N-1, 1] = 0), else
    over [F // 4, F // 2);
  * ``pps`` rows hand the covariance a phase per source [N,C,Fin,F] (phase_stride = C Fin F): random phases on "mix" rows,
    the mixture's phase repeated on "rank1" rows (random ones would destroy the rank); the others the shared [C,Fin,F] one.
The smallest non-zero reference intermediate over all rows (a^2, v, lam, the diagonal of S, ||z||; bins where every source
is silent have S = FLT_MIN I by definition and are not counted) is 5.4e-31 (row T07; the host test prints it per row and asserts
1e-32, six orders above FLT_MIN = 1.2e-38): subnormals are out of scope.

MEASURED holds the worst |error| / bound per launcher on an MI355X, from the output of test_gpu_mwf_gates.py
(profiles/mwf_gates_mi355x.txt): at most 0.111 for a covariance and 0.055 for an image."""
import numpy as np

import mwf_ref as M
import mwf_tv_ref as T

FIN = M.FIN
F_LONG = M.F_LONG                                   # 4173 = 2 * 2048 + 77
DECAY_PHASE = (0.0, 0.2, 0.4, 0.6, 0.8)
ZERO_ROW, QUIET_ROW = 2, 3

# id: (H, C, N, F, kind, pps, reg, note)
ROWS = {
    # ---- TV = false -------------------------------------------------------------------------------------------------
    "I01": (0, 1, 1, 1, "mix", False, 1e-3, "C = 1; one frame: a chain of one term, R = 1 exactly where the row is not silent"),
    "I02": (0, 2, 4, 63, "mix", True, 1e-3, "N = 4 at C = 2; a lone ragged wave"),
    "I03": (0, 3, 2, 64, "mix", False, 1e-3, "C = 3; exactly one wave of frames"),
    "I04": (0, 4, 4, 2048, "mix", True, 1e-3, "C = 4 well conditioned; one whole chunk, every thread's chain is 8 terms"),
    "I05": (0, 4, 3, 130, "rank1", False, 1e-3, "C = 4 rank 1 (the issue's row): S is rank 3 of 4 without lam"),
    "I06": (0, 5, 2, 255, "mix", True, 1e-3, "C = 5 well conditioned: one frame short of the block"),
    "I07": (0, 5, 8, 256, "rank1", True, 1e-3, "C = 5 rank 1, N = 8 (bins with five sources and more are full rank); one full apply tile"),
    "I08": (0, 6, 2, 257, "mix", False, 1e-3, "C = 6 well conditioned; a one-frame last apply tile, chains of 2 and 1"),
    "I09": (0, 6, 3, 63, "rank1", False, 1e-3, "C = 6 rank 1"),
    "I10": (0, 7, 3, 2047, "mix", True, 1e-3, "C = 7 well conditioned; chain of 8 with a ragged tail (thread 255 has 7)"),
    "I11": (0, 7, 2, 65, "rank1", False, 1e-3, "C = 7 rank 1; 65 frames: a second wave with one frame"),
    "I12": (0, 8, 8, 63, "mix", False, 1e-3, "N = 8, C = 8: all 8 * 128 floats of s_R, every `n < N` guard true"),
    "I13": (0, 2, 1, 65, "mix", True, 1e-3, "N = 1 at C = 2"),
    "I14": (0, 8, 1, 2049, "mix", False, 1e-3, "N = 1 at C = 8; two chunks, the last of one frame"),
    "I15": (0, 2, 5, F_LONG, "mix", True, 1e-3, "N = 5 at C = 2; three chunks (2048, 2048, 77), 17 apply tiles"),
    "I16": (0, 8, 4, 256, "mix", True, 1e-3, "N = 4 at C = 8"),
    "I17": (0, 2, 8, 300, "rank1", False, 1e-3, "N = 8 at C = 2"),
    "I18": (0, 2, 2, 300, "rank1", True, 1e-3, "the issue's rank-1 stereo row, kappa to C / reg = 2000"),
    "I19": (0, 8, 5, 64, "rank1", False, 1e-3, "N = 5 at C = 8, rank 1"),
    "I20": (0, 4, 2, 65, "mix", False, 1.0, "reg = 1: lam is the size of S"),
    "I21": (0, 2, 3, 257, "mix", False, 0.0, "reg = 0 on a well-conditioned row (asserted: kappa < 1e3): lam = FLT_MIN"),
    "I22": (0, 3, 3, 2049, "rank1", True, 1e-3, "C = 3 rank 1; the one-frame chunk with a phase per source"),
    # ---- TV = true --------------------------------------------------------------------------------------------------
    "T01": (64, 1, 1, 64, "mix", False, 1e-3, "C = 1; F = H: one segment, the last centre one past the last frame"),
    "T02": (64, 2, 1, 65, "mix", True, 1e-3, "N = 1 at C = 2; F = H + 1: a segment of one frame at u = 0"),
    "T03": (64, 3, 2, 128, "mix", False, 1e-3, "C = 3; F = 2 H"),
    "T04": (64, 4, 4, 129, "mix", True, 1e-3, "C = 4 well conditioned, N = 4 at C = 4; F = 2 H + 1"),
    "T05": (64, 4, 3, 300, "rank1", False, 1e-3, "C = 4 rank 1; 5 segments: three idle waves of the second workgroup return"),
    "T06": (64, 5, 8, 512, "rank1", True, 1e-3, "C = 5 rank 1, N = 8 (as I07); 8 segments: two full workgroups"),
    "T07": (64, 2, 2, F_LONG, "rank1", False, 1e-3, "66 segments, 67 centres; every apply tile meets five centres; the last tile's staging clamps to centre 66"),
    "T08": (192, 5, 3, 192, "mix", False, 1e-3, "C = 5 well conditioned; F = H = 192 (lane chain of 3)"),
    "T09": (192, 6, 2, 193, "mix", True, 1e-3, "C = 6 well conditioned (NOUT = 2); F = H + 1"),
    "T10": (192, 6, 2, 384, "rank1", False, 1e-3, "C = 6 rank 1; F = 2 H: tile 1 starts in segment 1 at frame 256"),
    "T11": (192, 7, 3, 385, "mix", False, 1e-3, "C = 7 well conditioned; F = 2 H + 1"),
    "T12": (192, 7, 2, 257, "rank1", True, 1e-3, "C = 7 rank 1; H does not divide the tile: seg - k0 = 1 in tile 0, one-frame tile 1"),
    "T13": (192, 8, 8, 513, "mix", True, 1e-3, "N = 8, C = 8: the LDS maximum of s_R, 5 * 8 * 128 floats (NOUT = 3); seg - k0 = 1 in tiles 0 and 1"),
    "T14": (4096, 2, 4, 1, "mix", False, 1e-3, "N = 4 at C = 2; F = 1: one centre, K - 1 = 0 clamps both reads"),
    "T15": (4096, 8, 1, 63, "mix", False, 1e-3, "N = 1 at C = 8; F < H = 4096"),
    "T16": (4096, 2, 5, 100, "rank1", False, 1e-3, "N = 5 at C = 2; F < H"),
    "T17": (4096, 3, 2, 4097, "mix", True, 1e-3, "lane chain of 64 terms; the second segment is one frame at u = 0"),
    "T18": (64, 2, 8, 257, "mix", False, 1e-3, "N = 8 at C = 2"),
    "T19": (64, 8, 4, 257, "mix", False, 1e-3, "N = 4 at C = 8; a one-frame last tile whose staging clamps four of its five centres"),
    "T20": (64, 8, 5, 65, "mix", True, 1e-3, "N = 5 at C = 8"),
    "T21": (64, 3, 2, 129, "mix", False, 1.0, "reg = 1 under TV"),
    "T22": (192, 1, 3, 513, "mix", True, 1e-3, "C = 1 at a span that is no power of two: the weights are rounded"),
    # ---- leaks ------------------------------------------------------------------------------------------------------
    "L01": (0, 2, 4, 257, "mix", False, 1e-3, "only source 1 sounds: the others' covariances and images are exactly 0"),
    "L02": (0, 6, 2, 130, "mix", True, 1e-3, "channel 3 exactly zero: its row and column of every R and its output are exactly 0"),
    "L03": (64, 3, 4, 129, "mix", True, 1e-3, "L01 under TV"),
    "L04": (192, 6, 2, 257, "mix", False, 1e-3, "L02 under TV"),
}
LEAK_SOURCE, LEAK_CHANNEL = 1, 3

# worst |error| / bound on an MI355X, (covariance launcher, apply launcher); test_gpu_mwf_gates.py prints them
MEASURED = {
    "I01": (0.0417, 0.00946), "I02": (0.0754, 0.0288), "I03": (0.0652, 0.0127), "I04": (0.0497, 0.0255), "I05": (0.1, 0.000216),
    "I06": (0.073, 0.00768), "I07": (0.0805, 0.000203), "I08": (0.0579, 0.00468), "I09": (0.0777, 4.63e-05), "I10": (0.0584, 0.0157),
    "I11": (0.111, 3.17e-05), "I12": (0.0696, 0.00067), "I13": (0.0563, 0.0139), "I14": (0.0397, 0.00734), "I15": (0.0576, 0.0552),
    "I16": (0.0625, 0.00505), "I17": (0.0823, 0.00661), "I18": (0.0452, 0.013), "I19": (0.0736, 5.33e-05), "I20": (0.0606, 0.0155),
    "I21": (0.066, 0.0288), "I22": (0.0431, 0.00263), "L01": (0.0448, 0.0298), "L02": (0.096, 2.53e-05), "L03": (0.0662, 0.0148),
    "L04": (0.0561, 1.62e-05), "T01": (0.0465, 0.0453), "T02": (0.0517, 0.00875), "T03": (0.0956, 0.018), "T04": (0.0882, 0.0135),
    "T05": (0.111, 0.000518), "T06": (0.0923, 0.000402), "T07": (0.0787, 0.0299), "T08": (0.0722, 0.00637), "T09": (0.0683, 0.00492),
    "T10": (0.0748, 0.000137), "T11": (0.0864, 0.0089), "T12": (0.0688, 2.88e-05), "T13": (0.0646, 0.0116), "T14": (0.0186, 1.63e-05),
    "T15": (0.0163, 5.49e-05), "T16": (0.0179, 0.0293), "T17": (0.0184, 0.0381), "T18": (0.0956, 0.0378), "T19": (0.073, 0.00716),
    "T20": (0.0791, 0.00189), "T21": (0.0733, 0.0268), "T22": (0.0577, 0.0495),
}


def row(rid):
    H, C, N, F, kind, pps, reg, note = ROWS[rid]
    return {"id": rid, "H": H, "C": C, "N": N, "F": F, "kind": kind, "pps": pps, "reg": reg, "note": note}


def silent_run(F, H):
    """frames over which the last source is exactly zero"""
    return (1, 2 * H) if H and F > 2 * H else (F // 4, F // 2)


def decay(F):
    """[FIN, F] amplitude factors: 80 dB of exponential decay with another phase per bin row, row 3 at -120 dB, row 2 zero"""
    t = np.arange(F)[None, :] / float(F)
    g = 10.0 ** (-4.0 * np.mod(t + np.array(DECAY_PHASE)[:, None], 1.0))
    g[QUIET_ROW] *= 1e-6
    g[ZERO_ROW] = 0.0
    return g


def inputs(rid):
    """-> dict of float32 arrays: xmag, xph [C,FIN,F], ymag [N,C,FIN,F], yph [C,FIN,F] or [N,C,FIN,F]"""
    r = row(rid)
    H, C, N, F = r["H"], r["C"], r["N"], r["F"]
    seed = 7000 + sorted(ROWS).index(rid)
    g = np.random.default_rng(seed)
    if r["kind"] == "mix":
        X = 30.0 * (g.standard_normal((C, FIN, F)) + 1j * g.standard_normal((C, FIN, F))) / np.sqrt(2.0)
        xmag, xph = np.abs(X), np.angle(X).astype(np.float32)
        mask = g.random((N, FIN, F))
        ymag = mask[:, None] * xmag[None]
    else:
        sc = T.moving_sources(C, N, FIN, F, seed) if H else M.panned_sources(C, N, FIN, F, seed)
        xmag, xph, ymag = sc["xmag"].astype(np.float64), sc["xph"], sc["ymag"].astype(np.float64)
    d = decay(F)
    xmag, ymag = (xmag * d).astype(np.float32), (ymag * d).astype(np.float32)
    a, b = silent_run(F, H)
    ymag[N - 1, :, :, a:b] = 0
    if rid in ("L01", "L03"):
        ymag[np.arange(N) != LEAK_SOURCE] = 0
    if rid in ("L02", "L04"):
        xmag[LEAK_CHANNEL], ymag[:, LEAK_CHANNEL] = 0, 0
    if not r["pps"]:
        yph = xph
    elif r["kind"] == "mix":
        yph = g.uniform(-np.pi, np.pi, ymag.shape).astype(np.float32)
    else:
        yph = np.ascontiguousarray(np.broadcast_to(xph, ymag.shape))
    return {"xmag": xmag, "xph": xph, "ymag": ymag, "yph": yph}


# what the rows are aimed at ------------------------------------------------------------------------------------------------
def rank1(rid):
    return ROWS[rid][4] == "rank1"


MUTANT_ROWS = {
    # mutant: (launcher, rows)
    1: ("cov", [r for r in ROWS if ROWS[r][1] >= 2]),
    2: ("cov", [r for r in ROWS if ROWS[r][1] >= 3]),
    3: ("cov", [r for r in ROWS if ROWS[r][0] == 0 and ROWS[r][3] >= 2048]),
    # C = 1 has R = 1 whatever the weights are
    # ... and F >= H: on a short row at H = 4096 the weights 1 - j / 4097 and 1 - j / 4096 differ by 6e-6 at the most, and a
    # common factor on every u cancels in sum u Y Y^H / sum u v
    4: ("cov", [r for r in ROWS if ROWS[r][0] and ROWS[r][3] >= ROWS[r][0] and ROWS[r][1] >= 2]),
    # seen where a frame reads the last centre with u > 0 (on a short row at H = 4096 u stays below F / H = 0.025), C >= 2
    5: ("apply", [r for r in ROWS if ROWS[r][0] and ROWS[r][3] >= ROWS[r][0] and (ROWS[r][3] - 1) % ROWS[r][0] != 0 and ROWS[r][1] >= 2]),
    6: ("cov", [r for r in ROWS if ROWS[r][0] and ROWS[r][3] > 1 and ROWS[r][1] >= 2]),
    7: ("apply", [r for r in ROWS if rank1(r)]),
    8: ("cov", [r for r in ROWS if ROWS[r][2] >= 4 and r[0] != "L"]),
    9: ("both", [r for r in ROWS if ROWS[r][1] == 7]),
    # time-invariant rows: the old gate it must pass is mwf_ref.BOUND_Y = 3.04e-5 (mwf_tv_ref.BOUND_Y is below 1e-5)
    10: ("apply", ["I04", "I10", "I14", "I15"]),
}
