"""not-gpu: the Wiener filter's per-entry gates proven without a device.  The rows of mwf_cases.py reach what
their notes claim; the float64 reference with bounds (mwf_gates_ref.py) is the existing restatement to 1e-12 of the per-bin
scale; the float32 controls pass every gate on every row; every mutant fails every row it is aimed at.  Run with -s for the
worst ratio per row and the factor of every mutant."""
import numpy as np
import pytest

import avsep_amd

import mwf_cases as Cs
import mwf_gates_ref as G
import mwf_ref as M
import mwf_tv_ref as T

R = {rid: Cs.row(rid) for rid in Cs.ROWS}


def _where(**kw):
    return [r for r in R.values() if all(r[k] == v for k, v in kw.items())]


def test_rows_reach_what_their_notes_claim():
    lib = avsep_amd.lib.load()
    for r in R.values():
        H, C, N, F = r["H"], r["C"], r["N"], r["F"]
        got = lib.avsep_mwf_tv_workspace_bytes(N, C, Cs.FIN, F, H) if H else lib.avsep_mwf_workspace_bytes(N, C, Cs.FIN, F)
        assert got == G.workspace_bytes(N, C, Cs.FIN, F, H) > 0, r["id"]
        assert max(x.nbytes for x in Cs.inputs(r["id"]).values()) <= 4 << 20
    # every instantiation of both kernel templates: C = 1 ... 8 under both TV; C = 4 ... 7 well conditioned and rank 1 under both
    for tv in (False, True):
        rows = [r for r in R.values() if bool(r["H"]) == tv and r["id"][0] != "L"]
        assert {r["C"] for r in rows} == set(range(1, 9))
        for C in (4, 5, 6, 7):
            assert {r["kind"] for r in rows if r["C"] == C} == {"mix", "rank1"}, (tv, C)
        for C in (2, 8):
            assert {r["N"] for r in rows if r["C"] == C} >= {1, 4, 5, 8}, (tv, C)
        assert any(r["pps"] for r in rows) and any(not r["pps"] for r in rows)
    assert {r["F"] for r in _where(H=0)} >= {1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, Cs.F_LONG}
    assert {(r["H"], r["F"]) for r in R.values() if r["H"]} >= {
        (64, 64), (64, 65), (64, 128), (64, 129), (192, 192), (192, 193), (192, 384), (192, 385), (192, 257), (192, 513),
        (64, Cs.F_LONG), (4096, 1), (4096, 63), (4096, 100), (4096, 4097)}
    assert {r["reg"] for r in R.values()} == {1e-3, 1.0, 0.0} and [r["id"] for r in _where(reg=0.0)] == ["I21"]
    # chunks, chains and tiles
    assert [G.chunks(R[i]["F"]) for i in ("I04", "I10", "I14", "I15", "I22")] == [1, 1, 2, 3, 2]
    assert Cs.F_LONG - 2 * G.CHUNK == 77 and R["I14"]["F"] - G.CHUNK == 1 and R["I08"]["F"] - G.BLOCK == 1
    assert G.K["cov.chain"](2047, 0) == G.K["cov.chain"](2048, 0) == G.K["cov.chain"](Cs.F_LONG, 0) == 8 and G.K["cov.chain"](257, 0) == 2
    # segments, centres, spans
    seg = {i: G.cdiv(R[i]["F"], R[i]["H"]) for i in R if R[i]["H"]}
    cen = {i: T.centres(R[i]["F"], R[i]["H"]) for i in R if R[i]["H"]}
    assert seg["T05"] == 5 and seg["T06"] == 8 and (seg["T07"], cen["T07"]) == (66, 67)
    assert cen["T14"] == 1 and cen["T01"] == 2 and cen["T02"] == 2 and cen["T17"] == 2 and seg["T17"] == 2 and cen["T15"] == 2
    assert G.K["cov.chain"](4097, 4096) == 64 and G.K["cov.chain"](192, 192) == 3
    for i in ("T12", "T13"):                                                    # the span does not divide the 256-frame tile
        assert 256 % R[i]["H"] != 0
    def reach(i):                                                               # the largest seg - k0 over the row's waves
        return max(w // R[i]["H"] - (w // 256 * 256) // R[i]["H"] for w in range(0, R[i]["F"], 64))
    assert [reach(i) for i in ("T12", "T13", "T22", "T07", "T19", "T17")] == [1, 1, 1, 3, 3, 0]     # H = 192 cannot reach 2
    # NOUT of the TV store and the LDS of s_R
    assert [G.nout(C) for C in range(1, 9)] == [1, 1, 1, 1, 1, 2, 2, 3]
    assert (R["T13"]["N"], R["T13"]["C"]) == (8, 8) and 5 * 8 * 2 * 8 * 8 * 4 == 20480
    # the silent run covers centre 1's whole support where the row has it
    for i in ("T05", "T06", "T07", "T11", "T13"):
        a, b = Cs.silent_run(R[i]["F"], R[i]["H"])
        W = T.hat_weights(R[i]["F"], R[i]["H"])
        assert (W[1, :a] == 0).all() and (W[1, b:] == 0).all() and (Cs.inputs(i)["ymag"][-1, :, :, a:b] == 0).all()
    for m, (_, rows) in Cs.MUTANT_ROWS.items():
        assert rows and set(rows) <= set(R), m
    assert set(Cs.MEASURED) == set(R) and all(0 <= q < 1 for pair in Cs.MEASURED.values() for q in pair)


def test_constants_are_the_sums_of_their_terms():
    """k_cov and k_apply at the corners, written out (the table G.K holds the source lines)."""
    # invariant, C = 2, F = 4173: num 12 + 8 + 6 + 3 + 3 = 32 -> ceil(sqrt 2 * 32) = 46; den 4 + 8 + 6 + 3 + 3 = 24; division 1
    assert G.k_cov(2, Cs.F_LONG) == 46 + 24 + 1
    # TV, H = 64 (weights exact), C = 8: num 12 + 1 + 1 + 6 + 1 = 21 -> 30; den 10 + 1 + 1 + 6 + 1 = 19
    assert G.k_cov(8, 513, 64) == 30 + 19 + 1
    # TV, H = 192: the weights are rounded, 2 in place of 1; what w inherits from u is counted per entry (cov_ref's kw <= 2 H)
    assert G.k_cov(8, 513, 192) == 34 + 22 + 1
    assert G.k_weight(64) == G.k_weight(4096) == G.k_weight(0) == 0 and G.k_weight(192) == 192
    assert list(G.k_weight(192, [0, 96, 190, 191])) == [1, 2, 96, 192] and list(G.k_weight(64, [0, 63])) == [0, 0]
    # apply, C = 2, N = 2: S 4 + 1 + 2 = 7, lam 7, solve ceil(2.83 * 7) = 20, X 5, R z ceil(1.414 * (5 + 4 + 1)) = 15, polar 13
    assert G.k_apply(2, 2) == 7 + 7 + 20 + 5 + 15 + 13
    assert G.k_apply(8, 8) == 19 + 13 + 71 + 5 + 32 + 13
    assert G.k_apply(8, 8, 64) == G.k_apply(8, 8) + 2 + 2 and all(G.k_apply(C, N) < 160 for C in range(1, 9) for N in range(1, 9))


def _exact_cov_statements(cov, absref):
    re, im = cov.real, cov.imag
    assert (np.diagonal(im, axis1=-2, axis2=-1) == 0).all()
    assert np.array_equal(re, np.swapaxes(re, -1, -2)) and (im == -np.swapaxes(im, -1, -2)).all()
    assert (cov[absref == 0] == 0).all()


@pytest.mark.parametrize("rid", sorted(Cs.ROWS))
def test_reference_controls_and_mutants(rid):
    r, x = R[rid], Cs.inputs(rid)
    H, C, N, F, reg = r["H"], r["C"], r["N"], r["F"], r["reg"]
    xmag, xph, ymag, yph = x["xmag"], x["xph"], x["ymag"], x["yph"]
    assert all(a.dtype == np.float32 for a in x.values()) and yph.ndim == (4 if r["pps"] else 3)
    kc, ka = G.k_cov(C, F, H), G.k_apply(C, N, H, F)
    # -- covariance: the reference is the restatement; the control is inside the gate -----------------------------------
    ref_c, absref, v, kw = G.cov_ref(ymag, yph, H)
    old = (T.cov(ymag, yph, H) if H else M.cov(ymag, yph))[0]
    assert old.shape == ref_c.shape and (np.abs(ref_c - old) <= 1e-12 * absref).all()
    cc = G.cov_control(ymag, yph, H)
    assert cc.dtype == np.complex64 and cc.shape == ref_c.shape
    rc, zc = G.cov_gate(cc, ref_c, absref, kc, kw)
    _exact_cov_statements(cc, absref)
    # -- apply on the control's fp32 covariances -------------------------------------------------------------------------
    ref = G.apply_ref(xmag, xph, ymag, cc, H, reg)
    reg64 = float(np.float32(reg))
    c128 = cc.astype(np.complex128)
    oldY = T.apply(xmag, xph, v, c128, H, reg64) if H else M.apply(xmag, xph, v, c128, reg64)
    assert (np.sqrt((np.abs(ref["Y"] - oldY) ** 2).sum(1)) <= 1e-12 * ref["scale"]).all()
    mag, ph = G.apply_control(xmag, xph, ymag, cc, H, reg)
    assert np.isfinite(mag).all() and np.isfinite(ph).all() and (mag >= 0).all() and (np.abs(ph) <= np.float32(np.pi)).all()
    assert (mag[np.broadcast_to(v[:, None] == 0, mag.shape)] == 0).all() and (ph[np.broadcast_to(v[:, None] == 0, ph.shape)] == 0).all()
    Yc = M.polar_to_complex(mag, ph)
    ra, za = G.apply_gate(Yc, ref, ka)
    a2 = ymag[ymag > 0].astype(np.float64) ** 2
    small = min(ref["small"], float(a2.min()))
    kmax = float(ref["kappa"].max())
    print(f"{rid} H={H} C={C} N={N} F={F} {r['kind']}: k_cov {kc}+{int(np.max(kw))} control {rc:.3f}; k_apply {int(ka.min())}..{int(ka.max())} control {ra:.3f}; "
          f"kappa <= {kmax:.3g}; smallest intermediate {small:.2e}")
    assert rc <= 1 and zc == 0 and ra <= 1 and za == 0
    assert small >= 1e-32                                                           # six orders above FLT_MIN: no subnormals
    if reg == 0.0:
        assert kmax < 1e3
    if rid in ("L01", "L03"):
        off = np.arange(N) != Cs.LEAK_SOURCE
        assert (cc[off] == 0).all() and (mag[off] == 0).all() and (ph[off] == 0).all() and np.abs(cc[Cs.LEAK_SOURCE]).max() > 0.1
    if rid in ("L02", "L04"):
        q = Cs.LEAK_CHANNEL
        assert (cc[..., q, :] == 0).all() and (cc[..., :, q] == 0).all() and (mag[:, q] == 0).all() and (ph[:, q] == 0).all()
    # -- mutants ------------------------------------------------------------------------------------------------------------
    for m, (launcher, rows) in sorted(Cs.MUTANT_ROWS.items()):
        if rid not in rows:
            continue
        if launcher in ("cov", "both"):
            f, z = G.cov_gate(G.cov_control(ymag, yph, H, mutant=m), ref_c, absref, kc, kw)
            print(f"    mutant {m} ({G.MUTANTS[m]}), covariance: {f:.3g} x the bound, {z} entries that must be 0 are not")
            assert f > 1 or z > 0, (m, rid)
        if m == 10:
            bad, level = G.quiet_bin_error(ref["Y"], Yc)
            assert 0.5e-4 <= level <= 2e-4
            f, z = G.apply_gate(bad, ref, ka)
            old_gate = M.rel_err(bad, ref["Y"])
            print(f"    mutant 10 at a bin {20 * np.log10(level):.1f} dB down: old gate {old_gate:.2e} <= {M.BOUND_Y:.2e}; new gate {f:.3g} x the bound")
            assert old_gate <= M.BOUND_Y and f > 1
        elif launcher in ("apply", "both"):
            f, z = G.apply_gate(M.polar_to_complex(*G.apply_control(xmag, xph, ymag, cc, H, reg, mutant=m)), ref, ka)
            print(f"    mutant {m} ({G.MUTANTS[m]}), apply: {f:.3g} x the bound")
            assert f > 1 or z > 0, (m, rid)
