"""gpu: avsep_amd.score.score_stems and the three entry points of csrc/bss_windows.hip against the numpy restatement
tests/score_ref.py (pinned on the CPU by test_score_host.py), the batch scorer bss_eval_sources on the same kernels against
oracle/bss_eval.py, and both for determinism."""
import json

import numpy as np
import pytest
import torch

import score_ref as SR
from conftest import assert_close
from recipes import score as _score

pytestmark = pytest.mark.gpu
NAMES = ("sdr", "isr", "sir", "sar")
DB_TOL = 1e-3

#         S  C  L     flen win   hop
CASES = [(2, 1, 3000, 16, 1000, 500),        # overlapping windows
         (2, 2, 3001, 16, 1000, 1000),       # a dropped remainder of 1
         (3, 1, 2500, 32, 800, 400),         # three sources
         (3, 2, 2200, 8, 700, 700),          # six rows and six right-hand sides
         (2, 2, 6000, 512, 6000, 6000),      # the 2048-unknown limit, one window
         (2, 2, 4453, 16, 1453, 1000),       # two 2048-sample chunks of the correlation kernel and an odd remainder of 357:
#                                              windows start inside a chunk (1000, 3000) and the last one ends exactly at L
         (2, 2, 2500, 13, 900, 450),         # flen no multiple of 8: discarded lags and zero-padded taps
         (3, 1, 2300, 24, 700, 700)]         # three groups of 8 lags: 64 of the correlation kernel's 256 threads idle


def make_inputs(S, C, L, seed):
    """Coloured sources, estimates from a random mixing matrix over ALL rows plus 3 % noise (test_bss_eval_kernels_vs_oracle's
    recipe, across channels)."""
    rs = np.random.RandomState(seed)
    P = S * C
    s = rs.randn(P, L)
    s[:, 1:] += 0.6 * s[:, :-1]
    e = (np.eye(P) + 0.2 * rs.randn(P, P)) @ s + 0.03 * rs.randn(P, L)
    return s.reshape(S, C, L), e.reshape(S, C, L)


_cache = {}


def case_data(case):
    """Inputs and the restatement's result in both filter modes, computed once per case and shared (never modified)."""
    if case not in _cache:
        S, C, L, flen, win, hop = case
        s, e = make_inputs(S, C, L, 1000 * S + 100 * C + flen)
        _cache[case] = (s, e, {f: SR.score_stems(s, e, win, hop, f, flen, permute=False) for f in ("track", "window")})
    return _cache[case]


def assert_scores(got, ref, what, need_all=True):
    """Every score within 1e-3 dB of the restatement; with need_all, every restatement score must be finite and below 100 dB,
    so that no comparison is skipped."""
    n = 0
    for k in NAMES:
        for g, r, where in [(got[k], ref[k], "median"), (got["frames"][k], ref["frames"][k], "frames")] + \
                           ([(got["track"][k], ref["track"][k], "track")] if "track" in ref else []):
            g, r = g.cpu().numpy(), np.asarray(r)
            assert g.shape == r.shape, (what, k, where, g.shape, r.shape)
            ok = np.isfinite(r) & (r < 100)
            if need_all:
                assert ok.all(), f"{what} {k} {where}: the restatement is not finite and below 100 dB everywhere: {r}"
            print(f"{what} {k} {where}: max |d| = {np.abs(g - r)[ok].max() if ok.any() else 0:.3e} dB over {ok.sum()} values")
            assert np.all(np.abs(g - r)[ok] < DB_TOL), (what, k, where, g, r)
            n += int(ok.sum())
    return n


@pytest.mark.parametrize("filters", ["track", "window"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "S%d-C%d-L%d-f%d-w%d-h%d" % c)
def test_scores_against_the_restatement(dev, case, filters):
    S, C, L, flen, win, hop = case
    s, e, ref = case_data(case)
    got = _score().score_stems(torch.from_numpy(s).to(dev), torch.from_numpy(e).to(dev), win, hop, filters, flen, permute=False)
    assert got["window_starts"] == ref[filters]["window_starts"] and got["perm"] == list(range(S))
    assert ("track" in got) == (filters == "track")
    assert_scores(got, ref[filters], f"{case} {filters}")


@pytest.mark.parametrize("case", CASES, ids=lambda c: "S%d-C%d-L%d-f%d-w%d-h%d" % c)
def test_correlations_and_solved_systems(dev, case):
    """The pieces: R and D of the whole recording and of the windows against np.correlate (1e-11), one own-source and one
    all-sources system against numpy.linalg.solve on the same Gram matrix (1e-6)."""
    SC = _score()
    S, C, L, flen, win, hop = case
    P = S * C
    s, e, _ = case_data(case)
    rr, er = torch.from_numpy(s.reshape(P, L)).to(dev), torch.from_numpy(e.reshape(P, L)).to(dev)
    starts, wlen = SR.plan_windows(L, win, hop)
    for seg_starts, n in (([0], L), (starts, wlen)):
        R, D = SC.seg_corr(rr, er, flen, seg_starts, n)
        for i, a in enumerate(seg_starts):
            Rn, Dn = SR.correlations(s.reshape(P, L)[:, a:a + n], e.reshape(P, L)[:, a:a + n], flen)
            assert_close(R[i], torch.from_numpy(Rn), 1e-11, f"lagged correlations, segment {a}+{n}")
            assert_close(D[i], torch.from_numpy(Dn.transpose(1, 0, 2).copy()), 1e-11, f"right-hand sides, segment {a}+{n}")
    R, D = SC.seg_corr(rr, er, flen, [0], L)
    for G in (C, P):
        Cf = SC.solve_groups(R, D, G, flen)
        assert Cf.shape == (P // G, G * flen, G)
        g = P // G - 1                                                        # the last group
        rows = list(range(g * G, g * G + G))
        A = SC._gram(R, 0, rows, flen).cpu().numpy()
        rhs = D[0, g * G:g * G + G, g * G:g * G + G].permute(1, 2, 0).reshape(G * flen, G).cpu().numpy()
        assert_close(Cf[g], torch.from_numpy(np.linalg.solve(A, rhs)), 1e-6, f"filters of a group of {G} rows vs numpy.linalg.solve")


def test_correlations_many_chunks_per_block(dev):
    """Past 128 chunks of 2048 samples a block of the correlation kernel walks more than one chunk: 130 chunks and an odd
    remainder, two segments that start at odd offsets, against np.correlate."""
    SC = _score()
    P, flen, n = 2, 8, 130 * 2048 + 77
    L = n + 1001
    rs = np.random.RandomState(9)
    s = rs.randn(P, L)
    s[:, 1:] += 0.6 * s[:, :-1]
    e = s[::-1] * 0.5 + 0.1 * rs.randn(P, L)
    R, D = SC.seg_corr(torch.from_numpy(s).to(dev), torch.from_numpy(e.copy()).to(dev), flen, [3, 1001], n)
    for i, a in enumerate((3, 1001)):
        Rn, Dn = SR.correlations(s[:, a:a + n], e[:, a:a + n], flen)
        assert_close(R[i], torch.from_numpy(Rn), 1e-11, "lagged correlations")
        assert_close(D[i], torch.from_numpy(Dn.transpose(1, 0, 2).copy()), 1e-11, "right-hand sides")


@pytest.mark.parametrize("S,L,flen", [(2, 6000, 512), (3, 3000, 64)])
def test_one_full_window_is_the_merged_mono_scorer(dev, S, L, flen):
    """C = 1, filters="window", one full-length window: SIR and SAR of bss_eval.bss_eval_sources, which runs the same
    kernels, so oracle/bss_eval.py on the CPU is the arbiter of both (1e-3 dB), and of bss_eval_sources' SDR; score_stems'
    SDR is the plain ratio (1e-9 dB against torch float64)."""
    from avsep_amd import bss_eval as PB
    from oracle import bss_eval as OB
    s, e = make_inputs(S, 1, L, 40 + S)
    st, et = torch.from_numpy(s).to(dev), torch.from_numpy(e).to(dev)
    got = _score().score_stems(st, et, L, L, "window", flen, permute=False)
    sdr, sir, sar = PB.bss_eval_sources(st[:, 0][None], et[:, 0][None], flen)
    osdr, osir, osar = (torch.from_numpy(np.asarray(x)).to(dev) for x in OB.bss_eval_sources(s[:, 0], e[:, 0], flen))
    assert got["frames"]["sir"].shape == (S, 1)
    for name, ours, ref in (("score_stems sir", got["sir"], osir), ("score_stems sar", got["sar"], osar),
                            ("bss_eval_sources sdr", sdr[0], osdr), ("bss_eval_sources sir", sir[0], osir),
                            ("bss_eval_sources sar", sar[0], osar)):
        assert torch.isfinite(ref).all() and (ref < 100).all(), (name, ref)
        print(f"{name}: max |d| = {(ours - ref).abs().max().item():.3e} dB")
        assert (ours - ref).abs().max().item() < DB_TOL, (name, ours, ref)
    plain = 10 * torch.log10((st ** 2).sum((1, 2)) / ((et - st) ** 2).sum((1, 2)))
    assert (got["sdr"] - plain).abs().max().item() < 1e-9


_batch = {}


def batch_inputs(dev):
    """B = 3, S = 2, L = 3000 (not a multiple of the correlation kernel's 2048-sample chunk: samples 1 and 2 start inside a
    chunk), flen = 64; make_inputs' recipe per sample."""
    if not _batch:
        pairs = [make_inputs(2, 1, 3000, 500 + b) for b in range(3)]
        _batch["s"], _batch["e"] = (np.stack([p[k][:, 0] for p in pairs]) for k in (0, 1))
    return torch.from_numpy(_batch["s"]).to(dev), torch.from_numpy(_batch["e"]).to(dev), 64


def _same_triple(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def test_bss_eval_sources_two_calls_give_identical_bits(dev):
    from avsep_amd import bss_eval as PB
    st, et, flen = batch_inputs(dev)
    a = PB.bss_eval_sources(st, et, flen)
    assert all(x.shape == (3, 2) and torch.isfinite(x).all() for x in a)
    assert _same_triple(a, PB.bss_eval_sources(st, et, flen))


def test_bss_eval_sources_a_sample_alone_is_the_sample_in_the_batch(dev):
    from avsep_amd import bss_eval as PB
    st, et, flen = batch_inputs(dev)
    a = PB.bss_eval_sources(st, et, flen)
    for b in range(3):
        one = PB.bss_eval_sources(st[b:b + 1], et[b:b + 1], flen)
        assert _same_triple([x[b:b + 1] for x in a], one), b


def test_bss_eval_sources_split_into_batches_is_the_unsplit_call(dev, monkeypatch):
    from avsep_amd import bss_eval as PB
    st, et, flen = batch_inputs(dev)
    a = PB.bss_eval_sources(st, et, flen)
    calls = []
    seg_corr = PB.seg_corr
    monkeypatch.setattr(PB, "seg_corr", lambda r, e, f, starts, n: calls.append(len(starts)) or seg_corr(r, e, f, starts, n))
    monkeypatch.setattr(PB, "_BATCH_BYTES", 1)                # below one segment's workspace: one sample per batch
    assert _same_triple(a, PB.bss_eval_sources(st, et, flen))
    assert calls == [1, 1, 1], calls


def _same_bits(a, b):
    return all(torch.equal(a[k], b[k]) and torch.equal(a["frames"][k], b["frames"][k]) for k in NAMES) and \
        all(torch.equal(a["track"][k], b["track"][k]) for k in NAMES if "track" in a)


def test_determinism_independence_and_permutation(dev):
    SC = _score()
    S, C, L, flen, win, hop = CASES[5]
    s, e, ref = case_data(CASES[5])
    st, et = torch.from_numpy(s).to(dev), torch.from_numpy(e).to(dev)
    for filters in ("track", "window"):
        a = SC.score_stems(st, et, win, hop, filters, flen, permute=False)
        b = SC.score_stems(st, et, win, hop, filters, flen, permute=False)
        assert not any(torch.isnan(a["frames"][k]).any() for k in NAMES)
        assert _same_bits(a, b), "two runs give identical bits"
        # the estimates handed over in another order come back matched, with the same bits
        c = SC.score_stems(st, et[[1, 0]].contiguous(), win, hop, filters, flen, permute=True)
        assert c["perm"] == [1, 0] and _same_bits(a, c)
        assert SC.score_stems(st, et, win, hop, filters, flen, permute=True)["perm"] == [0, 1]
    # a window scored alone is the window scored among all windows, bit for bit
    allw = SC.score_stems(st, et, win, hop, "window", flen, permute=False)
    for w, a0 in enumerate(allw["window_starts"]):
        one = SC.score_stems(st[:, :, a0:a0 + win].contiguous(), et[:, :, a0:a0 + win].contiguous(), win, hop, "window", flen,
                             permute=False)
        for k in NAMES:
            assert torch.equal(one["frames"][k][:, 0], allw["frames"][k][:, w]), (k, w)


def test_silent_window_is_nan_and_leaves_its_neighbours_alone(dev):
    SC = _score()
    S, C, L, flen, win, hop = CASES[1]
    s, e, _ = case_data(CASES[1])
    z = s.copy()
    z[1, :, 1000:2000] = 0.0                                  # reference 1 is silent in window 1
    st, et, zt = (torch.from_numpy(x).to(dev) for x in (s, e, z))
    for filters in ("track", "window"):
        got = SC.score_stems(zt, et, win, hop, filters, flen, permute=False)
        ref = SR.score_stems(z, e, win, hop, filters, flen, permute=False)
        for k in NAMES:
            f = got["frames"][k]
            assert torch.isnan(f[:, 1]).all() and torch.isfinite(f[:, [0, 2]]).all(), (filters, k, f)
            assert np.isnan(ref["frames"][k][:, 1]).all()
        assert_scores(got, ref, f"silent window, {filters}", need_all=False) >= 4 * (S + 2 * S)
    plain = SC.score_stems(st, et, win, hop, "window", flen, permute=False)
    for k in NAMES:                                           # own filters per window: the neighbours have not changed a bit
        assert torch.equal(got["frames"][k][:, [0, 2]], plain["frames"][k][:, [0, 2]])


def test_dual_mono_takes_the_least_squares_fallback(dev, monkeypatch):
    """A mono file saved as stereo: the Gram matrices are exactly singular (two identical block rows) and the host solves
    them by minimum-norm least squares, as the restatement does (np.linalg.lstsq)."""
    SC = _score()
    S, L, flen = 2, 3000, 16
    s1, e1 = make_inputs(S, 1, L, 77)
    s, e = np.repeat(s1, 2, 1), np.repeat(e1, 2, 1)
    st, et = torch.from_numpy(s).to(dev), torch.from_numpy(e).to(dev)
    R, D = SC.seg_corr(st.reshape(4, L), et.reshape(4, L), flen, [0], L)
    assert torch.equal(R[0, 0, 0], R[0, 0, 1]) and torch.equal(R[0, 1, 0], R[0, 0, 0]) and torch.equal(R[0, 2, 3], R[0, 3, 3])
    assert torch.equal(R[0, 0, 1], R[0, 0, 1].flip(0)), "the blocks of identical rows are the same bits, and symmetric"
    solved = []
    lstsq = torch.linalg.lstsq
    monkeypatch.setattr(torch.linalg, "lstsq", lambda A, b, **k: solved.append(A.shape[0]) or lstsq(A, b, **k))
    SC.solve_groups(R, D, 4, flen)
    SC.solve_groups(R, D, 2, flen)
    assert solved == [4 * flen, 2 * flen, 2 * flen], "every system goes to the host's minimum-norm least squares"
    for filters in ("track", "window"):
        got = SC.score_stems(st, et, 1000, 1000, filters, flen, permute=False)
        ref = SR.score_stems(s, e, 1000, 1000, filters, flen, permute=False)
        assert_scores(got, ref, f"dual-mono {filters}", need_all=False)
        for k in ("sdr", "sar"):
            r = ref["frames"][k]
            assert np.all(np.isfinite(r) & (r < 100)), (k, r)


def test_one_source_and_limits(dev, monkeypatch):
    SC = _score()
    s, e = make_inputs(1, 2, 2000, 3)
    got = SC.score_stems(torch.from_numpy(s).to(dev), torch.from_numpy(e).to(dev), 500, 500, "track", 8)
    ref = SR.score_stems(s, e, 500, 500, "track", 8)
    assert torch.isposinf(got["frames"]["sir"]).all() and torch.isposinf(got["sir"]).all() and torch.isposinf(got["track"]["sir"]).all()
    for k in ("sdr", "isr", "sar"):
        assert np.abs(got["frames"][k].cpu().numpy() - ref["frames"][k]).max() < DB_TOL
    # a 2-D input is C = 1
    s2, e2 = make_inputs(2, 1, 1500, 4)
    a = SC.score_stems(torch.from_numpy(s2[:, 0]).to(dev), torch.from_numpy(e2[:, 0]).to(dev), 500, 500, "window", 8)
    b = SC.score_stems(torch.from_numpy(s2).to(dev), torch.from_numpy(e2).to(dev), 500, 500, "window", 8)
    assert _same_bits(a, b)
    # over a limit: AvsepError that names it, before anything is launched

    def no_launch(*a, **k):
        raise AssertionError("a kernel was launched")
    from avsep_amd import bss_eval as PB
    assert not hasattr(SC, "call"), "score.py launches nothing itself: every launch goes through bss_eval.call"
    monkeypatch.setattr(PB, "call", no_launch)
    z = torch.zeros((3, 2, 1000), device=dev)
    with pytest.raises(SC.AvsepError, match="P \\* flen <= 2048"):
        SC.score_stems(z, z, 500, 500, "track", 342)
    with pytest.raises(SC.AvsepError, match="<= 8 rows"):
        SC.score_stems(torch.zeros((3, 3, 100), device=dev), torch.zeros((3, 3, 100), device=dev), 50, 50)
    with pytest.raises(SC.AvsepError):
        SC.score_stems(torch.zeros((2, 2, 100)), torch.zeros((2, 2, 100)), 50, 50)          # CPU tensors: no fallback
    with pytest.raises(SC.AvsepError, match="<= 8 rows"):
        PB.bss_eval_sources(torch.zeros((1, 9, 100), device=dev), torch.zeros((1, 9, 100), device=dev), 8)
    with pytest.raises(SC.AvsepError, match="P \\* flen <= 2048"):
        PB.bss_eval_sources(torch.zeros((2, 5, 1000), device=dev), torch.zeros((2, 5, 1000), device=dev))


def test_cli_round_trip(dev, tmp_path, capsys):
    """Two stereo references and two estimates as 16-bit WAVs: the JSON holds what score_stems gives on the same samples."""
    SC = _score()
    from avsep_amd import separate as SEP
    rate, L = 8000, 4000
    s, e = make_inputs(2, 2, L, 21)
    paths = []
    for name, x in (("ref", s), ("est", e[[1, 0]])):                          # the estimates are written in the other order
        for j in range(2):
            paths.append(str(tmp_path / f"{name}{j}.wav"))
            SEP.write_wav_pcm_channels(paths[-1], np.clip(np.round(x[j].T * 4000), -32768, 32767).astype(np.int16), rate)
    out = str(tmp_path / "scores.json")
    SC.cli(["--ref", paths[0], paths[1], "--est", paths[2], paths[3], "--win", "0.25", "--hop", "0.125", "--flen", "16", "--json", out])
    printed = capsys.readouterr().out.strip().splitlines()
    assert len(printed) == 2 and all(k in printed[0] for k in ("SDR", "ISR", "SIR", "SAR"))
    doc = json.load(open(out))
    refs, ests, r = SC.read_stems(paths[:2], paths[2:])
    want = SC.score_stems(torch.from_numpy(refs).to(dev), torch.from_numpy(ests).to(dev), 2000, 1000, "track", 16)
    assert r == rate and doc["rate"] == rate and (doc["win"], doc["hop"], doc["flen"], doc["filters"]) == (2000, 1000, 16, "track")
    assert doc["perm"] == want["perm"] == [1, 0] and doc["window_starts"] == [0, 1000, 2000]
    for k in NAMES:
        assert doc[k] == want[k].tolist() and doc["frames"][k] == want["frames"][k].tolist() and doc["track"][k] == want["track"][k].tolist()
