"""not-gpu: the numpy restatement of the windowed image-form BSS-eval (tests/score_ref.py) pinned on known answers, on the
merged oracle (oracle/bss_eval.py) and on the plain SDR formula; the host side of avsep_amd/score.py (window planning, the
permutation rule, the command line's checks)."""
import numpy as np
import pytest

import score_ref as SR
from recipes import score as _score


# ---- window planning and the permutation rule (restatement and package agree) ------------------------------------------------------
@pytest.mark.parametrize("L,win,hop,starts,wlen", [
    (3001, 1000, 1000, [0, 1000, 2000], 1000),              # a remainder of 1 is dropped
    (3999, 1000, 1000, [0, 1000, 2000], 1000),              # and one of win - 1
    (700, 1000, 500, [0], 700),                             # L < win: one window, the whole signal
    (3000, 1000, 500, [0, 500, 1000, 1500, 2000], 1000),    # hop < win: overlapping, the last one ends at L
    (1000, 1000, 1, [0], 1000),
    (2500, 800, 1200, [0, 1200], 800),                      # hop > win: gaps
])
def test_window_planning(L, win, hop, starts, wlen):
    assert SR.plan_windows(L, win, hop) == (starts, wlen)
    assert _score().plan_windows(L, win, hop) == (starts, wlen)


def test_window_planning_rejects_nonpositive_sizes():
    S = _score()
    for win, hop in ((0, 10), (10, 0), (-1, 5)):
        with pytest.raises(S.AvsepError):
            S.plan_windows(100, win, hop)


def test_permutation_tie_rule_and_swapped_estimates():
    S = _score()
    assert S.best_permutation([[3.0, 3.0], [3.0, 3.0]]) == [0, 1]                      # a tie: the first in lexicographic order
    assert S.best_permutation([[1.0, 9.0], [9.0, 1.0]]) == [1, 0]
    m = [[0.0, 0.0, 5.0], [5.0, 0.0, 0.0], [0.0, 5.0, 0.0]]                           # estimate 1 is reference 0, 2 is 1, 0 is 2
    assert S.best_permutation(m) == [1, 2, 0]
    assert S.best_permutation([[2.0]]) == [0]
    rs = np.random.RandomState(3)
    refs = rs.randn(3, 2, 500)
    ests = refs + 0.1 * rs.randn(3, 2, 500)
    order = [2, 0, 1]                                                                  # file i holds the estimate of reference order[i]
    shuffled = ests[np.argsort(order)]
    assert SR.best_permutation(refs, ests) == [0, 1, 2]
    perm = SR.best_permutation(refs, shuffled)
    assert np.array_equal(shuffled[perm], ests)
    assert SR.best_permutation(refs, np.stack([refs[0]] * 3) * 0 + 1.0) == [0, 1, 2]   # identical estimates: a tie
    a = SR.score_stems(refs[:2], ests[:2], 250, 250, "track", 4)
    b = SR.score_stems(refs[:2], ests[:2][::-1], 250, 250, "track", 4)
    assert a["perm"] == [0, 1] and b["perm"] == [1, 0]
    for k in ("sdr", "isr", "sir", "sar"):
        assert np.array_equal(a["frames"][k], b["frames"][k])


# ---- known answers through the restatement ---------------------------------------------------------------------------------------
def test_known_answer_leak_of_the_other_source():
    """e_j = s_j + 0.1 s_k on independent white sources: SIR = 20 dB; the own-source projection picks up only the chance
    correlation of s_k with the flen delays of s_j, 0.01 * flen / L of the source's energy: ISR about 67 dB here."""
    rs = np.random.RandomState(0)
    L, flen = 200000, 4
    s = rs.randn(2, L)
    e = np.stack([s[0] + 0.1 * s[1], s[1] + 0.1 * s[0]])
    r = SR.score_stems(s, e, L, L, "track", flen, permute=False)
    assert np.all(np.abs(r["sir"] - 20.0) < 1.0), r["sir"]
    assert np.all(r["isr"] > 60.0), r["isr"]
    assert np.all(np.abs(r["track"]["sir"] - 20.0) < 1.0)


def test_known_answer_filtered_reference_is_spatial_distortion_only():
    """Every channel of every reference through its own 12-tap FIR (the references end in 16 zeros, so the filtered signal ends
    inside the recording): the own-source projection reproduces the estimate, ISR is the plain ratio sum s^2 / sum (h*s - s)^2
    and nothing is left for SIR and SAR."""
    rs = np.random.RandomState(1)
    S, C, L, flen = 2, 2, 6000, 16
    s = rs.randn(S, C, L)
    s[:, :, -16:] = 0.0
    h = 0.4 * rs.randn(S, C, 12)
    h[:, :, 0] += 1.0
    e = np.stack([np.stack([np.convolve(s[j, c], h[j, c])[:L] for c in range(C)]) for j in range(S)])
    r = SR.score_stems(s, e, L, L, "track", flen, permute=False)
    plain = 10 * np.log10((s ** 2).sum((1, 2)) / ((e - s) ** 2).sum((1, 2)))
    assert np.all(np.abs(r["isr"] - plain) < 0.1), (r["isr"], plain)
    assert np.all(r["sir"] > 60.0) and np.all(r["sar"] > 60.0), (r["sir"], r["sar"])
    assert np.all(plain < 15.0)                                               # (the filters are far from the identity)


def test_known_answer_one_percent_noise():
    """+1 % white noise: SAR = 40 dB, less the P * flen / L = 0.3 % of the noise that the projection absorbs (as
    test_bss_eval_vs_oracle notes for the mono scorer)."""
    rs = np.random.RandomState(2)
    S, C, L, flen = 2, 1, 20000, 16
    s = rs.randn(S, C, L)
    e = s + 0.01 * rs.randn(S, C, L)
    r = SR.score_stems(s, e, L, L, "window", flen, permute=False)
    assert np.all(np.abs(r["sar"] - 40.0) < 1.0), r["sar"]
    assert np.all(np.abs(r["sdr"] - 40.0) < 1.0), r["sdr"]


def test_known_answer_cross_channel_leak_is_isr_not_sir():
    """e[j,0] = s[j,0] + 0.3 s[j,1]: the estimate still lies in the span of its own source's channels, so the leak is spatial
    distortion (ISR = 10 log10(2 / 0.09) = 13.5 dB on white channels) and no interference."""
    rs = np.random.RandomState(4)
    S, C, L, flen = 2, 2, 8000, 8
    s = rs.randn(S, C, L)
    e = s.copy()
    e[:, 0] += 0.3 * s[:, 1]
    r = SR.score_stems(s, e, L, L, "track", flen, permute=False)
    assert np.all(np.abs(r["isr"] - 10 * np.log10(2 / 0.09)) < 0.5), r["isr"]
    assert np.all(r["sir"] > 60.0), r["sir"]


# ---- cross-checks ---------------------------------------------------------------------------------------------------------------
def _coloured_mix(S, C, L, seed):
    rs = np.random.RandomState(seed)
    s = rs.randn(S * C, L)
    s[:, 1:] += 0.6 * s[:, :-1]
    mix = np.eye(S * C) + 0.2 * rs.randn(S * C, S * C)
    e = mix @ s + 0.03 * rs.randn(S * C, L)
    return s.reshape(S, C, L), e.reshape(S, C, L)


@pytest.mark.parametrize("S,L,flen", [(2, 3000, 32), (3, 2000, 16)])
def test_restatement_equals_the_merged_oracle_at_one_channel(S, L, flen):
    """C = 1, one full-length window with its own filters, is mir_eval's bss_eval_sources: SIR and SAR of the restatement
    against oracle/bss_eval.py (FFT correlations, the same normal equations) within 1e-6 dB."""
    from oracle import bss_eval as OB
    s, e = _coloured_mix(S, 1, L, 10 + S)
    r = SR.score_stems(s, e, L, L, "window", flen, permute=False)
    _, sir, sar = OB.bss_eval_sources(s[:, 0], e[:, 0], flen)
    assert np.max(np.abs(r["sir"] - sir)) < 1e-6 and np.max(np.abs(r["sar"] - sar)) < 1e-6, (r["sir"], sir, r["sar"], sar)
    assert r["frames"]["sir"].shape == (S, 1)


def test_restatement_sdr_is_the_plain_formula():
    s, e = _coloured_mix(2, 2, 2400, 7)
    for filters in ("track", "window"):
        r = SR.score_stems(s, e, 800, 400, filters, 8, permute=False)
        assert r["window_starts"] == [0, 400, 800, 1200, 1600]
        for w, a in enumerate(r["window_starts"]):
            plain = 10 * np.log10((s[:, :, a:a + 800] ** 2).sum((1, 2)) / ((e - s)[:, :, a:a + 800] ** 2).sum((1, 2)))
            assert np.max(np.abs(r["frames"]["sdr"][:, w] - plain)) < 1e-9
    t = SR.score_stems(s, e, 800, 400, "track", 8, permute=False)["track"]["sdr"]
    assert np.max(np.abs(t - 10 * np.log10((s ** 2).sum((1, 2)) / ((e - s) ** 2).sum((1, 2))))) < 1e-9


# ---- silence --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filters", ["track", "window"])
def test_silent_window_is_nan_and_the_median_ignores_it(filters):
    s, e = _coloured_mix(2, 1, 4000, 5)
    s[0, :, 1000:2000] = 0.0                                  # reference 0 is silent in window 1
    r = SR.score_stems(s, e, 1000, 1000, filters, 8, permute=False)
    for k in ("sdr", "isr", "sir", "sar"):
        f = r["frames"][k]
        assert np.all(np.isnan(f[:, 1])) and np.all(np.isfinite(f[:, [0, 2, 3]])), (k, f)
        assert np.allclose(r[k], np.median(f[:, [0, 2, 3]], axis=1), rtol=0, atol=0)
    e2 = e.copy()
    e2[1, :, 3000:] = 0.0                                     # and a silent estimate counts as well
    r2 = SR.score_stems(s, e2, 1000, 1000, filters, 8, permute=False)
    assert np.all(np.isnan(r2["frames"]["sar"][:, [1, 3]])) and np.all(np.isfinite(r2["frames"]["sar"][:, [0, 2]]))


def test_one_source_has_infinite_sir():
    s, e = _coloured_mix(1, 2, 1500, 6)
    r = SR.score_stems(s, e, 500, 500, "track", 8)
    assert np.all(np.isposinf(r["frames"]["sir"])) and np.isposinf(r["sir"][0]) and np.isfinite(r["isr"][0])


# ---- the command line's host side ------------------------------------------------------------------------------------------------
def _write(path, rate, ch, n, seed):
    from avsep_amd import separate as SEP
    pcm = (np.random.RandomState(seed).randn(n, ch) * 3000).astype(np.int16)
    SEP.write_wav_pcm_channels(str(path), pcm, rate)
    return pcm


def test_cli_arguments():
    S = _score()
    a = S.parse_args(["--ref", "a.wav", "b.wav", "--est", "x.wav", "y.wav"])
    assert (a.win, a.hop, a.filters, a.flen, a.json) == (1.0, 1.0, "track", 512, None) and a.ref == ["a.wav", "b.wav"]
    a = S.parse_args(["--ref", "a.wav", "--est", "x.wav", "--win", "0.5", "--hop", "0.25", "--filters", "window", "--flen", "64",
                      "--json", "o.json"])
    assert (a.win, a.hop, a.filters, a.flen, a.json) == (0.5, 0.25, "window", 64, "o.json")
    with pytest.raises(SystemExit, match="one estimate per reference"):
        S.parse_args(["--ref", "a.wav", "b.wav", "--est", "x.wav"])
    with pytest.raises(SystemExit):
        S.parse_args(["--ref", "a.wav", "--est", "x.wav", "--filters", "clip"])
    with pytest.raises(SystemExit, match="positive"):
        S.parse_args(["--ref", "a.wav", "--est", "x.wav", "--hop", "0"])


def test_cli_reads_stems_and_refuses_mixed_rates_and_channel_counts(tmp_path):
    S = _score()
    a = _write(tmp_path / "a.wav", 16000, 2, 900, 0)
    b = _write(tmp_path / "b.wav", 16000, 2, 800, 1)
    _write(tmp_path / "r.wav", 22050, 2, 800, 2)
    _write(tmp_path / "m.wav", 16000, 1, 800, 3)
    p = lambda n: str(tmp_path / n)                                           # noqa: E731
    refs, ests, rate = S.read_stems([p("a.wav"), p("b.wav")], [p("b.wav"), p("a.wav")])
    assert rate == 16000 and refs.shape == ests.shape == (2, 2, 800) and refs.dtype == np.float64     # trimmed to the shortest
    assert np.array_equal(refs[0], a[:800].T / 32768.0) and np.array_equal(ests[0], b.T / 32768.0)
    with pytest.raises(SystemExit, match="22050 Hz.*does not resample"):
        S.read_stems([p("a.wav"), p("b.wav")], [p("a.wav"), p("r.wav")])
    with pytest.raises(SystemExit, match="1 channel.*one channel count"):
        S.read_stems([p("a.wav"), p("m.wav")], [p("a.wav"), p("b.wav")])
    # the limits are checked before a GPU is asked for: five stereo sources are ten rows
    with pytest.raises(SystemExit, match="P = S \\* C <= 8"):
        S.cli(["--ref"] + [p("a.wav")] * 5 + ["--est"] + [p("b.wav")] * 5)
    with pytest.raises(SystemExit, match="P \\* flen <= 2048"):
        S.cli(["--ref", p("a.wav"), p("b.wav"), p("a.wav"), "--est", p("b.wav"), p("a.wav"), p("b.wav"), "--flen", "512"])


def test_limits_name_themselves():
    S = _score()
    S.check_limits(2, 2, 512)
    S.check_limits(4, 1, 512)
    S.check_limits(3, 2, 341)
    for args, what in (((3, 2, 342), "P \\* flen <= 2048"), ((3, 3, 8), "<= 8 rows"), ((0, 1, 8), "1 <= S"), ((2, 2, 0), "flen")):
        with pytest.raises(S.AvsepError, match=what):
            S.check_limits(*args)
