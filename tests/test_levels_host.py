"""not-gpu: the host half of avsep_amd/levels.py (coefficients, weights, gating, the output gain, refusals, levels.json) and the
float64 reference tests/levels_ref.py against the anchors of ITU-R BS.1770-4 / EBU Tech 3341."""
import ctypes
import json
import math

import numpy as np
import pytest
import torch

import avsep_amd as P
from avsep_amd import levels as LV
from avsep_amd import separate as S
from avsep_amd.lib import AvsepError

import levels_ref as REF

INF = math.inf


def test_k_weighting_is_the_standards_table_at_48_khz():
    want = np.array([[1.53512485958697, -2.69169618940638, 1.19839281085285, 1.0, -1.69065929318241, 0.73248077421585],
                     [1.0, -2.0, 1.0, 1.0, -1.99004745483398, 0.99007225036621]])
    assert np.abs(LV.k_weighting(48000) - want).max() <= 1e-12
    assert np.abs(REF.k_weighting(48000) - want).max() <= 1e-12
    for rate in (8000, 11025, 44100, 96000, 192000):
        sos = LV.k_weighting(rate)
        assert sos.shape == (2, 6) and sos.dtype == np.float64 and np.abs(sos - REF.k_weighting(rate)).max() <= 1e-15
    for rate in (7999, 192001, 48000.0, "48000", True):
        with pytest.raises(AvsepError):
            LV.k_weighting(rate)


def test_peak_filter_and_channel_weights():
    for rate, os in ((8000, 4), (48000, 4), (95999, 4), (96000, 2), (191999, 2), (192000, 1)):
        got, g = LV.peak_filter(rate)
        assert got == os == REF.oversampling(rate) and g.shape == (20 * os + 1,) and g.dtype == np.float64
        assert np.abs(g - REF.interpolation_filter(os)).max() <= 1e-15
    assert np.array_equal(LV.peak_filter(192000)[1], (np.arange(21) == 10).astype(np.float64))
    for C in (1, 2, 3, 4, 5, 7):
        assert LV.channel_weights(C).tolist() == [1.0] * C
    assert LV.channel_weights(6).tolist() == [1, 1, 1, 0, 1.41, 1.41]
    assert LV.channel_weights(8).tolist() == [1, 1, 1, 0, 1.41, 1.41, 1.41, 1.41]


def _both(E, h, weights):
    got = LV.loudness_from_energies(np.asarray(E, dtype=np.float64), h, weights)
    got = (got["integrated"][0], got["momentary_max"][0], got["short_term_max"][0])
    want = REF.gating(np.asarray(E, dtype=np.float64), h, weights)
    for a, b in zip(got, want):
        assert a == b or abs(a - b) <= 1e-12, (got, want)
    return got


def test_gating_on_hand_made_energies():
    h = 100
    # silence: nothing passes the absolute gate
    assert _both(np.zeros((2, 40)), h, [1.0, 1.0]) == (-INF, -INF, -INF)
    # a level below -70 LUFS everywhere: a momentary value exists, an integrated one does not
    quiet = np.full((1, 40), h * 10.0 ** ((-80.0 + 0.691) / 10.0))
    i, m, s = _both(quiet, h, [1.0])
    assert i == -INF and abs(m + 80.0) < 1e-9 and abs(s + 80.0) < 1e-9
    # only the relative gate removes blocks: 20 sub-blocks at -20 LUFS, 20 at -45 (above -70, below -20 - 10 - ...)
    loud, soft = h * 10.0 ** ((-20.0 + 0.691) / 10.0), h * 10.0 ** ((-45.0 + 0.691) / 10.0)
    E = np.concatenate([np.full(20, loud), np.full(20, soft)])[None]
    i, m, s = _both(E, h, [1.0])
    p = [E[0, j:j + 4].sum() / (4 * h) for j in range(37)]
    l = [REF.lufs(v) for v in p]
    assert all(v > -70.0 for v in l), "the absolute gate removes nothing here"
    gamma = REF.lufs(np.mean(p)) - 10.0
    kept = [v for v, lv in zip(p, l) if lv > gamma]
    assert 0 < len(kept) < len(p), "the relative gate removes some blocks"
    assert abs(i - REF.lufs(np.mean(kept))) < 1e-12 and abs(m + 20.0) < 1e-9 and i > REF.lufs(np.mean(p)) + 1.0
    # S = 3: no block at all; S = 29: blocks, no short-term window; S = 30: one
    assert _both(np.full((1, 3), loud), h, [1.0]) == (-INF, -INF, -INF)
    i, m, s = _both(np.full((1, 29), loud), h, [1.0])
    assert abs(i + 20.0) < 1e-9 and abs(m + 20.0) < 1e-9 and s == -INF
    assert abs(_both(np.full((1, 30), loud), h, [1.0])[2] + 20.0) < 1e-9
    # weights: a channel of weight 0 does not count, 1.41 counts 1.41 times
    E6 = np.full((6, 8), loud)
    E6[3] *= 1e6
    assert abs(_both(E6, h, LV.channel_weights(6))[0] - (-20.0 + 10.0 * math.log10(3 + 2 * 1.41))) < 1e-9
    # several programmes in one call, each on its own
    out = LV.loudness_from_energies(np.stack([np.zeros((1, 40)), E]), h)
    assert out["integrated"][0] == -INF and out["momentary_max"][0] == -INF
    assert abs(out["integrated"][1] - _both(E, h, [1.0])[0]) < 1e-12


def test_output_gain():
    assert LV.output_gain(-30.0, [0.5, 0.9]) == (1.0, None)
    g, why = LV.output_gain(-30.0, [0.5, 0.9], loudness=-23.0)
    assert why == "loudness" and abs(g - 10.0 ** (7.0 / 20.0)) < 1e-15
    g, why = LV.output_gain(-30.0, [[0.5], [0.9]], loudness=-23.0, peak=-1.0)
    assert why == "peak" and abs(g - 10.0 ** (-1.0 / 20.0) / 0.9) < 1e-15
    g, why = LV.output_gain(-30.0, [0.05, 0.09], loudness=-23.0, peak=-1.0)
    assert why == "loudness" and abs(g - 10.0 ** (7.0 / 20.0)) < 1e-15
    g, why = LV.output_gain(-INF, torch.tensor([[1.5, 0.2]], dtype=torch.float64), peak=-1.0)
    assert why == "peak" and abs(g - 10.0 ** (-1.0 / 20.0) / 1.5) < 1e-15
    assert LV.output_gain(-INF, [0.5], peak=-1.0) == (1.0, None), "a stem under the ceiling is left alone"
    assert LV.output_gain(-30.0, [0.0], peak=-1.0) == (1.0, None)
    with pytest.raises(AvsepError, match="silent"):
        LV.output_gain(-INF, [0.5], loudness=-23.0)


def test_measure_refuses_before_any_launch(monkeypatch):
    def unreachable(*a, **k):
        raise AssertionError("a launch was reached")
    monkeypatch.setattr(P.kernels, "loudness_energies", unreachable)
    monkeypatch.setattr(P.kernels, "true_peak", unreachable)
    monkeypatch.setattr(P.kernels, "call", unreachable)
    monkeypatch.setattr(P.lib, "call", unreachable)
    x = torch.zeros(2, 4800)
    for bad, rate in ((x, 48000), (x.double(), 48000), (x[0], 48000), (x[None, None], 48000), (x.numpy(), 48000),
                      (x, 7999), (x, 192001), (x, 48000.5), (torch.zeros(2, 0), 48000)):
        with pytest.raises(AvsepError):
            LV.measure(bad, rate)
    # malformed arguments are refused before the device is looked at: these are CPU tensors, and the message names the argument
    for w in ([1.0], [1.0, -1.0], [1.0, math.nan], [[1.0, 1.0]]):
        with pytest.raises(AvsepError, match="weight"):
            LV.measure(x, 48000, weights=w)
    monkeypatch.undo()
    monkeypatch.setattr(P.kernels, "call", unreachable)              # the wrappers themselves, their launches still unreachable
    monkeypatch.setattr(P.lib, "call", unreachable)
    sos = LV.k_weighting(48000)
    for bad in (sos[:1], sos[:, :5], np.where(np.arange(12).reshape(2, 6) == 4, np.nan, sos), sos * 2.0):
        with pytest.raises(AvsepError, match="sos"):
            P.kernels.loudness_energies(x, bad, 4800)
    for h in (0, 4801, 2.5, True):
        with pytest.raises(AvsepError, match="h="):
            P.kernels.loudness_energies(x, sos, h)
    for taps, os in ((torch.zeros(21, 2, dtype=torch.float64), 4), (torch.zeros(21, 4), 4), (torch.zeros(20, 4, dtype=torch.float64), 4),
                     (np.zeros((21, 4)), 4)):
        with pytest.raises(AvsepError, match="table"):
            P.kernels.true_peak(x, taps, os)
    for os in (0, 3, 8):
        with pytest.raises(AvsepError, match="os="):
            P.kernels.true_peak(x, torch.zeros(21, 4, dtype=torch.float64), os)
    monkeypatch.undo()
    # well-formed arguments on a CPU tensor: the device is what is refused
    with pytest.raises(AvsepError, match="no CPU fallback"):
        P.kernels.loudness_energies(x, sos, 4800)
    with pytest.raises(AvsepError, match="no CPU fallback"):
        P.kernels.true_peak(x, torch.zeros(21, 4, dtype=torch.float64), 4)
    with pytest.raises(AvsepError, match="no CPU fallback"):
        LV.measure(x, 48000)


def test_entry_points_refuse_before_any_launch():
    """Every refusal is AVSEP_ERR_ARG (-1) or AVSEP_ERR_WORKSPACE (-3): a launch on this machine would be AVSEP_ERR_LAUNCH."""
    L = P.lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    sos = np.ascontiguousarray(LV.k_weighting(48000))
    big = 1 << 40

    def energies(x=p, s=None, R=1, Ln=9600, h=4800, E=p, ws=p, nbytes=big):
        s = None if s is False else np.ascontiguousarray(sos if s is None else s, dtype=np.float64)      # False: a null pointer
        return L.avsep_loudness_energies(x, None if s is None else s.ctypes.data, R, Ln, h, E, ws, nbytes, None)
    for kw in (dict(x=None), dict(s=False), dict(E=None), dict(ws=None), dict(R=0), dict(R=65536), dict(h=0), dict(h=9601),
               dict(Ln=0), dict(h=-1)):
        assert energies(**kw) == -1, kw
    assert energies(Ln=2 ** 31 - 1, h=2 ** 31 - 1, nbytes=0) == -3, "the largest h is planned in 64 bits: a defined answer"
    assert L.avsep_loudness_energies_workspace_bytes(1, 2 ** 31 - 1, 2 ** 31 - 1) == 8 * (5 * 2 ** 24 + 4)
    for i, v in ((0, np.nan), (4, np.inf), (11, -np.inf), (3, 2.0), (9, 0.5)):
        s = sos.copy()
        s.flat[i] = v
        assert energies(s=s) == -1, (i, v)
    need = L.avsep_loudness_energies_workspace_bytes(1, 9600, 4800)
    assert need > 0 and energies(nbytes=need - 1) == -3
    assert L.avsep_loudness_energies_workspace_bytes(0, 9600, 4800) == 0 and L.avsep_loudness_energies_workspace_bytes(1, 100, 101) == 0
    # the workspace follows the plan: a function of h, S and R only
    assert L.avsep_loudness_energies_workspace_bytes(3, 9600 + 4799, 4800) == 3 * need

    def peak(x=p, taps=p, R=1, Ln=100, os=4, peaks=p, ws=p, nbytes=big):
        return L.avsep_true_peak(x, taps, R, Ln, os, peaks, ws, nbytes, None)
    for kw in (dict(x=None), dict(taps=None), dict(peaks=None), dict(ws=None), dict(R=0), dict(R=65536), dict(Ln=0), dict(os=0),
               dict(os=3), dict(os=8), dict(os=4, Ln=1 << 29), dict(os=2, Ln=1 << 30)):
        assert peak(**kw) == -1, kw
    need = L.avsep_true_peak_workspace_bytes(2, 100)
    assert need > 0 and peak(R=2, nbytes=need - 1) == -3
    assert L.avsep_true_peak_workspace_bytes(0, 100) == 0 and L.avsep_true_peak_workspace_bytes(1, 0) == 0


def test_separate_flags_are_checked_at_parse_time():
    base = ["--wav", "mix.wav", "--audio_only", "--id", "run"]
    a = S.parse_args(base)
    assert a.levels is False and a.peak is None and a.loudness is None
    a = S.parse_args(base + ["--levels", "--peak", "-1", "--loudness", "-23"])
    assert a.levels is True and a.peak == -1.0 and a.loudness == -23.0
    assert S.parse_args(base + ["--peak", "0", "--loudness", "0"]).peak == 0.0
    assert S.parse_args(base + ["--loudness", "-70"]).loudness == -70.0
    for bad in (["--peak", "1"], ["--loudness", "3"], ["--loudness", "-80"], ["--peak", "nan"], ["--loudness", "nan"]):
        with pytest.raises(SystemExit):
            S.parse_args(base + bad)


def _stub(P_, C, integrated, peak):
    return {"integrated": torch.tensor(integrated, dtype=torch.float64), "momentary_max": torch.tensor(integrated, dtype=torch.float64) + 1.0,
            "short_term_max": torch.full((P_,), -INF, dtype=torch.float64),
            "true_peak": torch.full((P_, C), peak, dtype=torch.float64), "sample_peak": torch.zeros((P_, C), dtype=torch.float64)}


def test_levels_json_schema_from_a_stubbed_measurement():
    rep = LV.report(44100, 10.0 ** (-6.0 / 20.0), "peak", _stub(1, 2, [-23.0], 0.5), _stub(2, 2, [-26.0, -INF], 0.25))
    rep = json.loads(json.dumps(rep, allow_nan=False))              # strict JSON: -inf must have become null
    assert set(rep) == {"rate", "gain_db", "limited_by", "mixture", "sources"}
    assert rep["rate"] == 44100 and abs(rep["gain_db"] + 6.0) < 1e-12 and rep["limited_by"] == "peak"
    five = {"integrated_lufs", "momentary_max_lufs", "short_term_max_lufs", "true_peak_dbtp", "sample_peak_dbfs"}
    assert set(rep["mixture"]) == five and len(rep["sources"]) == 2 and all(set(s) == five for s in rep["sources"])
    assert rep["mixture"]["integrated_lufs"] == -23.0 and rep["mixture"]["momentary_max_lufs"] == -22.0
    assert rep["mixture"]["short_term_max_lufs"] is None and rep["sources"][1]["integrated_lufs"] is None
    assert len(rep["mixture"]["true_peak_dbtp"]) == 2 and abs(rep["mixture"]["true_peak_dbtp"][0] - 20.0 * math.log10(0.5)) < 1e-12
    assert rep["sources"][0]["sample_peak_dbfs"] == [None, None]
    rep = LV.report(48000, 1.0, None, _stub(1, 1, [-INF], 0.0), _stub(1, 1, [-INF], 0.0))
    assert rep["gain_db"] == 0.0 and rep["limited_by"] is None and json.dumps(rep, allow_nan=False)


def test_scaled_moves_every_figure_by_the_gain():
    m = dict(_stub(2, 2, [-23.0, -INF], 0.5), energies=torch.ones((2, 2, 3), dtype=torch.float64))
    s = LV.scaled(m, 0.5)
    db = 20.0 * math.log10(0.5)
    assert abs(s["integrated"][0].item() - (-23.0 + db)) < 1e-12 and s["integrated"][1].item() == -INF
    assert abs(s["momentary_max"][0].item() - (-22.0 + db)) < 1e-12 and (s["short_term_max"] == -INF).all()
    assert (s["true_peak"] == 0.25).all() and (s["sample_peak"] == 0.0).all() and (s["energies"] == 0.25).all()
    assert m["true_peak"][0, 0] == 0.5, "the measurement itself is left as it was"


# ---------------------------------------------------------------------------------------------------------------------
# the reference against the standard's anchors (and the package's host arithmetic on the reference's energies)
# ---------------------------------------------------------------------------------------------------------------------
def _sine(f, rate, seconds, dbfs=0.0, phase=0.0):
    return 10.0 ** (dbfs / 20.0) * np.sin(2.0 * np.pi * f * np.arange(int(seconds * rate)) / rate + phase)


def _host(x, rate, weights=None):
    """The package's gating over the reference's energies."""
    x = np.atleast_2d(x)
    out = LV.loudness_from_energies(REF.energies(x, rate)[0], REF.sub_block(rate), weights)
    return out["integrated"][0], out["momentary_max"][0], out["short_term_max"][0]


@pytest.mark.parametrize("rate,want", [(48000, -3.010), (44100, -3.008), (11025, -2.969), (8000, -2.996)])
def test_reference_full_scale_997_hz_sine(rate, want):
    x = _sine(997.0, rate, 5.0)
    got = REF.loudness(x, rate)
    assert abs(got[0] - want) < 1e-3 and abs(got[1] - want) < 5e-3 and abs(got[2] - want) < 1e-3
    for a, b in zip(_host(x, rate), got):
        assert abs(a - b) < 1e-12


def test_reference_stereo_and_gated_anchors():
    x = _sine(1000.0, 48000, 5.0, -23.0)
    assert abs(REF.loudness(np.stack([x, x]), 48000)[0] + 22.99) < 0.01
    two = np.concatenate([_sine(1000.0, 48000, 10.0, -36.0), _sine(1000.0, 48000, 10.0, -23.0)])
    got = REF.loudness(np.stack([two, two]), 48000)
    assert abs(got[0] + 23.06) < 0.01, "the relative gate drops the quiet half"
    for a, b in zip(_host(np.stack([two, two]), 48000), got):
        assert abs(a - b) < 1e-12


def test_reference_true_peak_anchors():
    for rate in (8000, 11025, 48000, 96000):
        n = np.arange(4096)
        x = np.sin(2.0 * np.pi * n / 4.0 + np.pi / 4.0)              # rate / 4 at 45 degrees: every sample is 0.7071
        sample, peak, bound = REF.true_peak(x, rate)
        assert abs(20.0 * math.log10(sample) + 3.0103) < 1e-3 and -0.4 <= 20.0 * math.log10(peak) <= 0.2 and bound < 1e-14
    fade = np.ones(8192)                                             # a sine cut off at full swing overshoots at the cut: fade it
    fade[:512] = 0.5 - 0.5 * np.cos(np.pi * np.arange(512) / 512.0)
    fade[-512:] = fade[:512][::-1]
    for frac in (0.1, 1.0 / 6.0, 0.45):
        x = fade * np.sin(2.0 * np.pi * frac * np.arange(8192) + 0.3)
        assert abs(20.0 * math.log10(REF.true_peak(x, 48000)[1])) < 0.04
    assert REF.true_peak(np.array([0.25, -0.5]), 192000)[:2] == (0.5, 0.5)


def test_reference_bound_is_the_documented_size():
    assert 2.0e-10 < REF.sample_bound(48000, 1.0) < 4.0e-10          # 2.9e-10 for |x| <= 1
    # a state dropped at a sub-block edge misses the bound by orders of magnitude (what the GPU test must catch)
    rate, h = 11025, 1103
    x = np.stack([np.ones(2 * h), np.random.default_rng(0).uniform(-1, 1, 2 * h)])
    E, A = REF.energies(x, rate)
    cut = REF.energies(x[:, h:], rate)[0]                            # the second sub-block, filtered from rest at the edge
    assert (np.abs(cut[:, 0] - E[:, 1]) > 1e3 * REF.energy_bound(rate, 1.0, A, h)[:, 1]).all()
