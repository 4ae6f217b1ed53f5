"""not-gpu: the float64 restatement tests/limiter_ref.py against the limiter's definition (include/avsep.h), and
the host half of the feature: limiter_plan, the entry point's refusals, the flags of separate and the report's block."""
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

import limiter_ref as REF
from recipes import no_gpu_call

U = 2.0 ** -53
HALF_WIDTHS = (1, 55, 240, 480, 1920)
RATE_OF = {1: 11025, 55: 11025, 240: 48000, 480: 96000, 1920: 192000}


def _lengths(A):
    return sorted({1, A, 2 * A + 1, 2047, 2049, 4096 + A + 3})


@pytest.mark.parametrize("A", HALF_WIDTHS)
def test_reference_gain_never_rises_above_the_required_gain(A):
    """g <= r up to the rounding of the (2A + 1)-term sum, at every sample, the first and last A included; and a hold that
    stops at the row's ends (what the definition's step 3 rules out) misses that by orders of magnitude."""
    worst = 0.0
    for L in _lengths(A):
        x = REF.recipe(RATE_OF[A], A, L, 3)
        ref = REF.limit(x, RATE_OF[A], -1.0, 1.0, A)
        assert ref["g"].shape == ref["r"].shape == (L,) and ref["h"].shape == (L + 2 * A,)
        over = float((ref["g"] - ref["r"]).max())
        worst = max(worst, over)
        assert over <= (2 * A + 8) * U, (A, L, over)
        assert (ref["g"] <= 1.0).all() and (ref["g"] > 0.0).all()
        assert (np.abs(ref["y"].astype(np.float64)) <= ref["c"] * (1.0 + 2.0 ** -23)).all(), "no sample passes the ceiling"
        assert np.abs(REF.smooth(ref["h"], ref["w"], reverse=True) - ref["g"]).max() <= REF.gain_bound(1.0, ref["s_max"], ref["c"], A)
    print(f"A={A}: worst g - r = {worst:.3e}")
    # the envelope cut off at the ends of the row: the spike at sample 0 is met by a gain far above what it needs
    x = REF.recipe(RATE_OF[A], A, 2049, 3)
    ref = REF.limit(x, RATE_OF[A], -1.0, 1.0, A)
    h_cut = ref["h"].copy()
    h_cut[:A], h_cut[-A:] = 1.0, 1.0
    assert (REF.smooth(h_cut, ref["w"]) - ref["r"]).max() > 0.1


def test_reference_leaves_a_quiet_programme_alone():
    g = np.random.default_rng(3)
    x = (0.2 * g.uniform(-1, 1, (2, 3000))).astype(np.float32)
    for rate, A in ((11025, 55), (48000, 240), (192000, 1920)):
        p, _ = REF.detector(x, rate)
        G = 0.999 * 10.0 ** (-1.0 / 20.0) / p.max()
        ref = REF.limit(x, rate, -1.0, G, A)
        assert G * p.max() <= ref["c"]
        assert (ref["g"] == 1.0).all(), "one minus a smoothed reduction of exactly zero"
        assert np.array_equal(ref["y"], (x.astype(np.float64) * G).astype(np.float32))


def test_reference_is_linked_and_programmes_are_independent():
    g = np.random.default_rng(4)
    x = (0.1 * g.uniform(-1, 1, (3, 1500))).astype(np.float32)
    quiet = REF.limit(x, 48000, -1.0, 1.0, 48)
    assert (quiet["g"] == 1.0).all()
    x[2, 700] = 1.5
    ref = REF.limit(x, 48000, -1.0, 1.0, 48)
    low = ref["g"] < 1.0
    assert low[700 - 48:700 + 49].all() and not low[:700 - 96 - 11].any() and not low[700 + 96 + 11:].any()
    for row in (0, 1):                                               # the rows without the spike are turned down as well
        assert np.array_equal(ref["y"][row], (x[row].astype(np.float64) * ref["g"]).astype(np.float32))
        assert (np.abs(ref["y"][row, low]) < np.abs(x[row, low])).sum() > 90
    alone = REF.limit(x[2:], 48000, -1.0, 1.0, 48)
    assert np.array_equal(alone["g"], ref["g"]), "rows 0 and 1 stay under the ceiling: the spike's row decides alone"
    other = REF.recipe(48000, 48, 1500, 3)
    assert not np.array_equal(REF.limit(other, 48000, -1.0, 1.0, 48)["g"], ref["g"]), "another programme, another curve"


def test_limiter_plan():
    for rate, ms, A in ((48000, 5.0, 240), (11025, 5.0, 55), (96000, 5.0, 480), (192000, 10.0, 1920), (8000, 0.01, 1),
                        (11025, 0.1, 1), (44100, 1.0, 44), (48000, 0.03125, 2), (192000, 2048 / 192.0, 2048)):
        got, w = LV.limiter_plan(rate, ms)
        assert got == A == REF.plan(rate, ms)[0] == max(1, round(rate * ms / 1000.0)), (rate, ms)
        assert w.dtype == np.float64 and w.shape == (2 * A + 1,) and np.array_equal(w, w[::-1]) and (w > 0).all()
        assert abs(w.sum() - 1.0) <= 4 * U and np.abs(w - REF.weights(A)).max() <= 4 * U and w.argmax() == A
    for rate, ms in ((192000, 10.7), (48000, 43.0), (8000, 257.0)):
        with pytest.raises(AvsepError, match="2048 samples"):
            LV.limiter_plan(rate, ms)
    for ms in (0.0, -1.0, math.nan, math.inf, "fast", None):
        with pytest.raises(AvsepError, match="look-ahead"):
            LV.limiter_plan(48000, ms)
    with pytest.raises(AvsepError):
        LV.limiter_plan(7999, 5.0)


def test_limit_refuses_before_any_launch(monkeypatch):
    no_gpu_call(monkeypatch)
    x = torch.zeros(2, 3, 500)
    for bad in (x.double(), x[0, 0], x[None], x.numpy(), torch.zeros(2, 3, 0), torch.zeros(1, 65, 10)):
        with pytest.raises(AvsepError, match="limit takes"):
            LV.limit(bad, 48000, -1.0)
    for kw in (dict(ceiling_db=0.5), dict(ceiling_db=math.nan), dict(ceiling_db=-math.inf), dict(gain=0.0), dict(gain=-1.0),
               dict(gain=math.inf), dict(gain=math.nan), dict(lookahead_ms=0.0), dict(lookahead_ms=50.0), dict(rate=48000.0)):
        args = dict(rate=48000, ceiling_db=-1.0)
        args.update(kw)
        with pytest.raises(AvsepError):
            LV.limit(x, **args)
    monkeypatch.undo()
    with pytest.raises(AvsepError, match="no CPU fallback"):
        LV.limit(x, 48000, -1.0)
    taps, w = torch.zeros(21, 4, dtype=torch.float64), torch.from_numpy(LV.limiter_plan(48000, 5.0)[1])
    with pytest.raises(AvsepError, match="no CPU fallback"):
        P.kernels.limiter(x, taps, w, 4, 1.0, 0.5)
    for kw in (dict(taps=taps[:, :2]), dict(w=w[:-1]), dict(w=w.float()), dict(w=torch.zeros(4099, dtype=torch.float64)), dict(os=3),
               dict(pre_gain=0.0), dict(ceiling=1.5), dict(ceiling=0.0), dict(out=torch.zeros(2, 3, 499))):
        args = dict(taps=taps, w=w, os=4, pre_gain=1.0, ceiling=0.5)
        args.update(kw)
        with pytest.raises(AvsepError, match="limiter"):
            P.kernels.limiter(x, **args)


def test_entry_point_refuses_before_any_launch():
    """Every refusal is AVSEP_ERR_ARG (-1) or AVSEP_ERR_WORKSPACE (-3): a launch on a machine without a GPU would be
    AVSEP_ERR_LAUNCH."""
    L = P.lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    big = 1 << 40

    def limiter(x=p, taps=p, w=p, P_=1, C=2, Ln=100, os=4, A=240, G=1.0, c=0.5, y=p, gain=p, stats=p, ws=p, nbytes=0):
        return L.avsep_limiter(x, taps, w, P_, C, Ln, os, A, G, c, y, gain, stats, ws, nbytes, None)
    for kw in (dict(x=None), dict(taps=None), dict(w=None), dict(y=None), dict(stats=None), dict(ws=None), dict(P_=0), dict(P_=65536),
               dict(C=0), dict(C=65), dict(Ln=0), dict(os=0), dict(os=3), dict(os=8), dict(os=4, Ln=1 << 29), dict(os=2, Ln=1 << 30),
               dict(A=0), dict(A=2049), dict(A=-1), dict(G=0.0), dict(G=-1.0), dict(G=math.inf), dict(G=math.nan), dict(c=0.0),
               dict(c=-0.5), dict(c=1.0000001), dict(c=math.nan)):
        assert limiter(nbytes=big, **kw) == -1, kw
    # well-formed arguments with a short workspace: past the argument checks, before any launch
    need = L.avsep_limiter_workspace_bytes(1, 2, 100)
    assert need == 8 * (100 + 3) and limiter(nbytes=need - 1) == -3
    assert limiter(nbytes=need - 1, gain=None) == -3, "gain may be NULL"
    assert limiter(nbytes=need - 1, c=1.0, A=2048, C=64, os=1, Ln=(1 << 31) - 1) == -3
    assert limiter(nbytes=need - 1, A=1, G=1e-300) == -3
    # r [P][L] and three partials per tile of 2048 samples; C does not count
    assert L.avsep_limiter_workspace_bytes(3, 64, 2049) == 3 * 8 * (2049 + 6) == L.avsep_limiter_workspace_bytes(3, 1, 2049)
    for bad in ((0, 1, 10), (65536, 1, 10), (1, 0, 10), (1, 65, 10), (1, 1, 0)):
        assert L.avsep_limiter_workspace_bytes(*bad) == 0, bad


def test_separate_limit_flags_are_checked_at_parse_time():
    base = ["--wav", "mix.wav", "--audio_only", "--id", "run"]
    a = S.parse_args(base)
    assert a.limit is None and a.limit_lookahead == 5.0
    a = S.parse_args(base + ["--limit", "-1", "--loudness", "-16", "--limit_lookahead", "1.5"])
    assert a.limit == -1.0 and a.loudness == -16.0 and a.limit_lookahead == 1.5 and a.peak is None
    assert S.parse_args(base + ["--limit", "0"]).limit == 0.0
    assert S.parse_args(base + ["--limit", "-1", "--limit_lookahead", "200"]).limit_lookahead == 200.0, "1600 samples at 8 kHz"
    for bad in (["--limit", "1"], ["--limit", "nan"], ["--limit=-inf"],["--limit", "-1", "--peak", "-1"],
                ["--limit", "-1", "--peak", "-3", "--loudness", "-16"], ["--limit", "-1", "--limit_lookahead", "257"],
                ["--limit", "-1", "--limit_lookahead", "0"], ["--limit", "-1", "--limit_lookahead", "nan"],
                ["--limit", "-1", "--limit_lookahead", "200", "--out_rate", "model"]):      # 2205 samples at the model's 11 025 Hz
        with pytest.raises(SystemExit):
            S.parse_args(base + bad)
    for bad in (["a.wav", "b.wav", "--limit", "-1", "--out", "o.wav"], ["a.wav", "--limit", "-1"], ["a.wav", "--limit", "0.5", "--out", "o.wav"],
                ["a.wav", "--out", "o.wav"]):
        with pytest.raises(SystemExit):
            LV.cli(bad)


def _stub(P_, C, integrated, peak):
    return {"integrated": torch.tensor(integrated, dtype=torch.float64), "momentary_max": torch.tensor(integrated, dtype=torch.float64) + 1.0,
            "short_term_max": torch.full((P_,), -math.inf, dtype=torch.float64),
            "true_peak": torch.full((P_, C), peak, dtype=torch.float64), "sample_peak": torch.zeros((P_, C), dtype=torch.float64)}


def test_the_limiter_block_of_the_report():
    info = {"peak_in": torch.tensor([2.0], dtype=torch.float64), "min_gain": torch.tensor([0.25], dtype=torch.float64),
            "limited_share": torch.tensor([0.125], dtype=torch.float64), "trim": torch.tensor([10.0 ** (-0.002 / 20.0)], dtype=torch.float64)}
    block = LV.limiter_figures(info, -1.0, 5.0)
    rep = LV.report(48000, 2.0, "limiter", _stub(1, 2, [-16.5], 0.89), _stub(2, 2, [-20.0, -math.inf], 0.8), block)
    rep = json.loads(json.dumps(rep, allow_nan=False))
    assert set(rep) == {"rate", "gain_db", "limited_by", "mixture", "sources", "limiter"}, "every key it had, and the block"
    assert rep["limited_by"] == "limiter" and abs(rep["gain_db"] - 20.0 * math.log10(2.0)) < 1e-12
    lim = rep["limiter"]
    assert set(lim) == {"ceiling_dbtp", "lookahead_ms", "max_reduction_db", "limited_share", "trim_db"}
    assert lim["ceiling_dbtp"] == -1.0 and lim["lookahead_ms"] == 5.0 and lim["limited_share"] == 0.125
    assert abs(lim["max_reduction_db"] - 20.0 * math.log10(4.0)) < 1e-12 and abs(lim["trim_db"] + 0.002) < 1e-12
    # nothing limited: no reduction, no trim; a curve that reaches 0 has no finite figure
    info = {"min_gain": torch.tensor([1.0, 0.0], dtype=torch.float64), "limited_share": torch.tensor([0.0, 1.0], dtype=torch.float64),
            "trim": torch.ones(2, dtype=torch.float64)}
    idle = LV.limiter_figures(info, -0.5, 1.0)
    assert idle["max_reduction_db"] == 0.0 and idle["trim_db"] == 0.0 and idle["limited_share"] == 0.0 and json.dumps(idle, allow_nan=False)
    assert LV.limiter_figures(info, -0.5, 1.0, 1)["max_reduction_db"] is None
    # without the block the report is what it was
    assert set(LV.report(48000, 1.0, None, _stub(1, 1, [-20.0], 0.1), _stub(1, 1, [-20.0], 0.1))) == {"rate", "gain_db", "limited_by", "mixture", "sources"}
