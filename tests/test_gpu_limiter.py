"""gpu: avsep_limiter (csrc/levels.hip) and avsep_amd.levels.limit against the float64 restatement tests/limiter_ref.py, and the
--limit flags of avsep_amd.separate and avsep_amd.levels.  The bounds are the reference's derived ones (limiter_ref.gain_bound,
output_bound; levels_ref.true_peak); the worst ratios are printed (pytest -s) before they are asserted."""
import json
import math
import wave

import numpy as np
import pytest
import torch

import avsep_amd as P
from avsep_amd import levels as LV
from avsep_amd import resample as RS
from avsep_amd import separate as S
from avsep_amd import wavio as W
from avsep_amd.lib import AvsepError

import levels_ref as LREF
import limiter_ref as REF
from recipes import file_bytes as _bytes, nets as _nets, tone_mix_panned as _tone_mix

pytestmark = pytest.mark.gpu

CEILING_DB = -1.0
C_LIN = 10.0 ** (CEILING_DB / 20.0)
# (rate, A): os of 4, 4, 4, 2 and 1; the last is the largest LDS plan the tests reach.  The look-ahead that gives A at the rate.
PLANS = ((11025, 1), (11025, 55), (48000, 240), (96000, 480), (192000, 1920))
MS = {(11025, 1): 0.1, (11025, 55): 5.0, (48000, 240): 5.0, (96000, 480): 5.0, (192000, 1920): 10.0}


def _lengths(A):
    return sorted({1, A, 2 * A + 1, 2047, 2049, 4096 + A + 3})


def _hot_noise(C, L, seed):
    """Uniform noise 10 dB over full scale, float32 [C, L]."""
    return (10.0 ** 0.5 * np.random.default_rng(seed).uniform(-1.0, 1.0, (C, L))).astype(np.float32)


def _quarter_sine(L):
    """rate / 4 at 45 degrees: every sample is 0.7071, the true peak 1; float32 [1, L]."""
    return np.sin(2.0 * np.pi * np.arange(L) / 4.0 + np.pi / 4.0).astype(np.float32)[None]


_refs = {}


def _ref(key, x, rate, A, G=1.0):
    """The reference of one programme, computed once per key and shared by the tests that need it (read-only)."""
    if key not in _refs:
        ref = REF.limit(x, rate, CEILING_DB, G, A)
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _refs[key] = ref
    return _refs[key]


def _recipe_case(rate, A, L, C):
    x = REF.recipe(rate, A, L, C)
    return x, _ref(("recipe", rate, A, L, C), x, rate, A)


def _run(x, rate, A, dev, G=1.0, trim=False):
    """x float32 [P, C, L] (numpy) through LV.limit -> (y, gain as numpy; info)."""
    assert LV.limiter_plan(rate, MS[(rate, A)])[0] == A
    y, info = LV.limit(torch.from_numpy(np.ascontiguousarray(x)).to(dev), rate, CEILING_DB, gain=G, lookahead_ms=MS[(rate, A)], trim=trim,
                       return_gain=True)
    assert y.dtype == torch.float32 and tuple(y.shape) == x.shape and info["gain"].dtype == torch.float64
    assert tuple(info["gain"].shape) == (x.shape[0], x.shape[2]) and info["gain"].is_cuda
    return y.cpu().numpy(), info["gain"].cpu().numpy(), info


def _check_programme(x, ref, y, g, info, p, G, what, dev, rate):
    """Programme p of a call against its reference: the gain and the output inside their bounds, the three statistics exact."""
    Bg = REF.gain_bound(G, ref["s_max"], ref["c"], ref["A"])
    eg = np.abs(g - ref["g"])
    By = REF.output_bound(ref["y"], x, G, Bg)
    ey = np.abs(y.astype(np.float64) - ref["y"].astype(np.float64))
    fy = float(np.max(ey / np.where(By > 0, By, 1.0)))
    print(f"{what}: worst |g - g_ref| / Bg = {eg.max() / Bg:.3e}, worst |y - y_ref| / bound = {fy:.3e}, reference share "
          f"{(ref['g'] < 1.0).mean():.4f}, min g {ref['g'].min():.4f}")
    assert np.isfinite(g).all() and (eg <= Bg).all(), f"gain: worst ratio to the bound {eg.max() / Bg:.3e}"
    assert (ey <= By).all(), f"output: worst ratio to the bound {fy:.3e}"
    m = LV.measure(torch.from_numpy(np.ascontiguousarray(x)).to(dev), rate)
    assert info["peak_in"][p].item() == m["true_peak"].max().item() * G, "the detector's maximum is the meter's largest true peak, bit for bit"
    assert info["min_gain"][p].item() == g.min() and info["limited_share"][p].item() == (g < 1.0).sum() / g.size
    assert info["trim"][p].item() == 1.0


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("rate,A,L", [(r, A, L) for r, A in PLANS for L in _lengths(A)])
def test_gain_and_output_are_inside_the_bounds(dev, rate, A, L, C):
    x, ref = _recipe_case(rate, A, L, C)
    share = float((ref["g"] < 1.0).mean())
    # a condition on the REFERENCE, checked before the GPU is looked at: the cases meant to be limited in part are
    if A <= 240 and L >= 2047:
        assert 0.0 < share < 1.0, share
    else:
        assert share > 0.0
    y, g, info = _run(x[None], rate, A, dev)
    _check_programme(x, ref, y[0], g[0], info, 0, 1.0, f"recipe rate={rate} A={A} L={L} C={C}", dev, rate)


def test_two_programmes_that_differ(dev):
    rate, A, L = 48000, 240, 4096 + 240 + 3
    a, ref_a = _recipe_case(rate, A, L, 3)
    b = a[::-1].copy()
    b[:, 2047:2049] = 0.0                                            # two of its spikes are gone, the others sit in other rows
    ref_b = _ref(("recipe-b", rate, A, L), b, rate, A)
    assert not np.array_equal(ref_a["g"], ref_b["g"]) and 0.0 < (ref_b["g"] < 1.0).mean() < 1.0
    y, g, info = _run(np.stack([a, b]), rate, A, dev)
    _check_programme(a, ref_a, y[0], g[0], info, 0, 1.0, "programme 0 of 2", dev, rate)
    _check_programme(b, ref_b, y[1], g[1], info, 1, 1.0, "programme 1 of 2", dev, rate)


@pytest.mark.parametrize("G", [0.5, 2.0])
def test_pre_gain_with_everything_limited(dev, G):
    """Noise 10 dB over full scale: at either pre-gain a sample over the ceiling lies inside every window, so every gain is
    below 1 (asserted on the reference)."""
    rate, A, L = 48000, 240, 4096 + 240 + 3
    x = _hot_noise(2, L, 21)
    ref = _ref(("hot", G), x, rate, A, G)
    assert (ref["g"] < 1.0).all()
    y, g, info = _run(x[None], rate, A, dev, G=G)
    _check_programme(x, ref, y[0], g[0], info, 0, G, f"hot noise G={G}", dev, rate)


def test_an_untouched_programme_comes_back_exactly(dev):
    rate, A, L = 48000, 240, 4096 + 240 + 3
    x = (0.2 * np.random.default_rng(8).uniform(-1, 1, (3, L))).astype(np.float32)
    xd = torch.from_numpy(x).to(dev)
    G = 0.999 * C_LIN / LV.measure(xd, rate)["true_peak"].max().item()
    assert G > 1.0
    y, info = LV.limit(xd, rate, CEILING_DB, gain=G, return_gain=True)
    assert torch.equal(info["gain"], torch.ones_like(info["gain"])), "one minus a reduction of exactly zero"
    assert torch.equal(y, (xd.double() * G).float())
    assert info["min_gain"][0].item() == 1.0 and info["limited_share"][0].item() == 0.0 and info["trim"][0].item() == 1.0
    assert tuple(y.shape) == (3, L), "[C, L] in, [C, L] out"


def test_same_bits_alone_in_a_batch_again_and_in_place(dev):
    rate, A, L = 48000, 240, 4096 + 240 + 3
    x, _ = _recipe_case(rate, A, L, 3)
    other = _hot_noise(3, L, 5)
    xd = torch.from_numpy(x).to(dev)
    y, info = LV.limit(xd[None], rate, CEILING_DB, trim=False, return_gain=True)
    y2, info2 = LV.limit(torch.from_numpy(np.stack([other, x])).to(dev), rate, CEILING_DB, trim=False, return_gain=True)
    assert torch.equal(y2[1], y[0]) and torch.equal(info2["gain"][1], info["gain"][0]), "as programme 1 of 2"
    assert info2["min_gain"][1] == info["min_gain"][0] and info2["limited_share"][1] == info["limited_share"][0]
    y3, info3 = LV.limit(xd[None], rate, CEILING_DB, trim=False, return_gain=True)
    assert torch.equal(y3, y) and torch.equal(info3["gain"], info["gain"]), "a second call"
    os, taps = LV.peak_table(rate, dev)
    w = torch.from_numpy(LV.limiter_plan(rate, 5.0)[1]).to(dev)
    buf = xd[None].clone()
    out, gain, stats = P.kernels.limiter(buf, taps, w, os, 1.0, C_LIN, return_gain=True, out=buf)
    assert out.data_ptr() == buf.data_ptr() and torch.equal(buf, y) and torch.equal(gain, info["gain"]), "y aliasing x"
    _, none, stats2 = P.kernels.limiter(xd[None], taps, w, os, 1.0, C_LIN)
    assert none is None and torch.equal(stats2, stats), "without the gain store"


def _ceiling_inputs():
    rate, A, L = 48000, 240, 4096 + 240 + 3
    return {"recipe": (_recipe_case(rate, A, L, 3)[0], 1.0), "hot noise": (_hot_noise(2, L, 21), 2.0), "quarter sine": (_quarter_sine(L), 2.0)}


@pytest.mark.parametrize("name", ["recipe", "hot noise", "quarter sine"])
def test_the_ceiling_holds_after_the_trim(dev, name):
    """With the trim the true peak of y is at most c, up to the f32 rounding of the trimmed samples (2^-24 s_max(y)) and the
    meter's own bound; without it the overshoot is the reference's own."""
    rate, A = 48000, 240
    x, G = _ceiling_inputs()[name]
    ref = _ref(("ceiling", name), x, rate, A, G)
    want = REF.overshoot_db(ref["y"], rate, ref["c"])
    y, _, _ = _run(x[None], rate, A, dev, G=G)
    got = REF.overshoot_db(y[0], rate, ref["c"])
    print(f"{name}: overshoot without the trim {got:+.6f} dB, the reference's {want:+.6f} dB")
    assert abs(got - want) <= 1e-3
    yt, _, info = _run(x[None], rate, A, dev, G=G, trim=True)
    _, bound, s_max = REF.true_peak(yt[0], rate)
    top = LV.measure(torch.from_numpy(yt).to(dev), rate)["true_peak"].max().item()
    print(f"{name}: trim {20.0 * math.log10(info['trim'][0].item()):+.6f} dB, true peak after it {20.0 * math.log10(top):+.6f} dBTP")
    assert top <= ref["c"] + 2.0 ** -24 * s_max + bound
    assert (info["trim"][0].item() < 1.0) == (got > 0.0) or abs(got) < 1e-6, "trimmed exactly when the curve alone overshoots"
    assert top >= ref["c"] * (1.0 - 1e-3), "the programme sits at the ceiling, not under it"


@pytest.mark.parametrize("bad", [math.nan, math.inf, -math.inf])
def test_a_non_finite_sample(dev, bad):
    rate, A, L = 48000, 240, 5000
    x = np.stack([REF.recipe(rate, A, L, 2), REF.recipe(rate, A, L, 2, seed=1)])
    x[1, 0, 4097] = bad
    os, taps = LV.peak_table(rate, dev)
    w = torch.from_numpy(LV.limiter_plan(rate, 5.0)[1]).to(dev)
    _, _, stats = P.kernels.limiter(torch.from_numpy(x).to(dev), taps, w, os, 1.0, C_LIN)
    stats = stats.cpu().numpy()
    assert stats[1, 0] == math.inf and np.isfinite(stats[0]).all()
    with pytest.raises(AvsepError, match="programme 1"):
        LV.limit(torch.from_numpy(x).to(dev), rate, CEILING_DB)


# ---------------------------------------------------------------------------------------------------------------------
# the command lines
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """The "hot" fixture of test_gpu_levels.py: a tiny random-weight model saved as a checkpoint; a 2 s 48 kHz stereo mixture as
    a 16-bit file and, eight times as hot (so that its stems overshoot full scale), as a float file."""
    d = tmp_path_factory.mktemp("limiter_cli")
    mb = P.ModelBuilder()
    torch.manual_seed(11)
    snd = mb.build_sound(arch="unet5", fc_dim=2, fusion_type="hidsep", att_type="sig")
    frm = mb.build_frame(arch="resnet18dilated", fc_dim=256, pool_type="maxpool")
    torch.save(snd.state_dict(), str(d / "sound.pth"))
    torch.save(frm.state_dict(), str(d / "frame.pth"))
    mix = _tone_mix(2 * 48000, 48000, 8)
    pcm = np.clip(np.rint(mix * 32768.0), -32768, 32767).astype(np.int16)
    with wave.open(str(d / "mix16.wav"), "wb") as w:
        w.setnchannels(2); w.setsampwidth(2); w.setframerate(48000)
        w.writeframes(pcm.astype("<i2").tobytes())
    W.write_frames(str(d / "hot.wav"), np.frombuffer((8.0 * mix).astype("<f4").tobytes(), dtype=np.uint8), 48000, 2, "f32")
    rng = np.random.default_rng(3)
    ones = []
    for n in range(2):
        np.save(str(d / f"one{n}.npy"), rng.standard_normal((3, 64, 64)).astype(np.float32))
        ones.append(str(d / f"one{n}.npy"))
    flags = ["--arch_sound", "unet5", "--num_channels", "2", "--vis_channels", "256", "--img_pool", "maxpool", "--not_pool_vis",
             "--fusion_type", "hidsep", "--att_type", "sig", "--weights_sound", str(d / "sound.pth"),
             "--weights_frame", str(d / "frame.pth"), "--frames", *ones, "--binary_mask", "0"]
    return d, flags


def _read_rows(path, dev):
    raw, info = W.read_frames(str(path))
    return RS.split_frames(torch.from_numpy(raw).to(dev), info.fmt, info.channels, info.rate, info.rate)[1:], info


def _under_the_ceiling(rows, rate, extra=0.0):
    """rows f32 [C, L] on the GPU: their largest true peak against c + 2^-24 s_max + the meter's bound (+ extra)."""
    top = LV.measure(rows, rate)["true_peak"].max().item()
    _, bound, s_max = REF.true_peak(rows.cpu().numpy(), rate)
    return top, C_LIN + 2.0 ** -24 * s_max + bound + extra


def test_cli_limit_reaches_the_loudness_the_scalar_ceiling_cannot(dev, case, tmp_path, capsys):
    d, flags = case
    target = 0.0                                                     # the hot mixture measures +0.06 LUFS and its stems pass full scale
    common = ["--wav", str(d / "hot.wav"), "--loudness", str(target), "--out_format", "f32", *flags]
    out = S.cli(common + ["--out", str(tmp_path / "lim"), "--limit", "-1"])
    said = capsys.readouterr().out
    S.cli(common + ["--out", str(tmp_path / "peak"), "--peak", "-1"])
    lim, peak = (json.loads(_bytes(tmp_path / k / "levels.json")) for k in ("lim", "peak"))
    assert peak["limited_by"] == "peak", "the target is one the scalar ceiling cannot reach"
    assert lim["limited_by"] == "limiter" and "limited by limiter" in said and "limiter" not in peak
    assert set(lim) == set(peak) | {"limiter"} and set(lim["limiter"]) == {"ceiling_dbtp", "lookahead_ms", "max_reduction_db", "limited_share", "trim_db"}
    assert lim["limiter"]["ceiling_dbtp"] == -1.0 and lim["limiter"]["lookahead_ms"] == 5.0 and 0.0 < lim["limiter"]["limited_share"] <= 1.0
    assert lim["limiter"]["max_reduction_db"] > 0.0 and lim["limiter"]["trim_db"] <= 0.0 and lim["gain_db"] > peak["gain_db"]
    miss_lim, miss_peak = (abs(r["mixture"]["integrated_lufs"] - target) for r in (lim, peak))
    print(f"mixture against {target} LUFS: {miss_lim:.3f} LU with --limit, {miss_peak:.3f} LU with --peak; limiter {lim['limiter']}")
    assert miss_lim < miss_peak
    # the written stems: under the ceiling, and what the report says of them
    stems, stems_peak = [], []
    for n in range(2):
        got, info = _read_rows(tmp_path / "lim" / f"source{n}.wav", dev)
        assert info.fmt == "f32" and info.rate == 48000 and info.channels == 1
        top, bound = _under_the_ceiling(got, 48000)
        assert top <= bound, (n, top, bound)
        assert abs(lim["sources"][n]["true_peak_dbtp"][0] - 20.0 * math.log10(top)) < 1e-9, "measured again after the limiter"
        stems.append(got[0].double())
        stems_peak.append(_read_rows(tmp_path / "peak" / f"source{n}.wav", dev)[0][0].double())
    # the stems sum to the limited mixture as well as the --peak run's sum to theirs: the limiter's residual is that run's
    # under the curve, sample by sample, up to one f32 rounding per term of either sum and rounding step (a trimmed stem has
    # been rounded twice; the --peak run's stems are f32 products with the f32 value of its gain, which is then that run's gain)
    rows = RS.resample(out["wavs"], 11025, 48000)
    assert out["wavs"].abs().max().item() > 1.0, "the stems come back unclamped"
    G, Gp = 10.0 ** (lim["gain_db"] / 20.0), float(np.float32(10.0 ** (peak["gain_db"] / 20.0)))
    y, info = LV.limit(rows[None], 48000, -1.0, gain=G, return_gain=True)
    for n in range(2):
        assert torch.allclose(y[0, n].double(), stems[n], rtol=1e-6, atol=0.0), "ONE programme of all the rows"
    mono = S.load_mixture(str(d / "hot.wav"), W.probe(str(d / "hot.wav")), 48000, dev)[0].double()
    n = min(mono.shape[0], rows.shape[1])
    curve = info["gain"][0, :n] * (G * info["trim"][0].item())
    res_lim = stems[0][:n] + stems[1][:n] - mono[:n] * curve
    res_peak = stems_peak[0][:n] + stems_peak[1][:n] - mono[:n] * Gp
    scale = curve / Gp
    steps = 2.0 if info["trim"][0].item() < 1.0 else 1.0
    margin = 2.0 ** -24 * (steps * (stems[0][:n].abs() + stems[1][:n].abs()) + (mono[:n] * curve).abs()
                           + scale * (stems_peak[0][:n].abs() + stems_peak[1][:n].abs() + (mono[:n] * Gp).abs()))
    print(f"residuals: limiter {res_lim.abs().max().item():.3e}, peak {res_peak.abs().max().item():.3e}, worst difference / margin "
          f"{((res_lim - scale * res_peak).abs() / margin.clamp_min(1e-300)).max().item():.3e}")
    assert ((res_lim - scale * res_peak).abs() <= margin).all()
    assert res_peak.abs().max().item() > 1e-3, "the separation loses something: the two residuals are not both nothing"


def test_cli_without_the_new_flags_writes_the_bytes_it_wrote_before(dev, case, tmp_path):
    d, flags = case
    argv = ["--wav", str(d / "mix16.wav"), *flags]
    S.cli(argv + ["--out", str(tmp_path / "plain")])
    args = S.parse_args(argv + ["--out", str(tmp_path / "old")])
    wav, _ = S.load_mixture(args.wav, W.probe(args.wav), args.audRate, dev)
    frames = [torch.from_numpy(np.load(p)).float()[None].to(dev) for p in args.frames]
    out = S.separate_long(_nets(args, dev), wav, frames, args)
    (tmp_path / "old").mkdir()
    for n, w in enumerate(RS.resample(out["wavs"], args.audRate, 48000, out_s16=True).cpu().numpy()):
        S.write_wav_pcm(str(tmp_path / "old" / f"source{n}.wav"), w, 48000)
    for n in range(2):
        assert _bytes(tmp_path / "plain" / f"source{n}.wav") == _bytes(tmp_path / "old" / f"source{n}.wav")
    assert not (tmp_path / "plain" / "levels.json").exists()
    # --peak without --limit reports what it reported: no limiter block
    S.cli(["--wav", str(d / "hot.wav"), *flags, "--out", str(tmp_path / "peak"), "--peak", "-1", "--out_format", "f32"])
    rep = json.loads(_bytes(tmp_path / "peak" / "levels.json"))
    assert set(rep) == {"rate", "gain_db", "limited_by", "mixture", "sources"} and rep["limited_by"] == "peak"


def test_levels_limit_command_on_a_24_bit_stereo_file(dev, tmp_path, capsys):
    rate, L = 48000, 48000
    x = 3.0 * _tone_mix(L, rate, 5).T                                # its second half is clipped by the 24-bit writer,
    x[:, :L // 2] /= 3.0                                             # its first half stays under the ceiling
    x = torch.from_numpy(x.astype(np.float32).copy()).to(dev)
    W.write_frames(str(tmp_path / "in.wav"), RS.join_frames(x, rate, rate, "s24").cpu().numpy(), rate, 2, "s24")
    res = LV.cli([str(tmp_path / "in.wav"), "--limit", "-1", "--out", str(tmp_path / "out.wav"), "--json", str(tmp_path / "l.json")])
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 3 and "dBTP" in lines[0] and "dBTP" in lines[1] and lines[2].startswith("limiter at -1.00 dBTP")
    assert json.loads(_bytes(tmp_path / "l.json")) == json.loads(json.dumps(res)) and set(res) == {"input", "output", "limiter"}
    a, ia = _read_rows(tmp_path / "in.wav", dev)
    b, ib = _read_rows(tmp_path / "out.wav", dev)
    assert (ib.fmt, ib.rate, ib.channels) == (ia.fmt, ia.rate, ia.channels) == ("s24", rate, 2) and b.shape == a.shape
    assert max(res["input"]["true_peak_dbtp"]) > 0.0 and 0.0 < res["limiter"]["limited_share"] < 1.0
    # every written sample is within 2^-24 of the limited one: the oversampled row moves by at most that times sum |taps|
    g = LREF.interpolation_filter(4)
    top, bound = _under_the_ceiling(b, rate, extra=2.0 ** -24 * max(np.abs(g[p::4]).sum() for p in range(4)))
    print(f"24-bit file: true peak {20.0 * math.log10(top):+.6f} dBTP after the limiter, {res['limiter']}")
    assert top <= bound and top >= C_LIN * (1.0 - 1e-3)
    assert abs(max(res["output"]["true_peak_dbtp"]) - 20.0 * math.log10(top)) < 1e-3
    # the channels share one curve: where both are well away from zero, their ratios out / in agree to the 24-bit rounding
    a, b = a.double(), b.double()
    both = (a.abs() > 0.1).all(0)
    ratio = b[:, both] / a[:, both]
    assert both.sum().item() > 1000 and ((ratio[0] - ratio[1]).abs() <= 2.0 * 2.0 ** -24 / 0.1).all()
    assert ratio.min().item() < 0.95 and ratio.max().item() > 0.999, "a curve, not one gain"
