"""Host tests (no GPU) of tests/stftref.py, the float64 reference and the gates of tests/test_gpu_stft.py.

1. The reference is right: against torch.stft / torch.istft in float64 and against oracle.stft.
2. The gates are feasible: a float32 numpy evaluation of both operations (float32 basis, float32 matmul, float32 window-sum-
   square summed the plain way) passes every gate on every row of tests/stft_cases.py.  Its worst ratio per row is the "f32"
   figure beside the row there: 0.0161 of the bound at the most (2048/512 forward), 3.2e-7 of absref.
3. The gates see defects: nine float32 mutants, each aimed at a set of rows; a mutant fails every row it is aimed at.

Two of the mutants need a word.

* A dropped last basis tap (sample n_fft - 1) weighs win[n_fft - 1] ~ (pi / n_fft)^2 against tau * sum |win| ~ tau * n_fft / 4:
  no gate at tau = 2e-5 can see it beyond n_fft ~ 100, so it is aimed at 16/4 alone (the other rows are printed).
* The imaginary part of DC and Nyquist: in a DFT written as a matrix product its basis row is sin(0) or sin(pi n), zero by
  itself, so "not ignored" changes nothing there (the ck = 0 rule of stft_basis_kernel removes a residue of 1e-16).  It
  matters for an inverse real transform done as a half-length complex one: its first packed bin is
  (X_0 + conj X_h) + i (X_0 - conj X_h), h = n_fft / 2, and with Im X_0 = a_0, Im X_h = a_h not zeroed every frame gains
  -(a_h + (-1)^n a_0) / n_fft at sample n.  That is the mutant."""
import numpy as np
import pytest
import torch

import stft_cases as SC
import stftref as SR


# ---------------------------------------------------------------------------------------------------------------------
# 1. the reference
# ---------------------------------------------------------------------------------------------------------------------
GEOMETRIES = [(1022, 256, 3000), (1024, 256, 2048), (200, 64, 777), (16, 4, 50), (256, 192, 1000), (766, 254, 2540)]


def _wave(R, L, seed):
    return (torch.randn(R, L, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * 0.3).float().numpy()


@pytest.mark.parametrize("n_fft,hop,L", GEOMETRIES)
@pytest.mark.parametrize("mode", ["reflect", "constant"])
def test_stft_is_torch_stft_in_float64(n_fft, hop, L, mode):
    x = _wave(2, L, L)
    re, im, a_re, a_im = SR.stft(x, n_fft, hop, mode == "reflect")
    win = torch.from_numpy(SR.window(n_fft).copy())
    z = torch.stft(torch.from_numpy(x).double(), n_fft, hop_length=hop, window=win, center=True, pad_mode=mode,
                   return_complex=True).numpy()
    assert z.shape == re.shape == (2, n_fft // 2 + 1, 1 + L // hop)
    ratio, at = SR.worst(np.abs(z - (re + 1j * im)), 1e-12 * np.hypot(a_re, a_im))
    assert ratio <= 1.0, (ratio, at)
    assert (a_re >= np.abs(re)).all() and (a_im >= np.abs(im)).all()


@pytest.mark.parametrize("name,mode", SC.FORWARD_ROWS)
def test_stft_is_the_oracle_to_float32_rounding(name, mode):
    """oracle.stft.stft multiplies by a float32 window in float32 (2^-23 per term) and casts to complex64 (2^-24)."""
    from oracle import stft as OS
    n_fft, hop = SC.FORWARD[name][:2]
    x = SC.forward_input(name)
    re, im, a_re, a_im = SC.forward_ref(name, mode)
    for r in range(x.shape[0]):
        z = OS.stft(x[r], n_fft, hop, mode).astype(np.complex128)
        ratio, at = SR.worst(np.abs(z - (re[r] + 1j * im[r])), 2.0 ** -22 * np.hypot(a_re[r], a_im[r]))
        assert ratio <= 1.0, (name, r, ratio, at)


def _real_edges(phase, n_fft):
    phase = phase.copy()
    phase[:, (0, n_fft // 2), :] = 0.0
    return phase


@pytest.mark.parametrize("name", ["I2", "I3", "I5", "I6", "I7", "I9", "I11", "I12"])
def test_istft_is_torch_istft_in_float64(name):
    n_fft, hop, R, frames = SC.INVERSE[name][:4]
    mag, phase = SC.inverse_input(name, "b")
    phase = _real_edges(phase, n_fft)
    out_len = hop * (frames - 1)
    y, ya = SR.istft(mag, phase, n_fft, hop, out_len)
    m, p = torch.from_numpy(mag).double(), torch.from_numpy(phase).double()
    z = torch.complex(m * torch.cos(p), m * torch.sin(p))
    t = torch.istft(z, n_fft, hop_length=hop, window=torch.from_numpy(SR.window(n_fft).copy()), center=True, length=out_len).numpy()
    ratio, at = SR.worst(np.abs(t - y), 1e-12 * ya)
    assert ratio <= 1.0, (ratio, at)
    assert (ya >= np.abs(y)).all()


@pytest.mark.parametrize("name", ["I2", "I6", "I12"])
def test_istft_is_the_oracle(name):
    from oracle import stft as OS
    n_fft, hop, R, frames = SC.INVERSE[name][:4]
    mag, phase = SC.inverse_input(name, "a")
    y, ya = SC.inverse_ref(name, "a")
    z = mag.astype(np.float64) * np.exp(1j * phase.astype(np.float64))
    for r in range(R):
        o = OS.istft(z[r], hop).astype(np.float64)
        ratio, at = SR.worst(np.abs(o - y[r]), 2.0 ** -23 * ya[r])          # the oracle returns float32
        assert o.shape == y[r].shape and ratio <= 1.0, (r, ratio, at)


@pytest.mark.parametrize("name", ["I1", "I6", "I9"])
def test_istft_ignores_the_imaginary_part_of_dc_and_nyquist(name):
    """cos(-p) is cos(p) bit for bit and sin(-p) is -sin(p): the negated phase at the two bins changes their imaginary
    part by twice its value and nothing else."""
    n_fft, hop, R, frames = SC.INVERSE[name][:4]
    mag, phase = SC.inverse_input(name, "b")
    assert (np.abs(mag[::2, (0, n_fft // 2), 0] * np.sin(phase[::2, (0, n_fft // 2), 0])) > 1e-3).any()
    flipped = phase.copy()
    flipped[:, (0, n_fft // 2), :] *= -1.0
    y, ya = SC.inverse_ref(name, "b")
    y2, ya2 = SR.istft(mag, flipped, n_fft, hop, hop * (frames - 1))
    assert np.array_equal(y, y2) and np.array_equal(ya, ya2)


def test_the_inputs_are_what_the_table_says():
    for name, (n_fft, hop, R, L, modes, path, fam) in SC.FORWARD.items():
        x = SC.forward_input(name)
        assert x.shape == (R, L) and x.dtype == np.float32 and (x[:, L // 3:L // 3 + 3 * hop] == 0).all()
        assert np.abs(x[0, :hop]).max() > 1e3 * np.abs(x[0, -hop:]).max() or L < 6 * hop
        if R > 1:
            assert (x[1] == 0).all()
        if R > 2:
            assert 0 < np.abs(x[2]).max() < 2e-3
        fast = 3 * hop < n_fft <= 4 * hop and hop % 4 == 0 and hop <= 1024 and 1 + L // hop >= 32
        assert path == ("fast" if fast else "fallback") and L > n_fft // 2
    assert 1 + SC.FORWARD["F1"][3] // 256 == 32 and 1 + SC.FORWARD["B1"][3] // 256 == 31
    assert 32 * (512 + 1) * 4 == 65664 and 32 * (1024 + 1) * 4 == 131200 and 32 * (256 + 1) * 4 == 32896
    for name, kind in SC.INVERSE_ROWS:
        mag, phase = SC.inverse_input(name, kind)
        n_fft, hop, R, frames = SC.INVERSE[name][:4]
        assert mag.shape == phase.shape == (R, n_fft // 2 + 1, frames) and (mag[1] == 0).all() and (mag >= 0).all()
        if kind == "b":
            assert (mag[:, :, 1:min(3, frames)] == 0).all() and np.abs(phase).max() > 2.9 * np.pi
            assert (np.abs(np.sin(phase[:, (0, n_fft // 2)])) > 0.05).all()


# ---------------------------------------------------------------------------------------------------------------------
# 2. / 3. the float32 evaluation and its mutants
# ---------------------------------------------------------------------------------------------------------------------
F32 = np.float32


def _bf16(x):
    return (np.ascontiguousarray(x, dtype=F32).view(np.uint32) & np.uint32(0xFFFF0000)).view(F32)


def _leak(x):
    return (x + F32(1e-4) * np.roll(x, -1, axis=0)).astype(F32)


def f32_stft(x, n_fft, hop, reflect, mutant=None):
    R, L = x.shape
    pad, frames = n_fft // 2, 1 + L // hop
    mode = "reflect" if reflect else "constant"
    if reflect and mutant == "symmetric":
        mode = "symmetric"
    xp = np.pad(x, ((0, 0), (pad, pad)), mode=mode)
    if reflect and mutant == "reflect_off_by_one":
        ids = np.pad(np.arange(L), (pad + 1, pad + 1), mode="reflect")
        xp = np.concatenate([x[:, ids[:pad]], x, x[:, ids[L + pad + 2:]]], axis=1)
    step = hop + 1 if mutant == "hop_plus_1" else hop
    xp = np.pad(xp, ((0, 0), (0, frames)))
    fr = xp[:, np.arange(n_fft)[:, None] + step * np.arange(frames)[None, :]]
    ang, win = SR.dft_angles(n_fft), SR.window(n_fft)
    c, s = (win * np.cos(ang)).astype(F32), (-win * np.sin(ang)).astype(F32)
    if mutant == "tap_dropped":
        c[:, n_fft - 1] = 0
        s[:, n_fft - 1] = 0
    re, im = c @ fr, s @ fr
    assert re.dtype == F32
    if mutant == "leak":
        re, im = _leak(re), _leak(im)
    mag, phase = np.sqrt(re * re + im * im), np.arctan2(im, re)
    if mutant == "bf16":
        mag, phase = _bf16(mag), _bf16(phase)
    return mag, phase


def f32_istft(mag, phase, n_fft, hop, out_len, mutant=None):
    R, bins, frames = mag.shape
    re, im = mag * np.cos(phase), mag * np.sin(phase)
    assert re.dtype == F32
    ang, win = SR.dft_angles(n_fft), SR.window(n_fft)
    ck = np.full(bins, 2.0)
    ck[0] = ck[n_fft // 2] = 1.0
    cki = ck.copy()
    cki[0] = cki[n_fft // 2] = 0.0
    bc = (win[None, :] * ck[:, None] * np.cos(ang) / n_fft).T.astype(F32)
    bs = (-win[None, :] * cki[:, None] * np.sin(ang) / n_fft).T.astype(F32)
    td = bc @ re + bs @ im
    if mutant == "dc_nyquist_imag":          # what a packed half-length transform adds when the two are not zeroed
        sign = np.where(np.arange(n_fft) % 2 == 0, 1.0, -1.0).astype(F32)
        extra = -(im[:, n_fft // 2, None, :] + sign[None, :, None] * im[:, 0, None, :]) / F32(n_fft)
        td = td + win.astype(F32)[None, :, None] * extra
    w = (F32(0.5) - F32(0.5) * np.cos(F32(2.0 * np.pi) * np.arange(n_fft, dtype=F32) / F32(n_fft))).astype(F32)
    total = n_fft + hop * (frames - 1)
    y, wss = np.zeros((R, total), F32), np.zeros(total, F32)
    g = np.arange(n_fft)
    for f in range(frames):
        pos = f * hop + g
        keep = np.ones(n_fft, bool)
        if mutant == "f_lo_plus_1":
            f_lo = np.maximum(0, np.trunc((pos - n_fft + hop) / hop).astype(np.int64))
            keep = f >= f_lo + 1
        y[:, pos[keep]] += td[:, keep, f]
        wss[pos[keep]] += w[keep] * w[keep]
    if mutant != "no_wss_division":
        ok = wss > SR.TINY
        y[:, ok] /= wss[ok]
    out = y[:, n_fft // 2:n_fft // 2 + out_len]
    if mutant == "leak":
        out = _leak(out)
    if mutant == "bf16":
        out = _bf16(out)
    return out


def _forward_ratios(name, mode, mutant=None):
    n_fft, hop = SC.FORWARD[name][:2]
    mag, phase = f32_stft(SC.forward_input(name), n_fft, hop, mode == "reflect", mutant)
    ref = SC.forward_ref(name, mode)
    return SR.gate_mag(mag, ref)[0], SR.gate_phase(mag, phase, ref)[0]


def _inverse_ratio(name, kind, mutant=None):
    n_fft, hop, R, frames = SC.INVERSE[name][:4]
    mag, phase = SC.inverse_input(name, kind)
    return SR.gate_inverse(f32_istft(mag, phase, n_fft, hop, hop * (frames - 1), mutant), SC.inverse_ref(name, kind))[0]


@pytest.mark.parametrize("name,mode", SC.FORWARD_ROWS)
def test_float32_control_passes_the_forward_gates(name, mode):
    m, p = _forward_ratios(name, mode)
    print(f"{name} {mode}: magnitude {m:.4f}, phase {p:.4f}")
    assert m <= 1.0 and p <= 1.0


@pytest.mark.parametrize("name,kind", SC.INVERSE_ROWS)
def test_float32_control_passes_the_inverse_gate(name, kind):
    e = _inverse_ratio(name, kind)
    print(f"{name} {kind}: {e:.4f}")
    assert e <= 1.0


@pytest.mark.parametrize("name,cut", SC.SHORT_ROWS)
def test_float32_control_passes_the_short_outputs(name, cut):
    n_fft, hop, R, frames = SC.INVERSE[name][:4]
    out_len = SC.short_len(name, cut)
    for kind in "ab":
        mag, phase = SC.inverse_input(name, kind)
        ref = SC.inverse_ref(name, kind, out_len)
        assert ref[0].shape == (R, out_len) and np.array_equal(ref[0], SC.inverse_ref(name, kind)[0][:, :out_len])
        assert SR.gate_inverse(f32_istft(mag, phase, n_fft, hop, out_len), ref)[0] <= 1.0


_REFLECT = [r for r in SC.FORWARD_ROWS if r[1] == "reflect"]
_MANY_ROWS = [r for r in SC.FORWARD_ROWS if SC.FORWARD[r[0]][2] > 1]
_B_ROWS = [r for r in SC.INVERSE_ROWS if r[1] == "b"]
# mutant: (forward rows it is aimed at, inverse rows it is aimed at)
MUTANTS = {
    "symmetric": (_REFLECT, []),
    "reflect_off_by_one": (_REFLECT, []),
    "hop_plus_1": (SC.FORWARD_ROWS, []),
    "tap_dropped": ([("F7", "reflect")], []),
    "dc_nyquist_imag": ([], _B_ROWS),
    "no_wss_division": ([], SC.INVERSE_ROWS),
    "f_lo_plus_1": ([], _B_ROWS),              # on a consistent spectrum (a) every frame holds the same signal: dropping one is exact
    "leak": (_MANY_ROWS, SC.INVERSE_ROWS),
    "bf16": (SC.FORWARD_ROWS, SC.INVERSE_ROWS),
}
_FORWARD_ONLY = ("symmetric", "reflect_off_by_one", "hop_plus_1", "tap_dropped")
_INVERSE_ONLY = ("dc_nyquist_imag", "no_wss_division", "f_lo_plus_1")


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_the_gates_see_the_mutant(mutant):
    fwd, inv = MUTANTS[mutant]
    assert fwd or inv
    passed = []
    for name, mode in (SC.FORWARD_ROWS if mutant not in _INVERSE_ONLY else []):
        m, p = _forward_ratios(name, mode, mutant)
        print(f"{mutant} {name} {mode}: magnitude {m:.3g}, phase {p:.3g}{'' if (name, mode) in fwd else '  (not aimed)'}")
        if (name, mode) in fwd and not (m > 1.0 or p > 1.0):
            passed.append((name, mode))
    for name, kind in (SC.INVERSE_ROWS if mutant not in _FORWARD_ONLY else []):
        e = _inverse_ratio(name, kind, mutant)
        print(f"{mutant} {name} {kind}: {e:.3g}{'' if (name, kind) in inv else '  (not aimed)'}")
        if (name, kind) in inv and not e > 1.0:
            passed.append((name, kind))
    assert not passed, f"{mutant} passes {passed}"
