"""The recipes the pipeline tests share: the small net pairs, the tone mixtures, the CLI argument namespace, the PCM writer,
the "launches are unreachable" guard, buffers with guard elements around them and a few one-liners.  A plain helper module
like glue_cases.py: no fixtures, no tests, and the package is imported only inside the functions that need it.  A recipe that
only one test file uses, and every float64 reference (*ref.py), stays with that file."""
import argparse
import itertools

import numpy as np
import torch


# ---- the package -------------------------------------------------------------------------------------------------------
def pkg():
    import avsep_amd
    return avsep_amd


def lib():
    import avsep_amd
    return avsep_amd.lib.load()


def score():
    from avsep_amd import score
    return score


def no_gpu_call(monkeypatch):
    """Any kernel call from here on fails the test: the refusals below come from the argument checks."""
    import avsep_amd

    def boom(*a, **k):
        raise AssertionError("reached the GPU path")
    monkeypatch.setattr(avsep_amd.lib, "call", boom)
    monkeypatch.setattr(avsep_amd.kernels, "call", boom)
    monkeypatch.setattr(avsep_amd.lib, "require_gpu", boom)


# ---- arithmetic one-liners of the reference modules --------------------------------------------------------------------
def cdiv(a, b):
    return -(-a // b)


def f32(v):
    """The fp32 value of a constant of the kernels, as float."""
    return float(torch.tensor(v, dtype=torch.float32))


def out_hw(h):
    return (h + 2 - 3) // 2 + 1


# ---- arguments and nets ------------------------------------------------------------------------------------------------
def args(**kw):
    a = argparse.Namespace(num_mix=2, log_freq=1, binary_mask=1, mask_thres=0.5, output_activation="sigmoid",
                           img_activation="relu", not_pool_vis=False, fusion_type="hidsep", stft_frame=1022, stft_hop=256,
                           stft_pad_mode="reflect")
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def nets(args, dev):
    """The (sound, frame) pair the CLI builds from its arguments, eval mode."""
    mb = pkg().ModelBuilder()
    frm = mb.build_frame(arch=args.arch_frame, fc_dim=args.vis_channels, pool_type=args.img_pool, weights=args.weights_frame)
    snd = mb.build_sound(arch=args.arch_sound, fc_dim=args.num_channels, weights=args.weights_sound,
                         fusion_type=args.fusion_type, att_type=args.att_type)
    return snd.to(dev).eval(), frm.to(dev).eval()


def small_nets(dev, seed):
    """The unet5 / ngf 8 + ResnetDilated(fc_dim=32) pair, wide init, eval mode -> ((sound, frame), the generator)."""
    from oracle import nets as O
    P = pkg()
    torch.manual_seed(seed)
    gen = torch.Generator().manual_seed(seed)
    osnd = O.Unet(fc_dim=2, num_downs=5, ngf=8, fusion_type="hidsep", att_type="sig")
    O.wide_init(osnd, gen)
    ofrm = O.VisualNet(fc_dim=32, pool_type="maxpool", dilate_scale=16)
    snd = P.models.Unet(fc_dim=2, num_downs=5, ngf=8, fusion_type="hidsep", att_type="sig")
    frm = P.models.ResnetDilated(None, fc_dim=32, pool_type="maxpool")
    snd.load_state_dict(osnd.state_dict()); frm.load_state_dict(ofrm.state_dict())
    return (snd.to(dev).eval(), frm.to(dev).eval()), gen


# ---- windows -----------------------------------------------------------------------------------------------------------
def starts_t(starts, dev):
    return torch.tensor(starts, dtype=torch.int32, device=dev)


def random_perms(Kw, N, seed):
    cands = list(itertools.permutations(range(N)))
    g = torch.Generator().manual_seed(seed)
    return [list(cands[i]) for i in torch.randint(0, len(cands), (Kw,), generator=g).tolist()]


# ---- signals -----------------------------------------------------------------------------------------------------------
def tone_mix(L, seed, rate=11025):
    """A deterministic mixture with spectral structure: drifting partials plus a little noise, |x| < 1; float32 [L]."""
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(L, dtype=torch.float64) / rate
    x = torch.zeros(L, dtype=torch.float64)
    for f0, a, v in ((220.0, 0.25, 0.3), (523.25, 0.2, 0.11), (1318.5, 0.12, 0.05), (3200.0, 0.06, 0.7)):
        x += a * torch.sin(2 * np.pi * f0 * t * (1 + 0.01 * torch.sin(2 * np.pi * v * t)))
    x += 0.02 * torch.randn(L, generator=g, dtype=torch.float64)
    return x.float()


def tone_mix_panned(Ln, rate, seed, pans=(0.8, 0.3)):
    """The partials of tone_mix, one channel per pan, panned differently below and above 1 kHz so that the channels are
    not copies of each other; float64 [Ln, len(pans)]."""
    g = np.random.default_rng(seed)
    t = np.arange(Ln, dtype=np.float64) / rate
    ch = []
    for pan in pans:
        x = np.zeros(Ln)
        for f0, a, v in ((220.0, 0.25, 0.3), (523.25, 0.2, 0.11), (1318.5, 0.12, 0.05), (3200.0, 0.06, 0.7)):
            x += a * (pan if f0 < 1000 else 1 - pan) * np.sin(2 * np.pi * f0 * t * (1 + 0.01 * np.sin(2 * np.pi * v * t)))
        ch.append(x + 0.02 * g.standard_normal(Ln))
    return np.stack(ch, 1)


def tone_mix_stereo(Ln, rate, seed):
    """tone_mix_panned as a stereo recording with spectral structure below the model's Nyquist, int16 [Ln, 2]."""
    return np.clip(np.rint(tone_mix_panned(Ln, rate, seed) * 32768.0), -32768, 32767).astype(np.int16)


def tones(Ln, partials, seed, rate=11025):
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(Ln, dtype=torch.float64) / rate
    x = torch.zeros(Ln, dtype=torch.float64)
    for f0, a, v in partials:
        x += a * torch.sin(2 * np.pi * f0 * t * (1 + 0.01 * torch.sin(2 * np.pi * v * t)))
    return (x + 0.01 * torch.randn(Ln, generator=g, dtype=torch.float64)).float()


def istft_gain(n_fft, hop, frames):
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft) / n_fft)
    s1, s2 = np.zeros(n_fft + hop * (frames - 1)), np.zeros(n_fft + hop * (frames - 1))
    for m in range(frames):
        s1[m * hop:m * hop + n_fft] += w
        s2[m * hop:m * hop + n_fft] += w * w
    keep = slice(n_fft // 2, len(s1) - n_fft // 2)
    return float((s1[keep] / s2[keep]).max())


# ---- guarded buffers ---------------------------------------------------------------------------------------------------
GUARD = 256                                            # elements before and after every buffer


def _guarded(n, dtype, fill, dev):
    """A buffer of n elements inside a larger one filled with ``fill`` -> (the whole, the view)."""
    whole = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=dev)
    return whole, whole[GUARD:GUARD + n]


def _guards_intact(whole, fill):
    return bool((whole[:GUARD] == fill).all()) and bool((whole[-GUARD:] == fill).all())


# ---- files -------------------------------------------------------------------------------------------------------------
def write_pcm(path, pcm, rate):
    import wave
    with wave.open(path, "wb") as w:
        w.setnchannels(pcm.shape[1]); w.setsampwidth(2); w.setframerate(rate)
        w.writeframes(pcm.astype("<i2").tobytes())


def file_bytes(path):
    with open(str(path), "rb") as f:
        return f.read()
