"""Long-form separation on cuda:0: a recording of --seconds (default 600 s at 11 025 Hz, L = 6 615 000) through
separate_long with the full-size model (train_MUSIC flags: unet7 + resnet18dilated, fp32), stride 128, batch 16.

Prints (1) seconds of audio separated per second of wall time, audio-visual and audio-only, with the split between
STFT, window prepare, visual trunk, U-Net, agreement (+ host alignment), stitch and iSTFT — each stage of the real
separate_long call wrapped in device synchronisations; (2) avsep_window_prepare and avsep_mask_stitch alone: time,
algorithmic bytes, bytes/s against the 8 TB/s HBM peak, and the same result composed from the older entry points
(gathered slices + K.warp + log; K.warp(.., 0) on every window + a torch cross-fade), outputs compared.
With --channels C (C >= 1) also (3) the audio-visual call with the recording's C channels kept (separate_long(channels=...)):
wall time and stage split, the stages of the channel path (second STFT, stitch_channels, iSTFT over N*C rows) next to the
mono ones; and avsep_mask_stitch on the C magnitudes alone against C launches of it on one magnitude each, outputs
compared bit for bit.
With --wiener K as well (4) that call runs K passes of the multichannel Wiener filter (separate_long(wiener=K)): the stage
split gains mwf_cov and mwf_apply; and kernels.mwf alone (one pass on the soft source images of the C channels) against the
same result composed on the device from torch ops (torch.polar, einsum, torch.linalg.solve on complex64), the two timed in
alternation: time, algorithmic bytes, share of the HBM peak, outputs compared as complex numbers.
With --wiener_span H as well (4b) the audio-visual call runs those passes with time-varying covariances
(separate_long(wiener_span=H)): the stage split gains mwf_cov_tv and mwf_apply_tv; and one pass of kernels.mwf(span=H) is
event-timed against one time-invariant pass of kernels.mwf on the same inputs, the two in alternation: time, algorithmic
bytes (the invariant pass's plus the slab and covariance traffic) and share of the HBM peak.  --wiener_span_rows runs
only that comparison, without the model: C = 2 and 8 channels, N = 2, spans 64 ... 4096, on a spectrogram as long as --seconds.
With --phase_iters K (5) the audio-visual call runs K mixture-consistent phase iterations (separate_long(phase_iters=K), with
the channels and the Wiener passes of the options above when they are given): wall time, and the split gains misi (and
misi_channels); and one kernels.Stft.misi call of K passes on the recording at N = 2, G = 1 and N = 2, G = 2 against the same
result composed on the device from Stft.istft, torch arithmetic and Stft.stft, the two timed in alternation with device
events; the two kernels the call adds (overlap-add + consistency, re-phase) are timed per launch from a profiler trace of
one call: algorithmic bytes per pass and their share of the HBM peak.
Every number is a median over --reps runs after warm-up; the last line is one JSON object.
Usage: python tools/longform_bench.py [--seconds 600] [--reps 5] [--kernel-reps 20] [--channels C [--wiener K [--wiener_span H]]] [--phase_iters K]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import avsep_amd as P  # noqa: E402
from avsep_amd import separate as S  # noqa: E402
from stage_clock import StageClock  # noqa: E402

HBM_PEAK = 8.0e12


def median_ms(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return statistics.median(out)


def alternating_median_ms(fns, reps, warmup=2):
    """Medians of several functions timed in alternation (a, b, a, b, ...) with device events, after warm-up of each."""
    for fn in fns:
        for _ in range(warmup):
            fn()
    out = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            out[i].append(e0.elapsed_time(e1))
    return [statistics.median(o) for o in out]


def staged_run(nets, wav, frames, args, use_vis, stride, batch, channels=None, wiener=0, phase_iters=0, wiener_span=0):
    K = P.kernels
    clk = StageClock()
    # with channels the second call of each transform is the channel path's: C rows in, N*C rows out
    clk.wrap(K.Stft, "stft", "stft" if channels is None else ["stft", "stft_channels"])
    clk.wrap(K.Stft, "istft", "istft" if channels is None else ["istft", "istft_channels"])
    clk.wrap(K.Stft, "misi", "misi" if channels is None else ["misi", "misi_channels"])
    tv = "_tv" if wiener_span else ""                                    # one pair of wrappers serves both filters; a run has one span
    clk.wrap(K, "_mwf_cov", "mwf_cov" + tv)
    clk.wrap(K, "_mwf_apply", "mwf_apply" + tv)
    clk.wrap(K, "window_prepare", "window_prepare")
    clk.wrap(K, "window_agreement", "agreement")
    clk.wrap(S, "align_permutations", "agreement")
    clk.wrap(K, "mask_stitch", "stitch" if channels is None else ["stitch", "stitch_channels"])
    clk.wrap(nets[0], "forward", "unet")
    clk.wrap(nets[1], "forward", "visual_trunk")
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        S.separate_long(nets, wav, frames, args, use_vis, stride, batch, channels=channels, wiener=wiener, phase_iters=phase_iters,
                        wiener_span=wiener_span)
        torch.cuda.synchronize()
        total = (time.perf_counter() - t0) * 1e3
    finally:
        clk.restore()
    clk.ms["other"] = total - sum(clk.ms.values())
    clk.ms["total"] = total
    return clk.ms


def whole_runs(nets, wav, frames, args, use_vis, stride, batch, reps, channels=None, wiener=0, phase_iters=0, wiener_span=0):
    """Median wall time of the unwrapped call, and the median per-stage split of wrapped calls."""
    def once():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        S.separate_long(nets, wav, frames, args, use_vis, stride, batch, channels=channels, wiener=wiener, phase_iters=phase_iters,
                        wiener_span=wiener_span)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    once()                                                               # warm-up: code objects, conv plans
    wall = statistics.median(once() for _ in range(reps))
    splits = [staged_run(nets, wav, frames, args, use_vis, stride, batch, channels, wiener, phase_iters, wiener_span) for _ in range(reps)]
    split = {k: statistics.median(s.get(k, 0.0) for s in splits) for k in splits[0]}
    return wall, split


def composed_prepare(mag, starts_t, width=256):
    """The older entry points: gather the K slices (zero past the end), +1e-10, K.warp, log."""
    Fin, F = mag.shape
    padded = torch.cat([mag, mag.new_zeros(Fin, width)], 1)
    idx = starts_t.long()[:, None] + torch.arange(width, device=mag.device)[None]       # [K,W]
    slices = padded[:, idx].permute(1, 0, 2).unsqueeze(1)                                # [K,1,Fin,W]
    w = P.kernels.warp((slices + 1e-10).contiguous(), 256, width, 1)
    return w, torch.log(w)


def composed_stitch(masks, starts_t, perm, mag, binary, thres, width=256):
    """The older entry points: K.warp(.., 0) on every (window, source), triangular weights, one index_add_ per tensor,
    divide, threshold, multiply.  (Recordings of at least one window: every window lies inside the recording.)"""
    Kw, N, Fo, W = masks.shape
    Fin, F = mag.shape
    picked = torch.gather(masks, 1, perm.long()[:, :, None, None].expand(-1, -1, Fo, W))
    lin = P.kernels.warp(picked.reshape(Kw * N, 1, Fo, W), Fin, W, 0).reshape(Kw, N, Fin, W)
    j = torch.arange(W, device=mag.device)
    tri = torch.minimum(j + 1, W - j).float()
    idx = (starts_t.long()[:, None] + j[None]).reshape(-1)
    acc = torch.zeros(N, Fin, F, device=mag.device)
    acc.index_add_(2, idx, (lin * tri).permute(1, 2, 0, 3).reshape(N, Fin, Kw * W))
    wsum = torch.zeros(F, device=mag.device).index_add_(0, idx, tri.repeat(Kw))
    M = acc / wsum
    return mag * ((M > thres).float() if binary else M), M


def kernel_rows(mag, starts_t, masks, perm, args, reps):
    K = P.kernels
    Fin, F = mag.shape
    Kw, N, Fo, W = masks.shape
    rows = {}
    # window prepare
    a = K.window_prepare(mag, starts_t)
    b = composed_prepare(mag, starts_t)
    bytes_prep = 4 * (Fin * F + 2 * Kw * Fo * W)
    ms_f = median_ms(lambda: K.window_prepare(mag, starts_t), reps)
    ms_c = median_ms(lambda: composed_prepare(mag, starts_t), reps)
    rows["window_prepare"] = {"fused_ms": ms_f, "composed_ms": ms_c, "algorithmic_bytes": bytes_prep,
                              "fused_bytes_per_s": bytes_prep / (ms_f * 1e-3), "share_of_hbm_peak": bytes_prep / (ms_f * 1e-3) / HBM_PEAK,
                              "max_abs_diff_vs_composed": max((a[0] - b[0]).abs().max().item(), (a[1] - b[1]).abs().max().item())}
    # mask stitch (binary masks as the flagship configuration has them; without the optional mask output)
    binary, thres = bool(args.binary_mask), args.mask_thres
    a = K.mask_stitch(masks, starts_t, perm, mag, False, thres, want_mask=True)
    b = composed_stitch(masks, starts_t, perm, mag, False, thres)
    bytes_st = 4 * (Kw * N * Fo * W + Fin * F + N * Fin * F) + 4 * (Kw + Kw * N)
    ms_f = median_ms(lambda: K.mask_stitch(masks, starts_t, perm, mag, binary, thres), reps)
    ms_c = median_ms(lambda: composed_stitch(masks, starts_t, perm, mag, binary, thres), reps)
    rows["mask_stitch"] = {"fused_ms": ms_f, "composed_ms": ms_c, "algorithmic_bytes": bytes_st,
                           "fused_bytes_per_s": bytes_st / (ms_f * 1e-3), "share_of_hbm_peak": bytes_st / (ms_f * 1e-3) / HBM_PEAK,
                           "max_abs_diff_vs_composed": (a[1] - b[1]).abs().max().item()}
    # agreement: reads both windows' shared halves for every (k, i, j)
    ms_a = median_ms(lambda: K.window_agreement(masks, starts_t), reps)
    rows["window_agreement"] = {"fused_ms": ms_a}
    return rows


def channel_stitch_row(mag_c, starts_t, masks, perm, args, reps):
    """avsep_mask_stitch on mag_c [C,Fin,F] against C launches of it on one channel each (stacked: what the caller would
    have to do for the [N,C,Fin,F] layout one iSTFT takes; and the launches alone, without the stack)."""
    K = P.kernels
    Cc, Fin, F = mag_c.shape
    Kw, N, Fo, W = masks.shape
    binary, thres = bool(args.binary_mask), args.mask_thres
    rows = [mag_c[c].contiguous() for c in range(Cc)]

    def launches():
        return [K.mask_stitch(masks, starts_t, perm, m, binary, thres)[0] for m in rows]
    a = K.mask_stitch(masks, starts_t, perm, mag_c, binary, thres)[0]
    same = bool(torch.equal(a, torch.stack(launches(), 1)))
    nbytes = 4 * (Kw * N * Fo * W + Cc * Fin * F + N * Cc * Fin * F) + 4 * (Kw + Kw * N)
    ms_f = median_ms(lambda: K.mask_stitch(masks, starts_t, perm, mag_c, binary, thres), reps)
    ms_l = median_ms(launches, reps)
    ms_s = median_ms(lambda: torch.stack(launches(), 1), reps)
    return {"channels": Cc, "fused_ms": ms_f, "launches_ms": ms_l, "launches_stacked_ms": ms_s, "algorithmic_bytes": nbytes,
            "fused_bytes_per_s": nbytes / (ms_f * 1e-3), "share_of_hbm_peak": nbytes / (ms_f * 1e-3) / HBM_PEAK,
            "launches_over_fused": ms_l / ms_f, "bit_identical_to_launches": same}


FLT_MIN = 1.1754943508222875e-38


def composed_mwf(xmag, xph, ymag, yph, reg=1e-3):
    """One pass of the filter from torch ops on the device (complex64): the five steps of include/avsep.h as they stand."""
    X = torch.polar(xmag, xph)                                                          # [C,Fin,F]
    Y = torch.polar(ymag, yph.expand_as(ymag).contiguous())                             # [N,C,Fin,F]
    Cc = X.shape[0]
    v = (ymag * ymag).sum(1) / Cc                                                       # [N,Fin,F]
    R = torch.einsum("ncft,ndft->nfcd", Y, Y.conj()) / v.sum(-1).clamp_min(FLT_MIN)[:, :, None, None]
    Sm = torch.einsum("nft,nfcd->ftcd", v.to(R.dtype), R)
    lam = reg * torch.diagonal(Sm, dim1=-2, dim2=-1).real.sum(-1) / Cc + FLT_MIN
    Sm = Sm + lam[:, :, None, None] * torch.eye(Cc, device=X.device, dtype=R.dtype)
    z = torch.linalg.solve(Sm, X.permute(1, 2, 0).contiguous())                         # [Fin,F,C]
    Wn = torch.einsum("nfcd,ftd->ncft", R, z) * v[:, None]
    return Wn.abs(), Wn.angle()


def mwf_row(mag_c, phase_c, masks_lin, reps):
    """kernels.mwf (one pass) on the soft source images masks_lin [N,Fin,F] x mag_c [C,Fin,F] against composed_mwf."""
    K = P.kernels
    Cc, Fin, F = mag_c.shape
    N = masks_lin.shape[0]
    ymag = (masks_lin[:, None] * mag_c[None]).contiguous()
    a = torch.polar(*K.mwf(mag_c, phase_c, ymag, phase_c))
    b = torch.polar(*composed_mwf(mag_c, phase_c, ymag, phase_c))
    diff = ((a - b).abs().max() / b.abs().max()).item()
    del a, b
    # cov reads ymag and the shared phase; apply reads X (magnitude, phase) and ymag, and writes magnitude and phase
    nbytes = 4 * Fin * F * (N * Cc + Cc + 2 * Cc + N * Cc + 2 * N * Cc)
    ms_f, ms_c = alternating_median_ms([lambda: K.mwf(mag_c, phase_c, ymag, phase_c),
                                        lambda: composed_mwf(mag_c, phase_c, ymag, phase_c)], reps)
    return {"channels": Cc, "sources": N, "fused_ms": ms_f, "composed_ms": ms_c, "algorithmic_bytes": nbytes,
            "fused_bytes_per_s": nbytes / (ms_f * 1e-3), "share_of_hbm_peak": nbytes / (ms_f * 1e-3) / HBM_PEAK,
            "composed_over_fused": ms_c / ms_f, "max_rel_diff_vs_composed": diff}


def mwf_tv_row(mag_c, phase_c, masks_lin, span, reps):
    """One pass of kernels.mwf(span=H) (time-varying covariances) against one time-invariant pass of kernels.mwf on the
    same soft source images, the two timed in alternation."""
    K = P.kernels
    Cc, Fin, F = mag_c.shape
    N = masks_lin.shape[0]
    ymag = (masks_lin[:, None] * mag_c[None]).contiguous()
    inv_bytes = 4 * Fin * F * (N * Cc + Cc + 2 * Cc + N * Cc + 2 * N * Cc)
    # on top of the invariant pass: two slabs of C (C + 1) + 1 floats per (segment, source, row) written once and read once,
    # and the K covariances per (source, row) written once and read once
    segments, centres = -(-F // span), K.mwf_centres(F, span)
    nbytes = inv_bytes + 2 * 4 * N * Fin * (segments * 2 * (Cc * (Cc + 1) + 1) + centres * Cc * Cc * 2)
    ms_tv, ms_inv = alternating_median_ms([lambda: K.mwf(mag_c, phase_c, ymag, phase_c, span=span),
                                           lambda: K.mwf(mag_c, phase_c, ymag, phase_c)], reps)
    return {"channels": Cc, "sources": N, "span": span, "local_ms": ms_tv, "invariant_ms": ms_inv, "local_over_invariant": ms_tv / ms_inv,
            "algorithmic_bytes": nbytes, "invariant_algorithmic_bytes": inv_bytes, "local_bytes_per_s": nbytes / (ms_tv * 1e-3),
            "share_of_hbm_peak": nbytes / (ms_tv * 1e-3) / HBM_PEAK,
            "invariant_share_of_hbm_peak": inv_bytes / (ms_inv * 1e-3) / HBM_PEAK}


def wiener_span_rows(seconds, reps, dev):
    """mwf_tv_row over channels and spans on a random spectrogram of ``seconds`` at 11 025 Hz (Fin = 512, hop 256)."""
    Fin, F, N = 512, int(round(seconds * 11025)) // 256 + 1, 2
    rows = []
    with torch.no_grad():
        for Cc in (2, 8):
            mag = torch.rand(Fin, F, device=dev) * 30
            lin = torch.rand(N, Fin, F, device=dev)
            ph_c = (torch.rand(Cc, Fin, F, device=dev) * 2 - 1) * 3.14159
            mag_r = (mag[None] * (0.5 + torch.rand(Cc, Fin, F, device=dev))).contiguous()
            for span in (64, 128, 256, 1024, 4096):
                r = mwf_tv_row(mag_r, ph_c, lin, span, reps)
                rows.append(r)
                print(f"mwf C={Cc} N={N} F={F}, covariances every {span} frames: {r['local_ms']:.3f} ms ({100 * r['share_of_hbm_peak']:.0f}% of "
                      f"8 TB/s on {r['algorithmic_bytes'] / 1e6:.0f} MB); time-invariant pass {r['invariant_ms']:.3f} ms "
                      f"({100 * r['invariant_share_of_hbm_peak']:.0f}%): {r['local_over_invariant']:.2f} x", flush=True)
            del mag, lin, ph_c, mag_r
    return rows


def composed_misi(plan, mix, A, phase, passes):
    """The passes from the older entry points: Stft.istft, torch arithmetic, Stft.stft (magnitude and angle written, the
    magnitude thrown away, the angle read back through the inverse)."""
    N, G, bins, F = A.shape
    rows = A.reshape(N * G, bins, F)
    s = plan.istft(rows, phase.expand(N, G, bins, F).reshape(N * G, bins, F).contiguous()).reshape(N, G, -1)
    for _ in range(passes):
        e = mix - s.sum(0)
        _, ph = plan.stft((s + e / N).reshape(N * G, -1))
        s = plan.istft(rows, ph).reshape(N, G, -1)
    return s


def misi_kernel_times(fn):
    """Per-launch device time (ms) of the two kernels csrc/misi.hip adds, from a profiler trace of one call; None where the
    trace does not name them."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            fn()
            torch.cuda.synchronize()
        out = {}
        for ev in prof.key_averages():
            for name in ("misi_ola_kernel", "misi_rephase_kernel"):
                if name in ev.key and ev.count:
                    us = getattr(ev, "device_time_total", None) or getattr(ev, "cuda_time_total", 0.0)
                    tot, cnt = out.get(name, (0.0, 0))
                    out[name] = (tot + us, cnt + ev.count)
        return {k: t / c * 1e-3 for k, (t, c) in out.items() if t > 0}
    except Exception as e:                                                # a tool's extra: the rows above do not depend on it
        print(f"profiler trace unavailable ({type(e).__name__}: {e}); per-kernel times not measured", flush=True)
        return {}


def misi_row(plan, wav, mag, phase, G, passes, reps):
    """One Stft.misi call of ``passes`` passes for N = 2 stems of each of G mixtures as long as the recording, against
    composed_misi; the two timed in alternation."""
    N = 2
    bins, F = mag.shape
    out_len = plan.hop * (F - 1)
    gains = torch.linspace(1.0, 0.5, G, device=wav.device)[:, None]
    mix = (wav[None, :out_len] * gains).contiguous()
    A = (torch.rand(N, 1, bins, F, device=wav.device) * (mag[None, None] * gains[None, :, :, None])).contiguous()
    ph = phase[None].expand(G, -1, -1).contiguous()
    a, b = plan.misi(mix, A, ph, passes), composed_misi(plan, mix, A, ph, passes)
    diff = ((a - b).abs().max() / b.abs().max()).item()
    del a, b
    ms_f, ms_c = alternating_median_ms([lambda: plan.misi(mix, A, ph, passes), lambda: composed_misi(plan, mix, A, ph, passes)], reps)
    R = N * G
    # per pass: the overlap-add reads the inverse GEMM's output, the table and the mixture and writes the projected stems; the
    # re-phase reads both planes of the forward GEMM's output and the magnitudes and writes the inverse GEMM's operand
    bytes_ola = 4 * (R * plan.n_fft * F + out_len + G * out_len + R * out_len)
    bytes_reph = 4 * R * bins * F * 5
    per = misi_kernel_times(lambda: plan.misi(mix, A, ph, passes))
    row = {"sources": N, "groups": G, "passes": passes, "fused_ms": ms_f, "composed_ms": ms_c, "composed_over_fused": ms_c / ms_f,
           "fused_ms_per_pass": ms_f / passes, "max_rel_diff_vs_composed": diff,
           "ola_algorithmic_bytes_per_pass": bytes_ola, "rephase_algorithmic_bytes_per_pass": bytes_reph}
    for key, name, nb in (("ola", "misi_ola_kernel", bytes_ola), ("rephase", "misi_rephase_kernel", bytes_reph)):
        if name in per:
            row[f"{key}_ms"] = per[name]
            row[f"{key}_share_of_hbm_peak"] = nb / (per[name] * 1e-3) / HBM_PEAK
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=600.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernel-reps", type=int, default=20)
    ap.add_argument("--stride", type=int, default=128)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--frame-size", type=int, default=224)
    ap.add_argument("--channels", type=int, default=0, help="also measure the call that keeps C channels (0: skip)")
    ap.add_argument("--wiener", type=int, default=0, help="with --channels: also K passes of the multichannel Wiener filter (0: skip)")
    ap.add_argument("--wiener_span", type=int, default=0, help="with --wiener: also the passes with time-varying covariances H frames apart "
                                                               "(a multiple of 64 in 64 ... 4096; 0: skip)")
    ap.add_argument("--wiener_span_rows", action="store_true", help="only one local against one time-invariant pass of kernels.mwf, "
                                                                    "C = 2 and 8, spans 64 ... 4096 (no model)")
    ap.add_argument("--phase_iters", type=int, default=0, help="also K mixture-consistent phase iterations: the call and Stft.misi alone (0: skip)")
    ap.add_argument("--mwf-reps", type=int, default=5, help="timed repetitions of the mwf row (the composition is slow)")
    o = ap.parse_args()
    if o.wiener and o.channels < 1:
        raise SystemExit("--wiener measures the channel path: pass --channels C as well")
    if o.wiener_span and not o.wiener:
        raise SystemExit("--wiener_span measures the Wiener passes: pass --wiener K as well")
    if o.wiener_span and not (64 <= o.wiener_span <= 4096 and o.wiener_span % 64 == 0):
        raise SystemExit(f"--wiener_span takes a multiple of 64 frames in 64 ... 4096, got {o.wiener_span}")
    if not torch.cuda.is_available():
        raise SystemExit("longform_bench measures on an MI355X; there is nothing to report without one")
    dev = torch.device("cuda", 0)
    if o.wiener_span_rows:
        torch.manual_seed(0)
        print(json.dumps({"seconds": o.seconds, "mwf_tv_rows": wiener_span_rows(o.seconds, o.mwf_reps, dev)}), flush=True)
        return
    args = P.arguments.train_music_args()
    args.stft_pad_mode = "reflect"
    torch.manual_seed(0)
    mb = P.ModelBuilder()
    snd = mb.build_sound(arch=args.arch_sound, fc_dim=args.num_channels, fusion_type=args.fusion_type, att_type=args.att_type)
    frm = mb.build_frame(arch=args.arch_frame, fc_dim=args.vis_channels, pool_type=args.img_pool)
    nets = (snd.to(dev).eval(), frm.to(dev).eval())
    L = int(round(o.seconds * args.audRate))
    wav = (torch.rand(L, device=dev) * 2 - 1) * 0.3
    frames = [torch.randn(1, 3, o.frame_size, o.frame_size, device=dev) for _ in range(args.num_mix)]
    audio_s = L / args.audRate
    result = {"seconds": audio_s, "samples": L, "stride_frames": o.stride, "batch": o.batch, "model": f"{args.arch_sound}+{args.arch_frame}",
              "precision": P.kernels.get_precision() if hasattr(P.kernels, "get_precision") else "f32"}
    for name, use_vis in (("av", True), ("ao", False)):
        wall, split = whole_runs(nets, wav, frames, args, use_vis, o.stride, o.batch, o.reps)
        result[name] = {"wall_ms": wall, "audio_seconds_per_second": audio_s / (wall * 1e-3), "split_ms": split}
        print(f"{name.upper()}: {wall:9.1f} ms for {audio_s:.0f} s of audio = {audio_s / (wall * 1e-3):8.1f} x real time", flush=True)
        for k, v in split.items():
            print(f"    {k:16s} {v:9.2f} ms", flush=True)
    if o.channels > 0:
        gains = torch.linspace(1.0, 0.5, o.channels, device=dev)[:, None]
        ch = (wav[None] * gains).contiguous()                             # C channels of the recording, as long as wav
        wall, split = whole_runs(nets, wav, frames, args, True, o.stride, o.batch, o.reps, channels=ch)
        result["av_channels"] = {"channels": o.channels, "wall_ms": wall, "audio_seconds_per_second": audio_s / (wall * 1e-3),
                                 "split_ms": split}
        print(f"AV, {o.channels} channels kept: {wall:9.1f} ms = {audio_s / (wall * 1e-3):8.1f} x real time", flush=True)
        for k, v in split.items():
            print(f"    {k:16s} {v:9.2f} ms", flush=True)
        if o.wiener:
            wall, split = whole_runs(nets, wav, frames, args, True, o.stride, o.batch, o.reps, channels=ch, wiener=o.wiener)
            result["av_channels_wiener"] = {"channels": o.channels, "wiener": o.wiener, "wall_ms": wall,
                                            "audio_seconds_per_second": audio_s / (wall * 1e-3), "split_ms": split}
            print(f"AV, {o.channels} channels kept, Wiener x{o.wiener}: {wall:9.1f} ms = {audio_s / (wall * 1e-3):8.1f} x real time", flush=True)
            for k, v in split.items():
                print(f"    {k:16s} {v:9.2f} ms", flush=True)
        if o.wiener_span:
            wall, split = whole_runs(nets, wav, frames, args, True, o.stride, o.batch, o.reps, channels=ch, wiener=o.wiener,
                                     wiener_span=o.wiener_span)
            result["av_channels_wiener_span"] = {"channels": o.channels, "wiener": o.wiener, "wiener_span": o.wiener_span, "wall_ms": wall,
                                                 "audio_seconds_per_second": audio_s / (wall * 1e-3), "split_ms": split}
            print(f"AV, {o.channels} channels kept, Wiener x{o.wiener}, covariances every {o.wiener_span} frames: {wall:9.1f} ms = "
                  f"{audio_s / (wall * 1e-3):8.1f} x real time", flush=True)
            for k, v in split.items():
                print(f"    {k:16s} {v:9.2f} ms", flush=True)
    if o.phase_iters:
        ch = (wav[None] * torch.linspace(1.0, 0.5, o.channels, device=dev)[:, None]).contiguous() if o.channels > 0 else None
        wall, split = whole_runs(nets, wav, frames, args, True, o.stride, o.batch, o.reps, channels=ch, wiener=o.wiener,
                                 phase_iters=o.phase_iters, wiener_span=o.wiener_span)
        result["av_phase_iters"] = {"channels": o.channels, "wiener": o.wiener, "phase_iters": o.phase_iters, "wall_ms": wall,
                                    "audio_seconds_per_second": audio_s / (wall * 1e-3), "split_ms": split}
        print(f"AV, phase iterations x{o.phase_iters}" + (f", {o.channels} channels kept" if o.channels else "")
              + (f", Wiener x{o.wiener}" if o.wiener else "") + f": {wall:9.1f} ms = {audio_s / (wall * 1e-3):8.1f} x real time", flush=True)
        for k, v in split.items():
            print(f"    {k:16s} {v:9.2f} ms", flush=True)
        del ch
    with torch.no_grad():
        plan = P.kernels.Stft(dev, args.stft_frame, args.stft_hop, "reflect")
        if o.phase_iters:
            m1, p1 = plan.stft(wav[None])
            for G in (1, 2):
                r = result.setdefault("misi", {})[f"N2_G{G}"] = misi_row(plan, wav, m1[0], p1[0], G, o.phase_iters, o.reps)
                per = ", ".join(f"{k} {r[k + '_ms']:.3f} ms / launch ({100 * r[k + '_share_of_hbm_peak']:.0f}% of 8 TB/s on "
                                f"{r[k + '_algorithmic_bytes_per_pass'] / 1e6:.0f} MB)" for k in ("ola", "rephase") if k + "_ms" in r)
                print(f"misi N=2 G={G}, {o.phase_iters} passes: {r['fused_ms']:.3f} ms ({r['fused_ms_per_pass']:.3f} ms / pass); composed from "
                      f"istft + torch + stft {r['composed_ms']:.3f} ms ({r['composed_over_fused']:.2f} x); max |diff| / max |ref| "
                      f"{r['max_rel_diff_vs_composed']:.2e}" + (f"; {per}" if per else "; per-kernel times not measured"), flush=True)
            del m1, p1
        mag = plan.stft(wav[None], want_phase=False)[0][0].contiguous()
        starts = S.plan_windows(mag.shape[1], o.stride)
        starts_t = torch.tensor(starts, dtype=torch.int32, device=dev)
        masks = torch.rand(len(starts), args.num_mix, 256, 256, device=dev)
        perm = torch.arange(args.num_mix, dtype=torch.int32, device=dev).repeat(len(starts), 1)
        result["frames"], result["windows"] = mag.shape[1], len(starts)
        result["kernels"] = kernel_rows(mag, starts_t, masks, perm, args, o.kernel_reps)
        if o.channels > 0:
            mag_c = (mag[None] * gains[:, :, None]).contiguous()
            r = result["kernels"]["mask_stitch_channels"] = channel_stitch_row(mag_c, starts_t, masks, perm, args, o.kernel_reps)
            print(f"mask_stitch_channels C={o.channels}: {r['fused_ms']:.3f} ms ({r['fused_bytes_per_s'] / 1e12:.2f} TB/s algorithmic, "
                  f"{100 * r['share_of_hbm_peak']:.0f}% of 8 TB/s); {o.channels} launches of mask_stitch {r['launches_ms']:.3f} ms "
                  f"({r['launches_over_fused']:.2f} x; stacked to [N,C,Fin,F] {r['launches_stacked_ms']:.3f} ms); "
                  f"bit-identical {r['bit_identical_to_launches']}", flush=True)
        if o.wiener:
            lin = torch.rand(args.num_mix, mag.shape[0], mag.shape[1], device=dev)
            ph_c = (torch.rand(o.channels, mag.shape[0], mag.shape[1], device=dev) * 2 - 1) * 3.14159
            mag_r = (mag[None] * (0.5 + torch.rand(o.channels, mag.shape[0], mag.shape[1], device=dev))).contiguous()
            r = result["kernels"]["mwf"] = mwf_row(mag_r, ph_c, lin, o.mwf_reps)
            print(f"mwf C={o.channels} N={args.num_mix}, one pass: {r['fused_ms']:.3f} ms ({r['fused_bytes_per_s'] / 1e12:.2f} TB/s algorithmic, "
                  f"{100 * r['share_of_hbm_peak']:.0f}% of 8 TB/s); composed from torch ops {r['composed_ms']:.3f} ms "
                  f"({r['composed_over_fused']:.1f} x); max |diff| / max |ref| {r['max_rel_diff_vs_composed']:.2e}", flush=True)
            if o.wiener_span:
                r = result["kernels"]["mwf_tv"] = mwf_tv_row(mag_r, ph_c, lin, o.wiener_span, o.mwf_reps)
                print(f"mwf C={o.channels} N={args.num_mix}, one pass with covariances every {o.wiener_span} frames: {r['local_ms']:.3f} ms "
                      f"({r['local_bytes_per_s'] / 1e12:.2f} TB/s algorithmic, {100 * r['share_of_hbm_peak']:.0f}% of 8 TB/s); "
                      f"time-invariant pass {r['invariant_ms']:.3f} ms ({100 * r['invariant_share_of_hbm_peak']:.0f}%): "
                      f"{r['local_over_invariant']:.2f} x", flush=True)
    for k, r in result["kernels"].items():
        if k in ("mask_stitch_channels", "mwf", "mwf_tv"):
            continue
        if "composed_ms" in r:
            print(f"{k}: fused {r['fused_ms']:.3f} ms ({r['fused_bytes_per_s'] / 1e12:.2f} TB/s algorithmic, "
                  f"{100 * r['share_of_hbm_peak']:.0f}% of 8 TB/s), composed {r['composed_ms']:.3f} ms "
                  f"({r['composed_ms'] / r['fused_ms']:.1f} x), max |diff| {r['max_abs_diff_vs_composed']:.2e}", flush=True)
        else:
            print(f"{k}: {r['fused_ms']:.3f} ms", flush=True)
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
