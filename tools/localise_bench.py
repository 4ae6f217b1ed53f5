"""Localisation on cuda:0: a 6 s clip (L = 65 535 at 11 025 Hz, one 256-frame window) with --frames video frames (default
180) of 224 x 224 through the full-size model (train_MUSIC flags: unet7 + resnet18dilated, fp32), in the two-frame form
and in duet.

Prints (a) wall time of localise() with the split STFT + window prepare + encoder / visual trunk / maps kernel / overlay
kernel — each stage of the real call wrapped in device synchronisations; (b) the same maps from the existing path, the
reference's own procedure: inference.NetWrapper.forward once per video frame on the clip's spectrogram (STFT computed once
outside the loop, nothing rendered); (c) avsep_localise_maps and avsep_heatmap_overlay alone: time between device events
around 20 back-to-back launches, algorithmic bytes, bytes/s against the 8 TB/s HBM peak.  Every number is a median over
--reps runs after warm-up; the last line is one JSON object.
Usage: python tools/localise_bench.py [--frames 180] [--reps 5] [--kernel-reps 20]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import avsep_amd as P  # noqa: E402
from avsep_amd import localise as L  # noqa: E402
from stage_clock import StageClock  # noqa: E402

HBM_PEAK = 8.0e12


def median_ms(fn, reps, warmup=3, inner=20):
    """Median over `reps` windows of `inner` back-to-back calls between two device events, per call: one launch of tens of
    microseconds between two events would mostly measure the events."""
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / inner)
    return statistics.median(out)


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def staged_run(nets, wav, frames, times, args, batch):
    K = P.kernels
    clk = StageClock()
    clk.wrap(K.Stft, "stft", "stft_encoder")
    clk.wrap(K, "window_prepare", "stft_encoder")
    clk.wrap(nets[0], "bottleneck", "stft_encoder")
    clk.wrap(nets[1], "forward", "visual_trunk")
    clk.wrap(K, "localise_maps", "maps_kernel")
    clk.wrap(K, "heatmap_overlay", "overlay_kernel")
    try:
        total, _ = wall_ms(lambda: L.localise(nets, wav, frames, times, args, batch=batch))
    finally:
        clk.restore()
    clk.ms["other"] = total - sum(clk.ms.values())
    clk.ms["total"] = total
    return clk.ms


def per_frame_loop(wrap, mag, frames, args):
    """The existing path: one whole forward pass (warp, U-Net encoder and decoder, trunk) per video frame, batch 1."""
    maps = []
    with torch.no_grad():
        for t in range(frames[0].shape[0]):
            maps.append(wrap.forward((mag, None), [f[t:t + 1] for f in frames], args, True)["maps"])
    return torch.cat(maps, 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=180)
    ap.add_argument("--frame-size", type=int, default=224)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernel-reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=16)
    o = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("localise_bench measures on an MI355X; there is nothing to report without one")
    dev = torch.device("cuda", 0)
    args = P.arguments.train_music_args()
    args.stft_pad_mode = "reflect"
    torch.manual_seed(0)
    mb = P.ModelBuilder()
    snd = mb.build_sound(arch=args.arch_sound, fc_dim=args.num_channels, fusion_type=args.fusion_type, att_type=args.att_type)
    frm = mb.build_frame(arch=args.arch_frame, fc_dim=args.vis_channels, pool_type=args.img_pool)
    nets = (snd.to(dev).eval(), frm.to(dev).eval())
    wrap = P.inference.NetWrapper(nets)
    T, S, Ls = o.frames, o.frame_size, args.audLen
    wav = (torch.rand(Ls, device=dev) * 2 - 1) * 0.3
    times = torch.arange(T, dtype=torch.float64) * (Ls / args.audRate / T)
    with torch.no_grad():
        mag = P.kernels.Stft(dev, args.stft_frame, args.stft_hop, "reflect").stft(wav[None], want_phase=False)[0][:, None].contiguous()
    result = {"frames": T, "frame_size": S, "samples": Ls, "batch": o.batch, "model": f"{args.arch_sound}+{args.arch_frame}",
              "precision": P.kernels.get_precision(), "flop_expectation": "5.1 TFLOP per-frame loop vs 1.2 TFLOP batched (duet, 180 frames)"}
    for name, n_in in (("two_frames", 2), ("duet", 1)):
        frames = [torch.randn(T, 3, S, S, device=dev) for _ in range(n_in)]
        L.localise(nets, wav, frames, times, args, batch=o.batch)                                # warm-up: code objects, conv plans
        fast = statistics.median(wall_ms(lambda: L.localise(nets, wav, frames, times, args, batch=o.batch))[0] for _ in range(o.reps))
        no_render = statistics.median(wall_ms(lambda: L.localise(nets, wav, frames, times, args, batch=o.batch, render=False))[0]
                                      for _ in range(o.reps))
        splits = [staged_run(nets, wav, frames, times, args, o.batch) for _ in range(o.reps)]
        split = {k: statistics.median(s.get(k, 0.0) for s in splits) for k in splits[0]}
        per_frame_loop(wrap, mag, frames, args)                                                  # warm-up
        runs = [wall_ms(lambda: per_frame_loop(wrap, mag, frames, args)) for _ in range(o.reps)]
        slow = statistics.median(r[0] for r in runs)
        got = L.localise(nets, wav, frames, times, args, batch=o.batch, render=False)["maps"]
        diff = (got - runs[-1][1]).abs().max().item()
        result[name] = {"localise_ms": fast, "localise_without_overlays_ms": no_render, "split_ms": split, "per_frame_loop_ms": slow,
                        "speedup_maps_only": slow / no_render, "speedup_with_overlays": slow / fast, "max_abs_diff_maps": diff}
        print(f"{name}: localise {fast:.1f} ms ({no_render:.1f} ms without overlays), per-frame loop {slow:.1f} ms "
              f"-> {slow / no_render:.1f} x (maps only), {slow / fast:.1f} x (with overlays); max |diff| {diff:.2e}", flush=True)
        for k, v in split.items():
            print(f"    {k:16s} {v:9.2f} ms", flush=True)
        # the two kernels alone
        C = 2
        feats = [torch.randn(T, 256, 14, 14, device=dev) for _ in range(n_in)]
        x = torch.randn(1, 512, 2, 2, device=dev)
        win = torch.zeros(T, dtype=torch.int32, device=dev)
        vs = feats * 2 if n_in == 1 else feats
        maps, _, _ = P.kernels.localise_maps(x, win, vs, "sig")
        table = torch.from_numpy(L.jet_table()).to(dev)
        fr = frames * 2 if n_in == 1 else frames
        ms_m = median_ms(lambda: P.kernels.localise_maps(x, win, vs, "sig"), o.kernel_reps)
        ms_o = median_ms(lambda: P.kernels.heatmap_overlay(maps, fr, table, 102), o.kernel_reps)
        b_m = 4 * (n_in * T * 256 * 196 + x.numel()) + 4 * T * C * 196
        b_o = 12 * S * S * T * n_in + 3 * S * S * T * C + 4 * T * C * 196
        result[name]["kernels"] = {
            "localise_maps": {"ms": ms_m, "algorithmic_bytes": b_m, "bytes_per_s": b_m / (ms_m * 1e-3),
                              "share_of_hbm_peak": b_m / (ms_m * 1e-3) / HBM_PEAK},
            "heatmap_overlay": {"ms": ms_o, "algorithmic_bytes": b_o, "bytes_per_s": b_o / (ms_o * 1e-3),
                                "share_of_hbm_peak": b_o / (ms_o * 1e-3) / HBM_PEAK}}
        for k, r in result[name]["kernels"].items():
            print(f"    {k}: {r['ms'] * 1e3:.1f} us, {r['algorithmic_bytes'] / 1e6:.1f} MB, {r['bytes_per_s'] / 1e12:.2f} TB/s "
                  f"({100 * r['share_of_hbm_peak']:.0f}% of 8 TB/s)", flush=True)
        del frames, feats
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
