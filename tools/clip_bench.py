"""Separating a filmed recording on cuda:0: ten minutes of 11 025 Hz audio (L = 6 615 000) with two 8 fps stacks of 224 x 224
frames (T = 4 800 each) through separate_long(frame_times=...) and the full-size model (train_MUSIC flags: unet7 +
resnet18dilated, fp32).

Prints (a) wall time of the whole call with the stacks on the GPU and the split visual trunk / window_reduce / everything
else — the two stages of the real call wrapped in device synchronisations; (b) the same call with the stacks on the host
(moved batch by batch); (c) the same call with ONE shared frame per source, what a caller had before; (d) avsep_window_reduce
alone on the call's own table and feature shape [T, 256, 14, 14]: time between device events around back-to-back launches,
bytes (every frame once + the output: what the algorithm needs; and as issued, every frame once per window that holds it),
bytes/s against the 8 TB/s HBM peak, beside its composition from index_select + mean per window, and their largest
difference.  Every number is a median over --reps runs after a warm-up; the last line is one JSON object.
Usage: python tools/clip_bench.py [--minutes 10] [--fps 8] [--reps 3] [--kernel-reps 10] [--skip-host] [--kernel-only]"""
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


def median_ms(fn, reps, warmup=2, inner=10):
    """Median over `reps` windows of `inner` back-to-back calls between two device events, per call."""
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


def staged_run(call, net_frame):
    """One call with net_frame.forward and kernels.window_reduce bracketed by device synchronisations."""
    clk = StageClock()
    clk.ms.update(visual_trunk=0.0, window_reduce=0.0)
    clk.wrap(net_frame, "forward", "visual_trunk")
    clk.wrap(P.kernels, "window_reduce", "window_reduce")
    try:
        total, _ = wall_ms(call)
    finally:
        clk.restore()
    clk.ms["other"] = total - clk.ms["visual_trunk"] - clk.ms["window_reduce"]
    clk.ms["total"] = total
    return clk.ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=10.0)
    ap.add_argument("--fps", type=float, default=8.0)
    ap.add_argument("--frame-size", type=int, default=224)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernel-reps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--skip-host", action="store_true", help="leave out the run with the stacks on the host")
    ap.add_argument("--kernel-only", action="store_true", help="section (d) alone: no network is built or run")
    o = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("clip_bench measures on an MI355X; there is nothing to report without one")
    dev = torch.device("cuda", 0)
    args = P.arguments.train_music_args()
    args.stft_pad_mode = "reflect"
    torch.manual_seed(0)
    Ls = int(round(o.minutes * 60 * args.audRate))
    T, Sz = int(round(o.minutes * 60 * o.fps)), o.frame_size
    times = torch.arange(T, dtype=torch.float64) / o.fps
    result = {"samples": Ls, "video_frames": T, "fps": o.fps, "frame_size": Sz, "batch": o.batch,
              "model": f"{args.arch_sound}+{args.arch_frame}", "precision": P.kernels.get_precision()}
    if not o.kernel_only:
        whole_call(o, args, dev, Ls, T, Sz, times, result)
    kernel_alone(o, args, dev, Ls, T, times, result)
    print(json.dumps(result), flush=True)


def whole_call(o, args, dev, Ls, T, Sz, times, result):
    mb = P.ModelBuilder()
    snd = mb.build_sound(arch=args.arch_sound, fc_dim=args.num_channels, fusion_type=args.fusion_type, att_type=args.att_type)
    frm = mb.build_frame(arch=args.arch_frame, fc_dim=args.vis_channels, pool_type=args.img_pool)
    nets = (snd.to(dev).eval(), frm.to(dev).eval())
    wav = (torch.rand(Ls, device=dev) * 2 - 1) * 0.3
    stacks = [torch.randn(T, 3, Sz, Sz, device=dev) for _ in range(2)]

    def clip_call(frames):
        return lambda: S.separate_long(nets, wav, frames, args, True, 128, batch=o.batch, frame_times=times)

    def med(call):
        call()                                                                  # warm-up: code objects, conv plans
        return statistics.median(wall_ms(call)[0] for _ in range(o.reps))
    on_gpu = clip_call(stacks)
    result["clip_ms"] = med(on_gpu)
    splits = [staged_run(on_gpu, nets[1]) for _ in range(o.reps)]
    result["clip_split_ms"] = {k: statistics.median(s[k] for s in splits) for k in splits[0]}
    result["windows"] = len(on_gpu()["starts"])
    print(f"clip, stacks on the GPU: {result['clip_ms']:.1f} ms for {result['windows']} windows, {T} frames per source", flush=True)
    for k, v in result["clip_split_ms"].items():
        print(f"    {k:16s} {v:9.2f} ms", flush=True)
    shared = [s[:1].contiguous() for s in stacks]
    result["shared_frame_ms"] = med(lambda: S.separate_long(nets, wav, shared, args, True, 128, batch=o.batch))
    print(f"one shared frame per source: {result['shared_frame_ms']:.1f} ms", flush=True)
    if not o.skip_host:
        host = [s.cpu() for s in stacks]
        result["clip_host_stacks_ms"] = med(clip_call(host))
        print(f"clip, stacks on the host: {result['clip_host_stacks_ms']:.1f} ms", flush=True)
        del host


def kernel_alone(o, args, dev, Ls, T, times, result):
    """Section (d): the kernel on the call's table and the feature shape of this model at 224 x 224."""
    starts = S.plan_windows(Ls // args.stft_hop + 1, 128)
    ranges = S.frames_of_windows(times, starts, args.audRate, args.stft_hop)
    f = torch.randn(T, 256, 14, 14, device=dev)
    Pn, Kw = f[0].numel(), ranges.shape[0]
    index = [torch.arange(a, a + n, device=dev) for a, n in ranges.tolist()]

    def composed():
        return torch.stack([f.index_select(0, i).mean(0) for i in index])
    diff = (P.kernels.window_reduce(f, ranges) - composed()).abs().max().item()
    table, out = ranges.to(dev), torch.empty(Kw, *f.shape[1:], device=dev)     # the entry point itself: the table is up already

    def launch():
        P.lib.call("avsep_window_reduce", P.lib.ptr(f), P.lib.ptr(table), T, Kw, Pn, 0, P.lib.ptr(out))
    ms_k = median_ms(launch, o.kernel_reps)
    ms_w = median_ms(lambda: P.kernels.window_reduce(f, ranges), o.kernel_reps)
    ms_c = median_ms(composed, o.kernel_reps, inner=3)
    need = 4 * Pn * (T + Kw)
    issued = 4 * Pn * (int(ranges[:, 1].sum()) + Kw)
    result["window_reduce"] = {"ms": ms_k, "windows": Kw, "frames_per_window": float(ranges[:, 1].double().mean()), "P": Pn,
                               "algorithmic_bytes": need, "issued_bytes": issued, "bytes_per_s": need / (ms_k * 1e-3),
                               "issued_bytes_per_s": issued / (ms_k * 1e-3), "share_of_hbm_peak": need / (ms_k * 1e-3) / HBM_PEAK,
                               "wrapper_ms": ms_w, "composed_ms": ms_c, "speedup": ms_c / ms_k, "max_abs_diff": diff}
    r = result["window_reduce"]
    print(f"window_reduce [{T},{Pn}] -> [{Kw},{Pn}] ({r['frames_per_window']:.1f} frames per window): {ms_k:.3f} ms, "
          f"{need / 1e9:.2f} GB needed ({r['bytes_per_s'] / 1e12:.2f} TB/s, {100 * r['share_of_hbm_peak']:.0f}% of 8 TB/s), "
          f"{issued / 1e9:.2f} GB issued ({r['issued_bytes_per_s'] / 1e12:.2f} TB/s); with the wrapper's table check and "
          f"upload {ms_w:.3f} ms; index_select + mean per window "
          f"{ms_c:.3f} ms -> {r['speedup']:.1f} x; max |diff| {diff:.2e}", flush=True)


if __name__ == "__main__":
    main()
