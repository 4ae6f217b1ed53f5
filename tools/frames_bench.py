"""Frames as shot on cuda:0 (csrc/frames.hip): ten minutes of 8 fps video, 4 800 uint8 frames of 360 x 640, through
frames.prepare at 224 (resize to 224 x 398, centre crop, ImageNet normalisation).

Prints and writes to --out (default profiles/frames_bench.json):
  (a) the kernel on the whole stack in one launch and on one trunk batch of --batch frames: time between device events, median
      of --reps after warm-up, per frame; the bytes the algorithm needs (of every input row only the columns the 224 cropped
      columns reach, once, plus the float32 output once) and the bytes of the whole frames plus the output, bytes/s of the
      former against the 8 TB/s HBM peak and the 6.29 TB/s a float4 copy reaches (MI355X_MICROARCH.md);
  (b) dataset.VideoTransform (Pillow) on one CPU core over --cpu-frames of the same frames, per frame, and the largest
      difference between the two results (0: they are equal bit for bit);
  (c) separate_long(frame_times=...) with the full-size model (train_MUSIC flags: unet7 + resnet18dilated, fp32) on ten minutes
      of audio and two such stacks on the host: wall time with uint8 stacks (prepared on the GPU batch by batch) and the share
      frames.prepare holds of it (the call bracketed by device synchronisations), beside the same call with the prepared float
      stacks on the host, which is what a caller had to hold before; the bytes each form moves up are printed beside the times
      (a 360 x 640 frame is 0.69 MB as shot and 0.60 MB prepared; frames shot at the trunk's own 224 x 224 are a quarter of that).
The last line is one JSON object.
Usage: python tools/frames_bench.py [--minutes 10] [--fps 8] [--reps 20] [--batch 16] [--cpu-frames 100] [--kernel-only] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import avsep_amd as P  # noqa: E402
from avsep_amd import dataset as D  # noqa: E402
from avsep_amd import frames as F  # noqa: E402
from avsep_amd import separate as S  # noqa: E402
from stage_clock import StageClock  # noqa: E402

HBM_PEAK, HBM_COPY = 8.0e12, 6.29e12
H, W, SIZE = 360, 640, 224


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


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def frame_bytes(plan):
    """Per frame: (bytes the algorithm needs, bytes of the whole frame and the output)."""
    hbound, vbound = plan.tables[1].numpy().astype(np.int64), plan.tables[3].numpy().astype(np.int64)
    (w, h), (i, j), s = plan.size, plan.crop, plan.img_size
    xa, xb, ya, yb = max(j, 0), min(j + s, w), max(i, 0), min(i + s, h)
    cols = hbound[xb - 1].sum() - hbound[xa, 0]
    rows = vbound[yb - 1].sum() - vbound[ya, 0]
    out = 3 * s * s * 4
    return int(rows * cols * 3 + out), plan.H * plan.W * 3 + out


def kernel_rows(o, dev, stack, plan, result):
    need, whole = frame_bytes(plan)
    result["bytes_per_frame"] = {"needed": need, "whole_frame_and_output": whole}
    for name, n in (("whole_stack", stack.shape[0]), ("trunk_batch", min(o.batch, stack.shape[0]))):
        part = stack[:n]
        ms = median_ms(lambda: F.prepare(part, plan), o.reps)
        rate = need * n / (ms * 1e-3)
        result[name] = {"frames": n, "ms": ms, "us_per_frame": 1e3 * ms / n, "needed_bytes_per_s": rate,
                        "whole_bytes_per_s": whole * n / (ms * 1e-3), "share_of_hbm_peak": rate / HBM_PEAK,
                        "share_of_float4_copy_rate": rate / HBM_COPY}
        print(f"{name}: {n} frames in {ms:.3f} ms, {1e3 * ms / n:.2f} us per frame, {rate / 1e12:.2f} TB/s of needed bytes "
              f"({100 * rate / HBM_PEAK:.0f}% of 8 TB/s, {100 * rate / HBM_COPY:.0f}% of the 6.29 TB/s of a float4 copy)", flush=True)


def cpu_row(o, stack, plan, result):
    from PIL import Image
    n = min(o.cpu_frames, stack.shape[0])
    host = stack[:n].cpu().numpy()
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        vt = D.VideoTransform(SIZE, False)
        t0 = time.perf_counter()
        ref = vt([Image.fromarray(f) for f in host]).permute(1, 0, 2, 3)
        ms = (time.perf_counter() - t0) * 1e3
    finally:
        torch.set_num_threads(threads)
    diff = (F.prepare(stack[:n], plan).cpu() - ref).abs().max().item()
    result["video_transform_cpu"] = {"frames": n, "us_per_frame": 1e3 * ms / n, "max_abs_diff_to_kernel": diff}
    print(f"VideoTransform on one CPU core: {1e3 * ms / n:.0f} us per frame over {n} frames; max |kernel - Pillow| = {diff}", flush=True)


def separate_rows(o, dev, stack, plan, result):
    args = P.arguments.train_music_args()
    args.stft_pad_mode = "reflect"
    assert args.imgSize == SIZE
    torch.manual_seed(0)
    mb = P.ModelBuilder()
    snd = mb.build_sound(arch=args.arch_sound, fc_dim=args.num_channels, fusion_type=args.fusion_type, att_type=args.att_type)
    frm = mb.build_frame(arch=args.arch_frame, fc_dim=args.vis_channels, pool_type=args.img_pool)
    nets = (snd.to(dev).eval(), frm.to(dev).eval())
    T = stack.shape[0]
    wav = (torch.rand(int(round(o.minutes * 60 * args.audRate)), device=dev) * 2 - 1) * 0.3
    times = torch.arange(T, dtype=torch.float64) / o.fps
    shot = stack.cpu()
    prepared = torch.cat([F.prepare(stack[a:a + 256], plan).cpu() for a in range(0, T, 256)], 0)

    def call(fr):
        return lambda: S.separate_long(nets, wav, [fr, fr], args, True, 128, batch=o.batch, frame_times=times)

    def med(fn):
        fn()                                                                    # warm-up: code objects, conv plans
        return statistics.median(wall_ms(fn)[0] for _ in range(3))
    rows = {"uint8_stacks_ms": med(call(shot)), "float_stacks_ms": med(call(prepared))}
    clk = StageClock()
    clk.wrap(F, "prepare", "frames_prepare")
    try:
        rows["uint8_stacks_synchronised_ms"] = wall_ms(call(shot))[0]
    finally:
        clk.restore()
    rows["frames_prepare_ms"] = clk.ms["frames_prepare"]
    rows["frames_prepare_share"] = clk.ms["frames_prepare"] / rows["uint8_stacks_synchronised_ms"]
    rows["host_bytes_uint8"], rows["host_bytes_float"] = 2 * shot.numel(), 2 * prepared.numel() * 4
    result["separate_fps"] = rows
    print(f"separate_long with two stacks of {T} frames on the host: {rows['uint8_stacks_ms']:.0f} ms as shot (uint8, "
          f"{rows['host_bytes_uint8'] / 1e9:.1f} GB up), {rows['float_stacks_ms']:.0f} ms prepared (float32, "
          f"{rows['host_bytes_float'] / 1e9:.1f} GB up); frames.prepare, bracketed by synchronisations, takes "
          f"{rows['frames_prepare_ms']:.1f} of {rows['uint8_stacks_synchronised_ms']:.0f} ms = {100 * rows['frames_prepare_share']:.1f}%",
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=10.0)
    ap.add_argument("--fps", type=float, default=8.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--cpu-frames", type=int, default=100)
    ap.add_argument("--kernel-only", action="store_true", help="sections (a) and (b): no network is built or run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frames_bench.json"))
    o = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("frames_bench measures on an MI355X; there is nothing to report without one")
    dev = torch.device("cuda", 0)
    T = int(round(o.minutes * 60 * o.fps))
    g = torch.Generator(device=dev).manual_seed(0)
    stack = torch.randint(0, 256, (T, H, W, 3), dtype=torch.uint8, device=dev, generator=g)
    plan = F.plan(H, W, SIZE)
    result = {"frames": T, "frame": [H, W], "img_size": SIZE, "resized": list(plan.size), "crop": list(plan.crop), "reps": o.reps}
    kernel_rows(o, dev, stack, plan, result)
    cpu_row(o, stack, plan, result)
    if not o.kernel_only:
        separate_rows(o, dev, stack, plan, result)
    result["command"] = "python tools/frames_bench.py"
    os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
    with open(o.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
