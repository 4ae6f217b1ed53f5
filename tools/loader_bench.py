"""The training loader with the frames prepared in the workers (classic) and on the GPU (MUSICMixDataset(raw_frames=True),
train.py --gpu_frames), on cuda:0.  Writes a seeded synthetic dataset into a temporary folder (11 videos of 360 x 640 JPEGs at
8 fps and their WAVs; nothing is downloaded) and measures, at the train_MUSIC shape (2 sources, 3 frames, imgSize 224):

  (a) ds[i] on one CPU core, per item, in both modes;
  (b) dataset.to_device of a batch of --batch items in both modes: a host clock around a device synchronise, median after
      warm-up; the batch kernel alone between device events; the bytes each mode moves up;
  (c) mixtures/s of the DataLoader with 1, 4, 8 and 16 workers in both modes (to_device included; the batches queued while the
      workers start are drained before the clock runs), beside the step rates of the README (856 mixtures/s in fp32, 2 155 in
      bf16);
  (d) the single form (frames.prepare, the rows of tools/frames_bench.py) of this build and, with --parent-lib, of a library
      built from the parent commit's csrc/frames.hip, in alternating rounds in the same process: median, minimum and maximum
      of the rounds' medians for both.
Prints each figure as it is measured, writes --out (default profiles/loader_bench.json); the last line is one JSON object.
Usage: python tools/loader_bench.py [--batch 64] [--items 24] [--batches 4] [--workers 1,4,8,16] [--sections items,to_device,loader,single]
       [--parent-lib FILE] [--out FILE]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import avsep_amd as P  # noqa: E402
from avsep_amd import dataset as D  # noqa: E402
from avsep_amd import frames as F  # noqa: E402

H, W, FPS, RATE, SECS = 360, 640, 8.0, 11025, 12.0
STEP_RATES = {"fp32": 856.0, "bf16": 2155.0}           # README: mixtures/s of the train step


def write_dataset(root):
    """11 classes x 1 video: smooth seeded pictures (a JPEG of about 70 KB, as a filmed frame has) and a tone per class."""
    from PIL import Image
    from scipy.io import wavfile
    rs, rows = np.random.RandomState(0), []
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    for ci, cls in enumerate(D.MUSIC11_CLASSES):
        vid = f"{cls[:3]}00xyz"
        apath, fdir = os.path.join(root, "audio", cls, vid + ".wav"), os.path.join(root, "frames", cls, vid + ".mp4")
        os.makedirs(os.path.dirname(apath), exist_ok=True)
        os.makedirs(fdir, exist_ok=True)
        t = np.arange(int(SECS * RATE)) / RATE
        wavfile.write(apath, RATE, (0.4 * np.sin(2 * np.pi * 110.0 * (ci + 1) * t) * 32767).astype(np.int16))
        nf = int(SECS * FPS)
        for i in range(nf + 1):
            ph = rs.rand(3, 4) * 6.28
            img = np.stack([127 + 100 * np.sin(xx / (20 + 9 * c) + ph[c, 0] + i / 9) * np.cos(yy / (15 + 7 * c) + ph[c, 1]) for c in range(3)], 2)
            img += rs.randn(H, W, 3) * 12
            Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(os.path.join(fdir, f"{i:06d}.jpg"), quality=85)
        rows.append([apath, fdir, str(nf), str(FPS), str(SECS), cls])
    lst = os.path.join(root, "list.csv")
    with open(lst, "w") as f:
        f.write("\n".join(",".join(r) for r in rows) + "\n")
    size = os.path.getsize(os.path.join(fdir, "000000.jpg"))
    return lst, size


def loader_flags(repeat):
    a = P.arguments.train_music_args()
    a.one_frame, a.num_frames, a.stride_frames, a.margin = False, 3, 2, 1.0
    a.train_repeat = a.val_repeat = repeat
    return a


def sync_ms(fn, reps, warmup=2):
    out = []
    for r in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if r >= warmup:
            out.append((time.perf_counter() - t0) * 1e3)
    return out


def event_ms(fn, reps, warmup=3):
    out = []
    for r in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if r >= warmup:
            out.append(e0.elapsed_time(e1))
    return out


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)}


def item_rows(o, lst, a, result):
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        for mode, raw in (("classic", False), ("raw", True)):
            ds = D.MUSICMixDataset(lst, vars(a), split="train", raw_frames=raw)
            ds[0]
            t0 = time.perf_counter()
            for i in range(o.items):
                ds[i]
            result[f"item_ms_{mode}"] = (time.perf_counter() - t0) * 1e3 / o.items
            print(f"ds[i], {mode}: {result[f'item_ms_{mode}']:.2f} ms per item on one core ({o.items} items)", flush=True)
    finally:
        torch.set_num_threads(threads)


def to_device_rows(o, lst, a, dev, result):
    hosts = {}
    for mode, raw in (("classic", False), ("raw", True)):
        ds = D.MUSICMixDataset(lst, vars(a), split="train", raw_frames=raw)
        host = D.collate([ds[i % len(ds)] for i in range(o.batch)])
        hosts[mode] = {k: (v.pin_memory() if torch.is_tensor(v) else [t.pin_memory() for t in v] if k in ("audios", "frames") else v)
                       for k, v in host.items()}
        ms = sync_ms(lambda: D.to_device(hosts[mode], dev), o.reps)
        up = sum(t.numel() * t.element_size() for t in hosts[mode]["frames"]) if not raw else hosts[mode]["frames_u8"].numel()
        result[f"to_device_ms_{mode}"], result[f"frame_bytes_up_{mode}"] = spread(ms), up
        print(f"to_device, {mode}: {statistics.median(ms):.2f} ms for {o.batch} x 2 x 3 frames (min {min(ms):.2f}, max {max(ms):.2f}), "
              f"{up / 1e6:.1f} MB of frames up", flush=True)
    same = all(torch.equal(x, y) for x, y in zip(D.to_device(hosts["raw"], dev)["frames"], D.to_device(hosts["classic"], dev)["frames"]))
    result["raw_equals_classic"] = bool(same)
    b = hosts["raw"]
    N, B, T, _ = b["frame_shapes"].shape
    crops = [tuple(c) for c in b["frame_crops"].reshape(N * B, 2).tolist() for _ in range(T)]
    flips = [f for f in b["frame_flips"].reshape(-1).tolist() for _ in range(T)]
    t0 = time.perf_counter()
    plan = F.plan_batch(b["frame_shapes"].reshape(-1, 2).tolist(), 224, train=True, crops=crops, flips=flips, layout=(N * B, T))
    result["plan_batch_ms"] = (time.perf_counter() - t0) * 1e3
    px = b["frames_u8"].to(dev)
    ms = event_ms(lambda: F.prepare_batch(px, plan), o.reps)
    result["batch_kernel_ms"] = spread(ms)
    result["batch_kernel_us_per_frame"] = 1e3 * statistics.median(ms) / plan.n
    result["batch_launch"] = {"frames": plan.n, "grid_y": plan.launches[0][2], "lds_bytes": plan.launches[0][3]}
    print(f"prepare_batch alone: {statistics.median(ms):.3f} ms for {plan.n} frames = {result['batch_kernel_us_per_frame']:.2f} us per "
          f"frame (rows upload and output allocation included; LDS {plan.launches[0][3]} bytes); plan_batch {result['plan_batch_ms']:.2f} ms "
          f"on the host; raw == classic: {same}", flush=True)


def loader_rows(o, lst, a, dev, result):
    rows = {}
    for workers in o.workers:
        for mode, raw in (("classic", False), ("raw", True)):
            loader = D.make_loader([lst], a, "train", o.batch, True, workers=workers, raw_frames=raw)
            it = iter(loader)
            # the workers start together and keep two batches each in flight: what is queued by the time the first batches
            # are through says nothing of the rate, so those are drained first and the clock runs on what is produced after
            for _ in range(2 * workers + 1):
                D.to_device(next(it), dev)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            count = max(o.batches, 2 * workers)
            for _ in range(count):
                D.to_device(next(it), dev)
            torch.cuda.synchronize()
            rate = count * o.batch / (time.perf_counter() - t0)
            del it, loader
            rows[f"{mode}_{workers}"] = rate
            print(f"loader, {workers:2d} workers, {mode}: {rate:.0f} mixtures/s (the step takes {STEP_RATES['fp32']:.0f} in fp32, "
                  f"{STEP_RATES['bf16']:.0f} in bf16)", flush=True)
    result["loader_mixtures_per_s"] = rows
    result["step_mixtures_per_s"] = STEP_RATES


def single_form_rows(o, dev, result):
    """frames.prepare's launch through this build's library and through the parent's, alternating."""
    T = 1200
    g = torch.Generator(device=dev).manual_seed(0)
    stack = torch.randint(0, 256, (T, H, W, 3), dtype=torch.uint8, device=dev, generator=g)
    plan = F.plan(H, W, 224)
    hc, hb, vc, vb, lut = plan.on(dev)
    out = torch.empty(T, 3, 224, 224, device=dev)
    libs = {"child": P.lib.load()}
    if o.parent_lib:
        par = ctypes.CDLL(o.parent_lib)
        par.avsep_frames_prepare.restype, par.avsep_frames_prepare.argtypes = P.lib.SIGNATURES["avsep_frames_prepare"]
        libs["parent"] = par
    w, h = plan.size

    def launch(lib, n):
        rc = lib.avsep_frames_prepare(stack.data_ptr(), n, H, W, hc.data_ptr(), hb.data_ptr(), w, hc.shape[1], vc.data_ptr(), vb.data_ptr(),
                                      h, vc.shape[1], 224, plan.crop[0], plan.crop[1], 0, lut.data_ptr(), out.data_ptr(), None,
                                      P.lib.stream())
        assert rc == 0
    res = {}
    for name, n in (("whole_stack", T), ("trunk_batch", 16)):
        meds = {k: [] for k in libs}
        for _ in range(o.rounds):
            for k, lib in libs.items():
                meds[k].append(statistics.median(event_ms(lambda: launch(lib, n), o.reps)))
        res[name] = {k: dict(spread(v), us_per_frame=1e3 * statistics.median(v) / n) for k, v in meds.items()}
        print(f"single form, {name} ({n} frames): " + "; ".join(
            f"{k} {1e3 * statistics.median(v) / n:.3f} us per frame (rounds {1e3 * min(v) / n:.3f} ... {1e3 * max(v) / n:.3f})"
            for k, v in meds.items()), flush=True)
    result["single_form"] = res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--items", type=int, default=24)
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--workers", type=lambda s: [int(v) for v in s.split(",")], default=[1, 4, 8, 16])
    ap.add_argument("--sections", type=lambda v: v.split(","), default=["items", "to_device", "loader", "single"])
    ap.add_argument("--parent-lib", default=None, help="a shared library with the parent commit's avsep_frames_prepare")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loader_bench.json"))
    o = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loader_bench measures on an MI355X; there is nothing to report without one")
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    result = {"batch": o.batch, "num_mix": 2, "num_frames": 3, "frame": [H, W], "img_size": 224}
    with tempfile.TemporaryDirectory() as root:
        lst, size = write_dataset(root)
        result["jpeg_bytes"] = size
        a = loader_flags(repeat=max(1, (4 * max(o.workers) + o.batches + 2) * o.batch // 11 + 1))
        if "items" in o.sections:
            item_rows(o, lst, a, result)
        if "to_device" in o.sections:
            to_device_rows(o, lst, a, dev, result)
        if "loader" in o.sections:
            loader_rows(o, lst, a, dev, result)
    if "single" in o.sections:
        single_form_rows(o, dev, result)
    result["command"] = "python tools/loader_bench.py"
    os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
    with open(o.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
