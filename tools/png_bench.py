"""The GPU PNG decoder (csrc/png.hip, avsep_amd/png.py) on cuda:0, beside Pillow on one core.  The files are made here with
Pillow from seeded synthetic pictures (nothing is downloaded): 360 x 640 RGB, Pillow's default compression and filters.

  (a) one loader-sized batch, --files (384) files in one plan: png.plan on the host, the upload of streams, rows and palettes,
      and the inflate, unfilter and colour stages, each between device events (median of --reps after warm-up), per batch and
      per frame; the result checked against Pillow on --check files;
  (b) Pillow (Image.open(..).convert("RGB")) on one CPU core over --cpu-files of the same files, per file;
  (c) one clip, --clip (4 800) files (the batch's files repeated in order): png.decode end to end (plan, upload, every chunk, the
      status read), a host clock around a device synchronise;
  (d) the share of a `separate --fps --gpu_decode` run: two such clips decoded, against the ten-minute run of
      tools/frames_bench.py (its recorded wall time in profiles/frames_bench.json, frames already in memory there).
Prints each figure as it is measured and writes --out (default profiles/png_bench.json); the last line is one JSON object.
Usage: python tools/png_bench.py [--files 384] [--clip 4800] [--reps 5] [--out FILE]"""
import argparse
import io
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import avsep_amd as P  # noqa: E402,F401
from avsep_amd import kernels as K  # noqa: E402
from avsep_amd import png  # noqa: E402
from loader_bench import event_ms, spread, sync_ms  # noqa: E402

H, W = 360, 640
GRAIN = 0.3                          # standard deviation of the noise on the pictures, grey levels


def make_file(i):
    """Picture i, seeded: smooth structure and a little grain, as PNG bytes."""
    from PIL import Image
    rs = np.random.RandomState(i)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    ph = rs.rand(3, 2) * 6.28
    img = np.stack([127 + 100 * np.sin(xx / (20 + 9 * c) + ph[c, 0] + i / 9) * np.cos(yy / (15 + 7 * c) + ph[c, 1]) for c in range(3)], 2)
    img += rs.randn(H, W, 3) * GRAIN
    b = io.BytesIO()
    Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(b, "PNG")
    return b.getvalue()


def make_files(n, workers=16):
    """n such files, made by a pool of host processes (before this process opens the GPU)."""
    from concurrent.futures import ProcessPoolExecutor
    with ProcessPoolExecutor(max_workers=workers) as pool:
        return list(pool.map(make_file, range(n), chunksize=4))


def pillow(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"), dtype=np.uint8)


def batch_rows(o, dev, files, result):
    t0 = time.perf_counter()
    p = png.plan(files)
    plan_ms = (time.perf_counter() - t0) * 1e3
    n = len(p.images)
    assert not p.fallback and n == len(files) and len(p.chunks) == 1
    ch = p.chunks[0]
    host = [torch.from_numpy(p.bytes).pin_memory(), torch.from_numpy(p.images.view(np.uint8)).pin_memory()]
    up = event_ms(lambda: [t.to(dev, non_blocking=True) for t in host], o.reps)
    data, images = [t.to(dev) for t in host]
    tables = torch.zeros(1, dtype=torch.uint8, device=dev)
    ws = torch.empty(ch.ws_bytes, dtype=torch.uint8, device=dev)
    pixels = torch.empty(p.pixel_bytes, dtype=torch.uint8, device=dev)
    status = torch.zeros(n, dtype=torch.int32, device=dev)
    # the stages in their order, an event between each two: unfiltering works in place, so a stage means something only after
    # the one before it
    runs = []
    for r in range(1 + o.reps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        torch.cuda.synchronize()
        ev[0].record()
        K.png_inflate(data, images, ws, ch.ws_bytes, status)
        ev[1].record()
        K.png_pixels(ws, ch.ws_bytes, images, ch.max_pixels, tables, status, pixels, stages=1)
        ev[2].record()
        K.png_pixels(ws, ch.ws_bytes, images, ch.max_pixels, tables, status, pixels, stages=2)
        ev[3].record()
        torch.cuda.synchronize()
        if r:
            runs.append([ev[k].elapsed_time(ev[k + 1]) for k in range(3)])
    inflate, unfilter, colour = (list(v) for v in zip(*runs))
    assert not status.any().item(), status.cpu().numpy()[:8]
    got = pixels.cpu().numpy()
    same = all(np.array_equal(got[int(p.offsets[i]):int(p.offsets[i + 1])].reshape(H, W, 3), pillow(files[i])) for i in range(min(o.check, n)))
    med = statistics.median
    result["batch"] = {
        "files": n, "file_bytes_mean": sum(map(len, files)) / n, "stream_bytes": int(len(p.bytes)), "scanline_bytes": ch.ws_bytes,
        "decoded_bytes": p.pixel_bytes, "plan_ms": plan_ms, "upload_ms": spread(up), "inflate_ms": spread(inflate),
        "unfilter_ms": spread(unfilter), "colour_ms": spread(colour), "inflate_us_per_frame": 1e3 * med(inflate) / n,
        "unfilter_us_per_frame": 1e3 * med(unfilter) / n, "colour_us_per_frame": 1e3 * med(colour) / n,
        "stages_ms_per_frame": (med(inflate) + med(unfilter) + med(colour)) / n, "equals_pillow": bool(same), "checked": min(o.check, n)}
    r = result["batch"]
    print(f"batch of {n} files ({r['file_bytes_mean'] / 1e3:.1f} KB each, {r['stream_bytes'] / 1e6:.1f} MB up for {p.pixel_bytes / 1e6:.0f} MB "
          f"decoded): plan {plan_ms:.1f} ms on the host, upload {med(up):.2f} ms, inflate {med(inflate):.2f} ms = "
          f"{r['inflate_us_per_frame']:.0f} us per frame, unfilter {med(unfilter):.2f} ms = {r['unfilter_us_per_frame']:.0f} us per frame, "
          f"colour {med(colour):.2f} ms = {r['colour_us_per_frame']:.1f} us per frame; equal to Pillow on {r['checked']} files: {same}", flush=True)
    # one file alone: what the serial part of a file costs
    q = png.plan(files[:1])
    d1, i1 = torch.from_numpy(q.bytes).to(dev), torch.from_numpy(q.images.view(np.uint8)).to(dev)
    st1 = torch.zeros(1, dtype=torch.int32, device=dev)
    one = event_ms(lambda: K.png_inflate(d1, i1, ws, q.chunks[0].ws_bytes, st1), o.reps, warmup=1)
    result["one_file_inflate_ms"] = spread(one)
    print(f"one file alone, inflate: {med(one):.2f} ms", flush=True)


def pillow_row(o, files, result):
    n = min(o.cpu_files, len(files))
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        pillow(files[0])
        t0 = time.perf_counter()
        for f in files[:n]:
            pillow(f)
        ms = (time.perf_counter() - t0) * 1e3
    finally:
        torch.set_num_threads(threads)
    result["pillow_one_core"] = {"files": n, "ms_per_file": ms / n}
    print(f"Pillow on one core: {ms / n:.2f} ms per file over {n} files", flush=True)


def clip_row(o, dev, files, result):
    clip = [files[i % len(files)] for i in range(o.clip)]
    png.decode(clip[:len(files)], dev)
    ms = sync_ms(lambda: png.decode(clip, dev), 2, warmup=0)
    t0 = time.perf_counter()
    chunks = len(png.plan(clip).chunks)
    plan_ms = (time.perf_counter() - t0) * 1e3
    med = statistics.median(ms)
    result["clip"] = {"files": o.clip, "chunks": chunks, "decode_ms": spread(ms), "ms_per_frame": med / o.clip, "plan_ms": plan_ms}
    print(f"clip of {o.clip} files, png.decode end to end (plan {plan_ms:.0f} ms, upload, {chunks} chunks, status read): {med:.0f} ms = "
          f"{med / o.clip:.3f} ms per frame", flush=True)
    recorded = os.path.join(ROOT, "profiles", "frames_bench.json")
    if os.path.exists(recorded):
        run = json.load(open(recorded))["separate_fps"]["uint8_stacks_synchronised_ms"]
        pil = result.get("pillow_one_core", {}).get("ms_per_file")
        result["separate_fps"] = {"recorded_run_ms": run, "two_clips_decode_ms": 2 * med, "share_gpu_decode": 2 * med / (2 * med + run)}
        if pil is not None:
            result["separate_fps"].update(two_clips_pillow_ms=2 * o.clip * pil, share_pillow=2 * o.clip * pil / (2 * o.clip * pil + run))
        print("separate --fps, two clips: " + json.dumps(result["separate_fps"]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=384)
    ap.add_argument("--clip", type=int, default=4800)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--check", type=int, default=16)
    ap.add_argument("--cpu-files", type=int, default=96)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png_bench.json"))
    o = ap.parse_args()
    files = make_files(o.files)                     # first: the pool forks, and a forked child must not inherit an open GPU
    if not torch.cuda.is_available():
        raise SystemExit("png_bench measures on an MI355X; there is nothing to report without one")
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    result = {"frame": [H, W], "colour": "RGB", "grain": GRAIN, "reps": o.reps}
    batch_rows(o, dev, files, result)
    pillow_row(o, files, result)
    clip_row(o, dev, files, result)
    result["command"] = "python tools/png_bench.py"
    os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
    with open(o.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
