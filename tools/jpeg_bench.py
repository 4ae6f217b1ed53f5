"""The GPU JPEG decoder (csrc/jpeg.hip, avsep_amd/jpeg.py) on cuda:0, beside Pillow on one core.  The files are made here with
Pillow from seeded synthetic pictures (nothing is downloaded): 360 x 640, 4:2:0, quality 75, without restart intervals, as ffmpeg
writes the MUSIC frames.

  (a) one loader batch, --files (384) files in one plan: jpeg.plan on the host, the upload of bytes, rows and tables, the entropy
      stage and the pixel stage, each between device events (median of --reps after warm-up), per batch and per frame; the
      result checked against Pillow on --check files;
  (b) Pillow (Image.open(..).convert("RGB")) on one CPU core over --cpu-files of the same files, per file;
  (c) one clip, --clip (4 800) files (the batch's files repeated in order): jpeg.decode end to end (plan, upload, every chunk, the
      status read), a host clock around a device synchronise;
  (d) the loader at the train_MUSIC shape (tools/loader_bench.py's dataset): ds[i] on one core, to_device of a batch and the
      one-worker loader rate, for --gpu_frames alone (the parent commit's path, unchanged) and with --gpu_decode, in the same run.
Prints each figure as it is measured and writes --out (default profiles/jpeg_bench.json); the last line is one JSON object.
  --progressive: (a) and, over the same pictures saved with progressive=True: the entropy stage level by level and in
      all, the bound check, the pixel stage, jpeg.plan, jpeg.decode end to end, Pillow on one core on the progressive files, and
      the stages of ONE file alone (its serial part); written to profiles/jpeg_progressive_bench.json.
Usage: python tools/jpeg_bench.py [--files 384] [--clip 4800] [--reps 10] [--sections batch,pillow,clip,loader] [--progressive]
       [--out FILE]"""
import argparse
import io
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
import avsep_amd as P  # noqa: E402,F401
from avsep_amd import dataset as D  # noqa: E402
from avsep_amd import jpeg  # noqa: E402
from avsep_amd import kernels as K  # noqa: E402
from loader_bench import event_ms, loader_flags, spread, sync_ms, write_dataset  # noqa: E402

H, W = 360, 640


def make_files(n, **form):
    """n seeded pictures with smooth structure and grain, as JPEG bytes (form: further arguments of Pillow's save)."""
    from PIL import Image
    rs, out = np.random.RandomState(0), []
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    for i in range(n):
        ph = rs.rand(3, 2) * 6.28
        img = np.stack([127 + 100 * np.sin(xx / (20 + 9 * c) + ph[c, 0] + i / 9) * np.cos(yy / (15 + 7 * c) + ph[c, 1]) for c in range(3)], 2)
        img += rs.randn(H, W, 3) * 12
        b = io.BytesIO()
        Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(b, "JPEG", quality=75, subsampling=2, **form)
        out.append(b.getvalue())
    return out


def pillow(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"), dtype=np.uint8)


def batch_rows(o, dev, files, result):
    t0 = time.perf_counter()
    p = jpeg.plan(files)
    plan_ms = (time.perf_counter() - t0) * 1e3
    n = len(p.images)
    assert not p.fallback and n == len(files)
    host = [torch.from_numpy(p.bytes).pin_memory(), torch.from_numpy(p.tables).pin_memory(),
            torch.from_numpy(p.images.view(np.uint8)).pin_memory()] + [torch.from_numpy(ch.segs.view(np.uint8)).pin_memory() for ch in p.chunks]
    up = event_ms(lambda: [t.to(dev, non_blocking=True) for t in host], o.reps)
    data, tables, images, *segs = [t.to(dev) for t in host]
    blocks = max(ch.blocks for ch in p.chunks)
    coef = torch.empty(blocks * 64, dtype=torch.int16, device=dev)
    planes = torch.empty(blocks * 64, dtype=torch.uint8, device=dev)
    pixels = torch.empty(p.pixel_bytes, dtype=torch.uint8, device=dev)
    status = torch.zeros(n, dtype=torch.int32, device=dev)
    size = jpeg.IMAGE.itemsize

    def entropy():
        for ch, sg in zip(p.chunks, segs):
            K.jpeg_entropy(data, images[ch.a * size:ch.b * size], sg, tables, coef, ch.blocks, status[ch.a:ch.b])

    def both():
        for ch, sg in zip(p.chunks, segs):
            rows, st = images[ch.a * size:ch.b * size], status[ch.a:ch.b]
            K.jpeg_entropy(data, rows, sg, tables, coef, ch.blocks, st)
            K.jpeg_pixels(coef, planes, ch.blocks, rows, ch.max_blocks, ch.max_pixels, tables, st, pixels)

    ent_ms = event_ms(entropy, o.reps, warmup=1)
    ent = statistics.median(ent_ms)
    tot = statistics.median(event_ms(both, o.reps, warmup=1))
    both()
    torch.cuda.synchronize()
    assert not status.any().item()
    got = pixels.cpu().numpy()
    same = all(np.array_equal(got[int(p.offsets[i]):int(p.offsets[i + 1])].reshape(H, W, 3), pillow(files[i])) for i in range(min(o.check, n)))
    result["batch"] = {
        "files": n, "chunks": len(p.chunks), "file_bytes_mean": sum(map(len, files)) / n, "entropy_bytes": int(len(p.bytes)),
        "decoded_bytes": p.pixel_bytes, "workspace_bytes": blocks * 192, "plan_ms": plan_ms, "upload_ms": spread(up),
        "entropy_ms": ent, "entropy_ms_spread": spread(ent_ms), "entropy_us_per_frame": 1e3 * ent / n, "entropy_and_pixels_ms": tot, "pixels_ms": tot - ent,
        "pixels_us_per_frame": 1e3 * (tot - ent) / n, "equals_pillow": bool(same), "checked": min(o.check, n)}
    r = result["batch"]
    print(f"batch of {n} files ({r['file_bytes_mean'] / 1e3:.1f} KB each, {r['entropy_bytes'] / 1e6:.1f} MB up for {p.pixel_bytes / 1e6:.0f} MB "
          f"decoded, {len(p.chunks)} chunk(s)): plan {plan_ms:.1f} ms on the host, upload {statistics.median(up):.2f} ms, entropy stage "
          f"{ent:.2f} ms = {r['entropy_us_per_frame']:.0f} us per frame, pixel stage {r['pixels_ms']:.2f} ms = "
          f"{r['pixels_us_per_frame']:.1f} us per frame (both stages {tot:.2f} ms, the difference); equal to Pillow on {r['checked']} files: "
          f"{same}", flush=True)


def scan_stage(p, dev):
    """The device buffers of a one-chunk progressive plan and one launcher per step of its entropy stage -> (steps, buffers):
    steps = [(name, fn)]: every level (the first one zeroes the workspace), the bound check, the pixel stage."""
    ch = p.chunks[0]
    assert len(p.chunks) == 1 and not len(ch.segs)
    data, tables, images, scans = (torch.from_numpy(a).to(dev) for a in (p.bytes, p.tables, p.images.view(np.uint8), ch.scans.view(np.uint8)))
    coef = torch.empty(ch.blocks * 64, dtype=torch.int16, device=dev)
    planes = torch.empty(ch.blocks * 64, dtype=torch.uint8, device=dev)
    pixels = torch.empty(p.pixel_bytes, dtype=torch.uint8, device=dev)
    status = torch.zeros(len(p.images), dtype=torch.int32, device=dev)
    size = jpeg.SCAN.itemsize
    steps = [(f"level_{level}", lambda level=level, a=a, b=b: K.jpeg_scans(data, images, scans[a * size:b * size], level, a == 0, tables,
                                                                            coef, ch.blocks, status)) for level, a, b in ch.levels]
    steps.append(("bound", lambda: K.jpeg_coef_bound(coef, ch.blocks, images, ch.max_blocks, tables, status)))
    steps.append(("pixels", lambda: K.jpeg_pixels(coef, planes, ch.blocks, images, ch.max_blocks, ch.max_pixels, tables, status, pixels)))
    return steps, (pixels, status)


def sequence_ms(steps, status, reps):
    """The steps in their order, an event between each two (a level only means something after the levels before it) ->
    {name: median ms}, "entropy": everything before the pixel stage."""
    runs = []
    for r in range(1 + reps):
        status.zero_()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(steps) + 1)]
        torch.cuda.synchronize()
        ev[0].record()
        for k, (_, fn) in enumerate(steps):
            fn()
            ev[k + 1].record()
        torch.cuda.synchronize()
        if r:
            runs.append([ev[k].elapsed_time(ev[k + 1]) for k in range(len(steps))] + [ev[0].elapsed_time(ev[len(steps) - 1])])
    return {name: statistics.median(v) for name, v in zip([n for n, _ in steps] + ["entropy"], zip(*runs))}


def progressive_rows(o, dev, files, result):
    """The same pictures saved progressive, beside the baseline rows of this run: the entropy stage level by level and in
    all, the pixel stage, jpeg.plan on the host, jpeg.decode end to end, Pillow on one core on the PROGRESSIVE files, and the
    serial part of ONE file (a plan of one file: one lane baseline, one lane per scan and level progressive)."""
    prog = make_files(len(files), progressive=True)
    t0 = time.perf_counter()
    p = jpeg.plan(prog, progressive=True)
    plan_ms = (time.perf_counter() - t0) * 1e3
    n = len(p.images)
    assert not p.fallback and n == len(prog)
    steps, (pixels, status) = scan_stage(p, dev)
    for _, fn in steps:
        fn()
    torch.cuda.synchronize()
    assert not status.any().item()
    got = pixels.cpu().numpy()
    same = all(np.array_equal(got[int(p.offsets[i]):int(p.offsets[i + 1])].reshape(H, W, 3), pillow(prog[i])) for i in range(min(o.check, n)))
    row = {"files": n, "file_bytes_mean": sum(map(len, prog)) / n, "scan_rows": int(len(p.chunks[0].scans)), "plan_ms": plan_ms,
           "equals_pillow": bool(same), "checked": min(o.check, n)}
    row.update({f"{name}_ms": ms for name, ms in sequence_ms(steps, status, o.reps).items()})
    row["entropy_us_per_frame"] = 1e3 * row["entropy_ms"] / n
    row["decode_ms"] = statistics.median(sync_ms(lambda: jpeg.decode(prog, dev, progressive=True), o.reps, warmup=1))
    row["decode_ms_baseline"] = statistics.median(sync_ms(lambda: jpeg.decode(files, dev), o.reps, warmup=1))
    t0 = time.perf_counter()
    jpeg.plan(files)
    row["plan_ms_baseline"] = (time.perf_counter() - t0) * 1e3
    threads, m = torch.get_num_threads(), min(o.cpu_files, n)
    torch.set_num_threads(1)
    try:
        for name, fs in (("pillow_ms_per_file", prog), ("pillow_ms_per_file_baseline", files)):
            pillow(fs[0])
            t0 = time.perf_counter()
            for f in fs[:m]:
                pillow(f)
            row[name] = (time.perf_counter() - t0) * 1e3 / m
    finally:
        torch.set_num_threads(threads)
    # one file alone: what a file's slowest chain of lanes costs
    one, (_, status1) = scan_stage(jpeg.plan(prog[:1], progressive=True), dev)
    row["one_file"] = sequence_ms(one, status1, o.reps)
    q = jpeg.plan(files[:1])
    d1, t1, i1, s1 = (torch.from_numpy(a).to(dev) for a in (q.bytes, q.tables, q.images.view(np.uint8), q.chunks[0].segs.view(np.uint8)))
    c1, st1 = torch.empty(q.chunks[0].blocks * 64, dtype=torch.int16, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    row["one_file"]["baseline_entropy"] = statistics.median(event_ms(lambda: K.jpeg_entropy(d1, i1, s1, t1, c1, q.chunks[0].blocks, st1),
                                                                      o.reps, warmup=1))
    result["progressive"] = row
    print("progressive: " + json.dumps(row), flush=True)


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
    jpeg.decode(clip[:len(files)], dev)
    ms = sync_ms(lambda: jpeg.decode(clip, dev), 2, warmup=0)
    chunks = len(jpeg.plan(clip).chunks)
    result["clip"] = {"files": o.clip, "chunks": chunks, "decode_ms": spread(ms), "ms_per_frame": statistics.median(ms) / o.clip}
    print(f"clip of {o.clip} files, jpeg.decode end to end (plan, upload, {chunks} chunks, status read): {statistics.median(ms):.0f} ms = "
          f"{statistics.median(ms) / o.clip:.3f} ms per frame", flush=True)


def loader_rows(o, dev, result):
    rows = {}
    with tempfile.TemporaryDirectory() as root:
        lst, _ = write_dataset(root)
        a = loader_flags(repeat=max(1, (8 + o.batches) * o.batch // 11 + 1))
        modes = (("gpu_frames", {}), ("gpu_frames_gpu_decode", {"jpeg_bytes": True}))
        threads = torch.get_num_threads()
        torch.set_num_threads(1)
        try:
            for mode, kw in modes:
                ds = D.MUSICMixDataset(lst, vars(a), split="train", raw_frames=True, **kw)
                ds[0]
                t0 = time.perf_counter()
                for i in range(o.items):
                    ds[i]
                rows[f"item_ms_{mode}"] = (time.perf_counter() - t0) * 1e3 / o.items
                print(f"ds[i], {mode}: {rows[f'item_ms_{mode}']:.2f} ms per item on one core ({o.items} items)", flush=True)
        finally:
            torch.set_num_threads(threads)
        outs = {}
        for mode, kw in modes:
            ds = D.MUSICMixDataset(lst, vars(a), split="train", raw_frames=True, **kw)
            host = D.collate([ds[i % len(ds)] for i in range(o.batch)])
            host = {k: (v.pin_memory() if torch.is_tensor(v) and v.numel() else v) for k, v in host.items()}
            ms = sync_ms(lambda: D.to_device(host, dev), o.reps)
            key = "frames_jpeg" if kw else "frames_u8"
            rows[f"to_device_ms_{mode}"], rows[f"frame_bytes_up_{mode}"] = spread(ms), host[key].numel()
            outs[mode] = D.to_device(host, dev)["frames"]
            print(f"to_device, {mode}: {statistics.median(ms):.2f} ms for {o.batch} x 2 x 3 frames, {host[key].numel() / 1e6:.1f} MB of frames "
                  f"up", flush=True)
        rows["batches_equal"] = all(torch.equal(x, y) for x, y in zip(*outs.values()))
        for mode, kw in modes:
            loader = D.make_loader([lst], a, "train", o.batch, True, workers=1, raw_frames=True, **kw)
            it = iter(loader)
            for _ in range(3):
                D.to_device(next(it), dev)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(o.batches):
                D.to_device(next(it), dev)
            torch.cuda.synchronize()
            rows[f"loader_1_worker_mixtures_per_s_{mode}"] = o.batches * o.batch / (time.perf_counter() - t0)
            del it, loader
            print(f"loader, 1 worker, {mode}: {rows[f'loader_1_worker_mixtures_per_s_{mode}']:.0f} mixtures/s", flush=True)
    result["loader"] = rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=384)
    ap.add_argument("--clip", type=int, default=4800)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--check", type=int, default=16)
    ap.add_argument("--cpu-files", type=int, default=96)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--items", type=int, default=24)
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--sections", type=lambda v: v.split(","), default=["batch", "pillow", "clip", "loader"])
    ap.add_argument("--progressive", action="store_true",
                    help="the pass over the same pictures saved progressive, beside the baseline batch rows (writes "
                         "profiles/jpeg_progressive_bench.json unless --out is given)")
    ap.add_argument("--out", default=None)
    o = ap.parse_args()
    if o.progressive:
        o.sections = ["batch", "progressive"]
    o.out = o.out or os.path.join(ROOT, "profiles", "jpeg_progressive_bench.json" if o.progressive else "jpeg_bench.json")
    if not torch.cuda.is_available():
        raise SystemExit("jpeg_bench measures on an MI355X; there is nothing to report without one")
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    result = {"frame": [H, W], "quality": 75, "sampling": "4:2:0", "reps": o.reps}
    files = make_files(o.files)
    if "batch" in o.sections:
        batch_rows(o, dev, files, result)
    if "progressive" in o.sections:
        progressive_rows(o, dev, files, result)
    if "pillow" in o.sections:
        pillow_row(o, files, result)
    if "clip" in o.sections:
        clip_row(o, dev, files, result)
    if "loader" in o.sections:
        loader_rows(o, dev, result)
    result["command"] = "python tools/jpeg_bench.py" + (" --progressive" if o.progressive else "")
    os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
    with open(o.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
