"""The GPU JPEG encoder (csrc/jpeg_enc.hip, avsep_amd/jpeg.py: encode) on cuda:0, beside Pillow on one core on the same pixels.
The pictures are seeded synthetic ones (nothing is downloaded): smooth structure with grain, as spectrogram and overlay images have.

  (a) a validation batch's images, --images (192) of 512 x 256 x 3 at Pillow's defaults (quality 75, 4:2:0) in one plan: the four
      stages (coefficients, count, pack, stuff) each between device events (median of --reps after warm-up), jpeg.encode end to
      end (plan, launches, the two size reads, the copy of the files to the host) under a host clock around a device synchronise,
      and the files checked against Pillow's on --check of them;
  (b) a clip's overlays, --frames (4 800) of 224 x 224 x 3 at quality 90, through jpeg.encode in chunks of localise.JPG_CHUNK as
      `localise --jpg` does, end to end; the stages of one chunk between device events;
  (c) Pillow (Image.fromarray(a).save(f, "JPEG", ...)) on one CPU core over --cpu-files of the same pictures, per file, both shapes;
  (d) visuals.output_visuals on one validation batch of 8 items at the shipped shapes with and without args.gpu_encode, the two
      alternating in one run (without the flag is the parent commit's path, unchanged).
Prints each figure as it is measured and writes --out (default profiles/jpeg_encode_bench.json); the last line is one JSON object.
Usage: python tools/jpeg_encode_bench.py [--images 192] [--frames 4800] [--reps 10] [--sections batch,clip,pillow,visuals] [--out FILE]"""
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
import avsep_amd as P  # noqa: E402
from avsep_amd import jpeg  # noqa: E402
from avsep_amd import kernels as K  # noqa: E402
from avsep_amd import localise as L  # noqa: E402
from avsep_amd import visuals as V  # noqa: E402
from loader_bench import event_ms, spread, sync_ms  # noqa: E402


def pictures(n, H, W, dev, seed=0):
    """n seeded pictures -> uint8 [n,H,W,3] on the device (made there: they are only the encoder's input)."""
    g = torch.Generator(device=dev).manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    ph = torch.rand(n, 3, 2, generator=g, device=dev) * 6.28
    c = torch.arange(3, device=dev, dtype=torch.float32).view(1, 3, 1, 1)
    img = 127 + 100 * torch.sin(xx / (20 + 9 * c) + ph[:, :, 0, None, None]) * torch.cos(yy / (15 + 7 * c) + ph[:, :, 1, None, None])
    img += torch.randn(n, 3, H, W, generator=g, device=dev) * 12
    return img.clamp_(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def pillow_file(a, **kw):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(a).save(b, "JPEG", **kw)
    return b.getvalue()


def stage_rows(stack, reps, **kw):
    """The four stages of one chunk of ``stack`` [n,H,W,3] between device events -> dict."""
    dev = stack.device
    p = jpeg.encode_plan([tuple(stack.shape[1:])] * stack.shape[0], **kw)
    ch = p.chunks[0]
    n = ch.b - ch.a
    pixels = stack.reshape(-1)[:int(p.offsets[ch.b])]
    rows = torch.from_numpy(np.ascontiguousarray(ch.images).view(np.uint8)).to(dev)
    tables = torch.from_numpy(p.tables).to(dev)
    B, I = ch.blocks, ch.intervals
    i64 = lambda m: torch.empty(m, dtype=torch.int64, device=dev)      # noqa: E731
    i32 = lambda m: torch.empty(m, dtype=torch.int32, device=dev)      # noqa: E731
    coef, bits, pos = torch.empty(B * 64, dtype=torch.int16, device=dev), i32(B), i64(B + 1)
    ivl_bytes, ivl_off, out_off, ff0, ivl_out, tiles = i32(I), i64(I + 1), i64(I + 1), i64(I), i32(I), i64(-(-B // 256))
    coef_f = lambda: K.jpeg_enc_coef(pixels, rows, tables, coef, B)                                              # noqa: E731
    count_f = lambda: K.jpeg_enc_count(coef, B, rows, I, tables, bits, pos, ivl_bytes, ivl_off, tiles)            # noqa: E731
    out = {"images": n, "blocks": B, "intervals": I, "pixel_bytes": int(pixels.numel())}
    out["coef_ms"] = spread(event_ms(coef_f, reps))
    out["count_ms"] = spread(event_ms(count_f, reps))
    nbytes = max(4, -(-int(ivl_off[I].item()) // 4) * 4)
    stream, groups = torch.empty(nbytes, dtype=torch.uint8, device=dev), -(-nbytes // 64)
    grp, ffpos = i32(groups), i64(groups + 1)
    pack_f = lambda: K.jpeg_enc_pack(coef, B, rows, I, tables, pos, ivl_off, stream, grp, ffpos, ff0, ivl_out, out_off, tiles)   # noqa: E731
    out["pack_ms"] = spread(event_ms(pack_f, reps))
    data, sizes = torch.empty(int(out_off[I].item()), dtype=torch.uint8, device=dev), i64(2 * n)
    stuff_f = lambda: K.jpeg_enc_stuff(stream, rows, I, ivl_off, ffpos, ff0, out_off, data, sizes)                # noqa: E731
    out["stuff_ms"] = spread(event_ms(stuff_f, reps))
    out["unstuffed_bytes"], out["encoded_bytes"] = nbytes, int(data.numel())
    out["stages_ms"] = sum(out[k]["median"] for k in ("coef_ms", "count_ms", "pack_ms", "stuff_ms"))
    return out


def batch_section(o, dev, result):
    stack = pictures(o.images, 512, 256, dev)
    r = stage_rows(stack, o.reps)
    whole = sync_ms(lambda: jpeg.encode(stack), o.reps)
    files = jpeg.encode(stack)
    host = stack[:o.check].cpu().numpy()
    r["encode_ms"], r["us_per_image"] = spread(whole), 1e3 * statistics.median(whole) / o.images
    r["equals_pillow"], r["checked"] = all(f == pillow_file(a) for f, a in zip(files, host)), len(host)
    result["batch"] = r
    print(f"batch of {o.images} images of 512 x 256 x 3 ({r['pixel_bytes'] / 1e6:.0f} MB in, {r['encoded_bytes'] / 1e6:.1f} MB out): "
          + ", ".join(f"{k[:-3]} {r[k]['median']:.3f} ms" for k in ("coef_ms", "count_ms", "pack_ms", "stuff_ms"))
          + f" (stages {r['stages_ms']:.3f} ms); jpeg.encode end to end {statistics.median(whole):.2f} ms = {r['us_per_image']:.1f} us per "
          f"image; equal to Pillow on {r['checked']} files: {r['equals_pillow']}", flush=True)


def clip_section(o, dev, result):
    stack = pictures(min(o.frames, L.JPG_CHUNK), 224, 224, dev, seed=1)
    r = stage_rows(stack, o.reps, quality=90)

    def clip():
        for t0 in range(0, o.frames, L.JPG_CHUNK):
            jpeg.encode(stack[:min(L.JPG_CHUNK, o.frames - t0)], quality=90)
    whole = sync_ms(clip, 3, warmup=1)
    files = jpeg.encode(stack[:o.check], quality=90)
    r["frames"], r["encode_ms"], r["us_per_frame"] = o.frames, spread(whole), 1e3 * statistics.median(whole) / o.frames
    r["equals_pillow"] = all(f == pillow_file(a, quality=90) for f, a in zip(files, stack[:o.check].cpu().numpy()))
    result["clip"] = r
    print(f"clip of {o.frames} frames of 224 x 224 x 3, quality 90, chunks of {L.JPG_CHUNK}: one chunk's stages "
          + ", ".join(f"{k[:-3]} {r[k]['median']:.3f} ms" for k in ("coef_ms", "count_ms", "pack_ms", "stuff_ms"))
          + f"; jpeg.encode end to end {statistics.median(whole):.0f} ms = {r['us_per_frame']:.1f} us per frame; equal to Pillow: "
          f"{r['equals_pillow']}", flush=True)


def pillow_section(o, dev, result):
    rows = {}
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        for name, (H, W), kw, seed in (("batch", (512, 256), {}, 0), ("clip", (224, 224), {"quality": 90}, 1)):
            host = pictures(o.cpu_files, H, W, dev, seed).cpu().numpy()
            pillow_file(host[0], **kw)
            t0 = time.perf_counter()
            for a in host:
                pillow_file(a, **kw)
            rows[name] = {"files": len(host), "ms_per_file": (time.perf_counter() - t0) * 1e3 / len(host)}
            print(f"Pillow on one core, {H} x {W} x 3 {kw or 'defaults'}: {rows[name]['ms_per_file']:.3f} ms per file over {len(host)} files",
                  flush=True)
    finally:
        torch.set_num_threads(threads)
    result["pillow_one_core"] = rows


def visuals_section(o, dev, result):
    argv = ("--arch_sound unet7 --arch_frame resnet18dilated --img_pool maxpool --num_channels 2 --img_activation relu "
            "--output_activation sigmoid --vis_channels 256 --fusion_type hidsep --not_pool_vis --att_type sig --binary_mask 1 "
            "--loss bce --weighted_loss 1 --num_mix 2 --log_freq 1 --num_frames 3 --imgSize 224 --audLen 65535 --num_vis 8").split()
    args = P.ArgParser().parse_train_arguments(argv, verbose=False)
    torch.manual_seed(0)
    mb = P.ModelBuilder()
    snd = mb.build_sound(arch=args.arch_sound, fc_dim=args.num_channels, fusion_type=args.fusion_type, att_type=args.att_type)
    frm = mb.build_frame(arch=args.arch_frame, fc_dim=args.vis_channels, pool_type=args.img_pool)
    wrap = P.NetWrapper((snd.to(dev), frm.to(dev)), mb.build_criterion(arch=args.loss, use_pit=True), mb.build_criterion(arch=args.loss))
    wrap.eval()
    B = 8
    g = torch.Generator().manual_seed(1)
    audios = [(torch.rand(B, args.audLen, generator=g) - 0.5).to(dev) * 0.6 for _ in range(2)]
    b = {"audios": audios, "audio_mix": audios[0] + audios[1], "id": [f"item{j}" for j in range(B)],
         "frames": [torch.randn(B, 3, args.num_frames, args.imgSize, args.imgSize, generator=g).to(dev) for _ in range(2)]}
    times = {False: [], True: []}
    with tempfile.TemporaryDirectory() as d, torch.no_grad():
        _, outputs = wrap.forward(b, args, True)
        m = P.evaluate.calc_metrics(b, outputs, args, wrap.stft_plan)
        for it in range(2 * (o.reps + 1)):
            flag = bool(it % 2)
            args.vis, args.gpu_encode = os.path.join(d, str(flag)), flag
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            V.output_visuals([], b, outputs, args, m, True, wrap.stft_plan)
            torch.cuda.synchronize()
            if it >= 2:
                times[flag].append((time.perf_counter() - t0) * 1e3)
        same = all(open(os.path.join(d, "False", "av", i, f), "rb").read() == open(os.path.join(d, "True", "av", i, f), "rb").read()
                   for i in os.listdir(os.path.join(d, "False", "av")) for f in os.listdir(os.path.join(d, "False", "av", i)) if f.endswith(".jpg"))
    result["output_visuals"] = {"items": B, "pillow_ms": spread(times[False]), "gpu_encode_ms": spread(times[True]), "jpgs_equal": same}
    print(f"output_visuals, {B} items: {statistics.median(times[False]):.1f} ms through Pillow, {statistics.median(times[True]):.1f} ms with "
          f"gpu_encode; the .jpg files equal: {same}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=192)
    ap.add_argument("--frames", type=int, default=4800)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--check", type=int, default=16)
    ap.add_argument("--cpu-files", type=int, default=96)
    ap.add_argument("--sections", type=lambda v: v.split(","), default=["batch", "clip", "pillow", "visuals"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_encode_bench.json"))
    o = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("jpeg_encode_bench measures on an MI355X; there is nothing to report without one")
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    result = {"reps": o.reps}
    for name, fn in (("batch", batch_section), ("clip", clip_section), ("pillow", pillow_section), ("visuals", visuals_section)):
        if name in o.sections:
            fn(o, dev, result)
    result["command"] = "python tools/jpeg_encode_bench.py"
    os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
    with open(o.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
