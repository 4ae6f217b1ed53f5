"""Evaluation visuals on cuda:0 (avsep_spec_image, csrc/visuals.hip; avsep_amd/visuals.py).

Two shapes: "reference", the spectrograms of one validation batch of the reference's evaluate() (64 items x 3 images of
[512, 256]: [192, 512, 256] at cell 1, masked with a threshold, JET: the predamp form), and "strip", a ten-minute recording
([3, 512, 25 840] at cell 13, masked, JET: the source pictures of `separate --report`).  Prints and writes to --out (default
profiles/visuals_bench.json):
(1) kernels.spec_image, event-timed, median of --reps after warm-up, the bytes it has to move (magnitudes and masks in, pixels
    out) against the 8 TB/s HBM peak;
(2) the same image composed from existing torch ops on the GPU (mul, log10, clamp, to(uint8), table gather, flip; amax over
    padded cells for the strip), timed the same way, and whether its bytes equal the kernel's;
(3) the NumPy f32 restatement on one CPU core (the reference's own arithmetic), median of --cpu-reps, on --cpu-items of the
    192 reference images scaled up, and on the whole strip;
(4) the share of a `--mode eval --visuals` pass: visuals.output_visuals (images, iSTFTs, every file) for one batch of 8 items
    against forward + metrics of the same batch (unet7 / resnet18dilated, random weights, random waveforms);
(5) the share of a `separate --report` run on a recording of --seconds seconds (audio only, random weights): visuals.report
    against the whole command.
The last line is one JSON object.
Usage: python tools/visuals_bench.py [--seconds 600] [--reps 20] [--cpu-reps 3] [--sections kernels,cpu,eval,cli] [--out FILE]"""
import argparse
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
from avsep_amd import kernels as K  # noqa: E402
from avsep_amd import separate as S  # noqa: E402
from avsep_amd import visuals as V  # noqa: E402
from levels_bench import HBM_PEAK, median_ms  # noqa: E402

SHAPES = {"reference": ((192, 512, 256), 1, 0.5), "strip": ((3, 512, 25840), 13, None)}


def draw(shape, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    mag = (10.0 ** (torch.rand(shape, generator=g) * 1.5) - 1.0).float()
    return mag.to(dev), torch.rand(shape, generator=g).to(dev)


def torch_image(mag, mask, thres, cell, table):
    """The picture from library ops, one launch each."""
    m = (mask > thres).float() if thres is not None else mask
    p = mag * m
    if cell > 1:
        R, F, T = p.shape
        W = -(-T // cell)
        p = torch.nn.functional.pad(p, (0, W * cell - T), value=float("-inf")).view(R, F, W, cell).amax(-1)
    lv = (torch.log10(p + 1.0) * 200.0).clamp(0.0, 255.0).to(torch.uint8)
    return table[lv.long()].flip(1)


def numpy_image(mag, mask, thres, cell, table):
    """utils.py:90-98 and main.py:367-386 as the reference writes them, f32, one core."""
    m = (mask > thres).astype(np.float32) if thres is not None else mask
    p = mag * m
    if cell > 1:
        R, F, T = p.shape
        W = -(-T // cell)
        p = np.pad(p, ((0, 0), (0, 0), (0, W * cell - T)), constant_values=-np.inf).reshape(R, F, W, cell).max(-1)
    v = np.log10(p + 1.0) * 200.0
    v[v > 255] = 255
    return table[v.astype(np.uint8)][:, ::-1]


def kernel_section(dev, reps):
    table = V.jet(dev)
    out = {}
    for name, (shape, cell, thres) in SHAPES.items():
        mag, mask = draw(shape, dev)
        W = -(-shape[2] // cell)
        moved = 2 * 4 * mag.numel() + 3 * shape[0] * shape[1] * W
        img = torch.empty((shape[0], shape[1], W, 3), dtype=torch.uint8, device=dev)
        ms = median_ms(lambda: K.spec_image(mag, mask, thres, cell, table=table, out=img), reps)
        ms_t = median_ms(lambda: torch_image(mag, mask, thres, cell, table), reps)
        same = bool(torch.equal(img, torch_image(mag, mask, thres, cell, table)))
        differ = int((img != torch_image(mag, mask, thres, cell, table)).any(-1).sum())
        out[name] = {"shape": list(shape), "cell": cell, "threshold": thres, "bytes": moved, "spec_image_ms": ms,
                     "share_of_hbm_peak": moved / (ms * 1e-3) / HBM_PEAK, "torch_ops_ms": ms_t, "torch_over_kernel": ms_t / ms,
                     "torch_bytes_equal": same, "pixels_that_differ": differ}
        print(f"{name} {list(shape)} cell {cell}: spec_image {ms:.4f} ms ({moved / 1e6:.1f} MB, {100 * out[name]['share_of_hbm_peak']:.1f}% of "
              f"8 TB/s), torch ops {ms_t:.4f} ms ({ms_t / ms:.2f}x), {differ} pixels differ", flush=True)
        del mag, mask, img
    return out


def cpu_section(reps, items):
    torch.set_num_threads(1)
    table = V.jet("cpu").numpy()
    out = {"threads": 1}
    for name, (shape, cell, thres) in SHAPES.items():
        use = (min(items, shape[0]),) + shape[1:] if name == "reference" else shape
        mag, mask = (t.numpy() for t in draw(use, "cpu"))
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            numpy_image(mag, mask, thres, cell, table)
            ts.append((time.perf_counter() - t0) * 1e3)
        ms = statistics.median(ts) * shape[0] / use[0]
        out[name + "_ms"] = ms
        out[name + "_images_timed"] = use[0]
        print(f"NumPy restatement, one core, {name}: {ms:.0f} ms ({use[0]} of {shape[0]} images timed)", flush=True)
    return out


def eval_section(dev, reps):
    """One validation batch of 8 items at the shipped shapes: forward + metrics against output_visuals."""
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
    out = {"batch": B}
    with tempfile.TemporaryDirectory() as d, torch.no_grad():
        args.vis = d

        def batch():
            return {"audios": audios, "audio_mix": audios[0] + audios[1], "id": [f"item{j}" for j in range(B)],
                    "frames": [torch.randn(B, 3, args.num_frames, args.imgSize, args.imgSize, generator=g).to(dev) for _ in range(2)]}
        for use_vis in (True, False):
            step, vis = [], []
            for it in range(reps + 1):
                b = batch()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                _, outputs = wrap.forward(b, args, use_vis)
                m = P.evaluate.calc_metrics(b, outputs, args, wrap.stft_plan)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                V.output_visuals([], b, outputs, args, m, use_vis, wrap.stft_plan)
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                if it:                                                   # the first pass warms code objects and conv plans
                    step.append((t1 - t0) * 1e3)
                    vis.append((t2 - t1) * 1e3)
            imgs = median_ms(lambda: V.item_images(b, outputs, args), reps)
            key = "av" if use_vis else "ao"
            out[key] = {"forward_and_metrics_ms": statistics.median(step), "output_visuals_ms": statistics.median(vis),
                        "item_images_ms": imgs,
                        "share_of_a_visualised_batch": statistics.median(vis) / (statistics.median(vis) + statistics.median(step))}
            print(f"eval batch of {B} ({key}): forward + metrics {out[key]['forward_and_metrics_ms']:.1f} ms, output_visuals "
                  f"{out[key]['output_visuals_ms']:.1f} ms (its images on the GPU: {imgs:.3f} ms)", flush=True)
    return out


def cli_section(seconds, dev):
    rng = np.random.default_rng(1)
    rate = 11025
    spent = []
    inner = V.report

    def timed(*a, **k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = inner(*a, **k)
        torch.cuda.synchronize()
        spent.append((time.perf_counter() - t0) * 1e3)
        return r
    with tempfile.TemporaryDirectory() as d:
        S.write_wav_pcm(os.path.join(d, "mix.wav"), rng.integers(-30000, 30000, size=int(seconds * rate)).astype(np.int16), rate)
        argv = ["--wav", os.path.join(d, "mix.wav"), "--out", os.path.join(d, "out"), "--audio_only", "--report", "--binary_mask", "0",
                "--arch_sound", "unet7", "--num_channels", "2", "--vis_channels", "256", "--img_pool", "maxpool", "--not_pool_vis",
                "--fusion_type", "hidsep", "--att_type", "sig", "--weights_sound", os.path.join(d, "sound.pth"),
                "--weights_frame", os.path.join(d, "frame.pth")]
        args = S.parse_args(argv)
        torch.manual_seed(0)
        mb = P.ModelBuilder()
        torch.save(mb.build_sound(arch=args.arch_sound, fc_dim=args.num_channels, fusion_type=args.fusion_type,
                                  att_type=args.att_type).state_dict(), os.path.join(d, "sound.pth"))
        torch.save(mb.build_frame(arch=args.arch_frame, fc_dim=args.vis_channels, pool_type=args.img_pool).state_dict(),
                   os.path.join(d, "frame.pth"))
        runs = []
        V.report = timed
        try:
            for it in range(2):                                          # the first pass warms code objects and conv plans
                spent.clear()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                S.cli(argv)
                torch.cuda.synchronize()
                runs.append(((time.perf_counter() - t0) * 1e3, sum(spent)))
        finally:
            V.report = inner
    total, rep = runs[1]
    print(f"separate --report on {seconds:.0f} s: {total:.0f} ms, {rep:.1f} ms of it in visuals.report ({100 * rep / total:.2f}%)", flush=True)
    return {"seconds": seconds, "total_ms": total, "report_ms": rep, "share_of_wall": rep / total}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=600.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cpu-reps", type=int, default=3)
    ap.add_argument("--cpu-items", type=int, default=24)
    ap.add_argument("--sections", default="kernels,cpu,eval,cli")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "visuals_bench.json"))
    o = ap.parse_args()
    sections = set(o.sections.split(","))
    if not sections or sections - {"kernels", "cpu", "eval", "cli"}:
        raise SystemExit(f"--sections takes kernels, cpu, eval, cli, got {o.sections!r}")
    if not torch.cuda.is_available():
        raise SystemExit("visuals_bench measures on an MI355X; there is nothing to report without one")
    dev = torch.device("cuda", 0)
    result = {}
    if "kernels" in sections:
        result["kernels"] = kernel_section(dev, o.reps)
    if "eval" in sections:
        result["eval_pass"] = eval_section(dev, 3)
    if "cli" in sections:
        result["separate_cli"] = cli_section(o.seconds, dev)
    if "cpu" in sections:
        result["cpu"] = cpu_section(o.cpu_reps, o.cpu_items)
    result["command"] = "python tools/visuals_bench.py" + ("" if o.sections == "kernels,cpu,eval,cli" else f" --sections {o.sections}")
    with open(o.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
