"""Sample-rate conversion on cuda:0 (csrc/resample.hip), ten minutes of audio per case.

Prints and writes to --out (default profiles/resample_bench.json):
(1) avsep_resample_poly alone on the four cases a 44.1 / 48 kHz file meets on its way through `separate` — 44.1 kHz stereo PCM
    -> 11 025, 48 kHz mono f32 -> 11 025, two sources 11 025 -> 44.1 kHz int16, two sources 11 025 -> 48 kHz int16 — event-timed,
    median of --reps after warm-up, with algorithmic bytes (input + output + filter table, each once), bytes/s and the
    share of the 8 TB/s HBM peak;
(2) scipy.signal.resample_poly on this machine's CPU for the same four cases (float64 in, as dataset.read_wav_segment
    calls it; the PCM case includes its down-mix), median of --cpu-reps;
(3) the `separate` command line's stages on a ten-minute 48 kHz mono file with the full-size model (train_MUSIC flags:
    unet7 + resnet18dilated, fp32): read, upload, resample in, separate_long, resample out (one join_frames per stem, as
    the command line writes them), download, write — each bracketed by device synchronisations, median of --cli-reps —
    and the share of the wall time each resample takes.
(4) the two ends of `--channels keep` on a 48 kHz stereo file: avsep_resample_split (PCM -> down-mix + 2 channels at 11 025)
    and avsep_resample_join (2 channels at 11 025 -> 48 kHz interleaved int16), each against the same result composed on the
    device without them — resample_pcm for the down-mix, a de-interleave to f32 rows and one batched resample for the
    channels; resample(out_s16) and a transpose back to interleaved frames — outputs compared bit for bit, in the same
    process, alternating.
(5) beside every 16-bit row of (1) and (4) the same work on 24-bit PCM and 32-bit float frames (resample_frames,
    split_frames, join_frames; a mono stem is one join_frames call of one channel, which the `_s16_per_stem` rows time for
    16-bit output against the one batched launch of the `_s16` rows), frames and outputs as the bytes of a file.
    --sections picks among kernels, channels, cli.
The last line is one JSON object.
Usage: python tools/resample_bench.py [--seconds 600] [--reps 20] [--cpu-reps 3] [--cli-reps 3] [--sections kernels,channels,cli]
       [--out FILE]"""
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
import avsep_amd as P  # noqa: E402
from avsep_amd import resample as RS  # noqa: E402
from avsep_amd import separate as S  # noqa: E402
from avsep_amd import wavio as W  # noqa: E402

HBM_PEAK = 8.0e12
MODEL_RATE = 11025


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


def cpu_median_ms(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def kernel_cases(seconds, dev, reps, cpu_reps):
    from scipy.signal import resample_poly
    rng = np.random.default_rng(0)
    cases = {}

    def add(name, x_np, rate_in, rate_out, in_ch, out_fmt, cpu_fn):
        up, down = RS.rational(rate_in, rate_out)
        filt = RS.filter_table(up, down, dev)
        x = torch.from_numpy(x_np).to(dev)
        if in_ch:                                                        # 16-bit frames as the bytes they are
            x = x.view(torch.uint8).reshape(-1)
        in_fmt = "s16" if in_ch else "f32"
        y = P.kernels.resample_poly(x, filt, up, down, in_ch, in_fmt, out_fmt)
        nbytes = x.numel() * x.element_size() + y.numel() * y.element_size() + filt.numel() * 4
        ms = median_ms(lambda: P.kernels.resample_poly(x, filt, up, down, in_ch, in_fmt, out_fmt), reps)
        cpu_ms = cpu_median_ms(cpu_fn, cpu_reps)
        cases[name] = {"up": up, "down": down, "taps_per_output": -(-(20 * max(up, down) + 1) // up), "rows": y.shape[0],
                       "samples_in": x_np.shape[0] if in_ch else x_np.shape[1], "samples_out": y.shape[1], "kernel_ms": ms,
                       "algorithmic_bytes": nbytes, "bytes_per_s": nbytes / (ms * 1e-3),
                       "share_of_hbm_peak": nbytes / (ms * 1e-3) / HBM_PEAK, "scipy_cpu_ms": cpu_ms, "scipy_over_kernel": cpu_ms / ms}
        c = cases[name]
        print(f"{name}: {up}/{down}, kernel {ms:.3f} ms ({c['bytes_per_s'] / 1e12:.2f} TB/s algorithmic, "
              f"{100 * c['share_of_hbm_peak']:.1f}% of 8 TB/s), scipy on this CPU {cpu_ms:.0f} ms ({cpu_ms / ms:.0f} x)", flush=True)

    pcm = rng.integers(-20000, 20000, size=(int(seconds * 44100), 2)).astype(np.int16)
    add("pcm_stereo_44100_to_11025", pcm, 44100, MODEL_RATE, 2, "f32",
        lambda: resample_poly(pcm.astype(np.float64).mean(1) / 32768.0, 1, 4))
    mono = (rng.random((1, int(seconds * 48000)), dtype=np.float32) * 2 - 1) * 0.5
    mono64 = mono[0].astype(np.float64)
    add("f32_mono_48000_to_11025", mono, 48000, MODEL_RATE, 0, "f32", lambda: resample_poly(mono64, 147, 640))
    src = (rng.random((2, int(seconds * MODEL_RATE)), dtype=np.float32) * 2 - 1) * 0.5
    src64 = src.astype(np.float64)
    add("two_sources_11025_to_44100_s16", src, MODEL_RATE, 44100, 0, "s16", lambda: resample_poly(src64, 4, 1, axis=1))
    add("two_sources_11025_to_48000_s16", src, MODEL_RATE, 48000, 0, "s16", lambda: resample_poly(src64, 640, 147, axis=1))

    def add_fn(name, fn, rate_in, rate_out, nbytes_in, like):
        """A *_frames row beside the 16-bit row ``like``: the same samples in another format."""
        up, down = RS.rational(rate_in, rate_out)
        y = fn()
        ys = y if isinstance(y, list) else [y]
        nbytes = nbytes_in + sum(t.numel() * t.element_size() for t in ys) + RS.filter_table(up, down, dev).numel() * 4
        ms = median_ms(fn, reps)
        cases[name] = {"up": up, "down": down, "kernel_ms": ms, "algorithmic_bytes": nbytes, "bytes_per_s": nbytes / (ms * 1e-3),
                       "share_of_hbm_peak": nbytes / (ms * 1e-3) / HBM_PEAK, "over_the_s16_row": ms / cases[like]["kernel_ms"]}
        print(f"{name}: {up}/{down}, kernel {ms:.3f} ms ({nbytes / (ms * 1e-3) / 1e12:.2f} TB/s algorithmic, "
              f"{100 * cases[name]['share_of_hbm_peak']:.1f}% of 8 TB/s), {cases[name]['over_the_s16_row']:.2f} x the s16 row", flush=True)

    for fmt in ("s24", "f32"):
        raw = frames_of(pcm, fmt).to(dev)
        add_fn(f"{fmt}_stereo_44100_to_11025", lambda: RS.resample_frames(raw, fmt, 2, 44100, MODEL_RATE), 44100, MODEL_RATE,
               raw.numel(), "pcm_stereo_44100_to_11025")
        del raw
    srcs = torch.from_numpy(src).to(dev)
    for rate in (44100, 48000):
        for fmt in ("s16_per_stem", "s24", "f32"):
            add_fn(f"two_sources_11025_to_{rate}_{fmt}", lambda: [RS.join_frames(srcs[n:n + 1], MODEL_RATE, rate, fmt[:3]) for n in range(2)],
                   MODEL_RATE, rate, srcs.numel() * 4, f"two_sources_11025_to_{rate}_s16")
    return cases


def frames_of(pcm, fmt):
    """int16 [L, C] -> the same samples as a file's bytes in ``fmt`` (s24: shifted left by 8; f32: over 32768), uint8 [L*C*bytes]."""
    if fmt == "f32":
        return torch.from_numpy((pcm.astype(np.float32) / 32768.0).view(np.uint8).reshape(-1))
    out = np.zeros(pcm.shape + (3,), np.uint8)
    out[..., 1:] = np.ascontiguousarray(pcm.astype("<i2")).view(np.uint8).reshape(pcm.shape + (2,))
    return torch.from_numpy(out.reshape(-1))


def channel_cases(seconds, dev, reps, rate=48000, channels=2):
    """split and join against their compositions from resample_pcm / resample and torch copies."""
    rng = np.random.default_rng(2)
    pcm = torch.from_numpy(rng.integers(-20000, 20000, size=(int(seconds * rate), channels)).astype(np.int16)).to(dev)
    x = torch.from_numpy((rng.random((channels, int(seconds * MODEL_RATE)), dtype=np.float32) * 2 - 1) * 0.5).to(dev)

    def split_composed():
        rows = (pcm.t().contiguous().float() / 32768.0)                                   # de-interleave: [C, L] f32
        return torch.cat([RS.resample_pcm(pcm, rate, MODEL_RATE)[None], RS.resample(rows, rate, MODEL_RATE)])

    def join_composed():
        return RS.resample(x, MODEL_RATE, rate, out_s16=True).t().contiguous()
    out = {}
    for name, fused, composed, src in (("split_pcm_stereo_48000_to_11025", lambda: RS.split_pcm(pcm, rate, MODEL_RATE), split_composed, pcm),
                                       ("join_stereo_11025_to_48000_s16", lambda: RS.join_pcm(x, MODEL_RATE, rate), join_composed, x)):
        a, b = fused(), composed()
        up, down = RS.rational(rate, MODEL_RATE) if src is pcm else RS.rational(MODEL_RATE, rate)
        nbytes = src.numel() * src.element_size() + a.numel() * a.element_size() + RS.filter_table(up, down, dev).numel() * 4
        ms_f, ms_c = [], []
        for _ in range(3):                                                            # alternate the two variants
            ms_f.append(median_ms(fused, reps))
            ms_c.append(median_ms(composed, reps))
        ms_f, ms_c = statistics.median(ms_f), statistics.median(ms_c)
        out[name] = {"up": up, "down": down, "channels": channels, "kernel_ms": ms_f, "composed_ms": ms_c,
                     "composed_over_kernel": ms_c / ms_f, "algorithmic_bytes": nbytes, "bytes_per_s": nbytes / (ms_f * 1e-3),
                     "share_of_hbm_peak": nbytes / (ms_f * 1e-3) / HBM_PEAK, "bit_identical_to_composed": bool(torch.equal(a, b))}
        c = out[name]
        print(f"{name}: {up}/{down}, kernel {ms_f:.3f} ms ({c['bytes_per_s'] / 1e12:.2f} TB/s algorithmic, "
              f"{100 * c['share_of_hbm_peak']:.1f}% of 8 TB/s), composed {ms_c:.3f} ms ({ms_c / ms_f:.2f} x), "
              f"bit-identical {c['bit_identical_to_composed']}", flush=True)
    # the same two ends on 24-bit and float frames: one launch each, as their 16-bit rows
    pcm_np = pcm.cpu().numpy()
    for fmt in ("s24", "f32"):
        raw = frames_of(pcm_np, fmt).to(dev)
        for name, fn, like, nin in ((f"split_{fmt}_stereo_48000_to_11025", lambda: RS.split_frames(raw, fmt, channels, rate, MODEL_RATE),
                                     "split_pcm_stereo_48000_to_11025", raw.numel()),
                                    (f"join_stereo_11025_to_48000_{fmt}", lambda: RS.join_frames(x, MODEL_RATE, rate, fmt),
                                     "join_stereo_11025_to_48000_s16", x.numel() * 4)):
            up, down = RS.rational(rate, MODEL_RATE) if name.startswith("split") else RS.rational(MODEL_RATE, rate)
            y = fn()
            nbytes = nin + y.numel() * y.element_size() + RS.filter_table(up, down, dev).numel() * 4
            ms = median_ms(fn, reps)
            out[name] = {"up": up, "down": down, "channels": channels, "kernel_ms": ms, "algorithmic_bytes": nbytes,
                         "bytes_per_s": nbytes / (ms * 1e-3), "share_of_hbm_peak": nbytes / (ms * 1e-3) / HBM_PEAK,
                         "over_the_s16_row": ms / out[like]["kernel_ms"]}
            print(f"{name}: {up}/{down}, kernel {ms:.3f} ms ({nbytes / (ms * 1e-3) / 1e12:.2f} TB/s algorithmic, "
                  f"{100 * out[name]['share_of_hbm_peak']:.1f}% of 8 TB/s), {out[name]['over_the_s16_row']:.2f} x the s16 row", flush=True)
        del raw
    return out


def cli_stages(seconds, dev, reps, frame_size=224):
    """The stages of separate.cli on a 48 kHz mono file, timed one by one (each ends in a device synchronise)."""
    args = P.arguments.train_music_args()
    args.stft_pad_mode = "reflect"
    torch.manual_seed(0)
    mb = P.ModelBuilder()
    snd = mb.build_sound(arch=args.arch_sound, fc_dim=args.num_channels, fusion_type=args.fusion_type, att_type=args.att_type)
    frm = mb.build_frame(arch=args.arch_frame, fc_dim=args.vis_channels, pool_type=args.img_pool)
    nets = (snd.to(dev).eval(), frm.to(dev).eval())
    frames = [torch.randn(1, 3, frame_size, frame_size, device=dev) for _ in range(args.num_mix)]
    rate = 48000
    rng = np.random.default_rng(1)
    runs = []
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "mix.wav")
        S.write_wav_pcm(path, rng.integers(-10000, 10000, size=int(seconds * rate)).astype(np.int16), rate)
        for it in range(reps + 1):                                       # the first pass warms code objects and conv plans
            ms = {}

            def stage(name, fn):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r = fn()
                torch.cuda.synchronize()
                ms[name] = (time.perf_counter() - t0) * 1e3
                return r
            pcm = stage("read_wav_pcm", lambda: W.read_frames(path)[0])
            up = stage("upload_pcm", lambda: torch.from_numpy(pcm).to(dev))
            wav = stage("resample_in", lambda: RS.resample_frames(up, "s16", 1, rate, args.audRate))
            out = stage("separate_long", lambda: S.separate_long(nets, wav, frames, args))
            s16 = stage("resample_out", lambda: [RS.join_frames(w[None], args.audRate, rate, "s16") for w in out["wavs"]])
            host = stage("download_s16", lambda: [w.cpu().numpy() for w in s16])
            stage("write_wav_pcm", lambda: [W.write_frames(os.path.join(d, f"source{n}.wav"), w, rate, 1, "s16") for n, w in enumerate(host)])
            ms["total"] = sum(ms.values())
            if it:
                runs.append(ms)
    split = {k: statistics.median(r[k] for r in runs) for k in runs[0]}
    share = {k: split[k] / split["total"] for k in ("resample_in", "resample_out")}
    print(f"separate on {seconds:.0f} s at {rate} Hz: " + ", ".join(f"{k} {v:.2f} ms" for k, v in split.items()), flush=True)
    print(f"    resample in {100 * share['resample_in']:.2f}% and out {100 * share['resample_out']:.2f}% of the wall time", flush=True)
    return {"file_rate": rate, "model": f"{args.arch_sound}+{args.arch_frame}", "split_ms": split, "share_of_wall": share}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=600.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cpu-reps", type=int, default=3)
    ap.add_argument("--cli-reps", type=int, default=3)
    ap.add_argument("--sections", default="kernels,channels,cli", help="comma-separated: kernels, channels, cli")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample_bench.json"))
    o = ap.parse_args()
    sections = set(o.sections.split(","))
    if not sections or sections - {"kernels", "channels", "cli"}:
        raise SystemExit(f"--sections takes kernels, channels, cli, got {o.sections!r}")
    if not torch.cuda.is_available():
        raise SystemExit("resample_bench measures on an MI355X; there is nothing to report without one")
    dev = torch.device("cuda", 0)
    result = {"seconds": o.seconds, "kernel_reps": o.reps, "cpu_reps": o.cpu_reps, "cpu_threads": torch.get_num_threads()}
    if "kernels" in sections:
        result["kernels"] = kernel_cases(o.seconds, dev, o.reps, o.cpu_reps)
    if "channels" in sections:
        result["channels"] = channel_cases(o.seconds, dev, o.reps)
    if "cli" in sections:
        result["separate_cli"] = cli_stages(o.seconds, dev, o.cli_reps)
    result["command"] = "python tools/resample_bench.py" + ("" if o.sections == "kernels,channels,cli" else f" --sections {o.sections}")
    with open(o.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
