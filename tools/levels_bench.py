"""Stem levels on cuda:0 (csrc/levels.hip): levels.measure on [2, 2, seconds * 48000] — ten minutes of 48 kHz stereo, two stems.

Prints and writes to --out (default profiles/levels_bench.json):
(1) avsep_loudness_energies and avsep_true_peak alone, event-timed, median of --reps after warm-up, with the bytes each has
    to read (the rows once for the peak, twice for the energies) and the share of the 8 TB/s HBM peak; levels.measure as a
    whole (both kernels, the energies' way to the host, the gating);
(2) what measuring on the host would cost: the device-to-host copy of the same rows (it would come first; pageable and pinned), then
    scipy.signal.sosfilt + block sums and scipy.signal.upfirdn + max on a pool of --threads threads (sosfilt is serial in
    time: one thread per row; the oversampler is cut into --threads chunks with their halo), median of --cpu-reps;
(3) the share of a `separate --peak -1 --channels keep` run on a file of that length (the full-size model, train_MUSIC's flags, random
    weights) that levels.measure takes: the command line is run as it is, with a device-synchronised stopwatch round measure.
The last line is one JSON object.
Usage: python tools/levels_bench.py [--seconds 600] [--reps 10] [--cpu-reps 1] [--threads 16] [--sections kernels,cpu,cli] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import avsep_amd as P  # noqa: E402
from avsep_amd import levels as LV  # noqa: E402
from avsep_amd import separate as S  # noqa: E402

HBM_PEAK = 8.0e12
RATE = 48000


def median_ms(fn, reps, warmup=2):
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


def wall_ms(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def kernel_section(x, reps):
    rows = x.reshape(-1, x.shape[-1])
    h = (RATE + 5) // 10
    sos = LV.k_weighting(RATE)
    os_, taps = LV.peak_table(RATE, x.device)
    nbytes = rows.numel() * 4
    out = {"rows": rows.shape[0], "samples": rows.shape[1], "sub_block": h}
    for name, fn, passes in (("loudness_energies", lambda: P.kernels.loudness_energies(rows, sos, h), 2),
                             ("true_peak", lambda: P.kernels.true_peak(rows, taps, os_), 1)):
        ms = median_ms(fn, reps)
        out[name] = {"kernel_ms": ms, "bytes_read": passes * nbytes, "bytes_per_s": passes * nbytes / (ms * 1e-3),
                     "share_of_hbm_peak": passes * nbytes / (ms * 1e-3) / HBM_PEAK}
        print(f"{name}: {ms:.3f} ms ({out[name]['bytes_per_s'] / 1e12:.2f} TB/s, {100 * out[name]['share_of_hbm_peak']:.1f}% of 8 TB/s)", flush=True)
    out["measure_wall_ms"] = wall_ms(lambda: LV.measure(x, RATE), reps)
    out["device_to_host_ms"] = wall_ms(lambda: rows.cpu(), max(2, reps // 3))                  # into pageable memory, as .cpu() does
    pinned = torch.empty(rows.shape, dtype=rows.dtype, pin_memory=True)
    out["device_to_pinned_host_ms"] = wall_ms(lambda: pinned.copy_(rows), max(2, reps // 3))
    print(f"levels.measure as a whole {out['measure_wall_ms']:.3f} ms; the rows' device-to-host copy alone {out['device_to_host_ms']:.1f} ms "
          f"pageable, {out['device_to_pinned_host_ms']:.1f} ms pinned", flush=True)
    return out


def cpu_section(x, reps, threads):
    from scipy import signal
    rows = x.reshape(-1, x.shape[-1]).cpu().numpy().astype(np.float64)
    h = (RATE + 5) // 10
    sos = LV.k_weighting(RATE)
    os_, g = LV.peak_filter(RATE)

    def energies(r):
        y = signal.sosfilt(sos, rows[r])
        S_ = y.size // h
        y = y[:S_ * h].reshape(S_, h)
        return (y * y).sum(1)

    def peak(job):
        r, lo, hi = job
        seg = rows[r, max(0, lo - 10):min(rows.shape[1], hi + 10)]
        return np.abs(signal.upfirdn(g, seg, up=os_)).max()
    per = max(1, threads // rows.shape[0])
    edges = np.linspace(0, rows.shape[1], per + 1).astype(int)
    jobs = [(r, edges[i], edges[i + 1]) for r in range(rows.shape[0]) for i in range(per)]
    out = {}
    with ThreadPoolExecutor(threads) as pool:
        for name, fn in (("sosfilt_block_sums", lambda: list(pool.map(energies, range(rows.shape[0])))),
                         ("upfirdn_max", lambda: list(pool.map(peak, jobs)))):
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter()
                fn()
                ts.append((time.perf_counter() - t0) * 1e3)
            out[name + "_ms"] = statistics.median(ts)
            print(f"CPU {name} on {threads} threads: {out[name + '_ms']:.0f} ms", flush=True)
    out["threads"] = threads
    return out


def cli_section(seconds, dev):
    """`separate --peak -1 --channels keep --out_format f32` on a stereo 48 kHz file, the time inside levels.measure against the whole run."""
    rng = np.random.default_rng(1)
    spent = []
    inner = LV.measure

    def timed(*a, **k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = inner(*a, **k)
        torch.cuda.synchronize()
        spent.append((time.perf_counter() - t0) * 1e3)
        return r
    with tempfile.TemporaryDirectory() as d:
        S.write_wav_pcm_channels(os.path.join(d, "mix.wav"), rng.integers(-30000, 30000, size=(int(seconds * RATE), 2)).astype(np.int16), RATE)
        argv = ["--wav", os.path.join(d, "mix.wav"), "--out", os.path.join(d, "out"), "--audio_only", "--channels", "keep", "--peak", "-1",
                "--out_format", "f32", "--binary_mask", "0", "--arch_sound", "unet7", "--num_channels", "2", "--vis_channels", "256", "--img_pool", "maxpool",
                "--not_pool_vis", "--fusion_type", "hidsep", "--att_type", "sig", "--weights_sound", os.path.join(d, "sound.pth"), "--weights_frame", os.path.join(d, "frame.pth")]
        args = S.parse_args(argv)                                        # the model the command line will build
        torch.manual_seed(0)
        mb = P.ModelBuilder()
        torch.save(mb.build_sound(arch=args.arch_sound, fc_dim=args.num_channels, fusion_type=args.fusion_type,
                                  att_type=args.att_type).state_dict(), os.path.join(d, "sound.pth"))
        torch.save(mb.build_frame(arch=args.arch_frame, fc_dim=args.vis_channels, pool_type=args.img_pool).state_dict(),
                   os.path.join(d, "frame.pth"))
        runs = []
        LV.measure = timed
        try:
            for it in range(2):                                          # the first pass warms code objects and conv plans
                spent.clear()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                S.cli(argv)
                torch.cuda.synchronize()
                runs.append(((time.perf_counter() - t0) * 1e3, sum(spent), len(spent)))
        finally:
            LV.measure = inner
    total, meas, calls = min(runs[1:])
    print(f"separate --peak -1 on {seconds:.0f} s of 48 kHz stereo: {total:.0f} ms, {meas:.1f} ms of it in {calls} calls of levels.measure "
          f"({100 * meas / total:.2f}%)", flush=True)
    return {"total_ms": total, "measure_ms": meas, "measure_calls": calls, "share_of_wall": meas / total}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=600.0)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--cpu-reps", type=int, default=1)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--sections", default="kernels,cpu,cli")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "levels_bench.json"))
    o = ap.parse_args()
    sections = set(o.sections.split(","))
    if not sections or sections - {"kernels", "cpu", "cli"}:
        raise SystemExit(f"--sections takes kernels, cpu, cli, got {o.sections!r}")
    if not torch.cuda.is_available():
        raise SystemExit("levels_bench measures on an MI355X; there is nothing to report without one")
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    x = ((torch.rand((2, 2, int(o.seconds * RATE)), generator=g) * 2 - 1) * 0.5).to(dev)
    result = {"seconds": o.seconds, "shape": list(x.shape), "rate": RATE}
    if "kernels" in sections:
        result["kernels"] = kernel_section(x, o.reps)
    if "cpu" in sections:
        result["cpu"] = cpu_section(x, o.cpu_reps, o.threads)
    del x
    if "cli" in sections:
        result["separate_cli"] = cli_section(o.seconds, dev)
    result["command"] = "python tools/levels_bench.py" + ("" if o.sections == "kernels,cpu,cli" else f" --sections {o.sections}")
    with open(o.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
