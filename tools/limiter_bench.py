"""The linked look-ahead limiter on cuda:0 (avsep_limiter, csrc/levels.hip): levels.limit on [1, 4, seconds * 48000] — ten minutes
of 48 kHz stereo, two stems, ONE programme of four rows, at the default look-ahead of 5 ms (A = 240).

Two inputs: "sparse", quiet noise with one spike per --spike-every samples, so that roughly 1 % of the samples are limited at
pre-gain 1 (every other tile of avsep_limiter's second launch skips minimum and sum), and "dense", the same rows at pre-gain 8,
where every sample is limited.  Prints and writes to --out (default profiles/limiter_bench.json):
(1) avsep_limiter as a whole, event-timed, median of --reps after warm-up, with and without the gain store; its three launches
    one by one as torch.profiler sees them (median per kernel name; events cannot be placed between the launches of one call);
    the bytes each launch moves against the 8 TB/s HBM peak; avsep_true_peak on the same rows beside the detector, since they
    share the arithmetic; levels.limit as a whole (limiter, the measurement of y, the trim);
(2) the float64 SciPy restatement on the CPU on a pool of --threads threads (the row cut into chunks with their halo:
    upfirdn, minimum_filter1d, oaconvolve, the product), median of --cpu-reps;
(3) the share of a `separate --loudness -16 --limit -1 --channels keep` run on a file of that length (the full-size model,
    train_MUSIC's flags, random weights) that levels.limit takes.
The last line is one JSON object.
Usage: python tools/limiter_bench.py [--seconds 600] [--reps 10] [--cpu-reps 1] [--threads 16] [--sections kernels,cpu,cli] [--out FILE]"""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
import avsep_amd as P  # noqa: E402
from avsep_amd import levels as LV  # noqa: E402
from avsep_amd import separate as S  # noqa: E402
from levels_bench import HBM_PEAK, RATE, median_ms, wall_ms  # noqa: E402

CEILING_DB = -1.0
LOOKAHEAD_MS = 5.0
KERNELS = ("lim_detect_kernel", "lim_apply_kernel", "lim_stats_kernel")


def make_rows(seconds, spike_every, dev):
    """f32 [1, 4, L]: 0.1 * uniform noise, one spike of +-1.5 every ``spike_every`` samples, in turn in each of the four rows."""
    L = int(seconds * RATE)
    g = torch.Generator().manual_seed(0)
    x = (torch.rand((1, 4, L), generator=g) * 2 - 1) * 0.1
    pos = torch.arange(spike_every // 2, L, spike_every)
    x[0, torch.arange(pos.numel()) % 4, pos] = torch.where(torch.arange(pos.numel()) % 2 == 0, 1.5, -1.5)
    return x.to(dev)


def per_launch_ms(fn, reps):
    """Median device time per kernel name over ``reps`` calls of fn, from torch.profiler; None where it records no kernels."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
        times = {}
        for ev in prof.events():
            for name in KERNELS + ("tp_tile_kernel",):
                if name in ev.name and ev.device_time > 0:
                    times.setdefault(name, []).append(ev.device_time / 1e3)
        return {k: statistics.median(v) for k, v in times.items()} or None
    except Exception as e:                                               # a profiler that is not there: the whole-call times stand
        print(f"torch.profiler gave no per-launch times ({type(e).__name__}: {e})", flush=True)
        return None


def kernel_section(x, reps):
    _, C, L = x.shape
    os_, taps = LV.peak_table(RATE, x.device)
    A, w = LV.limiter_plan(RATE, LOOKAHEAD_MS)
    w = torch.from_numpy(w).to(x.device)
    c = 10.0 ** (CEILING_DB / 20.0)
    rows = x.reshape(C, L)
    tiles = -(-L // 2048)
    moved = {"lim_detect_kernel": 4 * C * L + 8 * L, "lim_apply_kernel": (8 * L + 8 * 4 * A * tiles) + 2 * 4 * C * L,
             "lim_stats_kernel": 24 * tiles}
    out = {"rows": C, "samples": L, "half_width": A, "ceiling_dbtp": CEILING_DB}
    ms = median_ms(lambda: P.kernels.true_peak(rows, taps, os_), reps)
    out["true_peak"] = {"kernel_ms": ms, "bytes": 4 * C * L, "share_of_hbm_peak": 4 * C * L / (ms * 1e-3) / HBM_PEAK}
    print(f"avsep_true_peak on the same rows: {ms:.3f} ms", flush=True)
    y = torch.empty_like(x)
    for name, G in (("sparse", 1.0), ("dense", 8.0)):
        def run(gain=False):
            return P.kernels.limiter(x, taps, w, os_, G, c, return_gain=gain, out=y)
        stats = run()[2].cpu()
        r = {"pre_gain": G, "limited_share": stats[0, 2].item() / L, "min_gain": stats[0, 1].item(),
             "call_ms": median_ms(run, reps), "call_with_gain_store_ms": median_ms(lambda: run(True), reps)}
        r["bytes"] = sum(moved.values())
        r["share_of_hbm_peak"] = r["bytes"] / (r["call_ms"] * 1e-3) / HBM_PEAK
        launches = per_launch_ms(run, reps)
        if launches:
            r["launch_ms"] = {k: launches[k] for k in KERNELS if k in launches}
            r["launch_share_of_hbm_peak"] = {k: moved[k] / (v * 1e-3) / HBM_PEAK for k, v in r["launch_ms"].items()}
        xs = x[0]
        r["limit_wall_ms"] = wall_ms(lambda: LV.limit(xs, RATE, CEILING_DB, gain=G, lookahead_ms=LOOKAHEAD_MS), reps)
        out[name] = r
        print(f"{name} (pre-gain {G:g}, {100 * r['limited_share']:.2f} % limited): avsep_limiter {r['call_ms']:.3f} ms "
              f"({100 * r['share_of_hbm_peak']:.1f}% of 8 TB/s), {r['call_with_gain_store_ms']:.3f} ms with the gain store, launches "
              f"{r.get('launch_ms')}; levels.limit as a whole {r['limit_wall_ms']:.3f} ms", flush=True)
    return out


def cpu_section(x, reps, threads):
    from scipy import ndimage, signal
    rows = x[0].cpu().numpy().astype(np.float64)
    C, L = rows.shape
    os_, g = LV.peak_filter(RATE)
    A, w = LV.limiter_plan(RATE, LOOKAHEAD_MS)
    c = 10.0 ** (CEILING_DB / 20.0)
    halo = 2 * A + 10
    edges = np.linspace(0, L, threads + 1).astype(int)
    out = {"threads": threads}

    def chunk(job, G):
        lo, hi = job
        a, b = max(0, lo - halo), min(L, hi + halo)
        p = np.zeros(b - a)
        for r_ in range(C):
            u = np.abs(signal.upfirdn(g, rows[r_, a:b], up=os_))[10 * os_:10 * os_ + os_ * (b - a)]
            p = np.maximum(p, np.maximum(np.abs(rows[r_, a:b]), u.reshape(-1, os_).max(1)))
        with np.errstate(divide="ignore"):
            r = np.minimum(1.0, c / (G * p))
        h = ndimage.minimum_filter1d(r, 2 * A + 1, mode="constant", cval=1.0)
        gain = 1.0 - signal.oaconvolve(1.0 - h, w, mode="same")
        return (rows[:, lo:hi] * (G * gain[lo - a:lo - a + hi - lo])).astype(np.float32)
    with ThreadPoolExecutor(threads) as pool:
        for name, G in (("sparse", 1.0), ("dense", 8.0)):
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter()
                list(pool.map(lambda job: chunk(job, G), zip(edges[:-1], edges[1:])))
                ts.append((time.perf_counter() - t0) * 1e3)
            out[name + "_ms"] = statistics.median(ts)
            print(f"CPU restatement ({name}) on {threads} threads: {out[name + '_ms']:.0f} ms", flush=True)
        y_cpu = np.concatenate(list(pool.map(lambda job: chunk(job, 1.0), zip(edges[:-1], edges[1:]))), axis=1)
    if x.is_cuda:                                                        # the restatement computes what the kernels compute
        y_gpu = LV.limit(x[0], RATE, CEILING_DB, lookahead_ms=LOOKAHEAD_MS, trim=False)[0].cpu().numpy()
        out["sparse_max_abs_diff_to_gpu"] = float(np.abs(y_cpu.astype(np.float64) - y_gpu).max())
        print(f"CPU restatement against avsep_limiter: largest difference {out['sparse_max_abs_diff_to_gpu']:.3e}", flush=True)
    return out


def cli_section(seconds, dev):
    """`separate --loudness -16 --limit -1 --channels keep --out_format f32` on a stereo 48 kHz file: the time inside levels.limit
    against the whole run."""
    rng = np.random.default_rng(1)
    spent = []
    inner = LV.limit

    def timed(*a, **k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = inner(*a, **k)
        torch.cuda.synchronize()
        spent.append((time.perf_counter() - t0) * 1e3)
        return r
    with tempfile.TemporaryDirectory() as d:
        S.write_wav_pcm_channels(os.path.join(d, "mix.wav"), rng.integers(-30000, 30000, size=(int(seconds * RATE), 2)).astype(np.int16), RATE)
        argv = ["--wav", os.path.join(d, "mix.wav"), "--out", os.path.join(d, "out"), "--audio_only", "--channels", "keep", "--loudness", "-16",
                "--limit", "-1", "--out_format", "f32", "--binary_mask", "0", "--arch_sound", "unet7", "--num_channels", "2", "--vis_channels", "256",
                "--img_pool", "maxpool", "--not_pool_vis", "--fusion_type", "hidsep", "--att_type", "sig",
                "--weights_sound", os.path.join(d, "sound.pth"), "--weights_frame", os.path.join(d, "frame.pth")]
        args = S.parse_args(argv)                                        # the model the command line will build
        torch.manual_seed(0)
        mb = P.ModelBuilder()
        torch.save(mb.build_sound(arch=args.arch_sound, fc_dim=args.num_channels, fusion_type=args.fusion_type,
                                  att_type=args.att_type).state_dict(), os.path.join(d, "sound.pth"))
        torch.save(mb.build_frame(arch=args.arch_frame, fc_dim=args.vis_channels, pool_type=args.img_pool).state_dict(),
                   os.path.join(d, "frame.pth"))
        runs = []
        LV.limit = timed
        try:
            for it in range(2):                                          # the first pass warms code objects and conv plans
                spent.clear()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                S.cli(argv)
                torch.cuda.synchronize()
                runs.append(((time.perf_counter() - t0) * 1e3, sum(spent), len(spent)))
        finally:
            LV.limit = inner
        with open(os.path.join(d, "out", "levels.json")) as f:
            rep = json.load(f)
    total, lim, calls = min(runs[1:])
    print(f"separate --loudness -16 --limit -1 on {seconds:.0f} s of 48 kHz stereo: {total:.0f} ms, {lim:.1f} ms of it in {calls} call of "
          f"levels.limit ({100 * lim / total:.2f}%); {rep['limiter']}", flush=True)
    return {"total_ms": total, "limit_ms": lim, "limit_calls": calls, "share_of_wall": lim / total, "limiter": rep["limiter"],
            "limited_by": rep["limited_by"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=600.0)
    ap.add_argument("--spike-every", type=int, default=98000, help="samples between spikes of the sparse input (4A + 20 = 980 limited each)")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--cpu-reps", type=int, default=1)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--sections", default="kernels,cpu,cli")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "limiter_bench.json"))
    o = ap.parse_args()
    sections = set(o.sections.split(","))
    if not sections or sections - {"kernels", "cpu", "cli"}:
        raise SystemExit(f"--sections takes kernels, cpu, cli, got {o.sections!r}")
    if not torch.cuda.is_available():
        raise SystemExit("limiter_bench measures on an MI355X; there is nothing to report without one")
    dev = torch.device("cuda", 0)
    x = make_rows(o.seconds, o.spike_every, dev)
    result = {"seconds": o.seconds, "shape": list(x.shape), "rate": RATE, "lookahead_ms": LOOKAHEAD_MS}
    if "kernels" in sections:
        result["kernels"] = kernel_section(x, o.reps)
    if "cpu" in sections:
        result["cpu"] = cpu_section(x, o.cpu_reps, o.threads)
    del x
    if "cli" in sections:
        result["separate_cli"] = cli_section(o.seconds, dev)
    result["command"] = "python tools/limiter_bench.py" + ("" if o.sections == "kernels,cpu,cli" else f" --sections {o.sections}")
    with open(o.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
