"""Full-band stems on cuda:0 (csrc/fullband.hip): what `separate --band full` adds to `--band model` on ten minutes of 48 kHz
stereo with two stems (N = 2 sources, G = 2 channels, 1022 / 256 STFT at 11 025 Hz).

Prints and writes to --out (default profiles/fullband_bench.json), event-timed, median of --reps after warm-up, each with its
algorithmic bytes (every operand and the result once), bytes/s and the share of the 8 TB/s HBM peak:
  band_gains    kernels.band_gains over the top octave (bins 256 ... 511) of [2,2,512,F] stem and [2,512,F] mixture magnitudes;
  band_extend   resample.band_extend: stems [2,2,Lm], low [2,L], file [2,Lf], gains -> [2,2,Lout] at 48 kHz;
  resample      resample.resample of the same four stem rows: what --band model computes for the same file;
and the ratio (band_gains + band_extend) / resample.  The last line is one JSON object.
Usage: python tools/fullband_bench.py [--seconds 600] [--reps 20] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import avsep_amd as P  # noqa: E402
from avsep_amd import resample as RS  # noqa: E402

HBM_PEAK = 8.0e12
MODEL_RATE, FILE_RATE = 11025, 48000
N, G, BINS, HOP = 2, 2, 512, 256


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


def nbytes(*tensors):
    return sum(t.numel() * t.element_size() for t in tensors)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=600.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fullband_bench.json"))
    o = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fullband_bench measures on an MI355X; there is nothing to report without one")
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    L = int(o.seconds * MODEL_RATE)
    F = L // HOP + 1
    Lm = HOP * (F - 1)
    up, down = RS.rational(MODEL_RATE, FILE_RATE)
    filt = RS.filter_table(up, down, dev)
    mix_mag = torch.rand(G, BINS, F, device=dev, generator=g)
    stem_mag = mix_mag[None] * torch.rand(N, G, BINS, F, device=dev, generator=g)
    stems = torch.rand(N, G, Lm, device=dev, generator=g) - 0.5
    low = torch.rand(G, L, device=dev, generator=g) - 0.5
    file = torch.rand(G, int(o.seconds * FILE_RATE), device=dev, generator=g) - 0.5
    rows = stems.reshape(N * G, Lm)
    gains = P.kernels.band_gains(stem_mag, mix_mag)
    out = RS.band_extend(stems, low, file, gains, MODEL_RATE, FILE_RATE, HOP)
    plain = RS.resample(rows, MODEL_RATE, FILE_RATE)
    lo = BINS // 2
    cases = {
        "band_gains": (lambda: P.kernels.band_gains(stem_mag, mix_mag),
                       (nbytes(stem_mag, mix_mag) * (BINS - lo)) // BINS + nbytes(gains)),
        "band_extend": (lambda: RS.band_extend(stems, low, file, gains, MODEL_RATE, FILE_RATE, HOP),
                        nbytes(stems, low, file[:, :out.shape[2]], gains, filt, out)),
        "resample": (lambda: RS.resample(rows, MODEL_RATE, FILE_RATE), nbytes(rows, filt, plain)),
    }
    result = {"seconds": o.seconds, "reps": o.reps, "sources": N, "channels": G, "frames": F, "up": up, "down": down,
              "samples_out": out.shape[2], "rows": {}}
    for name, (fn, b) in cases.items():
        ms = median_ms(fn, o.reps)
        result["rows"][name] = {"kernel_ms": ms, "algorithmic_bytes": b, "bytes_per_s": b / (ms * 1e-3),
                                "share_of_hbm_peak": b / (ms * 1e-3) / HBM_PEAK}
        print(f"{name}: {ms:.3f} ms ({b / (ms * 1e-3) / 1e12:.2f} TB/s algorithmic, {100 * b / (ms * 1e-3) / HBM_PEAK:.1f}% of 8 TB/s)",
              flush=True)
    r = result["rows"]
    result["full_over_model"] = (r["band_gains"]["kernel_ms"] + r["band_extend"]["kernel_ms"]) / r["resample"]["kernel_ms"]
    print(f"--band full's kernels take {result['full_over_model']:.2f} x the resample of --band model", flush=True)
    result["command"] = "python tools/fullband_bench.py"
    os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
    with open(o.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
