#!/usr/bin/env python
"""Seconds per stage of avsep_amd.score.score_stems on a long recording, and the new correlation kernel against the parent's.

    python tools/score_bench.py [--minutes 10] [--rate 44100] [--sources 2] [--channels 2] [--flen 512] [--win 1.0] [--hop 1.0]

Ten minutes of two stereo sources at 44.1 kHz (coloured noise, mixed estimates) go through score_stems in both filter
modes; the stages of filters="track" (correlations, the two kinds of solve, window energies, track energies) are timed on
their own.  In the same run avsep_bss_corr (bsseval.hip: one lag per thread, two LDS reads per FMA, float64 atomics) is timed
at the identical one-segment shape (B = 1, the rows as pseudo-sources): the same sums as avsep_bss_seg_corr, which forms every
reference pair once.  Measurement bookkeeping only; prints one JSON line at the end."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch                                                                      # noqa: E402


def timed(fn, reps=1):
    """Seconds of the fastest of `reps` runs after one warm-up run, by device events."""
    fn()
    best = float("inf")
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b) / 1e3)
    return best, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=10.0)
    ap.add_argument("--rate", type=int, default=44100)
    ap.add_argument("--sources", type=int, default=2)
    ap.add_argument("--channels", type=int, default=2)
    ap.add_argument("--flen", type=int, default=512)
    ap.add_argument("--win", type=float, default=1.0)
    ap.add_argument("--hop", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--skip_window_mode", action="store_true")
    o = ap.parse_args()
    import avsep_amd                                                              # noqa: F401
    from avsep_amd import score as SC
    from avsep_amd.lib import call, ptr
    dev = torch.device("cuda", 0)
    S, C, flen = o.sources, o.channels, o.flen
    Pn, L = S * C, int(round(o.minutes * 60 * o.rate))
    win, hop = int(round(o.win * o.rate)), int(round(o.hop * o.rate))
    g = torch.Generator(device=dev).manual_seed(0)
    refs = torch.randn((Pn, L), dtype=torch.float64, device=dev, generator=g)
    refs[:, 1:] += 0.6 * refs[:, :-1].clone()
    mix = torch.eye(Pn, dtype=torch.float64, device=dev) + 0.2 * torch.randn((Pn, Pn), dtype=torch.float64, device=dev, generator=g)
    ests = mix @ refs + 0.03 * torch.randn((Pn, L), dtype=torch.float64, device=dev, generator=g)
    starts, wlen = SC.plan_windows(L, win, hop)
    res = {"shape": {"S": S, "C": C, "L": L, "flen": flen, "win": win, "hop": hop, "windows": len(starts)}}

    # the stages of filters="track"
    t_corr, (R, D) = timed(lambda: SC.seg_corr(refs, ests, flen, [0], L), o.reps)
    t_all, C_all = timed(lambda: SC.solve_groups(R, D, Pn, flen), o.reps)
    t_own, C_own = timed(lambda: SC.solve_groups(R, D, C, flen), o.reps)
    t_win, _ = timed(lambda: SC.window_energies(refs, ests, C, flen, [0], L, C_all, C_own, [0] * len(starts), starts, wlen), o.reps)
    t_trk, _ = timed(lambda: SC.window_energies(refs, ests, C, flen, [0], L, C_all, C_own, [0], [0], L + flen - 1), o.reps)
    res["track_stages_s"] = {"seg_corr": t_corr, "solve_all": t_all, "solve_own": t_own, "window_energies": t_win, "track_energies": t_trk}

    # the parent's kernel for the same sums: B = 1, the rows as pseudo-sources
    Rp = torch.empty((1, Pn, Pn, 2 * flen - 1), dtype=torch.float64, device=dev)
    Dp = torch.empty((1, Pn, Pn, flen), dtype=torch.float64, device=dev)
    t_par, _ = timed(lambda: call("avsep_bss_corr", ptr(refs), ptr(ests), 1, Pn, Pn, L, flen, ptr(Rp), ptr(Dp)), o.reps)
    res["parent_bss_corr_s"] = t_par
    res["corr_speedup"] = t_par / t_corr
    res["corr_max_rel_diff"] = max(((R[0] - Rp[0]).abs().max() / Rp.abs().max()).item(), ((D[0] - Dp[0]).abs().max() / Dp.abs().max()).item())
    fma = (Pn * (Pn + 1) // 2 * (2 * flen - 1) + Pn * Pn * flen) * L
    res["seg_corr_tfma_per_s"] = fma / t_corr / 1e12

    r3 = refs.reshape(S, C, L)
    e3 = ests.reshape(S, C, L)
    for mode in ("track",) + (() if o.skip_window_mode else ("window",)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = SC.score_stems(r3, e3, win, hop, mode, flen)
        torch.cuda.synchronize()
        res[f"score_stems_{mode}_s"] = time.perf_counter() - t0
        res[f"{mode}_medians_db"] = {k: [round(v, 3) for v in out[k].tolist()] for k in ("sdr", "isr", "sir", "sar")}
    for k, v in res.items():
        print(k, v)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
