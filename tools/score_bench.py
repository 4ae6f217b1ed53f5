#!/usr/bin/env python
"""Seconds per stage of avsep_amd.score.score_stems on a long recording, and of avsep_amd.bss_eval.bss_eval_sources on a batch.

    python tools/score_bench.py [--minutes 10] [--rate 44100] [--sources 2] [--channels 2] [--flen 512] [--win 1.0] [--hop 1.0]
                                [--batch 8 --len 65535] [--reps 5]

Ten minutes of two stereo sources at 44.1 kHz (coloured noise, mixed estimates) go through score_stems in both filter
modes; the stages of filters="track" (correlations, the two kinds of solve, window energies, track energies) are timed on
their own.  With --batch B, a [B, --sources, --len] mono batch goes through bss_eval_sources and through its stages (the same
kernels on the batch-as-segments layout).  Every figure is the median of --reps timed calls after one warm-up call, by device
events, with the spread (max - min) of those calls beside it.  Measurement bookkeeping only; prints one JSON line at the end."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch                                                                      # noqa: E402


def timed(fn, reps):
    """({"median_s", "spread_s"} of `reps` runs after one warm-up run, by device events; the last result)."""
    out = fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) / 1e3)
    return {"median_s": statistics.median(ts), "spread_s": max(ts) - min(ts)}, out


def inputs(shape, dev, seed):
    """Coloured sources [..., P, L] and estimates from a random mixing matrix over the rows plus 3 % noise."""
    g = torch.Generator(device=dev).manual_seed(seed)
    Pn = shape[-2]
    refs = torch.randn(shape, dtype=torch.float64, device=dev, generator=g)
    refs[..., 1:] += 0.6 * refs[..., :-1].clone()
    mix = torch.eye(Pn, dtype=torch.float64, device=dev) + 0.2 * torch.randn((Pn, Pn), dtype=torch.float64, device=dev, generator=g)
    return refs, mix @ refs + 0.03 * torch.randn(shape, dtype=torch.float64, device=dev, generator=g)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=10.0)
    ap.add_argument("--rate", type=int, default=44100)
    ap.add_argument("--sources", type=int, default=2)
    ap.add_argument("--channels", type=int, default=2)
    ap.add_argument("--flen", type=int, default=512)
    ap.add_argument("--win", type=float, default=1.0)
    ap.add_argument("--hop", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip_window_mode", action="store_true")
    ap.add_argument("--batch", type=int, default=0, help="time bss_eval_sources on [batch, sources, len] instead of score_stems")
    ap.add_argument("--len", type=int, default=65535)
    o = ap.parse_args()
    import avsep_amd                                                              # noqa: F401
    from avsep_amd import bss_eval as PB, score as SC
    dev = torch.device("cuda", 0)
    S, C, flen = o.sources, o.channels, o.flen

    if o.batch:
        B, L = o.batch, o.len
        refs, ests = inputs((B, S, L), dev, 0)
        res = {"shape": {"B": B, "S": S, "L": L, "flen": flen}}
        res["bss_eval_sources"], (sdr, sir, sar) = timed(lambda: PB.bss_eval_sources(refs, ests, flen), o.reps)
        rr, er = (x.transpose(0, 1).reshape(S, B * L).contiguous() for x in (refs, ests))
        seg = [b * L for b in range(B)]
        st = res["stages"] = {}
        st["seg_corr"], (R, D) = timed(lambda: SC.seg_corr(rr, er, flen, seg, L), o.reps)
        st["solve_all"], C_all = timed(lambda: SC.solve_groups(R, D, S, flen), o.reps)
        st["solve_own"], C_own = timed(lambda: SC.solve_groups(R, D, 1, flen), o.reps)
        st["energies"], _ = timed(lambda: SC.window_energies(rr, er, 1, flen, seg, L, C_all, C_own, range(B), [0] * B, L + flen - 1), o.reps)
        res["sample0_db"] = {"sdr": sdr[0].tolist(), "sir": sir[0].tolist(), "sar": sar[0].tolist()}
    else:
        Pn, L = S * C, int(round(o.minutes * 60 * o.rate))
        win, hop = int(round(o.win * o.rate)), int(round(o.hop * o.rate))
        refs, ests = inputs((Pn, L), dev, 0)
        starts, wlen = SC.plan_windows(L, win, hop)
        res = {"shape": {"S": S, "C": C, "L": L, "flen": flen, "win": win, "hop": hop, "windows": len(starts)}}

        # the stages of filters="track"
        st = res["track_stages"] = {}
        st["seg_corr"], (R, D) = timed(lambda: SC.seg_corr(refs, ests, flen, [0], L), o.reps)
        st["solve_all"], C_all = timed(lambda: SC.solve_groups(R, D, Pn, flen), o.reps)
        st["solve_own"], C_own = timed(lambda: SC.solve_groups(R, D, C, flen), o.reps)
        st["window_energies"], _ = timed(lambda: SC.window_energies(refs, ests, C, flen, [0], L, C_all, C_own, [0] * len(starts), starts, wlen),
                                         o.reps)
        st["track_energies"], _ = timed(lambda: SC.window_energies(refs, ests, C, flen, [0], L, C_all, C_own, [0], [0], L + flen - 1), o.reps)
        fma = (Pn * (Pn + 1) // 2 * (2 * flen - 1) + Pn * Pn * flen) * L
        res["seg_corr_tfma_per_s"] = fma / st["seg_corr"]["median_s"] / 1e12

        r3, e3 = refs.reshape(S, C, L), ests.reshape(S, C, L)
        for mode in ("track",) + (() if o.skip_window_mode else ("window",)):
            res[f"score_stems_{mode}"], out = timed(lambda: SC.score_stems(r3, e3, win, hop, mode, flen), o.reps)
            res[f"{mode}_medians_db"] = {k: [round(v, 3) for v in out[k].tolist()] for k in ("sdr", "isr", "sir", "sar")}
    for k, v in res.items():
        print(k, v)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
