"""Score separated stems against their references: windowed image-form BSS-eval (SDR / ISR / SIR / SAR).

    python -m avsep_amd.score --ref a.wav b.wav --est sep/source0.wav sep/source1.wav \
        [--win 1.0 --hop 1.0 --filters track|window --flen 512 --json scores.json]

The reference scores 6 s mono training batches with mir_eval's bss_eval_sources (main.py:260-266; bss_eval.py here).  Music
stems are conventionally scored with the image form of the same decomposition (Vincent et al. 2006, `bss_decomp_mtifilt`):
every estimate channel is projected, by least squares, on `flen` delayed copies of (a) the channels of its own true source
and (b) the channels of all true sources; with rows q = source * C + channel, s = r_q zero-padded by flen - 1,

    e_spat = p_own - s      e_interf = p_all - p_own      e_artif = e_q - p_all

and, energies summed over the channels of a source and a sample range T,

    SDR = 10 log10  sum s^2 / sum (e_q - s)^2             ISR = 10 log10  sum s^2 / sum e_spat^2
    SIR = 10 log10  sum (s + e_spat)^2 / sum e_interf^2   SAR = 10 log10  sum p_all^2 / sum e_artif^2

taken in short windows, the median over windows reported.  filters="track" fits one set of filters on the whole recording
and scores every window (and the whole padded recording: "track") with it; filters="window" fits every window on its own
(one full-length window at C = 1 is bss_eval_sources' SIR and SAR, and runs the same code).  Everything is float64 on the GPU
through the three entry points of csrc/bss_windows.hip, whose host layer is bss_eval.py: lagged correlations read in place (no
window is copied), a dense LU per (segment, source group), and the two FIR projections with their residual energies (no
projected waveform is stored); exactly singular Gram matrices (dual-mono: a mono file saved as stereo) take its host
least-squares path.  Here: window planning, the permutation, silence, the medians and the command line.
"""
import argparse
import itertools
import json
import math

import numpy as np
import torch

from . import lib
from .bss_eval import (MAX_ROWS, MAX_UNKNOWNS, TERMS, _gram, _i64, check_limits, seg_corr, segment_energies,      # noqa: F401
                       solve_groups, window_energies)
from .lib import AvsepError


def plan_windows(L, win, hop):
    """-> (window starts, window length): window w covers [w * hop, w * hop + win), w = 0 ... (L - win) // hop; a remainder
    is dropped; a signal shorter than one window is one window, the whole signal."""
    if win < 1 or hop < 1:
        raise AvsepError(f"win and hop are positive sample counts, got win={win} hop={hop}")
    if L < win:
        return [0], L
    return [w * hop for w in range((L - win) // hop + 1)], win


def best_permutation(sdr_db):
    """sdr_db[i][j]: plain track SDR (dB) of estimate i against reference j.  -> perm with perm[j] = the estimate scored
    against reference j, the one with the largest mean; the lexicographically first on ties."""
    S = len(sdr_db)
    best, best_mean = None, None
    for perm in itertools.permutations(range(S)):
        m = sum(float(sdr_db[perm[j]][j]) for j in range(S)) / S
        if best is None or m > best_mean:
            best, best_mean = perm, m
    return list(best)


def _scores(sums, S):
    """[..., S, 8] -> sdr, isr, sir, sar [...] in dB."""
    db = lambda a, b: 10 * torch.log10(a / b)                              # noqa: E731
    sdr, isr = db(sums[..., 0], sums[..., 1]), db(sums[..., 0], sums[..., 2])
    sir = db(sums[..., 3], sums[..., 4]) if S > 1 else torch.full_like(sdr, math.inf)
    return sdr, isr, sir, db(sums[..., 5], sums[..., 6])


def _silent_windows(refs, ests, starts, wlen):
    """[W] bool: some reference source or some estimate has exactly zero energy over all its channels inside the window."""
    silent = torch.zeros((len(starts),), dtype=torch.bool, device=refs.device)
    a = _i64(starts, refs.device)
    for x in (refs, ests):
        nz = ((x * x) != 0).any(1).to(torch.int64)                            # [S, L]
        cs = torch.nn.functional.pad(nz.cumsum(1), (1, 0))
        silent |= ((cs[:, a + wlen] - cs[:, a]) == 0).any(0)
    return silent


def _median(frames, S, name):
    if name == "sir" and S == 1:
        return torch.full((S,), math.inf, dtype=torch.float64, device=frames.device)
    return torch.nanquantile(frames, 0.5, dim=1)          # the mean of the two middle windows when their count is even


def score_stems(refs, ests, win, hop, filters="track", flen=512, permute=True):
    """refs, ests: [S, C, L] (or [S, L]: C = 1) tensors on the GPU; win, hop in samples.  -> dict:
    "perm" (perm[j] = the estimate scored against reference j), "sdr" / "isr" / "sir" / "sar" [S] (nanmedian over windows),
    "frames" {the four names: [S, W]}, "window_starts", and with filters="track" "track" {the four names: [S]}.

    With permute=True the estimates are matched to the references by the permutation with the largest mean track-level
    PLAIN SDR, sum s_j^2 / sum (e_i - s_j)^2 over the whole recording (S^2 energy sums, no extra solve; the first
    permutation in lexicographic order on ties).  This is deliberately simpler than mir_eval, which solves every
    (estimate, reference) pair and takes the permutation with the largest mean SIR.
    A window in which a reference source or an estimate is exactly silent is NaN for every source and metric."""
    lib.require_gpu(refs)
    lib.require_gpu(ests)
    if filters not in ("track", "window"):
        raise AvsepError(f"filters is 'track' or 'window', got {filters!r}")
    if refs.dim() == 2:
        refs = refs[:, None]
    if ests.dim() == 2:
        ests = ests[:, None]
    if refs.dim() != 3 or refs.shape != ests.shape:
        raise AvsepError(f"refs and ests are [S, C, L] of one shape, got {tuple(refs.shape)} and {tuple(ests.shape)}")
    S, C, L = refs.shape
    check_limits(S, C, flen)
    if L < 1:
        raise AvsepError("score_stems needs at least one sample")
    starts, wlen = plan_windows(L, int(win), int(hop))
    refs, ests = refs.double().contiguous(), ests.double().contiguous()
    P, W, dev = S * C, len(starts), refs.device

    perm = list(range(S))
    if permute and S > 1:
        es = (refs * refs).sum((1, 2))
        plain = [[(10 * torch.log10(es[j] / ((ests[i] - refs[j]) ** 2).sum())).item() for j in range(S)] for i in range(S)]
        perm = best_permutation(plain)
        if perm != list(range(S)):
            ests = ests[perm].contiguous()
    rr, er = refs.reshape(P, L), ests.reshape(P, L)
    silent = _silent_windows(refs, ests, starts, wlen)
    out = {"perm": perm, "window_starts": list(starts)}
    frames = torch.full((W, S, TERMS), math.nan, dtype=torch.float64, device=dev)

    if filters == "track":
        R, D = seg_corr(rr, er, flen, [0], L)
        C_all, C_own = solve_groups(R, D, P, flen), solve_groups(R, D, C, flen)
        frames = window_energies(rr, er, C, flen, [0], L, C_all, C_own, [0] * W, starts, wlen)
        track = window_energies(rr, er, C, flen, [0], L, C_all, C_own, [0], [0], L + flen - 1)[0]
        out["track"] = dict(zip(("sdr", "isr", "sir", "sar"), _scores(track, S)))
    else:
        live = [w for w, z in enumerate(silent.tolist()) if not z]                 # silent windows are not solved
        if live:
            frames[live] = segment_energies(rr, er, C, flen, [starts[w] for w in live], wlen)
    frames[silent] = math.nan
    names = ("sdr", "isr", "sir", "sar")
    out["frames"] = {k: v.t().contiguous() for k, v in zip(names, _scores(frames, S))}      # [S, W]
    if S == 1:
        out["frames"]["sir"][:, silent] = math.nan
    for k in names:
        out[k] = _median(out["frames"][k], S, k)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------------------------------------------------
def build_parser():
    p = argparse.ArgumentParser(prog="python -m avsep_amd.score",
                                description="Score separated stems against their references: windowed SDR / ISR / SIR / SAR "
                                            "(image-form BSS-eval, median over windows).")
    p.add_argument("--ref", nargs="+", required=True, help="the true stems, one WAV per source (16-, 24- or 32-bit PCM or 32-bit float)")
    p.add_argument("--est", nargs="+", required=True, help="the separated stems, as many files (matched to --ref by plain SDR)")
    p.add_argument("--win", type=float, default=1.0, help="window length in seconds")
    p.add_argument("--hop", type=float, default=1.0, help="seconds between window starts")
    p.add_argument("--filters", choices=("track", "window"), default="track",
                   help="track: one set of distortion filters for the recording (default); window: one per window")
    p.add_argument("--flen", type=int, default=512, help="taps of the distortion filters")
    p.add_argument("--json", default=None, help="write the scores (medians, per-window frames, track) to this file")
    return p


def parse_args(argv=None):
    args = build_parser().parse_args(argv)
    if len(args.ref) != len(args.est):
        raise SystemExit(f"--ref names {len(args.ref)} files and --est {len(args.est)}: one estimate per reference")
    if args.win <= 0 or args.hop <= 0:
        raise SystemExit("--win and --hop are positive numbers of seconds")
    return args


def read_stems(ref_paths, est_paths):
    """-> (refs, ests: float64 numpy [S, C, L] in [-1, 1), rate).  All files share one rate and one channel count (nothing is
    resampled or down-mixed here); the lengths are trimmed to the shortest file."""
    from . import wavio
    paths = list(ref_paths) + list(est_paths)
    data = []
    for path in paths:                               # every format decodes to its exact values on the host (wavio.decode)
        try:
            raw, info = wavio.read_frames(path)
        except AvsepError as e:
            raise SystemExit(str(e))
        data.append((wavio.decode(raw, info.fmt, info.channels), info.rate))
    rate, ch = data[0][1], data[0][0].shape[1]
    for path, (pcm, r) in zip(paths, data):
        if r != rate:
            raise SystemExit(f"{path}: sample rate {r} Hz, but {paths[0]} has {rate} Hz: the scorer does not resample, "
                             "bring the files to one rate first")
        if pcm.shape[1] != ch:
            raise SystemExit(f"{path}: {pcm.shape[1]} channel(s), but {paths[0]} has {ch}: all stems need one channel count")
    L = min(pcm.shape[0] for pcm, _ in data)
    if L < 1:
        raise SystemExit("the shortest file is empty")
    x = np.stack([pcm[:L].T for pcm, _ in data])                                             # [2 S, C, L]
    return x[:len(ref_paths)], x[len(ref_paths):], rate


def _jsonable(t):
    """Strict JSON has no NaN / Infinity: a silent window is null, an infinite ratio the string "inf" / "-inf"."""
    one = lambda v: None if math.isnan(v) else (v if math.isfinite(v) else str(v))      # noqa: E731
    return [[one(v) for v in row] for row in t.tolist()] if t.dim() == 2 else [one(v) for v in t.tolist()]


def cli(argv=None):
    args = parse_args(argv)
    refs, ests, rate = read_stems(args.ref, args.est)
    try:
        check_limits(refs.shape[0], refs.shape[1], args.flen)
    except AvsepError as e:
        raise SystemExit(str(e))
    if not torch.cuda.is_available():
        raise AvsepError("scoring runs on an MI355X; there is no CPU fallback")
    dev = torch.device("cuda", 0)
    win, hop = max(1, int(round(args.win * rate))), max(1, int(round(args.hop * rate)))
    res = score_stems(torch.from_numpy(refs).to(dev), torch.from_numpy(ests).to(dev), win, hop, args.filters, args.flen)
    names = ("sdr", "isr", "sir", "sar")
    for j, path in enumerate(args.ref):
        line = "  ".join(f"{k.upper()} {res[k][j].item():7.2f} dB" for k in names)
        print(f"source {j} ({path} <- {args.est[res['perm'][j]]}): {line}")
    if args.json:
        doc = {"rate": rate, "win": win, "hop": hop, "filters": args.filters, "flen": args.flen, "perm": res["perm"],
               "window_starts": res["window_starts"]}
        doc.update({k: _jsonable(res[k]) for k in names})
        doc["frames"] = {k: _jsonable(res["frames"][k]) for k in names}
        if "track" in res:
            doc["track"] = {k: _jsonable(res["track"][k]) for k in names}
        with open(args.json, "w") as f:
            json.dump(doc, f, allow_nan=False)
    return res


if __name__ == "__main__":
    cli()
