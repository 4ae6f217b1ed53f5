"""Separate a recording of any length (the reference stops at one 65 535-sample tile: SURVEY.md §5.7; its glue for
one tile is main.py:205-246 / inference.py:433-475).

The recording gets ONE STFT.  Its spectrogram is cut into overlapping windows of 256 frames (``plan_windows``), all
windows are warped straight out of the recording (``avsep_window_prepare``) and go through the eval-mode U-Net as a
batch.  The warped masks are un-warped, cross-faded with a triangular weight on the recording's linear-frequency grid
and multiplied with the mixture magnitude in one kernel (``avsep_mask_stitch``); ONE iSTFT per source with the whole
recording's phase gives the waveforms.  Masks, not waveforms, are stitched: a per-chunk iSTFT has its own centre padding
and window-sum-square normalisation at both ends, the grid_sample warp damps every tile's edge columns, and neither
shows up when the blend happens before a single inverse transform.  A recording of one tile reduces to
``evaluate.reconstruct``.

Without frames the model has no fixed source order (permutation-invariant training plus a random swap per sample), so
for ``use_vis=False`` the swap draw is pinned to "no swap" and consecutive windows are aligned on the frames they share
(``avsep_window_agreement`` + ``align_permutations``) before blending.

CLI: ``python -m avsep_amd.separate --wav mix.wav --frames a.npy b.npy [--fps 8] --id <experiment> --out dir`` (flag set of
arguments.py; 16-, 24- or 32-bit PCM or 32-bit float WAV at any rate, read by wavio.py: a file that is not at ``--audRate``
is resampled on the GPU, resample.py, and the sources are written at the file's rate unless ``--out_rate model``, in the
file's sample format unless ``--out_format`` names another).

The model is trained on mono and always sees the down-mix.  With ``channels`` (``--channels keep``) the one blended mask is
also applied to each channel's own magnitude (``avsep_mask_stitch`` with C channels) and inverted with that channel's own phase,
so a stereo file gives stereo sources.  ``wiener=k`` (``--wiener k``) then runs k passes of a multichannel Wiener filter
(``kernels.mwf``) over those source images: the masked channels give every source a spatial covariance per bin, and each
time-frequency bin of the mixture is filtered again with them, so a source keeps its own place in the stereo image.
``wiener_span=H`` (``--wiener_span H``) estimates those covariances locally, around centres H frames apart, and blends the
two next to every frame: for sources that move through the image over the recording.

A masked magnitude on the mixture's phase is not the STFT of any signal.  ``phase_iters=k`` (``--phase_iters k``) runs k
mixture-consistent phase iterations (MISI, ``kernels.Stft.misi``) in place of the one inverse transform: every stem gets a
phase of its own under the magnitude it was given.  The gain grows with the quality of the magnitudes; thresholded
(binary) masks gain nothing from it.

A filmed recording brings a clip, not a frame.  With ``frame_times`` (``--fps``, the flags of localise) every video frame is
put on the recording's time axis, goes through the visual trunk once, and every window is separated with the mean feature of
the frames that fall into it (``frames_of_windows``, ``avsep_window_reduce``): what training's forward_multiframe feeds the
fusion.  One frame list for two sources is a duet, one camera on both players.
"""
import itertools
import math
import os
import wave

import numpy as np
import torch

from . import kernels as K
from . import lib
from .lib import AvsepError
from .models import activate

WIDTH = 256        # frames per window: the tile the network is trained on
MAX_WIENER = 8     # passes of the multichannel Wiener filter a call may ask for
MAX_PHASE_ITERS = 32   # mixture-consistent phase iterations a call may ask for
FOUT = 256         # log-frequency bins of the warped tile (inference.py:48-51)


def plan_windows(F, stride, width=WIDTH):
    """Start frames of the windows over F frames: 0, stride, 2*stride, ... while a window ends before F, then one last
    window right-aligned at F - width.  One window [0] when F <= width.  Strictly ascending."""
    F, stride, width = int(F), int(stride), int(width)
    if F < 1 or width < 1 or not 1 <= stride <= width:
        raise ValueError(f"plan_windows needs F >= 1 and 1 <= stride <= width, got F={F} stride={stride} width={width}")
    starts, s = [], 0
    while s + width < F:
        starts.append(s)
        s += stride
    starts.append(max(0, F - width))
    return starts


def align_permutations(D):
    """D [K-1,N,N] (``kernels.window_agreement``, any device) -> int32 [K,N] on the CPU: row k lists, per output source,
    the channel of window k that carries it.  Window 0 is the identity; window k+1 takes the permutation p of its
    channels with the least sum_n D[k, perm[k][n], p[n]] (all N! candidates in itertools.permutations order, the first
    wins a tie — as PitWrapper does)."""
    D = torch.as_tensor(D).detach().cpu().double()
    if D.dim() != 3 or D.shape[1] != D.shape[2]:
        raise ValueError(f"align_permutations takes [K-1,N,N], got {tuple(D.shape)}")
    N = D.shape[1]
    if not 1 <= N <= 3:
        raise ValueError("align_permutations enumerates N! candidates: N <= 3")
    cands = list(itertools.permutations(range(N)))
    perms = [list(range(N))]
    for k in range(D.shape[0]):
        cur, best, best_cost = perms[-1], None, None
        for p in cands:
            cost = sum(D[k, cur[n], p[n]].item() for n in range(N))
            if best is None or cost < best_cost:
                best, best_cost = p, cost
        perms.append(list(best))
    return torch.tensor(perms, dtype=torch.int32)


def frame_columns(frame_times, starts, rate, hop, width=WIDTH, who="frame_columns"):
    """The STFT column of every video frame -> int64 [T] (NumPy).  frame_times: seconds from the start of the recording;
    starts: plan_windows' start columns.  A frame at t lies at column c = floor(t * rate / hop + 0.5) (columns are centred on
    j * hop; halves round up), clamped to the recording's columns [0, starts[-1] + width - 1].  The one rule both
    ``localise.window_of_frames`` and ``frames_of_windows`` place frames by; ``who`` names the caller in the errors."""
    t = np.asarray(torch.as_tensor(frame_times).detach().cpu().numpy(), dtype=np.float64).reshape(-1)    # float64 in: no copy
    s = np.asarray(list(starts), dtype=np.int64)
    if s.size < 1 or (np.diff(s) <= 0).any() or s[0] < 0:
        raise ValueError(f"{who} needs ascending window starts, got {list(starts)}")
    if not np.isfinite(t).all():
        raise ValueError(f"{who} needs finite frame times")
    return np.clip(np.floor(t * float(rate) / float(hop) + 0.5).astype(np.int64), 0, int(s[-1]) + int(width) - 1)


def frames_of_windows(frame_times, starts, rate, hop, width=WIDTH):
    """The video frames every window is separated with -> int32 [K,2] (CPU), row k = (first, count): the contiguous run of
    frames whose column c (``frame_columns``) lies in starts[k] <= c < starts[k] + width.  frame_times [T], T >= 1, finite and
    non-decreasing (else ValueError), which is what makes the run contiguous; they are taken as float64 (a Python list too).
    A window that holds no frame gets the ONE frame whose column is nearest to its centre, |2 * starts[k] + width - 2 * c| in
    doubled integer units as ``localise.window_of_frames`` measures it, the lower index on a tie.  Every row has count >= 1,
    0 <= first and first + count <= T."""
    t = torch.as_tensor(frame_times, dtype=torch.float64).detach().cpu().numpy().reshape(-1)     # once, in float64
    c = frame_columns(t, starts, rate, hop, width, who="frames_of_windows")
    if t.size < 1:
        raise ValueError("frames_of_windows needs at least one frame")
    if (np.diff(t) < 0).any():
        raise ValueError("frames_of_windows needs non-decreasing frame times")
    s = np.asarray(list(starts), dtype=np.int64)
    first = np.searchsorted(c, s, side="left")
    count = np.searchsorted(c, s + int(width), side="left") - first
    empty = count == 0
    if empty.any():
        dist = np.abs(2 * s[empty, None] + int(width) - 2 * c[None, :])          # twice the distance: integers
        first[empty] = np.argmin(dist, axis=1)                                   # the first minimum: the lower index
        count[empty] = 1
    return torch.from_numpy(np.stack([first, count], 1).astype(np.int32))


def is_shot(fr):
    """Frames as shot: a uint8 tensor, [T,H,W,3] RGB (prepared frames are floats [T,3,H,W])."""
    return torch.is_tensor(fr) and fr.dtype == torch.uint8


def trunk_features(net_frame, fr, batch, dev, pool, activation=None, img_size=None):
    """fr [T,3,H,W] through the visual trunk, ``batch`` frames at a time (each batch is moved to ``dev``, as float32) ->
    the features of all T frames, concatenated.  activation: applied to every batch's features (img_activation); None
    leaves it out.  fr uint8 [T,H,W,3], frames as shot: every batch goes to ``dev`` as the bytes it is and is prepared there
    (``frames.prepare``, the validation form at ``img_size``, which is then required).  The one trunk loop of
    ``separate_long`` (frames and clips) and of ``localise``."""
    parts, shot = [], None
    if is_shot(fr):
        from . import frames as FR
        if img_size is None:
            raise AvsepError("uint8 frames are prepared at args.imgSize, which these args do not have")
        shot = FR.plan(FR.check_stack(fr, "separate_long / localise")[1], fr.shape[2], img_size)
    for i in range(0, fr.shape[0], batch):
        x = fr[i:i + batch].to(dev)
        f = net_frame.forward(x.float().contiguous() if shot is None else FR.prepare(x.contiguous(), shot), pool=pool)
        parts.append(f if activation is None else activate(f, activation))
    return parts[0] if len(parts) == 1 else torch.cat(parts, 0)


def _visual_features(net_frame, frames, args, Kw, batch, act=True):
    """One feature tensor per source: [1,...] for a frame shared by all windows, [K,...] for one frame per window.
    act=False (the duet) leaves img_activation out."""
    feats = []
    for n, fr in enumerate(frames):
        if fr.dim() != 4 or fr.shape[0] not in (1, Kw):
            raise AvsepError(f"frames[{n}] must be [1,3,H,W] or [{Kw},3,H,W] (one per window; uint8 frames as shot: "
                             f"[1,H,W,3] or [{Kw},H,W,3]), got {tuple(fr.shape)}")
        if is_shot(fr) != is_shot(frames[0]):
            raise AvsepError(f"frames must be of one kind, all uint8 as shot or all prepared floats; frames[{n}] is {fr.dtype}, "
                             f"frames[0] {frames[0].dtype}")
        lib.require_gpu(fr)
        feats.append(trunk_features(net_frame, fr, batch, fr.device, args.not_pool_vis, args.img_activation if act else None,
                                    getattr(args, "imgSize", None)))
    return feats


def _clip_features(net_frame, frames, frame_times, starts, args, batch, dev, act=True):
    """One feature tensor [K,...] per source from a clip: every frame goes through the trunk once, ``batch`` at a time (a
    stack on the CPU is moved batch by batch), and every window gets the mean of its frames' features (``frames_of_windows``,
    ``kernels.window_reduce``) before img_activation: forward_multiframe's mean, then the activation, the order of
    main.py:119-122.  act=False (the duet) leaves the activation out.  Pooled features (args.not_pool_vis) are refused: the
    fusion takes spatial maps only."""
    if args.not_pool_vis:
        raise AvsepError("separate_long(frame_times=...) needs a spatial visual feature map: the fusion does not take pooled "
                         "features (not_pool_vis); kernels.window_reduce(op='max' | 'mean') reduces pooled vectors on its own")
    times = torch.as_tensor(frame_times, dtype=torch.float64).reshape(-1)
    T = frames[0].shape[0] if torch.is_tensor(frames[0]) and frames[0].dim() == 4 else 0
    for n, fr in enumerate(frames):
        if not torch.is_tensor(fr) or fr.dim() != 4 or fr.shape[3 if is_shot(fr) else 1] != 3 \
                or tuple(fr.shape) != tuple(frames[0].shape) or fr.dtype != frames[0].dtype:
            raise AvsepError(f"with frame_times, frames[{n}] must be [T,3,H,W] (or uint8 [T,H,W,3]) like frames[0], "
                             f"got {lib.got(fr)}")
    if T < 1 or times.numel() != T:
        raise AvsepError(f"separate_long needs one time per video frame: {T} frames, {times.numel()} times")
    try:
        ranges = frames_of_windows(times, starts, args.audRate, args.stft_hop, WIDTH)
    except ValueError as e:
        raise AvsepError(f"separate_long(frame_times=...): {e}") from e
    feats = []
    for fr in frames:
        w = K.window_reduce(trunk_features(net_frame, fr, batch, dev, False, None, getattr(args, "imgSize", None)).float().contiguous(),
                            ranges, "mean")
        feats.append(activate(w, args.img_activation) if act else w)
    return feats


def _check_filter(channels, wiener, phase_iters, wiener_span):
    """separate_long's checks of the arguments that need neither the recording, nor ``args``, nor the nets: they run first."""
    if isinstance(wiener, bool) or not isinstance(wiener, int) or not 0 <= wiener <= MAX_WIENER:
        raise AvsepError(f"separate_long takes wiener as an int in 0 ... {MAX_WIENER} (passes of the multichannel Wiener filter), got {wiener!r}")
    if isinstance(phase_iters, bool) or not isinstance(phase_iters, int) or not 0 <= phase_iters <= MAX_PHASE_ITERS:
        raise AvsepError(f"separate_long takes phase_iters as an int in 0 ... {MAX_PHASE_ITERS} (mixture-consistent phase iterations), got {phase_iters!r}")
    if wiener and channels is None:
        raise AvsepError("separate_long(wiener=...) filters the recording's channels: pass channels= as well")
    K.mwf_span_check("separate_long(wiener_span=...)", wiener_span)
    if wiener_span and not wiener:
        raise AvsepError("separate_long(wiener_span=...) is the span of the Wiener filter's covariances: it needs wiener >= 1")


def _check_inputs(nets, wav, frames, args, use_vis, channels, return_maps):
    """separate_long's checks of the recording, its channels, the nets and the frame list -> whether the call is a duet."""
    net_sound, net_frame = nets
    lib.require_gpu(wav)
    if wav.dim() != 1 or wav.numel() < args.stft_frame:
        raise AvsepError(f"separate_long takes one recording [L] with L >= stft_frame, got {tuple(wav.shape)}")
    if channels is not None:
        if not torch.is_tensor(channels) or channels.dtype != torch.float32 or channels.dim() != 2 or channels.shape[0] < 1 \
                or channels.shape[1] != wav.numel() or channels.device != wav.device:
            raise AvsepError(f"separate_long takes channels as float32 [C,{wav.numel()}] on {wav.device} (the recording's "
                             f"channels, as long as wav), got {lib.got(channels)}")
    if net_sound.training or (use_vis and net_frame.training):
        raise AvsepError("separate_long needs the nets in eval(): call .eval() on both before separating")
    if use_vis:
        if args.fusion_type == "MixVis":
            raise NotImplementedError("long-form separation does not provide the MixVis fusion")
        if len(frames) == 1 and args.num_mix != 1:
            if args.num_mix != 2:
                raise AvsepError(f"one frame tensor for all sources is a duet: it needs num_mix == 2, got {args.num_mix}")
        elif len(frames) != args.num_mix:
            raise AvsepError(f"separate_long needs one frame tensor per source ({args.num_mix}), got {len(frames)}")
    if return_maps and (not use_vis or args.not_pool_vis):
        raise AvsepError("separate_long(return_maps=True) returns the fusion's attention maps: it needs frames (use_vis) and a "
                         "spatial visual feature map (pooled features, not_pool_vis, have none)")
    return bool(use_vis) and len(frames) == 1 and args.num_mix == 2


def _window_masks(net_sound, logm, starts_t, feats, args, batch, align, return_maps=False):
    """The windows logm [K,1,256,256] through the U-Net, ``batch`` at a time -> (masks [K,N,256,256] in the network's channel
    order, perms int32 [K,N] on the CPU, maps [K,N,h,w] or None).  feats: one visual feature tensor per source, [1,...]
    (broadcast over the windows) or [K,...]; None is the audio-only branch, whose swap draw is pinned to "no swap" for the
    call.  align: the channel order is the network's own (audio only, the duet), so consecutive windows are aligned on the
    frames they share; else perms is the identity.  return_maps: the fusion's attention maps, maps[k, n] for output source n."""
    Kw, N, dev = logm.shape[0], args.num_mix, logm.device
    masks = torch.empty((Kw, N, FOUT, WIDTH), dtype=torch.float32, device=dev)
    att, pinned = [], net_sound.ao_draws
    try:
        for i in range(0, Kw, batch):
            b, vs = min(batch, Kw - i), None
            if feats is None:        # "no swap" for every window: a bool coin for two sources, permutation index 0 for more
                net_sound.ao_draws = torch.zeros(b, dtype=torch.bool if N == 2 else torch.int64)
            else:
                vs = [(f.expand(b, *f.shape[1:]) if f.shape[0] == 1 else f[i:i + b]).contiguous() for f in feats]
            feat, meta = net_sound(logm[i:i + b], vs)
            if feats is not None:    # every source's channel on its own, as inference.NetWrapper.forward_av
                for n in range(N):
                    masks[i:i + b, n] = activate(feat[:, n].unsqueeze(1), args.output_activation)[:, 0]
            elif feat.shape[1] != N:
                raise AvsepError(f"net_sound gives {feat.shape[1]} channels for num_mix={N}")
            else:
                masks[i:i + b] = activate(feat, args.output_activation)
            if return_maps:
                att.append(meta[1].float())
    finally:
        net_sound.ao_draws = pinned
    if align:
        perms = align_permutations(K.window_agreement(masks, starts_t))
    else:
        perms = torch.arange(N, dtype=torch.int32).repeat(Kw, 1)
    maps = None
    if return_maps:                                                      # maps[k, n]: channel perms[k][n] of window k
        att = att[0] if len(att) == 1 else torch.cat(att, 0)
        maps = att.gather(1, perms.to(dev).long()[:, :, None, None].expand(-1, -1, *att.shape[2:])).contiguous()
    return masks, perms, maps


def _inverse(plan, rows, mags, phases, phase_iters, clamp):
    """The magnitudes mags [N,G,Fin,F] of the N stems of each of the G ``rows`` [G,L] -> their waveforms [N,G,hop*(F-1)]: one
    iSTFT over the N*G rows, or ``phase_iters`` mixture-consistent iterations against the rows.  phases: [G,Fin,F], the rows'
    own, shared by their stems, or [N,G,Fin,F], one per stem (the Wiener filter's).  clamp: to [-1,1].  The mono path is
    G = 1 with the down-mix as the one row."""
    N, G, Fin, Fr = mags.shape
    if phase_iters:                                                      # every row is the mixture of its N stems
        out = plan.misi(rows[:, :plan.hop * (Fr - 1)], mags, phases, phase_iters)
    else:
        if phases.dim() == 3:
            phases = phases[None].expand(N, -1, -1, -1).contiguous()
        out = plan.istft(mags.reshape(N * G, Fin, Fr), phases.reshape(N * G, Fin, Fr)).reshape(N, G, -1)
    return out.clamp_(-1.0, 1.0) if clamp else out


def separate_long(nets, wav, frames, args, use_vis=True, stride_frames=128, batch=16, return_masks=False, channels=None,
                  wiener=0, phase_iters=0, clamp=True, wiener_span=0, band_gains=False, frame_times=None, return_maps=False):
    """Separate one recording ``wav`` [L] (on the GPU, L >= args.stft_frame; several recordings: one call each).

    nets: (net_sound, net_frame), both in eval() — train-mode BatchNorm over the windows of one recording is never what
    the caller wants, and raises AvsepError.  frames: list of N tensors, each [1,3,H,W] (one frame for the whole
    recording: its feature map is computed once and broadcast over the windows) or [K,3,H,W] (one frame per window,
    K = len(plan_windows(F, stride_frames))); ignored for use_vis=False.  Activations and ``pool`` as in
    inference.NetWrapper.forward_av.  ``fusion_type == 'MixVis'`` is not provided: NotImplementedError.

    Wherever a frame tensor is a float [T,3,H,W] it may be uint8 [T,H,W,3] instead, RGB frames as shot, of any size: they are
    resized, cropped and normalised on the GPU as dataset.VideoTransform's validation form does at args.imgSize
    (``frames.prepare``, bit for bit), batch by batch inside the trunk loop, so a clip on the host goes up as bytes.  Float
    frames take the path they always took.

    A one-element frames list with num_mix == 2 is a duet (one camera, two players), in any of the frame forms: the one feature
    tensor feeds both sources and, as in inference.NetWrapper and localise, img_activation is not applied to it.  With the same
    map on both sides the fusion's two permutation scores tie and the first wins, so a window's channel order is the network's
    own, as in the audio-only branch: consecutive windows are aligned on the frames they share and "perms" says how.  A
    one-element list with any other num_mix is an AvsepError.

    frame_times: None, or the times [T] of a clip's video frames in seconds from the start of ``wav``, finite and
    non-decreasing.  frames are then N tensors [T,3,H,W] of equal shape (or one, the duet), on the GPU or on the CPU (moved
    ``batch`` frames at a time).  Every frame goes through net_frame once; window k gets the mean of the features of the frames
    that fall into it (``frames_of_windows``; the nearest frame if none does), then img_activation: forward_multiframe's
    mean over a window's frames in place of one frame picked by hand.  Needs args.audRate and spatial visual features: with
    args.not_pool_vis (pooled vectors, which the fusion does not take) it is an AvsepError.  None is the path above, bit for
    bit.

    return_maps: True adds "maps", f32 [K,N,h,w]: the fusion's attention maps of every window, maps[k,n] for output source n
    (channel perms[k][n]).  Needs use_vis and spatial visual features (not args.not_pool_vis): AvsepError otherwise.

    Returns {"wavs": [N, hop*(F-1)] clamped to [-1,1], "starts": list, "perms": int32 [K,N] (CPU)}; with return_masks
    also "masks" [K,N,256,256] (warped, per window, network channel order) and "lin_masks" [N,Fin,F] (blended).

    channels: f32 [C, L] on wav's device, the recording's channels (``wav`` stays the network's input; nothing on the way
    to the masks changes).  The blended mask of every source is then also multiplied into each channel's magnitude and
    inverted with that channel's phase: the result gains "channel_wavs" [N, C, hop*(F-1)], clamped to [-1,1].

    wiener: int in 0 ... 8, passes of the multichannel Wiener filter (``kernels.mwf``, relative regulariser 1e-3) over the
    masked channels before their iSTFT; needs ``channels`` (C = 1 gives the single-channel Wiener gain).  0 is the path
    above, bit for bit.  With wiener >= 1 the channel stitch uses the SOFT mask whatever ``args.binary_mask`` says: the
    filter weighs every source by the power its mask leaves it, and a thresholded mask has thrown that posterior away.
    Each source then gets its own phase (one iSTFT over N*C rows), and the sources of a bin sum to the mixture over
    1 + ~1e-3, not to the mixture exactly.  The covariances are one per bin row for the whole recording (time-invariant)
    unless ``wiener_span`` says otherwise.  "wavs", "perms", "masks" and "lin_masks" do not depend on ``wiener``.

    wiener_span: int, 0 or a multiple of 64 frames in 64 ... 4096; needs wiener >= 1.  0 is the time-invariant filter above,
    bit for bit.  With H > 0 every pass estimates one covariance per bin row and centre (frames 0, H, 2H, ...), each from
    the frames within H of it under a triangular weight, and filters frame t with the blend of the two centres next to it
    (``kernels.mwf(span=H)``): a source that moves through the image is followed instead of smeared over its path.  Fewer
    frames go into each estimate, so sources that stay put lose a few tenths of a dB; 64 ... 128 frames suit pans that cross
    the image within some hundreds of frames.  "wavs", "perms", "masks" and "lin_masks" do not depend on it.

    phase_iters: int in 0 ... 32, mixture-consistent phase iterations (``kernels.Stft.misi``) in place of the one inverse
    transform.  0 is the path above, bit for bit.  With k >= 1 "wavs" are the stitched magnitudes after k passes against
    ``wav[:hop*(F-1)]``, started from the mixture's phase; "channel_wavs" the channel magnitudes after k passes, every
    channel's N stems against that channel, started from the channel's own phase or, with ``wiener``, from the filter's
    magnitudes and per-source phases.  The stems are clamped as before and are not forced to sum to the mixture.
    "perms", "masks" and "lin_masks" do not depend on it.

    clamp: False leaves "wavs" and "channel_wavs" as the inverse transform gives them, overshoots past full scale included
    (levels.py then measures them and rescales instead of clipping).  Nothing else changes.

    band_gains: True adds "band_gains", f32 [N, C, F] with ``channels`` and [N, 1, F] without: per STFT frame the share of the
    mixture's RMS amplitude every source holds over the top octave of the model's band (``kernels.band_gains``), from the
    magnitudes that go into the inverse transform (with ``wiener`` the filtered ones, per channel) against the mixture's.
    ``resample.band_extend`` hands a file's band above the model's to the stems under these gains.  Nothing else changes;
    False is the path above, bit for bit.
    """
    _check_filter(channels, wiener, phase_iters, wiener_span)
    duet = _check_inputs(nets, wav, frames, args, use_vis, channels, return_maps)
    net_sound, net_frame = nets
    dev, binary, thres = wav.device, bool(args.binary_mask), getattr(args, "mask_thres", 0.5)
    with torch.no_grad():
        plan = K.Stft(dev, args.stft_frame, args.stft_hop, getattr(args, "stft_pad_mode", "reflect"))
        mag, phase = plan.stft(wav.float().contiguous()[None])
        mag, phase = mag[0], phase[0]                                    # [Fin, F]
        starts = plan_windows(mag.shape[1], stride_frames, WIDTH)
        starts_t = torch.tensor(starts, dtype=torch.int32, device=dev)
        _, logm = K.window_prepare(mag, starts_t, FOUT, WIDTH)
        feats = None                                                     # audio only
        if use_vis and frame_times is None:
            feats = _visual_features(net_frame, frames, args, len(starts), batch, act=not duet)
        elif use_vis:
            feats = _clip_features(net_frame, frames, frame_times, starts, args, batch, dev, act=not duet)
        if duet:                                                         # the one map on both sides of the fusion
            feats = feats * 2
        masks, perms, maps = _window_masks(net_sound, logm, starts_t, feats, args, batch, duet or not use_vis, return_maps)
        perms_d = perms.to(dev)
        mags, lin = K.mask_stitch(masks, starts_t, perms_d, mag, binary, thres, return_masks)
        wavs = _inverse(plan, wav.float()[None], mags[:, None], phase[None], phase_iters, clamp)[:, 0]
        if band_gains and channels is None:
            gains = K.band_gains(mags[:, None], mag[None])
        if channels is not None:                                         # the same masks on every channel's own STFT
            mag_c, phases_c = plan.stft(channels.contiguous())
            mags_c, _ = K.mask_stitch(masks, starts_t, perms_d, mag_c, binary and not wiener, thres)
            if wiener:                                                   # soft source images in, one phase per source out
                mags_c, phases_c = K.mwf(mag_c, phases_c, mags_c, phases_c, iterations=wiener, span=wiener_span)
            if band_gains:                                               # of what is inverted below: after the filter, per channel
                gains = K.band_gains(mags_c, mag_c)
            channel_wavs = _inverse(plan, channels, mags_c, phases_c, phase_iters, clamp)
    out = {"wavs": wavs, "starts": starts, "perms": perms}
    if channels is not None:
        out["channel_wavs"] = channel_wavs
    if band_gains:
        out["band_gains"] = gains
    if return_masks:
        out.update(masks=masks, lin_masks=lin)
    if return_maps:
        out["maps"] = maps
    return out


# ---------------------------------------------------------------------------------------------------------------------
# 16-bit PCM WAV through the standard library (the host's own statement of what a 16-bit file means: the command lines
# read and write through wavio.py and the kernels), and the command line
# ---------------------------------------------------------------------------------------------------------------------
def read_wav(path):
    """-> (float32 mono waveform in [-1, 1), sample rate).  16-bit PCM only; channels are averaged."""
    with wave.open(path, "rb") as w:
        if w.getsampwidth() != 2 or w.getcomptype() != "NONE":
            raise AvsepError(f"{path}: only uncompressed 16-bit PCM WAV is read (sample width {w.getsampwidth()} bytes)")
        rate, ch = w.getframerate(), w.getnchannels()
        data = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2").astype(np.float32) / 32768.0
    if ch > 1:
        data = data.reshape(-1, ch).mean(1)
    return data, rate


def write_wav(path, data, rate):
    """float waveform in [-1, 1] -> mono 16-bit PCM (x * 32768 rounded, +1.0 clips to 32767: read_wav's inverse)."""
    pcm = np.clip(np.round(np.asarray(data, dtype=np.float64) * 32768.0), -32768, 32767).astype("<i2")
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(int(rate))
        w.writeframes(pcm.tobytes())


def wav_rate(path):
    """The sample rate in the file's header."""
    with wave.open(path, "rb") as w:
        return w.getframerate()


def read_wav_pcm(path):
    """-> (int16 [L, C] frames exactly as they lie in the file, sample rate).  16-bit PCM only; nothing is converted."""
    with wave.open(path, "rb") as w:
        if w.getsampwidth() != 2 or w.getcomptype() != "NONE":
            raise AvsepError(f"{path}: only uncompressed 16-bit PCM WAV is read (sample width {w.getsampwidth()} bytes)")
        rate, ch = w.getframerate(), w.getnchannels()
        data = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2").astype(np.int16)      # a writable copy in native order
    return data.reshape(-1, ch), rate


def write_wav_pcm(path, pcm, rate):
    """int16 mono [L] -> 16-bit PCM WAV, sample for sample."""
    pcm = np.asarray(pcm)
    if pcm.dtype != np.int16 or pcm.ndim != 1:
        raise AvsepError(f"write_wav_pcm takes int16 mono [L], got {pcm.dtype} {pcm.shape}")
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(int(rate))
        w.writeframes(pcm.astype("<i2", copy=False).tobytes())


def write_wav_pcm_channels(path, pcm, rate):
    """int16 [L, C] frames -> 16-bit PCM WAV with C channels, sample for sample (read_wav_pcm's inverse)."""
    pcm = np.asarray(pcm)
    if pcm.dtype != np.int16 or pcm.ndim != 2 or pcm.shape[1] < 1:
        raise AvsepError(f"write_wav_pcm_channels takes int16 frames [L,C], got {pcm.dtype} {pcm.shape}")
    with wave.open(path, "wb") as w:
        w.setnchannels(pcm.shape[1])
        w.setsampwidth(2)
        w.setframerate(int(rate))
        w.writeframes(np.ascontiguousarray(pcm).astype("<i2", copy=False).tobytes())


def load_mixture(path, info, model_rate, dev, keep=False):
    """The file ``path`` (info: its wavio.probe) on ``dev`` at ``model_rate`` -> (mono f32 [L], the network's input; with
    ``keep`` its channels f32 [C, L], else None).  The frames go up as the bytes they are and are converted, down-mixed and
    filtered by one kernel (resample_frames / split_frames); at the model's rate that is read_wav's array for a 16-bit file."""
    from . import resample as R
    from . import wavio
    raw = torch.from_numpy(wavio.read_frames(path)[0]).to(dev)
    if keep:
        rows = R.split_frames(raw, info.fmt, info.channels, info.rate, model_rate)
        return rows[0], rows[1:]
    return R.resample_frames(raw, info.fmt, info.channels, info.rate, model_rate), None


def build_parser():
    from .arguments import ArgParser
    ap = ArgParser()
    ap.add_train_arguments()
    ap.add_other_arguments()
    p = ap.parser
    p.description = "Separate a WAV of any length with a trained checkpoint (windowed inference, stitched masks)."
    p.add_argument("--wav", required=True, help="mixture, a WAV file (16-, 24- or 32-bit PCM or 32-bit float) at any sample rate "
                                                "(resampled to --audRate on the GPU)")
    p.add_argument("--out_format", choices=("file", "s16", "s24", "f32"), default="file",
                   help="sample format of the written sources: the input file's own (default; a 32-bit PCM file gives 24-bit), "
                        "16-bit PCM, 24-bit PCM or 32-bit float")
    p.add_argument("--out_rate", choices=("file", "model"), default="file",
                   help="rate of the written sources: the input file's own (default) or the model's --audRate")
    p.add_argument("--channels", choices=("mix", "keep"), default="mix",
                   help="mix: the sources are mono (default); keep: every source is written with the file's channels "
                        "(the model still hears the down-mix; its masks go onto each channel)")
    p.add_argument("--wiener", type=int, default=0, metavar="K",
                   help="with --channels keep: K passes (0 ... 8) of a multichannel Wiener filter over the masked channels, "
                        "so every source keeps its own place in the stereo image (0, the default: the mask on every channel)")
    p.add_argument("--wiener_span", type=int, default=0, metavar="FRAMES",
                   help="with --wiener: estimate the spatial covariances locally, around centres FRAMES STFT frames apart (a "
                        "multiple of 64 in 64 ... 4096), for sources that move through the image (0, the default: one "
                        "covariance for the whole recording)")
    p.add_argument("--phase_iters", type=int, default=0, metavar="K",
                   help="K mixture-consistent phase iterations (0 ... 32) in place of the one inverse transform: every source "
                        "gets a phase of its own (0, the default: the mixture's phase; no gain with --binary_mask 1)")
    p.add_argument("--band", choices=("model", "full"), default="model",
                   help="model: the sources end at the model's band, half of --audRate (default); full: every source also gets "
                        "its share of what the file holds above that band, frame by frame as much as it holds of the band's top "
                        "octave (needs the file's rate as the output rate)")
    p.add_argument("--levels", action="store_true",
                   help="measure the mixture and the written sources (BS.1770-4 loudness, true peak) into <out>/levels.json")
    p.add_argument("--peak", type=float, default=None, metavar="DBTP",
                   help="rescale instead of clipping: one gain for all sources so that no true peak exceeds DBTP (<= 0)")
    p.add_argument("--loudness", type=float, default=None, metavar="LUFS",
                   help="one gain for all sources that brings the mixture to LUFS (-70 ... 0) integrated loudness; "
                        "with --peak the ceiling wins")
    p.add_argument("--limit", type=float, default=None, metavar="DBTP",
                   help="a linked look-ahead true-peak limiter in place of the clip: ONE gain curve for all sources and channels "
                        "that turns the level down around the peaks only, so that no true peak exceeds DBTP (<= 0) and "
                        "--loudness is reached elsewhere (not with --peak)")
    p.add_argument("--limit_lookahead", type=float, default=5.0, metavar="MS",
                   help="with --limit: the limiter's look-ahead in milliseconds (default 5; at most 2048 samples at the output rate)")
    p.add_argument("--frames", nargs="*", default=[], help="one .npy per source: [3,H,W], [1,3,H,W] or [K,3,H,W]; with --fps a "
                                                           "stack [T,3,H,W], and ONE stack with --num_mix 2 is a duet.  Frames as "
                                                           "shot: a uint8 .npy [H,W,3] or [T,H,W,3], or a folder of .jpg / .png "
                                                           "files in name order, prepared on the GPU at --imgSize")
    p.add_argument("--gpu_decode", action="store_true",
                   help="decode the image files of a --frames folder on the GPU (baseline and progressive JPEGs and 8-bit PNGs, .png files included; "
                        "anything else is read through Pillow as without the flag): the same pixels, without the one-core decode")
    p.add_argument("--fps", type=float, default=None, help="video frames per second of the .npy stacks (needs the spatial visual "
                                                           "features of --not_pool_vis)")
    p.add_argument("--frame_offset", type=float, default=0.0, help="time of the first video frame, seconds from the WAV's start")
    p.add_argument("--maps", action="store_true", help="also write the attention map of every window and source to <out>/maps.npy "
                                                       "(needs the spatial visual features of --not_pool_vis)")
    p.add_argument("--report", action="store_true",
                   help="also write <out>/report.html with mix.png, source<n>.png (mask x mixture magnitude) and mask<n>.png, "
                        "rendered on the GPU (needs Pillow)")
    p.add_argument("--report_width", type=int, default=2048, metavar="PX",
                   help="with --report: the pictures are at most PX pixels wide; ceil(frames / PX) STFT frames share a column")
    p.add_argument("--out", default="separated", help="output directory (source<n>.wav)")
    p.add_argument("--audio_only", action="store_true", help="no frames: audio-only branch with aligned windows")
    p.add_argument("--window_stride", type=int, default=128, help="STFT frames between window starts (<= 256)")
    p.add_argument("--window_batch", type=int, default=16, help="windows per U-Net pass")
    p.add_argument("--latest", action="store_true", help="load *_latest.pth instead of *_best.pth")
    return p


def parse_args(argv=None):
    args = build_parser().parse_args(argv)
    duet = len(args.frames) == 1 and args.num_mix == 2 and args.fps is not None     # one camera on both players: a clip
    if not args.audio_only and len(args.frames) != args.num_mix and not duet:
        raise SystemExit(f"--frames needs {args.num_mix} files (one per source), one stack with --fps for a duet of two, or pass "
                         f"--audio_only")
    if args.fps is not None and args.audio_only:
        raise SystemExit("--fps places video frames on the recording: it cannot go with --audio_only")
    if args.fps is not None and not args.fps > 0:
        raise SystemExit("--fps must be positive")
    if args.fps is not None and args.not_pool_vis:
        raise SystemExit("--fps separates with the clip's feature maps: pass --not_pool_vis as well (the fusion does not take pooled "
                         "visual features)")
    if args.maps and (args.audio_only or args.not_pool_vis):
        raise SystemExit("--maps writes the fusion's attention maps: it needs frames and the spatial visual features of "
                         "--not_pool_vis (pass that flag as well)")
    if not 0 <= args.wiener <= MAX_WIENER:
        raise SystemExit(f"--wiener takes 0 ... {MAX_WIENER} passes, got {args.wiener}")
    if not 0 <= args.phase_iters <= MAX_PHASE_ITERS:
        raise SystemExit(f"--phase_iters takes 0 ... {MAX_PHASE_ITERS} passes, got {args.phase_iters}")
    if args.wiener and args.channels != "keep":
        raise SystemExit("--wiener filters the file's channels: it needs --channels keep")
    if args.wiener_span and not (K.MWF_MIN_SPAN <= args.wiener_span <= K.MWF_MAX_SPAN and args.wiener_span % 64 == 0):
        raise SystemExit(f"--wiener_span takes 0 or a multiple of 64 frames in {K.MWF_MIN_SPAN} ... {K.MWF_MAX_SPAN}, got {args.wiener_span}")
    if args.wiener_span and not args.wiener:
        raise SystemExit("--wiener_span is the span of the Wiener filter's covariances: it needs --wiener K with K >= 1")
    if args.report_width < 1:
        raise SystemExit(f"--report_width takes a positive number of pixels, got {args.report_width}")
    if args.band == "full" and args.out_rate == "model":
        raise SystemExit("--band full adds what the file holds above the model's band: it cannot be written at --out_rate model")
    if args.peak is not None and not args.peak <= 0.0:
        raise SystemExit(f"--peak takes a true-peak ceiling of at most 0 dBTP, got {args.peak}")
    if args.loudness is not None and not -70.0 <= args.loudness <= 0.0:
        raise SystemExit(f"--loudness takes a target in -70 ... 0 LUFS, got {args.loudness}")
    if args.limit is not None:
        from . import levels as LV
        if not args.limit <= 0.0 or math.isinf(args.limit):
            raise SystemExit(f"--limit takes a finite true-peak ceiling of at most 0 dBTP, got {args.limit}")
        if args.peak is not None:
            raise SystemExit("--limit and --peak both set the ceiling: pass one of them (--peak: one gain for the whole run; "
                             "--limit: a gain curve around the peaks)")
        try:                                         # at the rate the sources are written at if it is known, else at the lowest
            LV.limiter_plan(args.audRate if args.out_rate == "model" else LV.MIN_RATE, args.limit_lookahead)
        except AvsepError as e:
            raise SystemExit(f"--limit_lookahead: {e}")
    return args


def open_recording(args, what, keep=False, levels=False):
    """The command lines' way from ``args.wav`` to (info: its wavio.probe; the down-mix f32 [L] at --audRate on cuda:0, the
    network's input; with ``keep`` its channels f32 [C, L], else None).  What the file cannot be answers the shell
    (SystemExit) before a GPU is asked for; ``what`` is the caller's noun in "no CPU fallback".  levels: the rate the
    sources are written at (--out_rate) must be one levels.py measures."""
    from . import resample as R
    from . import wavio
    try:
        info = wavio.probe(args.wav)
    except AvsepError as e:
        raise SystemExit(str(e))
    if info.channels > (R.MAX_KEPT_CHANNELS if keep else R.MAX_CHANNELS):
        raise SystemExit(f"{args.wav}: " + (f"--channels keep takes files of up to {R.MAX_KEPT_CHANNELS} channels" if keep else
                                            f"files of up to {R.MAX_CHANNELS} channels are read") + f", this one has {info.channels}")
    if info.rate != args.audRate:
        try:
            R.check_rates(info.rate, args.audRate)
        except AvsepError as e:
            raise SystemExit(f"{args.wav}: {e}")
    if levels:
        from . import levels as LV
        measured_rate = info.rate if args.out_rate == "file" else args.audRate
        if not LV.MIN_RATE <= measured_rate <= LV.MAX_RATE:
            raise SystemExit(f"{args.wav}: levels are measured at {LV.MIN_RATE} ... {LV.MAX_RATE} Hz, the sources are written at {measured_rate} Hz")
        if args.limit is not None:
            try:
                LV.limiter_plan(measured_rate, args.limit_lookahead)
            except AvsepError as e:
                raise SystemExit(f"{args.wav}: --limit_lookahead: {e}")
    if not torch.cuda.is_available():
        raise AvsepError(f"{what} runs on an MI355X; there is no CPU fallback")
    # the raw frames go up; down-mix (and with keep every channel beside it), conversion and filter are one kernel
    return (info, *load_mixture(args.wav, info, args.audRate, torch.device("cuda", 0), keep))


def load_nets(args, dev):
    """The command lines' nets -> (net_sound, net_frame) on ``dev`` in eval(): built from the flags, with the weights of
    --weights_sound / --weights_frame or, without them, of the checkpoint --ckpt/--id (--latest: *_latest.pth)."""
    from . import checkpoint as ckpt
    from .models import ModelBuilder
    args.ckpt = os.path.join(args.ckpt, args.id)
    if not args.weights_sound:
        args.weights_sound, args.weights_frame = ckpt.resume_paths(args, best=not args.latest)
    builder = ModelBuilder()
    net_frame = builder.build_frame(arch=args.arch_frame, fc_dim=args.vis_channels, pool_type=args.img_pool,
                                    weights=args.weights_frame)
    net_sound = builder.build_sound(arch=args.arch_sound, fc_dim=args.num_channels, weights=args.weights_sound,
                                    fusion_type=args.fusion_type, att_type=args.att_type)
    return net_sound.to(dev).eval(), net_frame.to(dev).eval()


def output_mixture(path, info, out_rate, low, keep):
    """What the stems are stems of, at the output rate, f32 [C, L]: the file's channels under --channels keep, else the
    down-mix row.  At the model's rate these are the network's own inputs ``low``; at the file's the file is read again."""
    if out_rate != info.rate:
        return low
    mono, channels = load_mixture(path, info, info.rate, low.device, keep)
    return channels if keep else mono[None]


def output_rows(stems, low, mix, gains, args, out_rate):
    """The stems [N, C, L] at the output rate, f32 [N, C, Lout], as separate_long left them (clamped or not): resampled, or
    with ``gains`` (--band full: separate_long's band_gains; ``mix`` is then output_mixture's rows at the file's rate)
    extended by the file's band above the model's."""
    from . import resample as R
    N, Cc, Lm = stems.shape
    if gains is not None:
        return R.band_extend(stems.contiguous(), low, mix, gains, args.audRate, out_rate, args.stft_hop)
    return R.resample(stems.reshape(N * Cc, Lm).contiguous(), args.audRate, out_rate).reshape(N, Cc, -1)


def write_stems(out_dir, rows, rate_in, rate_out, fmt):
    """rows f32 [N, C, L] at ``rate_in`` -> <out_dir>/source<n>.wav with C channels at ``rate_out`` in the sample format
    ``fmt``: the kernel writes the file's frames, every stem is one join (at equal rates a conversion alone)."""
    from . import resample as R
    from . import wavio
    for n, r in enumerate(rows):
        wavio.write_frames(os.path.join(out_dir, f"source{n}.wav"), R.join_frames(r.contiguous(), rate_in, rate_out, fmt).cpu().numpy(),
                           rate_out, r.shape[0], fmt)


def limit_rows(rows, mix, rate, gain, args):
    """--limit: the stems ``rows`` f32 [N, C, L] go through levels.limit as ONE programme of N*C rows at the pre-gain ``gain``;
    the mixture ``mix`` f32 [Cm, Lmix] gets the same curve and the same trim in float64 (past the stems' end, where there is
    nothing to limit, the pre-gain and the trim alone) -> (rows, mix, the "limiter" block of levels.json)."""
    from . import levels as LV
    N, Cc, Lr = rows.shape
    try:
        y, info = LV.limit(rows.reshape(1, N * Cc, Lr), rate, args.limit, gain=gain, lookahead_ms=args.limit_lookahead,
                           return_gain=True)
    except AvsepError as e:
        raise SystemExit(f"{args.wav}: {e}")
    flat = gain * float(info["trim"][0])
    n = min(Lr, mix.shape[1])
    curve = torch.full((mix.shape[1],), flat, dtype=torch.float64, device=mix.device)
    curve[:n] = info["gain"][0, :n] * flat
    mix = (mix.double() * curve).float()
    return y.reshape(N, Cc, Lr), mix, LV.limiter_figures(info, args.limit, args.limit_lookahead)


def cli(argv=None):
    args = parse_args(argv)
    keep = args.channels == "keep"
    levelled = args.peak is not None or args.loudness is not None or args.limit is not None
    info, wav, channels = open_recording(args, "separation", keep, levels=args.levels or levelled)
    rate, dev = info.rate, wav.device
    out_fmt = {"file": "s24" if info.fmt == "s32" else info.fmt}.get(args.out_format, args.out_format)
    nets = load_nets(args, dev)
    frames, times = [], None
    from . import frames as FR
    for path in args.frames:
        fr = FR.load_stack(path, dev if args.gpu_decode else None)       # uint8 [T,H,W,3]: frames as shot, prepared on the GPU batch by batch
        if not is_shot(fr):
            fr = fr.float()
        if args.fps is not None:                     # a clip stays on the host: the trunk takes it up batch by batch
            if fr.dim() != 4:
                raise SystemExit(f"{path}: with --fps every .npy is a stack [T,3,H,W], this one is {tuple(fr.shape)}")
            frames.append(fr)
        else:
            frames.append((fr[None] if fr.dim() == 3 else fr).to(dev))
    if args.fps is not None and not args.audio_only:
        times = args.frame_offset + torch.arange(frames[0].shape[0], dtype=torch.float64) / args.fps
    full = args.band == "full" and rate > args.audRate       # at or below the model's rate the file holds nothing above its band
    out = separate_long(nets, wav, frames, args, use_vis=not args.audio_only,
                        stride_frames=args.window_stride, batch=args.window_batch, channels=channels, wiener=args.wiener,
                        phase_iters=args.phase_iters, clamp=not (levelled or full), wiener_span=args.wiener_span,
                        **({"band_gains": True} if full else {}), **({"frame_times": times} if times is not None else {}),
                        **({"return_maps": True} if args.maps else {}), **({"return_masks": True} if args.report else {}))
    os.makedirs(args.out, exist_ok=True)
    if args.maps:
        np.save(os.path.join(args.out, "maps.npy"), out["maps"].cpu().numpy())
    out_rate = rate if args.out_rate == "file" else args.audRate
    stems = out["channel_wavs"] if keep else out["wavs"][:, None]
    rate_in, report = args.audRate, None
    if levelled or full or args.levels:              # the mixture and the stems at the output rate, once for all that follows
        low = channels if keep else wav[None]
        mix = output_mixture(args.wav, info, out_rate, low, keep)
        rows = output_rows(stems, low, mix, out["band_gains"] if full else None, args, out_rate)
        if full and not levelled:                    # the full-band rows are clamped as a whole; levelled ones are rescaled instead
            rows = rows.clamp_(-1.0, 1.0)
        if levelled or args.levels:                  # measured as they are written, but for the one gain (None, None: gain 1)
            from . import levels as LV
            m_stems, m_mix = LV.measure(rows, out_rate), LV.measure(mix, out_rate)
            try:
                gain, limited_by = LV.output_gain(m_mix["integrated"][0], m_stems["true_peak"], args.loudness, args.peak)
            except AvsepError as e:
                raise SystemExit(f"{args.wav}: {e}")
            limiter = None
            if args.limit is not None:               # one programme of all N*C rows: one curve, so the stems still sum to the mixture
                rows, mix, limiter = limit_rows(rows, mix, out_rate, gain, args)
                m_stems, m_mix = LV.measure(rows, out_rate), LV.measure(mix, out_rate)     # not linear: measured again
                if limiter["limited_share"] > 0.0:
                    limited_by = "limiter"
            elif gain != 1.0:                        # both meters are linear: the figures after the gain follow from those before
                rows = rows * gain
                m_stems, m_mix = LV.scaled(m_stems, gain), LV.scaled(m_mix, gain)
            report = LV.report(out_rate, gain, limited_by, m_mix, m_stems, limiter)
        if levelled or full:                         # written from the rows; else from the model-rate stems, resampled by the join
            stems, rate_in = rows, out_rate
    write_stems(args.out, stems, rate_in, out_rate, out_fmt)
    if args.report:                                  # after the stems: the page offers them beside their pictures
        from . import visuals
        visuals.report(args.out, wav, out["lin_masks"], args, args.report_width, title=os.path.basename(args.wav))
    if report is not None:
        import json
        with open(os.path.join(args.out, "levels.json"), "w") as f:
            json.dump(report, f, indent=1)
    kept = f", {channels.shape[0]} channel{'s' if channels.shape[0] != 1 else ''} each" if keep else ""
    if report is not None and report["limited_by"]:
        kept += f", gain {report['gain_db']:+.2f} dB (limited by {report['limited_by']})"
        if report["limited_by"] == "limiter":
            lim = report["limiter"]
            most = "to silence" if lim["max_reduction_db"] is None else f"by up to {lim['max_reduction_db']:.2f} dB"
            kept += f", limiter at {lim['ceiling_dbtp']:.2f} dBTP: {100.0 * lim['limited_share']:.2f} % of the samples turned down, {most}"
    if args.wiener:
        kept += f", multichannel Wiener filter x{args.wiener}"
        if args.wiener_span:
            kept += (f" with local covariances every {args.wiener_span} frames "
                     f"({args.wiener_span * args.stft_hop / args.audRate:.2f} s)")
    if args.phase_iters:
        kept += f", phase iterations x{args.phase_iters}"
    if full:
        kept += ", full band"
    elif args.band == "full":
        kept += ", the file's rate is within the model's band: --band full wrote what --band model writes"
    print(f"{len(out['starts'])} windows -> {args.out}/source[0-{args.num_mix - 1}].wav{kept}")
    return out


if __name__ == "__main__":
    cli()
