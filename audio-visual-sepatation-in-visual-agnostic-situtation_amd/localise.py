"""Localise the sounding objects over a clip: one attention heat map per video frame and source (the reference's demo,
inference.py:537-578 ``vis_video`` + :509-534 ``plot_save_att``, which runs one whole forward pass and one OpenCV round trip
per video frame).

The visual features enter the U-Net only at its bottleneck and the maps need only the global max-pool of that bottleneck,
never the decoder.  So the recording gets ONE STFT, its windows (``separate.plan_windows``) go through the ENCODER once
(``Unet.bottleneck``), all video frames go through the visual trunk as batches, ONE kernel computes every frame's maps
against the window nearest to it (``avsep_localise_maps``) and ONE kernel colours, resizes and blends them over the frames
on the device (``avsep_heatmap_overlay``).  A recording of one tile has one window: the same audio for every frame, which is
the reference's ``vis_video``.

Three deliberate deviations from ``plot_save_att``: the frame is de-normalised with rounding and clamping
(the reference truncates and wraps), the 8-bit resize and the blend are integer formulas stated in include/avsep.h (parity
with cv2.resize / cv2.addWeighted is within a level, not pinned).

CLI: ``python -m avsep_amd.localise --wav mix.wav --frames a.npy [b.npy] --fps 8 --id <experiment> --out dir`` (flag set of
arguments.py; one .npy with ``--num_mix 2`` is a duet: one camera, two players).
"""
import os

import numpy as np
import torch

from . import kernels as K
from . import lib
from .lib import AvsepError
from .separate import FOUT, WIDTH, frame_columns, is_shot, load_nets, open_recording, plan_windows, trunk_features


def jet_table():
    """uint8 [256,3] RGB: Octave's jet(256), the colour map cv2.COLORMAP_JET tabulates (not matplotlib's 'jet')."""
    x = 4.0 * np.arange(256, dtype=np.float64) / 256.0
    return np.stack([np.rint(255.0 * np.clip(1.5 - np.abs(x - k), 0.0, 1.0)) for k in (3.0, 2.0, 1.0)], 1).astype(np.uint8)


def window_of_frames(frame_times, starts, rate, hop, width=WIDTH):
    """The window each video frame is scored against -> int32 [T] (CPU).  frame_times: seconds from the start of the
    recording; starts: plan_windows' start columns.  A frame at t lies at STFT column c = round(t * rate / hop) (columns are
    centred on j * hop; halves round up), clamped to the recording's columns [0, starts[-1] + width - 1]; it gets the window
    whose centre start + width / 2 is nearest to c, the lower index on a tie."""
    c = frame_columns(frame_times, starts, rate, hop, width, who="window_of_frames")            # the column rule, shared with separate.frames_of_windows
    s = np.asarray(list(starts), dtype=np.int64)
    dist = np.abs(2 * s[None, :] + int(width) - 2 * c[:, None])                 # twice the distance: integers
    return torch.from_numpy(np.argmin(dist, axis=1).astype(np.int32))


def _frame_features(net_frame, fr, args, batch, act):
    f = trunk_features(net_frame, fr, batch, fr.device, args.not_pool_vis, args.img_activation if act else None)
    if f.dim() != 4:
        raise AvsepError(f"localisation needs a spatial visual feature map [T,Dc,h,w], net_frame gives {tuple(f.shape)}")
    return f.float().contiguous()


def localise(nets, wav, frames, frame_times, args, stride_frames=128, batch=16, alpha=0.4, render=True):
    """Attention maps (and heat-map overlays) of every video frame of one recording.

    nets: (net_sound, net_frame), both in eval() (else AvsepError).  wav [L] on the GPU, L >= args.stft_frame.  frames: list
    of C = args.num_mix tensors [T,3,H,W] (ImageNet-normalised floats), or a one-element list = duet (num_mix 2 only): the
    same feature map feeds both sources and, as inference.NetWrapper.forward_av, img_activation is not applied to it.
    A frame tensor may be uint8 [T,H,W,3] instead, RGB frames as shot: they are prepared on the GPU at args.imgSize
    (``frames.prepare``, dataset.VideoTransform's validation form bit for bit) and the overlays are drawn over the prepared
    frames.
    frame_times [T]: seconds from the start of wav.  fusion_type hidsep / CoLoc_Sel (their maps are the same); MixVis:
    NotImplementedError; pooled visual features (args.not_pool_vis): AvsepError.

    Returns {"maps": float32 [T,C,h,w] (maps[t,c]: the audio block the winning permutation pairs with visual input c, what
    the fusion's att_maps are for that frame), "best": int32 [T], "scores": float32 [T,C!], "window": int32 [T] (CPU),
    "starts": list, and with render "overlays": uint8 [C,T,H,W,3] RGB}.
    """
    net_sound, net_frame = nets
    lib.require_gpu(wav)
    if wav.dim() != 1 or wav.numel() < args.stft_frame:
        raise AvsepError(f"localise takes one recording [L] with L >= stft_frame, got {tuple(wav.shape)}")
    if net_sound.training or net_frame.training:
        raise AvsepError("localise needs the nets in eval(): call .eval() on both first")
    if args.fusion_type == "MixVis":
        raise NotImplementedError("localisation does not provide the MixVis fusion")
    if args.fusion_type not in ("hidsep", "CoLoc_Sel"):
        raise AvsepError(f"localisation needs a CoLoc fusion (hidsep / CoLoc_Sel), got {args.fusion_type!r}")
    if args.not_pool_vis:
        raise AvsepError("localisation needs a spatial visual feature map: pooled features (not_pool_vis) have no 'where'")
    Cn = args.num_mix
    duet = len(frames) == 1
    if Cn not in (2, 3) or (duet and Cn != 2) or (not duet and len(frames) != Cn):
        raise AvsepError(f"localise takes num_mix in (2, 3) and one frame tensor per source, or ONE for a duet of two; got "
                         f"num_mix={Cn} and {len(frames)} frame tensors")
    T = frames[0].shape[0]
    for n, fr in enumerate(frames):
        lib.require_gpu(fr)
        if fr.dim() != 4 or fr.shape[3 if is_shot(fr) else 1] != 3 or tuple(fr.shape) != tuple(frames[0].shape) \
                or fr.dtype != frames[0].dtype:
            raise AvsepError(f"frames[{n}] must be [T,3,H,W] (or uint8 [T,H,W,3]) like frames[0], got {fr.dtype} {tuple(fr.shape)}")
    times = torch.as_tensor(frame_times).reshape(-1)
    if T < 1 or times.numel() != T:
        raise AvsepError(f"localise needs one time per video frame: {T} frames, {times.numel()} times")
    if not 0.0 <= alpha <= 1.0:
        raise AvsepError(f"alpha must lie in [0, 1], got {alpha}")
    dev = wav.device
    with torch.no_grad():
        plan = K.Stft(dev, args.stft_frame, args.stft_hop, getattr(args, "stft_pad_mode", "reflect"))
        mag = plan.stft(wav.float().contiguous()[None], want_phase=False)[0][0].contiguous()      # [Fin, F]
        starts = plan_windows(mag.shape[1], stride_frames, WIDTH)
        starts_t = torch.tensor(starts, dtype=torch.int32, device=dev)
        _, logm = K.window_prepare(mag, starts_t, FOUT, WIDTH)
        x = net_sound.bottleneck(logm, batch)                                                      # [K, D, Fq, Tq]
        if is_shot(frames[0]):                                                                     # the overlays need every prepared frame
            from . import frames as FR
            if getattr(args, "imgSize", None) is None:
                raise AvsepError("uint8 frames are prepared at args.imgSize, which these args do not have")
            for fr in frames:
                FR.check_stack(fr, "localise")
            shot = FR.plan(frames[0].shape[1], frames[0].shape[2], args.imgSize)
            frames = [torch.cat([FR.prepare(fr[i:i + batch], shot) for i in range(0, T, batch)], 0) for fr in frames]
        frames = [fr.float().contiguous() for fr in frames]
        feats = [_frame_features(net_frame, fr, args, batch, act=not duet) for fr in frames]
        if feats[0].shape[1] != x.shape[1] // Cn:
            raise AvsepError(f"visual channels {feats[0].shape[1]} != bottleneck // {Cn} = {x.shape[1] // Cn}")
        window = window_of_frames(times, starts, args.audRate, args.stft_hop, WIDTH)
        maps, best, scores = K.localise_maps(x, window.to(dev), feats * 2 if duet else feats, net_sound.att_type)
        out = {"maps": maps, "best": best, "scores": scores, "window": window, "starts": starts}
        if render:
            table = torch.from_numpy(jet_table()).to(dev)
            out["overlays"] = K.heatmap_overlay(maps, frames * 2 if duet else frames, table, int(round(256 * alpha)))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# command line
# ---------------------------------------------------------------------------------------------------------------------
JPG_CHUNK = 512                  # frames per jpeg.encode call of --jpg


def build_parser():
    from .arguments import ArgParser
    ap = ArgParser()
    ap.add_train_arguments()
    ap.add_other_arguments()
    p = ap.parser
    p.description = "Heat maps of where each source sounds, per video frame, from a trained checkpoint."
    p.add_argument("--wav", required=True, help="mixture, a WAV file (16-, 24- or 32-bit PCM or 32-bit float) at any sample rate "
                                                "(resampled to --audRate on the GPU)")
    p.add_argument("--frames", nargs="+", required=True,
                   help="one .npy [T,3,H,W] (normalised floats) per source; ONE file with --num_mix 2 is a duet.  Frames as shot: "
                        "a uint8 .npy [T,H,W,3], or a folder of .jpg / .png files in name order, prepared on the GPU at --imgSize")
    p.add_argument("--fps", type=float, required=True, help="video frames per second of the .npy stacks")
    p.add_argument("--gpu_decode", action="store_true",
                   help="decode the image files of a --frames folder on the GPU (baseline and progressive JPEGs and 8-bit PNGs, .png files included; "
                        "anything else is read through Pillow as without the flag): the same pixels, without the one-core decode")
    p.add_argument("--frame_offset", type=float, default=0.0, help="time of the first video frame, seconds from the WAV's start")
    p.add_argument("--out", default="localised", help="output directory (maps.npy, overlay_source<c>.npy)")
    p.add_argument("--png", action="store_true", help="also write one PNG per frame and source (needs Pillow)")
    p.add_argument("--jpg", action="store_true",
                   help="also write one JPEG per frame and source, encoded on the GPU: the file Pillow's save(f, 'JPEG', quality=Q) writes")
    p.add_argument("--jpg_quality", type=int, default=90, help="quality of the --jpg files, 1 .. 100")
    p.add_argument("--alpha", type=float, default=0.4, help="weight of the heat map in the blend")
    p.add_argument("--window_stride", type=int, default=128, help="STFT frames between window starts (<= 256)")
    p.add_argument("--window_batch", type=int, default=16, help="windows / video frames per network pass")
    p.add_argument("--latest", action="store_true", help="load *_latest.pth instead of *_best.pth")
    return p


def parse_args(argv=None):
    args = build_parser().parse_args(argv)
    if args.num_mix not in (2, 3):
        raise SystemExit("--num_mix must be 2 or 3")
    if len(args.frames) != args.num_mix and not (len(args.frames) == 1 and args.num_mix == 2):
        raise SystemExit(f"--frames needs {args.num_mix} files (one per source), or one file for a duet with --num_mix 2")
    if not args.fps > 0:
        raise SystemExit("--fps must be positive")
    if not 0.0 <= args.alpha <= 1.0:
        raise SystemExit("--alpha must lie in [0, 1]")
    if not 1 <= args.jpg_quality <= 100:
        raise SystemExit("--jpg_quality must lie in [1, 100]")
    if not 1 <= args.window_stride <= WIDTH:
        raise SystemExit(f"--window_stride must lie in [1, {WIDTH}]")
    return args


def cli(argv=None):
    args = parse_args(argv)
    wav = open_recording(args, "localisation")[1]      # frame times are in seconds: only the input side needs the model's rate
    dev = wav.device
    nets = load_nets(args, dev)
    from . import frames as FR
    frames = [fr.to(dev) if is_shot(fr) else fr.float().to(dev) for fr in (FR.load_stack(path, dev if args.gpu_decode else None) for path in args.frames)]
    times = args.frame_offset + torch.arange(frames[0].shape[0], dtype=torch.float64) / args.fps
    out = localise(nets, wav, frames, times, args, stride_frames=args.window_stride,
                   batch=args.window_batch, alpha=args.alpha)
    os.makedirs(args.out, exist_ok=True)
    np.save(os.path.join(args.out, "maps.npy"), out["maps"].cpu().numpy())
    overlays = out["overlays"].cpu().numpy()
    for c in range(overlays.shape[0]):
        np.save(os.path.join(args.out, f"overlay_source{c}.npy"), overlays[c])
    if args.png:
        try:
            from PIL import Image
        except ImportError as e:
            raise AvsepError("--png writes through Pillow, which is not installed; the .npy stacks have been written") from e
        for c in range(overlays.shape[0]):
            for t in range(overlays.shape[1]):
                Image.fromarray(overlays[c, t]).save(os.path.join(args.out, f"source{c}_frame{t:05d}.png"))
    if args.jpg:
        from . import jpeg
        stack = out["overlays"]
        for c in range(stack.shape[0]):
            for t0 in range(0, stack.shape[1], JPG_CHUNK):                   # only the encoded bytes come back, a chunk at a time
                for t, data in enumerate(jpeg.encode(stack[c, t0:t0 + JPG_CHUNK], quality=args.jpg_quality), t0):
                    with open(os.path.join(args.out, f"source{c}_frame{t:05d}.jpg"), "wb") as f:
                        f.write(data)
    print(f"{overlays.shape[1]} frames x {overlays.shape[0]} sources over {len(out['starts'])} windows -> {args.out}/")
    return out


if __name__ == "__main__":
    cli()
