"""Frames as shot: uint8 RGB stacks [T,H,W,3] (or a folder of image files) -> the float32 [T,3,S,S] the visual trunk is trained
on, prepared on the GPU (``avsep_frames_prepare``, csrc/frames.hip), bit for bit what ``dataset.VideoTransform`` gives the same
frames: Pillow's 8-bit bicubic resize, the crop, the flip, the ImageNet normalisation.

Exactness is by construction.  Every floating-point decision is taken here, on the host, in Python floats (float64), the way
Pillow's Resample.c takes it: ``resize_tables`` gives the fixed-point weights of each axis, ``plan`` adds the target size
(``dataset._resize_size``), the crop (Python's ``round``: halves to even) and the 256 x 3 table of normalised values, computed
with the transform's own torch expression.  The kernel adds int32 products and looks values up.

Limits (AvsepError): frames uint8, contiguous, [T,H,W,3], 1 <= T <= 65535 per call of the kernel (``prepare`` cuts longer
stacks), sides at most 4096, 8 <= S <= 1024, and at most MAX_KSIZE = 81 taps per output, which is a downscale of up to 20 on
either axis: a 2160 x 3840 frame at S = 224 has 41.  The training loader does not come through here; ``train``, ``crop`` and
``flip`` exist so that it can.
"""
import math
import os

import numpy as np
import torch

from . import dataset
from . import kernels as K
from .lib import AvsepError

MAX_SIDE = 4096
MIN_SIZE, MAX_SIZE = 8, 1024
MAX_KSIZE = 81                 # taps per output: support 2 * scale to either side, scale <= 20
PRECISION_BITS = 22            # Pillow's fixed point for 8-bit images
IMAGE_SUFFIXES = (".jpg", ".jpeg", ".png")


def _bicubic(t):
    a = -0.5
    t = abs(t)
    if t < 1.0:
        return ((a + 2.0) * t - (a + 3.0)) * t * t + 1
    if t < 2.0:
        return (((t - 5) * t + 8) * t - 4) * a
    return 0.0


def resize_tables(n_in, n_out):
    """The coefficient table of one axis resized from ``n_in`` to ``n_out`` samples, as Pillow's precompute_coeffs and
    normalize_coeffs_8bpc make it -> (coef int32 [n_out, ksize], bound int32 [n_out, 2] = (first input index, count)), NumPy.
    Output xx is clip((2^21 + sum_k coef[xx, k] * in[first + k]) >> 22, 0, 255); entries past count are 0."""
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < 1:
        raise AvsepError(f"resize_tables takes sizes >= 1, got {n_in} -> {n_out}")
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    coef = np.zeros((n_out, ksize), dtype=np.int32)
    bound = np.zeros((n_out, 2), dtype=np.int32)
    one = float(1 << PRECISION_BITS)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)                 # int() truncates, as the C cast
        xmax = min(int(center + support + 0.5), n_in) - xmin
        w = [_bicubic((x + xmin - center + 0.5) / fs) for x in range(xmax)]
        ww = 0.0
        for v in w:                                                # ascending order
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        coef[xx, :xmax] = [int(-0.5 + v * one) if v < 0 else int(0.5 + v * one) for v in w]
        bound[xx] = (xmin, xmax)
    return coef, bound


def norm_table():
    """float32 [256,3]: (v / 255 - mean) / std per byte value and channel, in dataset.VideoTransform's own expression."""
    v = torch.arange(256, dtype=torch.uint8)[None, :, None].expand(3, 256, 1).contiguous()
    mean, std = torch.tensor(dataset._MEAN).view(3, 1, 1), torch.tensor(dataset._STD).view(3, 1, 1)
    return ((v.float().div_(255.0) - mean) / std)[:, :, 0].t().contiguous()


class Plan:
    """What ``prepare`` needs for frames of one size: see ``plan``.  The tables live on the host until ``on`` uploads them, once
    per device."""

    def __init__(self, H, W, img_size, size, crop, flip, hcoef, hbound, vcoef, vbound):
        self.H, self.W, self.img_size, self.size, self.crop, self.flip = H, W, img_size, size, crop, flip
        self.tables = [torch.from_numpy(a) for a in (hcoef, hbound, vcoef, vbound)] + [norm_table()]
        self._dev = {}

    def on(self, dev):
        dev = torch.device(dev)
        if dev not in self._dev:
            self._dev[dev] = [t.to(dev) for t in self.tables]
        return self._dev[dev]


def _is_int(v):
    return not isinstance(v, bool) and isinstance(v, (int, np.integer))


def plan(H, W, img_size, train=False, crop=None, flip=False, max_size=448):
    """The preparation of H x W frames for a trunk that takes img_size x img_size -> Plan.  Validation form (train False): the
    shorter side to img_size (the longer capped at max_size), centre crop; crop must be None.  Training form: the shorter side
    to int(img_size * 1.1), and ``crop`` = (i, j), the top-left corner the caller drew (None: the centre).  flip: mirror left
    to right after the crop."""
    for name, v in (("H", H), ("W", W), ("img_size", img_size)):
        if not _is_int(v):
            raise AvsepError(f"frames.plan takes {name} as an int, got {v!r}")
    H, W, S = int(H), int(W), int(img_size)
    if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
        raise AvsepError(f"frames.plan takes frames with sides in 1 ... {MAX_SIDE}, got {H} x {W}")
    if not MIN_SIZE <= S <= MAX_SIZE:
        raise AvsepError(f"frames.plan takes img_size in {MIN_SIZE} ... {MAX_SIZE}, got {S}")
    if max_size is not None and (not _is_int(max_size) or max_size < 1):
        raise AvsepError(f"frames.plan takes max_size as a positive int or None, got {max_size!r}")
    if not isinstance(train, bool) or not isinstance(flip, bool):
        raise AvsepError(f"frames.plan takes train and flip as bools, got {train!r} and {flip!r}")
    if crop is not None and not train:
        raise AvsepError("frames.plan(crop=...) is the training form's drawn corner: the validation form crops the centre")
    w, h = dataset._resize_size(W, H, int(S * 1.1) if train else S, max_size)
    if not (1 <= w <= MAX_SIDE and 1 <= h <= MAX_SIDE):
        raise AvsepError(f"frames.plan: {H} x {W} frames resize to {h} x {w}, outside 1 ... {MAX_SIDE}")
    if crop is None:
        crop = (int(round((h - S) / 2.0)), int(round((w - S) / 2.0)))
    elif len(crop) != 2 or not all(_is_int(c) for c in crop) or not all(-MAX_SIDE <= c <= MAX_SIDE for c in crop):
        raise AvsepError(f"frames.plan takes crop as two ints (i, j) within +-{MAX_SIDE}, got {crop!r}")
    for n_in, n_out, axis in ((W, w, "columns"), (H, h, "rows")):
        ksize = int(math.ceil(2.0 * max(n_in / n_out, 1.0))) * 2 + 1
        if ksize > MAX_KSIZE:
            raise AvsepError(f"frames.plan: {n_in} -> {n_out} {axis} takes {ksize} taps per output, more than {MAX_KSIZE} (a "
                             f"downscale of up to 20): resize the frames first")
    return Plan(H, W, S, (w, h), (int(crop[0]), int(crop[1])), flip, *resize_tables(W, w), *resize_tables(H, h))


def check_stack(frames, who="frames.prepare"):
    """frames must be a uint8 tensor [T,H,W,3], contiguous, T >= 1 -> its shape."""
    if not torch.is_tensor(frames) or frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3 \
            or frames.shape[0] < 1 or not frames.is_contiguous():
        got = f"{frames.dtype} {tuple(frames.shape)}" + ("" if frames.is_contiguous() else ", not contiguous") \
            if torch.is_tensor(frames) else type(frames).__name__
        raise AvsepError(f"{who} takes uint8 RGB frames [T,H,W,3], contiguous, T >= 1; got {got}")
    return tuple(frames.shape)


def prepare(frames_u8, plan, return_u8=False):
    """frames_u8 uint8 [T,H,W,3] on the GPU, plan = plan(H, W, ...) -> float32 [T,3,S,S] (with return_u8 also the cropped and
    flipped pixels, uint8 [T,S,S,3]) through the kernel."""
    T, H, W, _ = check_stack(frames_u8)
    if not isinstance(plan, Plan) or (H, W) != (plan.H, plan.W):
        raise AvsepError(f"frames.prepare: the plan is for {getattr(plan, 'H', '?')} x {getattr(plan, 'W', '?')} frames, "
                         f"these are {H} x {W}")
    return K.frames_prepare(frames_u8, plan.on(frames_u8.device), plan.size, plan.img_size, plan.crop, plan.flip, return_u8)


def load_stack(path):
    """The one place a frame file or folder is read -> a CPU tensor.  A ``.npy`` of floats comes back as it is (prepared
    frames, the earlier form); a ``.npy`` of uint8 must be [T,H,W,3] or [H,W,3] and comes back as uint8 [T,H,W,3]; a directory
    gives its .jpg / .jpeg / .png files in name order, each read as ``dataset._load_frames`` reads it, as uint8 [T,H,W,3].
    What cannot be read ends with SystemExit: this is the command lines' reader."""
    if os.path.isdir(path):
        names = sorted(n for n in os.listdir(path) if n.lower().endswith(IMAGE_SUFFIXES))
        if not names:
            raise SystemExit(f"{path}: no .jpg, .jpeg or .png file in this folder")
        try:
            from PIL import Image
        except ImportError:
            raise SystemExit(f"{path}: image files are read through Pillow, which is not installed; pass a uint8 .npy [T,H,W,3]")
        first, stack = None, None
        for t, n in enumerate(names):
            a = np.asarray(Image.open(os.path.join(path, n)).convert("RGB"), dtype=np.uint8)
            if first is None:
                first, stack = a.shape, np.empty((len(names),) + a.shape, dtype=np.uint8)
            if a.shape != first:
                raise SystemExit(f"{path}: frames of unequal size: {n} is {a.shape[0]} x {a.shape[1]}, {names[0]} is "
                                 f"{first[0]} x {first[1]}")
            stack[t] = a
        return torch.from_numpy(stack)
    a = np.load(path)
    if a.dtype != np.uint8:
        return torch.from_numpy(a)
    if a.ndim == 3 and a.shape[2] == 3:
        a = a[None]
    if a.ndim != 4 or a.shape[3] != 3 or a.shape[0] < 1:
        raise SystemExit(f"{path}: a uint8 .npy holds frames as shot, [T,H,W,3] or [H,W,3] (RGB last); this one is {a.shape}")
    return torch.from_numpy(np.ascontiguousarray(a))
