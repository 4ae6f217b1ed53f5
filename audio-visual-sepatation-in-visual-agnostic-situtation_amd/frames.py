"""Frames as shot: uint8 RGB stacks [T,H,W,3] (or a folder of image files) -> the float32 [T,3,S,S] the visual trunk is trained
on, prepared on the GPU (``avsep_frames_prepare``, csrc/frames.hip), bit for bit what ``dataset.VideoTransform`` gives the same
frames: Pillow's 8-bit bicubic resize, the crop, the flip, the ImageNet normalisation.

Exactness is by construction.  Every floating-point decision is taken here, on the host, in Python floats (float64), the way
Pillow's Resample.c takes it: ``resize_tables`` gives the fixed-point weights of each axis, ``plan`` adds the target size
(``dataset._resize_size``), the crop (Python's ``round``: halves to even) and the 256 x 3 table of normalised values, computed
with the transform's own torch expression.  The kernel adds int32 products and looks values up.

Limits (AvsepError): frames uint8, contiguous, [T,H,W,3], 1 <= T <= 65535 per call of the kernel (``prepare`` cuts longer
stacks), sides at most 4096, 8 <= S <= 1024, and at most MAX_KSIZE = 81 taps per output, which is a downscale of up to 20 on
either axis: a 2160 x 3840 frame at S = 224 has 41.

The training loader comes through the batch form: ``plan_batch`` takes the frames of a whole batch, each with its own size,
drawn crop and flip, and ``prepare_batch`` prepares them in one launch (``avsep_frames_prepare_batch``) straight into the
[B,3,T,S,S] the step takes (``dataset.to_device`` with ``MUSICMixDataset(raw_frames=True)``).  The tables of an axis pair are
computed once per process (``axis_tables``) and shared by every frame and plan that has the pair.
"""
import functools
import math
import os

import numpy as np
import torch

from . import dataset
from . import kernels as K
from .lib import AvsepError, FramesRow, got

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


@functools.lru_cache(maxsize=1024)
def axis_tables(n_in, n_out):
    """``resize_tables(n_in, n_out)``, computed once per process and axis pair.  The arrays are shared: read them only."""
    return resize_tables(n_in, n_out)


@functools.lru_cache(maxsize=1)
def norm_table():
    """float32 [256,3]: (v / 255 - mean) / std per byte value and channel, in dataset.VideoTransform's own expression.
    Computed once; read only."""
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


def _check_form(img_size, train, max_size, who):
    """What every frame of a plan shares: img_size, train, max_size -> S."""
    if not _is_int(img_size):
        raise AvsepError(f"{who} takes img_size as an int, got {img_size!r}")
    S = int(img_size)
    if not MIN_SIZE <= S <= MAX_SIZE:
        raise AvsepError(f"{who} takes img_size in {MIN_SIZE} ... {MAX_SIZE}, got {S}")
    if max_size is not None and (not _is_int(max_size) or max_size < 1):
        raise AvsepError(f"{who} takes max_size as a positive int or None, got {max_size!r}")
    if not isinstance(train, bool):
        raise AvsepError(f"{who} takes train as a bool, got {train!r}")
    return S


def _geometry(H, W, S, train, crop, max_size, who):
    """One frame's target size and crop: the rules of ``plan``, for ``plan`` and for every frame of ``plan_batch``
    -> (H, W, (w, h), (i, j))."""
    for name, v in (("H", H), ("W", W)):
        if not _is_int(v):
            raise AvsepError(f"{who} takes {name} as an int, got {v!r}")
    H, W = int(H), int(W)
    if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
        raise AvsepError(f"{who} takes frames with sides in 1 ... {MAX_SIDE}, got {H} x {W}")
    if crop is not None and not train:
        raise AvsepError(f"{who}(crop=...) is the training form's drawn corner: the validation form crops the centre")
    w, h = dataset._resize_size(W, H, int(S * 1.1) if train else S, max_size)
    if not (1 <= w <= MAX_SIDE and 1 <= h <= MAX_SIDE):
        raise AvsepError(f"{who}: {H} x {W} frames resize to {h} x {w}, outside 1 ... {MAX_SIDE}")
    if crop is None:
        crop = (int(round((h - S) / 2.0)), int(round((w - S) / 2.0)))
    elif len(crop) != 2 or not all(_is_int(c) for c in crop) or not all(-MAX_SIDE <= c <= MAX_SIDE for c in crop):
        raise AvsepError(f"{who} takes crop as two ints (i, j) within +-{MAX_SIDE}, got {crop!r}")
    for n_in, n_out, axis in ((W, w, "columns"), (H, h, "rows")):
        ksize = int(math.ceil(2.0 * max(n_in / n_out, 1.0))) * 2 + 1
        if ksize > MAX_KSIZE:
            raise AvsepError(f"{who}: {n_in} -> {n_out} {axis} takes {ksize} taps per output, more than {MAX_KSIZE} (a "
                             f"downscale of up to 20): resize the frames first")
    return H, W, (w, h), (int(crop[0]), int(crop[1]))


def plan(H, W, img_size, train=False, crop=None, flip=False, max_size=448):
    """The preparation of H x W frames for a trunk that takes img_size x img_size -> Plan.  Validation form (train False): the
    shorter side to img_size (the longer capped at max_size), centre crop; crop must be None.  Training form: the shorter side
    to int(img_size * 1.1), and ``crop`` = (i, j), the top-left corner the caller drew (None: the centre).  flip: mirror left
    to right after the crop."""
    S = _check_form(img_size, train, max_size, "frames.plan")
    if not isinstance(flip, bool):
        raise AvsepError(f"frames.plan takes train and flip as bools, got {train!r} and {flip!r}")
    H, W, (w, h), crop = _geometry(H, W, S, train, crop, max_size, "frames.plan")
    return Plan(H, W, S, (w, h), crop, flip, *axis_tables(W, w), *axis_tables(H, h))


def check_stack(frames, who="frames.prepare"):
    """frames must be a uint8 tensor [T,H,W,3], contiguous, T >= 1 -> its shape."""
    if not torch.is_tensor(frames) or frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3 \
            or frames.shape[0] < 1 or not frames.is_contiguous():
        loose = ", not contiguous" if torch.is_tensor(frames) and not frames.is_contiguous() else ""
        raise AvsepError(f"{who} takes uint8 RGB frames [T,H,W,3], contiguous, T >= 1; got {got(frames)}{loose}")
    return tuple(frames.shape)


def prepare(frames_u8, plan, return_u8=False):
    """frames_u8 uint8 [T,H,W,3] on the GPU, plan = plan(H, W, ...) -> float32 [T,3,S,S] (with return_u8 also the cropped and
    flipped pixels, uint8 [T,S,S,3]) through the kernel."""
    T, H, W, _ = check_stack(frames_u8)
    if not isinstance(plan, Plan) or (H, W) != (plan.H, plan.W):
        raise AvsepError(f"frames.prepare: the plan is for {getattr(plan, 'H', '?')} x {getattr(plan, 'W', '?')} frames, "
                         f"these are {H} x {W}")
    return K.frames_prepare(frames_u8, plan.on(frames_u8.device), plan.size, plan.img_size, plan.crop, plan.flip, return_u8)


ROW = np.dtype(FramesRow)      # one frame of a batch, as the library reads it (include/avsep.h: avsep_frames_row)


class _Packed:
    """The tables of a batch's axis pairs in one int32 buffer: ``offsets[(n_in, n_out)]`` = (coef, bound) in words, ``taps``
    the pair's taps per output.  Uploaded once per device."""

    def __init__(self, pairs):
        self.offsets, self.taps, parts, at = {}, {}, [], 0
        for pair in pairs:
            coef, bound = axis_tables(*pair)
            self.offsets[pair], self.taps[pair] = (at, at + coef.size), coef.shape[1]
            parts += [coef.reshape(-1), bound.reshape(-1)]
            at += coef.size + bound.size
        self.host = torch.from_numpy(np.concatenate(parts))
        self.lut = norm_table()
        self._dev = {}

    def on(self, dev):
        dev = torch.device(dev)
        if dev not in self._dev:
            self._dev[dev] = (self.host.to(dev), self.lut.to(dev))
        return self._dev[dev]


@functools.lru_cache(maxsize=64)
def _packed(pairs):
    return _Packed(pairs)


class BatchPlan:
    """What ``prepare_batch`` needs for the frames of one batch: see ``plan_batch``.  ``rows`` (NumPy, dtype ROW) holds one
    checked row per frame, ``launches`` the (first row, end row, grid y, LDS bytes, smallest tile height) of every launch."""

    def __init__(self, img_size, rows, sizes, crops, pixel_bytes, out_shape, plane, packed, launches):
        self.img_size, self.rows, self.sizes, self.crops, self.pixel_bytes = img_size, rows, sizes, crops, pixel_bytes
        self.out_shape, self.plane, self.packed, self.launches = out_shape, plane, packed, launches
        self.n = len(rows)


def plan_batch(shapes, img_size, train=False, crops=None, flips=None, max_size=448, layout=None):
    """The preparation of n frames of any sizes in one launch -> BatchPlan.  shapes: n pairs (H, W), in the order the frames
    lie in the byte buffer, back to back.  Per frame the rules of ``plan``: the target size is ``dataset._resize_size``, the
    crop is ``crops[r]`` = (i, j) (training form only) or the frame's own centre where that is None (``crops=None``: all
    centred), ``flips[r]`` mirrors it (``None``: none).  layout None: the output is [n,3,S,S]; layout (B, T) with B * T == n:
    the loader's [B,3,T,S,S], frame r being clip r // T, time r % T."""
    who = "frames.plan_batch"
    S = _check_form(img_size, train, max_size, who)
    shapes = list(shapes)
    n = len(shapes)
    if n < 1 or any(len(s) != 2 for s in shapes):
        raise AvsepError(f"{who} takes at least one frame shape (H, W), got {shapes[:4]!r}{' ...' if n > 4 else ''}")
    crops = [None] * n if crops is None else list(crops)
    flips = [False] * n if flips is None else list(flips)
    if len(crops) != n or len(flips) != n or not all(isinstance(f, (bool, np.bool_)) for f in flips):
        raise AvsepError(f"{who} takes one crop (or None) and one bool flip per frame: {n} frames, {len(crops)} crops, "
                         f"{len(flips)} flips")
    if layout is None:
        out_shape, plane = (n, 3, S, S), S * S
        out_off = [r * 3 * S * S for r in range(n)]
    else:
        if len(layout) != 2 or not all(_is_int(v) and v >= 1 for v in layout) or layout[0] * layout[1] != n:
            raise AvsepError(f"{who} takes layout as None ([n,3,S,S]) or (B, T) with B * T == {n} ([B,3,T,S,S]), got {layout!r}")
        B, T = int(layout[0]), int(layout[1])
        out_shape, plane = (B, 3, T, S, S), T * S * S
        out_off = [((r // T) * 3 * T + r % T) * S * S for r in range(n)]
    geo = [_geometry(H, W, S, train, crop, max_size, who) for (H, W), crop in zip(shapes, crops)]
    pairs = tuple(dict.fromkeys(p for H, W, (w, h), _ in geo for p in ((W, w), (H, h))))      # distinct, in order of appearance
    packed = _packed(pairs)
    rows, at = np.zeros(n, dtype=ROW), 0
    for r, (H, W, (w, h), (ci, cj)) in enumerate(geo):
        (hc, hb), (vc, vb) = packed.offsets[(W, w)], packed.offsets[(H, h)]
        rows[r] = (at, out_off[r], H, W, w, h, packed.taps[(W, w)], packed.taps[(H, h)], hc, hb, vc, vb, ci, cj, int(flips[r]),
                   0, 0, 0, 0, 0)
        at += H * W * 3
    out_floats = int(np.prod(out_shape))
    launches = []
    for a in range(0, n, K.FRAMES_MAX_T):
        b = min(n, a + K.FRAMES_MAX_T)
        launches.append((a, b) + K.frames_batch_plan(rows[a:b], S, at, packed.host.numel(), out_floats, plane))
    return BatchPlan(S, rows, [g[2] for g in geo], [g[3] for g in geo], at, out_shape, plane, packed, launches)


def prepare_batch(pixels_u8, batch_plan):
    """pixels_u8: uint8 [bytes] on the GPU, the frames of ``batch_plan`` = plan_batch(...) back to back -> float32 in the
    plan's layout, [n,3,S,S] or [B,3,T,S,S], through the kernel: one launch (per 65535 frames)."""
    if not isinstance(batch_plan, BatchPlan):
        raise AvsepError(f"frames.prepare_batch takes a plan of frames.plan_batch, got {type(batch_plan).__name__}")
    if not torch.is_tensor(pixels_u8) or pixels_u8.dtype != torch.uint8 or pixels_u8.dim() != 1 or not pixels_u8.is_contiguous() \
            or pixels_u8.numel() != batch_plan.pixel_bytes:
        raise AvsepError(f"frames.prepare_batch takes the plan's {batch_plan.pixel_bytes} bytes as one contiguous uint8 tensor "
                         f"[bytes]; got {got(pixels_u8)}")
    K.lib.require_gpu(pixels_u8)
    dev = pixels_u8.device
    tables, lut = batch_plan.packed.on(dev)
    rows = torch.from_numpy(batch_plan.rows.view(np.uint8)).to(dev, non_blocking=True)
    out = torch.empty(batch_plan.out_shape, dtype=torch.float32, device=dev)
    for a, b, grid_y, lds, _ in batch_plan.launches:
        K.frames_prepare_batch(pixels_u8, rows[a * ROW.itemsize:b * ROW.itemsize], tables, lut, batch_plan.img_size, out,
                               batch_plan.plane, grid_y, lds)
    return out


def load_stack(path, device=None):
    """The one place a frame file or folder is read -> a CPU tensor.  A ``.npy`` of floats comes back as it is (prepared
    frames, the earlier form); a ``.npy`` of uint8 must be [T,H,W,3] or [H,W,3] and comes back as uint8 [T,H,W,3]; a directory
    gives its .jpg / .jpeg / .png files in name order, each read as ``dataset._load_frames`` reads it, as uint8 [T,H,W,3].
    What cannot be read ends with SystemExit: this is the command lines' reader.
    With ``device`` (a GPU) a folder's frames are decoded there (``png.decode_stack``: baseline and progressive JPEG files and
    8-bit PNG files through the kernels, whatever the kernels refuse through Pillow) and the stack comes back on that device, the
    same bytes."""
    if os.path.isdir(path):
        names = sorted(n for n in os.listdir(path) if n.lower().endswith(IMAGE_SUFFIXES))
        if not names:
            raise SystemExit(f"{path}: no .jpg, .jpeg or .png file in this folder")
        if device is not None:
            from . import png
            return png.decode_stack([os.path.join(path, n) for n in names], device)
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
