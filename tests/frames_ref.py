"""NumPy restatement of what dataset.VideoTransform does to a stack of uint8 RGB frames: Pillow's 8-bit bicubic resize
(Resample.c: float64 coefficient tables, 22-bit fixed point, a horizontal and a vertical pass with a rounding to uint8
between them), the crop (zero outside the resized image), the flip and the ImageNet normalisation.  The reference of
tests/test_frames_host.py (against Pillow itself) and tests/test_gpu_frames.py (against the kernel); it shares no code with
avsep_amd/frames.py.  The tables are built for all output positions at once, column by column, so the weights are added in
ascending order as the C loop adds them."""
import numpy as np
import torch

from avsep_amd import dataset as D

BITS = 22


def _bicubic(t):
    a = -0.5
    t = np.abs(t)
    near = ((a + 2.0) * t - (a + 3.0)) * t * t + 1
    far = (((t - 5) * t + 8) * t - 4) * a
    return np.where(t < 1.0, near, np.where(t < 2.0, far, 0.0))


def tables(n_in, n_out):
    """-> (int32 [n_out, ksize] fixed-point weights, int32 [n_out, 2] (first input index, count))."""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ksize = int(np.ceil(support)) * 2 + 1
    center = (np.arange(n_out, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)             # astype truncates, as the C cast
    count = np.minimum((center + support + 0.5).astype(np.int64), n_in) - xmin
    x = np.arange(ksize, dtype=np.int64)[None, :]
    inside = x < count[:, None]
    w = np.where(inside, _bicubic((x + xmin[:, None] - center[:, None] + 0.5) / fs), 0.0)
    ww = np.zeros(n_out, dtype=np.float64)
    for c in range(ksize):                                                      # ascending; the zeros past count add nothing
        ww = ww + w[:, c]
    w = np.where((ww != 0.0)[:, None], w / np.where(ww != 0.0, ww, 1.0)[:, None], w)
    fixed = np.where(w < 0, -0.5 + w * (1 << BITS), 0.5 + w * (1 << BITS)).astype(np.int64)      # truncation toward zero
    fixed = np.where(inside, fixed, 0)
    return fixed.astype(np.int32), np.stack([xmin, count], 1).astype(np.int32)


def _pass(img, k, b, axis):
    """One pass along ``axis`` of img uint8 [T,H,W,3] -> uint8 with that axis at len(k)."""
    src = np.moveaxis(img, axis, 1).astype(np.int64)                             # [T, n_in, ...]
    out = np.empty((src.shape[0], k.shape[0]) + src.shape[2:], dtype=np.uint8)
    for o in range(k.shape[0]):
        lo, n = int(b[o, 0]), int(b[o, 1])
        acc = np.tensordot(src[:, lo:lo + n], k[o, :n].astype(np.int64), axes=([1], [0])) + (1 << (BITS - 1))
        assert np.abs(acc).max() < 2 ** 31                                      # the kernel's accumulator is int32, as Pillow's
        out[:, o] = np.clip(acc >> BITS, 0, 255)                                 # >> of a negative int64 is arithmetic
    return np.moveaxis(out, 1, axis)


def norm_table():
    """float32 [256,3]: dataset.VideoTransform's own expression for every byte value."""
    v = torch.arange(256, dtype=torch.uint8).view(1, 256, 1).expand(3, 256, 1).contiguous()
    mean, std = torch.tensor(D._MEAN).view(3, 1, 1), torch.tensor(D._STD).view(3, 1, 1)
    return ((v.float().div_(255.0) - mean) / std)[:, :, 0].t().contiguous().numpy()


def centre_crop(h, w, S):
    return int(round((h - S) / 2.0)), int(round((w - S) / 2.0))


def prepare(frames, S, train=False, crop=None, flip=False, max_size=448):
    """frames uint8 [T,H,W,3] -> dict: "out" float32 [T,3,S,S], "resized" uint8 [T,h,w,3] (after both passes),
    "mid" uint8 [T,H,w,3] (after the horizontal pass), "cropped" uint8 [T,S,S,3] (after crop and flip), "size" (w, h),
    "crop" (i, j)."""
    frames = np.ascontiguousarray(frames)
    T, H, W, _ = frames.shape
    w, h = D._resize_size(W, H, int(S * 1.1) if train else S, max_size)
    mid = frames if w == W else _pass(frames, *tables(W, w), axis=2)
    resized = mid if h == H else _pass(mid, *tables(H, h), axis=1)
    i, j = crop if crop is not None else centre_crop(h, w, S)
    cropped = np.zeros((T, S, S, 3), dtype=np.uint8)
    y0, y1, x0, x1 = max(i, 0), min(i + S, h), max(j, 0), min(j + S, w)
    if y0 < y1 and x0 < x1:
        cropped[:, y0 - i:y1 - i, x0 - j:x1 - j] = resized[:, y0:y1, x0:x1]
    if flip:
        cropped = cropped[:, :, ::-1]
    cropped = np.ascontiguousarray(cropped)
    lut = norm_table()
    out = np.stack([lut[cropped[..., c], c] for c in range(3)], 1)              # [T,3,S,S]
    return {"out": np.ascontiguousarray(out, dtype=np.float32), "resized": resized, "mid": mid, "cropped": cropped,
            "size": (w, h), "crop": (i, j)}
