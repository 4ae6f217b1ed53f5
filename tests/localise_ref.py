"""NumPy restatement of the heat-map overlay (include/avsep.h, avsep_heatmap_overlay), written from its five stated steps
and never importing the code under test.  Integer steps in int64, fp32 steps on float32 arrays (NumPy rounds every fp32
operation to nearest and never fuses a multiply with an add)."""
import numpy as np

MEAN = np.array([0.485, 0.456, 0.406], dtype=np.float32)
STD = np.array([0.229, 0.224, 0.225], dtype=np.float32)


def jet_ref():
    """Octave jet(256): entry i, channel k in (3, 2, 1) for (R, G, B) = rint(255 * clip(1.5 - |4 i / 256 - k|, 0, 1))."""
    t = np.empty((256, 3), dtype=np.uint8)
    for i in range(256):
        for ch, k in enumerate((3, 2, 1)):
            t[i, ch] = int(np.rint(255.0 * min(max(1.5 - abs(4.0 * i / 256.0 - k), 0.0), 1.0)))
    return t


def levels(m):
    """Step 1: float32 [h,w] -> uint8 levels; a constant map is level 0."""
    m = np.asarray(m, dtype=np.float32)
    mn, mx = m.min(), m.max()
    if mx == mn:
        return np.zeros(m.shape, dtype=np.uint8)
    q = (np.float32(255.0) * (m - mn)) / (mx - mn)
    assert q.dtype == np.float32
    return np.trunc(q).astype(np.uint8)


def _axis(n, N):
    X = np.arange(N, dtype=np.int64)
    num = (2 * X + 1) * n - N
    x0 = num // (2 * N)                      # floor
    rem = num - x0 * 2 * N
    c1 = (rem * 2048 + N) // (2 * N)
    return np.clip(x0, 0, n - 1), np.clip(x0 + 1, 0, n - 1), 2048 - c1, c1


def resize_levels(q, H, W):
    """Step 2: uint8 [h,w] -> uint8 [H,W]."""
    q = np.asarray(q).astype(np.int64)
    h, w = q.shape
    y0, y1, cy0, cy1 = _axis(h, H)
    x0, x1, cx0, cx1 = _axis(w, W)
    acc = (q[y0][:, x0] * cx0[None] * cy0[:, None] + q[y0][:, x1] * cx1[None] * cy0[:, None]
           + q[y1][:, x0] * cx0[None] * cy1[:, None] + q[y1][:, x1] * cx1[None] * cy1[:, None] + (1 << 21)) >> 22
    return acc.astype(np.uint8)


def frame_pixels(x):
    """Step 4: normalised float32 [3,H,W] -> uint8 [H,W,3], rounded and clamped."""
    x = np.asarray(x, dtype=np.float32)
    v = (x * STD[:, None, None] + MEAN[:, None, None]) * np.float32(255.0) + np.float32(0.5)
    assert v.dtype == np.float32
    return np.clip(np.floor(v), 0, 255).astype(np.uint8).transpose(1, 2, 0)


def normalise(img):
    """uint8 [H,W,3] -> float32 [3,H,W] as dataset.py does it (/255, - mean, / std, all float32)."""
    x = np.asarray(img, dtype=np.uint8).transpose(2, 0, 1).astype(np.float32) / np.float32(255.0)
    return (x - MEAN[:, None, None]) / STD[:, None, None]


def overlay(m, frame, table, alpha256):
    """All five steps for one map [h,w] over one normalised frame [3,H,W] -> uint8 [H,W,3]."""
    H, W = frame.shape[-2:]
    level = resize_levels(levels(m), H, W)
    colour = np.asarray(table, dtype=np.uint8)[level].astype(np.int64)          # step 3
    p = frame_pixels(frame).astype(np.int64)
    return ((colour * alpha256 + p * (256 - alpha256) + 128) >> 8).astype(np.uint8)
