"""A float64 NumPy restatement of avsep_spec_image's rule (include/avsep.h), written from the reference's
utils.py:90-98 (magnitude2heatmap) and main.py:352-386 (mask product, clip * 255, the [::-1] flips): the product is taken in
f32 as the kernel takes it, everything after it is float64 and the level is floor.  And the per-pixel gate the GPU tests
hold the kernel to.  A plain helper module: no tests, no fixtures, the package is not imported here.

The gate.  A pixel's level must equal the float64 floor, except where the float64 value v lies within BAND of an integer;
there either neighbour passes.  BAND is derived, not measured: v <= 300 wherever it is not saturated anyway, and the f32
rounding of c + 1, of log10f and of the multiply by the scale together stay below about 5e-7 relative, i.e. 1.5e-4 in
level units; 1e-3 leaves a factor of six.  An f32 mean adds its own share: a sum of n non-negative terms in any fixed order
is within k * 6e-8 relative of the exact one, k = the additions on the longest path to the result.  That is k = cell - 1 in
frame order (cell <= 32: at most 1.9e-6 relative, 5.6e-4 level units at v = 300 on the linear scale, 1.6e-4 on the log
scale at scale 200, where dv = scale / ln 10 * relative) and k = ceil(cell / 64) + 5 for the lane-strided sum and butterfly
of longer cells.  With the 1.5e-4 above, the band covers every staged cell on both scales, and long cells up to about
2 600 frames on the linear scale and 10 000 on the log scale at scale 200; the mean cases of the GPU tests (cells 2 ... 33
on both scales, 5003 on the log scale: 84 additions, 4.4e-4 + 1.5e-4) lie inside that.  Beyond it the band is NOT derived:
a mean over a longer cell may legitimately leave it, and a test of one would need the wider band this formula gives.  The
maximum adds nothing.  Pixels inside the band may be at most SHARE of a case, so the band cannot carry a wrong kernel."""
import numpy as np

BAND = 1e-3
SHARE = 0.01


def jet_table():
    """Octave's jet(256), uint8 [256,3] RGB: what cv2.COLORMAP_JET tabulates (restated here so that the reference side of a
    comparison does not come from the package under test)."""
    x = 4.0 * np.arange(256, dtype=np.float64) / 256.0
    return np.stack([np.rint(255.0 * np.clip(1.5 - np.abs(x - k), 0.0, 1.0)) for k in (3.0, 2.0, 1.0)], 1).astype(np.uint8)


def values(mag, mask=None, thres=None, cell=1, reduce="max", log=True, scale=200.0):
    """-> float64 [R,F,W], W = ceil(T / cell): v of every pixel, rows already flipped (image row 0 = source row F - 1)."""
    mag = np.asarray(mag, dtype=np.float32)
    if mask is None:
        p = mag
    else:
        mask = np.asarray(mask, dtype=np.float32)
        m = mask if thres is None else (mask > np.float32(thres)).astype(np.float32)
        with np.errstate(all="ignore"):
            p = mag * m                                                  # one f32 multiply
        assert p.dtype == np.float32
    p = p.astype(np.float64)
    R, F, T = p.shape
    W = -(-T // cell)
    c = np.empty((R, F, W), dtype=np.float64)
    for w in range(W):
        seg = p[:, :, w * cell:min((w + 1) * cell, T)]
        c[:, :, w] = seg.max(-1) if reduce == "max" else seg.sum(-1) / seg.shape[-1]
    with np.errstate(all="ignore"):
        v = np.log10(c + 1.0) * float(scale) if log else c * float(scale)
    return v[:, ::-1]


def levels_of(v):
    """floor, saturated at 255; a negative value and a NaN are level 0 -> uint8."""
    with np.errstate(all="ignore"):
        lv = np.where(v > 255.0, 255.0, np.floor(v))
        lv = np.where(np.isnan(v) | (v < 0.0), 0.0, lv)
    return lv.astype(np.uint8)


def image(levels, table=None):
    """levels uint8 [...] -> uint8 [..., 3] through the table, [..., 1] without."""
    return levels[..., None] if table is None else np.asarray(table)[levels]


def spec_image(mag, mask=None, thres=None, cell=1, reduce="max", log=True, scale=200.0, table=None):
    return image(levels_of(values(mag, mask, thres, cell, reduce, log, scale)), table)


def gate(got, v, table=None):
    """got: the kernel's uint8 [R,F,W,ch]; v: values() of the same case.  -> (expected uint8 [R,F,W,ch], the share of
    pixels inside the band).  ``expected`` is the float64 floor everywhere, except that a pixel inside the band takes the
    other neighbour where the kernel gave exactly that: the caller compares with equality."""
    lo, hi = levels_of(v - BAND), levels_of(v + BAND)
    exact = levels_of(v)
    band = lo != hi
    exp = image(exact, table)
    for other in (lo, hi):
        alt = image(other, table)
        take = band & (other != exact) & np.all(np.asarray(got) == alt, axis=-1)
        exp = np.where(take[..., None], alt, exp)
    return exp, float(band.mean())


def draw(shape, seed):
    """Magnitudes 10**(u / 200) - 1 with u uniform in [0, 300) (levels 0 ... 299 under log / 200: the 255 clamp is used) and
    masks uniform in [0, 1), f32."""
    rng = np.random.default_rng(seed)
    mag = (10.0 ** (rng.uniform(0.0, 300.0, shape) / 200.0) - 1.0).astype(np.float32)
    return mag, rng.uniform(0.0, 1.0, shape).astype(np.float32)
