"""The pictures and settings the JPEG encoder's tests share: a thinned product of sizes, forms, qualities, restart settings and
contents in which every value of every axis occurs with every form, Pillow's file for each, and the restatement's stages.
A plain helper module: no fixtures, no tests."""
import functools
import io

import numpy as np

# H x W.  8, 24 and 40 rows: a multiple of 8 but not of 16 (a 4:2:0 file's bottom luma blocks are dummies); the strip and
# 72 x 136 have more blocks than one 256-element tile of the kernels' running sums
SIZES = [(1, 1), (5, 3), (8, 8), (16, 16), (17, 23), (24, 5), (9, 40), (33, 65), (40, 48), (8, 4104), (72, 136)]
FORMS = [("grey", None), ("444", 0), ("422", 1), ("420", 2)]
QUALITIES = [1, 30, 75, 95, 100]
RESTARTS = [("none", {}), ("1mcu", dict(restart_blocks=1)), ("2mcu", dict(restart_blocks=2)), ("1row", dict(restart_rows=1))]
CONTENTS = ["noise", "smooth", "flat0", "flat255", "checker", "basis77"]


def content(name, H, W, grey, seed=0):
    """One picture -> uint8 [H,W] (grey) or [H,W,3]."""
    yy, xx = np.mgrid[0:H, 0:W]
    if name == "noise":                                   # at quality 100 dense in 0xFF bytes
        return np.random.default_rng(seed * 7919 + H * 1009 + W).integers(0, 256, (H, W) if grey else (H, W, 3), dtype=np.uint8)
    if name == "smooth":
        g = (128 + 100 * np.sin(xx / 5.0) * np.cos(yy / 7.0)).astype(np.uint8)
        return g if grey else np.stack([g, 255 - g, (g // 2 + xx) % 256], -1).astype(np.uint8)
    if name in ("flat0", "flat255"):
        return np.full((H, W) if grey else (H, W, 3), 0 if name == "flat0" else 255, dtype=np.uint8)
    if name == "checker":                                 # one-pixel 0 / 255: the largest coefficients
        g = (((yy + xx) & 1) * 255).astype(np.uint8)
        return g if grey else np.stack([g, g, 255 - g], -1)
    if name == "basis77":                                 # flat 128 + the (7,7) basis pattern: 62 zeros before one value, hence ZRL
        g = np.rint(128 + 60 * np.cos((2 * (xx % 8) + 1) * 7 * np.pi / 16) * np.cos((2 * (yy % 8) + 1) * 7 * np.pi / 16)).astype(np.uint8)
        return g if grey else np.stack([g, np.full_like(g, 128), 255 - g], -1)
    raise ValueError(name)


def pillow_args(subsampling, quality, restart):
    kw = dict(quality=quality)
    if subsampling is not None:
        kw["subsampling"] = subsampling
    if "restart_blocks" in restart:
        kw["restart_marker_blocks"] = restart["restart_blocks"]
    if "restart_rows" in restart:
        kw["restart_marker_rows"] = restart["restart_rows"]
    return kw


def pillow_file(a, **kw):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(a).save(b, "JPEG", **kw)
    return b.getvalue()


@functools.lru_cache(maxsize=1)
def grid():
    """-> [(name, picture, dict(quality, subsampling, restart_blocks, restart_rows))] in a fixed order.  Per form: every size
    with two contents, the qualities and restart settings taken in turn; then the cases wanted by name."""
    out = []
    for form, sub in FORMS:
        k = 0
        for i, (H, W) in enumerate(SIZES):
            for what in (CONTENTS[i % 6], CONTENTS[(i + 3) % 6]):
                if (H, W) == (8, 4104) and what != CONTENTS[i % 6] and form in ("444", "422"):
                    continue                              # the strip: one content for these two forms, it is the slowest to restate
                q, (rname, restart) = QUALITIES[k % 5], RESTARTS[k % 4]
                k += 1
                out.append((form, H, W, what, q, rname, restart, sub))
        for (H, W), what, q, r in (((40, 48), "noise", 100, 0), ((17, 23), "noise", 100, 1), ((24, 5), "noise", 100, 3),
                                   ((40, 48), "basis77", 95, 3), ((17, 23), "checker", 100, 2), ((8, 8), "flat255", 1, 1),
                                   ((72, 136), "noise", 100, 2)):
            out.append((form, H, W, what, q, RESTARTS[r][0], RESTARTS[r][1], sub))
    cases = []
    for form, H, W, what, q, rname, restart, sub in out:
        args = dict(quality=q, subsampling=2 if sub is None else sub, restart_blocks=0, restart_rows=0)
        args.update(restart)
        cases.append((f"{H}x{W}-{form}-{what}-q{q}-{rname}", content(what, H, W, form == "grey"), args))
    return cases


@functools.lru_cache(maxsize=1)
def grid_pillow():
    """Pillow's file of every grid case, in grid order."""
    return [pillow_file(a, **pillow_args(None if a.ndim == 2 else kw["subsampling"], kw["quality"],
                                         {k: v for k, v in kw.items() if k.startswith("restart") and v})) for _, a, kw in grid()]


@functools.lru_cache(maxsize=1)
def grid_reference():
    """The restatement's Encoded of every grid case: computed once, read only."""
    import jpeg_encode_ref
    return [jpeg_encode_ref.encode(a, **kw) for _, a, kw in grid()]
