"""not-gpu: the JPEG encoder's rule against Pillow's own files.  The integer restatement (tests/jpeg_encode_ref.py) gives
Pillow's bytes for every grid case; jpeg.encode_header gives Pillow's bytes up to SOS for every quality, form and restart
setting; jpeg.encode_plan's geometry (blocks, dummy blocks, intervals, chunks) is the restatement's; wrong arguments raise."""
import numpy as np
import pytest

from avsep_amd import jpeg
from avsep_amd.lib import AvsepError

import jpeg_encode_cases as EC
import jpeg_encode_ref as R


def test_restatement_writes_pillows_files():
    cases, want, got = EC.grid(), EC.grid_pillow(), EC.grid_reference()
    assert len(cases) >= 100
    for form, _ in EC.FORMS:                                                  # every axis value occurs with every form
        names = [n for n, _, _ in cases if f"-{form}-" in n]
        for H, W in EC.SIZES:
            assert any(n.startswith(f"{H}x{W}-") for n in names), (form, H, W)
        for tag in [f"-q{q}-" for q in EC.QUALITIES] + [f"-{r}" for r, _ in EC.RESTARTS] + [f"-{c}-" for c in EC.CONTENTS]:
            assert any(tag in n for n in names), (form, tag)
    for (name, _, _), w, g in zip(cases, want, got):
        assert g.file == w, name
    # the grid holds what it is meant to hold: dummy blocks, ZRL runs, streams dense in 0xFF
    by_name = {n: g for (n, _, _), g in zip(cases, got)}
    assert by_name["24x5-420-noise-q100-1row"].dummy.sum() == 5 and by_name["17x23-420-noise-q100-1mcu"].dummy.any()
    zrl = by_name["40x48-grey-basis77-q95-1row"]
    assert (zrl.coef[:, 40:63] == 0).all() and (zrl.coef[:, 63] != 0).all()
    dense = by_name["40x48-444-noise-q100-none"].file
    assert dense.count(b"\xff\x00") > len(dense) // 256                      # more stuffed bytes than random bytes would have


@pytest.mark.parametrize("form,sub", EC.FORMS)
def test_header_is_pillows_up_to_sos(form, sub):
    grey = form == "grey"
    for H, W in ((1, 1), (17, 23), (40, 48)):
        a = EC.content("smooth", H, W, grey)
        for q in range(1, 101):
            for _, restart in (EC.RESTARTS if q % 10 == 5 or (H, W) == (17, 23) else EC.RESTARTS[:1]):
                f = EC.pillow_file(a, **EC.pillow_args(sub, q, restart))
                end = f.index(b"\xff\xda")
                end += 2 + int.from_bytes(f[end + 2:end + 4], "big")
                got = jpeg.encode_header(a.shape, q, 2 if sub is None else sub, **restart)
                assert got == f[:end], (form, H, W, q, restart)
                assert got == R.header(a.shape, q, 2 if sub is None else sub, **restart)
    assert jpeg.encode_header((8, 8, 3)) == jpeg.encode_header((8, 8, 3), 75, "4:2:0", 0, 0)
    assert jpeg.encode_header((8, 8, 3), 75, "4:2:2") == jpeg.encode_header((8, 8, 3), 75, 1)


def test_plan_geometry_is_the_restatements():
    cases, ref = EC.grid(), EC.grid_reference()
    shapes = [a.shape for _, a, _ in cases]
    keys = ("quality", "subsampling", "restart_blocks", "restart_rows")
    args = {k: [kw[k] for _, _, kw in cases] for k in keys}
    p = jpeg.encode_plan(shapes, **args)
    assert len(p.chunks) == 1 and len(p.chunks[0].images) == len(cases)
    ch = p.chunks[0]
    assert ch.blocks == sum(len(r.bits) for r in ref) and ch.intervals == sum(len(r.intervals) for r in ref)
    for (name, a, kw), r, row, header, form in zip(cases, ref, ch.images, p.headers, p.forms):
        ncomp, hs, vs, mcux, mcuy, restart = R.geometry(a.shape, kw["subsampling"], kw["restart_blocks"], kw["restart_rows"])
        assert (row["ncomp"], row["hs"], row["vs"], row["mcux"], row["mcuy"], row["restart"]) == (ncomp, hs, vs, mcux, mcuy, restart), name
        assert form == (a.shape[0], a.shape[1], ncomp, hs, vs, mcux, mcuy, restart) and r.file.startswith(header), name
        # the interval boundaries, in blocks from the image's first
        per_mcu = hs * vs + ncomp - 1
        per = restart if restart else mcux * mcuy
        mine = [(k * per * per_mcu, (min((k + 1) * per, mcux * mcuy) - k * per) * per_mcu) for k in range(-(-mcux * mcuy // per))]
        assert mine == [(b0, n) for b0, n, _ in r.intervals], name
        # the dummy blocks: luma blocks beyond the picture's blocks
        dummy = []
        for m in range(mcux * mcuy):
            for i in range(per_mcu):
                dummy.append(i < hs * vs and not ((m // mcux) * vs + i // hs < -(-a.shape[0] // 8) and (m % mcux) * hs + i % hs < -(-a.shape[1] // 8)))
        assert np.array_equal(np.array(dummy), r.dummy), name
    starts = np.concatenate([[0], np.cumsum([len(r.bits) for r in ref])])
    assert np.array_equal(ch.images["block0"], starts[:-1])
    assert np.array_equal(ch.images["interval0"], np.concatenate([[0], np.cumsum([len(r.intervals) for r in ref])])[:-1])
    assert np.array_equal(ch.images["pix_off"], p.offsets[:-1]) and p.pixel_bytes == sum(a.size for _, a, _ in cases)
    # a small cap: chunks of whole images, each within the cap, blocks and intervals counted from 0 again
    cap = 1600 * 128
    small = jpeg.encode_plan(shapes, cap=cap, **args)
    assert len(small.chunks) >= 3 and [c.a for c in small.chunks[1:]] == [c.b for c in small.chunks[:-1]]
    assert small.chunks[0].a == 0 and small.chunks[-1].b == len(cases)
    for c in small.chunks:
        assert c.blocks <= 1600 and c.images["block0"][0] == 0 and c.images["interval0"][0] == 0
        assert c.blocks == sum(len(r.bits) for r in ref[c.a:c.b]) and c.intervals == sum(len(r.intervals) for r in ref[c.a:c.b])
    assert np.array_equal(np.concatenate([c.images["pix_off"] for c in small.chunks]), p.offsets[:-1])
    with pytest.raises(AvsepError, match="more than the workspace cap"):
        jpeg.encode_plan(shapes, cap=1000 * 128, **args)                      # the 4:4:4 strip alone has 1539 blocks


def test_wrong_arguments_raise():
    ok = (16, 16, 3)
    for bad in (dict(quality=0), dict(quality=101), dict(quality="keep"), dict(quality=75.0), dict(subsampling=3),
                dict(subsampling="4:1:1"), dict(subsampling=None), dict(restart_blocks=-1), dict(restart_blocks=65536),
                dict(restart_rows=-1), dict(restart_rows=1.5)):
        with pytest.raises(AvsepError):
            jpeg.encode_header(ok, **bad)
        with pytest.raises(AvsepError):
            jpeg.encode_plan([ok], **bad)
    for shape in ((16,), (16, 16, 4), (16, 16, 1), (0, 16), (16, 0, 3), (jpeg.MAX_SIDE + 1, 8), (8, jpeg.MAX_SIDE + 1, 3), (2, 16, 16, 3)):
        with pytest.raises(AvsepError):
            jpeg.encode_header(shape)
        with pytest.raises(AvsepError):
            jpeg.encode_plan([shape])
    with pytest.raises(AvsepError):
        jpeg.encode_plan([])
    with pytest.raises(AvsepError):
        jpeg.encode_plan([ok, ok], quality=[75])
    with pytest.raises(AvsepError):
        jpeg.encode_plan([ok], cap=64)
    with pytest.raises(TypeError):
        jpeg.encode_plan([ok], optimize=True)
    with pytest.raises(TypeError):
        jpeg.encode([], progressive=True)
    import torch
    with pytest.raises(AvsepError):                                           # no CPU fallback
        jpeg.encode([torch.zeros(16, 16, 3, dtype=torch.uint8)])
    with pytest.raises(AvsepError):
        jpeg.encode(torch.zeros(2, 16, 16, 4, dtype=torch.uint8))
    # the library's own check of the rows
    p = jpeg.encode_plan([ok, (9, 40)], restart_blocks=[2, 0])
    from avsep_amd import kernels as K
    ch = p.chunks[0]
    K.jpeg_enc_plan_check(ch.images, p.pixel_bytes, len(p.tables), ch.blocks, ch.intervals)
    for field, value in (("mcux", 2), ("hs", 3), ("H", 0), ("block0", 1), ("interval0", 5), ("pix_off", p.pixel_bytes), ("restart", -1)):
        rows = ch.images.copy()
        rows[field][1] = value
        with pytest.raises(AvsepError):
            K.jpeg_enc_plan_check(rows, p.pixel_bytes, len(p.tables), ch.blocks, ch.intervals)
    rows = ch.images.copy()
    rows["ac"][0][2] = len(p.tables) - 255
    with pytest.raises(AvsepError):
        K.jpeg_enc_plan_check(rows, p.pixel_bytes, len(p.tables), ch.blocks, ch.intervals)
    with pytest.raises(AvsepError):
        K.jpeg_enc_plan_check(ch.images, p.pixel_bytes, len(p.tables), ch.blocks + 1, ch.intervals)


def test_both_planners_lay_pictures_out_alike():
    """jpeg.plan over Pillow's files and jpeg.encode_plan over the same shapes and settings: the same rows, chunks and counts."""
    cases = [(EC.content("smooth", H, W, sub is None), sub, restart) for H, W in ((1, 1), (8, 8), (17, 23), (9, 40), (33, 65))
             for _, sub in EC.FORMS for _, restart in EC.RESTARTS]
    assert len(cases) == 80
    files = [EC.pillow_file(a, **EC.pillow_args(sub, 75, restart)) for a, sub, restart in cases]
    args = dict(subsampling=[2 if sub is None else sub for _, sub, _ in cases],
                restart_blocks=[r.get("restart_blocks", 0) for _, _, r in cases], restart_rows=[r.get("restart_rows", 0) for _, _, r in cases])
    for cap, chunks in ((jpeg.WORKSPACE_CAP, 1), (200 * 128, 13), (135 * 128, 20)):    # 135 blocks: 33 x 65 at 4:4:4, the largest
        d, e = jpeg.plan(files, cap), jpeg.encode_plan([a.shape for a, _, _ in cases], cap=cap, **args)
        assert not d.fallback and len(d.images) == 80
        assert [(c.a, c.b) for c in d.chunks] == [(c.a, c.b) for c in e.chunks] and len(d.chunks) == chunks
        for c, f in zip(d.chunks, e.chunks):
            assert c.blocks == f.blocks and len(c.segs) == f.intervals == c.intervals, (cap, c.a)
        rows = np.concatenate([c.images for c in e.chunks])
        for field in "H W ncomp hs vs mcux mcuy restart block0 interval0".split():
            assert np.array_equal(d.images[field], rows[field]), (cap, field)
        # interval0 is where the image's segment rows begin
        for c in d.chunks:
            first = [int(np.flatnonzero(c.segs["image"] == r)[0]) for r in range(c.b - c.a)]
            assert np.array_equal(d.images["interval0"][c.a:c.b], first), cap
