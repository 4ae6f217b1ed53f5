"""not-gpu: the host side of the GPU JPEG decoder.  The NumPy restatement (tests/jpeg_ref.py) equals Pillow byte for byte on the
grid of sizes and forms; jpeg.probe reads the markers and refuses, with the reason, what the kernels do not decode; jpeg.plan
packs segments, shared tables and offsets, and avsep_jpeg_plan_check refuses every range outside its buffer; the loader's
jpeg_bytes form draws what the raw form draws; and the entropy decoder itself (csrc/jpeg_parts.h), compiled with the host compiler
under the address and undefined-behaviour sanitizers into a stand-alone program, decodes the grid to the restatement's
coefficients and ends every damaged input with its status set and no sanitizer report.  tests/test_gpu_jpeg.py holds the kernels
against the same restatement."""
import os
import random
import shutil
import subprocess

import numpy as np
import pytest
import torch

import avsep_amd as P
from avsep_amd import dataset as D
from avsep_amd import jpeg

import jpeg_cases as JC
import jpeg_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement against Pillow ------------------------------------------------------------------------------------
def test_restatement_equals_pillow_on_the_grid():
    files, ref = JC.grid(), JC.grid_reference()
    assert len(files) == 63
    forms = set()
    for (name, d), (info, px, _) in zip(files, ref):
        assert np.array_equal(px, JC.pillow(d)), name
        forms.add((len(info.components), info.components[0][1], info.components[0][2], bool(info.restart)))
    assert forms == {(3, 1, 1, False), (3, 2, 1, False), (3, 2, 2, False), (3, 2, 2, True), (1, 1, 1, False)}


def test_arithmetic_bound_is_the_headers():
    """AVSEP_JPEG_MAX_COEF is what the constants of the inverse DCT give: with the largest sum of absolute weights
    any value of a pass has, G, the column pass stays within int32 for G M + 2^10 < 2^31 and the row pass, whose inputs are at
    most ((G M + 2^10) >> 11) + 1, for G M1 + 2^17 < 2^31."""
    G, _ = R.pass_gain()
    M = R.arith_bound()
    assert (G, M) == (61214, 1173)
    hdr = open(os.path.join(ROOT, "include", "avsep.h")).read()
    assert f"#define AVSEP_JPEG_MAX_COEF {M}\n" in hdr
    for m, fits in ((M, True), (M + 1, False)):
        m1 = ((G * m + 1024) >> 11) + 1
        assert (G * m + 1024 < 2 ** 31 and G * m1 + 2 ** 17 < 2 ** 31) == fits


# ---- probe -------------------------------------------------------------------------------------------------------------
def test_probe_fields():
    d = JC.encode(JC.picture(33, 65), subsampling=2, quality=85, restart_marker_blocks=2)
    info = jpeg.probe(d)
    assert (info.H, info.W, info.restart) == (33, 65, 2)
    assert info.components == [(1, 2, 2, 0), (2, 1, 1, 1), (3, 1, 1, 1)] and info.scan == [(0, 0), (1, 1), (1, 1)]
    assert sorted(info.qtables) == [0, 1] and all(q.shape == (64,) and q.dtype == np.uint8 for q in info.qtables.values())
    assert sorted(info.huffman) == [(0, 0), (0, 1), (1, 0), (1, 1)]
    for counts, values in info.huffman.values():
        assert counts.shape == (16,) and int(counts.sum()) == len(values)
    assert d[info.data_end:info.data_end + 2] == b"\xff\xd9" and d[info.data_begin - 3:info.data_begin] == b"\x00\x3f\x00"
    ones = jpeg.probe(JC.encode(JC.picture(8, 8), subsampling=0, quality=100))
    assert all(np.array_equal(q, np.ones(64, dtype=np.uint8)) for q in ones.qtables.values())
    assert ones.components[0][1:3] == (1, 1)
    g = jpeg.probe(JC.encode(JC.picture(9, 40), grey=True))
    assert g.components == [(1, 1, 1, 0)] and (g.H, g.W, g.restart) == (9, 40, 0)
    assert jpeg.geometry(info) == (2, 2, 5, 3, 90) and jpeg.geometry(g) == (1, 1, 5, 2, 10)


def test_probe_refuses_with_the_reason():
    from PIL import Image
    import io
    good = JC.encode(JC.picture(16, 16), subsampling=2, quality=85)
    info = jpeg.probe(good)
    b = io.BytesIO()
    Image.fromarray(np.dstack([JC.picture(16, 16), JC.picture(16, 16)[:, :, :1]])).convert("CMYK").save(b, "JPEG")
    cases = [(JC.encode(JC.picture(16, 16), progressive=True), "progressive"),
             (b.getvalue(), "4 components"),
             (good[:info.data_begin - 20], "ends before its SOS"),
             (good[:info.data_end], "no EOI"),
             (JC.encode(JC.picture(16, 16), fmt="PNG"), "not a JPEG"),
             (good + good[2:], None)]
    for d, reason in cases[:-1]:
        with pytest.raises(jpeg.Unsupported, match=reason):
            jpeg.probe(d)
    # a second frame after the first EOI is not part of the file's first image: Pillow reads the first, and so does probe
    assert jpeg.probe(cases[-1][0]).data_end == info.data_end
    two_scans = good[:info.data_end] + good[info.data_begin - 14:]
    with pytest.raises(jpeg.Unsupported, match="more than one scan"):
        jpeg.probe(two_scans)
    assert isinstance(jpeg.Unsupported("x"), ValueError) and "\n" not in str(jpeg.Unsupported("one line"))


# ---- plan --------------------------------------------------------------------------------------------------------------
def test_plan_segments_tables_and_offsets():
    a = JC.encode(JC.picture(33, 65), subsampling=2, quality=85, restart_marker_blocks=2)
    b = JC.encode(JC.picture(17, 23), subsampling=2, quality=85)
    c = JC.encode(JC.picture(9, 40), subsampling=0, quality=85)
    png = JC.encode(JC.picture(5, 7), fmt="PNG")
    p = jpeg.plan([a, png, b, c])
    assert p.fallback == [1] and "not a JPEG" in p.reasons[1] and p.index == [0, 2, 3]
    assert p.shapes == [(33, 65), (5, 7), (17, 23), (9, 40)]
    assert p.offsets.tolist() == [0, 33 * 65 * 3, 33 * 65 * 3 + 105, 33 * 65 * 3 + 105 + 17 * 23 * 3, p.pixel_bytes]
    assert p.images["pix_off"].tolist() == [p.offsets[0], p.offsets[2], p.offsets[3]]
    assert p.images["block0"].tolist() == [0, 90, 90 + 24] and len(p.chunks) == 1 and p.chunks[0].blocks == 90 + 24 + 30
    assert (p.chunks[0].max_blocks, p.chunks[0].max_pixels) == (90, 33 * 65)
    # the segments of the first file against its RST markers: 15 MCUs in intervals of 2 -> 8 segments, RST0 .. RST6 between them
    ia = jpeg.probe(a)
    segs = p.chunks[0].segs
    mine = segs[segs["image"] == 0]
    assert len(mine) == 8 and mine["mcu0"].tolist() == list(range(0, 15, 2)) and mine["mcus"].tolist() == [2] * 7 + [1]
    ent = a[ia.data_begin:ia.data_end]
    assert bytes(p.bytes[:len(ent)]) == ent and int(mine["begin"][0]) == 0 and int(mine["end"][-1]) == len(ent)
    for k in range(7):
        assert ent[int(mine["end"][k]):int(mine["begin"][k + 1])] == bytes([0xFF, 0xD0 + k])
    rest = segs[segs["image"] != 0]
    assert rest["image"].tolist() == [1, 2] and rest["mcu0"].tolist() == [0, 0] and rest["mcus"].tolist() == [2 * 2, 5 * 2]
    assert int(rest["begin"][0]) == len(ent) and int(rest["end"][1]) == len(p.bytes)
    # files written with the same settings share their tables; 2 quantisation + 4 Huffman tables in all
    assert p.images["quant"].tolist() == [p.images["quant"][0].tolist()] * 3
    assert p.images["dc"][0].tolist() == p.images["dc"][1].tolist() == p.images["dc"][2].tolist()
    assert len(p.tables) == 2 * jpeg.QUANT_WORDS + 4 * jpeg.HUFF_WORDS
    q0 = p.tables[p.images["quant"][0][0]:][:64]
    assert np.array_equal(q0[R.ZIGZAG], ia.qtables[0])                                       # natural order in the buffer
    # a cap of 100 blocks: one image per chunk, each chunk counting its blocks from 0
    small = jpeg.plan([a, b, c], cap=100 * 128)
    assert [(ch.a, ch.b, ch.blocks) for ch in small.chunks] == [(0, 1, 90), (1, 3, 54)]
    assert small.images["block0"].tolist() == [0, 0, 24] and small.chunks[1].segs["image"].tolist() == [0, 1]
    tiny = jpeg.plan([a, b], cap=50 * 128)                                                   # a does not fit at all: Pillow's
    assert tiny.fallback == [0] and "workspace cap" in tiny.reasons[0] and tiny.index == [1]


def test_huffman_words_decode_every_code():
    info = jpeg.probe(JC.encode(JC.picture(16, 16), subsampling=2, quality=85))
    for counts, values in info.huffman.values():
        w = jpeg.huffman_words(counts, values)
        look, maxcode, valoff, vals = w[:256], w[256:273], w[273:290], w[290:]
        for (length, code), v in R.huffman_codes(counts, values).items():
            assert code <= maxcode[length] and vals[valoff[length] + code] == v
            if length <= 8:
                assert all(look[(code << (8 - length)) + i] == (length << 8 | v) for i in range(1 << (8 - length)))
        assert maxcode[0] == -1


def test_plan_check_refusals():
    L = P.lib.load()
    a = JC.encode(JC.picture(33, 65), subsampling=2, quality=85, restart_marker_blocks=2)
    b = JC.encode(JC.picture(9, 40), grey=True)
    p = jpeg.plan([a, b])
    ch = p.chunks[0]

    def check(images=None, segs=None, **kw):
        images = np.ascontiguousarray(p.images if images is None else images)
        segs = np.ascontiguousarray(ch.segs if segs is None else segs)
        v = dict(nbytes=len(p.bytes), words=len(p.tables), pixels=p.pixel_bytes, blocks=ch.blocks)
        v.update(kw)
        return L.avsep_jpeg_plan_check(images.ctypes.data, len(images), segs.ctypes.data, len(segs), *v.values())

    assert check() == 0
    for kw in (dict(nbytes=len(p.bytes) - 1), dict(words=len(p.tables) - 1), dict(pixels=p.pixel_bytes - 1), dict(blocks=ch.blocks - 1),
               dict(nbytes=0), dict(words=0), dict(pixels=0), dict(blocks=0)):
        assert check(**kw) == -1, kw
    for field, row, value in (("H", 0, 0), ("W", 0, 16385), ("ncomp", 0, 2), ("hs", 0, 3), ("vs", 1, 2), ("mcux", 0, 6), ("mcuy", 0, 2),
                              ("pix_off", 1, -1), ("block0", 1, 91), ("restart", 0, -1), ("restart", 0, 3)):
        im = p.images.copy()
        im[field][row] = value
        assert check(images=im) == -1, (field, value)
    for field in ("quant", "dc", "ac"):
        for value in (-1, len(p.tables) - 63):
            im = p.images.copy()
            im[field][0][2] = value
            assert check(images=im) == -1, (field, value)
    for field, row, value in (("begin", 0, -1), ("end", 8, len(p.bytes) + 1), ("end", 3, int(ch.segs["begin"][3]) - 1), ("image", 0, 2),
                              ("image", 0, -1), ("mcu0", 1, 3), ("mcus", 1, 3), ("mcus", 7, 2), ("mcus", 8, 0), ("mcu0", 8, 1)):
        sg = ch.segs.copy()
        sg[field][row] = value
        assert check(segs=sg) == -1, (field, row, value)
    assert L.avsep_jpeg_plan_check(None, 1, ch.segs.ctypes.data, 1, 1, 1, 1, 1) == -1
    with pytest.raises(P.lib.AvsepError, match="avsep_jpeg_plan_check refused"):
        P.kernels.jpeg_plan_check(p.images, ch.segs, len(p.bytes), len(p.tables), p.pixel_bytes, ch.blocks - 1)
    assert np.dtype(P.lib.JpegImage).itemsize == 96 and np.dtype(P.lib.JpegSegment).itemsize == 32


# ---- the loader --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def disk(tmp_path_factory):
    """The three-size dataset of the raw-frames tests and its loader arguments."""
    import test_frames_batch_host as BH
    lst = BH.make_disk_dataset(tmp_path_factory.mktemp("jpeg"))
    return lst, BH.loader_args()


@pytest.mark.parametrize("split", ["train", "val"])
def test_jpeg_items_draw_what_raw_items_draw(disk, split):
    lst, a = disk
    kw = dict(split=split, seed=a.seed, raw_frames=True)
    raw, byt = D.MUSICMixDataset(lst, vars(a), **kw), D.MUSICMixDataset(lst, vars(a), jpeg_bytes=True, **kw)
    for k, i in ((0, 0), (7, 1), (123, 2), (5, 5)):
        random.seed(k)
        r = raw[i]
        state = random.getstate()
        random.seed(k + 1000)
        j = byt[i]
        assert random.getstate() == state, (split, i)
        assert "frames_u8" not in j and j["id"] == r["id"] and j["infos"] == r["infos"] and torch.equal(j["class"], r["class"])
        assert torch.equal(j["audio_mix"], r["audio_mix"]) and all(torch.equal(x, y) for x, y in zip(j["audios"], r["audios"]))
        assert j["frame_crops"] == r["frame_crops"] and j["frame_flips"] == r["frame_flips"]
        for n in range(2):
            assert torch.equal(j["frame_shapes"][n], r["frame_shapes"][n]) and j["frames_fallback"][n] == []
            assert j["frame_bytes"][n].dtype == torch.int64 and int(j["frame_bytes"][n].sum()) == j["frames_jpeg"][n].numel()
            data, at = j["frames_jpeg"][n].numpy().tobytes(), 0
            for t, nb in enumerate(j["frame_bytes"][n].tolist()):                            # whole files, in time order
                assert data[at:at + 2] == b"\xff\xd8" and data[at + nb - 2:at + nb] == b"\xff\xd9"
                at += nb
    with pytest.raises(ValueError, match="raw_frames"):
        D.MUSICMixDataset(lst, vars(a), split=split, jpeg_bytes=True)


def test_collate_of_a_mixed_batch(disk):
    """One frame file is a PNG under its .jpg name: the worker decodes it, collate carries its pixels and its index."""
    lst, a = disk
    from PIL import Image
    kw = dict(split="val", seed=a.seed, raw_frames=True)
    raw, byt = D.MUSICMixDataset(lst, vars(a), **kw), D.MUSICMixDataset(lst, vars(a), jpeg_bytes=True, **kw)
    before = D.collate([raw[0], raw[1]])
    first = byt[1]
    clip, nb = first["infos"][1][1], first["frame_bytes"][1].tolist()
    middle = first["frames_jpeg"][1].numpy().tobytes()[nb[0]:nb[0] + nb[1]]                  # the file of frame 1 of source 1
    target = next(os.path.join(clip, n) for n in sorted(os.listdir(clip)) if open(os.path.join(clip, n), "rb").read() == middle)
    pixels = JC.pillow(middle)
    try:
        Image.fromarray(pixels).save(target, "PNG")
        items = [byt[0], byt[1]]
        assert [t for t, _ in items[1]["frames_fallback"][1]] == [1] and items[1]["frames_fallback"][0] == []
        out = D.collate(items)
        assert "frames_u8" not in out and "frames" not in out
        B, T = 2, 3
        assert out["fallback_index"].tolist() == [(1 * B + 1) * T + 1]
        assert torch.equal(out["fallback_u8"], torch.from_numpy(pixels.reshape(-1).copy()))
        assert tuple(out["frame_bytes"].shape) == (2, B, T) and int(out["frame_bytes"].sum()) == out["frames_jpeg"].numel()
        assert torch.equal(out["frame_shapes"], before["frame_shapes"]) and torch.equal(out["frame_flips"], before["frame_flips"])
        assert out["frame_crops"] is None and before["frame_crops"] is None and (out["imgSize"], out["split"]) == (64, "val")
        # without jpeg_bytes the raw batch is what it was: same keys, same bytes (the PNG decodes to the same pixels)
        after = D.collate([raw[0], raw[1]])
        assert set(after) == set(before) and "frames_jpeg" not in after and torch.equal(after["frames_u8"], before["frames_u8"])
    finally:
        with open(target, "wb") as f:
            f.write(middle)
    clean = D.collate([byt[0], byt[1]])
    assert clean["fallback_index"].numel() == 0 and clean["fallback_u8"].numel() == 0


# ---- the entropy decoder on the CPU, under the sanitizers ----------------------------------------------------------------
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "the damaged-input test needs a host C++ compiler"
    exe = str(tmp_path_factory.mktemp("jpeg_host") / "jpeg_entropy_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(os.path.dirname(P.lib.LIB_PATH), "csrc"),
                    os.path.join(ROOT, "tests", "jpeg_entropy_host.cpp"), "-o", exe], check=True)
    return exe


def _run(exe, tmp_path, p, ch):
    case, dump = str(tmp_path / "case.bin"), str(tmp_path / "dump.bin")
    JC.write_case(case, p, ch)
    r = subprocess.run([exe, case, dump], capture_output=True, text=True)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
    return JC.read_dump(dump, ch.b - ch.a, len(ch.segs), ch.blocks)


def test_host_entropy_decodes_the_grid(host_program, tmp_path):
    p = jpeg.plan([d for _, d in JC.grid()])
    assert not p.fallback and len(p.chunks) == 1
    status, result, coef = _run(host_program, tmp_path, p, p.chunks[0])
    assert not status.any() and not result.any()
    at = 0
    for (name, _), (info, _, co), row in zip(JC.grid(), JC.grid_reference(), p.images):
        w = R.workspace(info, co)
        assert int(row["block0"]) * 64 == at and np.array_equal(coef[at:at + len(w)], w), name
        at += len(w)
    assert at == len(coef)


def test_host_entropy_flags_every_damaged_input(host_program, tmp_path):
    good, bad = JC.damaged()
    expect = {"cut at half": 1, "cut one byte short": 1, "an AC run past 63": 8, "a DC size of 15": 4, "a stray marker": 16}
    p = jpeg.plan([good] + [d for _, d in bad] + [good])
    assert not p.fallback, p.reasons                   # every damaged file passes the markers: it is the lane that meets the damage
    status, result, coef = _run(host_program, tmp_path, p, p.chunks[0])
    assert status[0] == 0 and status[-1] == 0
    info = jpeg.probe(good)
    w = R.workspace(info, R.coefficients(info, good))
    for r in (0, len(bad) + 1):                        # the good files on either side are whole
        at = int(p.images["block0"][r]) * 64
        assert np.array_equal(coef[at:at + len(w)], w)
    for (name, _), st in zip(bad, status[1:-1]):
        assert st != 0 and st in jpeg.STATUS, (name, st)
        assert name not in expect or st == expect[name], (name, st)
    # rows the lane must not trust: each one stops with its bit and nothing out of range is touched (the sanitizers watch)
    base = jpeg.plan([good])
    for field, value, bit in (("block0", 1, 256), ("mcux", 9, 256), ("H", 0, 256), ("quant", len(base.tables) - 63, 64),
                              ("ac", -1, 64), ("dc", len(base.tables), 64)):
        q = jpeg.plan([good])
        if field in ("quant", "ac", "dc"):
            q.images[field][0][1] = value
        else:
            q.images[field][0] = value
        assert _run(host_program, tmp_path, q, q.chunks[0])[0][0] == bit, field
    for field, value, bit in (("begin", -1, 1), ("end", len(base.bytes) + 1, 1), ("mcus", 16, 32), ("mcu0", -1, 32), ("mcus", 14, 512),
                              ("image", 1, 0)):
        q = jpeg.plan([good])
        q.chunks[0].segs[field][0] = value
        st, res, _ = _run(host_program, tmp_path, q, q.chunks[0])
        assert st[0] == bit and (bit != 0 or res[0] == 256), field
    # a coefficient beyond the bound: the quantiser of the DC term raised until 1173 is passed
    q = jpeg.plan([good])
    q.tables[q.images["quant"][0][0]] = 255
    assert _run(host_program, tmp_path, q, q.chunks[0])[0][0] == 128
