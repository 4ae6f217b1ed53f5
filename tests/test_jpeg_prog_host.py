"""not-gpu: the host side of the progressive JPEG decoder.  jpeg.probe_scans reads every scan of a SOF2 file and refuses, with
the reason, what avsep_jpeg_scans does not decode; the NumPy restatement of the four scan paths (tests/jpeg_prog_ref.py) gives
the coefficients of each file's baseline twin and, through jpeg_ref's pixel stage, Pillow's pixels of the progressive file;
jpeg.plan(..., progressive=True) packs scan rows with their levels, and avsep_jpeg_scan_check refuses every row outside its
rules or buffers; and the scan decoder itself (csrc/jpeg_parts.h: jp_decode_scan), compiled with the host compiler under the
address and undefined-behaviour sanitizers into a stand-alone program, decodes the grid and the written files to the
restatement's coefficients and ends every damaged input with its status set and no sanitizer report.
tests/test_gpu_jpeg_prog.py holds the kernels against the same restatement."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import avsep_amd as P
from avsep_amd import jpeg

import jpeg_cases as JC
import jpeg_prog_cases as PC
import jpeg_prog_ref as PR
import jpeg_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _script(info):
    return [(tuple(s.comps), s.ss, s.se, s.ah, s.al) for s in info.scans]


# ---- probe_scans -------------------------------------------------------------------------------------------------------
def test_probe_scans_fields_on_the_grid():
    files, ref = PC.grid(), PC.grid_reference()
    assert len(files) == 75
    for (name, d, twin), (info, _, _) in zip(files, ref):
        base = jpeg.probe(twin)
        assert (info.H, info.W, info.components) == (base.H, base.W, base.components), name
        assert all(np.array_equal(info.qtables[k], base.qtables[k]) for k in base.qtables), name
        assert _script(info) == (PC.PILLOW_GREY if len(info.components) == 1 else PC.PILLOW_COLOUR), name
        hs, vs, mcux, mcuy, _ = jpeg.geometry(base)
        for s in info.scans:
            assert d[s.begin - 3:s.begin] == bytes([s.ss, s.se, s.ah << 4 | s.al]) and d[s.end] == 0xFF and d[s.end + 1] not in (0, 0xFF)
            assert s.restart == base.restart and (s.tables[0] is None) == (s.ss == 0 and s.ah > 0), name
            c = s.comps[0]
            real = -(-(info.W if c == 0 else -(-info.W // hs)) // 8) * -(-(info.H if c == 0 else -(-info.H // vs)) // 8)
            assert s.units == (mcux * mcuy if len(s.comps) > 1 else real), name
            want = -(-s.units // s.restart) - 1 if s.restart else 0
            assert len(s.rst) == want and all(d[p] == 0xFF and d[p + 1] == 0xD0 + k % 8 for k, p in enumerate(s.rst)), name
            segs = jpeg.scan_segments(s)
            assert sum(n for _, _, _, n in segs) == s.units and segs[0][0] == s.begin and segs[-1][1] == s.end
        assert d[info.scans[-1].end:info.scans[-1].end + 2] == b"\xff\xd9"
    # the real block grid differs from the MCU-padded one in the grid: 17 x 23 at 4:2:0 has 3 x 3 luma blocks in a 4 x 4 workspace
    info = ref[[n for n, _, _ in files].index("17x23-420")][0]
    assert info.scans[1].units == 9 and info.scans[0].units == 4 and jpeg._form(info).blocks == 24


def test_levels_of_every_script():
    names = [n for n, _, _ in PC.grid()]
    colour, grey = (PC.grid_reference()[names.index(n)][0] for n in ("33x65-420", "33x65-grey"))
    assert [s.level for s in colour.scans] == [0, 0, 0, 0, 0, 1, 1, 1, 1, 2]
    assert [s.level for s in grey.scans] == [0, 0, 0, 1, 1, 2]
    for name, _, info, _ in PC.written():
        script = name.split("/")[1]
        assert [s.level for s in info.scans] == PC.SCRIPT_LEVELS[script], name
        assert [(tuple(s.comps), s.ss, s.se, s.ah, s.al) for s in info.scans] == [e[:5] for e in PC.SCRIPTS[script]]
        if script == "restarts-differ":
            assert [s.restart for s in info.scans] == [e[5] for e in PC.SCRIPTS[script]]


def _drop_last_scan(d, info):
    return d[:info.scans[-2].end] + b"\xff\xd9"


def test_probe_scans_refuses_with_the_reason():
    names = [n for n, _, _ in PC.grid()]
    k = names.index("33x65-420")
    good, info = PC.grid()[k][1], PC.grid_reference()[k][0]
    co = PC.grid_reference()[k][2]

    def written(script, **kw):
        return PC.write_progressive(co, info, script, **kw)

    def sos(ss, se, ah, al, comps=b"\x01\x00"):
        """good with the parameters (and components) of its scan 1, the first luma AC scan, replaced"""
        s = info.scans[1]
        return good[:s.begin - 3 - len(comps)] + comps + bytes([ss, se, ah << 4 | al]) + good[s.begin:]

    dqt = good.index(b"\xff\xdb")
    dqt_len = struct.unpack(">H", good[dqt + 2:dqt + 4])[0]
    many = [((0, 1, 2), 0, 0, 0, 0)] + [((c,), k, k, 0, 0) for c in range(3) for k in range(1, 64)]
    cases = [(_drop_last_scan(good, info), "incomplete progression: coefficient 1 of component 0 ends at Al=1"),
             (written(PC.SCRIPTS["dc-al0"][:-1]), "incomplete progression: coefficient 1 of component 2 has no scan"),
             (good[:info.scans[2].end] + good[dqt:dqt + 2 + dqt_len] + good[info.scans[2].end:], "quantisation table after the first scan"),
             (written(many), f"more than {jpeg.MAX_SCANS} scans"),
             (PC.grid()[k][2], "not progressive"),
             (sos(0, 5, 0, 2), "a band outside"), (sos(6, 5, 0, 2), "a band outside"), (sos(1, 64, 0, 2), "a band outside"),
             (sos(1, 5, 0, 14), "bit position above 13"), (sos(1, 5, 1, 0), "coefficient 1 of component 0 has no first scan"),
             (written([((0, 1, 2), 0, 0, 0, 1), ((0,), 1, 63, 0, 2), ((0,), 1, 63, 1, 0)]), "stands at Al=2"),
             (written([((0, 1, 2), 0, 0, 0, 1), ((0,), 1, 63, 0, 2), ((0,), 1, 63, 2, 0)]), "stands at Al=2"),
             (written([((0,), 0, 0, 0, 0), ((1,), 1, 63, 0, 0)]), "AC of component 1 before its DC"),
             (written([((1, 0, 2), 0, 0, 0, 0)]), "out of frame order"),
             (written([((0, 1), 0, 0, 0, 0), ((0,), 0, 0, 0, 0)]), "stands at Al=0"),
             (good[:info.scans[-1].end], "no EOI"),
             (good[:info.scans[4].begin + 5], "no EOI"),
             (good.replace(b"\xff\xc2", b"\xff\xca", 1), "SOF10"),
             (JC.encode(JC.picture(8, 8), fmt="PNG"), "not a JPEG")]
    for d, reason in cases:
        with pytest.raises(jpeg.Unsupported, match=reason):
            jpeg.probe_scans(d)
    # restart markers must match every scan's own interval, and stand in order
    rst = PC.grid()[names.index("33x65-420rst")][1]
    ri = jpeg.probe_scans(rst)
    p = int(ri.scans[1].rst[2])
    with pytest.raises(jpeg.Unsupported, match="restart markers out of order"):
        jpeg.probe_scans(rst[:p + 1] + b"\xd5" + rst[p + 2:])
    dri = rst.index(b"\xff\xdd")
    with pytest.raises(jpeg.Unsupported, match="scan 0: 7 restart markers where the interval of 3 units asks for 4"):
        jpeg.probe_scans(rst[:dri + 4] + b"\x00\x03" + rst[dri + 6:])
    # an AC scan over two components: the header of the DC scan with a band
    s0 = info.scans[0]
    with pytest.raises(jpeg.Unsupported, match="an AC scan takes one"):
        jpeg.probe_scans(good[:s0.begin - 3] + bytes([1, 5, 0]) + good[s0.begin:])
    assert all("\n" not in str(e) for e in [jpeg.Unsupported("x")])


# ---- the restatement ---------------------------------------------------------------------------------------------------
def test_restatement_equals_the_baseline_twin_and_pillow():
    for (name, d, twin), (info, px, co) in zip(PC.grid(), PC.grid_reference()):
        base = jpeg.probe(twin)
        for a, b in zip(co, R.coefficients(base, twin)):
            assert np.array_equal(a, b), name
        assert np.array_equal(R.colour(info, R.planes(info, co)), px), name                  # Pillow's decode of the PROGRESSIVE file
        assert np.array_equal(px, JC.pillow(twin)), name


def test_restatement_reads_back_what_the_writer_wrote():
    assert len(PC.written()) == 2 * len(PC.SCRIPTS)
    for name, d, info, co in PC.written():
        got = PR.coefficients(info, d)
        assert all(np.array_equal(a, b) for a, b in zip(got, co)), name
        assert np.array_equal(R.colour(info, R.planes(info, got)), JC.pillow(d)), name


# ---- plan --------------------------------------------------------------------------------------------------------------
def _mixed():
    names = [n for n, _, _ in PC.grid()]
    prog = [PC.grid()[names.index(n)][1] for n in ("33x65-420rst", "17x23-grey", "9x40-444")]
    base = [JC.grid()[k][1] for k in (30, 51)]                              # 17 x 23 and 33 x 65 at 4:2:0
    png = JC.encode(JC.picture(5, 7), fmt="PNG")
    return [prog[0], base[0], png, prog[1], base[1], prog[2]]


def test_plan_without_the_flag_is_unchanged():
    files = _mixed()
    p = jpeg.plan(files)
    assert p.fallback == [0, 2, 3, 5] and all("progressive" in p.reasons[i] for i in (0, 3, 5)) and p.index == [1, 4]
    assert all(len(ch.scans) == 0 and ch.scans.dtype == jpeg.SCAN for ch in p.chunks)
    q = jpeg.plan([files[1], files[4]])
    assert np.array_equal(p.bytes, q.bytes) and np.array_equal(p.tables, q.tables) and np.array_equal(p.chunks[0].segs, q.chunks[0].segs)
    assert all(p.images[f].tolist() == q.images[f].tolist() for f in jpeg.IMAGE.names if f != "pix_off") and p.shapes[1] == q.shapes[0]


def test_plan_with_the_flag_rows_scan_rows_tables_and_chunks():
    files = _mixed()
    p = jpeg.plan(files, progressive=True)
    assert p.fallback == [2] and "not a JPEG" in p.reasons[2] and p.index == [0, 1, 3, 4, 5] and len(p.chunks) == 1
    ch = p.chunks[0]
    infos = {0: jpeg.probe_scans(files[0]), 2: jpeg.probe_scans(files[3]), 4: jpeg.probe_scans(files[5])}   # by row
    blocks = [90, jpeg._form(jpeg.probe(files[1])).blocks, 9, jpeg._form(jpeg.probe(files[4])).blocks, 30]
    assert p.images["block0"].tolist() == np.concatenate([[0], np.cumsum(blocks)[:-1]]).tolist() and ch.blocks == sum(blocks)
    assert p.images["pix_off"].tolist() == [int(p.offsets[i]) for i in p.index]
    assert p.images["restart"][[0, 2, 4]].tolist() == [0, 0, 0]
    assert len(ch.segs) == 2 and ch.segs["image"].tolist() == [1, 3]
    # one scan row per (scan, restart interval), in rising order of level; the bytes are the scans' bytes back to back
    rows = ch.scans
    assert rows.dtype.itemsize == 72 and (np.diff(rows["level"]) >= 0).all()
    for r, info in infos.items():
        mine = rows[rows["image"] == r]
        assert len(mine) == sum(len(s.rst) + 1 for s in info.scans)
        at = 0
        order = np.lexsort((mine["unit0"], mine["begin"]))
        mine = mine[order]
        for s in info.scans:
            for b, e, u0, n in jpeg.scan_segments(s):
                row = mine[at]
                at += 1
                assert (row["ss"], row["se"], row["ah"], row["al"], row["level"]) == (s.ss, s.se, s.ah, s.al, s.level)
                assert row["comps"] == sum(1 << c for c in s.comps) and (row["unit0"], row["units"]) == (u0, n)
                assert bytes(p.bytes[int(row["begin"]):int(row["end"])]) == files[p.index[r]][b:e]
                for c, t in zip(s.comps, s.tables):
                    if t is not None:
                        assert np.array_equal(p.tables[row["table"][c]:][:jpeg.HUFF_WORDS], jpeg.huffman_words(*t))
    # the image row of a progressive file points at a valid table; equal tables are shared (the two 4:4:4 / 4:2:0 quantisers)
    assert all(0 <= int(v) <= len(p.tables) - jpeg.HUFF_WORDS for v in p.images["dc"].reshape(-1))
    assert p.images["quant"][[0, 1, 3, 4]].tolist() == [p.images["quant"][0].tolist()] * 4        # quality 85, progressive or not
    assert p.images["dc"][0].tolist() == p.images["ac"][0].tolist() == [int(rows[rows["image"] == 0]["table"][0][0])] * 3
    # under a small cap the chunks hold their own rows, image indices counted per chunk
    small = jpeg.plan(files, cap=100 * 128, progressive=True)
    assert [(c.a, c.b, c.blocks, len(c.scans), len(c.segs)) for c in small.chunks] == [(0, 1, 90, 140, 0), (1, 3, 33, 6, 1),
                                                                                       (3, 4, 90, 0, 1), (4, 5, 30, 10, 0)]
    assert small.images["block0"].tolist() == [0, 0, 24, 0, 0]
    for c in small.chunks:
        assert c.blocks <= 100 and (len(c.scans) == 0 or int(c.scans["image"].max()) < c.b - c.a)
        assert (np.diff(c.scans["level"]) >= 0).all()
    assert sum(len(c.scans) for c in small.chunks) == len(rows) and sum(len(c.segs) for c in small.chunks) == 2
    tiny = jpeg.plan(files, cap=50 * 128, progressive=True)
    assert 0 in tiny.fallback and "workspace cap" in tiny.reasons[0]


def test_scan_check_refusals():
    L = P.lib.load()
    files = _mixed()
    p = jpeg.plan([files[0], files[3]], progressive=True)
    ch = p.chunks[0]

    def check(images=None, scans=None, **kw):
        images = np.ascontiguousarray(p.images if images is None else images)
        scans = np.ascontiguousarray(ch.scans if scans is None else scans)
        v = dict(nbytes=len(p.bytes), words=len(p.tables), pixels=p.pixel_bytes, blocks=ch.blocks)
        v.update(kw)
        return L.avsep_jpeg_scan_check(images.ctypes.data, len(images), scans.ctypes.data, len(scans), *v.values())

    assert check() == 0
    for kw in (dict(nbytes=len(p.bytes) - 1), dict(words=len(p.tables) - 1), dict(pixels=p.pixel_bytes - 1), dict(blocks=ch.blocks - 1),
               dict(nbytes=0), dict(words=0), dict(pixels=0), dict(blocks=0)):
        assert check(**kw) == -1, kw
    for field, row, value in (("H", 0, 0), ("ncomp", 0, 2), ("mcux", 0, 6), ("block0", 1, 91), ("pix_off", 1, -1)):
        im = p.images.copy()
        im[field][row] = value
        assert check(images=im) == -1, (field, value)
    ac = int(np.flatnonzero((ch.scans["ss"] > 0) & (ch.scans["image"] == 0))[0])
    dc = int(np.flatnonzero((ch.scans["ss"] == 0) & (ch.scans["ah"] == 0) & (ch.scans["image"] == 0))[0])
    grey = int(np.flatnonzero(ch.scans["image"] == 1)[0])
    units = int(ch.scans["units"][ac])
    for field, row, value in (("begin", 0, -1), ("end", 3, len(p.bytes) + 1), ("end", 3, int(ch.scans["begin"][3]) - 1), ("image", 0, 2),
                              ("image", 0, -1), ("comps", ac, 0), ("comps", ac, 8), ("comps", ac, 3), ("comps", grey, 2),
                              ("ss", ac, 64), ("se", ac, 64), ("se", ac, 0), ("se", dc, 1), ("ss", ac, -1), ("ah", ac, 14),
                              ("al", ac, 14), ("ah", ac, 1), ("al", ac, -1), ("level", ac, -1), ("level", ac, 64),
                              ("unit0", ac, -1), ("units", ac, 0), ("unit0", ac, 45), ("units", ac, 46), ("unit0", dc, 15)):
        sc = ch.scans.copy()
        sc[field][row] = value
        assert check(scans=sc) == -1, (field, row, value)
    for value in (-1, len(p.tables) - jpeg.HUFF_WORDS + 1):
        sc = ch.scans.copy()
        sc["table"][ac][0] = value
        assert check(scans=sc) == -1, value
        sc = ch.scans.copy()
        sc["table"][ac][1] = value                   # a component outside the mask: its table is not read
        assert check(scans=sc) == 0
    assert units >= 1 and L.avsep_jpeg_scan_check(None, 1, ch.scans.ctypes.data, 1, 1, 1, 1, 1) == -1
    with pytest.raises(P.lib.AvsepError, match="avsep_jpeg_scan_check refused"):
        P.kernels.jpeg_scan_check(p.images, ch.scans, len(p.bytes), len(p.tables), p.pixel_bytes, ch.blocks - 1)
    assert np.dtype(P.lib.JpegScan).itemsize == 72 and np.dtype(P.lib.JpegImage).itemsize == 96
    hdr = open(os.path.join(ROOT, "include", "avsep.h")).read()
    assert f"#define AVSEP_JPEG_MAX_SCANS {jpeg.MAX_SCANS} " in hdr and jpeg.MAX_SCANS >= 32
    assert set(jpeg.STATUS) == {1 << k for k in range(12)}


# ---- the scan decoder on the CPU, under the sanitizers -------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "the damaged-input test needs a host C++ compiler"
    exe = str(tmp_path_factory.mktemp("jpeg_scan_host") / "jpeg_scan_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(os.path.dirname(P.lib.LIB_PATH), "csrc"),
                    os.path.join(ROOT, "tests", "jpeg_scan_host.cpp"), "-o", exe], check=True)
    return exe


def _run(exe, tmp_path, p, ch, scans=None, levels=None):
    case, dump = str(tmp_path / "case.bin"), str(tmp_path / "dump.bin")
    PC.write_case(case, p, ch, scans, levels)
    r = subprocess.run([exe, case, dump], capture_output=True, text=True)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
    return JC.read_dump(dump, ch.b - ch.a, len(ch.scans if scans is None else scans), ch.blocks)


def test_host_scans_decode_the_grid_and_the_written_files(host_program, tmp_path):
    cases = [(n, d, info, co) for (n, d, _), (info, _, co) in zip(PC.grid(), PC.grid_reference())] + PC.written()
    p = jpeg.plan([d for _, d, _, _ in cases], progressive=True)
    assert not p.fallback and len(p.chunks) == 1 and len(p.chunks[0].segs) == 0
    status, result, coef = _run(host_program, tmp_path, p, p.chunks[0])
    assert not status.any() and not result.any()
    at = 0
    for (name, _, info, co), row in zip(cases, p.images):
        w = R.workspace(info, co)
        assert int(row["block0"]) * 64 == at and np.array_equal(coef[at:at + len(w)], w), name
        at += len(w)
    assert at == len(coef)


def test_host_scans_flag_every_damaged_input(host_program, tmp_path):
    good, bad = PC.damaged()
    expect = {"a scan cut at half": 1, "a scan cut one byte short": 1, "a refinement symbol of size 2": 1024,
              "an end-of-band run past the segment": 2048, "a stray marker": 16}
    p = jpeg.plan([good] + [d for _, d in bad] + [good], progressive=True)
    assert not p.fallback, p.reasons                   # every damaged file passes the markers: it is the lane that meets the damage
    status, result, coef = _run(host_program, tmp_path, p, p.chunks[0])
    info = jpeg.probe_scans(good)
    w = R.workspace(info, PR.coefficients(info, good))
    for r in (0, len(bad) + 1):                        # the good files on either side are whole
        at = int(p.images["block0"][r]) * 64
        assert status[r] == 0 and np.array_equal(coef[at:at + len(w)], w)
    for (name, _), st in zip(bad, status[1:-1]):
        assert st != 0 and all(bit in jpeg.STATUS for bit in (1 << k for k in range(12)) if st & bit), (name, st)
        assert name not in expect or st == expect[name], (name, st)
    # a lane of a later level leaves a flagged image alone: the image whose first AC scan was cut has no refinement applied
    cut = 1 + [n for n, _ in bad].index("a scan cut at half")
    ch = p.chunks[0]
    later = (ch.scans["image"] == cut) & (ch.scans["level"] > 0)
    assert later.any() and not result[later].any()
    # rows the lane must not trust: each one stops with its bit and nothing out of range is touched (the sanitizers watch)
    base = jpeg.plan([good], progressive=True)
    n = len(base.chunks[0].scans)
    ac = int(np.flatnonzero(base.chunks[0].scans["ss"] > 0)[0])
    for field, value, bit in (("block0", 1, 256), ("mcux", 9, 256), ("H", 0, 256)):
        q = jpeg.plan([good], progressive=True)
        q.images[field][0] = value
        assert _run(host_program, tmp_path, q, q.chunks[0])[0][0] == bit, field
    for field, row, value, bit in (("ss", ac, 64, 256), ("se", ac, 64, 256), ("se", 0, 5, 256), ("ah", ac, 1, 256), ("al", ac, 14, 256),
                                   ("comps", ac, 6, 256), ("comps", ac, 8, 256), ("level", ac, 1, 256), ("level", ac, -1, 256),
                                   ("begin", 0, -1, 1), ("end", n - 1, len(base.bytes) + 1, 1), ("units", ac, 46, 32),
                                   ("unit0", ac, -1, 32), ("units", 0, 16, 32), ("units", ac, 30, 512 | 2048), ("image", 0, 1, 0),
                                   ("table", ac, -1, 64), ("table", ac, len(base.tables) - 545, 64)):
        q = jpeg.plan([good], progressive=True)
        sc = q.chunks[0].scans.copy()
        if field == "table":
            sc[field][row][0] = value
        else:
            sc[field][row] = value
        st, res, _ = _run(host_program, tmp_path, q, q.chunks[0], scans=sc, levels=PC.launch_levels(q.chunks[0]))
        assert (st[0] & bit) != 0 and (st[0] & ~bit) == 0 if bit else (st[0] == 0 and res[row] == 256), (field, value, st[0])
    # a band moved by one: the stream no longer fits it, and whatever the lane meets, it stops inside its buffers
    for field, value in (("ss", 2), ("se", 4)):
        q = jpeg.plan([good], progressive=True)
        sc = q.chunks[0].scans.copy()
        sc[field][ac] = value
        assert _run(host_program, tmp_path, q, q.chunks[0], scans=sc)[0][0] != 0, field
