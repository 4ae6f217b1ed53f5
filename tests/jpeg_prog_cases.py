"""The progressive JPEG files the decoder's tests share: Pillow's files over the grid of sizes and forms with their baseline
twins, a test-side scan writer for the scan scripts Pillow cannot write, the damaged set, and the case file the host program of
tests/jpeg_scan_host.cpp reads.  A plain helper module: no fixtures, no tests."""
import functools
import struct

import numpy as np

import jpeg_cases as JC
import jpeg_ref as R

FORMS = [("444", dict(subsampling=0, quality=85)), ("422", dict(subsampling=1, quality=85)), ("420", dict(subsampling=2, quality=85)),
         ("420rst", dict(subsampling=2, quality=85, restart_marker_blocks=2)), ("420q30", dict(subsampling=2, quality=30)),
         ("444q100", dict(subsampling=0, quality=100)), ("grey", dict(grey=True)), ("greyrst", dict(grey=True, restart_marker_blocks=2))]

# Pillow's (libjpeg's jpeg_simple_progression) scripts: (components, Ss, Se, Ah, Al)
PILLOW_COLOUR = [((0, 1, 2), 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((2,), 1, 63, 0, 1), ((1,), 1, 63, 0, 1), ((0,), 6, 63, 0, 2),
                 ((0,), 1, 63, 2, 1), ((0, 1, 2), 0, 0, 1, 0), ((2,), 1, 63, 1, 0), ((1,), 1, 63, 1, 0), ((0,), 1, 63, 1, 0)]
PILLOW_GREY = [((0,), 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((0,), 6, 63, 0, 2), ((0,), 1, 63, 2, 1), ((0,), 0, 0, 1, 0), ((0,), 1, 63, 1, 0)]


def flat(H, W):
    return np.full((H, W, 3), (90, 140, 200), dtype=np.uint8)


def noise(H, W):
    return np.random.default_rng(7).integers(0, 256, (H, W, 3)).astype(np.uint8)


@functools.lru_cache(maxsize=1)
def grid():
    """The progressive grid -> [(name, progressive file, its baseline twin)], in a fixed order: 72 files of the sizes and forms,
    two flat pictures (their AC scans one long end-of-band run, no correction bits) and one of noise at quality 100 (nearly
    every coefficient takes correction bits)."""
    pictures = [(f"{H}x{W}-{name}", JC.picture(H, W), form) for H, W in JC.SIZES for name, form in FORMS]
    pictures += [("40x48-flat", flat(40, 48), dict(subsampling=2)), ("128x128-flat", flat(128, 128), dict(subsampling=2)),
                 ("40x48-noise", noise(40, 48), dict(subsampling=0, quality=100))]
    return [(name, JC.encode(a, progressive=True, **form), JC.encode(a, **form)) for name, a, form in pictures]


@functools.lru_cache(maxsize=1)
def grid_reference():
    """Per grid file (ScanInfo, Pillow's pixels of the PROGRESSIVE file, the restatement's coefficients): computed once, read only."""
    import jpeg_prog_ref as PR
    from avsep_amd import jpeg
    out = []
    for _, d, _ in grid():
        info = jpeg.probe_scans(d)
        out.append((info, JC.pillow(d), PR.coefficients(info, d)))
    return out


# ---- the scan writer ---------------------------------------------------------------------------------------------------
# one fixed table per class that holds every symbol: DC 0 .. 11 in 4 bits; AC 128 symbols in 8 bits and 128 in 9
DC_TABLE = ([0, 0, 0, 12] + [0] * 12, bytes(range(12)))
AC_TABLE = ([0] * 7 + [128, 128] + [0] * 7, bytes(range(256)))


def _codes(counts, values):
    return {v: (length, code) for (length, code), v in R.huffman_codes(counts, values).items()}


class _Out:
    def __init__(self):
        self.bits = []

    def put(self, value, n):
        self.bits += [(value >> (n - 1 - i)) & 1 for i in range(n)]

    def symbol(self, codes, s):
        length, code = codes[s]
        self.put(code, length)

    def segment(self):
        """The bits so far, padded with ones, as stuffed bytes; the writer starts over."""
        bits = self.bits + [1] * (-len(self.bits) % 8)
        self.bits = []
        return bytes(np.packbits(np.array(bits, dtype=np.uint8))).replace(b"\xff", b"\xff\x00") if bits else b""


def _scan_bytes(info, coefs, scan_blocks, table, ss, se, ah, al, restart):
    """The entropy-coded bytes of one scan, RSTn markers between its intervals (libjpeg's jcphuff.c, restated).
    scan_blocks: per unit the [(component, block row, block column)] of the stream's order."""
    codes, out, data = _codes(*table) if table else None, _Out(), b""
    pred, eobrun, pending = [0, 0, 0], 0, []                                 # pending: the correction bits an end-of-band run owes

    def flush_eobrun():
        nonlocal eobrun, pending
        if eobrun:
            n = eobrun.bit_length() - 1
            out.symbol(codes, n << 4)
            out.put(eobrun & ((1 << n) - 1), n)
            eobrun = 0
        for b in pending:
            out.put(b, 1)
        pending = []

    for u, blocks in enumerate(scan_blocks):
        if restart and u and u % restart == 0:
            flush_eobrun()
            data += out.segment() + bytes([0xFF, 0xD0 + (u // restart - 1) % 8])
            pred = [0, 0, 0]
        for c, by, bx in blocks:
            blk = coefs[c][by, bx]
            if ss == 0 and ah == 0:
                v = int(blk[0]) >> al
                d, pred[c] = v - pred[c], v
                n = abs(d).bit_length()
                out.symbol(codes, n)
                out.put((d if d >= 0 else d - 1) & ((1 << n) - 1), n)
            elif ss == 0:
                out.put((int(blk[0]) >> al) & 1, 1)
            elif ah == 0:
                r = 0
                for k in range(ss, se + 1):
                    t = int(blk[R.ZIGZAG[k]])
                    m = abs(t) >> al
                    if m == 0:
                        r += 1
                        continue
                    flush_eobrun()
                    while r > 15:
                        out.symbol(codes, 0xF0)
                        r -= 16
                    n = m.bit_length()
                    out.symbol(codes, r << 4 | n)
                    out.put((m if t > 0 else ~m) & ((1 << n) - 1), n)
                    r = 0
                if r:
                    eobrun += 1
                    if eobrun == 0x7FFF:
                        flush_eobrun()
            else:
                mags = [abs(int(blk[R.ZIGZAG[k]])) >> al for k in range(64)]
                eob = max([k for k in range(ss, se + 1) if mags[k] == 1], default=0)
                r, br = 0, []
                for k in range(ss, se + 1):
                    m = mags[k]
                    if m == 0:
                        r += 1
                        continue
                    while r > 15 and k <= eob:
                        flush_eobrun()
                        out.symbol(codes, 0xF0)
                        r -= 16
                        for b in br:
                            out.put(b, 1)
                        br = []
                    if m > 1:
                        br.append(m & 1)
                        continue
                    flush_eobrun()
                    out.symbol(codes, r << 4 | 1)
                    out.put(0 if blk[R.ZIGZAG[k]] < 0 else 1, 1)
                    for b in br:
                        out.put(b, 1)
                    r, br = 0, []
                if r or br:
                    eobrun += 1
                    pending += br
                    if eobrun == 0x7FFF or len(pending) > 937:
                        flush_eobrun()
    flush_eobrun()
    return data + out.segment()


def write_progressive(coefs, info, script, restart=0):
    """A legal SOF2 file of the picture ``info`` describes (a probed file: H, W, components, qtables) holding ``coefs`` (per
    component int [blocks high, blocks wide, 64], natural order, as jpeg_ref lays them out), cut into the scans of ``script``:
    [(components, Ss, Se, Ah, Al)] or, with a restart interval of its own, [(components, Ss, Se, Ah, Al, units)]; ``restart`` is
    the interval of the others.  One fixed Huffman table per class that holds every symbol.  What a script's one-component scans
    do not visit (the padding blocks) is not written: see jpeg_prog_ref.real_only."""
    import jpeg_prog_ref as PR
    from avsep_amd import jpeg
    seg = jpeg._segment
    out = b"\xff\xd8" + seg(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    for t, q in sorted(info.qtables.items()):
        out += seg(0xDB, bytes([t]) + bytes(q))
    out += seg(0xC2, struct.pack(">BHHB", 8, info.H, info.W, len(info.components)) +
               b"".join(bytes([i, h << 4 | v, t]) for i, h, v, t in info.components))
    out += seg(0xC4, bytes([0x00]) + bytes(DC_TABLE[0]) + DC_TABLE[1]) + seg(0xC4, bytes([0x10]) + bytes(AC_TABLE[0]) + AC_TABLE[1])
    interval = 0
    for entry in script:
        comps, ss, se, ah, al = entry[:5]
        ri = entry[5] if len(entry) > 5 else restart
        if ri != interval:
            out += seg(0xDD, struct.pack(">H", ri))
            interval = ri
        units = jpeg._scan_units(info.H, info.W, info.components, list(comps))
        fake = jpeg.Scan(list(comps), ss, se, ah, al, [], ri, 0, 0, None, units, 0)
        blocks = [PR.blocks_of(info, fake, u) for u in range(units)]
        table = None if ss == 0 and ah else (DC_TABLE if ss == 0 else AC_TABLE)
        out += seg(0xDA, bytes([len(comps)]) + b"".join(bytes([info.components[c][0], 0]) for c in comps) + bytes([ss, se, ah << 4 | al]))
        out += _scan_bytes(info, coefs, blocks, table, ss, se, ah, al, ri)
    return out + b"\xff\xd9"


# the scripts Pillow cannot write (colour files); every one a complete progression
SCRIPTS = {
    "dc-al0": [((0, 1, 2), 0, 0, 0, 0), ((0,), 1, 63, 0, 0), ((1,), 1, 63, 0, 0), ((2,), 1, 63, 0, 0)],
    "ac-chain-3": [((0, 1, 2), 0, 0, 0, 0), ((0,), 1, 63, 0, 2), ((1,), 1, 63, 0, 2), ((2,), 1, 63, 0, 2), ((0,), 1, 63, 2, 1),
                   ((1,), 1, 63, 2, 1), ((2,), 1, 63, 2, 1), ((0,), 1, 63, 1, 0), ((1,), 1, 63, 1, 0), ((2,), 1, 63, 1, 0)],
    "y-split-8": [((0, 1, 2), 0, 0, 0, 1), ((0,), 1, 8, 0, 1), ((0,), 9, 63, 0, 1), ((1,), 1, 63, 0, 0), ((2,), 1, 63, 0, 0),
                  ((0, 1, 2), 0, 0, 1, 0), ((0,), 9, 63, 1, 0), ((0,), 1, 8, 1, 0)],
    "chroma-dc-pair": [((0,), 0, 0, 0, 1), ((1, 2), 0, 0, 0, 0), ((0,), 1, 63, 0, 1), ((2,), 1, 63, 0, 0), ((1,), 1, 63, 0, 0),
                       ((0,), 0, 0, 1, 0), ((0,), 1, 63, 1, 0)],
    "restarts-differ": [((0, 1, 2), 0, 0, 0, 1, 2), ((0,), 1, 63, 0, 1, 3), ((1,), 1, 63, 0, 1, 0), ((2,), 1, 63, 0, 1, 1),
                        ((0, 1, 2), 0, 0, 1, 0, 4), ((0,), 1, 63, 1, 0, 5), ((1,), 1, 63, 1, 0, 2), ((2,), 1, 63, 1, 0, 0)],
}
SCRIPT_LEVELS = {"dc-al0": [0, 0, 0, 0], "ac-chain-3": [0, 0, 0, 0, 1, 1, 1, 2, 2, 2], "y-split-8": [0, 0, 0, 0, 0, 1, 1, 1],
                 "chroma-dc-pair": [0, 0, 0, 0, 0, 1, 1], "restarts-differ": [0, 0, 0, 0, 1, 1, 1, 1]}
WRITTEN_SOURCES = ["33x65-420", "17x23-422", "40x48-noise", "9x40-444"]      # grid files whose coefficients the writer takes


@functools.lru_cache(maxsize=1)
def written():
    """The writer's files -> [(name, file, ScanInfo, the coefficients put in)]: every script over coefficients of grid files
    (so inside the arithmetic bound by construction), the padding blocks' unvisited terms cleared."""
    import jpeg_prog_ref as PR
    from avsep_amd import jpeg
    names = [n for n, _, _ in grid()]
    out = []
    for k, (script_name, script) in enumerate(SCRIPTS.items()):
        for src in (WRITTEN_SOURCES[k % len(WRITTEN_SOURCES)], WRITTEN_SOURCES[(k + 1) % len(WRITTEN_SOURCES)]):
            info, _, co = grid_reference()[names.index(src)]
            co = PR.real_only(info, co, keep_dc=all(len(e[0]) > 1 for e in script if e[1] == 0))
            d = write_progressive(co, info, script)
            out.append((f"{src}/{script_name}", d, jpeg.probe_scans(d), co))
    return out


# ---- the damaged set ---------------------------------------------------------------------------------------------------
def with_scan_bytes(data, scan, entropy):
    return data[:scan.begin] + bytes(entropy) + data[scan.end:]


def with_dht_values(data, info, k, change):
    """``data`` with every value v of the Huffman tables defined between scan k - 1 and scan k replaced by change(v)."""
    out, at = bytearray(data), info.scans[k - 1].end if k else 2
    while at < info.scans[k].begin:
        m, L = data[at + 1], struct.unpack(">H", data[at + 2:at + 4])[0]
        if m == 0xC4:
            p, end = at + 4, at + 2 + L
            while p < end:
                n = sum(data[p + 1:p + 17])
                out[p + 17:p + 17 + n] = bytes(change(v) for v in data[p + 17:p + 17 + n])
                p += 17 + n
        at += 2 + L
    return bytes(out)


@functools.lru_cache(maxsize=1)
def damaged():
    """The damaged set, all of one good 33 x 65 4:2:0 progressive file -> (the good file, [(name, bytes)]).  Scan 1 is the first
    luma AC scan, scan 9 the last luma refinement scan (Pillow writes a Huffman table of its own before each)."""
    from avsep_amd import jpeg
    good = JC.encode(JC.picture(33, 65, seed=1), subsampling=2, quality=85, progressive=True)
    info = jpeg.probe_scans(good)
    first, refine = info.scans[1], info.scans[9]
    e, r = good[first.begin:first.end], good[refine.begin:refine.end]
    flipped = bytearray(r)
    for i in range(48, len(r), 97):
        flipped[i] ^= 0xFF
    return good, [("a scan cut at half", with_scan_bytes(good, first, e[:len(e) // 2])),
                  ("a scan cut one byte short", with_scan_bytes(good, refine, r[:-1])),
                  ("a flipped byte every 97", with_scan_bytes(good, refine, flipped)),
                  ("a refinement symbol of size 2", with_dht_values(good, info, 9, lambda v: v + 1 if v & 15 == 1 else v)),
                  ("an end-of-band run past the segment", with_dht_values(good, info, 9, lambda v: 0xE0 if v & 15 == 0 and v >> 4 < 15 else v)),
                  ("a stray marker", with_scan_bytes(good, first, e[:len(e) // 3] + b"\xff\x01" + e[len(e) // 3:]))]


# ---- the host program's files --------------------------------------------------------------------------------------------
def launch_levels(chunk):
    """Per scan row of a chunk the level of the launch that holds it: the rows' own levels, as the planner wrote them."""
    return np.ascontiguousarray(chunk.scans["level"], dtype=np.int32)


def write_case(path, plan, chunk, scans=None, levels=None):
    """One chunk of a jpeg.plan(..., progressive=True) as the case file of tests/jpeg_scan_host.cpp."""
    images = np.ascontiguousarray(plan.images[chunk.a:chunk.b])
    scans = chunk.scans if scans is None else scans
    levels = launch_levels(chunk) if levels is None else levels
    with open(path, "wb") as f:
        f.write(struct.pack("<5q", len(plan.bytes), len(images), len(scans), len(plan.tables), chunk.blocks))
        for a in (plan.bytes, images, scans, levels, plan.tables):
            f.write(np.ascontiguousarray(a).tobytes())
