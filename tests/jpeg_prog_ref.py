"""NumPy restatement of the four scan paths of a progressive JPEG file (T.81 Annex G; csrc/jpeg_parts.h: jp_decode_scan): it
decodes a ``jpeg.ScanInfo`` scan by scan, in file order, into integer coefficients laid out as tests/jpeg_ref.py lays them out,
so that jpeg_ref's pixel stage (planes, colour) runs on them unchanged.  The oracle of the coefficient workspace: a progressive
file and its baseline twin hold the same coefficients, and tests/test_jpeg_prog_host.py pins that."""
import numpy as np

import jpeg_ref as R


def _real_blocks_across(info, c):
    hs = info.components[0][1] if len(info.components) == 3 else 1
    return -(-(info.W if c == 0 else -(-info.W // hs)) // 8)


def blocks_of(info, scan, u):
    """The blocks of unit ``u`` of a scan -> [(component, block row, block column)] in the stream's order."""
    hs, vs, mcux, mcuy, comps = R.geometry(info)
    if len(scan.comps) == 1:
        by, bx = divmod(u, _real_blocks_across(info, scan.comps[0]))
        return [(scan.comps[0], by, bx)]
    my, mx = divmod(u, mcux)
    return [(c, my * comps[c][3] + by, mx * comps[c][2] + bx) for c in scan.comps for by in range(comps[c][3]) for bx in range(comps[c][2])]


def _correct(bits, blk, nat, p1):
    if bits.take(1) and (blk[nat] & p1) == 0:
        blk[nat] += p1 if blk[nat] >= 0 else -p1


def decode_scan(info, scan, data, out):
    """One scan of ``data`` into ``out`` (per component int64 [blocks high, blocks wide, 64], natural order)."""
    codes = [R.huffman_codes(*t) if t is not None else None for t in scan.tables]
    per = scan.restart if scan.restart else scan.units
    p1 = 1 << scan.al
    for s, (b, e) in enumerate(R.split_segments(data, scan.begin, scan.end)):
        bits, pred, eobrun = R._Bits(data[b:e]), [0, 0, 0], 0
        for u in range(s * per, min((s + 1) * per, scan.units)):
            for c, by, bx in blocks_of(info, scan, u):
                blk, table = out[c][by, bx], codes[scan.comps.index(c)]
                if scan.ss == 0 and scan.ah == 0:                            # DC first
                    size = bits.symbol(table)
                    pred[c] += R._extend(bits.take(size), size)
                    blk[0] = pred[c] * p1
                elif scan.ss == 0:                                           # DC refinement
                    if bits.take(1):
                        blk[0] |= p1
                elif scan.ah == 0:                                           # AC first
                    if eobrun:
                        eobrun -= 1
                        continue
                    k = scan.ss
                    while k <= scan.se:
                        rs = bits.symbol(table)
                        r, size = rs >> 4, rs & 15
                        if size == 0:
                            if r == 15:
                                k += 16
                                continue
                            eobrun = (1 << r) + bits.take(r) - 1
                            break
                        k += r
                        blk[R.ZIGZAG[k]] = R._extend(bits.take(size), size) * p1
                        k += 1
                else:                                                        # AC refinement (G.1.2.3)
                    k = scan.ss
                    if eobrun == 0:
                        while k <= scan.se:
                            rs = bits.symbol(table)
                            r, size, val = rs >> 4, rs & 15, 0
                            if size:
                                assert size == 1, "a refinement symbol of a size other than 0 or 1"
                                val = p1 if bits.take(1) else -p1
                            elif r != 15:
                                eobrun = (1 << r) + bits.take(r)
                                break
                            while k <= scan.se:
                                nat = R.ZIGZAG[k]
                                if blk[nat] != 0:
                                    _correct(bits, blk, nat, p1)
                                else:
                                    r -= 1
                                    if r < 0:
                                        break
                                k += 1
                            if size:
                                blk[R.ZIGZAG[k]] = val
                            k += 1
                    if eobrun:
                        for k in range(k, scan.se + 1):
                            if blk[R.ZIGZAG[k]] != 0:
                                _correct(bits, blk, R.ZIGZAG[k], p1)
                        eobrun -= 1
        assert eobrun == 0


def coefficients(info, data):
    """The quantised coefficients of every block of a progressive file -> as jpeg_ref.coefficients gives a baseline file's."""
    out = [np.zeros((bh, bw, 64), dtype=np.int64) for bw, bh, _, _ in R.geometry(info)[4]]
    for scan in info.scans:
        decode_scan(info, scan, data, out)
    return out


def real_only(info, coefs, keep_dc=True):
    """``coefs`` with the AC terms (and, without keep_dc, the DC terms) of the padding blocks, those outside a component's real
    block grid, set to 0: what a progressive file, whose one-component scans walk the real grid, can hold of them."""
    out = [c.copy() for c in coefs]
    hs, vs = R.geometry(info)[:2]
    for c, co in enumerate(out):
        bw = _real_blocks_across(info, c)
        bh = -(-(info.H if c == 0 else -(-info.H // vs)) // 8)
        pad = np.ones(co.shape[:2], dtype=bool)
        pad[:bh, :bw] = False
        co[pad, 0 if not keep_dc else 1:] = 0
    return out
